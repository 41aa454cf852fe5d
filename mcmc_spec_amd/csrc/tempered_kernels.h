// tempered_kernels.h -- part of the single translation unit msx.hip (included there, after move_kernels.h).
// Parallel tempering (include/msx.h, msx_tempered_*): T rungs of nw walkers, all of ONE context, rung t
// sampling lpr + beta_t * ll.  The rungs are the T members of a run in the general layout (move_kernels.h: member t owns
// walkers [t nw, (t + 1) nw) and entries [t ns, (t + 1) ns) of every half-step's T ns), so moves_draw_kernel draws them as
// it is.  New here: the step kernel on TWO value buffers, the swap sweep and the swap draws.
#ifndef MSX_TEMPERED_KERNELS_H
#define MSX_TEMPERED_KERNELS_H

namespace {

constexpr unsigned int kSwapStream = 14u;    // the counter generator's stream of the swap draws (0..13: move_kernels.h)
constexpr unsigned int kSwapStride = 4096u;  // index = (t - 1) * kSwapStride + w

// ---- the step -------------------------------------------------------------------------------------------------------------
// move_step_kernel's shape, one workgroup per rung: (1) APPLIES half-step j -- ln u < (fac + P(q)) - P(s) with
// P(x) = lpr(x) + beta * ll(x) in two roundings, P(s) from the stored lpr and ll; a proposal whose prior status is
// MSX_W_REJECT is rejected by its -inf and its likelihood status is not looked at; an error status of the prior, or of the
// likelihood on a proposal the prior admits, goes to the rung's worst status -- (2) meets at a barrier and (3) PROPOSES
// half-step j + 1 with move_step_kernel's contraction-free expressions.  The chain's rows are the swap kernel's to write.
struct TemperedStepArgs {
    double *coords, *ll, *lpr, *q;
    const double *new_lpr, *new_ll;
    const int32_t *st_lpr, *st_ll;
    int64_t *nacc;
    int32_t ndim, a_on, p_on, nw, ns;  // nw, ns: per rung
    MoveChunk a, p;                    // the applied and the proposed half-step's arrays (move_step_kernel's)
    int32_t *worst;                    // [T]
    double beta[MSX_MAX_GROUP];
};
__global__ void __launch_bounds__(256) tempered_step_kernel(TemperedStepArgs A) {
    const int m = blockIdx.x;
    const int n = A.ns, ndim = A.ndim;
    const int64_t b = (int64_t)m * A.ns, off = (int64_t)m * A.nw;
    const double beta = A.beta[m];
    if (A.a_on) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma clang fp contract(off)
            const int64_t e = b + i;
            const int64_t si = off + A.a.sidx[e];
            const double pl = A.new_lpr[e], lk = A.new_ll[e];
            const int sp = A.st_lpr[e], sl = A.st_ll[e];
            if (sp > MSX_W_REJECT) atomicMax(A.worst + m, sp);
            if (sp != MSX_W_REJECT && sl > MSX_W_REJECT) atomicMax(A.worst + m, sl);
            const double prod_q = beta * lk;
            const double p_q = pl + prod_q;
            const double old_ll = A.ll[si], old_lpr = A.lpr[si];
            const double prod_s = beta * old_ll;
            const double p_s = old_lpr + prod_s;
            const double lnpdiff = (A.a.fac[e] + p_q) - p_s;
            const bool acc = A.a.logu[e] < lnpdiff;  // NaN differences compare false, like the host loop
            if (acc) {
                for (int d = 0; d < ndim; ++d) A.coords[si * ndim + d] = A.q[e * ndim + d];
                A.ll[si] = lk;
                A.lpr[si] = pl;
                A.nacc[si] = A.nacc[si] + 1;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (A.p_on) {
        const int kind = A.p.kind[m];
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int64_t e = b + i;
            const int64_t si = off + A.p.sidx[e], c1 = A.p.c1[e], c2 = A.p.c2[e];
            const double g = A.p.g[e];
            for (int d = 0; d < ndim; ++d) {
#pragma clang fp contract(off)
                // no FMA contraction: the bits NumPy's `c - (c - s) * z` and `s + g * (c1 - c2)` give
                const double sv = A.coords[si * ndim + d];
                const double cv = A.coords[c1 * ndim + d];
                double qv;
                if (kind == MSX_MOVE_STRETCH) {
                    const double diff = cv - sv;
                    const double prod = diff * g;
                    qv = cv - prod;
                } else {
                    const double diff = cv - A.coords[c2 * ndim + d];
                    const double prod = g * diff;
                    qv = sv + prod;
                }
                A.q[e * ndim + d] = qv;
            }
        }
    }
}

// ---- the swap sweep ---------------------------------------------------------------------------------------------------------
// One thread per walker index w, looping over the rungs from the hottest down: walker w of rung t meets walker w of rung
// t - 1 and they exchange coordinates, ll and lpr when ln u < db[t - 1] * (ll[t][w] - ll[t - 1][w]) (contraction off; a NaN
// compares false).  Serial in t -- a walker can travel several rungs -- and parallel in w: thread w touches column w only.
// Then the iteration's rows of the three chains.  Accepted swaps per pair: the wave's ballot, one atomic add per wave.
struct TemperedSwapArgs {
    double *coords, *ll, *lpr;
    const double *logu;                      // [T - 1][nw] of this iteration
    double *chain_row, *ll_row, *lpr_row;    // [T][nw][ndim], [T][nw], [T][nw]
    unsigned long long *nswap;               // [T - 1], running
    int32_t ntemps, nw, ndim;
    double db[MSX_MAX_GROUP];                // db[p] = beta[p] - beta[p + 1], formed on the host
};
__global__ void __launch_bounds__(256) tempered_swap_kernel(TemperedSwapArgs A) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = w < A.nw;
    const int ndim = A.ndim;
    for (int t = A.ntemps - 1; t >= 1; --t) {
        bool sw = false;
        if (live) {
#pragma clang fp contract(off)
            const int64_t hi = (int64_t)t * A.nw + w, lo = hi - A.nw;
            const double l_hi = A.ll[hi], l_lo = A.ll[lo];
            const double d = l_hi - l_lo;
            const double lnr = A.db[t - 1] * d;
            sw = A.logu[(int64_t)(t - 1) * A.nw + w] < lnr;
            if (sw) {
                A.ll[hi] = l_lo;
                A.ll[lo] = l_hi;
                const double p_hi = A.lpr[hi], p_lo = A.lpr[lo];
                A.lpr[hi] = p_lo;
                A.lpr[lo] = p_hi;
                for (int k = 0; k < ndim; ++k) {
                    const double x_hi = A.coords[hi * ndim + k], x_lo = A.coords[lo * ndim + k];
                    A.coords[hi * ndim + k] = x_lo;
                    A.coords[lo * ndim + k] = x_hi;
                }
            }
        }
        const unsigned long long votes = __ballot(sw);
        if ((threadIdx.x & (warpSize - 1)) == 0 && votes != 0ull) atomicAdd(A.nswap + (t - 1), (unsigned long long)__popcll(votes));
    }
    if (!live) return;
    for (int t = 0; t < A.ntemps; ++t) {
        const int64_t i = (int64_t)t * A.nw + w;
        for (int k = 0; k < ndim; ++k) A.chain_row[i * ndim + k] = A.coords[i * ndim + k];
        A.ll_row[i] = A.ll[i];
        A.lpr_row[i] = A.lpr[i];
    }
}

// ---- the swap draws ---------------------------------------------------------------------------------------------------------
// ln u of stream 14 for a chunk: logu [nsteps][T - 1][nw], iteration first_iter + st, index p * 4096 + w for the pair
// (p + 1, p); the logarithm is the one the generator takes for the accept draws (draw_iteration).  Grid (nsteps, T - 1,
// ceil(nw / 256)).
__global__ void __launch_bounds__(256) tempered_swap_draw_kernel(unsigned long long seed0, int64_t first_iter, int32_t nw, double *logu) {
    const int w = blockIdx.z * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const unsigned int p = blockIdx.y;
    const int64_t st = blockIdx.x;
    const double u = counter_uniform(seed0, (unsigned long long)(first_iter + st), kSwapStream, p * kSwapStride + (unsigned int)w);
    logu[(st * gridDim.y + p) * nw + w] = log(u);
}

}  // namespace

#endif  // MSX_TEMPERED_KERNELS_H
