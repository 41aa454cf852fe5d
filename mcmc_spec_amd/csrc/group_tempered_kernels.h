// group_tempered_kernels.h -- part of the single translation unit msx.hip (included there, after tempered_kernels.h).
// Parallel tempering for a TARGET GROUP (include/msx.h, msx_group_tempered_*): K targets, each with a
// ladder of T rungs, as K T members of one ensemble in the general layout -- member m = k T + t is rung t of target k and owns
// counts[k] walkers.  A target's rungs are contiguous, so a half-step's proposals are the K blocks of T counts[k] / 2 walkers
// the group kernel scores (group_kernel.h) and moves_draw_kernel draws the K T members as it is.  New here: the step on a
// member table, the sweep, the swap draws and the ladder step, each with a target axis.  Every run keeps its K ladders in
// device memory, [K T], whether they move or not.
#ifndef MSX_GROUP_TEMPERED_KERNELS_H
#define MSX_GROUP_TEMPERED_KERNELS_H

namespace {

// ---- the step -------------------------------------------------------------------------------------------------------------
// tempered_step_kernel's rule and expressions (tempered_step_body.h), one workgroup per member with the member's place from
// M: entries [astart, astart + nh) of the half-step, walkers from off on.  The rung's beta is ladder[m].
struct GroupTemperedStepArgs {
    double *coords, *ll, *lpr, *q;
    const double *new_lpr, *new_ll;
    const int32_t *st_lpr, *st_ll;
    int64_t *nacc;
    int32_t ndim, a_on, p_on;
    MoveChunk a, p;                    // the applied and the proposed half-step's arrays; kind at its iteration's member 0
    int32_t *worst;                    // [K T]
    const double *ladder;              // [K T]
};
__global__ void __launch_bounds__(256) group_tempered_step_kernel(GroupTemperedStepArgs A, MoveMembers M) {
    const int m = blockIdx.x;
    const int n = M.nh[m], ndim = A.ndim;
    const int64_t b = M.astart[m], off = M.off[m];
    const double beta = A.ladder[m];
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

// ---- the targets' places ------------------------------------------------------------------------------------------------------
// by value: target k's walkers per rung, its first walker in the ensemble (rung 0's) and its first swap draw in an
// iteration's row of sum_k (T - 1) nw[k]
struct GroupLadderTable {
    int32_t nw[MSX_MAX_GROUP], woff[MSX_MAX_GROUP], soff[MSX_MAX_GROUP];
};

// ---- the swap sweep ---------------------------------------------------------------------------------------------------------
// tempered_swap_kernel's sweep (tempered_swap_body.h) with a target axis: grid (ceil(max nw / 256), K), thread w of row k
// owns column w of target k and loops over that target's rungs from the hottest down; db = ladder[t - 1] - ladder[t], the
// subtraction NumPy's.  Every lane of a wave reaches every ballot -- a lane past its target's walkers votes false -- and
// only a whole workgroup past them returns early.  Accepted swaps: one atomic add per wave into nswap[k T + t - 1].
struct GroupTemperedSwapArgs {
    double *coords, *ll, *lpr;
    const double *logu;                      // this iteration's row: target k's [T - 1][nw[k]] at soff[k]
    double *chain_row, *ll_row, *lpr_row;    // [sum T nw][ndim], [sum T nw], [sum T nw]
    unsigned long long *nswap;               // [K T], running: pair (t, t - 1) of target k at k T + t - 1
    const double *ladder;                    // [K T]
    int32_t ntemps, ndim;
};
__global__ void __launch_bounds__(256) group_tempered_swap_kernel(GroupTemperedSwapArgs A, GroupLadderTable G) {
    const int k = blockIdx.y;
    const int nw = G.nw[k];
    if ((int)(blockIdx.x * blockDim.x) >= nw) return;  // (the whole workgroup)
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = w < nw;
    const int ndim = A.ndim, T = A.ntemps;
    const int64_t w0 = G.woff[k];
    const double *ladder = A.ladder + (int64_t)k * T;
    const double *logu = A.logu + G.soff[k];
    unsigned long long *nswap = A.nswap + (int64_t)k * T;
    for (int t = T - 1; t >= 1; --t) {
        bool sw = false;
        if (live) {
#pragma clang fp contract(off)
            const int64_t hi = w0 + (int64_t)t * nw + w, lo = hi - nw;
            const double l_hi = A.ll[hi], l_lo = A.ll[lo];
            const double d = l_hi - l_lo;
            const double db = ladder[t - 1] - ladder[t];
            const double lnr = db * d;
            sw = logu[(int64_t)(t - 1) * nw + w] < lnr;
            if (sw) {
                A.ll[hi] = l_lo;
                A.ll[lo] = l_hi;
                const double p_hi = A.lpr[hi], p_lo = A.lpr[lo];
                A.lpr[hi] = p_lo;
                A.lpr[lo] = p_hi;
                for (int d2 = 0; d2 < ndim; ++d2) {
                    const double x_hi = A.coords[hi * ndim + d2], x_lo = A.coords[lo * ndim + d2];
                    A.coords[hi * ndim + d2] = x_lo;
                    A.coords[lo * ndim + d2] = x_hi;
                }
            }
        }
        const unsigned long long votes = __ballot(sw);
        if ((threadIdx.x & (warpSize - 1)) == 0 && votes != 0ull) atomicAdd(nswap + (t - 1), (unsigned long long)__popcll(votes));
    }
    if (!live) return;
    for (int t = 0; t < T; ++t) {
        const int64_t i = w0 + (int64_t)t * nw + w;
        for (int d = 0; d < ndim; ++d) A.chain_row[i * ndim + d] = A.coords[i * ndim + d];
        A.ll_row[i] = A.ll[i];
        A.lpr_row[i] = A.lpr[i];
    }
}

// ---- the swap draws ---------------------------------------------------------------------------------------------------------
// tempered_swap_draw_kernel with a target axis: grid (nsteps, K (T - 1), ceil(max nw / 256)); target k's draws are stream 14 of
// seed0[k] (its rung 0's key) at index p * 4096 + w -- the numbers its own ladder draws alone.  logu [nsteps][sum (T - 1) nw].
struct GroupSwapSeeds {
    unsigned long long seed0[MSX_MAX_GROUP];
};
__global__ void __launch_bounds__(256)
group_tempered_swap_draw_kernel(GroupSwapSeeds S, GroupLadderTable G, int64_t first_iter, int32_t pairs, int64_t row, double *logu) {
    const int k = blockIdx.y / pairs;
    const unsigned int p = blockIdx.y - k * pairs;
    const int nw = G.nw[k];
    const int w = blockIdx.z * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const int64_t st = blockIdx.x;
    const double u = counter_uniform(S.seed0[k], (unsigned long long)(first_iter + st), kSwapStream, p * kSwapStride + (unsigned int)w);
    logu[st * row + G.soff[k] + (int64_t)p * nw + w] = log(u);
}

// ---- the ladder step ----------------------------------------------------------------------------------------------------------
// tempered_adapt_kernel with a target axis: one workgroup of 64 threads per target after each iteration's sweep, on the
// target's own slice of the ladder, of the counters and of (k, skipped), with its own lag and time -- the inline ladder_*
// pieces of tempered_kernels.h in the same order, so the host definition, msx_ladder_step and this kernel give the same bits.
struct GroupAdaptTable {
    double nw[MSX_MAX_GROUP], lag[MSX_MAX_GROUP], time[MSX_MAX_GROUP];
};
struct GroupAdaptArgs {
    double *beta;                            // [K T] the ladders, moved in place
    const unsigned long long *nswap;         // [K T] running (the sweep's launch has finished: stream order)
    unsigned long long *prev;                // [K T] nswap at the previous iteration's end
    long long *state;                        // [K][2]: k, skipped
    double *beta_row;                        // [K T] of the chunk's beta_chain
    int32_t ntemps;
};
__global__ void __launch_bounds__(64) group_tempered_adapt_kernel(GroupAdaptArgs A, GroupAdaptTable P) {
    __shared__ double Ti[MSX_MAX_GROUP], r[MSX_MAX_GROUP], g[MSX_MAX_GROUP], c[MSX_MAX_GROUP], nb[MSX_MAX_GROUP];
    __shared__ int ok;
    const int t = threadIdx.x, T = A.ntemps, k = blockIdx.x;
    double *beta = A.beta + (int64_t)k * T, *beta_row = A.beta_row + (int64_t)k * T;
    const unsigned long long *nswap = A.nswap + (int64_t)k * T;
    unsigned long long *prev = A.prev + (int64_t)k * T;
    long long *state = A.state + 2 * k;
    double b = 0.0;
    if (t < T) {
#pragma clang fp contract(off)
        b = beta[t];
        beta_row[t] = b;
        Ti[t] = 1.0 / b;
        nb[t] = b;
    }
    if (t < T - 1) {
#pragma clang fp contract(off)
        const unsigned long long now = nswap[t];
        const double cnt = (double)(long long)(now - prev[t]);
        prev[t] = now;
        r[t] = cnt / P.nw[k];
    }
    if (T <= 2) {  // nothing is free to move
        if (t == 0) state[0] = state[0] + 1;
        return;
    }
    __syncthreads();
    const double kappa = ladder_kappa((double)state[0], P.lag[k], P.time[k]);
    if (t >= 1 && t < T) g[t] = ladder_gap(t, T, Ti, r, kappa);
    __syncthreads();
    if (t == 0) ladder_sums(T, g, c);
    __syncthreads();
    if (t >= 1 && t < T - 1) {
#pragma clang fp contract(off)
        nb[t] = ladder_place(Ti[0], Ti[T - 1] - Ti[0], c[t], c[T - 1]);
    }
    __syncthreads();
    if (t == 0) {
        ok = ladder_valid(T, nb) ? 1 : 0;
        if (!ok) state[1] = state[1] + 1;
    }
    __syncthreads();   // (every thread has read state[0] before the barriers above; thread 0 bumps it last)
    if (ok && t >= 1 && t < T - 1) beta[t] = nb[t];
    if (t == 0) state[0] = state[0] + 1;
}

}  // namespace

#endif  // MSX_GROUP_TEMPERED_KERNELS_H
