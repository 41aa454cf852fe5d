// move_kernels.h -- part of the single translation unit msx.hip (included there, after logprob_kernel.h).
// Moves other than the stretch move, and mixtures of moves (include/msx.h, msx_*_enqueue_moves*):
// the kernels of the path BESIDE the fused kernel.  The fused kernel's proposal is the stretch move's and stays as it is;
// a chunk with a set of moves runs, per half-step, the plain evaluation between two launches of move_step_kernel.
#ifndef MSX_MOVE_KERNELS_H
#define MSX_MOVE_KERNELS_H

namespace {

// A chunk in the GENERAL layout lives in its slot where the stretch chunk's arrays live (SamplerRun::in_bytes: [zz | zfac |
// logu | sidx | cidx | partner | records], each L = lay(nsteps) * 2 * ns entries), the same six arrays read as
//   g = zz, fac = zfac, logu; sidx (the member's own index of the moving walker), cidx (likewise, the complementary half),
//   c1 = partner (ENSEMBLE index of C[p1], as run_pack / draw_iteration resolve the stretch move's partner)
// and, in the records' place (24 bytes per entry, of which this takes 4 and a few words):
//   c2 [L]  the ensemble index of C[p2] (= c1 on a stretch entry)        kind [lay(nsteps)][k]  the member's move
struct MoveChunk {
    const double *g, *fac, *logu;
    const int32_t *sidx, *c1, *c2, *kind;
};

// the members' places in a half-step's ns entries and in the ensemble; by value (a single target: one member)
struct MoveMembers {
    int32_t astart[MSX_MAX_GROUP], nh[MSX_MAX_GROUP], off[MSX_MAX_GROUP];
};

// ---- the draw -----------------------------------------------------------------------------------------------------------
// The set as the kernel takes it: cumulative weights (summed in order, as np.cumsum does) and g0 resolved on the host.
struct MoveSetDev {
    int32_t n, kind[MSX_MAX_MOVES];
    double cum[MSX_MAX_MOVES], a[MSX_MAX_MOVES], g0[MSX_MAX_MOVES], sigma[MSX_MAX_MOVES];
};

// One iteration `it` of one ensemble of nw walkers keyed by `seed` in the general layout, by the whole workgroup.  The
// split and the stretch move's numbers are draw_iteration's own (logprob_kernel.h: the same sort, streams 0..6), written
// with the chosen move's `a`; a DE iteration then overwrites p1 / g / fac and every iteration writes p2:
//   stream 7, index 0        the iteration's move: the first i with u < cum[i]
//   stream 8 + 3h, index j   the ordered pair of distinct walkers of the complementary half
//   streams 9 + 3h, 10 + 3h  Box-Muller: n = sqrt(-2 ln(1 - u1)) cos(2 pi u2), g = g0 (1 + sigma n)
// resolve / woff / o0 / hstride as draw_iteration takes them; kind_out: where the iteration's kind goes.
__device__ __forceinline__ void draw_moves_iteration(unsigned long long seed, const MoveSetDev &S, unsigned long long it, int nw, int32_t ndim,
                                                     int32_t resolve, int32_t woff, int64_t o0, int64_t hstride, int32_t *sidx, int32_t *cidx,
                                                     int32_t *p1, int32_t *p2, double *g, double *fac, double *logu, int32_t *kind_out) {
    const double um = counter_uniform(seed, it, 7u, 0u);
    int mi = 0;
    while (mi < S.n - 1 && !(um < S.cum[mi])) ++mi;
    const int kind = S.kind[mi];
    draw_iteration(seed, kind == MSX_MOVE_STRETCH ? S.a[mi] : 2.0, it, 0ull, nw, ndim, resolve, 0, woff, o0, hstride, sidx, cidx, p1, g, fac,
                   logu, (SmpRec *)nullptr);
    __threadfence_block();
    __syncthreads();  // (the complementary half's indices below were written by other threads)
    if (threadIdx.x == 0) *kind_out = kind;
    const int ns = nw / 2;
    for (int t = threadIdx.x; t < 2 * ns; t += kDrawThreads) {
#pragma clang fp contract(off)
        const int h = t / ns, j = t - h * ns;
        const int64_t o = o0 + h * hstride + j;
        if (kind == MSX_MOVE_STRETCH) {
            p2[o] = p1[o];
            continue;
        }
        const int32_t *comp = cidx + (o0 + h * hstride);  // the complementary half, the member's own indices
        const double ud = counter_uniform(seed, it, 8u + 3u * (unsigned int)h, (unsigned int)j);
        const double u1 = counter_uniform(seed, it, 9u + 3u * (unsigned int)h, (unsigned int)j);
        const double u2 = counter_uniform(seed, it, 10u + 3u * (unsigned int)h, (unsigned int)j);
        const long long npairs = (long long)ns * (long long)(ns - 1);
        long long p = (long long)floor(ud * (double)npairs);
        p = p < npairs - 1 ? p : npairs - 1;
        const int j1 = (int)(p / (ns - 1)), r = (int)(p % (ns - 1));
        const int j2 = r + (r >= j1 ? 1 : 0);
        const double rad = sqrt(-2.0 * log(1.0 - u1));
        const double ang = 6.283185307179586 * u2;
        const double n = rad * cos(ang);
        const double t1 = S.sigma[mi] * n;
        const double t2 = 1.0 + t1;
        p1[o] = resolve ? woff + comp[j1] : j1;
        p2[o] = resolve ? woff + comp[j2] : j2;
        g[o] = S.g0[mi] * t2;
        fac[o] = 0.0;
    }
}

// one workgroup per iteration of the chunk and member: grid (nsteps, k), the arrays [..][2][ns_total], kind [nsteps][k]
struct MoveDrawTable {
    unsigned long long seed[MSX_MAX_GROUP];
    MoveMembers M;  // nh: the member's WALKERS here (not its half)
};
__global__ void __launch_bounds__(kDrawThreads)
moves_draw_kernel(MoveDrawTable T, MoveSetDev S, int64_t first_iter, int32_t ndim, int32_t resolve, int64_t ns_total, int32_t *sidx, int32_t *cidx,
                  int32_t *p1, int32_t *p2, double *g, double *fac, double *logu, int32_t *kind) {
    const int64_t st = blockIdx.x;
    const int m = blockIdx.y;
    draw_moves_iteration(T.seed[m], S, (unsigned long long)(first_iter + st), T.M.nh[m], ndim, resolve, T.M.off[m],
                         st * 2 * ns_total + T.M.astart[m], ns_total, sidx, cidx, p1, p2, g, fac, logu, kind + st * gridDim.y + m);
}

// ---- the step -------------------------------------------------------------------------------------------------------------
// One workgroup per member; one launch (1) APPLIES half-step j -- the accept rule ln u < (fac + ln p(q)) - ln p(s) on the
// proposals q and their log-probabilities `newlp` (an error status travels as the NaN's payload: walker_done), the
// coordinates, log-probabilities and acceptance counts in place, the walker's row of the chain and of the log-probability
// chain, the worst status by atomicMax: what sampler_apply_kernel and walker_done write -- (2) meets at a barrier, and (3)
// PROPOSES half-step j + 1 into q from the just-updated ensemble.  A member's entries [astart, astart + nh) of q belong to
// its workgroup alone, and a move reads its own member's walkers only: the barrier is all the ordering there is.  a_on /
// p_on switch a part off (a chunk's first launch only proposes, its last only applies).
struct MoveStepArgs {
    double *coords, *logp, *q;
    const double *newlp;
    int64_t *nacc;
    int32_t ndim, a_on, p_on, kind_stride;
    MoveChunk a, p;                  // the applied and the proposed half-step's arrays (at that half-step's first entry;
                                     // kind at its iteration's first member)
    double *chain_row, *lp_row;      // of the applied half-step's iteration
    int32_t *worst;                  // [k]
};
__global__ void __launch_bounds__(256) move_step_kernel(MoveStepArgs A, MoveMembers M) {
    const int m = blockIdx.x;
    const int b = M.astart[m], n = M.nh[m];
    const int64_t off = M.off[m];
    const int ndim = A.ndim;
    if (A.a_on) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int64_t e = b + i;
            const int64_t si = off + A.a.sidx[e];
            const double out = A.newlp[e];
            const int st = status_of_nan(out);
            if (st > MSX_W_REJECT) atomicMax(A.worst + m, st);
            const double old = A.logp[si];
            const double lnpdiff = (A.a.fac[e] + out) - old;
            const bool acc = A.a.logu[e] < lnpdiff;  // NaN differences compare false, like the host loop
            for (int d = 0; d < ndim; ++d) {
                const double v = acc ? A.q[e * ndim + d] : A.coords[si * ndim + d];
                if (acc) A.coords[si * ndim + d] = v;
                A.chain_row[si * ndim + d] = v;
            }
            if (acc) {
                A.logp[si] = out;
                A.nacc[si] = A.nacc[si] + 1;
            }
            A.lp_row[si] = acc ? out : old;
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
                // no FMA contraction: the proposals must have the bits NumPy's `c - (c - s) * z` and `s + g * (c1 - c2)` give
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

}  // namespace

#endif  // MSX_MOVE_KERNELS_H
