// tempered_kernels.h -- part of the single translation unit msx.hip (included there, after move_kernels.h).
// Parallel tempering (include/msx.h, msx_tempered_*): T rungs of nw walkers, all of ONE context, rung t
// sampling lpr + beta_t * ll.  The rungs are the T members of a run in the general layout (move_kernels.h: member t owns
// walkers [t nw, (t + 1) nw) and entries [t ns, (t + 1) ns) of every half-step's T ns), so moves_draw_kernel draws them as
// it is.  New here: the step kernel on TWO value buffers, the swap sweep and the swap draws; and, for an adaptive run
// (DESIGN.md section 19), the ladder as device state, the step and sweep instantiations that read it and the kernel that
// moves it.
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
#define MSX_TEMPERED_BETA(m) A.beta[m]
#include "tempered_step_body.h"
#undef MSX_TEMPERED_BETA
}
// the adaptive run's instantiation: the rung's beta from the ladder in device memory (A.beta is not looked at)
__global__ void __launch_bounds__(256) tempered_step_adaptive_kernel(TemperedStepArgs A, const double *ladder) {
#define MSX_TEMPERED_BETA(m) ladder[m]
#include "tempered_step_body.h"
#undef MSX_TEMPERED_BETA
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
#define MSX_TEMPERED_DB(t) A.db[(t) - 1]
#include "tempered_swap_body.h"
#undef MSX_TEMPERED_DB
}
// the adaptive run's instantiation: db from the ladder in device memory, the subtraction NumPy's (A.db is not looked at)
__global__ void __launch_bounds__(256) tempered_swap_adaptive_kernel(TemperedSwapArgs A, const double *ladder) {
#define MSX_TEMPERED_DB(t) (ladder[(t) - 1] - ladder[t])
#include "tempered_swap_body.h"
#undef MSX_TEMPERED_DB
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

// ---- the adaptive ladder (mcmc_spec_amd.tempered.ladder_step is the definition) -----------------------
// The pieces of one ladder step, float64 + - * / only and contraction off, shared by the host entry msx_ladder_step and by
// tempered_adapt_kernel: the same text gives NumPy's bits on both sides.
__host__ __device__ inline double ladder_exp(const double x) {
#pragma clang fp contract(off)
    // exp for |x| <= 1: the degree-12 Taylor polynomial in x / 8 (Horner from the top, c[k] = 1 / k!), squared three times
    const double c[13] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                          1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0};
    const double y = x * 0.125;
    double p = c[12];
    for (int k = 11; k >= 0; --k) {
        const double py = p * y;
        p = py + c[k];
    }
    p = p * p;
    p = p * p;
    p = p * p;
    return p;
}
__host__ __device__ inline double ladder_kappa(const double k, const double lag, const double time) {
#pragma clang fp contract(off)
    const double sum = k + lag;
    const double decay = lag / sum;
    return decay / time;
}
// the gap below rung p (1 <= p <= T - 1) after the step: Ti[p] - Ti[p - 1], scaled for a free rung (p <= T - 2)
__host__ __device__ inline double ladder_gap(const int p, const int T, const double *Ti, const double *r, const double kappa) {
#pragma clang fp contract(off)
    const double g = Ti[p] - Ti[p - 1];
    if (p > T - 2) return g;
    const double dr = r[p - 1] - r[p];
    const double dS = kappa * dr;
    return g * ladder_exp(dS);
}
__host__ __device__ inline void ladder_sums(const int T, const double *g, double *c) {  // in index order: ONE thread's
#pragma clang fp contract(off)
    c[1] = g[1];
    for (int p = 2; p < T; ++p) c[p] = c[p - 1] + g[p];
}
__host__ __device__ inline double ladder_place(const double Ti0, const double span, const double cp, const double clast) {
#pragma clang fp contract(off)
    const double frac = cp / clast;
    const double prod = span * frac;
    const double sum = Ti0 + prod;
    return 1.0 / sum;
}
__host__ __device__ inline bool ladder_valid(const int T, const double *nb) {  // finite and strictly descending
    for (int t = 0; t < T; ++t) {
        const double v = nb[t];
        if (!(v - v == 0.0)) return false;
        if (t > 0 && !(v < nb[t - 1])) return false;
    }
    return true;
}

// One workgroup of 64 threads after each iteration's sweep: thread t < T writes beta_row[t], the ladder the iteration ran
// with, and does rung t's share (1 / beta, the pair's count since the last snapshot, the scaled gap, the final division);
// the running sum and the validity check are thread 0's, between barriers.  state: [0] k, [1] skipped (running).
struct TemperedAdaptArgs {
    double *beta;                            // [T] the ladder, moved in place
    const unsigned long long *nswap;         // [T - 1] running (the sweep's launch has finished: stream order)
    unsigned long long *prev;                // [T - 1] nswap at the previous iteration's end
    long long *state;                        // k, skipped
    double *beta_row;                        // [T] of the chunk's beta_chain
    double nw, lag, time;
    int32_t ntemps;
};
__global__ void __launch_bounds__(64) tempered_adapt_kernel(TemperedAdaptArgs A) {
    __shared__ double Ti[MSX_MAX_GROUP], r[MSX_MAX_GROUP], g[MSX_MAX_GROUP], c[MSX_MAX_GROUP], nb[MSX_MAX_GROUP];
    __shared__ int ok;
    const int t = threadIdx.x, T = A.ntemps;
    double b = 0.0;
    if (t < T) {
#pragma clang fp contract(off)
        b = A.beta[t];
        A.beta_row[t] = b;
        Ti[t] = 1.0 / b;
        nb[t] = b;
    }
    if (t < T - 1) {
#pragma clang fp contract(off)
        const unsigned long long now = A.nswap[t];
        const double cnt = (double)(long long)(now - A.prev[t]);
        A.prev[t] = now;
        r[t] = cnt / A.nw;
    }
    if (T <= 2) {  // nothing is free to move
        if (t == 0) A.state[0] = A.state[0] + 1;
        return;
    }
    __syncthreads();
    const double kappa = ladder_kappa((double)A.state[0], A.lag, A.time);
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
        if (!ok) A.state[1] = A.state[1] + 1;
    }
    __syncthreads();   // (every thread has read state[0] before the barriers above; thread 0 bumps it last)
    if (ok && t >= 1 && t < T - 1) A.beta[t] = nb[t];
    if (t == 0) A.state[0] = A.state[0] + 1;
}

}  // namespace

#endif  // MSX_TEMPERED_KERNELS_H
