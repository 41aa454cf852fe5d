// Block means and log-mean-exponentials of one column of a device chain series (msx_series_evidence, include/msx.h;
// DESIGN.md section 18): what thermodynamic integration and the stepping stone make of a tempered run's ln L.
//
// A series holds [ndim][nw][cap] doubles; for column c, walker w the selection x[t] = series[discard + t * thin], t < n',
// is cut into B consecutive blocks, block b = rows [b n' / B, (b + 1) n' / B).  Four kernels:
//   evd_part_kernel    one workgroup per (walker, block): the block's sum and maximum;
//   evd_mean_kernel    one workgroup per member: the walkers' sums in walker order -> the block means and maxima, then
//                      the blocks' sums in block order -> the mean of everything;
//   evd_exp_kernel     one workgroup per (walker, block): sum of exp(db (x - M)), M the MEMBER's maximum of that block;
//   evd_lme_kernel     one workgroup per member: walkers in order, then the blocks combined by rescaling, in order.
// A workgroup's sum: thread i adds the block's elements i, i + 256, ... one after the other, then a fixed tree over the
// 256 threads.  So the order of every sum depends on (n', W_m, B) alone -- not on thin, the buffer's capacity, the
// alignment or the launch -- and the bits do not either; that is why the loads are one double per lane for thin == 1 as
// for thin > 1 (consecutive lanes read consecutive doubles: 512 contiguous bytes per wave instruction).  tests/
// evidence_numpy.py restates the arithmetic.  Only plain C++ stores; no atomics; no workgroup waits for another.
#pragma once

constexpr int kEvdThreads = 256;   // one workgroup's stride through its block, and the width of its tree
constexpr int kEvdMaxBlocks = 64;  // blocks per call (one thread each in the member kernels)

struct EvdDb { double v[MSX_MAX_GROUP]; };   // db[m], by value (k <= MSX_MAX_GROUP)

// the maximum that ignores NaN (fmax's rule, written out: a NaN in the data shows in the sums, not in M)
__device__ __forceinline__ double evd_max(double a, double b) { return b > a ? b : a; }

__device__ __forceinline__ void evd_block(int64_t np, int32_t nblocks, int64_t b, int64_t *lo, int64_t *hi) {
    // floor(b n' / B): n' < 2^47 rows at B <= 64 (a series' rows are far fewer)
    *lo = b * np / nblocks;
    *hi = (b + 1) * np / nblocks;
}

// psum, pmax [nw][B]
__global__ void __launch_bounds__(kEvdThreads) evd_part_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, int32_t col,
                                                              int64_t np, int64_t discard, int64_t thin, int32_t nblocks,
                                                              double *__restrict__ psum, double *__restrict__ pmax) {
#pragma clang fp contract(off)
    __shared__ double rs[kEvdThreads], rm[kEvdThreads];
    const int64_t w = blockIdx.x, b = blockIdx.y;
    int64_t lo, hi;
    evd_block(np, nblocks, b, &lo, &hi);
    const double *x = rows + ((int64_t)col * nw + w) * cap + discard;
    double acc = 0.0, mx = -INFINITY;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kEvdThreads) {
        const double v = x[t * thin];
        acc = acc + v;
        mx = evd_max(mx, v);
    }
    rs[threadIdx.x] = acc;
    rm[threadIdx.x] = mx;
    __syncthreads();
    for (int h = kEvdThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + h];
            rm[threadIdx.x] = evd_max(rm[threadIdx.x], rm[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[w * nblocks + b] = rs[0];
        pmax[w * nblocks + b] = rm[0];
    }
}

// mean_out [k][B + 1] (0: everything; 1 + b: block b), mmax [k][B].  grid k, kEvdMaxBlocks threads.
__global__ void __launch_bounds__(kEvdMaxBlocks) evd_mean_kernel(const double *__restrict__ psum, const double *__restrict__ pmax,
                                                                const int64_t *__restrict__ member_off, int64_t np, int32_t nblocks,
                                                                double *__restrict__ mean_out, double *__restrict__ mmax) {
#pragma clang fp contract(off)
    __shared__ double bs[kEvdMaxBlocks];
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int b = threadIdx.x;
    if (b < nblocks) {
        int64_t lo, hi;
        evd_block(np, nblocks, b, &lo, &hi);
        double s = 0.0, mx = -INFINITY;
        for (int64_t w = w0; w < w1; ++w) {
            s = s + psum[w * nblocks + b];
            mx = evd_max(mx, pmax[w * nblocks + b]);
        }
        bs[b] = s;
        mmax[m * nblocks + b] = mx;
        mean_out[m * (nblocks + 1) + 1 + b] = s / (double)((hi - lo) * (w1 - w0));
    }
    __syncthreads();
    if (b == 0) {
        double s = 0.0;
        for (int j = 0; j < nblocks; ++j) s = s + bs[j];
        mean_out[m * (nblocks + 1)] = s / (double)(np * (w1 - w0));
    }
}

// pexp [nw][B]: sum over the block of exp(db[m] (x - mmax[m][b])), a -inf element counting as 0
__global__ void __launch_bounds__(kEvdThreads) evd_exp_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, int32_t col,
                                                             int64_t np, int64_t discard, int64_t thin, int32_t nblocks,
                                                             const int64_t *__restrict__ member_off, int32_t k, EvdDb db,
                                                             const double *__restrict__ mmax, double *__restrict__ pexp) {
#pragma clang fp contract(off)
    __shared__ double rs[kEvdThreads];
    const int64_t w = blockIdx.x, b = blockIdx.y;
    int m = 0;
    while (m + 1 < k && member_off[m + 1] <= w) ++m;   // (k <= 64 uniform steps)
    int64_t lo, hi;
    evd_block(np, nblocks, b, &lo, &hi);
    const double *x = rows + ((int64_t)col * nw + w) * cap + discard;
    const double d = db.v[m], M = mmax[m * nblocks + b];
    double acc = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kEvdThreads) {
        const double v = x[t * thin];
        const double diff = v - M;
        const double arg = d * diff;
        acc = acc + (v == -INFINITY ? 0.0 : exp(arg));
    }
    rs[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kEvdThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) pexp[w * nblocks + b] = rs[0];
}

// ln((1 / N) S) + db M of a sum S of exp(db (x - M)) over N values: -inf when nothing weighs (S == 0: all -inf)
__device__ __forceinline__ double evd_lme(double d, double M, double S, double N) {
#pragma clang fp contract(off)
    if (S == 0.0) return -INFINITY;
    const double a = d * M;
    const double l = log(S / N);
    return a + l;
}

// lme_out [k][B + 1].  The total: M = the blocks' maximum, S = sum_b S_b exp(db (M_b - M)) in block order (a block
// with S_b == 0 adds 0).  grid k, kEvdMaxBlocks threads.
__global__ void __launch_bounds__(kEvdMaxBlocks) evd_lme_kernel(const double *__restrict__ pexp, const double *__restrict__ mmax,
                                                               const int64_t *__restrict__ member_off, int64_t np, int32_t nblocks,
                                                               EvdDb db, double *__restrict__ lme_out) {
#pragma clang fp contract(off)
    __shared__ double bs[kEvdMaxBlocks];
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int b = threadIdx.x;
    const double d = db.v[m];
    if (b < nblocks) {
        int64_t lo, hi;
        evd_block(np, nblocks, b, &lo, &hi);
        double s = 0.0;
        for (int64_t w = w0; w < w1; ++w) s = s + pexp[w * nblocks + b];
        bs[b] = s;
        lme_out[m * (nblocks + 1) + 1 + b] = evd_lme(d, mmax[m * nblocks + b], s, (double)((hi - lo) * (w1 - w0)));
    }
    __syncthreads();
    if (b == 0) {
        double M = -INFINITY;
        for (int j = 0; j < nblocks; ++j) M = evd_max(M, mmax[m * nblocks + j]);
        double S = 0.0;
        for (int j = 0; j < nblocks; ++j) {
            const double diff = mmax[m * nblocks + j] - M;
            const double arg = d * diff;
            const double term = bs[j] * exp(arg);
            S = S + (bs[j] == 0.0 ? 0.0 : term);
        }
        lme_out[m * (nblocks + 1)] = evd_lme(d, M, S, (double)(np * (w1 - w0)));
    }
}
