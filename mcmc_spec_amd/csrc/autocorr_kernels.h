// Autocorrelation of chains held on the device (msx_series_*, include/msx.h).
//
// A series holds a chain as [ndim][nw][cap] doubles: each walker-dimension series is contiguous.  For the rows
// x = rows[0:n][discard::thin] (n' of them) of member m and dimension d the library computes
//     f[m][d][j] = (1 / W_m) sum_{k in m} acov_k(tau) / acov_k(0),   tau = lag0 + j,
//     acov_k(tau) = sum_{t < n' - tau} y_k[t] y_k[t + tau],   y = x - mean(x)
// by direct sums (what _autocorr_1d's zero-padded FFT computes).  Three kernels:
//   acf_mean_kernel   one workgroup per series: the mean, in a fixed order;
//   acf_lag_kernel    one workgroup per (series, lag tile, superblock of kAcfSuper rows): partial sums;
//   acf_reduce_kernel one thread per (member, dimension, lag): superblocks in order, then the member's walkers in order.
// The summation order of every acov_k(tau) depends on n' alone -- not on the lag tile tau falls in, the launch, or how
// the rows were appended -- so the bits do not either.  Only plain C++ stores.
#pragma once

constexpr int kAcfR = 5;                      // lags per lane, consecutive: each LDS read of the window feeds 5 FMAs
constexpr int kAcfLanes = 64;
constexpr int kAcfLagTile = kAcfLanes * kAcfR;  // 320 lags per workgroup
constexpr int kAcfWaves = 4;                  // ... each wave one block of kAcfBlock rows of the workgroup's superblock
constexpr int kAcfBlock = 128 * kAcfR;        // 640 rows (a multiple of kAcfR: the unrolled loop has no tail)
constexpr int kAcfSuper = kAcfWaves * kAcfBlock;  // 2560 rows per workgroup
constexpr int kAcfThreads = kAcfLanes * kAcfWaves;
constexpr int kAcfMeanThreads = 256;

// rows [nsteps][nw][ndim] (a chunk's chain in its slot, or uploaded rows) -> series rows row0 .. row0 + nsteps - 1.
// One thread per element, in the series' order (consecutive threads write consecutive rows of one walker-dimension).
__global__ void series_put_kernel(const double *__restrict__ in, int64_t nsteps, int64_t nw, int32_t ndim,
                                  double *__restrict__ out, int64_t cap, int64_t row0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = nsteps * nw * ndim;
    if (i >= total) return;
    const int64_t t = i % nsteps, rest = i / nsteps, w = rest % nw, d = rest / nw;
    out[(d * nw + w) * cap + row0 + t] = in[(t * nw + w) * ndim + d];
}

// series rows row0 .. row0 + nrows - 1 -> [nrows][nw][ndim] (msx_series_read)
__global__ void series_get_kernel(const double *__restrict__ in, int64_t cap, int64_t row0, int64_t nrows, int64_t nw,
                                  int32_t ndim, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = nrows * nw * ndim;
    if (i >= total) return;
    const int64_t d = i % ndim, rest = i / ndim, w = rest % nw, t = rest / nw;
    out[i] = in[(d * nw + w) * cap + row0 + t];
}

// The requested series: s = q * nw + w is walker w of the q-th requested dimension dims[q].
struct AcfDims { int32_t nd; int32_t d[8]; };

__device__ __forceinline__ const double *acf_series(const double *rows, int64_t cap, int64_t nw, const AcfDims &dims, int64_t s) {
    const int64_t q = s / nw, w = s % nw;
    return rows + ((int64_t)dims.d[q] * nw + w) * cap;
}

// mean of x[t] = series[discard + t * thin], t < np: each thread sums its stride sequentially, then a fixed tree
__global__ void __launch_bounds__(kAcfMeanThreads) acf_mean_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw,
                                                                   AcfDims dims, int64_t np, int64_t discard, int64_t thin,
                                                                   double *__restrict__ mean) {
    __shared__ double red[kAcfMeanThreads];
    const int64_t s = blockIdx.x;
    const double *x = acf_series(rows, cap, nw, dims, s) + discard;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < np; t += kAcfMeanThreads) acc += x[t * thin];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kAcfMeanThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[s] = red[0] / (double)np;
}

// Partial sums of acov(tau) over one superblock [S0, S0 + kAcfSuper) of rows for the lags [tau_lo, tau_lo + kAcfLagTile)
// of one series -> part[(s * nsuper + S) * pstride + tau - lag_base].  grid (series, lag tiles, superblocks).
//
// LDS: A = y[S0 .. S0 + kAcfSuper), B = y[S0 + tau_lo .. S0 + tau_lo + kAcfSuper + kAcfLagTile), zero past n'.  Wave v
// sums rows [S0 + v * kAcfBlock, + kAcfBlock); lane i owns the lags tau_lo + 5i .. tau_lo + 5i + 4 and keeps the five
// values of B they read at row t in registers, sliding one element per row: per row one broadcast read of A, one read
// of B (lanes 5 doubles apart: odd stride, so the 32 lanes of a ds_read_b64 group hit 64 distinct banks) and 5 FMAs.
// A term whose row or partner row lies past n' multiplies a zero and leaves the sum's bits as they are (the sums start
// at +0 and never become -0), so a wave may run its whole block whatever its lanes' lags are.  The four blocks' sums are
// added in block order.
__global__ void __launch_bounds__(kAcfThreads) acf_lag_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, AcfDims dims,
                                                              int64_t np, int64_t discard, int64_t thin,
                                                              const double *__restrict__ mean, int64_t lag_base, int64_t nlag,
                                                              double *__restrict__ part, int64_t nsuper, int64_t pstride) {
    __shared__ double lds[2 * kAcfSuper + kAcfLagTile];
    double *A = lds, *B = lds + kAcfSuper;
    const int64_t s = blockIdx.x, S = blockIdx.z;
    const int64_t tile_lo = lag_base + (int64_t)blockIdx.y * kAcfLagTile;
    const int64_t S0 = S * kAcfSuper;
    const double *x = acf_series(rows, cap, nw, dims, s) + discard;
    const double mu = mean[s];
    for (int i = threadIdx.x; i < kAcfSuper; i += kAcfThreads) {
        const int64_t t = S0 + i;
        A[i] = t < np ? x[t * thin] - mu : 0.0;
    }
    for (int i = threadIdx.x; i < kAcfSuper + kAcfLagTile; i += kAcfThreads) {
        const int64_t t = S0 + tile_lo + i;
        B[i] = t < np ? x[t * thin] - mu : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x % kAcfLanes, wave = threadIdx.x / kAcfLanes;
    const int b0 = wave * kAcfBlock;   // the wave's rows, relative to S0
    const int l0 = lane * kAcfR;       // the lane's first lag, relative to tile_lo
    double acc[kAcfR];
#pragma unroll
    for (int r = 0; r < kAcfR; ++r) acc[r] = 0.0;
    // rows the wave has to visit: t < n' - tile_lo (a wave-uniform bound), rounded up to a multiple of kAcfR
    int64_t lim = np - tile_lo - S0 - b0;
    lim = lim < 0 ? 0 : (lim > kAcfBlock ? kAcfBlock : lim);
    const int nrow = (int)((lim + kAcfR - 1) / kAcfR) * kAcfR;
    double w[kAcfR];  // w[(u + r) % kAcfR] = B[b0 + tt + u + l0 + r]
#pragma unroll
    for (int r = 0; r < kAcfR - 1; ++r) w[r] = B[b0 + l0 + r];
    for (int tt = 0; tt < nrow; tt += kAcfR) {
#pragma unroll
        for (int u = 0; u < kAcfR; ++u) {
            w[(u + kAcfR - 1) % kAcfR] = B[b0 + tt + u + l0 + kAcfR - 1];
            const double a = A[b0 + tt + u];
#pragma unroll
            for (int r = 0; r < kAcfR; ++r) acc[r] = fma(a, w[(u + r) % kAcfR], acc[r]);
        }
    }
    __syncthreads();  // (A and B are done with: the blocks' sums go where A was)
#pragma unroll
    for (int r = 0; r < kAcfR; ++r) A[wave * kAcfLagTile + l0 + r] = acc[r];
    __syncthreads();
    for (int j = threadIdx.x; j < kAcfLagTile; j += kAcfThreads) {
        const int64_t tau = tile_lo + j;
        if (tau - lag_base >= nlag) continue;
        double v = A[j];
#pragma unroll
        for (int b = 1; b < kAcfWaves; ++b) v = v + A[b * kAcfLagTile + j];
        part[(s * nsuper + S) * pstride + (tau - lag_base)] = v;
    }
}

// f[(m * nd + q) * nlag + j]: acov_k(tau) = superblocks summed in order (part), acov_k(0) likewise (part0); the ratios
// of member m's walkers summed in walker order, then divided by W_m -- as the host sums _autocorr_1d over walkers.  A
// walker whose acov(0) is 0 contributes 1.  member_off: [k + 1] walker offsets.
__global__ void acf_reduce_kernel(const double *__restrict__ part, const double *__restrict__ part0, int64_t nsuper, int64_t pstride,
                                  int64_t nw, int32_t nd, const int64_t *__restrict__ member_off, int32_t k, int64_t nlag,
                                  double *__restrict__ f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)k * nd * nlag) return;
    const int64_t j = i % nlag, mq = i / nlag, q = mq % nd, m = mq / nd;
    const int64_t w0 = member_off[m], w1 = member_off[m + 1];
    double sum = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        const int64_t s = q * nw + w;
        double a0 = 0.0, a = 0.0;
        for (int64_t S = 0; S < nsuper; ++S) {
            a0 = a0 + part0[s * nsuper + S];
            a = a + part[(s * nsuper + S) * pstride + j];
        }
        sum += a0 == 0.0 ? 1.0 : a / a0;
    }
    f[i] = sum / (double)(w1 - w0);
}
