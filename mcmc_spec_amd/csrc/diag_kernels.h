// Between-walker convergence and plain moments of a device chain series (msx_series_moments, include/msx.h; DESIGN.md
// section 21): what split R-hat is made of (within, var_plus, between) and the pooled mean and covariance of each member.
//
// A series holds [ndim][nw][cap] doubles; for column c, walker w the selection x[t] = series[discard + t * thin], t < n'.
// With h = n' / 2 a walker gives two half-chains, rows [0, h) and [n' - h, n'); half-chain j = 2 w + half.  Five kernels:
//   diag_sum_kernel      one workgroup per (walker, column, part): the sum of half 0, of half 1, and of all n' rows;
//   diag_mean_kernel     one workgroup per member: the walkers' totals in walker order -> the member's mean;
//   diag_dev_kernel      one workgroup per (walker, column, half): sum of (x - m_j)^2, m_j = S_j / h;
//   diag_cross_kernel    one workgroup per (walker, column pair d <= e): sum of (x_d - mean_d)(x_e - mean_e), the MEMBER's means;
//   diag_combine_kernel  one workgroup per member: the half-chains in order j -> within, between, var_plus; the walkers'
//                        cross products in walker order -> cov, mirrored.
// A workgroup's sum: thread i adds its range's elements i, i + 256, ... one after the other, then a fixed tree over the 256
// threads.  So the order of every sum depends on (n', W_m) alone -- not on thin, discard, the buffer's capacity or the
// launch -- and the bits do not either; the loads are one double per lane for thin == 1 as for thin > 1 (consecutive lanes
// read consecutive rows).  tests/diag_numpy.py restates the arithmetic.  Only plain C++ stores; no atomics; no workgroup
// waits for another; everything returned is float64 + - * / (the square root of R-hat is the host's).
#pragma once

constexpr int kDiagThreads = 256;   // one workgroup's stride through its range, and the width of its tree
constexpr int kDiagMaxPairs = MSX_MAX_DIM * (MSX_MAX_DIM + 1) / 2;

struct DiagCols { int32_t c[MSX_MAX_DIM]; int32_t n; };   // the columns asked for, by value (n <= MSX_MAX_DIM)

// the fixed tree over rs[0 .. 255]; the result is rs[0]
__device__ __forceinline__ void diag_tree(double *rs) {
#pragma clang fp contract(off)
    __syncthreads();
    for (int s = kDiagThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + s];
        __syncthreads();
    }
}

// part 0: rows [0, h); part 1: rows [n' - h, n'); part 2: rows [0, n')
__device__ __forceinline__ void diag_range(int64_t np, int part, int64_t *lo, int64_t *hi) {
    const int64_t h = np / 2;
    *lo = part == 1 ? np - h : 0;
    *hi = part == 0 ? h : np;
}

// pair p of nc columns in the order (0,0) (0,1) .. (0,nc-1) (1,1) ..
__device__ __forceinline__ void diag_pair(int p, int nc, int *d, int *e) {
    int a = 0;
    while (p >= nc - a) {   // (at most MSX_MAX_DIM uniform steps)
        p -= nc - a;
        ++a;
    }
    *d = a;
    *e = a + p;
}

// psum [3][nc][nw].  grid (nw, nc, 3)
__global__ void __launch_bounds__(kDiagThreads) diag_sum_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, DiagCols cols,
                                                               int64_t np, int64_t discard, int64_t thin, double *__restrict__ psum) {
#pragma clang fp contract(off)
    __shared__ double rs[kDiagThreads];
    const int64_t w = blockIdx.x;
    const int q = blockIdx.y, part = blockIdx.z;
    int64_t lo, hi;
    diag_range(np, part, &lo, &hi);
    const double *x = rows + ((int64_t)cols.c[q] * nw + w) * cap + discard;
    double acc = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kDiagThreads) acc = acc + x[t * thin];
    rs[threadIdx.x] = acc;
    diag_tree(rs);
    if (threadIdx.x == 0) psum[((int64_t)part * cols.n + q) * nw + w] = rs[0];
}

// mean [k][nc]: the walkers' totals (part 2) in walker order, over N = n' W_m.  grid k, MSX_MAX_DIM threads
__global__ void __launch_bounds__(MSX_MAX_DIM) diag_mean_kernel(const double *__restrict__ psum, const int64_t *__restrict__ member_off,
                                                               int64_t nw, int32_t nc, int64_t np, double *__restrict__ mean) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int q = threadIdx.x;
    if (q >= nc) return;
    double s = 0.0;
    for (int64_t w = w0; w < w1; ++w) s = s + psum[((int64_t)2 * nc + q) * nw + w];
    mean[m * nc + q] = s / (double)(np * (w1 - w0));
}

// pss [2][nc][nw]: sum over the half of (x - m_j)^2, m_j = psum / h.  grid (nw, nc, 2)
__global__ void __launch_bounds__(kDiagThreads) diag_dev_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, DiagCols cols,
                                                               int64_t np, int64_t discard, int64_t thin,
                                                               const double *__restrict__ psum, double *__restrict__ pss) {
#pragma clang fp contract(off)
    __shared__ double rs[kDiagThreads];
    const int64_t w = blockIdx.x;
    const int q = blockIdx.y, part = blockIdx.z;
    int64_t lo, hi;
    diag_range(np, part, &lo, &hi);
    const int64_t at = ((int64_t)part * cols.n + q) * nw + w;
    const double mj = psum[at] / (double)(np / 2);
    const double *x = rows + ((int64_t)cols.c[q] * nw + w) * cap + discard;
    double acc = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kDiagThreads) {
        const double dv = x[t * thin] - mj;
        const double sq = dv * dv;
        acc = acc + sq;
    }
    rs[threadIdx.x] = acc;
    diag_tree(rs);
    if (threadIdx.x == 0) pss[at] = rs[0];
}

// pcross [npairs][nw]: sum over all n' rows of (x_d - mean_d)(x_e - mean_e), the member's means.  grid (nw, npairs)
__global__ void __launch_bounds__(kDiagThreads) diag_cross_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, DiagCols cols,
                                                                 int64_t np, int64_t discard, int64_t thin,
                                                                 const int64_t *__restrict__ member_off, int32_t k,
                                                                 const double *__restrict__ mean, double *__restrict__ pcross) {
#pragma clang fp contract(off)
    __shared__ double rs[kDiagThreads];
    const int64_t w = blockIdx.x;
    const int p = blockIdx.y;
    int m = 0;
    while (m + 1 < k && member_off[m + 1] <= w) ++m;   // (k <= 64 uniform steps)
    int d, e;
    diag_pair(p, cols.n, &d, &e);
    const double md = mean[(int64_t)m * cols.n + d], me = mean[(int64_t)m * cols.n + e];
    const double *xd = rows + ((int64_t)cols.c[d] * nw + w) * cap + discard;
    const double *xe = rows + ((int64_t)cols.c[e] * nw + w) * cap + discard;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < np; t += kDiagThreads) {
        const double a = xd[t * thin] - md;
        const double b = xe[t * thin] - me;
        const double pr = a * b;
        acc = acc + pr;
    }
    rs[threadIdx.x] = acc;
    diag_tree(rs);
    if (threadIdx.x == 0) pcross[(int64_t)p * nw + w] = rs[0];
}

// within, var_plus, between [k][nc]; cov [k][nc][nc] when pcross is given.  grid k, kDiagMaxPairs threads
__global__ void __launch_bounds__(kDiagMaxPairs) diag_combine_kernel(const double *__restrict__ psum, const double *__restrict__ pss,
                                                                    const double *__restrict__ pcross,
                                                                    const int64_t *__restrict__ member_off, int64_t nw, int32_t nc,
                                                                    int64_t np, double *__restrict__ within,
                                                                    double *__restrict__ var_plus, double *__restrict__ between,
                                                                    double *__restrict__ cov) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int i = threadIdx.x;
    const int64_t h = np / 2;
    const double dh = (double)h, dh1 = (double)(h - 1), J = (double)(2 * (w1 - w0)), J1 = (double)(2 * (w1 - w0) - 1);
    if (i < nc) {
        double sm = 0.0, sv = 0.0;
        for (int64_t w = w0; w < w1; ++w)
            for (int part = 0; part < 2; ++part) {
                const int64_t at = ((int64_t)part * nc + i) * nw + w;
                sm = sm + psum[at] / dh;
                sv = sv + pss[at] / dh1;
            }
        const double mbar = sm / J;
        double sb = 0.0;
        for (int64_t w = w0; w < w1; ++w)
            for (int part = 0; part < 2; ++part) {
                const double dv = psum[((int64_t)part * nc + i) * nw + w] / dh - mbar;
                const double sq = dv * dv;
                sb = sb + sq;
            }
        const double wi = sv / J, be = sb / J1;
        const double f = dh1 / dh;
        const double fw = f * wi;
        within[m * nc + i] = wi;
        between[m * nc + i] = be;
        var_plus[m * nc + i] = fw + be;
    }
    if (pcross && i < nc * (nc + 1) / 2) {
        int d, e;
        diag_pair(i, nc, &d, &e);
        double s = 0.0;
        for (int64_t w = w0; w < w1; ++w) s = s + pcross[(int64_t)i * nw + w];
        const double v = s / (double)(np * (w1 - w0) - 1);
        cov[(m * nc + d) * nc + e] = v;
        cov[(m * nc + e) * nc + d] = v;
    }
}
