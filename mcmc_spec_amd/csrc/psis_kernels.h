// Pareto-smoothed importance sampling of a log-weight series (msx_series_psis, include/msx.h): the
// generalised Pareto fit of Zhang & Stephens (2009) to the largest weights of every member, its shape khat, and the weights
// with their tail replaced by the fitted quantiles (Vehtari, Simpson, Gelman, Yao & Gabry 2024).  mcmc_spec_amd/psis.py is the
// definition.
//
// A series holds [ndim][nw][cap] doubles; the selection, the members and the FLAT index i = t * W_m + (w - off[m]) are
// reweight_kernels.h's.  The cutoff's order statistic comes from the multi-workgroup radix selection (summary_kernels.h) before
// these kernels run; here
//   psis_scan_kernel    one workgroup per walker: the maximum of the selection's values that are not bad, and how many are bad;
//   psis_fill_kernel    rows [0, n) of the outputs: weight 0, log-weight -inf (the selected rows are overwritten next);
//   psis_reduce_kernel  one workgroup per member: the shifted values into the weights' rows, the tail (value, 32-bit flat
//                       index) compacted into LDS in whatever order the lanes arrive, a bitonic sort there by (value, index)
//                       -- a total order, so the arrival order leaves no trace --, the fit, the replacement, the scatter, the
//                       maximum, the log-sum-exp and the final weights.
// LDS: MSX_PSIS_TAIL_MAX values (8 B) and indices (4 B) = 48 KB, and under 5 KB of sums and fit tables: three workgroups fit a CU's
// 160 KiB, and a launch has one workgroup per member.
// SUMS over the tail: lane l of 256 adds elements l, l + 256, .. one after the other, then rw_tree.  Sums over the member: lane
// l adds, walker after walker, the selection's rows l, l + 256, .., then rw_tree.  The integer count of bad values is an
// integer atomicAdd; the tail's slots come from an integer atomicAdd in LDS.  Only plain C++ stores; no float atomics; no
// workgroup waits for another.
#pragma once

constexpr int kPsThreads = 256;
constexpr int kPsTailMax = MSX_PSIS_TAIL_MAX;
constexpr int kPsFitMax = 96;    // m = 30 + floor(sqrt(n)) <= 94 for n <= 4096
static_assert((kPsTailMax & (kPsTailMax - 1)) == 0, "the sort pads the tail to a power of two");
static_assert(kPsThreads == kRwThreads, "rw_tree adds over the workgroup's 256 lanes");

// pmax [nw]: the maximum of walker w's selected values that are not bad (-inf: none); nbad [k] += its bad ones.  grid nw
__global__ void __launch_bounds__(kPsThreads) psis_scan_kernel(const double *__restrict__ logw, int64_t cap, int64_t np, int64_t discard,
                                                              int64_t thin, const int64_t *__restrict__ member_off, int32_t k,
                                                              double *__restrict__ pmax, unsigned long long *__restrict__ nbad) {
    __shared__ double rm[kPsThreads];
    __shared__ long long rc[kPsThreads];
    const int64_t w = blockIdx.x;
    const double *x = logw + w * cap + discard;
    double mx = -INFINITY;
    long long bad = 0;
    for (int64_t t = threadIdx.x; t < np; t += kPsThreads) {
        const double v = x[t * thin];
        if (rw_bad(v)) ++bad;
        else if (v > mx) mx = v;
    }
    rm[threadIdx.x] = mx;
    rc[threadIdx.x] = bad;
    __syncthreads();
    for (int s = kPsThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            if (rm[threadIdx.x + s] > rm[threadIdx.x]) rm[threadIdx.x] = rm[threadIdx.x + s];
            rc[threadIdx.x] += rc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pmax[w] = rm[0];
        if (rc[0] > 0) atomicAdd(nbad + rw_member(member_off, k, w), (unsigned long long)rc[0]);   // (integers: any order)
    }
}

// wt[w][t] = 0 and lwt[w][t] = -inf (lwt may be null) for t < n.  grid (row tiles, nw)
__global__ void __launch_bounds__(kPsThreads) psis_fill_kernel(int64_t n, double *__restrict__ wt, int64_t wcap, double *__restrict__ lwt,
                                                              int64_t lcap) {
    const int64_t t = (int64_t)blockIdx.x * kPsThreads + threadIdx.x, w = blockIdx.y;
    if (t >= n) return;
    wt[w * wcap + t] = 0.0;
    if (lwt) lwt[w * lcap + t] = -INFINITY;
}

// the workgroup's sum of v in the fixed tree, on every lane
__device__ __forceinline__ double psis_sum(double v, double *rs) {
    __syncthreads();   // (every lane has read the previous result)
    rs[threadIdx.x] = v;
    rw_tree(rs);
    return rs[0];
}
__device__ __forceinline__ double psis_max(double v, double *rs) {
    __syncthreads();
    rs[threadIdx.x] = v;
    __syncthreads();
    for (int s = kPsThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && rs[threadIdx.x + s] > rs[threadIdx.x]) rs[threadIdx.x] = rs[threadIdx.x + s];
        __syncthreads();
    }
    return rs[0];
}

// the tail in LDS and the tables of its fit
struct PsisTail {
    double *key;         // [MSX_PSIS_TAIL_MAX] the shifted values, then the exceedances, then the fitted quantiles
    unsigned int *idx;   // [MSX_PSIS_TAIL_MAX] the samples' indices
    double *rs;          // [256] the sums' tree
    double *fb, *fL, *fw;   // [kPsFitMax] b_i, L_i, w_i
    double *bbar;
};

// key / idx [0, n) ascending by (value, index): a bitonic sort over the next power of two, padded with (+inf, 2^32 - 1).  All
// lanes call it after a barrier behind the last write; it ends with one.
__device__ __forceinline__ void psis_sort(const PsisTail &T, int n) {
    const int tid = threadIdx.x;
    int P = 1;
    while (P < n) P <<= 1;
    for (int j = n + tid; j < P; j += kPsThreads) {
        T.key[j] = INFINITY;
        T.idx[j] = 0xffffffffu;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kPsThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = T.key[i], b = T.key[l];
                    const unsigned int ia = T.idx[i], ib = T.idx[l];
                    const bool gt = a > b || (a == b && ia > ib);
                    if (gt == ((i & k2) == 0)) {
                        T.key[i] = b; T.key[l] = a;
                        T.idx[i] = ib; T.idx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
}

// The sorted tail key[0, n), n >= MSX_PSIS_MIN_TAIL, shifted values above `cutoff`: Zhang & Stephens' fit of t_j = exp(key_j) -
// exp(cutoff) and key_j = min(log(exp(cutoff) + the fitted quantile at (j + 0.5) / n), 0).  Returns khat on every lane; ends
// with a barrier.
__device__ __forceinline__ double psis_fit_replace(const PsisTail &T, int n, double cutoff) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double *key = T.key;
    const double dn = (double)n, exp_c = exp(cutoff);
    for (int j = tid; j < n; j += kPsThreads) key[j] = exp(key[j]) - exp_c;
    __syncthreads();
    const int mf = 30 + (int)floor(sqrt(dn));
    const double tq = key[(int)(dn / 4.0 + 0.5) - 1], tl = key[n - 1], dm = (double)mf;
    if (tid < mf) {
        const double r = sqrt(dm / ((double)(tid + 1) - 0.5));
        T.fb[tid] = 1.0 / tl + (1.0 - r) / (3.0 * tq);
    }
    __syncthreads();
    for (int i = 0; i < mf; ++i) {
        const double b = T.fb[i];
        double part = 0.0;
        for (int j = tid; j < n; j += kPsThreads) part = part + log1p(-b * key[j]);
        const double ki = psis_sum(part, T.rs) / dn;
        if (tid == 0) T.fL[i] = dn * (log(-b / ki) - ki - 1.0);
    }
    __syncthreads();
    if (tid < mf) {
        double s = 0.0;
        for (int l = 0; l < mf; ++l) s = s + exp(T.fL[l] - T.fL[tid]);
        T.fw[tid] = 1.0 / s;
    }
    __syncthreads();
    if (tid == 0) {
        double sb = 0.0, sw = 0.0;
        for (int i = 0; i < mf; ++i) {
            sb = sb + T.fb[i] * T.fw[i];
            sw = sw + T.fw[i];
        }
        *T.bbar = sb / sw;
    }
    __syncthreads();
    const double b = *T.bbar;
    double part = 0.0;
    for (int j = tid; j < n; j += kPsThreads) part = part + log1p(-b * key[j]);
    const double kf = psis_sum(part, T.rs) / dn;
    const double sigma = -kf / b;
    const double khat = (dn * kf + 5.0) / (dn + 10.0);
    __syncthreads();
    for (int j = tid; j < n; j += kPsThreads) {
        const double l1 = log1p(-((double)j + 0.5) / dn);
        const double q = fabs(khat) < 1e-30 ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
        const double v = log(exp_c + q);
        key[j] = v > 0.0 ? 0.0 : v;
    }
    __syncthreads();
    return khat;
}

struct PsisArgs {
    const double *logw;          // the log-weights' series rows (ndim = 1)
    int64_t cap;
    int64_t np, discard, thin;
    const int64_t *member_off;   // [k + 1] walkers
    const double *pmax;          // [nw] psis_scan_kernel's
    const double *cut;           // [k] the order statistic of rank S - tail_len - 1, as a log-weight (not shifted)
    double *wt;                  // the weights' series rows
    int64_t wcap;
    double *lwt;                 // the normalised log-weights' rows, or null
    int64_t lcap;
    double *res;                 // [k][3]: khat, status, tail count
    long long *tail_index;       // [k][MSX_PSIS_TAIL_MAX] or null
};

// grid k
__global__ void __launch_bounds__(kPsThreads) psis_reduce_kernel(PsisArgs A) {
#pragma clang fp contract(off)
    __shared__ double key[kPsTailMax];
    __shared__ unsigned int idx[kPsTailMax];
    __shared__ double rs[kPsThreads];
    __shared__ double fb[kPsFitMax], fL[kPsFitMax], fw[kPsFitMax];
    __shared__ unsigned int cnt;
    __shared__ double bbar;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int64_t w0 = A.member_off[m], w1 = A.member_off[m + 1], W = w1 - w0, np = A.np;
    double *ro = A.res + (int64_t)m * 3;
    long long *ti = A.tail_index ? A.tail_index + (int64_t)m * kPsTailMax : nullptr;
    if (ti)
        for (int j = tid; j < kPsTailMax; j += kPsThreads) ti[j] = -1;
    double M = -INFINITY;
    for (int64_t w = w0; w < w1; ++w)
        if (A.pmax[w] > M) M = A.pmax[w];
    if (M == -INFINITY) {   // nothing finite: the fill kernel's zeros stand
        if (tid == 0) {
            ro[0] = INFINITY;
            ro[1] = (double)MSX_PSIS_SHORT_TAIL;
            ro[2] = 0.0;
        }
        return;
    }
    const double xc = A.cut[m] - M;
    const double cutoff = xc > MSX_PSIS_LOG_TINY ? xc : MSX_PSIS_LOG_TINY;
    if (tid == 0) cnt = 0u;
    __syncthreads();
    // the shifted values into the weights' rows; the tail into LDS
    for (int64_t w = w0; w < w1; ++w) {
        const double *lx = A.logw + w * A.cap + A.discard;
        double *wx = A.wt + w * A.wcap + A.discard;
        for (int64_t t = tid; t < np; t += kPsThreads) {
            const double v = lx[t * A.thin];
            const bool bad = rw_bad(v);
            const double x = v - M;
            wx[t * A.thin] = bad ? -INFINITY : x;
            if (!bad && x > cutoff) {
                const unsigned int slot = atomicAdd(&cnt, 1u);
                if (slot < (unsigned int)kPsTailMax) {   // (the host has checked tail_len: the tail cannot be longer)
                    key[slot] = x;
                    idx[slot] = (unsigned int)(t * W + (w - w0));
                }
            }
        }
    }
    __syncthreads();
    const int n = cnt < (unsigned int)kPsTailMax ? (int)cnt : kPsTailMax;
    const PsisTail T{key, idx, rs, fb, fL, fw, &bbar};
    psis_sort(T, n);
    if (ti)
        for (int j = tid; j < n; j += kPsThreads) ti[j] = (long long)idx[j];
    double khat = INFINITY;
    if (n >= MSX_PSIS_MIN_TAIL) {
        khat = psis_fit_replace(T, n, cutoff);
        for (int j = tid; j < n; j += kPsThreads) {
            const int64_t i = idx[j];
            A.wt[(w0 + i % W) * A.wcap + A.discard + (i / W) * A.thin] = key[j];
        }
    }
    if (tid == 0) {
        ro[0] = khat;
        ro[1] = (double)(n >= MSX_PSIS_MIN_TAIL ? MSX_PSIS_OK : MSX_PSIS_SHORT_TAIL);
        ro[2] = (double)n;
    }
    __threadfence_block();
    __syncthreads();   // (the scattered values are read by other lanes below)
    double mx = -INFINITY;
    for (int64_t w = w0; w < w1; ++w) {
        const double *wx = A.wt + w * A.wcap + A.discard;
        for (int64_t t = tid; t < np; t += kPsThreads) {
            const double v = wx[t * A.thin];
            if (v > mx) mx = v;
        }
    }
    const double top = psis_max(mx, rs);
    double part = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        const double *wx = A.wt + w * A.wcap + A.discard;
        for (int64_t t = tid; t < np; t += kPsThreads) part = part + exp(wx[t * A.thin] - top);
    }
    const double lse = top + log(psis_sum(part, rs));
    for (int64_t w = w0; w < w1; ++w) {
        double *wx = A.wt + w * A.wcap + A.discard;
        double *lx = A.lwt ? A.lwt + w * A.lcap + A.discard : nullptr;
        for (int64_t t = tid; t < np; t += kPsThreads) {
            const double v = wx[t * A.thin];
            wx[t * A.thin] = exp(v - top);
            if (lx) lx[t * A.thin] = v - lse;
        }
    }
}
