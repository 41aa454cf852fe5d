// Posterior modes of a device chain series (msx_series_modes, msx_series_mode_labels, include/msx.h):
// a Gaussian mixture over d <= MSX_MAX_DIM columns of every member by EM, hard labels, and the members' samples by label.
// mcmc_spec_amd/modes.py is the definition.
//
// A series holds [ndim][nw][cap] doubles; the selection is x[t] = series[discard + t * thin], t < n'.  A JOB is a (member,
// start); its K components' parameters are [c | mu (d) | L packed by rows (d (d + 1) / 2)], c = ln w - sum ln diag L -
// (d / 2) ln 2 pi, in units z = (x - center) / scale.  A sample with a non-finite selected value is bad: it enters no sum.
//   mode_stats_kernel<D>   grid (walker x 4,096-row tile, start x component), 256 threads, lanes on consecutive rows: the
//                          E-step of its rows from the job's parameters (iteration 0: the hard assignment of the start's
//                          thresholds), then S = sum r, sum r z, the upper triangle of sum r z z^T and sum lse in
//                          registers, a fixed tree over the 256 threads, one partial per workgroup;
//   mode_mstep_kernel      one workgroup per job: the partials in (walker, tile) order -> w, mu, Sigma, its Cholesky factor,
//                          loglik, niter, status and the frozen flag, all in device memory;
//   mode_label_kernel<D>   grid (walker x tile): argmax_k lp_k per row as uint8 (255: bad), and the tile's count per label;
//   mode_scan_kernel       one workgroup per member: the exclusive scan of those counts in (walker, tile) order per label;
//   mode_scatter_kernel    grid (walker x tile): every row to its label's series at scan + its rank in the tile (ballots).
// A workgroup's sum: thread i adds rows i, i + 256, .. of its tile one after the other, then the tree; the M-step adds the
// workgroups' partials one after the other.  So the order of every sum depends on (n', W_m) alone -- not on thin, discard,
// the buffer's capacity or the other jobs of the launch -- and the bits do not either.  Only plain C++ stores; no atomics;
// no workgroup waits for another; a frozen job's workgroups return on its flag.
#pragma once

constexpr int kModeThreads = 256;     // a workgroup: its stride through its tile, and the width of its tree
constexpr int kModeTile = 4096;       // rows of one workgroup
constexpr int kModeBatch = 8;         // sums that go through the tree together
constexpr int kModeBad = 255;         // the label of a bad sample
constexpr int kModeMaxP = 1 + MSX_MAX_DIM + MSX_MAX_DIM * (MSX_MAX_DIM + 1) / 2;   // a component's parameters
constexpr int kModeMaxAcc = kModeMaxP + 1;                                            // S, S z, S z z^T, lse
constexpr double kModeLn2Pi = 1.8378770664093453;

struct ModeCols { int32_t c[MSX_MAX_DIM]; int32_t n; };   // the columns asked for, by value
struct ModeDst { double *rows; int64_t cap; };            // a label's series: [ndim][1][cap]

// the series' and the job's state, by value
struct ModeSel {
    const double *rows;           // [ndim][nw][cap]
    int64_t cap, nw, np, discard, thin;
    const int64_t *member_off;    // [k + 1]
    int32_t k;
    ModeCols cols;
    const double *center, *scale; // [k][d]
};

__device__ __forceinline__ int mode_member(const int64_t *member_off, int k, int64_t w) {
    int m = 0;
    while (m + 1 < k && member_off[m + 1] <= w) ++m;   // (k <= 64 uniform steps)
    return m;
}

// B sums at once through the fixed tree over the 256 threads: rs[b][0 .. 255] -> rs[b][0]
template <int B>
__device__ __forceinline__ void mode_tree(double (*rs)[kModeThreads]) {
#pragma clang fp contract(off)
    __syncthreads();
    for (int s = kModeThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int b = 0; b < B; ++b) rs[b][threadIdx.x] = rs[b][threadIdx.x] + rs[b][threadIdx.x + s];
        }
        __syncthreads();
    }
}

// lp of one component at z: c - |L^-1 (z - mu)|^2 / 2 by forward substitution; p = [c | mu | L by rows]
template <int D>
__device__ __forceinline__ double mode_lp(const double *p, const double (&z)[D]) {
#pragma clang fp contract(off)
    double y[D];
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = z[i] - p[1 + i];
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double t = p[1 + D + i * (i + 1) / 2 + j] * y[j];
            v = v - t;
        }
        y[i] = v / p[1 + D + i * (i + 1) / 2 + i];
        const double sq = y[i] * y[i];
        q = q + sq;
    }
    const double hq = 0.5 * q;
    return p[0] - hq;
}

// part [start x comp][walker x tile][2 + D + D (D + 1) / 2].  hard != 0: iteration 0, r = (thresholds <= x_c) == comp.
// grid (nw * ntiles, nstarts * ncomp)
template <int D>
__global__ void __launch_bounds__(kModeThreads) mode_stats_kernel(ModeSel S, int32_t nstarts, int32_t ncomp, int32_t hard,
                                                                 const int32_t *__restrict__ split_series_col,
                                                                 const double *__restrict__ split_at,
                                                                 const double *__restrict__ params,
                                                                 const int32_t *__restrict__ frozen, double *__restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NT = D * (D + 1) / 2, P = 1 + D + NT, NACC = P + 1;
    __shared__ double rs[kModeBatch][kModeThreads];
    __shared__ double prm[MSX_MODES_MAX][P];
    __shared__ double cs[2][D];
    __shared__ double thr[MSX_MODES_MAX];
    const int64_t ntiles = (S.np + kModeTile - 1) / kModeTile;
    const int64_t w = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int start = blockIdx.y / ncomp, comp = blockIdx.y % ncomp;
    const int m = mode_member(S.member_off, S.k, w);
    const int64_t job = (int64_t)m * nstarts + start;
    if (frozen[job]) return;
    if (hard) {
        if ((int)threadIdx.x < ncomp - 1) thr[threadIdx.x] = split_at[job * (ncomp - 1) + threadIdx.x];
    } else {
        for (int i = threadIdx.x; i < ncomp * P; i += kModeThreads) prm[i / P][i % P] = params[(job * ncomp + i / P) * P + i % P];
    }
    if ((int)threadIdx.x < D) {
        cs[0][threadIdx.x] = S.center[(int64_t)m * D + threadIdx.x];
        cs[1][threadIdx.x] = S.scale[(int64_t)m * D + threadIdx.x];
    }
    __syncthreads();
    const double *xs = hard ? S.rows + ((int64_t)split_series_col[start] * S.nw + w) * S.cap + S.discard : nullptr;
    double acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.0;
    const int64_t t1 = tile * kModeTile + kModeTile < S.np ? tile * kModeTile + kModeTile : S.np;
    for (int64_t t = tile * kModeTile + threadIdx.x; t < t1; t += kModeThreads) {
        double z[D];
        bool good = true;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const double x = S.rows[((int64_t)S.cols.c[q] * S.nw + w) * S.cap + S.discard + t * S.thin];
            good = good && isfinite(x);
            const double dv = x - cs[0][q];
            z[q] = dv / cs[1][q];
        }
        if (!good) continue;
        double r, lse;
        if (hard) {
            const double x = xs[t * S.thin];
            int c = 0;
            for (int j = 0; j < ncomp - 1; ++j) c += thr[j] <= x ? 1 : 0;
            r = c == comp ? 1.0 : 0.0;
            lse = 0.0;
        } else {
            double lp[MSX_MODES_MAX];
#pragma unroll
            for (int j = 0; j < MSX_MODES_MAX; ++j) lp[j] = -INFINITY;
#pragma unroll 1
            for (int kk = 0; kk < ncomp; ++kk) {   // (a loop, so that a component's parameters are read where they are used)
                const double v = mode_lp<D>(prm[kk], z);
#pragma unroll
                for (int j = 0; j < MSX_MODES_MAX; ++j) lp[j] = j == kk ? v : lp[j];
            }
            double mx = -INFINITY, mine = -INFINITY;
#pragma unroll
            for (int j = 0; j < MSX_MODES_MAX; ++j) {
                mx = lp[j] > mx ? lp[j] : mx;
                mine = j == comp ? lp[j] : mine;
            }
            double se = 0.0;
#pragma unroll
            for (int kk = 0; kk < MSX_MODES_MAX; ++kk)
                if (kk < ncomp) {
                    const double e = exp(lp[kk] - mx);
                    se = se + e;
                }
            lse = mx + log(se);
            r = exp(mine - lse);
        }
        acc[0] = acc[0] + r;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const double rz = r * z[q];
            acc[1 + q] = acc[1 + q] + rz;
#pragma unroll
            for (int e = q; e < D; ++e) {
                const double rzz = rz * z[e];
                // pair (q, e), q <= e, in the order (0,0) (0,1) .. (0,D-1) (1,1) ..
                acc[1 + D + q * D - q * (q - 1) / 2 + (e - q)] = acc[1 + D + q * D - q * (q - 1) / 2 + (e - q)] + rzz;
            }
        }
        acc[NACC - 1] = acc[NACC - 1] + lse;
    }
    double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NACC;
#pragma unroll
    for (int a0 = 0; a0 < NACC; a0 += kModeBatch) {
#pragma unroll
        for (int b = 0; b < kModeBatch; ++b) rs[b][threadIdx.x] = a0 + b < NACC ? acc[a0 + b < NACC ? a0 + b : 0] : 0.0;
        mode_tree<kModeBatch>(rs);
        if ((int)threadIdx.x < kModeBatch && a0 + (int)threadIdx.x < NACC) out[a0 + threadIdx.x] = rs[threadIdx.x][0];
        __syncthreads();
    }
}

// One job's M-step after iteration `it` (0: the hard assignment).  params [job][K][P]; weight [job][K], mean [job][K][d],
// cov [job][K][d][d]; loglik, prev, ngood [job]; niter, status, frozen [job].  grid k * nstarts, 256 threads
__global__ void __launch_bounds__(kModeThreads) mode_mstep_kernel(const double *__restrict__ part, const int64_t *__restrict__ member_off,
                                                                 int64_t nw, int64_t ntiles, int32_t nstarts, int32_t ncomp, int32_t d,
                                                                 int32_t it, int32_t max_iter, double tol, double ridge,
                                                                 double *__restrict__ params, double *__restrict__ weight,
                                                                 double *__restrict__ mean, double *__restrict__ cov,
                                                                 double *__restrict__ loglik, double *__restrict__ prev,
                                                                 double *__restrict__ ngood, int32_t *__restrict__ niter,
                                                                 int32_t *__restrict__ status, int32_t *__restrict__ frozen) {
#pragma clang fp contract(off)
    __shared__ double sm[MSX_MODES_MAX][kModeMaxAcc];
    __shared__ double mu[MSX_MODES_MAX][MSX_MAX_DIM];
    __shared__ double sg[MSX_MODES_MAX][MSX_MAX_DIM][MSX_MAX_DIM];
    __shared__ double lo[MSX_MODES_MAX][MSX_MAX_DIM][MSX_MAX_DIM];
    __shared__ int collapsed;
    __shared__ double good;
    const int64_t job = blockIdx.x;
    if (frozen[job]) return;
    const int m = (int)(job / nstarts), start = (int)(job % nstarts);
    const int64_t w0 = member_off[m], w1 = member_off[m + 1];
    const int nt = d * (d + 1) / 2, P = 1 + d + nt, nacc = P + 1;
    const int i = threadIdx.x;
    if (i < ncomp * nacc) {
        const int kk = i / nacc, a = i % nacc;
        const double *src = part + ((int64_t)(start * ncomp + kk) * (nw * ntiles)) * nacc + a;
        double s = 0.0;
        for (int64_t w = w0; w < w1; ++w)
            for (int64_t tile = 0; tile < ntiles; ++tile) s = s + src[(w * ntiles + tile) * nacc];
        sm[kk][a] = s;
    }
    __syncthreads();
    if (i == 0) {
        int bad = 0;
        double tot = 0.0;
        for (int kk = 0; kk < ncomp; ++kk) {
            bad |= !(sm[kk][0] >= 1.0);
            tot = tot + sm[kk][0];
        }
        if (it == 0) ngood[job] = tot;   // (0 / 1 responsibilities: an exact count)
        good = it == 0 ? tot : ngood[job];
        collapsed = bad;
    }
    __syncthreads();
    const double ll = sm[0][nacc - 1];
    if (collapsed) {
        if (i == 0) {
            if (it > 0) { loglik[job] = ll; niter[job] = it; }
            status[job] = 2;
            frozen[job] = 1;
        }
        return;
    }
    if (i < ncomp) {
        const int kk = i;
        const double s0 = sm[kk][0], wgt = s0 / good;
        for (int q = 0; q < d; ++q) mu[kk][q] = sm[kk][1 + q] / s0;
        int p = 1 + d;
        for (int q = 0; q < d; ++q)
            for (int e = q; e < d; ++e, ++p) {
                const double a = sm[kk][p] / s0;
                const double b = mu[kk][q] * mu[kk][e];
                double v = a - b;
                if (e == q) v = v + ridge;
                sg[kk][q][e] = v;
                sg[kk][e][q] = v;
            }
        double logdet = 0.0;
        for (int r = 0; r < d; ++r)
            for (int c = 0; c <= r; ++c) {
                double s = sg[kk][r][c];
                for (int j = 0; j < c; ++j) {
                    const double t = lo[kk][r][j] * lo[kk][c][j];
                    s = s - t;
                }
                if (r == c) {
                    lo[kk][r][c] = sqrt(s);
                    logdet = logdet + log(lo[kk][r][c]);
                } else {
                    lo[kk][r][c] = s / lo[kk][c][c];
                }
            }
        double *pp = params + (job * ncomp + kk) * P;
        const double hd = 0.5 * (double)d;
        const double cst = hd * kModeLn2Pi;
        const double lw = log(wgt) - logdet;
        pp[0] = lw - cst;
        for (int q = 0; q < d; ++q) pp[1 + q] = mu[kk][q];
        for (int r = 0; r < d; ++r)
            for (int c = 0; c <= r; ++c) pp[1 + d + r * (r + 1) / 2 + c] = lo[kk][r][c];
        weight[job * ncomp + kk] = wgt;
        for (int q = 0; q < d; ++q) {
            mean[(job * ncomp + kk) * d + q] = mu[kk][q];
            for (int e = 0; e < d; ++e) cov[((job * ncomp + kk) * d + q) * d + e] = sg[kk][q][e];
        }
    }
    if (i == 0 && it > 0) {
        loglik[job] = ll;
        niter[job] = it;
        const double df = ll - prev[job];
        const double lim = tol * fabs(ll);
        if (it >= 2 && fabs(df) <= lim) {
            status[job] = 0;
            frozen[job] = 1;
        } else {
            status[job] = 1;
        }
        prev[job] = ll;
    }
}

// labels [nw][n'] and tilecount [walker x tile][MSX_MODES_MAX]: params [k][K][P] (one start per member).  grid nw * ntiles
template <int D>
__global__ void __launch_bounds__(kModeThreads) mode_label_kernel(ModeSel S, int32_t ncomp, const double *__restrict__ params,
                                                                 uint8_t *__restrict__ labels, int64_t *__restrict__ tilecount) {
#pragma clang fp contract(off)
    constexpr int NT = D * (D + 1) / 2, P = 1 + D + NT;
    __shared__ int32_t ri[MSX_MODES_MAX][kModeThreads];
    __shared__ double prm[MSX_MODES_MAX][P];
    __shared__ double cs[2][D];
    const int64_t ntiles = (S.np + kModeTile - 1) / kModeTile;
    const int64_t w = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int m = mode_member(S.member_off, S.k, w);
    for (int i = threadIdx.x; i < ncomp * P; i += kModeThreads) prm[i / P][i % P] = params[((int64_t)m * ncomp + i / P) * P + i % P];
    if ((int)threadIdx.x < D) {
        cs[0][threadIdx.x] = S.center[(int64_t)m * D + threadIdx.x];
        cs[1][threadIdx.x] = S.scale[(int64_t)m * D + threadIdx.x];
    }
    __syncthreads();
    int32_t cnt[MSX_MODES_MAX];
#pragma unroll
    for (int kk = 0; kk < MSX_MODES_MAX; ++kk) cnt[kk] = 0;
    const int64_t t1 = tile * kModeTile + kModeTile < S.np ? tile * kModeTile + kModeTile : S.np;
    for (int64_t t = tile * kModeTile + threadIdx.x; t < t1; t += kModeThreads) {
        double z[D];
        bool good = true;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const double x = S.rows[((int64_t)S.cols.c[q] * S.nw + w) * S.cap + S.discard + t * S.thin];
            good = good && isfinite(x);
            const double dv = x - cs[0][q];
            z[q] = dv / cs[1][q];
        }
        int lab = kModeBad;
        if (good) {
            double best = -INFINITY;
            lab = 0;
#pragma unroll 1
            for (int kk = 0; kk < ncomp; ++kk) {
                const double lp = mode_lp<D>(prm[kk], z);
                if (lp > best) {   // (the lowest k on ties; a NaN never wins)
                    best = lp;
                    lab = kk;
                }
            }
#pragma unroll
            for (int kk = 0; kk < MSX_MODES_MAX; ++kk) cnt[kk] += lab == kk ? 1 : 0;
        }
        labels[w * S.np + t] = (uint8_t)lab;
    }
#pragma unroll
    for (int kk = 0; kk < MSX_MODES_MAX; ++kk) ri[kk][threadIdx.x] = cnt[kk];
    __syncthreads();
    for (int s = kModeThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int kk = 0; kk < MSX_MODES_MAX; ++kk) ri[kk][threadIdx.x] += ri[kk][threadIdx.x + s];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < MSX_MODES_MAX) tilecount[(int64_t)blockIdx.x * MSX_MODES_MAX + threadIdx.x] = ri[threadIdx.x][0];
}

// base [walker x tile][MSX_MODES_MAX]: the rows of label j before this tile among the member's, walker then tile ascending;
// total [k][MSX_MODES_MAX].  grid k, MSX_MODES_MAX threads
__global__ void __launch_bounds__(MSX_MODES_MAX) mode_scan_kernel(const int64_t *__restrict__ tilecount, const int64_t *__restrict__ member_off,
                                                                 int64_t ntiles, int64_t *__restrict__ base, int64_t *__restrict__ total) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x, i0 = member_off[m] * ntiles, i1 = member_off[m + 1] * ntiles;
    const int j = threadIdx.x;
    int64_t run = 0;
    for (int64_t i = i0; i < i1; ++i) {
        base[i * MSX_MODES_MAX + j] = run;
        run += tilecount[i * MSX_MODES_MAX + j];
    }
    total[m * MSX_MODES_MAX + j] = run;
}

// every labelled row's ndim coordinates to dst[m * ncomp + label], at base + its rank among the tile's rows of that label
// (ballot prefixes: rows ascending).  grid nw * ntiles
__global__ void __launch_bounds__(kModeThreads) mode_scatter_kernel(ModeSel S, int32_t ndim, int32_t ncomp, const uint8_t *__restrict__ labels,
                                                                   const int64_t *__restrict__ base, const ModeDst *__restrict__ dst) {
#pragma clang fp contract(off)
    constexpr int kWaves = kModeThreads / 64;
    __shared__ int32_t wtot[kWaves][MSX_MODES_MAX];
    const int64_t ntiles = (S.np + kModeTile - 1) / kModeTile;
    const int64_t w = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int m = mode_member(S.member_off, S.k, w);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t run[MSX_MODES_MAX];
#pragma unroll
    for (int j = 0; j < MSX_MODES_MAX; ++j) run[j] = base[(int64_t)blockIdx.x * MSX_MODES_MAX + j];
    for (int pass = 0; pass < kModeTile / kModeThreads; ++pass) {   // (uniform: every thread takes every pass)
        const int64_t t = tile * kModeTile + (int64_t)pass * kModeThreads + threadIdx.x;
        const int lab = t < S.np ? (int)labels[w * S.np + t] : kModeBad;
        int before[MSX_MODES_MAX];
#pragma unroll
        for (int j = 0; j < MSX_MODES_MAX; ++j) {
            const unsigned long long b = __ballot(lab == j);
            before[j] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wtot[wave][j] = __popcll(b);
        }
        __syncthreads();
        int64_t pos = -1;
        int mine = 0;
#pragma unroll
        for (int j = 0; j < MSX_MODES_MAX; ++j) {
            int ahead = 0, all = 0;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                ahead += v < wave ? wtot[v][j] : 0;
                all += wtot[v][j];
            }
            if (lab == j) {
                pos = run[j] + ahead + before[j];
                mine = j;
            }
            run[j] += all;
        }
        if (pos >= 0 && mine < ncomp) {
            const ModeDst D = dst[(int64_t)m * ncomp + mine];
            if (pos < D.cap)
                for (int c = 0; c < ndim; ++c) D.rows[(int64_t)c * D.cap + pos] = S.rows[((int64_t)c * S.nw + w) * S.cap + S.discard + t * S.thin];
        }
        __syncthreads();
    }
}

#define MSX_MODE_INSTANCES(D)                                                                                                    \
    template __global__ void mode_stats_kernel<D>(ModeSel, int32_t, int32_t, int32_t, const int32_t *, const double *, const double *, \
                                                  const int32_t *, double *);                                                     \
    template __global__ void mode_label_kernel<D>(ModeSel, int32_t, const double *, uint8_t *, int64_t *);
MSX_MODE_INSTANCES(1) MSX_MODE_INSTANCES(2) MSX_MODE_INSTANCES(3) MSX_MODE_INSTANCES(4)
MSX_MODE_INSTANCES(5) MSX_MODE_INSTANCES(6) MSX_MODE_INSTANCES(7) MSX_MODE_INSTANCES(8)
#undef MSX_MODE_INSTANCES
