// Importance reweighting of a device chain series (msx_series_logprob / _lincomb / _weights / _wmoments / _resample,
// include/msx.h): log-probabilities of chain rows as a series, log-weights as a linear combination of
// series columns, the weights and Kish's effective sample size, weighted moments, and systematic resampling.
//
// A series holds [ndim][nw][cap] doubles.  For walker w the selection is x[t] = series[discard + t * thin], t < n'; member
// m's FLAT sample is in (row, walker) order: flat index i = t * W_m + (w - off[m]), N_m = n' W_m of them.
//
// SUMS (weights' statistics, the weighted moments) are the evidence kernels' order: one workgroup per walker, thread i adds
// the walker's elements i, i + 256, ... one after the other, a fixed tree over the 256 threads, then the member's walkers in
// walker order.  The order depends on (n', W_m) alone.
//
// THE PREFIX SUMS of msx_series_resample are a three-phase scan over tiles of MSX_RESAMPLE_TILE consecutive flat samples:
//   rw_scan_local_kernel  one workgroup per tile: lane l of 256 adds its MSX_RESAMPLE_TILE / 256 consecutive values one
//                         after the other (s_0 = v_0, s_e = s_{e-1} + v_e); the lanes' totals are scanned serially in lane
//                         order (E_0 = 0, E_{l+1} = E_l + total_l); local_i = E_l + s_e.  The tile's sum is E_256.
//   rw_scan_tiles_kernel  one workgroup per member: the tiles' sums scanned serially in tile order (B_0 = 0, B_{j+1} = B_j +
//                         sum_j); W = B_{ntiles}.
//   rw_scan_add_kernel    C_i = B_tile + local_i.
// Both serial levels are what makes C non-decreasing for non-negative weights IN FLOATING POINT: a lane's last local value
// is exactly the next lane's base, a tile's last C is exactly the next tile's base, and x -> base + x is monotone.  "The
// first i with C_i > t" is then one well-defined index and a binary search finds it.  A tree or a look-back at either level
// would leave C off by an ulp across a boundary and the drawn index would depend on how the search walks.  The bits of C
// depend on the N_m values alone.  Only plain C++ stores; no float atomics; no workgroup waits for another.
#pragma once

constexpr int kRwThreads = 256;
constexpr int kRwTile = MSX_RESAMPLE_TILE;
constexpr int kRwPer = kRwTile / kRwThreads;   // consecutive values per lane
constexpr int kRwMaxSrc = 8;                   // msx_series_lincomb's terms
constexpr unsigned int kRwStream = 15;         // the counter generator's stream of u0 (the samplers draw from streams 0 .. 14)
static_assert(kRwTile % kRwThreads == 0, "a tile is a whole number of values per lane");

// the member of walker w (k <= 64 uniform steps)
__device__ __forceinline__ int rw_member(const int64_t *__restrict__ member_off, int32_t k, int64_t w) {
    int m = 0;
    while (m + 1 < k && member_off[m + 1] <= w) ++m;
    return m;
}

// the fixed tree over rs[0 .. 255]; the result is rs[0]
__device__ __forceinline__ void rw_tree(double *rs) {
#pragma clang fp contract(off)
    __syncthreads();
    for (int s = kRwThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + s];
        __syncthreads();
    }
}
__device__ __forceinline__ void rw_tree_i64(long long *rs) {
    __syncthreads();
    for (int s = kRwThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) rs[threadIdx.x] = rs[threadIdx.x] + rs[threadIdx.x + s];
        __syncthreads();
    }
}

// ---- msx_series_logprob: rows of one member <-> the evaluation's [n][ndim] batch ----------------------------------------
// theta [(r * W + j) * ndim + d] = series[d][w0 + j][row0 + r], r < nrows, j < W
__global__ void rw_gather_theta_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, int32_t ndim, int64_t w0, int64_t W,
                                       int64_t row0, int64_t nrows, double *__restrict__ theta) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = nrows * W * ndim;
    if (i >= total) return;
    const int64_t r = i % nrows, rest = i / nrows, j = rest % W, d = rest / W;   // (consecutive threads read consecutive rows)
    theta[(r * W + j) * ndim + d] = rows[(d * nw + w0 + j) * cap + row0 + r];
}

// dst[0][w0 + j][row0 + r] = the sample's value: a rejected sample -inf, an error status NaN; worst[0] = the worst status
__global__ void rw_put_logp_kernel(const double *__restrict__ logp, const int32_t *__restrict__ status, int64_t W, int64_t nrows,
                                   int64_t w0, int64_t row0, double *__restrict__ dst, int64_t dcap, int32_t *__restrict__ worst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = nrows * W;
    if (i >= total) return;
    const int64_t r = i % nrows, j = i / nrows;
    const int32_t st = status[r * W + j];
    double v = logp[r * W + j];
    if (st == MSX_W_REJECT) v = -INFINITY;
    if (st > MSX_W_REJECT) {
        v = __longlong_as_double(0x7ff8000000000000ll);
        atomicMax(worst, st);   // (an integer maximum: the same whatever the order)
    }
    dst[(w0 + j) * dcap + row0 + r] = v;
}

// ---- msx_series_lincomb ---------------------------------------------------------------------------------------------------
struct RwTerms {
    const double *p[kRwMaxSrc];   // the term's column: series rows + col * nw * cap
    int64_t cap[kRwMaxSrc];
    double coef[kRwMaxSrc];
    int32_t n;
};

// dst[0][w][row] = ((coef_0 x_0) + coef_1 x_1) + ...: a product, then an addition, in term order.  grid (row tiles, nw)
__global__ void __launch_bounds__(kRwThreads) rw_lincomb_kernel(RwTerms T, int64_t row0, int64_t nrows, double *__restrict__ dst, int64_t dcap) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * kRwThreads + threadIdx.x, w = blockIdx.y;
    if (r >= nrows) return;
    double acc = T.coef[0] * T.p[0][w * T.cap[0] + row0 + r];
    for (int j = 1; j < T.n; ++j) {
        const double term = T.coef[j] * T.p[j][w * T.cap[j] + row0 + r];
        acc = acc + term;
    }
    dst[w * dcap + row0 + r] = acc;
}

// ---- msx_series_weights ---------------------------------------------------------------------------------------------------
// "bad": NaN or +inf
__device__ __forceinline__ bool rw_bad(double v) { return v != v || v == INFINITY; }

// pmax [nw]: the maximum of walker w's values of rows [0, n) that are not bad (-inf when there is none)
__global__ void __launch_bounds__(kRwThreads) rw_max_kernel(const double *__restrict__ logw, int64_t cap, int64_t n, double *__restrict__ pmax) {
    __shared__ double rm[kRwThreads];
    const int64_t w = blockIdx.x;
    const double *x = logw + w * cap;
    double mx = -INFINITY;
    for (int64_t t = threadIdx.x; t < n; t += kRwThreads) {
        const double v = x[t];
        if (!rw_bad(v) && v > mx) mx = v;
    }
    rm[threadIdx.x] = mx;
    __syncthreads();
    for (int s = kRwThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && rm[threadIdx.x + s] > rm[threadIdx.x]) rm[threadIdx.x] = rm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) pmax[w] = rm[0];
}

// out[0][w][t] = exp(logw - M_m) for every row t < n; a bad value, and every value of a member without a finite one: 0.
// grid (row tiles, nw)
__global__ void __launch_bounds__(kRwThreads) rw_exp_kernel(const double *__restrict__ logw, int64_t cap, int64_t n,
                                                           const int64_t *__restrict__ member_off, int32_t k,
                                                           const double *__restrict__ pmax, double *__restrict__ out, int64_t ocap) {
#pragma clang fp contract(off)
    __shared__ double sM;
    const int64_t w = blockIdx.y;
    if (threadIdx.x == 0) {
        const int m = rw_member(member_off, k, w);
        double M = -INFINITY;
        for (int64_t j = member_off[m]; j < member_off[m + 1]; ++j)
            if (pmax[j] > M) M = pmax[j];
        sM = M;
    }
    __syncthreads();
    const double M = sM;
    const int64_t t = (int64_t)blockIdx.x * kRwThreads + threadIdx.x;
    if (t >= n) return;
    const double v = logw[w * cap + t];
    const double diff = v - M;
    out[w * ocap + t] = (rw_bad(v) || M == -INFINITY) ? 0.0 : exp(diff);
}

// pcnt [2][nw] (bad, zero) and psum [2][nw] (sum w, sum w^2) of walker w's selection.  grid nw
__global__ void __launch_bounds__(kRwThreads) rw_stat_kernel(const double *__restrict__ logw, int64_t cap, const double *__restrict__ wt,
                                                            int64_t wcap, int64_t nw, int64_t np, int64_t discard, int64_t thin,
                                                            long long *__restrict__ pcnt, double *__restrict__ psum) {
#pragma clang fp contract(off)
    __shared__ double rs[kRwThreads];
    __shared__ long long rc[kRwThreads];
    const int64_t w = blockIdx.x;
    const double *lx = logw + w * cap + discard, *wx = wt + w * wcap + discard;
    double s1 = 0.0, s2 = 0.0;
    long long nbad = 0, nzero = 0;
    for (int64_t t = threadIdx.x; t < np; t += kRwThreads) {
        const double v = wx[t * thin];
        const double sq = v * v;
        s1 = s1 + v;
        s2 = s2 + sq;
        const bool bad = rw_bad(lx[t * thin]);
        nbad += bad ? 1 : 0;
        nzero += (!bad && v == 0.0) ? 1 : 0;
    }
    rs[threadIdx.x] = s1;
    rw_tree(rs);
    if (threadIdx.x == 0) psum[w] = rs[0];
    __syncthreads();
    rs[threadIdx.x] = s2;
    rw_tree(rs);
    if (threadIdx.x == 0) psum[nw + w] = rs[0];
    rc[threadIdx.x] = nbad;
    rw_tree_i64(rc);
    if (threadIdx.x == 0) pcnt[w] = rc[0];
    __syncthreads();
    rc[threadIdx.x] = nzero;
    rw_tree_i64(rc);
    if (threadIdx.x == 0) pcnt[nw + w] = rc[0];
}

// stats [k][6]: count, nbad, nzero, sum w, sum w^2, (sum w)^2 / sum w^2 (0 when nothing weighs).  one thread per member
__global__ void rw_stat_combine_kernel(const long long *__restrict__ pcnt, const double *__restrict__ psum,
                                       const int64_t *__restrict__ member_off, int32_t k, int64_t nw, int64_t np,
                                       double *__restrict__ stats) {
#pragma clang fp contract(off)
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= k) return;
    const int64_t w0 = member_off[m], w1 = member_off[m + 1];
    double s1 = 0.0, s2 = 0.0;
    long long nbad = 0, nzero = 0;
    for (int64_t w = w0; w < w1; ++w) {
        s1 = s1 + psum[w];
        s2 = s2 + psum[nw + w];
        nbad += pcnt[w];
        nzero += pcnt[nw + w];
    }
    const double sq = s1 * s1;
    double *o = stats + (int64_t)m * 6;
    o[0] = (double)(np * (w1 - w0));
    o[1] = (double)nbad;
    o[2] = (double)nzero;
    o[3] = s1;
    o[4] = s2;
    o[5] = s2 > 0.0 ? sq / s2 : 0.0;
}

// ---- msx_series_wmoments --------------------------------------------------------------------------------------------------
struct RwCols { int32_t c[MSX_MAX_DIM]; int32_t n; };

// psum [nc + 1][nw]: q < nc: sum of w x_q; q == nc: sum of w.  A zero weight enters no sum.  grid (nw, nc + 1)
__global__ void __launch_bounds__(kRwThreads) rw_wsum_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, RwCols cols,
                                                            const double *__restrict__ wt, int64_t wcap, int64_t np, int64_t discard,
                                                            int64_t thin, double *__restrict__ psum) {
#pragma clang fp contract(off)
    __shared__ double rs[kRwThreads];
    const int64_t w = blockIdx.x;
    const int q = blockIdx.y;
    const double *wx = wt + w * wcap + discard;
    const double *x = q < cols.n ? rows + ((int64_t)cols.c[q] * nw + w) * cap + discard : nullptr;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < np; t += kRwThreads) {
        const double v = wx[t * thin];
        if (v == 0.0) continue;
        const double term = x ? v * x[t * thin] : v;
        acc = acc + term;
    }
    rs[threadIdx.x] = acc;
    rw_tree(rs);
    if (threadIdx.x == 0) psum[(int64_t)q * nw + w] = rs[0];
}

// sumw [k], mean [k][nc]: the walkers' sums in walker order; mean = sum w x / sum w.  grid k, MSX_MAX_DIM + 1 threads
__global__ void __launch_bounds__(MSX_MAX_DIM + 1) rw_wmean_kernel(const double *__restrict__ psum, const int64_t *__restrict__ member_off,
                                                                  int64_t nw, int32_t nc, double *__restrict__ sumw,
                                                                  double *__restrict__ mean) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int q = threadIdx.x;
    if (q > nc) return;
    double sw = 0.0, s = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        sw = sw + psum[(int64_t)nc * nw + w];
        s = s + psum[(int64_t)q * nw + w];
    }
    if (q == nc) sumw[m] = sw;
    else mean[m * nc + q] = s / sw;
}

// pair p of nc columns in the order (0,0) (0,1) .. (0,nc-1) (1,1) ..
__device__ __forceinline__ void rw_pair(int p, int nc, int *d, int *e) {
    int a = 0;
    while (p >= nc - a) {
        p -= nc - a;
        ++a;
    }
    *d = a;
    *e = a + p;
}

// pcross [npairs][nw]: sum of w ((x_d - mean_d)(x_e - mean_e)), the member's means.  grid (nw, npairs)
__global__ void __launch_bounds__(kRwThreads) rw_wcross_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, RwCols cols,
                                                              const double *__restrict__ wt, int64_t wcap, int64_t np, int64_t discard,
                                                              int64_t thin, const int64_t *__restrict__ member_off, int32_t k,
                                                              const double *__restrict__ mean, double *__restrict__ pcross) {
#pragma clang fp contract(off)
    __shared__ double rs[kRwThreads];
    const int64_t w = blockIdx.x;
    const int p = blockIdx.y;
    const int m = rw_member(member_off, k, w);
    int d, e;
    rw_pair(p, cols.n, &d, &e);
    const double md = mean[(int64_t)m * cols.n + d], me = mean[(int64_t)m * cols.n + e];
    const double *xd = rows + ((int64_t)cols.c[d] * nw + w) * cap + discard;
    const double *xe = rows + ((int64_t)cols.c[e] * nw + w) * cap + discard;
    const double *wx = wt + w * wcap + discard;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < np; t += kRwThreads) {
        const double v = wx[t * thin];
        if (v == 0.0) continue;
        const double a = xd[t * thin] - md;
        const double b = xe[t * thin] - me;
        const double pr = a * b;
        const double term = v * pr;
        acc = acc + term;
    }
    rs[threadIdx.x] = acc;
    rw_tree(rs);
    if (threadIdx.x == 0) pcross[(int64_t)p * nw + w] = rs[0];
}

// cov [k][nc][nc]: the walkers' cross sums in walker order over sum w, mirrored.  grid k, MSX_MAX_DIM (MSX_MAX_DIM + 1) / 2 threads
__global__ void rw_wcov_kernel(const double *__restrict__ pcross, const int64_t *__restrict__ member_off, int64_t nw, int32_t nc,
                               const double *__restrict__ sumw, double *__restrict__ cov) {
#pragma clang fp contract(off)
    const int64_t m = blockIdx.x, w0 = member_off[m], w1 = member_off[m + 1];
    const int i = threadIdx.x;
    if (i >= nc * (nc + 1) / 2) return;
    int d, e;
    rw_pair(i, nc, &d, &e);
    double s = 0.0;
    for (int64_t w = w0; w < w1; ++w) s = s + pcross[(int64_t)i * nw + w];
    const double v = s / sumw[m];
    cov[(m * nc + d) * nc + e] = v;
    cov[(m * nc + e) * nc + d] = v;
}

// ---- msx_series_resample --------------------------------------------------------------------------------------------------
// What the scan kernels know of the call: member m's tiles are tile_off[m] .. tile_off[m + 1] - 1 of the launch, its flat
// samples samp_off[m] .. of C.
struct RwScan {
    const double *wt;            // the weights' series rows (ndim = 1)
    int64_t wcap;
    int64_t np, discard, thin;
    const int64_t *member_off;   // [k + 1] walkers
    const int64_t *tile_off;     // [k + 1]
    const int64_t *samp_off;     // [k + 1]
    int32_t k;
};

// local [sum N]: the tile-local inclusive scan; tsum [tiles]; tlast [tiles]: the tile's last flat index with w > 0 (-1:
// none); tbad [tiles]: its values that are negative, NaN or infinite.  grid tiles
__global__ void __launch_bounds__(kRwThreads) rw_scan_local_kernel(RwScan S, double *__restrict__ local, double *__restrict__ tsum,
                                                                  long long *__restrict__ tlast, long long *__restrict__ tbad) {
#pragma clang fp contract(off)
    __shared__ double base[kRwThreads];
    __shared__ long long rl[kRwThreads], rb[kRwThreads];
    const int64_t tile = blockIdx.x;
    const int m = rw_member(S.tile_off, S.k, tile);
    const int64_t w0 = S.member_off[m], W = S.member_off[m + 1] - w0, N = S.np * W;
    const int64_t i0 = (tile - S.tile_off[m]) * kRwTile + (int64_t)threadIdx.x * kRwPer;
    double s[kRwPer];
    double run = 0.0;
    long long last = -1, bad = 0;
    for (int e = 0; e < kRwPer; ++e) {
        const int64_t i = i0 + e;
        double v = 0.0;
        if (i < N) {
            v = S.wt[(w0 + i % W) * S.wcap + S.discard + (i / W) * S.thin];
            if (v > 0.0) last = i;
            if (!(v >= 0.0) || v == INFINITY) ++bad;
        }
        run = e == 0 ? v : run + v;
        s[e] = run;
    }
    base[threadIdx.x] = run;
    rl[threadIdx.x] = last;
    rb[threadIdx.x] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {   // the lanes' totals, serially in lane order: base[l] = E_l, the tile's sum = E_256
        double acc = 0.0;
        long long la = -1, ba = 0;
        for (int l = 0; l < kRwThreads; ++l) {
            const double t = base[l];
            base[l] = acc;
            acc = acc + t;
            la = rl[l] > la ? rl[l] : la;
            ba += rb[l];
        }
        tsum[tile] = acc;
        tlast[tile] = la;
        tbad[tile] = ba;
    }
    __syncthreads();
    const double E = base[threadIdx.x];
    for (int e = 0; e < kRwPer; ++e) {
        const int64_t i = i0 + e;
        if (i < N) local[S.samp_off[m] + i] = E + s[e];
    }
}

// tsum [tiles] -> the tiles' exclusive bases in place, serially in tile order; total [k] = W; mlast [k], mbad [k].  grid k
__global__ void __launch_bounds__(kRwThreads) rw_scan_tiles_kernel(const int64_t *__restrict__ tile_off, double *__restrict__ tsum,
                                                                  const long long *__restrict__ tlast, const long long *__restrict__ tbad,
                                                                  double *__restrict__ total, long long *__restrict__ mlast,
                                                                  long long *__restrict__ mbad) {
#pragma clang fp contract(off)
    __shared__ double buf[kRwTile];
    __shared__ long long rl[kRwThreads], rb[kRwThreads];
    __shared__ double carry;
    const int m = blockIdx.x;
    const int64_t t0 = tile_off[m], t1 = tile_off[m + 1];
    long long last = -1, bad = 0;
    if (threadIdx.x == 0) carry = 0.0;
    for (int64_t c0 = t0; c0 < t1; c0 += kRwTile) {
        const int64_t cnt = t1 - c0 < kRwTile ? t1 - c0 : kRwTile;
        __syncthreads();
        for (int64_t j = threadIdx.x; j < cnt; j += kRwThreads) {
            buf[j] = tsum[c0 + j];
            last = tlast[c0 + j] > last ? tlast[c0 + j] : last;
            bad += tbad[c0 + j];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double acc = carry;
            for (int64_t j = 0; j < cnt; ++j) {
                const double t = buf[j];
                buf[j] = acc;
                acc = acc + t;
            }
            carry = acc;
        }
        __syncthreads();
        for (int64_t j = threadIdx.x; j < cnt; j += kRwThreads) tsum[c0 + j] = buf[j];
    }
    rl[threadIdx.x] = last;
    rb[threadIdx.x] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long la = -1, ba = 0;
        for (int l = 0; l < kRwThreads; ++l) {
            la = rl[l] > la ? rl[l] : la;
            ba += rb[l];
        }
        total[m] = carry;
        mlast[m] = la;
        mbad[m] = ba;
    }
}

// C_i = B_tile + local_i, in place.  grid tiles
__global__ void __launch_bounds__(kRwThreads) rw_scan_add_kernel(RwScan S, const double *__restrict__ tbase, double *__restrict__ C) {
#pragma clang fp contract(off)
    const int64_t tile = blockIdx.x;
    const int m = rw_member(S.tile_off, S.k, tile);
    const int64_t N = S.np * (S.member_off[m + 1] - S.member_off[m]);
    const int64_t i0 = (tile - S.tile_off[m]) * kRwTile + (int64_t)threadIdx.x * kRwPer;
    const double B = tbase[tile];
    for (int e = 0; e < kRwPer; ++e) {
        const int64_t i = i0 + e;
        if (i < N) {
            const int64_t at = S.samp_off[m] + i;
            C[at] = B + C[at];
        }
    }
}

// one member's draw: t_j = (j + u0) * step in two roundings, j < nout
struct RwDraw {
    double step, u0;
    int64_t nout, last;   // last: the last flat index with w > 0
    int64_t out_off;      // the member's first entry of idx
    double *dst;          // the member's dst rows [ndim][1][dcap] (nullptr with nout == 0)
    int64_t dcap;
};

// sample j = the first i with C_i > t_j, clamped to `last`; all ndim coordinates of it to row j of the member's dst, and i
// to idx.  grid (ceil(max nout / 256), k)
__global__ void __launch_bounds__(kRwThreads) rw_draw_kernel(RwScan S, const double *__restrict__ C, const RwDraw *__restrict__ draws,
                                                            const double *__restrict__ rows, int64_t cap, int64_t nw, int32_t ndim,
                                                            long long *__restrict__ idx) {
#pragma clang fp contract(off)
    const int m = blockIdx.y;
    const RwDraw D = draws[m];
    const int64_t j = (int64_t)blockIdx.x * kRwThreads + threadIdx.x;
    if (j >= D.nout) return;
    const int64_t w0 = S.member_off[m], W = S.member_off[m + 1] - w0, N = S.np * W;
    const double *c = C + S.samp_off[m];
    const double pos = (double)j + D.u0;
    const double t = pos * D.step;
    int64_t lo = 0, hi = N;   // the first i in [0, N] with C_i > t (N: none)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (c[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    const int64_t i = lo > D.last ? D.last : lo;
    idx[D.out_off + j] = i;
    const int64_t w = w0 + i % W, r = S.discard + (i / W) * S.thin;
    for (int d = 0; d < ndim; ++d) D.dst[(int64_t)d * D.dcap + j] = rows[((int64_t)d * nw + w) * cap + r];
}
