// The split pool of a device chain series, transformed: average ranks by a segmented radix sort, normal scores, folding
// and indicators (msx_series_split_transform), and the chain-averaged autocovariance of a series whose walkers are the
// chains (msx_series_chain_acov); include/msx.h, DESIGN.md section 26.  mcmc_spec_amd/diagnostics.py is the definition.
//
// The selection x = rows[0:n][discard::thin] (n' rows) of a source member of W walkers becomes a member of J = 2 W walkers
// and h = n' / 2 rows of dst: walker j = 2 w + half holds rows [0, h) or [n' - h, n') of source walker w (diag_kernels.h's
// half-chains).  A SEGMENT is one (member, column): S = h J values, element e = j h + i.  Its ranks come from a sort of
// (key, e) pairs -- the key is summary_kernels.h's order-preserving image of the double with -0 folded onto +0 -- by
// least-significant-digit radix passes of 8 bits over tiles of kRankTile elements, one workgroup per tile, a tile never
// crossing a segment:
//   rank_key_kernel      keys and positions of a round's segments; every segment's counts of all eight digits (atomicAdd),
//                        from which the host drops the passes whose digit is the same all over every segment;
//   rank_hist_kernel     a pass's digit counts per tile (plain stores into the tile's own row);
//   rank_scan_kernel     one workgroup per segment: per digit the tiles' counts become offsets, tiles in order; the digits'
//                        totals become bases;
//   rank_scatter_kernel  the tile's pairs to base + tile offset + their STABLE place inside the tile;
//   rank_flag_kernel     after the last pass: per tile the first and the last index at which a run of equal keys begins;
//   rank_assign_kernel   every element's run [a, b) -> twice its average rank a + b + 1 -> the value, stored at the place
//                        of dst the position names.
// Three launches per pass; no workgroup waits for another inside a launch.  The place of a pair inside a tile is its
// count of earlier pairs with its digit, found by ballots in element order, so the sort is stable and its output does not
// depend on the order in which anything lands; the only atomics are integer counts.  Ranks are integers, and the normal
// score is AS 241's PPND16 with the coefficients of diagnostics.ndtri in the same order, float64 + - * /, log and sqrt.
// Only plain C++ stores and atomicAdd.
#pragma once

constexpr int kRankThreads = 256;
constexpr int kRankPer = 8;                               // elements per thread
constexpr int kRankTile = kRankThreads * kRankPer;        // 2048 elements per workgroup
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankDigitBits = 8;
constexpr int kRankDigits = 1 << kRankDigitBits;
constexpr int kRankPasses = 64 / kRankDigitBits;

// transforms (MSX_SPLIT_* of include/msx.h)
constexpr int kSplitIdentity = 0, kSplitRanknorm = 1, kSplitFoldRanknorm = 2, kSplitIndicator = 3, kSplitRank2 = 4;

// One (member, column) of a round.  base: its first pair in the round's key / position arrays; tile0: its first row in
// the per-tile tables.
struct RankSeg {
    int64_t base, S, tile0, ntiles;
    int64_t w0;          // the member's first SOURCE walker (its first walker of dst is 2 w0)
    double param;        // FOLD_RANKNORM: the median; INDICATOR: the threshold
    uint32_t col;        // the column's code
    int32_t jc;          // the column's index in dst
};

// the source selection and the destination's layout
struct RankGeom {
    const double *rows;  // source [ndim][nw][cap]
    int64_t cap, nw, np, h, discard, thin;
    double *dst;         // destination [ncols][2 nw][dcap]
    int64_t dcap;
};

// element e of a segment: the source value, and its place in dst
__device__ __forceinline__ double rank_src(const RankGeom &g, const RankSeg &s, int64_t e) {
    const int64_t j = e / g.h, i = e - j * g.h;
    const SumCol c = sum_col(g.rows, g.cap, g.nw, s.w0 + (j >> 1), g.discard, s.col);
    return c.at(((j & 1) ? g.np - g.h + i : i) * g.thin);
}
__device__ __forceinline__ int64_t rank_dst(const RankGeom &g, const RankSeg &s, int64_t e) {
    const int64_t j = e / g.h, i = e - j * g.h;
    return ((int64_t)s.jc * 2 * g.nw + 2 * s.w0 + j) * g.dcap + i;
}

// the sort's key: -0 and +0 tie; every NaN above +inf
__device__ __forceinline__ unsigned long long rank_key(double y) { return sum_key(y == 0.0 ? 0.0 : y); }
__device__ __forceinline__ bool rank_key_finite(unsigned long long k) { return k > 0x000fffffffffffffull && k < 0xfff0000000000000ull; }

// AS 241, PPND16: diagnostics.ndtri's arithmetic, term by term
#define RANK_H8(c0, c1, c2, c3, c4, c5, c6, c7, r) ((((((((c7) * (r) + (c6)) * (r) + (c5)) * (r) + (c4)) * (r) + (c3)) * (r) + (c2)) * (r) + (c1)) * (r) + (c0))
__device__ __forceinline__ double rank_ndtri(double p) {
#pragma clang fp contract(off)
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = RANK_H8(3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                                   4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3, r);
        const double den = RANK_H8(1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
                                   3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3, r);
        return q * num / den;
    }
    if (!(p > 0.0 && p < 1.0)) return p == 0.0 ? -INFINITY : (p == 1.0 ? INFINITY : NAN);
    double r = sqrt(-log(q < 0.0 ? p : 1.0 - p)), v;
    if (r <= 5.0) {
        r = r - 1.6;
        const double num = RANK_H8(1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                                   1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4, r);
        const double den = RANK_H8(1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                                   1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9, r);
        v = num / den;
    } else {
        r = r - 5.0;
        const double num = RANK_H8(6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                                   2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7, r);
        const double den = RANK_H8(1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                                   1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15, r);
        v = num / den;
    }
    return q < 0.0 ? -v : v;
}

// IDENTITY and INDICATOR: element by element, no sort.  grid (tiles of the largest segment, segments)
__global__ void __launch_bounds__(kRankThreads) rank_plain_kernel(RankGeom g, const RankSeg *__restrict__ segs, int32_t transform) {
#pragma clang fp contract(off)
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    const int64_t e0 = (int64_t)blockIdx.x * kRankTile;
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + u * kRankThreads + threadIdx.x;
        if (e >= s.S) break;
        const double x = rank_src(g, s, e);
        g.dst[rank_dst(g, s, e)] = transform == kSplitIndicator ? (x != x || s.param != s.param ? NAN : (x <= s.param ? 1.0 : 0.0)) : x;
    }
}

// keys[base + e], pos[base + e] = e; hist8[(segment * 8 + pass) * 256 + digit] += 1.  grid (tiles, segments)
__global__ void __launch_bounds__(kRankThreads) rank_key_kernel(RankGeom g, const RankSeg *__restrict__ segs, int32_t transform,
                                                               unsigned long long *__restrict__ keys, uint32_t *__restrict__ pos,
                                                               uint32_t *__restrict__ hist8) {
#pragma clang fp contract(off)
    __shared__ unsigned int bins[kRankPasses * kRankDigits];
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    for (int i = threadIdx.x; i < kRankPasses * kRankDigits; i += kRankThreads) bins[i] = 0u;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kRankTile;
    for (int u = 0; u < kRankPer; ++u) {   // (uniform trips: sel_count needs whole waves)
        const int64_t e = e0 + u * kRankThreads + threadIdx.x;
        const bool ok = e < s.S;
        unsigned long long key = 0ull;
        if (ok) {
            const double x = rank_src(g, s, e);
            key = rank_key(transform == kSplitFoldRanknorm ? fabs(x - s.param) : x);
            keys[s.base + e] = key;
            pos[s.base + e] = (uint32_t)e;
        }
#pragma unroll
        for (int p = 0; p < kRankPasses; ++p)
            sel_count(bins + p * kRankDigits, ok, (unsigned int)(key >> (p * kRankDigitBits)) & (unsigned int)(kRankDigits - 1));
    }
    __syncthreads();
    uint32_t *h = hist8 + (int64_t)blockIdx.y * (kRankPasses * kRankDigits);
    for (int i = threadIdx.x; i < kRankPasses * kRankDigits; i += kRankThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(h + i, v);
    }
}

// tile_hist[(tile0 + tile) * 256 + digit] = the tile's keys with that digit at `shift`.  grid (tiles, segments)
__global__ void __launch_bounds__(kRankThreads) rank_hist_kernel(const RankSeg *__restrict__ segs, const unsigned long long *__restrict__ keys,
                                                                int32_t shift, uint32_t *__restrict__ tile_hist) {
    __shared__ unsigned int bins[kRankDigits];
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kRankTile;
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + u * kRankThreads + threadIdx.x;
        const bool ok = e < s.S;
        const unsigned long long key = ok ? keys[s.base + e] : 0ull;
        sel_count(bins, ok, (unsigned int)(key >> shift) & (unsigned int)(kRankDigits - 1));
    }
    __syncthreads();
    tile_hist[(s.tile0 + blockIdx.x) * kRankDigits + threadIdx.x] = bins[threadIdx.x];
}

// Per segment: thread d turns the tiles' counts of digit d into the offsets of the tiles among the keys with that digit
// (tiles in order); the digits' totals, scanned in digit order, are digit_base[segment * 256 + d].  grid segments
__global__ void __launch_bounds__(kRankDigits) rank_scan_kernel(const RankSeg *__restrict__ segs, uint32_t *__restrict__ tile_hist,
                                                               uint32_t *__restrict__ digit_base) {
    __shared__ unsigned int tot[kRankDigits];
    const RankSeg s = segs[blockIdx.x];
    const int d = threadIdx.x;
    unsigned int run = 0u;
    for (int64_t t = 0; t < s.ntiles; ++t) {
        uint32_t *p = tile_hist + (s.tile0 + t) * kRankDigits + d;
        const unsigned int v = *p;
        *p = run;
        run += v;
    }
    tot[d] = run;
    __syncthreads();
    for (int step = 1; step < kRankDigits; step <<= 1) {   // inclusive scan of the totals
        const unsigned int add = d >= step ? tot[d - step] : 0u;
        __syncthreads();
        tot[d] += add;
        __syncthreads();
    }
    digit_base[(int64_t)blockIdx.x * kRankDigits + d] = tot[d] - run;
}

// The tile's pairs to their places of the pass.  Wave v owns the tile's elements [512 v, 512 v + 512) in eight steps of
// 64; in a step the lanes that share a digit find each other by eight ballots, the lowest of them takes the wave's count
// of that digit so far (an atomicAdd on a counter no other wave touches) and hands it to the others, and a lane's place is
// that count plus the lanes below it with its digit: element order, whatever the hardware does first.
__global__ void __launch_bounds__(kRankThreads) rank_scatter_kernel(const RankSeg *__restrict__ segs, const unsigned long long *__restrict__ keys_in,
                                                                   const uint32_t *__restrict__ pos_in, int32_t shift,
                                                                   const uint32_t *__restrict__ tile_hist, const uint32_t *__restrict__ digit_base,
                                                                   unsigned long long *__restrict__ keys_out, uint32_t *__restrict__ pos_out) {
    __shared__ unsigned int cnt[kRankWaves * kRankDigits];
    __shared__ unsigned int start[kRankDigits];
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    for (int i = threadIdx.x; i < kRankWaves * kRankDigits; i += kRankThreads) cnt[i] = 0u;
    start[threadIdx.x] = tile_hist[(s.tile0 + blockIdx.x) * kRankDigits + threadIdx.x] + digit_base[(int64_t)blockIdx.y * kRankDigits + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t e0 = (int64_t)blockIdx.x * kRankTile + (int64_t)wave * (64 * kRankPer);
    unsigned long long key[kRankPer];
    uint32_t pv[kRankPer], place[kRankPer];
    unsigned int *mine = cnt + wave * kRankDigits;
#pragma unroll
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + u * 64 + lane;
        const bool ok = e < s.S;
        key[u] = ok ? keys_in[s.base + e] : 0ull;
        pv[u] = ok ? pos_in[s.base + e] : 0u;
        const unsigned int digit = (unsigned int)(key[u] >> shift) & (unsigned int)(kRankDigits - 1);
        unsigned long long peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < kRankDigitBits; ++b) {
            const unsigned long long has = __ballot((digit >> b) & 1u);
            peers &= ((digit >> b) & 1u) ? has : ~has;
        }
        const int leader = ok ? __ffsll((long long)peers) - 1 : lane;
        unsigned int before = 0u;
        if (ok && lane == leader) before = atomicAdd(mine + digit, (unsigned int)__popcll(peers));
        before = (unsigned int)__shfl((int)before, leader);
        place[u] = before + (unsigned int)__popcll(peers & below);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + u * 64 + lane;
        if (e >= s.S) continue;
        const unsigned int digit = (unsigned int)(key[u] >> shift) & (unsigned int)(kRankDigits - 1);
        unsigned int at = start[digit] + place[u];
        for (int v = 0; v < wave; ++v) at += cnt[v * kRankDigits + digit];
        if ((int64_t)at < s.S) {   // (always: the offsets are counts of these keys)
            keys_out[s.base + at] = key[u];
            pos_out[s.base + at] = pv[u];
        }
    }
}

// the smallest (op 0) or largest (op 1) of the threads' values; the result is red[0]
__device__ __forceinline__ void rank_minmax(long long *red, long long v, int op) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int st = kRankThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const long long a = red[threadIdx.x], b = red[threadIdx.x + st];
            red[threadIdx.x] = op ? (a > b ? a : b) : (a < b ? a : b);
        }
        __syncthreads();
    }
}

// A run of equal keys begins at index i of the sorted segment when i == 0 or key[i] != key[i - 1].  Per tile: the first
// such index (S when none) and the last (-1 when none).  grid (tiles, segments)
__global__ void __launch_bounds__(kRankThreads) rank_flag_kernel(const RankSeg *__restrict__ segs, const unsigned long long *__restrict__ keys,
                                                                long long *__restrict__ tile_first, long long *__restrict__ tile_last) {
    __shared__ long long red[kRankThreads];
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    const int64_t e0 = (int64_t)blockIdx.x * kRankTile;
    long long first = s.S, last = -1;
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + u * kRankThreads + threadIdx.x;
        if (e >= s.S) break;
        if (e == 0 || keys[s.base + e] != keys[s.base + e - 1]) {
            first = e < first ? e : first;
            last = e;
        }
    }
    rank_minmax(red, first, 0);
    if (threadIdx.x == 0) tile_first[s.tile0 + blockIdx.x] = red[0];
    __syncthreads();
    rank_minmax(red, last, 1);
    if (threadIdx.x == 0) tile_last[s.tile0 + blockIdx.x] = red[0];
}

// Every element of the sorted segment: its run [a, b) of equal keys -- a the last run start at or before it, b the first
// after it, looked for in its tile and then in the other tiles' tables -- has the ranks a + 1 .. b, so twice its average
// rank is a + b + 1.  The value goes to the place of dst its position names: twice the rank (RANK2), or the normal score
// ndtri((r - 3/8) / (S + 1/4)); NaN all over a segment that holds a non-finite value or one distinct value.  Thread i owns
// the tile's elements 8 i .. 8 i + 7.  grid (tiles, segments)
__global__ void __launch_bounds__(kRankThreads) rank_assign_kernel(RankGeom g, const RankSeg *__restrict__ segs, int32_t transform,
                                                                  const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ pos,
                                                                  const long long *__restrict__ tile_first, const long long *__restrict__ tile_last) {
#pragma clang fp contract(off)
    __shared__ unsigned long long lk[kRankTile + 1];
    __shared__ long long red[kRankThreads];
    __shared__ long long scan_a[kRankThreads], scan_b[kRankThreads];
    const RankSeg s = segs[blockIdx.y];
    if ((int64_t)blockIdx.x >= s.ntiles) return;
    const int64_t tile = blockIdx.x, e0 = tile * kRankTile;
    // the run that reaches into the tile from the left, and the first run start to the right of it
    long long v = -1;
    for (int64_t t = threadIdx.x; t < tile; t += kRankThreads) {
        const long long c = tile_last[s.tile0 + t];
        v = c > v ? c : v;
    }
    rank_minmax(red, v, 1);
    const long long carry_a = red[0];
    __syncthreads();
    v = s.S;
    for (int64_t t = tile + 1 + threadIdx.x; t < s.ntiles; t += kRankThreads) {
        const long long c = tile_first[s.tile0 + t];
        v = c < v ? c : v;
    }
    rank_minmax(red, v, 0);
    const long long carry_b = red[0];
    // lk[1 + i] = key[e0 + i], lk[0] = the key before the tile
    for (int i = threadIdx.x; i < kRankTile + 1; i += kRankThreads) {
        const int64_t e = e0 + i - 1;
        lk[i] = e >= 0 && e < s.S ? keys[s.base + e] : 0ull;
    }
    __syncthreads();
    const unsigned long long kmin = keys[s.base], kmax = keys[s.base + s.S - 1];
    const bool bad = kmin == kmax || !rank_key_finite(kmin) || !rank_key_finite(kmax);
    bool flag[kRankPer];
    long long a[kRankPer], b[kRankPer];
    long long la = -1, lb = s.S;
#pragma unroll
    for (int u = 0; u < kRankPer; ++u) {
        const int i = threadIdx.x * kRankPer + u;
        const int64_t e = e0 + i;
        flag[u] = e < s.S && (e == 0 || lk[i + 1] != lk[i]);
        if (flag[u]) la = e;
        a[u] = la;
    }
#pragma unroll
    for (int u = kRankPer - 1; u >= 0; --u) {
        b[u] = lb;
        if (flag[u]) lb = e0 + threadIdx.x * kRankPer + u;
    }
    // la: the thread's last run start (-1: none); lb: its first (S: none).  Scans over the threads, both ways
    scan_a[threadIdx.x] = la;
    scan_b[threadIdx.x] = lb;
    __syncthreads();
    for (int step = 1; step < kRankThreads; step <<= 1) {
        const int t = threadIdx.x;
        const long long pa = t >= step ? scan_a[t - step] : -1;
        const long long pb = t + step < kRankThreads ? scan_b[t + step] : (long long)s.S;
        __syncthreads();
        scan_a[t] = pa > scan_a[t] ? pa : scan_a[t];
        scan_b[t] = pb < scan_b[t] ? pb : scan_b[t];
        __syncthreads();
    }
    long long left = threadIdx.x > 0 ? scan_a[threadIdx.x - 1] : -1;
    long long right = threadIdx.x + 1 < kRankThreads ? scan_b[threadIdx.x + 1] : (long long)s.S;
    left = carry_a > left ? carry_a : left;
    right = carry_b < right ? carry_b : right;
    const double denom = (double)s.S + 0.25;
#pragma unroll
    for (int u = 0; u < kRankPer; ++u) {
        const int64_t e = e0 + threadIdx.x * kRankPer + u;
        if (e >= s.S) continue;
        const long long ra = a[u] > left ? a[u] : left, rb = b[u] < right ? b[u] : right;
        const double twice = (double)(ra + rb + 1);
        double out;
        if (bad) out = NAN;
        else if (transform == kSplitRank2) out = twice;
        else out = rank_ndtri((twice / 2.0 - 0.375) / denom);
        const int64_t at = (int64_t)pos[s.base + e];
        if (at < s.S) g.dst[rank_dst(g, s, at)] = out;
    }
}

// ---- the chain-averaged autocovariance (msx_series_chain_acov): autocorr_kernels.h's sums, not normalised ----------------
// acov[(m * nd + q) * nlag + j] = (sum over member m's chains, in walker order, of acov_w(lag_base + j)) / (W_m n'), every
// acov_w = the superblocks' partial sums in order (acf_lag_kernel's `part`).  One thread per (member, column, lag).
__global__ void acov_reduce_kernel(const double *__restrict__ part, int64_t nsuper, int64_t pstride, int64_t nw, int32_t nd,
                                   const int64_t *__restrict__ member_off, int32_t k, int64_t nlag, int64_t np, double *__restrict__ acov) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)k * nd * nlag) return;
    const int64_t j = i % nlag, mq = i / nlag, q = mq % nd, m = mq / nd;
    const int64_t w0 = member_off[m], w1 = member_off[m + 1];
    double sum = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        const int64_t sidx = q * nw + w;
        double a = 0.0;
        for (int64_t S = 0; S < nsuper; ++S) a = a + part[(sidx * nsuper + S) * pstride + j];
        sum = sum + a;
    }
    acov[i] = sum / ((double)(w1 - w0) * (double)np);
}

// between[m * nd + q] = var (ddof = 1) of the chains' means of member m, in walker order.  One thread per (member, column).
__global__ void acov_between_kernel(const double *__restrict__ mean, int64_t nw, int32_t nd, const int64_t *__restrict__ member_off, int32_t k,
                                    double *__restrict__ between) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)k * nd) return;
    const int64_t q = i % nd, m = i / nd, w0 = member_off[m], w1 = member_off[m + 1];
    double sum = 0.0;
    for (int64_t w = w0; w < w1; ++w) sum = sum + mean[q * nw + w];
    const double mbar = sum / (double)(w1 - w0);
    double ss = 0.0;
    for (int64_t w = w0; w < w1; ++w) {
        const double d = mean[q * nw + w] - mbar;
        ss = ss + d * d;
    }
    between[i] = ss / (double)(w1 - w0 - 1);
}
