// Order statistics and binned marginals of chains held on the device (msx_series_order_stats / _hist / _hist2d,
// include/msx.h).  The second consumer of a series, next to autocorr_kernels.h.
//
// A series holds a chain as [ndim][nw][cap] doubles.  The selection is x = rows[0:n][discard::thin] (n' rows); member m
// contributes its W_m walkers, so its flat sample of a column has N_m = n' W_m values.  A COLUMN is a 32-bit code: c < ndim
// is coordinate c, MSX_COL_RATIO(a, b) the correctly rounded quotient x[a] / x[b].  Everything here is integer counts and
// selected elements: no result depends on a summation order.
//
// Every streaming kernel runs on a grid (walker, row tile, column): one workgroup reads one tile of one walker's
// contiguous series (lanes read consecutive rows), counts into LDS with integer atomics and flushes the counters that are
// not zero to a global table with 64-bit adds.  Workgroups are independent; nothing waits inside a launch.
//   sel_pass_kernel  one radix pass of the selection: digit histograms of the keys that carry a rank's prefix;
//   sel_pick_kernel  one wave per (member, column): the digit of every rank, the prefixes of the next pass;
//   hist_kernel      1-D counts against explicit edges held in LDS;
//   hist2d_kernel    2-D counts, up to 128 x 128 bins (64 KB of 32-bit counters) in LDS.
// Only plain C++ stores and atomicAdd.
#pragma once

constexpr int kSumThreads = 256;
constexpr int kSumTile = 4096;          // rows of one walker per workgroup (selection passes, 1-D counts)
constexpr int kSumTile2d = 16384;       // ... of the 2-D counts, whose flush visits up to 16,384 counters; a 32-bit
                                        // counter holds 2^32 - 1 > kSumTile2d, so none can overflow before its flush
constexpr int kSelDigitBits = 8;
constexpr int kSelDigits = 1 << kSelDigitBits;
constexpr int kSelPasses = 64 / kSelDigitBits;
constexpr int kSelRanks = 16;           // ranks of one (member, column) resolved together (more: further launches)
constexpr int kHistMaxEdges = 4097;
constexpr int kHist2dMaxBins = 128;     // per axis
constexpr uint32_t kColRatioBit = 0x80000000u;   // MSX_COL_RATIO(a, b) = kColRatioBit | a << 8 | b

// The state of one (member, column)'s selection between passes.  A SLOT is a distinct prefix among the ranks' prefixes:
// ranks inside a run of equal values share one all the way down, so ties cost nothing extra.
struct SelState {
    int32_t nranks, nslots;
    int32_t slot[kSelRanks];                 // the slot of each rank's prefix
    unsigned long long prefix[kSelRanks];    // per rank: the key's digits resolved so far (the key after the last pass)
    long long rem[kSelRanks];                // per rank: its rank among the keys that carry its prefix
    unsigned long long slot_prefix[kSelRanks];
};

// np.sort's order: -inf < finite < +inf < NaN (every NaN, whatever its sign bit, takes the top key)
__device__ __forceinline__ unsigned long long sum_key(double x) { return x != x ? ~0ull : key_of(x); }

// the member of walker w (off: [k + 1] walker offsets; wave-uniform)
__device__ __forceinline__ int sum_member(const int64_t *__restrict__ off, int k, int64_t w) {
    int m = 0;
    while (m + 1 < k && w >= off[m + 1]) ++m;
    return m;
}

// One column of one walker: x(t) = a[t * thin] or a[t * thin] / b[t * thin] (plain IEEE division: NumPy's bits).
struct SumCol {
    const double *a, *b;
    __device__ __forceinline__ double at(int64_t i) const { return b ? a[i] / b[i] : a[i]; }
};
__device__ __forceinline__ SumCol sum_col(const double *__restrict__ rows, int64_t cap, int64_t nw, int64_t w, int64_t discard,
                                          uint32_t code) {
    SumCol c;
    if (code & kColRatioBit) {
        c.a = rows + ((int64_t)((code >> 8) & 0xffu) * nw + w) * cap + discard;
        c.b = rows + ((int64_t)(code & 0xffu) * nw + w) * cap + discard;
    } else {
        c.a = rows + ((int64_t)code * nw + w) * cap + discard;
        c.b = nullptr;
    }
    return c;
}

// bins[digit] += 1 for the lanes with `hit`, in LDS.  The lanes that share the first hit lane's digit are counted by one
// add (a chain is runs of equal values, and the leading digits of a column are the same everywhere: without this a
// wave's 64 adds would queue on one counter); the others add for themselves.  Called by whole waves.
__device__ __forceinline__ void sel_count(unsigned int *bins, bool hit, unsigned int digit) {
    const unsigned long long todo = __ballot(hit);
    if (!todo) return;
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, leader);
    const unsigned long long same = __ballot(hit && digit == d0);
    if ((int)(threadIdx.x & 63u) == leader) atomicAdd(bins + d0, (unsigned int)__popcll(same));
    else if (hit && digit != d0) atomicAdd(bins + digit, 1u);
}

// One pass (digit at `shift`) over the tile [blockIdx.y * kSumTile, + kSumTile) of walker blockIdx.x, column blockIdx.z:
// hist[(job * kSelRanks + slot) * kSelDigits + digit] += the keys whose higher digits equal the slot's prefix.
// job = member * ncols + column.
__global__ void __launch_bounds__(kSumThreads) sel_pass_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw,
                                                               int64_t np, int64_t discard, int64_t thin,
                                                               const int64_t *__restrict__ off, int32_t k,
                                                               const uint32_t *__restrict__ cols, int32_t ncols, int32_t shift,
                                                               const SelState *__restrict__ state,
                                                               unsigned long long *__restrict__ hist) {
    __shared__ unsigned int bins[kSelRanks * kSelDigits];
    __shared__ unsigned long long spre[kSelRanks];
    const int64_t w = blockIdx.x, t0 = (int64_t)blockIdx.y * kSumTile;
    const int jc = blockIdx.z;
    const int64_t job = (int64_t)sum_member(off, k, w) * ncols + jc;
    const SelState *st = state + job;
    const int nslots = st->nslots < kSelRanks ? st->nslots : kSelRanks;
    for (int i = threadIdx.x; i < nslots * kSelDigits; i += kSumThreads) bins[i] = 0u;
    if ((int)threadIdx.x < nslots) spre[threadIdx.x] = st->slot_prefix[threadIdx.x];
    __syncthreads();
    const unsigned long long pmask = shift + kSelDigitBits >= 64 ? 0ull : ~0ull << (shift + kSelDigitBits);
    const SumCol c = sum_col(rows, cap, nw, w, discard, cols[jc]);
    int64_t lim = np - t0;
    lim = lim > kSumTile ? kSumTile : lim;
    for (int base = 0; base < lim; base += 4 * kSumThreads) {   // (wave-uniform trips: sel_count needs whole waves)
        double x[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kSumThreads + (int)threadIdx.x;
            ok[u] = i < lim;
            x[u] = ok[u] ? c.at((t0 + i) * thin) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long key = sum_key(x[u]);
            const unsigned int digit = (unsigned int)(key >> shift) & (unsigned int)(kSelDigits - 1);
            for (int s = 0; s < nslots; ++s) sel_count(bins + s * kSelDigits, ok[u] && (key & pmask) == spre[s], digit);
        }
    }
    __syncthreads();
    unsigned long long *h = hist + job * (int64_t)(kSelRanks * kSelDigits);
    for (int i = threadIdx.x; i < nslots * kSelDigits; i += kSumThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(h + i, (unsigned long long)v);
    }
}

// After a pass: lane r of job blockIdx.x's wave walks its rank's slot histogram to the digit that holds the rank, lane 0
// then names the distinct prefixes of the next pass.  The histograms are zeroed for it.
__global__ void __launch_bounds__(64) sel_pick_kernel(SelState *__restrict__ state, unsigned long long *__restrict__ hist,
                                                      int32_t shift) {
    __shared__ unsigned long long h[kSelRanks * kSelDigits];
    __shared__ unsigned long long pre[kSelRanks];
    SelState *st = state + blockIdx.x;
    unsigned long long *g = hist + (int64_t)blockIdx.x * (kSelRanks * kSelDigits);
    const int nslots = st->nslots < kSelRanks ? st->nslots : kSelRanks, nranks = st->nranks < kSelRanks ? st->nranks : kSelRanks;
    for (int i = threadIdx.x; i < nslots * kSelDigits; i += 64) {
        h[i] = g[i];
        g[i] = 0ull;
    }
    __syncthreads();
    if ((int)threadIdx.x < nranks) {
        const int r = threadIdx.x;
        const unsigned long long *hs = h + (st->slot[r] & (kSelRanks - 1)) * kSelDigits;
        long long rem = st->rem[r];
        int d = 0;
        for (; d < kSelDigits - 1; ++d) {
            const long long cnt = (long long)hs[d];
            if (rem < cnt) break;
            rem -= cnt;
        }
        const unsigned long long p = st->prefix[r] | ((unsigned long long)d << shift);
        st->prefix[r] = p;
        st->rem[r] = rem;
        pre[r] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ns = 0;
        for (int r = 0; r < nranks; ++r) {
            int s = -1;
            for (int q = 0; q < r && s < 0; ++q)
                if (pre[q] == pre[r]) s = st->slot[q];
            if (s < 0) {
                s = ns++;
                st->slot_prefix[s] = pre[r];
            }
            st->slot[r] = s;
        }
        st->nslots = ns;
    }
}

// The bin of x among `ne` ascending edges in LDS, by comparisons alone: the last b with e[b] <= x (NumPy's
// searchsorted(e, x, 'right') - 1), -1 when there is none: below e[0], NaN, above the last edge, or ON the last edge
// unless closed_last (then the last bin, np.histogram's convention; the reference's loop counts it nowhere).
__device__ __forceinline__ int hist_bin(const double *e, int ne, int closed_last, double x) {
    int lo = 0, hi = ne;    // edges [0, lo) are <= x, edges [hi, ne) are not
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    int b = lo - 1;
    if (b >= ne - 1) b = closed_last && x == e[ne - 1] ? ne - 2 : -1;
    return b;
}

// counts[job * (nedges - 1) + b] += the tile's values in bin b of edges[job * nedges ..]; job = member * ncols + column.
// Dynamic LDS: nedges doubles, then nedges - 1 32-bit counters (at most 49,164 bytes).
__global__ void __launch_bounds__(kSumThreads) hist_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, int64_t np,
                                                           int64_t discard, int64_t thin, const int64_t *__restrict__ off,
                                                           int32_t k, const uint32_t *__restrict__ cols, int32_t ncols,
                                                           const double *__restrict__ edges, int32_t nedges, int32_t closed_last,
                                                           unsigned long long *__restrict__ counts) {
    extern __shared__ double lds1d[];
    double *e = lds1d;
    unsigned int *bins = (unsigned int *)(lds1d + nedges);
    const int64_t w = blockIdx.x, t0 = (int64_t)blockIdx.y * kSumTile;
    const int jc = blockIdx.z;
    const int64_t job = (int64_t)sum_member(off, k, w) * ncols + jc;
    for (int i = threadIdx.x; i < nedges; i += kSumThreads) e[i] = edges[job * nedges + i];
    for (int i = threadIdx.x; i < nedges - 1; i += kSumThreads) bins[i] = 0u;
    __syncthreads();
    const SumCol c = sum_col(rows, cap, nw, w, discard, cols[jc]);
    int64_t lim = np - t0;
    lim = lim > kSumTile ? kSumTile : lim;
    for (int base = 0; base < lim; base += 4 * kSumThreads) {
        double x[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kSumThreads + (int)threadIdx.x;
            ok[u] = i < lim;
            x[u] = ok[u] ? c.at((t0 + i) * thin) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = ok[u] ? hist_bin(e, nedges, closed_last, x[u]) : -1;
            if (b >= 0) atomicAdd(bins + b, 1u);
        }
    }
    __syncthreads();
    unsigned long long *g = counts + job * (int64_t)(nedges - 1);
    for (int i = threadIdx.x; i < nedges - 1; i += kSumThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(g + i, (unsigned long long)v);
    }
}

// counts[job][bx][by] += the tile's (x, y) in bin (bx, by); job = member * npairs + pair; ex [job][nx], ey [job][ny].
// Dynamic LDS: nx + ny doubles, then (nx - 1)(ny - 1) 32-bit counters.
__global__ void __launch_bounds__(kSumThreads) hist2d_kernel(const double *__restrict__ rows, int64_t cap, int64_t nw, int64_t np,
                                                             int64_t discard, int64_t thin, const int64_t *__restrict__ off,
                                                             int32_t k, const uint32_t *__restrict__ cols, int32_t npairs,
                                                             const double *__restrict__ ex, int32_t nx,
                                                             const double *__restrict__ ey, int32_t ny, int32_t closed_last,
                                                             unsigned long long *__restrict__ counts) {
    extern __shared__ double lds2d[];
    double *sx = lds2d, *sy = lds2d + nx;
    unsigned int *bins = (unsigned int *)(lds2d + nx + ny);
    const int by_n = ny - 1, nb = (nx - 1) * by_n;
    const int64_t w = blockIdx.x, t0 = (int64_t)blockIdx.y * kSumTile2d;
    const int jp = blockIdx.z;
    const int64_t job = (int64_t)sum_member(off, k, w) * npairs + jp;
    for (int i = threadIdx.x; i < nx; i += kSumThreads) sx[i] = ex[job * nx + i];
    for (int i = threadIdx.x; i < ny; i += kSumThreads) sy[i] = ey[job * ny + i];
    for (int i = threadIdx.x; i < nb; i += kSumThreads) bins[i] = 0u;
    __syncthreads();
    const SumCol cx = sum_col(rows, cap, nw, w, discard, cols[2 * jp]);
    const SumCol cy = sum_col(rows, cap, nw, w, discard, cols[2 * jp + 1]);
    int64_t lim = np - t0;
    lim = lim > kSumTile2d ? kSumTile2d : lim;
    for (int base = 0; base < lim; base += 4 * kSumThreads) {
        double x[4], y[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kSumThreads + (int)threadIdx.x;
            ok[u] = i < lim;
            x[u] = ok[u] ? cx.at((t0 + i) * thin) : 0.0;
            y[u] = ok[u] ? cy.at((t0 + i) * thin) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bx = ok[u] ? hist_bin(sx, nx, closed_last, x[u]) : -1;
            const int by = ok[u] ? hist_bin(sy, ny, closed_last, y[u]) : -1;
            if (bx >= 0 && by >= 0) atomicAdd(bins + bx * by_n + by, 1u);
        }
    }
    __syncthreads();
    unsigned long long *g = counts + job * (int64_t)nb;
    for (int i = threadIdx.x; i < nb; i += kSumThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(g + i, (unsigned long long)v);
    }
}
