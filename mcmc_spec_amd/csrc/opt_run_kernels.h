// opt_run_kernels.h -- part of the single translation unit msx.hip (included there, in this order).
// The device-resident pre-optimiser (msx_opt_run_*): fit_spec's per-chain state machine
// (mft6.py:935-1103: step-size schedule, proposal, bounds test, repair-loop counters, opt_prior terms, accept rule) as
// ONE THREAD PER CHAIN, in a small kernel that sits between two OPT_STEP launches of the unchanged hot kernel.
#ifndef MSX_OPT_RUN_KERNELS_H
#define MSX_OPT_RUN_KERNELS_H

namespace {

// a trip's record flag (include/msx.h: MSX_OPT_TRIP_*; bits 8.. of an error flag carry the walker status)
constexpr int kTripIdle = 0, kTripOob = 1, kTripRejected = 2, kTripAccepted = 3, kTripError = 4;
// what a chain's thread leaves for itself between the two halves of a trip (tflag): kTripIdle / kTripOob, or
constexpr int kTripEval = 2;       // ... the proposal is being evaluated; bit 4: drawn with the fine step sizes
constexpr int kOptRunThreads = 64;

// The run: constants, tables and the chains' state, all in device memory.  Passed by value.
struct OptRunDev {
    int32_t nch, ndim, nspec, dist_fit, rad_prior;
    int32_t nedges, nmu, niso;
    double steps;          // nstep of fit_spec (a double: compared with the fractional n of odd step counts)
    int64_t cap;           // 50 * steps proposals per chain
    double tmin, tmax;     // min(tlim), max(tlim)
    double pprior, psig;   // the parallax prior
    const double *av_edges, *av_mu, *av_sig;  // the A_V(distance) table given to the run
    const double *iso_t, *iso_l;              // the isochrone, sorted by Teff: Teff, luminosity
    // state per chain
    double *gi;            // [nch][ndim] current best, rows [T.., A_V, rad.., plx]
    double *chi, *n;       // [nch]
    int64_t *total_n;      // [nch]
    double *rad0, *dist0;  // [nch][nspec], [nch]: the start point's radii and parallax (the step sizes' scale)
    int32_t *done;         // [nch]
    // the trip in flight: the proposals (the OPT_STEP launch's theta; a row of NaNs = nothing to evaluate: the hot
    // kernel's workgroup leaves after its recipe, with a status nobody reads), what the launch returned
    double *theta;         // [nch][ndim]
    int32_t *tflag;        // [nch]
    const double *like;    // [nch]
    const int32_t *status; // [nch]
};

// _step_sizes (optimizer.py; mft6.py:952-955, :970-973)
template <int NS>
__device__ __forceinline__ void opt_step_sizes(const OptRunDev &R, int64_t c, bool fine, double *si) {
#pragma clang fp contract(off)
    constexpr int ns = NS;
    _Pragma("unroll") for (int k = 0; k < ns; ++k) si[k] = fine ? 20.0 : 250.0;
    si[ns] = fine ? 0.01 : 0.05;
    _Pragma("unroll") for (int k = 0; k < ns; ++k) si[ns + 1 + k] = (fine ? 0.05 : 0.1) * R.rad0[c * ns + k];
    const double f = fine ? (ns == 2 ? 0.005 : 0.01) : (ns == 2 ? 0.02 : 0.05);
    si[2 * ns + 1] = f * R.dist0[c];
}

// _in_bounds (mft6.py:981-982)
template <int NS>
__device__ __forceinline__ bool opt_in_bounds(const OptRunDev &R, const double *v) {
    constexpr int ns = NS;
    bool ok = true;
    _Pragma("unroll") for (int k = 0; k < ns; ++k) ok = ok && (R.tmin < v[k]) && (v[k] < R.tmax);
    const double av = v[ns], r0 = v[ns + 1], r1 = v[ns + 2], plx = v[2 * ns + 1];
    return ok && (0.0 <= av) && (0.05 <= r0) && (r0 <= 1.5) && (0.05 < r1) && (r1 < 1.0) && (1.0 / 10 > plx) && (plx > 1.0 / 3000);
}

// _repair_count (mft6.py:1071-1103): the seven loops, in order, on a private copy; only the counter survives
template <int NS>
__device__ __forceinline__ int64_t opt_repair_count(const OptRunDev &R, const double *var, int64_t total_n) {
#pragma clang fp contract(off)
    constexpr int ns = NS;
    const int64_t cap = R.cap;
    double T[MSX_MAX_SPEC], rad[MSX_MAX_SPEC];
    _Pragma("unroll") for (int k = 0; k < ns; ++k) { T[k] = var[k]; rad[k] = var[ns + 1 + k]; }
    double av = var[ns], plx = var[2 * ns + 1];
    total_n += 1;
    for (;;) {
        bool any = false;
        _Pragma("unroll") for (int k = 0; k < ns; ++k) any = any || T[k] < R.tmin;
        if (!(any && total_n < cap)) break;
        total_n += 1;
        _Pragma("unroll") for (int k = 0; k < ns; ++k)
            if (T[k] < R.tmin) T[k] = T[k] + 100.0;
    }
    for (;;) {
        bool any = false;
        _Pragma("unroll") for (int k = 0; k < ns; ++k) any = any || T[k] > R.tmax;
        if (!(any && total_n < cap)) break;
        total_n += 1;
        _Pragma("unroll") for (int k = 0; k < ns; ++k)
            if (T[k] > R.tmax) T[k] = T[k] - 100.0;
    }
    while (T[0] < T[1] && total_n < cap) { total_n += 1; T[1] = T[1] - 100.0; }
    while (av < 0.0 && total_n < cap) { total_n += 1; av = av + 0.1; }
    for (;;) {
        bool any = false;
        _Pragma("unroll") for (int k = 0; k < ns; ++k) any = any || rad[k] < 0.05;
        if (!(any && total_n < cap)) break;
        total_n += 1;
        _Pragma("unroll") for (int k = 0; k < ns; ++k)
            if (rad[k] < 0.05) rad[k] = rad[k] + 0.01;
    }
    while (plx > 1.0 / 100 && total_n < cap) { total_n += 1; const double d = 0.01 * fabs(plx); plx = plx - d; }
    while (plx < 1.0 / 3000 && total_n < cap) { total_n += 1; const double d = 0.01 * fabs(plx); plx = plx + d; }
    return total_n;
}

// opt_prior with one-element lists (mft6.py:839-843)
__device__ __forceinline__ double opt_prior_one(double v, double p, double s) {
#pragma clang fp contract(off)
    const double z = (v - p) / s;
    return z * z;
}

// #{xs[i] <= x} of a sorted table (np.searchsorted(xs, x, side='right'))
__device__ __forceinline__ int opt_count_le(const double *xs, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// np.interp inside the table's range (cnt = #{xs <= x}), every operation rounded on its own like NumPy's C loop
// (recipe.h's interp_from_count is the same statement compiled with contraction on)
__device__ __forceinline__ double opt_interp(const double *xs, const double *ys, int n, double x, int cnt) {
#pragma clang fp contract(off)
    const int j = cnt - 1;
    if (j >= n - 1) return ys[n - 1];
    const double x0 = xs[j], y0 = ys[j];
    if (x0 == x) return y0;
    const double slope = (ys[j + 1] - y0) / (xs[j + 1] - x0);
    const double rise = slope * (x - x0);
    return rise + y0;
}

// The accept half of trip t - 1 (rec / flags non-null) and the propose half of trip t (z non-null) of every chain, one
// thread per chain.  `live` non-null (the chunk's last launch): counts the chains that would draw again.
template <int NS>
__global__ void __launch_bounds__(kOptRunThreads)
opt_run_trip_kernel(OptRunDev R, const double *__restrict__ z, double *__restrict__ rec, int32_t *__restrict__ flags,
                    int32_t *__restrict__ worst, int32_t *__restrict__ live) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * kOptRunThreads + threadIdx.x;
    if (c >= R.nch) return;
    constexpr int ns = NS, nd = 2 * NS + 2;
    double *gi = R.gi + c * nd, *var = R.theta + c * nd;
    const double half = R.steps / 2;
    if (rec) {
        // ---- the trip's last lines (optimizer.py, the loop behind the launch; mft6.py:991-1063) ----
        const int tf = R.tflag[c], kind = tf & 15;
        const bool fine = (tf >> 4) & 1;
        int flag = kind == kTripEval ? kTripRejected : kind;
        double test = NAN;
        double *row = rec + c * (nd + 2);
        bool named = false;  // (a failed evaluation: the record names the proposal, not the chain's best)
        if (kind == kTripEval) {
            const int st = R.status[c];
            if (st > MSX_W_REJECT) {
                flag = kTripError | (st << 8);
                atomicMax(worst, st);
                R.done[c] = 1;
                named = true;
            } else {
                const double av = var[ns], plx = var[2 * ns + 1];
                // _av_lookup: searchsorted(edges, 1 / plx, 'right') - 1, clipped; sigma 0 -> 0.05 (mft6.py:927-928, :994-995)
                int b = opt_count_le(R.av_edges, R.nedges, 1.0 / plx) - 1;
                b = b < 0 ? 0 : (b > R.nmu - 1 ? R.nmu - 1 : b);
                const double sg = R.av_sig[b] == 0.0 ? 0.05 : R.av_sig[b];
                test = R.like[c] + opt_prior_one(av, R.av_mu[b], sg);                 // mft6.py:1030
                if (R.dist_fit) test = test + opt_prior_one(plx, R.pprior, R.psig);   // mft6.py:1034-1035
                if (R.rad_prior) {  // mft6.py:1037-1050: the isochrone's radii, sigma = the current radius step sizes
                    double mr[MSX_MAX_SPEC];
                    _Pragma("unroll") for (int k = 0; k < ns; ++k) {
                        const int cnt = opt_count_le(R.iso_t, R.niso, var[k]);
                        mr[k] = model_radius(opt_interp(R.iso_t, R.iso_l, R.niso, var[k], cnt), var[k]);
                    }
                    double tot = 0.0;
                    _Pragma("unroll") for (int k = 0; k < ns; ++k) {
                        const double p = k == 0 ? mr[0] : mr[k] / mr[0];
                        const double s = (fine ? 0.05 : 0.1) * R.rad0[c * ns + k];
                        if (p != 0.0) tot = tot + opt_prior_one(var[ns + 1 + k], p, s);
                    }
                    test = test + tot;
                }
                if (test < R.chi[c]) {  // mft6.py:1053-1063
                    _Pragma("unroll") for (int d = 0; d < nd; ++d) gi[d] = var[d];
                    R.chi[c] = test;
                    R.n[c] = R.n[c] > half ? half + 1.0 : 0.0;
                    flag = kTripAccepted;
                }
            }
        }
        _Pragma("unroll") for (int d = 0; d < nd; ++d) row[d] = named ? var[d] : gi[d];
        row[nd] = R.chi[c];
        row[nd + 1] = test;
        flags[c] = flag;
    }
    if (z) {
        // ---- the trip's first lines: ONE draw (optimizer.py:138-149; mft6.py:935-985, :1071-1103) ----
        int tf = kTripIdle;
        bool eval = false;
        const double n = R.n[c];
        const int64_t total_n = R.total_n[c];
        if (!R.done[c]) {
            if (!(n < R.steps && total_n < R.cap)) {
                R.done[c] = 1;
            } else {
                const bool fine = n > half;
                double si[2 * MSX_MAX_SPEC + 2], v[2 * MSX_MAX_SPEC + 2];
                opt_step_sizes<NS>(R, c, fine, si);
                // a rounded multiply, then a rounded add: the bits of NumPy's loc + scale * z.  (Plain operators under this
                // kernel's `fp contract(off)`: the rounding intrinsics of the HIP headers are inline functions compiled
                // with the header's contraction setting, and their product and sum were fused again after inlining.)
                _Pragma("unroll") for (int d = 0; d < nd; ++d) {
                    const double step = si[d] * z[c * nd + d];
                    v[d] = gi[d] + step;
                }
                if (opt_in_bounds<NS>(R, v)) {
                    if constexpr (NS == 3) {  // mft6.py:984-985 (one pass ends the reference's loop: 0 < 0.9 r < r)
                        if (v[ns + 3] >= v[ns + 2] || v[ns + 3] < 0.0) v[ns + 3] = v[ns + 2] * 0.9;
                    }
                    R.total_n[c] = total_n + 1;
                    R.n[c] = n + 1.0;
                    _Pragma("unroll") for (int d = 0; d < nd; ++d) var[d] = v[d];
                    tf = kTripEval | (fine ? 16 : 0);
                    eval = true;
                } else {
                    R.total_n[c] = opt_repair_count<NS>(R, v, total_n);
                    tf = kTripOob;
                }
            }
        }
        if (!eval)
            _Pragma("unroll") for (int d = 0; d < nd; ++d) var[d] = NAN;
        R.tflag[c] = tf;
    }
    if (live && !R.done[c] && R.n[c] < R.steps && R.total_n[c] < R.cap) atomicAdd(live, 1);
}

}  // namespace

#endif  // MSX_OPT_RUN_KERNELS_H
