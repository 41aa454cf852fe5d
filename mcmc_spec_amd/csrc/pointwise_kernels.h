// pointwise_kernels.h -- part of the single translation unit msx.hip (included there, behind psis_kernels.h).
// Pointwise model checks (include/msx.h, msx_predictive_pointwise / msx_series_pointwise): the terms of
// the log-likelihood per OBSERVATION and sample, and per observation lppd, WAIC and PSIS-LOO with its khat.  The observations
// are the npix pixels, then the nc contrast filters, then the np photometry bands.  The unchanged sample pass of the predictive
// check (predictive_sample_kernel) leaves every sample's record; then, for a tile of observations,
//   pointwise_pixel_kernel  the pixels' terms of the valid samples, SAMPLE-CONTIGUOUS per pixel through an LDS transpose:
//                           coef * z^2, coef = (-0.5 (nc + np)) / npix rounded once, z^2 pred_resid's bits, one product;
//   pointwise_band_kernel   the filters' terms, one thread per valid sample from its record and A_V: -0.5 * s with s the
//                           summand of the sample pass, (z z) / (err err), in its roundings (the halving is exact);
//   pointwise_reduce_kernel one workgroup per observation over its `count` terms x: lppd = logsumexp(x) - log count; p_waic =
//                           the two-pass variance (ddof 1); PSIS of the ratios -x with the tail length the host hands over
//                           (psis_kernels.h's sort and fit; the cutoff by median.h's radix_select: the ratio of ascending rank
//                           S - M - 1 is minus the term of ascending rank M); elpd_loo = logsumexp(pre + x) - logsumexp(pre)
//                           with pre the shifted ratios, smoothed in the tail.
// A term that is NaN or -inf makes a BAD ratio (NaN, +inf): it weighs 0 and does not count in S; with fewer than M + 1
// countable ratios khat, elpd_loo and p_loo are NaN.  Sums: lane l of 256 adds elements l, l + 256, .. one after the other --
// first the samples outside the tail, then the tail in its order --, then rw_tree: a function of the ordered list of valid
// samples alone.  No float atomics; no workgroup waits for another.
#ifndef MSX_POINTWISE_KERNELS_H
#define MSX_POINTWISE_KERNELS_H

namespace {

constexpr int kPwOut = 6;   // lppd, p_waic, elpd_waic, elpd_loo, p_loo, khat

// pixels [p0, p0 + tp) of the valid samples vidx[0 .. count): vals[pixel * count + j].  grid as predictive_fill_kernel's
struct PwPixelLaunch {
    const ProdMember *M;
    const PredRec *rec;
    const int64_t *vidx;
    int64_t count, p0, tp;
    double coef;
    double *vals;
};
template <int NS>
__global__ void __launch_bounds__(kPredThreads) pointwise_pixel_kernel(const PwPixelLaunch L) {
#pragma clang fp contract(off)
    __shared__ double s_w[NS * 4 * kProdThreads];
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    __shared__ double s_par[5][kPredTile];
    __shared__ int32_t s_red[kPredTile];
    __shared__ double s_tile[kPredTile][kPredTile + 1];
    const ProdMember *M = L.M;
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * kPredTile;
    if (tid < kPredTile && j0 + tid < L.count) {
        const PredRec *r = L.rec + L.vidx[j0 + tid];
#pragma unroll
        for (int c = 0; c < 4 * NS; ++c) {
            s_w[c * kProdThreads + tid] = r->w[c];
            s_rn[c * kProdThreads + tid] = r->node[c];
        }
        s_par[0][tid] = r->scale; s_par[1][tid] = r->c0; s_par[2][tid] = r->c1; s_par[3][tid] = r->c2; s_par[4][tid] = r->redc;
        s_red[tid] = r->redden;
    }
    __syncthreads();
    const int hi = tid / kPredTile, lo = tid % kPredTile;  // compute: (sample hi, pixel lo); store: (pixel hi, sample lo)
    const int64_t nwl = M->nwl;
    const ProdRecipe R{s_rn + hi, s_w + hi};
    const bool have = j0 + hi < L.count;
    for (int64_t pc = (int64_t)blockIdx.y * kPredTile; pc < L.tp; pc += (int64_t)gridDim.y * kPredTile) {
        if (have && pc + lo < L.tp) {
            const int64_t p = L.p0 + pc + lo;
            double m[NS], dn, z, z2;
            const double tot = spectra_pixel<NS>(M, R, nwl, s_red[hi] != 0, s_par[4][hi], p, m);
            const double model = tot * s_par[0][hi];
            pred_resid(model, M->pix_flux[p], M->pix_err[p], M->pix_u[p], s_par[1][hi], s_par[2][hi], s_par[3][hi], dn, z, z2);
            s_tile[lo][hi] = L.coef * z2;
        }
        __syncthreads();
        if (j0 + lo < L.count && pc + hi < L.tp) L.vals[(pc + hi) * L.count + j0 + lo] = s_tile[hi][lo];
        __syncthreads();
    }
}

// filters [f0, f0 + tf) of the nc + np (contrast filters first) of the valid samples: vals[(f - f0) * count + j].  grid
// ceil(count / 256)
struct PwBandLaunch {
    const ProdMember *M;
    const PredRec *rec;
    const int64_t *vidx;
    PredSrc src;
    int64_t count;
    int32_t f0, tf;
    double *vals;
};
template <int NS>
__global__ void __launch_bounds__(kPredThreads) pointwise_band_kernel(const PwBandLaunch L) {
    __shared__ double s_w[NS * 4 * kProdThreads];
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    const ProdMember *M = L.M;
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kPredThreads + tid;
    if (j >= L.count) return;   // (no barrier below: a thread reads its own slots alone)
    const int64_t smp = L.vidx[j];
    const PredRec *r = L.rec + smp;
#pragma unroll
    for (int c = 0; c < 4 * NS; ++c) {
        s_w[c * kProdThreads + tid] = r->w[c];
        s_rn[c * kProdThreads + tid] = r->node[c];
    }
    const ProdRecipe R{s_rn + tid, s_w + tid};
    const double a_v = L.src.base[pred_offset(L.src, smp, L.src.sw, L.src.sr) + NS * L.src.sd];
    const bool redden = r->redden != 0;
    const int nc = M->nc, np = M->np, nb = nc + np;
    for (int f = L.f0; f < L.f0 + L.tf; ++f) {
        double s;
        if (f < nc) {
            const int sec = (NS == 3 && f >= nc / 2) ? 2 : 1;
            const double mag_s = -2.5 * log10(star_integral(M->band_tab, nb, f, R, sec));
            const double con = mag_s - -2.5 * log10(star_integral(M->band_tab, nb, f, R, 0));
            const double z = con - M->cmag[f];
            s = (z * z) / (M->cerr[f] * M->cerr[f]);
        } else {
            const int g = f - nc;
            const double mag = -2.5 * log10(composite_integral<NS>(M->band_tab, nb, f, R) / M->pzero[g]);
            const double mred = redden ? mag + a_v * M->pk[g] : mag;
            const double z = mred - M->pmag[g];
            s = (z * z) / (M->perr[g] * M->perr[g]);
        }
        L.vals[(int64_t)(f - L.f0) * L.count + j] = -0.5 * s;
    }
}

// grid: the tile's observations; x = vals + blockIdx.x * count.  out [6][n_obs] at observation o0 + blockIdx.x
struct PwReduceLaunch {
    const double *vals;
    int64_t count, o0, n_obs, tail_len;
    double *out;
};
__global__ void __launch_bounds__(kPredThreads) pointwise_reduce_kernel(const PwReduceLaunch L) {
#pragma clang fp contract(off)
    __shared__ BlockScratch S;
    __shared__ double key[kPsTailMax];
    __shared__ unsigned int idx[kPsTailMax];
    __shared__ double rs[kPsThreads];
    __shared__ double fb[kPsFitMax], fL[kPsFitMax], fw[kPsFitMax];
    __shared__ unsigned int cnt;
    __shared__ double bbar;
    const int tid = threadIdx.x;
    const int n = (int)L.count;
    const double *x = L.vals + (int64_t)blockIdx.x * L.count;
    double *out = L.out + L.o0 + blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // one pass: the largest term, the smallest countable one, the sum, what is bad and how it sorts
    double mx = -INFINITY, mn = INFINITY, part = 0.0, nlow = 0.0, nnan = 0.0, nbad = 0.0;
    for (int j = tid; j < n; j += kPredThreads) {
        const double v = x[j];
        part = part + v;
        if (v != v) {
            nnan += 1.0; nbad += 1.0;
            if (__double_as_longlong(v) < 0) nlow += 1.0;   // (a NaN with the sign bit set takes the lowest keys)
        } else {
            if (v > mx) mx = v;
            if (v == -INFINITY) { nbad += 1.0; nlow += 1.0; }
            else if (v < mn) mn = v;
        }
    }
    const double dn = (double)n;
    const double mean = psis_sum(part, rs) / dn;
    const double top = psis_max(mx, rs);
    const double low = -psis_max(-mn, rs);   // the smallest countable term: the largest ratio is -low
    const int n_low = (int)psis_sum(nlow, rs), n_nan = (int)psis_sum(nnan, rs), n_bad = (int)psis_sum(nbad, rs);   // (small integers: exact)
    part = 0.0;
    for (int j = tid; j < n; j += kPredThreads) part = part + exp(x[j] - top);
    const double sum_e = psis_sum(part, rs);
    const double lppd = n_nan ? nan : (top == -INFINITY ? -INFINITY : (top + log(sum_e)) - log(dn));
    part = 0.0;
    for (int j = tid; j < n; j += kPredThreads) {
        const double d = x[j] - mean;
        part = part + d * d;
    }
    const double p_waic = psis_sum(part, rs) / (double)(n - 1);
    if (tid == 0) {
        out[0] = lppd;
        out[L.n_obs] = p_waic;
        out[2 * L.n_obs] = lppd - p_waic;
    }
    const int Sc = n - n_bad, M = (int)L.tail_len;
    if (M > Sc - 1 || low == INFINITY) {   // too few countable ratios for this tail; or none that is finite
        if (tid == 0) out[3 * L.n_obs] = out[4 * L.n_obs] = out[5 * L.n_obs] = nan;
        return;
    }
    // ratios lr = -x, shifted by their maximum -low: xs = (-x) - (-low).  The cutoff: the ratio of ascending rank Sc - M - 1
    // = minus the term of ascending rank M among the countable ones, below which n_low bad ones sort
    __syncthreads();
    const unsigned long long kc = radix_select(x, n, (unsigned int)(M + n_low), 0ull, ~0ull, S);
    const double xc = -val_of(kc) - -low;
    const double cutoff = xc > MSX_PSIS_LOG_TINY ? xc : MSX_PSIS_LOG_TINY;
    if (tid == 0) cnt = 0u;
    __syncthreads();
    for (int j = tid; j < n; j += kPredThreads) {
        const double v = x[j];
        const bool bad = v != v || v == -INFINITY;
        const double xs = -v - -low;
        if (!bad && xs > cutoff) {
            const unsigned int slot = atomicAdd(&cnt, 1u);
            if (slot < (unsigned int)kPsTailMax) {   // (at most M <= MSX_PSIS_TAIL_MAX lie strictly above the cutoff)
                key[slot] = xs;
                idx[slot] = (unsigned int)j;
            }
        }
    }
    __syncthreads();
    const int nt = cnt < (unsigned int)kPsTailMax ? (int)cnt : kPsTailMax;
    const PsisTail T{key, idx, rs, fb, fL, fw, &bbar};
    psis_sort(T, nt);
    double khat = INFINITY;
    if (nt >= MSX_PSIS_MIN_TAIL) khat = psis_fit_replace(T, nt, cutoff);
    // pre = xs outside the tail, key inside; a = pre + x.  Their maxima, then the two sums
    double m1 = -INFINITY, m2 = -INFINITY;
    for (int j = tid; j < n; j += kPredThreads) {
        const double v = x[j];
        const bool bad = v != v || v == -INFINITY;
        const double xs = -v - -low;
        if (bad || xs > cutoff) continue;
        const double a = xs + v;
        if (xs > m1) m1 = xs;
        if (a > m2) m2 = a;
    }
    for (int j = tid; j < nt; j += kPredThreads) {
        const double a = key[j] + x[idx[j]];
        if (key[j] > m1) m1 = key[j];
        if (a > m2) m2 = a;
    }
    const double t1 = psis_max(m1, rs), t2 = psis_max(m2, rs);
    double s1 = 0.0, s2 = 0.0;
    for (int j = tid; j < n; j += kPredThreads) {
        const double v = x[j];
        const bool bad = v != v || v == -INFINITY;
        const double xs = -v - -low;
        if (bad || xs > cutoff) continue;
        const double a = xs + v;
        s1 = s1 + exp(xs - t1);
        s2 = s2 + exp(a - t2);
    }
    for (int j = tid; j < nt; j += kPredThreads) {
        const double a = key[j] + x[idx[j]];
        s1 = s1 + exp(key[j] - t1);
        s2 = s2 + exp(a - t2);
    }
    const double lse1 = t1 + log(psis_sum(s1, rs)), lse2 = t2 + log(psis_sum(s2, rs));
    if (tid == 0) {
        const double elpd = lse2 - lse1;
        out[3 * L.n_obs] = elpd;
        out[4 * L.n_obs] = lppd - elpd;
        out[5 * L.n_obs] = khat;
    }
}

}  // namespace

#endif  // MSX_POINTWISE_KERNELS_H
