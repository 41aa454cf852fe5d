// product_kernels.h -- part of the single translation unit msx.hip (included there, in this order).
// derived columns of samples (include/msx.h, msx_products_batch / msx_series_derive): one thread per sample, the recipe by
// one thread with its small tables in LDS, the columns from the per-node band tables.
#ifndef MSX_PRODUCT_KERNELS_H
#define MSX_PRODUCT_KERNELS_H

namespace {

constexpr int kProdThreads = 256;
constexpr int kProdIsoMax = 256, kProdNodeMax = 64;  // tables up to these sizes are copied to LDS; longer ones are read where they are
constexpr uint32_t kPcolBandMag = 1, kPcolBandMagSum = 2, kPcolDmag = 3, kPcolPriCorr = 4, kPcolSecCorr = 5, kPcolContrast = 6,
                   kPcolPhot = 7, kPcolLogg = 8, kPcolMass = 9, kPcolLum = 10;

// What a sample's evaluation reads of one context: its staged problem's recipe tables and bands, and its staged products.
// The kernels read it through a pointer to a device copy (a by-value DevProblem has the scratch hazard of dev_types.h).
struct ProdMember {
    const double *teff_nodes, *logg_nodes;
    const uint8_t *present;
    const double *iso_t, *iso_g;             // the problem's isochrone: log g(Teff)                     mft6.py:87-98
    const double *piso_t, *piso_m, *piso_l;  // the product isochrone: mass, luminosity                   mft6.py:2650,:2679
    const double *band_tab;                  // [rows][nc + np] the problem's band integrals per node
    const double *prod_tab;                  // [rows][npb] the product bands'
    double pzero[MSX_MAX_BANDS];
    double zero_mag[MSX_MAX_BANDS];
    int32_t kind[MSX_MAX_BANDS];
    int32_t nt, ng, node_stride, niso, npiso, nc, np, npb, nspec, dist_fit;
    // the spectra of samples (products_spectra_kernel): the grid rows, the CCM89 curve and the data pixels' resample tables
    const double *grid, *kgrid;
    const int64_t *pix_lo;
    const double *pix_t;
    int64_t nwl, npix;
    double median_flux;
    int32_t use_av, no_spectrum;
    // the posterior predictive check (predictive_kernels.h): what the likelihood compares the model with
    const double *pix_flux, *pix_err, *pix_u;  // data, sigma, the fit abscissa                           mft6.py:195,:120
    double minv[9];                            // the inverse Gram matrix of [1, u, u^2]
    double cmag[MSX_MAX_BANDS], cerr[MSX_MAX_BANDS], pmag[MSX_MAX_BANDS], perr[MSX_MAX_BANDS], pk[MSX_MAX_BANDS];
};

// one launch: samples are (walker, row) of a [walkers][rows] rectangle per member; element d of sample (w, r) sits at
// base[w * sw + (row0 + r) * sr + d * sd] -- a batch is one row of n walkers, a series [ndim][nw][cap] has sw = cap, sr = 1
struct ProdLaunch {
    const ProdMember *members;  // [k]
    const int64_t *off;         // [k + 1] the members' walker offsets; null: one member of n_single walkers
    int64_t n_single;
    const double *in;
    double *out;
    int64_t in_sw, in_sr, in_sd, out_sw, out_sr, out_sd, row0, nrows;
    const uint32_t *cols;
    int32_t ncols;
    int32_t need_piso;          // a MASS or LUM column is asked for: Teff must lie inside the product isochrone
    int32_t *status;            // [walkers] (batches) or null
    int32_t *worst;             // [k] or null
};

// a column code the tables of a context can answer (one rule for the host's check and the kernel's)
__host__ __device__ inline bool pcol_known(uint32_t code, int ndim, int nspec, int npb, int nc, int np) {
    const uint32_t kind = code >> 24;
    const int b = (int)((code >> 8) & 0xffu), s = (int)(code & 0xffu);
    if (kind == 0) return (int64_t)code < ndim;
    if ((code & 0x00ff0000u) != 0) return false;
    switch (kind) {
    case kPcolBandMag: case kPcolDmag: return b < npb && s < nspec;
    case kPcolBandMagSum: case kPcolPriCorr: case kPcolSecCorr: return b < npb && s == 0;
    case kPcolContrast: return b == 0 && s < nc;
    case kPcolPhot: return b == 0 && s < np;
    case kPcolLogg: case kPcolMass: case kPcolLum: return b == 0 && s < nspec;
    default: return false;
    }
}

struct ProdTabs {
    const double *teff, *logg, *iso_t, *iso_g, *piso_t, *piso_m, *piso_l;
};

// #{i : xs[i] <= x} of an ascending table
__device__ __forceinline__ int prod_count_le(const double *xs, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// bracket_nodes (recipe.h; mft6.py:439-453 / :467-477) inlined: out-parameters of a call would live in scratch
__device__ __forceinline__ int prod_bracket(const double *nodes, int n, double v, int &i1, int &i2) {
    int best = 0;
    double bd = fabs(nodes[0] - v);
    for (int i = 1; i < n; ++i) {
        const double d = fabs(nodes[i] - v);
        if (d < bd) { bd = d; best = i; }
    }
    const double nb = nodes[best];
    int other = nb == v ? best : (nb > v ? best - 1 : best + 1);
    if (other == -1) other = n - 1;  // Python's index -1: the last node
    i1 = best;
    i2 = other < n ? other : best;
    return other >= n ? MSX_W_INDEXERROR : MSX_W_OK;
}

// A sample's recipe lives in LDS, corner c of the thread at [c * kProdThreads]: the columns pick a star at run time, and
// a register array indexed at run time would go to scratch
struct ProdRecipe {
    int32_t *node;
    double *w;
};
// star s's integral in column b of a per-node table of row length nb: the blend of its four corners
__device__ __forceinline__ double star_integral(const double *__restrict__ tab, int nb, int b, const ProdRecipe &R, int s) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc += R.w[(4 * s + c) * kProdThreads] * tab[(int64_t)R.node[(4 * s + c) * kProdThreads] * nb + b];
    return acc;
}
// ... and of the stars summed in star order (mft6.py:744,751)
template <int NS>
__device__ __forceinline__ double composite_integral(const double *__restrict__ tab, int nb, int b, const ProdRecipe &R) {
    double tot = star_integral(tab, nb, b, R, 0);
#pragma unroll
    for (int s = 1; s < NS; ++s) tot += star_integral(tab, nb, b, R, s);
    return tot;
}

// One sample's recipe into R: the isochrone's log g per star, the brackets, the bilinear weights times the scale.  Returns
// the status (MSX_W_*); R is complete only for MSX_W_OK.
template <int NS>
__device__ __forceinline__ int products_recipe(const ProdMember *__restrict__ M, const ProdTabs &T, const double *__restrict__ in,
                                               int64_t in_sd, bool need_piso, const ProdRecipe &R) {
    constexpr int ND = 2 * NS + 2;
    double t[ND];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        t[k] = in[k * in_sd];
        finite = finite && isfinite(t[k]);
    }
    const int nt = M->nt, ng = M->ng, niso = M->niso, npiso = M->npiso;
    int st = finite ? MSX_W_OK : MSX_W_REJECT;
    // the reference interpolates every star's log g before it builds the first spectrum (mft6.py:2491): a Teff outside the
    // isochrone, on any star, raises first
    if (st == MSX_W_OK) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (!(t[s] >= T.iso_t[0]) || !(t[s] <= T.iso_t[niso - 1])) st = MSX_W_VALUEERROR;
            if (need_piso && (!(t[s] >= T.piso_t[0]) || !(t[s] <= T.piso_t[npiso - 1]))) st = MSX_W_VALUEERROR;
        }
    }
    if (st == MSX_W_OK) {
        const double plx = t[2 * NS + 1];
        const bool use_distance = M->dist_fit != 0;
        const int stride = M->node_stride;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (st != MSX_W_OK) continue;
            const double lg = interp_from_count(T.iso_t, T.iso_g, niso, t[s], prod_count_le(T.iso_t, niso, t[s]));  // mft6.py:95
            int t1 = 0, t2 = 0, g1 = 0, g2 = 0;
            st = prod_bracket(T.teff, nt, t[s], t1, t2);
            if (st == MSX_W_OK) st = prod_bracket(T.logg, ng, lg, g1, g2);
            if (st != MSX_W_OK) continue;
            const int n11 = t1 * ng + g1, n12 = t1 * ng + g2, n21 = t2 * ng + g1, n22 = t2 * ng + g2;
            if (!M->present[n11] || !M->present[n12] || !M->present[n21] || !M->present[n22]) { st = MSX_W_KEYERROR; continue; }
            const double a = (g1 == g2) ? 0.0 : (lg - T.logg[g1]) / (T.logg[g2] - T.logg[g1]);
            const double b = (t1 == t2) ? 0.0 : (t[s] - T.teff[t1]) / (T.teff[t2] - T.teff[t1]);
            double sc;
            if (use_distance) {
                const double di = 1.0 / plx;  // mft6.py:690
                const double r = (s == 0) ? t[NS + 1] : t[NS + 1] * t[NS + 1 + s];
                const double q = r * kRsunCm / (di * kPcCm);  // mft6.py:691,700
                sc = q * q;
            } else {
                sc = (s == 0) ? 1.0 : t[NS + 1 + s] * t[NS + 1 + s];  // mft6.py:703: the radius ratio squared
            }
            const int off = s * stride;  // component grid: star s reads copy s
            R.node[(4 * s) * kProdThreads] = n11 + off; R.node[(4 * s + 1) * kProdThreads] = n12 + off;
            R.node[(4 * s + 2) * kProdThreads] = n21 + off; R.node[(4 * s + 3) * kProdThreads] = n22 + off;
            R.w[(4 * s) * kProdThreads] = (1.0 - b) * (1.0 - a) * sc; R.w[(4 * s + 1) * kProdThreads] = (1.0 - b) * a * sc;
            R.w[(4 * s + 2) * kProdThreads] = b * (1.0 - a) * sc; R.w[(4 * s + 3) * kProdThreads] = b * a * sc;
        }
    }
    return st;
}

// One sample: status (MSX_W_*), and its columns written at out[j * out_sd] (NaN unless MSX_W_OK).
template <int NS>
__device__ __forceinline__ int products_eval(const ProdMember *__restrict__ M, const ProdTabs &T, const double *__restrict__ in,
                                             int64_t in_sd, const uint32_t *cols, int ncols, bool need_piso, const ProdRecipe &R,
                                             double *__restrict__ out, int64_t out_sd) {
    constexpr int ND = 2 * NS + 2;
    const int st = products_recipe<NS>(M, T, in, in_sd, need_piso, R);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (st != MSX_W_OK) {
        for (int j = 0; j < ncols; ++j) out[j * out_sd] = nan;
        return st;
    }
    const double ratio = in[(NS + 2) * in_sd];  // R2 / R1                                   mft6.py:2504
    const int niso = M->niso, npiso = M->npiso;
    const int nc = M->nc, nb = M->nc + M->np, npb = M->npb;
    for (int j = 0; j < ncols; ++j) {
        const uint32_t code = cols[j];
        const uint32_t kind = code >> 24;
        const int b = (int)((code >> 8) & 0xffu), s = (int)(code & 0xffu);
        double v = nan;
        if (!pcol_known(code, ND, NS, npb, nc, nb - nc)) {
            // (the host entry points refuse such a code; a caller of the device-pointer one gets NaN, never a read past a table)
        } else if (kind == 0) {  // a coordinate (read again: the registers that hold theta are not indexed at run time)
            v = in[(int64_t)code * in_sd];
        } else if (kind <= kPcolSecCorr) {
            const double zm = M->kind[b] == MSX_PB_MEAN ? M->zero_mag[b] : 0.0;
            if (kind == kPcolBandMag) {
                v = -2.5 * log10(star_integral(M->prod_tab, npb, b, R, s)) - zm;  // mft6.py:802,:813,:825
            } else if (kind == kPcolBandMagSum) {
                v = -2.5 * log10(composite_integral<NS>(M->prod_tab, npb, b, R)) - zm;  // mft6.py:812
            } else {
                const int sec = kind == kPcolDmag ? s : 1;
                const double mag_s = -2.5 * log10(star_integral(M->prod_tab, npb, b, R, sec)) - zm;
                const double mag_0 = -2.5 * log10(star_integral(M->prod_tab, npb, b, R, 0)) - zm;
                const double dmag = mag_s - mag_0;  // mft6.py:2505
                if (kind == kPcolDmag) v = dmag;
                else if (kind == kPcolPriCorr) v = sqrt(1.0 + pow(10.0, -0.4 * dmag));  // mft6.py:2544
                else v = ratio * sqrt(1.0 + pow(10.0, 0.4 * dmag));                      // mft6.py:2545
            }
        } else if (kind == kPcolContrast) {
            const int sec = (NS == 3 && s >= nc / 2) ? 2 : 1;  // mft6.py:747-749
            const double mag_s = -2.5 * log10(star_integral(M->band_tab, nb, s, R, sec));  // mft6.py:733
            v = mag_s - -2.5 * log10(star_integral(M->band_tab, nb, s, R, 0));              // mft6.py:741
        } else if (kind == kPcolPhot) {
            v = -2.5 * log10(composite_integral<NS>(M->band_tab, nb, nc + s, R) / M->pzero[s]);  // mft6.py:780-782
        } else {  // the isochrones at T_s
            const double ts = in[(int64_t)s * in_sd];
            if (kind == kPcolLogg) {
                v = interp_from_count(T.iso_t, T.iso_g, niso, ts, prod_count_le(T.iso_t, niso, ts));  // mft6.py:95
            } else {
                const double *ys = kind == kPcolMass ? T.piso_m : T.piso_l;
                v = interp_from_count(T.piso_t, ys, npiso, ts, prod_count_le(T.piso_t, npiso, ts));  // mft6.py:2685-2690
            }
        }
        out[j * out_sd] = v;
    }
    return MSX_W_OK;
}

// the small tables of a workgroup's member into LDS (s_iso [5 kProdIsoMax], s_node [2 kProdNodeMax]); longer ones are read
// where they are.  All threads call it; the caller's barrier follows.
__device__ __forceinline__ void load_prod_tabs(const ProdMember *__restrict__ M, ProdTabs &T, double *s_iso, double *s_node) {
    const int tid = threadIdx.x;
    const int niso = M->niso, npiso = M->npiso, nt = M->nt, ng = M->ng;
    T.iso_t = M->iso_t; T.iso_g = M->iso_g; T.piso_t = M->piso_t; T.piso_m = M->piso_m; T.piso_l = M->piso_l;
    T.teff = M->teff_nodes; T.logg = M->logg_nodes;
    if (niso <= kProdIsoMax) {
        for (int i = tid; i < niso; i += kProdThreads) { s_iso[i] = M->iso_t[i]; s_iso[kProdIsoMax + i] = M->iso_g[i]; }
        T.iso_t = s_iso; T.iso_g = s_iso + kProdIsoMax;
    }
    if (npiso <= kProdIsoMax) {
        for (int i = tid; i < npiso; i += kProdThreads) {
            s_iso[2 * kProdIsoMax + i] = M->piso_t[i]; s_iso[3 * kProdIsoMax + i] = M->piso_m[i]; s_iso[4 * kProdIsoMax + i] = M->piso_l[i];
        }
        T.piso_t = s_iso + 2 * kProdIsoMax; T.piso_m = s_iso + 3 * kProdIsoMax; T.piso_l = s_iso + 4 * kProdIsoMax;
    }
    if (nt <= kProdNodeMax) {
        for (int i = tid; i < nt; i += kProdThreads) s_node[i] = M->teff_nodes[i];
        T.teff = s_node;
    }
    if (ng <= kProdNodeMax) {
        for (int i = tid; i < ng; i += kProdThreads) s_node[kProdNodeMax + i] = M->logg_nodes[i];
        T.logg = s_node + kProdNodeMax;
    }
}

// grid (blocks of a member's samples, members): the block's member is uniform, so its small tables go to LDS once
template <int NS>
__global__ void __launch_bounds__(kProdThreads) products_kernel(const ProdLaunch L) {
    __shared__ double s_iso[5 * kProdIsoMax];
    __shared__ double s_node[2 * kProdNodeMax];
    __shared__ uint32_t s_cols[MSX_MAX_PCOLS];
    __shared__ double s_w[NS * 4 * kProdThreads];
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    const int m = blockIdx.y;
    const int64_t w0 = L.off ? L.off[m] : 0, nwalk = L.off ? L.off[m + 1] - w0 : L.n_single;
    const int64_t count = nwalk * L.nrows;
    if ((int64_t)blockIdx.x * kProdThreads >= count) return;  // (the whole block)
    const ProdMember *M = L.members + m;
    const int tid = threadIdx.x;
    ProdTabs T;
    load_prod_tabs(M, T, s_iso, s_node);
    const int ncols = L.ncols < MSX_MAX_PCOLS ? L.ncols : MSX_MAX_PCOLS;
    for (int i = tid; i < ncols; i += kProdThreads) s_cols[i] = L.cols[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kProdThreads + tid;
    if (i >= count) return;
    // consecutive threads take consecutive rows of one walker: a series' rows are its contiguous axis
    const int64_t wk = w0 + i / L.nrows, row = L.row0 + i % L.nrows;
    const ProdRecipe R{s_rn + tid, s_w + tid};
    const int st = products_eval<NS>(M, T, L.in + wk * L.in_sw + row * L.in_sr, L.in_sd, s_cols, ncols, L.need_piso != 0, R,
                                     L.out + wk * L.out_sw + row * L.out_sr, L.out_sd);
    if (L.status) L.status[wk] = st;
    if (L.worst && st != MSX_W_OK) atomicMax(L.worst + m, st);
}


// ---- spectra of samples on the data pixels (msx_products_spectra): one workgroup per sample --------------------------
// out [1 + NS][npix] in PIXEL order: rows 1.. each star's spectrum scaled as in make_composite, reddened by the sample's
// A_V on the model grid and resampled to the data pixels (mft6.py:2394-2402: with y the star's blend at the two grid
// samples that bracket the pixel, e = 10^(-0.4 A_V k) there, m = e_lo y_lo + (e_hi y_hi - e_lo y_lo) t); row 0 their sum in
// star order (:744, :751).  flags & MSX_SPEC_MEDIAN_SCALE: row 0 times median(data) / median(row 0) (:2409), the exact
// median by median.h's radix_select.  A_V <= 0, or a problem staged without extinction: no reddening (mft6.py:1161).
// one data pixel of a sample whose recipe is R: m [NS] each star's value, returned their sum in star order.  The one
// statement of a pixel's arithmetic: products_spectra_kernel and the predictive kernels (predictive_kernels.h) both call
// it, so a sample's pixel has the same bits wherever it is computed.
template <int NS>
__device__ __forceinline__ double spectra_pixel(const ProdMember *__restrict__ M, const ProdRecipe &R, int64_t nwl, bool redden,
                                                double redc, int64_t p, double (&m)[NS]) {
    const int64_t lo = M->pix_lo[p];
    const double t = M->pix_t[p];
    const double e_lo = redden ? exp2(redc * M->kgrid[lo]) : 1.0, e_hi = redden ? exp2(redc * M->kgrid[lo + 1]) : 1.0;
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double y_lo = 0.0, y_hi = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double w = R.w[(4 * s + c) * kProdThreads];
            const double *row = M->grid + (int64_t)R.node[(4 * s + c) * kProdThreads] * nwl + lo;
            y_lo = fma(w, row[0], y_lo);
            y_hi = fma(w, row[1], y_hi);
        }
        const double a = e_lo * y_lo, b = e_hi * y_hi;
        m[s] = a + (b - a) * t;  // interp1d(ww, extinct(ww, star, e))(wl)   mft6.py:2395-2402
        tot = s == 0 ? m[s] : tot + m[s];
    }
    return tot;
}

struct SpecLaunch {
    const ProdMember *M;
    const double *theta;
    double *out, *scale_out;
    int32_t *status;
    int32_t ndim, flags;
};
template <int NS>
__global__ void __launch_bounds__(kProdThreads) products_spectra_kernel(const SpecLaunch L) {
    __shared__ double s_iso[5 * kProdIsoMax];
    __shared__ double s_node[2 * kProdNodeMax];
    __shared__ double s_w[NS * 4 * kProdThreads];
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    __shared__ int s_st;
    __shared__ BlockScratch S;
    const ProdMember *M = L.M;
    const int tid = threadIdx.x;
    const int64_t smp = blockIdx.x;
    ProdTabs T;
    load_prod_tabs(M, T, s_iso, s_node);
    __syncthreads();
    const double *th = L.theta + smp * L.ndim;
    const ProdRecipe R{s_rn, s_w};  // thread 0's slots: the workgroup's one recipe
    if (tid == 0) s_st = products_recipe<NS>(M, T, th, 1, false, R);
    __syncthreads();
    const int st = s_st;
    const int64_t npix = M->npix, nwl = M->nwl;
    double *out = L.out + smp * (1 + NS) * npix;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) L.status[smp] = st;
    if (st != MSX_W_OK) {
        for (int64_t p = tid; p < (1 + NS) * npix; p += kProdThreads) out[p] = nan;
        if (tid == 0) L.scale_out[smp] = nan;
        return;
    }
    const double a_v = th[NS];
    const bool redden = M->use_av != 0 && a_v > 0.0;  // mft6.py:1161
    const double redc = -0.4 * kLog2Of10 * a_v;
    for (int64_t p = tid; p < npix; p += kProdThreads) {
        double m[NS];
        const double tot = spectra_pixel<NS>(M, R, nwl, redden, redc, p, m);
#pragma unroll
        for (int s = 0; s < NS; ++s) out[(1 + s) * npix + p] = m[s];
        out[p] = tot;
    }
    if (!(L.flags & MSX_SPEC_MEDIAN_SCALE)) {
        if (tid == 0) L.scale_out[smp] = 1.0;
        return;
    }
    __threadfence_block();
    __syncthreads();
    const unsigned int k1 = (unsigned int)((npix - 1) >> 1);
    const unsigned long long v1 = radix_select(out, (int)npix, k1, 0ull, ~0ull, S);
    __syncthreads();
    const unsigned long long v2 = (npix & 1) ? v1 : radix_select(out, (int)npix, k1 + 1, 0ull, ~0ull, S);
    const double med = v1 == v2 ? val_of(v1) : (val_of(v1) + val_of(v2)) / 2.0;  // np.median: the mean of the two middle elements
    const double factor = M->median_flux / med;  // mft6.py:2409
    __syncthreads();
    for (int64_t p = tid; p < npix; p += kProdThreads) out[p] *= factor;
    if (tid == 0) L.scale_out[smp] = factor;
}

// one row per star of make_composite's blend over grid samples [j0, j0 + n) (msx_composite_parts): composite_kernel's sum,
// star by star, on an explicit window.  grid (blocks of samples, stars).
__global__ void composite_parts_kernel(DevProblem P, const WalkerDesc *__restrict__ Dp, int64_t j0, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= n || Dp->status != MSX_W_OK) return;
    double acc = 0.0;
    for (int c = 0; c < 4; ++c) acc = fma(Dp->w[4 * s + c], P.grid[(int64_t)Dp->node[4 * s + c] * P.nwl + j0 + i], acc);
    out[(int64_t)s * n + i] = acc;
}

}  // namespace

#endif  // MSX_PRODUCT_KERNELS_H
