// predictive_kernels.h -- part of the single translation unit msx.hip (included there, in this order).
// posterior predictive checks (include/msx.h, msx_predictive_batch / msx_series_predictive): a chain
// streamed through the model once more and reduced per data pixel.  Three kernels --
//   sample : one workgroup per sample: the recipe, row 0 into a work row, its exact median, the quadratic fit of data / model,
//            the three chi^2 terms; leaves the sample's record (recipe, scale, fit coefficients)
//   fill   : a tile of pixels of the valid samples from their records, written SAMPLE-CONTIGUOUS per (row, pixel) through an
//            LDS transpose (rows: composite, stars, data_n, z, z^2)
//   reduce : one workgroup per (row, pixel): min, max, the two-pass mean and variance in a fixed order, radix selection
// -- none waits for another workgroup, none adds doubles atomically, ScratchSize 0 (tests/test_predictive_abi.py).
#ifndef MSX_PREDICTIVE_KERNELS_H
#define MSX_PREDICTIVE_KERNELS_H

namespace {

constexpr int kPredThreads = kProdThreads;
constexpr int kPredTile = 16;   // samples x pixels of a fill workgroup's transpose tile (16 x 16 = its threads)
constexpr int kPredExtra = 3;   // rows behind the spectra: data_n, z, z^2
static_assert(kPredTile * kPredTile == kPredThreads, "one thread per element of the transpose tile");

// where the samples are: sample i is walker w0 + i % W of row row0 + (i / W) * rstep, its element d at
// base[walker * sw + row * sr + d * sd] -- a batch [n][ndim] has W = n, sw = ndim, sd = 1; a series [ndim][nw][cap] has
// sw = cap, sr = 1, sd = nw * cap, and i runs in (row, walker) order: get_chain(flat=True)'s
struct PredSrc {
    const double *base;
    int64_t W, w0, sw, sr, sd, row0, rstep;
};
__device__ __forceinline__ int64_t pred_offset(const PredSrc &S, int64_t i, int64_t sw, int64_t sr) {
    return (S.w0 + i % S.W) * sw + (S.row0 + (i / S.W) * S.rstep) * sr;
}

// what the sample pass leaves of a sample for the fill pass
struct PredRec {
    double scale, c0, c1, c2;  // median(data) / median(row 0); the fit's coefficients                mft6.py:1173,:195
    double redc;               // the reddening's exp2 coefficient
    double w[4 * MSX_MAX_SPEC];
    int32_t node[4 * MSX_MAX_SPEC];
    int32_t redden, pad;
};

// data_n = data / P(u), z = (model - data_n) / sigma, z^2 (mft6.py:196, :120); no contraction: `model` is a product, and
// a pixel's z must not depend on which kernel forms it
__device__ __forceinline__ void pred_resid(double model, double flux, double err, double u, double c0, double c1, double c2,
                                           double &dn, double &z, double &z2) {
#pragma clang fp contract(off)
    const double poly = fma(fma(c2, u, c1), u, c0);
    dn = flux / poly;
    z = (model - dn) / err;
    z2 = z * z;
}

// the workgroup's sum of v in a fixed order: lanes by wave_sum, then waves 0.. serially (slot: S.q[which])
__device__ __forceinline__ double pred_block_sum(double v, BlockScratch &S, int which) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double ws = wave_sum(v);
    __syncthreads();  // (whoever still reads the slot's previous contents is done)
    if (lane == 0) S.q[which][wave] = ws;
    __syncthreads();
    double tot = S.q[which][0];
#pragma unroll
    for (int x = 1; x < kPredThreads / kWave; ++x) tot += S.q[which][x];
    return tot;
}

struct PredSampleLaunch {
    const ProdMember *M;
    PredSrc src;
    int64_t i0;          // the batch's first sample; workgroup b takes sample i0 + b and work row b
    double *work;        // [batch][npix]
    PredRec *rec;        // [all samples]
    int32_t *status;     // [all samples]
    double *terms;       // element d of sample i at terms[pred_offset(src, i, t_sw, t_sr) + d * t_sd]; or null
    int64_t t_sw, t_sr, t_sd;
};
template <int NS>
__global__ void __launch_bounds__(kPredThreads) predictive_sample_kernel(const PredSampleLaunch L) {
    __shared__ double s_iso[5 * kProdIsoMax];
    __shared__ double s_node[2 * kProdNodeMax];
    __shared__ double s_w[NS * 4 * kProdThreads];
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    __shared__ int s_st;
    __shared__ BlockScratch S;
    const ProdMember *M = L.M;
    const int tid = threadIdx.x;
    const int64_t smp = L.i0 + blockIdx.x;
    ProdTabs T;
    load_prod_tabs(M, T, s_iso, s_node);
    __syncthreads();
    const double *th = L.src.base + pred_offset(L.src, smp, L.src.sw, L.src.sr);
    const int64_t sd = L.src.sd;
    const ProdRecipe R{s_rn, s_w};  // thread 0's slots: the workgroup's one recipe
    if (tid == 0) s_st = products_recipe<NS>(M, T, th, sd, false, R);
    __syncthreads();
    const int st = s_st;
    const int64_t npix = M->npix, nwl = M->nwl;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double *terms = L.terms ? L.terms + pred_offset(L.src, smp, L.t_sw, L.t_sr) : nullptr;
    if (tid == 0) L.status[smp] = st;
    if (st != MSX_W_OK) {
        if (tid == 0 && terms) {
#pragma unroll
            for (int d = 0; d < 4; ++d) terms[d * L.t_sd] = nan;
        }
        return;
    }
    const double a_v = th[NS * sd];
    const bool redden = M->use_av != 0 && a_v > 0.0;  // mft6.py:1161
    const double redc = -0.4 * kLog2Of10 * a_v;
    double *work = L.work + (int64_t)blockIdx.x * npix;
    for (int64_t p = tid; p < npix; p += kPredThreads) {
        double m[NS];
        work[p] = spectra_pixel<NS>(M, R, nwl, redden, redc, p, m);
    }
    __threadfence_block();
    __syncthreads();
    // the median scale, as products_spectra_kernel forms it
    const unsigned int k1 = (unsigned int)((npix - 1) >> 1);
    const unsigned long long v1 = radix_select(work, (int)npix, k1, 0ull, ~0ull, S);
    __syncthreads();
    const unsigned long long v2 = (npix & 1) ? v1 : radix_select(work, (int)npix, k1 + 1, 0ull, ~0ull, S);
    const double med = v1 == v2 ? val_of(v1) : (val_of(v1) + val_of(v2)) / 2.0;
    const double factor = M->median_flux / med;  // mft6.py:1173, :2409
    // the quadratic fit of data / model against [1, u, u^2]                                     mft6.py:193-195
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int64_t p = tid; p < npix; p += kPredThreads) {
        const double model = work[p] * factor, u = M->pix_u[p];
        const double f = M->pix_flux[p] / model;
        q0 += f; q1 += f * u; q2 += f * (u * u);
    }
    q0 = pred_block_sum(q0, S, 0);
    q1 = pred_block_sum(q1, S, 1);
    q2 = pred_block_sum(q2, S, 2);
    const double c0 = M->minv[0] * q0 + M->minv[1] * q1 + M->minv[2] * q2;
    const double c1 = M->minv[3] * q0 + M->minv[4] * q1 + M->minv[5] * q2;
    const double c2 = M->minv[6] * q0 + M->minv[7] * q1 + M->minv[8] * q2;
    double chi = 0.0;
    for (int64_t p = tid; p < npix; p += kPredThreads) {
        double dn, z, z2;
        pred_resid(work[p] * factor, M->pix_flux[p], M->pix_err[p], M->pix_u[p], c0, c1, c2, dn, z, z2);
        chi += z2;
    }
    chi = pred_block_sum(chi, S, 0);
    if (tid != 0) return;
    PredRec rec;
    rec.scale = factor; rec.c0 = c0; rec.c1 = c1; rec.c2 = c2; rec.redc = redc; rec.redden = redden ? 1 : 0; rec.pad = 0;
#pragma unroll
    for (int c = 0; c < 4 * MSX_MAX_SPEC; ++c) {
        rec.w[c] = c < 4 * NS ? R.w[c * kProdThreads] : 0.0;
        rec.node[c] = c < 4 * NS ? R.node[c * kProdThreads] : 0;
    }
    L.rec[smp] = rec;
    if (!terms) return;
    const int nc = M->nc, np = M->np, nb = nc + np;
    double chi_c = 0.0, chi_p = 0.0;
    for (int f = 0; f < nc; ++f) {
        const int sec = (NS == 3 && f >= nc / 2) ? 2 : 1;  // mft6.py:747-749
        const double mag_s = -2.5 * log10(star_integral(M->band_tab, nb, f, R, sec));  // mft6.py:733
        const double con = mag_s - -2.5 * log10(star_integral(M->band_tab, nb, f, R, 0));  // mft6.py:741
        const double z = con - M->cmag[f];
        chi_c += (z * z) / (M->cerr[f] * M->cerr[f]);  // mft6.py:120,:1182
    }
    for (int f = 0; f < np; ++f) {
        const double mag = -2.5 * log10(composite_integral<NS>(M->band_tab, nb, nc + f, R) / M->pzero[f]);  // mft6.py:780-782
        const double mred = redden ? mag + a_v * M->pk[f] : mag;  // mft6.py:1163
        const double z = mred - M->pmag[f];
        chi_p += (z * z) / (M->perr[f] * M->perr[f]);  // mft6.py:1188
    }
    const double iic = chi / (double)npix;  // mft6.py:1179
    const double total = M->no_spectrum ? chi_c + chi_p : (iic * (double)nb + chi_c) + chi_p;  // mft6.py:1191
    terms[0] = iic; terms[L.t_sd] = chi_c; terms[2 * L.t_sd] = chi_p; terms[3 * L.t_sd] = total;
}

// pixels [p0, p0 + tp) of the valid samples vidx[0 .. count): vals[(r * tp + pixel) * count + j], r = 0 the scaled composite,
// 1 .. NS the stars, then data_n, z, z^2.  grid (groups of kPredTile samples, strides over the tile's pixel chunks)
struct PredFillLaunch {
    const ProdMember *M;
    const PredRec *rec;
    const int64_t *vidx;
    int64_t count, p0, tp;
    double *vals;
};
template <int NS>
__global__ void __launch_bounds__(kPredThreads) predictive_fill_kernel(const PredFillLaunch L) {
    constexpr int NR = 1 + NS + kPredExtra;
    __shared__ double s_w[NS * 4 * kProdThreads];    // (ProdRecipe's layout: slot j of corner c at [c * kProdThreads + j])
    __shared__ int32_t s_rn[NS * 4 * kProdThreads];
    __shared__ double s_par[5][kPredTile];
    __shared__ int32_t s_red[kPredTile];
    __shared__ double s_tile[NR][kPredTile][kPredTile + 1];
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
            const double model = tot * s_par[0][hi];  // row 0 of msx_products_spectra with MSX_SPEC_MEDIAN_SCALE
            pred_resid(model, M->pix_flux[p], M->pix_err[p], M->pix_u[p], s_par[1][hi], s_par[2][hi], s_par[3][hi], dn, z, z2);
            s_tile[0][lo][hi] = model;
#pragma unroll
            for (int s = 0; s < NS; ++s) s_tile[1 + s][lo][hi] = m[s];
            s_tile[1 + NS][lo][hi] = dn; s_tile[2 + NS][lo][hi] = z; s_tile[3 + NS][lo][hi] = z2;
        }
        __syncthreads();
        if (j0 + lo < L.count && pc + hi < L.tp) {
#pragma unroll
            for (int r = 0; r < NR; ++r) L.vals[((int64_t)r * L.tp + pc + hi) * L.count + j0 + lo] = s_tile[r][hi][lo];
        }
        __syncthreads();
    }
}

// grid (pixels of the tile, rows): x = the (row, pixel)'s count values in sample order.  Rows 0 .. NS: band [4][1 + NS][npix]
// = mean, variance (ddof 1), min, max and ostat [nranks][1 + NS][npix] = the elements of ranks[]; rows behind: resid
// [3][npix] = the mean.  A sum is every thread's own stride in order, the lanes by wave_sum, the waves serially: a function
// of the ordered list alone.  The variance is two-pass: sum (x - mean)^2 over the same order.
struct PredReduceLaunch {
    const double *vals;
    int64_t count, p0, tp, npix;
    int32_t nrows;  // 1 + NS
    int32_t nranks;
    const int64_t *ranks;
    double *band, *ostat, *resid;
};
__global__ void __launch_bounds__(kPredThreads) predictive_reduce_kernel(const PredReduceLaunch L) {
    __shared__ BlockScratch S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.y;
    const int64_t p = L.p0 + blockIdx.x, n = L.count;
    const double *x = L.vals + ((int64_t)row * L.tp + blockIdx.x) * n;
    double part = 0.0, vmin = INFINITY, vmax = -INFINITY;
    for (int64_t j = tid; j < n; j += kPredThreads) {
        const double v = x[j];
        part += v;
        vmin = min_nc(vmin, v);
        vmax = max_nc(vmax, v);
    }
    const double mean = pred_block_sum(part, S, 0) / (double)n;
    if (row >= L.nrows) {
        if (tid == 0) L.resid[(int64_t)(row - L.nrows) * L.npix + p] = mean;
        return;
    }
    part = 0.0;
    for (int64_t j = tid; j < n; j += kPredThreads) {
        const double d = x[j] - mean;
        part += d * d;
    }
    const double var = pred_block_sum(part, S, 1) / (double)(n - 1);  // n == 1: 0 / 0, np.var(ddof=1)'s NaN
    const double wlo = wave_min_f64(vmin), whi = wave_max_f64(vmax);
    if (lane == 0) { S.chi[wave] = wlo; S.q[2][wave] = whi; }
    __syncthreads();
    double lo = S.chi[0], hi = S.q[2][0];
#pragma unroll
    for (int w = 1; w < kPredThreads / kWave; ++w) { lo = min_nc(lo, S.chi[w]); hi = max_nc(hi, S.q[2][w]); }
    const int64_t at = (int64_t)row * L.npix + p, plane = (int64_t)L.nrows * L.npix;
    if (tid == 0) { L.band[at] = mean; L.band[plane + at] = var; L.band[2 * plane + at] = lo; L.band[3 * plane + at] = hi; }
    // (fmin / fmax do not order -0 and +0: a zero bound stands for both, as in exact_range)
    const unsigned long long kmin = key_of(lo == 0.0 ? -0.0 : lo), kmax = key_of(hi == 0.0 ? 0.0 : hi);
    unsigned long long v = 0ull;
    for (int r = 0; r < L.nranks; ++r) {
        if (r == 0 || L.ranks[r] != L.ranks[r - 1]) {
            __syncthreads();
            v = radix_select(x, (int)n, (unsigned int)L.ranks[r], kmin, kmax, S);
        }
        if (tid == 0) L.ostat[(int64_t)r * plane + at] = val_of(v);
    }
}

}  // namespace

#endif  // MSX_PREDICTIVE_KERNELS_H
