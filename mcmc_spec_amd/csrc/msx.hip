// msx.hip -- gfx950 (CDNA4) kernels + C ABI for mcmc_spec's per-walker log-likelihood path.
//
// What is in here (rows of SURVEY.md §8a; reference = /root/reference/mft6.py):
//   A0  staged grid [nt][ng][nwl] in HBM                      (specs dict, :342-383)
//   A1  isochrone Teff -> logg / luminosity lookup            (get_logg :87-98, get_radius :66-85)
//   A2  nearest-node bracket + bilinear blend                 (get_spec :387-563)
//   A3  Gaussian instrumental broadening, LDS-tiled FIR       (broaden :124-152 -> instrBroadGaussFast)
//   A4  flux scaling + component sum                          (make_composite :687-707,:740-751)
//   A5  contrast magnitudes via per-node band integrals       (:713-741)
//   A6  unresolved photometry via per-node band integrals     (:755-783)
//   A7  CCM89 reddening                                       (extinct :46-64)
//   A8  resample to data pixels, median scale, quadratic fit  (:1169-1174, norm_spec :193-196)
//   A9  chi^2 + combine                                       (chisq :115-122, :1178-1205)
//   f1  prior box + Gaussian terms                            (logprior :1207-1272, logposterior :1459-1470)
//
// Layout of the translation unit (device code in headers, included below in this order):
//   dev_types.h        constants, DevProblem (by-value kernel argument), WalkerDesc (LDS)
//   wave_ops.h         DPP reductions / scans, order-preserving keys
//   blend.h            the per-pixel model arithmetic shared by the fused, linked and pair forms
//   recipe.h           phase 0: gates, isochrone, brackets, weights, prior and band terms
//   median.h           exact median selects (block_median, logbin_median, radix fallback)
//   logprob_kernel.h   the hot kernel and its variants (fused; linked = several workgroups per walker in one launch)
//   logprob_body.h     the fused kernel's body, included as text by logprob_kernel and logprob_group_kernel
//   group_kernel.h     target groups: the fused body over the walkers of several staged problems in one launch
//   pair_kernel.h      the pair form: two walkers of one grid cell per workgroup, one set of row loads
//   opt_run_kernels.h  the device-resident pre-optimiser: fit_spec's per-chain state machine, one thread per chain
//   staging_kernels.h  CCM89, pair gather, band integrals, broadening, resample, composite, stream copy
//   summary_kernels.h  order statistics and binned marginals of a device chain series
//   evidence_kernels.h block means and log-mean-exponentials of a series column (thermodynamic integration, stepping stone)
//   diag_kernels.h     split R-hat's within / between variances and the pooled mean and covariance of a series' members
//   msx.hip            host context + the C ABI of include/msx.h
//
// Design notes (details in DESIGN.md):
//   * one workgroup per walker; the walker's Npix-long model vector lives in LDS for the exact
//     median (radix select), the 3-term fit and the chi^2 pass; all sums are float64 with a fixed
//     reduction order (wave shuffles, then LDS across waves) -> bit-reproducible run to run.
//   * the resample (A8) only ever touches the two model samples bracketing each data pixel, and
//     those indices are static per dataset, so staging gathers them once into a pixel-major
//     "pair table" pairs[node][pix] = {flux[lo], flux[lo+1]}: every hot-loop load is a 16-byte
//     per-lane, fully coalesced read (1 KiB per wave instruction).
//   * wave = 64 lanes everywhere; no MFMA (nothing here is a GEMM); no CUDA-compat shims.

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <mutex>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/msx.h"

// The device code lives in the headers below (one translation unit; every kernel variant is instantiated here).
#include "dev_types.h"
#include "wave_ops.h"
#include "blend.h"
#include "recipe.h"
#include "median.h"
#include "logprob_kernel.h"
#include "move_kernels.h"
#include "tempered_kernels.h"
#include "group_tempered_kernels.h"
#include "group_kernel.h"
#include "pair_kernel.h"
#include "staging_kernels.h"
#include "inpath_kernels.h"
#include "autocorr_kernels.h"
#include "summary_kernels.h"
#include "evidence_kernels.h"
#include "diag_kernels.h"
#include "product_kernels.h"
#include "predictive_kernels.h"
#include "mode_kernels.h"
#include "reweight_kernels.h"
#include "psis_kernels.h"
#include "pointwise_kernels.h"
#include "rank_kernels.h"
#include "opt_run_kernels.h"

// ================================================================================================
// host side: context + C ABI
// ================================================================================================
struct msx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    hipDeviceProp_t prop;
    // grid
    int64_t nwl = 0;
    int nt = 0, ng = 0;
    std::vector<double> h_wl, h_teff, h_logg;  // host copies of the wavelength axis and the node lists
    double *d_grid = nullptr, *d_wl = nullptr, *d_kgrid = nullptr, *d_teff = nullptr, *d_logg = nullptr;
    uint8_t *d_present = nullptr;
    bool grid_staged = false;
    // problem
    bool problem_staged = false;
    DevProblem P;
    std::vector<void *> prob_allocs;
    void *h_pin = nullptr;        // pinned host staging for the host-pointer entry points
    int64_t cap_walkers = 0;
    double *d_misc = nullptr;  // composite args / desc / small outputs
    double *d_spec = nullptr;
    int64_t cap_spec = 0;
    double *d_opt_flux = nullptr, *d_opt_med = nullptr;
    int32_t *d_opt_chain = nullptr;
    int64_t opt_chains = 0, cap_chain = 0;
    int max_dyn_lds = 0;
    bool pf_ok = false;   // the LDS-staged-statics variants fit (msx_stage_problem)
    bool pf256_ok = false; // ... the 256-thread two-per-CU one (two workgroups of it in a CU's LDS)
    bool model_in_global = false;
    // RCCL all-gather of log-probabilities: communicator + its own stream + per-slot events
    void *rccl_comm = nullptr;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr;
    hipEvent_t ev_done[4] = {nullptr, nullptr, nullptr, nullptr};
    int comm_world = 0, comm_rank = 0;
    // LOOPBACK group (msx_comm_init_loopback): `comm_world` contexts of this process stand for the ranks of one job;
    // the all-gather of the sharded sampler becomes same-process device copies between their gathered vectors, driven
    // in lock-step by msx_sampler_enqueue_group.  No RCCL: the rank >= 1 paths run on a one-GPU box (tests).
    std::vector<msx_ctx *> loop_peers;   // all members in rank order (this context at [comm_rank]); empty = none
    hipEvent_t loop_eval_done = nullptr; // this rank's block of log p(q) is in its gathered vector
    hipEvent_t loop_copied = nullptr;    // this rank has copied every peer's block (peers may overwrite theirs)
    // Scratch rows (walkers per sub-batch), sized once at msx_stage_problem and only for the forms that can run on
    // the staged spectrum: model vectors of the GM variants (> 17,152 pixels) and of the linked form's scratch-row exit
    // (2..8 segments of 8192 pixels), the segments' partials and arrival counters.  No launch allocates.
    double *d_model_scratch = nullptr;
    SegPart *d_segparts = nullptr;  // linked form: [scratch_rows][segments]
    unsigned long long *d_seg_flag = nullptr;  // linked form: [scratch_rows] arrival counters (a multiple of 2 x segments between launches), + the poison word
    int nseg = 1;                   // segments of the staged spectrum (8192 pixels each)
    int64_t scratch_rows = 0;       // 0 = neither form applies: launches are never cut into sub-batches
    int32_t path = 0;               // MSX_PATH_AUTO / _FUSED / _PAIR / _LINKED (msx_set_path)
    // in-path broadening (inpath_kernels.h; msx_set_broadening, MSX_PATH_INPATH): the raw window rows kept by
    // msx_broaden_grid, the taps' parameters, and the form's scratch (sized at msx_stage_problem)
    int32_t broaden_placement = 0;  // MSX_BROADEN_STAGING / MSX_BROADEN_IN_PATH (takes effect at the next msx_broaden_grid)
    double *d_raw_win = nullptr;    // [nt * ng][raw_n]: the window before the broadening
    int64_t raw_i0 = 0, raw_n = 0;
    int raw_lx = 0;
    double raw_dx = 0.0, raw_sigma = 0.0;
    bool grid_rotated = false;      // msx_rot_broaden_grid ran since the last msx_broaden_grid / grid: no raw window (named in INPATH's refusal)
    int32_t ncomp = 1;              // copies of the node rows (msx_split_components / msx_stage_grid_components): d_grid is [ncomp][nt*ng][nwl]
    InpathRec *d_inp_rec = nullptr;
    double *d_inp_tmp = nullptr, *d_inp_given = nullptr;
    const int64_t *d_pix_lo = nullptr;
    const double *d_pix_err = nullptr;  // sigma per pixel as staged (the predictive check's z; the hot path reads 1 / sigma^2)
    int64_t inp_rows = 0, inp_gstride = 0;  // walkers per sub-batch (0: the staged problem has no in-path form)
    // pair form (pair_kernel.h): binaries of <= 4096 pixels with the register-resident recipe
    int64_t pair_rows = 0;          // walkers per sub-batch = capacity of the planner's item lists (0: no pair form here)
    // MSX_PATH_AUTO takes the pair form from this many walkers on (MSX_PAIR_MIN; 0 = never); set per problem by
    // msx_stage_problem, with the measurements behind the rule
    int64_t pair_min_walkers = 4096;
    int32_t *d_pair_plan = nullptr; // the planner's output (pair_kernel.h: header, pairs, singles)
    PairItem *d_pair_items = nullptr;   // ... and its items: the pairs' recipes, [pair_rows / 2]
    PairRec *d_pair_singles = nullptr;  // ... the singles', [pair_rows]
    // {pairs, singles} of the planner's last run, written by the device into host memory and read here WITHOUT waiting
    // for it (so possibly a launch or two old): MSX_PATH_AUTO's only evidence of whether pairing pays (pair_worth_it)
    int32_t *h_pair_stats = nullptr;
    int64_t pair_auto_launches = 0;
    int32_t linked = -1;            // MSX_LINKED: -1 = automatic (walkers x segments <= #CUs), 0 never, 1 whenever possible
    bool linked_poisoned = false;   // a hand-over of the linked form timed out on this context (seen by a synchronous
                                    // entry point): MSX_PATH_AUTO takes the fused form until the problem is staged again
    bool recipe_fast = false;       // the register-resident recipe applies (small tables)
    unsigned char *d_recipe_block = nullptr;  // ... and its tables in one block (dev_types.h), freed with the problem
    struct SamplerRun *smp = nullptr;  // device-resident sampler in flight (msx_sampler_begin .. _end)
    struct OptRun *opt_run = nullptr;  // device-resident pre-optimiser in flight (msx_opt_run_begin .. _end)
    struct TemperedRun *tmp = nullptr; // tempered ladder in flight (msx_tempered_begin .. _end); excludes smp
    bool smp_overlap_launch = false;   // the launch being queued is a half-step of an overlapped run: fused form, bit 20
    bool probe_launch = false;         // ... is msx_probe_launch's: the kernel leaves clock stamps (bit 21)
    int32_t last_form = 0;             // MSX_FORM_* of the last launch queued (msx_last_form)
    int32_t smp_overlap_policy = -1;   // msx_sampler_policy: -1 = overlap half-steps when the rule allows, 0 = never
    int32_t store_dtype = MSX_STORE_F64;  // msx_set_grid_storage: what the NEXT msx_stage_problem builds the R table in
    bool store_f32 = false;               // ... and what the staged problem holds
    // target groups (msx_group_*): the problem's GENERATION, counted up whenever the staged problem is dropped (free_problem:
    // restaging, grid staging, broadening, rotation, splitting) -- a group refuses a member whose generation moved -- and
    // the groups this context belongs to (back-pointers: msx_destroy clears its slots in them, msx_group_destroy leaves)
    uint64_t prob_gen = 0;
    std::vector<struct msx_group *> groups;
    // derived posteriors (msx_stage_products; product_kernels.h): the product bands' per-node table and the product
    // isochrone (prod_allocs), this context's record for the kernels (host copy + device copy), the window of plot=True,
    // and the device buffer the host-pointer batches go through.  Dropped with the problem (free_problem).
    bool products_staged = false;
    ProdMember PM;
    ProdMember *d_prod_member = nullptr;
    std::vector<void *> prod_allocs;
    char *d_prod_buf = nullptr;
    size_t prod_buf_bytes = 0;
};
static void sampler_free(msx_ctx *c);
static void opt_run_free(msx_ctx *c);
static void tempered_free(msx_ctx *c);

// A TARGET GROUP (include/msx.h): 1..MSX_MAX_GROUP staged contexts on one device whose walkers one launch of
// logprob_group_kernel evaluates, each against its own member's problem.  The group owns snapshots of the members'
// DevProblems and launch records in device memory; the tables they point to stay the members' own.
struct msx_group {
    int device = 0;
    std::string err;
    std::vector<msx_ctx *> members;       // nullptr: the member was destroyed (msx_destroy clears the slot)
    std::vector<uint64_t> gen;            // the members' problem generations at msx_group_create
    std::vector<DevProblem> probs;        // host copies of the snapshots (the launch plan reads them)
    std::vector<char> pf_ok, pf256_ok;    // the members' LDS-staged-statics variants fit
    int32_t nspec = 0;
    int64_t cus = 256;
    DevProblem *d_probs = nullptr;        // [k] the snapshots: sampler, probe, optimiser and in-path fields cleared
    GroupMember *d_members = nullptr;     // [k] their launch records
    void *h_pin = nullptr;                // pinned host staging of msx_group_logprob_batch
    int64_t cap_walkers = 0;
    struct GroupRun *run = nullptr;       // the device-resident sampler in flight (msx_group_sampler_begin .. _end)
    struct GroupTemperedRun *trun = nullptr;  // ... or the tempered ladders (msx_group_tempered_begin .. _end); excludes run
};
static void group_run_drain(msx_group *g);
static void group_run_free(msx_group *g);
static void group_tempered_drain(msx_group *g);
static void group_tempered_free(msx_group *g);

// A DEVICE CHAIN SERIES (include/msx.h, msx_series_*): a chain kept on the device as
// [ndim][nw][cap] doubles, filled by the runs it is attached to (run_finish) or from the host, read by the
// autocorrelation kernels (autocorr_kernels.h) on its own stream.  It belongs to whoever created it, not to a context:
// it outlives runs, and at most one run at a time appends to it.
struct msx_series {
    int device = 0;
    std::string err;
    hipStream_t stream = nullptr;        // append / read / acf
    int64_t nw = 0;
    int32_t ndim = 0;
    std::vector<int64_t> off;            // [k + 1] the members' walker offsets
    int64_t *d_off = nullptr;
    double *d_rows = nullptr;
    int64_t cap = 0, rows = 0;           // rows: written or queued to be written
    // growth while a run is attached happens at enqueue time, in the run's compute-stream order: the copy into the new
    // buffer sits behind the chunks already queued.  Readers wait for `grown` (recorded after the latest copy); the
    // buffers it replaced are freed when no run is attached (hipFree would wait for the whole device)
    hipEvent_t grown = nullptr;
    bool grown_set = false;
    std::vector<void *> retired;
    char *d_scratch = nullptr;           // acf's partial sums and results, append's / read's staging
    size_t scratch_bytes = 0;
    struct SamplerRun *run = nullptr;    // the run appending to it (msx_*sampler_attach_series .. the run's end)
    struct TemperedRun *trun = nullptr;  // ... or the tempered run (msx_series_attach_tempered .. msx_tempered_end)
    struct GroupTemperedRun *gtrun = nullptr;  // ... or a group's (msx_group_tempered_attach_series .. msx_group_tempered_end)
};
static void group_tempered_detach(msx_series *sr);

namespace {

// RCCL is resolved at run time from the copy PyTorch-ROCm already mapped (same SONAME librccl.so.1 as
// /opt/rocm's), so the process never holds two RCCL instances; nothing is linked at build time.
struct RcclUniqueId { char internal[128]; };
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclUniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, RcclUniqueId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
RcclApi &rccl() {
    static RcclApi api;
    if (api.handle) return api;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names) {
        api.handle = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
        if (api.handle) break;
    }
    for (int i = 0; !api.handle && i < 3; ++i) api.handle = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!api.handle) return api;
    api.GetUniqueId = (int (*)(RcclUniqueId *))dlsym(api.handle, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(void **, int, RcclUniqueId, int))dlsym(api.handle, "ncclCommInitRank");
    api.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(api.handle, "ncclAllGather");
    api.CommDestroy = (int (*)(void *))dlsym(api.handle, "ncclCommDestroy");
    api.GetErrorString = (const char *(*)(int))dlsym(api.handle, "ncclGetErrorString");
    api.ok = api.GetUniqueId && api.CommInitRank && api.AllGather && api.CommDestroy && api.GetErrorString;
    return api;
}
constexpr int kNcclFloat64 = 8;  // ncclFloat64 / ncclDouble (rccl.h)

int raise_dynamic_lds_limits(msx_ctx *c);  // (defined next to the launchers)

int fail(msx_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}
int fail(msx_group *g, int code, const std::string &msg) {
    if (g) g->err = msg;
    return code;
}
int fail(msx_series *sr, int code, const std::string &msg) {
    if (sr) sr->err = msg;
    return code;
}

// (h: an msx_ctx or an msx_group)
#define HIP_TRY(h, expr)                                                                           \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(h, MSX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));       \
    } while (0)

template <typename T>
int dev_alloc_copy(msx_ctx *c, std::vector<void *> *track, const T *host, int64_t count, T **out) {
    *out = nullptr;
    if (count <= 0) {
        // keep kernels simple: always a valid pointer
        HIP_TRY(c, hipMalloc((void **)out, 16));
        if (track) track->push_back(*out);
        return MSX_OK;
    }
    HIP_TRY(c, hipMalloc((void **)out, sizeof(T) * count));
    if (track) track->push_back(*out);
    HIP_TRY(c, hipMemcpy(*out, host, sizeof(T) * count, hipMemcpyHostToDevice));
    return MSX_OK;
}

void free_problem(msx_ctx *c) {
    sampler_free(c);  // a sampler in flight holds pointers into the problem's tables
    opt_run_free(c);  // ... and a pre-optimiser run into the chains' data vectors
    tempered_free(c); // ... and a tempered ladder
    for (msx_group *g : c->groups) group_run_drain(g);  // ... and so does a group's (its next enqueue is refused)
    ++c->prob_gen;    // (target groups holding a snapshot of the problem refuse this member from now on)
    for (void *p : c->prob_allocs) (void)hipFree(p);
    c->prob_allocs.clear();
    c->problem_staged = false;
    for (void *p : c->prod_allocs) (void)hipFree(p);  // the products read the problem's tables: they go with it
    c->prod_allocs.clear();
    if (c->d_prod_buf) (void)hipFree(c->d_prod_buf);
    c->d_prod_buf = nullptr; c->prod_buf_bytes = 0;
    c->d_prod_member = nullptr;
    c->products_staged = false;
    if (c->d_opt_flux) (void)hipFree(c->d_opt_flux);
    if (c->d_opt_med) (void)hipFree(c->d_opt_med);
    c->d_opt_flux = c->d_opt_med = nullptr;
    c->opt_chains = 0;
    if (c->h_pair_stats) (void)hipHostFree(c->h_pair_stats);
    c->h_pair_stats = nullptr;
    void *sp[] = {c->d_model_scratch, c->d_segparts, c->d_seg_flag, c->d_pair_plan, c->d_pair_items, c->d_pair_singles,
                  c->d_inp_rec, c->d_inp_tmp, c->d_inp_given};
    for (void *p : sp)
        if (p) (void)hipFree(p);
    c->d_segparts = nullptr; c->d_seg_flag = nullptr; c->d_model_scratch = nullptr; c->scratch_rows = 0;
    c->d_pair_plan = nullptr; c->d_pair_items = nullptr; c->d_pair_singles = nullptr; c->pair_rows = 0;
    c->linked_poisoned = false;
    c->d_inp_rec = nullptr; c->d_inp_tmp = c->d_inp_given = nullptr; c->d_pix_lo = nullptr; c->inp_rows = 0;
}

void free_grid(msx_ctx *c) {
    void *ptrs[] = {c->d_grid, c->d_wl, c->d_kgrid, c->d_teff, c->d_logg, c->d_present};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    c->d_grid = c->d_wl = c->d_kgrid = c->d_teff = c->d_logg = nullptr;
    c->d_present = nullptr;
    if (c->d_raw_win) (void)hipFree(c->d_raw_win);
    c->d_raw_win = nullptr; c->raw_n = 0;
    c->grid_rotated = false;
    c->ncomp = 1;
    c->grid_staged = false;
}

// the staged rows: nt*ng per copy, ncomp copies
int64_t grid_rows(const msx_ctx *c) { return (int64_t)c->ncomp * c->nt * c->ng; }

int conv_taps(double mean_wl, double dx, double resolution, double maxsig, double *sigma_out, int *lx_out) {
    // pyasl.instrBroadGaussFast: fwhm = mean(wl)/R; sigma = fwhm/(2 sqrt(2 ln 2)); broadGaussFast:
    // lx = int(((sigma*maxsig)/dx)*2.0) + 1
    const double fwhm = 1.0 / resolution * mean_wl;
    const double sigma = fwhm / (2.0 * sqrt(2.0 * log(2.0)));
    const int lx = (int)(((sigma * maxsig) / dx) * 2.0) + 1;
    *sigma_out = sigma;
    *lx_out = lx;
    return lx;
}

int check_even_spacing(msx_ctx *c, const double *wl, int64_t n) {
    // broadGaussFast: abs(max(dxs) - min(dxs)) > mean(dxs)*1e-6 -> error
    double mx = -INFINITY, mn = INFINITY, sum = 0.0;
    for (int64_t i = 1; i < n; ++i) {
        const double d = wl[i] - wl[i - 1];
        mx = d > mx ? d : mx;
        mn = d < mn ? d : mn;
        sum += d;
    }
    if (fabs(mx - mn) > (sum / (double)(n - 1)) * 1e-6)
        return fail(c, MSX_ERR_RANGE, "broaden: the wavelength axis is not equidistant");
    return MSX_OK;
}

int launch_conv(msx_ctx *c, const double *d_in, int64_t in_stride, double *d_tmp, int64_t rows, int64_t n, int lx,
                double dx, double sigma) {
    const size_t lds = sizeof(double) * ((size_t)lx + kConvTile + lx - 1);
    if (lds > 150 * 1024) return fail(c, MSX_ERR_RANGE, "broaden: kernel too long for the LDS tile");
    if ((int)lds > 64 * 1024)
        HIP_TRY(c, hipFuncSetAttribute((const void *)broaden_conv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
    dim3 g((unsigned)((n + kConvTile - 1) / kConvTile), (unsigned)rows);
    hipLaunchKernelGGL(broaden_conv_kernel, g, dim3(256), lds, c->stream, d_in, in_stride, d_tmp, n, n, lx, dx, sigma);
    HIP_TRY(c, hipGetLastError());
    return MSX_OK;
}

// The host-pointer entry points' pinned (device-mapped, coherent) staging of n walkers: the kernel reads theta from, and
// writes its n results to, the buffer itself -- 48 + 12 bytes per walker over PCIe instead of two copy commands (41 -> 38 us
// per 256-walker call, 122 -> 111 us at 2,048).  [cap x MSX_MAX_DIM theta | cap log p | cap status]: *pin grows to cap =
// max(n, 1024) walkers when n does not fit; the statuses follow the n log-probs.
struct PinnedStaging {
    double *theta, *logp;
    int32_t *status;
};
hipError_t pinned_staging(void **pin, int64_t *cap, int64_t n, PinnedStaging *out) {
    if (n > *cap) {
        if (*pin) (void)hipHostFree(*pin);
        *pin = nullptr; *cap = 0;
        const int64_t want = std::max<int64_t>(n, 1024);
        const hipError_t e = hipHostMalloc(pin, (sizeof(double) * (MSX_MAX_DIM + 1) + sizeof(int32_t)) * want, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        *cap = want;
    }
    out->theta = reinterpret_cast<double *>(*pin);
    out->logp = out->theta + *cap * MSX_MAX_DIM;
    out->status = reinterpret_cast<int32_t *>(out->logp + n);
    return hipSuccess;
}

// block_threads as the entry points take it: MSX_BLOCK_512_SHARED is 512 with shared512; nothing else but 0, 256, 512
template <class H>
int decode_block(H *h, int32_t &block_threads, bool &shared512) {
    shared512 = block_threads == MSX_BLOCK_512_SHARED;  // 512 threads, the <= 128-VGPR variant that shares a CU with another workgroup
    if (shared512) block_threads = 512;
    if (block_threads != 0 && block_threads != 256 && block_threads != 512)
        return fail(h, MSX_ERR_INVALID, "block_threads must be 0, 256, 512 or MSX_BLOCK_512_SHARED");
    return MSX_OK;
}

// msx_launch_info's and msx_group_launch_info's answer: out8 = the plan's {form, threads, -, -, dynamic LDS, requested
// bytes, workgroups, walkers per sub-batch} with the kernel's VGPRs and static LDS filled in, and its name
template <class H>
int launch_info_out(H *h, const void *fn, std::array<int64_t, 8> v, const std::string &nm, char *name, int32_t name_len,
                    int64_t *out8) {
    hipFuncAttributes at;
    HIP_TRY(h, hipFuncGetAttributes(&at, fn));
    v[2] = at.numRegs;
    v[3] = (int64_t)at.sharedSizeBytes;
    std::copy(v.begin(), v.end(), out8);
    if (name && name_len > 0) {
        strncpy(name, nm.c_str(), (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    return MSX_OK;
}

// A synchronous entry point has seen the walkers' statuses: MSX_W_HANDOVER anywhere means the linked form's flags are
// no longer trustworthy on this context (the device-side poison word says the same to every later linked launch).
// (The pair form's bounded wait -- a spill row's lease never granted -- reports the same status: the launch is over when a
// synchronous entry point reads it, nobody holds a row, so the leases are cleared for the launches that follow.)
void note_handover(msx_ctx *c, const int32_t *status, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (status[i] == MSX_W_HANDOVER) {
            c->linked_poisoned = true;
            if (c->d_pair_plan) (void)hipMemsetAsync(c->d_pair_plan + kPairHdrInts, 0, sizeof(int32_t) * kPairSpillRows, c->stream);
            return;
        }
}

// ---- the fused form's launch rules, over plain inputs: a context's launch (plan_launch) and a target group's
// (plan_group_launch, over its longest member, the AND of its members' flags and its total walkers) both read them ------

// The workgroup size for n walkers of npix pixels on `cus` CUs.
int pick_block(int64_t cus, int64_t n, int64_t npix) {
    // Measured at 4096 px: up to one walker per CU, 512 threads owning the CU with the pixel statics in
    // LDS; up to 2 per CU, 512 threads sharing the CU two by two (<= 128 VGPRs); beyond, 256 threads three per CU
    // (512 / 1024 / 2048 walkers: 28.3 / 48.2 / 87.8 us shared-512 against 29.2 / 47.2 / 77.6 us with 256 threads).
    // Long spectra (model vector > half the LDS): 512 threads, one workgroup per CU.
    // The choice only affects speed: every variant sums in the same order (see phase A), so a walker's value
    // has the same bits whichever one evaluates it.
    if (npix >= 8192) return 512;
    if (n <= cus) return 512;
    if (npix <= 2048) return 256;  // short spectra (512 walkers x 1194 px: 17.8 us with 256 threads, 20.2 shared-512)
    if (n <= 2 * cus) return 512;
    return 256;
}

// Which variant of `block` threads n walkers of npix pixels want: SH (two workgroups per CU) and / or PF (u and the data
// flux staged in LDS; pf_ok / pf256_ok: its statics fit, at 512 / 256 threads).  shared512: MSX_BLOCK_512_SHARED.
struct FusedShape {
    bool sh = false, pf = false;
};
FusedShape fused_shape(int64_t cus, int64_t n, int64_t npix, int block, bool shared512, bool pf_ok, bool pf256_ok) {
    FusedShape f;
    if (block == 256) {
        // at most two walkers per CU (config 5's 512 x 1194 px): the variant compiled for two workgroups per CU has the
        // registers for quad trips (16.0 against 16.3 us); beyond, three per CU matter more.  With u and the data flux
        // staged in LDS (PF) when two such workgroups still fit a CU.
        f.sh = n <= 2 * cus;
        f.pf = f.sh && pf256_ok;
    } else {
        // PF: 512-thread workgroups that own their CU (long spectra: one per CU anyway) and whose 3 npix doubles fit
        // (256 walkers x 4096 px 16.7-16.9 us against 17.0-17.1 for the <= 128-VGPR variant).  Between one and two
        // walkers per CU, or when asked for: the <= 128-VGPR variant, two workgroups per CU.
        const bool own_cu = n <= cus || sizeof(double) * (size_t)npix > 70 * 1024;
        f.pf = !shared512 && own_cu && pf_ok;
        f.sh = !f.pf && (shared512 || !own_cu);
    }
    return f;
}

// no pad pixels, and npair a whole number of trips of `trip` elements (the fused variants' FULL entries: 2 x threads)
bool whole_trips(const DevProblem &P, int64_t trip) { return P.npix == 2 * P.npair && P.npair % trip == 0; }

// dynamic LDS of a fused variant: the model vector; PF adds u and the data flux in the tables' pair layout
size_t fused_dyn_lds(const DevProblem &P, bool pf) {
    return pf ? sizeof(double) * (size_t)((P.npix + 1) & ~1ll) + 2 * sizeof(double2) * (size_t)P.npair : sizeof(double) * (size_t)P.npix;
}

// bytes a fused variant requests from the memory system per walker
//   blend: 12-B {R f64, H f32} per corner (8-B with the R table in float32) + {k_lo f64, dk f32} + data flux, u (f64) per pixel
//   chi^2 pass: 1/err^2, and -- unless the variant kept them in LDS (PF) -- u and data flux again
int64_t fused_bytes(const DevProblem &P, bool pf, bool r32) {
    const int64_t per_corner = r32 ? 8 : 12;  // {R f64 | f32, H f32}
    return P.npix * (per_corner * (int64_t)P.nspec * 4 + 12 + 16 + (pf ? 8 : 24)) + 8 * (2 * P.nspec + 2) + 12;
}

}  // namespace

// ---- launchers ------------------------------------------------------------------------------------------------
namespace {

struct LaunchArgs {
    const double *theta;
    double *logp;
    int32_t *status;
    int64_t n;
    int32_t ndim, mode;
    hipStream_t s;
    int niso_nt, ng_mode_fast;
};

// The leading, preloaded arguments' packed words (logprob_kernel decodes them; logprob_group_kernel ORs in its launch's mode):
// niso | nt << 16, and ng | mode << 8 | fast << 16 | smp_on << 17 | dist_fit << 18 | use_av << 19; `fast` = the recipe's
// small tables fit the register-resident recipe.
void pack_leading_words(const DevProblem &P, bool fast, int mode, int *niso_nt, int *ng_mode_fast) {
    *niso_nt = (int)(std::min<int64_t>(P.niso, 0xffff) | ((int64_t)std::min<int64_t>(P.nt, 0x7fff) << 16));
    *ng_mode_fast = (int)std::min<int64_t>(P.ng, 0xff) | (mode << 8) | ((fast ? 1 : 0) << 16) | ((P.smp_on ? 1 : 0) << 17) |
                    ((P.dist_fit ? 1 : 0) << 18) | ((P.use_av ? 1 : 0) << 19);
}

// A copy of the staged problem whose per-walker pointers start at walker `off` of the caller's batch (sub-batches)
DevProblem problem_at(const DevProblem &P0, int64_t off, int mode, int ndim) {
    DevProblem P = P0;
    if (off == 0) return P;
    if (P.opt_chain) P.opt_chain += off;
    if (mode == MSX_MODE_OPT_INIT) { P.opt_flux += off * P.npix; P.opt_med += off; }
    if (P.smp_on) {
        P.smp_sidx += off; P.smp_cidx += off; P.smp_partner += off;
        P.smp_zz += off; P.smp_zfac += off; P.smp_logu += off; P.smp_rec += off;
        P.smp_q += off * ndim;
    }
    return P;
}

// ---- the variants of logprob_kernel, as a TABLE: the launcher, msx_launch_info (what bench.py prints as the roofline's
// kernel) and the dynamic-LDS limits all read this one list -- nobody mirrors the choice -------------------------------
struct Variant {
    const void *fn;
    int ns, threads;
    bool gm, sh, pf, lk, r32;
    int full;  // FULL bits of the variant (logprob_kernel.h): 1 blend, 2 chi^2 pass
    bool given;  // model values given (in-path broadening)
    const char *what;
};
template <int NS, int T, bool GM, bool SH, bool PF, bool LK, bool R32 = false, int FULL = 0, bool GIVEN = false>
Variant variant(const char *what) {
    return {(const void *)logprob_kernel<NS, T, GM, SH, PF, LK, R32, FULL, GIVEN>, NS, T, GM, SH, PF, LK, R32, FULL, GIVEN, what};
}
const Variant kVariants[] = {
    //     NS  threads GM     SH     PF     LK     R32    FULL
    variant<2, 256, false, false, false, false>("three workgroups per CU"),
    variant<2, 256, false, true, false, false>("two per CU, four pixels per lane and trip"),
    variant<2, 256, false, true, true, false>("two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    variant<2, 512, false, false, false, false>("one workgroup per CU, four pixels per lane and trip"),
    variant<2, 512, false, true, false, false>("<= 128 VGPRs: two workgroups fit a CU; rows one star at a time"),
    variant<2, 512, false, false, true, false>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    variant<3, 256, false, false, false, false>("three workgroups per CU"),
    variant<3, 512, false, false, false, false>("one workgroup per CU, four pixels per lane and trip"),
    variant<3, 512, false, false, true, false>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    variant<2, 512, false, false, false, true>("one workgroup per walker and 8192-pixel segment; partial sums and histogram counters exchanged inside the launch; the segment's data flux staged in LDS; four pixels per lane and trip"),
    variant<3, 512, false, false, false, true>("one workgroup per walker and 8192-pixel segment; partial sums and histogram counters exchanged inside the launch; the segment's data flux staged in LDS; four pixels per lane and trip"),
    variant<2, 512, true, false, false, false>("model vector in global memory (spectra beyond the LDS), sub-batched"),
    variant<3, 512, true, false, false, false>("model vector in global memory (spectra beyond the LDS), sub-batched"),
    // the fused binary variants once more over the FLOAT32 copy of the R table (msx_set_grid_storage(MSX_STORE_F32))
    variant<2, 256, false, false, false, false, true>("three workgroups per CU; R table stored in float32"),
    variant<2, 256, false, true, false, false, true>("two per CU, four pixels per lane and trip; R table stored in float32"),
    variant<2, 256, false, true, true, false, true>("two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; R table stored in float32"),
    variant<2, 512, false, false, false, false, true>("one workgroup per CU, four pixels per lane and trip; R table stored in float32"),
    variant<2, 512, false, true, false, false, true>("<= 128 VGPRs: two workgroups fit a CU; rows one star at a time; R table stored in float32"),
    variant<2, 512, false, false, true, false, true>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; R table stored in float32"),
    // the binary variants once more for spectra that fill their trips exactly (FULL: no clamps, no validity selects; bit 0
    // in the blend, bit 1 in the chi^2 pass).  Same box, general / FULL, us per batch of 4096 px -- 256 threads, both bits:
    // 512 walkers 24.2 / 23.1, 1,024: 39.5 / 37.8, 2,048: 63.3 / 60.4, 2,304: 68.9 / 66.7.  512 threads, one workgroup per
    // CU (the 256-walker headline), per step: both bits 14.35 -> 14.55 (slower), the blend's alone 14.67 -> 14.96 (slower:
    // without the clamps the scheduler orders the trip's loads differently), the chi^2 pass's alone 14.63 -> 14.36.
    // (The 256-thread bits measured against 1 and 2 as well: profiles/r4_ab_full.txt.)
    variant<2, 256, false, false, false, false, false, 3>("three workgroups per CU; whole trips, no clamps"),
    variant<2, 256, false, true, false, false, false, 3>("two per CU, four pixels per lane and trip; whole trips, no clamps"),
    variant<2, 256, false, true, true, false, false, 3>("two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; whole trips, no clamps"),
    variant<2, 512, false, false, true, false, false, 2>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; whole trips, no clamps in the chi^2 pass"),
    variant<2, 512, false, true, false, false, false, 2>("<= 128 VGPRs: two workgroups fit a CU; rows one star at a time; whole trips, no clamps in the chi^2 pass"),
    variant<2, 512, false, false, true, false, true, 2>("float32-stored grid table R; one workgroup per CU, u / flux staged in LDS; whole trips, no clamps in the chi^2 pass"),
    // the linked form for whole-trip segments: no clamps in the segment's chi^2 pass and candidates' gather
    variant<2, 512, false, false, false, true, false, 2>("linked: one workgroup per walker and 8192-pixel segment; whole trips, no clamps in the chi^2 pass"),
    // in-path broadening (inpath_kernels.h): the model values are given, the blend is compiled out
    variant<2, 512, false, false, false, false, false, 0, true>("model values given by the in-path broadening kernels; four pixels per lane and trip"),
};

// The pair kernel (pair_kernel.h): 512 threads, two workgroups per CU at <= 128 VGPRs: 16 waves per CU (the 256-thread
// variants -- two per CU at 256 VGPRs, 8 waves -- measured 411.8 us against 344.8 at 16,384 walkers and are not built);
// NT element trips per lane, the smallest that covers the spectrum (2 / 4 = up to 2048 / 4096 pixels).  Always the
// variant that loads the extinction terms: a problem staged without extinction -- every walker at redc = 0 -- takes the
// unreddened values from it all the same and pays for the H rows; the variant without them spilled registers at 4096
// pixels and is not built.  FULL: the spectrum fills the variant exactly -- no clamps, no validity selects.
struct PairVariant {
    void (*fn)(const double *, const unsigned char *, int, int, int64_t, double, double, const int32_t *, DevProblem, double *, int32_t *);
    int nt;
    bool full;
};
const PairVariant kPairVariants[] = {
    {logprob_pair_kernel<512, 2, true>, 2, false},
    {logprob_pair_kernel<512, 2, true, true>, 2, true},
    {logprob_pair_kernel<512, 4, true>, 4, false},
    {logprob_pair_kernel<512, 4, true, true>, 4, true},
};

// The entry of kVariants with `want`'s shape (ns, threads, gm, sh, pf, lk, r32, given); its FULL one if it has one and
// the spectrum is whole trips of it (`whole`).  nullptr: the table has no entry of that shape.
const Variant *find_variant(const Variant &want, bool whole) {
    const Variant *hit = nullptr;
    for (const Variant &v : kVariants)
        if (v.ns == want.ns && v.threads == want.threads && v.gm == want.gm && v.sh == want.sh && v.pf == want.pf &&
            v.lk == want.lk && v.r32 == want.r32 && v.given == want.given && (v.full == 0 || whole) && (!hit || v.full != 0))
            hit = &v;
    return hit;
}

// THE launch decision, for the launcher (per sub-batch), msx_launch_info and msx_bytes_per_eval alike: how a launch of n
// walkers in form f with workgroups of block_threads (0: automatic; shared512: MSX_BLOCK_512_SHARED) runs.
struct LaunchPlan {
    int64_t rows = 0;  // walkers per sub-batch of the form
    int64_t m = 0;     // walkers of the first sub-batch: min(n, rows)
    int block = 0;     // the workgroup size asked for (the variant's own may differ: linked, GM, in-path take 512)
    const Variant *v = nullptr;       // the logprob_kernel variant (fused, linked, in-path) ...
    const PairVariant *pv = nullptr;  // ... or the pair kernel's
    const void *fn = nullptr;
    int threads = 0;
    size_t dyn_lds = 0;
    int64_t grid = 0;
    int64_t bytes = 0;  // requested from the memory system per walker (requested_bytes_of)
};


// One launch of the planned logprob_kernel variant over A.n = pl.m walkers.
int launch_logprob(msx_ctx *c, const DevProblem &P, const LaunchArgs &A, const LaunchPlan &pl) {
    // the kernel's arguments, in its own order (the leading 14 dwords arrive preloaded in SGPRs: logprob_kernel)
    const double *a_theta = P.smp_on ? (const double *)P.smp_coords : A.theta;
    const unsigned char *a_rblk = (const unsigned char *)c->d_recipe_block;
    int a_niso_nt = A.niso_nt, a_word = A.ng_mode_fast;
    int64_t a_n = A.n;
    double a_tmin = P.tmin, a_tmax = P.tmax;
    const SmpRec *a_rec = P.smp_rec;
    DevProblem a_P = P;
    double *a_logp = A.logp;
    int32_t *a_status = A.status;
    void *args[] = {&a_theta, &a_rblk, &a_niso_nt, &a_word, &a_n, &a_tmin, &a_tmax, &a_rec, &a_P, &a_logp, &a_status};
    HIP_TRY(c, hipLaunchKernel(pl.fn, dim3((unsigned)pl.grid), dim3((unsigned)pl.threads), args, pl.dyn_lds, A.s));
    return MSX_OK;
}

// The in-path broadening form over A.n <= inp_rows walkers (inpath_kernels.h): recipe -> composite of the raw window rows,
// convolved -> edge patches, reddening, resample -> logprob_kernel<GIVEN>.
int launch_inpath(msx_ctx *c, const DevProblem &P, const LaunchArgs &A, const LaunchPlan &pl) {
    const int64_t m = A.n, nwin = c->raw_n;
    hipLaunchKernelGGL(inpath_recipe_kernel, dim3((unsigned)((m + kPlanThreads - 1) / kPlanThreads)), dim3(kPlanThreads), 0, A.s, A.theta,
                       (const unsigned char *)c->d_recipe_block, A.niso_nt, A.ng_mode_fast, m, P.tmin, P.tmax, c->d_inp_rec, P);
    HIP_TRY(c, hipGetLastError());
    const size_t lds = sizeof(double) * ((size_t)c->raw_lx + ((size_t)(kConvTile + c->raw_lx - 1) * 5) / 4 + 2);
    // (the tile fits: checked, and the kernel's dynamic-LDS limit raised, at msx_stage_problem -- a launch neither allocates nor
    // changes function attributes, so that it can be captured like the others)
    hipLaunchKernelGGL(inpath_conv_kernel, dim3((unsigned)((nwin + kConvTile - 1) / kConvTile), (unsigned)m), dim3(256), lds, A.s,
                       c->d_raw_win, nwin, c->d_inp_rec, c->d_inp_tmp, nwin, nwin, c->raw_lx, c->raw_dx, c->raw_sigma);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(inpath_resample_kernel, dim3((unsigned)((c->inp_gstride + 255) / 256), (unsigned)m), dim3(256), 0, A.s, c->d_inp_tmp,
                       nwin, nwin, c->raw_i0, c->d_inp_rec, c->d_pix_lo, P.pix_t, c->d_kgrid, (int64_t)P.npix, c->d_inp_given, c->inp_gstride);
    HIP_TRY(c, hipGetLastError());
    DevProblem Pg = P;
    Pg.given = c->d_inp_given;
    Pg.given_stride = c->inp_gstride;
    return launch_logprob(c, Pg, A, pl);
}

// Does MSX_PATH_AUTO take the linked form for n walkers (of a problem and mode that have one)?  While every workgroup
// gets a CU of its own: the walker's workgroups wait for each other.
bool auto_takes_linked(const msx_ctx *c, int64_t n) {
    const int64_t cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
    return c->d_seg_flag != nullptr && c->recipe_fast && !c->P.no_spectrum && !c->linked_poisoned && c->linked != 0 &&
           c->path != MSX_PATH_FUSED && c->path != MSX_PATH_PAIR && (c->linked > 0 || c->path == MSX_PATH_LINKED || n * c->nseg <= cus);
}

// Does MSX_PATH_AUTO take the pair form for the next large batch?  A walker the planner cannot pair costs the pair kernel
// a whole workgroup (two per CU: 0.042 us per item at 16,384 walkers) where the fused kernel runs three per CU (0.027 us
// per walker), so pairing pays while singles < 0.75 pairs -- an ensemble in a handful of grid cells, the normal state of
// a chain -- and does not for one spread over the grid (burn-in from a wide start: 16,384 walkers 521 us against 440).
// The evidence is the planner's count of its last run, which the device leaves in host memory; it is read without
// synchronising, so it may lag.  While it says "spread" the fused kernel runs, and every 32nd qualifying launch goes
// through the pair form anyway to look again.  (The choice is frozen into a captured hipGraph like any launch
// parameter.)  Values never depend on it.
bool pair_worth_it(msx_ctx *c, bool peek = false) {
    const int32_t np = ((volatile int32_t *)c->h_pair_stats)[0], ns = ((volatile int32_t *)c->h_pair_stats)[1];
    const bool pays = 4 * (int64_t)ns < 3 * (int64_t)np;
    if (peek) return pays;  // (msx_launch_info: what the next launch would take, without counting as one)
    return pays || (++c->pair_auto_launches % 32) == 0;
}

// Which FORM of the path a launch of n walkers in `mode` takes (msx_logprob_batch_dev decides with this; msx_launch_info
// and msx_bytes_per_eval ask with peek = true).  err != MSX_OK: an explicit msx_set_path that the staged problem cannot take.
struct FormChoice {
    bool linked = false, pair = false, inpath = false;
    int err = MSX_OK;
    const char *msg = "";
};
FormChoice decide_form(msx_ctx *c, int64_t n, int mode, bool peek) {
    FormChoice f;
    const DevProblem &Pc = c->P;
    const bool fast = c->recipe_fast;
    const bool lp_mode = mode == MSX_MODE_LOGLIKE || mode == MSX_MODE_LOGPOST || mode == MSX_MODE_CHISQ;
    // linked (logprob_kernel<..., LK>): few walkers x long spectrum -- one workgroup per (walker, 8192-pixel segment); the
    // walker's workgroups exchange their segments' partial sums and counters inside the kernel and each makes the chi^2 /
    // median pass over its own segment, so a launch of <= #CUs / segments walkers uses segments x as many CUs and every
    // workgroup's chain of latencies is 8192 pixels long.  Only the likelihood / posterior / chi^2 modes of a problem
    // with a spectrum term and the register-resident recipe.  MSX_PATH_AUTO takes it while walkers x segments <= #CUs
    // (one workgroup per CU: they wait for each other).  MSX_LINKED=0 / 1 in the environment: never / whenever possible.
    // A context on which a meeting has once timed out is POISONED until the problem is staged again: AUTO takes the
    // fused form, an explicit MSX_PATH_LINKED is refused (and the kernel itself fails every walker, for callers of
    // the device entry point who never looked at the statuses).
    const bool can_link = c->d_seg_flag != nullptr && fast && !Pc.no_spectrum && lp_mode;
    f.linked = can_link && auto_takes_linked(c, n) && !c->smp_overlap_launch;
    if (c->path == MSX_PATH_LINKED) {
        if (!can_link) { f.err = MSX_ERR_STATE; f.msg = "msx_set_path(LINKED): needs a spectrum of 2..8 segments of 8192 pixels, the register-resident recipe and a likelihood / posterior / chi^2 mode"; return f; }
        if (c->linked_poisoned) { f.err = MSX_ERR_STATE; f.msg = "msx_set_path(LINKED): a hand-over timed out on this context (MSX_W_HANDOVER); stage the problem again"; return f; }
        f.linked = true;
    }
    // pair (pair_kernel.h): many walkers -- two walkers of one grid cell per workgroup share one set of row loads
    const bool can_pair = c->pair_rows > 0 && fast && !Pc.smp_on && Pc.nspec == 2 && lp_mode;
    f.pair = can_pair && n >= c->pair_min_walkers && pair_worth_it(c, peek);
    if (c->path == MSX_PATH_FUSED || c->path == MSX_PATH_LINKED) f.pair = false;
    if (c->path == MSX_PATH_PAIR) {
        if (!can_pair) { f.err = MSX_ERR_STATE; f.msg = "msx_set_path(PAIR): needs a binary of <= 4096 pixels, the register-resident recipe and a likelihood / posterior / chi^2 mode"; return f; }
        f.pair = true;
    }
    if (c->probe_launch) f.pair = false;  // (the pair form carries no clock stamps)
    if (c->store_f32) {  // float32-stored R table: the fused variants compiled for it, nothing else
        if (c->path == MSX_PATH_PAIR || c->path == MSX_PATH_LINKED) { f.err = MSX_ERR_STATE; f.msg = "float32 grid storage (msx_set_grid_storage): the fused form only"; return f; }
        f.pair = false; f.linked = false;
    }
    if (f.pair) f.linked = false;
    // in-path broadening (inpath_kernels.h): never taken by MSX_PATH_AUTO -- the per-node placement is the reference's
    if (c->path == MSX_PATH_INPATH) {
        if (c->ncomp > 1) {
            f.err = MSX_ERR_STATE;
            f.msg = "msx_set_path(INPATH): the grid holds one copy per component (msx_split_components); the per-walker form reads one raw window and would not match it";
            return f;
        }
        if (c->inp_rows <= 0 && c->grid_rotated) {
            f.err = MSX_ERR_STATE;
            f.msg = "msx_set_path(INPATH): the grid was rotationally broadened (msx_rot_broaden_grid); the per-walker form applies the Gaussian only and would not match it";
            return f;
        }
        if (c->inp_rows <= 0 || !fast || Pc.smp_on || !lp_mode || c->store_f32 || c->probe_launch) {
            f.err = MSX_ERR_STATE;
            f.msg = "msx_set_path(INPATH): needs msx_set_broadening(MSX_BROADEN_IN_PATH) before msx_broaden_grid, a binary whose data pixels lie inside that window, float64 tables, the register-resident recipe and a likelihood / posterior / chi^2 mode";
            return f;
        }
        f.inpath = true; f.pair = false; f.linked = false;
    }
    return f;
}

// bytes the form / variant a launch takes requests from the memory system, per walker
int64_t requested_bytes_of(const msx_ctx *c, const FormChoice &f, const Variant *v) {
    const int64_t npix = c->P.npix;
    // the pair form: two walkers per set of loads -- rows, extinction terms, the fit sweep's data flux / u, the pass's three
    // vectors -- + the planner's record
    if (f.pair) return npix * (12 * 8 + 12 + 16 + 24) / 2 + (int64_t)sizeof(PairRec) + 8 * 6 + 12;
    int64_t b = fused_bytes(c->P, v && v->pf, v && v->r32);
    // the linked form: every segment's workgroup reads theta and writes its partials (counters, sums, range; chi^2 sum
    // and candidates: <= 64 of them as a rule), reads the other segments' partials, and one of them their candidates
    if (f.linked) {
        const int64_t S = c->nseg, part = 4 * kSegBins + 64, fin = 16 + 8 * 64;
        b += (S - 1) * (8 * (2 * c->P.nspec + 2)) + S * (part + fin) + S * (S - 1) * part + (S - 1) * fin;
    }
    return b;
}

LaunchPlan plan_launch(const msx_ctx *c, const FormChoice &f, int64_t n, int block_threads, bool shared512) {
    const DevProblem &P = c->P;
    const int64_t cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
    LaunchPlan pl;
    // sub-batches: the in-path form's rows, the pair form's item lists, and the scratch of the linked form and of the
    // fused kernel's global model vectors (spectra beyond the LDS)
    pl.rows = f.inpath ? c->inp_rows : f.pair ? c->pair_rows : (f.linked || c->model_in_global) ? c->scratch_rows : n;
    pl.m = std::min(n, pl.rows);
    const int64_t m = pl.m;
    pl.block = (f.linked || f.inpath) ? 512 : block_threads > 0 ? block_threads : pick_block(cus, m, P.npix);
    if (f.pair) {
        // a trip of the pair kernel is NT x 512 elements
        const int nt = P.npair <= 2 * 512 ? 2 : 4;
        for (const PairVariant &pv : kPairVariants)
            if (pv.nt == nt && pv.full == whole_trips(P, nt * 512)) pl.pv = &pv;
        pl.fn = pl.pv ? (const void *)pl.pv->fn : nullptr;
        pl.threads = 512;
        pl.grid = m;
        pl.bytes = requested_bytes_of(c, f, nullptr);
        return pl;
    }
    // 1. the shape the launch wants
    const int B = pl.block;
    Variant want = {};
    want.ns = P.nspec == 2 ? 2 : 3;
    want.threads = 512;
    want.lk = f.linked;       // one workgroup per walker and segment
    want.given = f.inpath;    // model values given by the in-path kernels
    want.gm = !f.linked && !f.inpath && c->model_in_global;  // spectra longer than the LDS: the model vector in global scratch
    want.r32 = c->store_f32;  // (msx_stage_problem has checked that the problem has such variants: fused binaries)
    if (!want.lk && !want.given && !want.gm) {
        want.threads = B;
        const FusedShape fs = fused_shape(cus, m, P.npix, B, shared512, c->pf_ok, c->pf256_ok);
        want.sh = fs.sh;
        want.pf = fs.pf;
    }
    // 2. its entry of the table -- triples have no SH variant (twelve corners do not fit its 128 VGPRs) and take the plain
    //    one; the FULL entry when the spectrum is whole trips of 2 x threads elements
    const bool whole = whole_trips(P, 2 * (int64_t)want.threads);
    pl.v = find_variant(want, whole);
    if (!pl.v) {
        want.sh = want.pf = false;
        pl.v = find_variant(want, whole);
    }
    if (!pl.v) return pl;
    pl.fn = pl.v->fn;
    pl.threads = pl.v->threads;
    // dynamic LDS: the fused variants' (linked: one segment of the model vector, and the segment's data flux behind it)
    pl.dyn_lds = pl.v->lk ? sizeof(double) * (size_t)(2 * kSegElems) + sizeof(double2) * (size_t)kSegElems
                 : pl.v->gm ? 0
                 : fused_dyn_lds(P, pl.v->pf);
    // (linked: block = (walker / 8) * 8 segments + segment * 8 + walker % 8, see the kernel)
    pl.grid = pl.v->lk ? ((m + 7) & ~7ll) * c->nseg : m;
    pl.bytes = requested_bytes_of(c, f, pl.v);
    return pl;
}

// ---- target groups (group_kernel.h): the instances of logprob_group_kernel, in a table of their own -- the fused
// entries of kVariants that a group can take (no GM, linked, in-path or float32 storage) -- except the three-per-CU
// FULL one, which as a group instance spilled 36 bytes per lane to scratch: whole-trip members take the plain entry there
// (same bits) ----------------------------------------------------------------------------------------------------------
struct GroupVariant {
    const void *fn;
    const void *smp_fn;  // the same entry as a half-step of the group's device-resident sampler (SMP)
    int ns, threads;
    bool sh, pf;
    int full;
    const char *what;
};
// SMP = false: no sampler instance of this entry -- as one it spilled 36 bytes per lane to scratch (the sampler's scalars
// on top of the member lookup's); the group's sampler takes a neighbour there (group_smp_variant, same bits)
template <int NS, int T, bool SH, bool PF, int FULL = 0, bool SMP = true>
GroupVariant group_variant(const char *what) {
    const void *smp = nullptr;
    if constexpr (SMP) smp = (const void *)logprob_group_kernel<NS, T, SH, PF, FULL, true>;
    return {(const void *)logprob_group_kernel<NS, T, SH, PF, FULL>, smp, NS, T, SH, PF, FULL, what};
}
const GroupVariant kGroupVariants[] = {
    //           NS  threads SH     PF    FULL
    group_variant<2, 256, false, false>("three workgroups per CU"),
    group_variant<2, 256, true, false>("two per CU, four pixels per lane and trip"),
    group_variant<2, 256, true, true, 0, false>("two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    group_variant<2, 512, false, false>("one workgroup per CU, four pixels per lane and trip"),
    group_variant<2, 512, true, false, 0, false>("<= 128 VGPRs: two workgroups fit a CU; rows one star at a time"),
    group_variant<2, 512, false, true>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    group_variant<3, 256, false, false>("three workgroups per CU"),
    group_variant<3, 512, false, false>("one workgroup per CU, four pixels per lane and trip"),
    group_variant<3, 512, false, true>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip"),
    group_variant<2, 256, true, false, 3>("two per CU, four pixels per lane and trip; whole trips, no clamps"),
    group_variant<2, 256, true, true, 3>("two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; whole trips, no clamps"),
    group_variant<2, 512, false, true, 2>("one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip; whole trips, no clamps in the chi^2 pass"),
    group_variant<2, 512, true, false, 2, false>("<= 128 VGPRs: two workgroups fit a CU; rows one star at a time; whole trips, no clamps in the chi^2 pass"),
};

struct GroupPlan {
    const GroupVariant *v = nullptr;
    size_t dyn_lds = 0;
    int64_t bytes = 0;  // requested from the memory system per walker, averaged over the launch's walkers
};

// plan_launch's rules for the fused form (fused_shape, whole_trips), applied to the launch's walkers and its longest member,
// restricted to the entries every member with walkers can take: FULL only if every one of them is whole trips of it, PF
// only if every one's statics fit (pf_ok / pf256_ok).  counts[m] = member m's walkers; total = their sum (> 0).
GroupPlan group_plan_lds(const msx_group *g, const int64_t *counts, int64_t total, const GroupVariant *v);
GroupPlan plan_group_launch(const msx_group *g, const int64_t *counts, int64_t total, int block_threads, bool shared512) {
    const int k = (int)g->members.size();
    int64_t npix = 0;
    bool pf = true, pf256 = true;
    for (int m = 0; m < k; ++m)
        if (counts[m] > 0) {
            npix = std::max<int64_t>(npix, g->probs[m].npix);
            pf = pf && g->pf_ok[m];
            pf256 = pf256 && g->pf256_ok[m];
        }
    const int B = block_threads > 0 ? block_threads : pick_block(g->cus, total, npix);
    bool whole = true;
    for (int m = 0; m < k; ++m)
        if (counts[m] > 0) whole = whole && whole_trips(g->probs[m], 2 * (int64_t)B);
    FusedShape want = fused_shape(g->cus, total, npix, B, shared512, pf, pf256);
    const int ns = g->nspec == 2 ? 2 : 3;
    const GroupVariant *hit = nullptr;
    for (int attempt = 0; attempt < 2 && !hit; ++attempt) {
        if (attempt == 1) want.sh = want.pf = false;  // triples have no SH variant
        for (const GroupVariant &v : kGroupVariants)
            if (v.ns == ns && v.threads == B && v.sh == want.sh && v.pf == want.pf && (v.full == 0 || whole) && (!hit || v.full != 0))
                hit = &v;
    }
    return hit ? group_plan_lds(g, counts, total, hit) : GroupPlan();
}

// the plan's dynamic LDS (the largest member's) and bytes (averaged over the walkers) for entry v
GroupPlan group_plan_lds(const msx_group *g, const int64_t *counts, int64_t total, const GroupVariant *v) {
    GroupPlan pl;
    pl.v = v;
    double bytes = 0.0;
    for (int m = 0; m < (int)g->members.size(); ++m) {
        if (counts[m] <= 0) continue;
        pl.dyn_lds = std::max(pl.dyn_lds, fused_dyn_lds(g->probs[m], v->pf));
        bytes += (double)fused_bytes(g->probs[m], v->pf, false) * (double)counts[m];
    }
    pl.bytes = (int64_t)(bytes / (double)total + 0.5);
    return pl;
}

// The pair form over A.n walkers (pair_kernel.h), in the planned variant.
int launch_pair(msx_ctx *c, const DevProblem &P, const LaunchArgs &A, const LaunchPlan &pl) {
    // 1. the planner: every walker's recipe (one thread per walker), final values of the rejected / failed ones, and
    //    who shares a workgroup
    const int32_t *plan = c->d_pair_plan;
    hipLaunchKernelGGL(pair_plan_kernel, dim3((unsigned)((A.n + kPlanThreads - 1) / kPlanThreads)), dim3(kPlanThreads), 0, A.s, A.theta,
                       (const unsigned char *)c->d_recipe_block, A.niso_nt, A.ng_mode_fast, (int64_t)A.n, P.tmin, P.tmax,
                       c->d_pair_plan, c->d_pair_items, c->d_pair_singles, A.logp, A.status, c->h_pair_stats, P);
    HIP_TRY(c, hipGetLastError());
    // 2. the planner's items: singles + pairs <= n workgroups; those beyond the planner's count leave after one load
    hipLaunchKernelGGL(pl.pv->fn, dim3((unsigned)pl.grid), dim3((unsigned)pl.threads), 0, A.s, A.theta, (const unsigned char *)c->d_recipe_block,
                       A.niso_nt, A.ng_mode_fast, (int64_t)A.n, P.tmin, P.tmax, plan, P, A.logp, A.status);
    HIP_TRY(c, hipGetLastError());
    return MSX_OK;
}

// Every variant that takes dynamic LDS may be launched with up to the CU's 160 KiB minus its own static LDS.
// The limit is a property of the FUNCTION in this process, not of a context: it is raised once, to the maximum,
// so that contexts staged with different spectrum lengths can never lower it under one another.
hipError_t raise_one(const void *kernel) {
    hipFuncAttributes at;
    hipError_t e = hipFuncGetAttributes(&at, kernel);
    if (e != hipSuccess) return e;
    const int room = (160 * 1024 - (int)at.sharedSizeBytes) & ~15;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, room);
}
hipError_t raise_all() {
    hipError_t e = hipSuccess;
    for (const Variant &v : kVariants)
        if (e == hipSuccess && !v.gm) e = raise_one(v.fn);
    for (const GroupVariant &v : kGroupVariants) {
        if (e == hipSuccess) e = raise_one(v.fn);
        if (e == hipSuccess && v.smp_fn) e = raise_one(v.smp_fn);
    }
    if (e == hipSuccess) e = raise_one((const void *)broaden_conv_kernel);
    if (e == hipSuccess) e = raise_one((const void *)rot_broaden_kernel<true>);
    return e;
}
constexpr int kMaxDevices = 64;
int raise_dynamic_lds_limits(msx_ctx *c) {
    // once per device and process; contexts may be created and staged from several host threads
    static std::mutex mu;
    static bool done[kMaxDevices] = {};
    if (c->device < 0 || c->device >= kMaxDevices)
        return fail(c, MSX_ERR_INVALID, "device index beyond the per-device table of dynamic-LDS limits (64 devices)");
    std::lock_guard<std::mutex> lock(mu);
    if (done[c->device]) return MSX_OK;
    HIP_TRY(c, raise_all());
    done[c->device] = true;
    return MSX_OK;
}

// pyasl.rotBroad's checks and constants for the slice wl[0..n): MSX_ERR_RANGE on a bad v sin i / limb (or an axis the
// kernel cannot take); vc = vsini / c, binnu = int(floor(vc * max(wl) / dwl)) + 1
int rot_params(msx_ctx *c, const double *wl, int64_t n, double vsini, double limb, double *vc, int *binnu) {
    if (!isfinite(vsini) || !isfinite(limb))
        return fail(c, MSX_ERR_RANGE, "rotational broadening: vsini and limb must be finite");
    if (vsini <= 0.0) return fail(c, MSX_ERR_RANGE, "rotational broadening: vsini must be positive.");
    if (limb < 0.0 || limb > 1.0)
        return fail(c, MSX_ERR_RANGE, "rotational broadening: Linear limb-darkening coefficient, epsilon, should be '0 < epsilon < 1'.");
    int rc = check_even_spacing(c, wl, n);
    if (rc) return rc;
    const double dwl = wl[1] - wl[0];
    if (!(dwl > 0.0) || !(wl[0] > 0.0))
        return fail(c, MSX_ERR_RANGE, "rotational broadening: needs an ascending axis of positive wavelengths");
    *vc = vsini / 299792.458;
    const double b = floor((*vc * wl[n - 1]) / dwl);
    if (!(b < (double)kRotMaxBinnu))
        return fail(c, MSX_ERR_RANGE, "rotational broadening: vsini too large for this axis (more than 2^19 samples of halo)");
    *binnu = (int)b + 1;
    return MSX_OK;
}

// rot_broaden_kernel over `rows` rows of n samples (out of place): the LDS-staged form while the tile's span fits
int launch_rot(msx_ctx *c, const double *d_in, int64_t in_stride, const double *d_wl, int64_t n, int64_t rows, double dwl,
               double vc, double eps, int binnu, double *d_out, int64_t out_stride) {
    int rc = raise_dynamic_lds_limits(c);
    if (rc) return rc;
    const dim3 g((unsigned)((n + kRotTile - 1) / kRotTile), (unsigned)((rows + kRotRows - 1) / kRotRows));
    const size_t lds = rot_lds_bytes(binnu);
    if (lds <= (size_t)(160 * 1024))
        hipLaunchKernelGGL(rot_broaden_kernel<true>, g, dim3(kRotTile), lds, c->stream, d_in, in_stride, d_wl, n, rows, dwl, vc,
                           eps, binnu, d_out, out_stride);
    else
        hipLaunchKernelGGL(rot_broaden_kernel<false>, g, dim3(kRotTile), 0, c->stream, d_in, in_stride, d_wl, n, rows, dwl, vc,
                           eps, binnu, d_out, out_stride);
    HIP_TRY(c, hipGetLastError());
    return MSX_OK;
}

// msx_rot_broaden_grid over copies [comp0, comp0 + ncopy) of the staged rows (`who` names the entry in the messages)
int rot_grid_rows(msx_ctx *c, int comp0, int ncopy, int64_t i0, int64_t n, double vsini, double limb, const char *who) {
    if (!c->grid_staged) return fail(c, MSX_ERR_STATE, std::string(who) + ": no grid staged");
    if (i0 < 0 || n < 2 || i0 + n > c->nwl) return fail(c, MSX_ERR_INVALID, std::string(who) + ": bad window");
    HIP_TRY(c, hipSetDevice(c->device));
    const double *wl = c->h_wl.data() + i0;
    double vc;
    int binnu;
    int rc = rot_params(c, wl, n, vsini, limb, &vc, &binnu);
    if (rc) return rc;
    const int64_t rows = (int64_t)ncopy * c->nt * c->ng;
    double *const g0 = c->d_grid + (int64_t)comp0 * c->nt * c->ng * c->nwl;
    double *d_tmp = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_tmp, sizeof(double) * rows * n));
    rc = launch_rot(c, g0 + i0, c->nwl, c->d_wl + i0, n, rows, wl[1] - wl[0], vc, limb, binnu, d_tmp, n);
    if (rc == MSX_OK) {
        hipError_t e = hipMemcpy2DAsync(g0 + i0, sizeof(double) * c->nwl, d_tmp, sizeof(double) * n, sizeof(double) * n,
                                        (size_t)rows, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d_tmp);
    // the raw window of the in-path form is the unrotated grid: the per-walker Gaussian would no longer match the grid
    if (c->d_raw_win) { (void)hipFree(c->d_raw_win); c->d_raw_win = nullptr; c->raw_n = 0; }
    c->grid_rotated = true;
    // any staged problem (R/H and band tables) was derived from the unrotated grid
    free_problem(c);
    return rc;
}

}  // namespace

extern "C" {

int msx_create(int device, msx_ctx **out) {
    if (!out) return MSX_ERR_INVALID;
    *out = nullptr;
    msx_ctx *c = new msx_ctx();
    c->device = device;
    memset(&c->P, 0, sizeof(c->P));
    if (const char *e = getenv("MSX_LINKED")) c->linked = e[0] == '1' ? 1 : 0;
    *out = c;  // returned even on failure so the caller can read msx_last_error
    HIP_TRY(c, hipSetDevice(device));
    HIP_TRY(c, hipGetDeviceProperties(&c->prop, device));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(c, hipMalloc((void **)&c->d_misc, 4096));
    return MSX_OK;
}

void msx_destroy(msx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    sampler_free(c);
    free_problem(c);
    free_grid(c);
    void *ptrs[] = {c->d_misc, c->d_spec, c->d_opt_flux, c->d_opt_med, c->d_opt_chain};
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (c->rccl_comm && rccl().ok) (void)rccl().CommDestroy(c->rccl_comm);
    for (msx_ctx *p : c->loop_peers)  // a loopback group ends with its first member
        if (p != c) { p->loop_peers.clear(); p->comm_world = 0; p->comm_rank = 0; }
    for (msx_group *g : c->groups)  // target groups outlive their members: the slot is cleared, the group refuses it
        for (msx_ctx *&m : g->members)
            if (m == c) m = nullptr;
    if (c->loop_eval_done) (void)hipEventDestroy(c->loop_eval_done);
    if (c->loop_copied) (void)hipEventDestroy(c->loop_copied);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
    for (hipEvent_t e : c->ev_done)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *msx_last_error(msx_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

int msx_device_info(msx_ctx *c, int64_t *out3, char *name, int name_len) {
    if (!c || !out3) return MSX_ERR_INVALID;
    out3[0] = c->prop.multiProcessorCount;
    out3[1] = (int64_t)c->prop.totalGlobalMem;
    out3[2] = c->prop.clockRate;
    if (name && name_len > 0) {
        strncpy(name, c->prop.name, name_len - 1);
        name[name_len - 1] = 0;
    }
    return MSX_OK;
}

int msx_stage_grid(msx_ctx *c, const double *wl, int64_t nwl, const double *teff_nodes, int32_t nt,
                   const double *logg_nodes, int32_t ng, const double *flux, const uint8_t *present) {
    return msx_stage_grid_components(c, wl, nwl, teff_nodes, nt, logg_nodes, ng, flux, present, 1);
}

int msx_stage_grid_components(msx_ctx *c, const double *wl, int64_t nwl, const double *teff_nodes, int32_t nt,
                              const double *logg_nodes, int32_t ng, const double *flux, const uint8_t *present,
                              int32_t ncomp) {
    if (!c || !wl || !teff_nodes || !logg_nodes || !flux || nwl < 2 || nt < 1 || ng < 1)
        return fail(c, MSX_ERR_INVALID, "msx_stage_grid: bad arguments");
    if (ncomp < 1 || ncomp > MSX_MAX_SPEC)
        return fail(c, MSX_ERR_RANGE, "msx_stage_grid_components: ncomp must be 1, 2 or 3 (one copy per component, at most MSX_MAX_SPEC)");
    HIP_TRY(c, hipSetDevice(c->device));
    free_problem(c);
    free_grid(c);
    const int64_t nn = (int64_t)nt * ng;
    c->nwl = nwl; c->nt = nt; c->ng = ng;
    c->h_wl.assign(wl, wl + nwl);
    c->h_teff.assign(teff_nodes, teff_nodes + nt);
    c->h_logg.assign(logg_nodes, logg_nodes + ng);
    HIP_TRY(c, hipMalloc((void **)&c->d_grid, sizeof(double) * ncomp * nn * nwl));
    HIP_TRY(c, hipMemcpy(c->d_grid, flux, sizeof(double) * ncomp * nn * nwl, hipMemcpyHostToDevice));
    c->ncomp = ncomp;
    int rc;
    if ((rc = dev_alloc_copy(c, nullptr, wl, nwl, &c->d_wl))) return rc;
    if ((rc = dev_alloc_copy(c, nullptr, teff_nodes, (int64_t)nt, &c->d_teff))) return rc;
    if ((rc = dev_alloc_copy(c, nullptr, logg_nodes, (int64_t)ng, &c->d_logg))) return rc;
    std::vector<uint8_t> pres(nn, 1);
    if (present) pres.assign(present, present + nn);
    if ((rc = dev_alloc_copy(c, nullptr, pres.data(), nn, &c->d_present))) return rc;
    HIP_TRY(c, hipMalloc((void **)&c->d_kgrid, sizeof(double) * nwl));
    hipLaunchKernelGGL(ccm89_kernel, dim3((unsigned)((nwl + 255) / 256)), dim3(256), 0, c->stream, c->d_wl, nwl, 3.1,
                       c->d_kgrid);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->grid_staged = true;
    return MSX_OK;
}

int msx_ccm89_k(msx_ctx *c, const double *wl, int64_t n, double rv, double *out) {
    if (!c || !wl || !out || n < 0) return fail(c, MSX_ERR_INVALID, "msx_ccm89_k: bad arguments");
    if (n == 0) return MSX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_in, sizeof(double) * n));
    HIP_TRY(c, hipMalloc((void **)&d_out, sizeof(double) * n));
    HIP_TRY(c, hipMemcpy(d_in, wl, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ccm89_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, rv, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return MSX_OK;
}

int msx_resample_linear(msx_ctx *c, const double *x, const double *y, int64_t n, const double *xq, int64_t m,
                        double *out) {
    if (!c || !x || !y || !xq || !out || n < 2 || m < 0) return fail(c, MSX_ERR_INVALID, "msx_resample_linear: bad arguments");
    if (m == 0) return MSX_OK;
    for (int64_t i = 1; i < n; ++i)
        if (!(x[i] >= x[i - 1])) return fail(c, MSX_ERR_INVALID, "msx_resample_linear: x must be sorted ascending");
    double qmin = INFINITY, qmax = -INFINITY;
    for (int64_t i = 0; i < m; ++i) { qmin = xq[i] < qmin ? xq[i] : qmin; qmax = xq[i] > qmax ? xq[i] : qmax; }
    if (qmin < x[0]) return fail(c, MSX_ERR_RANGE, "A value in x_new is below the interpolation range's minimum value.");
    if (qmax > x[n - 1]) return fail(c, MSX_ERR_RANGE, "A value in x_new is above the interpolation range's maximum value.");
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_x = nullptr, *d_y = nullptr, *d_q = nullptr, *d_o = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_x, sizeof(double) * n));
    HIP_TRY(c, hipMalloc((void **)&d_y, sizeof(double) * n));
    HIP_TRY(c, hipMalloc((void **)&d_q, sizeof(double) * m));
    HIP_TRY(c, hipMalloc((void **)&d_o, sizeof(double) * m));
    hipError_t e = hipMemcpy(d_x, x, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_y, y, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_q, xq, sizeof(double) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, d_x, d_y, n, d_q, m, d_o);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_o, sizeof(double) * m, hipMemcpyDeviceToHost);
    (void)hipFree(d_x); (void)hipFree(d_y); (void)hipFree(d_q); (void)hipFree(d_o);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    return MSX_OK;
}

int msx_broaden(msx_ctx *c, const double *wl, const double *flux, int64_t n, double resolution, double maxsig,
                double *out) {
    if (!c || !wl || !flux || !out || n < 16 || !(resolution > 0) || !(maxsig > 0))
        return fail(c, MSX_ERR_INVALID, "msx_broaden: bad arguments (need n >= 16)");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = check_even_spacing(c, wl, n);
    if (rc) return rc;
    double mean = 0.0;
    for (int64_t i = 0; i < n; ++i) mean += wl[i];
    mean /= (double)n;
    double sigma;
    int lx;
    conv_taps(mean, wl[1] - wl[0], resolution, maxsig, &sigma, &lx);
    if (lx < 1) return fail(c, MSX_ERR_RANGE, "msx_broaden: empty kernel");
    double *d_in = nullptr, *d_tmp = nullptr, *d_out = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_in, sizeof(double) * n));
    HIP_TRY(c, hipMalloc((void **)&d_tmp, sizeof(double) * n));
    HIP_TRY(c, hipMalloc((void **)&d_out, sizeof(double) * n));
    HIP_TRY(c, hipMemcpy(d_in, flux, sizeof(double) * n, hipMemcpyHostToDevice));
    rc = launch_conv(c, d_in, n, d_tmp, 1, n, lx, wl[1] - wl[0], sigma);
    if (rc == MSX_OK) {
        hipLaunchKernelGGL(broaden_patch_kernel, dim3((unsigned)((n + 255) / 256), 1), dim3(256), 0, c->stream, d_tmp, n,
                           d_out, n, n);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d_in);
    (void)hipFree(d_tmp);
    (void)hipFree(d_out);
    return rc;
}

int msx_broaden_grid(msx_ctx *c, int64_t i0, int64_t n, double resolution, double maxsig) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->grid_staged) return fail(c, MSX_ERR_STATE, "msx_broaden_grid: no grid staged");
    if (i0 < 0 || n < 16 || i0 + n > c->nwl || !(resolution > 0) || !(maxsig > 0))
        return fail(c, MSX_ERR_INVALID, "msx_broaden_grid: bad window");
    HIP_TRY(c, hipSetDevice(c->device));
    const double *wl = c->h_wl.data() + i0;
    int rc = check_even_spacing(c, wl, n);
    if (rc) return rc;
    double mean = 0.0;
    for (int64_t i = 0; i < n; ++i) mean += wl[i];
    mean /= (double)n;
    double sigma;
    int lx;
    conv_taps(mean, wl[1] - wl[0], resolution, maxsig, &sigma, &lx);
    const int64_t rows = grid_rows(c);
    // in-path placement (msx_set_broadening): the window's rows as they are NOW are kept for the per-walker form; the grid
    // is broadened in place all the same, so that every other form -- and the band tables -- see the reference's live path
    if (c->d_raw_win) { (void)hipFree(c->d_raw_win); c->d_raw_win = nullptr; c->raw_n = 0; }
    c->grid_rotated = false;
    if (c->broaden_placement == MSX_BROADEN_IN_PATH) {
        HIP_TRY(c, hipMalloc((void **)&c->d_raw_win, sizeof(double) * rows * n));
        HIP_TRY(c, hipMemcpy2D(c->d_raw_win, sizeof(double) * n, c->d_grid + i0, sizeof(double) * c->nwl, sizeof(double) * n, (size_t)rows,
                               hipMemcpyDeviceToDevice));
        c->raw_i0 = i0; c->raw_n = n; c->raw_lx = lx; c->raw_dx = wl[1] - wl[0]; c->raw_sigma = sigma;
    }
    double *d_tmp = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_tmp, sizeof(double) * rows * n));
    rc = launch_conv(c, c->d_grid + i0, c->nwl, d_tmp, rows, n, lx, wl[1] - wl[0], sigma);
    if (rc == MSX_OK) {
        hipLaunchKernelGGL(broaden_patch_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0,
                           c->stream, d_tmp, n, c->d_grid + i0, c->nwl, n);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d_tmp);
    // any staged problem was derived from the pre-broadening grid
    free_problem(c);
    return rc;
}

int msx_rot_broaden(msx_ctx *c, const double *wl, const double *flux, int64_t n, double vsini, double limb, double *out) {
    if (!c || !wl || !flux || !out || n < 2) return fail(c, MSX_ERR_INVALID, "msx_rot_broaden: bad arguments (need n >= 2)");
    HIP_TRY(c, hipSetDevice(c->device));
    double vc;
    int binnu;
    int rc = rot_params(c, wl, n, vsini, limb, &vc, &binnu);
    if (rc) return rc;
    double *d_wl = nullptr, *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_wl, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_in, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, sizeof(double) * n);
    if (e == hipSuccess) e = hipMemcpy(d_wl, wl, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in, flux, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    if (rc == MSX_OK) rc = launch_rot(c, d_in, n, d_wl, n, 1, wl[1] - wl[0], vc, limb, binnu, d_out, n);
    if (rc == MSX_OK) {
        e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d_wl);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

int msx_rot_broaden_grid(msx_ctx *c, int64_t i0, int64_t n, double vsini, double limb) {
    if (!c) return MSX_ERR_INVALID;
    return rot_grid_rows(c, 0, c->ncomp, i0, n, vsini, limb, "msx_rot_broaden_grid");
}

int msx_rot_broaden_grid_component(msx_ctx *c, int32_t comp, int64_t i0, int64_t n, double vsini, double limb) {
    if (!c) return MSX_ERR_INVALID;
    if (c->grid_staged && (comp < 0 || comp >= c->ncomp))
        return fail(c, MSX_ERR_RANGE, "msx_rot_broaden_grid_component: comp is not a copy of the staged grid (0 <= comp < ncomp)");
    return rot_grid_rows(c, comp, 1, i0, n, vsini, limb, "msx_rot_broaden_grid_component");
}

int msx_split_components(msx_ctx *c, int32_t ncomp) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->grid_staged) return fail(c, MSX_ERR_STATE, "msx_split_components: no grid staged");
    if (ncomp < 1 || ncomp > MSX_MAX_SPEC)
        return fail(c, MSX_ERR_RANGE, "msx_split_components: ncomp must be 1, 2 or 3 (one copy per component, at most MSX_MAX_SPEC)");
    if (c->ncomp != 1) return fail(c, MSX_ERR_STATE, "msx_split_components: the grid is split already");
    HIP_TRY(c, hipSetDevice(c->device));
    free_problem(c);  // its tables index the one copy
    if (ncomp == 1) return MSX_OK;
    const size_t copy = sizeof(double) * (size_t)c->nt * c->ng * c->nwl;
    double *d = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d, copy * ncomp));
    hipError_t e = hipSuccess;
    for (int s = 0; s < ncomp && e == hipSuccess; ++s)
        e = hipMemcpyAsync(reinterpret_cast<char *>(d) + copy * s, c->d_grid, copy, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(c, MSX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(c->d_grid);
    c->d_grid = d;
    c->ncomp = ncomp;
    return MSX_OK;
}

int msx_read_node(msx_ctx *c, int32_t it, int32_t ig, double *out) { return msx_read_node_component(c, 0, it, ig, out); }

int msx_read_node_component(msx_ctx *c, int32_t comp, int32_t it, int32_t ig, double *out) {
    if (!c || !out) return MSX_ERR_INVALID;
    if (!c->grid_staged) return fail(c, MSX_ERR_STATE, "msx_read_node: no grid staged");
    if (it < 0 || it >= c->nt || ig < 0 || ig >= c->ng) return fail(c, MSX_ERR_INVALID, "msx_read_node: bad node");
    if (comp < 0 || comp >= c->ncomp)
        return fail(c, MSX_ERR_RANGE, "msx_read_node_component: comp is not a copy of the staged grid (0 <= comp < ncomp)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(out, c->d_grid + (((int64_t)comp * c->nt + it) * c->ng + ig) * c->nwl, sizeof(double) * c->nwl,
                         hipMemcpyDeviceToHost));
    return MSX_OK;
}

int msx_stage_problem(msx_ctx *c, const msx_problem *p) {
    if (!c || !p) return MSX_ERR_INVALID;
    if (p->struct_size != (int32_t)sizeof(msx_problem))
        return fail(c, MSX_ERR_INVALID, "msx_stage_problem: struct_size mismatch (header/library skew)");
    if (!c->grid_staged) return fail(c, MSX_ERR_STATE, "msx_stage_problem: stage the grid first");
    if (p->nspec < 2 || p->nspec > MSX_MAX_SPEC) return fail(c, MSX_ERR_INVALID, "nspec must be 2 or 3");
    if (c->ncomp > 1 && p->nspec != c->ncomp)
        return fail(c, MSX_ERR_RANGE, "msx_stage_problem: the grid holds one copy per component (ncomp = " + std::to_string(c->ncomp) +
                                          "): nspec = " + std::to_string(p->nspec) + " must equal ncomp");
    if (p->npix < 4) return fail(c, MSX_ERR_INVALID, "npix too small");
    if (p->n_contrast < 0 || p->n_contrast > MSX_MAX_BANDS || p->n_phot < 0 || p->n_phot > MSX_MAX_BANDS)
        return fail(c, MSX_ERR_INVALID, "too many bands");
    if (p->niso < 2) return fail(c, MSX_ERR_INVALID, "isochrone table needs >= 2 rows");
    if (p->win_j0 < 0 || p->win_n < 1 || p->win_j0 + p->win_n > c->nwl)
        return fail(c, MSX_ERR_RANGE, "composite window is outside the staged grid");
    const int64_t need_lds = (int64_t)sizeof(double) * p->npix;
    const bool model_in_global = need_lds > 134 * 1024;  // > 17,152 pixels (160 KiB - ~25 KiB of static LDS): the GM variants
    for (int64_t i = 0; i < p->npix; ++i)
        if (p->pix_lo[i] < 0 || p->pix_lo[i] + 1 >= c->nwl)
            return fail(c, MSX_ERR_RANGE, "A value in x_new is outside the interpolation range (data pixel vs model grid)");
    const int nb = p->n_contrast + p->n_phot;
    for (int b = 0; b < nb; ++b)
        if (p->band_i0[b] < 0 || p->band_len[b] < 0 || p->band_i0[b] + p->band_len[b] > c->nwl)
            return fail(c, MSX_ERR_RANGE, "band weights run outside the staged grid");
    HIP_TRY(c, hipSetDevice(c->device));
    free_problem(c);
    std::vector<void *> &tr = c->prob_allocs;
    DevProblem &P = c->P;
    memset(&P, 0, sizeof(P));
    P.grid = c->d_grid; P.kgrid = c->d_kgrid; P.nwl = c->nwl; P.nt = c->nt; P.ng = c->ng;
    P.node_stride = c->ncomp > 1 ? c->nt * c->ng : 0;  // component s reads copy s: node + s * stride
    P.teff_nodes = c->d_teff; P.logg_nodes = c->d_logg; P.present = c->d_present;
    P.npix = p->npix; P.median_flux = p->median_flux; P.nspec = p->nspec;
    memcpy(P.minv, p->fit_minv, sizeof(P.minv));
    P.nc = p->n_contrast; P.np = p->n_phot;
    for (int i = 0; i < P.nc; ++i) { P.cmag[i] = p->cmag[i]; P.cerr[i] = p->cerr[i]; P.civar[i] = 1.0 / (p->cerr[i] * p->cerr[i]); }
    for (int i = 0; i < P.np; ++i) {
        P.pmag[i] = p->pmag[i]; P.perr[i] = p->perr[i]; P.pzero[i] = p->phot_zero[i]; P.pk[i] = p->phot_k[i];
        P.pivar[i] = 1.0 / (p->perr[i] * p->perr[i]);
    }
    P.win_j0 = p->win_j0; P.win_n = p->win_n;
    P.niso = p->niso; P.nav = p->nav; P.tmin = p->tmin; P.tmax = p->tmax;
    memcpy(P.pmean, p->prior_mean, sizeof(P.pmean));
    memcpy(P.psig, p->prior_sig, sizeof(P.psig));
    P.use_av = p->use_av; P.dist_fit = p->dist_fit; P.rad_prior = p->rad_prior; P.has_prior = p->has_prior_list;
    P.no_spectrum = p->no_spectrum;
    int rc;
    double *d;
    if ((rc = dev_alloc_copy(c, &tr, p->pix_t, p->npix, &d))) return rc; P.pix_t = d;
    if ((rc = dev_alloc_copy(c, &tr, p->pix_u, p->npix, &d))) return rc; P.pix_u = d;
    if ((rc = dev_alloc_copy(c, &tr, p->pix_flux, p->npix, &d))) return rc; P.pix_flux = d;
    {
        std::vector<double> ivar(p->npix);
        for (int64_t i = 0; i < p->npix; ++i) ivar[i] = 1.0 / (p->pix_err[i] * p->pix_err[i]);
        if ((rc = dev_alloc_copy(c, &tr, ivar.data(), p->npix, &d))) return rc;
        P.pix_ivar = d;
    }
    if ((rc = dev_alloc_copy(c, &tr, p->pix_err, p->npix, &d))) return rc; c->d_pix_err = d;
    if ((rc = dev_alloc_copy(c, &tr, p->iso_teff, (int64_t)p->niso, &d))) return rc; P.iso_t = d;
    if ((rc = dev_alloc_copy(c, &tr, p->iso_logg, (int64_t)p->niso, &d))) return rc; P.iso_g = d;
    if ((rc = dev_alloc_copy(c, &tr, p->iso_lum, (int64_t)p->niso, &d))) return rc; P.iso_l = d;
    if ((rc = dev_alloc_copy(c, &tr, p->av_edges_pc, (int64_t)(p->nav > 0 ? p->nav + 1 : 0), &d))) return rc; P.av_edges = d;
    if ((rc = dev_alloc_copy(c, &tr, p->av_mu, (int64_t)p->nav, &d))) return rc; P.av_mu = d;
    if ((rc = dev_alloc_copy(c, &tr, p->av_sig, (int64_t)p->nav, &d))) return rc; P.av_sig = d;

    const int64_t nn = grid_rows(c);  // every copy's rows
    // the blend's tables in two-pixel elements (logprob_kernel.h "TABLE LAYOUT"): per node R (f64) + H (f32),
    // per pixel k[lo], dk, data flux, u
    int64_t *d_lo = nullptr;
    if ((rc = dev_alloc_copy(c, &tr, p->pix_lo, p->npix, &d_lo))) return rc;
    const int64_t npair = ((p->npix + 511) / 512) * 256;
    double2 *d_r2 = nullptr, *d_kl2 = nullptr, *d_f2 = nullptr, *d_u2 = nullptr, *d_iv2 = nullptr;
    float2 *d_h2 = nullptr, *d_dk2 = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_r2, sizeof(double2) * nn * npair)); tr.push_back(d_r2);
    HIP_TRY(c, hipMalloc((void **)&d_h2, sizeof(float2) * nn * npair)); tr.push_back(d_h2);
    HIP_TRY(c, hipMalloc((void **)&d_kl2, sizeof(double2) * npair)); tr.push_back(d_kl2);
    HIP_TRY(c, hipMalloc((void **)&d_dk2, sizeof(float2) * npair)); tr.push_back(d_dk2);
    HIP_TRY(c, hipMalloc((void **)&d_f2, sizeof(double2) * npair)); tr.push_back(d_f2);
    HIP_TRY(c, hipMalloc((void **)&d_u2, sizeof(double2) * npair)); tr.push_back(d_u2);
    HIP_TRY(c, hipMalloc((void **)&d_iv2, sizeof(double2) * npair)); tr.push_back(d_iv2);
    dim3 gg((unsigned)((npair + 255) / 256), (unsigned)nn);
    hipLaunchKernelGGL(gather_rh_kernel, gg, dim3(256), 0, c->stream, c->d_grid, c->nwl, d_lo, P.pix_t, p->npix, npair, d_r2, d_h2);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(gather_statics_kernel, dim3(gg.x), dim3(256), 0, c->stream, c->d_kgrid, d_lo, P.pix_flux, P.pix_u,
                       P.pix_ivar, p->npix, npair, d_kl2, d_dk2, d_f2, d_u2, d_iv2);
    HIP_TRY(c, hipGetLastError());
    P.r2 = d_r2; P.h2 = d_h2; P.kl2 = d_kl2; P.dk2 = d_dk2; P.f2 = d_f2; P.u2 = d_u2; P.iv2 = d_iv2; P.npair = npair;
    c->d_pix_lo = d_lo;
    c->inp_rows = 0;
    P.given = nullptr; P.given_stride = 0;
    if (c->d_raw_win && p->nspec == 2 && !model_in_global && !p->no_spectrum) {
        // the in-path form needs both model samples of every data pixel inside the window that msx_broaden_grid kept raw
        bool inside = true;
        for (int64_t i = 0; i < p->npix && inside; ++i) inside = p->pix_lo[i] >= c->raw_i0 && p->pix_lo[i] + 1 < c->raw_i0 + c->raw_n;
        if (inside) {
            const int64_t gstride = 2 * npair;
            int64_t budget = 256ll << 20;
            if (const char *e = getenv("MSX_INPATH_MB")) budget = std::max<int64_t>(1, atoll(e)) << 20;
            int64_t rows_i = budget / (int64_t)(sizeof(double) * (c->raw_n + gstride) + sizeof(InpathRec));
            rows_i = std::max<int64_t>(16, std::min<int64_t>(rows_i, 16384));
            HIP_TRY(c, hipMalloc((void **)&c->d_inp_rec, sizeof(InpathRec) * rows_i));
            HIP_TRY(c, hipMalloc((void **)&c->d_inp_tmp, sizeof(double) * rows_i * c->raw_n));
            HIP_TRY(c, hipMalloc((void **)&c->d_inp_given, sizeof(double) * rows_i * gstride));
            const size_t lds_conv = sizeof(double) * ((size_t)c->raw_lx + ((size_t)(kConvTile + c->raw_lx - 1) * 5) / 4 + 2);
            if (lds_conv > 150 * 1024) return fail(c, MSX_ERR_RANGE, "in-path broadening: kernel too long for the LDS tile");
            if (lds_conv > 48 * 1024)
                HIP_TRY(c, hipFuncSetAttribute((const void *)inpath_conv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            c->inp_rows = rows_i; c->inp_gstride = gstride;
        }
    }
    c->store_f32 = false;
    if (c->store_dtype == MSX_STORE_F32) {
        // A separately labelled storage precision (store_dtype): the R table rounded to float32, read by the
        // fused binary variants compiled for it.  Everything else keeps float64 -- and the forms that have no such variant
        // (pair, linked, triples, spectra beyond the LDS) are refused rather than mixed in: one staged problem, one precision.
        if (p->nspec != 2 || model_in_global)
            return fail(c, MSX_ERR_STATE, "msx_set_grid_storage(MSX_STORE_F32): binaries of at most 17,152 pixels only");
        float2 *d_r2f = nullptr;
        HIP_TRY(c, hipMalloc((void **)&d_r2f, sizeof(float2) * nn * npair)); tr.push_back(d_r2f);
        const int64_t tot = nn * npair;
        hipLaunchKernelGGL(narrow_r_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, d_r2, d_r2f, tot);
        HIP_TRY(c, hipGetLastError());
        P.r2f = d_r2f;
        c->store_f32 = true;
    }
    float2 *const d_r2f_for_quads = const_cast<float2 *>(P.r2f);
    {   // the float32 tables in quads, for the 512-thread variants
        const int64_t nquad = (npair + 1023) / 1024 * 512;
        float4 *d_h4 = nullptr, *d_dk4 = nullptr, *d_h4b = nullptr, *d_dk4b = nullptr;
        HIP_TRY(c, hipMalloc((void **)&d_h4, sizeof(float4) * nn * nquad)); tr.push_back(d_h4);
        HIP_TRY(c, hipMalloc((void **)&d_dk4, sizeof(float4) * nquad)); tr.push_back(d_dk4);
        HIP_TRY(c, hipMalloc((void **)&d_h4b, sizeof(float4) * nn * nquad)); tr.push_back(d_h4b);
        HIP_TRY(c, hipMalloc((void **)&d_dk4b, sizeof(float4) * nquad)); tr.push_back(d_dk4b);
        const unsigned gq = (unsigned)((nquad + 255) / 256);
        hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, (unsigned)nn), dim3(256), 0, c->stream, d_h2, npair, nquad, (int64_t)512, d_h4);
        hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, 1), dim3(256), 0, c->stream, d_dk2, npair, nquad, (int64_t)512, d_dk4);
        hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, (unsigned)nn), dim3(256), 0, c->stream, d_h2, npair, nquad, (int64_t)256, d_h4b);
        hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, 1), dim3(256), 0, c->stream, d_dk2, npair, nquad, (int64_t)256, d_dk4b);
        HIP_TRY(c, hipGetLastError());
        P.h4 = d_h4; P.dk4 = d_dk4; P.h4b = d_h4b; P.dk4b = d_dk4b; P.nquad = nquad;
        if (d_r2f_for_quads) {  // float32 storage: the R table by quad too
            float4 *d_r4f = nullptr, *d_r4fb = nullptr;
            HIP_TRY(c, hipMalloc((void **)&d_r4f, sizeof(float4) * nn * nquad)); tr.push_back(d_r4f);
            HIP_TRY(c, hipMalloc((void **)&d_r4fb, sizeof(float4) * nn * nquad)); tr.push_back(d_r4fb);
            hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, (unsigned)nn), dim3(256), 0, c->stream, d_r2f_for_quads, npair, nquad, (int64_t)512, d_r4f);
            hipLaunchKernelGGL(gather_quads_kernel, dim3(gq, (unsigned)nn), dim3(256), 0, c->stream, d_r2f_for_quads, npair, nquad, (int64_t)256, d_r4fb);
            HIP_TRY(c, hipGetLastError());
            P.r4f = d_r4f; P.r4fb = d_r4fb;
        }
    }
    // band integrals
    double *d_tab = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_tab, sizeof(double) * std::max<int64_t>(1, nn * nb))); tr.push_back(d_tab);
    if (nb > 0) {
        std::vector<int64_t> woff(nb);
        int64_t tot = 0;
        for (int b = 0; b < nb; ++b) { woff[b] = tot; tot += p->band_len[b]; }
        double *d_w = nullptr;
        int64_t *d_woff = nullptr, *d_i0 = nullptr, *d_len = nullptr;
        if ((rc = dev_alloc_copy(c, &tr, p->band_w, tot, &d_w))) return rc;
        if ((rc = dev_alloc_copy(c, &tr, woff.data(), (int64_t)nb, &d_woff))) return rc;
        if ((rc = dev_alloc_copy(c, &tr, p->band_i0, (int64_t)nb, &d_i0))) return rc;
        if ((rc = dev_alloc_copy(c, &tr, p->band_len, (int64_t)nb, &d_len))) return rc;
        hipLaunchKernelGGL(band_integral_kernel, dim3((unsigned)nb, (unsigned)nn), dim3(256), 0, c->stream, c->d_grid,
                           c->nwl, d_w, d_woff, d_i0, d_len, nb, d_tab);
        HIP_TRY(c, hipGetLastError());
    }
    P.band_tab = d_tab;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->max_dyn_lds = (int)need_lds;
    c->model_in_global = model_in_global;
    {   // the PF variants' dynamic LDS -- model + u2 + f2 -- must fit beside their static LDS (asked of the functions
        // themselves: the static part has grown over the rounds, a constant here once let 5,800..6,270 pixels through).
        // 512 threads: one workgroup per CU; 256 threads: two of them in a CU's LDS.
        const int64_t dyn_pf = (int64_t)sizeof(double) * ((p->npix + 1) & ~1ll) + 32 * npair;
        c->pf_ok = !model_in_global;
        c->pf256_ok = true;
        for (const Variant &v : kVariants) {
            if (!v.pf) continue;
            hipFuncAttributes at;
            HIP_TRY(c, hipFuncGetAttributes(&at, v.fn));
            if (v.threads == 512) c->pf_ok = c->pf_ok && dyn_pf <= ((160 * 1024 - (int64_t)at.sharedSizeBytes) & ~15ll);
            else c->pf256_ok = c->pf256_ok && 2 * (dyn_pf + (int64_t)at.sharedSizeBytes) <= 160 * 1024;
        }
    }
    if ((rc = raise_dynamic_lds_limits(c))) return rc;
    c->recipe_fast = P.niso <= 4 * kWave && P.nt <= kWave && P.ng <= 32 && P.nav + 1 <= 2 * kWave;
    c->d_recipe_block = nullptr;
    if (c->recipe_fast) {  // the recipe's tables behind one (preloaded) pointer
        void *blk = nullptr;
        HIP_TRY(c, hipMalloc(&blk, kRecipeBlockBytes));
        tr.push_back(blk);
        c->d_recipe_block = (unsigned char *)blk;
        HIP_TRY(c, hipMemsetAsync(blk, 0, kRecipeBlockBytes, c->stream));
        const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbIsoT, P.iso_t, sizeof(double) * P.niso, dd, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbIsoG, P.iso_g, sizeof(double) * P.niso, dd, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbTeff, P.teff_nodes, sizeof(double) * P.nt, dd, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbLogg, P.logg_nodes, sizeof(double) * P.ng, dd, c->stream));
        std::vector<uint8_t> pres((size_t)(P.nt * P.ng));
        HIP_TRY(c, hipMemcpyAsync(pres.data(), P.present, pres.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<uint32_t> pmask((size_t)P.nt, 0u);
        for (int64_t t = 0; t < P.nt; ++t)
            for (int64_t g = 0; g < P.ng; ++g)
                if (pres[(size_t)(t * P.ng + g)]) pmask[(size_t)t] |= 1u << g;
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbPresent, pmask.data(), sizeof(uint32_t) * pmask.size(),
                                  hipMemcpyHostToDevice, c->stream));
        // the packed copies for the wave form's lanes (dev_types.h): entry + right neighbour, slopes, pads
        std::vector<unsigned char> pack((size_t)(kRecipeBlockBytes - kRbIsoPack), 0);
        {
            double *iso = reinterpret_cast<double *>(pack.data());
            for (int i = 0; i < 4 * kWave; ++i) {
                const bool in = i < P.niso, nx = i + 1 < P.niso;
                const double x = in ? p->iso_teff[i] : INFINITY, y = in ? p->iso_logg[i] : 0.0;
                const double xn = nx ? p->iso_teff[i + 1] : INFINITY, yn = nx ? p->iso_logg[i + 1] : 0.0;
                iso[4 * i] = x; iso[4 * i + 1] = xn; iso[4 * i + 2] = y;
                iso[4 * i + 3] = nx ? (yn - y) / (xn - x) : 0.0;  // np.interp's slope (IEEE division, like the device's)
            }
            double *tp = reinterpret_cast<double *>(pack.data() + (kRbTeffPack - kRbIsoPack));
            double *gp = reinterpret_cast<double *>(pack.data() + (kRbLoggPack - kRbIsoPack));
            uint32_t *mp = reinterpret_cast<uint32_t *>(pack.data() + (kRbMaskPack - kRbIsoPack));
            for (int l = 0; l < kWave; ++l) {
                tp[2 * l] = l < P.nt ? c->h_teff[(size_t)l] : INFINITY;
                tp[2 * l + 1] = l + 1 < P.nt ? c->h_teff[(size_t)l + 1] : INFINITY;
                gp[2 * l] = l < P.ng ? c->h_logg[(size_t)l] : INFINITY;
                gp[2 * l + 1] = l + 1 < P.ng ? c->h_logg[(size_t)l + 1] : INFINITY;
                mp[2 * l] = l < P.nt ? pmask[(size_t)l] : 0u;
                mp[2 * l + 1] = l + 1 < P.nt ? pmask[(size_t)l + 1] : 0u;
            }
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_recipe_block + kRbIsoPack, pack.data(), pack.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    // Scratch, sized once here so that no launch ever allocates or synchronises -- and only for the forms the staged
    // spectrum can take: the GM variants (model vectors beyond the LDS) and the linked form (2..8 segments).  A batch
    // beyond `scratch_rows` walkers is then cut into sub-batches.  Everything else (config 2, 3, 5) allocates nothing.
    c->nseg = (int)((npair + kSegElems - 1) / kSegElems);
    const bool can_link = c->nseg >= 2 && c->nseg <= 8;  // (a workgroup of the linked form holds one segment: up to 65,536 pixels)
    P.linked_fault = 0;  // (msx_test_hook)
    if (model_in_global || can_link) {
        int64_t budget = 96ll << 20;
        if (const char *e = getenv("MSX_SCRATCH_MB")) budget = std::max<int64_t>(1, atoll(e)) << 20;
        int64_t sb = budget / (int64_t)(sizeof(double) * p->npix);
        sb = std::max<int64_t>(256, std::min<int64_t>(sb, 16384));
        HIP_TRY(c, hipMalloc((void **)&c->d_model_scratch, sizeof(double) * sb * p->npix));
        c->scratch_rows = sb;
        P.model_scratch = c->d_model_scratch;
        if (can_link) {
            HIP_TRY(c, hipMalloc((void **)&c->d_segparts, sizeof(SegPart) * sb * c->nseg));
            P.segparts = c->d_segparts;
            // hand-over flags, and behind them the poison word (cleared together, here and nowhere else)
            HIP_TRY(c, hipMalloc((void **)&c->d_seg_flag, sizeof(unsigned long long) * (sb + 1)));
            HIP_TRY(c, hipMemset(c->d_seg_flag, 0, sizeof(unsigned long long) * (sb + 1)));
            P.seg_flag = c->d_seg_flag;
            P.linked_poison = reinterpret_cast<int32_t *>(c->d_seg_flag + sb);
        }
    }
    c->linked_poisoned = false;
    // the pair form: binaries of <= 4096 pixels (model values in registers), register-resident recipe.  Its spill path
    // (vectors the early histogram cannot handle) leases one of kPairSpillRows scratch rows (32 MB at 4096 pixels); the
    // planner's items take 256 bytes per walker of a sub-batch.
    if (p->nspec == 2 && p->npix <= kPairMaxPix && c->recipe_fast && !p->no_spectrum) {
        const int64_t rows = 16384;
        HIP_TRY(c, hipMalloc((void **)&c->d_model_scratch, sizeof(double) * kPairSpillRows * p->npix));
        P.model_scratch = c->d_model_scratch;
        // the planner's header and, behind it, the leases of the spill rows
        const size_t plan_bytes = sizeof(int32_t) * (size_t)(kPairHdrInts + kPairSpillRows);
        HIP_TRY(c, hipMalloc((void **)&c->d_pair_plan, plan_bytes));
        HIP_TRY(c, hipMemset(c->d_pair_plan, 0, plan_bytes));
        P.pair_lease = c->d_pair_plan + kPairHdrInts;
        HIP_TRY(c, hipMalloc((void **)&c->d_pair_items, sizeof(PairItem) * (size_t)((rows + 1) / 2)));
        HIP_TRY(c, hipMalloc((void **)&c->d_pair_singles, sizeof(PairRec) * (size_t)rows));
        P.pair_items = c->d_pair_items;
        P.pair_singles = c->d_pair_singles;
        HIP_TRY(c, hipHostMalloc((void **)&c->h_pair_stats, 2 * sizeof(int32_t), hipHostMallocDefault));
        c->h_pair_stats[0] = 1; c->h_pair_stats[1] = 0;  // (nothing known yet: try)
        c->pair_auto_launches = 0;
        c->pair_rows = rows;
        // From where the pair form pays (the planner costs 10.4 us whatever the batch; 14.6 before its searches went 4-ary
        // and side by side, round 4): measured on 256 CUs in one process, fused (FULL variants) against pair, us per batch
        // -- 4096 px (profiles/r4_crossover_4096px.jsonl): 1,024 walkers 39.6 / 42.2, 1,536: 49.7 / 48.9, 2,048: 61.4 / 57.2,
        // 2,304: 66.9 / 61.6, 3,072: 85.2 / 73.5, 4,096: 109.5 / 89.6.  1194 px (r4_crossover_1194px.jsonl): 2,304 walkers
        // 45.8 / 45.7, 3,072: 55.4 / 53.2, 4,096: 72.2 / 64.0, 6,144: 104.5 / 85.7.  In walkers per CU: 8 for the long
        // spectra, 12 for the short ones.
        {
            const int64_t cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
            c->pair_min_walkers = (p->npix > 3072 ? 8 : 12) * cus;
        }
        if (const char *e = getenv("MSX_PAIR_MIN")) c->pair_min_walkers = atoll(e) > 0 ? std::max<int64_t>(2, atoll(e)) : INT64_MAX;
    }
#ifdef MSX_STAMPS
    {   // diagnostic build only: per-walker shader-clock stamps
        unsigned long long *st = nullptr;
        HIP_TRY(c, hipMalloc((void **)&st, sizeof(unsigned long long) * 16 * 65536)); tr.push_back(st);
        HIP_TRY(c, hipMemset(st, 0, sizeof(unsigned long long) * 16 * 65536));
        P.stamps = st;
    }
#endif
    {   // the clock probe's stamps (msx_probe_launch)
        unsigned long long *cp = nullptr;
        HIP_TRY(c, hipMalloc((void **)&cp, sizeof(unsigned long long) * 4 * kProbeWalkers)); tr.push_back(cp);
        HIP_TRY(c, hipMemset(cp, 0, sizeof(unsigned long long) * 4 * kProbeWalkers));
        P.clk_probe = cp;
    }
    c->problem_staged = true;
    return MSX_OK;
}

#ifdef MSX_STAMPS
int msx_diag_read_med_stamps(msx_ctx *c, int64_t n, unsigned long long *out) {
    if (!c || n > 65536) return MSX_ERR_INVALID;
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_med_stamps), sizeof(unsigned long long) * 8 * n));
    return MSX_OK;
}
int msx_diag_read_stamps(msx_ctx *c, int64_t n, unsigned long long *out) {
    if (!c || !c->problem_staged || n > 65536) return MSX_ERR_INVALID;
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(out, c->P.stamps, sizeof(unsigned long long) * 16 * n, hipMemcpyDeviceToHost));
    return MSX_OK;
}
#endif

int msx_set_grid_storage(msx_ctx *c, int32_t store_dtype) {
    if (!c || (store_dtype != MSX_STORE_F64 && store_dtype != MSX_STORE_F32))
        return fail(c, MSX_ERR_INVALID, "msx_set_grid_storage: MSX_STORE_F64 or MSX_STORE_F32");
    c->store_dtype = store_dtype;
    return MSX_OK;
}

int msx_set_path(msx_ctx *c, int32_t path) {
    if (!c || (path != MSX_PATH_AUTO && path != MSX_PATH_FUSED && path != MSX_PATH_LINKED && path != MSX_PATH_PAIR && path != MSX_PATH_INPATH))
        return fail(c, MSX_ERR_INVALID, "msx_set_path: bad path (MSX_PATH_AUTO, _FUSED, _PAIR, _LINKED or _INPATH)");
    c->path = path;
    return MSX_OK;
}

int msx_set_broadening(msx_ctx *c, int32_t placement) {
    if (!c || (placement != MSX_BROADEN_STAGING && placement != MSX_BROADEN_IN_PATH))
        return fail(c, MSX_ERR_INVALID, "msx_set_broadening: MSX_BROADEN_STAGING or MSX_BROADEN_IN_PATH");
    c->broaden_placement = placement;
    return MSX_OK;
}

int msx_logprob_batch_dev(msx_ctx *c, int32_t mode, const double *d_theta, int64_t n, int32_t ndim, double *d_logp,
                          int32_t *d_status, void *hip_stream, int32_t block_threads) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_logprob_batch: no problem staged");
    if (n < 0 || !d_theta || !d_logp || !d_status) return fail(c, MSX_ERR_INVALID, "msx_logprob_batch: bad arguments");
    if (ndim != 2 * c->P.nspec + 2)
        return fail(c, MSX_ERR_INVALID, "P0 doesn't match what I was expecting (ndim must be 2*nspec+2)");
    if (mode < 0 || mode > 5) return fail(c, MSX_ERR_INVALID, "msx_logprob_batch: bad mode");
    if ((mode == MSX_MODE_OPT_STEP || mode == MSX_MODE_OPT_INIT) && !c->P.opt_flux)
        return fail(c, MSX_ERR_STATE, "optimiser modes go through msx_opt_init / msx_opt_step");
    if (n == 0) return MSX_OK;
    bool shared512;
    if (int rc = decode_block(c, block_threads, shared512)) return rc;
    const DevProblem &Pc = c->P;
    LaunchArgs A;
    A.ndim = ndim; A.mode = mode; A.s = (hipStream_t)hip_stream;
    pack_leading_words(Pc, c->recipe_fast, mode, &A.niso_nt, &A.ng_mode_fast);

    // ---- which form of the path (decide_form) ---------------------------------------------------------------
    const FormChoice form = decide_form(c, n, mode, false);
    if (form.err != MSX_OK) return fail(c, form.err, form.msg);
    if (c->smp_overlap_launch) A.ng_mode_fast |= 1 << 20;
    if (c->probe_launch) A.ng_mode_fast |= 1 << 21;
    if (form.linked) A.ng_mode_fast |= c->nseg << 24;
    c->last_form = form.inpath ? MSX_FORM_INPATH : form.pair ? MSX_FORM_PAIR : form.linked ? MSX_FORM_LINKED : MSX_FORM_FUSED;
    // ---- how (plan_launch), per sub-batch: the last one, if shorter, is planned for its own walker count ------------
    LaunchPlan pl = plan_launch(c, form, n, block_threads, shared512);
    for (int64_t off = 0; off < n; off += pl.rows) {
        const int64_t m = std::min<int64_t>(pl.rows, n - off);
        if (m != pl.m) pl = plan_launch(c, form, m, block_threads, shared512);
        if (!pl.fn) return fail(c, MSX_ERR_STATE, "no kernel variant for this launch");
        A.theta = d_theta + off * ndim; A.logp = d_logp + off; A.status = d_status + off; A.n = m;
        const DevProblem P = problem_at(Pc, off, mode, ndim);
        const int rc = form.inpath ? launch_inpath(c, P, A, pl) : form.pair ? launch_pair(c, P, A, pl) : launch_logprob(c, P, A, pl);
        if (rc) return rc;
    }
    return MSX_OK;
}

int msx_probe_launch(msx_ctx *c, int32_t mode, const double *d_theta, int64_t n, int32_t ndim, double *d_logp,
                     int32_t *d_status, void *hip_stream, int32_t block_threads, double *out4) {
    if (!c || !out4) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_probe_launch: no problem staged");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t m = std::min<int64_t>(n, kProbeWalkers);
    HIP_TRY(c, hipMemsetAsync(c->P.clk_probe, 0, sizeof(unsigned long long) * 4 * (size_t)m, (hipStream_t)hip_stream));
    c->probe_launch = true;
    const int rc = msx_logprob_batch_dev(c, mode, d_theta, n, ndim, d_logp, d_status, hip_stream, block_threads);
    c->probe_launch = false;
    if (rc != MSX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)hip_stream));
    std::vector<unsigned long long> h((size_t)(4 * m));
    HIP_TRY(c, hipMemcpy(h.data(), c->P.clk_probe, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    std::vector<double> mhz, chain;
    unsigned long long w0 = ~0ull, w1 = 0ull;
    for (int64_t i = 0; i < m; ++i) {
        const unsigned long long a = h[(size_t)(4 * i)], ca = h[(size_t)(4 * i + 1)], b = h[(size_t)(4 * i + 2)], cb = h[(size_t)(4 * i + 3)];
        if (a == 0ull || b <= a) continue;  // (a walker the pair planner or an early exit finished: no stamps)
        mhz.push_back((double)(cb - ca) / (double)(b - a) * 100.0);  // wall clock: 100 MHz
        chain.push_back((double)(b - a) / 100.0);
        w0 = std::min(w0, a); w1 = std::max(w1, b);
    }
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (mhz.empty()) return MSX_OK;
    std::sort(mhz.begin(), mhz.end()); std::sort(chain.begin(), chain.end());
    out4[0] = mhz[mhz.size() / 2];
    out4[1] = chain[chain.size() / 2];
    out4[2] = chain.back();
    out4[3] = (double)(w1 - w0) / 100.0;
    return MSX_OK;
}

int msx_logprob_batch(msx_ctx *c, int32_t mode, const double *theta, int64_t n, int32_t ndim, double *logp_out,
                      int32_t *status_out) {
    if (!c) return MSX_ERR_INVALID;
    if (!theta || !logp_out || !status_out || n < 0) return fail(c, MSX_ERR_INVALID, "msx_logprob_batch: bad arguments");
    // everything the copy below relies on is checked BEFORE the pinned staging buffer is sized or written
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_logprob_batch: no problem staged");
    if (ndim != 2 * c->P.nspec + 2 || ndim > MSX_MAX_DIM)
        return fail(c, MSX_ERR_INVALID, "P0 doesn't match what I was expecting (ndim must be 2*nspec+2)");
    if (n == 0) return MSX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PinnedStaging h;
    HIP_TRY(c, pinned_staging(&c->h_pin, &c->cap_walkers, n, &h));
    memcpy(h.theta, theta, sizeof(double) * n * ndim);
    int rc = msx_logprob_batch_dev(c, mode, h.theta, n, ndim, h.logp, h.status, c->stream, 0);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(logp_out, h.logp, sizeof(double) * n);
    memcpy(status_out, h.status, sizeof(int32_t) * n);
    note_handover(c, status_out, n);
    return MSX_OK;
}

int msx_opt_init(msx_ctx *c, const double *theta0, int64_t nchains, int32_t ndim, double *chi2_out,
                 int32_t *status_out) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_opt_init: no problem staged");
    if (!theta0 || !chi2_out || !status_out || nchains < 1) return fail(c, MSX_ERR_INVALID, "msx_opt_init: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    opt_run_free(c);  // (a run in flight reads the data vectors freed below)
    if (c->d_opt_flux) (void)hipFree(c->d_opt_flux);
    if (c->d_opt_med) (void)hipFree(c->d_opt_med);
    c->d_opt_flux = c->d_opt_med = nullptr; c->opt_chains = 0;
    c->P.opt_flux = c->P.opt_med = nullptr;
    HIP_TRY(c, hipMalloc((void **)&c->d_opt_flux, sizeof(double) * nchains * c->P.npix));
    HIP_TRY(c, hipMalloc((void **)&c->d_opt_med, sizeof(double) * nchains));
    c->opt_chains = nchains;
    c->P.opt_flux = c->d_opt_flux; c->P.opt_med = c->d_opt_med; c->P.opt_chain = nullptr;
    return msx_logprob_batch(c, MSX_MODE_OPT_INIT, theta0, nchains, ndim, chi2_out, status_out);
}

int msx_opt_step(msx_ctx *c, const double *theta, const int32_t *chain, int64_t n, int32_t ndim, double *chi2_out,
                 int32_t *status_out) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged || !c->P.opt_flux) return fail(c, MSX_ERR_STATE, "msx_opt_step: call msx_opt_init first");
    if (!theta || !chain || !chi2_out || !status_out || n < 0) return fail(c, MSX_ERR_INVALID, "msx_opt_step: bad arguments");
    if (n == 0) return MSX_OK;
    for (int64_t i = 0; i < n; ++i)
        if (chain[i] < 0 || chain[i] >= c->opt_chains) return fail(c, MSX_ERR_INVALID, "msx_opt_step: chain index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n > c->cap_chain) {
        if (c->d_opt_chain) (void)hipFree(c->d_opt_chain);
        c->d_opt_chain = nullptr; c->cap_chain = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_opt_chain, sizeof(int32_t) * std::max<int64_t>(n, 1024)));
        c->cap_chain = std::max<int64_t>(n, 1024);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_opt_chain, chain, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    c->P.opt_chain = c->d_opt_chain;
    return msx_logprob_batch(c, MSX_MODE_OPT_STEP, theta, n, ndim, chi2_out, status_out);
}

// ---- device-resident pre-optimiser ---------------------------------------------------
// fit_spec's chains (mft6.py:856-1137) with their state in HBM.  A TRIP is one draw of every chain: the chain's thread
// (opt_run_kernels.h) proposes, the UNCHANGED hot kernel evaluates the in-bounds proposals in MSX_MODE_OPT_STEP (one
// workgroup per chain; chains with nothing to evaluate hand it a row of NaNs and their workgroup leaves after its
// recipe), and the chain's thread applies the prior terms and the accept rule -- fused with the next trip's proposal,
// so a chunk of k trips is 2 k + 1 launches on the compute stream and nothing returns to the host in between.  Two
// slots, pipelined like the sampler's: chunk i + 1 is uploaded and queued while chunk i runs.
struct OptRun {
    OptRunDev R;
    int64_t nch = 0, cap_trips = 0;
    int32_t ndim = 0;
    bool failed = false;
    char *d_state = nullptr;
    int32_t *d_ident = nullptr;  // [nch] 0, 1, ...: chain of walker c (DevProblem::opt_chain)
    hipStream_t copy = nullptr, up = nullptr;
    struct Slot {
        char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
        hipEvent_t in_ready = nullptr, kernels_done = nullptr, out_ready = nullptr;
        int64_t ntrips = 0;
        bool busy = false;
    } slot[2];
    size_t in_bytes(int64_t t) const { return sizeof(double) * (size_t)(t * nch * ndim); }
    size_t rec_count(int64_t t) const { return (size_t)(t * nch * (ndim + 2)); }
    size_t out_bytes(int64_t t) const {  // [records | flags | live, worst]
        return sizeof(double) * rec_count(t) + sizeof(int32_t) * (size_t)(t * nch + 2);
    }
};

static void opt_run_free(msx_ctx *c) {
    OptRun *r = c->opt_run;
    if (!r) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (r->copy) (void)hipStreamSynchronize(r->copy);
    if (r->up) (void)hipStreamSynchronize(r->up);
    for (auto &sl : r->slot) {
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.in_ready) (void)hipEventDestroy(sl.in_ready);
        if (sl.kernels_done) (void)hipEventDestroy(sl.kernels_done);
        if (sl.out_ready) (void)hipEventDestroy(sl.out_ready);
    }
    if (r->d_state) (void)hipFree(r->d_state);
    if (r->copy) (void)hipStreamDestroy(r->copy);
    if (r->up) (void)hipStreamDestroy(r->up);
    delete r;
    c->opt_run = nullptr;
    c->P.opt_chain = nullptr;
}

int msx_opt_run_begin(msx_ctx *c, int64_t nchains, int32_t ndim, const double *gi0, const double *chi0, int64_t steps,
                      double tmin, double tmax, int32_t dist_fit, int32_t rad_prior, double plx_prior, double plx_sigma,
                      int32_t nedges, const double *av_edges, int32_t nav, const double *av_mu, const double *av_sig,
                      int32_t niso, const double *iso_teff, const double *iso_lum, int64_t max_chunk_trips) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged || !c->P.opt_flux) return fail(c, MSX_ERR_STATE, "msx_opt_run_begin: call msx_opt_init first");
    if (!gi0 || !chi0 || !av_edges || !av_mu || !av_sig || nedges < 1 || nav < 1 || steps < 1 || steps > (1ll << 40) ||
        max_chunk_trips < 1)
        return fail(c, MSX_ERR_INVALID, "msx_opt_run_begin: bad arguments");
    if (nchains != c->opt_chains) return fail(c, MSX_ERR_INVALID, "msx_opt_run_begin: one chain per row of msx_opt_init's theta0");
    if (ndim != 2 * c->P.nspec + 2 || ndim > MSX_MAX_DIM) return fail(c, MSX_ERR_INVALID, "P0 doesn't match what I was expecting");
    if (rad_prior && (!iso_teff || !iso_lum || niso < 2)) return fail(c, MSX_ERR_INVALID, "msx_opt_run_begin: rad_prior needs the isochrone");
    if (!rad_prior) niso = 0;
    for (int32_t i = 1; i < nedges; ++i)
        if (!(av_edges[i - 1] <= av_edges[i])) return fail(c, MSX_ERR_INVALID, "msx_opt_run_begin: av_edges must ascend");
    for (int32_t i = 1; i < niso; ++i)
        if (!(iso_teff[i - 1] <= iso_teff[i])) return fail(c, MSX_ERR_INVALID, "msx_opt_run_begin: iso_teff must ascend");
    HIP_TRY(c, hipSetDevice(c->device));
    opt_run_free(c);
    OptRun *r = new OptRun;
    c->opt_run = r;
    const int64_t nch = nchains;
    const int ns = c->P.nspec;
    r->nch = nch; r->ndim = ndim; r->cap_trips = max_chunk_trips;
    // state: doubles first [gi | chi | n | rad0 | dist0 | theta | like | tables], then int64 total_n, then the int32 arrays
    const size_t ntab = (size_t)nedges + 2 * (size_t)nav + 2 * (size_t)niso;
    const size_t ndbl = (size_t)(nch * ndim) * 2 + (size_t)nch * 4 + (size_t)(nch * ns) + ntab;
    const size_t state_bytes = sizeof(double) * ndbl + sizeof(int64_t) * (size_t)nch + sizeof(int32_t) * (size_t)(4 * nch);
    std::vector<double> h(ndbl, 0.0);
    hipError_t e = hipMalloc((void **)&r->d_state, state_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_state, 0, state_bytes, c->stream);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->up, hipStreamNonBlocking);
    for (auto &sl : r->slot) {
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_in, r->in_bytes(r->cap_trips));
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_out, r->out_bytes(r->cap_trips));
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_in, r->in_bytes(r->cap_trips), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_out, r->out_bytes(r->cap_trips), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.in_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.kernels_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.out_ready, hipEventDisableTiming);
    }
    if (e == hipSuccess) {
        OptRunDev &R = r->R;
        double *d = (double *)r->d_state;
        size_t o = 0;
        auto take = [&](size_t cnt) { double *p = d + o; o += cnt; return p; };
        R.gi = take((size_t)(nch * ndim));
        R.chi = take((size_t)nch);
        R.n = take((size_t)nch);
        R.rad0 = take((size_t)(nch * ns));
        R.dist0 = take((size_t)nch);
        R.theta = take((size_t)(nch * ndim));
        double *like = take((size_t)nch);
        R.like = like;
        double *t_edges = take((size_t)nedges), *t_mu = take((size_t)nav), *t_sig = take((size_t)nav);
        double *t_isot = take((size_t)niso), *t_isol = take((size_t)niso);
        R.av_edges = t_edges; R.av_mu = t_mu; R.av_sig = t_sig; R.iso_t = t_isot; R.iso_l = t_isol;
        R.total_n = (int64_t *)(d + ndbl);
        R.done = (int32_t *)(R.total_n + nch);
        R.tflag = R.done + nch;
        int32_t *status = R.tflag + nch;
        R.status = status;
        r->d_ident = status + nch;
        R.nch = (int32_t)nch; R.ndim = ndim; R.nspec = ns; R.dist_fit = dist_fit != 0; R.rad_prior = rad_prior != 0;
        R.nedges = nedges; R.nmu = nav; R.niso = niso;
        R.steps = (double)steps; R.cap = 50 * steps;
        R.tmin = tmin; R.tmax = tmax; R.pprior = plx_prior; R.psig = plx_sigma;
        // the host image of the doubles: the start points, their chi^2, n = 0, the step sizes' scales, the tables
        memcpy(h.data() + (R.gi - d), gi0, sizeof(double) * (size_t)(nch * ndim));
        memcpy(h.data() + (R.chi - d), chi0, sizeof(double) * (size_t)nch);
        for (int64_t k = 0; k < nch; ++k) {
            for (int s = 0; s < ns; ++s) h[(size_t)((R.rad0 - d) + k * ns + s)] = gi0[k * ndim + ns + 1 + s];
            h[(size_t)((R.dist0 - d) + k)] = gi0[k * ndim + 2 * ns + 1];
        }
        memcpy(h.data() + (t_edges - d), av_edges, sizeof(double) * (size_t)nedges);
        memcpy(h.data() + (t_mu - d), av_mu, sizeof(double) * (size_t)nav);
        memcpy(h.data() + (t_sig - d), av_sig, sizeof(double) * (size_t)nav);
        if (niso > 0) {
            memcpy(h.data() + (t_isot - d), iso_teff, sizeof(double) * (size_t)niso);
            memcpy(h.data() + (t_isol - d), iso_lum, sizeof(double) * (size_t)niso);
        }
        e = hipMemcpyAsync(d, h.data(), sizeof(double) * ndbl, hipMemcpyHostToDevice, c->stream);  // (behind the memset)
    }
    std::vector<int32_t> ident((size_t)nch);
    for (int64_t k = 0; k < nch; ++k) ident[(size_t)k] = (int32_t)k;
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_ident, ident.data(), sizeof(int32_t) * (size_t)nch, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (the host images above are consumed)
    if (e != hipSuccess) {
        opt_run_free(c);
        return fail(c, MSX_ERR_HIP, std::string("msx_opt_run_begin: ") + hipGetErrorString(e));
    }
    return MSX_OK;
}

static hipError_t opt_run_trip_launch(msx_ctx *c, const OptRun *r, const double *z, double *rec, int32_t *flags, int32_t *worst,
                                      int32_t *live) {
    const dim3 grid((unsigned int)((r->nch + kOptRunThreads - 1) / kOptRunThreads)), block(kOptRunThreads);
    if (r->R.nspec == 2)
        hipLaunchKernelGGL(opt_run_trip_kernel<2>, grid, block, 0, c->stream, r->R, z, rec, flags, worst, live);
    else
        hipLaunchKernelGGL(opt_run_trip_kernel<3>, grid, block, 0, c->stream, r->R, z, rec, flags, worst, live);
    return hipGetLastError();
}

int msx_opt_run_enqueue(msx_ctx *c, int32_t slot, int64_t ntrips, const double *z) {
    if (!c) return MSX_ERR_INVALID;
    OptRun *r = c->opt_run;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_opt_run_enqueue: call msx_opt_run_begin first");
    if (r->failed) return fail(c, MSX_ERR_STATE, "msx_opt_run_enqueue: an earlier chunk failed while it was queued; call msx_opt_run_end");
    if (slot < 0 || slot > 1 || !z || ntrips < 1 || ntrips > r->cap_trips)
        return fail(c, MSX_ERR_INVALID, "msx_opt_run_enqueue: bad arguments (slot 0|1, 1 <= ntrips <= max_chunk_trips)");
    OptRun::Slot &sl = r->slot[slot];
    if (sl.busy) return fail(c, MSX_ERR_STATE, "msx_opt_run_enqueue: the slot holds a chunk that was not collected");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t nch = r->nch;
    const int32_t ndim = r->ndim;
    memcpy(sl.h_in, z, r->in_bytes(ntrips));
    HIP_TRY(c, hipMemcpyAsync(sl.d_in, sl.h_in, r->in_bytes(ntrips), hipMemcpyHostToDevice, r->up));
    HIP_TRY(c, hipEventRecord(sl.in_ready, r->up));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.in_ready, 0));
    double *rec = (double *)sl.d_out;
    int32_t *flags = (int32_t *)(rec + r->rec_count(ntrips));
    int32_t *live = flags + ntrips * nch, *worst = live + 1;
    r->failed = true;  // (until every launch of the chunk is queued)
    HIP_TRY(c, hipMemsetAsync(live, 0, 2 * sizeof(int32_t), c->stream));
    c->P.opt_chain = r->d_ident;
    const double *dz = (const double *)sl.d_in;
    for (int64_t t = 0; t <= ntrips; ++t) {
        // the last lines of trip t - 1 and the first lines of trip t, then trip t's evaluation
        const bool prev = t > 0, next = t < ntrips;
        HIP_TRY(c, opt_run_trip_launch(c, r, next ? dz + t * nch * ndim : nullptr, prev ? rec + (t - 1) * nch * (ndim + 2) : nullptr,
                                       prev ? flags + (t - 1) * nch : nullptr, worst, next ? nullptr : live));
        if (next) {
            const int rc = msx_logprob_batch_dev(c, MSX_MODE_OPT_STEP, r->R.theta, nch, ndim, const_cast<double *>(r->R.like),
                                                 const_cast<int32_t *>(r->R.status), c->stream, 0);
            if (rc != MSX_OK) return rc;
        }
    }
    r->failed = false;
    HIP_TRY(c, hipEventRecord(sl.kernels_done, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(r->copy, sl.kernels_done, 0));
    HIP_TRY(c, hipMemcpyAsync(sl.h_out, sl.d_out, r->out_bytes(ntrips), hipMemcpyDeviceToHost, r->copy));
    HIP_TRY(c, hipEventRecord(sl.out_ready, r->copy));
    sl.ntrips = ntrips;
    sl.busy = true;
    return MSX_OK;
}

int msx_opt_run_collect(msx_ctx *c, int32_t slot, double *records, int32_t *flags, int64_t *live, int32_t *worst_status) {
    if (!c) return MSX_ERR_INVALID;
    OptRun *r = c->opt_run;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_opt_run_collect: call msx_opt_run_begin first");
    if (slot < 0 || slot > 1 || !records || !flags || !live || !worst_status) return fail(c, MSX_ERR_INVALID, "msx_opt_run_collect: bad arguments");
    OptRun::Slot &sl = r->slot[slot];
    if (!sl.busy) return fail(c, MSX_ERR_STATE, "msx_opt_run_collect: no chunk queued in this slot");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(sl.out_ready));
    sl.busy = false;
    const double *hr = (const double *)sl.h_out;
    const int32_t *hf = (const int32_t *)(hr + r->rec_count(sl.ntrips));
    memcpy(records, hr, sizeof(double) * r->rec_count(sl.ntrips));
    memcpy(flags, hf, sizeof(int32_t) * (size_t)(sl.ntrips * r->nch));
    *live = hf[sl.ntrips * r->nch];
    *worst_status = hf[sl.ntrips * r->nch + 1];
    if (*worst_status == MSX_W_HANDOVER) c->linked_poisoned = true;
    return MSX_OK;
}

int msx_opt_run_end(msx_ctx *c, double *gi, double *chi, double *n, int64_t *total_n) {
    if (!c) return MSX_ERR_INVALID;
    OptRun *r = c->opt_run;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_opt_run_end: no run in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = hipStreamSynchronize(c->stream);
    const size_t nch = (size_t)r->nch;
    if (e == hipSuccess && gi) e = hipMemcpy(gi, r->R.gi, sizeof(double) * nch * (size_t)r->ndim, hipMemcpyDeviceToHost);
    if (e == hipSuccess && chi) e = hipMemcpy(chi, r->R.chi, sizeof(double) * nch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && n) e = hipMemcpy(n, r->R.n, sizeof(double) * nch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total_n) e = hipMemcpy(total_n, r->R.total_n, sizeof(int64_t) * nch, hipMemcpyDeviceToHost);
    opt_run_free(c);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_opt_run_end: ") + hipGetErrorString(e));
    return MSX_OK;
}

// ---- device-resident sampler, pipelined -------------------------------------------------------------------
// begin: ensemble state + two slots (device chunk buffers, pinned host staging, events).  enqueue(slot): the
// chunk's randomness goes host -> pinned -> device on the copy stream while the previous chunk's kernels run,
// its 2*nsteps fused launches go on the compute stream, its chain comes back on the copy stream.  collect(slot)
// waits for that slot only.  With two slots the compute stream never drains between chunks.
struct SamplerRun {
    int32_t mode = 0, ndim = 0;
    int64_t nw = 0, ns = 0, cap_steps = 0;
    bool failed = false;  // an enqueue returned an error after queuing part of its launches
    // sharded run (msx_sampler_shard): this rank evaluates block `rank` of every half-step's ns proposals
    bool sharded = false;
    int32_t world = 1, rank = 0;
    int64_t shard_m = 0;            // ceil(ns / world): walkers per rank, and the all-gather's count
    double *d_newlp_all = nullptr;  // [shard_m * world] gathered log p(q) of the half-step
    char *d_state = nullptr;
    double *d_coords = nullptr, *d_logp = nullptr, *d_q = nullptr, *d_newlp = nullptr;
    int64_t *d_nacc = nullptr;
    int32_t *d_wst = nullptr;
    hipStream_t copy = nullptr, up = nullptr;  // downloads / uploads: separate queues, or chunk i+1's upload
                                               // would wait behind chunk i's download (which waits for its kernels)
    // Overlapped half-steps (one GPU, a half-step that fills at most half the CUs): half-step j goes to stream j & 1
    // and starts while j - 1 is still running; its workgroups wait per walker for the versions they read (SmpRec,
    // logprob_kernel.h), the coordinates are double-buffered by version parity, and an event keeps j behind j - 3 --
    // the last launch that may still read what j overwrites (j - 2 shares j's stream).
    int overlap = -1;               // -1: decided at the first chunk; 0 / 1
    hipStream_t s2 = nullptr;
    hipEvent_t hs_done[4] = {nullptr, nullptr, nullptr, nullptr}, chunk_open = nullptr, s2_done = nullptr;
    int64_t steps_done = 0;         // iterations queued so far = every walker's version when they are done
    uint32_t *d_ver = nullptr;
    unsigned long long *d_gran = nullptr;  // [2][nw][kGranPerWalker] the hand-over's tagged granules (dev_types.h)
    struct Slot {
        char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
        hipEvent_t in_ready = nullptr, kernels_done = nullptr, out_ready = nullptr;
        int64_t nsteps = 0;
        bool busy = false;
    } slot[2];
    // The ensemble's members: the context's run has one; a target group's run (msx_group_sampler_*) one per target, their
    // walkers concatenated.  Member m owns walkers [m_off[m], m_off[m] + m_nw[m]) and entries [m_astart[m], + m_nw[m] / 2)
    // of every half-step's ns.
    std::vector<int64_t> m_nw, m_off, m_astart;
    // A chunk's arrays in its slot are laid out for `layout_steps` iterations whatever its length, or (0) for its own
    // length: the group's launches read their per-half-step pointers from snapshots built once, at begin.
    int64_t layout_steps = 0;
    int32_t nworst = 1;  // worst statuses behind a chunk's acceptance counts (the group's run: one per member)
    // the device chain series the run appends its chunks to (msx_sampler_attach_series), and the row its next chunk starts at
    struct msx_series *series = nullptr;
    int64_t series_row = 0;
    int64_t lay(int64_t st) const { return layout_steps > 0 ? layout_steps : st; }
    double *coords_now() const { return d_coords + (overlap == 1 ? (steps_done & 1) * nw * ndim : 0); }
    size_t in_bytes(int64_t st) const {  // [zz | zfac | logu | sidx | cidx | partner | records]
        return (size_t)(st * 2 * ns) * (3 * sizeof(double) + 3 * sizeof(int32_t) + sizeof(SmpRec));
    }
    size_t out_bytes(int64_t st) const {  // [chain | log p chain | acceptance counts | worst statuses (16-byte padded)]
        return sizeof(double) * (size_t)(st * nw * ndim + st * nw) + sizeof(int64_t) * (size_t)nw + 16 * (size_t)((4 * nworst + 15) / 16);
    }
};

// A series' buffer holds at least `need` rows; its first `keep` rows carry over, copied on `st` (a buffer it replaces is
// retired: freed when no run is attached).  `grown` is recorded on `st` after the copy.
static hipError_t series_reserve(msx_series *sr, int64_t need, int64_t keep, hipStream_t st) {
    if (need <= sr->cap) return hipSuccess;
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(2 * sr->cap, 256));
    double *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, sizeof(double) * (size_t)(cap * sr->nw * sr->ndim));
    if (e != hipSuccess) return e;
    if (keep > 0)
        e = hipMemcpy2DAsync(d, sizeof(double) * (size_t)cap, sr->d_rows, sizeof(double) * (size_t)sr->cap, sizeof(double) * (size_t)keep,
                             (size_t)(sr->nw * sr->ndim), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(sr->grown, st);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return e;
    }
    sr->grown_set = true;
    if (sr->d_rows) sr->retired.push_back(sr->d_rows);
    sr->d_rows = d;
    sr->cap = cap;
    return hipSuccess;
}

// the chunk's rows [nsteps][nw][ndim] at `chain` appended to the run's series, on the compute stream (before the chunk's
// kernels_done event, so a collected chunk's rows are in the series)
static hipError_t series_put_chunk(SamplerRun *r, const double *chain, int64_t nsteps, hipStream_t compute) {
    msx_series *sr = r->series;
    if (!sr) return hipSuccess;
    const int64_t row0 = r->series_row;
    hipError_t e = series_reserve(sr, row0 + nsteps, row0, compute);
    if (e != hipSuccess) return e;
    const int64_t total = nsteps * r->nw * r->ndim;
    hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, compute, chain, nsteps, r->nw,
                       (int32_t)r->ndim, sr->d_rows, sr->cap, row0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    r->series_row = row0 + nsteps;
    sr->rows = r->series_row;
    return hipSuccess;
}

// ---- the pipeline's pieces that the context's run (msx_sampler_*) and a target group's (msx_group_sampler_*) share ----
// streams, events and the two slots' buffers (cap_steps, ns, nw, ndim, layout_steps and nworst set)
static hipError_t run_open(SamplerRun *r) {
    hipError_t e = hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->s2, hipStreamNonBlocking);
    for (auto &ev : r->hs_done)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->chunk_open, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->s2_done, hipEventDisableTiming);
    for (auto &sl : r->slot) {
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_in, r->in_bytes(r->cap_steps));
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_out, r->out_bytes(r->cap_steps));
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_in, r->in_bytes(r->cap_steps), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_out, r->out_bytes(r->cap_steps), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.in_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.kernels_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.out_ready, hipEventDisableTiming);
    }
    return e;
}

// waits for what the run queued (on `compute` and its own streams) and frees it
static void run_close(SamplerRun *r, hipStream_t compute) {
    (void)hipStreamSynchronize(compute);
    if (r->copy) (void)hipStreamSynchronize(r->copy);
    if (r->up) (void)hipStreamSynchronize(r->up);
    for (auto &sl : r->slot) {
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.in_ready) (void)hipEventDestroy(sl.in_ready);
        if (sl.kernels_done) (void)hipEventDestroy(sl.kernels_done);
        if (sl.out_ready) (void)hipEventDestroy(sl.out_ready);
    }
    if (r->s2) (void)hipStreamSynchronize(r->s2);
    for (auto &ev : r->hs_done)
        if (ev) (void)hipEventDestroy(ev);
    if (r->chunk_open) (void)hipEventDestroy(r->chunk_open);
    if (r->s2_done) (void)hipEventDestroy(r->s2_done);
    if (r->s2) (void)hipStreamDestroy(r->s2);
    if (r->d_state) (void)hipFree(r->d_state);
    if (r->d_newlp_all) (void)hipFree(r->d_newlp_all);
    if (r->series) r->series->run = nullptr;  // (the series outlives the run)
    if (r->copy) (void)hipStreamDestroy(r->copy);
    if (r->up) (void)hipStreamDestroy(r->up);
    delete r;
}

// The chunk's host randomness -- [nsteps][2][ns] each, the members' active halves side by side, indices member-local --
// into the slot's pinned staging, laid out for lay(nsteps) iterations: [zz | zfac | logu | sidx | cidx | partner | records].
// Every index is dereferenced on the device: checked here.  partner is resolved to the ensemble index of the
// complementary walker, so that the kernel's proposal needs two dependent loads (record, coordinates) instead of three,
// and the records carry ensemble indices (member offset + local index).  nullptr, or what is wrong.
static const char *run_pack(SamplerRun *r, SamplerRun::Slot &sl, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                            const int32_t *partner, const double *zz, const double *zfac, const double *logu) {
    const int64_t ns = r->ns, nh = nsteps * 2 * ns, L = r->lay(nsteps) * 2 * ns;
    const size_t km = r->m_nw.size();
    // pinned staging, doubles first
    double *hz = (double *)sl.h_in;
    int32_t *hi = (int32_t *)(hz + 3 * L);
    memcpy(hz, zz, sizeof(double) * nh); memcpy(hz + L, zfac, sizeof(double) * nh); memcpy(hz + 2 * L, logu, sizeof(double) * nh);
    memcpy(hi, sidx, sizeof(int32_t) * nh); memcpy(hi + L, cidx, sizeof(int32_t) * nh);
    memcpy(hi + 2 * L, partner, sizeof(int32_t) * nh);
    for (int64_t row = 0; row < 2 * nsteps; ++row)
        for (size_t m = 0; m < km; ++m) {
            const int64_t b = row * ns + r->m_astart[m];
            const uint32_t mw = (uint32_t)r->m_nw[m], mh = mw / 2;
            for (int64_t j = b; j < b + (int64_t)mh; ++j)
                if ((uint32_t)hi[j] >= mw || (uint32_t)hi[L + j] >= mw || (uint32_t)hi[2 * L + j] >= mh)
                    return "walker / partner index out of range";
        }
    for (int64_t row = 0; row < 2 * nsteps; ++row)
        for (size_t m = 0; m < km; ++m) {
            const int64_t b = row * ns + r->m_astart[m], e = b + r->m_nw[m] / 2, off = r->m_off[m];
            for (int64_t j = b; j < e; ++j) hi[2 * L + j] = (int32_t)(off + hi[L + b + hi[2 * L + j]]);
        }
    if (r->overlap == 1) {
        // the version protocol rests on every walker moving exactly once per iteration: the two half-steps' walkers must
        // be a permutation of the ensemble (emcee's random split is; checked here because a violation would not fail
        // until a workgroup's wait runs out on the device).  (The context's run only: one member, L = nh.)
        std::vector<int64_t> seen((size_t)r->nw, -1);
        for (int64_t i = 0; i < nh; ++i) {
            const int64_t it = i / (2 * ns);
            if (seen[(size_t)hi[i]] == it) return "a walker appears twice in one iteration's two half-steps";
            seen[(size_t)hi[i]] = it;
        }
    }
    // ... and the proposal's inputs once more as one record per walker (the kernel's first load), with the versions of
    // the two walkers the move reads: before iteration k every walker has version k; the second half-step's partners
    // were updated by the first
    SmpRec *hr = (SmpRec *)(hi + 3 * L);
    for (int64_t row = 0; row < 2 * nsteps; ++row)
        for (size_t m = 0; m < km; ++m) {
            const int64_t b = row * ns + r->m_astart[m], e = b + r->m_nw[m] / 2, off = r->m_off[m];
            const int64_t k = r->steps_done + row / 2, half = row & 1;
            for (int64_t i = b; i < e; ++i) {
                hr[i].si = (int32_t)(off + hi[i]); hr[i].ci = hi[2 * L + i]; hr[i].zz = hz[i];
                hr[i].ver_own = r->overlap == 1 ? (uint32_t)k : 0u;
                hr[i].ver_partner = r->overlap == 1 ? (uint32_t)(k + half) : 0u;
            }
        }
    return nullptr;
}

// the packed slot up on the upload stream; `compute` waits for it
static hipError_t run_upload(SamplerRun *r, SamplerRun::Slot &sl, int64_t nsteps, hipStream_t compute) {
    hipError_t e = hipMemcpyAsync(sl.d_in, sl.h_in, r->in_bytes(r->lay(nsteps)), hipMemcpyHostToDevice, r->up);
    if (e == hipSuccess) e = hipEventRecord(sl.in_ready, r->up);
    if (e == hipSuccess) e = hipStreamWaitEvent(compute, sl.in_ready, 0);
    return e;
}

// begin: the run's initial state up on `s` -- coordinates, log p and the acceptance counts (naccept, or zeros) -- and `s`
// synchronised, so the caller's arrays are consumed on return
static hipError_t run_load_state(SamplerRun *r, hipStream_t s, const double *coords, const double *logp, const int64_t *naccept) {
    hipError_t e = hipMemcpyAsync(r->d_coords, coords, sizeof(double) * r->nw * r->ndim, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_logp, logp, sizeof(double) * r->nw, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = naccept ? hipMemcpyAsync(r->d_nacc, naccept, sizeof(int64_t) * r->nw, hipMemcpyHostToDevice, s)
                    : hipMemsetAsync(r->d_nacc, 0, sizeof(int64_t) * r->nw, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

static void sampler_free(msx_ctx *c) {
    SamplerRun *r = c->smp;
    if (!r) return;
    (void)hipSetDevice(c->device);
    run_close(r, c->stream);
    c->smp = nullptr;
    c->P.smp_on = 0;
    c->P.smp_defer = 0;
    c->P.smp_overlap = 0;
    c->smp_overlap_launch = false;
}

int msx_sampler_begin(msx_ctx *c, int32_t mode, int64_t nw, int32_t ndim, int64_t max_chunk_steps, const double *coords,
                      const double *logp, const int64_t *naccept) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_sampler_begin: no problem staged");
    if (!coords || !logp || nw < 2 || (nw & 1) || max_chunk_steps < 1)
        return fail(c, MSX_ERR_INVALID, "msx_sampler_begin: bad arguments (need an even number of walkers)");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, "P0 doesn't match what I was expecting");
    if (mode != MSX_MODE_LOGPOST && mode != MSX_MODE_LOGLIKE) return fail(c, MSX_ERR_INVALID, "msx_sampler_begin: bad mode");
    if (c->tmp) return fail(c, MSX_ERR_STATE, "msx_sampler_begin: a tempered run is in flight on this context (msx_tempered_end)");
    HIP_TRY(c, hipSetDevice(c->device));
    sampler_free(c);
    SamplerRun *r = new SamplerRun;
    c->smp = r;
    r->mode = mode; r->ndim = ndim; r->nw = nw; r->ns = nw / 2; r->cap_steps = max_chunk_steps;
    r->m_nw = {nw}; r->m_off = {0}; r->m_astart = {0};
    const int64_t ns = r->ns;
    // (two coordinate buffers, two half-steps' worth of per-launch outputs: overlapped half-steps)
    const size_t gran_words = (size_t)(2 * nw * kGranPerWalker);
    std::vector<unsigned long long> hg;  // (lives until the stream has been synchronised below)
    const size_t state_bytes = sizeof(double) * (size_t)(2 * nw * ndim + nw + 2 * ns * ndim + 2 * ns) + sizeof(int64_t) * (size_t)nw +
                               sizeof(int32_t) * (size_t)(2 * ns) + sizeof(uint32_t) * (size_t)nw + 64 + sizeof(unsigned long long) * gran_words;
    hipError_t e = hipMalloc((void **)&r->d_state, state_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_state, 0, state_bytes, c->stream);
    if (e == hipSuccess) e = run_open(r);
    if (e == hipSuccess) {
        r->d_coords = (double *)r->d_state; r->d_logp = r->d_coords + 2 * nw * ndim; r->d_q = r->d_logp + nw;
        r->d_newlp = r->d_q + 2 * ns * ndim; r->d_nacc = (int64_t *)(r->d_newlp + 2 * ns); r->d_wst = (int32_t *)(r->d_nacc + nw);
        r->d_ver = (uint32_t *)(r->d_wst + 2 * ns);
        r->d_gran = (unsigned long long *)(((uintptr_t)(r->d_ver + nw) + 15) & ~(uintptr_t)15);

        // the granules of version 0 (buffer 0); buffer 1 carries a version nobody asks for until it is written
        hg.assign(gran_words, granule(0u, 0xffffffffu));
        for (int64_t w = 0; w < nw; ++w) {
            unsigned long long *g = hg.data() + (size_t)w * kGranPerWalker;
            for (int d = 0; d < ndim; ++d) {
                unsigned long long b;
                memcpy(&b, &coords[w * ndim + d], 8);
                g[2 * d] = granule((unsigned int)(b >> 32), 0u);
                g[2 * d + 1] = granule((unsigned int)b, 0u);
            }
            unsigned long long lb;
            memcpy(&lb, &logp[w], 8);
            g[kGranLogp] = granule((unsigned int)(lb >> 32), 0u);
            g[kGranLogp + 1] = granule((unsigned int)lb, 0u);
            g[kGranNacc] = granule((unsigned int)(naccept ? naccept[w] : 0), 0u);
        }
        e = hipMemcpyAsync(r->d_gran, hg.data(), sizeof(unsigned long long) * gran_words, hipMemcpyHostToDevice, c->stream);  // (behind the memset)
    }
    if (e == hipSuccess) e = run_load_state(r, c->stream, coords, logp, naccept);
    if (e != hipSuccess) {
        sampler_free(c);
        return fail(c, MSX_ERR_HIP, std::string("msx_sampler_begin: ") + hipGetErrorString(e));
    }
    return MSX_OK;
}

int msx_sampler_shard(msx_ctx *c, int32_t rank, int32_t world) {
    if (!c) return MSX_ERR_INVALID;
    SamplerRun *r = c->smp;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_sampler_shard: call msx_sampler_begin first");
    if (world < 1 || rank < 0 || rank >= world) return fail(c, MSX_ERR_INVALID, "msx_sampler_shard: bad rank / world");
    const bool have_comm = c->rccl_comm || !c->loop_peers.empty();
    if (world > 1 && (!have_comm || c->comm_world != world || c->comm_rank != rank))
        return fail(c, MSX_ERR_STATE, "msx_sampler_shard: msx_comm_init(rank, world) or msx_comm_init_loopback must come first");
    for (auto &sl : r->slot)
        if (sl.busy) return fail(c, MSX_ERR_STATE, "msx_sampler_shard: chunks are already in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    r->world = world; r->rank = rank;
    r->shard_m = (r->ns + world - 1) / world;
    if (r->d_newlp_all) (void)hipFree(r->d_newlp_all);
    r->d_newlp_all = nullptr;
    HIP_TRY(c, hipMalloc((void **)&r->d_newlp_all, sizeof(double) * (size_t)(r->shard_m * world)));
    HIP_TRY(c, hipMemset(r->d_newlp_all, 0, sizeof(double) * (size_t)(r->shard_m * world)));
    r->sharded = true;
    return MSX_OK;
}

// ---- one chunk of the device-resident sampler, in pieces ------------------------------------------------------
// msx_sampler_enqueue = prepare; { eval; gather; apply } per half-step; finish.  The loopback group's entry point
// (msx_sampler_enqueue_group) runs the same pieces for all its ranks in lock-step, with device copies for the gather.
struct ChunkPtrs {
    int64_t nh = 0;
    double *d_zz = nullptr, *d_zfac = nullptr, *d_logu = nullptr;
    int32_t *d_sidx = nullptr, *d_cidx = nullptr, *d_partner = nullptr;
    const SmpRec *d_rec = nullptr;
    double *d_chain = nullptr, *d_lpchain = nullptr;
    int64_t *d_nacc_snap = nullptr;
    int32_t *d_worst = nullptr;
};

// where a chunk of nsteps iterations lives in its slot (SamplerRun::lay)
static void run_chunk_ptrs(const SamplerRun *r, const SamplerRun::Slot &sl, int64_t nsteps, ChunkPtrs *cp) {
    const int64_t L = r->lay(nsteps), nh = L * 2 * r->ns;
    cp->nh = nsteps * 2 * r->ns;
    cp->d_zz = (double *)sl.d_in; cp->d_zfac = cp->d_zz + nh; cp->d_logu = cp->d_zfac + nh;
    cp->d_sidx = (int32_t *)(cp->d_logu + nh); cp->d_cidx = cp->d_sidx + nh; cp->d_partner = cp->d_cidx + nh;
    cp->d_rec = (const SmpRec *)(cp->d_partner + nh);
    cp->d_chain = (double *)sl.d_out; cp->d_lpchain = cp->d_chain + L * r->nw * r->ndim;
    cp->d_nacc_snap = (int64_t *)(cp->d_lpchain + L * r->nw);
    cp->d_worst = (int32_t *)(cp->d_nacc_snap + r->nw);
}

// the chunk's launches are queued on `compute`: snapshot the acceptance counters behind them, then bring the slot's
// results back on the download stream
static hipError_t run_finish(SamplerRun *r, int32_t slot, int64_t nsteps, const ChunkPtrs &cp, hipStream_t compute) {
    SamplerRun::Slot &sl = r->slot[slot];
    // the chunk's rows into the attached series, then: acceptance counters keep running while this chunk's results
    // travel -- snapshot them in stream order
    hipError_t e = series_put_chunk(r, cp.d_chain, nsteps, compute);
    if (e == hipSuccess) e = hipMemcpyAsync(cp.d_nacc_snap, r->d_nacc, sizeof(int64_t) * r->nw, hipMemcpyDeviceToDevice, compute);
    if (e == hipSuccess) e = hipEventRecord(sl.kernels_done, compute);
    if (e == hipSuccess) e = hipStreamWaitEvent(r->copy, sl.kernels_done, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_out, sl.d_out, r->out_bytes(r->lay(nsteps)), hipMemcpyDeviceToHost, r->copy);
    if (e == hipSuccess) e = hipEventRecord(sl.out_ready, r->copy);
    if (e != hipSuccess) return e;
    sl.nsteps = nsteps;
    sl.busy = true;
    return hipSuccess;
}

// waits for the slot's results and copies them out: chain [nsteps][nw][ndim], log p [nsteps][nw], naccept [nw], worst [nworst]
static hipError_t run_collect(SamplerRun *r, int32_t slot, double *chain_out, double *logp_out, int64_t *naccept, int32_t *worst) {
    SamplerRun::Slot &sl = r->slot[slot];
    const hipError_t e = hipEventSynchronize(sl.out_ready);
    if (e != hipSuccess) return e;
    const int64_t st = sl.nsteps, nw = r->nw, L = r->lay(st);
    const double *h_chain = (const double *)sl.h_out, *h_lp = h_chain + L * nw * r->ndim;
    const int64_t *h_nacc = (const int64_t *)(h_lp + L * nw);
    memcpy(chain_out, h_chain, sizeof(double) * st * nw * r->ndim);
    memcpy(logp_out, h_lp, sizeof(double) * st * nw);
    memcpy(naccept, h_nacc, sizeof(int64_t) * nw);
    memcpy(worst, h_nacc + nw, sizeof(int32_t) * r->nworst);
    sl.busy = false;
    return hipSuccess;
}

// The checks of an enqueue, in order: a run in flight, the slot and chunk length (args_ok: the caller's arrays), a run
// that failed part-way, a slot not collected yet.  MSX_OK, or the code with *err set.  who / begin / end: the entry point
// and its family's begin and end.
static int run_enqueue_check(std::string *err, const SamplerRun *r, const char *who, const char *begin, const char *end, int32_t slot,
                             int64_t nsteps, bool args_ok) {
    const std::string w(who);
    int code = MSX_OK;
    if (!r) { code = MSX_ERR_STATE; *err = w + ": call " + begin + " first"; }
    else if (slot < 0 || slot > 1 || nsteps < 1 || nsteps > r->cap_steps || !args_ok) { code = MSX_ERR_INVALID; *err = w + ": bad arguments"; }
    else if (r->failed) { code = MSX_ERR_STATE; *err = w + ": an earlier enqueue failed part-way; end this run (" + end + ") and begin again"; }
    else if (r->slot[slot].busy) { code = MSX_ERR_STATE; *err = w + ": slot not collected yet"; }
    return code;
}

// msx_sampler_collect / msx_group_sampler_collect: the checks, then the slot's results (run_collect)
static int run_collect_checked(std::string *err, SamplerRun *r, const char *who, const char *begin, int32_t slot, double *chain_out,
                               double *logp_out, int64_t *naccept, int32_t *worst) {
    const std::string w(who);
    if (!r) { *err = w + ": call " + begin + " first"; return MSX_ERR_STATE; }
    if (slot < 0 || slot > 1 || !chain_out || !logp_out || !naccept || !worst) { *err = w + ": bad arguments"; return MSX_ERR_INVALID; }
    if (!r->slot[slot].busy) { *err = w + ": nothing enqueued in this slot"; return MSX_ERR_STATE; }
    const hipError_t e = run_collect(r, slot, chain_out, logp_out, naccept, worst);
    if (e != hipSuccess) { *err = w + ": " + hipGetErrorString(e); return MSX_ERR_HIP; }
    return MSX_OK;
}

// end: everything the run queued on `compute` (and its second stream) done, then its state down (coords / logp: nullptr
// for none).  The caller frees the run.
static hipError_t run_save_state(const SamplerRun *r, int device, hipStream_t compute, double *coords, double *logp) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamSynchronize(compute);
    if (e == hipSuccess && r->s2) e = hipStreamSynchronize(r->s2);
    if (e == hipSuccess && coords) e = hipMemcpy(coords, r->coords_now(), sizeof(double) * r->nw * r->ndim, hipMemcpyDeviceToHost);
    if (e == hipSuccess && logp) e = hipMemcpy(logp, r->d_logp, sizeof(double) * r->nw, hipMemcpyDeviceToHost);
    return e;
}

// (draw != nullptr: the chunk's randomness is drawn on the device -- sampler_draw_kernel, keyed by draw->seed and the
// stream's ABSOLUTE iteration numbers from draw->first_iter, which the caller carries across runs -- instead of coming from
// the host's arrays.  The records' versions stay the RUN's: r->steps_done, as run_pack counts them.)
struct DeviceDraw { unsigned long long seed; double a; int64_t first_iter; };
static int chunk_prepare(msx_ctx *c, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                         const int32_t *partner, const double *zz, const double *zfac, const double *logu, ChunkPtrs *cp,
                         const DeviceDraw *draw = nullptr) {
    SamplerRun *r = c->smp;
    if (int rc = run_enqueue_check(&c->err, r, "msx_sampler_enqueue", "msx_sampler_begin", "msx_sampler_end", slot, nsteps,
                                   draw || (sidx && cidx && partner && zz && zfac && logu)))
        return rc;
    if (draw && (r->nw > kDrawMaxWalkers || !(draw->a > 1.0) || draw->first_iter < 0))
        return fail(c, MSX_ERR_INVALID, "msx_sampler_enqueue_drawn: the device generator takes up to 4096 walkers, a stretch scale a > 1 and a first iteration >= 0");
    SamplerRun::Slot &sl = r->slot[slot];
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t ns = r->ns, nw = r->nw, nh = nsteps * 2 * ns;
    const int ndim = r->ndim;
    // Overlapped half-steps?  Decided once per run, here (sharding is set up after msx_sampler_begin): an unsharded run
    // whose half-step takes the fused kernel (one workgroup per walker) and fills at most HALF the CUs -- two half-steps
    // are resident together, and a workgroup that waits for a walker of the half-step before it must never keep that
    // walker's workgroup off the chip.  MSX_SMP_OVERLAP=0 in the environment: never.
    if (r->overlap < 0) {
        const int64_t cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
        const char *e = getenv("MSX_SMP_OVERLAP");
        // (Not on a context that holds a communicator: RCCL's kernels take CUs this rule counts on.  Two half-steps of
        // config 2's ensemble need every CU of the chip -- one workgroup each -- so anything else resident on the device
        // (another process, another context's launches) can keep a waiting workgroup's producer off the chip: the wait is
        // bounded, the chunk then ends with MSX_W_HANDOVER and the run is lost -- msx_sampler_policy(ctx, 0) or
        // MSX_SMP_OVERLAP=0 gives the plain launches on a device that is shared.)
        r->overlap = !(e && e[0] == '0') && c->smp_overlap_policy != 0 && !r->sharded && !c->rccl_comm && c->loop_peers.empty() &&
                     2 * ns <= cus && !c->model_in_global && c->recipe_fast &&
                     c->path != MSX_PATH_LINKED && c->path != MSX_PATH_PAIR && !auto_takes_linked(c, ns);
    }
    if (draw) {
        // the chunk's arrays, written where the host-fed path uploads them: [zz | zfac | logu | sidx | cidx | partner | records]
        double *g_zz = (double *)sl.d_in, *g_zfac = g_zz + nh, *g_logu = g_zfac + nh;
        int32_t *g_sidx = (int32_t *)(g_logu + nh), *g_cidx = g_sidx + nh, *g_partner = g_cidx + nh;
        SmpRec *g_rec = (SmpRec *)(g_partner + nh);
        hipLaunchKernelGGL(sampler_draw_kernel, dim3((unsigned)nsteps), dim3(kDrawThreads), 0, c->stream, draw->seed, draw->a, draw->first_iter,
                           r->steps_done, nw, (int32_t)ndim, 1, (int32_t)(r->overlap == 1), g_sidx, g_cidx, g_partner, g_zz, g_zfac, g_logu, g_rec);
        HIP_TRY(c, hipGetLastError());
    } else {
        if (const char *why = run_pack(r, sl, nsteps, sidx, cidx, partner, zz, zfac, logu))
            return fail(c, MSX_ERR_INVALID, std::string("msx_sampler_enqueue: ") + why);
        HIP_TRY(c, run_upload(r, sl, nsteps, c->stream));
    }
    run_chunk_ptrs(r, sl, nsteps, cp);
    HIP_TRY(c, hipMemsetAsync(cp->d_worst, 0, sizeof(int32_t) * r->nworst, c->stream));
    DevProblem &P = c->P;
    P.smp_on = 1;
    P.smp_coords = r->d_coords; P.smp_logp = r->d_logp; P.smp_q = r->d_q; P.smp_naccept = r->d_nacc; P.smp_worst = cp->d_worst;
    P.smp_overlap = r->overlap == 1; P.smp_stride = nw * ndim; P.smp_ver = r->d_ver;
    P.smp_gran = r->d_gran; P.smp_gwalkers = nw;
    if (r->overlap == 1) {  // the second stream's launches of this chunk come after the chunk's inputs and the cleared status
        HIP_TRY(c, hipEventRecord(r->chunk_open, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(r->s2, r->chunk_open, 0));
    }
    return MSX_OK;
}

// the half-step's pointers; then this rank's evaluation: the whole half-step fused (unsharded), or log p(q) of its
// block of the proposals only, accept deferred (sharded)
static int chunk_half_eval(msx_ctx *c, const ChunkPtrs &cp, int64_t st, int half) {
    SamplerRun *r = c->smp;
    DevProblem &P = c->P;
    const int64_t ns = r->ns, nw = r->nw;
    const int ndim = r->ndim;
    const int64_t off = (st * 2 + half) * ns;
    P.smp_sidx = cp.d_sidx + off; P.smp_cidx = cp.d_cidx + off; P.smp_partner = cp.d_partner + off;
    P.smp_zz = cp.d_zz + off; P.smp_zfac = cp.d_zfac + off; P.smp_logu = cp.d_logu + off; P.smp_rec = cp.d_rec + off;
    P.smp_chain_row = cp.d_chain + st * nw * ndim; P.smp_lp_row = cp.d_lpchain + st * nw;
    if (r->overlap == 1) {
        // half-step j on stream j & 1, behind j - 3 (see SamplerRun); per-launch outputs nobody reads go to the
        // stream's own half of their arrays
        const int64_t j = (r->steps_done + st) * 2 + half;
        hipStream_t s = (j & 1) ? r->s2 : c->stream;
        if (j >= 3) HIP_TRY(c, hipStreamWaitEvent(s, r->hs_done[(j - 3) & 3], 0));
        P.smp_q = r->d_q + (j & 1) * ns * ndim;
        c->smp_overlap_launch = true;
        const int rc = msx_logprob_batch_dev(c, r->mode, P.smp_q, ns, ndim, r->d_newlp + (j & 1) * ns, r->d_wst + (j & 1) * ns, s, 0);
        c->smp_overlap_launch = false;
        if (rc != MSX_OK) return rc;
        HIP_TRY(c, hipEventRecord(r->hs_done[j & 3], s));
        return MSX_OK;
    }
    if (!r->sharded) return msx_logprob_batch_dev(c, r->mode, r->d_q, ns, ndim, r->d_newlp, r->d_wst, c->stream, 0);
    // sharded: (1) this rank's block of proposals -> log p(q) only; (2) ONE all-gather of shard_m float64 per rank, in
    // place in the gathered vector; (3) every rank finishes the half-step for all ns walkers
    const int64_t lo = std::min<int64_t>(r->rank * r->shard_m, ns), hi = std::min<int64_t>(lo + r->shard_m, ns);
    int rc = MSX_OK;
    if (hi > lo) {
        const DevProblem keep = P;
        P.smp_defer = 1;
        P.smp_sidx += lo; P.smp_cidx += lo; P.smp_partner += lo; P.smp_zz += lo; P.smp_zfac += lo; P.smp_logu += lo;
        P.smp_rec += lo;
        P.smp_q = r->d_q + lo * ndim;
        rc = msx_logprob_batch_dev(c, r->mode, r->d_q + lo * ndim, hi - lo, ndim, r->d_newlp_all + lo, r->d_wst + lo, c->stream, 0);
        P = keep;
    }
    return rc;
}

static int chunk_half_gather_rccl(msx_ctx *c) {
    SamplerRun *r = c->smp;
    if (!(c->rccl_comm && c->comm_world == r->world)) return MSX_OK;  // (world 1 without a communicator: nothing to do)
    // (a one-rank communicator still runs the collective)
    const int nrc = rccl().AllGather(r->d_newlp_all + r->rank * r->shard_m, r->d_newlp_all, (size_t)r->shard_m, kNcclFloat64,
                                     c->rccl_comm, c->stream);
    if (nrc != 0) return fail(c, MSX_ERR_HIP, std::string("ncclAllGather: ") + rccl().GetErrorString(nrc));
    return MSX_OK;
}

static int chunk_half_apply(msx_ctx *c) {
    SamplerRun *r = c->smp;
    if (!r->sharded) return MSX_OK;
    hipLaunchKernelGGL(sampler_apply_kernel, dim3((unsigned)((r->ns + 255) / 256)), dim3(256), 0, c->stream, c->P,
                       r->d_newlp_all, r->ns, r->ndim);
    if (hipGetLastError() != hipSuccess) return fail(c, MSX_ERR_HIP, "sampler_apply_kernel launch failed");
    return MSX_OK;
}

static int chunk_finish(msx_ctx *c, int32_t slot, int64_t nsteps, const ChunkPtrs &cp, int rc) {
    SamplerRun *r = c->smp;
    DevProblem &P = c->P;
    P.smp_on = 0;
    P.smp_defer = 0;
    if (rc != MSX_OK) {
        // some of this chunk's half-steps may already be queued: the resident state is no longer the state any
        // host-side bookkeeping expects.  Refuse everything but msx_sampler_end from here on.
        r->failed = true;
        return rc;
    }
    if (r->overlap == 1) {  // the chunk's last half-step ran on the second stream
        HIP_TRY(c, hipEventRecord(r->s2_done, r->s2));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, r->s2_done, 0));
    }
    r->steps_done += nsteps;
    HIP_TRY(c, run_finish(r, slot, nsteps, cp, c->stream));
    return MSX_OK;
}

// msx_sampler_enqueue (draw = nullptr) and msx_sampler_enqueue_drawn
static int sampler_enqueue(msx_ctx *c, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                           const int32_t *partner, const double *zz, const double *zfac, const double *logu, const DeviceDraw *draw) {
    if (!c) return MSX_ERR_INVALID;
    if (c->smp && c->smp->sharded && c->smp->world > 1) {
        if (!c->loop_peers.empty())
            return fail(c, MSX_ERR_STATE, std::string(who) + ": the ranks of a loopback group advance together (msx_sampler_enqueue_group)");
        if (!c->rccl_comm || c->comm_world != c->smp->world)
            return fail(c, MSX_ERR_STATE, std::string(who) + ": the run is sharded over a communicator that no longer exists");
    }
    ChunkPtrs cp;
    int rc = chunk_prepare(c, slot, nsteps, sidx, cidx, partner, zz, zfac, logu, &cp, draw);
    if (rc != MSX_OK) return rc;
    for (int64_t st = 0; st < nsteps && rc == MSX_OK; ++st)
        for (int half = 0; half < 2 && rc == MSX_OK; ++half) {
            rc = chunk_half_eval(c, cp, st, half);
            if (rc == MSX_OK && c->smp->sharded) rc = chunk_half_gather_rccl(c);
            if (rc == MSX_OK) rc = chunk_half_apply(c);
        }
    return chunk_finish(c, slot, nsteps, cp, rc);
}

int msx_sampler_enqueue(msx_ctx *c, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                        const int32_t *partner, const double *zz, const double *zfac, const double *logu) {
    return sampler_enqueue(c, "msx_sampler_enqueue", slot, nsteps, sidx, cidx, partner, zz, zfac, logu, nullptr);
}

int msx_sampler_enqueue_drawn(msx_ctx *c, int32_t slot, int64_t nsteps, uint64_t seed, double a, int64_t first_iter) {
    const DeviceDraw dd = {(unsigned long long)seed, a, first_iter};
    return sampler_enqueue(c, "msx_sampler_enqueue_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &dd);
}

int msx_sampler_draw(msx_ctx *c, uint64_t seed, double a, int64_t first_iter, int64_t nsteps, int64_t nw, int32_t ndim,
                     int32_t *sidx, int32_t *cidx, int32_t *partner, double *zz, double *zfac, double *logu) {
    if (!c || !sidx || !cidx || !partner || !zz || !zfac || !logu || nsteps < 1 || nw < 2 || (nw & 1) || nw > kDrawMaxWalkers ||
        first_iter < 0 || ndim < 1 || !(a > 1.0))
        return fail(c, MSX_ERR_INVALID, "msx_sampler_draw: bad arguments (an even number of walkers, at most 4096; a > 1)");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t nh = nsteps * nw;
    char *d = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d, (size_t)nh * (3 * sizeof(double) + 3 * sizeof(int32_t))));
    double *g_zz = (double *)d, *g_zfac = g_zz + nh, *g_logu = g_zfac + nh;
    int32_t *g_sidx = (int32_t *)(g_logu + nh), *g_cidx = g_sidx + nh, *g_partner = g_cidx + nh;
    hipLaunchKernelGGL(sampler_draw_kernel, dim3((unsigned)nsteps), dim3(kDrawThreads), 0, c->stream, (unsigned long long)seed, a, first_iter,
                       (int64_t)0, nw, ndim, 0, 0, g_sidx, g_cidx, g_partner, g_zz, g_zfac, g_logu, (SmpRec *)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(zz, g_zz, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(zfac, g_zfac, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(logu, g_logu, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sidx, g_sidx, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cidx, g_cidx, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(partner, g_partner, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_sampler_draw: ") + hipGetErrorString(e));
    return MSX_OK;
}

int msx_sampler_enqueue_group(msx_ctx **ctxs, int32_t world, int32_t slot, int64_t nsteps, const int32_t *sidx,
                              const int32_t *cidx, const int32_t *partner, const double *zz, const double *zfac,
                              const double *logu) {
    if (!ctxs || world < 1 || !ctxs[0]) return MSX_ERR_INVALID;
    msx_ctx *c0 = ctxs[0];
    for (int r = 0; r < world; ++r) {
        msx_ctx *c = ctxs[r];
        if (!c || (int)c->loop_peers.size() != world || c->loop_peers[(size_t)r] != c || c->comm_rank != r)
            return fail(c0, MSX_ERR_STATE, "msx_sampler_enqueue_group: the contexts are not the ranks 0..world-1 of one loopback group");
        if (!c->smp || !c->smp->sharded || c->smp->world != world || c->smp->rank != r)
            return fail(c0, MSX_ERR_STATE, "msx_sampler_enqueue_group: every rank needs msx_sampler_begin + msx_sampler_shard(rank, world) first");
        if (c->smp->ns != c0->smp->ns || c->smp->ndim != c0->smp->ndim)
            return fail(c0, MSX_ERR_STATE, "msx_sampler_enqueue_group: the ranks hold different ensembles");
    }
    std::vector<ChunkPtrs> cp((size_t)world);
    std::vector<int> rcs((size_t)world, MSX_OK);
    int rc = MSX_OK;
    for (int r = 0; r < world && rc == MSX_OK; ++r)   // every rank is fed the same randomness
        rc = rcs[(size_t)r] = chunk_prepare(ctxs[r], slot, nsteps, sidx, cidx, partner, zz, zfac, logu, &cp[(size_t)r]);
    if (rc != MSX_OK) {  // nothing is queued yet on the ranks after the failing one; the prepared ones are unwound
        for (int r = 0; r < world; ++r) { ctxs[r]->P.smp_on = 0; ctxs[r]->P.smp_defer = 0; }
        if (ctxs[0] != c0 || c0->err.empty()) c0->err = "msx_sampler_enqueue_group: a rank refused the chunk";
        return rc;
    }
    const int64_t m = c0->smp->shard_m;
    for (int64_t st = 0; st < nsteps && rc == MSX_OK; ++st)
        for (int half = 0; half < 2 && rc == MSX_OK; ++half) {
            // (1) every rank evaluates its block into its own gathered vector -- once the peers have taken the
            //     previous half-step's block out of it
            for (int r = 0; r < world && rc == MSX_OK; ++r) {
                msx_ctx *c = ctxs[r];
                for (int p = 0; p < world; ++p)
                    if (p != r && hipStreamWaitEvent(c->stream, ctxs[p]->loop_copied, 0) != hipSuccess) rc = fail(c0, MSX_ERR_HIP, "loopback: hipStreamWaitEvent");
                if (rc == MSX_OK) rc = chunk_half_eval(c, cp[(size_t)r], st, half);
                if (rc == MSX_OK && hipEventRecord(c->loop_eval_done, c->stream) != hipSuccess) rc = fail(c0, MSX_ERR_HIP, "loopback: hipEventRecord");
            }
            // (2) the all-gather: rank r copies block p out of rank p's vector, in place at p * m; (3) apply
            for (int r = 0; r < world && rc == MSX_OK; ++r) {
                msx_ctx *c = ctxs[r];
                for (int p = 0; p < world && rc == MSX_OK; ++p) {
                    if (p == r) continue;
                    hipError_t e = hipStreamWaitEvent(c->stream, ctxs[p]->loop_eval_done, 0);
                    if (e == hipSuccess)
                        e = hipMemcpyAsync(c->smp->d_newlp_all + p * m, ctxs[p]->smp->d_newlp_all + p * m, sizeof(double) * (size_t)m,
                                           hipMemcpyDeviceToDevice, c->stream);
                    if (e != hipSuccess) rc = fail(c0, MSX_ERR_HIP, std::string("loopback all-gather: ") + hipGetErrorString(e));
                }
                if (rc == MSX_OK && hipEventRecord(c->loop_copied, c->stream) != hipSuccess) rc = fail(c0, MSX_ERR_HIP, "loopback: hipEventRecord");
                if (rc == MSX_OK) rc = chunk_half_apply(c);
            }
        }
    int out = rc;
    for (int r = 0; r < world; ++r) {
        const int f = chunk_finish(ctxs[r], slot, nsteps, cp[(size_t)r], rc);
        if (out == MSX_OK) out = f;
    }
    return out;
}

int msx_sampler_collect(msx_ctx *c, int32_t slot, double *chain_out, double *logp_out, int64_t *naccept,
                        int32_t *worst_status) {
    if (!c) return MSX_ERR_INVALID;
    return run_collect_checked(&c->err, c->smp, "msx_sampler_collect", "msx_sampler_begin", slot, chain_out, logp_out, naccept, worst_status);
}

int msx_sampler_end(msx_ctx *c, double *coords, double *logp) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->smp) return MSX_OK;
    const hipError_t e = run_save_state(c->smp, c->device, c->stream, coords, logp);
    sampler_free(c);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_sampler_end: ") + hipGetErrorString(e));
    return MSX_OK;
}

int msx_sampler_policy(msx_ctx *c, int32_t overlap) {
    if (!c || (overlap != -1 && overlap != 0)) return fail(c, MSX_ERR_INVALID, "msx_sampler_policy: -1 (automatic) or 0 (never overlap half-steps)");
    c->smp_overlap_policy = overlap;
    return MSX_OK;
}

int msx_sampler_overlapped(msx_ctx *c, int32_t *out) {
    if (!c || !out) return MSX_ERR_INVALID;
    if (!c->smp) return fail(c, MSX_ERR_STATE, "msx_sampler_overlapped: call msx_sampler_begin first");
    *out = c->smp->overlap;
    return MSX_OK;
}

// one synchronous chunk (the pipelined entry points above, used back to back)
int msx_sampler_run(msx_ctx *c, int32_t mode, int64_t nw, int32_t ndim, int64_t nsteps, double *coords, double *logp,
                    const int32_t *sidx, const int32_t *cidx, const int32_t *partner, const double *zz,
                    const double *zfac, const double *logu, double *chain_out, double *logp_out, int64_t *naccept,
                    int32_t *worst_status) {
    if (!c) return MSX_ERR_INVALID;
    if (!coords || !logp || !chain_out || !logp_out || !naccept || !worst_status || nsteps < 1)
        return fail(c, MSX_ERR_INVALID, "msx_sampler_run: bad arguments (need an even number of walkers)");
    int rc = msx_sampler_begin(c, mode, nw, ndim, nsteps, coords, logp, naccept);
    if (rc == MSX_OK) rc = msx_sampler_enqueue(c, 0, nsteps, sidx, cidx, partner, zz, zfac, logu);
    if (rc == MSX_OK) rc = msx_sampler_collect(c, 0, chain_out, logp_out, naccept, worst_status);
    if (rc == MSX_OK) return msx_sampler_end(c, coords, logp);
    const std::string keep = c->err;
    sampler_free(c);
    c->err = keep;
    return rc;
}

int msx_make_composite(msx_ctx *c, const double *teff, const double *logg, const double *rad, int32_t use_distance,
                       double plx, double *spec_out, double *contrast_out, double *phot_out, int32_t *status_out) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_make_composite: no problem staged");
    if (!teff || !logg || !rad || !spec_out || !status_out) return fail(c, MSX_ERR_INVALID, "msx_make_composite: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    const int ns = c->P.nspec;
    double args[3 * MSX_MAX_SPEC + 1];
    for (int i = 0; i < ns; ++i) { args[i] = teff[i]; args[ns + i] = logg[i]; args[2 * ns + i] = rad[i]; }
    args[3 * ns] = plx;
    if (c->P.win_n > c->cap_spec) {
        if (c->d_spec) (void)hipFree(c->d_spec);
        c->d_spec = nullptr; c->cap_spec = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_spec, sizeof(double) * c->P.win_n));
        c->cap_spec = c->P.win_n;
    }
    double *d_args = c->d_misc;
    WalkerDesc *d_desc = reinterpret_cast<WalkerDesc *>(c->d_misc + 64);
    static_assert(sizeof(WalkerDesc) + 64 * sizeof(double) <= 4096, "misc buffer too small");
    HIP_TRY(c, hipMemcpyAsync(d_args, args, sizeof(double) * (3 * ns + 1), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(composite_setup_kernel, dim3(1), dim3(64), 0, c->stream, c->P, d_args, (int)use_distance, d_desc);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((c->P.win_n + 255) / 256)), dim3(256), 0, c->stream, c->P, d_desc,
                       c->d_spec);
    HIP_TRY(c, hipGetLastError());
    WalkerDesc h;
    HIP_TRY(c, hipMemcpyAsync(&h, d_desc, sizeof(WalkerDesc), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *status_out = h.status;
    if (h.status != MSX_W_OK) return MSX_OK;
    HIP_TRY(c, hipMemcpy(spec_out, c->d_spec, sizeof(double) * c->P.win_n, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->P.nc && contrast_out; ++i) contrast_out[i] = h.contrast[i];
    for (int i = 0; i < c->P.np && phot_out; ++i) phot_out[i] = h.phot[i];
    return MSX_OK;
}

int msx_comm_unique_id(msx_ctx *c, uint8_t *out128) {
    if (!c || !out128) return MSX_ERR_INVALID;
    if (!rccl().ok) return fail(c, MSX_ERR_STATE, "RCCL (librccl.so.1) could not be resolved in this process");
    RcclUniqueId id;
    const int rc = rccl().GetUniqueId(&id);
    if (rc != 0) return fail(c, MSX_ERR_HIP, std::string("ncclGetUniqueId: ") + rccl().GetErrorString(rc));
    memcpy(out128, id.internal, 128);
    return MSX_OK;
}

int msx_comm_init(msx_ctx *c, const uint8_t *id128, int32_t rank, int32_t world) {
    if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(c, MSX_ERR_INVALID, "msx_comm_init: bad arguments");
    if (!rccl().ok) return fail(c, MSX_ERR_STATE, "RCCL (librccl.so.1) could not be resolved in this process");
    if (c->rccl_comm) return fail(c, MSX_ERR_STATE, "msx_comm_init: communicator already initialised");
    HIP_TRY(c, hipSetDevice(c->device));
    RcclUniqueId id;
    memcpy(id.internal, id128, 128);
    const int rc = rccl().CommInitRank(&c->rccl_comm, world, id, rank);
    if (rc != 0) {
        c->rccl_comm = nullptr;
        return fail(c, MSX_ERR_HIP, std::string("ncclCommInitRank: ") + rccl().GetErrorString(rc));
    }
    HIP_TRY(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
    for (hipEvent_t &e : c->ev_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->comm_world = world;
    c->comm_rank = rank;
    return MSX_OK;
}

int msx_comm_init_loopback(msx_ctx **ctxs, int32_t world) {
    if (!ctxs || world < 1 || !ctxs[0]) return MSX_ERR_INVALID;
    msx_ctx *c0 = ctxs[0];
    for (int r = 0; r < world; ++r) {
        if (!ctxs[r]) return fail(c0, MSX_ERR_INVALID, "msx_comm_init_loopback: null context");
        if (ctxs[r]->rccl_comm || !ctxs[r]->loop_peers.empty())
            return fail(c0, MSX_ERR_STATE, "msx_comm_init_loopback: a context already belongs to a communicator");
        if (ctxs[r]->device != c0->device)
            return fail(c0, MSX_ERR_INVALID, "msx_comm_init_loopback: the ranks of a loopback group share one device");
        for (int q = 0; q < r; ++q)
            if (ctxs[q] == ctxs[r]) return fail(c0, MSX_ERR_INVALID, "msx_comm_init_loopback: one context per rank");
    }
    HIP_TRY(c0, hipSetDevice(c0->device));
    for (int r = 0; r < world; ++r) {
        msx_ctx *c = ctxs[r];
        HIP_TRY(c0, hipEventCreateWithFlags(&c->loop_eval_done, hipEventDisableTiming));
        HIP_TRY(c0, hipEventCreateWithFlags(&c->loop_copied, hipEventDisableTiming));
        // (recorded once so that the first half-step's waits find completed events)
        HIP_TRY(c0, hipEventRecord(c->loop_eval_done, c->stream));
        HIP_TRY(c0, hipEventRecord(c->loop_copied, c->stream));
        c->loop_peers.assign(ctxs, ctxs + world);
        c->comm_world = world;
        c->comm_rank = r;
    }
    return MSX_OK;
}

int msx_comm_allgather_dev(msx_ctx *c, const double *d_send, double *d_recv, int64_t count, void *compute_stream,
                           int32_t slot) {
    if (!c || !d_send || !d_recv || count < 1 || slot < 0 || slot > 3) return fail(c, MSX_ERR_INVALID, "msx_comm_allgather_dev: bad arguments");
    if (!c->rccl_comm) return fail(c, MSX_ERR_STATE, "msx_comm_allgather_dev: call msx_comm_init first");
    // the collective starts once everything queued so far on the compute stream is done, runs on the
    // communicator's own stream (so the next launch overlaps it) and signals the slot's event
    HIP_TRY(c, hipEventRecord(c->ev_ready, (hipStream_t)compute_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->comm_stream, c->ev_ready, 0));
    const int rc = rccl().AllGather(d_send, d_recv, (size_t)count, kNcclFloat64, c->rccl_comm, c->comm_stream);
    if (rc != 0) return fail(c, MSX_ERR_HIP, std::string("ncclAllGather: ") + rccl().GetErrorString(rc));
    HIP_TRY(c, hipEventRecord(c->ev_done[slot], c->comm_stream));
    return MSX_OK;
}

int msx_comm_wait_slot(msx_ctx *c, int32_t slot, void *compute_stream) {
    if (!c || slot < 0 || slot > 3) return MSX_ERR_INVALID;
    if (!c->rccl_comm) return fail(c, MSX_ERR_STATE, "msx_comm_wait_slot: call msx_comm_init first");
    HIP_TRY(c, hipStreamWaitEvent((hipStream_t)compute_stream, c->ev_done[slot], 0));
    return MSX_OK;
}

int msx_stream_copy_gbps(msx_ctx *c, int64_t bytes, int32_t iters, double *gbps_out) {
    if (!c || !gbps_out || bytes < 4096 || iters < 1) return fail(c, MSX_ERR_INVALID, "msx_stream_copy_gbps: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n4 = bytes / 16;
    float4 *a = nullptr, *b = nullptr;
    HIP_TRY(c, hipMalloc((void **)&a, n4 * 16));
    HIP_TRY(c, hipMalloc((void **)&b, n4 * 16));
    HIP_TRY(c, hipMemsetAsync(a, 1, n4 * 16, c->stream));
    hipEvent_t e0, e1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    const int cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
    double best = 0.0;
    for (int variant = 0; variant < 4; ++variant) {
        for (int per_cu : {8, 16, 32}) {
            const dim3 g((unsigned)(cus * per_cu)), bthreads(256);
            auto go = [&]() {
                switch (variant) {
                    case 0: hipLaunchKernelGGL((copy_float4_kernel<4, false>), g, bthreads, 0, c->stream, a, b, n4); break;
                    case 1: hipLaunchKernelGGL((copy_float4_kernel<8, false>), g, bthreads, 0, c->stream, a, b, n4); break;
                    case 2: hipLaunchKernelGGL((copy_float4_kernel<4, true>), g, bthreads, 0, c->stream, a, b, n4); break;
                    default: hipLaunchKernelGGL((copy_float4_kernel<8, true>), g, bthreads, 0, c->stream, a, b, n4); break;
                }
            };
            go();
            HIP_TRY(c, hipEventRecord(e0, c->stream));
            for (int i = 0; i < iters; ++i) go();
            HIP_TRY(c, hipEventRecord(e1, c->stream));
            HIP_TRY(c, hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
            const double gbps = (2.0 * (double)(n4 * 16) * iters) / ((double)ms * 1e-3) / 1e9;
            best = gbps > best ? gbps : best;
        }
    }
    *gbps_out = best;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    return MSX_OK;
}

int msx_bytes_per_eval(msx_ctx *c, int64_t n, int64_t *requested_bytes) {
    if (!c || !requested_bytes || n < 1) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_bytes_per_eval: no problem staged");
    const FormChoice f = decide_form(c, n, MSX_MODE_LOGPOST, true);
    if (f.err != MSX_OK) return fail(c, f.err, f.msg);
    *requested_bytes = plan_launch(c, f, n, 0, false).bytes;
    return MSX_OK;
}

int msx_launch_info(msx_ctx *c, int32_t mode, int64_t n, int32_t block_threads, char *name, int32_t name_len, int64_t *out8) {
    if (!c || !out8 || n < 1) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_launch_info: no problem staged");
    HIP_TRY(c, hipSetDevice(c->device));
    bool shared512;
    if (int rc = decode_block(c, block_threads, shared512)) return rc;
    const FormChoice f = decide_form(c, n, mode, true);
    if (f.err != MSX_OK) return fail(c, f.err, f.msg);
    // (the first sub-batch stands for the launch: sub-batches only differ in their walker count)
    const LaunchPlan pl = plan_launch(c, f, n, block_threads, shared512);
    if (!pl.fn) return fail(c, MSX_ERR_STATE, "no kernel variant for this launch");
    std::string nm;
    if (pl.pv) {
        nm = std::string("pair_plan_kernel + logprob_pair_kernel<512 threads, ") + std::to_string(pl.pv->nt) +
             " element trips per lane" + (pl.pv->full ? ", FULL" : "") + "> (planner: one thread per walker; two walkers of one grid cell per workgroup, one set of row loads, model values in registers; two workgroups per CU)";
    } else {
        const Variant *v = pl.v;
        nm = std::string("logprob_kernel<NS=") + std::to_string(v->ns) + ", " + std::to_string(v->threads) + " threads" +
             (v->lk ? ", linked" : v->gm ? ", GM" : v->pf && v->sh ? ", SH, PF" : v->pf ? ", PF" : v->sh ? ", SH" : "") + (v->r32 ? ", R32" : "") + (v->full == 3 ? ", FULL" : v->full == 2 ? ", FULL(chi2 pass)" : "") + (v->given ? ", GIVEN" : "") + "> (" + v->what + ")";
        if (f.inpath) nm = "inpath_recipe_kernel + inpath_conv_kernel + inpath_resample_kernel + " + nm;
    }
    const int form = f.inpath ? MSX_FORM_INPATH : f.pair ? MSX_FORM_PAIR : f.linked ? MSX_FORM_LINKED : MSX_FORM_FUSED;
    return launch_info_out(c, pl.fn, {form, pl.threads, 0, 0, (int64_t)pl.dyn_lds, pl.bytes, pl.grid, pl.m}, nm, name, name_len, out8);
}

int msx_last_form(msx_ctx *c, int32_t *form) {
    if (!c || !form) return MSX_ERR_INVALID;
    *form = c->last_form;
    return MSX_OK;
}

int msx_pair_stats(msx_ctx *c, int64_t *out2) {
    if (!c || !out2) return MSX_ERR_INVALID;
    if (!c->d_pair_plan) return fail(c, MSX_ERR_STATE, "msx_pair_stats: the staged problem has no pair form");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    int32_t h[2];
    HIP_TRY(c, hipMemcpy(h, c->d_pair_plan, sizeof(h), hipMemcpyDeviceToHost));
    out2[0] = h[0];
    out2[1] = h[1];
    return MSX_OK;
}

// ---- target groups (include/msx.h, group_kernel.h) -------------------------------------------------------------------
int msx_group_create(msx_ctx **ctxs, int32_t k, msx_group **out) {
    if (!out) return MSX_ERR_INVALID;
    msx_group *g = new msx_group();
    *out = g;  // returned even on failure so the caller can read msx_group_last_error
    if (!ctxs) return fail(g, MSX_ERR_INVALID, "msx_group_create: null context list");
    if (k < 1 || k > MSX_MAX_GROUP)
        return fail(g, MSX_ERR_RANGE, "msx_group_create: 1 to " + std::to_string(MSX_MAX_GROUP) + " members, " + std::to_string(k) + " given");
    for (int m = 0; m < k; ++m) {
        const msx_ctx *c = ctxs[m];
        const std::string who = "msx_group_create: member " + std::to_string(m);
        if (!c) return fail(g, MSX_ERR_INVALID, who + " is a null context");
        if (!c->problem_staged) return fail(g, MSX_ERR_STATE, who + ": no problem staged");
        if (c->device != ctxs[0]->device)
            return fail(g, MSX_ERR_STATE, who + " is on device " + std::to_string(c->device) + ", member 0 on device " +
                                               std::to_string(ctxs[0]->device) + ": a group lives on one device");
        if (c->P.nspec != ctxs[0]->P.nspec)
            return fail(g, MSX_ERR_RANGE, who + " has nspec = " + std::to_string(c->P.nspec) + ", member 0 nspec = " +
                                               std::to_string(ctxs[0]->P.nspec) + ": the members of a group share nspec (and ndim)");
        if (c->store_f32)
            return fail(g, MSX_ERR_STATE, who + " is staged with float32 grid storage (msx_set_grid_storage): groups take float64 tables only");
        if (c->model_in_global)
            return fail(g, MSX_ERR_RANGE, who + " has " + std::to_string(c->P.npix) +
                                               " pixels: groups take spectra of at most 17,152 pixels (the model vector in LDS)");
    }
    g->device = ctxs[0]->device;
    g->nspec = ctxs[0]->P.nspec;
    g->cus = ctxs[0]->prop.multiProcessorCount > 0 ? ctxs[0]->prop.multiProcessorCount : 256;
    std::vector<GroupMember> recs((size_t)k);
    for (int m = 0; m < k; ++m) {
        msx_ctx *c = ctxs[m];
        DevProblem q = c->P;
        // the fused form's fields only: no sampler, clock probe, optimiser or in-path inputs
        q.opt_flux = nullptr; q.opt_med = nullptr; q.opt_chain = nullptr;
        q.smp_on = 0; q.smp_defer = 0; q.smp_coords = nullptr; q.smp_logp = nullptr; q.smp_q = nullptr;
        q.smp_sidx = q.smp_cidx = q.smp_partner = nullptr;
        q.smp_zz = q.smp_zfac = q.smp_logu = nullptr;
        q.smp_rec = nullptr; q.smp_naccept = nullptr; q.smp_chain_row = q.smp_lp_row = nullptr; q.smp_worst = nullptr;
        q.smp_overlap = 0; q.smp_stride = 0; q.smp_ver = nullptr; q.smp_gran = nullptr; q.smp_gwalkers = 0;
        q.clk_probe = nullptr;
        q.given = nullptr; q.given_stride = 0;
        q.linked_fault = 0;
        g->probs.push_back(q);
        g->pf_ok.push_back(c->pf_ok);
        g->pf256_ok.push_back(c->pf256_ok);
        g->members.push_back(c);
        g->gen.push_back(c->prob_gen);
        GroupMember &r = recs[(size_t)m];
        r.rblk = (const unsigned char *)c->d_recipe_block;
        pack_leading_words(q, c->recipe_fast, 0, &r.niso_nt, &r.ng_fast);  // (q.smp_on = 0)
        r.tmin = q.tmin;
        r.tmax = q.tmax;
    }
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipMalloc((void **)&g->d_probs, sizeof(DevProblem) * (size_t)k));
    HIP_TRY(g, hipMalloc((void **)&g->d_members, sizeof(GroupMember) * (size_t)k));
    HIP_TRY(g, hipMemcpy(g->d_probs, g->probs.data(), sizeof(DevProblem) * (size_t)k, hipMemcpyHostToDevice));
    HIP_TRY(g, hipMemcpy(g->d_members, recs.data(), sizeof(GroupMember) * (size_t)k, hipMemcpyHostToDevice));
    for (msx_ctx *c : g->members)  // (back-pointers, once per context: a context may stand for several members)
        if (std::find(c->groups.begin(), c->groups.end(), g) == c->groups.end()) c->groups.push_back(g);
    return MSX_OK;
}

void msx_group_destroy(msx_group *g) {
    if (!g) return;
    group_run_free(g);  // a run still open ends here
    group_tempered_free(g);
    for (msx_ctx *c : g->members)
        if (c) c->groups.erase(std::remove(c->groups.begin(), c->groups.end(), g), c->groups.end());
    (void)hipSetDevice(g->device);
    if (g->d_probs) (void)hipFree(g->d_probs);
    if (g->d_members) (void)hipFree(g->d_members);
    if (g->h_pin) (void)hipHostFree(g->h_pin);
    delete g;
}

const char *msx_group_last_error(msx_group *g) { return g ? g->err.c_str() : "null group"; }

// Every member alive and still holding the problem the group snapshotted; the counts valid.  *total = their sum.
static int group_check(msx_group *g, const char *who, int32_t mode, const int64_t *counts, int32_t ndim, int64_t *total) {
    if (g->members.empty()) return fail(g, MSX_ERR_STATE, std::string(who) + ": the group was not created");
    for (size_t m = 0; m < g->members.size(); ++m) {
        const msx_ctx *c = g->members[m];
        if (!c)
            return fail(g, MSX_ERR_STATE, std::string(who) + ": member " + std::to_string(m) + " was destroyed (msx_destroy) before its group");
        if (c->prob_gen != g->gen[m])
            return fail(g, MSX_ERR_STATE, std::string(who) + ": member " + std::to_string(m) +
                                               "'s problem was dropped or staged again since msx_group_create; create the group again");
    }
    if (mode < MSX_MODE_LOGLIKE || mode > MSX_MODE_LOGPRIOR)
        return fail(g, MSX_ERR_INVALID, std::string(who) + ": mode must be MSX_MODE_LOGLIKE, _LOGPOST, _CHISQ or _LOGPRIOR");
    if (ndim != 2 * g->nspec + 2)
        return fail(g, MSX_ERR_INVALID, "P0 doesn't match what I was expecting (ndim must be 2*nspec+2)");
    if (!counts) return fail(g, MSX_ERR_INVALID, std::string(who) + ": null counts");
    int64_t t = 0;
    for (size_t m = 0; m < g->members.size(); ++m) {
        if (counts[m] < 0) return fail(g, MSX_ERR_INVALID, std::string(who) + ": member " + std::to_string(m) + " has a negative walker count");
        t += counts[m];
        if (t > 0x7fffffff) return fail(g, MSX_ERR_RANGE, std::string(who) + ": more than 2^31 - 1 walkers in one launch");
    }
    *total = t;
    return MSX_OK;
}

int msx_group_logprob_batch_dev(msx_group *g, int32_t mode, const double *d_theta, const int64_t *counts, int32_t ndim,
                                double *d_logp, int32_t *d_status, void *hip_stream, int32_t block_threads) {
    if (!g) return MSX_ERR_INVALID;
    int64_t total = 0;
    if (int rc = group_check(g, "msx_group_logprob_batch", mode, counts, ndim, &total)) return rc;
    if (total == 0) return MSX_OK;
    if (!d_theta || !d_logp || !d_status) return fail(g, MSX_ERR_INVALID, "msx_group_logprob_batch: bad arguments");
    bool shared512;
    if (int rc = decode_block(g, block_threads, shared512)) return rc;
    const GroupPlan pl = plan_group_launch(g, counts, total, block_threads, shared512);
    if (!pl.v) return fail(g, MSX_ERR_STATE, "no kernel variant for this group launch");
    GroupStarts st;
    st.k = (int32_t)g->members.size();
    int64_t acc = 0;
    for (int m = 0; m < st.k; ++m) { st.start[m] = (int32_t)acc; acc += counts[m]; }
    for (int m = st.k; m <= MSX_MAX_GROUP; ++m) st.start[m] = (int32_t)acc;
    // the kernel's arguments, in its own order
    const double *a_theta = d_theta;
    const void *a_members = g->d_members, *a_probs = g->d_probs;  // (read by the kernel through the constant address space)
    int a_mode = mode;
    int64_t a_n = total;
    double *a_logp = d_logp;
    int32_t *a_status = d_status;
    const SmpRec *a_rec = nullptr;
    void *args[] = {&a_theta, &a_members, &a_probs, &a_mode, &a_n, &st, &a_logp, &a_status, &a_rec};
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipLaunchKernel(pl.v->fn, dim3((unsigned)total), dim3((unsigned)pl.v->threads), args, pl.dyn_lds, (hipStream_t)hip_stream));
    return MSX_OK;
}

int msx_group_logprob_batch(msx_group *g, int32_t mode, const double *theta, const int64_t *counts, int32_t ndim,
                            double *logp_out, int32_t *status_out) {
    if (!g) return MSX_ERR_INVALID;
    int64_t n = 0;
    if (int rc = group_check(g, "msx_group_logprob_batch", mode, counts, ndim, &n)) return rc;
    if (n == 0) return MSX_OK;
    if (!theta || !logp_out || !status_out) return fail(g, MSX_ERR_INVALID, "msx_group_logprob_batch: bad arguments");
    HIP_TRY(g, hipSetDevice(g->device));
    PinnedStaging h;
    HIP_TRY(g, pinned_staging(&g->h_pin, &g->cap_walkers, n, &h));
    memcpy(h.theta, theta, sizeof(double) * n * ndim);
    hipStream_t s = g->members[0]->stream;  // member 0's stream
    if (int rc = msx_group_logprob_batch_dev(g, mode, h.theta, counts, ndim, h.logp, h.status, s, 0)) return rc;
    HIP_TRY(g, hipStreamSynchronize(s));
    memcpy(logp_out, h.logp, sizeof(double) * n);
    memcpy(status_out, h.status, sizeof(int32_t) * n);
    return MSX_OK;
}

int msx_group_launch_info(msx_group *g, int32_t mode, const int64_t *counts, int32_t block_threads, char *name, int32_t name_len,
                          int64_t *out8) {
    if (!g || !out8) return MSX_ERR_INVALID;
    int64_t total = 0;
    if (int rc = group_check(g, "msx_group_launch_info", mode, counts, 2 * g->nspec + 2, &total)) return rc;
    if (total < 1) return fail(g, MSX_ERR_INVALID, "msx_group_launch_info: no walkers");
    bool shared512;
    if (int rc = decode_block(g, block_threads, shared512)) return rc;
    const GroupPlan pl = plan_group_launch(g, counts, total, block_threads, shared512);
    if (!pl.v) return fail(g, MSX_ERR_STATE, "no kernel variant for this group launch");
    const GroupVariant *v = pl.v;
    const std::string nm = std::string("logprob_group_kernel<NS=") + std::to_string(v->ns) + ", " + std::to_string(v->threads) + " threads" +
                           (v->pf && v->sh ? ", SH, PF" : v->pf ? ", PF" : v->sh ? ", SH" : "") +
                           (v->full == 3 ? ", FULL" : v->full == 2 ? ", FULL(chi2 pass)" : "") + "> (" + v->what + ")";
    HIP_TRY(g, hipSetDevice(g->device));
    return launch_info_out(g, v->fn, {MSX_FORM_FUSED, v->threads, 0, 0, (int64_t)pl.dyn_lds, pl.bytes, total, total}, nm, name, name_len, out8);
}

// ---- a target group's device-resident sampler (include/msx.h, msx_group_sampler_*) -------------------------------------
// One resident ensemble for the whole group -- the members' walkers concatenated, [sum nw_k][ndim] -- and SamplerRun's
// pipeline (slots, upload / download streams, events, chunk packing).  Each half-step is ONE plain launch of the group
// kernel's SMP instance over the members' active halves (sum nw_k / 2 walkers, GroupStarts over nw_k / 2).  What changes
// from one half-step to the next (the records, zfac, log u, the chain rows) reaches the kernel without an upload: a slot's
// buffers never move and the chunks are laid out for cap_steps iterations (SamplerRun::layout_steps), so one set of member
// snapshots per (slot, step, half) is built at begin, and each launch passes its set as g_probs and its records as
// g_smp_rec.  Every record's si / ci is a GROUP-level ensemble index; each member's snapshots carry its own smp_worst.
struct GroupRun {
    SamplerRun *r = nullptr;
    hipStream_t stream = nullptr;  // the run's compute stream (its own: members may be destroyed while it is open)
    DevProblem *d_snap = nullptr;  // [2 slots][cap_steps][2 halves][k members]
    const void *fn = nullptr;      // the planned SMP instance
    int threads = 0;
    size_t dyn_lds = 0;
    GroupStarts st;                // over the members' active halves
};

// a member's problem is about to go (free_problem): let the launches that read its tables finish
static void group_run_drain(msx_group *g) {
    group_tempered_drain(g);
    if (g->run && g->run->stream) (void)hipStreamSynchronize(g->run->stream);
}

static void group_run_free(msx_group *g) {
    GroupRun *gr = g->run;
    if (!gr) return;
    (void)hipSetDevice(g->device);
    if (gr->r) run_close(gr->r, gr->stream);
    if (gr->stream) (void)hipStreamDestroy(gr->stream);
    if (gr->d_snap) (void)hipFree(gr->d_snap);
    delete gr;
    g->run = nullptr;
}

int msx_group_sampler_begin(msx_group *g, int32_t mode, const int64_t *counts, int32_t ndim, int64_t max_chunk_steps,
                            const double *coords, const double *logp, const int64_t *naccept) {
    if (!g) return MSX_ERR_INVALID;
    if (g->trun) return fail(g, MSX_ERR_STATE, "msx_group_sampler_begin: a tempered run is in flight on this group (msx_group_tempered_end)");
    int64_t total = 0;
    if (int rc = group_check(g, "msx_group_sampler_begin", mode, counts, ndim, &total)) return rc;
    if (mode != MSX_MODE_LOGPOST && mode != MSX_MODE_LOGLIKE)
        return fail(g, MSX_ERR_INVALID, "msx_group_sampler_begin: mode must be MSX_MODE_LOGPOST or MSX_MODE_LOGLIKE");
    const int k = (int)g->members.size();
    for (int m = 0; m < k; ++m)
        if (counts[m] < 2 || (counts[m] & 1))
            return fail(g, MSX_ERR_INVALID, "msx_group_sampler_begin: member " + std::to_string(m) + " has " + std::to_string(counts[m]) +
                                                 " walkers: the stretch move needs an even number, at least 2");
    if (!coords || !logp || max_chunk_steps < 1) return fail(g, MSX_ERR_INVALID, "msx_group_sampler_begin: bad arguments");
    HIP_TRY(g, hipSetDevice(g->device));
    group_run_free(g);
    std::vector<int64_t> half((size_t)k);
    for (int m = 0; m < k; ++m) half[(size_t)m] = counts[m] / 2;
    const int64_t ns = total / 2;
    GroupPlan pl = plan_group_launch(g, half.data(), ns, 0, false);
    if (pl.v && !pl.v->smp_fn) {  // no sampler instance of the planned entry: its neighbour without PF, then without SH
        const GroupVariant *sub = nullptr;
        for (int pass = 0; pass < 2 && !sub; ++pass)
            for (const GroupVariant &v : kGroupVariants)
                if (!sub && v.smp_fn && v.ns == pl.v->ns && v.threads == pl.v->threads && v.sh == (pass == 0 && pl.v->sh) && !v.pf && v.full == 0)
                    sub = &v;
        pl = sub ? group_plan_lds(g, half.data(), ns, sub) : GroupPlan();
    }
    if (!pl.v) return fail(g, MSX_ERR_STATE, "msx_group_sampler_begin: no kernel variant for this group launch");
    GroupRun *gr = new GroupRun;
    g->run = gr;
    gr->fn = pl.v->smp_fn; gr->threads = pl.v->threads; gr->dyn_lds = pl.dyn_lds;
    gr->st.k = k;
    SamplerRun *r = gr->r = new SamplerRun;
    r->mode = mode; r->ndim = ndim; r->nw = total; r->ns = ns; r->cap_steps = max_chunk_steps;
    r->overlap = 0;  // plain launches, one half-step after the other
    r->layout_steps = max_chunk_steps;
    r->nworst = k;
    int64_t off = 0, astart = 0;
    for (int m = 0; m < k; ++m) {
        r->m_nw.push_back(counts[m]); r->m_off.push_back(off); r->m_astart.push_back(astart);
        gr->st.start[m] = (int32_t)astart;
        off += counts[m]; astart += half[(size_t)m];
    }
    for (int m = k; m <= MSX_MAX_GROUP; ++m) gr->st.start[m] = (int32_t)astart;
    // [coords | logp | q | newlp | nacc | wst]
    const size_t state_bytes = sizeof(double) * (size_t)(total * ndim + total + ns * ndim + ns) + sizeof(int64_t) * (size_t)total +
                               sizeof(int32_t) * (size_t)ns;
    const size_t snap_count = (size_t)(2 * max_chunk_steps * 2 * k);
    hipError_t e = hipStreamCreateWithFlags(&gr->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&r->d_state, state_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&gr->d_snap, sizeof(DevProblem) * snap_count);
    if (e == hipSuccess) e = run_open(r);
    std::vector<DevProblem> snaps;
    if (e == hipSuccess) {
        r->d_coords = (double *)r->d_state; r->d_logp = r->d_coords + total * ndim; r->d_q = r->d_logp + total;
        r->d_newlp = r->d_q + ns * ndim; r->d_nacc = (int64_t *)(r->d_newlp + ns); r->d_wst = (int32_t *)(r->d_nacc + total);
        // the member snapshots of every (slot, step, half): msx_group_create's, with the sampler's fields pointing at the
        // group's ensemble and at this half-step's place in the slot
        snaps.reserve(snap_count);
        for (int slot = 0; slot < 2; ++slot) {
            ChunkPtrs cp;
            run_chunk_ptrs(r, r->slot[slot], max_chunk_steps, &cp);
            for (int64_t st = 0; st < max_chunk_steps; ++st)
                for (int h = 0; h < 2; ++h)
                    for (int m = 0; m < k; ++m) {
                        DevProblem q = g->probs[(size_t)m];
                        const int64_t o = (st * 2 + h) * ns;
                        q.smp_on = 1;
                        q.smp_coords = r->d_coords; q.smp_logp = r->d_logp; q.smp_q = r->d_q; q.smp_naccept = r->d_nacc;
                        q.smp_sidx = cp.d_sidx + o; q.smp_cidx = cp.d_cidx + o; q.smp_partner = cp.d_partner + o;
                        q.smp_zz = cp.d_zz + o; q.smp_zfac = cp.d_zfac + o; q.smp_logu = cp.d_logu + o; q.smp_rec = cp.d_rec + o;
                        q.smp_chain_row = cp.d_chain + st * total * ndim; q.smp_lp_row = cp.d_lpchain + st * total;
                        q.smp_worst = cp.d_worst + m;
                        q.smp_stride = total * ndim; q.smp_gwalkers = total;
                        snaps.push_back(q);
                    }
        }
        e = hipMemcpyAsync(gr->d_snap, snaps.data(), sizeof(DevProblem) * snap_count, hipMemcpyHostToDevice, gr->stream);
    }
    if (e == hipSuccess) e = run_load_state(r, gr->stream, coords, logp, naccept);  // (the snapshots, too, are consumed on return)
    if (e != hipSuccess) {
        group_run_free(g);
        return fail(g, MSX_ERR_HIP, std::string("msx_group_sampler_begin: ") + hipGetErrorString(e));
    }
    return MSX_OK;
}

// (draw != nullptr: the chunk's randomness is drawn on the device -- ONE group_draw_kernel launch on the run's stream, ahead
// of the chunk's half-steps, member m keyed by draw->seeds[m] and the absolute iteration numbers from draw->first_iter --
// instead of coming from the host's arrays: nothing is packed, nothing uploaded)
struct GroupDeviceDraw { const uint64_t *seeds; double a; int64_t first_iter; };
static int group_sampler_enqueue(msx_group *g, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                 const int32_t *partner, const double *zz, const double *zfac, const double *logu,
                                 const GroupDeviceDraw *draw) {
    if (!g) return MSX_ERR_INVALID;
    const std::string w(who);
    GroupRun *gr = g->run;
    if (int rc = run_enqueue_check(&g->err, gr ? gr->r : nullptr, who, "msx_group_sampler_begin", "msx_group_sampler_end", slot, nsteps,
                                   draw ? draw->seeds != nullptr : (sidx && cidx && partner && zz && zfac && logu)))
        return rc;
    SamplerRun *r = gr->r;
    if (draw) {
        if (!(draw->a > 1.0) || draw->first_iter < 0)
            return fail(g, MSX_ERR_INVALID, w + ": the device generator takes a stretch scale a > 1 and a first iteration >= 0");
        for (size_t m = 0; m < r->m_nw.size(); ++m)
            if (r->m_nw[m] > kDrawMaxWalkers)
                return fail(g, MSX_ERR_INVALID, w + ": member " + std::to_string(m) + " has " + std::to_string(r->m_nw[m]) +
                                                    " walkers; the device generator takes up to 4096 per member");
    }
    // a member restaged or destroyed since begin: the snapshots point at tables that are gone -- the run is over
    int64_t total = 0;
    std::vector<int64_t> counts(r->m_nw);
    if (int rc = group_check(g, who, r->mode, counts.data(), r->ndim, &total)) {
        r->failed = true;
        return rc;
    }
    SamplerRun::Slot &sl = r->slot[slot];
    HIP_TRY(g, hipSetDevice(g->device));
    if (!draw)
        if (const char *why = run_pack(r, sl, nsteps, sidx, cidx, partner, zz, zfac, logu)) return fail(g, MSX_ERR_INVALID, w + ": " + why);
    ChunkPtrs cp;
    run_chunk_ptrs(r, sl, nsteps, &cp);
    const int k = (int)g->members.size();
    hipError_t e = hipSuccess;
    if (draw) {
        GroupDrawTable T;
        memset(&T, 0, sizeof(T));
        for (int m = 0; m < k; ++m) {
            T.seed[m] = (unsigned long long)draw->seeds[m];
            T.nw[m] = (int32_t)r->m_nw[(size_t)m]; T.off[m] = (int32_t)r->m_off[(size_t)m]; T.astart[m] = (int32_t)r->m_astart[(size_t)m];
        }
        // (the slot was collected: no launch still reads its arrays, and the run's stream orders this one before the half-steps)
        hipLaunchKernelGGL(group_draw_kernel, dim3((unsigned)nsteps, (unsigned)k), dim3(kDrawThreads), 0, gr->stream, T, draw->a,
                           draw->first_iter, (int32_t)r->ndim, r->ns, cp.d_sidx, cp.d_cidx, cp.d_partner, cp.d_zz, cp.d_zfac, cp.d_logu,
                           const_cast<SmpRec *>(cp.d_rec));
        e = hipGetLastError();
    } else {
        e = run_upload(r, sl, nsteps, gr->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(cp.d_worst, 0, sizeof(int32_t) * (size_t)k, gr->stream);
    // the kernel's arguments, in its own order; per half-step only the snapshot set and the records move
    const double *a_theta = r->d_coords;
    const void *a_members = g->d_members;
    const void *a_probs = nullptr;
    int a_mode = r->mode;
    int64_t a_n = r->ns;
    double *a_logp = r->d_newlp;
    int32_t *a_status = r->d_wst;
    const SmpRec *a_rec = nullptr;
    void *args[] = {&a_theta, &a_members, &a_probs, &a_mode, &a_n, &gr->st, &a_logp, &a_status, &a_rec};
    for (int64_t st = 0; st < nsteps && e == hipSuccess; ++st)
        for (int h = 0; h < 2 && e == hipSuccess; ++h) {
            a_probs = gr->d_snap + (((int64_t)slot * r->cap_steps + st) * 2 + h) * k;
            a_rec = cp.d_rec + (st * 2 + h) * r->ns;
            e = hipLaunchKernel(gr->fn, dim3((unsigned)r->ns), dim3((unsigned)gr->threads), args, gr->dyn_lds, gr->stream);
        }
    if (e == hipSuccess) e = run_finish(r, slot, nsteps, cp, gr->stream);
    if (e != hipSuccess) {
        r->failed = true;  // some of the chunk's half-steps may be queued: only msx_group_sampler_end from here on
        return fail(g, MSX_ERR_HIP, w + ": " + hipGetErrorString(e));
    }
    r->steps_done += nsteps;
    return MSX_OK;
}

int msx_group_sampler_enqueue(msx_group *g, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                              const int32_t *partner, const double *zz, const double *zfac, const double *logu) {
    return group_sampler_enqueue(g, "msx_group_sampler_enqueue", slot, nsteps, sidx, cidx, partner, zz, zfac, logu, nullptr);
}

int msx_group_sampler_enqueue_drawn(msx_group *g, int32_t slot, int64_t nsteps, const uint64_t *seeds, double a, int64_t first_iter) {
    const GroupDeviceDraw dd = {seeds, a, first_iter};
    return group_sampler_enqueue(g, "msx_group_sampler_enqueue_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &dd);
}

int msx_group_sampler_collect(msx_group *g, int32_t slot, double *chain_out, double *logp_out, int64_t *naccept,
                              int32_t *worst_status) {
    if (!g) return MSX_ERR_INVALID;
    if (g->run && g->run->r->failed)
        return fail(g, MSX_ERR_STATE, "msx_group_sampler_collect: the run failed; end it (msx_group_sampler_end) and begin again");
    return run_collect_checked(&g->err, g->run ? g->run->r : nullptr, "msx_group_sampler_collect", "msx_group_sampler_begin", slot,
                               chain_out, logp_out, naccept, worst_status);
}

int msx_group_sampler_end(msx_group *g, double *coords, double *logp) {
    if (!g) return MSX_ERR_INVALID;
    if (!g->run) return MSX_OK;
    const hipError_t e = run_save_state(g->run->r, g->device, g->run->stream, coords, logp);
    group_run_free(g);
    if (e != hipSuccess) return fail(g, MSX_ERR_HIP, std::string("msx_group_sampler_end: ") + hipGetErrorString(e));
    return MSX_OK;
}

// ---- moves other than the stretch move, and mixtures (include/msx.h, msx_*_enqueue_moves*; move_kernels.h) --------------
// The path BESIDE the fused kernel: a chunk of nsteps iterations is  step(propose 0) ; { eval ; step(apply j, propose j + 1) }
// ... eval ; step(apply 2 nsteps - 1)  -- the unchanged plain evaluation plus one launch per half-step (and one per chunk).
// The context's run is the one-member case of the group's.

// where the general layout's arrays live in a slot (move_kernels.h, MoveChunk); kind [lay][k]
struct MoveChunkPtrs {
    double *g, *fac, *logu;
    int32_t *sidx, *cidx, *c1, *c2, *kind;
};
static MoveChunkPtrs move_chunk_ptrs(const SamplerRun *r, const ChunkPtrs &cp, int64_t nsteps) {
    const int64_t L = r->lay(nsteps) * 2 * r->ns;
    int32_t *c2 = (int32_t *)const_cast<SmpRec *>(cp.d_rec);
    return {cp.d_zz, cp.d_zfac, cp.d_logu, cp.d_sidx, cp.d_cidx, cp.d_partner, c2, c2 + L};
}

// msx_move_set -> the kernel's form; nullptr, or what is wrong with it.  min_nw: the smallest member
static const char *move_set_dev(const msx_move_set *set, int32_t ndim, int64_t min_nw, MoveSetDev *S) {
    if (!set || set->n < 1 || set->n > MSX_MAX_MOVES) return "a set holds 1..MSX_MAX_MOVES moves";
    memset(S, 0, sizeof(*S));
    S->n = set->n;
    double cum = 0.0;
    for (int i = 0; i < set->n; ++i) {
        const int kd = set->kind[i];
        if (kd != MSX_MOVE_STRETCH && kd != MSX_MOVE_DE) return "unknown kind of move";
        if (!std::isfinite(set->weight[i]) || !(set->weight[i] > 0.0)) return "weights must be finite and > 0";
        if (kd == MSX_MOVE_STRETCH && !(std::isfinite(set->a[i]) && set->a[i] > 1.0)) return "a stretch move needs a scale a > 1";
        if (kd == MSX_MOVE_DE && !(std::isfinite(set->sigma[i]) && set->sigma[i] >= 0.0 && std::isfinite(set->gamma0[i])))
            return "a DE move needs a finite sigma >= 0 and a finite gamma0";
        if (kd == MSX_MOVE_DE && min_nw < 4) return "the DE move needs two distinct walkers in each half: at least 4 walkers";
        cum += set->weight[i];
        S->kind[i] = kd; S->cum[i] = cum; S->a[i] = set->a[i]; S->sigma[i] = set->sigma[i];
        S->g0[i] = set->gamma0[i] > 0.0 ? set->gamma0[i] : 2.38 / std::sqrt(2.0 * (double)ndim);
    }
    if (std::fabs(cum - 1.0) > 1e-12) return "the weights must be normalised (sum 1 within 1e-12)";
    return nullptr;
}

static MoveMembers move_members(const SamplerRun *r, bool walkers) {
    MoveMembers M;
    memset(&M, 0, sizeof(M));
    for (size_t m = 0; m < r->m_nw.size(); ++m) {
        M.astart[m] = (int32_t)r->m_astart[m]; M.off[m] = (int32_t)r->m_off[m];
        M.nh[m] = (int32_t)(walkers ? r->m_nw[m] : r->m_nw[m] / 2);
    }
    return M;
}

// The chunk's host randomness in the general layout -- [nsteps][2][ns] each, kind [nsteps][k], indices member-local -- into
// the slot's pinned staging (run_pack's place and checks): every index is dereferenced on the device.  nullptr, or what is wrong.
static const char *run_pack_moves(SamplerRun *r, SamplerRun::Slot &sl, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                  const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                                  const double *logu) {
    const int64_t ns = r->ns, nh = nsteps * 2 * ns, L = r->lay(nsteps) * 2 * ns;
    const size_t km = r->m_nw.size();
    for (int64_t i = 0; i < nsteps * (int64_t)km; ++i)
        if (kind[i] != MSX_MOVE_STRETCH && kind[i] != MSX_MOVE_DE) return "kind out of range";
    double *hz = (double *)sl.h_in;
    int32_t *hi = (int32_t *)(hz + 3 * L);
    int32_t *hc2 = hi + 3 * L, *hk = hc2 + L;
    memcpy(hz, g, sizeof(double) * nh); memcpy(hz + L, fac, sizeof(double) * nh); memcpy(hz + 2 * L, logu, sizeof(double) * nh);
    memcpy(hi, sidx, sizeof(int32_t) * nh); memcpy(hi + L, cidx, sizeof(int32_t) * nh);
    memcpy(hk, kind, sizeof(int32_t) * nsteps * km);
    for (int64_t row = 0; row < 2 * nsteps; ++row)
        for (size_t m = 0; m < km; ++m) {
            const int64_t b = row * ns + r->m_astart[m], off = r->m_off[m];
            const uint32_t mw = (uint32_t)r->m_nw[m], mh = mw / 2;
            const bool de = kind[(row / 2) * (int64_t)km + (int64_t)m] == MSX_MOVE_DE;
            for (int64_t j = b; j < b + (int64_t)mh; ++j) {
                if ((uint32_t)sidx[j] >= mw || (uint32_t)cidx[j] >= mw || (uint32_t)p1[j] >= mh || (uint32_t)p2[j] >= mh)
                    return "walker / partner index out of range";
                if (de && p1[j] == p2[j]) return "a DE entry needs two distinct walkers (p1 != p2)";
            }
            for (int64_t j = b; j < b + (int64_t)mh; ++j) {  // (the complementary half is checked: resolve)
                hi[2 * L + j] = (int32_t)(off + cidx[b + p1[j]]);
                hc2[j] = (int32_t)(off + cidx[b + p2[j]]);
            }
        }
    return nullptr;
}

// What a chunk's launches need besides the run: the stream, and the plain evaluation of the ns proposals in r->d_q.
struct MoveTarget {
    hipStream_t stream;
    msx_ctx *c;      // the context's run, or
    msx_group *g;    // the group's
    std::vector<int64_t> half;
};
static int move_eval(const MoveTarget &t, SamplerRun *r) {
    if (t.c) return msx_logprob_batch_dev(t.c, r->mode, r->d_q, r->ns, r->ndim, r->d_newlp, r->d_wst, t.stream, 0);
    return msx_group_logprob_batch_dev(t.g, r->mode, r->d_q, t.half.data(), r->ndim, r->d_newlp, r->d_wst, t.stream, 0);
}

// the chunk's 2 nsteps + 1 step launches and 2 nsteps evaluations; MSX_OK, or the failing call's code (*herr: a HIP error's)
static int move_chunk_launches(const MoveTarget &t, SamplerRun *r, const ChunkPtrs &cp, const MoveChunkPtrs &mp, int64_t nsteps, hipError_t *herr) {
    const int64_t ns = r->ns, nw = r->nw;
    const int k = (int)r->m_nw.size();
    const MoveMembers M = move_members(r, false);
    MoveStepArgs A;
    memset(&A, 0, sizeof(A));
    A.coords = r->d_coords; A.logp = r->d_logp; A.q = r->d_q; A.newlp = r->d_newlp; A.nacc = r->d_nacc;
    A.ndim = r->ndim; A.worst = cp.d_worst;
    auto half_arrays = [&](int64_t j) {  // half-step j of the chunk
        const int64_t o = j * ns;
        return MoveChunk{mp.g + o, mp.fac + o, mp.logu + o, mp.sidx + o, mp.c1 + o, mp.c2 + o, mp.kind + (j / 2) * k};
    };
    for (int64_t j = 0; j <= 2 * nsteps; ++j) {
        A.a_on = j > 0; A.p_on = j < 2 * nsteps;
        if (A.a_on) {
            A.a = half_arrays(j - 1);
            A.chain_row = cp.d_chain + ((j - 1) / 2) * nw * r->ndim; A.lp_row = cp.d_lpchain + ((j - 1) / 2) * nw;
        }
        if (A.p_on) A.p = half_arrays(j);
        hipLaunchKernelGGL(move_step_kernel, dim3((unsigned)k), dim3(256), 0, t.stream, A, M);
        *herr = hipGetLastError();
        if (*herr != hipSuccess) return MSX_ERR_HIP;
        if (A.p_on)
            if (int rc = move_eval(t, r)) return rc;
    }
    return MSX_OK;
}

struct MoveDraw { const uint64_t *seeds; const msx_move_set *set; int64_t first_iter; };

// one chunk of either run: the checks the families share, the chunk's arrays (drawn or packed and uploaded), the launches
static int moves_enqueue(std::string *err, const MoveTarget &t, SamplerRun *r, const std::string &w, int32_t slot, int64_t nsteps,
                         const int32_t *sidx, const int32_t *cidx, const int32_t *kind, const int32_t *p1, const int32_t *p2,
                         const double *g, const double *fac, const double *logu, const MoveDraw *draw) {
    auto bad = [&](int code, const std::string &msg) { *err = w + ": " + msg; return code; };
    if (r->sharded) return bad(MSX_ERR_STATE, "the sharded run is stretch only");
    if (r->overlap == 1) return bad(MSX_ERR_STATE, "this run's stretch chunks overlap their half-steps; a run with moves takes plain launches from its first chunk (msx_sampler_policy(ctx, 0))");
    MoveSetDev S;
    if (draw) {
        int64_t min_nw = r->m_nw[0], max_nw = r->m_nw[0];
        for (int64_t n : r->m_nw) { min_nw = std::min(min_nw, n); max_nw = std::max(max_nw, n); }
        if (max_nw > kDrawMaxWalkers || draw->first_iter < 0) return bad(MSX_ERR_INVALID, "the device generator takes up to 4096 walkers per ensemble and a first iteration >= 0");
        if (const char *why = move_set_dev(draw->set, r->ndim, min_nw, &S)) return bad(MSX_ERR_INVALID, why);
    }
    SamplerRun::Slot &sl = r->slot[slot];
    if (!draw)
        if (const char *why = run_pack_moves(r, sl, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu)) return bad(MSX_ERR_INVALID, why);
    r->overlap = 0;
    ChunkPtrs cp;
    run_chunk_ptrs(r, sl, nsteps, &cp);
    const MoveChunkPtrs mp = move_chunk_ptrs(r, cp, nsteps);
    const int k = (int)r->m_nw.size();
    hipError_t e = hipSuccess;
    if (draw) {
        MoveDrawTable T;
        memset(&T, 0, sizeof(T));
        T.M = move_members(r, true);
        for (int m = 0; m < k; ++m) T.seed[m] = (unsigned long long)draw->seeds[m];
        // (the slot was collected: no launch still reads its arrays, and the stream orders this one before the half-steps)
        hipLaunchKernelGGL(moves_draw_kernel, dim3((unsigned)nsteps, (unsigned)k), dim3(kDrawThreads), 0, t.stream, T, S, draw->first_iter,
                           (int32_t)r->ndim, 1, r->ns, mp.sidx, mp.cidx, mp.c1, mp.c2, mp.g, mp.fac, mp.logu, mp.kind);
        e = hipGetLastError();
    } else {
        e = run_upload(r, sl, nsteps, t.stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(cp.d_worst, 0, sizeof(int32_t) * (size_t)r->nworst, t.stream);
    int rc = MSX_OK;
    if (e == hipSuccess) rc = move_chunk_launches(t, r, cp, mp, nsteps, &e);
    if (e == hipSuccess && rc == MSX_OK) e = run_finish(r, slot, nsteps, cp, t.stream);
    if (e != hipSuccess || rc != MSX_OK) {
        r->failed = true;  // some of the chunk's half-steps may be queued: only the run's end from here on
        if (e != hipSuccess) return bad(MSX_ERR_HIP, hipGetErrorString(e));
        if (t.c ? !t.c->err.empty() : !t.g->err.empty()) *err = t.c ? t.c->err : t.g->err;
        return rc;
    }
    r->steps_done += nsteps;
    return MSX_OK;
}

static int sampler_enqueue_moves(msx_ctx *c, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                 const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                                 const double *logu, const MoveDraw *draw) {
    if (!c) return MSX_ERR_INVALID;
    SamplerRun *r = c->smp;
    if (int rc = run_enqueue_check(&c->err, r, who, "msx_sampler_begin", "msx_sampler_end", slot, nsteps,
                                   draw ? draw->set != nullptr : (sidx && cidx && kind && p1 && p2 && g && fac && logu)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->P.smp_on = 0;  // (the plain evaluation)
    c->P.smp_defer = 0;
    MoveTarget t{c->stream, c, nullptr, {}};
    std::string err;
    const int rc = moves_enqueue(&err, t, r, who, slot, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu, draw);
    if (rc != MSX_OK) c->err = err;
    return rc;
}

int msx_sampler_enqueue_moves(msx_ctx *c, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx, const int32_t *kind,
                              const int32_t *p1, const int32_t *p2, const double *g, const double *fac, const double *logu) {
    return sampler_enqueue_moves(c, "msx_sampler_enqueue_moves", slot, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu, nullptr);
}

int msx_sampler_enqueue_moves_drawn(msx_ctx *c, int32_t slot, int64_t nsteps, uint64_t seed, const msx_move_set *set, int64_t first_iter) {
    const MoveDraw dd = {&seed, set, first_iter};
    return sampler_enqueue_moves(c, "msx_sampler_enqueue_moves_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, &dd);
}

int msx_sampler_draw_moves(msx_ctx *c, uint64_t seed, const msx_move_set *set, int64_t first_iter, int64_t nsteps, int64_t nw, int32_t ndim,
                           int32_t *sidx, int32_t *cidx, int32_t *kind, int32_t *p1, int32_t *p2, double *g, double *fac, double *logu) {
    if (!c) return MSX_ERR_INVALID;
    if (!sidx || !cidx || !kind || !p1 || !p2 || !g || !fac || !logu || nsteps < 1 || nw < 2 || (nw & 1) || nw > kDrawMaxWalkers ||
        first_iter < 0 || ndim < 1)
        return fail(c, MSX_ERR_INVALID, "msx_sampler_draw_moves: bad arguments (an even number of walkers, at most 4096)");
    MoveSetDev S;
    if (const char *why = move_set_dev(set, ndim, nw, &S)) return fail(c, MSX_ERR_INVALID, std::string("msx_sampler_draw_moves: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t nh = nsteps * nw;
    char *d = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d, (size_t)nh * (3 * sizeof(double) + 4 * sizeof(int32_t)) + (size_t)nsteps * sizeof(int32_t)));
    double *g_g = (double *)d, *g_fac = g_g + nh, *g_logu = g_fac + nh;
    int32_t *g_sidx = (int32_t *)(g_logu + nh), *g_cidx = g_sidx + nh, *g_p1 = g_cidx + nh, *g_p2 = g_p1 + nh, *g_kind = g_p2 + nh;
    MoveDrawTable T;
    memset(&T, 0, sizeof(T));
    T.seed[0] = (unsigned long long)seed;
    T.M.nh[0] = (int32_t)nw;
    hipLaunchKernelGGL(moves_draw_kernel, dim3((unsigned)nsteps, 1u), dim3(kDrawThreads), 0, c->stream, T, S, first_iter, ndim, 0, nw / 2, g_sidx,
                       g_cidx, g_p1, g_p2, g_g, g_fac, g_logu, g_kind);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(g, g_g, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(fac, g_fac, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(logu, g_logu, sizeof(double) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sidx, g_sidx, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cidx, g_cidx, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(p1, g_p1, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(p2, g_p2, sizeof(int32_t) * nh, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(kind, g_kind, sizeof(int32_t) * nsteps, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_sampler_draw_moves: ") + hipGetErrorString(e));
    return MSX_OK;
}

static int group_sampler_enqueue_moves(msx_group *g, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                       const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *gg, const double *fac,
                                       const double *logu, const MoveDraw *draw) {
    if (!g) return MSX_ERR_INVALID;
    GroupRun *gr = g->run;
    if (int rc = run_enqueue_check(&g->err, gr ? gr->r : nullptr, who, "msx_group_sampler_begin", "msx_group_sampler_end", slot, nsteps,
                                   draw ? (draw->seeds && draw->set) : (sidx && cidx && kind && p1 && p2 && gg && fac && logu)))
        return rc;
    SamplerRun *r = gr->r;
    // a member restaged or destroyed since begin: the run is over (group_sampler_enqueue)
    int64_t total = 0;
    std::vector<int64_t> counts(r->m_nw);
    if (int rc = group_check(g, who, r->mode, counts.data(), r->ndim, &total)) {
        r->failed = true;
        return rc;
    }
    HIP_TRY(g, hipSetDevice(g->device));
    MoveTarget t{gr->stream, nullptr, g, {}};
    for (int64_t n : r->m_nw) t.half.push_back(n / 2);
    std::string err;
    const int rc = moves_enqueue(&err, t, r, who, slot, nsteps, sidx, cidx, kind, p1, p2, gg, fac, logu, draw);
    if (rc != MSX_OK) g->err = err;
    return rc;
}

int msx_group_sampler_enqueue_moves(msx_group *g, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx, const int32_t *kind,
                                    const int32_t *p1, const int32_t *p2, const double *gg, const double *fac, const double *logu) {
    return group_sampler_enqueue_moves(g, "msx_group_sampler_enqueue_moves", slot, nsteps, sidx, cidx, kind, p1, p2, gg, fac, logu, nullptr);
}

int msx_group_sampler_enqueue_moves_drawn(msx_group *g, int32_t slot, int64_t nsteps, const uint64_t *seeds, const msx_move_set *set,
                                          int64_t first_iter) {
    const MoveDraw dd = {seeds, set, first_iter};
    return group_sampler_enqueue_moves(g, "msx_group_sampler_enqueue_moves_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, &dd);
}

// ---- parallel tempering (include/msx.h, msx_tempered_*; tempered_kernels.h) ------------------------
// The path beside the fused kernel once more: T rungs of nw walkers, all of this context's problem, as the T members of one
// ensemble in the general layout.  An iteration is
//   step(propose 0) ; prior ; like ; step(apply 0, propose 1) ; prior ; like ; step(apply 1) ; swap
// with `prior` / `like` the UNCHANGED plain evaluation of the T ns proposals in MSX_MODE_LOGPRIOR / _LOGLIKE, each into
// buffers of its own.  Plain launches on the context's stream; nothing allocates or synchronises after begin.
struct TemperedRun {
    int32_t T = 0, ndim = 0;
    int64_t nw = 0, ns = 0, cap_steps = 0;   // nw, ns: per rung
    bool failed = false;                     // an enqueue returned an error after queuing part of its launches
    bool enqueued = false;                   // an enqueue has queued something (msx_series_attach_tempered comes before)
    // the device series the run appends its chunks to (msx_series_attach_tempered): the coordinates [T nw][ndim] and
    // (ll, lpr) [T nw][2], rung t member t; either may be absent.  series_row: the row the next chunk starts at
    struct msx_series *s_chain = nullptr, *s_dens = nullptr;
    int64_t series_row = 0;
    double beta[MSX_MAX_GROUP], db[MSX_MAX_GROUP];
    // an adaptive run (msx_ladder_adapt): the ladder, the sweep's counters at the previous iteration's
    // end and (k, skipped) live in device memory, and every chunk carries beta_chain [st][T], the ladder each iteration ran with
    bool adaptive = false;
    double lag = 0.0, time = 0.0;
    char *d_adapt = nullptr;
    double *d_beta = nullptr;
    unsigned long long *d_prev = nullptr;
    long long *d_kstate = nullptr;
    char *d_state = nullptr;
    double *d_coords = nullptr, *d_ll = nullptr, *d_lpr = nullptr, *d_q = nullptr, *d_new_lpr = nullptr, *d_new_ll = nullptr;
    int64_t *d_nacc = nullptr;
    unsigned long long *d_nswap = nullptr;
    int32_t *d_st_lpr = nullptr, *d_st_ll = nullptr;
    hipStream_t copy = nullptr, up = nullptr;
    struct Slot {
        char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
        hipEvent_t in_ready = nullptr, kernels_done = nullptr, out_ready = nullptr;
        int64_t nsteps = 0;
        bool busy = false, collected = false;   // collected: h_out holds the last collected chunk (msx_ladder_betas)
    } slot[2];
    // a chunk of st iterations in its slot, laid out for its own length:
    //   in  [g | fac | logu  (st 2 T ns doubles each) | swap_logu (st (T-1) nw doubles) | sidx | cidx | c1 | c2 (int32) | kind (st T)]
    //   out [chain st T nw ndim | ll st T nw | lpr st T nw | naccept T nw (int64) | nswap MSX_MAX_GROUP (int64) | worst MSX_MAX_GROUP (int32)
    //        | beta_chain st T (doubles): an adaptive run's only, though the slots always have room for it]
    int64_t entries(int64_t st) const { return st * 2 * T * ns; }
    size_t in_bytes(int64_t st) const {
        return sizeof(double) * (size_t)(3 * entries(st) + st * (T - 1) * nw) + sizeof(int32_t) * (size_t)(4 * entries(st) + st * T);
    }
    size_t out_bytes(int64_t st) const {
        return fixed_out_bytes(st) + (adaptive ? sizeof(double) * (size_t)(st * T) : 0);
    }
    size_t fixed_out_bytes(int64_t st) const {
        return sizeof(double) * (size_t)(st * T * nw * (ndim + 2)) + sizeof(int64_t) * (size_t)(T * nw + MSX_MAX_GROUP) + sizeof(int32_t) * MSX_MAX_GROUP;
    }
    size_t cap_out_bytes() const { return fixed_out_bytes(cap_steps) + sizeof(double) * (size_t)(cap_steps * T); }
};

struct TemperedIn {
    double *g, *fac, *logu, *swap_logu;
    int32_t *sidx, *cidx, *c1, *c2, *kind;
};
static TemperedIn tempered_in(const TemperedRun *r, char *base, int64_t st) {
    const int64_t L = r->entries(st);
    TemperedIn p;
    p.g = (double *)base; p.fac = p.g + L; p.logu = p.fac + L; p.swap_logu = p.logu + L;
    p.sidx = (int32_t *)(p.swap_logu + st * (r->T - 1) * r->nw); p.cidx = p.sidx + L; p.c1 = p.cidx + L; p.c2 = p.c1 + L; p.kind = p.c2 + L;
    return p;
}
struct TemperedOut {
    double *chain, *ll, *lpr;
    int64_t *nacc, *nswap;
    int32_t *worst;
    double *betas;   // beta_chain [st][T]
};
static TemperedOut tempered_out(const TemperedRun *r, char *base, int64_t st) {
    const int64_t rows = st * r->T * r->nw;
    TemperedOut p;
    p.chain = (double *)base; p.ll = p.chain + rows * r->ndim; p.lpr = p.ll + rows;
    p.nacc = (int64_t *)(p.lpr + rows); p.nswap = p.nacc + r->T * r->nw; p.worst = (int32_t *)(p.nswap + MSX_MAX_GROUP);
    p.betas = (double *)(p.worst + MSX_MAX_GROUP);
    return p;
}

static void tempered_free(msx_ctx *c) {
    TemperedRun *r = c->tmp;
    if (!r) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (r->copy) (void)hipStreamSynchronize(r->copy);
    if (r->up) (void)hipStreamSynchronize(r->up);
    for (auto &sl : r->slot) {
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.in_ready) (void)hipEventDestroy(sl.in_ready);
        if (sl.kernels_done) (void)hipEventDestroy(sl.kernels_done);
        if (sl.out_ready) (void)hipEventDestroy(sl.out_ready);
    }
    if (r->d_state) (void)hipFree(r->d_state);
    if (r->d_adapt) (void)hipFree(r->d_adapt);
    if (r->s_chain) r->s_chain->trun = nullptr;  // (the series outlive the run)
    if (r->s_dens) r->s_dens->trun = nullptr;
    if (r->copy) (void)hipStreamDestroy(r->copy);
    if (r->up) (void)hipStreamDestroy(r->up);
    delete r;
    c->tmp = nullptr;
}

int msx_tempered_begin(msx_ctx *c, int32_t ntemps, const double *betas, int64_t nw, int32_t ndim, int64_t max_chunk_steps,
                       const double *coords, const double *ll, const double *lpr) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_tempered_begin: no problem staged");
    if (c->smp || c->tmp) return fail(c, MSX_ERR_STATE, "msx_tempered_begin: a run is already in flight on this context (msx_sampler_end / msx_tempered_end)");
    if (c->rccl_comm || !c->loop_peers.empty()) return fail(c, MSX_ERR_STATE, "msx_tempered_begin: a tempered run is one GPU; this context holds a communicator");
    if (c->smp_overlap_policy != 0)
        return fail(c, MSX_ERR_STATE, "msx_tempered_begin: the run takes plain launches; set msx_sampler_policy(ctx, 0) first");
    if (!betas || !coords || !ll || !lpr || max_chunk_steps < 1) return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: bad arguments");
    if (ntemps < 1 || ntemps > MSX_MAX_GROUP) return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: a ladder has 1..MSX_MAX_GROUP rungs");
    for (int t = 0; t < ntemps; ++t)
        if (!std::isfinite(betas[t]) || !(betas[t] > 0.0) || (t > 0 && !(betas[t] < betas[t - 1])))
            return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: betas must be finite, > 0 and strictly descending");
    if (nw < 2 || (nw & 1)) return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: a rung needs an even number of walkers");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, "P0 doesn't match what I was expecting");
    if ((int64_t)ntemps * nw * (int64_t)ndim * max_chunk_steps > ((int64_t)1 << 31))
        return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: the chunk is too long for this ladder (ntemps x nw x ndim x steps <= 2^31)");
    for (int64_t i = 0; i < (int64_t)ntemps * nw; ++i)
        if (!std::isfinite(lpr[i]) || std::isnan(ll[i]))
            return fail(c, MSX_ERR_INVALID, "msx_tempered_begin: an initial walker lies outside the prior (lpr not finite) or its ll is NaN");
    HIP_TRY(c, hipSetDevice(c->device));
    TemperedRun *r = new TemperedRun;
    c->tmp = r;
    r->T = ntemps; r->ndim = ndim; r->nw = nw; r->ns = nw / 2; r->cap_steps = max_chunk_steps;
    memset(r->beta, 0, sizeof(r->beta)); memset(r->db, 0, sizeof(r->db));
    for (int t = 0; t < ntemps; ++t) r->beta[t] = betas[t];
    for (int t = 0; t + 1 < ntemps; ++t) r->db[t] = betas[t] - betas[t + 1];
    const int64_t W = (int64_t)ntemps * nw, H = (int64_t)ntemps * r->ns;
    const size_t state_bytes = sizeof(double) * (size_t)(W * ndim + 2 * W + H * ndim + 2 * H) + sizeof(int64_t) * (size_t)(W + MSX_MAX_GROUP) +
                               sizeof(int32_t) * (size_t)(2 * H);
    hipError_t e = hipMalloc((void **)&r->d_state, state_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_state, 0, state_bytes, c->stream);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->up, hipStreamNonBlocking);
    for (auto &sl : r->slot) {
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_in, r->in_bytes(r->cap_steps));
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_out, r->cap_out_bytes());
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_in, r->in_bytes(r->cap_steps), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_out, r->cap_out_bytes(), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.in_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.kernels_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.out_ready, hipEventDisableTiming);
    }
    if (e == hipSuccess) {
        r->d_coords = (double *)r->d_state; r->d_ll = r->d_coords + W * ndim; r->d_lpr = r->d_ll + W; r->d_q = r->d_lpr + W;
        r->d_new_lpr = r->d_q + H * ndim; r->d_new_ll = r->d_new_lpr + H;
        r->d_nacc = (int64_t *)(r->d_new_ll + H); r->d_nswap = (unsigned long long *)(r->d_nacc + W);
        r->d_st_lpr = (int32_t *)(r->d_nswap + MSX_MAX_GROUP); r->d_st_ll = r->d_st_lpr + H;
        e = hipMemcpyAsync(r->d_coords, coords, sizeof(double) * (size_t)(W * ndim), hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_ll, ll, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_lpr, lpr, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        tempered_free(c);
        return fail(c, MSX_ERR_HIP, std::string("msx_tempered_begin: ") + hipGetErrorString(e));
    }
    return MSX_OK;
}

// Makes the run begun by msx_tempered_begin adaptive from k0: the ladder goes to device memory, where
// the step and sweep instantiations read it and tempered_adapt_kernel moves it after every iteration's sweep.
int msx_ladder_adapt(msx_ctx *c, double lag, double time, int64_t k0) {
    if (!c) return MSX_ERR_INVALID;
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_ladder_adapt: call msx_tempered_begin first");
    if (r->enqueued || r->adaptive)
        return fail(c, MSX_ERR_STATE, "msx_ladder_adapt: call once, between msx_tempered_begin and the run's first enqueue");
    if (!std::isfinite(lag) || !(lag > 0.0) || !std::isfinite(time) || !(time >= 1.0) || k0 < 0)
        return fail(c, MSX_ERR_INVALID, "msx_ladder_adapt: lag must be finite and > 0, time finite and >= 1, k0 >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(double) * MSX_MAX_GROUP + sizeof(unsigned long long) * MSX_MAX_GROUP + sizeof(long long) * 2;
    hipError_t e = hipMalloc((void **)&r->d_adapt, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_adapt, 0, bytes, c->stream);
    if (e == hipSuccess) {
        r->d_beta = (double *)r->d_adapt; r->d_prev = (unsigned long long *)(r->d_beta + MSX_MAX_GROUP);
        r->d_kstate = (long long *)(r->d_prev + MSX_MAX_GROUP);
        e = hipMemcpyAsync(r->d_beta, r->beta, sizeof(double) * (size_t)r->T, hipMemcpyHostToDevice, c->stream);
    }
    const long long k = (long long)k0;
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_kstate, &k, sizeof(k), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (r->d_adapt) (void)hipFree(r->d_adapt);
        r->d_adapt = nullptr;
        return fail(c, MSX_ERR_HIP, std::string("msx_ladder_adapt: ") + hipGetErrorString(e));
    }
    r->adaptive = true; r->lag = lag; r->time = time;
    return MSX_OK;
}

// The current ladder of the run, behind everything queued (it waits for the compute stream); k: the adaptive iterations done,
// skipped: the ladder steps skipped in this run.  A fixed run: the begin ladder, 0, 0.
int msx_ladder_current(msx_ctx *c, double *betas, int64_t *k, int64_t *skipped) {
    if (!c) return MSX_ERR_INVALID;
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_ladder_current: call msx_tempered_begin first");
    if (!betas) return fail(c, MSX_ERR_INVALID, "msx_ladder_current: bad arguments");
    long long st[2] = {0, 0};
    if (r->adaptive) {
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(betas, r->d_beta, sizeof(double) * (size_t)r->T, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(st, r->d_kstate, sizeof(st), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_ladder_current: ") + hipGetErrorString(e));
    } else {
        memcpy(betas, r->beta, sizeof(double) * (size_t)r->T);
    }
    if (k) *k = (int64_t)st[0];
    if (skipped) *skipped = (int64_t)st[1];
    return MSX_OK;
}

// The ladders the last collected chunk of `slot` ran with, [nsteps][T], until the slot is enqueued again.  A fixed run: the
// begin ladder in every row.
int msx_ladder_betas(msx_ctx *c, int32_t slot, double *out) {
    if (!c) return MSX_ERR_INVALID;
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_ladder_betas: call msx_tempered_begin first");
    if (slot < 0 || slot > 1 || !out) return fail(c, MSX_ERR_INVALID, "msx_ladder_betas: bad arguments");
    const TemperedRun::Slot &sl = r->slot[slot];
    if (sl.busy || !sl.collected) return fail(c, MSX_ERR_STATE, "msx_ladder_betas: no collected chunk in this slot");
    if (r->adaptive) {
        memcpy(out, tempered_out(r, sl.h_out, sl.nsteps).betas, sizeof(double) * (size_t)(sl.nsteps * r->T));
    } else {
        for (int64_t st = 0; st < sl.nsteps; ++st) memcpy(out + st * r->T, r->beta, sizeof(double) * (size_t)r->T);
    }
    return MSX_OK;
}

// One ladder step on the host: the inline pieces tempered_adapt_kernel calls (tempered_kernels.h), in its order.  No
// context, no GPU.  betas (T) strictly descending, counts (T - 1) the iteration's swaps; betas_out (T); *skipped 0 or 1.
int msx_ladder_step(int32_t ntemps, const double *betas, const int64_t *counts, int64_t nw, int64_t k, double lag, double time,
                    double *betas_out, int32_t *skipped) {
    if (ntemps < 1 || ntemps > MSX_MAX_GROUP || !betas || !betas_out || (!counts && ntemps > 1) || nw < 1 || k < 0) return MSX_ERR_INVALID;
    if (!std::isfinite(lag) || !(lag > 0.0) || !std::isfinite(time) || !(time >= 1.0)) return MSX_ERR_INVALID;
    const int T = ntemps;
    double Ti[MSX_MAX_GROUP], rr[MSX_MAX_GROUP], g[MSX_MAX_GROUP], cs[MSX_MAX_GROUP], nb[MSX_MAX_GROUP];
    for (int t = 0; t < T; ++t) betas_out[t] = nb[t] = betas[t];
    if (skipped) *skipped = 0;
    if (T <= 2) return MSX_OK;
    for (int t = 0; t < T; ++t) Ti[t] = 1.0 / betas[t];
    for (int t = 0; t < T - 1; ++t) rr[t] = (double)counts[t] / (double)nw;
    const double kappa = ladder_kappa((double)k, lag, time);
    for (int p = 1; p < T; ++p) g[p] = ladder_gap(p, T, Ti, rr, kappa);
    ladder_sums(T, g, cs);
    const double span = Ti[T - 1] - Ti[0];
    for (int p = 1; p < T - 1; ++p) nb[p] = ladder_place(Ti[0], span, cs[p], cs[T - 1]);
    if (!ladder_valid(T, nb)) {
        if (skipped) *skipped = 1;
        return MSX_OK;
    }
    for (int t = 0; t < T; ++t) betas_out[t] = nb[t];
    return MSX_OK;
}

// The chunk's host randomness -- the T members' general layouts [nsteps][T][2][ns], kind [nsteps][T], indices rung-local,
// swap_logu [nsteps][T - 1][nw] -- checked (run_pack_moves' checks: every index is dereferenced on the device) and packed
// into the slot's pinned staging in the device's order [nsteps][2][T][ns].  nullptr, or what is wrong.
static const char *tempered_pack(const TemperedRun *r, char *h_in, int64_t nsteps, const int32_t *sidx, const int32_t *cidx, const int32_t *kind,
                                 const int32_t *p1, const int32_t *p2, const double *g, const double *fac, const double *logu,
                                 const double *swap_logu) {
    const int64_t ns = r->ns, T = r->T;
    const uint32_t mw = (uint32_t)r->nw, mh = (uint32_t)ns;
    for (int64_t i = 0; i < nsteps * T; ++i)
        if (kind[i] != MSX_MOVE_STRETCH && kind[i] != MSX_MOVE_DE) return "kind out of range";
    for (int64_t i = 0; i < nsteps * T; ++i)
        if (kind[i] == MSX_MOVE_DE && r->nw < 4) return "the DE move needs two distinct walkers in each half: at least 4 walkers";
    const int64_t n = nsteps * T * 2 * ns;
    for (int64_t i = 0; i < n; ++i) {
        if ((uint32_t)sidx[i] >= mw || (uint32_t)cidx[i] >= mw || (uint32_t)p1[i] >= mh || (uint32_t)p2[i] >= mh)
            return "walker / partner index out of range";
        if (kind[i / (2 * ns)] == MSX_MOVE_DE && p1[i] == p2[i]) return "a DE entry needs two distinct walkers (p1 != p2)";
    }
    const TemperedIn P = tempered_in(r, h_in, nsteps);
    for (int64_t st = 0; st < nsteps; ++st)
        for (int64_t t = 0; t < T; ++t)
            for (int h = 0; h < 2; ++h) {
                const int64_t src = ((st * T + t) * 2 + h) * ns, dst = ((st * 2 + h) * T + t) * ns;
                memcpy(P.g + dst, g + src, sizeof(double) * ns); memcpy(P.fac + dst, fac + src, sizeof(double) * ns);
                memcpy(P.logu + dst, logu + src, sizeof(double) * ns);
                memcpy(P.sidx + dst, sidx + src, sizeof(int32_t) * ns); memcpy(P.cidx + dst, cidx + src, sizeof(int32_t) * ns);
                for (int64_t j = 0; j < ns; ++j) {  // resolved to ensemble indices, as run_pack_moves does
                    P.c1[dst + j] = (int32_t)(t * r->nw + cidx[src + p1[src + j]]);
                    P.c2[dst + j] = (int32_t)(t * r->nw + cidx[src + p2[src + j]]);
                }
            }
    memcpy(P.kind, kind, sizeof(int32_t) * nsteps * T);
    if (T > 1) memcpy(P.swap_logu, swap_logu, sizeof(double) * nsteps * (T - 1) * r->nw);
    return nullptr;
}

// The chunk's rows appended to the run's series on the compute stream (series_put_chunk's rules: growth at enqueue time, in
// stream order).  The slot's chain [st][T][nw][ndim] is [st][T nw][ndim]: series_put_kernel as it is; ll and lpr [st][T nw]
// are one-column chunks going to columns 0 and 1 of the density series.
static hipError_t tempered_put_chunk(TemperedRun *r, const TemperedOut &out, int64_t nsteps, hipStream_t compute) {
    const int64_t W = (int64_t)r->T * r->nw, row0 = r->series_row;
    if (msx_series *sr = r->s_chain) {
        hipError_t e = series_reserve(sr, row0 + nsteps, row0, compute);
        if (e != hipSuccess) return e;
        const int64_t total = nsteps * W * r->ndim;
        hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, compute, (const double *)out.chain, nsteps, W,
                           (int32_t)r->ndim, sr->d_rows, sr->cap, row0);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        sr->rows = row0 + nsteps;
    }
    if (msx_series *sr = r->s_dens) {
        hipError_t e = series_reserve(sr, row0 + nsteps, row0, compute);
        if (e != hipSuccess) return e;
        const int64_t total = nsteps * W;
        const double *src[2] = {out.ll, out.lpr};
        for (int col = 0; col < 2; ++col) {
            hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, compute, src[col], nsteps, W, (int32_t)1,
                               sr->d_rows + (int64_t)col * W * sr->cap, sr->cap, row0);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        sr->rows = row0 + nsteps;
    }
    r->series_row = row0 + nsteps;
    return hipSuccess;
}

static MoveDrawTable tempered_members(int32_t T, int64_t nw, const uint64_t *seeds) {
    MoveDrawTable Tb;
    memset(&Tb, 0, sizeof(Tb));
    for (int t = 0; t < T; ++t) {
        Tb.seed[t] = (unsigned long long)seeds[t];
        Tb.M.astart[t] = (int32_t)(t * (nw / 2)); Tb.M.nh[t] = (int32_t)nw; Tb.M.off[t] = (int32_t)(t * nw);
    }
    return Tb;
}

struct TemperedDraw { const uint64_t *seeds; const msx_move_set *set; int64_t first_iter; };

static int tempered_enqueue(msx_ctx *c, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                            const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                            const double *logu, const double *swap_logu, const TemperedDraw *draw) {
    if (!c) return MSX_ERR_INVALID;
    const std::string w(who);
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, w + ": call msx_tempered_begin first");
    const bool args_ok = draw ? (draw->seeds && draw->set) : (sidx && cidx && kind && p1 && p2 && g && fac && logu && (swap_logu || r->T == 1));
    if (slot < 0 || slot > 1 || nsteps < 1 || nsteps > r->cap_steps || !args_ok) return fail(c, MSX_ERR_INVALID, w + ": bad arguments");
    if (r->failed) return fail(c, MSX_ERR_STATE, w + ": an earlier enqueue failed part-way; end this run (msx_tempered_end) and begin again");
    TemperedRun::Slot &sl = r->slot[slot];
    if (sl.busy) return fail(c, MSX_ERR_STATE, w + ": slot not collected yet");
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, w + ": no problem staged");
    MoveSetDev S;
    if (draw) {
        if (r->nw > kDrawMaxWalkers || draw->first_iter < 0)
            return fail(c, MSX_ERR_INVALID, w + ": the device generator takes up to 4096 walkers per rung and a first iteration >= 0");
        if (const char *why = move_set_dev(draw->set, r->ndim, r->nw, &S)) return fail(c, MSX_ERR_INVALID, w + ": " + why);
    } else if (const char *why = tempered_pack(r, sl.h_in, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu, swap_logu)) {
        return fail(c, MSX_ERR_INVALID, w + ": " + why);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    r->enqueued = true;
    c->P.smp_on = 0;  // (the plain evaluation)
    c->P.smp_defer = 0;
    const int T = r->T, ndim = r->ndim;
    const int64_t ns = r->ns, nw = r->nw, H = T * ns;
    const TemperedIn in = tempered_in(r, sl.d_in, nsteps);
    const TemperedOut out = tempered_out(r, sl.d_out, nsteps);
    hipStream_t s = c->stream;
    hipError_t e = hipSuccess;
    int rc = MSX_OK;
    if (draw) {
        // (the slot was collected: no launch still reads its arrays, and the stream orders these before the half-steps)
        const MoveDrawTable Tb = tempered_members(T, nw, draw->seeds);
        hipLaunchKernelGGL(moves_draw_kernel, dim3((unsigned)nsteps, (unsigned)T), dim3(kDrawThreads), 0, s, Tb, S, draw->first_iter, (int32_t)ndim, 1,
                           H, in.sidx, in.cidx, in.c1, in.c2, in.g, in.fac, in.logu, in.kind);
        e = hipGetLastError();
        if (e == hipSuccess && T > 1) {
            hipLaunchKernelGGL(tempered_swap_draw_kernel, dim3((unsigned)nsteps, (unsigned)(T - 1), (unsigned)((nw + 255) / 256)), dim3(256), 0, s,
                               (unsigned long long)draw->seeds[0], draw->first_iter, (int32_t)nw, in.swap_logu);
            e = hipGetLastError();
        }
    } else {
        e = hipMemcpyAsync(sl.d_in, sl.h_in, r->in_bytes(nsteps), hipMemcpyHostToDevice, r->up);
        if (e == hipSuccess) e = hipEventRecord(sl.in_ready, r->up);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, sl.in_ready, 0);
    }
    if (e == hipSuccess) e = hipMemsetAsync(out.worst, 0, sizeof(int32_t) * MSX_MAX_GROUP, s);
    TemperedStepArgs A;
    memset(&A, 0, sizeof(A));
    A.coords = r->d_coords; A.ll = r->d_ll; A.lpr = r->d_lpr; A.q = r->d_q; A.new_lpr = r->d_new_lpr; A.new_ll = r->d_new_ll;
    A.st_lpr = r->d_st_lpr; A.st_ll = r->d_st_ll; A.nacc = r->d_nacc; A.ndim = ndim; A.nw = (int32_t)nw; A.ns = (int32_t)ns; A.worst = out.worst;
    memcpy(A.beta, r->beta, sizeof(A.beta));
    TemperedAdaptArgs D;
    memset(&D, 0, sizeof(D));
    D.beta = r->d_beta; D.nswap = r->d_nswap; D.prev = r->d_prev; D.state = r->d_kstate; D.nw = (double)nw; D.lag = r->lag; D.time = r->time;
    D.ntemps = T;
    TemperedSwapArgs W;
    memset(&W, 0, sizeof(W));
    W.coords = r->d_coords; W.ll = r->d_ll; W.lpr = r->d_lpr; W.nswap = r->d_nswap; W.ntemps = T; W.nw = (int32_t)nw; W.ndim = ndim;
    memcpy(W.db, r->db, sizeof(W.db));
    auto half_arrays = [&](int64_t j) {  // half-step j of the chunk
        const int64_t o = j * H;
        return MoveChunk{in.g + o, in.fac + o, in.logu + o, in.sidx + o, in.c1 + o, in.c2 + o, in.kind + (j / 2) * T};
    };
    for (int64_t st = 0; st < nsteps && e == hipSuccess && rc == MSX_OK; ++st) {
        for (int k = 0; k < 3 && e == hipSuccess && rc == MSX_OK; ++k) {  // propose 0 | apply 0, propose 1 | apply 1
            A.a_on = k > 0; A.p_on = k < 2;
            if (A.a_on) A.a = half_arrays(2 * st + k - 1);
            if (A.p_on) A.p = half_arrays(2 * st + k);
            if (r->adaptive) hipLaunchKernelGGL(tempered_step_adaptive_kernel, dim3((unsigned)T), dim3(256), 0, s, A, (const double *)r->d_beta);
            else hipLaunchKernelGGL(tempered_step_kernel, dim3((unsigned)T), dim3(256), 0, s, A);
            e = hipGetLastError();
            if (e != hipSuccess || !A.p_on) continue;
            rc = msx_logprob_batch_dev(c, MSX_MODE_LOGPRIOR, r->d_q, H, ndim, r->d_new_lpr, r->d_st_lpr, s, 0);
            if (rc == MSX_OK) rc = msx_logprob_batch_dev(c, MSX_MODE_LOGLIKE, r->d_q, H, ndim, r->d_new_ll, r->d_st_ll, s, 0);
        }
        if (e != hipSuccess || rc != MSX_OK) break;
        W.logu = in.swap_logu + st * (T - 1) * nw;
        W.chain_row = out.chain + st * T * nw * ndim; W.ll_row = out.ll + st * T * nw; W.lpr_row = out.lpr + st * T * nw;
        if (!r->adaptive) {
            hipLaunchKernelGGL(tempered_swap_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, W);
            e = hipGetLastError();
            continue;
        }
        hipLaunchKernelGGL(tempered_swap_adaptive_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, W, (const double *)r->d_beta);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        // the iteration's counts are complete once the sweep's launch has finished: a launch of its own, in stream order
        D.beta_row = out.betas + st * T;
        hipLaunchKernelGGL(tempered_adapt_kernel, dim3(1), dim3(64), 0, s, D);
        e = hipGetLastError();
    }
    // the chunk's rows into the attached series, before kernels_done: a collected chunk's rows are in place
    if (e == hipSuccess && rc == MSX_OK) e = tempered_put_chunk(r, out, nsteps, s);
    // the counters keep running while this chunk's results travel: snapshot them in stream order, then bring the slot back
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(out.nacc, r->d_nacc, sizeof(int64_t) * (size_t)(T * nw), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(out.nswap, r->d_nswap, sizeof(int64_t) * MSX_MAX_GROUP, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipEventRecord(sl.kernels_done, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipStreamWaitEvent(r->copy, sl.kernels_done, 0);
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(sl.h_out, sl.d_out, r->out_bytes(nsteps), hipMemcpyDeviceToHost, r->copy);
    if (e == hipSuccess && rc == MSX_OK) e = hipEventRecord(sl.out_ready, r->copy);
    if (e != hipSuccess || rc != MSX_OK) {
        r->failed = true;  // some of the chunk's half-steps may be queued: only the run's end from here on
        if (e != hipSuccess) return fail(c, MSX_ERR_HIP, w + ": " + hipGetErrorString(e));
        return rc;
    }
    sl.nsteps = nsteps;
    sl.busy = true;
    sl.collected = false;
    return MSX_OK;
}

int msx_tempered_enqueue(msx_ctx *c, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx, const int32_t *kind,
                         const int32_t *p1, const int32_t *p2, const double *g, const double *fac, const double *logu,
                         const double *swap_logu) {
    return tempered_enqueue(c, "msx_tempered_enqueue", slot, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu, swap_logu, nullptr);
}

int msx_tempered_enqueue_drawn(msx_ctx *c, int32_t slot, int64_t nsteps, const uint64_t *seeds, const msx_move_set *set, int64_t first_iter) {
    const TemperedDraw dd = {seeds, set, first_iter};
    return tempered_enqueue(c, "msx_tempered_enqueue_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, &dd);
}

int msx_tempered_draw(msx_ctx *c, int32_t ntemps, const uint64_t *seeds, const msx_move_set *set, int64_t first_iter, int64_t nsteps,
                      int64_t nw, int32_t ndim, int32_t *sidx, int32_t *cidx, int32_t *kind, int32_t *p1, int32_t *p2, double *g,
                      double *fac, double *logu, double *swap_logu) {
    if (!c) return MSX_ERR_INVALID;
    if (!seeds || !sidx || !cidx || !kind || !p1 || !p2 || !g || !fac || !logu || (!swap_logu && ntemps > 1) || ntemps < 1 ||
        ntemps > MSX_MAX_GROUP || nsteps < 1 || nw < 2 || (nw & 1) || nw > kDrawMaxWalkers || first_iter < 0 || ndim < 1)
        return fail(c, MSX_ERR_INVALID, "msx_tempered_draw: bad arguments (1..MSX_MAX_GROUP rungs of an even number of walkers, at most 4096)");
    MoveSetDev S;
    if (const char *why = move_set_dev(set, ndim, nw, &S)) return fail(c, MSX_ERR_INVALID, std::string("msx_tempered_draw: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t T = ntemps, ns = nw / 2, H = T * ns, L = nsteps * 2 * H, nsw = nsteps * (T - 1) * nw;
    char *d = nullptr;
    const size_t bytes = sizeof(double) * (size_t)(3 * L + nsw) + sizeof(int32_t) * (size_t)(4 * L + nsteps * T);
    HIP_TRY(c, hipMalloc((void **)&d, bytes));
    double *d_g = (double *)d, *d_fac = d_g + L, *d_logu = d_fac + L, *d_sw = d_logu + L;
    int32_t *d_sidx = (int32_t *)(d_sw + nsw), *d_cidx = d_sidx + L, *d_p1 = d_cidx + L, *d_p2 = d_p1 + L, *d_kind = d_p2 + L;
    const MoveDrawTable Tb = tempered_members(ntemps, nw, seeds);
    hipLaunchKernelGGL(moves_draw_kernel, dim3((unsigned)nsteps, (unsigned)T), dim3(kDrawThreads), 0, c->stream, Tb, S, first_iter, ndim, 0, H, d_sidx,
                       d_cidx, d_p1, d_p2, d_g, d_fac, d_logu, d_kind);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && T > 1) {
        hipLaunchKernelGGL(tempered_swap_draw_kernel, dim3((unsigned)nsteps, (unsigned)(T - 1), (unsigned)((nw + 255) / 256)), dim3(256), 0, c->stream,
                           (unsigned long long)seeds[0], first_iter, (int32_t)nw, d_sw);
        e = hipGetLastError();
    }
    std::vector<char> h(bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_tempered_draw: ") + hipGetErrorString(e));
    const double *h_g = (const double *)h.data(), *h_fac = h_g + L, *h_logu = h_fac + L, *h_sw = h_logu + L;
    const int32_t *h_sidx = (const int32_t *)(h_sw + nsw), *h_cidx = h_sidx + L, *h_p1 = h_cidx + L, *h_p2 = h_p1 + L, *h_kind = h_p2 + L;
    for (int64_t st = 0; st < nsteps; ++st)   // the device's [nsteps][2][T][ns] -> the members' [nsteps][T][2][ns]
        for (int64_t t = 0; t < T; ++t)
            for (int hh = 0; hh < 2; ++hh) {
                const int64_t dst = ((st * T + t) * 2 + hh) * ns, src = ((st * 2 + hh) * T + t) * ns;
                memcpy(g + dst, h_g + src, sizeof(double) * ns); memcpy(fac + dst, h_fac + src, sizeof(double) * ns);
                memcpy(logu + dst, h_logu + src, sizeof(double) * ns);
                memcpy(sidx + dst, h_sidx + src, sizeof(int32_t) * ns); memcpy(cidx + dst, h_cidx + src, sizeof(int32_t) * ns);
                memcpy(p1 + dst, h_p1 + src, sizeof(int32_t) * ns); memcpy(p2 + dst, h_p2 + src, sizeof(int32_t) * ns);
            }
    memcpy(kind, h_kind, sizeof(int32_t) * nsteps * T);
    if (T > 1) memcpy(swap_logu, h_sw, sizeof(double) * nsw);
    return MSX_OK;
}

int msx_tempered_collect(msx_ctx *c, int32_t slot, double *chain, double *ll_chain, double *lpr_chain, int64_t *naccept, int64_t *nswap,
                         int32_t *worst) {
    if (!c) return MSX_ERR_INVALID;
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, "msx_tempered_collect: call msx_tempered_begin first");
    if (slot < 0 || slot > 1 || !chain || !ll_chain || !lpr_chain || !naccept || !worst || (!nswap && r->T > 1))
        return fail(c, MSX_ERR_INVALID, "msx_tempered_collect: bad arguments");
    TemperedRun::Slot &sl = r->slot[slot];
    if (!sl.busy) return fail(c, MSX_ERR_STATE, "msx_tempered_collect: nothing enqueued in this slot");
    const hipError_t e = hipEventSynchronize(sl.out_ready);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_tempered_collect: ") + hipGetErrorString(e));
    const TemperedOut o = tempered_out(r, sl.h_out, sl.nsteps);
    const int64_t rows = sl.nsteps * r->T * r->nw;
    memcpy(chain, o.chain, sizeof(double) * rows * r->ndim);
    memcpy(ll_chain, o.ll, sizeof(double) * rows);
    memcpy(lpr_chain, o.lpr, sizeof(double) * rows);
    memcpy(naccept, o.nacc, sizeof(int64_t) * r->T * r->nw);
    if (r->T > 1) memcpy(nswap, o.nswap, sizeof(int64_t) * (r->T - 1));
    memcpy(worst, o.worst, sizeof(int32_t) * r->T);
    sl.busy = false;
    sl.collected = true;
    return MSX_OK;
}

int msx_tempered_end(msx_ctx *c, double *coords, double *ll, double *lpr) {
    if (!c) return MSX_ERR_INVALID;
    TemperedRun *r = c->tmp;
    if (!r) return MSX_OK;
    const int64_t W = (int64_t)r->T * r->nw;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && coords) e = hipMemcpy(coords, r->d_coords, sizeof(double) * (size_t)(W * r->ndim), hipMemcpyDeviceToHost);
    if (e == hipSuccess && ll) e = hipMemcpy(ll, r->d_ll, sizeof(double) * (size_t)W, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lpr) e = hipMemcpy(lpr, r->d_lpr, sizeof(double) * (size_t)W, hipMemcpyDeviceToHost);
    tempered_free(c);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_tempered_end: ") + hipGetErrorString(e));
    return MSX_OK;
}

// ---- device chain series ------------------------------------------------------------------------
static constexpr size_t kSeriesStageBytes = (size_t)64 << 20;   // append / read move rows through 64 MB pieces
static constexpr size_t kAcfPartBudget = (size_t)256 << 20;     // acf's partial sums per launch (lag ranges cut to fit)

// a scratch block of at least `bytes` (a smaller one is retired while a run is attached, freed otherwise)
static hipError_t series_scratch(msx_series *sr, size_t bytes) {
    if (bytes <= sr->scratch_bytes) return hipSuccess;
    if (sr->d_scratch) {
        if (sr->run || sr->trun || sr->gtrun) sr->retired.push_back(sr->d_scratch);
        else {
            (void)hipStreamSynchronize(sr->stream);
            (void)hipFree(sr->d_scratch);
        }
    }
    sr->d_scratch = nullptr;
    sr->scratch_bytes = 0;
    hipError_t e = hipMalloc((void **)&sr->d_scratch, bytes);
    if (e == hipSuccess) sr->scratch_bytes = bytes;
    return e;
}

// readers of the rows: behind the latest growth copy (queued on a run's compute stream, possibly behind chunks in flight)
static hipError_t series_wait_growth(msx_series *sr) {
    return sr->grown_set ? hipStreamWaitEvent(sr->stream, sr->grown, 0) : hipSuccess;
}

// frees what growth retired (no run attached: nothing queued reads it; the series' stream and the growth copy are done)
static void series_release(msx_series *sr) {
    if (sr->retired.empty()) return;
    (void)hipStreamSynchronize(sr->stream);
    if (sr->grown_set) (void)hipEventSynchronize(sr->grown);
    for (void *p : sr->retired) (void)hipFree(p);
    sr->retired.clear();
}

int msx_series_create(msx_ctx *c, int64_t nw, int32_t ndim, int32_t k, const int64_t *counts, int64_t cap_hint, msx_series **out) {
    if (!out) return MSX_ERR_INVALID;
    *out = nullptr;
    if (!c) return MSX_ERR_INVALID;
    if (nw < 1 || ndim < 1 || ndim > MSX_MAX_DIM || k < 1 || k > MSX_MAX_GROUP || !counts || cap_hint < 0)
        return fail(c, MSX_ERR_INVALID, "msx_series_create: bad arguments");
    int64_t tot = 0;
    for (int m = 0; m < k; ++m) {
        if (counts[m] < 1) return fail(c, MSX_ERR_INVALID, "msx_series_create: every member needs at least one walker");
        tot += counts[m];
    }
    if (tot != nw) return fail(c, MSX_ERR_INVALID, "msx_series_create: the members' walker counts do not add up to nw");
    HIP_TRY(c, hipSetDevice(c->device));
    msx_series *sr = new msx_series;
    sr->device = c->device; sr->nw = nw; sr->ndim = ndim;
    sr->off.assign(1, 0);
    for (int m = 0; m < k; ++m) sr->off.push_back(sr->off.back() + counts[m]);
    hipError_t e = hipStreamCreateWithFlags(&sr->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sr->grown, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&sr->d_off, sizeof(int64_t) * sr->off.size());
    if (e == hipSuccess) e = hipMemcpy(sr->d_off, sr->off.data(), sizeof(int64_t) * sr->off.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && cap_hint > 0) {
        e = series_reserve(sr, cap_hint, 0, sr->stream);
        sr->grown_set = false;
    }
    if (e != hipSuccess) {
        msx_series_destroy(sr);
        return fail(c, MSX_ERR_HIP, std::string("msx_series_create: ") + hipGetErrorString(e));
    }
    *out = sr;
    return MSX_OK;
}

void msx_series_destroy(msx_series *sr) {
    if (!sr) return;
    (void)hipSetDevice(sr->device);
    if (sr->run) {  // a run still appends to it: let what it queued finish, and detach it
        SamplerRun *r = sr->run;
        if (r->series == sr) r->series = nullptr;
        (void)hipDeviceSynchronize();
    }
    if (sr->trun) {  // ... or a tempered run
        TemperedRun *r = sr->trun;
        if (r->s_chain == sr) r->s_chain = nullptr;
        if (r->s_dens == sr) r->s_dens = nullptr;
        (void)hipDeviceSynchronize();
    }
    if (sr->gtrun) {  // ... or a group's
        group_tempered_detach(sr);
        (void)hipDeviceSynchronize();
    }
    if (sr->stream) (void)hipStreamSynchronize(sr->stream);
    if (sr->grown_set) (void)hipEventSynchronize(sr->grown);
    for (void *p : sr->retired) (void)hipFree(p);
    if (sr->d_rows) (void)hipFree(sr->d_rows);
    if (sr->d_scratch) (void)hipFree(sr->d_scratch);
    if (sr->d_off) (void)hipFree(sr->d_off);
    if (sr->grown) (void)hipEventDestroy(sr->grown);
    if (sr->stream) (void)hipStreamDestroy(sr->stream);
    delete sr;
}

const char *msx_series_last_error(msx_series *sr) { return sr ? sr->err.c_str() : "null series"; }

int msx_series_rows(msx_series *sr, int64_t *out) {
    if (!sr || !out) return MSX_ERR_INVALID;
    *out = sr->rows;
    return MSX_OK;
}

// the attach checks and the attach itself, for msx_sampler_attach_series and msx_group_sampler_attach_series
static int series_attach(std::string *err, msx_series *sr, SamplerRun *r, int device, int64_t at_row, const char *who, const char *begin) {
    const std::string w(who);
    if (!sr) { *err = w + ": bad arguments"; return MSX_ERR_INVALID; }
    if (!r) { *err = w + ": call " + begin + " first"; return MSX_ERR_STATE; }
    if (r->steps_done > 0 || r->slot[0].busy || r->slot[1].busy || r->series) {
        *err = w + ": attach once, between " + begin + " and the run's first enqueue";
        return MSX_ERR_STATE;
    }
    if (sr->run || sr->trun || sr->gtrun) { *err = w + ": the series is attached to another run in flight"; return MSX_ERR_STATE; }
    if (sr->device != device) { *err = w + ": the series lives on another device"; return MSX_ERR_INVALID; }
    bool same = sr->nw == r->nw && sr->ndim == r->ndim && sr->off.size() == r->m_nw.size() + 1;
    for (size_t m = 0; same && m < r->m_nw.size(); ++m) same = sr->off[m + 1] - sr->off[m] == r->m_nw[m];
    if (!same) { *err = w + ": the series' walkers, members or dimensions differ from the run's"; return MSX_ERR_INVALID; }
    if (at_row < 0 || at_row > sr->rows) { *err = w + ": at_row must lie in 0 .. the rows the series holds"; return MSX_ERR_INVALID; }
    series_release(sr);
    sr->rows = at_row;   // (rows at or after at_row are dropped: the run overwrites them)
    sr->run = r;
    r->series = sr;
    r->series_row = at_row;
    return MSX_OK;
}

int msx_sampler_attach_series(msx_ctx *c, msx_series *sr, int64_t at_row) {
    if (!c) return MSX_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    return series_attach(&c->err, sr, c->smp, c->device, at_row, "msx_sampler_attach_series", "msx_sampler_begin");
}

int msx_group_sampler_attach_series(msx_group *g, msx_series *sr, int64_t at_row) {
    if (!g) return MSX_ERR_INVALID;
    HIP_TRY(g, hipSetDevice(g->device));
    return series_attach(&g->err, sr, g->run ? g->run->r : nullptr, g->device, at_row, "msx_group_sampler_attach_series",
                         "msx_group_sampler_begin");
}

// A tempered run's two series: the T rungs are the T members, rung 0 first.  series_attach's rules.
int msx_series_attach_tempered(msx_ctx *c, msx_series *chain, msx_series *dens, int64_t at_row) {
    if (!c) return MSX_ERR_INVALID;
    const std::string w("msx_series_attach_tempered");
    if (!chain && !dens) return fail(c, MSX_ERR_INVALID, w + ": bad arguments (give the chain's series, the densities' or both)");
    TemperedRun *r = c->tmp;
    if (!r) return fail(c, MSX_ERR_STATE, w + ": call msx_tempered_begin first");
    if (r->enqueued || r->failed || r->slot[0].busy || r->slot[1].busy || r->s_chain || r->s_dens)
        return fail(c, MSX_ERR_STATE, w + ": attach once, between msx_tempered_begin and the run's first enqueue");
    HIP_TRY(c, hipSetDevice(c->device));
    msx_series *both[2] = {chain, dens};
    const int32_t want_dim[2] = {r->ndim, 2};
    if (chain == dens) return fail(c, MSX_ERR_INVALID, w + ": the chain and the densities need a series each");
    for (int i = 0; i < 2; ++i) {
        msx_series *sr = both[i];
        if (!sr) continue;
        if (sr->run || sr->trun || sr->gtrun) return fail(c, MSX_ERR_STATE, w + ": the series is attached to another run in flight");
        if (sr->device != c->device) return fail(c, MSX_ERR_INVALID, w + ": the series lives on another device");
        bool same = sr->nw == (int64_t)r->T * r->nw && sr->ndim == want_dim[i] && (int64_t)sr->off.size() == (int64_t)r->T + 1;
        for (int t = 0; same && t < r->T; ++t) same = sr->off[t + 1] - sr->off[t] == r->nw;
        if (!same)
            return fail(c, MSX_ERR_INVALID, w + ": a series needs ntemps members of nw walkers each and the run's ndim (the densities: ndim = 2)");
        if (at_row < 0 || at_row > sr->rows) return fail(c, MSX_ERR_INVALID, w + ": at_row must lie in 0 .. the rows each series holds");
    }
    for (msx_series *sr : both) {
        if (!sr) continue;
        series_release(sr);
        sr->rows = at_row;   // (rows at or after at_row are dropped: the run overwrites them)
        sr->trun = r;
    }
    r->s_chain = chain;
    r->s_dens = dens;
    r->series_row = at_row;
    return MSX_OK;
}

int msx_series_append(msx_series *sr, const double *rows, int64_t nrows) {
    if (!sr) return MSX_ERR_INVALID;
    if (!rows || nrows < 1) return fail(sr, MSX_ERR_INVALID, "msx_series_append: bad arguments");
    if (sr->run || sr->trun || sr->gtrun) return fail(sr, MSX_ERR_STATE, "msx_series_append: a run in flight appends to this series");
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t per = sr->nw * sr->ndim;
    const int64_t piece = std::max<int64_t>(1, (int64_t)(kSeriesStageBytes / (sizeof(double) * (size_t)per)));
    HIP_TRY(sr, series_reserve(sr, sr->rows + nrows, sr->rows, sr->stream));
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * (size_t)(std::min(piece, nrows) * per)));
    for (int64_t p = 0; p < nrows; p += piece) {
        const int64_t cnt = std::min(piece, nrows - p), total = cnt * per;
        HIP_TRY(sr, hipMemcpyAsync(sr->d_scratch, rows + p * per, sizeof(double) * (size_t)total, hipMemcpyHostToDevice, sr->stream));
        hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sr->stream, (const double *)sr->d_scratch,
                           cnt, sr->nw, sr->ndim, sr->d_rows, sr->cap, sr->rows + p);
        HIP_TRY(sr, hipGetLastError());
    }
    HIP_TRY(sr, hipStreamSynchronize(sr->stream));
    sr->rows += nrows;
    return MSX_OK;
}

int msx_series_read(msx_series *sr, int64_t row0, int64_t nrows, double *out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!out || row0 < 0 || nrows < 1 || row0 + nrows > sr->rows) return fail(sr, MSX_ERR_INVALID, "msx_series_read: bad arguments (rows past the series)");
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t per = sr->nw * sr->ndim;
    const int64_t piece = std::max<int64_t>(1, (int64_t)(kSeriesStageBytes / (sizeof(double) * (size_t)per)));
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * (size_t)(std::min(piece, nrows) * per)));
    HIP_TRY(sr, series_wait_growth(sr));
    for (int64_t p = 0; p < nrows; p += piece) {
        const int64_t cnt = std::min(piece, nrows - p), total = cnt * per;
        hipLaunchKernelGGL(series_get_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sr->stream, (const double *)sr->d_rows,
                           sr->cap, row0 + p, cnt, sr->nw, sr->ndim, (double *)sr->d_scratch);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(out + p * per, sr->d_scratch, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, sr->stream));
        HIP_TRY(sr, hipStreamSynchronize(sr->stream));
    }
    return MSX_OK;
}

int msx_series_acf(msx_series *sr, int64_t n, int64_t discard, int64_t thin, int64_t lag0, int64_t nlag, uint32_t dim_mask,
                   double *f_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!f_out || n < 1 || n > sr->rows || discard < 0 || thin < 1 || lag0 < 0 || nlag < 1)
        return fail(sr, MSX_ERR_INVALID, "msx_series_acf: bad arguments (n must lie in 1 .. the rows the series holds)");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (lag0 + nlag > np) return fail(sr, MSX_ERR_INVALID, "msx_series_acf: lags past the thinned chain's length");
    AcfDims dims = {};
    for (int d = 0; d < sr->ndim; ++d)
        if (dim_mask >> d & 1u) dims.d[dims.nd++] = d;
    if (dims.nd == 0 || (dim_mask >> sr->ndim) != 0) return fail(sr, MSX_ERR_INVALID, "msx_series_acf: dim_mask names no dimension, or one past ndim");
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int k = (int)sr->off.size() - 1, nd = dims.nd;
    const int64_t nser = (int64_t)nd * sr->nw, nsuper = (np + kAcfSuper - 1) / kAcfSuper;
    // lags per launch: whole tiles, as many as the partial sums' budget allows
    const int64_t per_lag = nser * nsuper * (int64_t)sizeof(double);
    int64_t sub = std::max<int64_t>(1, (int64_t)kAcfPartBudget / per_lag / kAcfLagTile) * kAcfLagTile;
    sub = std::min(sub, nlag);
    // scratch: [mean nser | part0 nser * nsuper | part nser * nsuper * sub | f k * nd * sub]
    const size_t doubles = (size_t)(nser + nser * nsuper + nser * nsuper * sub + (int64_t)k * nd * sub);
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * doubles));
    double *d_mean = (double *)sr->d_scratch, *d_part0 = d_mean + nser, *d_part = d_part0 + nser * nsuper;
    double *d_f = d_part + nser * nsuper * sub;
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    hipLaunchKernelGGL(acf_mean_kernel, dim3((unsigned)nser), dim3(kAcfMeanThreads), 0, st, (const double *)sr->d_rows, sr->cap,
                       sr->nw, dims, np, discard, thin, d_mean);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(acf_lag_kernel, dim3((unsigned)nser, 1u, (unsigned)nsuper), dim3(kAcfThreads), 0, st, (const double *)sr->d_rows,
                       sr->cap, sr->nw, dims, np, discard, thin, (const double *)d_mean, (int64_t)0, (int64_t)1, d_part0, nsuper, (int64_t)1);
    HIP_TRY(sr, hipGetLastError());
    std::vector<double> h((size_t)((int64_t)k * nd * sub));
    for (int64_t lb = lag0; lb < lag0 + nlag; lb += sub) {
        const int64_t cnt = std::min(sub, lag0 + nlag - lb), nout = (int64_t)k * nd * cnt;
        hipLaunchKernelGGL(acf_lag_kernel, dim3((unsigned)nser, (unsigned)((cnt + kAcfLagTile - 1) / kAcfLagTile), (unsigned)nsuper),
                           dim3(kAcfThreads), 0, st, (const double *)sr->d_rows, sr->cap, sr->nw, dims, np, discard, thin,
                           (const double *)d_mean, lb, cnt, d_part, nsuper, cnt);
        HIP_TRY(sr, hipGetLastError());
        hipLaunchKernelGGL(acf_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, (const double *)d_part,
                           (const double *)d_part0, nsuper, cnt, sr->nw, (int32_t)nd, (const int64_t *)sr->d_off, (int32_t)k, cnt, d_f);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(h.data(), d_f, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, st));
        HIP_TRY(sr, hipStreamSynchronize(st));
        for (int m = 0; m < k; ++m)
            for (int q = 0; q < nd; ++q)
                memcpy(f_out + ((int64_t)m * sr->ndim + dims.d[q]) * nlag + (lb - lag0), h.data() + ((int64_t)m * nd + q) * cnt,
                       sizeof(double) * (size_t)cnt);
    }
    return MSX_OK;
}

// ---- block means and log-mean-exponentials of a series column (evidence_kernels.h) ------------------
int msx_series_evidence(msx_series *sr, int64_t n, int64_t discard, int64_t thin, int32_t col, const double *db, int32_t nblocks,
                        double *mean_out, double *lme_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!mean_out || discard < 0 || thin < 1 || (db && !lme_out))
        return fail(sr, MSX_ERR_INVALID, "msx_series_evidence: bad arguments (discard >= 0, thin >= 1, lme_out with db)");
    if (n < 1 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, "msx_series_evidence: n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (np < 1) return fail(sr, MSX_ERR_RANGE, "msx_series_evidence: the selection rows[0:n][discard::thin] is empty");
    if (col < 0 || col >= sr->ndim) return fail(sr, MSX_ERR_RANGE, "msx_series_evidence: col outside the series");
    if (nblocks < 1 || nblocks > kEvdMaxBlocks || nblocks > np)
        return fail(sr, MSX_ERR_RANGE, "msx_series_evidence: nblocks must lie in 1 .. min(n', 64)");
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int k = (int)sr->off.size() - 1;
    const int64_t B = nblocks, parts = sr->nw * B;
    // scratch: [psum nw B | pmax nw B | pexp nw B | mmax k B | mean k (B + 1) | lme k (B + 1)]
    const int64_t nout = (int64_t)k * (B + 1);
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * (size_t)(3 * parts + k * B + 2 * nout)));
    double *d_psum = (double *)sr->d_scratch, *d_pmax = d_psum + parts, *d_pexp = d_pmax + parts, *d_mmax = d_pexp + parts;
    double *d_mean = d_mmax + k * B, *d_lme = d_mean + nout;
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    const dim3 grid((unsigned)sr->nw, (unsigned)B);
    hipLaunchKernelGGL(evd_part_kernel, grid, dim3(kEvdThreads), 0, st, (const double *)sr->d_rows, sr->cap, sr->nw, col, np, discard, thin,
                       nblocks, d_psum, d_pmax);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(evd_mean_kernel, dim3((unsigned)k), dim3(kEvdMaxBlocks), 0, st, (const double *)d_psum, (const double *)d_pmax,
                       (const int64_t *)sr->d_off, np, nblocks, d_mean, d_mmax);
    HIP_TRY(sr, hipGetLastError());
    if (db) {
        EvdDb D;
        memset(&D, 0, sizeof(D));
        for (int m = 0; m < k; ++m) D.v[m] = db[m];
        hipLaunchKernelGGL(evd_exp_kernel, grid, dim3(kEvdThreads), 0, st, (const double *)sr->d_rows, sr->cap, sr->nw, col, np, discard, thin,
                           nblocks, (const int64_t *)sr->d_off, (int32_t)k, D, (const double *)d_mmax, d_pexp);
        HIP_TRY(sr, hipGetLastError());
        hipLaunchKernelGGL(evd_lme_kernel, dim3((unsigned)k), dim3(kEvdMaxBlocks), 0, st, (const double *)d_pexp, (const double *)d_mmax,
                           (const int64_t *)sr->d_off, np, nblocks, D, d_lme);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(lme_out, d_lme, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(sr, hipMemcpyAsync(mean_out, d_mean, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, st));
    HIP_TRY(sr, hipStreamSynchronize(st));
    return MSX_OK;
}

// ---- split R-hat's parts and the pooled moments of a series' members (diag_kernels.h) ---------------
int msx_series_moments(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols, double *within,
                       double *var_plus, double *between, double *mean, double *cov) {
    if (!sr) return MSX_ERR_INVALID;
    if (!within || !var_plus || !between || !mean || discard < 0 || thin < 1 || ncols < 1)
        return fail(sr, MSX_ERR_INVALID, "msx_series_moments: bad arguments (discard >= 0, thin >= 1, ncols >= 1, every output but cov)");
    if (n < 1 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, "msx_series_moments: n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (np < 4) return fail(sr, MSX_ERR_RANGE, "msx_series_moments: the selection rows[0:n][discard::thin] needs at least 4 rows");
    if (ncols > MSX_MAX_DIM) return fail(sr, MSX_ERR_RANGE, "msx_series_moments: more columns than a series is wide (MSX_MAX_DIM)");
    DiagCols C;
    memset(&C, 0, sizeof(C));
    C.n = ncols;
    if (!cols && ncols != sr->ndim) return fail(sr, MSX_ERR_RANGE, "msx_series_moments: cols == NULL means all columns (ncols = ndim)");
    for (int32_t q = 0; q < ncols; ++q) {
        const uint32_t c = cols ? cols[q] : (uint32_t)q;
        if (c >= (uint32_t)sr->ndim) return fail(sr, MSX_ERR_RANGE, "msx_series_moments: a column outside the series");
        C.c[q] = (int32_t)c;
    }
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int k = (int)sr->off.size() - 1;
    const int64_t nc = ncols, npairs = cov ? nc * (nc + 1) / 2 : 0, nw = sr->nw;
    // scratch: [psum 3 nc nw | pss 2 nc nw | pcross npairs nw | mean k nc | within k nc | var_plus k nc | between k nc | cov k nc nc]
    const int64_t kc = (int64_t)k * nc, ncov = cov ? kc * nc : 0;
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * (size_t)((5 * nc + npairs) * nw + 4 * kc + ncov)));
    double *d_psum = (double *)sr->d_scratch, *d_pss = d_psum + 3 * nc * nw, *d_pcross = d_pss + 2 * nc * nw;
    double *d_mean = d_pcross + npairs * nw, *d_within = d_mean + kc, *d_vplus = d_within + kc, *d_between = d_vplus + kc;
    double *d_cov = d_between + kc;
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    hipLaunchKernelGGL(diag_sum_kernel, dim3((unsigned)nw, (unsigned)nc, 3u), dim3(kDiagThreads), 0, st, (const double *)sr->d_rows, sr->cap,
                       nw, C, np, discard, thin, d_psum);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(diag_mean_kernel, dim3((unsigned)k), dim3(MSX_MAX_DIM), 0, st, (const double *)d_psum, (const int64_t *)sr->d_off, nw,
                       (int32_t)nc, np, d_mean);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(diag_dev_kernel, dim3((unsigned)nw, (unsigned)nc, 2u), dim3(kDiagThreads), 0, st, (const double *)sr->d_rows, sr->cap,
                       nw, C, np, discard, thin, (const double *)d_psum, d_pss);
    HIP_TRY(sr, hipGetLastError());
    if (cov) {
        hipLaunchKernelGGL(diag_cross_kernel, dim3((unsigned)nw, (unsigned)npairs), dim3(kDiagThreads), 0, st, (const double *)sr->d_rows,
                           sr->cap, nw, C, np, discard, thin, (const int64_t *)sr->d_off, (int32_t)k, (const double *)d_mean, d_pcross);
        HIP_TRY(sr, hipGetLastError());
    }
    hipLaunchKernelGGL(diag_combine_kernel, dim3((unsigned)k), dim3(kDiagMaxPairs), 0, st, (const double *)d_psum, (const double *)d_pss,
                       (const double *)(cov ? d_pcross : nullptr), (const int64_t *)sr->d_off, nw, (int32_t)nc, np, d_within, d_vplus,
                       d_between, cov ? d_cov : nullptr);
    HIP_TRY(sr, hipGetLastError());
    // (mean .. between lie side by side: one copy, then the host splits them)
    std::vector<double> hbuf((size_t)(4 * kc));
    HIP_TRY(sr, hipMemcpyAsync(hbuf.data(), d_mean, sizeof(double) * (size_t)(4 * kc), hipMemcpyDeviceToHost, st));
    if (cov) HIP_TRY(sr, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)ncov, hipMemcpyDeviceToHost, st));
    HIP_TRY(sr, hipStreamSynchronize(st));
    memcpy(mean, hbuf.data(), sizeof(double) * (size_t)kc);
    memcpy(within, hbuf.data() + kc, sizeof(double) * (size_t)kc);
    memcpy(var_plus, hbuf.data() + 2 * kc, sizeof(double) * (size_t)kc);
    memcpy(between, hbuf.data() + 3 * kc, sizeof(double) * (size_t)kc);
    return MSX_OK;
}

// ---- order statistics and binned marginals of a series (summary_kernels.h) --------------------------
static constexpr size_t kSummaryTableBudget = (size_t)64 << 20;   // global count tables per launch (columns cut to fit)

// the selection rows[0:n][discard::thin] -> n' (MSX_ERR_RANGE when n lies past the rows held or nothing is selected)
static int summary_selection(msx_series *sr, const char *who, int64_t n, int64_t discard, int64_t thin, int64_t *np_out) {
    const std::string w(who);
    if (discard < 0 || thin < 1) return fail(sr, MSX_ERR_INVALID, w + ": bad arguments (discard >= 0, thin >= 1)");
    if (n < 1 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, w + ": n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (np < 1) return fail(sr, MSX_ERR_RANGE, w + ": the selection rows[0:n][discard::thin] is empty");
    if ((np + kSumTile - 1) / kSumTile > 65535) return fail(sr, MSX_ERR_RANGE, w + ": more rows than one launch covers");
    *np_out = np;
    return MSX_OK;
}

static int summary_columns(msx_series *sr, const char *who, const uint32_t *cols, int64_t count) {
    for (int64_t j = 0; j < count; ++j) {
        const uint32_t c = cols[j];
        const bool ok = c & kColRatioBit ? (c & 0x7fff0000u) == 0 && (int)((c >> 8) & 0xffu) < sr->ndim && (int)(c & 0xffu) < sr->ndim
                                         : (int64_t)c < sr->ndim;
        if (!ok) return fail(sr, MSX_ERR_RANGE, std::string(who) + ": unknown column (a coordinate < ndim or MSX_COL_RATIO(a, b))");
    }
    return MSX_OK;
}

// edge vectors [count][ne]: ascending (equal neighbours allowed, as np.histogram allows them), no NaN
static int summary_edges(msx_series *sr, const char *who, const double *edges, int64_t count, int32_t ne) {
    for (int64_t v = 0; v < count; ++v)
        for (int32_t i = 0; i + 1 < ne; ++i)
            if (!(edges[v * ne + i] <= edges[v * ne + i + 1]))
                return fail(sr, MSX_ERR_RANGE, std::string(who) + ": every edge vector must ascend");
    return MSX_OK;
}

int msx_series_order_stats(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                           const int64_t *ranks, int32_t nranks, double *out, int64_t *count_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!cols || ncols < 1 || !ranks || nranks < 1 || !out) return fail(sr, MSX_ERR_INVALID, "msx_series_order_stats: bad arguments");
    int64_t np = 0;
    int rc = summary_selection(sr, "msx_series_order_stats", n, discard, thin, &np);
    if (rc == MSX_OK) rc = summary_columns(sr, "msx_series_order_stats", cols, ncols);
    if (rc != MSX_OK) return rc;
    const int k = (int)sr->off.size() - 1;
    for (int m = 0; m < k; ++m) {
        const int64_t N = np * (sr->off[m + 1] - sr->off[m]);
        for (int32_t r = 0; r < nranks; ++r)
            if (ranks[(int64_t)m * nranks + r] < 0 || ranks[(int64_t)m * nranks + r] >= N)
                return fail(sr, MSX_ERR_RANGE, "msx_series_order_stats: a rank outside 0 .. N_m - 1");
        if (count_out) count_out[m] = N;
    }
    HIP_TRY(sr, hipSetDevice(sr->device));
    // columns per launch: the digit histograms of k x columns jobs within the budget
    const size_t job_hist = sizeof(unsigned long long) * kSelRanks * kSelDigits;
    const int32_t ncl_max = (int32_t)std::min<size_t>(65535, std::max<size_t>(1, kSummaryTableBudget / (job_hist * (size_t)k)));
    const int32_t ncl_cap = std::min(ncols, ncl_max);
    const int64_t jobs_cap = (int64_t)k * ncl_cap;
    HIP_TRY(sr, series_scratch(sr, (job_hist + sizeof(SelState)) * (size_t)jobs_cap + sizeof(uint32_t) * (size_t)ncl_cap));
    unsigned long long *d_hist = (unsigned long long *)sr->d_scratch;
    SelState *d_state = (SelState *)(d_hist + jobs_cap * kSelRanks * kSelDigits);
    uint32_t *d_cols = (uint32_t *)(d_state + jobs_cap);
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    const dim3 grid_rows((unsigned)sr->nw, (unsigned)((np + kSumTile - 1) / kSumTile), 1u);
    std::vector<SelState> h;
    for (int32_t c0 = 0; c0 < ncols; c0 += ncl_cap) {
        const int32_t ncl = std::min(ncl_cap, ncols - c0);
        const int64_t jobs = (int64_t)k * ncl;
        HIP_TRY(sr, hipMemcpyAsync(d_cols, cols + c0, sizeof(uint32_t) * (size_t)ncl, hipMemcpyHostToDevice, st));
        for (int32_t r0 = 0; r0 < nranks; r0 += kSelRanks) {
            const int32_t nr = std::min<int32_t>(kSelRanks, nranks - r0);
            h.assign((size_t)jobs, SelState());
            for (int64_t j = 0; j < jobs; ++j) {
                SelState &s = h[(size_t)j];
                memset(&s, 0, sizeof(s));
                s.nranks = nr;
                s.nslots = 1;   // every rank starts from the empty prefix
                for (int32_t r = 0; r < nr; ++r) s.rem[r] = ranks[(j / ncl) * nranks + r0 + r];
            }
            HIP_TRY(sr, hipMemcpyAsync(d_state, h.data(), sizeof(SelState) * (size_t)jobs, hipMemcpyHostToDevice, st));
            HIP_TRY(sr, hipMemsetAsync(d_hist, 0, job_hist * (size_t)jobs, st));
            for (int p = 0; p < kSelPasses; ++p) {
                const int32_t shift = 64 - kSelDigitBits * (p + 1);
                hipLaunchKernelGGL(sel_pass_kernel, dim3(grid_rows.x, grid_rows.y, (unsigned)ncl), dim3(kSumThreads), 0, st,
                                   (const double *)sr->d_rows, sr->cap, sr->nw, np, discard, thin, (const int64_t *)sr->d_off,
                                   (int32_t)k, (const uint32_t *)d_cols, ncl, shift, (const SelState *)d_state, d_hist);
                HIP_TRY(sr, hipGetLastError());
                hipLaunchKernelGGL(sel_pick_kernel, dim3((unsigned)jobs), dim3(64), 0, st, d_state, d_hist, shift);
                HIP_TRY(sr, hipGetLastError());
            }
            HIP_TRY(sr, hipMemcpyAsync(h.data(), d_state, sizeof(SelState) * (size_t)jobs, hipMemcpyDeviceToHost, st));
            HIP_TRY(sr, hipStreamSynchronize(st));
            for (int64_t j = 0; j < jobs; ++j)
                for (int32_t r = 0; r < nr; ++r) {
                    const unsigned long long key = h[(size_t)j].prefix[r];
                    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;   // (val_of, on the host)
                    memcpy(out + ((j / ncl) * ncols + c0 + j % ncl) * nranks + r0 + r, &b, sizeof(double));
                }
        }
    }
    return MSX_OK;
}

int msx_series_hist(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                    const double *edges, int32_t nedges, int32_t closed_last, int64_t *counts_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!cols || ncols < 1 || !edges || !counts_out) return fail(sr, MSX_ERR_INVALID, "msx_series_hist: bad arguments");
    if (nedges < 2 || nedges > kHistMaxEdges) return fail(sr, MSX_ERR_RANGE, "msx_series_hist: nedges must lie in 2 .. 4097");
    const int k = (int)sr->off.size() - 1;
    int64_t np = 0;
    int rc = summary_selection(sr, "msx_series_hist", n, discard, thin, &np);
    if (rc == MSX_OK) rc = summary_columns(sr, "msx_series_hist", cols, ncols);
    if (rc == MSX_OK) rc = summary_edges(sr, "msx_series_hist", edges, (int64_t)k * ncols, nedges);
    if (rc != MSX_OK) return rc;
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t nb = nedges - 1;
    const size_t job_bytes = sizeof(double) * (size_t)nedges + sizeof(unsigned long long) * (size_t)nb;
    const int32_t ncl_cap = std::min<int32_t>(ncols, (int32_t)std::min<size_t>(65535, std::max<size_t>(1, kSummaryTableBudget / (job_bytes * (size_t)k))));
    const int64_t jobs_cap = (int64_t)k * ncl_cap;
    HIP_TRY(sr, series_scratch(sr, job_bytes * (size_t)jobs_cap + sizeof(uint32_t) * (size_t)ncl_cap));
    unsigned long long *d_counts = (unsigned long long *)sr->d_scratch;
    double *d_edges = (double *)(d_counts + jobs_cap * nb);
    uint32_t *d_cols = (uint32_t *)(d_edges + jobs_cap * nedges);
    const size_t lds = sizeof(double) * (size_t)nedges + sizeof(unsigned int) * (size_t)nb;
    if (lds > 48 * 1024) HIP_TRY(sr, hipFuncSetAttribute((const void *)hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    std::vector<double> he;
    std::vector<unsigned long long> hc;
    for (int32_t c0 = 0; c0 < ncols; c0 += ncl_cap) {
        const int32_t ncl = std::min(ncl_cap, ncols - c0);
        const int64_t jobs = (int64_t)k * ncl;
        he.resize((size_t)(jobs * nedges));
        hc.resize((size_t)(jobs * nb));
        for (int64_t j = 0; j < jobs; ++j)
            memcpy(he.data() + j * nedges, edges + ((j / ncl) * ncols + c0 + j % ncl) * nedges, sizeof(double) * (size_t)nedges);
        HIP_TRY(sr, hipMemcpyAsync(d_cols, cols + c0, sizeof(uint32_t) * (size_t)ncl, hipMemcpyHostToDevice, st));
        HIP_TRY(sr, hipMemcpyAsync(d_edges, he.data(), sizeof(double) * he.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(sr, hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * hc.size(), st));
        hipLaunchKernelGGL(hist_kernel, dim3((unsigned)sr->nw, (unsigned)((np + kSumTile - 1) / kSumTile), (unsigned)ncl), dim3(kSumThreads),
                           lds, st, (const double *)sr->d_rows, sr->cap, sr->nw, np, discard, thin, (const int64_t *)sr->d_off, (int32_t)k,
                           (const uint32_t *)d_cols, ncl, (const double *)d_edges, nedges, (int32_t)(closed_last != 0), d_counts);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(hc.data(), d_counts, sizeof(unsigned long long) * hc.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(sr, hipStreamSynchronize(st));
        for (int64_t j = 0; j < jobs; ++j)
            memcpy(counts_out + ((j / ncl) * ncols + c0 + j % ncl) * nb, hc.data() + j * nb, sizeof(int64_t) * (size_t)nb);
    }
    return MSX_OK;
}

int msx_series_hist2d(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *pairs, int32_t npairs,
                      const double *xedges, int32_t nx, const double *yedges, int32_t ny, int32_t closed_last, int64_t *counts_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!pairs || npairs < 1 || !xedges || !yedges || !counts_out) return fail(sr, MSX_ERR_INVALID, "msx_series_hist2d: bad arguments");
    if (nx < 2 || ny < 2 || nx > kHist2dMaxBins + 1 || ny > kHist2dMaxBins + 1)
        return fail(sr, MSX_ERR_RANGE, "msx_series_hist2d: 1 .. 128 bins (2 .. 129 edges) per axis");
    const int k = (int)sr->off.size() - 1;
    int64_t np = 0;
    int rc = summary_selection(sr, "msx_series_hist2d", n, discard, thin, &np);
    if (rc == MSX_OK) rc = summary_columns(sr, "msx_series_hist2d", pairs, 2 * (int64_t)npairs);
    if (rc == MSX_OK) rc = summary_edges(sr, "msx_series_hist2d", xedges, (int64_t)k * npairs, nx);
    if (rc == MSX_OK) rc = summary_edges(sr, "msx_series_hist2d", yedges, (int64_t)k * npairs, ny);
    if (rc != MSX_OK) return rc;
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t nb = (int64_t)(nx - 1) * (ny - 1);
    const size_t job_bytes = sizeof(double) * (size_t)(nx + ny) + sizeof(unsigned long long) * (size_t)nb;
    const int32_t npl_cap = std::min<int32_t>(npairs, (int32_t)std::min<size_t>(65535, std::max<size_t>(1, kSummaryTableBudget / (job_bytes * (size_t)k))));
    const int64_t jobs_cap = (int64_t)k * npl_cap;
    HIP_TRY(sr, series_scratch(sr, job_bytes * (size_t)jobs_cap + sizeof(uint32_t) * 2 * (size_t)npl_cap));
    unsigned long long *d_counts = (unsigned long long *)sr->d_scratch;
    double *d_ex = (double *)(d_counts + jobs_cap * nb), *d_ey = d_ex + jobs_cap * nx;
    uint32_t *d_cols = (uint32_t *)(d_ey + jobs_cap * ny);
    const size_t lds = sizeof(double) * (size_t)(nx + ny) + sizeof(unsigned int) * (size_t)nb;
    if (lds > 48 * 1024) HIP_TRY(sr, hipFuncSetAttribute((const void *)hist2d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    std::vector<double> hx, hy;
    std::vector<unsigned long long> hc;
    for (int32_t p0 = 0; p0 < npairs; p0 += npl_cap) {
        const int32_t npl = std::min(npl_cap, npairs - p0);
        const int64_t jobs = (int64_t)k * npl;
        hx.resize((size_t)(jobs * nx));
        hy.resize((size_t)(jobs * ny));
        hc.resize((size_t)(jobs * nb));
        for (int64_t j = 0; j < jobs; ++j) {
            const int64_t src = (j / npl) * npairs + p0 + j % npl;
            memcpy(hx.data() + j * nx, xedges + src * nx, sizeof(double) * (size_t)nx);
            memcpy(hy.data() + j * ny, yedges + src * ny, sizeof(double) * (size_t)ny);
        }
        HIP_TRY(sr, hipMemcpyAsync(d_cols, pairs + 2 * (int64_t)p0, sizeof(uint32_t) * 2 * (size_t)npl, hipMemcpyHostToDevice, st));
        HIP_TRY(sr, hipMemcpyAsync(d_ex, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(sr, hipMemcpyAsync(d_ey, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(sr, hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * hc.size(), st));
        hipLaunchKernelGGL(hist2d_kernel, dim3((unsigned)sr->nw, (unsigned)((np + kSumTile2d - 1) / kSumTile2d), (unsigned)npl),
                           dim3(kSumThreads), lds, st, (const double *)sr->d_rows, sr->cap, sr->nw, np, discard, thin,
                           (const int64_t *)sr->d_off, (int32_t)k, (const uint32_t *)d_cols, npl, (const double *)d_ex, nx,
                           (const double *)d_ey, ny, (int32_t)(closed_last != 0), d_counts);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(hc.data(), d_counts, sizeof(unsigned long long) * hc.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(sr, hipStreamSynchronize(st));
        for (int64_t j = 0; j < jobs; ++j)
            memcpy(counts_out + ((j / npl) * npairs + p0 + j % npl) * nb, hc.data() + j * nb, sizeof(int64_t) * (size_t)nb);
    }
    return MSX_OK;
}

// ---- derived posteriors ---------------------------------------------------------------------------
int msx_stage_products(msx_ctx *c, const msx_products *p) {
    if (!c || !p) return MSX_ERR_INVALID;
    if (p->struct_size != (int32_t)sizeof(msx_products))
        return fail(c, MSX_ERR_INVALID, "msx_stage_products: struct_size mismatch (header/library skew)");
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_stage_products: stage the problem first");
    if (p->nbands < 1 || p->nbands > MSX_MAX_BANDS || !p->band_kind || !p->band_i0 || !p->band_len || !p->band_w || !p->band_zero_mag)
        return fail(c, MSX_ERR_INVALID, "msx_stage_products: 1 .. MSX_MAX_BANDS product bands");
    if (p->niso < 2 || !p->iso_teff || !p->iso_mass || !p->iso_lum)
        return fail(c, MSX_ERR_INVALID, "msx_stage_products: the product isochrone needs >= 2 rows");
    for (int32_t i = 0; i + 1 < p->niso; ++i)
        if (!(p->iso_teff[i] <= p->iso_teff[i + 1])) return fail(c, MSX_ERR_INVALID, "msx_stage_products: the product isochrone must be sorted by Teff");
    const int nb = p->nbands;
    std::vector<int64_t> woff((size_t)nb);
    int64_t tot = 0;
    for (int b = 0; b < nb; ++b) {
        if (p->band_kind[b] != MSX_PB_TRAPZ && p->band_kind[b] != MSX_PB_SUM && p->band_kind[b] != MSX_PB_MEAN)
            return fail(c, MSX_ERR_RANGE, "msx_stage_products: unknown band kind");
        if (p->band_i0[b] < 0 || p->band_len[b] < 1 || p->band_i0[b] + p->band_len[b] > c->nwl)
            return fail(c, MSX_ERR_RANGE, "msx_stage_products: band weights run outside the staged grid");
        woff[(size_t)b] = tot;
        tot += p->band_len[b];
    }
    HIP_TRY(c, hipSetDevice(c->device));
    for (void *q : c->prod_allocs) (void)hipFree(q);
    c->prod_allocs.clear();
    c->d_prod_member = nullptr;  // (a restage that fails below leaves no products and no pointer to the freed record)
    c->products_staged = false;
    std::vector<void *> &tr = c->prod_allocs;
    const int64_t nn = grid_rows(c);
    int rc;
    double *d_w = nullptr, *d_tab = nullptr, *d_t = nullptr, *d_m = nullptr, *d_l = nullptr;
    int64_t *d_woff = nullptr, *d_i0 = nullptr, *d_len = nullptr;
    if ((rc = dev_alloc_copy(c, &tr, p->band_w, tot, &d_w))) return rc;
    if ((rc = dev_alloc_copy(c, &tr, woff.data(), (int64_t)nb, &d_woff))) return rc;
    if ((rc = dev_alloc_copy(c, &tr, p->band_i0, (int64_t)nb, &d_i0))) return rc;
    if ((rc = dev_alloc_copy(c, &tr, p->band_len, (int64_t)nb, &d_len))) return rc;
    HIP_TRY(c, hipMalloc((void **)&d_tab, sizeof(double) * (size_t)(nn * nb))); tr.push_back(d_tab);
    // one row of integrals per node and per copy of a component grid: the staged problem's own band kernel
    hipLaunchKernelGGL(band_integral_kernel, dim3((unsigned)nb, (unsigned)nn), dim3(256), 0, c->stream, c->d_grid, c->nwl, d_w, d_woff,
                       d_i0, d_len, nb, d_tab);
    HIP_TRY(c, hipGetLastError());
    if ((rc = dev_alloc_copy(c, &tr, p->iso_teff, (int64_t)p->niso, &d_t))) return rc;
    if ((rc = dev_alloc_copy(c, &tr, p->iso_mass, (int64_t)p->niso, &d_m))) return rc;
    if ((rc = dev_alloc_copy(c, &tr, p->iso_lum, (int64_t)p->niso, &d_l))) return rc;
    ProdMember &M = c->PM;
    memset(&M, 0, sizeof(M));
    const DevProblem &P = c->P;
    M.teff_nodes = P.teff_nodes; M.logg_nodes = P.logg_nodes; M.present = P.present;
    M.iso_t = P.iso_t; M.iso_g = P.iso_g; M.piso_t = d_t; M.piso_m = d_m; M.piso_l = d_l;
    M.band_tab = P.band_tab; M.prod_tab = d_tab;
    for (int i = 0; i < MSX_MAX_BANDS; ++i) M.pzero[i] = i < P.np ? P.pzero[i] : 1.0;
    for (int b = 0; b < nb; ++b) { M.kind[b] = p->band_kind[b]; M.zero_mag[b] = p->band_zero_mag[b]; }
    M.nt = P.nt; M.ng = P.ng; M.node_stride = P.node_stride; M.niso = P.niso; M.npiso = p->niso;
    M.nc = P.nc; M.np = P.np; M.npb = nb; M.nspec = P.nspec; M.dist_fit = P.dist_fit;
    M.grid = c->d_grid; M.kgrid = c->d_kgrid; M.pix_lo = c->d_pix_lo; M.pix_t = P.pix_t; M.nwl = c->nwl; M.npix = P.npix;
    M.median_flux = P.median_flux; M.use_av = P.use_av; M.no_spectrum = P.no_spectrum;
    M.pix_flux = P.pix_flux; M.pix_err = c->d_pix_err; M.pix_u = P.pix_u;
    memcpy(M.minv, P.minv, sizeof(M.minv));
    for (int i = 0; i < MSX_MAX_BANDS; ++i) {
        M.cmag[i] = P.cmag[i]; M.cerr[i] = P.cerr[i]; M.pmag[i] = P.pmag[i]; M.perr[i] = P.perr[i]; M.pk[i] = P.pk[i];
    }
    if ((rc = dev_alloc_copy(c, &tr, &M, (int64_t)1, &c->d_prod_member))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->products_staged = true;
    return MSX_OK;
}

// the codes against one context's tables; *need_piso: a MASS or LUM column is among them
static bool products_cols_ok(const msx_ctx *c, const uint32_t *cols, int32_t ncols, int32_t *need_piso) {
    const ProdMember &M = c->PM;
    for (int32_t j = 0; j < ncols; ++j) {
        if (!pcol_known(cols[j], 2 * M.nspec + 2, M.nspec, M.npb, M.nc, M.np)) return false;
        const uint32_t kind = cols[j] >> 24;
        if (kind == kPcolMass || kind == kPcolLum) *need_piso = 1;
    }
    return true;
}

static void products_launch(int nspec, const ProdLaunch &L, int64_t max_count, int k, hipStream_t st) {
    const dim3 grid((unsigned)((max_count + kProdThreads - 1) / kProdThreads), (unsigned)k);
    if (nspec == 2) hipLaunchKernelGGL(products_kernel<2>, grid, dim3(kProdThreads), 0, st, L);
    else hipLaunchKernelGGL(products_kernel<3>, grid, dim3(kProdThreads), 0, st, L);
}

// (need_piso < 0: the codes live on the device and were not looked at -- the product isochrone's range is then enforced)
static int products_batch_launch(msx_ctx *c, const double *d_theta, int64_t n, int32_t ndim, const uint32_t *d_cols, int32_t ncols,
                                 double *d_out, int32_t *d_status, hipStream_t st, int32_t need_piso) {
    ProdLaunch L;
    memset(&L, 0, sizeof(L));
    L.members = c->d_prod_member; L.off = nullptr; L.n_single = n;
    L.in = d_theta; L.in_sw = ndim; L.in_sr = 0; L.in_sd = 1;
    L.out = d_out; L.out_sw = ncols; L.out_sr = 0; L.out_sd = 1;
    L.row0 = 0; L.nrows = 1; L.cols = d_cols; L.ncols = ncols; L.need_piso = need_piso != 0;
    L.status = d_status; L.worst = nullptr;
    products_launch(c->P.nspec, L, n, 1, st);
    HIP_TRY(c, hipGetLastError());
    return MSX_OK;
}

static int products_batch_check(msx_ctx *c, const char *who, const void *theta, int64_t n, int32_t ndim, const void *cols, int32_t ncols,
                                const void *out, const void *status) {
    const std::string w(who);
    if (!theta || !cols || !out || !status || n < 0 || ncols < 1) return fail(c, MSX_ERR_INVALID, w + ": bad arguments");
    if (!c->problem_staged || !c->products_staged) return fail(c, MSX_ERR_STATE, w + ": no products staged (msx_stage_products)");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, w + ": ndim must be 2 * nspec + 2");
    if (ncols > MSX_MAX_PCOLS) return fail(c, MSX_ERR_RANGE, w + ": more than MSX_MAX_PCOLS columns");
    return MSX_OK;
}

int msx_products_batch_dev(msx_ctx *c, const double *d_theta, int64_t n, int32_t ndim, const uint32_t *d_cols, int32_t ncols,
                           double *d_out, int32_t *d_status, void *hip_stream) {
    if (!c) return MSX_ERR_INVALID;
    if (int rc = products_batch_check(c, "msx_products_batch_dev", d_theta, n, ndim, d_cols, ncols, d_out, d_status)) return rc;
    if (n == 0) return MSX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return products_batch_launch(c, d_theta, n, ndim, d_cols, ncols, d_out, d_status, (hipStream_t)hip_stream, -1);
}

int msx_products_batch(msx_ctx *c, const double *theta, int64_t n, int32_t ndim, const uint32_t *cols, int32_t ncols, double *out,
                       int32_t *status) {
    if (!c) return MSX_ERR_INVALID;
    if (int rc = products_batch_check(c, "msx_products_batch", theta, n, ndim, cols, ncols, out, status)) return rc;
    int32_t need_piso = 0;
    if (!products_cols_ok(c, cols, ncols, &need_piso))
        return fail(c, MSX_ERR_RANGE, "msx_products_batch: a column code the staged problem and products cannot answer");
    if (n == 0) return MSX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // [theta | out | status | cols] in one device buffer that grows with the batch
    const size_t b_theta = sizeof(double) * (size_t)(n * ndim), b_out = sizeof(double) * (size_t)(n * ncols);
    const size_t b_status = sizeof(int32_t) * (size_t)n, b_cols = sizeof(uint32_t) * (size_t)ncols;
    const size_t need = b_theta + b_out + b_status + b_cols;
    if (need > c->prod_buf_bytes) {
        if (c->d_prod_buf) (void)hipFree(c->d_prod_buf);
        c->d_prod_buf = nullptr; c->prod_buf_bytes = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_prod_buf, need));
        c->prod_buf_bytes = need;
    }
    double *d_theta = reinterpret_cast<double *>(c->d_prod_buf);
    double *d_out = reinterpret_cast<double *>(c->d_prod_buf + b_theta);
    int32_t *d_status = reinterpret_cast<int32_t *>(c->d_prod_buf + b_theta + b_out);
    uint32_t *d_cols = reinterpret_cast<uint32_t *>(c->d_prod_buf + b_theta + b_out + b_status);
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, b_theta, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_cols, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    if (int rc = products_batch_launch(c, d_theta, n, ndim, d_cols, ncols, d_out, d_status, c->stream, need_piso)) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, d_status, b_status, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MSX_OK;
}

int msx_products_spectra(msx_ctx *c, const double *theta, int64_t n, int32_t ndim, int32_t flags, double *out, double *scale_out,
                         int32_t *status) {
    if (!c) return MSX_ERR_INVALID;
    if (!theta || !out || !scale_out || !status || n < 0 || (flags & ~MSX_SPEC_MEDIAN_SCALE))
        return fail(c, MSX_ERR_INVALID, "msx_products_spectra: bad arguments");
    if (!c->problem_staged || !c->products_staged) return fail(c, MSX_ERR_STATE, "msx_products_spectra: no products staged (msx_stage_products)");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, "msx_products_spectra: ndim must be 2 * nspec + 2");
    if (c->P.npix > INT32_MAX) return fail(c, MSX_ERR_RANGE, "msx_products_spectra: too many pixels");
    if (n == 0) return MSX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int ns = c->P.nspec;
    const size_t b_out = sizeof(double) * (size_t)(n * (1 + ns) * c->P.npix), b_theta = sizeof(double) * (size_t)(n * ndim);
    const size_t b_scale = sizeof(double) * (size_t)n, b_status = sizeof(int32_t) * (size_t)n;
    const size_t need = b_out + b_theta + b_scale + b_status;
    if (need > c->prod_buf_bytes) {
        if (c->d_prod_buf) (void)hipFree(c->d_prod_buf);
        c->d_prod_buf = nullptr; c->prod_buf_bytes = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_prod_buf, need));
        c->prod_buf_bytes = need;
    }
    SpecLaunch L;
    memset(&L, 0, sizeof(L));
    L.M = c->d_prod_member;
    L.out = reinterpret_cast<double *>(c->d_prod_buf);
    double *d_theta = reinterpret_cast<double *>(c->d_prod_buf + b_out);
    L.theta = d_theta;
    L.scale_out = reinterpret_cast<double *>(c->d_prod_buf + b_out + b_theta);
    L.status = reinterpret_cast<int32_t *>(c->d_prod_buf + b_out + b_theta + b_scale);
    L.ndim = ndim; L.flags = flags;
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, b_theta, hipMemcpyHostToDevice, c->stream));
    if (ns == 2) hipLaunchKernelGGL(products_spectra_kernel<2>, dim3((unsigned)n), dim3(kProdThreads), 0, c->stream, L);
    else hipLaunchKernelGGL(products_spectra_kernel<3>, dim3((unsigned)n), dim3(kProdThreads), 0, c->stream, L);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, L.out, b_out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scale_out, L.scale_out, b_scale, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, L.status, b_status, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MSX_OK;
}

int msx_composite_parts(msx_ctx *c, const double *teff, const double *logg, const double *rad, int32_t use_distance, double plx,
                        int64_t j0, int64_t n, double *comp_out, int32_t *status) {
    if (!c) return MSX_ERR_INVALID;
    if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_composite_parts: no problem staged");
    if (!teff || !logg || !rad || !comp_out || !status) return fail(c, MSX_ERR_INVALID, "msx_composite_parts: bad arguments");
    if (j0 < 0 || n < 1 || j0 + n > c->nwl) return fail(c, MSX_ERR_RANGE, "msx_composite_parts: the window is outside the staged grid");
    HIP_TRY(c, hipSetDevice(c->device));
    const int ns = c->P.nspec;
    double args[3 * MSX_MAX_SPEC + 1];
    for (int i = 0; i < ns; ++i) { args[i] = teff[i]; args[ns + i] = logg[i]; args[2 * ns + i] = rad[i]; }
    args[3 * ns] = plx;
    double *d_out = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d_out, sizeof(double) * (size_t)(ns * n)));
    double *d_args = c->d_misc;
    WalkerDesc *d_desc = reinterpret_cast<WalkerDesc *>(c->d_misc + 64);
    WalkerDesc h;
    hipError_t e = hipMemcpyAsync(d_args, args, sizeof(double) * (3 * ns + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(composite_setup_kernel, dim3(1), dim3(64), 0, c->stream, c->P, d_args, (int)use_distance, d_desc);
        hipLaunchKernelGGL(composite_parts_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)ns), dim3(256), 0, c->stream, c->P, d_desc,
                           j0, n, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_desc, sizeof(WalkerDesc), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && h.status == MSX_W_OK) e = hipMemcpy(comp_out, d_out, sizeof(double) * (size_t)(ns * n), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, MSX_ERR_HIP, std::string("msx_composite_parts: ") + hipGetErrorString(e));
    *status = h.status;
    return MSX_OK;
}

int msx_series_derive(msx_series *src, msx_ctx **ctxs, const uint32_t *cols, int32_t ncols, int64_t row0, int64_t nrows, msx_series *dst,
                      int32_t *worst_status) {
    if (!src) return MSX_ERR_INVALID;
    if (!dst || !ctxs || !cols || ncols < 1 || row0 < 0 || nrows < 1) return fail(src, MSX_ERR_INVALID, "msx_series_derive: bad arguments");
    if (ncols > MSX_MAX_DIM) return fail(src, MSX_ERR_RANGE, "msx_series_derive: more columns than a series is wide (MSX_MAX_DIM)");
    if (dst == src || dst->device != src->device || dst->nw != src->nw || dst->off != src->off || dst->ndim != ncols)
        return fail(src, MSX_ERR_INVALID, "msx_series_derive: dst must be another series on the same device with src's members and ndim = ncols");
    if (dst->run || dst->trun || dst->gtrun) return fail(src, MSX_ERR_STATE, "msx_series_derive: a run in flight appends to dst");
    if (row0 + nrows > src->rows) return fail(src, MSX_ERR_RANGE, "msx_series_derive: rows past the ones src holds");
    if (row0 > dst->rows) return fail(src, MSX_ERR_RANGE, "msx_series_derive: row0 past the rows dst holds (it would leave a gap)");
    const int k = (int)src->off.size() - 1;
    int32_t need_piso = 0;
    int nspec = 0;
    for (int m = 0; m < k; ++m) {
        const msx_ctx *c = ctxs[m];
        const std::string who = "msx_series_derive: member " + std::to_string(m);
        if (!c) return fail(src, MSX_ERR_INVALID, who + " is null");
        if (c->device != src->device) return fail(src, MSX_ERR_INVALID, who + " lives on another device");
        if (!c->problem_staged || !c->products_staged) return fail(src, MSX_ERR_STATE, who + " has no staged products (msx_stage_products)");
        if (m == 0) nspec = c->PM.nspec;
        if (c->PM.nspec != nspec || src->ndim != 2 * nspec + 2)
            return fail(src, MSX_ERR_INVALID, who + ": src's ndim must be 2 * nspec + 2 of every member");
        if (!products_cols_ok(c, cols, ncols, &need_piso))
            return fail(src, MSX_ERR_RANGE, who + " cannot answer a column code (band, star, filter or coordinate it does not have)");
    }
    HIP_TRY(src, hipSetDevice(src->device));
    hipStream_t st = src->stream;
    // dst grows the way append grows it: the copy and its event on the stream that then writes the rows
    HIP_TRY(src, series_reserve(dst, row0 + nrows, dst->rows, st));
    const size_t b_mem = sizeof(ProdMember) * (size_t)k, b_worst = sizeof(int32_t) * (size_t)k, b_cols = sizeof(uint32_t) * (size_t)ncols;
    HIP_TRY(src, series_scratch(src, b_mem + b_worst + b_cols));
    ProdMember *d_mem = reinterpret_cast<ProdMember *>(src->d_scratch);
    int32_t *d_worst = reinterpret_cast<int32_t *>(src->d_scratch + b_mem);
    uint32_t *d_cols = reinterpret_cast<uint32_t *>(src->d_scratch + b_mem + b_worst);
    std::vector<ProdMember> mem((size_t)k);
    int64_t max_count = 0;
    for (int m = 0; m < k; ++m) {
        mem[(size_t)m] = ctxs[m]->PM;
        max_count = std::max(max_count, (src->off[(size_t)m + 1] - src->off[(size_t)m]) * nrows);
    }
    HIP_TRY(src, hipMemcpyAsync(d_mem, mem.data(), b_mem, hipMemcpyHostToDevice, st));
    HIP_TRY(src, hipMemsetAsync(d_worst, 0, b_worst, st));
    HIP_TRY(src, hipMemcpyAsync(d_cols, cols, b_cols, hipMemcpyHostToDevice, st));
    HIP_TRY(src, series_wait_growth(src));
    if (dst->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, dst->grown, 0));
    ProdLaunch L;
    memset(&L, 0, sizeof(L));
    L.members = d_mem; L.off = src->d_off;
    L.in = src->d_rows; L.in_sw = src->cap; L.in_sr = 1; L.in_sd = src->nw * src->cap;
    L.out = dst->d_rows; L.out_sw = dst->cap; L.out_sr = 1; L.out_sd = dst->nw * dst->cap;
    L.row0 = row0; L.nrows = nrows; L.cols = d_cols; L.ncols = ncols; L.need_piso = need_piso;
    L.status = nullptr; L.worst = d_worst;
    products_launch(nspec, L, max_count, k, st);
    HIP_TRY(src, hipGetLastError());
    std::vector<int32_t> worst((size_t)k, 0);
    HIP_TRY(src, hipMemcpyAsync(worst.data(), d_worst, b_worst, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipStreamSynchronize(st));
    if (worst_status) memcpy(worst_status, worst.data(), b_worst);
    dst->rows = std::max(dst->rows, row0 + nrows);
    return MSX_OK;
}

// ---- posterior predictive checks (predictive_kernels.h) --------------------------------------------
static constexpr size_t kPredDefaultBytes = (size_t)256 << 20;  // scratch_bytes == 0
static size_t pred_align(size_t b) { return (b + 255) & ~(size_t)255; }

// one member's run: the samples of `src` (all of them get terms and a status), of which sample i is REDUCED when its row
// index i / W is sel0 + j * selstep and its status is MSX_W_OK
struct PredJob {
    const msx_ctx *c;
    PredSrc src;
    int64_t nall, sel0, selstep, nsel;
    double *d_terms;  // device; null: no terms wanted
    int64_t t_sw, t_sr, t_sd;
};
struct PredSizes {
    int64_t npix, nrows, nvr;  // nrows = 1 + nspec; nvr = rows of the value buffer (+ data_n, z, z^2)
    size_t b_rec, b_status, b_vidx, b_ranks, b_band, b_ostat, b_resid, b_big, total;
};
// the smallest scratch a job can run in: one work row of the sample pass, or one pixel's values of every selected sample
static size_t pred_min_bytes(int64_t npix, int nspec, int64_t nsel) {
    return sizeof(double) * (size_t)std::max(npix, (int64_t)(1 + nspec + kPredExtra) * nsel);
}
static PredSizes pred_sizes(const PredJob &J, int32_t nq, size_t budget) {
    PredSizes Z;
    Z.npix = J.c->PM.npix; Z.nrows = 1 + J.c->PM.nspec; Z.nvr = Z.nrows + kPredExtra;
    const size_t most = sizeof(double) * (size_t)Z.npix * (size_t)std::max(J.nall, Z.nvr * J.nsel);  // everything at once
    Z.b_big = pred_align(std::min(budget, most));
    Z.b_rec = pred_align(sizeof(PredRec) * (size_t)J.nall);
    Z.b_status = pred_align(sizeof(int32_t) * (size_t)J.nall);
    Z.b_vidx = pred_align(sizeof(int64_t) * (size_t)J.nsel);
    Z.b_ranks = pred_align(sizeof(int64_t) * (size_t)std::max(1, 2 * nq));
    Z.b_band = pred_align(sizeof(double) * (size_t)(4 * Z.nrows * Z.npix));
    Z.b_ostat = pred_align(sizeof(double) * (size_t)std::max((int64_t)1, 2 * nq * Z.nrows * Z.npix));
    Z.b_resid = pred_align(sizeof(double) * (size_t)(kPredExtra * Z.npix));
    Z.total = Z.b_rec + Z.b_status + Z.b_vidx + Z.b_ranks + Z.b_band + Z.b_ostat + Z.b_resid + Z.b_big;
    return Z;
}

// NumPy's interpolation of its default ('linear') quantile method, with its roundings (mcmc_spec_amd/summary.py, _lerp)
static double pred_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    if (t == 0.0) return a;
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// Runs the job on `st` inside d_arena (pred_sizes(...).total bytes) and waits for it.  status_out [nall] or null; band
// [4][nrows][npix], quant [nq][nrows][npix] or null, resid [3][npix]: host.  *err gets the message of a failure.
static int pred_run(const PredJob &J, hipStream_t st, char *d_arena, const PredSizes &Z, size_t budget, const double *q, int32_t nq,
                    double *band, double *quant, double *resid, int32_t *status_out, int64_t *count_out, int32_t *worst_out,
                    std::string *err) {
#define PRED_TRY(expr)                                                                              \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) { *err = std::string(#expr) + ": " + hipGetErrorString(e__); return MSX_ERR_HIP; } \
    } while (0)
    const int ns = J.c->PM.nspec;
    const int64_t npix = Z.npix, nrows = Z.nrows, nvr = Z.nvr;
    char *at = d_arena;
    PredRec *d_rec = reinterpret_cast<PredRec *>(at); at += Z.b_rec;
    int32_t *d_status = reinterpret_cast<int32_t *>(at); at += Z.b_status;
    int64_t *d_vidx = reinterpret_cast<int64_t *>(at); at += Z.b_vidx;
    int64_t *d_ranks = reinterpret_cast<int64_t *>(at); at += Z.b_ranks;
    double *d_band = reinterpret_cast<double *>(at); at += Z.b_band;
    double *d_ostat = reinterpret_cast<double *>(at); at += Z.b_ostat;
    double *d_resid = reinterpret_cast<double *>(at); at += Z.b_resid;
    double *d_big = reinterpret_cast<double *>(at);
    const size_t big = std::min(budget, Z.b_big);
    // the sample pass, in batches of as many work rows as the scratch holds
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(J.nall, (int64_t)(big / (sizeof(double) * (size_t)npix))));
    PredSampleLaunch SL;
    memset(&SL, 0, sizeof(SL));
    SL.M = J.c->d_prod_member; SL.src = J.src; SL.work = d_big; SL.rec = d_rec; SL.status = d_status;
    SL.terms = J.d_terms; SL.t_sw = J.t_sw; SL.t_sr = J.t_sr; SL.t_sd = J.t_sd;
    for (int64_t i0 = 0; i0 < J.nall; i0 += batch) {
        SL.i0 = i0;
        const dim3 grid((unsigned)std::min(batch, J.nall - i0));
        if (ns == 2) hipLaunchKernelGGL(predictive_sample_kernel<2>, grid, dim3(kPredThreads), 0, st, SL);
        else hipLaunchKernelGGL(predictive_sample_kernel<3>, grid, dim3(kPredThreads), 0, st, SL);
        PRED_TRY(hipGetLastError());
    }
    std::vector<int32_t> status((size_t)J.nall);
    PRED_TRY(hipMemcpyAsync(status.data(), d_status, sizeof(int32_t) * (size_t)J.nall, hipMemcpyDeviceToHost, st));
    PRED_TRY(hipStreamSynchronize(st));
    if (status_out) memcpy(status_out, status.data(), sizeof(int32_t) * (size_t)J.nall);
    std::vector<int64_t> vidx;
    vidx.reserve((size_t)J.nsel);
    int32_t worst = 0;
    for (int64_t i = 0; i < J.nall; ++i) {
        worst = std::max(worst, status[(size_t)i]);
        const int64_t ri = i / J.src.W;
        if (ri >= J.sel0 && (ri - J.sel0) % J.selstep == 0 && status[(size_t)i] == MSX_W_OK) vidx.push_back(i);
    }
    const int64_t count = (int64_t)vidx.size();
    *count_out = count;
    if (worst_out) *worst_out = worst;
    const double nan = (double)NAN;
    const size_t plane = (size_t)(nrows * npix);
    if (count == 0) {
        std::fill(band, band + 4 * plane, nan);
        if (quant) std::fill(quant, quant + (size_t)nq * plane, nan);
        std::fill(resid, resid + (size_t)(kPredExtra * npix), nan);
        return MSX_OK;
    }
    // ranks floor(h), min(floor(h) + 1, N - 1) of NumPy's virtual index h = (N - 1) q, and the weight h - floor(h)
    const int nranks = quant ? 2 * nq : 0;
    std::vector<int64_t> ranks((size_t)std::max(1, nranks), 0);
    std::vector<double> wt((size_t)std::max(1, (int)nq), 0.0);
    for (int r = 0; r < (quant ? nq : 0); ++r) {
        const double h = (double)(count - 1) * q[r], fl = floor(h);
        ranks[(size_t)(2 * r)] = (int64_t)fl;
        ranks[(size_t)(2 * r + 1)] = std::min((int64_t)fl + 1, count - 1);
        wt[(size_t)r] = h - fl;
    }
    PRED_TRY(hipMemcpyAsync(d_vidx, vidx.data(), sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice, st));
    PRED_TRY(hipMemcpyAsync(d_ranks, ranks.data(), sizeof(int64_t) * ranks.size(), hipMemcpyHostToDevice, st));
    // pixel tiles sized from the scratch by the SELECTED samples (not by how many turned out valid)
    const int64_t tile = std::max<int64_t>(1, std::min<int64_t>(npix, (int64_t)(big / (sizeof(double) * (size_t)(nvr * J.nsel)))));
    PredFillLaunch FL;
    memset(&FL, 0, sizeof(FL));
    FL.M = J.c->d_prod_member; FL.rec = d_rec; FL.vidx = d_vidx; FL.count = count; FL.vals = d_big;
    PredReduceLaunch RL;
    memset(&RL, 0, sizeof(RL));
    RL.vals = d_big; RL.count = count; RL.npix = npix; RL.nrows = (int32_t)nrows; RL.nranks = nranks; RL.ranks = d_ranks;
    RL.band = d_band; RL.ostat = d_ostat; RL.resid = d_resid;
    for (int64_t p0 = 0; p0 < npix; p0 += tile) {
        const int64_t tp = std::min(tile, npix - p0);
        FL.p0 = RL.p0 = p0; FL.tp = RL.tp = tp;
        const int64_t gx = (count + kPredTile - 1) / kPredTile, chunks = (tp + kPredTile - 1) / kPredTile;
        const dim3 fgrid((unsigned)gx, (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, 2048 / std::min<int64_t>(gx, 2048))));
        if (ns == 2) hipLaunchKernelGGL(predictive_fill_kernel<2>, fgrid, dim3(kPredThreads), 0, st, FL);
        else hipLaunchKernelGGL(predictive_fill_kernel<3>, fgrid, dim3(kPredThreads), 0, st, FL);
        PRED_TRY(hipGetLastError());
        hipLaunchKernelGGL(predictive_reduce_kernel, dim3((unsigned)tp, (unsigned)nvr), dim3(kPredThreads), 0, st, RL);
        PRED_TRY(hipGetLastError());
    }
    std::vector<double> ostat((size_t)nranks * plane);
    PRED_TRY(hipMemcpyAsync(band, d_band, sizeof(double) * 4 * plane, hipMemcpyDeviceToHost, st));
    if (nranks) PRED_TRY(hipMemcpyAsync(ostat.data(), d_ostat, sizeof(double) * ostat.size(), hipMemcpyDeviceToHost, st));
    PRED_TRY(hipMemcpyAsync(resid, d_resid, sizeof(double) * (size_t)(kPredExtra * npix), hipMemcpyDeviceToHost, st));
    PRED_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < (quant ? nq : 0); ++r)
        for (size_t e = 0; e < plane; ++e)
            quant[(size_t)r * plane + e] = pred_lerp(ostat[(size_t)(2 * r) * plane + e], ostat[(size_t)(2 * r + 1) * plane + e], wt[(size_t)r]);
    return MSX_OK;
#undef PRED_TRY
}

static bool pred_q_ok(const double *q, int32_t nq) {
    for (int32_t r = 0; r < nq; ++r)
        if (!(q[r] >= 0.0 && q[r] <= 1.0)) return false;  // (a NaN fails the comparison too)
    return true;
}

int msx_predictive_batch(msx_ctx *c, const double *theta, int64_t n, int32_t ndim, const double *q, int32_t nq, int64_t scratch_bytes,
                         double *band, double *quant, double *resid, double *terms, int32_t *status, int64_t *count) {
    if (!c) return MSX_ERR_INVALID;
    if (!theta || !band || !resid || !terms || !status || !count || n < 1 || nq < 0 || scratch_bytes < 0 || (quant && (!q || nq < 1)))
        return fail(c, MSX_ERR_INVALID, "msx_predictive_batch: bad arguments");
    if (!c->problem_staged || !c->products_staged) return fail(c, MSX_ERR_STATE, "msx_predictive_batch: no products staged (msx_stage_products)");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, "msx_predictive_batch: ndim must be 2 * nspec + 2");
    if (c->P.npix > INT32_MAX || n > INT32_MAX) return fail(c, MSX_ERR_RANGE, "msx_predictive_batch: too many pixels or samples");
    if (quant && !pred_q_ok(q, nq)) return fail(c, MSX_ERR_RANGE, "msx_predictive_batch: quantiles must lie in [0, 1]");
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kPredDefaultBytes;
    if (budget < pred_min_bytes(c->P.npix, c->P.nspec, n))
        return fail(c, MSX_ERR_RANGE, "msx_predictive_batch: scratch_bytes holds neither one model row nor one pixel's values of the n samples (8 * max(npix, (nspec + 4) * n) bytes)");
    HIP_TRY(c, hipSetDevice(c->device));
    PredJob J;
    memset(&J, 0, sizeof(J));
    J.c = c; J.nall = n; J.sel0 = 0; J.selstep = 1; J.nsel = n;
    const PredSizes Z = pred_sizes(J, quant ? nq : 0, budget);
    const size_t b_theta = pred_align(sizeof(double) * (size_t)(n * ndim)), b_terms = pred_align(sizeof(double) * (size_t)(4 * n));
    const size_t need = b_theta + b_terms + Z.total;
    if (need > c->prod_buf_bytes) {
        if (c->d_prod_buf) (void)hipFree(c->d_prod_buf);
        c->d_prod_buf = nullptr; c->prod_buf_bytes = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_prod_buf, need));
        c->prod_buf_bytes = need;
    }
    double *d_theta = reinterpret_cast<double *>(c->d_prod_buf), *d_terms = reinterpret_cast<double *>(c->d_prod_buf + b_theta);
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, sizeof(double) * (size_t)(n * ndim), hipMemcpyHostToDevice, c->stream));
    J.src.base = d_theta; J.src.W = n; J.src.w0 = 0; J.src.sw = ndim; J.src.sr = 0; J.src.sd = 1; J.src.row0 = 0; J.src.rstep = 1;
    J.d_terms = d_terms; J.t_sw = 4; J.t_sr = 0; J.t_sd = 1;
    std::string err;
    if (int rc = pred_run(J, c->stream, c->d_prod_buf + b_theta + b_terms, Z, budget, q, quant ? nq : 0, band, quant, resid, status, count,
                          nullptr, &err))
        return fail(c, rc, "msx_predictive_batch: " + err);
    HIP_TRY(c, hipMemcpyAsync(terms, d_terms, sizeof(double) * (size_t)(4 * n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MSX_OK;
}

int msx_series_predictive(msx_series *src, msx_ctx **ctxs, int64_t n, int64_t discard, int64_t thin, const double *q, int32_t nq,
                          int64_t scratch_bytes, double *band, double *quant, double *resid, msx_series *dst, int64_t *count,
                          int32_t *worst_status) {
    if (!src) return MSX_ERR_INVALID;
    if (!ctxs || !band || !resid || !count || discard < 0 || thin < 1 || nq < 0 || scratch_bytes < 0 || (quant && (!q || nq < 1)))
        return fail(src, MSX_ERR_INVALID, "msx_series_predictive: bad arguments (discard >= 0, thin >= 1, band, resid, count)");
    if (dst && (dst == src || dst->device != src->device || dst->nw != src->nw || dst->off != src->off || dst->ndim != 4))
        return fail(src, MSX_ERR_INVALID, "msx_series_predictive: the terms go to another series on the same device with src's members and ndim = 4");
    if (dst && (dst->run || dst->trun || dst->gtrun)) return fail(src, MSX_ERR_STATE, "msx_series_predictive: a run in flight appends to the terms' series");
    if (n < 1 || n > src->rows) return fail(src, MSX_ERR_RANGE, "msx_series_predictive: n must lie in 1 .. the rows the series holds");
    const int64_t np = discard < n ? (n - discard + thin - 1) / thin : 0;
    if (np < 1) return fail(src, MSX_ERR_RANGE, "msx_series_predictive: the selection rows[0:n][discard::thin] is empty");
    if (quant && !pred_q_ok(q, nq)) return fail(src, MSX_ERR_RANGE, "msx_series_predictive: quantiles must lie in [0, 1]");
    const int k = (int)src->off.size() - 1;
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kPredDefaultBytes;
    const int32_t nqq = quant ? nq : 0;
    int nspec = 0;
    std::vector<PredJob> jobs((size_t)k);
    size_t arena = 0;
    for (int m = 0; m < k; ++m) {
        const msx_ctx *c = ctxs[m];
        const std::string who = "msx_series_predictive: member " + std::to_string(m);
        if (!c) return fail(src, MSX_ERR_INVALID, who + " is null");
        if (c->device != src->device) return fail(src, MSX_ERR_INVALID, who + " lives on another device");
        if (!c->problem_staged || !c->products_staged) return fail(src, MSX_ERR_STATE, who + " has no staged products (msx_stage_products)");
        if (m == 0) nspec = c->PM.nspec;
        if (c->PM.nspec != nspec || src->ndim != 2 * nspec + 2)
            return fail(src, MSX_ERR_INVALID, who + ": src's ndim must be 2 * nspec + 2 of every member");
        const int64_t W = src->off[(size_t)m + 1] - src->off[(size_t)m];
        PredJob &J = jobs[(size_t)m];
        memset(&J, 0, sizeof(J));
        J.c = c;
        J.src.W = W; J.src.w0 = src->off[(size_t)m];
        // with a terms series every row 0 .. n - 1 is evaluated and the selection picks among them; without, the selection alone
        if (dst) { J.src.row0 = 0; J.src.rstep = 1; J.nall = n * W; J.sel0 = discard; J.selstep = thin; }
        else { J.src.row0 = discard; J.src.rstep = thin; J.nall = np * W; J.sel0 = 0; J.selstep = 1; }
        J.nsel = np * W;
        if (c->PM.npix > INT32_MAX || J.nsel > INT32_MAX) return fail(src, MSX_ERR_RANGE, who + ": too many pixels or samples");
        if (budget < pred_min_bytes(c->PM.npix, nspec, J.nsel))
            return fail(src, MSX_ERR_RANGE, who + ": scratch_bytes holds neither one model row nor one pixel's values of its samples (8 * max(npix, (nspec + 4) * N_m) bytes)");
        arena = std::max(arena, pred_sizes(J, nqq, budget).total);
    }
    HIP_TRY(src, hipSetDevice(src->device));
    hipStream_t st = src->stream;
    if (dst) HIP_TRY(src, series_reserve(dst, n, dst->rows, st));  // (grows the way append grows it)
    HIP_TRY(src, series_scratch(src, arena));
    HIP_TRY(src, series_wait_growth(src));
    if (dst && dst->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, dst->grown, 0));
    size_t o_band = 0, o_quant = 0, o_resid = 0;
    for (int m = 0; m < k; ++m) {
        PredJob &J = jobs[(size_t)m];
        J.src.base = src->d_rows; J.src.sw = src->cap; J.src.sr = 1; J.src.sd = src->nw * src->cap;
        if (dst) { J.d_terms = dst->d_rows; J.t_sw = dst->cap; J.t_sr = 1; J.t_sd = dst->nw * dst->cap; }
        const PredSizes Z = pred_sizes(J, nqq, budget);
        const size_t plane = (size_t)(Z.nrows * Z.npix);
        std::string err;
        int32_t worst = 0;
        if (int rc = pred_run(J, st, src->d_scratch, Z, budget, q, nqq, band + o_band, quant ? quant + o_quant : nullptr, resid + o_resid,
                              nullptr, count + m, &worst, &err))
            return fail(src, rc, "msx_series_predictive: member " + std::to_string(m) + ": " + err);
        if (worst_status) worst_status[m] = worst;
        o_band += 4 * plane; o_quant += (size_t)nqq * plane; o_resid += (size_t)(kPredExtra * Z.npix);
    }
    if (dst) dst->rows = std::max(dst->rows, n);
    return MSX_OK;
}

// ---- posterior modes: mixture fit, labels, the samples by mode (mode_kernels.h) -----------------------
// what both calls check of the selection, the columns and the standardisation; fills S (rows and the device tables apart)
static int modes_selection(msx_series *sr, const char *who, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                           const double *center, const double *scale, int32_t ncomp, ModeSel *S) {
    const std::string w(who);
    if (!center || !scale || discard < 0 || thin < 1 || ncols < 1)
        return fail(sr, MSX_ERR_INVALID, w + ": bad arguments (discard >= 0, thin >= 1, ncols >= 1, center and scale)");
    if (n < 1 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, w + ": n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (np < 4) return fail(sr, MSX_ERR_RANGE, w + ": the selection rows[0:n][discard::thin] needs at least 4 rows");
    if (ncols > MSX_MAX_DIM) return fail(sr, MSX_ERR_RANGE, w + ": more columns than a series is wide (MSX_MAX_DIM)");
    if (ncomp < 1 || ncomp > MSX_MODES_MAX) return fail(sr, MSX_ERR_RANGE, w + ": ncomp must lie in 1 .. MSX_MODES_MAX");
    memset(S, 0, sizeof(*S));
    S->cols.n = ncols;
    if (!cols && ncols != sr->ndim) return fail(sr, MSX_ERR_RANGE, w + ": cols == NULL means all columns (ncols = ndim)");
    for (int32_t q = 0; q < ncols; ++q) {
        const uint32_t c = cols ? cols[q] : (uint32_t)q;
        if (c >= (uint32_t)sr->ndim) return fail(sr, MSX_ERR_RANGE, w + ": a column outside the series");
        S->cols.c[q] = (int32_t)c;
    }
    const int k = (int)sr->off.size() - 1;
    for (int64_t i = 0; i < (int64_t)k * ncols; ++i)
        if (!std::isfinite(center[i]) || !std::isfinite(scale[i]) || !(scale[i] > 0.0))
            return fail(sr, MSX_ERR_INVALID, w + ": every center must be finite, every scale finite and > 0");
    for (int m = 0; m < k; ++m)
        if ((sr->off[(size_t)m + 1] - sr->off[(size_t)m]) * np <= (int64_t)ncomp * (ncols + 1))
            return fail(sr, MSX_ERR_RANGE, w + ": a member needs more than ncomp (ncols + 1) samples");
    const int64_t ntiles = (np + kModeTile - 1) / kModeTile;
    if (sr->nw * ntiles > 0x7fffffff) return fail(sr, MSX_ERR_RANGE, w + ": more rows than one launch covers");
    S->cap = sr->cap; S->nw = sr->nw; S->np = np; S->discard = discard; S->thin = thin; S->k = k;
    return MSX_OK;
}

static size_t mode_align(size_t b) { return (b + 15) & ~(size_t)15; }

#define MODE_DISPATCH(D, KERNEL, ...)                                     \
    switch (D) {                                                          \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;            \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;            \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;            \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;            \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;            \
    case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;            \
    case 7: hipLaunchKernelGGL(KERNEL<7>, __VA_ARGS__); break;            \
    default: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;           \
    }

int msx_series_modes(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols, const double *center,
                     const double *scale, int32_t ncomp, int32_t nstarts, const int32_t *split_col, const double *split_at, int32_t max_iter,
                     double tol, double ridge, double *weight, double *mean, double *cov, double *loglik, int32_t *niter, int32_t *status,
                     int64_t *nbad) {
    if (!sr) return MSX_ERR_INVALID;
    const std::string who("msx_series_modes");
    if (!weight || !mean || !cov || !loglik || !niter || !status || !nbad || !split_col || nstarts < 1 || max_iter < 1 || !(tol >= 0.0) ||
        !(ridge >= 0.0) || !std::isfinite(ridge))
        return fail(sr, MSX_ERR_INVALID, who + ": bad arguments (every output, split_col, nstarts >= 1, max_iter >= 1, tol >= 0, ridge >= 0)");
    ModeSel S;
    if (int rc = modes_selection(sr, "msx_series_modes", n, discard, thin, cols, ncols, center, scale, ncomp, &S)) return rc;
    if (ncomp > 1 && !split_at) return fail(sr, MSX_ERR_INVALID, who + ": split_at is needed with ncomp > 1");
    if (nstarts > 64) return fail(sr, MSX_ERR_RANGE, who + ": at most 64 starts");
    const int k = S.k, d = ncols, nthr = ncomp - 1;
    std::vector<int32_t> scol((size_t)nstarts);
    for (int32_t s = 0; s < nstarts; ++s) {
        if (split_col[s] < 0 || split_col[s] >= ncols) return fail(sr, MSX_ERR_RANGE, who + ": a split_col outside 0 .. ncols - 1");
        scol[(size_t)s] = S.cols.c[split_col[s]];
    }
    const int64_t njobs = (int64_t)k * nstarts;
    for (int64_t j = 0; j < njobs; ++j)
        for (int i = 0; i < nthr; ++i) {
            const double a = split_at[j * nthr + i];
            if (std::isnan(a) || (i > 0 && !(split_at[j * nthr + i - 1] <= a))) return fail(sr, MSX_ERR_RANGE, who + ": a start's thresholds must not descend");
        }
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t ntiles = (S.np + kModeTile - 1) / kModeTile, nwt = sr->nw * ntiles;
    const int P = 1 + d + d * (d + 1) / 2, nacc = P + 1;
    // scratch: [part | params | weight mean cov loglik (downloaded in one piece) | prev | ngood | center | scale | split_at |
    //           niter status (one piece) | frozen | split columns]
    const size_t b_part = mode_align(sizeof(double) * (size_t)(nstarts * ncomp) * (size_t)nwt * (size_t)nacc);
    const size_t b_params = mode_align(sizeof(double) * (size_t)(njobs * ncomp * P));
    const int64_t n_w = njobs * ncomp, n_mean = n_w * d, n_cov = n_mean * d, n_out = n_w + n_mean + n_cov + njobs;
    const size_t b_out = mode_align(sizeof(double) * (size_t)n_out), b_job = mode_align(sizeof(double) * (size_t)njobs);
    const size_t b_cs = mode_align(sizeof(double) * (size_t)(k * d)), b_at = mode_align(sizeof(double) * (size_t)std::max<int64_t>(njobs * nthr, 1));
    const size_t b_ij = mode_align(sizeof(int32_t) * (size_t)(2 * njobs)), b_fr = mode_align(sizeof(int32_t) * (size_t)njobs);
    const size_t b_sc = mode_align(sizeof(int32_t) * (size_t)nstarts);
    HIP_TRY(sr, series_scratch(sr, b_part + b_params + b_out + 2 * b_job + 2 * b_cs + b_at + b_ij + b_fr + b_sc));
    char *p = sr->d_scratch;
    double *d_part = (double *)p; p += b_part;
    double *d_params = (double *)p; p += b_params;
    double *d_out = (double *)p; p += b_out;
    double *d_weight = d_out, *d_mean = d_weight + n_w, *d_cov = d_mean + n_mean, *d_loglik = d_cov + n_cov;
    double *d_prev = (double *)p; p += b_job;
    double *d_ngood = (double *)p; p += b_job;
    double *d_center = (double *)p; p += b_cs;
    double *d_scale = (double *)p; p += b_cs;
    double *d_at = (double *)p; p += b_at;
    int32_t *d_niter = (int32_t *)p, *d_status = d_niter + njobs; p += b_ij;
    int32_t *d_frozen = (int32_t *)p; p += b_fr;
    int32_t *d_scol = (int32_t *)p;
    hipStream_t st = sr->stream;
    // the state every job starts from: no parameters (NaN), loglik NaN, niter 0, status collapsed until an iteration ran
    std::vector<double> h_out((size_t)n_out, std::numeric_limits<double>::quiet_NaN());
    std::vector<int32_t> h_ij((size_t)(2 * njobs), 0);
    for (int64_t j = 0; j < njobs; ++j) h_ij[(size_t)(njobs + j)] = MSX_MODES_COLLAPSED;
    HIP_TRY(sr, hipMemcpyAsync(d_out, h_out.data(), sizeof(double) * (size_t)n_out, hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemcpyAsync(d_niter, h_ij.data(), sizeof(int32_t) * (size_t)(2 * njobs), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemsetAsync(d_frozen, 0, sizeof(int32_t) * (size_t)njobs, st));
    HIP_TRY(sr, hipMemsetAsync(d_prev, 0, 2 * b_job, st));
    HIP_TRY(sr, hipMemcpyAsync(d_center, center, sizeof(double) * (size_t)(k * d), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemcpyAsync(d_scale, scale, sizeof(double) * (size_t)(k * d), hipMemcpyHostToDevice, st));
    if (nthr > 0) HIP_TRY(sr, hipMemcpyAsync(d_at, split_at, sizeof(double) * (size_t)(njobs * nthr), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemcpyAsync(d_scol, scol.data(), sizeof(int32_t) * (size_t)nstarts, hipMemcpyHostToDevice, st));
    HIP_TRY(sr, series_wait_growth(sr));
    S.rows = sr->d_rows; S.cap = sr->cap; S.member_off = sr->d_off; S.center = d_center; S.scale = d_scale;
    const dim3 sgrid((unsigned)nwt, (unsigned)(nstarts * ncomp));
    for (int32_t it = 0; it <= max_iter; ++it) {
        MODE_DISPATCH(d, mode_stats_kernel, sgrid, dim3(kModeThreads), 0, st, S, nstarts, ncomp, (int32_t)(it == 0), (const int32_t *)d_scol,
                      (const double *)d_at, (const double *)d_params, (const int32_t *)d_frozen, d_part);
        HIP_TRY(sr, hipGetLastError());
        hipLaunchKernelGGL(mode_mstep_kernel, dim3((unsigned)njobs), dim3(kModeThreads), 0, st, (const double *)d_part, (const int64_t *)sr->d_off,
                           sr->nw, ntiles, nstarts, ncomp, (int32_t)d, it, max_iter, tol, ridge, d_params, d_weight, d_mean, d_cov, d_loglik, d_prev,
                           d_ngood, d_niter, d_status, d_frozen);
        HIP_TRY(sr, hipGetLastError());
    }
    std::vector<double> h_good((size_t)njobs);
    HIP_TRY(sr, hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(sr, hipMemcpyAsync(h_ij.data(), d_niter, sizeof(int32_t) * (size_t)(2 * njobs), hipMemcpyDeviceToHost, st));
    HIP_TRY(sr, hipMemcpyAsync(h_good.data(), d_ngood, sizeof(double) * (size_t)njobs, hipMemcpyDeviceToHost, st));
    HIP_TRY(sr, hipStreamSynchronize(st));
    memcpy(weight, h_out.data(), sizeof(double) * (size_t)n_w);
    memcpy(mean, h_out.data() + n_w, sizeof(double) * (size_t)n_mean);
    memcpy(cov, h_out.data() + n_w + n_mean, sizeof(double) * (size_t)n_cov);
    memcpy(loglik, h_out.data() + n_w + n_mean + n_cov, sizeof(double) * (size_t)njobs);
    memcpy(niter, h_ij.data(), sizeof(int32_t) * (size_t)njobs);
    memcpy(status, h_ij.data() + njobs, sizeof(int32_t) * (size_t)njobs);
    for (int m = 0; m < k; ++m)   // (start 0's count: every start of a member sees the same samples)
        nbad[m] = (sr->off[(size_t)m + 1] - sr->off[(size_t)m]) * S.np - (int64_t)h_good[(size_t)m * nstarts];
    return MSX_OK;
}

int msx_series_mode_labels(msx_series *sr, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols, const double *center,
                           const double *scale, int32_t ncomp, const double *weight, const double *mean, const double *cov, uint8_t *labels_out,
                           int64_t *counts_out, msx_series **dst) {
    if (!sr) return MSX_ERR_INVALID;
    const std::string who("msx_series_mode_labels");
    if (!weight || !mean || !cov || !counts_out) return fail(sr, MSX_ERR_INVALID, who + ": bad arguments (weight, mean, cov and counts_out)");
    ModeSel S;
    if (int rc = modes_selection(sr, "msx_series_mode_labels", n, discard, thin, cols, ncols, center, scale, ncomp, &S)) return rc;
    const int k = S.k, d = ncols;
    const int P = 1 + d + d * (d + 1) / 2;
    const int64_t nmode = (int64_t)k * ncomp;
    // every component's [c | mu | L by rows] from the caller's weight, mean and covariance
    std::vector<double> prm((size_t)(nmode * P));
    for (int64_t c = 0; c < nmode; ++c) {
        double *pp = prm.data() + c * P, *L = pp + 1 + d;
        const double *sg = cov + c * d * d;
        if (!(weight[c] >= 0.0)) return fail(sr, MSX_ERR_RANGE, who + ": a weight that is negative or NaN");
        double logdet = 0.0;
        for (int r = 0; r < d; ++r)
            for (int q = 0; q <= r; ++q) {
                double s = sg[r * d + q];
                for (int j = 0; j < q; ++j) s -= L[r * (r + 1) / 2 + j] * L[q * (q + 1) / 2 + j];
                if (r == q) {
                    if (!(s > 0.0) || !std::isfinite(s)) return fail(sr, MSX_ERR_RANGE, who + ": a covariance without a Cholesky factor");
                    L[r * (r + 1) / 2 + q] = std::sqrt(s);
                    logdet += std::log(L[r * (r + 1) / 2 + q]);
                } else {
                    L[r * (r + 1) / 2 + q] = s / L[q * (q + 1) / 2 + q];
                }
            }
        pp[0] = std::log(weight[c]) - logdet - 0.5 * d * kModeLn2Pi;
        for (int q = 0; q < d; ++q) {
            if (!std::isfinite(mean[c * d + q])) return fail(sr, MSX_ERR_RANGE, who + ": a mean that is not finite");
            pp[1 + q] = mean[c * d + q];
        }
    }
    if (dst)
        for (int64_t c = 0; c < nmode; ++c) {
            msx_series *t = dst[c];
            if (!t || t == sr || t->device != sr->device || t->nw != 1 || t->off.size() != 2 || t->ndim != sr->ndim)
                return fail(sr, MSX_ERR_INVALID, who + ": every dst must be another series on the same device with one walker, one member and src's ndim");
            for (int64_t e = 0; e < c; ++e)
                if (dst[e] == t) return fail(sr, MSX_ERR_INVALID, who + ": a dst is listed twice");
            if (t->run || t->trun || t->gtrun) return fail(sr, MSX_ERR_STATE, who + ": a run in flight appends to a dst");
        }
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int64_t ntiles = (S.np + kModeTile - 1) / kModeTile, nwt = sr->nw * ntiles;
    // scratch: [params | center | scale | tilecount | base | total | dst table | labels]
    const size_t b_prm = mode_align(sizeof(double) * prm.size()), b_cs = mode_align(sizeof(double) * (size_t)(k * d));
    const size_t b_tc = mode_align(sizeof(int64_t) * (size_t)(nwt * MSX_MODES_MAX)), b_tot = mode_align(sizeof(int64_t) * (size_t)(k * MSX_MODES_MAX));
    const size_t b_dst = mode_align(sizeof(ModeDst) * (size_t)nmode), b_lab = mode_align((size_t)(sr->nw * S.np));
    HIP_TRY(sr, series_scratch(sr, b_prm + 2 * b_cs + 2 * b_tc + b_tot + b_dst + b_lab));
    char *p = sr->d_scratch;
    double *d_prm = (double *)p; p += b_prm;
    double *d_center = (double *)p; p += b_cs;
    double *d_scale = (double *)p; p += b_cs;
    int64_t *d_tc = (int64_t *)p; p += b_tc;
    int64_t *d_base = (int64_t *)p; p += b_tc;
    int64_t *d_total = (int64_t *)p; p += b_tot;
    ModeDst *d_dst = (ModeDst *)p; p += b_dst;
    uint8_t *d_lab = (uint8_t *)p;
    hipStream_t st = sr->stream;
    HIP_TRY(sr, hipMemcpyAsync(d_prm, prm.data(), sizeof(double) * prm.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemcpyAsync(d_center, center, sizeof(double) * (size_t)(k * d), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, hipMemcpyAsync(d_scale, scale, sizeof(double) * (size_t)(k * d), hipMemcpyHostToDevice, st));
    HIP_TRY(sr, series_wait_growth(sr));
    S.rows = sr->d_rows; S.cap = sr->cap; S.member_off = sr->d_off; S.center = d_center; S.scale = d_scale;
    MODE_DISPATCH(d, mode_label_kernel, dim3((unsigned)nwt), dim3(kModeThreads), 0, st, S, ncomp, (const double *)d_prm, d_lab, d_tc);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(mode_scan_kernel, dim3((unsigned)k), dim3(MSX_MODES_MAX), 0, st, (const int64_t *)d_tc, (const int64_t *)sr->d_off, ntiles,
                       d_base, d_total);
    HIP_TRY(sr, hipGetLastError());
    std::vector<int64_t> total((size_t)(k * MSX_MODES_MAX));
    std::vector<uint8_t> lab;
    HIP_TRY(sr, hipMemcpyAsync(total.data(), d_total, sizeof(int64_t) * total.size(), hipMemcpyDeviceToHost, st));
    if (labels_out) {
        lab.resize((size_t)(sr->nw * S.np));
        HIP_TRY(sr, hipMemcpyAsync(lab.data(), d_lab, lab.size(), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(sr, hipStreamSynchronize(st));
    for (int m = 0; m < k; ++m)
        for (int j = 0; j < ncomp; ++j) counts_out[m * ncomp + j] = total[(size_t)(m * MSX_MODES_MAX + j)];
    if (labels_out)   // device [nw][n'] -> host [n'][nw]
        for (int64_t w = 0; w < sr->nw; ++w)
            for (int64_t t = 0; t < S.np; ++t) labels_out[t * sr->nw + w] = lab[(size_t)(w * S.np + t)];
    if (!dst) return MSX_OK;
    // every dst holds exactly its label's rows: grown the way append grows a series (nothing carried over), then filled
    std::vector<ModeDst> table((size_t)nmode);
    for (int64_t c = 0; c < nmode; ++c) {
        msx_series *t = dst[c];
        HIP_TRY(sr, series_reserve(t, counts_out[c], 0, st));
        table[(size_t)c].rows = t->d_rows;
        table[(size_t)c].cap = t->cap;
    }
    HIP_TRY(sr, hipMemcpyAsync(d_dst, table.data(), sizeof(ModeDst) * (size_t)nmode, hipMemcpyHostToDevice, st));
    for (int64_t c = 0; c < nmode; ++c)
        if (dst[c]->grown_set) HIP_TRY(sr, hipStreamWaitEvent(st, dst[c]->grown, 0));
    hipLaunchKernelGGL(mode_scatter_kernel, dim3((unsigned)nwt), dim3(kModeThreads), 0, st, S, (int32_t)sr->ndim, ncomp, (const uint8_t *)d_lab,
                       (const int64_t *)d_base, (const ModeDst *)d_dst);
    HIP_TRY(sr, hipGetLastError());
    HIP_TRY(sr, hipStreamSynchronize(st));
    for (int64_t c = 0; c < nmode; ++c) dst[c]->rows = counts_out[c];
    return MSX_OK;
}
#undef MODE_DISPATCH

// ---- importance reweighting of a series (reweight_kernels.h) ----------------------------------------
static constexpr int64_t kRwEvalBatch = (int64_t)1 << 16;   // samples per evaluation launch of msx_series_logprob (its scratch's bound)

static bool rw_same_members(const msx_series *a, const msx_series *b) { return a->device == b->device && a->nw == b->nw && a->off == b->off; }
static bool rw_attached(const msx_series *s) { return s->run || s->trun || s->gtrun; }
static size_t rw_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the selection rows[0:n][discard::thin] -> n' (msx_series_moments' codes)
static int rw_selection(msx_series *sr, const std::string &who, int64_t n, int64_t discard, int64_t thin, int64_t *np_out) {
    if (discard < 0 || thin < 1) return fail(sr, MSX_ERR_INVALID, who + ": bad arguments (discard >= 0, thin >= 1)");
    if (n < 1 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, who + ": n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0;
    if (np < 1) return fail(sr, MSX_ERR_RANGE, who + ": the selection rows[0:n][discard::thin] is empty");
    *np_out = np;
    return MSX_OK;
}

// a weights series beside `sr`: one column, sr's members, the rows of the selection
static int rw_weights_ok(msx_series *sr, const std::string &who, const msx_series *w, int64_t n) {
    if (!w || w == sr || !rw_same_members(sr, w) || w->ndim != 1)
        return fail(sr, MSX_ERR_INVALID, who + ": the weights must be another series on the same device with ndim = 1 and the same members");
    if (n > w->rows) return fail(sr, MSX_ERR_RANGE, who + ": n past the rows the weights hold");
    return MSX_OK;
}

int msx_series_logprob(msx_series *src, msx_ctx **ctxs, int32_t mode, int64_t row0, int64_t nrows, msx_series *dst, int32_t *worst_status) {
    if (!src) return MSX_ERR_INVALID;
    const std::string who("msx_series_logprob");
    if (!dst || !ctxs || row0 < 0 || nrows < 1) return fail(src, MSX_ERR_INVALID, who + ": bad arguments");
    if (mode != MSX_MODE_LOGPOST && mode != MSX_MODE_LOGPRIOR && mode != MSX_MODE_LOGLIKE)
        return fail(src, MSX_ERR_INVALID, who + ": mode must be MSX_MODE_LOGPOST, MSX_MODE_LOGPRIOR or MSX_MODE_LOGLIKE");
    if (dst == src || !rw_same_members(src, dst) || dst->ndim != 1)
        return fail(src, MSX_ERR_INVALID, who + ": dst must be another series on the same device with src's members and ndim = 1");
    if (rw_attached(dst)) return fail(src, MSX_ERR_STATE, who + ": a run in flight appends to dst");
    if (row0 + nrows > src->rows) return fail(src, MSX_ERR_RANGE, who + ": rows past the ones src holds");
    if (row0 > dst->rows) return fail(src, MSX_ERR_RANGE, who + ": row0 past the rows dst holds (it would leave a gap)");
    const int k = (int)src->off.size() - 1;
    int64_t maxW = 0;
    for (int m = 0; m < k; ++m) {
        const msx_ctx *c = ctxs[m];
        const std::string mem = who + ": member " + std::to_string(m);
        if (!c) return fail(src, MSX_ERR_INVALID, mem + " is null");
        if (c->device != src->device) return fail(src, MSX_ERR_INVALID, mem + " lives on another device");
        if (!c->problem_staged) return fail(src, MSX_ERR_STATE, mem + " has no staged problem");
        if (c->smp || c->tmp || c->opt_run) return fail(src, MSX_ERR_STATE, mem + " has a run in flight (end it first)");
        if (src->ndim != 2 * c->P.nspec + 2) return fail(src, MSX_ERR_INVALID, mem + ": src's ndim must be 2 * nspec + 2");
        maxW = std::max(maxW, src->off[(size_t)m + 1] - src->off[(size_t)m]);
    }
    HIP_TRY(src, hipSetDevice(src->device));
    hipStream_t st = src->stream;
    HIP_TRY(src, series_reserve(dst, row0 + nrows, dst->rows, st));
    // scratch, bounded by the batch: [theta | logp | status | worst]
    const int64_t rows_per = std::min(nrows, std::max<int64_t>(1, kRwEvalBatch / maxW)), cap_s = rows_per * maxW;
    const size_t b_theta = rw_align(sizeof(double) * (size_t)(cap_s * src->ndim)), b_logp = rw_align(sizeof(double) * (size_t)cap_s);
    const size_t b_status = rw_align(sizeof(int32_t) * (size_t)cap_s), b_worst = sizeof(int32_t) * (size_t)k;
    HIP_TRY(src, series_scratch(src, b_theta + b_logp + b_status + b_worst));
    double *d_theta = (double *)src->d_scratch, *d_logp = (double *)(src->d_scratch + b_theta);
    int32_t *d_status = (int32_t *)(src->d_scratch + b_theta + b_logp), *d_worst = (int32_t *)(src->d_scratch + b_theta + b_logp + b_status);
    HIP_TRY(src, hipMemsetAsync(d_worst, 0, b_worst, st));
    HIP_TRY(src, series_wait_growth(src));
    if (dst->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, dst->grown, 0));
    for (int m = 0; m < k; ++m) {
        const int64_t w0 = src->off[(size_t)m], W = src->off[(size_t)m + 1] - w0;
        for (int64_t rb = 0; rb < nrows; rb += rows_per) {
            const int64_t cnt = std::min(rows_per, nrows - rb), ns = cnt * W, total = ns * src->ndim;
            hipLaunchKernelGGL(rw_gather_theta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double *)src->d_rows,
                               src->cap, src->nw, (int32_t)src->ndim, w0, W, row0 + rb, cnt, d_theta);
            HIP_TRY(src, hipGetLastError());
            if (int rc = msx_logprob_batch_dev(ctxs[m], mode, d_theta, ns, src->ndim, d_logp, d_status, st, 0)) {
                (void)hipStreamSynchronize(st);
                return fail(src, rc, who + ": member " + std::to_string(m) + ": " + ctxs[m]->err);
            }
            hipLaunchKernelGGL(rw_put_logp_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, (const double *)d_logp,
                               (const int32_t *)d_status, W, cnt, w0, row0 + rb, dst->d_rows, dst->cap, d_worst + m);
            HIP_TRY(src, hipGetLastError());
        }
    }
    std::vector<int32_t> worst((size_t)k, 0);
    HIP_TRY(src, hipMemcpyAsync(worst.data(), d_worst, b_worst, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipStreamSynchronize(st));
    if (worst_status) memcpy(worst_status, worst.data(), b_worst);
    dst->rows = std::max(dst->rows, row0 + nrows);
    return MSX_OK;
}

int msx_series_lincomb(int32_t nsrc, msx_series **srcs, const int32_t *cols, const double *coef, int64_t row0, int64_t nrows, msx_series *dst) {
    if (!dst) return MSX_ERR_INVALID;
    const std::string who("msx_series_lincomb");
    if (!srcs || !cols || !coef || nsrc < 1 || nsrc > kRwMaxSrc || row0 < 0 || nrows < 1)
        return fail(dst, MSX_ERR_INVALID, who + ": bad arguments (1 .. 8 terms, row0 >= 0, nrows >= 1)");
    if (dst->ndim != 1) return fail(dst, MSX_ERR_INVALID, who + ": dst needs ndim = 1");
    if (rw_attached(dst)) return fail(dst, MSX_ERR_STATE, who + ": a run in flight appends to dst");
    for (int j = 0; j < nsrc; ++j) {
        const msx_series *s = srcs[j];
        if (!s || s == dst || !rw_same_members(dst, s))
            return fail(dst, MSX_ERR_INVALID, who + ": every source must be another series on dst's device with dst's members");
        if (cols[j] < 0 || cols[j] >= s->ndim) return fail(dst, MSX_ERR_RANGE, who + ": a column outside its series");
        if (row0 + nrows > s->rows) return fail(dst, MSX_ERR_RANGE, who + ": rows past the ones a source holds");
    }
    if (row0 > dst->rows) return fail(dst, MSX_ERR_RANGE, who + ": row0 past the rows dst holds (it would leave a gap)");
    if (dst->nw > 65535) return fail(dst, MSX_ERR_RANGE, who + ": more walkers than one launch covers");
    HIP_TRY(dst, hipSetDevice(dst->device));
    hipStream_t st = dst->stream;
    HIP_TRY(dst, series_reserve(dst, row0 + nrows, dst->rows, st));
    RwTerms T;
    memset(&T, 0, sizeof(T));
    T.n = nsrc;
    for (int j = 0; j < nsrc; ++j) {
        msx_series *s = srcs[j];
        if (s->grown_set) HIP_TRY(dst, hipStreamWaitEvent(st, s->grown, 0));
        T.p[j] = s->d_rows + (int64_t)cols[j] * s->nw * s->cap;
        T.cap[j] = s->cap;
        T.coef[j] = coef[j];
    }
    HIP_TRY(dst, series_wait_growth(dst));
    hipLaunchKernelGGL(rw_lincomb_kernel, dim3((unsigned)((nrows + kRwThreads - 1) / kRwThreads), (unsigned)dst->nw), dim3(kRwThreads), 0, st, T,
                       row0, nrows, dst->d_rows, dst->cap);
    HIP_TRY(dst, hipGetLastError());
    HIP_TRY(dst, hipStreamSynchronize(st));
    dst->rows = std::max(dst->rows, row0 + nrows);
    return MSX_OK;
}

int msx_series_weights(msx_series *logw, int64_t n, int64_t discard, int64_t thin, msx_series *w_dst, double *stats) {
    if (!logw) return MSX_ERR_INVALID;
    const std::string who("msx_series_weights");
    if (!w_dst || !stats) return fail(logw, MSX_ERR_INVALID, who + ": bad arguments (w_dst and stats)");
    if (logw->ndim != 1 || w_dst == logw || !rw_same_members(logw, w_dst) || w_dst->ndim != 1)
        return fail(logw, MSX_ERR_INVALID, who + ": the log-weights and w_dst must be two series of ndim = 1 on one device with the same members");
    if (rw_attached(w_dst)) return fail(logw, MSX_ERR_STATE, who + ": a run in flight appends to w_dst");
    int64_t np = 0;
    if (int rc = rw_selection(logw, who, n, discard, thin, &np)) return rc;
    if (logw->nw > 65535) return fail(logw, MSX_ERR_RANGE, who + ": more walkers than one launch covers");
    HIP_TRY(logw, hipSetDevice(logw->device));
    hipStream_t st = logw->stream;
    HIP_TRY(logw, series_reserve(w_dst, n, w_dst->rows, st));
    const int k = (int)logw->off.size() - 1;
    const int64_t nw = logw->nw;
    // scratch: [pmax nw | psum 2 nw | stats 6 k | pcnt 2 nw]
    HIP_TRY(logw, series_scratch(logw, sizeof(double) * (size_t)(3 * nw + 6 * k) + sizeof(long long) * (size_t)(2 * nw)));
    double *d_pmax = (double *)logw->d_scratch, *d_psum = d_pmax + nw, *d_stats = d_psum + 2 * nw;
    long long *d_pcnt = (long long *)(d_stats + 6 * k);
    HIP_TRY(logw, series_wait_growth(logw));
    if (w_dst->grown_set) HIP_TRY(logw, hipStreamWaitEvent(st, w_dst->grown, 0));
    hipLaunchKernelGGL(rw_max_kernel, dim3((unsigned)nw), dim3(kRwThreads), 0, st, (const double *)logw->d_rows, logw->cap, n, d_pmax);
    HIP_TRY(logw, hipGetLastError());
    hipLaunchKernelGGL(rw_exp_kernel, dim3((unsigned)((n + kRwThreads - 1) / kRwThreads), (unsigned)nw), dim3(kRwThreads), 0, st,
                       (const double *)logw->d_rows, logw->cap, n, (const int64_t *)logw->d_off, (int32_t)k, (const double *)d_pmax, w_dst->d_rows,
                       w_dst->cap);
    HIP_TRY(logw, hipGetLastError());
    hipLaunchKernelGGL(rw_stat_kernel, dim3((unsigned)nw), dim3(kRwThreads), 0, st, (const double *)logw->d_rows, logw->cap,
                       (const double *)w_dst->d_rows, w_dst->cap, nw, np, discard, thin, d_pcnt, d_psum);
    HIP_TRY(logw, hipGetLastError());
    hipLaunchKernelGGL(rw_stat_combine_kernel, dim3(1), dim3(MSX_MAX_GROUP), 0, st, (const long long *)d_pcnt, (const double *)d_psum,
                       (const int64_t *)logw->d_off, (int32_t)k, nw, np, d_stats);
    HIP_TRY(logw, hipGetLastError());
    HIP_TRY(logw, hipMemcpyAsync(stats, d_stats, sizeof(double) * (size_t)(6 * k), hipMemcpyDeviceToHost, st));
    HIP_TRY(logw, hipStreamSynchronize(st));
    w_dst->rows = std::max(w_dst->rows, n);
    return MSX_OK;
}

int msx_series_wmoments(msx_series *src, msx_series *w, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                        double *sumw, double *mean, double *cov) {
    if (!src) return MSX_ERR_INVALID;
    const std::string who("msx_series_wmoments");
    if (!sumw || !mean || ncols < 1) return fail(src, MSX_ERR_INVALID, who + ": bad arguments (ncols >= 1, every output but cov)");
    int64_t np = 0;
    if (int rc = rw_selection(src, who, n, discard, thin, &np)) return rc;
    if (int rc = rw_weights_ok(src, who, w, n)) return rc;
    if (ncols > MSX_MAX_DIM) return fail(src, MSX_ERR_RANGE, who + ": more columns than a series is wide (MSX_MAX_DIM)");
    if (!cols && ncols != src->ndim) return fail(src, MSX_ERR_RANGE, who + ": cols == NULL means all columns (ncols = ndim)");
    RwCols C;
    memset(&C, 0, sizeof(C));
    C.n = ncols;
    for (int32_t q = 0; q < ncols; ++q) {
        const uint32_t c = cols ? cols[q] : (uint32_t)q;
        if (c >= (uint32_t)src->ndim) return fail(src, MSX_ERR_RANGE, who + ": a column outside the series");
        C.c[q] = (int32_t)c;
    }
    HIP_TRY(src, hipSetDevice(src->device));
    const int k = (int)src->off.size() - 1;
    const int64_t nc = ncols, npairs = cov ? nc * (nc + 1) / 2 : 0, nw = src->nw, kc = (int64_t)k * nc, ncov = cov ? kc * nc : 0;
    // scratch: [psum (nc + 1) nw | pcross npairs nw | sumw k | mean k nc | cov k nc nc]
    HIP_TRY(src, series_scratch(src, sizeof(double) * (size_t)((nc + 1 + npairs) * nw + k + kc + ncov)));
    double *d_psum = (double *)src->d_scratch, *d_pcross = d_psum + (nc + 1) * nw, *d_sumw = d_pcross + npairs * nw;
    double *d_mean = d_sumw + k, *d_cov = d_mean + kc;
    hipStream_t st = src->stream;
    HIP_TRY(src, series_wait_growth(src));
    if (w->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, w->grown, 0));
    hipLaunchKernelGGL(rw_wsum_kernel, dim3((unsigned)nw, (unsigned)(nc + 1)), dim3(kRwThreads), 0, st, (const double *)src->d_rows, src->cap, nw,
                       C, (const double *)w->d_rows, w->cap, np, discard, thin, d_psum);
    HIP_TRY(src, hipGetLastError());
    hipLaunchKernelGGL(rw_wmean_kernel, dim3((unsigned)k), dim3(MSX_MAX_DIM + 1), 0, st, (const double *)d_psum, (const int64_t *)src->d_off, nw,
                       (int32_t)nc, d_sumw, d_mean);
    HIP_TRY(src, hipGetLastError());
    if (cov) {
        hipLaunchKernelGGL(rw_wcross_kernel, dim3((unsigned)nw, (unsigned)npairs), dim3(kRwThreads), 0, st, (const double *)src->d_rows, src->cap,
                           nw, C, (const double *)w->d_rows, w->cap, np, discard, thin, (const int64_t *)src->d_off, (int32_t)k,
                           (const double *)d_mean, d_pcross);
        HIP_TRY(src, hipGetLastError());
        hipLaunchKernelGGL(rw_wcov_kernel, dim3((unsigned)k), dim3(MSX_MAX_DIM * (MSX_MAX_DIM + 1) / 2), 0, st, (const double *)d_pcross,
                           (const int64_t *)src->d_off, nw, (int32_t)nc, (const double *)d_sumw, d_cov);
        HIP_TRY(src, hipGetLastError());
        HIP_TRY(src, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)ncov, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> hbuf((size_t)(k + kc));   // (sumw and mean lie side by side: one copy)
    HIP_TRY(src, hipMemcpyAsync(hbuf.data(), d_sumw, sizeof(double) * hbuf.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipStreamSynchronize(st));
    memcpy(sumw, hbuf.data(), sizeof(double) * (size_t)k);
    memcpy(mean, hbuf.data() + k, sizeof(double) * (size_t)kc);
    return MSX_OK;
}

int msx_series_resample(msx_series *src, msx_series *w, int64_t n, int64_t discard, int64_t thin, uint64_t seed, const int64_t *nout,
                        msx_series **dst, int64_t *index_out) {
    if (!src) return MSX_ERR_INVALID;
    const std::string who("msx_series_resample");
    if (!nout || !dst) return fail(src, MSX_ERR_INVALID, who + ": bad arguments (nout and dst)");
    int64_t np = 0;
    if (int rc = rw_selection(src, who, n, discard, thin, &np)) return rc;
    if (int rc = rw_weights_ok(src, who, w, n)) return rc;
    const int k = (int)src->off.size() - 1;
    int64_t max_out = 0, sum_out = 0;
    for (int m = 0; m < k; ++m) {
        if (nout[m] < 0) return fail(src, MSX_ERR_INVALID, who + ": a negative nout");
        max_out = std::max(max_out, nout[m]);
        sum_out += nout[m];
        msx_series *t = dst[m];
        if (!t || t == src || t == w || t->device != src->device || t->nw != 1 || t->off.size() != 2 || t->ndim != src->ndim)
            return fail(src, MSX_ERR_INVALID, who + ": every dst must be another series on the same device with one walker, one member and src's ndim");
        for (int e = 0; e < m; ++e)
            if (dst[e] == t) return fail(src, MSX_ERR_INVALID, who + ": a dst is listed twice");
        if (rw_attached(t)) return fail(src, MSX_ERR_STATE, who + ": a run in flight appends to a dst");
    }
    HIP_TRY(src, hipSetDevice(src->device));
    std::vector<int64_t> tile_off((size_t)k + 1, 0), samp_off((size_t)k + 1, 0);
    for (int m = 0; m < k; ++m) {
        const int64_t N = np * (src->off[(size_t)m + 1] - src->off[(size_t)m]);
        tile_off[(size_t)m + 1] = tile_off[(size_t)m] + (N + kRwTile - 1) / kRwTile;
        samp_off[(size_t)m + 1] = samp_off[(size_t)m] + N;
    }
    const int64_t tiles = tile_off[(size_t)k], sumN = samp_off[(size_t)k];
    if (tiles > 0x7fffffff) return fail(src, MSX_ERR_RANGE, who + ": more samples than one launch covers");
    // scratch: [C sumN | tsum tiles | total k | tlast tiles | tbad tiles | mlast k | mbad k | tile_off k + 1 | samp_off k + 1 | idx sum_out | draws k]
    const size_t b_C = rw_align(sizeof(double) * (size_t)sumN), b_t = rw_align(sizeof(double) * (size_t)tiles), b_k = rw_align(8 * ((size_t)k + 1));
    const size_t b_idx = rw_align(sizeof(long long) * (size_t)std::max<int64_t>(sum_out, 1)), b_draw = rw_align(sizeof(RwDraw) * (size_t)k);
    HIP_TRY(src, series_scratch(src, b_C + 3 * b_t + 5 * b_k + b_idx + b_draw));
    char *p = src->d_scratch;
    double *d_C = (double *)p; p += b_C;
    double *d_tsum = (double *)p; p += b_t;
    double *d_total = (double *)p; p += b_k;
    long long *d_tlast = (long long *)p; p += b_t;
    long long *d_tbad = (long long *)p; p += b_t;
    long long *d_mlast = (long long *)p; p += b_k;
    long long *d_mbad = (long long *)p; p += b_k;
    int64_t *d_tile_off = (int64_t *)p; p += b_k;
    int64_t *d_samp_off = (int64_t *)p; p += b_k;
    long long *d_idx = (long long *)p; p += b_idx;
    RwDraw *d_draws = (RwDraw *)p;
    hipStream_t st = src->stream;
    HIP_TRY(src, hipMemcpyAsync(d_tile_off, tile_off.data(), sizeof(int64_t) * tile_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(src, hipMemcpyAsync(d_samp_off, samp_off.data(), sizeof(int64_t) * samp_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(src, series_wait_growth(src));
    if (w->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, w->grown, 0));
    RwScan S;
    memset(&S, 0, sizeof(S));
    S.wt = w->d_rows; S.wcap = w->cap; S.np = np; S.discard = discard; S.thin = thin;
    S.member_off = src->d_off; S.tile_off = d_tile_off; S.samp_off = d_samp_off; S.k = k;
    hipLaunchKernelGGL(rw_scan_local_kernel, dim3((unsigned)tiles), dim3(kRwThreads), 0, st, S, d_C, d_tsum, d_tlast, d_tbad);
    HIP_TRY(src, hipGetLastError());
    hipLaunchKernelGGL(rw_scan_tiles_kernel, dim3((unsigned)k), dim3(kRwThreads), 0, st, (const int64_t *)d_tile_off, d_tsum,
                       (const long long *)d_tlast, (const long long *)d_tbad, d_total, d_mlast, d_mbad);
    HIP_TRY(src, hipGetLastError());
    std::vector<double> total((size_t)k);
    std::vector<long long> mlast((size_t)k), mbad((size_t)k);
    HIP_TRY(src, hipMemcpyAsync(total.data(), d_total, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipMemcpyAsync(mlast.data(), d_mlast, sizeof(long long) * (size_t)k, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipMemcpyAsync(mbad.data(), d_mbad, sizeof(long long) * (size_t)k, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipStreamSynchronize(st));
    // refused before anything is written to a dst
    for (int m = 0; m < k; ++m) {
        if (mbad[(size_t)m] > 0) return fail(src, MSX_ERR_RANGE, who + ": member " + std::to_string(m) + " has a weight that is negative, NaN or infinite");
        if (nout[m] > 0 && (!(total[(size_t)m] > 0.0) || !std::isfinite(total[(size_t)m]) || mlast[(size_t)m] < 0))
            return fail(src, MSX_ERR_RANGE, who + ": member " + std::to_string(m) + "'s weights sum to zero (or overflow): nothing to draw from");
    }
    if (sum_out == 0) {
        for (int m = 0; m < k; ++m) dst[m]->rows = 0;
        return MSX_OK;
    }
    hipLaunchKernelGGL(rw_scan_add_kernel, dim3((unsigned)tiles), dim3(kRwThreads), 0, st, S, (const double *)d_tsum, d_C);
    HIP_TRY(src, hipGetLastError());
    std::vector<RwDraw> draws((size_t)k);
    int64_t at = 0;
    for (int m = 0; m < k; ++m) {
        msx_series *t = dst[m];
        RwDraw &D = draws[(size_t)m];
        memset(&D, 0, sizeof(D));
        D.nout = nout[m];
        D.out_off = at;
        at += nout[m];
        if (nout[m] == 0) continue;
        HIP_TRY(src, series_reserve(t, nout[m], 0, st));   // (grown the way append grows a series; nothing carried over)
        D.step = total[(size_t)m] / (double)nout[m];
        D.u0 = counter_uniform(seed, (unsigned long long)m, kRwStream, 0u);
        D.last = mlast[(size_t)m];
        D.dst = t->d_rows;
        D.dcap = t->cap;
    }
    HIP_TRY(src, hipMemcpyAsync(d_draws, draws.data(), sizeof(RwDraw) * (size_t)k, hipMemcpyHostToDevice, st));
    for (int m = 0; m < k; ++m)
        if (dst[m]->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, dst[m]->grown, 0));
    hipLaunchKernelGGL(rw_draw_kernel, dim3((unsigned)((max_out + kRwThreads - 1) / kRwThreads), (unsigned)k), dim3(kRwThreads), 0, st, S,
                       (const double *)d_C, (const RwDraw *)d_draws, (const double *)src->d_rows, src->cap, src->nw, (int32_t)src->ndim, d_idx);
    HIP_TRY(src, hipGetLastError());
    if (index_out) HIP_TRY(src, hipMemcpyAsync(index_out, d_idx, sizeof(int64_t) * (size_t)sum_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(src, hipStreamSynchronize(st));
    for (int m = 0; m < k; ++m) dst[m]->rows = nout[m];
    return MSX_OK;
}

// ---- Pareto-smoothed importance sampling (psis_kernels.h) -------------------------------------------
int msx_series_psis(msx_series *logw, int64_t n, int64_t discard, int64_t thin, const int64_t *tail_len, msx_series *w_dst,
                    msx_series *lw_dst, double *khat, int32_t *status, int64_t *tail_count, double *stats, int64_t *tail_index) {
    if (!logw) return MSX_ERR_INVALID;
    const std::string who("msx_series_psis");
    if (!tail_len || !w_dst || !khat || !status || !tail_count || !stats)
        return fail(logw, MSX_ERR_INVALID, who + ": bad arguments (tail_len, w_dst, khat, status, tail_count and stats)");
    if (logw->ndim != 1 || w_dst == logw || !rw_same_members(logw, w_dst) || w_dst->ndim != 1)
        return fail(logw, MSX_ERR_INVALID, who + ": the log-weights and w_dst must be two series of ndim = 1 on one device with the same members");
    if (lw_dst && (lw_dst == logw || lw_dst == w_dst || !rw_same_members(logw, lw_dst) || lw_dst->ndim != 1))
        return fail(logw, MSX_ERR_INVALID, who + ": lw_dst must be a third series of ndim = 1 on the same device with the same members");
    if (rw_attached(w_dst) || (lw_dst && rw_attached(lw_dst))) return fail(logw, MSX_ERR_STATE, who + ": a run in flight appends to a destination");
    int64_t np = 0;
    if (int rc = rw_selection(logw, who, n, discard, thin, &np)) return rc;
    if (logw->nw > 65535) return fail(logw, MSX_ERR_RANGE, who + ": more walkers than one launch covers");
    const int k = (int)logw->off.size() - 1;
    const int64_t nw = logw->nw;
    for (int m = 0; m < k; ++m) {
        if (np * (logw->off[(size_t)m + 1] - logw->off[(size_t)m]) > 0x7fffffffll)
            return fail(logw, MSX_ERR_RANGE, who + ": a member of 2^31 samples or more");
        if (tail_len[m] < 1 || tail_len[m] > MSX_PSIS_TAIL_MAX)
            return fail(logw, MSX_ERR_RANGE, who + ": member " + std::to_string(m) + "'s tail_len lies outside 1 .. MSX_PSIS_TAIL_MAX");
    }
    HIP_TRY(logw, hipSetDevice(logw->device));
    hipStream_t st = logw->stream;
    // scratch, w_dst's (the selection below uses logw's): [pmax nw | psum 2 nw | cut k | res 3 k | stats 6 k | pcnt 2 nw | nbad k | tail k TAIL_MAX]
    const size_t b_tail = tail_index ? sizeof(long long) * (size_t)k * MSX_PSIS_TAIL_MAX : 0;
    HIP_TRY(logw, series_scratch(w_dst, sizeof(double) * (size_t)(3 * nw + 10 * k) + sizeof(long long) * (size_t)(2 * nw + k) + b_tail));
    double *d_pmax = (double *)w_dst->d_scratch, *d_psum = d_pmax + nw, *d_cut = d_psum + 2 * nw, *d_res = d_cut + k, *d_stats = d_res + 3 * k;
    long long *d_pcnt = (long long *)(d_stats + 6 * k);
    unsigned long long *d_nbad = (unsigned long long *)(d_pcnt + 2 * nw);
    long long *d_tail = tail_index ? (long long *)(d_nbad + k) : nullptr;
    HIP_TRY(logw, series_wait_growth(logw));
    HIP_TRY(logw, hipMemsetAsync(d_nbad, 0, sizeof(unsigned long long) * (size_t)k, st));
    hipLaunchKernelGGL(psis_scan_kernel, dim3((unsigned)nw), dim3(kPsThreads), 0, st, (const double *)logw->d_rows, logw->cap, np, discard, thin,
                       (const int64_t *)logw->d_off, (int32_t)k, d_pmax, d_nbad);
    HIP_TRY(logw, hipGetLastError());
    std::vector<unsigned long long> nbad((size_t)k);
    HIP_TRY(logw, hipMemcpyAsync(nbad.data(), d_nbad, sizeof(unsigned long long) * (size_t)k, hipMemcpyDeviceToHost, st));
    HIP_TRY(logw, hipStreamSynchronize(st));
    std::vector<int64_t> ranks((size_t)k);
    for (int m = 0; m < k; ++m) {
        const int64_t S = np * (logw->off[(size_t)m + 1] - logw->off[(size_t)m]) - (int64_t)nbad[(size_t)m];
        if (tail_len[m] > S - 1)
            return fail(logw, MSX_ERR_RANGE, who + ": member " + std::to_string(m) + "'s tail_len lies outside 1 .. S - 1 (S = " + std::to_string(S) +
                                                 " samples that are not NaN or +inf)");
        ranks[(size_t)m] = S - tail_len[m] - 1;   // (NaN and +inf take the top keys of the selection: the bad values lie above every rank < S)
    }
    std::vector<double> cut((size_t)k);
    const uint32_t col0 = 0;
    if (int rc = msx_series_order_stats(logw, n, discard, thin, &col0, 1, ranks.data(), 1, cut.data(), nullptr)) return rc;
    HIP_TRY(logw, series_reserve(w_dst, n, w_dst->rows, st));
    if (lw_dst) HIP_TRY(logw, series_reserve(lw_dst, n, lw_dst->rows, st));
    if (w_dst->grown_set) HIP_TRY(logw, hipStreamWaitEvent(st, w_dst->grown, 0));
    if (lw_dst && lw_dst->grown_set) HIP_TRY(logw, hipStreamWaitEvent(st, lw_dst->grown, 0));
    HIP_TRY(logw, hipMemcpyAsync(d_cut, cut.data(), sizeof(double) * (size_t)k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(psis_fill_kernel, dim3((unsigned)((n + kPsThreads - 1) / kPsThreads), (unsigned)nw), dim3(kPsThreads), 0, st, n, w_dst->d_rows,
                       w_dst->cap, lw_dst ? lw_dst->d_rows : nullptr, lw_dst ? lw_dst->cap : 0);
    HIP_TRY(logw, hipGetLastError());
    PsisArgs A;
    memset(&A, 0, sizeof(A));
    A.logw = logw->d_rows; A.cap = logw->cap; A.np = np; A.discard = discard; A.thin = thin;
    A.member_off = logw->d_off; A.pmax = d_pmax; A.cut = d_cut;
    A.wt = w_dst->d_rows; A.wcap = w_dst->cap;
    A.lwt = lw_dst ? lw_dst->d_rows : nullptr; A.lcap = lw_dst ? lw_dst->cap : 0;
    A.res = d_res; A.tail_index = d_tail;
    hipLaunchKernelGGL(psis_reduce_kernel, dim3((unsigned)k), dim3(kPsThreads), 0, st, A);
    HIP_TRY(logw, hipGetLastError());
    hipLaunchKernelGGL(rw_stat_kernel, dim3((unsigned)nw), dim3(kRwThreads), 0, st, (const double *)logw->d_rows, logw->cap,
                       (const double *)w_dst->d_rows, w_dst->cap, nw, np, discard, thin, d_pcnt, d_psum);
    HIP_TRY(logw, hipGetLastError());
    hipLaunchKernelGGL(rw_stat_combine_kernel, dim3(1), dim3(MSX_MAX_GROUP), 0, st, (const long long *)d_pcnt, (const double *)d_psum,
                       (const int64_t *)logw->d_off, (int32_t)k, nw, np, d_stats);
    HIP_TRY(logw, hipGetLastError());
    std::vector<double> hbuf((size_t)(9 * k));   // (res and stats lie side by side: one copy)
    HIP_TRY(logw, hipMemcpyAsync(hbuf.data(), d_res, sizeof(double) * hbuf.size(), hipMemcpyDeviceToHost, st));
    if (tail_index) HIP_TRY(logw, hipMemcpyAsync(tail_index, d_tail, b_tail, hipMemcpyDeviceToHost, st));
    HIP_TRY(logw, hipStreamSynchronize(st));
    for (int m = 0; m < k; ++m) {
        khat[m] = hbuf[(size_t)m * 3];
        status[m] = (int32_t)hbuf[(size_t)m * 3 + 1];
        tail_count[m] = (int64_t)hbuf[(size_t)m * 3 + 2];
    }
    memcpy(stats, hbuf.data() + 3 * k, sizeof(double) * (size_t)(6 * k));
    w_dst->rows = std::max(w_dst->rows, n);
    if (lw_dst) lw_dst->rows = std::max(lw_dst->rows, n);
    return MSX_OK;
}

// ---- pointwise model checks: PSIS-LOO, WAIC, khat per observation (pointwise_kernels.h) -------------
static int64_t pw_nobs(const msx_ctx *c) { return (c->PM.no_spectrum ? 0 : c->PM.npix) + c->PM.nc + c->PM.np; }
// the smallest scratch a job can run in: one work row of the sample pass, or one observation's terms of every selected sample
static size_t pw_min_bytes(int64_t npix, int64_t nsel) { return sizeof(double) * (size_t)std::max(npix, nsel); }
// ceil(min(S / 5, 3 sqrt(S / reff))): the papers' tail length, computed here on the host, once (psis.tail_len's expression)
static int64_t pw_tail_len(int64_t S, double reff) {
    const double dS = (double)S;
    return (int64_t)ceil(std::min(dS / 5.0, 3.0 * sqrt(dS / reff)));
}
struct PwSizes {
    size_t b_rec, b_status, b_vidx, b_out, b_big, total;
};
static PwSizes pw_sizes(const PredJob &J, size_t budget) {
    PwSizes Z;
    const int64_t npix = J.c->PM.npix, nobs = pw_nobs(J.c);
    const size_t most = sizeof(double) * (size_t)std::max(npix * J.nall, nobs * J.nsel);  // everything at once
    Z.b_big = pred_align(std::min(budget, most));
    Z.b_rec = pred_align(sizeof(PredRec) * (size_t)J.nall);
    Z.b_status = pred_align(sizeof(int32_t) * (size_t)J.nall);
    Z.b_vidx = pred_align(sizeof(int64_t) * (size_t)J.nsel);
    Z.b_out = pred_align(sizeof(double) * (size_t)(kPwOut * nobs));
    Z.total = Z.b_rec + Z.b_status + Z.b_vidx + Z.b_out + Z.b_big;
    return Z;
}

// Runs the job on `st` inside d_arena (pw_sizes(...).total bytes) and waits for it.  out [6][n_obs], status_out [nall] or null,
// ll_out [n_obs][count] or null: host; nothing is written to them before the job has succeeded up to the tail's check.
static int pw_run(const PredJob &J, hipStream_t st, char *d_arena, const PwSizes &Z, size_t budget, double reff, double *out,
                  int32_t *status_out, int64_t *count_out, int64_t *tail_out, int32_t *worst_out, double *ll_out, std::string *err) {
#define PW_TRY(expr)                                                                                \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) { *err = std::string(#expr) + ": " + hipGetErrorString(e__); return MSX_ERR_HIP; } \
    } while (0)
    const int ns = J.c->PM.nspec;
    const int64_t npix = J.c->PM.npix, nobs = pw_nobs(J.c), nb = J.c->PM.nc + J.c->PM.np, npx = nobs - nb;
    char *at = d_arena;
    PredRec *d_rec = reinterpret_cast<PredRec *>(at); at += Z.b_rec;
    int32_t *d_status = reinterpret_cast<int32_t *>(at); at += Z.b_status;
    int64_t *d_vidx = reinterpret_cast<int64_t *>(at); at += Z.b_vidx;
    double *d_out = reinterpret_cast<double *>(at); at += Z.b_out;
    double *d_big = reinterpret_cast<double *>(at);
    const size_t big = std::min(budget, Z.b_big);
    // the unchanged sample pass of the predictive check, without its terms
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(J.nall, (int64_t)(big / (sizeof(double) * (size_t)std::max<int64_t>(npix, 1)))));
    PredSampleLaunch SL;
    memset(&SL, 0, sizeof(SL));
    SL.M = J.c->d_prod_member; SL.src = J.src; SL.work = d_big; SL.rec = d_rec; SL.status = d_status;
    for (int64_t i0 = 0; i0 < J.nall; i0 += batch) {
        SL.i0 = i0;
        const dim3 grid((unsigned)std::min(batch, J.nall - i0));
        if (ns == 2) hipLaunchKernelGGL(predictive_sample_kernel<2>, grid, dim3(kPredThreads), 0, st, SL);
        else hipLaunchKernelGGL(predictive_sample_kernel<3>, grid, dim3(kPredThreads), 0, st, SL);
        PW_TRY(hipGetLastError());
    }
    std::vector<int32_t> status((size_t)J.nall);
    PW_TRY(hipMemcpyAsync(status.data(), d_status, sizeof(int32_t) * (size_t)J.nall, hipMemcpyDeviceToHost, st));
    PW_TRY(hipStreamSynchronize(st));
    std::vector<int64_t> vidx;
    vidx.reserve((size_t)J.nsel);
    int32_t worst = 0;
    for (int64_t i = 0; i < J.nall; ++i) {
        worst = std::max(worst, status[(size_t)i]);
        const int64_t ri = i / J.src.W;
        if (ri >= J.sel0 && (ri - J.sel0) % J.selstep == 0 && status[(size_t)i] == MSX_W_OK) vidx.push_back(i);
    }
    const int64_t count = (int64_t)vidx.size();
    const int64_t tail = count >= 2 ? std::min(pw_tail_len(count, reff), count - 1) : 0;
    if (tail > MSX_PSIS_TAIL_MAX) {
        *err = "the tail of " + std::to_string(count) + " samples is longer than MSX_PSIS_TAIL_MAX";
        return MSX_ERR_RANGE;
    }
    if (status_out) memcpy(status_out, status.data(), sizeof(int32_t) * (size_t)J.nall);
    *count_out = count;
    if (tail_out) *tail_out = tail;
    if (worst_out) *worst_out = worst;
    if (count < 2 || tail < 1) {   // nothing to leave out
        std::fill(out, out + kPwOut * nobs, (double)NAN);
        return MSX_OK;
    }
    PW_TRY(hipMemcpyAsync(d_vidx, vidx.data(), sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice, st));
    // observation tiles sized from the scratch by the SELECTED samples (not by how many turned out valid)
    const int64_t tile = std::max<int64_t>(1, (int64_t)(big / (sizeof(double) * (size_t)J.nsel)));
    PwPixelLaunch XL;
    memset(&XL, 0, sizeof(XL));
    XL.M = J.c->d_prod_member; XL.rec = d_rec; XL.vidx = d_vidx; XL.count = count; XL.vals = d_big;
    XL.coef = (-0.5 * (double)nb) / (double)npix;
    PwBandLaunch BL;
    memset(&BL, 0, sizeof(BL));
    BL.M = J.c->d_prod_member; BL.rec = d_rec; BL.vidx = d_vidx; BL.src = J.src; BL.count = count; BL.vals = d_big;
    PwReduceLaunch RL;
    memset(&RL, 0, sizeof(RL));
    RL.vals = d_big; RL.count = count; RL.n_obs = nobs; RL.tail_len = tail; RL.out = d_out;
    for (int64_t o0 = 0; o0 < nobs;) {
        const bool pixels = o0 < npx;
        const int64_t to = std::min(tile, (pixels ? npx : nobs) - o0);   // (a tile holds pixels or filters, not both)
        if (pixels) {
            XL.p0 = o0; XL.tp = to;
            const int64_t gx = (count + kPredTile - 1) / kPredTile, chunks = (to + kPredTile - 1) / kPredTile;
            const dim3 fgrid((unsigned)gx, (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, 2048 / std::min<int64_t>(gx, 2048))));
            if (ns == 2) hipLaunchKernelGGL(pointwise_pixel_kernel<2>, fgrid, dim3(kPredThreads), 0, st, XL);
            else hipLaunchKernelGGL(pointwise_pixel_kernel<3>, fgrid, dim3(kPredThreads), 0, st, XL);
        } else {
            BL.f0 = (int32_t)(o0 - npx); BL.tf = (int32_t)to;
            const dim3 bgrid((unsigned)((count + kPredThreads - 1) / kPredThreads));
            if (ns == 2) hipLaunchKernelGGL(pointwise_band_kernel<2>, bgrid, dim3(kPredThreads), 0, st, BL);
            else hipLaunchKernelGGL(pointwise_band_kernel<3>, bgrid, dim3(kPredThreads), 0, st, BL);
        }
        PW_TRY(hipGetLastError());
        RL.o0 = o0;
        hipLaunchKernelGGL(pointwise_reduce_kernel, dim3((unsigned)to), dim3(kPredThreads), 0, st, RL);
        PW_TRY(hipGetLastError());
        if (ll_out) PW_TRY(hipMemcpyAsync(ll_out + o0 * count, d_big, sizeof(double) * (size_t)(to * count), hipMemcpyDeviceToHost, st));
        o0 += to;
    }
    PW_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)(kPwOut * nobs), hipMemcpyDeviceToHost, st));
    PW_TRY(hipStreamSynchronize(st));
    return MSX_OK;
#undef PW_TRY
}

int msx_pointwise_nobs(msx_ctx *c, int64_t *npix, int32_t *n_contrast, int32_t *n_phot) {
    if (!c) return MSX_ERR_INVALID;
    if (!npix || !n_contrast || !n_phot) return fail(c, MSX_ERR_INVALID, "msx_pointwise_nobs: bad arguments");
    if (!c->problem_staged || !c->products_staged) return fail(c, MSX_ERR_STATE, "msx_pointwise_nobs: no products staged (msx_stage_products)");
    *npix = c->PM.no_spectrum ? 0 : c->PM.npix;
    *n_contrast = c->PM.nc;
    *n_phot = c->PM.np;
    return MSX_OK;
}

int msx_predictive_pointwise(msx_ctx *c, const double *theta, int64_t n, int32_t ndim, double reff, int64_t scratch_bytes, double *out,
                             int32_t *status, int64_t *count, int64_t *tail_len, double *ll_out) {
    if (!c) return MSX_ERR_INVALID;
    const std::string who("msx_predictive_pointwise");
    if (!theta || !out || !status || !count || n < 1 || scratch_bytes < 0 || !(reff > 0.0) || !std::isfinite(reff))
        return fail(c, MSX_ERR_INVALID, who + ": bad arguments (theta, out, status, count, n >= 1, scratch_bytes >= 0, reff > 0)");
    if (!c->problem_staged || !c->products_staged) return fail(c, MSX_ERR_STATE, who + ": no products staged (msx_stage_products)");
    if (ndim != 2 * c->P.nspec + 2) return fail(c, MSX_ERR_INVALID, who + ": ndim must be 2 * nspec + 2");
    if (c->P.npix > INT32_MAX || n > INT32_MAX) return fail(c, MSX_ERR_RANGE, who + ": too many pixels or samples");
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kPredDefaultBytes;
    if (budget < pw_min_bytes(c->P.npix, n))
        return fail(c, MSX_ERR_RANGE, who + ": scratch_bytes holds neither one model row nor one observation's terms of the n samples (8 * max(npix, n) bytes)");
    if (ll_out && sizeof(double) * (size_t)pw_nobs(c) * (size_t)n > (size_t)MSX_POINTWISE_MATRIX_MAX)
        return fail(c, MSX_ERR_RANGE, who + ": the pointwise matrix is larger than MSX_POINTWISE_MATRIX_MAX bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    PredJob J;
    memset(&J, 0, sizeof(J));
    J.c = c; J.nall = n; J.sel0 = 0; J.selstep = 1; J.nsel = n;
    const PwSizes Z = pw_sizes(J, budget);
    const size_t b_theta = pred_align(sizeof(double) * (size_t)(n * ndim));
    const size_t need = b_theta + Z.total;
    if (need > c->prod_buf_bytes) {
        if (c->d_prod_buf) (void)hipFree(c->d_prod_buf);
        c->d_prod_buf = nullptr; c->prod_buf_bytes = 0;
        HIP_TRY(c, hipMalloc((void **)&c->d_prod_buf, need));
        c->prod_buf_bytes = need;
    }
    double *d_theta = reinterpret_cast<double *>(c->d_prod_buf);
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, sizeof(double) * (size_t)(n * ndim), hipMemcpyHostToDevice, c->stream));
    J.src.base = d_theta; J.src.W = n; J.src.w0 = 0; J.src.sw = ndim; J.src.sr = 0; J.src.sd = 1; J.src.row0 = 0; J.src.rstep = 1;
    std::string err;
    if (int rc = pw_run(J, c->stream, c->d_prod_buf + b_theta, Z, budget, reff, out, status, count, tail_len, nullptr, ll_out, &err))
        return fail(c, rc, who + ": " + err);
    return MSX_OK;
}

int msx_series_pointwise(msx_series *src, msx_ctx **ctxs, int64_t n, int64_t discard, int64_t thin, double reff, int64_t scratch_bytes,
                         double *out, int64_t *count, int64_t *tail_len, int32_t *worst_status, double *ll_out) {
    if (!src) return MSX_ERR_INVALID;
    const std::string who("msx_series_pointwise");
    if (!ctxs || !out || !count || discard < 0 || thin < 1 || scratch_bytes < 0 || !(reff > 0.0) || !std::isfinite(reff))
        return fail(src, MSX_ERR_INVALID, who + ": bad arguments (ctxs, out, count, discard >= 0, thin >= 1, scratch_bytes >= 0, reff > 0)");
    if (n < 1 || n > src->rows) return fail(src, MSX_ERR_RANGE, who + ": n must lie in 1 .. the rows the series holds");
    const int64_t np = discard < n ? (n - discard + thin - 1) / thin : 0;
    if (np < 1) return fail(src, MSX_ERR_RANGE, who + ": the selection rows[0:n][discard::thin] is empty");
    const int k = (int)src->off.size() - 1;
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kPredDefaultBytes;
    int nspec = 0;
    std::vector<PredJob> jobs((size_t)k);
    size_t arena = 0, matrix = 0;
    for (int m = 0; m < k; ++m) {
        const msx_ctx *c = ctxs[m];
        const std::string mem = who + ": member " + std::to_string(m);
        if (!c) return fail(src, MSX_ERR_INVALID, mem + " is null");
        if (c->device != src->device) return fail(src, MSX_ERR_INVALID, mem + " lives on another device");
        if (!c->problem_staged || !c->products_staged) return fail(src, MSX_ERR_STATE, mem + " has no staged products (msx_stage_products)");
        if (m == 0) nspec = c->PM.nspec;
        if (c->PM.nspec != nspec || src->ndim != 2 * nspec + 2) return fail(src, MSX_ERR_INVALID, mem + ": src's ndim must be 2 * nspec + 2 of every member");
        const int64_t W = src->off[(size_t)m + 1] - src->off[(size_t)m];
        PredJob &J = jobs[(size_t)m];
        memset(&J, 0, sizeof(J));
        J.c = c;
        J.src.W = W; J.src.w0 = src->off[(size_t)m];
        J.src.row0 = discard; J.src.rstep = thin; J.nall = np * W; J.sel0 = 0; J.selstep = 1; J.nsel = np * W;
        if (c->PM.npix > INT32_MAX || J.nsel > INT32_MAX) return fail(src, MSX_ERR_RANGE, mem + ": too many pixels or samples");
        if (budget < pw_min_bytes(c->PM.npix, J.nsel))
            return fail(src, MSX_ERR_RANGE, mem + ": scratch_bytes holds neither one model row nor one observation's terms of its samples (8 * max(npix, N_m) bytes)");
        matrix += sizeof(double) * (size_t)pw_nobs(c) * (size_t)J.nsel;
        arena = std::max(arena, pw_sizes(J, budget).total);
    }
    if (ll_out && matrix > (size_t)MSX_POINTWISE_MATRIX_MAX) return fail(src, MSX_ERR_RANGE, who + ": the pointwise matrices are larger than MSX_POINTWISE_MATRIX_MAX bytes");
    HIP_TRY(src, hipSetDevice(src->device));
    hipStream_t st = src->stream;
    HIP_TRY(src, series_scratch(src, arena));
    HIP_TRY(src, series_wait_growth(src));
    size_t o_out = 0, o_ll = 0;
    for (int m = 0; m < k; ++m) {
        PredJob &J = jobs[(size_t)m];
        J.src.base = src->d_rows; J.src.sw = src->cap; J.src.sr = 1; J.src.sd = src->nw * src->cap;
        const PwSizes Z = pw_sizes(J, budget);
        std::string err;
        int32_t worst = 0;
        if (int rc = pw_run(J, st, src->d_scratch, Z, budget, reff, out + o_out, nullptr, count + m, tail_len ? tail_len + m : nullptr, &worst,
                            ll_out ? ll_out + o_ll : nullptr, &err))
            return fail(src, rc, who + ": member " + std::to_string(m) + ": " + err);
        if (worst_status) worst_status[m] = worst;
        o_out += (size_t)(kPwOut * pw_nobs(J.c)); o_ll += (size_t)pw_nobs(J.c) * (size_t)J.nsel;
    }
    return MSX_OK;
}

// ---- the split pool, transformed: ranks by a segmented radix sort (rank_kernels.h) --------------------
static constexpr size_t kRankDefaultBytes = (size_t)256 << 20;
static int64_t rank_tiles(int64_t S) { return (S + kRankTile - 1) / kRankTile; }

// one segment's share of a round's arena: [keys 2 x 8 S | tile_first, tile_last 16 T | RankSeg | positions 2 x 4 S | tile_hist
// 1024 T | hist8 8192 | digit_base 1024]; the 8-byte arrays come first, so a round's arena is the sum of its segments' shares
int64_t msx_split_scratch_bytes(int64_t S) {
    if (S < 1) return 0;
    return 24 * S + (int64_t)(sizeof(uint32_t) * kRankDigits + 2 * sizeof(long long)) * rank_tiles(S) +
           (int64_t)(sizeof(RankSeg) + sizeof(uint32_t) * (kRankPasses + 1) * kRankDigits);
}

int msx_series_split_transform(msx_series *src, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                               int32_t transform, const double *param, int64_t scratch_bytes, msx_series *dst) {
    if (!src) return MSX_ERR_INVALID;
    const char *who = "msx_series_split_transform";
    const std::string w(who);
    const bool ranked = transform == kSplitRanknorm || transform == kSplitFoldRanknorm || transform == kSplitRank2;
    const bool reads_param = transform == kSplitFoldRanknorm || transform == kSplitIndicator;
    if (!dst || dst == src || !cols || ncols < 1 || discard < 0 || thin < 1 || scratch_bytes < 0 || transform < kSplitIdentity ||
        transform > kSplitRank2 || (reads_param && !param))
        return fail(src, MSX_ERR_INVALID, w + ": bad arguments (another series as dst, cols, discard >= 0, thin >= 1, a known transform and its param)");
    if (dst->device != src->device) return fail(src, MSX_ERR_INVALID, w + ": dst lives on another device");
    if (rw_attached(dst)) return fail(src, MSX_ERR_STATE, w + ": a run in flight appends to dst");
    if (n < 1 || n > src->rows) return fail(src, MSX_ERR_RANGE, w + ": n must lie in 1 .. the rows the series holds");
    const int64_t np = n > discard ? (n - discard + thin - 1) / thin : 0, h = np / 2;
    if (np < 4) return fail(src, MSX_ERR_RANGE, w + ": the selection rows[0:n][discard::thin] needs at least 4 rows");
    if (ncols > MSX_MAX_DIM) return fail(src, MSX_ERR_RANGE, w + ": more columns than a series is wide (MSX_MAX_DIM)");
    if (int rc = summary_columns(src, who, cols, ncols)) return rc;
    const int k = (int)src->off.size() - 1;
    if ((int64_t)k * ncols > 65535) return fail(src, MSX_ERR_RANGE, w + ": more segments (members x columns) than one launch covers");
    bool shaped = dst->nw == 2 * src->nw && dst->ndim == ncols && dst->off.size() == src->off.size();
    for (int m = 0; shaped && m <= k; ++m) shaped = dst->off[(size_t)m] == 2 * src->off[(size_t)m];
    if (!shaped) return fail(src, MSX_ERR_RANGE, w + ": dst needs 2 nw walkers, members of 2 W_m walkers and ndim = ncols");
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kRankDefaultBytes;
    std::vector<RankSeg> segs((size_t)k * (size_t)ncols);
    for (int m = 0; m < k; ++m)
        for (int32_t j = 0; j < ncols; ++j) {
            RankSeg &s = segs[(size_t)m * (size_t)ncols + (size_t)j];
            memset(&s, 0, sizeof(s));
            s.w0 = src->off[(size_t)m];
            s.S = 2 * (src->off[(size_t)m + 1] - src->off[(size_t)m]) * h;
            s.ntiles = rank_tiles(s.S);
            s.col = cols[j];
            s.jc = j;
            s.param = reads_param ? param[(size_t)m * (size_t)ncols + (size_t)j] : 0.0;
            if (s.S > (int64_t)INT32_MAX) return fail(src, MSX_ERR_RANGE, w + ": a member's column holds 2^31 values or more");
            if (ranked && (size_t)msx_split_scratch_bytes(s.S) > budget)
                return fail(src, MSX_ERR_RANGE, w + ": scratch_bytes is below one segment's need (msx_split_scratch_bytes)");
        }
    // rounds of consecutive segments within the budget (all of them at once when nothing is sorted)
    std::vector<size_t> cut(1, 0);
    size_t arena = 0, used = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const size_t need = ranked ? (size_t)msx_split_scratch_bytes(segs[i].S) : sizeof(RankSeg);
        if (ranked && used && used + need > budget) {
            cut.push_back(i);
            used = 0;
        }
        used += need;
        arena = std::max(arena, used);
    }
    cut.push_back(segs.size());
    HIP_TRY(src, hipSetDevice(src->device));
    hipStream_t st = src->stream;
    HIP_TRY(src, series_scratch(src, arena));     // (first: a failure here leaves dst's buffer as it was)
    HIP_TRY(src, series_reserve(dst, h, 0, st));  // (every row 0 .. h - 1 is written below)
    HIP_TRY(src, series_wait_growth(src));
    if (dst->grown_set) HIP_TRY(src, hipStreamWaitEvent(st, dst->grown, 0));
    const RankGeom g = {src->d_rows, src->cap, src->nw, np, h, discard, thin, dst->d_rows, dst->cap};
    std::vector<uint32_t> h8;
    for (size_t r = 0; r + 1 < cut.size(); ++r) {
        RankSeg *S0 = segs.data() + cut[r];
        const int64_t G = (int64_t)(cut[r + 1] - cut[r]);
        int64_t N = 0, T = 0, tmax = 0;
        for (int64_t i = 0; i < G; ++i) {
            S0[i].base = N;
            S0[i].tile0 = T;
            N += S0[i].S;
            T += S0[i].ntiles;
            tmax = std::max(tmax, S0[i].ntiles);
        }
        const dim3 grid((unsigned)tmax, (unsigned)G);
        if (!ranked) {
            RankSeg *d_segs = (RankSeg *)src->d_scratch;
            HIP_TRY(src, hipMemcpyAsync(d_segs, S0, sizeof(RankSeg) * (size_t)G, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(rank_plain_kernel, grid, dim3(kRankThreads), 0, st, g, (const RankSeg *)d_segs, transform);
            HIP_TRY(src, hipGetLastError());
            HIP_TRY(src, hipStreamSynchronize(st));
            continue;
        }
        unsigned long long *d_ka = (unsigned long long *)src->d_scratch, *d_kb = d_ka + N;
        long long *d_first = (long long *)(d_kb + N), *d_last = d_first + T;
        RankSeg *d_segs = (RankSeg *)(d_last + T);
        uint32_t *d_pa = (uint32_t *)(d_segs + G), *d_pb = d_pa + N, *d_th = d_pb + N;
        uint32_t *d_h8 = d_th + T * kRankDigits, *d_db = d_h8 + G * kRankPasses * kRankDigits;
        HIP_TRY(src, hipMemcpyAsync(d_segs, S0, sizeof(RankSeg) * (size_t)G, hipMemcpyHostToDevice, st));
        HIP_TRY(src, hipMemsetAsync(d_h8, 0, sizeof(uint32_t) * (size_t)(G * kRankPasses * kRankDigits), st));
        hipLaunchKernelGGL(rank_key_kernel, grid, dim3(kRankThreads), 0, st, g, (const RankSeg *)d_segs, transform, d_ka, d_pa, d_h8);
        HIP_TRY(src, hipGetLastError());
        h8.resize((size_t)(G * kRankPasses * kRankDigits));
        HIP_TRY(src, hipMemcpyAsync(h8.data(), d_h8, sizeof(uint32_t) * h8.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(src, hipStreamSynchronize(st));
        for (int p = 0; p < kRankPasses; ++p) {
            // a digit that is the same all over every segment of the round moves nothing: no pass
            bool uniform = true;
            for (int64_t i = 0; uniform && i < G; ++i) {
                const uint32_t *hp = h8.data() + (size_t)((i * kRankPasses + p) * kRankDigits);
                uniform = std::find(hp, hp + kRankDigits, (uint32_t)S0[i].S) != hp + kRankDigits;
            }
            if (uniform) continue;
            const int32_t shift = p * kRankDigitBits;
            hipLaunchKernelGGL(rank_hist_kernel, grid, dim3(kRankThreads), 0, st, (const RankSeg *)d_segs, (const unsigned long long *)d_ka,
                               shift, d_th);
            HIP_TRY(src, hipGetLastError());
            hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)G), dim3(kRankDigits), 0, st, (const RankSeg *)d_segs, d_th, d_db);
            HIP_TRY(src, hipGetLastError());
            hipLaunchKernelGGL(rank_scatter_kernel, grid, dim3(kRankThreads), 0, st, (const RankSeg *)d_segs, (const unsigned long long *)d_ka,
                               (const uint32_t *)d_pa, shift, (const uint32_t *)d_th, (const uint32_t *)d_db, d_kb, d_pb);
            HIP_TRY(src, hipGetLastError());
            std::swap(d_ka, d_kb);
            std::swap(d_pa, d_pb);
        }
        hipLaunchKernelGGL(rank_flag_kernel, grid, dim3(kRankThreads), 0, st, (const RankSeg *)d_segs, (const unsigned long long *)d_ka, d_first,
                           d_last);
        HIP_TRY(src, hipGetLastError());
        hipLaunchKernelGGL(rank_assign_kernel, grid, dim3(kRankThreads), 0, st, g, (const RankSeg *)d_segs, transform,
                           (const unsigned long long *)d_ka, (const uint32_t *)d_pa, (const long long *)d_first, (const long long *)d_last);
        HIP_TRY(src, hipGetLastError());
        HIP_TRY(src, hipStreamSynchronize(st));
    }
    dst->rows = h;
    return MSX_OK;
}

// ---- the chain-averaged autocovariance of a series whose walkers are the chains ----------------------
int msx_series_chain_acov(msx_series *sr, int64_t n, int64_t lag0, int64_t nlag, const uint32_t *cols, int32_t ncols, double *acov_out,
                          double *meanvar_out, double *between_out) {
    if (!sr) return MSX_ERR_INVALID;
    if (!acov_out || !meanvar_out || !between_out || !cols || ncols < 1 || lag0 < 0 || nlag < 1)
        return fail(sr, MSX_ERR_INVALID, "msx_series_chain_acov: bad arguments (outputs, cols, lag0 >= 0, nlag >= 1)");
    if (n < 2 || n > sr->rows) return fail(sr, MSX_ERR_RANGE, "msx_series_chain_acov: n must lie in 2 .. the rows the series holds");
    if (lag0 + nlag > n) return fail(sr, MSX_ERR_RANGE, "msx_series_chain_acov: lags past the chains' length");
    if (ncols > MSX_MAX_DIM) return fail(sr, MSX_ERR_RANGE, "msx_series_chain_acov: more columns than a series is wide (MSX_MAX_DIM)");
    AcfDims dims = {};
    for (int32_t q = 0; q < ncols; ++q) {
        if (cols[q] >= (uint32_t)sr->ndim) return fail(sr, MSX_ERR_RANGE, "msx_series_chain_acov: a column outside the series");
        dims.d[dims.nd++] = (int32_t)cols[q];
    }
    HIP_TRY(sr, hipSetDevice(sr->device));
    const int k = (int)sr->off.size() - 1, nd = dims.nd;
    const int64_t np = n, nser = (int64_t)nd * sr->nw, nsuper = (np + kAcfSuper - 1) / kAcfSuper;
    const int64_t per_lag = nser * nsuper * (int64_t)sizeof(double);
    int64_t sub = std::max<int64_t>(1, (int64_t)kAcfPartBudget / per_lag / kAcfLagTile) * kAcfLagTile;
    sub = std::min(sub, nlag);
    const int64_t kd = (int64_t)k * nd;
    // scratch: [mean nser | part0 nser * nsuper | part nser * nsuper * sub | acov k * nd * sub | A(0) k * nd | between k * nd]
    HIP_TRY(sr, series_scratch(sr, sizeof(double) * (size_t)(nser + nser * nsuper + nser * nsuper * sub + kd * sub + 2 * kd)));
    double *d_mean = (double *)sr->d_scratch, *d_part0 = d_mean + nser, *d_part = d_part0 + nser * nsuper;
    double *d_f = d_part + nser * nsuper * sub, *d_a0 = d_f + kd * sub, *d_btw = d_a0 + kd;
    HIP_TRY(sr, series_wait_growth(sr));
    hipStream_t st = sr->stream;
    hipLaunchKernelGGL(acf_mean_kernel, dim3((unsigned)nser), dim3(kAcfMeanThreads), 0, st, (const double *)sr->d_rows, sr->cap, sr->nw, dims,
                       np, (int64_t)0, (int64_t)1, d_mean);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(acf_lag_kernel, dim3((unsigned)nser, 1u, (unsigned)nsuper), dim3(kAcfThreads), 0, st, (const double *)sr->d_rows,
                       sr->cap, sr->nw, dims, np, (int64_t)0, (int64_t)1, (const double *)d_mean, (int64_t)0, (int64_t)1, d_part0, nsuper,
                       (int64_t)1);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(acov_reduce_kernel, dim3((unsigned)((kd + 255) / 256)), dim3(256), 0, st, (const double *)d_part0, nsuper, (int64_t)1,
                       sr->nw, (int32_t)nd, (const int64_t *)sr->d_off, (int32_t)k, (int64_t)1, np, d_a0);
    HIP_TRY(sr, hipGetLastError());
    hipLaunchKernelGGL(acov_between_kernel, dim3((unsigned)((kd + 255) / 256)), dim3(256), 0, st, (const double *)d_mean, sr->nw, (int32_t)nd,
                       (const int64_t *)sr->d_off, (int32_t)k, d_btw);
    HIP_TRY(sr, hipGetLastError());
    std::vector<double> h((size_t)(kd * sub)), h2((size_t)(2 * kd));
    HIP_TRY(sr, hipMemcpyAsync(h2.data(), d_a0, sizeof(double) * (size_t)(2 * kd), hipMemcpyDeviceToHost, st));
    for (int64_t lb = lag0; lb < lag0 + nlag; lb += sub) {
        const int64_t cnt = std::min(sub, lag0 + nlag - lb), nout = kd * cnt;
        hipLaunchKernelGGL(acf_lag_kernel, dim3((unsigned)nser, (unsigned)((cnt + kAcfLagTile - 1) / kAcfLagTile), (unsigned)nsuper),
                           dim3(kAcfThreads), 0, st, (const double *)sr->d_rows, sr->cap, sr->nw, dims, np, (int64_t)0, (int64_t)1,
                           (const double *)d_mean, lb, cnt, d_part, nsuper, cnt);
        HIP_TRY(sr, hipGetLastError());
        hipLaunchKernelGGL(acov_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, (const double *)d_part, nsuper, cnt, sr->nw,
                           (int32_t)nd, (const int64_t *)sr->d_off, (int32_t)k, cnt, np, d_f);
        HIP_TRY(sr, hipGetLastError());
        HIP_TRY(sr, hipMemcpyAsync(h.data(), d_f, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, st));
        HIP_TRY(sr, hipStreamSynchronize(st));
        for (int64_t mq = 0; mq < kd; ++mq)
            memcpy(acov_out + mq * nlag + (lb - lag0), h.data() + mq * cnt, sizeof(double) * (size_t)cnt);
    }
    for (int64_t mq = 0; mq < kd; ++mq) {
        meanvar_out[mq] = h2[(size_t)mq] * (double)n / (double)(n - 1);
        between_out[mq] = h2[(size_t)(kd + mq)];
    }
    return MSX_OK;
}

int msx_test_hook(msx_ctx *c, int32_t what, int32_t value) {
    if (!c) return MSX_ERR_INVALID;
    if (what == MSX_HOOK_LINKED_FAULT) {
        if (!c->problem_staged) return fail(c, MSX_ERR_STATE, "msx_test_hook: no problem staged");
        c->P.linked_fault = value != 0;
        return MSX_OK;
    }
    if (what == MSX_HOOK_PAIR_LEASES) {
        if (!c->problem_staged || !c->d_pair_plan) return fail(c, MSX_ERR_STATE, "msx_test_hook: the staged problem has no pair form");
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipDeviceSynchronize());
        std::vector<int32_t> v((size_t)kPairSpillRows, value != 0 ? 1 : 0);
        HIP_TRY(c, hipMemcpy(c->d_pair_plan + kPairHdrInts, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
        return MSX_OK;
    }
    return fail(c, MSX_ERR_INVALID, "msx_test_hook: unknown hook");
}

#include "group_tempered_run.h"

}  // extern "C"
