/* msx.h -- C ABI of the MI355X (gfx950) implementation of mcmc_spec's per-walker log-likelihood path.
 *
 * The reference (kendallsullivan/mcmc_spec, mft6.py) is pure Python and exposes no FFI of its own
 * (SURVEY.md §8b); this header is therefore the boundary a maintainer would bind with ctypes (the
 * stub is shown in INTEGRATION.md).  Each entry point names the reference code it stands in for.
 *
 * Conventions
 *   - every call returns MSX_OK (0) or a negative MSX_ERR_* code; nothing throws across the ABI;
 *     msx_last_error(ctx) returns a human-readable message for the last failing call on that ctx.
 *   - the caller owns every host buffer; they are consumed before the call returns.
 *   - the ctx owns every device buffer.  One ctx per device; calls on one ctx must be serialised by
 *     the caller, different ctxs may be driven concurrently from different host threads.
 *   - all floating point data are IEEE float64, arrays are C-contiguous.
 *   - "*_dev" entry points take DEVICE pointers and a hipStream_t (as void*) and do not synchronise.
 */
#ifndef MSX_H
#define MSX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSX_OK 0
#define MSX_ERR_INVALID (-1) /* bad argument / inconsistent sizes                          */
#define MSX_ERR_HIP (-2)     /* a HIP runtime call failed (message has the hipError string) */
#define MSX_ERR_STATE (-3)   /* call order: grid or problem not staged yet                  */
#define MSX_ERR_RANGE (-4)   /* a value is outside the staged tables (Python: ValueError)   */

/* per-walker status written next to each log-probability (reference error conventions) */
#define MSX_W_OK 0
#define MSX_W_REJECT 1     /* prior box / non-finite -> log-prob = -inf        (mft6.py:1228,1230) */
#define MSX_W_KEYERROR 2   /* a needed grid node is not staged                 (mft6.py:489-500)   */
#define MSX_W_INDEXERROR 3 /* logg/Teff bracket runs past the last node        (mft6.py:453,477)   */
#define MSX_W_VALUEERROR 4 /* Teff outside the isochrone table                 (mft6.py:95)        */
#define MSX_W_HANDOVER 5   /* device fault, not a reference error: a linked launch's workgroups did not meet (MSX_PATH_LINKED) */

/* evaluation modes for msx_logprob_batch* (modes 4 and 5 are reached through msx_opt_step / msx_opt_init) */
#define MSX_MODE_LOGLIKE 0      /* loglikelihood   (mft6.py:1139-1205)                              */
#define MSX_MODE_LOGPOST 1      /* logposterior = logprior gate + loglikelihood (mft6.py:1459-1470) */
#define MSX_MODE_CHISQ 2        /* loglikelihood(optimize=True): returns total chi^2 (mft6.py:1198) */
#define MSX_MODE_LOGPRIOR 3     /* logprior alone (mft6.py:1207-1272); needs no spectrum pass       */
#define MSX_MODE_OPT_STEP 4     /* fit_spec proposal chi^2 (mft6.py:997-1028); via msx_opt_step      */
#define MSX_MODE_OPT_INIT 5     /* fit_spec initial guess (mft6.py:871-907); via msx_opt_init        */

#define MSX_MAX_SPEC 3
#define MSX_MAX_BANDS 8
#define MSX_MAX_DIM 8
#define MSX_MAX_GROUP 64        /* members of a target group (msx_group_create)                     */

typedef struct msx_ctx msx_ctx;
typedef struct msx_group msx_group;

/* Everything that is static per dataset.  Built on the host by mcmc_spec_amd/staging.py from the
 * reference's own arguments (data, err, fr, ctm, ptm, matrix, prior ...); copied at stage time. */
typedef struct msx_problem {
    int32_t struct_size; /* sizeof(msx_problem), ABI check */
    int32_t nspec;       /* 2 (binary, ndim 6) or 3 (triple, ndim 8)          mft6.py:1145,1153 */
    int64_t npix;        /* data pixels                                                          */
    /* A8 resample tables: for pixel p the model samples wl[lo], wl[lo+1] bracket the pixel and
     * t = (x - x_lo)/(x_hi - x_lo)                                              mft6.py:1169-1170 */
    const int64_t *pix_lo;
    const double *pix_t;
    const double *pix_u;    /* wavelength mapped to [-1,1] for the quadratic fit   mft6.py:195     */
    const double *pix_flux; /* data (already median-normalised by the caller)      mft6.py:3507    */
    const double *pix_err;  /* sigma per pixel                                     mft6.py:120     */
    double median_flux;     /* np.median(data)                                     mft6.py:1173    */
    double fit_minv[9];     /* inverse Gram matrix of [1,u,u^2] (row major)        mft6.py:195     */
    /* A5/A6 band integrals are linear in the node spectrum: out = sum_i w[i]*flux[node][i0+i]    */
    int32_t n_contrast;     /* contrast filters (first in the band list)           mft6.py:717     */
    int32_t n_phot;         /* photometric bands                                   mft6.py:771     */
    const int64_t *band_i0; /* [n_contrast+n_phot] first grid index of each band                   */
    const int64_t *band_len;
    const double *band_w;   /* concatenated weights                                                */
    const double *cmag, *cerr;       /* [n_contrast] observed contrasts            mft6.py:1182    */
    const double *pmag, *perr;       /* [n_phot] observed magnitudes               mft6.py:1188    */
    const double *phot_zero;         /* [n_phot] zero-point flux per band          mft6.py:780-782 */
    const double *phot_k;            /* [n_phot] CCM89 a+b/Rv at phot_cwl          mft6.py:1163    */
    int64_t win_j0, win_n;  /* make_composite's window into the grid wavelength    mft6.py:687,542 */
    /* A1 isochrone, sorted by Teff (stable)                                        mft6.py:87-98   */
    int32_t niso;
    const double *iso_teff, *iso_logg, *iso_lum;
    /* prior                                                         mft6.py:1207-1272 */
    int32_t nav;            /* A_V(distance) table bins; 0 = no A_V prior term                     */
    const double *av_edges_pc; /* [nav+1] */
    const double *av_mu, *av_sig; /* [nav] */
    double tmin, tmax;      /* Teff box                                             mft6.py:1227    */
    double prior_mean[MSX_MAX_DIM]; /* Gaussian priors; mean == 0 -> unused         mft6.py:1257-1260 */
    double prior_sig[MSX_MAX_DIM];
    int32_t use_av;         /* `a` / `av` flag                                      mft6.py:1161,1229 */
    int32_t dist_fit;       /* 1: the parallax is a fitted parameter with its box / Gaussian terms (mft6.py:1212-1272);
                             * 0: the `dist_fit=False` branch, radius-ratio scaling only (mft6.py:1275-1327)  */
    int32_t rad_prior;      /*                                                      mft6.py:1262    */
    int32_t has_prior_list; /* `prior != 0`                                         mft6.py:1241    */
    int32_t no_spectrum;    /* 1 = the mft6_nospec.py variant: total = contrast + photometry chi^2 only
                             * (mft6_nospec.py:1163-1196); the spectral phases are skipped            */
} msx_problem;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int msx_create(int device, msx_ctx **out);
void msx_destroy(msx_ctx *ctx);
const char *msx_last_error(msx_ctx *ctx);
/* device facts for reports: out[0]=CUs, out[1]=total global memory bytes, out[2]=clock kHz */
int msx_device_info(msx_ctx *ctx, int64_t *out3, char *name, int name_len);

/* ---- A0: the staged grid (replaces the `specs` dict, mft6.py:342-383 / consumed :481-500) ----- */
/* flux is [nt][ng][nwl]; present is [nt][ng] (0 = node absent -> KeyError when touched) or NULL.  */
int msx_stage_grid(msx_ctx *ctx, const double *wl, int64_t nwl, const double *teff_nodes, int32_t nt,
                   const double *logg_nodes, int32_t ng, const double *flux, const uint8_t *present);

/* ---- A7: CCM89 k(lambda) = a(x) + b(x)/R_V at arbitrary wavelengths [A] (extinction.ccm89 with
 * a_v = 1, mft6.py:62); the per-grid-sample table is built inside msx_stage_grid with R_V = 3.1.  */
int msx_ccm89_k(msx_ctx *ctx, const double *wl, int64_t n, double rv, double *out);

/* ---- f3: the resample step of the grid loader: interp1d(x, y)(xq), x sorted ascending, host buffers
 * (mft6.py:369-371).  MSX_ERR_RANGE when a query lies outside [x[0], x[n-1]] (scipy raises ValueError). */
int msx_resample_linear(msx_ctx *ctx, const double *x, const double *y, int64_t n, const double *xq, int64_t m,
                        double *out);

/* ---- A3: instrumental broadening (pyasl.instrBroadGaussFast + edge patches, mft6.py:124-152) -- */
/* one spectrum, host buffers; used by the drop-in `broaden()`                                     */
int msx_broaden(msx_ctx *ctx, const double *wl, const double *flux, int64_t n, double resolution,
                double maxsig, double *out);
/* every staged node, in place, over grid samples [i0, i0+n): the staging step mft6.py:366-378     */
int msx_broaden_grid(msx_ctx *ctx, int64_t i0, int64_t n, double resolution, double maxsig);
/* Rotational broadening (pyasl.rotBroad(wl, flux, limb, vsini), edgeHandling "firstlast"; mft6.py:133-134; DESIGN.md
 * "Rotational broadening"): v sin i [km/s] > 0, linear limb darkening 0 <= limb <= 1, both finite, else MSX_ERR_RANGE; an
 * ascending, evenly spaced axis (positive wavelengths).  msx_broaden then msx_rot_broaden is the reference's broaden(). */
/* one host spectrum: rotation only                                                                  */
int msx_rot_broaden(msx_ctx *ctx, const double *wl, const double *flux, int64_t n, double vsini, double limb,
                    double *out);
/* every staged node, in place, over grid samples [i0, i0+n) (the same window as msx_broaden_grid, after it).  Like
 * msx_broaden_grid it drops the staged problem; it also releases the raw window kept for MSX_PATH_INPATH (that form
 * applies the Gaussian only): problems staged afterwards refuse the in-path form until the next msx_broaden_grid. */
int msx_rot_broaden_grid(msx_ctx *ctx, int64_t i0, int64_t n, double vsini, double limb);
/* ---- Component grids (DESIGN.md "Component grids"): one v sin i / limb per star.  A component grid holds ncomp copies of
 * every node row, copy s at rows [s nt ng, (s+1) nt ng); component s of every walker reads copy s.  1 <= ncomp <=
 * MSX_MAX_SPEC, else MSX_ERR_RANGE; an ordinary grid is ncomp = 1.  msx_broaden_grid / msx_rot_broaden_grid act on every
 * copy.  Problems staged on a component grid need nspec == ncomp (MSX_ERR_RANGE) and refuse MSX_PATH_INPATH.            */
/* duplicate the staged rows into ncomp contiguous copies (device to device; drops the staged problem)                   */
int msx_split_components(msx_ctx *ctx, int32_t ncomp);
/* msx_stage_grid with flux [ncomp][nt][ng][nwl] (present [nt][ng] is shared by the copies)                               */
int msx_stage_grid_components(msx_ctx *ctx, const double *wl, int64_t nwl, const double *teff_nodes, int32_t nt,
                              const double *logg_nodes, int32_t ng, const double *flux, const uint8_t *present,
                              int32_t ncomp);
/* msx_rot_broaden_grid on copy comp only (the same checks and errors)                                                   */
int msx_rot_broaden_grid_component(msx_ctx *ctx, int32_t comp, int64_t i0, int64_t n, double vsini, double limb);
/* msx_read_node of copy comp                                                                                            */
int msx_read_node_component(msx_ctx *ctx, int32_t comp, int32_t it, int32_t ig, double *out);
/* Where the broadening is PLACED: MSX_BROADEN_STAGING (default) -- once per grid node, by msx_broaden_grid: the
 * reference's live path; MSX_BROADEN_IN_PATH -- msx_broaden_grid additionally keeps the window's rows as they were, and
 * the problems staged afterwards get the per-walker form MSX_PATH_INPATH (below) beside all the others.  Takes effect at the
 * next msx_broaden_grid. */
#define MSX_BROADEN_STAGING 0
#define MSX_BROADEN_IN_PATH 1
int msx_set_broadening(msx_ctx *ctx, int32_t placement);
/* copy one staged node back to the host (tests / the drop-in `specs` view)                        */
int msx_read_node(msx_ctx *ctx, int32_t it, int32_t ig, double *out_nwl);

/* ---- problem staging -------------------------------------------------------------------------- */
int msx_stage_problem(msx_ctx *ctx, const msx_problem *p);

/* ---- the hot path: log-probability of a whole ensemble in one launch -------------------------- */
/* theta is [n][ndim] row-major (ndim = 2*nspec+2); logp_out [n]; status_out [n] (MSX_W_*).        */
int msx_logprob_batch(msx_ctx *ctx, int32_t mode, const double *theta, int64_t n, int32_t ndim,
                      double *logp_out, int32_t *status_out);
/* same with device pointers on a caller stream; does not synchronise (no launch allocates: every scratch buffer is
 * sized by msx_stage_problem).  block_threads: 0 = auto (up to #CUs walkers, spectra of >= 8192 pixels, triples: 512
 * threads, one workgroup per CU; binaries below 8192 pixels between #CUs and 2 x #CUs walkers: 512 threads in the
 * <= 128-VGPR variant, two of which fit a CU; beyond, and from #CUs walkers on for spectra of <= 2048 pixels: 256
 * threads, three per CU), or 256 / 512, or MSX_BLOCK_512_SHARED = 512 threads in the <= 128-VGPR variant whatever
 * the batch size (what a launch wants when another kernel, e.g. a collective, holds CUs at the same time).  The
 * choice affects speed only: every variant produces the same bits.                                               */
#define MSX_BLOCK_512_SHARED 1512
int msx_logprob_batch_dev(msx_ctx *ctx, int32_t mode, const double *d_theta, int64_t n, int32_t ndim,
                          double *d_logp, int32_t *d_status, void *hip_stream, int32_t block_threads);

/* Three forms of the same path, same bits.
 * FUSED: one launch, one workgroup per walker.
 * PAIR: for large batches of a binary with <= 4096 pixels: a planner kernel (one thread per walker: the recipe, the
 * prior and band terms, who shares a grid cell with whom) and a kernel that evaluates TWO walkers of one grid cell
 * per workgroup from one set of loads, model values in registers (16,384 walkers 316 us against 419 fused).
 * MSX_PATH_AUTO takes it from 8 walkers per CU on (2,048; spectra of <= 3,072 pixels: 12 per CU; MSX_PAIR_MIN in the
 * environment) while the planner's last count says the ensemble pairs (msx_pair_stats); DESIGN.md section 5.1.
 * LINKED: for few walkers x long spectra (2..8 segments of 8192 pixels), one workgroup per (walker, segment) in ONE
 * launch, so that e.g. 128 walkers x 16,384 pixels use 256 CUs instead of 128 and each workgroup's chain of latencies
 * is 8192 pixels long.  A walker's workgroups are equals: each blends its segment, they exchange the segments' fit
 * sums / value ranges / histogram counters inside the kernel (a bounded wait: 20 ms), each makes the chi^2 / median-
 * candidates pass over its own segment, and whichever finishes last ranks the candidates and completes the walker.
 * MSX_PATH_AUTO takes it while walkers x segments <= #CUs (MSX_LINKED=0 in the environment: never; =1: whenever the
 * spectrum has 2..8 segments): 128 walkers x 16,384 px 27.2 us against 31.9 fused, 8..64 walkers 23.5..24.5 us
 * (DESIGN.md); also under the device-resident sampler.
 * A meeting that times out fails its walker with MSX_W_HANDOVER and POISONS the context's linked form: a device-side
 * word makes every later linked launch fail ALL its walkers with MSX_W_HANDOVER (never a value computed from stale
 * counters), MSX_PATH_AUTO takes the fused form once a synchronous entry point has seen the status, an explicit
 * MSX_PATH_LINKED is refused with MSX_ERR_STATE -- until msx_stage_problem clears counters and word together.
 * (Values 2 and 3 were the split and wide forms of rounds 1-2: measured slower than FUSED at every size and removed;
 * the measurements are kept in DESIGN.md.)                                                                        */
#define MSX_PATH_AUTO 0
#define MSX_PATH_FUSED 1
#define MSX_PATH_PAIR 2
#define MSX_PATH_LINKED 4
/* In-path broadening (SURVEY A3 placement (ii); mft6.py:124-152 applied per evaluation, the call the reference keeps
 * commented out at :550): the instrumental broadening is applied PER WALKER to the unreddened composite inside the data
 * window -- composite of the raw window rows with the recipe's weights, Gaussian FIR, the two edge patches, then reddening
 * and the resample to the data pixels -- instead of once per grid node at staging.  Broadening is linear: the values agree
 * with every other form to the order of the sums (~1e-13 relative), not bit for bit.  Never taken by MSX_PATH_AUTO (the
 * per-node placement is the reference's live path); needs msx_set_broadening(MSX_BROADEN_IN_PATH) BEFORE
 * msx_broaden_grid, a binary whose data pixels all lie inside that window, float64 tables, a likelihood / posterior /
 * chi^2 mode.  Costs a walker eight raw rows of the window and a convolution where the table form reads resampled pixels:
 * several times the headline path's time. */
#define MSX_PATH_INPATH 8
int msx_set_path(msx_ctx *ctx, int32_t path);

/* ---- f4: the pre-optimiser's chi^2 (fit_spec, mft6.py:856-1137) on the same kernel --------------- */
/* msx_opt_init: one chain per row of theta0 [nchains][ndim].  Normalises the data against each chain's
 * initial (un-reddened) model like mft6.py:884-889, keeps the normalised vector and its median on the
 * device, and returns the initial likelihood chi^2 = 3*iic*(n_c+n_p) + contrast + phot (mft6.py:893-904;
 * the opt_prior terms of :910-929 are added by the host driver).                                        */
int msx_opt_init(msx_ctx *ctx, const double *theta0, int64_t nchains, int32_t ndim, double *chi2_out,
                 int32_t *status_out);
/* msx_opt_step: proposal i belongs to chain[i]; returns the chi^2 of mft6.py:1011-1028 (no per-proposal
 * continuum fit, spectrum weight 3) against that chain's stored data vector.                            */
int msx_opt_step(msx_ctx *ctx, const double *theta, const int32_t *chain, int64_t n, int32_t ndim,
                 double *chi2_out, int32_t *status_out);

/* ---- f4 on the device: fit_spec's random-walk descent with the chains' state in HBM ----------
 * After msx_opt_init, one chain per row of its theta0.  A TRIP is ONE draw of every chain (the body of fit_spec's while
 * loop, mft6.py:935-1103): step sizes from the chain's phase, proposal gi + si * z (rounded multiply, rounded add), the
 * bounds test; out of bounds -> the seven repair loops advance total_n and nothing is evaluated; in bounds -> the
 * proposal's chi^2 in MSX_MODE_OPT_STEP against the chain's stored data vector, the opt_prior terms (A_V against the
 * table's bin of 1 / plx; the parallax if dist_fit; the radii against the isochrone's if rad_prior, sigma = the radius
 * step sizes) and the accept rule test < chi.  A chain is finished when n >= steps or total_n >= 50 * steps.
 * begin: gi0 [nchains][ndim] the start points (rows [T.., A_V, rad.., plx]: msx_opt_init's theta0), chi0 [nchains] their
 * chi^2 INCLUDING the prior terms (the host adds them as fit_spec does, mft6.py:909-929); tmin / tmax the Teff box;
 * av_edges [nedges] ascending, av_mu / av_sig [nav] the A_V(distance) table of THIS run (bin = #{edges <= 1 / plx} - 1,
 * clipped to [0, nav - 1]; sigma 0 reads 0.05); iso_teff / iso_lum [niso] the isochrone sorted by Teff (read only with
 * rad_prior).  Argument errors are reported before any device work.  A run still open ends; so does msx_opt_init,
 * restaging the problem or destroying the ctx.                                                                        */
#define MSX_OPT_TRIP_IDLE 0      /* the chain was finished before this trip                                  */
#define MSX_OPT_TRIP_OOB 1       /* the draw was out of bounds: repair loops counted, nothing evaluated      */
#define MSX_OPT_TRIP_REJECTED 2  /* evaluated, test >= chi                                                   */
#define MSX_OPT_TRIP_ACCEPTED 3  /* evaluated, test < chi: the record's gi is the proposal                   */
#define MSX_OPT_TRIP_ERROR 4     /* evaluated with a walker error: flag = 4 | MSX_W_* << 8, the record's gi slot names
                                  * the PROPOSAL, its test is NaN, and the chain stops                              */
int msx_opt_run_begin(msx_ctx *ctx, int64_t nchains, int32_t ndim, const double *gi0, const double *chi0, int64_t steps,
                      double tmin, double tmax, int32_t dist_fit, int32_t rad_prior, double plx_prior, double plx_sigma,
                      int32_t nedges, const double *av_edges, int32_t nav, const double *av_mu, const double *av_sig,
                      int32_t niso, const double *iso_teff, const double *iso_lum, int64_t max_chunk_trips);
/* one chunk of ntrips <= max_chunk_trips trips into slot 0|1 without waiting for it: z [ntrips][nchains][ndim] standard
 * normals (chain c's k-th draw of the run is its slice of the run's k-th trip), uploaded on a stream of its own;
 * 2 * ntrips + 1 launches on the compute stream and no host round trip between them.                                   */
int msx_opt_run_enqueue(msx_ctx *ctx, int32_t slot, int64_t ntrips, const double *z);
/* waits for the chunk in `slot`: records [ntrips][nchains][ndim + 2] = {gi[ndim], chi, test} of every chain AFTER each
 * trip (test: NaN unless evaluated), flags [ntrips][nchains] MSX_OPT_TRIP_*, *live = chains that would draw again after
 * the chunk (0: the run is over), *worst_status = the worst walker status above MSX_W_REJECT of the chunk's evaluations. */
int msx_opt_run_collect(msx_ctx *ctx, int32_t slot, double *records, int32_t *flags, int64_t *live, int32_t *worst_status);
/* ends the run (waits for it); any of gi [nchains][ndim], chi, n [nchains] (a double: steps / 2 + 1 is fractional for
 * odd steps), total_n [nchains] may be NULL.                                                                           */
int msx_opt_run_end(msx_ctx *ctx, double *gi, double *chi, double *n, int64_t *total_n);

/* ---- f2 on the device: nsteps iterations of the affine-invariant stretch move (Goodman & Weare 2010, the
 * default move of emcee 3; the loop the reference drives at mft6.py:1494-1524) with the walker state resident in
 * HBM.  Per half-step there is ONE launch of the fused log-probability kernel: its first lines build each active
 * walker's proposal q = c - (c - s) z from the resident coordinates, its last lines apply the accept rule and write
 * the walker's row of the chain -- no separate proposal / accept kernels and no host round trip.  The host supplies
 * the randomness of every half-step h = 2*step + half, each an array of nw/2 entries: the active walkers sidx, the
 * complementary half cidx, partner (index into cidx), z = ((a-1)u+1)^2/a, zfac = (ndim-1) ln z and logu = ln(u')
 * for the accept test logu < zfac + lp(q) - lp(s).
 * coords/logp are updated in place; chain_out [nsteps][nw][ndim] and logp_out [nsteps][nw] hold the state after
 * every step; naccept[nw] accumulates; worst_status returns the largest MSX_W_* error seen (0 = none).        */
int msx_sampler_run(msx_ctx *ctx, int32_t mode, int64_t nw, int32_t ndim, int64_t nsteps, double *coords, double *logp,
                    const int32_t *sidx, const int32_t *cidx, const int32_t *partner, const double *zz,
                    const double *zfac, const double *logu, double *chain_out, double *logp_out, int64_t *naccept,
                    int32_t *worst_status);

/* The same loop, pipelined (what mcmc_spec_amd.sampler.DeviceEnsembleSampler drives): begin uploads the ensemble
 * state and sets up two slots; enqueue(slot) stages one chunk of randomness (arrays of nsteps*2*(nw/2) entries, laid
 * out as for msx_sampler_run; indices are range-checked on the host) and queues its 2*nsteps fused launches WITHOUT
 * waiting -- uploads, launches and chain downloads run on three HIP streams; collect(slot) waits for that chunk only
 * and returns its chain rows, the cumulative acceptance counts as of its last step and its worst status.  Enqueue
 * chunk i+1 before collecting chunk i and the GPU never idles between chunks.  end() optionally returns the final
 * state (coords/logp may be NULL) and frees everything; restaging the problem or destroying the ctx ends a run too. */
int msx_sampler_begin(msx_ctx *ctx, int32_t mode, int64_t nw, int32_t ndim, int64_t max_chunk_steps, const double *coords,
                      const double *logp, const int64_t *naccept /* NULL = zeros */);
/* Sharded form of the same run: call once between msx_sampler_begin and the first enqueue, on every
 * rank, after msx_comm_init(rank, world).  Every rank holds the whole ensemble in HBM and must be fed the same
 * randomness; per half-step rank r evaluates block r of the nw/2 proposals (ceil((nw/2)/world) walkers), ONE RCCL
 * all-gather of that many float64 log-probabilities per rank crosses xGMI on the compute stream, and a small kernel
 * applies the accept rule for all walkers on every rank -- so every rank's chain is bit-identical to the one-GPU
 * chain and nothing returns to the host between half-steps.  world = 1 is allowed (no collective): the same three
 * device steps on one GPU.  A walker error (MSX_W_*) on any rank reaches every rank's worst_status: it travels as
 * the payload of the NaN log-probability it produces.                                                            */
int msx_sampler_shard(msx_ctx *ctx, int32_t rank, int32_t world);
int msx_sampler_enqueue(msx_ctx *ctx, int32_t slot /* 0|1 */, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                        const int32_t *partner, const double *zz, const double *zfac, const double *logu);
/* The chunk's randomness drawn ON THE DEVICE instead of coming from the host: a counter-based generator (SplitMix64's
 * output function over counters made of (seed, absolute iteration of the stream, stream, index)) yields, per iteration, the
 * random split of the ensemble into two halves (walkers sorted by a 64-bit key) and, per half-step and walker, the stretch
 * factor z = ((a - 1) u + 1)^2 / a, the partner floor(u ns) in the complementary half and ln u of the accept draw -- the
 * quantities msx_sampler_enqueue takes from the host (emcee's stretch move; mft6.py:1491-1494 drives it).  One launch per
 * chunk, no upload; every rank of a sharded run draws the same numbers from the same seed.  Up to 4096 walkers.
 * msx_sampler_draw returns the same stream to the host (arrays [nsteps][2][nw/2] as for msx_sampler_enqueue; `partner`
 * indexes the complementary half): the host loop fed with it reproduces the device-drawn chain bit for bit
 * (tests/test_gpu_overlap.py), and mcmc_spec_amd/sampler.py::counter_draws restates the generator in NumPy.
 * first_iter is the ABSOLUTE iteration of the chunk's first step in the seed's stream, as msx_sampler_draw takes it: the
 * caller carries it from chunk to chunk and ACROSS runs (a run begun after burn-in goes on where the burn-in's last queued
 * chunk stopped; the run's own count of steps starts at 0 again and plays no part in the stream -- it numbers only the
 * hand-over versions of an overlapped run).  a not > 1, first_iter < 0 or more than 4096 walkers: MSX_ERR_INVALID, and
 * nothing is queued (tests/test_gpu_sampler_runs.py).                                                                  */
int msx_sampler_enqueue_drawn(msx_ctx *ctx, int32_t slot, int64_t nsteps, uint64_t seed, double a, int64_t first_iter);
int msx_sampler_draw(msx_ctx *ctx, uint64_t seed, double a, int64_t first_iter, int64_t nsteps, int64_t nw, int32_t ndim,
                     int32_t *sidx, int32_t *cidx, int32_t *partner, double *zz, double *zfac, double *logu);
int msx_sampler_collect(msx_ctx *ctx, int32_t slot, double *chain_out, double *logp_out, int64_t *naccept,
                        int32_t *worst_status);
int msx_sampler_end(msx_ctx *ctx, double *coords, double *logp);
/* OVERLAPPED half-steps (one GPU, unsharded, a half-step of at most #CUs / 2 walkers through the fused kernel with one
 * workgroup per CU -- config 2's 256 walkers): consecutive half-steps go to two streams and run concurrently; a walker's
 * workgroup waits inside the kernel (bounded: 20 ms, then the chunk's worst_status is MSX_W_HANDOVER) until the two
 * walkers its move reads have reached the versions the move is defined on; what a move reads of a walker is handed over
 * as 8-byte words {32 bits of payload | version}, each written by one agent-scope store and double-buffered by version
 * parity, so the load that sees the version has the data -- a half-step's launch, start-up and slowest walker no longer
 * sit between two dependent evaluations (256 walkers x 4096 px: 28 us per iteration; 31.3 with a version word behind the
 * data, 38.0 with plain launches).
 * Same chain, bit for bit.  Chosen by the first msx_sampler_enqueue of a run; MSX_SMP_OVERLAP=0 in the environment:
 * never.  *out = 1 if the run begun on ctx takes it, 0 if not, -1 before its first chunk.                           */
int msx_sampler_overlapped(msx_ctx *ctx, int32_t *out);
/* ... and the caller's say: overlap = -1 (default) lets the rule above decide, 0 never overlaps (plain launches, one
 * half-step after the other).  The rule counts on this context's launches having the device to themselves -- two
 * half-steps of 128 walkers need all 256 CUs at once -- and never takes the overlap on a context that holds a
 * communicator.  On a device shared with other work use 0: a waiting workgroup whose producer cannot get a CU ends, after
 * the 20 ms bound, as MSX_W_HANDOVER for the chunk, and the run has to be started again (the chain up to the last
 * collected chunk stands).  Takes effect at the next msx_sampler_begin.                                                */
int msx_sampler_policy(msx_ctx *ctx, int32_t overlap);

/* ---- moves other than the stretch move, and mixtures of moves (emcee 3's `moves=`) ---------------
 * An iteration is split into two halves as above; each ITERATION takes one move of a set, for both of its half-steps,
 * chosen with the set's normalised weights.  For entry j of a half-step, s the moving walker and C its complementary half
 * (nc walkers):
 *   MSX_MOVE_STRETCH (a)            c = C[p1], z = ((a - 1) u + 1)^2 / a, q = c - (c - s) z, factor (ndim - 1) ln z
 *   MSX_MOVE_DE (sigma, gamma0)     differential evolution (ter Braak 2006, as emcee 3's DEMove): an ordered pair of
 *                                   DISTINCT walkers C[p1], C[p2], uniform over the nc (nc - 1) pairs; g = g0 (1 + sigma n),
 *                                   n standard normal, g0 = gamma0, or 2.38 / sqrt(2 ndim) for gamma0 <= 0;
 *                                   q = s + g (C[p1] - C[p2]), factor 0 (gamma0 = 1: the mode-jumping variant)
 * and every move accepts when ln u < (factor + ln p(q)) - ln p(s) (a NaN difference compares false).
 * These chunks run BESIDE the fused kernel, whose proposal is the stretch move's: per half-step the plain evaluation
 * (msx_logprob_batch_dev / msx_group_logprob_batch_dev) scores proposals that a small kernel wrote, and the same small
 * kernel -- one workgroup per member, one launch -- applies the accept rule to them and proposes the next half-step.
 * Plain launches: the first msx_*_enqueue_moves* call of a run fixes overlap = 0 (a run whose stretch chunks already
 * overlap, and a sharded run, are refused with MSX_ERR_STATE).  begin, collect, end and attach_series are the calls above,
 * and chunks of either family may alternate within a run: both leave the same resident state.                        */
#define MSX_MOVE_STRETCH 0
#define MSX_MOVE_DE 1
#define MSX_MAX_MOVES 4
typedef struct {
    int32_t n;               /* moves in the set, 1..MSX_MAX_MOVES                               */
    int32_t kind[4];         /* MSX_MOVE_*                                                       */
    double weight[4];        /* normalised: > 0, summing to 1 within 1e-12                       */
    double a[4];             /* stretch scale (> 1) of a MSX_MOVE_STRETCH entry                  */
    double gamma0[4];        /* DE: g0; <= 0: 2.38 / sqrt(2 ndim)                                */
    double sigma[4];         /* DE: relative scatter of g (>= 0)                                 */
} msx_move_set;
/* host-drawn chunk in the GENERAL layout: sidx, cidx, p1, p2 (indices into the complementary half), g, fac, logu are
 * [nsteps][2][nw/2]; kind [nsteps] (one move per iteration).  Stretch entries carry p1 = p2 = partner, g = z, fac =
 * (ndim - 1) ln z; DE entries fac = 0.  Checked (MSX_ERR_INVALID, nothing queued): indices in range, kind a MSX_MOVE_*,
 * p1 != p2 on DE entries.                                                                                             */
int msx_sampler_enqueue_moves(msx_ctx *ctx, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                              const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                              const double *logu);
/* the same chunk DRAWN ON THE DEVICE by msx_sampler_enqueue_drawn's counter generator: the split (stream 0) and u_z, u_p,
 * u_a (streams 1..6) are the ones the stretch-only generator gives the same seed; stream 7, index 0 chooses the
 * iteration's move (the first i with u < weight[0] + .. + weight[i]); per half-step h, stream 8 + 3h index j is the DE
 * pair (p = min(floor(u nc (nc - 1)), nc (nc - 1) - 1), j1 = p / (nc - 1), r = p % (nc - 1), j2 = r + (r >= j1)) and
 * streams 9 + 3h, 10 + 3h the normal deviate n = sqrt(-2 ln(1 - u1)) cos(2 pi u2).  The set travels by value: one launch
 * per chunk, nothing uploaded.  first_iter as for msx_sampler_enqueue_drawn.  A bad set (n, a kind, a weight, weights
 * that do not sum to 1, a <= 1, sigma < 0), more than 4096 walkers, fewer than 4 with a DE move: MSX_ERR_INVALID.      */
int msx_sampler_enqueue_moves_drawn(msx_ctx *ctx, int32_t slot, int64_t nsteps, uint64_t seed, const msx_move_set *set,
                                    int64_t first_iter);
/* that stream on the host, in the general layout (p1, p2 index the complementary half): the host loop fed with it walks
 * the device-drawn chain bit for bit; mcmc_spec_amd/moves.py::counter_draws_moves restates it in NumPy                  */
int msx_sampler_draw_moves(msx_ctx *ctx, uint64_t seed, const msx_move_set *set, int64_t first_iter, int64_t nsteps,
                           int64_t nw, int32_t ndim, int32_t *sidx, int32_t *cidx, int32_t *kind, int32_t *p1, int32_t *p2,
                           double *g, double *fac, double *logu);

/* ---- parallel tempering: a temperature ladder on the device-resident sampler -------------------
 * ntemps ensembles ("rungs") of nw walkers on this context's staged problem; rung t samples
 *   P_t(x) = lpr(x) + beta_t * ll(x),   lpr = MSX_MODE_LOGPRIOR, ll = MSX_MODE_LOGLIKE,   1 = beta_0 > beta_1 > ... > 0
 * (any strictly descending positive ladder is taken), evaluated in two roundings: prod = beta_t * ll; P = lpr + prod.
 * Iteration i, for every rung independently, is one iteration of the general layout above for a member of nw walkers (the
 * split, the iteration's move, proposals, fac, ln u unchanged) with the accept rule ln u < (fac + P_t(q)) - P_t(s), P_t(s)
 * from the stored lpr and ll.  A proposal whose prior status is MSX_W_REJECT is rejected and its likelihood status ignored;
 * an error status of the prior, or of the likelihood on a proposal the prior admits, counts toward the rung's worst status.
 * After the second half-step THE SWAP SWEEP runs, for t = ntemps-1 down to 1 and every walker index w independently:
 * walker w of rung t and walker w of rung t-1 exchange coordinates, ll and lpr when
 *   ln u < (beta[t-1] - beta[t]) * (ll[t][w] - ll[t-1][w])      (the difference of the betas formed once, in float64;
 * a NaN compares false).  Serial in t: a walker can travel several rungs in one iteration.  The chain rows of iteration i
 * are the state after the sweep.  Beside the fused kernel, as the moves above: per half-step one small launch (one
 * workgroup per rung) and TWO plain evaluations of the ntemps * nw / 2 proposals, per iteration one launch for the sweep.
 * One GPU, plain launches: begin is refused (MSX_ERR_STATE) without a staged problem, with a run (msx_sampler_* or
 * msx_tempered_*) in flight, on a context that holds a communicator, and unless msx_sampler_policy(ctx, 0) was set.
 * MSX_ERR_INVALID: ntemps outside 1..MSX_MAX_GROUP, betas not finite, not > 0 or not strictly descending, nw odd or < 2, an
 * initial walker whose lpr is not finite or whose ll is NaN.  While a tempered run is in flight msx_sampler_begin is refused
 * (MSX_ERR_STATE; so is everything that needs its run, msx_sampler_attach_series included: no device series here).
 * coords [ntemps][nw][ndim], ll, lpr [ntemps][nw].  Memory: the state and two slots sized for max_chunk_steps.          */
int msx_tempered_begin(msx_ctx *ctx, int32_t ntemps, const double *betas, int64_t nw, int32_t ndim, int64_t max_chunk_steps,
                       const double *coords, const double *ll, const double *lpr);
/* host-drawn chunk: the ntemps members' general layouts -- sidx, cidx, p1, p2, g, fac, logu [nsteps][ntemps][2][nw/2], kind
 * [nsteps][ntemps], indices rung-local -- and swap_logu [nsteps][ntemps-1][nw], row p of an iteration for the pair of rungs
 * (p + 1, p) (NULL for one rung).  Checked as msx_sampler_enqueue_moves checks (MSX_ERR_INVALID, nothing queued).        */
int msx_tempered_enqueue(msx_ctx *ctx, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                         const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                         const double *logu, const double *swap_logu);
/* the same chunk DRAWN ON THE DEVICE: rung t is msx_sampler_enqueue_moves_drawn's stream of seeds[t] (streams 0..13), and
 * the swap draws are u = uniform(seeds[0], iteration, stream 14, index (t - 1) * 4096 + w) for the pair (t, t - 1).  A bad
 * set, more than 4096 walkers per rung, fewer than 4 with a DE move, first_iter < 0: MSX_ERR_INVALID, nothing queued.
 * Chunks of either family may alternate within a run.                                                                   */
int msx_tempered_enqueue_drawn(msx_ctx *ctx, int32_t slot, int64_t nsteps, const uint64_t *seeds, const msx_move_set *set,
                               int64_t first_iter);
/* that stream on the host, in msx_tempered_enqueue's layout (p1, p2 index the complementary half); needs no run           */
int msx_tempered_draw(msx_ctx *ctx, int32_t ntemps, const uint64_t *seeds, const msx_move_set *set, int64_t first_iter,
                      int64_t nsteps, int64_t nw, int32_t ndim, int32_t *sidx, int32_t *cidx, int32_t *kind, int32_t *p1,
                      int32_t *p2, double *g, double *fac, double *logu, double *swap_logu);
/* waits for the slot: chain [nsteps][ntemps][nw][ndim], ll_chain, lpr_chain [nsteps][ntemps][nw]; naccept [ntemps][nw] and
 * nswap [ntemps-1] (swaps accepted per pair) count since begin -- integers, exact whatever the launch; worst [ntemps]   */
int msx_tempered_collect(msx_ctx *ctx, int32_t slot, double *chain, double *ll_chain, double *lpr_chain, int64_t *naccept,
                         int64_t *nswap, int32_t *worst);
/* ends the run (no run: MSX_OK); its final state where the pointers are not NULL                                        */
int msx_tempered_end(msx_ctx *ctx, double *coords, double *ll, double *lpr);
/* (the ladder's device series: msx_series_attach_tempered, with the series below)                                       */

/* ---- adaptive ladders (mcmc_spec_amd.tempered.ladder_step is the definition) --------------------
 * msx_ladder_adapt, once between msx_tempered_begin and the run's first enqueue, makes the run adaptive from k0, the
 * adaptive iterations done before it: the ladder lives in device memory, every iteration's moves and sweep read it there
 * (db = beta[t-1] - beta[t] formed from it), and after each sweep a one-workgroup launch applies one ladder step with the
 * swaps that iteration accepted:  r = counts / nw;  kappa = (lag / (k + lag)) / time;  Ti = 1 / beta;  the gap
 * g[p] = Ti[p] - Ti[p-1] of each free rung p = 1..T-2 is scaled by ladder_exp(kappa * (r[p-1] - r[p])), the hottest gap kept;
 * c = the running sum of g in index order;  beta'[p] = 1 / (Ti[0] + (Ti[T-1] - Ti[0]) * (c[p] / c[T-1])).  Both ends stay;
 * ntemps <= 2 moves nothing; a result that is not finite or not strictly descending is dropped and counted as skipped.
 * float64 + - * / without contraction; ladder_exp is the degree-12 Taylor polynomial in x / 8 squared three times, never a
 * library's exp: the host definition, msx_ladder_step and the kernel give the same bits.  Everything else about the run is
 * msx_tempered_*'s above, unchanged.  MSX_ERR_STATE: no run, after the first enqueue, twice.  MSX_ERR_INVALID: lag not
 * finite or <= 0, time not finite or < 1 (the bound keeps |kappa (r - r')| <= 1), k0 < 0.                                */
int msx_ladder_adapt(msx_ctx *ctx, double lag, double time, int64_t k0);
/* the ladders [nsteps][ntemps] that the iterations of the chunk LAST COLLECTED from `slot` ran with, until the slot is
 * enqueued again (MSX_ERR_STATE before a collect and while a chunk is in the slot).  A fixed run: the begin ladder in every
 * row.                                                                                                                   */
int msx_ladder_betas(msx_ctx *ctx, int32_t slot, double *out);
/* the run's current ladder [ntemps], behind everything queued: waits for the compute stream.  k: adaptive iterations done
 * (k0 + those queued); skipped: ladder steps skipped in this run; either may be NULL.  A fixed run: the begin ladder, 0, 0. */
int msx_ladder_current(msx_ctx *ctx, double *betas, int64_t *k, int64_t *skipped);
/* one ladder step ON THE HOST, through the inline functions the kernel calls: needs no context and no GPU.  counts
 * [ntemps-1]: the iteration's swaps, pair p = rungs (p + 1, p); betas_out [ntemps]; *skipped 0 or 1 (may be NULL).
 * MSX_ERR_INVALID: ntemps outside 1..MSX_MAX_GROUP, nw < 1, k < 0, lag / time as above.  betas is taken as strictly
 * descending and > 0.                                                                                                    */
int msx_ladder_step(int32_t ntemps, const double *betas, const int64_t *counts, int64_t nw, int64_t k, double lag, double time,
                    double *betas_out, int32_t *skipped);

/* ---- A4-A6: make_composite (mft6.py:651-831, plot=False) -------------------------------------- */
/* teff/logg/rad are [nspec]; use_distance = 0 mirrors `distance=False` (mft6.py:701-703).         */
/* spec_out [win_n], contrast_out [n_contrast], phot_out [n_phot] (unreddened magnitudes).         */
int msx_make_composite(msx_ctx *ctx, const double *teff, const double *logg, const double *rad,
                       int32_t use_distance, double plx, double *spec_out, double *contrast_out,
                       double *phot_out, int32_t *status_out);

/* ---- the one collective of the sharded path -- an RCCL all-gather of `count` float64 log-probs per
 * rank.  The reference has no counterpart (its parallelism is multiprocessing.Pool, mft6.py:1744).  RCCL is
 * resolved at run time from the librccl.so.1 already mapped in the process (PyTorch-ROCm's).  The id comes
 * from rank 0 (msx_comm_unique_id) and reaches the other ranks by any side channel (bench.py: a
 * torch.distributed broadcast).  msx_comm_allgather_dev runs the collective on the ctx's communication stream
 * after everything queued on `compute_stream`, then signals event `slot` (0..3); msx_comm_wait_slot makes
 * `compute_stream` wait for that event before a buffer is reused -- so step i's all-gather overlaps step i+1. */
int msx_comm_unique_id(msx_ctx *ctx, uint8_t *out128);
int msx_comm_init(msx_ctx *ctx, const uint8_t *id128, int32_t rank, int32_t world);
int msx_comm_allgather_dev(msx_ctx *ctx, const double *d_send, double *d_recv, int64_t count, void *compute_stream,
                           int32_t slot);
int msx_comm_wait_slot(msx_ctx *ctx, int32_t slot, void *compute_stream);

/* ---- the "fake collective" -- a LOOPBACK group.  `world` contexts of ONE process on ONE device stand
 * for ranks 0..world-1 (ctxs[r] becomes rank r); the sharded sampler's all-gather becomes device copies between the
 * ranks' gathered vectors (rank r takes block p out of rank p's vector, in place at p * ceil(ns / world), exactly
 * where RCCL's in-place all-gather puts it).  Every rank-dependent line of the sharded path -- block offsets, ragged
 * and empty shards, the NaN-payload status, the apply kernel over the gathered vector -- then runs on a one-GPU box,
 * no RCCL involved.  After msx_sampler_begin + msx_sampler_shard(r, world) on every rank, msx_sampler_enqueue_group
 * queues one chunk on all ranks in lock-step (same randomness for all, as the sharded form requires) in place of the
 * per-rank msx_sampler_enqueue; collect / end stay per rank.  The group ends when its first member is destroyed.    */
int msx_comm_init_loopback(msx_ctx **ctxs, int32_t world);
int msx_sampler_enqueue_group(msx_ctx **ctxs, int32_t world, int32_t slot /* 0|1 */, int64_t nsteps, const int32_t *sidx,
                              const int32_t *cidx, const int32_t *partner, const double *zz, const double *zfac,
                              const double *logu);

/* ---- measurement helpers ----------------------------------------------------------------------- */
/* float4 device-to-device copy of `bytes` bytes, `iters` times; returns GB/s (read+write counted)  */
int msx_stream_copy_gbps(msx_ctx *ctx, int64_t bytes, int32_t iters, double *gbps_out);
/* bytes the hot kernel requests from the memory system per walker, for the form and variant an automatic launch of n
 * walkers of the staged problem takes (the one-workgroup-per-CU variants keep u and the data flux in LDS for the chi^2
 * pass: 132 instead of 148 bytes per pixel of a binary); the launcher's own plan, so always msx_launch_info's figure for
 * block_threads = 0, whatever the form (msx_set_path)                                                               */
int msx_bytes_per_eval(msx_ctx *ctx, int64_t n, int64_t *requested_bytes);

/* One launch of the fused / linked form over n walkers like msx_logprob_batch_dev -- with clock stamps: thread 0 of every
 * walker's workgroup (the first 4096 walkers) reads the 100 MHz wall clock and the shader-cycle counter at its first and
 * last line.  Synchronises; out4 = {median shader clock in MHz while the walkers ran, median and maximum of a walker's own
 * time in us, first walker's start -> last walker's end in us}.  What a short timed region cannot tell apart by itself: a
 * box whose GPU clocks lower under this load from a launch that waits.                                              */
int msx_probe_launch(msx_ctx *ctx, int32_t mode, const double *d_theta, int64_t n, int32_t ndim, double *d_logp,
                     int32_t *d_status, void *hip_stream, int32_t block_threads, double *out4);

/* STORAGE precision of the staged grid tables (SURVEY 8b's `store_dtype`).  MSX_STORE_F64 (default): the per-node pixel
 * table R = lo + (hi - lo) t in float64.  MSX_STORE_F32: R rounded to float32 (8 instead of 12 bytes per node-pixel through
 * the CU's L2 port, which the blend runs at the limit of) and widened in the registers -- the arithmetic stays float64, the
 * grid values carry 2^-24.  A SEPARATELY LABELLED precision: log-probabilities then agree with the reference to ~1e-7
 * relative at S/N 100 (tests/test_gpu_parity.py), inside BASELINE's 1e-6 but not the 1e-9 the float64 tables are held to;
 * bench.py reports it under its own label and never as the headline.  Takes effect at the next msx_stage_problem; fused
 * binaries of at most 17,152 pixels only (the pair and linked forms, triples and longer spectra are refused, not mixed in). */
#define MSX_STORE_F64 0
#define MSX_STORE_F32 1
int msx_set_grid_storage(msx_ctx *ctx, int32_t store_dtype);

/* What an automatic launch of n walkers in `mode` (block_threads as for msx_logprob_batch_dev) WOULD take, asked of the
 * plan the library's own launcher executes (nothing is queued): `name` receives the kernel's name and description, out8 = {form (MSX_FORM_*),
 * threads per workgroup, VGPRs, static LDS bytes, dynamic LDS bytes, bytes requested from the memory system per walker
 * (as msx_bytes_per_eval), workgroups of the first sub-batch, walkers of the first sub-batch}.                          */
#define MSX_FORM_FUSED 0
#define MSX_FORM_PAIR 1
#define MSX_FORM_LINKED 2
#define MSX_FORM_INPATH 3
int msx_launch_info(msx_ctx *ctx, int32_t mode, int64_t n, int32_t block_threads, char *name, int32_t name_len, int64_t *out8);
/* the form (MSX_FORM_*) the last launch queued on this context took (MSX_PATH_AUTO looks at the planner's lagging counts) */
int msx_last_form(msx_ctx *ctx, int32_t *form);

/* the planner's counts for the pair form's last launch (a sub-batch): out2[0] = pairs, out2[1] = walkers evaluated alone;
 * synchronises */
int msx_pair_stats(msx_ctx *ctx, int64_t *out2);

/* ---- target groups: the walkers of several staged targets in one launch -------------------------
 * A group is 1..MSX_MAX_GROUP contexts on one device, each with its own staged grid and problem (data, pixel count, bands,
 * priors, Teff box, A_V table, dist_fit / use_av / rad_prior, no_spectrum, ordinary / rotated / component grid may all
 * differ); they must share nspec (so ndim).  A launch evaluates a batch whose walkers come in contiguous blocks: the
 * first counts[0] are member 0's, the next counts[1] member 1's, ... (a count may be 0).  One workgroup per walker, the
 * fused form's; walker i of member m gets the bits and the status member m's own msx_logprob_batch gives it.  Modes
 * MSX_MODE_LOGLIKE, _LOGPOST, _CHISQ and _LOGPRIOR; no pair, linked or in-path form (the group's own sampler: below).
 * msx_group_create snapshots the members' staged problems (the tables stay theirs: keep the contexts alive).  Refused
 * there, naming the member: float32 grid storage (MSX_ERR_STATE), spectra over 17,152 pixels (MSX_ERR_RANGE), unequal
 * nspec (MSX_ERR_RANGE), members on different devices or without a problem (MSX_ERR_STATE).  A launch after a member's
 * problem was dropped or staged again (msx_stage_problem, grid staging, broadening, rotation, splitting) or after a
 * member was destroyed is refused with MSX_ERR_STATE; create the group again.  *out is set even on failure (read
 * msx_group_last_error, then msx_group_destroy).  Calls on a group are serialised by the caller like a context's.      */
int msx_group_create(msx_ctx **ctxs, int32_t k, msx_group **out);
void msx_group_destroy(msx_group *group);
const char *msx_group_last_error(msx_group *group);
/* host buffers: theta [sum counts][ndim], logp_out / status_out [sum counts]; counts [k]; synchronous, on member 0's stream */
int msx_group_logprob_batch(msx_group *group, int32_t mode, const double *theta, const int64_t *counts, int32_t ndim,
                            double *logp_out, int32_t *status_out);
/* device buffers on a caller stream (does not synchronise); counts is a HOST array [k]; block_threads as for
 * msx_logprob_batch_dev, the variant chosen by its rules for (all walkers, the longest member with walkers) among the ones
 * every member with walkers can take */
int msx_group_logprob_batch_dev(msx_group *group, int32_t mode, const double *d_theta, const int64_t *counts, int32_t ndim,
                                double *d_logp, int32_t *d_status, void *hip_stream, int32_t block_threads);
/* what that launch WOULD take, in msx_launch_info's shape: out8[5] is the members' bytes per walker averaged over the
 * launch's walkers, out8[6] = out8[7] = all walkers (one launch, no sub-batches) */
int msx_group_launch_info(msx_group *group, int32_t mode, const int64_t *counts, int32_t block_threads, char *name,
                          int32_t name_len, int64_t *out8);
/* ---- a target group's DEVICE-RESIDENT SAMPLER: msx_sampler_begin / _enqueue / _collect / _end over
 * a group.  One resident ensemble -- the members' walkers concatenated in member order, counts[m] of member m -- and per
 * half-step exactly ONE launch of the group kernel over the active half of every member's ensemble; no host round trip
 * between half-steps.  The chain of member m is the chain msx_sampler_* gives member m's context alone, fed the same
 * randomness.  counts[m] is even and >= 2 (MSX_ERR_INVALID), mode MSX_MODE_LOGPOST or _LOGLIKE; a member restaged or
 * destroyed since msx_group_create is refused (MSX_ERR_STATE).  Memory: besides the state and two slots as
 * msx_sampler_begin's, 2 * max_chunk_steps * 2 * k snapshots of the members' problems (about 1.2 KB each).
 * coords [sum counts][ndim], logp [sum counts], naccept [sum counts] or NULL (zeros).  A run still open ends.         */
int msx_group_sampler_begin(msx_group *group, int32_t mode, const int64_t *counts, int32_t ndim, int64_t max_chunk_steps,
                            const double *coords, const double *logp, const int64_t *naccept);
/* one chunk of nsteps <= max_chunk_steps iterations into slot 0|1, without waiting for it.  Each array is
 * [nsteps][2][sum counts / 2] in msx_sampler_enqueue's layout, its walker axis the members' active halves side by side
 * (member 0's counts[0] / 2 entries, then member 1's, ...); the indices are MEMBER-LOCAL (sidx, cidx < counts[m],
 * partner < counts[m] / 2) and range-checked (MSX_ERR_INVALID, nothing queued).  A member restaged or destroyed during the
 * run makes this fail with MSX_ERR_STATE; after that, and after any failure that queued part of a chunk, only
 * msx_group_sampler_end is accepted.                                                                                   */
int msx_group_sampler_enqueue(msx_group *group, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                              const int32_t *partner, const double *zz, const double *zfac, const double *logu);
/* the same chunk with its randomness DRAWN ON THE DEVICE: one launch of the counter-based generator (msx_sampler_draw's)
 * on the run's stream ahead of the chunk's half-steps, nothing packed or uploaded.  Member m draws from seeds[m] (seeds
 * [k]) with its own counts[m]: exactly the numbers msx_sampler_draw(seeds[m], a, first_iter, nsteps, counts[m], ndim) gives
 * that target alone, so member m's chain is the one its context walks fed that stream.  first_iter is the ABSOLUTE iteration
 * of the chunk's first step -- the caller's to carry from chunk to chunk and from run to run (msx_group_sampler_begin starts
 * no stream over).  seeds NULL, a not > 1, first_iter < 0 or a member of more than 4096 walkers (the generator's sort):
 * MSX_ERR_INVALID, nothing queued.  Otherwise as msx_group_sampler_enqueue, with which it may alternate within a run.   */
int msx_group_sampler_enqueue_drawn(msx_group *group, int32_t slot, int64_t nsteps, const uint64_t *seeds /* [k] */, double a,
                                    int64_t first_iter);
/* the group's chunks with a set of moves (msx_sampler_enqueue_moves, _moves_drawn above): arrays as for
 * msx_group_sampler_enqueue in the general layout, indices member-local, kind [nsteps][k] -- every member takes its own
 * move per iteration (drawn: from its own seed) -- and the same checks per member.  Member m's chain is the chain
 * msx_sampler_enqueue_moves* gives its context alone.  One step-kernel launch (a workgroup per member) and one plain group
 * evaluation per half-step.                                                                                            */
int msx_group_sampler_enqueue_moves(msx_group *group, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                    const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g,
                                    const double *fac, const double *logu);
int msx_group_sampler_enqueue_moves_drawn(msx_group *group, int32_t slot, int64_t nsteps, const uint64_t *seeds /* [k] */,
                                          const msx_move_set *set, int64_t first_iter);
/* waits for the chunk in `slot`: chain_out [nsteps][sum counts][ndim], logp_out [nsteps][sum counts], naccept [sum counts]
 * (cumulative over the run), worst_status [k] (the worst walker status of each member's walkers in the chunk)          */
int msx_group_sampler_collect(msx_group *group, int32_t slot, double *chain_out, double *logp_out, int64_t *naccept,
                              int32_t *worst_status);
/* ends the run (waits for it); coords / logp (may be NULL) receive the final state.  msx_group_destroy also ends it.  */
int msx_group_sampler_end(msx_group *group, double *coords, double *logp);

/* ---- device chain series: a chain kept on the device, and its autocorrelation -------------------
 * A series holds rows of nw walkers x ndim, laid out [ndim][nw][cap] so that each walker-dimension series is contiguous,
 * and belongs to whoever created it -- not to the context, whose device it lives on: it outlives runs, and two samplers
 * on one context keep two series.  k members of counts[m] walkers (sum = nw), in a group's member order; 1 member for a
 * plain run.  cap_hint: rows to allocate up front (0: on first use; the buffer grows by doubling).                      */
typedef struct msx_series msx_series;
int msx_series_create(msx_ctx *ctx, int64_t nw, int32_t ndim, int32_t k, const int64_t *counts, int64_t cap_hint,
                      msx_series **out);
/* waits for what a run attached to it still queues (the whole device), then frees it                                    */
void msx_series_destroy(msx_series *s);
const char *msx_series_last_error(msx_series *s);
/* rows held: written, or queued by an attached run's enqueues (a chunk's rows are in place once it is collected)         */
int msx_series_rows(msx_series *s, int64_t *out);
/* Attach `s` to the run begun on ctx / group, once, between *_begin and the first enqueue: every chunk of the run then
 * appends its iterations at rows at_row, at_row + 1, ... (a transpose queued on the run's compute stream before the
 * chunk's results are downloaded; every rank of a sharded run keeps its own identical series).  Rows at or after at_row
 * (0 <= at_row <= rows) are dropped.  The series must match the run: nw, ndim and the members' walker counts.  When the
 * run outgrows the buffer it is reallocated and copied at enqueue time, in compute-stream order (readers wait for that
 * copy).  The run detaches at its end (msx_sampler_end / msx_group_sampler_end, or destruction).                        */
int msx_sampler_attach_series(msx_ctx *ctx, msx_series *s, int64_t at_row);
int msx_group_sampler_attach_series(msx_group *group, msx_series *s, int64_t at_row);
/* A tempered run's series: called once, between msx_tempered_begin and the first enqueue, with the
 * rules above for at_row.  Either series may be NULL, not both.  Both have k = ntemps members of nw walkers each, member
 * t = rung t (member 0 is the posterior); chain has the run's ndim, dens has ndim = 2: column 0 is ll, column 1 is lpr.
 * Every chunk, host-drawn or device-drawn, appends its iterations' rows -- the state after the swap sweep, what
 * msx_tempered_collect returns -- at at_row, at_row + 1, ... on the compute stream before the chunk's results travel: a
 * collected chunk's rows are in place.  The series grow as above and are detached by msx_tempered_end.  MSX_ERR_STATE: no
 * tempered run, after the first enqueue, a series with a run attached.  MSX_ERR_INVALID: a series on another device, or
 * whose nw, ndim, k or counts do not match; at_row outside 0 .. the rows each series holds.                              */
int msx_series_attach_tempered(msx_ctx *ctx, msx_series *chain, msx_series *dens, int64_t at_row);
/* host rows [nrows][nw][ndim] appended (synchronous; refused while a run is attached)                                    */
int msx_series_append(msx_series *s, const double *rows, int64_t nrows);
/* rows row0 .. row0 + nrows - 1 back as [nrows][nw][ndim] (synchronous)                                                */
int msx_series_read(msx_series *s, int64_t row0, int64_t nrows, double *out);
/* The normalised autocorrelation of x = rows[0:n][discard::thin] (n' rows), for member m and each dimension d named in
 * dim_mask (bit d):  f_out[(m * ndim + d) * nlag + j] = (1/W_m) sum_{walkers k of m} acov_k(lag0 + j) / acov_k(0),
 * acov_k(tau) = sum_{t < n' - tau} y_k[t] y_k[t + tau], y = x - mean(x), by direct sums in an order fixed by n' alone
 * (the bits do not depend on the lags asked for, the launch or how the rows arrived).  A series with acov_k(0) == 0
 * contributes ones.  Entries of dimensions not in dim_mask are left as they are.  Needs n <= rows and
 * lag0 + nlag <= n'.  Runs on the series' own stream and waits for nothing but the latest growth copy: rows < n must be
 * in place (collected chunks, appended rows).  Synchronous.                                                              */
int msx_series_acf(msx_series *s, int64_t n, int64_t discard, int64_t thin, int64_t lag0, int64_t nlag, uint32_t dim_mask,
                   double *f_out);

/* ---- posterior summaries of a series: exact order statistics and binned marginals -------------
 * What the reference makes of a finished chain before it draws anything: np.median(sample, axis=0) (mft6.py:2025, :2730),
 * the 16 / 50 / 84 percentiles of corner's titles (:1554, :1595, :1636, :1662), the 75-edge marginal counts of T1, T2, R1,
 * R2 and R2 / R1 (:2033-2073) and corner's 50-bin 1-D and 2-D counts.  All three calls name their data the same way:
 *   - the selection x = rows[0:n][discard::thin] (n' rows), msx_series_acf's; member m contributes its W_m walkers, so its
 *     flat sample has N_m = n' W_m values per column;
 *   - a COLUMN is a 32-bit code: c < ndim is coordinate c, MSX_COL_RATIO(a, b) the value x[a] / x[b] (the correctly rounded
 *     IEEE quotient: the reference's ratio = r2 / r1, NumPy's bits).
 * They are synchronous, run on the series' own stream, wait for nothing but the latest growth copy and need n <= rows.
 * Results are integer counts and selected elements: exact, whatever the launch.  MSX_ERR_RANGE: n past the rows held, an
 * empty selection, an unknown column, and what each call names below.                                                     */
#define MSX_COL_RATIO(a, b) (0x80000000u | ((uint32_t)(a) << 8) | (uint32_t)(b))
/* out[(m * ncols + j) * nranks + r] = the element of zero-based rank ranks[m * nranks + r] in ascending order of member m's
 * flat sample of column cols[j]; count_out[m] (may be NULL) = N_m.  Order: -inf < finite < +inf < NaN (np.sort's); -0 and
 * +0 are equal and either may come back.  By radix selection on order-preserving keys: no sort.  MSX_ERR_RANGE: a rank
 * outside 0 .. N_m - 1.                                                                                                   */
int msx_series_order_stats(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                           const int64_t *ranks, int32_t nranks, double *out, int64_t *count_out);
/* counts_out[(m * ncols + j) * (nedges - 1) + b] = the values of member m's column cols[j] with e[b] <= x < e[b + 1],
 * e = edges[(m * ncols + j) * nedges ..] ascending.  closed_last != 0: values equal to the last edge count in the last bin
 * (np.histogram); 0: nowhere (the reference's loop, mft6.py:2046-2049).  Values below e[0], above the last edge and NaN
 * count nowhere.  Placement is by comparison with the edge values.  MSX_ERR_RANGE: nedges outside 2 .. 4097, edges that
 * do not ascend.                                                                                                          */
int msx_series_hist(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                    const double *edges, int32_t nedges, int32_t closed_last, int64_t *counts_out);
/* The same for column pairs (pairs[2 p], pairs[2 p + 1]) = (cx, cy): counts_out[((m * npairs + p) * (nx - 1) + bx) * (ny - 1)
 * + by], with xedges [k][npairs][nx] and yedges [k][npairs][ny] and the same edge rule on both axes (np.histogram2d with
 * closed_last != 0).  MSX_ERR_RANGE: more than 128 bins (129 edges) on an axis, fewer than 2 edges, edges that do not
 * ascend.                                                                                                                 */
int msx_series_hist2d(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *pairs, int32_t npairs,
                      const double *xedges, int32_t nx, const double *yedges, int32_t ny, int32_t closed_last,
                      int64_t *counts_out);

/* ---- block means and log-mean-exponentials of a series column ----------------------------------
 * What thermodynamic integration and the stepping stone make of a ladder's ln L (ptemcee's log_evidence_estimate); for any
 * series.  The selection x = rows[0:n][discard::thin] (n' rows) is msx_series_acf's; member m contributes column col of its
 * W_m walkers.  The n' rows are cut into nblocks consecutive blocks, block b = rows floor(b n' / B) .. floor((b + 1) n' / B)
 * - 1.  mean_out[m * (B + 1)] = the mean of all n' W_m values, mean_out[m * (B + 1) + 1 + b] = block b's mean.  lme_out, in
 * the same layout, = ln((1 / N) sum exp(db[m] x)), computed as db[m] M + ln((1 / N) sum exp(db[m] (x - M))) with M the
 * maximum of the values summed (a block's own; the total combines the blocks by rescaling to their maximum); written for
 * db >= 0.  db [k]; db == NULL skips lme_out.  -inf values give a -inf mean and weigh zero in lme; all -inf gives -inf,
 * never NaN; a NaN gives NaN.  The order of every sum is fixed by (n', W_m, nblocks) alone -- not by the launch, the
 * buffer's capacity, thin or how the rows arrived -- so the same input gives the same bits.  Synchronous, on the series'
 * own stream, waits for nothing but the latest growth copy.  MSX_ERR_RANGE: n past the rows held, an empty selection, col
 * outside the series, nblocks outside 1 .. min(n', 64).                                                                   */
int msx_series_evidence(msx_series *s, int64_t n, int64_t discard, int64_t thin, int32_t col, const double *db, int32_t nblocks,
                        double *mean_out, double *lme_out);

/* ---- between-walker convergence and plain moments of a series -----------------------------------
 * What split R-hat is made of, and the pooled mean and covariance, per member and column; for any series.  The selection x =
 * rows[0:n][discard::thin] (n' >= 4 rows) is msx_series_acf's.  With h = n' / 2 each walker gives two half-chains, rows
 * [0, h) and [n' - h, n') (an odd n' leaves the middle row to neither); half-chain j = 2 w + half of J = 2 W_m.  Per column
 * m_j = S_j / h, s2_j = sum (x - m_j)^2 / (h - 1), and over the half-chains in order j:
 *   within = (sum s2_j) / J,  between = sum (m_j - mbar)^2 / (J - 1) with mbar = (sum m_j) / J,
 *   var_plus = ((h - 1) / h) within + between;   split R-hat = sqrt(var_plus / within), the caller's.
 * mean = the walkers' sums over all n' rows, added in walker order, over N = n' W_m; cov[d][e] = sum (x_d - mean_d)(x_e -
 * mean_e) / (N - 1), the walkers' sums added in walker order, computed for d <= e and mirrored.  within, var_plus, between,
 * mean [k][ncols]; cov [k][ncols][ncols], or NULL: the cross products are then not computed.  cols [ncols]: coordinates <
 * ndim, at most MSX_MAX_DIM; NULL: all of them (ncols = ndim).  Everything is float64 + - * / in an order fixed by n' and
 * W_m alone -- not by thin, discard, the buffer's capacity or how the rows arrived -- so the same input gives the same bits.
 * Special values are IEEE's: a constant column has within = 0; a NaN or an infinity stays in its member's column.
 * Synchronous, on the series' own stream, waits for nothing but the latest growth copy.  MSX_ERR_INVALID: a null series or
 * output (cov apart), discard < 0, thin < 1, ncols < 1.  MSX_ERR_RANGE: n past the rows held, fewer than 4 rows selected, a
 * column >= ndim, ncols over MSX_MAX_DIM (or not ndim with cols NULL).  A refused call leaves the series as it was.         */
int msx_series_moments(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                       double *within, double *var_plus, double *between, double *mean, double *cov);

/* ---- parallel tempering for a target group: every target's ladder in one run -------------------
 * msx_tempered_*'s run with a target axis.  The group's K targets each get a ladder of ntemps rungs (one ntemps for the
 * group, K * ntemps <= MSX_MAX_GROUP) and counts[k] walkers per rung; the K * ntemps (target, rung) pairs are the members of
 * one ensemble in the general layout, target-major and rung-minor: member m = k * ntemps + t owns counts[k] walkers, the
 * coordinates are [sum_k ntemps * counts[k]][ndim], ll and lpr alike.  For member (k, t) an iteration is msx_tempered_*'s
 * iteration for rung t of target k alone -- the split, the moves, P = lpr + beta * ll in two roundings, the accept rule, the
 * prior-reject rule, the sweep from the hottest rung down with db = beta[t-1] - beta[t], the chain rows after the sweep -- so
 * target k's chain is bit for bit the chain of msx_tempered_* on its context alone.  Per iteration EIGHT launches for all
 * targets (step; prior; like; step; prior; like; step; swap -- the evaluations are msx_group_logprob_batch_dev over
 * ntemps * counts[k] / 2 proposals of target k), nine when adaptive; every run keeps its ladders in device memory.
 *
 * begin: betas [K][ntemps], each target's finite, > 0 and strictly descending; counts [K], each even and >= 2; coords, ll,
 * lpr in the layout above.  MSX_ERR_INVALID: K * ntemps outside 1..MSX_MAX_GROUP, bad betas or counts, ndim != 2 nspec + 2, a
 * chunk too long (walkers * ndim * steps > 2^31), an lpr that is not finite or a NaN ll.  MSX_ERR_STATE: a run of either
 * family (msx_group_sampler_*, msx_group_tempered_*) in flight on the group -- msx_group_sampler_begin likewise refuses while
 * a tempered run is in flight --, a member restaged or destroyed since msx_group_create, a member whose context has a run of
 * its own in flight or holds a communicator.                                                                              */
int msx_group_tempered_begin(msx_group *group, int32_t ntemps, const double *betas, const int64_t *counts, int32_t ndim,
                             int64_t max_chunk_steps, const double *coords, const double *ll, const double *lpr);
/* one host-drawn chunk: the general layout's arrays [nsteps][2][H], H = sum_k ntemps * counts[k] / 2, the members' halves side
 * by side in member order and every index member-local (p1, p2 index the complementary half); kind [nsteps][K * ntemps];
 * swap_logu [nsteps][sum_k (ntemps - 1) * counts[k]], target k's [ntemps - 1][counts[k]] block after target k - 1's (row p:
 * the pair (p + 1, p)).  msx_tempered_enqueue's checks per member.  A refused call queues nothing; after a member was restaged
 * or destroyed the call is refused with MSX_ERR_STATE and only msx_group_tempered_end is taken from then on.            */
int msx_group_tempered_enqueue(msx_group *group, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                               const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                               const double *logu, const double *swap_logu);
/* one chunk drawn on the device: member (k, t) from seeds[k * ntemps + t] (streams 0..13), target k's swap draws stream 14 of
 * seeds[k * ntemps] at index (t - 1) * 4096 + w -- the numbers msx_tempered_enqueue_drawn(seeds[k]) draws for that target
 * alone.  first_iter: the chunk's first ABSOLUTE iteration, one for the whole group.  MSX_ERR_INVALID: more than 4,096 walkers
 * per rung, first_iter < 0, a bad set (the DE move needs 4 walkers in every rung).                                        */
int msx_group_tempered_enqueue_drawn(msx_group *group, int32_t slot, int64_t nsteps, const uint64_t *seeds, const msx_move_set *set,
                                     int64_t first_iter);
/* waits for the chunk: chain [nsteps][sum ntemps * counts][ndim], ll_chain, lpr_chain [nsteps][sum ntemps * counts], naccept
 * [sum ntemps * counts] and nswap [K][ntemps - 1] running since begin, worst [K][ntemps] of this chunk                     */
int msx_group_tempered_collect(msx_group *group, int32_t slot, double *chain, double *ll_chain, double *lpr_chain, int64_t *naccept,
                               int64_t *nswap, int32_t *worst);
/* ends the run (no run: MSX_OK); the final state where asked for (any may be NULL)                                       */
int msx_group_tempered_end(msx_group *group, double *coords, double *ll, double *lpr);
/* the run's two series, once between begin and the first enqueue: K * ntemps members, member k * ntemps + t of counts[k]
 * walkers; `chain` with the run's ndim, `dens` with ndim 2 (ll, lpr); either may be NULL.  msx_series_attach_tempered's rules;
 * msx_series_acf, _order_stats, _hist, _hist2d and _evidence then work per member (db [K * ntemps]).                       */
int msx_group_tempered_attach_series(msx_group *group, msx_series *chain, msx_series *dens, int64_t at_row);
/* msx_ladder_adapt / _betas / _current with a target axis: lag, time, k0 [K] (target k's own; msx_ladder_adapt's bounds and
 * state rules); out [nsteps][K][ntemps]; betas [K][ntemps], k and skipped [K] (either may be NULL).                        */
int msx_group_ladder_adapt(msx_group *group, const double *lag, const double *time, const int64_t *k0);
int msx_group_ladder_betas(msx_group *group, int32_t slot, double *out);
int msx_group_ladder_current(msx_group *group, double *betas, int64_t *k, int64_t *skipped);

/* ---- derived posteriors: product bands and derived columns of samples -------------------------
 * What the reference makes of chain samples after the run: make_composite(..., plot=True) (mft6.py:786-828) gives each
 * star's Kepler-band and Gaia G magnitude, from which plot_results derives the Kepler contrast and the planet-radius
 * correction factors (mft6.py:2505, :2544-2545), and the isochrone gives masses and luminosities (mft6.py:2679-2690).
 * Band integrals are linear in the node spectra, so a product band is a per-node table built once at staging, as the
 * staged problem's own bands are; a sample then costs one thread a recipe and a few table look-ups.                     */
#define MSX_PB_TRAPZ 0 /* sum w S = np.trapz(S[mask] * interp1d(ran, tm)(wl[mask]), wl[mask])         mft6.py:792-799 */
#define MSX_PB_SUM 1   /* sum w S = np.sum(S[mask] * interp1d(ran, tm)(wl[mask])): the triple's        mft6.py:820-822 */
#define MSX_PB_MEAN 2  /* photon-counting mean flux (pyphot get_flux); magnitudes minus zero_mag       mft6.py:811-814 */
typedef struct msx_products {
    int32_t struct_size;      /* sizeof(msx_products), ABI check                                                         */
    int32_t nbands;           /* 1 .. MSX_MAX_BANDS product bands                                                        */
    const int32_t *band_kind; /* [nbands] MSX_PB_*                                                                       */
    const int64_t *band_i0;   /* [nbands] first grid sample of each band: the layout of msx_problem's band_w             */
    const int64_t *band_len;
    const double *band_w;     /* concatenated weights                                                                    */
    const double *band_zero_mag; /* [nbands] the zero-point magnitude subtracted from an MSX_PB_MEAN magnitude (others: unused) */
    /* the product isochrone, sorted by Teff as interp1d sorts it: the first 200 rows of age 9.0     mft6.py:2604-2605,:2650,:2679 */
    int32_t niso;
    const double *iso_teff, *iso_mass, *iso_lum;
} msx_products;
/* Valid after msx_stage_problem; builds the per-node table of the product bands (once per copy of a component grid).
 * Whatever drops the staged problem (staging it again, grid staging, broadening, rotation, splitting) drops the products.
 * MSX_ERR_STATE: no problem staged.  MSX_ERR_RANGE: a band outside the staged grid, an unknown kind.                    */
int msx_stage_products(msx_ctx *ctx, const msx_products *p);

/* A derived COLUMN is a 32-bit code (kind << 24 | band << 8 | star); codes below ndim are the sample's own coordinates.
 * b: a product band, s: a star (0 = primary), f / p: a contrast filter / photometric band of the staged problem.        */
#define MSX_PCOL_BANDMAG(b, s) (0x01000000u | ((uint32_t)(b) << 8) | (uint32_t)(s)) /* -2.5 log10(star s's integral in band b), minus zero_mag for MSX_PB_MEAN  mft6.py:802,:813-814,:825 */
#define MSX_PCOL_BANDMAG_SUM(b) (0x02000000u | ((uint32_t)(b) << 8))                /* the same of the stars' integrals summed in star order                     mft6.py:812 */
#define MSX_PCOL_DMAG(b, s) (0x03000000u | ((uint32_t)(b) << 8) | (uint32_t)(s))    /* BANDMAG(b, s) - BANDMAG(b, 0): the Kepler contrast for s = 1              mft6.py:2505 */
#define MSX_PCOL_PRI_CORR(b) (0x04000000u | ((uint32_t)(b) << 8))                   /* sqrt(1 + 10**(-0.4 DMAG(b, 1)))                                           mft6.py:2544 */
#define MSX_PCOL_SEC_CORR(b) (0x05000000u | ((uint32_t)(b) << 8))                   /* ratio sqrt(1 + 10**(0.4 DMAG(b, 1))), ratio = the sample's R2 / R1 coordinate  mft6.py:2504,:2545 */
#define MSX_PCOL_CONTRAST(f) (0x06000000u | (uint32_t)(f))                          /* the model contrast in the staged problem's filter f                       mft6.py:741,:747-749 */
#define MSX_PCOL_PHOT(p) (0x07000000u | (uint32_t)(p))                              /* the unreddened model magnitude in its photometric band p                  mft6.py:780-783 */
#define MSX_PCOL_LOGG(s) (0x08000000u | (uint32_t)(s))                              /* the isochrone's log g at T_s                                              mft6.py:95 */
#define MSX_PCOL_MASS(s) (0x09000000u | (uint32_t)(s))                              /* the product isochrone's mass at T_s                                       mft6.py:2685-2686 */
#define MSX_PCOL_LUM(s) (0x0a000000u | (uint32_t)(s))                               /* ... and luminosity                                                        mft6.py:2689-2690 */
#define MSX_MAX_PCOLS 64 /* columns of one msx_products_batch call (msx_series_derive: MSX_MAX_DIM, a series' width) */
/* theta [n][ndim] (ndim = 2 nspec + 2, the sampler's rows [T.., A_V, R1, ratios.., plx]) -> out [n][ncols], status [n]
 * (MSX_W_*).  One thread per sample: the isochrone's log g per star, the Teff and log g brackets, the bilinear weights
 * and the (R/d)^2 scale -- or, for a problem staged with dist_fit = 0, the ratio^2 scale of `distance=False`
 * (mft6.py:698-703) -- then the columns from the per-node tables.  No prior is applied.  A sample whose status is not
 * MSX_W_OK has NaN in every column: non-finite coordinates (MSX_W_REJECT), a Teff outside the isochrone -- the product
 * isochrone too when a MASS or LUM column is asked for -- (MSX_W_VALUEERROR), a missing node or a bracket past the grid.
 * MSX_ERR_STATE: no products staged.  MSX_ERR_RANGE: more than MSX_MAX_PCOLS columns, an unknown code, a band, star,
 * filter or coordinate the staged tables do not have.                                                                  */
int msx_products_batch(msx_ctx *ctx, const double *theta, int64_t n, int32_t ndim, const uint32_t *cols, int32_t ncols,
                       double *out, int32_t *status);
/* the same with device pointers (cols too) on a caller stream; does not synchronise; the codes are NOT checked        */
int msx_products_batch_dev(msx_ctx *ctx, const double *d_theta, int64_t n, int32_t ndim, const uint32_t *d_cols, int32_t ncols,
                           double *d_out, int32_t *d_status, void *hip_stream);
/* The same map over rows of a series: rows row0 .. row0 + nrows - 1 of src (ndim = 2 nspec + 2) become rows row0 .. of
 * dst, a series created with ndim = ncols and src's members; member m's walkers are evaluated with ctxs[m]'s problem and
 * products (k = the series' member count; the contexts live on the series' device and share nspec).  A derived row
 * carries the bits msx_products_batch gives that row.  dst grows as msx_series_append grows it and must hold at least
 * row0 rows; rows from row0 on are overwritten and dst then holds max(rows, row0 + nrows) rows.  Synchronous, on src's
 * stream; waits for nothing but the two series' latest growth copies: the rows read must be in place.  worst_status [k]
 * (may be NULL): the worst sample status per member.  Afterwards msx_series_order_stats / _hist / _hist2d / _acf work on
 * dst as on any series.  MSX_ERR_STATE: a member without staged products, a run attached to dst.  MSX_ERR_RANGE: ncols
 * over MSX_MAX_DIM, a bad code, rows past src.  MSX_ERR_INVALID: series that do not match.                              */
int msx_series_derive(msx_series *src, msx_ctx **ctxs, const uint32_t *cols, int32_t ncols, int64_t row0, int64_t nrows,
                      msx_series *dst, int32_t *worst_status);

/* The spectra of samples on the data pixels (mft6.py:2374-2415): out [n][1 + nspec][npix] in PIXEL order.  Rows 1 .. nspec
 * hold each star's spectrum, scaled as in make_composite, reddened by the sample's A_V on the model grid and resampled to
 * the staged problem's data pixels (:2394-2402); row 0 is their sum in star order (:744, :751).  With
 * MSX_SPEC_MEDIAN_SCALE in flags row 0 is multiplied by median(data) / median(row 0) (:2409; the exact median, median.h's
 * radix selection) and scale_out [n] receives the factor (1 without the flag).  A_V <= 0, or a problem staged without
 * extinction, follows the likelihood's rule: no reddening (:1161).  One workgroup per sample; status [n] as for
 * msx_products_batch (NaN rows and factor unless MSX_W_OK).  MSX_ERR_STATE: no products staged.                        */
#define MSX_SPEC_MEDIAN_SCALE 1
int msx_products_spectra(msx_ctx *ctx, const double *theta, int64_t n, int32_t ndim, int32_t flags, double *out, double *scale_out,
                         int32_t *status);
/* composite_kernel generalised (mft6.py:684-707): one row per star of the blend over grid samples [j0, j0 + n), scaled as
 * msx_make_composite scales it -- comp_out [nspec][n]; the composite is the rows' sum in star order.  teff / logg / rad
 * [nspec] and use_distance as for msx_make_composite.  Needs a staged problem (its nspec, its grid).  MSX_ERR_RANGE: a
 * window outside the staged grid.                                                                                      */
int msx_composite_parts(msx_ctx *ctx, const double *teff, const double *logg, const double *rad, int32_t use_distance, double plx,
                        int64_t j0, int64_t n, double *comp_out, int32_t *status);

/* ---- posterior predictive checks: bands, residuals and chi^2 terms of samples -----------------
 * What the reference's all_spec figure shows of a finished run (mft6.py:2361-2438) and what its likelihood adds up
 * (:1173-1191), for every sample of a chain and reduced per data pixel on the device.  For a sample theta (ndim = 2 nspec +
 * 2) on a context with a staged problem and staged products:
 *   ROWS 0 .. nspec are msx_products_spectra's rows with MSX_SPEC_MEDIAN_SCALE -- row 0 the composite times median(data) /
 *     median(row 0), rows 1.. each star -- and carry the bits that call gives the sample;
 *   data_n = data / P(u), P the quadratic least-squares fit of data / row 0 (norm_spec, :193-196, :1174);
 *   z = (row 0 - data_n) / sigma, so that chisq (:115-120) is z^2;
 *   TERMS chi_spec = sum(z^2) / npix (:1179), chi_contrast (:1182-1183), chi_phot with the magnitudes reddened as in
 *     :1161-1166 (:1188-1189), chi_total = chi_spec (nc + np) + chi_contrast + chi_phot (:1191; a problem staged with
 *     no_spectrum: chi_contrast + chi_phot).  A_V <= 0, or a problem staged without extinction: no reddening.
 * No prior is applied.  Only samples whose status is MSX_W_OK enter the reductions, in their order; count is how many did.
 * A sample that cannot be evaluated has NaN terms and its status is reported (msx_products_batch's codes).
 *
 * band  [4][1 + nspec][npix]: mean, variance (ddof = 1), min, max over the valid samples, per row and pixel, in PIXEL order;
 * quant [nq][1 + nspec][npix], or NULL: np.quantile's default (linear) quantiles at q [nq] -- the device selects the elements
 *   of ranks floor(h) and min(floor(h) + 1, N - 1), h = (N - 1) q, exactly (median.h's radix selection); the host
 *   interpolates with NumPy's roundings;
 * resid [3][npix]: the means over the valid samples of data_n, z and z^2;
 * terms [n][4]: chi_spec, chi_contrast, chi_phot, chi_total;  status [n];  count [1].
 * count == 0: every reduced output is NaN.  count == 1: the variance is NaN (np.var(ddof=1)).
 *
 * REPRODUCIBILITY.  Every reduced output is a function of the ordered list of the valid samples' values alone: a sum is
 * formed by 256 partial sums over every 256th value, combined in one fixed order, and the variance is the second of two
 * passes, sum (x - mean)^2 / (N - 1) in that order -- never from sums of squares of the raw values.  The bits do not depend
 * on scratch_bytes, the pixel tiles or sample batches it leads to, the launch, thin, discard, the buffer's capacity, how the
 * rows arrived, or on which of the two calls the samples came through.
 *
 * scratch_bytes bounds the temporary device memory of the two large buffers, which share it in turn: the sample pass's
 * work rows (npix doubles per sample in flight) and the value buffer of a pixel tile ((nspec + 4) N doubles per pixel, N
 * the samples selected); samples are evaluated in batches and pixels in tiles sized from it.  0: 256 MiB.  Beside it the
 * call keeps a 192-byte record per sample and the outputs.  Host pointers; synchronous.
 * MSX_ERR_RANGE: scratch_bytes below 8 * max(npix, (nspec + 4) N), a q outside [0, 1].  MSX_ERR_STATE: no products
 * staged.  MSX_ERR_INVALID: null pointers, n < 1, ndim != 2 nspec + 2.  A refused call writes nothing.                   */
int msx_predictive_batch(msx_ctx *ctx, const double *theta, int64_t n, int32_t ndim, const double *q, int32_t nq,
                         int64_t scratch_bytes, double *band, double *quant, double *resid, double *terms, int32_t *status,
                         int64_t *count);
/* The same over the selection rows[0:n][discard::thin] of a device chain (msx_series_acf's selection): member m's walkers
 * flattened in (row, walker) order -- get_chain(flat=True)'s -- and evaluated with ctxs[m] (k = the series' member count;
 * the contexts live on the series' device and share nspec; their npix may differ).  band, quant and resid are member-major:
 * member m's block is laid out as above, behind the blocks of the members before it.  count [k]; worst_status [k] (may be
 * NULL): the worst sample status among the rows evaluated.  terms_dst: NULL, or a series of ndim = 4 with src's members,
 * which receives the four terms of EVERY row 0 .. n - 1 (discard and thin only pick what is reduced; without it only the
 * selection is evaluated); it grows as msx_series_derive's dst does, rows 0 .. n - 1 are overwritten and it then holds
 * max(rows, n) rows, on which msx_series_order_stats / _hist / _acf / _moments work as on any series.  N above is the
 * member's selected samples.  Synchronous, on src's stream; waits for nothing but the two series' latest growth copies.
 * MSX_ERR_RANGE: n past the rows held, an empty selection, and the above.  MSX_ERR_STATE: a member without staged products,
 * a run attached to terms_dst.  MSX_ERR_INVALID: series that do not match.  A refused call leaves both series as they were. */
int msx_series_predictive(msx_series *src, msx_ctx **ctxs, int64_t n, int64_t discard, int64_t thin, const double *q, int32_t nq,
                          int64_t scratch_bytes, double *band, double *quant, double *resid, msx_series *terms_dst,
                          int64_t *count, int32_t *worst_status);

/* ---- posterior modes of a series: mixture fit, labels, the samples by mode ----------------------
 * A Gaussian mixture of ncomp components over ncols columns of every member, by EM; mcmc_spec_amd/modes.py is the definition
 * (standardised units z = (x - center) / scale, E-step through the Cholesky factor, the M-step with ridge on the diagonal,
 * the stopping rule, the statuses).  The selection rows[0:n][discard::thin] (n' rows) is msx_series_acf's; a sample with a
 * non-finite selected value enters no sum.  cols [ncols]: coordinates < ndim, at most MSX_MAX_DIM; NULL: all (ncols = ndim).
 * center, scale [k][ncols].  A JOB is a (member, start): start s assigns a sample to the component numbered by how many of
 * split_at[m][s][0 .. ncomp - 2] (raw units, not descending; NULL with ncomp = 1) are <= its column cols[split_col[s]], and the
 * M-step of that assignment gives the first parameters; then up to max_iter iterations, every job's queued back to back with
 * no host read in between (two launches an iteration; a job that stopped is skipped on a flag in device memory).
 * Out, components in start order: weight [k][nstarts][ncomp], mean [..][ncomp][ncols], cov [..][ncomp][ncols][ncols]
 * (standardised units, ridge included), loglik, niter, status [k][nstarts] (MSX_MODES_*), nbad [k].  The order of every sum
 * depends on (n', W_m) alone: the same input gives the same bits whatever thin, discard, the buffer's capacity, how the rows
 * arrived and how many jobs share the call.  Synchronous, on the series' own stream, waits for nothing but the latest growth
 * copy; reads no row at or past n.  Refused before any launch, the series as it was -- MSX_ERR_INVALID: a null series or
 * output, thin < 1, discard < 0, ncols < 1, nstarts < 1, a scale that is not finite or not > 0, a center that is not finite,
 * ridge < 0, tol < 0 (or NaN), max_iter < 1.  MSX_ERR_RANGE: n past the rows held, fewer than 4 rows selected, a column >=
 * ndim, ncols over MSX_MAX_DIM (or not ndim with cols NULL), ncomp outside 1 .. MSX_MODES_MAX, nstarts over 64, a split_col
 * outside 0 .. ncols - 1, thresholds that descend (or NaN), N_m = n' W_m <= ncomp (ncols + 1).                              */
#define MSX_MODES_MAX 4
#define MSX_MODES_CONVERGED 0 /* |loglik - previous| <= tol |loglik| after iteration niter >= 2 */
#define MSX_MODES_MAXITER 1   /* max_iter iterations run                                         */
#define MSX_MODES_COLLAPSED 2 /* an M-step found a component holding less than one sample        */
int msx_series_modes(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                     const double *center, const double *scale, int32_t ncomp, int32_t nstarts, const int32_t *split_col,
                     const double *split_at, int32_t max_iter, double tol, double ridge, double *weight, double *mean,
                     double *cov, double *loglik, int32_t *niter, int32_t *status, int64_t *nbad);
/* Labels under ONE mixture per member -- weight [k][ncomp], mean [k][ncomp][ncols], cov [k][ncomp][ncols][ncols], the
 * caller's (the call keeps no state) -- of the same selection: label = argmax_k lp_k, the lowest k on ties, 255 for a sample
 * with a non-finite selected value.  labels_out: host uint8 [n'][nw], or NULL; counts_out [k][ncomp].  dst: NULL, or
 * k * ncomp series created by the caller on s's device with nw = 1, one member, s's ndim and no run attached: dst[m * ncomp +
 * j] receives ALL ndim coordinates of member m's samples labelled j, walker ascending, then row ascending (per-tile counts, an
 * exclusive scan, ballot prefixes inside a tile: the same order every time).  It grows as msx_series_append grows a series
 * and ends holding exactly counts_out[m][j] rows, possibly none; msx_series_order_stats / _hist / _hist2d / _moments, and
 * msx_series_derive where products are staged, then work on a mode as on any series.  Synchronous, on s's stream.
 * msx_series_modes' refusals where they apply; also MSX_ERR_RANGE: a covariance without a Cholesky factor, a weight that is
 * negative or NaN; MSX_ERR_INVALID: a dst that does not match or is listed twice; MSX_ERR_STATE: a run attached to a dst.  */
int msx_series_mode_labels(msx_series *s, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                           const double *center, const double *scale, int32_t ncomp, const double *weight, const double *mean,
                           const double *cov, uint8_t *labels_out, int64_t *counts_out, msx_series **dst);

/* ---- importance reweighting of a series: re-scored rows, weights, weighted moments, resampling ----
 * Asking a finished chain another question -- another prior, another likelihood term, a ladder's rung -- without a second
 * run: the chain's rows are scored again, the difference of two log-densities is a log-weight, and the weighted chain is
 * summarised or resampled; mcmc_spec_amd/reweight.py is the NumPy definition of all but the first call.  Host pointers;
 * synchronous, on the named series' own stream; every call waits for nothing but the latest growth copies of the series it
 * touches: the rows read must be in place.  The selection rows[0:n][discard::thin] (n' rows) is msx_series_acf's; member m's
 * FLAT sample is in (row, walker) order -- get_chain(flat=True)'s --, flat index i = t W_m + walker, N_m = n' W_m.  A
 * "weights" series has ndim = 1 and the members of the series it weighs.  SUMS are formed per walker (element i, i + 256, ..
 * one after the other, then a fixed tree over the 256 partial sums) and then over the member's walkers in walker order:
 * float64 + - * / in an order fixed by (n', W_m) alone, so the same input gives the same bits whatever thin, discard, the
 * buffer's capacity and how the rows arrived.  A refused call leaves every series as it was.  Common refusals --
 * MSX_ERR_INVALID: null pointers, discard < 0, thin < 1, series that do not match (device, members, ndim); MSX_ERR_RANGE: n
 * or rows past the ones a series holds, an empty selection, a column outside its series; MSX_ERR_STATE: a run attached to a
 * series that would be written.                                                                                            */

/* Rows row0 .. row0 + nrows - 1 of src (ndim = 2 nspec + 2) through the unchanged evaluation (msx_logprob_batch_dev) with
 * ctxs[m]'s staged problem for member m, in `mode` (MSX_MODE_LOGPOST, MSX_MODE_LOGPRIOR or MSX_MODE_LOGLIKE), into the same
 * rows of dst: a series with src's members and ndim = 1, which grows and is overwritten as msx_series_derive's dst is.  A
 * value carries the bits msx_logprob_batch gives that theta on that context; a rejected sample (MSX_W_REJECT) gives -inf; a
 * sample with an error status gives NaN and its status is reported: worst_status [k] (may be NULL), the worst per member.
 * Rows are gathered and evaluated member by member in batches of at most 65,536 samples from the series' scratch; a sample's
 * bits do not depend on the launch it shares, so not on the batch.  No products need be staged.  MSX_ERR_STATE: a member
 * without a staged problem, or with a run of its own in flight.  MSX_ERR_INVALID: another mode, ndim != 2 nspec + 2.        */
int msx_series_logprob(msx_series *src, msx_ctx **ctxs, int32_t mode, int64_t row0, int64_t nrows, msx_series *dst,
                       int32_t *worst_status);
/* dst[row][walker] = ((coef[0] x_0) + coef[1] x_1) + ..., x_j = srcs[j][row][walker][cols[j]], for rows row0 .. row0 + nrows
 * - 1: each product rounded, then the additions in j order, no FMA contraction -- NumPy's bits for coef[0] * x0 + coef[1] * x1
 * + ...  IEEE special values pass through.  nsrc 1 .. 8; dst (ndim = 1) is none of the sources and shares their members; it
 * grows and is overwritten as msx_series_derive's dst is.  The result is a log-weight: lp_new - lp_old, (1 - beta) ll of a
 * ladder's dens series, +0.5 chi_contrast of a terms series, or any mixture.  On dst's stream; dst carries the error text.  */
int msx_series_lincomb(int32_t nsrc, msx_series **srcs, const int32_t *cols, const double *coef, int64_t row0, int64_t nrows,
                       msx_series *dst);
/* The weights of the log-weights logw (ndim = 1): per member M_m = the maximum over rows [0, n) of the values that are finite
 * or -inf, and w = exp(logw - M_m) into rows [0, n) of w_dst (it grows as above and then holds max(rows, n) rows).  A NaN or
 * +inf log-weight is BAD and weighs 0; -inf weighs 0; a member without a finite value has all weights 0.  stats [k][6] over
 * the SELECTION: count N_m, nbad, nzero (weights == 0 that are not bad), sum w, sum w^2 and Kish's effective sample size
 * (sum w)^2 / sum w^2 (0 when nothing weighs), the sums in the order above.  exp is the device library's.                 */
int msx_series_weights(msx_series *logw, int64_t n, int64_t discard, int64_t thin, msx_series *w_dst, double *stats);
/* Weighted moments of the selection of src under the weights w: per member sumw [k] = sum w (msx_series_weights' sum, its
 * bits), mean [k][ncols] = sum (w x) / sum w, and cov [k][ncols][ncols] (or NULL) = sum (w ((x_d - mean_d)(x_e - mean_e))) /
 * sum w -- the second of two passes, for d <= e and mirrored.  cols as msx_series_moments'.  A sample of zero weight enters
 * no sum, whatever its values; with a non-zero weight a non-finite value poisons its column, as IEEE arithmetic does.       */
int msx_series_wmoments(msx_series *src, msx_series *w, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols,
                        int32_t ncols, double *sumw, double *mean, double *cov);
/* Systematic resampling.  Member m's selected samples have the weights w_0 .. w_{N-1} in flat order; their inclusive prefix
 * sums C_i come from a three-phase scan over tiles of MSX_RESAMPLE_TILE consecutive samples:
 *   1. inside a tile, lane l of 256 adds its MSX_RESAMPLE_TILE / 256 consecutive values one after the other, and the lanes'
 *      totals are scanned serially in lane order: local_i = E_l + s_e; the tile's sum is the last of them;
 *   2. the tiles' sums are scanned serially in tile order: B_0 = 0, B_{j+1} = B_j + sum_j;
 *   3. C_i = B_tile + local_i.
 * The bits of C depend on N and the values alone, and C never decreases: each level's last value is exactly the next base.
 * W = C_{N-1}, step = W / nout[m], u0 = one uniform of the counter generator (stream 15, index 0, with the member's number
 * in the iteration's place), t_j = (j + u0) * step in two roundings for j < nout[m], and sample j is the first i with C_i >
 * t_j, clamped to the last i with w_i > 0: a sample of zero weight is never drawn.  dst [k]: caller-created series on src's
 * device with one walker, one member and src's ndim (msx_series_mode_labels' dst); dst[m] receives all ndim coordinates of
 * the drawn samples in j order and ends holding exactly nout[m] rows, possibly none.  index_out: NULL, or sum nout int64,
 * member after member: the drawn flat indices.  MSX_ERR_RANGE, before anything is written to a dst: a weight that is
 * negative, NaN or infinite; W == 0 (or not finite) for a member with nout > 0.  MSX_ERR_INVALID: a negative nout, a dst
 * that does not match or is listed twice.                                                                                  */
#define MSX_RESAMPLE_TILE 1024
int msx_series_resample(msx_series *src, msx_series *w, int64_t n, int64_t discard, int64_t thin, uint64_t seed,
                        const int64_t *nout, msx_series **dst, int64_t *index_out);

/* ---- Pareto-smoothed importance sampling of a log-weight series -----------------------------------
 * Kish's effective sample size looks healthy while the variance of the weights is infinite.  PSIS (Vehtari, Simpson, Gelman,
 * Yao & Gabry 2024) fits a generalised Pareto distribution to the largest weights by Zhang & Stephens' (2009) profile
 * posterior mean, reports its shape khat -- below about 0.7 the weighted estimates are reliable -- and replaces those weights
 * by the fitted quantiles.  mcmc_spec_amd/psis.py is the NumPy definition; the reference project has no counterpart.
 *
 * Per member, over the FLAT selection of logw (ndim = 1; the family's selection and flat order above), N_m values:
 *   bad      NaN and +inf are BAD as in msx_series_weights: they weigh 0 and do not count; S = N_m - nbad.  -inf weighs 0 and
 *            counts.
 *   shift    x = logw - max (the maximum of the values that are not bad, over the selection).
 *   cutoff   the element of ascending rank S - tail_len[m] - 1 (0-based) of x, by the radix selection of
 *            msx_series_order_stats over all of the member's workgroups, and not below MSX_PSIS_LOG_TINY.  tail_len comes from
 *            the host (ceil(min(S / 5, 3 sqrt(S / reff))) is the papers'); the device never recomputes it.
 *   tail     the samples with x strictly above the cutoff, ordered by (x, flat index): at most tail_len of them, fewer with
 *            ties across the cutoff.  Fewer than MSX_PSIS_MIN_TAIL: nothing is smoothed, khat = +inf, MSX_PSIS_SHORT_TAIL (a
 *            constant log-weight ends here, and so does a member without a finite value, whose weights are all 0).
 *   fit      t_j = exp(x_j) - exp(cutoff) ascending, n of them; m = 30 + floor(sqrt(n)); b_i = 1 / t_{n-1} + (1 - sqrt(m / (i -
 *            0.5))) / (3 t_q), i = 1 .. m, t_q = t[int(n / 4 + 0.5) - 1]; k_i = mean_j log1p(-b_i t_j); L_i = n (log(-b_i / k_i)
 *            - k_i - 1); w_i = 1 / sum_l exp(L_l - L_i); b = sum b_i w_i / sum w_i; k = mean_j log1p(-b t_j); sigma = -k / b;
 *            khat = (n k + 5) / (n + 10).
 *   replace  the tail's j-th value becomes min(log(exp(cutoff) + sigma expm1(-khat log1p(-p_j)) / khat), 0), p_j = (j + 0.5) /
 *            n (the limit -sigma log1p(-p_j) for |khat| < 1e-30).
 *   weights  w = exp(value - the largest value) into the selected rows of w_dst; every other row of [0, n) weighs 0.  lw_dst
 *            (may be NULL; as w_dst) receives value - logsumexp(values), the normalised log-weights, -inf elsewhere.
 * One workgroup per member compacts the tail (value and 32-bit flat index) into LDS, sorts it there, fits and replaces.  Sums
 * over the tail: lane l of 256 adds elements l, l + 256, .. one after the other, then a fixed tree; sums over the member: lane
 * l adds, walker after walker, rows l, l + 256, .., then the tree -- an order fixed by (n', W_m) and the tail's length alone.
 * No float atomics; no workgroup waits for another.  exp, log, log1p, expm1 and sqrt are the device library's.
 * Outputs per member: khat [k], status [k], tail_count [k], stats [k][6] (msx_series_weights' statistics of the smoothed
 * weights), tail_index (NULL, or [k][MSX_PSIS_TAIL_MAX]: the tail's flat indices in order, -1 past tail_count).  w_dst then
 * serves msx_series_wmoments and msx_series_resample as any weights series does.
 * Refusals, nothing written -- the family's, and MSX_ERR_RANGE: tail_len[m] outside 1 .. min(S - 1, MSX_PSIS_TAIL_MAX) (so
 * every member needs S >= 2), a member of 2^31 samples or more.                                                            */
#define MSX_PSIS_TAIL_MAX 4096
#define MSX_PSIS_MIN_TAIL 5
#define MSX_PSIS_LOG_TINY (-708.3964185322641) /* log of the smallest normal double */
#define MSX_PSIS_OK 0
#define MSX_PSIS_SHORT_TAIL 1
int msx_series_psis(msx_series *logw, int64_t n, int64_t discard, int64_t thin, const int64_t *tail_len, msx_series *w_dst,
                    msx_series *lw_dst, double *khat, int32_t *status, int64_t *tail_count, double *stats, int64_t *tail_index);

/* ---- pointwise model checks: PSIS-LOO, WAIC and khat per observation -----------------------------------
 * "Binary or triple?" for a user who ran a plain chain, and "which data can one sample not stand in for?".  The reference
 * project has no counterpart; the estimates are those of Vehtari, Gelman & Gabry (2017) with the PSIS above, and
 * mcmc_spec_amd/psis.py (pointwise_stats) is the NumPy definition.
 * OBSERVATIONS.  loglikelihood is -0.5 [(nc + np) sum_p z_p^2 / npix + sum_f chi_contrast,f + sum_f chi_phot,f] (mft6.py:1179-1191):
 * the observations are the npix pixels, then the nc contrast filters, then the np photometry bands, n_obs = npix + nc + np (nc +
 * np for a problem staged with no_spectrum).  A pixel's term is coef * z^2 with coef = (-0.5 (nc + np)) / npix rounded once and
 * z^2 the bits the predictive check forms; a filter's term is -0.5 s with s = (z z) / (err err) the summand of the predictive
 * check's chi_contrast / chi_phot in its roundings.  A sample's terms add up to its MSX_MODE_LOGLIKE value up to the order of
 * the sum.  These are the terms of the likelihood the reference SAMPLES, its (nc + np) / npix weighting and all, and pixels are
 * coupled through the continuum fit and the broadening: elpd_loo here is a per-term influence and a RELATIVE score between
 * models on identical data, errors and pixels -- not an absolute predictive density.
 * Per observation over the `count` samples that can be evaluated (the others are left out, as in the predictive check), out
 * [6][n_obs]: lppd = logsumexp_s(ll) - log count; p_waic = var_s(ll) (ddof 1, two passes); elpd_waic = lppd - p_waic; elpd_loo =
 * logsumexp_s(lw_s + ll_s) with lw the PSIS log-weights of the ratios -ll; p_loo = lppd - elpd_loo; khat.  The tail length is
 * min(ceil(min(count / 5, 3 sqrt(count / reff))), count - 1), computed on the host once (*tail_len); the cutoff is an exact order
 * statistic (radix selection).  A term that is NaN or -inf is a BAD ratio: with fewer than tail_len + 1 others khat, elpd_loo
 * and p_loo are NaN.  count < 2: every output NaN.  One workgroup per observation; sums in an order fixed by the ordered list of
 * valid samples alone; the bits do not depend on scratch_bytes.
 * status [n], count as msx_predictive_batch's.  ll_out: NULL, or [n_obs][count] -- the pointwise matrix itself, refused
 * (MSX_ERR_RANGE) above MSX_POINTWISE_MATRIX_MAX bytes for n_obs x n.  scratch_bytes: 0 (256 MiB) or at least 8 * max(npix, n).
 * MSX_ERR_RANGE also: a tail over MSX_PSIS_TAIL_MAX (more than 1.8 M samples).  MSX_ERR_STATE: no products staged.
 * MSX_ERR_INVALID: null pointers, n < 1, ndim != 2 nspec + 2, reff not > 0.  A refused call writes nothing.                   */
#define MSX_POINTWISE_MATRIX_MAX 1073741824
int msx_pointwise_nobs(msx_ctx *ctx, int64_t *npix, int32_t *n_contrast, int32_t *n_phot);
int msx_predictive_pointwise(msx_ctx *ctx, const double *theta, int64_t n, int32_t ndim, double reff, int64_t scratch_bytes,
                             double *out, int32_t *status, int64_t *count, int64_t *tail_len, double *ll_out);
/* The same over rows[0:n][discard::thin] of a device chain, member m's flat sample (N_m = n' W_m) evaluated with ctxs[m] as in
 * msx_series_predictive: out holds the members' [6][n_obs_m] one after the other, count / tail_len / worst_status [k] (the
 * latter two may be NULL), ll_out (or NULL) member m's [n_obs_m][count_m] at the start of its slot of n_obs_m * N_m doubles.
 * The bits are msx_predictive_pointwise's for the same samples.  MSX_ERR_RANGE: n past the rows held, an empty selection.      */
int msx_series_pointwise(msx_series *src, msx_ctx **ctxs, int64_t n, int64_t discard, int64_t thin, double reff,
                         int64_t scratch_bytes, double *out, int64_t *count, int64_t *tail_len, int32_t *worst_status, double *ll_out);

/* ---- the split pool, transformed: ranks, normal scores, folding, indicators ----------------------------
 * What rank-normalised R-hat, bulk / tail ESS and the Monte-Carlo standard errors (Vehtari et al. 2021) are made of;
 * mcmc_spec_amd/diagnostics.py is the definition.  The selection x = rows[0:n][discard::thin] (n' >= 4 rows) of src is
 * msx_series_acf's; h = n' / 2.  dst is another series on src's device with 2 nw walkers, ndim = ncols and members of 2 W_m
 * walkers: walker 2 w + half of dst receives, in rows 0 .. h - 1, the transformed rows [0, h) (half 0) or [n' - h, n') (half 1)
 * of source walker w -- msx_series_moments' half-chains as chains of their own; an odd n' leaves the middle row out.  dst grows
 * as msx_series_append grows a series and then holds exactly h rows, on which msx_series_order_stats (the IDENTITY series is
 * the split pool: its medians and quantiles), _hist, _read, _acf and msx_series_chain_acov work as on any series.  A member's
 * column is a SEGMENT of S = 2 W_m h values.  cols: coordinates or MSX_COL_RATIO codes, at most MSX_MAX_DIM.  Transforms:
 *   MSX_SPLIT_IDENTITY       x;
 *   MSX_SPLIT_RANKNORM       z = ndtri((r - 3/8) / (S + 1/4)), r the 1-based rank of x in its segment, ties sharing the mean of
 *                            their positions (twice a rank is an integer), -0 and +0 tied; ndtri is AS 241's PPND16 in
 *                            float64 + - * /, log and sqrt, the coefficients in diagnostics.ndtri's order;
 *   MSX_SPLIT_FOLD_RANKNORM  the same of |x - param[m * ncols + j]| (the caller's median of the segment);
 *   MSX_SPLIT_INDICATOR      1 where x <= param[m * ncols + j], 0 elsewhere, NaN for a NaN;
 *   MSX_SPLIT_RANK2          twice the rank itself, as a double (what the tests compare with 2 * rankdata).
 * A ranked segment that holds a non-finite value, or one distinct value, is NaN all over; nothing else is touched by it.  Ranks
 * come from a segmented radix sort of (key, position) pairs -- keys as msx_series_order_stats' -- in 8-bit passes of three
 * launches each (per-tile digit counts, scan, stable scatter); passes whose digit is the same all over every segment of a round
 * are dropped.  Ranks depend on the keys alone: the result has the same bits whatever the launch, the budget, or how the rows
 * arrived.  Scratch comes from src's scratch buffer: scratch_bytes (0: 256 MiB) bounds it, segments are sorted in as many rounds
 * as that needs, and MSX_ERR_RANGE refuses a budget below the largest segment's need (24 S bytes and its tables:
 * msx_split_scratch_bytes).  Synchronous, on src's stream; waits for nothing but the latest growth copies.
 * MSX_ERR_INVALID: a null series, dst == src or on another device, discard < 0, thin < 1, ncols < 1, cols NULL, an unknown
 * transform, param NULL where the transform reads it, scratch_bytes < 0.  MSX_ERR_STATE: a run in flight appends to dst.
 * MSX_ERR_RANGE: n past the rows held, fewer than 4 rows selected, an unknown column, more than MSX_MAX_DIM columns, a dst whose
 * walkers, members or ndim are not 2 nw, 2 W_m and ncols, a segment of 2^31 values or more, over 65,535 segments.  A refused call writes nothing.   */
#define MSX_SPLIT_IDENTITY 0
#define MSX_SPLIT_RANKNORM 1
#define MSX_SPLIT_FOLD_RANKNORM 2
#define MSX_SPLIT_INDICATOR 3
#define MSX_SPLIT_RANK2 4
int msx_series_split_transform(msx_series *src, int64_t n, int64_t discard, int64_t thin, const uint32_t *cols, int32_t ncols,
                               int32_t transform, const double *param, int64_t scratch_bytes, msx_series *dst);
/* the scratch one segment of S values needs (the smallest scratch_bytes msx_series_split_transform accepts for it)             */
int64_t msx_split_scratch_bytes(int64_t S);
/* The autocovariance of a series whose every walker is a chain (a dst of the call above), rows[0:n] (h = n >= 2), averaged over
 * each member's J chains: acov_out[(m * ncols + j) * nlag + t] = A(lag0 + t), A(t) = (1 / J) sum_chains (1 / h) sum_{i < h - t}
 * (y_i - m_c)(y_{i+t} - m_c); meanvar_out[m * ncols + j] = A(0) h / (h - 1); between_out = var (ddof 1) of the chains' means
 * m_c.  The sums are msx_series_acf's (the same kernels, the same order, fixed by h alone: identical bits for any lag tiling);
 * a chain's sums are then added in walker order.  cols: coordinates < ndim (no ratios), ncols <= MSX_MAX_DIM.  Needs
 * lag0 + nlag <= h.  MSX_ERR_INVALID: a null series or output, lag0 < 0, nlag < 1, ncols < 1, cols NULL.  MSX_ERR_RANGE: n past
 * the rows held or below 2, lags past h, a column >= ndim, more than MSX_MAX_DIM columns.                                       */
int msx_series_chain_acov(msx_series *s, int64_t n, int64_t lag0, int64_t nlag, const uint32_t *cols, int32_t ncols,
                          double *acov_out, double *meanvar_out, double *between_out);

/* ---- test hooks (used by tests/ only) ------------------------------------------------------------ */
/* MSX_HOOK_LINKED_FAULT: value != 0 makes the workgroups of the linked form skip their signal -- and the walkers of an
 * overlapped sampler run the publication of their new version -- so that every in-kernel wait runs into its bound;
 * takes effect at the next launch, without restaging                                                              */
#define MSX_HOOK_LINKED_FAULT 1
/* MSX_HOOK_PAIR_LEASES: value != 0 marks every scratch row of the pair form's spill path as leased (what a launch torn
 * down mid-spill would leave behind), 0 clears them: the next pair launch's spilling walkers must end with
 * MSX_W_HANDOVER inside the bound instead of hanging; synchronises                                                  */
#define MSX_HOOK_PAIR_LEASES 2
int msx_test_hook(msx_ctx *ctx, int32_t what, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* MSX_H */
