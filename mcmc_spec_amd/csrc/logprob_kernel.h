// logprob_kernel.h -- part of the single translation unit msx.hip (included there, in this order).
// THE HOT KERNEL logprob_kernel<NS,MAXT,GM,SH,PF,LK,R32,FULL,GIVEN> and the walker's last lines (walker_done).
#ifndef MSX_LOGPROB_KERNEL_H
#define MSX_LOGPROB_KERNEL_H

namespace {

__device__ __forceinline__ double nan_with_status(int st) {
    return __longlong_as_double(0x7ff8000000000000ll | (long long)(st & 0xff));
}
__device__ __forceinline__ int status_of_nan(double v) {  // 0 for anything that is not one of the NaNs above
    const long long b = __double_as_longlong(v);
    return ((b & 0x7ff8000000000000ll) == 0x7ff8000000000000ll && (b >> 63) == 0) ? (int)(b & 0xff) : 0;
}

// linked form: a store that is handed to another workgroup -- agent scope, i.e. written through the XCD's L2
__device__ __forceinline__ void publish_u64(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the walker's scalar arithmetic after the pixel loops, in ONE place: the fused kernel and the pair kernel
// (pair_kernel.h) must give a walker the same bits, so both call these and nothing else ---------------------------
// one pixel's contribution to the three fit sums of data / model against [1, u, u^2]      mft6.py:194-195
__device__ __forceinline__ void fit_accumulate(double m, double flux, double u, double &q0, double &q1, double &q2) {
    const double f = fast_div(flux, m);  // frac before the median scale, mft6.py:194
    const double f1 = f * u, f2 = f * (u * u);
    q0 += f; q1 += f1; q2 += f2;
}
// coefficients of the raw quadratic fit of data / model from the three fit sums (mft6.py:195; minv = inverse Gram matrix)
__device__ __forceinline__ void fit_coefs(const DevProblem &P, const double (&q)[3], double &c0, double &c1, double &c2) {
    c0 = P.minv[0] * q[0] + P.minv[1] * q[1] + P.minv[2] * q[2];
    c1 = P.minv[3] * q[0] + P.minv[4] * q[1] + P.minv[5] * q[2];
    c2 = P.minv[6] * q[0] + P.minv[7] * q[1] + P.minv[8] * q[2];
}
// one pixel's chi^2 term before the median's scale^2: (model - data / P(u))^2 / err^2      mft6.py:196,120
__device__ __forceinline__ double chi_term(double c0, double c1, double c2, double u, double f, double e, double xv, bool live) {
#pragma clang fp contract(off)
    // (no contraction: the term is a PRODUCT, added by the caller.  Where `live` is a compile-time true -- the pair kernel's
    // FULL variants -- nothing stands between this multiply and the caller's add any more, and a fused multiply-add there
    // would round differently from every variant that selects on `live`: a walker's bits must not depend on the variant.)
    const double poly = fma(fma(c2, u, c1), u, c0);
    const double r = xv - fast_div(f, poly);
    const double t = (r * r) * e;
    return live ? t : 0.0;
}
// the walker's value from its chi^2 sum (fused modes: before scale^2), the two medians and the recipe's scalars
__device__ __forceinline__ double fused_total(const DevProblem &P, double chi_sum, double med_data, double med_model, int npix,
                                              double chi_extra) {
    const double scale = fast_div(med_data, med_model);  // mft6.py:1173
    const double tot = chi_sum * (scale * scale);
    const double iic = fast_div(tot, (double)npix);                // mft6.py:1179
    return iic * (double)(P.nc + P.np) + chi_extra;                // mft6.py:1191
}
__device__ __forceinline__ double value_of_total(int mode, double total, double lp) {
    if (mode == MSX_MODE_CHISQ) return total;                      // mft6.py:1198-1199
    return isnan(total) ? -INFINITY : lp + (-0.5 * total);          // mft6.py:1202-1205, 1470
}

// Last lines of a walker (one lane): publish the value and, for the device-resident sampler, apply the
// stretch move's accept rule  log(u) < (ndim-1) ln z + ln p(q) - ln p(s)  (NaN differences compare false,
// like -inf - -inf on the host) and record the walker's row of the chain: a walker only changes in its
// own half-step, so its row after the step is written here.
// What the walker's last lines read of the problem, copied out of the by-value kernel argument ONCE per kernel (smp_view):
// walker_done is inlined at every exit of the kernel, and a by-value DevProblem with too many uses is no longer
// recognised as read-only by the compiler, which then keeps a private copy of all 1.2 KB of it in scratch
// (tests/test_abi.py watches the variants' scratch size).
struct SmpView {
    unsigned long long *clk_probe;  // non-null: a probe launch (see DevProblem)
    int32_t smp_on, smp_defer, smp_overlap, linked_fault;
    int64_t smp_stride;
    double *smp_coords, *smp_logp, *smp_chain_row, *smp_lp_row;
    int64_t *smp_naccept;
    int32_t *smp_worst;
    unsigned long long *smp_gran;
    int64_t smp_gwalkers;
};
__device__ __forceinline__ SmpView smp_view(const DevProblem &P, bool probe) {
    return {probe ? P.clk_probe : nullptr, P.smp_on, P.smp_defer, P.smp_overlap, P.linked_fault, P.smp_stride, P.smp_coords, P.smp_logp, P.smp_chain_row,
            P.smp_lp_row, P.smp_naccept, P.smp_worst, P.smp_gran, P.smp_gwalkers};
}
__device__ __forceinline__ void walker_done(const SmpView &P, const WalkerDesc &D, int64_t wk, int ndim, double out, int st,
                            double *__restrict__ logp, int32_t *__restrict__ status) {
    // an error status travels inside the NaN it produces (payload = MSX_W_*): the sharded sampler's all-gather
    // carries log-probabilities only, and every rank must learn of every rank's failures
    logp[wk] = (st > MSX_W_REJECT) ? nan_with_status(st) : out;
    status[wk] = st;
    if (P.clk_probe && wk < kProbeWalkers) {
        P.clk_probe[wk * 4 + 2] = wall_clock64();
        P.clk_probe[wk * 4 + 3] = (unsigned long long)__builtin_readcyclecounter();
    }
    if (!P.smp_on) return;
    if (st > MSX_W_REJECT) atomicMax(P.smp_worst, st);
    if (P.smp_defer) return;  // sharded: sampler_apply_kernel finishes the move after the all-gather
    const int64_t s = D.smp_s;
    const double lnpdiff = (D.smp_zfac + out) - D.smp_old;
    const bool acc = D.smp_logu < lnpdiff;
    if (P.smp_overlap) {
        // Overlapped half-steps: the next half-step's workgroups are already resident and poll for THIS walker's next
        // version.  What they read goes out as tagged granules (DevProblem::smp_gran): every word {32 bits | new version}
        // by one agent-scope store (through the L2, like the linked form's partials), into the buffer of the new version's
        // parity -- accepted or not: the other buffer still holds what workgroups of the half-steps in flight may be
        // reading.  No wait for the stores' acknowledgements and no flag behind them: a word that shows the version IS the
        // data.  (Rounds 1-3: data, vmcnt(0), then a version word; the reader polled the word, acquired and fetched the
        // data -- two more trips through the fabric per hand-over.)
        const unsigned int nv = D.smp_ver + 1u;
        const double newlp = acc ? out : D.smp_old;
        const long long nacc = D.smp_nacc + (acc ? 1 : 0);
        // (test hook: nobody publishes, so every wait of the following half-steps runs into its bound)
        if (!P.linked_fault) {
            unsigned long long *g = P.smp_gran + ((int64_t)(nv & 1u) * P.smp_gwalkers + s) * kGranPerWalker;
            for (int d = 0; d < ndim; ++d) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(acc ? D.theta[d] : D.smp_sv[d]);
                publish_u64(g + 2 * d, granule((unsigned int)(b >> 32), nv));
                publish_u64(g + 2 * d + 1, granule((unsigned int)b, nv));
            }
            const unsigned long long lb = (unsigned long long)__double_as_longlong(newlp);
            publish_u64(g + kGranLogp, granule((unsigned int)(lb >> 32), nv));
            publish_u64(g + kGranLogp + 1, granule((unsigned int)lb, nv));
            publish_u64(g + kGranNacc, granule((unsigned int)nacc, nv));
        }
        // ... and the plain arrays the host reads when the chunk is over (nobody on the device waits for these)
        double *row = P.smp_coords + (int64_t)(nv & 1u) * P.smp_stride + s * ndim;
        for (int d = 0; d < ndim; ++d) {
            const double v = acc ? D.theta[d] : D.smp_sv[d];
            row[d] = v;
            P.smp_chain_row[s * ndim + d] = v;
        }
        P.smp_logp[s] = newlp;
        P.smp_naccept[s] = nacc;
        P.smp_lp_row[s] = newlp;
        return;
    }
    if (acc) {
        P.smp_logp[s] = out;
        P.smp_naccept[s] = D.smp_nacc + 1;
    }
    for (int d = 0; d < ndim; ++d) {
        const double v = acc ? D.theta[d] : D.smp_sv[d];
        if (acc) P.smp_coords[s * ndim + d] = v;
        P.smp_chain_row[s * ndim + d] = v;
    }
    P.smp_lp_row[s] = acc ? out : D.smp_old;
}

// The chi^2 terms that ride along the median's pass over the model vector (see phase B in the kernel): u, data flux
// and 1/err^2 by table ELEMENT (two pixels 256 apart) -- the four pixels of a trip are the elements (base >> 1) + tid
// and + MAXT (pass_pixel).  u and flux come from LDS with PF, else from the tables; 1/err^2 always from its table.
// AHEAD = global loads run one trip ahead of their use, into the register set of the other parity (median.h,
//         pass_trips): the one-workgroup-per-CU variants, which have the registers and few waves to hide a load
//         behind.  Otherwise a trip's loads are issued at its start, before the trip's LDS reads.
// ALWAYS = the terms are wanted whatever `on` says (the early-histogram median only runs in the fused modes): no
//         run-time flag inside the pass, whose merge points would bring register copies back.
// Holds plain pointers, never a reference to the by-value kernel argument (see DevProblem).
// FLDS = the data flux (alone) comes from LDS: the linked form, whose workgroup has room for one more vector of its segment.
// FULL = every element / pixel of every trip is valid (the spectrum is whole trips: logprob_kernel's FULL): no clamps, no selects
template <int MAXT, bool PF, bool ALWAYS, bool AHEAD, bool FLDS = false, bool FULL = false>
struct ChiElem {
    static constexpr int VK = kMaxWaves / (MAXT / kWave);
    static constexpr int NSET = AHEAD ? 2 : 1;
    const double2 *u2, *f2, *iv2;
    int ne, npix;
    double c0, c1, c2;
    double acc[VK];  // one per slot this lane holds (see phase A and pass_pixel)
    bool on;
    double *red0;    // [MAXT] LDS: the lanes' partials of the chi^2 sum
    double2 nu[NSET][2], nf[NSET][2], nv[NSET][2];  // [register set][element of the trip]
    double tot_run;  // wave 0: the chi^2 sum over the segments finished so far (see phase A)
    template <int SET>
    __device__ __forceinline__ void load_trip(int base) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int e = (base >> 1) + j * MAXT + (int)threadIdx.x;
            e = (FULL || e < ne) ? e : ne - 1;
            const unsigned int o16 = (unsigned int)e << 4;
            nv[SET][j] = ld_off(iv2, o16);
            if (!PF) { nu[SET][j] = ld_off(u2, o16); if (!FLDS) nf[SET][j] = ld_off(f2, o16); }
        }
    }
    __device__ __forceinline__ void prime_from(int base) {  // before a pass that starts at pixel `base`
        if (!ALWAYS && !on) return;
        if (AHEAD) load_trip<0>(base);
    }
    __device__ __forceinline__ void prime() { prime_from(0); }  // before the pass (and before whatever the caller does first)
    template <int PAR>
    __device__ __forceinline__ void begin_trip(int base) {
        if (!ALWAYS && !on) return;
        if (!AHEAD) load_trip<0>(base);
    }
    // the four pixels of one trip (pass_pixel order)
    template <int PAR>
    __device__ __forceinline__ void process4(int base, const int (&p)[4], const double (&xv)[4]) {
        if (!ALWAYS && !on) return;
        constexpr int SET = AHEAD ? PAR : 0;
        double2 cu[2], cf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (PF) {
                int e = (base >> 1) + j * MAXT + (int)threadIdx.x;
                e = (FULL || e < ne) ? e : ne - 1;
                cu[j] = u2[e]; cf[j] = f2[e];  // LDS
            } else {
                cu[j] = nu[SET][j]; cf[j] = nf[SET][j];
                if (FLDS) {
                    int e = (base >> 1) + j * MAXT + (int)threadIdx.x;
                    e = (FULL || e < ne) ? e : ne - 1;
                    cf[j] = f2[e];  // LDS (f2 is the workgroup's staged copy, indexed by the element's own number)
                }
            }
        }
        // (FULL has no clamp inside load_trip: the trip requested behind the LAST one would lie past the tables' end --
        // it asks for the current trip again instead; uniform, two scalar instructions)
        if (AHEAD) load_trip<AHEAD ? 1 - PAR : 0>((FULL && base + 4 * MAXT >= npix) ? base : base + 4 * MAXT);
        const double u[4] = {cu[0].x, cu[0].y, cu[1].x, cu[1].y}, f[4] = {cf[0].x, cf[0].y, cf[1].x, cf[1].y};
        const double e[4] = {nv[SET][0].x, nv[SET][0].y, nv[SET][1].x, nv[SET][1].y};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[k & (VK - 1)] += chi_term(c0, c1, c2, u[k], f[k], e[k], xv[k], FULL || p[k] < npix);  // up to scale^2
        }
        // end of a segment of the canonical sum (8192 pixels), more pixels to come: fold it in.  (Uniform: every
        // thread of the workgroup walks the same trips.)
        const int next = base + 4 * MAXT;
        if ((next & (2 * kSegElems - 1)) == 0 && next < npix) {
            red0[threadIdx.x] = lane_partial<VK>(acc);
#pragma unroll
            for (int k = 0; k < VK; ++k) acc[k] = 0.0;
            __syncthreads();
            if ((threadIdx.x >> 6) == 0) tot_run += reduce_published<MAXT>(red0, (int)threadIdx.x & 63);
            __syncthreads();
        }
    }
    __device__ __forceinline__ void flush(BlockScratch &) {  // one partial per lane; wave 0 finishes at the very end
        if (!ALWAYS && !on) return;
        red0[threadIdx.x] = lane_partial<VK>(acc);
    }
};

// ------------------------------------------------------------------------------------------------
// THE HOT KERNEL: one workgroup per walker.
//   phase 0    one wave per star builds the walker's recipe from register-resident tables (prior gate, A1, A2,
//              A4); an idle wave computes the Gaussian prior terms (f1); with PF the remaining waves stage
//              pixel statics in LDS
//   phase A    blend + redden + resample into the model vector (LDS); fit sums, value range and the median's
//              logarithmic histogram are accumulated on the way                       (A2, A4, A7, A8.1)
//              wave 0 computes the contrast / photometry terms (A5/A6) while it waits at phase A's barrier
//   phase B+C  exact median (per-wave bin scan -> ONE pass that also carries the chi^2 terms and gathers the
//              median bin's candidates -> wave-0 rank); scale, chi^2 and the combine   (A8.2, A8.3, A9)
//              vectors the early histogram cannot handle take block_median (linear bins, radix fallback); the
//              pre-optimiser modes keep a separate chi^2 pass (phase C proper)
// ------------------------------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];

// MAXT = the workgroup size the variant is compiled for and launched with: 256 (three workgroups per CU, capped at
//        168 VGPRs) or 512 (one per CU; with SH: two per CU, capped at 128 VGPRs).
// GM = the walker's model vector lives in global memory (spectra longer than ~17k pixels) instead of LDS.
// SH = 512-thread variant that shares its CU with a second workgroup (MSX_BLOCK_512_SHARED).
// PF = the walker-independent pixel vectors u and data flux are staged in LDS, in the tables' own layout, by the waves
//      that idle during the recipe; the blend loop and the chi^2 pass read them there instead of pulling them through
//      the CU's L2 port, twice (one workgroup per CU only: 3 npix doubles of LDS).
// LK = the LINKED form of the same kernel, for few walkers x long spectra (one workgroup per walker leaves CUs idle
//      and is a chain of 16,384 pixels' latencies): one workgroup per (walker, SEGMENT of 8192 pixels), all of them
//      equals.  Each builds the recipe, blends ITS segment into LDS (fit sums, value range, histogram on the way) and
//      leaves those partials in P.segparts; the walker's workgroups MEET (an arrival counter per walker, agent-scope
//      release / acquire; the wait is bounded by kHandoverTicks, then the walker fails with MSX_W_HANDOVER and the
//      context's linked form is POISONED: see below); every one of them then adds up the partials in segment order --
//      exactly the fused kernel's association -- locates the median's bin from the summed histogram and makes the
//      chi^2 / candidates pass over its own segment; chi^2 sum and candidates go to P.segparts again, and whichever
//      workgroup ARRIVES LAST at the second meeting point (nobody waits there) ranks the candidates of all segments,
//      adds the chi^2 sums in segment order and finishes the walker.  The model vector never leaves the CUs; a
//      hand-over is 8 KB of counters and a few numbers.  (Vectors the early histogram cannot handle: every segment
//      goes to the scratch row and the last arrival runs block_median over it, as the GM variants do.)
//      Block = (walker / 8) * 8 S + segment * 8 + walker % 8: a walker's workgroups are 8 blocks apart -- blocks go
//      round-robin over the 8 XCDs, so they share an XCD (one L2: the hand-over's data never leaves it) and follow
//      each other in that XCD's dispatch queue: the workgroups of every walker dispatched earlier are resident or
//      done, so the wait needs no co-residency guarantee beyond in-order dispatch.
//      The counter is never reset: a launch adds 2 S to it, and a workgroup reads the launch's base off the value its
//      own first increment returns (old - old % 2S).  (64 bits: it does not wrap.)
//
// TABLE LAYOUT.  A CU pulls data from L2 at ~32 B per clock when every lane loads 16 bytes, and no faster per
// instruction when lanes load less -- so every per-pixel table the blend reads is stored in ELEMENTS of two pixels,
// element e = pixels {pa, pa + 256}, pa = (e >> 8) * 512 + (e & 255): a lane's 16-byte load (8-byte for the float32
// table) brings both of its pixels, for workgroups of 256 and of 512 threads alike.  Per grid node and pixel the
// tables hold R = lo + (hi - lo) t (float64) and H = hi t (float32): see blend_pixel_rh (blend.h).
// R32 = the R table is stored in FLOAT32 (msx_set_grid_storage(MSX_STORE_F32): 8 instead of 12 bytes per node-pixel through
//       the CU's L2 port, whose limit the blend runs at) and widened to float64 in the registers: the arithmetic is the
//       same float64 chain, the grid values carry 2^-24 instead of 2^-53.  A SEPARATELY LABELLED precision (SURVEY 8b's
//       store_dtype), never the default; fused binaries only.
// FULL = the spectrum is whole trips of the variant with no pad pixels (npix == 2 npair, npair a multiple of the trip:
//        BASELINE's 4096 pixels): every lane of every trip holds live pixels, so the clamps of element and pixel indices,
//        the per-pixel validity compares and their selects can be compiled out -- bit 0: of the blend, bit 1: of the chi^2
//        pass and the candidates' gather.  Same arithmetic on the same pixels: same bits (the launcher picks it; msx.hip,
//        plan_launch).  Which bits pay was measured per workgroup size (same box, alternating runs): the 256-thread
//        variants gain from both (2,048 walkers 63.3 -> 60.4 us), the 512-thread headline variant gains from the chi^2
//        pass's (14.63 -> 14.36 us per step) and LOSES with the blend's (14.67 -> 14.96: the loads' order changed); the
//        two-per-CU and the linked 512-thread variants likewise (config 4's share 26.2 -> 25.8 us with bit 1, 26.4 with both).
// GIVEN = the model values are not blended here: the in-path broadening kernels (inpath_kernels.h) have left them in
//        P.given[walker][pixel]; everything else -- recipe (for the walker's status, its prior and band terms), fit sums,
//        median, chi^2 pass -- is this kernel's.  One variant: 512 threads, quad trips.
template <int NS, int MAXT, bool GM = false, bool SH = false, bool PF = false, bool LK = false, bool R32 = false, int FULL = 0,
          bool GIVEN = false>
// (second launch bound = waves per SIMD the register allocation must leave room for: k workgroups of T threads per
// CU <=> k T / 256.  256 threads: three per CU = 168 VGPRs; 512 threads sharing a CU: two per CU = four waves per
// SIMD = 128 VGPRs.)
__global__ void __launch_bounds__(MAXT, MAXT == 256 ? (SH ? 2 : 3) : (MAXT == 512 && SH) ? 4 : 1)
logprob_kernel(const double *theta, const unsigned char *__restrict__ rblk, int niso_nt, int ng_mode_fast, int64_t n,
               double gate_tmin, double gate_tmax, const SmpRec *__restrict__ smp_rec, DevProblem P,
               double *__restrict__ logp, int32_t *__restrict__ status) {
#include "logprob_body.h"
}

// ------------------------------------------------------------------------------------------------
// Sharded device-resident sampler (SURVEY §8e + f2): every rank keeps the whole ensemble in HBM and evaluates its
// block of the half-step's proposals with smp_defer = 1; the only thing that crosses xGMI is ONE all-gather of
// log p(q) (ns / G float64 per rank).  This kernel then finishes the half-step on every rank, for every active
// walker: the proposal is rebuilt from the resident state (its inputs -- the walker itself and its partner in the
// complementary half -- are untouched until now, and the expression is the fused kernel's, contraction off), the
// accept rule is the fused kernel's, so all ranks stay bit-identical to each other and to the one-GPU chain.
// ------------------------------------------------------------------------------------------------
__global__ void sampler_apply_kernel(DevProblem P, const double *__restrict__ newlp, int64_t ns, int ndim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const int64_t si = P.smp_sidx[i], ci = P.smp_partner[i];
    const double zz = P.smp_zz[i];
    const double out = newlp[i];
    const int st = status_of_nan(out);
    if (st > MSX_W_REJECT) atomicMax(P.smp_worst, st);
    const double old = P.smp_logp[si];
    const double lnpdiff = (P.smp_zfac[i] + out) - old;
    const bool acc = P.smp_logu[i] < lnpdiff;  // NaN differences compare false, like the host loop
    for (int d = 0; d < ndim; ++d) {
#pragma clang fp contract(off)
        const double sv = P.smp_coords[si * ndim + d];
        const double cv = P.smp_coords[ci * ndim + d];
        const double diff = cv - sv;
        const double prod = diff * zz;
        const double qv = cv - prod;
        const double v = acc ? qv : sv;
        if (acc) P.smp_coords[si * ndim + d] = v;
        P.smp_chain_row[si * ndim + d] = v;
    }
    if (acc) {
        P.smp_logp[si] = out;
        P.smp_naccept[si] = P.smp_naccept[si] + 1;
    }
    P.smp_lp_row[si] = acc ? out : old;
}

// ------------------------------------------------------------------------------------------------
// The stretch move's randomness, drawn ON THE DEVICE (emcee's move as mft6.py:1491-1494 drives it): a
// COUNTER-BASED generator -- every number is a pure function of (seed, iteration, stream, index), so a chunk is one
// launch, any rank of a sharded run draws the same numbers without a broadcast, and the host can restate the stream
// (mcmc_spec_amd/sampler.py::counter_draws) to check it.  The generator is SplitMix64's output function over the
// counter sequence seed * K + (ctr + 1) * gamma (Steele, Lea & Flood 2014: the stream a SplitMix64 instance produces).
// One workgroup per iteration:
//   stream 0      one 64-bit key per walker; the walkers sorted by (key, index) are the iteration's random permutation,
//                 its first half the first half-step's walkers, its second half their complementary ensemble (and the
//                 other way round for the second half-step) -- emcee's randomised split
//   streams 1..6  per half-step h and position j: u_z -> z = ((a - 1) u_z + 1)^2 / a, u_p -> partner floor(u_p ns),
//                 u_a -> ln u_a of the accept draw
// and writes the chunk's arrays exactly as the host-fed entry point uploads them (msx.hip, chunk_prepare).
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned long long counter_mix64(unsigned long long seed, unsigned long long it, unsigned int stream,
                                                           unsigned int index) {
    const unsigned long long ctr = (it << 28) + ((unsigned long long)stream << 24) + (unsigned long long)index;
    unsigned long long x = seed * 0xD1342543DE82EF95ull + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__host__ __device__ inline double counter_uniform(unsigned long long seed, unsigned long long it, unsigned int stream, unsigned int index) {
    return (double)(counter_mix64(seed, it, stream, index) >> 11) * (1.0 / 9007199254740992.0);  // [0, 1), 53 bits
}
constexpr int kDrawMaxWalkers = 4096;  // (key, index) pairs of one iteration sorted in LDS: 48 KB
constexpr int kDrawThreads = 256;
// One iteration `it` of one ensemble of nw walkers keyed by `seed`, by the whole workgroup (kDrawThreads threads): the keys,
// the LDS sort, and per half-step h and position j the entry o0 + h * hstride + j of the chunk's arrays.  `it` is the
// generator's counter only -- the ABSOLUTE iteration of the stream, which goes on across runs; the records' hand-over
// versions of an overlapped run count from the RUN's start (msx_sampler_begin zeroes the walkers' versions) and come from
// `ver_it`, the iteration's number within the run (run_pack's k).  sidx and cidx stay the ensemble's own indices; the
// resolved partner and the records' si / ci -- what the kernels dereference -- are woff + the ensemble's own index (a
// target group's member: its offset in the group's ensemble), as run_pack leaves them.  resolve != 0: `partner` receives
// cidx[partner] (the ensemble index of the complementary walker: what the kernels read); 0: the raw index into the
// complementary half (what the host loop consumes)
__device__ __forceinline__ void draw_iteration(unsigned long long seed, double a, unsigned long long it, unsigned long long ver_it, int nw, int32_t ndim,
                                               int32_t resolve, int32_t overlap, int32_t woff, int64_t o0, int64_t hstride, int32_t *__restrict__ sidx,
                                               int32_t *__restrict__ cidx, int32_t *__restrict__ partner, double *__restrict__ zz,
                                               double *__restrict__ zfac, double *__restrict__ logu, SmpRec *__restrict__ rec) {
    __shared__ unsigned long long key[kDrawMaxWalkers];
    __shared__ int32_t idx[kDrawMaxWalkers];
    const int ns = nw / 2;
    int npad = 1;
    while (npad < nw) npad <<= 1;
    for (int i = threadIdx.x; i < npad; i += kDrawThreads) {
        key[i] = i < nw ? counter_mix64(seed, it, 0u, (unsigned int)i) : ~0ull;  // (pads sort last: index >= nw breaks the tie)
        idx[i] = i;
    }
    __syncthreads();
    // bitonic sort of (key, index), ascending
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += kDrawThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ka = key[i], kb = key[l];
                    const int32_t ia = idx[i], ib = idx[l];
                    const bool a_gt_b = ka > kb || (ka == kb && ia > ib);
                    const bool up = (i & k) == 0;
                    if (a_gt_b == up) { key[i] = kb; key[l] = ka; idx[i] = ib; idx[l] = ia; }
                }
            }
            __syncthreads();
        }
    }
    // the two half-steps of this iteration
    for (int t = threadIdx.x; t < 2 * ns; t += kDrawThreads) {
#pragma clang fp contract(off)
        const int h = t / ns, j = t - h * ns;
        const int32_t s_w = idx[h * ns + j];                    // the moving walker
        const int32_t *comp = idx + (1 - h) * ns;               // the complementary half
        const double uz = counter_uniform(seed, it, 1u + 3u * (unsigned int)h, (unsigned int)j);
        const double up = counter_uniform(seed, it, 2u + 3u * (unsigned int)h, (unsigned int)j);
        const double ua = counter_uniform(seed, it, 3u + 3u * (unsigned int)h, (unsigned int)j);
        const double t1 = (a - 1.0) * uz + 1.0;
        const double z = (t1 * t1) / a;                         // emcee: ((a - 1) u + 1)^2 / a
        int pj = (int)(up * (double)ns);
        pj = pj < ns - 1 ? pj : ns - 1;
        const int64_t o = o0 + h * hstride + j;
        sidx[o] = s_w;
        cidx[o] = comp[j];
        partner[o] = resolve ? woff + comp[pj] : pj;
        zz[o] = z;
        zfac[o] = ((double)ndim - 1.0) * log(z);
        logu[o] = log(ua);                                      // (u = 0: -inf, accepted by nothing -- like log(random()))
        if (rec) {
            SmpRec r;
            r.si = woff + s_w; r.ci = woff + comp[pj]; r.zz = z;
            r.ver_own = overlap ? (uint32_t)ver_it : 0u;
            r.ver_partner = overlap ? (uint32_t)(ver_it + (unsigned long long)h) : 0u;
            rec[o] = r;
        }
    }
}

// one workgroup per iteration of the chunk; the arrays [nsteps][2][nw / 2].  first_iter: the stream's (absolute) iteration of
// the chunk's first step; ver_first: that step's number within the run (the versions' base; unused unless overlap)
__global__ void __launch_bounds__(kDrawThreads)
sampler_draw_kernel(unsigned long long seed, double a, int64_t first_iter, int64_t ver_first, int64_t nw, int32_t ndim, int32_t resolve, int32_t overlap,
                    int32_t *__restrict__ sidx, int32_t *__restrict__ cidx, int32_t *__restrict__ partner, double *__restrict__ zz,
                    double *__restrict__ zfac, double *__restrict__ logu, SmpRec *__restrict__ rec) {
    const int64_t st = blockIdx.x;  // iteration of the chunk
    const int64_t ns = nw / 2;
    draw_iteration(seed, a, (unsigned long long)(first_iter + st), (unsigned long long)(ver_first + st), (int)nw, ndim, resolve, overlap, 0,
                   st * 2 * ns, ns, sidx, cidx, partner, zz, zfac, logu, rec);
}

// The same for a target group's run (msx_group_sampler_enqueue_drawn): grid (nsteps, k), one workgroup per iteration of the
// chunk and MEMBER.  Member m draws from its own seed with its own walker count -- the numbers sampler_draw_kernel gives
// that target alone -- and writes them where the host-fed chunk carries them: entry astart[m] + j of each half-step's
// ns_total, sidx / cidx member-local, the resolved partner and the records' si / ci the group's (off[m] + the member's own),
// versions 0 (plain launches).
struct GroupDrawTable {  // by value: a drawn chunk uploads nothing
    unsigned long long seed[MSX_MAX_GROUP];
    int32_t nw[MSX_MAX_GROUP], off[MSX_MAX_GROUP], astart[MSX_MAX_GROUP];
};
__global__ void __launch_bounds__(kDrawThreads)
group_draw_kernel(GroupDrawTable T, double a, int64_t first_iter, int32_t ndim, int64_t ns_total, int32_t *__restrict__ sidx,
                  int32_t *__restrict__ cidx, int32_t *__restrict__ partner, double *__restrict__ zz, double *__restrict__ zfac,
                  double *__restrict__ logu, SmpRec *__restrict__ rec) {
    const int64_t st = blockIdx.x;
    const int m = blockIdx.y;
    draw_iteration(T.seed[m], a, (unsigned long long)(first_iter + st), 0ull, T.nw[m], ndim, 1, 0, T.off[m], st * 2 * ns_total + T.astart[m],
                   ns_total, sidx, cidx, partner, zz, zfac, logu, rec);
}

}  // namespace

#endif  // MSX_LOGPROB_KERNEL_H
