// group_tempered_run.h -- part of the single translation unit msx.hip (included there, at the end of its extern "C" block).
// The host side of parallel tempering for a target group (include/msx.h, msx_group_tempered_* and msx_group_ladder_*;
// group_tempered_kernels.h).  msx_tempered_*'s pipeline with a target axis: K targets x T rungs are the
// K T members of one ensemble in the general layout, member m = k T + t with counts[k] walkers, and an iteration is
//   step(propose 0) ; prior ; like ; step(apply 0, propose 1) ; prior ; like ; step(apply 1) ; swap [; adapt]
// for ALL targets, `prior` / `like` the unchanged group launch (msx_group_logprob_batch_dev) over T counts[k] / 2 proposals of
// target k.  Plain launches on the run's own stream; nothing allocates or synchronises after begin (a growing series apart).

struct GroupTemperedRun {
    int32_t K = 0, T = 0, M = 0, ndim = 0;   // M = K T members
    std::vector<int64_t> nw;                 // [K] walkers per rung of target k
    std::vector<int64_t> eval_counts;        // [K] T nw[k] / 2: the group launch's counts
    int64_t W = 0, H = 0, SW = 0, max_nw = 0, cap_steps = 0;   // walkers, proposals per half-step, swap draws per iteration
    bool failed = false;                     // an enqueue failed part-way, or a member went away: only the run's end from here on
    bool enqueued = false;
    struct msx_series *s_chain = nullptr, *s_dens = nullptr;
    int64_t series_row = 0;
    std::vector<double> beta;                // [M] the ladders the run began with
    MoveMembers Mh, Mw;                      // the members' places; nh: the half (the step) / the walkers (the draw)
    GroupLadderTable G;
    bool adaptive = false;
    GroupAdaptTable P;
    char *d_state = nullptr;
    double *d_coords = nullptr, *d_ll = nullptr, *d_lpr = nullptr, *d_q = nullptr, *d_new_lpr = nullptr, *d_new_ll = nullptr, *d_ladder = nullptr;
    int64_t *d_nacc = nullptr;
    unsigned long long *d_nswap = nullptr, *d_prev = nullptr;
    long long *d_kstate = nullptr;           // [K][2]: k, skipped
    int32_t *d_st_lpr = nullptr, *d_st_ll = nullptr;
    hipStream_t stream = nullptr, copy = nullptr, up = nullptr;
    struct Slot {
        char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
        hipEvent_t in_ready = nullptr, kernels_done = nullptr, out_ready = nullptr;
        int64_t nsteps = 0;
        bool busy = false, collected = false;
    } slot[2];
    // a chunk of st iterations in its slot, laid out for its own length:
    //   in  [g | fac | logu  (st 2 H doubles each) | swap_logu (st SW doubles) | sidx | cidx | c1 | c2 (int32, st 2 H) | kind (st M)]
    //   out [chain st W ndim | ll st W | lpr st W | naccept W (int64) | nswap MSX_MAX_GROUP (int64) | worst MSX_MAX_GROUP (int32)
    //        | beta_chain st M (doubles): an adaptive run's only, though the slots always have room for it]
    int64_t entries(int64_t st) const { return st * 2 * H; }
    size_t in_bytes(int64_t st) const { return sizeof(double) * (size_t)(3 * entries(st) + st * SW) + sizeof(int32_t) * (size_t)(4 * entries(st) + st * M); }
    size_t fixed_out_bytes(int64_t st) const {
        return sizeof(double) * (size_t)(st * W * (ndim + 2)) + sizeof(int64_t) * (size_t)(W + MSX_MAX_GROUP) + sizeof(int32_t) * MSX_MAX_GROUP;
    }
    size_t out_bytes(int64_t st) const { return fixed_out_bytes(st) + (adaptive ? sizeof(double) * (size_t)(st * M) : 0); }
    size_t cap_out_bytes() const { return fixed_out_bytes(cap_steps) + sizeof(double) * (size_t)(cap_steps * M); }
};

struct GroupTemperedIn {
    double *g, *fac, *logu, *swap_logu;
    int32_t *sidx, *cidx, *c1, *c2, *kind;
};
static GroupTemperedIn group_tempered_in(const GroupTemperedRun *r, char *base, int64_t st) {
    const int64_t L = r->entries(st);
    GroupTemperedIn p;
    p.g = (double *)base; p.fac = p.g + L; p.logu = p.fac + L; p.swap_logu = p.logu + L;
    p.sidx = (int32_t *)(p.swap_logu + st * r->SW); p.cidx = p.sidx + L; p.c1 = p.cidx + L; p.c2 = p.c1 + L; p.kind = p.c2 + L;
    return p;
}
struct GroupTemperedOut {
    double *chain, *ll, *lpr;
    int64_t *nacc, *nswap;
    int32_t *worst;
    double *betas;   // beta_chain [st][M]
};
static GroupTemperedOut group_tempered_out(const GroupTemperedRun *r, char *base, int64_t st) {
    const int64_t rows = st * r->W;
    GroupTemperedOut p;
    p.chain = (double *)base; p.ll = p.chain + rows * r->ndim; p.lpr = p.ll + rows;
    p.nacc = (int64_t *)(p.lpr + rows); p.nswap = p.nacc + r->W; p.worst = (int32_t *)(p.nswap + MSX_MAX_GROUP);
    p.betas = (double *)(p.worst + MSX_MAX_GROUP);
    return p;
}

// a member's problem is about to go (free_problem): let the launches that read its tables finish
static void group_tempered_drain(msx_group *g) {
    if (g->trun && g->trun->stream) (void)hipStreamSynchronize(g->trun->stream);
}

static void group_tempered_free(msx_group *g) {
    GroupTemperedRun *r = g->trun;
    if (!r) return;
    (void)hipSetDevice(g->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
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
    if (r->s_chain) r->s_chain->gtrun = nullptr;  // (the series outlive the run)
    if (r->s_dens) r->s_dens->gtrun = nullptr;
    if (r->stream) (void)hipStreamDestroy(r->stream);
    if (r->copy) (void)hipStreamDestroy(r->copy);
    if (r->up) (void)hipStreamDestroy(r->up);
    delete r;
    g->trun = nullptr;
}

// a series is being destroyed while this run appends to it (msx_series_destroy): detach it
static void group_tempered_detach(msx_series *sr) {
    GroupTemperedRun *r = sr->gtrun;
    if (!r) return;
    if (r->s_chain == sr) r->s_chain = nullptr;
    if (r->s_dens == sr) r->s_dens = nullptr;
    sr->gtrun = nullptr;
}

// every member alive, still holding the problem the group snapshotted (group_check), and free for a group run
static int group_tempered_members_check(msx_group *g, const char *who, int32_t ndim) {
    int64_t total = 0;
    std::vector<int64_t> zeros(g->members.size(), 0);
    return group_check(g, who, MSX_MODE_LOGPRIOR, zeros.data(), ndim, &total);
}

int msx_group_tempered_begin(msx_group *g, int32_t ntemps, const double *betas, const int64_t *counts, int32_t ndim, int64_t max_chunk_steps,
                             const double *coords, const double *ll, const double *lpr) {
    if (!g) return MSX_ERR_INVALID;
    const std::string w("msx_group_tempered_begin");
    if (g->run || g->trun)
        return fail(g, MSX_ERR_STATE, w + ": a run is already in flight on this group (msx_group_sampler_end / msx_group_tempered_end)");
    const int64_t K = (int64_t)g->members.size();
    if (ntemps < 1 || K < 1 || K * (int64_t)ntemps > MSX_MAX_GROUP)
        return fail(g, MSX_ERR_INVALID, w + ": targets x rungs must lie in 1..MSX_MAX_GROUP (" + std::to_string(K) + " x " + std::to_string(ntemps) + " asked for)");
    if (!betas || !counts || !coords || !ll || !lpr || max_chunk_steps < 1) return fail(g, MSX_ERR_INVALID, w + ": bad arguments");
    if (int rc = group_tempered_members_check(g, "msx_group_tempered_begin", ndim)) return rc;
    for (int64_t k = 0; k < K; ++k) {
        const msx_ctx *c = g->members[(size_t)k];
        if (c->smp || c->tmp || c->opt_run)
            return fail(g, MSX_ERR_STATE, w + ": member " + std::to_string(k) + "'s context has a run of its own in flight");
        if (c->rccl_comm || !c->loop_peers.empty())
            return fail(g, MSX_ERR_STATE, w + ": member " + std::to_string(k) + "'s context holds a communicator; a tempered run is one GPU");
    }
    const int T = ntemps;
    int64_t W = 0, max_nw = 0;
    for (int64_t k = 0; k < K; ++k) {
        for (int t = 0; t < T; ++t) {
            const double b = betas[k * T + t];
            if (!std::isfinite(b) || !(b > 0.0) || (t > 0 && !(b < betas[k * T + t - 1])))
                return fail(g, MSX_ERR_INVALID, w + ": target " + std::to_string(k) + "'s betas must be finite, > 0 and strictly descending");
        }
        if (counts[k] < 2 || (counts[k] & 1))
            return fail(g, MSX_ERR_INVALID, w + ": target " + std::to_string(k) + " has " + std::to_string(counts[k]) +
                                                 " walkers per rung: a rung needs an even number, at least 2");
        W += (int64_t)T * counts[k];
        max_nw = std::max(max_nw, counts[k]);
        if (W > 0x7fffffff) return fail(g, MSX_ERR_INVALID, w + ": more than 2^31 - 1 walkers in one run");
    }
    if (W * (int64_t)ndim * max_chunk_steps > ((int64_t)1 << 31))
        return fail(g, MSX_ERR_INVALID, w + ": the chunk is too long for these ladders (walkers x ndim x steps <= 2^31)");
    for (int64_t i = 0; i < W; ++i)
        if (!std::isfinite(lpr[i]) || std::isnan(ll[i]))
            return fail(g, MSX_ERR_INVALID, w + ": an initial walker lies outside the prior (lpr not finite) or its ll is NaN");
    HIP_TRY(g, hipSetDevice(g->device));
    GroupTemperedRun *r = new GroupTemperedRun;
    g->trun = r;
    r->K = (int32_t)K; r->T = T; r->M = (int32_t)(K * T); r->ndim = ndim; r->W = W; r->H = W / 2; r->max_nw = max_nw; r->cap_steps = max_chunk_steps;
    r->beta.assign(betas, betas + K * T);
    memset(&r->Mh, 0, sizeof(r->Mh)); memset(&r->Mw, 0, sizeof(r->Mw)); memset(&r->G, 0, sizeof(r->G)); memset(&r->P, 0, sizeof(r->P));
    int64_t off = 0, soff = 0;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t n = counts[k];
        r->nw.push_back(n);
        r->eval_counts.push_back((int64_t)T * n / 2);
        r->G.nw[k] = (int32_t)n; r->G.woff[k] = (int32_t)off; r->G.soff[k] = (int32_t)soff;
        r->P.nw[k] = (double)n;
        for (int t = 0; t < T; ++t) {
            const int64_t m = k * T + t;
            r->Mh.astart[m] = r->Mw.astart[m] = (int32_t)(off / 2);
            r->Mh.off[m] = r->Mw.off[m] = (int32_t)off;
            r->Mh.nh[m] = (int32_t)(n / 2); r->Mw.nh[m] = (int32_t)n;
            off += n;
        }
        soff += (int64_t)(T - 1) * n;
    }
    r->SW = soff;
    const int64_t H = r->H, M = r->M;
    // [coords | ll | lpr | q | new_lpr | new_ll | ladder (doubles) | nacc | nswap | prev | kstate (64 bit) | st_lpr | st_ll (int32)]
    const size_t state_bytes = sizeof(double) * (size_t)(W * ndim + 2 * W + H * ndim + 2 * H + MSX_MAX_GROUP) +
                               sizeof(int64_t) * (size_t)(W + 4 * MSX_MAX_GROUP) + sizeof(int32_t) * (size_t)(2 * H);
    hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&r->d_state, state_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_state, 0, state_bytes, r->stream);
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
        r->d_new_lpr = r->d_q + H * ndim; r->d_new_ll = r->d_new_lpr + H; r->d_ladder = r->d_new_ll + H;
        r->d_nacc = (int64_t *)(r->d_ladder + MSX_MAX_GROUP); r->d_nswap = (unsigned long long *)(r->d_nacc + W);
        r->d_prev = r->d_nswap + MSX_MAX_GROUP; r->d_kstate = (long long *)(r->d_prev + MSX_MAX_GROUP);
        r->d_st_lpr = (int32_t *)(r->d_kstate + 2 * MSX_MAX_GROUP); r->d_st_ll = r->d_st_lpr + H;
        e = hipMemcpyAsync(r->d_coords, coords, sizeof(double) * (size_t)(W * ndim), hipMemcpyHostToDevice, r->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_ll, ll, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_lpr, lpr, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_ladder, r->beta.data(), sizeof(double) * (size_t)M, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) {
        group_tempered_free(g);
        return fail(g, MSX_ERR_HIP, w + ": " + hipGetErrorString(e));
    }
    return MSX_OK;
}

// Makes the run adaptive (DESIGN.md sections 19, 20): target k's ladder moves after every sweep with its own lag[k], time[k],
// from k0[k] adaptive iterations done.
int msx_group_ladder_adapt(msx_group *g, const double *lag, const double *time, const int64_t *k0) {
    if (!g) return MSX_ERR_INVALID;
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, "msx_group_ladder_adapt: call msx_group_tempered_begin first");
    if (r->enqueued || r->adaptive || r->failed)
        return fail(g, MSX_ERR_STATE, "msx_group_ladder_adapt: call once, between msx_group_tempered_begin and the run's first enqueue");
    if (!lag || !time || !k0) return fail(g, MSX_ERR_INVALID, "msx_group_ladder_adapt: bad arguments");
    for (int k = 0; k < r->K; ++k)
        if (!std::isfinite(lag[k]) || !(lag[k] > 0.0) || !std::isfinite(time[k]) || !(time[k] >= 1.0) || k0[k] < 0)
            return fail(g, MSX_ERR_INVALID, "msx_group_ladder_adapt: lag must be finite and > 0, time finite and >= 1, k0 >= 0 (target " +
                                                 std::to_string(k) + ")");
    HIP_TRY(g, hipSetDevice(g->device));
    std::vector<long long> st((size_t)(2 * r->K), 0);
    for (int k = 0; k < r->K; ++k) st[(size_t)(2 * k)] = (long long)k0[k];
    hipError_t e = hipMemcpyAsync(r->d_kstate, st.data(), sizeof(long long) * st.size(), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(g, MSX_ERR_HIP, std::string("msx_group_ladder_adapt: ") + hipGetErrorString(e));
    for (int k = 0; k < r->K; ++k) { r->P.lag[k] = lag[k]; r->P.time[k] = time[k]; }
    r->adaptive = true;
    return MSX_OK;
}

// The run's current ladders [K][T], behind everything queued (it waits for the compute stream); k, skipped [K].  A fixed
// run: the begin ladders, 0, 0.
int msx_group_ladder_current(msx_group *g, double *betas, int64_t *k, int64_t *skipped) {
    if (!g) return MSX_ERR_INVALID;
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, "msx_group_ladder_current: call msx_group_tempered_begin first");
    if (!betas) return fail(g, MSX_ERR_INVALID, "msx_group_ladder_current: bad arguments");
    std::vector<long long> st((size_t)(2 * r->K), 0);
    if (r->adaptive) {
        hipError_t e = hipSetDevice(g->device);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
        if (e == hipSuccess) e = hipMemcpy(betas, r->d_ladder, sizeof(double) * (size_t)r->M, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(st.data(), r->d_kstate, sizeof(long long) * st.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(g, MSX_ERR_HIP, std::string("msx_group_ladder_current: ") + hipGetErrorString(e));
    } else {
        memcpy(betas, r->beta.data(), sizeof(double) * (size_t)r->M);
    }
    for (int i = 0; i < r->K; ++i) {
        if (k) k[i] = (int64_t)st[(size_t)(2 * i)];
        if (skipped) skipped[i] = (int64_t)st[(size_t)(2 * i + 1)];
    }
    return MSX_OK;
}

// The ladders the last collected chunk of `slot` ran with, [nsteps][K][T], until the slot is enqueued again.
int msx_group_ladder_betas(msx_group *g, int32_t slot, double *out) {
    if (!g) return MSX_ERR_INVALID;
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, "msx_group_ladder_betas: call msx_group_tempered_begin first");
    if (slot < 0 || slot > 1 || !out) return fail(g, MSX_ERR_INVALID, "msx_group_ladder_betas: bad arguments");
    const GroupTemperedRun::Slot &sl = r->slot[slot];
    if (sl.busy || !sl.collected) return fail(g, MSX_ERR_STATE, "msx_group_ladder_betas: no collected chunk in this slot");
    if (r->adaptive) {
        memcpy(out, group_tempered_out(r, sl.h_out, sl.nsteps).betas, sizeof(double) * (size_t)(sl.nsteps * r->M));
    } else {
        for (int64_t st = 0; st < sl.nsteps; ++st) memcpy(out + st * r->M, r->beta.data(), sizeof(double) * (size_t)r->M);
    }
    return MSX_OK;
}

// The chunk's host randomness -- the general layout's arrays [nsteps][2][H], the members' halves side by side in member order
// and indices member-local, kind [nsteps][K T], swap_logu [nsteps][SW] with target k's [T - 1][nw_k] block at its place --
// checked (run_pack_moves' checks per member: every index is dereferenced on the device) and packed into the slot's pinned
// staging, c1 / c2 resolved to ensemble indices.  nullptr, or what is wrong.
static const char *group_tempered_pack(const GroupTemperedRun *r, char *h_in, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                       const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *g, const double *fac,
                                       const double *logu, const double *swap_logu) {
    const int64_t H = r->H, M = r->M;
    for (int64_t i = 0; i < nsteps * M; ++i)
        if (kind[i] != MSX_MOVE_STRETCH && kind[i] != MSX_MOVE_DE) return "kind out of range";
    for (int64_t i = 0; i < nsteps * M; ++i)
        if (kind[i] == MSX_MOVE_DE && r->Mw.nh[i % M] < 4) return "the DE move needs two distinct walkers in each half: at least 4 walkers";
    const GroupTemperedIn P = group_tempered_in(r, h_in, nsteps);
    for (int64_t row = 0; row < 2 * nsteps; ++row)
        for (int64_t m = 0; m < M; ++m) {
            const int64_t b = row * H + r->Mh.astart[m], off = r->Mh.off[m];
            const uint32_t mw = (uint32_t)r->Mw.nh[m], mh = mw / 2;
            const bool de = kind[(row / 2) * M + m] == MSX_MOVE_DE;
            for (int64_t j = b; j < b + (int64_t)mh; ++j) {
                if ((uint32_t)sidx[j] >= mw || (uint32_t)cidx[j] >= mw || (uint32_t)p1[j] >= mh || (uint32_t)p2[j] >= mh)
                    return "walker / partner index out of range";
                if (de && p1[j] == p2[j]) return "a DE entry needs two distinct walkers (p1 != p2)";
            }
            for (int64_t j = b; j < b + (int64_t)mh; ++j) {  // (the complementary half is checked: resolve)
                P.c1[j] = (int32_t)(off + cidx[b + p1[j]]);
                P.c2[j] = (int32_t)(off + cidx[b + p2[j]]);
            }
        }
    const int64_t L = r->entries(nsteps);
    memcpy(P.g, g, sizeof(double) * L); memcpy(P.fac, fac, sizeof(double) * L); memcpy(P.logu, logu, sizeof(double) * L);
    memcpy(P.sidx, sidx, sizeof(int32_t) * L); memcpy(P.cidx, cidx, sizeof(int32_t) * L);
    memcpy(P.kind, kind, sizeof(int32_t) * nsteps * M);
    if (r->SW > 0) memcpy(P.swap_logu, swap_logu, sizeof(double) * nsteps * r->SW);
    return nullptr;
}

// the chunk's rows appended to the run's series on the compute stream (tempered_put_chunk's rules)
static hipError_t group_tempered_put_chunk(GroupTemperedRun *r, const GroupTemperedOut &out, int64_t nsteps) {
    const int64_t W = r->W, row0 = r->series_row;
    if (msx_series *sr = r->s_chain) {
        hipError_t e = series_reserve(sr, row0 + nsteps, row0, r->stream);
        if (e != hipSuccess) return e;
        const int64_t total = nsteps * W * r->ndim;
        hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r->stream, (const double *)out.chain, nsteps, W,
                           (int32_t)r->ndim, sr->d_rows, sr->cap, row0);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        sr->rows = row0 + nsteps;
    }
    if (msx_series *sr = r->s_dens) {
        hipError_t e = series_reserve(sr, row0 + nsteps, row0, r->stream);
        if (e != hipSuccess) return e;
        const int64_t total = nsteps * W;
        const double *src[2] = {out.ll, out.lpr};
        for (int col = 0; col < 2; ++col) {
            hipLaunchKernelGGL(series_put_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r->stream, src[col], nsteps, W, (int32_t)1,
                               sr->d_rows + (int64_t)col * W * sr->cap, sr->cap, row0);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        sr->rows = row0 + nsteps;
    }
    r->series_row = row0 + nsteps;
    return hipSuccess;
}

struct GroupTemperedDraw { const uint64_t *seeds; const msx_move_set *set; int64_t first_iter; };

static int group_tempered_enqueue(msx_group *g, const char *who, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx,
                                  const int32_t *kind, const int32_t *p1, const int32_t *p2, const double *gg, const double *fac,
                                  const double *logu, const double *swap_logu, const GroupTemperedDraw *draw) {
    if (!g) return MSX_ERR_INVALID;
    const std::string w(who);
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, w + ": call msx_group_tempered_begin first");
    const bool args_ok = draw ? (draw->seeds && draw->set) : (sidx && cidx && kind && p1 && p2 && gg && fac && logu && (swap_logu || r->SW == 0));
    if (slot < 0 || slot > 1 || nsteps < 1 || nsteps > r->cap_steps || !args_ok) return fail(g, MSX_ERR_INVALID, w + ": bad arguments");
    if (r->failed) return fail(g, MSX_ERR_STATE, w + ": the run failed; end it (msx_group_tempered_end) and begin again");
    GroupTemperedRun::Slot &sl = r->slot[slot];
    if (sl.busy) return fail(g, MSX_ERR_STATE, w + ": slot not collected yet");
    // a member restaged or destroyed since begin: the launches would read tables that are gone -- the run is over
    if (int rc = group_tempered_members_check(g, who, r->ndim)) {
        r->failed = true;
        return rc;
    }
    MoveSetDev S;
    if (draw) {
        if (r->max_nw > kDrawMaxWalkers || draw->first_iter < 0)
            return fail(g, MSX_ERR_INVALID, w + ": the device generator takes up to 4096 walkers per rung and a first iteration >= 0");
        const int64_t min_nw = *std::min_element(r->nw.begin(), r->nw.end());
        if (const char *why = move_set_dev(draw->set, r->ndim, min_nw, &S)) return fail(g, MSX_ERR_INVALID, w + ": " + why);
    } else if (const char *why = group_tempered_pack(r, sl.h_in, nsteps, sidx, cidx, kind, p1, p2, gg, fac, logu, swap_logu)) {
        return fail(g, MSX_ERR_INVALID, w + ": " + why);
    }
    HIP_TRY(g, hipSetDevice(g->device));
    r->enqueued = true;
    const int T = r->T, K = r->K, M = r->M, ndim = r->ndim;
    const int64_t H = r->H, W = r->W;
    const GroupTemperedIn in = group_tempered_in(r, sl.d_in, nsteps);
    const GroupTemperedOut out = group_tempered_out(r, sl.d_out, nsteps);
    hipStream_t s = r->stream;
    const unsigned wgs = (unsigned)((r->max_nw + 255) / 256);
    hipError_t e = hipSuccess;
    int rc = MSX_OK;
    if (draw) {
        // (the slot was collected: no launch still reads its arrays, and the stream orders these before the half-steps)
        MoveDrawTable Tb;
        memset(&Tb, 0, sizeof(Tb));
        Tb.M = r->Mw;
        GroupSwapSeeds Sd;
        memset(&Sd, 0, sizeof(Sd));
        for (int m = 0; m < M; ++m) Tb.seed[m] = (unsigned long long)draw->seeds[m];
        for (int k = 0; k < K; ++k) Sd.seed0[k] = (unsigned long long)draw->seeds[k * T];
        hipLaunchKernelGGL(moves_draw_kernel, dim3((unsigned)nsteps, (unsigned)M), dim3(kDrawThreads), 0, s, Tb, S, draw->first_iter, (int32_t)ndim, 1,
                           H, in.sidx, in.cidx, in.c1, in.c2, in.g, in.fac, in.logu, in.kind);
        e = hipGetLastError();
        if (e == hipSuccess && T > 1) {
            hipLaunchKernelGGL(group_tempered_swap_draw_kernel, dim3((unsigned)nsteps, (unsigned)(K * (T - 1)), wgs), dim3(256), 0, s, Sd, r->G,
                               draw->first_iter, (int32_t)(T - 1), r->SW, in.swap_logu);
            e = hipGetLastError();
        }
    } else {
        e = hipMemcpyAsync(sl.d_in, sl.h_in, r->in_bytes(nsteps), hipMemcpyHostToDevice, r->up);
        if (e == hipSuccess) e = hipEventRecord(sl.in_ready, r->up);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, sl.in_ready, 0);
    }
    if (e == hipSuccess) e = hipMemsetAsync(out.worst, 0, sizeof(int32_t) * MSX_MAX_GROUP, s);
    GroupTemperedStepArgs A;
    memset(&A, 0, sizeof(A));
    A.coords = r->d_coords; A.ll = r->d_ll; A.lpr = r->d_lpr; A.q = r->d_q; A.new_lpr = r->d_new_lpr; A.new_ll = r->d_new_ll;
    A.st_lpr = r->d_st_lpr; A.st_ll = r->d_st_ll; A.nacc = r->d_nacc; A.ndim = ndim; A.worst = out.worst; A.ladder = r->d_ladder;
    GroupAdaptArgs D;
    memset(&D, 0, sizeof(D));
    D.beta = r->d_ladder; D.nswap = r->d_nswap; D.prev = r->d_prev; D.state = r->d_kstate; D.ntemps = T;
    GroupTemperedSwapArgs Sw;
    memset(&Sw, 0, sizeof(Sw));
    Sw.coords = r->d_coords; Sw.ll = r->d_ll; Sw.lpr = r->d_lpr; Sw.nswap = r->d_nswap; Sw.ladder = r->d_ladder; Sw.ntemps = T; Sw.ndim = ndim;
    auto half_arrays = [&](int64_t j) {  // half-step j of the chunk
        const int64_t o = j * H;
        return MoveChunk{in.g + o, in.fac + o, in.logu + o, in.sidx + o, in.c1 + o, in.c2 + o, in.kind + (j / 2) * M};
    };
    for (int64_t st = 0; st < nsteps && e == hipSuccess && rc == MSX_OK; ++st) {
        for (int k = 0; k < 3 && e == hipSuccess && rc == MSX_OK; ++k) {  // propose 0 | apply 0, propose 1 | apply 1
            A.a_on = k > 0; A.p_on = k < 2;
            if (A.a_on) A.a = half_arrays(2 * st + k - 1);
            if (A.p_on) A.p = half_arrays(2 * st + k);
            hipLaunchKernelGGL(group_tempered_step_kernel, dim3((unsigned)M), dim3(256), 0, s, A, r->Mh);
            e = hipGetLastError();
            if (e != hipSuccess || !A.p_on) continue;
            rc = msx_group_logprob_batch_dev(g, MSX_MODE_LOGPRIOR, r->d_q, r->eval_counts.data(), ndim, r->d_new_lpr, r->d_st_lpr, s, 0);
            if (rc == MSX_OK) rc = msx_group_logprob_batch_dev(g, MSX_MODE_LOGLIKE, r->d_q, r->eval_counts.data(), ndim, r->d_new_ll, r->d_st_ll, s, 0);
        }
        if (e != hipSuccess || rc != MSX_OK) break;
        Sw.logu = in.swap_logu + st * r->SW;
        Sw.chain_row = out.chain + st * W * ndim; Sw.ll_row = out.ll + st * W; Sw.lpr_row = out.lpr + st * W;
        hipLaunchKernelGGL(group_tempered_swap_kernel, dim3(wgs, (unsigned)K), dim3(256), 0, s, Sw, r->G);
        e = hipGetLastError();
        if (e != hipSuccess || !r->adaptive) continue;
        // the iteration's counts are complete once the sweep's launch has finished: a launch of its own, in stream order
        D.beta_row = out.betas + st * M;
        hipLaunchKernelGGL(group_tempered_adapt_kernel, dim3((unsigned)K), dim3(64), 0, s, D, r->P);
        e = hipGetLastError();
    }
    // the chunk's rows into the attached series, before kernels_done: a collected chunk's rows are in place
    if (e == hipSuccess && rc == MSX_OK) e = group_tempered_put_chunk(r, out, nsteps);
    // the counters keep running while this chunk's results travel: snapshot them in stream order, then bring the slot back
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(out.nacc, r->d_nacc, sizeof(int64_t) * (size_t)W, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(out.nswap, r->d_nswap, sizeof(int64_t) * MSX_MAX_GROUP, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipEventRecord(sl.kernels_done, s);
    if (e == hipSuccess && rc == MSX_OK) e = hipStreamWaitEvent(r->copy, sl.kernels_done, 0);
    if (e == hipSuccess && rc == MSX_OK) e = hipMemcpyAsync(sl.h_out, sl.d_out, r->out_bytes(nsteps), hipMemcpyDeviceToHost, r->copy);
    if (e == hipSuccess && rc == MSX_OK) e = hipEventRecord(sl.out_ready, r->copy);
    if (e != hipSuccess || rc != MSX_OK) {
        r->failed = true;  // some of the chunk's half-steps may be queued: only the run's end from here on
        if (e != hipSuccess) return fail(g, MSX_ERR_HIP, w + ": " + hipGetErrorString(e));
        return rc;
    }
    sl.nsteps = nsteps;
    sl.busy = true;
    sl.collected = false;
    return MSX_OK;
}

int msx_group_tempered_enqueue(msx_group *g, int32_t slot, int64_t nsteps, const int32_t *sidx, const int32_t *cidx, const int32_t *kind,
                               const int32_t *p1, const int32_t *p2, const double *gg, const double *fac, const double *logu,
                               const double *swap_logu) {
    return group_tempered_enqueue(g, "msx_group_tempered_enqueue", slot, nsteps, sidx, cidx, kind, p1, p2, gg, fac, logu, swap_logu, nullptr);
}

int msx_group_tempered_enqueue_drawn(msx_group *g, int32_t slot, int64_t nsteps, const uint64_t *seeds, const msx_move_set *set,
                                     int64_t first_iter) {
    const GroupTemperedDraw dd = {seeds, set, first_iter};
    return group_tempered_enqueue(g, "msx_group_tempered_enqueue_drawn", slot, nsteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, &dd);
}

int msx_group_tempered_collect(msx_group *g, int32_t slot, double *chain, double *ll_chain, double *lpr_chain, int64_t *naccept, int64_t *nswap,
                               int32_t *worst) {
    if (!g) return MSX_ERR_INVALID;
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, "msx_group_tempered_collect: call msx_group_tempered_begin first");
    if (slot < 0 || slot > 1 || !chain || !ll_chain || !lpr_chain || !naccept || !worst || (!nswap && r->T > 1))
        return fail(g, MSX_ERR_INVALID, "msx_group_tempered_collect: bad arguments");
    if (r->failed) return fail(g, MSX_ERR_STATE, "msx_group_tempered_collect: the run failed; end it (msx_group_tempered_end) and begin again");
    GroupTemperedRun::Slot &sl = r->slot[slot];
    if (!sl.busy) return fail(g, MSX_ERR_STATE, "msx_group_tempered_collect: nothing enqueued in this slot");
    const hipError_t e = hipEventSynchronize(sl.out_ready);
    if (e != hipSuccess) return fail(g, MSX_ERR_HIP, std::string("msx_group_tempered_collect: ") + hipGetErrorString(e));
    const GroupTemperedOut o = group_tempered_out(r, sl.h_out, sl.nsteps);
    const int64_t rows = sl.nsteps * r->W;
    memcpy(chain, o.chain, sizeof(double) * rows * r->ndim);
    memcpy(ll_chain, o.ll, sizeof(double) * rows);
    memcpy(lpr_chain, o.lpr, sizeof(double) * rows);
    memcpy(naccept, o.nacc, sizeof(int64_t) * r->W);
    for (int k = 0; k < r->K && r->T > 1; ++k)  // [K][T - 1] from the device's [K][T]
        memcpy(nswap + (int64_t)k * (r->T - 1), o.nswap + (int64_t)k * r->T, sizeof(int64_t) * (size_t)(r->T - 1));
    memcpy(worst, o.worst, sizeof(int32_t) * r->M);
    sl.busy = false;
    sl.collected = true;
    return MSX_OK;
}

int msx_group_tempered_end(msx_group *g, double *coords, double *ll, double *lpr) {
    if (!g) return MSX_ERR_INVALID;
    GroupTemperedRun *r = g->trun;
    if (!r) return MSX_OK;
    hipError_t e = hipSetDevice(g->device);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e == hipSuccess && coords) e = hipMemcpy(coords, r->d_coords, sizeof(double) * (size_t)(r->W * r->ndim), hipMemcpyDeviceToHost);
    if (e == hipSuccess && ll) e = hipMemcpy(ll, r->d_ll, sizeof(double) * (size_t)r->W, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lpr) e = hipMemcpy(lpr, r->d_lpr, sizeof(double) * (size_t)r->W, hipMemcpyDeviceToHost);
    group_tempered_free(g);
    if (e != hipSuccess) return fail(g, MSX_ERR_HIP, std::string("msx_group_tempered_end: ") + hipGetErrorString(e));
    return MSX_OK;
}

// The run's two series: K T members, member k T + t with counts[k] walkers; the chain's with the run's ndim, the densities'
// with ndim 2 (ll, lpr).  msx_series_attach_tempered's rules.
int msx_group_tempered_attach_series(msx_group *g, msx_series *chain, msx_series *dens, int64_t at_row) {
    if (!g) return MSX_ERR_INVALID;
    const std::string w("msx_group_tempered_attach_series");
    if (!chain && !dens) return fail(g, MSX_ERR_INVALID, w + ": bad arguments (give the chain's series, the densities' or both)");
    GroupTemperedRun *r = g->trun;
    if (!r) return fail(g, MSX_ERR_STATE, w + ": call msx_group_tempered_begin first");
    if (r->enqueued || r->failed || r->slot[0].busy || r->slot[1].busy || r->s_chain || r->s_dens)
        return fail(g, MSX_ERR_STATE, w + ": attach once, between msx_group_tempered_begin and the run's first enqueue");
    HIP_TRY(g, hipSetDevice(g->device));
    msx_series *both[2] = {chain, dens};
    const int32_t want_dim[2] = {r->ndim, 2};
    if (chain == dens) return fail(g, MSX_ERR_INVALID, w + ": the chain and the densities need a series each");
    for (int i = 0; i < 2; ++i) {
        msx_series *sr = both[i];
        if (!sr) continue;
        if (sr->run || sr->trun || sr->gtrun) return fail(g, MSX_ERR_STATE, w + ": the series is attached to another run in flight");
        if (sr->device != g->device) return fail(g, MSX_ERR_INVALID, w + ": the series lives on another device");
        bool same = sr->nw == r->W && sr->ndim == want_dim[i] && (int64_t)sr->off.size() == (int64_t)r->M + 1;
        for (int m = 0; same && m < r->M; ++m) same = sr->off[(size_t)m + 1] - sr->off[(size_t)m] == r->Mw.nh[m];
        if (!same)
            return fail(g, MSX_ERR_INVALID, w + ": a series needs targets x ntemps members, member k T + t of counts[k] walkers, and the run's ndim (the densities: ndim = 2)");
        if (at_row < 0 || at_row > sr->rows) return fail(g, MSX_ERR_INVALID, w + ": at_row must lie in 0 .. the rows each series holds");
    }
    for (msx_series *sr : both) {
        if (!sr) continue;
        series_release(sr);
        sr->rows = at_row;   // (rows at or after at_row are dropped: the run overwrites them)
        sr->gtrun = r;
    }
    r->s_chain = chain;
    r->s_dens = dens;
    r->series_row = at_row;
    return MSX_OK;
}
