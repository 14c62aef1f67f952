// vp_prove_gkr_fs (include/vpgpu.h): the GKR part non-interactive, every challenge drawn on the device.  The launch sequence is the per-round one of the
// interactive entry points (the inits they use, do_round, do_finalize) on the device tape, with the FS siblings of the round kernels (vp_kernels_gkrfs.h)
// drawing each challenge into the slot the next round reads, and k_gkr_fs_span for the steps between the sumchecks.  One stream, no host wait before the end.

extern "C" {

int vp_prove_gkr_fs(vp_ctx *ctx, const uint8_t state_in[32], uint8_t *transcript, uint64_t capacity, uint64_t *n_written, vp_F *tape_out, uint64_t *n_draws,
                    uint8_t state_out[32]) {
    if (!ctx) return VP_EINVAL;
    if (!has_circuit(ctx) || !ctx->evaluated) { ctx->err = "vp_prove_gkr_fs: vp_evaluate has not run"; return VP_EINVAL; }
    if (!state_in || !transcript || !tape_out || !n_draws || !state_out) { ctx->err = "vp_prove_gkr_fs: a null argument"; return VP_EINVAL; }
    if (ctx->shard_world > 1 || ctx->split_lw > 0 || ctx->rsh) { ctx->err = "vp_prove_gkr_fs: not on a chain-sharded, round-sharded or index-split context"; return VP_EINVAL; }
    if (ctx->rec) { ctx->err = "vp_prove_gkr_fs: a launch plan is being recorded"; return VP_EINVAL; }
    const u64 n_tr = ctx->n_tr, n_tape = ctx->n_tape, n_fs = sizeof(GkrFs) / sizeof(F), n_all = n_tr + n_tape + n_fs;
    if (capacity < n_tr * sizeof(F)) { ctx->err = "vp_prove_gkr_fs: transcript buffer size (vp_gkr_sizes)"; return VP_EINVAL; }
    if (n_all >> 32) { ctx->err = "vp_prove_gkr_fs: transcript and tape beyond 2^32 elements"; return VP_ELIMIT; }
    VP_ENTER(ctx);
    const int n = ctx->n_layers;
    const hipStream_t st = ctx->stream;
    if (ctx->h_io_cap < n_all) {
        if (ctx->h_io) (void) hipHostFree(ctx->h_io);
        ctx->h_io = nullptr; ctx->h_io_cap = 0;
        HIPCHK(hipHostMalloc((void **) &ctx->h_io, n_all * sizeof(F), hipHostMallocDefault));
        ctx->h_io_cap = n_all;
    }
    // a sumcheck the caller left unfinished on the interactive entry points is abandoned, as by vp_vres
    ctx->sc_open = false; ctx->r1_pending = 0; ctx->rlog.clear();
    ctx->st.launches = 0; ctx->st.rounds = 0;
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    GkrFs *fs = reinterpret_cast<GkrFs *>(ctx->d_tr + n_tr + 3 + VP_MAX_TAB);
    F *tr = ctx->d_tr, *tape = ctx->d_tape;
    {   // the chain: the caller's state, counter 0 (through pinned memory: the caller's buffer may be pageable)
        GkrFs h0{};
        memcpy(h0.s.w, state_in, 32);
        memcpy(ctx->h_io, &h0, sizeof h0);
        HIPCHK(hipMemcpyAsync(fs, ctx->h_io, sizeof h0, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipEventRecord(ctx->ev0, st));
    HIPCHK(hipMemsetAsync(tape, 0, n_tape * sizeof(F), st));                   // slots the schedule never draws stay zero
    HIPCHK(hipMemsetAsync(ctx->add_term(), 0, sizeof(F), st));
    u64 pos = 0, absorbed = 0;                                                 // transcript elements written / absorbed into the chain
    // E over the transcript elements not absorbed yet (the rounds absorb their own polynomials), then n_draw draws into slot[0 ..)
    auto span = [&](F *slot, u32 n_draw) {
        const u32 n_abs = (u32) (pos - absorbed);
        const int sl = prof_begin(ctx, st, VP_K_MERKLE, 1, 1, 16ull * (n_abs + n_draw), (u64) n_abs + n_draw);
        hipLaunchKernelGGL(k_gkr_fs_span, dim3(1), dim3(64), 0, st, fs, (const F *) (tr + absorbed), n_abs, slot, n_draw);
        prof_end(ctx, st, sl);
        count_launch(ctx);
        absorbed = pos;
    };
    // the rounds of the sumcheck just initialised: challenge j goes to slot[j], where round j + 2 and the finalize read it; then the claims
    auto sumcheck = [&](int rounds, F *slot, int n_claims) -> int {
        const F zero = f_zero();
        for (int j = 0; j < rounds; ++j) { VPCHK(do_round(ctx, j ? slot + (j - 1) : ctx->zero(), zero, tr + pos, nullptr, fs, slot + j)); pos += 3; }
        absorbed = pos;
        VPCHK(do_finalize(ctx, rounds ? slot + (rounds - 1) : ctx->zero(), zero, tr + pos, nullptr));
        pos += (u64) n_claims;
        return VP_OK;
    };
    const bool fast = ctx->opt.interactive_fast_init != 0;
    {   // r_liu of the output layer, Vres
        LayerDev &T = ctx->L[n - 1];
        span(tape, (u32) T.bl);
        VPCHK(run_beta_half(ctx, tape, T.bl, ctx->one()));
        hipLaunchKernelGGL(k_vres, dim3(1), dim3(VP_BLOCK), 0, st, ctx->bf, ctx->bs, T.bl >> 1, T.val, (u32) T.size, tr + pos, (F *) nullptr);
        count_launch(ctx);
        pos += 1;
    }
    for (int i = n - 1; i >= 1; --i) {
        const int pbl = ctx->L[i - 1].bl, mdb = ctx->L[i].max_dad_bl;
        span(tape + ctx->as_off[i], 1u);                                      // E(Vres) or E(vr) of the layer above; assert_random
        VPCHK(fast ? do_phase1_init_fast(ctx, i) : do_phase1_init(ctx, i, rliu_ptr(ctx, i), tape + ctx->as_off[i]));
        VPCHK(sumcheck(pbl, tape + ctx->ru_off[i], 1));
        if (mdb != -1) {
            span(nullptr, 0u);                                                 // E(claim_u) before phase 2's first polynomial
            VPCHK(fast ? do_phase2_init_fast(ctx, i) : do_phase2_init(ctx, i, tape + ctx->ru_off[i]));
            VPCHK(sumcheck(mdb, tape + ctx->rv_off[i], i));
        }
        span(tape + ctx->sig_off[i], (u32) n);                                // E(claim_u) or E over the layer's claims; every entry of sig
        VPCHK(fast ? do_liu_init_fast(ctx, i) : do_liu_init(ctx, i));
        VPCHK(sumcheck(pbl, tape + ctx->rliu_off[i], 1));
    }
    span(nullptr, 0u);                                                         // E(vr) of layer 1: the chain's closing state
    ctx->sc.phase = 0;                                                         // no sumcheck is open for vp_round / vp_finalize
    HIPCHK(hipEventRecord(ctx->ev1, st));
    if (pos != n_tr) { (void) hipStreamSynchronize(st); ctx->err = "internal: transcript size"; return VP_EINVAL; }
    // ---- transcript | tape | chain: one block in pinned memory, one wait
    hipLaunchKernelGGL(k_gkr_fs_ship, dim3(std::min<u32>(nblk(n_all), 256u)), dim3(VP_BLOCK), 0, st, (const F *) tr, (u32) n_tr, (const F *) tape, (u32) n_tape, (const GkrFs *) fs, ctx->h_io);
    VPCHK(check_stream(ctx));
    GkrFs out;
    memcpy(transcript, ctx->h_io, n_tr * sizeof(F));
    memcpy(tape_out, ctx->h_io + n_tr, n_tape * sizeof(F));
    memcpy(&out, ctx->h_io + n_tr + n_tape, sizeof out);
    memcpy(state_out, out.s.w, 32);
    *n_draws = out.ctr;
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->st.gkr_ms = ms;
    ctx->st.fold_ms = 0; ctx->st.fold_bytes = 0; ctx->st.fold_launches = 0;
    if (ctx->profiling) prof_collect(ctx);
    if (n_written) *n_written = n_tr * sizeof(F);
    return VP_OK;
}

}  // extern "C"
