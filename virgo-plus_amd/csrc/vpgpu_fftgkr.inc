// Part of vpgpu.hip (included at its end): vp_fft_gkr — lib/virgo's fft_circuit_gkr::fft_gkr (lib/virgo/src/fft_circuit_GKR.cpp:833-849),
// prover side, in one device pass (SURVEY.md §8f-3).  verify_poly_commitment runs that function between the commitment and the FRI commit
// phase (vpd_verifier.cpp:92) and adds its prover time to the reported "Polynomial commitment: prove time" (:94, src/verifier.cpp:183).
// It is a GKR over a fixed circuit whose verifier draws come from the same transcript-independent glibc stream as all the others
// (fieldElement.cpp:119-124), so — like vp_prove_gkr — the whole tape is taken up front and the 2 + 2 lg sumchecks run back to back:
// the circuit layers by dense elementwise kernels (vp_kernels_fftgkr.h), each sumcheck's mult / add tables by a closed form over the
// butterfly wiring, the rounds by the GKR path's own fold / segment / closing kernels (run_sumcheck_seg).
namespace {

struct FgkOffsets {
    int lg; u64 r, x, r0, r1, ru_a, rv_a, ru_m, rv_m, dep0, n;
    explicit FgkOffsets(int lg_) : lg(lg_) {
        r = 0; x = lg; r0 = x + 64; r1 = r0 + lg + 10; ru_a = r1 + lg + 10; rv_a = ru_a + lg + 6; ru_m = rv_a + lg + 6; rv_m = ru_m + lg;
        dep0 = rv_m + lg; n = dep0 + (u64) lg * (2 * lg + 2);
    }
    u64 ru_d(int d) const { return dep0 + (u64) d * (2 * lg + 2); }
    u64 rv_d(int d) const { return ru_d(d) + lg; }
    u64 alpha_d(int d) const { return rv_d(d) + lg; }
    u64 beta_d(int d) const { return alpha_d(d) + 1; }
    static u64 n_msgs(int lg) { return 64 + 3ull * (2ull * lg * lg + 2 * lg + 6) + 2 + 2ull * lg; }
};

}  // namespace

struct FgkState {
    int lg = 0;
    F *B = nullptr, *S = nullptr, *Pm = nullptr, *winv = nullptr, *sq = nullptr, *xsq = nullptr, *g = nullptr, *eu = nullptr, *hi = nullptr, *part = nullptr, *xt = nullptr;
    F *tape = nullptr, *msgs = nullptr;
    Dig *fs_state = nullptr; F *fs_part = nullptr;      // vp_fft_gkr_fs: the chain's state (behind msgs and tape, one block), per-workgroup sums of a round
    Lane lane;
    std::vector<void *> allocs;
    // asynchronous form (vp_fft_gkr_begin / _end): a stream and an event pair of its own, host copies that outlive the call
    hipStream_t own_stream = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr, e_dep = nullptr;
    int pending_lg = 0;
    // pinned host copies of the tape (in) and of the messages (out): the caller's buffers are pageable, and the runtime's first pageable copy in either direction
    // sets up its own staging (measured ~10 ms on the first vp_fft_gkr of a process, tools/first_use_probe.py)
    F *h_tape = nullptr, *h_msgs = nullptr;          // (h_tape carries 32 more elements behind the tape: the powers of the inverse root, sq_host)
    // the 2 lg sumchecks of the inverse FFT as one batch (fgk_prepare_batch): per-depth eq tables and v_u, a lane of tables per sumcheck, the job arrays of the
    // table kernels and the merged fold / segment / closing launches (every pointer in them is fixed once the buffers exist)
    int batch_lg = 0;
    F *G = nullptr, *EU = nullptr, *VU = nullptr;
    std::vector<Lane> blanes;
    FgTabJob *d_tab = nullptr; FgDotJob *d_dot = nullptr; FgIfftJob *d_ifft = nullptr;
    struct BNode { int kind; u32 first, count, grid, lds, map_off; };
    std::vector<BNode> bnodes;
    SfArgs *d_sf = nullptr; SegArgs *d_seg = nullptr; EmitArgs *d_emit = nullptr; BlkMap *d_map = nullptr;
    void release() { if (own_stream) (void) hipStreamSynchronize(own_stream); for (void *p : allocs) (void) hipFree(p); allocs.clear(); lg = 0; pending_lg = 0; batch_lg = 0; blanes.clear(); bnodes.clear();
                     if (h_tape) (void) hipHostFree(h_tape); if (h_msgs) (void) hipHostFree(h_msgs); h_tape = h_msgs = nullptr; }
    ~FgkState() { if (own_stream) { (void) hipStreamSynchronize(own_stream); (void) hipStreamDestroy(own_stream); } if (e0) (void) hipEventDestroy(e0); if (e1) (void) hipEventDestroy(e1); if (e_dep) (void) hipEventDestroy(e_dep); }
};
void vp_free_fgk(vp_ctx *ctx) { if (ctx->fgk) { ctx->fgk->release(); delete ctx->fgk; ctx->fgk = nullptr; } }

namespace {

template <class T> int fgk_alloc(vp_ctx *ctx, FgkState &s, T **p, size_t n) {
    *p = nullptr;
    HIPCHK(hipMalloc((void **) p, std::max<size_t>(n, 1) * sizeof(T)));
    s.allocs.push_back((void *) *p);
    return VP_OK;
}
int fgk_prepare(vp_ctx *ctx, int lg) {
    if (!ctx->fgk) ctx->fgk = new FgkState();
    FgkState &s = *ctx->fgk;
    if (s.lg == lg) return VP_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.release();
    const size_t N = (size_t) 1 << lg;
    const FgkOffsets o(lg);
    VPCHK(fgk_alloc(ctx, s, &s.B, (size_t) (lg + 1) * N)); VPCHK(fgk_alloc(ctx, s, &s.S, N)); VPCHK(fgk_alloc(ctx, s, &s.Pm, 64 * N));
    VPCHK(fgk_alloc(ctx, s, &s.winv, std::max<size_t>(1, N / 2))); VPCHK(fgk_alloc(ctx, s, &s.sq, 32)); VPCHK(fgk_alloc(ctx, s, &s.xsq, (size_t) 64 * lg)); VPCHK(fgk_alloc(ctx, s, &s.xt, ((size_t) 64 << std::min(lg, 9)) + ((size_t) 64 << (lg - std::min(lg, 9)))));
    VPCHK(fgk_alloc(ctx, s, &s.g, N)); VPCHK(fgk_alloc(ctx, s, &s.eu, N)); VPCHK(fgk_alloc(ctx, s, &s.hi, 64)); VPCHK(fgk_alloc(ctx, s, &s.part, (size_t) 64 * nblk(N)));
    // messages | tape | the chain's state in one block: vp_fft_gkr_fs returns all three in one copy
    VPCHK(fgk_alloc(ctx, s, &s.msgs, FgkOffsets::n_msgs(lg) + o.n + 2));
    s.tape = s.msgs + FgkOffsets::n_msgs(lg); s.fs_state = reinterpret_cast<Dig *>(s.tape + o.n);
    VPCHK(fgk_alloc(ctx, s, &s.fs_part, (size_t) 3 * MAX_BLOCKS));
    HIPCHK(hipHostMalloc((void **) &s.h_tape, (o.n + 32) * sizeof(F), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **) &s.h_msgs, (FgkOffsets::n_msgs(lg) + o.n + 2) * sizeof(F), hipHostMallocDefault));
    for (int b = 0; b < 2; ++b)
        for (int t = 0; t < 3; ++t) VPCHK(fgk_alloc(ctx, s, &s.lane.tab[b][t], t == 2 ? N : 64 * N));     // the add table exists only in the 2^lg-entry sumchecks
    VPCHK(fgk_alloc(ctx, s, &s.lane.part2, (size_t) 16 * MAX_BLOCKS * 3));
    // vp_fft_gkr_fs: its tail kernel holds up to 96 KB of tables in dynamic LDS (once per set of buffers, off the per-call path)
    HIPCHK(hipFuncSetAttribute((const void *) k_fg_fs_tail<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (FG_FS_TABLES * sizeof(F) * FG_FS_TAIL_N)));
    HIPCHK(hipFuncSetAttribute((const void *) k_fg_fs_tail<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (FG_FS_TABLES * sizeof(F) * FG_FS_TAIL_N)));
    s.lane.stream = ctx->stream;
    s.lg = lg;
    return VP_OK;
}

int fgk_sumcheck(vp_ctx *ctx, const F *V0, int rounds, int has_a, const F *r, F *out) {
    FusedSumcheck sc;
    sc.n_tab = 1; sc.rounds = rounds; sc.has_a = has_a; sc.phase = 3;                      // V of round 1 is read from V0; no V_u side output
    sc.off[0] = 0; sc.len0[0] = sc.valid0[0] = 1u << rounds;
    sc.V0 = V0; sc.r = r; sc.poly_out = out; sc.claims_out = out + 3 * rounds;
    return run_sumcheck_seg(ctx, sc);
}

// Everything the batched form of the inverse-FFT sumchecks needs, once per lg: buffers, the job arrays of the table kernels, and the fold / segment / closing
// launches of all 2 lg sumchecks merged step by step — recorded by running the per-sumcheck driver in record mode on a lane of its own each (the way the GKR
// plan is recorded); the sumchecks have one shape, so step t of every chain is the same kernel and becomes one launch.
template <class T> int fgk_upload(vp_ctx *ctx, FgkState &s, T **dst, const std::vector<T> &v) {
    VPCHK(fgk_alloc(ctx, s, dst, v.size()));
    if (!v.empty()) HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return VP_OK;
}
int fgk_prepare_batch(vp_ctx *ctx, int lg) {
    FgkState &s = *ctx->fgk;
    if (s.batch_lg == lg) return VP_OK;
    const size_t N = (size_t) 1 << lg;
    const FgkOffsets o(lg);
    const int ns = 2 * lg;
    VPCHK(fgk_alloc(ctx, s, &s.G, (size_t) lg * N)); VPCHK(fgk_alloc(ctx, s, &s.EU, (size_t) lg * N)); VPCHK(fgk_alloc(ctx, s, &s.VU, (size_t) lg));
    s.blanes.assign(ns, Lane());
    for (int c = 0; c < ns; ++c) {
        for (int b = 0; b < 2; ++b)
            for (int t = 0; t < 3; ++t) VPCHK(fgk_alloc(ctx, s, &s.blanes[c].tab[b][t], N));
        VPCHK(fgk_alloc(ctx, s, &s.blanes[c].part2, (size_t) 16 * MAX_BLOCKS * 3));
    }
    std::vector<FgTabJob> tab; std::vector<FgDotJob> dot; std::vector<FgIfftJob> ifft;
    u64 pos = 64 + (3 * (u64) (lg + 6) + 1) + (3 * (u64) lg + 1);               // behind the outputs, the addition layer and the multiplication layer
    std::vector<u64> pos_of(ns);
    for (int d = 0; d < lg; ++d) {
        const F *r0 = s.tape + (d ? o.ru_d(d - 1) : o.ru_m), *r1 = s.tape + (d ? o.rv_d(d - 1) : o.rv_m);
        const F *al = d ? s.tape + o.alpha_d(d - 1) : nullptr, *be = d ? s.tape + o.beta_d(d - 1) : nullptr;
        const F *pre = s.B + (size_t) (lg - d - 1) * N;
        F *g = s.G + (size_t) d * N, *eu = s.EU + (size_t) d * N;
        tab.push_back(FgTabJob{r0, r1, al, be, g});
        tab.push_back(FgTabJob{s.tape + o.ru_d(d), nullptr, nullptr, nullptr, eu});
        dot.push_back(FgDotJob{eu, pre, s.VU + d});                             // v_u = the layer's extension at r_u (what phase 1's last fold leaves)
        ifft.push_back(FgIfftJob{g, pre, nullptr, nullptr, s.blanes[2 * d].tab[0][1], s.blanes[2 * d].tab[0][2], d, 1});
        ifft.push_back(FgIfftJob{g, nullptr, eu, s.VU + d, s.blanes[2 * d + 1].tab[0][1], s.blanes[2 * d + 1].tab[0][2], d, 2});
        pos_of[2 * d] = pos; pos += 3 * (u64) lg + 1;
        pos_of[2 * d + 1] = pos; pos += 3 * (u64) lg + 1;
    }
    if (pos != FgkOffsets::n_msgs(lg)) { ctx->err = "internal: fft_gkr message count (batch)"; return VP_EINVAL; }
    VPCHK(fgk_upload(ctx, s, &s.d_tab, tab)); VPCHK(fgk_upload(ctx, s, &s.d_dot, dot)); VPCHK(fgk_upload(ctx, s, &s.d_ifft, ifft));
    // record the sumchecks
    PlanRec rec; rec.chains.resize(ns);
    PlanRec *keep_rec = ctx->rec; Lane *keep_ln = ctx->ln; const int keep_vreal = ctx->vreal; const bool keep_drop1 = ctx->drop_round1;
    const SfGenJob keep_gen = ctx->rec_gen;
    ctx->rec = &rec; ctx->vreal = 0; ctx->drop_round1 = false; ctx->rec_gen = SfGenJob{};
    int rc = VP_OK;
    for (int c = 0; c < ns && rc == VP_OK; ++c) {
        const int d = c >> 1;
        rec.cur = c; ctx->ln = &s.blanes[c];
        rc = fgk_sumcheck(ctx, s.B + (size_t) (lg - d - 1) * N, lg, 1, s.tape + ((c & 1) ? o.rv_d(d) : o.ru_d(d)), s.msgs + pos_of[c]);
    }
    ctx->rec = keep_rec; ctx->ln = keep_ln; ctx->vreal = keep_vreal; ctx->drop_round1 = keep_drop1; ctx->rec_gen = keep_gen;
    VPCHK(rc);
    // merge: step t of every chain into one launch
    std::vector<SfArgs> sf; std::vector<SegArgs> seg; std::vector<EmitArgs> emit; std::vector<BlkMap> map;
    s.bnodes.clear();
    const size_t T = rec.chains[0].size();
    for (int c = 1; c < ns; ++c) if (rec.chains[c].size() != T) { ctx->err = "internal: fft_gkr sumchecks of different shapes"; return VP_EINVAL; }
    for (size_t t = 0; t < T; ++t) {
        const int kind = rec.chains[0][t].kind;
        FgkState::BNode nd{kind, 0, 0, 0, 0, (u32) map.size()};
        nd.first = kind == NK_SF ? (u32) sf.size() : kind == NK_SEG ? (u32) seg.size() : (u32) emit.size();
        for (int c = 0; c < ns; ++c) {
            const PStep &st = rec.chains[c][t];
            if (st.kind != kind || (kind != NK_SF && kind != NK_SEG && kind != NK_EMIT)) { ctx->err = "internal: fft_gkr sumcheck step kinds"; return VP_EINVAL; }
            if (kind == NK_SF) sf.push_back(rec.sf[st.idx]); else if (kind == NK_SEG) seg.push_back(rec.seg[st.idx]); else emit.push_back(rec.emit[st.idx]);
            if (kind != NK_EMIT) for (u32 b = 0; b < st.grid; ++b) map.push_back(BlkMap{nd.count, b});
            nd.grid += st.grid; nd.lds = std::max(nd.lds, st.lds); ++nd.count;
        }
        s.bnodes.push_back(nd);
    }
    VPCHK(fgk_upload(ctx, s, &s.d_sf, sf)); VPCHK(fgk_upload(ctx, s, &s.d_seg, seg)); VPCHK(fgk_upload(ctx, s, &s.d_emit, emit)); VPCHK(fgk_upload(ctx, s, &s.d_map, map));
    s.batch_lg = lg;
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_fft_gkr_sizes(int lg, uint64_t *n_tape, uint64_t *n_msgs) {
    if (lg < 1 || lg > 20) return VP_EINVAL;
    if (n_tape) *n_tape = FgkOffsets(lg).n;
    if (n_msgs) *n_msgs = FgkOffsets::n_msgs(lg);
    return VP_OK;
}

// the circuit (build_circuit, :22-101) from the r and x slots of s.tape, in stream order: every layer, the products, the 64 outputs -> s.msgs[0..64)
static int fgk_circuit(vp_ctx *ctx, FgkState &s, int lg, hipStream_t st) {
    const FgkOffsets o(lg);
    const u32 N = 1u << lg;
    {
        F w = host_pow(host_root_of_unity(lg), (unsigned __int128) P61 * P61 - 2);                 // inv_rou (:36)
        F *sq_host = s.h_tape + o.n;
        for (int b = 0; b < 32; ++b) { sq_host[b] = w; w = f_mul(w, w); }
        HIPCHK(hipMemcpyAsync(s.sq, sq_host, 32 * sizeof(F), hipMemcpyHostToDevice, st));
    }
    const F inv_n = host_inv_real((u64) N);
    hipLaunchKernelGGL(k_fg_pows, dim3(nblk(std::max<u32>(1, N / 2))), dim3(VP_BLOCK), 0, st, (const F *) s.sq, std::max(0, lg - 1), std::max<u32>(1, N / 2), s.winv);
    hipLaunchKernelGGL(k_fg_expand, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.r), lg, s.B);
    for (int t = 1; t <= lg; ++t)
        hipLaunchKernelGGL(k_fg_butterfly, dim3(nblk(N / 2)), dim3(VP_BLOCK), 0, st, (const F *) (s.B + (size_t) (t - 1) * N), s.B + (size_t) t * N,
                           (const F *) s.winv, lg, lg - t, t == lg ? s.S : (F *) nullptr, inv_n);
    hipLaunchKernelGGL(k_fg_xsq, dim3(1), dim3(64), 0, st, (const F *) (s.tape + o.x), lg, s.xsq);
    hipLaunchKernelGGL(k_fg_xtab, dim3(nblk((64u << std::min(lg, 9)) + (64u << (lg - std::min(lg, 9))))), dim3(VP_BLOCK), 0, st, (const F *) s.xsq, lg, s.xt);
    hipLaunchKernelGGL(k_fg_polyeval, dim3(nblk(N), 64), dim3(VP_BLOCK), 0, st, (const F *) s.S, (const F *) s.xt, lg, s.Pm, s.part);
    hipLaunchKernelGGL(k_fg_rowsum, dim3(64), dim3(VP_BLOCK), 0, st, (const F *) s.part, nblk(N), s.msgs);
    return VP_OK;
}
// everything of vp_fft_gkr up to (not including) the wait, on stream `st` (the context's own, or FgkState::own_stream for the asynchronous form)
static int fgk_enqueue(vp_ctx *ctx, int lg, const vp_F *tape, uint64_t n_tape, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const FgkOffsets o(lg);
    const u64 n_out = FgkOffsets::n_msgs(lg);
    FgkState &s = *ctx->fgk;
    const u32 N = 1u << lg;
    s.lane.stream = st;
    // the drivers below use the context's current lane and its "all circuit values are real" switch: fft_gkr has its own tables and
    // complex values throughout
    Lane *keep_ln = ctx->ln; const int keep_vreal = ctx->vreal;
    ctx->ln = &s.lane; ctx->vreal = 0;
    struct Restore { vp_ctx *c; Lane *l; int v; ~Restore() { c->ln = l; c->vreal = v; } } restore{ctx, keep_ln, keep_vreal};
    memcpy(s.h_tape, tape, n_tape * sizeof(F));                   // the caller's buffer may go away before the copy runs
    HIPCHK(hipMemcpyAsync(s.tape, s.h_tape, n_tape * sizeof(F), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    VPCHK(fgk_circuit(ctx, s, lg, st));
    u64 pos = 64;
    // ---- addition layer (:190-309): claim point r_0[0..6), alpha = 1, beta = 0
    hipLaunchKernelGGL(k_fg_gtab, dim3(1), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.r0), (const F *) nullptr, 6, (const F *) nullptr, (const F *) nullptr, s.hi);
    hipLaunchKernelGGL(k_fg_add_init, dim3(nblk((u64) 64 * N)), dim3(VP_BLOCK), 0, st, (const F *) s.hi, lg, s.lane.tab[0][1]);
    VPCHK(fgk_sumcheck(ctx, s.Pm, lg + 6, 0, s.tape + o.ru_a, s.msgs + pos));
    pos += 3 * (lg + 6) + 1;
    // ---- multiplication layer (:311-447): claim point = the addition layer's r_u (lg + 6 coordinates), alpha = 1, beta = 0
    hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_a), (const F *) nullptr, lg, (const F *) nullptr, (const F *) nullptr, s.g);
    hipLaunchKernelGGL(k_fg_gtab, dim3(1), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_a + lg), (const F *) nullptr, 6, (const F *) nullptr, (const F *) nullptr, s.hi);
    hipLaunchKernelGGL(k_fg_mul_init, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) s.g, (const F *) s.hi, (const F *) s.xt, lg, s.lane.tab[0][1]);
    VPCHK(fgk_sumcheck(ctx, s.S, lg, 0, s.tape + o.ru_m, s.msgs + pos));
    pos += 3 * lg + 1;
    // ---- inverse FFT, top layer first (:458-768).  Depth d: claim points r_0 = previous r_u, r_1 = previous r_v, weights alpha, beta
    // (1, 0 before the first depth; drawn after every depth, :763-764)
    if (ctx->opt.fft_gkr_batched) {
        // round 4: the 2 lg sumchecks as one batch — three table launches and one launch per step of the (common) sumcheck shape
        VPCHK(fgk_prepare_batch(ctx, lg));
        hipLaunchKernelGGL(k_fg_gtab_multi, dim3(nblk(N), 2 * lg), dim3(VP_BLOCK), 0, st, (const FgTabJob *) s.d_tab, lg);
        hipLaunchKernelGGL(k_fg_dot_multi, dim3(lg), dim3(VP_BLOCK), 0, st, (const FgDotJob *) s.d_dot, N);
        hipLaunchKernelGGL(k_fg_ifft_multi, dim3(nblk(std::max<u32>(1, N / 2)), 2 * lg), dim3(VP_BLOCK), 0, st, (const FgIfftJob *) s.d_ifft, (const F *) s.winv, lg);
        for (const auto &nd : s.bnodes) {
            const BlkMap *mp = s.d_map + nd.map_off;
            if (nd.kind == NK_SF) hipLaunchKernelGGL(k_sumfold3b_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, (const SfArgs *) (s.d_sf + nd.first), mp);
            else if (nd.kind == NK_SEG) hipLaunchKernelGGL(k_seg_multi, dim3(nd.grid), dim3(VP_SEG_THREADS), 0, st, (const SegArgs *) (s.d_seg + nd.first), mp);
            else hipLaunchKernelGGL(k_emit_multi, dim3(nd.count), dim3(VP_EMIT_THREADS), nd.lds, st, (const EmitArgs *) (s.d_emit + nd.first));
        }
        pos += (u64) lg * 2 * (3 * (u64) lg + 1);
    } else
    for (int d = 0; d < lg; ++d) {
        const F *r0 = s.tape + (d ? o.ru_d(d - 1) : o.ru_m), *r1 = s.tape + (d ? o.rv_d(d - 1) : o.rv_m);
        const F *al = d ? s.tape + o.alpha_d(d - 1) : nullptr, *be = d ? s.tape + o.beta_d(d - 1) : nullptr;
        const F *pre = s.B + (size_t) (lg - d - 1) * N;
        hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, r0, r1, lg, al, be, s.g);
        hipLaunchKernelGGL(k_fg_ifft_p1, dim3(nblk(N / 2)), dim3(VP_BLOCK), 0, st, (const F *) s.g, pre, (const F *) s.winv, lg, d, s.lane.tab[0][1], s.lane.tab[0][2]);
        VPCHK(fgk_sumcheck(ctx, pre, lg, 1, s.tape + o.ru_d(d), s.msgs + pos));
        const F *vu = s.msgs + pos + 3 * lg;
        pos += 3 * lg + 1;
        hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_d(d)), (const F *) nullptr, lg, (const F *) nullptr, (const F *) nullptr, s.eu);
        hipLaunchKernelGGL(k_fg_ifft_p2, dim3(nblk(N / 2)), dim3(VP_BLOCK), 0, st, (const F *) s.g, (const F *) s.eu, vu, (const F *) s.winv, lg, d, s.lane.tab[0][1], s.lane.tab[0][2]);
        VPCHK(fgk_sumcheck(ctx, pre, lg, 1, s.tape + o.rv_d(d), s.msgs + pos));
        pos += 3 * lg + 1;
    }
    if (pos != n_out) { ctx->err = "internal: fft_gkr message count"; return VP_EINVAL; }
    HIPCHK(hipEventRecord(e1, st));
    return VP_OK;
}
static int fgk_check_args(vp_ctx *ctx, int lg, const vp_F *tape, uint64_t n_tape) {
    if (lg < 1 || lg > 20) { ctx->err = "vp_fft_gkr: lg out of range (1..20)"; return VP_ELIMIT; }
    if (n_tape != FgkOffsets(lg).n) { ctx->err = "vp_fft_gkr: tape size (vp_fft_gkr_sizes)"; return VP_EINVAL; }
    for (u64 i = 0; i < n_tape; ++i) if (tape[i].real >= P61 || tape[i].img >= P61) { ctx->err = "vp_fft_gkr: non-canonical tape element"; return VP_EINVAL; }
    if (ctx->rec) { ctx->err = "vp_fft_gkr: a launch plan is being recorded"; return VP_EINVAL; }
    return VP_OK;
}

int vp_fft_gkr(vp_ctx *ctx, int lg, const vp_F *tape, uint64_t n_tape, vp_F *msgs, uint64_t capacity, uint64_t *n_written) {
    if (!ctx || !tape || !msgs) return VP_EINVAL;
    VP_ENTER(ctx);                                       // before anything reads ctx->rec or writes ctx->err: calls on one context are serialised by its lock
    VPCHK(fgk_check_args(ctx, lg, tape, n_tape));
    const u64 n_out = FgkOffsets::n_msgs(lg);
    if (capacity < n_out) { ctx->err = "vp_fft_gkr: message buffer size (vp_fft_gkr_sizes)"; return VP_EINVAL; }
    if (ctx->fgk && ctx->fgk->pending_lg) { ctx->err = "vp_fft_gkr: an asynchronous run is pending (vp_fft_gkr_end / vp_fft_gkr_cancel)"; return VP_EINVAL; }
    VPCHK(fgk_prepare(ctx, lg));
    FgkState &s = *ctx->fgk;
    ctx->st.launches = 0; ctx->st.rounds = 0;
    VPCHK(fgk_enqueue(ctx, lg, tape, n_tape, ctx->stream, ctx->ev0, ctx->ev1));
    HIPCHK(hipMemcpyAsync(s.h_msgs, s.msgs, n_out * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy(msgs, s.h_msgs, n_out * sizeof(F));
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->commit_ms = ms;
    if (n_written) *n_written = n_out;
    return VP_OK;
}

int vp_fft_gkr_begin(vp_ctx *ctx, int lg, const vp_F *tape, uint64_t n_tape) {
    if (!ctx || !tape) return VP_EINVAL;
    VP_ENTER_Q(ctx);                                     // its own stream and buffers: nothing pending on the main stream is in its way
    VPCHK(fgk_check_args(ctx, lg, tape, n_tape));
    if (ctx->profiling) { ctx->err = "vp_fft_gkr_begin: not while launches are being profiled (use vp_fft_gkr)"; return VP_EINVAL; }
    // a run that was begun and never collected (its caller failed in between) is drained and dropped: it must not wedge the context
    if (ctx->fgk && ctx->fgk->pending_lg) { if (ctx->fgk->own_stream) (void) hipStreamSynchronize(ctx->fgk->own_stream); ctx->fgk->pending_lg = 0; }
    VPCHK(fgk_prepare(ctx, lg));
    FgkState &s = *ctx->fgk;
    if (!s.own_stream) {
        // highest priority: its launches are a few workgroups each and must not wait for a gap between the main stream's chip-filling kernels
        int pr_lo = 0, pr_hi = 0;
        (void) hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
        HIPCHK(hipStreamCreateWithPriority(&s.own_stream, hipStreamNonBlocking, pr_hi));
        HIPCHK(hipEventCreate(&s.e0)); HIPCHK(hipEventCreate(&s.e1));
    }
    // (a synchronous vp_fft_gkr drains the main stream before it returns: nothing of it can still be in flight here)
    // The run starts BEHIND whatever this context has queued on its main stream so far: the caller decides beside which kernels its few-workgroup launches
    // run.  Beside a leaf-hash launch they are expensive — that launch is exactly eight rounds of one workgroup per CU (2^21 leaves / 1024 / 256 CUs), and a
    // CU that serves something else for a moment pushes a ninth round onto the launch: 11.4 instead of 10.2 ms (tools/leaf_in_step.py) — beside the
    // transforms and the sumchecks they are free.
    if (!s.e_dep) HIPCHK(hipEventCreateWithFlags(&s.e_dep, hipEventDisableTiming));
    HIPCHK(hipEventRecord(s.e_dep, ctx->stream));
    HIPCHK(hipStreamWaitEvent(s.own_stream, s.e_dep, 0));
    const int rc = fgk_enqueue(ctx, lg, tape, n_tape, s.own_stream, s.e0, s.e1);
    s.lane.stream = ctx->stream;
    if (rc != VP_OK) { (void) hipStreamSynchronize(s.own_stream); return rc; }
    s.pending_lg = lg;
    return VP_OK;
}

int vp_fft_gkr_end(vp_ctx *ctx, vp_F *msgs, uint64_t capacity, uint64_t *n_written) {
    if (!ctx || !msgs) return VP_EINVAL;
    VP_ENTER_Q(ctx);                                     // its own stream and buffers: nothing pending on the main stream is in its way
    if (!ctx->fgk || !ctx->fgk->pending_lg) { ctx->err = "vp_fft_gkr_end: no run pending"; return VP_EINVAL; }
    FgkState &s = *ctx->fgk;
    const u64 n_out = FgkOffsets::n_msgs(s.pending_lg);
    if (capacity < n_out) { ctx->err = "vp_fft_gkr_end: message buffer size (vp_fft_gkr_sizes)"; return VP_EINVAL; }
    s.pending_lg = 0;
    HIPCHK(hipMemcpyAsync(s.h_msgs, s.msgs, n_out * sizeof(F), hipMemcpyDeviceToHost, s.own_stream));
    HIPCHK(hipStreamSynchronize(s.own_stream));
    HIPCHK(hipGetLastError());
    memcpy(msgs, s.h_msgs, n_out * sizeof(F));
    float ms = 0;
    hipEventElapsedTime(&ms, s.e0, s.e1);
    ctx->commit_ms = ms;
    if (n_written) *n_written = n_out;
    return VP_OK;
}

// Drop a run begun with vp_fft_gkr_begin without reading its messages (the caller's pass failed in between).  No run pending: VP_OK.
int vp_fft_gkr_cancel(vp_ctx *ctx) {
    if (!ctx) return VP_EINVAL;
    VP_ENTER_Q(ctx);                                     // its own stream and buffers: nothing pending on the main stream is in its way
    if (!ctx->fgk || !ctx->fgk->pending_lg) return VP_OK;
    if (ctx->fgk->own_stream) (void) hipStreamSynchronize(ctx->fgk->own_stream);
    ctx->fgk->pending_lg = 0;
    return VP_OK;
}

// ---- vp_fft_gkr_fs: every challenge drawn on the device (include/vpgpu.h; kernels: vp_kernels_fftgkr.h) ----------------------------------------------------
// One sumcheck over 2^rounds entries: V of round 1 is V0 (read only: a circuit layer), M and A are s.lane.tab[0][1 / 2].  Challenge k goes to tape slot slot0 + k,
// the messages to out[0 .. 3 rounds].  Above 2^FG_FS_TAIL_LOG entries a round is k_fg_fs_round + k_fg_fs_close, the folded tables alternating between the lane's
// two table sets; the rest is one k_fg_fs_tail, which also absorbs v and draws the n_extra slots from extra0.
static void fgk_fs_sumcheck(vp_ctx *ctx, FgkState &s, hipStream_t st, const F *V0, int rounds, bool has_a, u32 slot0, F *out, u32 extra0, u32 n_extra) {
    const int above = std::max(0, rounds - FG_FS_TAIL_LOG);
    const F *inV = V0, *inM = s.lane.tab[0][1], *inA = has_a ? s.lane.tab[0][2] : nullptr;
    int cur = 0;
    for (int k = 1; k <= above; ++k) {
        FgFsRound a{};
        a.n = 1u << (rounds - k + 1); a.fold = k > 1; a.part = s.fs_part;
        a.inV = inV; a.inM = inM; a.inA = inA;
        if (a.fold) {
            const int nxt = cur ^ 1;
            a.outV = s.lane.tab[nxt][0]; a.outM = s.lane.tab[nxt][1]; a.outA = has_a ? s.lane.tab[nxt][2] : nullptr;
            a.r = s.tape + slot0 + (k - 2);
            cur = nxt;
        }
        const u32 pairs = a.n >> 1, grid = grid_for(pairs);
        const u64 tabs = has_a ? 3 : 2;
        int sl = prof_begin(ctx, st, VP_K_ROUND, grid, 1, 16ull * tabs * ((a.fold ? 2ull * a.n : 0ull) + a.n), pairs, 1, (u32) k);
        if (has_a) hipLaunchKernelGGL(k_fg_fs_round<true>, dim3(grid), dim3(VP_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(k_fg_fs_round<false>, dim3(grid), dim3(VP_BLOCK), 0, st, a);
        prof_end(ctx, st, sl);
        sl = prof_begin(ctx, st, VP_K_EMIT, 1, 1, 48ull * grid, 4, 1, (u32) k);
        hipLaunchKernelGGL(k_fg_fs_close, dim3(1), dim3(VP_BLOCK), 0, st, (const F *) s.fs_part, grid, out + 3 * (k - 1), s.fs_state, s.tape, slot0 + (u32) (k - 1));
        prof_end(ctx, st, sl);
        ctx->st.launches += 2;
        if (a.fold) { inV = a.outV; inM = a.outM; inA = a.outA; }
    }
    FgFsTail t{};
    t.inV = inV; t.inM = inM; t.inA = inA; t.r_fold = above ? s.tape + slot0 + (above - 1) : nullptr;
    t.rounds = rounds - above; t.n = 1u << t.rounds;
    t.poly = out + 3 * above; t.state = s.fs_state; t.tape = s.tape; t.slot0 = slot0 + (u32) above; t.extra0 = extra0; t.n_extra = n_extra;
    const u32 lds = (u32) (FG_FS_TABLES * sizeof(F)) * t.n;
    const int sl = prof_begin(ctx, st, VP_K_SEG, 1, 1, 16ull * (has_a ? 3 : 2) * (above ? 2ull * t.n : t.n), 4ull * t.rounds + 1 + n_extra, (u32) t.rounds, (u32) above + 1);
    if (has_a) hipLaunchKernelGGL(k_fg_fs_tail<true>, dim3(1), dim3(VP_BLOCK), lds, st, t);
    else hipLaunchKernelGGL(k_fg_fs_tail<false>, dim3(1), dim3(VP_BLOCK), lds, st, t);
    prof_end(ctx, st, sl);
    ++ctx->st.launches;
    ctx->st.rounds += rounds;
}

int vp_fft_gkr_fs(vp_ctx *ctx, int lg, const uint8_t state_in[32], vp_F *msgs, uint64_t capacity, uint64_t *n_written, vp_F *tape_out, uint8_t state_out[32]) {
    if (!ctx) return VP_EINVAL;
    VP_ENTER(ctx);
    // every refusal before anything is allocated or queued
    if (!state_in || !msgs || !tape_out || !state_out) { ctx->err = "vp_fft_gkr_fs: a null argument"; return VP_EINVAL; }
    if (lg < 1 || lg > 19) { ctx->err = "vp_fft_gkr_fs: lg out of range (1..19)"; return VP_ELIMIT; }
    const FgkOffsets o(lg);
    const u64 n_out = FgkOffsets::n_msgs(lg);
    if (capacity < n_out) { ctx->err = "vp_fft_gkr_fs: message buffer size (vp_fft_gkr_sizes)"; return VP_EINVAL; }
    if (ctx->rec) { ctx->err = "vp_fft_gkr_fs: a launch plan is being recorded"; return VP_EINVAL; }
    if (ctx->fgk && ctx->fgk->pending_lg) { ctx->err = "vp_fft_gkr_fs: an asynchronous run is pending (vp_fft_gkr_end / vp_fft_gkr_cancel)"; return VP_EINVAL; }
    VPCHK(fgk_prepare(ctx, lg));
    FgkState &s = *ctx->fgk;
    const hipStream_t st = ctx->stream;
    const u32 N = 1u << lg;
    s.lane.stream = st;
    ctx->st.launches = 0; ctx->st.rounds = 0;
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    memcpy(s.h_tape, state_in, 32);                        // pinned; the caller's buffer may be pageable
    HIPCHK(hipMemcpyAsync(s.fs_state, s.h_tape, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->ev0, st));
    // ---- r and x, the circuit, the outputs, r_0 and r_1
    int sl = prof_begin(ctx, st, VP_K_MERKLE, 1, 1, 16ull * (lg + 64), (u64) lg + 64);
    hipLaunchKernelGGL(k_fg_fs_draw, dim3(1), dim3(64), 0, st, s.fs_state, (const F *) nullptr, 0u, s.tape, (u32) o.r, (u32) lg + 64u);
    prof_end(ctx, st, sl);
    VPCHK(fgk_circuit(ctx, s, lg, st));
    sl = prof_begin(ctx, st, VP_K_MERKLE, 1, 1, 16ull * (64 + 2 * (lg + 10)), 64ull + 2 * (lg + 10));
    hipLaunchKernelGGL(k_fg_fs_draw, dim3(1), dim3(64), 0, st, s.fs_state, (const F *) s.msgs, 64u, s.tape, (u32) o.r0, 2u * ((u32) lg + 10u));
    prof_end(ctx, st, sl);
    ctx->st.launches += 2;
    u64 pos = 64;
    // ---- addition layer: claim point r_0[0..6), alpha = 1, beta = 0; its r_v are drawn behind v_u
    hipLaunchKernelGGL(k_fg_gtab, dim3(1), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.r0), (const F *) nullptr, 6, (const F *) nullptr, (const F *) nullptr, s.hi);
    hipLaunchKernelGGL(k_fg_add_init, dim3(nblk((u64) 64 * N)), dim3(VP_BLOCK), 0, st, (const F *) s.hi, lg, s.lane.tab[0][1]);
    fgk_fs_sumcheck(ctx, s, st, s.Pm, lg + 6, false, (u32) o.ru_a, s.msgs + pos, (u32) o.rv_a, (u32) lg + 6u);
    pos += 3 * (lg + 6) + 1;
    // ---- multiplication layer: claim point = the addition layer's r_u
    hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_a), (const F *) nullptr, lg, (const F *) nullptr, (const F *) nullptr, s.g);
    hipLaunchKernelGGL(k_fg_gtab, dim3(1), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_a + lg), (const F *) nullptr, 6, (const F *) nullptr, (const F *) nullptr, s.hi);
    hipLaunchKernelGGL(k_fg_mul_init, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) s.g, (const F *) s.hi, (const F *) s.xt, lg, s.lane.tab[0][1]);
    fgk_fs_sumcheck(ctx, s, st, s.S, lg, false, (u32) o.ru_m, s.msgs + pos, (u32) o.rv_m, (u32) lg);
    pos += 3 * lg + 1;
    // ---- inverse FFT, top layer first, depth by depth (the per-depth loop of fgk_enqueue: depth d's tables need the draws of depth d - 1)
    for (int d = 0; d < lg; ++d) {
        const F *r0 = s.tape + (d ? o.ru_d(d - 1) : o.ru_m), *r1 = s.tape + (d ? o.rv_d(d - 1) : o.rv_m);
        const F *al = d ? s.tape + o.alpha_d(d - 1) : nullptr, *be = d ? s.tape + o.beta_d(d - 1) : nullptr;
        const F *pre = s.B + (size_t) (lg - d - 1) * N;
        hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, r0, r1, lg, al, be, s.g);
        hipLaunchKernelGGL(k_fg_ifft_p1, dim3(nblk(N / 2)), dim3(VP_BLOCK), 0, st, (const F *) s.g, pre, (const F *) s.winv, lg, d, s.lane.tab[0][1], s.lane.tab[0][2]);
        fgk_fs_sumcheck(ctx, s, st, pre, lg, true, (u32) o.ru_d(d), s.msgs + pos, 0u, 0u);
        const F *vu = s.msgs + pos + 3 * lg;
        pos += 3 * lg + 1;
        hipLaunchKernelGGL(k_fg_gtab, dim3(nblk(N)), dim3(VP_BLOCK), 0, st, (const F *) (s.tape + o.ru_d(d)), (const F *) nullptr, lg, (const F *) nullptr, (const F *) nullptr, s.eu);
        hipLaunchKernelGGL(k_fg_ifft_p2, dim3(nblk(N / 2)), dim3(VP_BLOCK), 0, st, (const F *) s.g, (const F *) s.eu, vu, (const F *) s.winv, lg, d, s.lane.tab[0][1], s.lane.tab[0][2]);
        fgk_fs_sumcheck(ctx, s, st, pre, lg, true, (u32) o.rv_d(d), s.msgs + pos, (u32) o.alpha_d(d), 2u);
        pos += 3 * lg + 1;
    }
    if (pos != n_out) { (void) hipStreamSynchronize(st); ctx->err = "internal: fft_gkr message count"; return VP_EINVAL; }
    HIPCHK(hipEventRecord(ctx->ev1, st));
    // ---- messages | tape | state: one block, one copy
    HIPCHK(hipMemcpyAsync(s.h_msgs, s.msgs, (n_out + o.n + 2) * sizeof(F), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    memcpy(msgs, s.h_msgs, n_out * sizeof(F));
    memcpy(tape_out, s.h_msgs + n_out, o.n * sizeof(F));
    memcpy(state_out, s.h_msgs + n_out + o.n, 32);
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->commit_ms = ms;
    if (ctx->profiling) prof_collect(ctx);
    if (n_written) *n_written = n_out;
    return VP_OK;
}

}  // extern "C"

// vp_warm (include/vpgpu.h): first-use set-up ahead of the first prover call.  VP_WARM_COMMITMENT: pc_warm (vpgpu_pc.inc).  VP_WARM_FFT_GKR: the buffers of
// fft_gkr at the size the commitment's verifier asks for (lg = input bit length - 6, vpd_verifier.cpp:92), ~20 device arrays.
// The HIP runtime builds its function object of a kernel (symbol lookup in the 5 MB code object, kernel descriptor, attributes) on the kernel's FIRST launch in
// the process: measured on MI355X (tools/first_use_probe.py), the ~25 kernels of vp_fft_gkr cost its first run 13-20 ms against 1.3 ms afterwards.  Asking
// for a kernel's attributes does the same work without a launch.
static void warm_kernel_functions() {
    static const void *const fns[] = {
        // commitment
        (const void *) k_ntt8_colsx<6>, (const void *) k_ntt8_colsx<7>, (const void *) k_ntt8_colsx<8>, (const void *) k_ntt8_cols<true>, (const void *) k_ntt8_cols<false>,
        (const void *) k_ntt8_rows<true>, (const void *) k_ntt8_rows<false>, (const void *) k_ntt_lds, (const void *) k_leaf_hash<false>, (const void *) k_leaf_hash<true>,
        (const void *) k_leaf_hash_c, (const void *) k_merkle_level, (const void *) k_merkle_top, (const void *) k_pc_products, (const void *) k_pc_quotient, (const void *) k_pc_rank1_check,
        (const void *) k_pc_dot, (const void *) k_pc_sum_parts, (const void *) k_pc_open, (const void *) k_beta_half, (const void *) k_beta_expand, (const void *) k_zero_f,
        (const void *) k_fri_fold, (const void *) k_fri_fold0_vo, (const void *) k_fri_fold0_vo3<true, VP_VO_GRP>, (const void *) k_fri_fold0_vo3<false, VP_VO_GRP>, (const void *) k_fri_fold0_vo3<true, 1>, (const void *) k_fri_fold0_vo3<false, 1>,
        // the commitment with a mask slice (its leaf chains: k_leaf_hash<true> above)
        (const void *) k_mask_vo, (const void *) k_fri_fold_one,
        // fft_gkr
        (const void *) k_fg_pows, (const void *) k_fg_expand, (const void *) k_fg_butterfly, (const void *) k_fg_xsq, (const void *) k_fg_xtab, (const void *) k_fg_polyeval,
        (const void *) k_fg_rowsum, (const void *) k_fg_gtab, (const void *) k_fg_add_init, (const void *) k_fg_mul_init, (const void *) k_fg_gtab_multi, (const void *) k_fg_dot_multi,
        (const void *) k_fg_ifft_multi, (const void *) k_fg_ifft_p1, (const void *) k_fg_ifft_p2, (const void *) k_sumfold3b<true>, (const void *) k_sumfold3b<false>,
        (const void *) k_seg<true>, (const void *) k_seg<false>, (const void *) k_emit,
        (const void *) k_fg_fs_draw, (const void *) k_fg_fs_round<true>, (const void *) k_fg_fs_round<false>, (const void *) k_fg_fs_close, (const void *) k_fg_fs_tail<true>, (const void *) k_fg_fs_tail<false>,
        // the batched proof and the interactive entry points
        (const void *) k_light_multi, (const void *) k_chunks_multi, (const void *) k_combine_multi, (const void *) k_dot_multi, (const void *) k_dotfin_multi,
        (const void *) k_sumfold3b_multi, (const void *) k_sumfold3b_gen_multi, (const void *) k_seg_multi, (const void *) k_emit_multi, (const void *) k_fixup,
        (const void *) k_beta_half_direct, (const void *) k_beta_half_multi, (const void *) k_vres, (const void *) k_vres2, (const void *) k_tape_in, (const void *) k_ship, (const void *) k_ticket,
        (const void *) k_round_main<0>, (const void *) k_round_main<1>, (const void *) k_round_fused, (const void *) k_round_final, (const void *) k_finalize, (const void *) k_phase,
        // vp_prove_gkr_fs
        (const void *) k_gkr_fs_span, (const void *) k_round_main_fs, (const void *) k_round_fused_fs, (const void *) k_round_final_fs, (const void *) k_gkr_fs_ship,
    };
    for (const void *f : fns) { hipFuncAttributes a; (void) hipFuncGetAttributes(&a, f); }
    (void) hipGetLastError();
}
int vp_warm(vp_ctx *ctx, uint32_t what) {
    if (!ctx || !ctx->evaluated) return VP_EINVAL;
    VP_ENTER(ctx);
    if (what) warm_kernel_functions();
    if (what & VP_WARM_COMMITMENT) VPCHK(pc_warm(ctx));
    if (what & VP_WARM_FFT_GKR) {
        const int lg = ctx->L[0].bl - 6;
        if (lg >= 1 && lg <= 20 && !(ctx->fgk && ctx->fgk->pending_lg) && !ctx->rec) {
            VPCHK(fgk_prepare(ctx, lg));
            if (ctx->opt.fft_gkr_batched) VPCHK(fgk_prepare_batch(ctx, lg));     // the batched form's ~240 small arrays and its recorded launches
            // the stream and events of vp_fft_gkr_begin, and the hardware queue behind the stream (the runtime makes it on the stream's first use)
            FgkState &s = *ctx->fgk;
            if (!s.own_stream) {
                int pr_lo = 0, pr_hi = 0;
                (void) hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
                HIPCHK(hipStreamCreateWithPriority(&s.own_stream, hipStreamNonBlocking, pr_hi));
                HIPCHK(hipEventCreate(&s.e0)); HIPCHK(hipEventCreate(&s.e1));
            }
            if (!s.e_dep) HIPCHK(hipEventCreateWithFlags(&s.e_dep, hipEventDisableTiming));
            // one run on an all-zero tape on each of the two streams fft_gkr can run on (its own: vp_fft_gkr_begin; the context's: vp_fft_gkr): whatever the
            // runtime sets up on a queue's first dispatch of these kernels (scratch for the closing kernels' private arrays, measured 7-14 ms) happens here; the
            // messages of the run are dropped
            {
                const std::vector<vp_F> zero_tape(FgkOffsets(lg).n, vp_F{0, 0});
                VPCHK(fgk_enqueue(ctx, lg, zero_tape.data(), zero_tape.size(), s.own_stream, s.e0, s.e1));
                HIPCHK(hipStreamSynchronize(s.own_stream));
                VPCHK(fgk_enqueue(ctx, lg, zero_tape.data(), zero_tape.size(), ctx->stream, ctx->ev0, ctx->ev1));
                HIPCHK(hipStreamSynchronize(ctx->stream));
                s.lane.stream = ctx->stream;
            }
        }
    }
    return check_stream(ctx);
}

