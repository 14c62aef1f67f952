// Part of vpgpu.hip (included at its end): host side of the commitment verifier's device loops, vp_pc_public_evals and vp_fri_query_digests
// (kernels: vp_kernels_pcverify.h).  Verifier-side helpers like vp_predicates: public data in, values out, no accept / reject here.
namespace {

bool pv_leaves_ok(int n, int n_queries, const uint64_t *leaf0) {
    const u64 lo = 1ull << (n - 7), hi = 1ull << (n - 2);                  // [N / 2, M / 2): pow = 2 leaf is even and in [N, M) (vpd_verifier.cpp:119-123)
    for (int q = 0; q < n_queries; ++q) if (leaf0[q] < lo || leaf0[q] >= hi) return false;
    return true;
}
u64 pv_answer_bytes(int n, u64 n_queries) {                               // vp_fri_query's layout for (n, n_queries)
    u64 per = 2 * (2080 + 32ull * (n - 1));
    for (int k = 0; k < n - 6; ++k) per += 2080 + 32ull * (n - 2 - k);
    return per * n_queries;
}
// the order-2^lm root table these calls transform and evaluate with: the context's own when it is of that order, else one kept for the size
int pv_root_table(vp_ctx *ctx, int lm, F **rt) {
    if (ctx->pc_rt && ctx->pc_lm == lm) { *rt = ctx->pc_rt; return VP_OK; }
    auto it = ctx->pv_rt.find(lm);
    if (it == ctx->pv_rt.end()) {
        F *t = nullptr;
        VPCHK(dalloc(ctx, &t, (size_t) 1 << (lm - 1)));
        VPCHK(pc_root_fill(ctx, t, lm));
        it = ctx->pv_rt.emplace(lm, t).first;
    }
    *rt = it->second;
    return VP_OK;
}

// The device arena both calls work in: kept on the context and grown to the largest request, like the transforms' scratch (pc_scratch_reserve) — a call
// allocates only when it needs more than any call before it, and nothing is freed per call (a hipFree would synchronise the whole device).
int pv_reserve(vp_ctx *ctx, size_t n_elems) {
    if (ctx->pv_buf && ctx->pv_cap >= n_elems) return VP_OK;
    F *fresh = nullptr;
    VPCHK(dalloc(ctx, &fresh, n_elems));
    if (ctx->pv_buf) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *) ctx->pv_buf);
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        (void) hipFree(ctx->pv_buf);
    }
    ctx->pv_buf = fresh; ctx->pv_cap = n_elems;
    return VP_OK;
}
// the transform launchers read the root table from the context: for the span of this object they see `rt`, and the context's own table is back on every way out
struct PvRootScope {
    vp_ctx *c; F *rt; int lm;
    PvRootScope(vp_ctx *ctx, F *t, int l) : c(ctx), rt(ctx->pc_rt), lm(ctx->pc_lm) { c->pc_rt = t; c->pc_lm = l; }
    ~PvRootScope() { c->pc_rt = rt; c->pc_lm = lm; }
    PvRootScope(const PvRootScope &) = delete; PvRootScope &operator=(const PvRootScope &) = delete;
};

// behind the checks: arena, table / upload, inverse transforms, the evaluation launch and its closing launch, one copy out
int pv_public_evals(vp_ctx *ctx, int n, const vp_F *point, const vp_F *pub, int n_queries, const uint64_t *leaf0, vp_F *out) {
    const int ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, rows = point ? 1 : 64, nq = (u32) n_queries;
    const u32 NP = N / 2, chunks = (NP + PEV_PAIRS - 1) / PEV_PAIRS;
    const size_t half = (size_t) 1 << ((ln + 1) / 2);
    // one arena: input rows | coefficients | partial sums | results | slice factors | point | half tables | leaves
    const size_t n_in = (size_t) rows * N, n_part = (size_t) rows * nq * chunks * 2, n_out = (size_t) nq * 128;
    const size_t total = 2 * n_in + n_part + n_out + 64 + 32 + 2 * half + (nq + 1) / 2;
    VPCHK(pv_reserve(ctx, total));
    F *base = ctx->pv_buf;
    F *d_in = base, *d_coef = d_in + n_in, *d_part = d_coef + n_in, *d_out = d_part + n_part, *d_scale = d_out + n_out, *d_r = d_scale + 64,
      *d_bf = d_r + 32, *d_bs = d_bf + half;
    u64 *d_leaf = reinterpret_cast<u64 *>(d_bs + half);
    F *rt = nullptr;
    VPCHK(pv_root_table(ctx, lm, &rt));
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    // small inputs through the pinned ring (taken by the stream before the call returns: check_stream below)
    unsigned char *h = nullptr;
    VPCHK(ring_alloc(ctx, (64 + 32) * sizeof(F) + (size_t) nq * 8, (void **) &h));
    F *h_scale = reinterpret_cast<F *>(h), *h_r = h_scale + 64;
    u64 *h_leaf = reinterpret_cast<u64 *>(h_r + 32);
    for (u32 q = 0; q < nq; ++q) h_leaf[q] = leaf0[q];
    HIPCHK(hipMemcpyAsync(d_leaf, h_leaf, (size_t) nq * 8, hipMemcpyHostToDevice, ctx->stream));
    if (point) {
        // eq(point, j N + i) = hi(j) lo(i): lo is built on the device (the eq builders of vp_commit_public_eq, on the low ln coordinates), hi's 64 values here
        for (int i = 0; i < ln; ++i) h_r[i] = f_make(point[i].real, point[i].img);
        h_r[ln] = f_one();
        for (u32 j = 0; j < 64; ++j) {
            F e = f_one();
            for (int i = 0; i < 6; ++i) { const F r = f_make(point[ln + i].real, point[ln + i].img); e = f_mul(e, ((j >> i) & 1u) ? r : f_sub(f_one(), r)); }
            h_scale[j] = e;
        }
        HIPCHK(hipMemcpyAsync(d_r, h_r, (size_t) (ln + 1) * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_scale, h_scale, 64 * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_beta_half, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, (const F *) d_r, ln, (const F *) (d_r + ln), d_bf, d_bs);
        PC_PROF(VP_K_PC_POINTWISE, grid_for(N), 1, 16ull * N, N,
                hipLaunchKernelGGL(k_beta_expand, dim3(grid_for(N)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) d_bf, (const F *) d_bs, ln >> 1, N, d_in));
    } else
        VPCHK(pc_upload_pub(ctx, pub, sizeof(F) << n, d_in));
    {   // the slices' interpolants: the commitment's inverse transforms (1 / N included), on the table of this size
        PvRootScope scope(ctx, rt, lm);
        VPCHK(pc_launch_ntt(ctx, d_in, d_coef, ln, lm, 1, rows, 1, N));
    }
    PolyEvalArgs a{};
    a.coef = d_coef; a.RT = rt; a.half_m = 1u << (lm - 1); a.leaf = d_leaf; a.part = d_part; a.ln = (u32) ln; a.n_q = nq; a.chunks = chunks;
    // query groups: enough workgroups to fill the chip when the rows are short, as few coefficient loads as that allows
    u32 groups = std::min<u32>(nq, std::max<u32>(1, 1024 / (chunks * rows)));
    a.q_per_group = (nq + groups - 1) / groups;
    groups = (nq + a.q_per_group - 1) / a.q_per_group;
    const dim3 g(chunks, rows, groups);
    // work: the products the launch executes — per row and query 2 PEV_PAIRS per workgroup (2 x 7 Horner steps + 2 scalings in each of 256 threads), = N for full rows
    PC_PROF(VP_K_PC_POLY_EVAL, g.x * g.y * g.z, rows, 16ull * N * rows * groups, (u64) rows * nq * 2ull * PEV_PAIRS * chunks,
            hipLaunchKernelGGL(k_pc_poly_eval, g, dim3(VP_BLOCK), 0, ctx->stream, a));
    PC_PROF(VP_K_PC_POLY_EVAL_FIN, nblk((u64) nq * 64), rows, 32ull * n_part / 2 + 16ull * n_out, (u64) nq * 64 * (point ? 3 : 1),
            hipLaunchKernelGGL(k_pc_poly_eval_fin, dim3(nblk((u64) nq * 64)), dim3(VP_BLOCK), 0, ctx->stream, a, point ? (const F *) d_scale : (const F *) nullptr, d_out));
    HIPCHK(hipMemcpyAsync(out, d_out, n_out * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    const int rc = check_stream(ctx);
    if (rc == VP_OK && ctx->profiling) prof_collect(ctx);
    return rc;
}

// the mask row: one row of ms values (the public mask, zero-padded) -> its interpolant on the ms-th roots by the commitment's inverse transform of that size (as
// pc_mask_lde runs it) -> k_pc_poly_eval over that one row on the domain of order M -> k_pc_mask_eval_fin.  The row length (lg) and the domain (lm) are independent.
int pv_mask_evals(vp_ctx *ctx, int n, const vp_F *pub_mask, u64 n_pub_mask, u32 ms, int n_queries, const uint64_t *leaf0, vp_F *out) {
    const int lm = n - 1, lg = ilog2(ms);
    const u32 nq = (u32) n_queries, NP = ms / 2, chunks = (NP + PEV_PAIRS - 1) / PEV_PAIRS;
    // one arena: values | coefficients | partial sums | results | leaves
    const size_t n_part = (size_t) nq * chunks * 2, n_out = (size_t) nq * 2;
    VPCHK(pv_reserve(ctx, 2 * (size_t) ms + n_part + n_out + (nq + 1) / 2));
    F *d_in = ctx->pv_buf, *d_coef = d_in + ms, *d_part = d_coef + ms, *d_out = d_part + n_part;
    u64 *d_leaf = reinterpret_cast<u64 *>(d_out + n_out);
    F *rt = nullptr;
    VPCHK(pv_root_table(ctx, lm, &rt));
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    F *h_mask = nullptr;                                // pinned until the stream has taken it (ms <= 2^16: 1 MB, the ring's largest single request)
    u64 *h_leaf = nullptr;
    VPCHK(ring_alloc(ctx, (size_t) ms * sizeof(F), (void **) &h_mask));
    VPCHK(ring_alloc(ctx, (size_t) nq * 8, (void **) &h_leaf));
    for (u32 i = 0; i < ms; ++i) h_mask[i] = i < n_pub_mask ? f_make(pub_mask[i].real, pub_mask[i].img) : f_zero();
    for (u32 q = 0; q < nq; ++q) h_leaf[q] = leaf0[q];
    HIPCHK(hipMemcpyAsync(d_in, h_mask, (size_t) ms * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_leaf, h_leaf, (size_t) nq * 8, hipMemcpyHostToDevice, ctx->stream));
    {
        PvRootScope scope(ctx, rt, lm);
        VPCHK(pc_launch_ntt(ctx, d_in, d_coef, lg, lm, 1, 1, 1, ms));
    }
    PolyEvalArgs a{};
    a.coef = d_coef; a.RT = rt; a.half_m = 1u << (lm - 1); a.leaf = d_leaf; a.part = d_part; a.ln = (u32) lg; a.n_q = nq; a.chunks = chunks;
    u32 groups = std::min<u32>(nq, std::max<u32>(1, 1024 / chunks));
    a.q_per_group = (nq + groups - 1) / groups;
    groups = (nq + a.q_per_group - 1) / a.q_per_group;
    const dim3 g(chunks, 1, groups);
    PC_PROF(VP_K_PC_POLY_EVAL, g.x * g.y * g.z, 1, 16ull * ms * groups, (u64) nq * 2ull * PEV_PAIRS * chunks,
            hipLaunchKernelGGL(k_pc_poly_eval, g, dim3(VP_BLOCK), 0, ctx->stream, a));
    PC_PROF(VP_K_PC_POLY_EVAL_FIN, nblk((u64) nq), 1, 32ull * n_part / 2 + 16ull * n_out, (u64) nq,
            hipLaunchKernelGGL(k_pc_mask_eval_fin, dim3(nblk((u64) nq)), dim3(VP_BLOCK), 0, ctx->stream, a, d_out));
    HIPCHK(hipMemcpyAsync(out, d_out, n_out * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    const int rc = check_stream(ctx);
    if (rc == VP_OK && ctx->profiling) prof_collect(ctx);
    return rc;
}

}  // namespace

extern "C" {

int vp_pc_mask_evals(vp_ctx *ctx, int n, const vp_F *pub_mask, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, vp_F *out) {
    if (!ctx) return VP_EINVAL;
    if (n < 7) { ctx->err = "vp_pc_mask_evals: the commitment needs an input layer of at least 2^7 wires"; return VP_EINVAL; }
    if (n > PC_MAX_N) { ctx->err = "vp_pc_mask_evals: input layer above 2^25 wires"; return VP_ELIMIT; }
    if (!out || !leaf0 || n_queries < 1 || n_queries > 4096) { ctx->err = "vp_pc_mask_evals: 1 .. 4096 queries, leaf0 and out"; return VP_EINVAL; }
    if (!pv_leaves_ok(n, n_queries, leaf0)) { ctx->err = "vp_pc_mask_evals: a leaf outside [N / 2, M / 2)"; return VP_EINVAL; }
    if (ms < 8 || (ms & (ms - 1)) || ms > (1ull << 16) || ms > (1ull << (n - 2))) { ctx->err = "vp_pc_mask_evals: ms is no power of two in [8, min(2^16, 2^(n-2))]"; return VP_EINVAL; }
    if (!pub_mask || n_pub_mask < 1 || n_pub_mask > ms) { ctx->err = "vp_pc_mask_evals: a public mask of 1 .. ms elements"; return VP_EINVAL; }
    for (u64 i = 0; i < n_pub_mask; ++i) if (pub_mask[i].real >= P61 || pub_mask[i].img >= P61) { ctx->err = "vp_pc_mask_evals: non-canonical limb in the public mask"; return VP_EINVAL; }
    VP_ENTER(ctx);
    return pv_mask_evals(ctx, n, pub_mask, n_pub_mask, (u32) ms, n_queries, leaf0, out);
}

int vp_pc_public_evals(vp_ctx *ctx, int n, const vp_F *point, const vp_F *pub, int n_queries, const uint64_t *leaf0, vp_F *out) {
    if (!ctx) return VP_EINVAL;
    if (n < 7) { ctx->err = "vp_pc_public_evals: the commitment needs an input layer of at least 2^7 wires"; return VP_EINVAL; }
    if (n > PC_MAX_N) { ctx->err = "vp_pc_public_evals: input layer above 2^25 wires"; return VP_ELIMIT; }
    if ((point == nullptr) == (pub == nullptr)) { ctx->err = "vp_pc_public_evals: exactly one of point and pub"; return VP_EINVAL; }
    if (!out || !leaf0 || n_queries < 1 || n_queries > 4096) { ctx->err = "vp_pc_public_evals: 1 .. 4096 queries, leaf0 and out"; return VP_EINVAL; }
    if (!pv_leaves_ok(n, n_queries, leaf0)) { ctx->err = "vp_pc_public_evals: a leaf outside [N / 2, M / 2)"; return VP_EINVAL; }
    const vp_F *v = point ? point : pub;
    const u64 nv = point ? (u64) n : 1ull << n;
    for (u64 i = 0; i < nv; ++i) if (v[i].real >= P61 || v[i].img >= P61) { ctx->err = "vp_pc_public_evals: non-canonical limb in the point / the public vector"; return VP_EINVAL; }
    VP_ENTER(ctx);
    return pv_public_evals(ctx, n, point, pub, n_queries, leaf0, out);
}

int vp_fri_query_digests(vp_ctx *ctx, int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out) {
    if (!ctx) return VP_EINVAL;
    if (n < 7) { ctx->err = "vp_fri_query_digests: the commitment needs an input layer of at least 2^7 wires"; return VP_EINVAL; }
    if (n > PC_MAX_N) { ctx->err = "vp_fri_query_digests: input layer above 2^25 wires"; return VP_ELIMIT; }
    if (!answer || !out || !leaf0 || n_queries < 1 || n_queries > 4096) { ctx->err = "vp_fri_query_digests: 1 .. 4096 queries, leaf0, answer and out"; return VP_EINVAL; }
    if (!pv_leaves_ok(n, n_queries, leaf0)) { ctx->err = "vp_fri_query_digests: a leaf outside [N / 2, M / 2)"; return VP_EINVAL; }
    if (n_bytes != pv_answer_bytes(n, (u64) n_queries)) { ctx->err = "vp_fri_query_digests: n_bytes is not the size of vp_fri_query's answer for (n, n_queries)"; return VP_EINVAL; }
    VP_ENTER(ctx);
    const u32 nq = (u32) n_queries, n_open = nq * (u32) (n - 4);
    // arena: leaves | answer | digests.  The answer is copied once, from the caller's memory; the leaf list (8 bytes a position) rides in front of it through the pinned ring
    const size_t in_words = (size_t) nq + n_bytes / 8, in_elems = (in_words + 1) / 2;
    VPCHK(pv_reserve(ctx, in_elems + (size_t) n_open * 4));
    u64 *d_in = reinterpret_cast<u64 *>(ctx->pv_buf);
    Dig *d_out = reinterpret_cast<Dig *>(ctx->pv_buf + in_elems);
    u64 *h_leaf = nullptr;
    VPCHK(ring_alloc(ctx, (size_t) nq * 8, (void **) &h_leaf));
    for (u32 q = 0; q < nq; ++q) h_leaf[q] = leaf0[q];
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    HIPCHK(hipMemcpyAsync(d_in, h_leaf, (size_t) nq * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_in + nq, answer, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    const u32 grid = (n_open + POD_THREADS - 1) / POD_THREADS;
    u64 perms = 0;
    for (int o = 0; o < n - 4; ++o) perms += 65 + (u64) (o < 2 ? n - 2 : n - 3 - (o - 2));
    PC_PROF(VP_K_PC_OPENING_DIGESTS, grid, n_open, n_bytes, perms * nq,
            hipLaunchKernelGGL(k_pc_opening_digests, dim3(grid), dim3(POD_THREADS), 0, ctx->stream, (const u64 *) d_in, (u32) n, nq, n_bytes / nq, d_out));
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t) n_open * 64, hipMemcpyDeviceToHost, ctx->stream));
    const int rc = check_stream(ctx);
    if (rc == VP_OK && ctx->profiling) prof_collect(ctx);
    return rc;
}

}  // extern "C"
