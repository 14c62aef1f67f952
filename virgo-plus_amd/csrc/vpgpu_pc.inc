// Part of vpgpu.hip (included at its end): host side of the Virgo polynomial commitment entry points.
// =====================================================================================================
// Virgo polynomial commitment — commit side
//
// The arithmetic between a public vector on the device and the encoded quotient h exists once, pc_quotient_slices, and runs over a PcSlices view: the
// 64 slices of a context here, a rank's 64 / W in vpgpu_pc_shard.inc.  What differs between the two stays with the callers: the form of the inner product,
// masks, hashing (at once or late), the pack and the collectives.  The virtual oracle and the first FRI fold read l, q, h, S_0 and the tensor pair through
// the same view; the eq corners of vp_commit_public_eq come from vp_pc_corners.h on both sides.
// =====================================================================================================
namespace {

constexpr int PC_MAX_LN = 13;            // largest in-LDS transform (2^13 x 16 B = 128 KiB)
// LDS transform size behind the register split of the longer transforms: 2^12 points = 64 KiB, so that TWO workgroups share a CU and
// one loads / stores while the other computes (a 2^13-point workgroup owns the CU alone and its load, butterfly and store phases
// run back to back).  Measured, same call, x1024 commit side: k_ntt_lds 19.5 -> 14.6 ms, but the 32-point register split in front of it
// (228 VGPRs, 97 instead of 41 multiplications per 32 / 16-point column) 9.1 -> 12.1 ms: 85.8 -> 84.5 ms in total.
#ifndef VP_NTT_SPLIT_LOG
#define VP_NTT_SPLIT_LOG 12
#endif
constexpr int PC_SPLIT_LN = VP_NTT_SPLIT_LOG;

// profiled calls (vp_set_profiling): every launch of the commitment is bracketed with events on the library stream (PC_PROF_IF: where the caller says so —
// the per-step FRI path leaves some launches out of the table)
#define PC_PROF_IF(on, kind, grid, jobs, bytes, work, ...)                                               \
    do {                                                                                                  \
        const int sl_ = (on) ? prof_begin(ctx, ctx->stream, (kind), (u32) (grid), (u32) (jobs), (u64) (bytes), (u64) (work)) : -1; \
        __VA_ARGS__;                                      /* the launch */                                \
        prof_end(ctx, ctx->stream, sl_);                                                                  \
    } while (0)
#define PC_PROF(kind, grid, jobs, bytes, work, ...) PC_PROF_IF(true, kind, grid, jobs, bytes, work, __VA_ARGS__)

F host_pow(F x, unsigned __int128 e) { F r = f_one(); while (e) { if (e & 1) r = f_mul(r, x); x = f_mul(x, x); e >>= 1; } return r; }
F host_root_of_unity(int log_order) {    // fieldElement::getRootOfUnity (fieldElement.cpp:237-249)
    F r = f_make(2147483648ull, 1033321771269002680ull);
    for (int i = 0; i < 62 - log_order; ++i) r = f_mul(r, r);
    return r;
}
F host_inv_real(u64 x) { return host_pow(f_make(x, 0), (unsigned __int128) P61 - 2); }   // RS_polynomial.cpp:214

// RT[j] = w^j for j < M/2, M = 2^lm (doubling, one small launch per level; done once per circuit).  pc_root_fill: into a table of the caller's.
int pc_root_fill(vp_ctx *ctx, F *rt, int lm) {
    const u32 half = 1u << (lm - 1);
    const F one = f_one();
    HIPCHK(hipMemcpyAsync(rt, &one, sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    F step = host_root_of_unity(lm);                    // w^(2^s)
    for (u32 have = 1; have < half; have <<= 1) {
        hipLaunchKernelGGL(k_root_table_step, dim3(nblk(have)), dim3(VP_BLOCK), 0, ctx->stream, rt, have, step);
        step = f_mul(step, step);
    }
    return VP_OK;
}
int pc_root_table(vp_ctx *ctx, int lm) {
    if (ctx->pc_lm == lm && ctx->pc_rt) return VP_OK;
    VPCHK(dalloc(ctx, &ctx->pc_rt, (size_t) 1 << (lm - 1)));
    VPCHK(pc_root_fill(ctx, ctx->pc_rt, lm));
    ctx->pc_lm = lm;
    return VP_OK;
}

// RTc[k] = w_(2^lo)^k, k < 2^(lo-1): the roots of a smaller order, contiguous, copied out of the order-2^lm table once (k_root_compact).
// Keyed by the table they come from (vp_test_fft swaps in a private one).
int pc_compact_roots(vp_ctx *ctx, int lm, int lo, const F **out) {
    if (lo >= lm || lo < 2) { *out = ctx->pc_rt; return VP_OK; }
    const auto key = std::make_pair((const void *) ctx->pc_rt, lo);
    auto it = ctx->pc_rtc.find(key);
    if (it == ctx->pc_rtc.end()) {
        F *t = nullptr;
        const u32 n = 1u << (lo - 1);
        VPCHK(dalloc(ctx, &t, (size_t) n));
        hipLaunchKernelGGL(k_root_compact, dim3(nblk(n)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) ctx->pc_rt, 1u << (lm - lo), n, t);
        it = ctx->pc_rtc.emplace(key, t).first;
    }
    *out = it->second;
    return VP_OK;
}

// RTn[k] = w_(2^lo)^k for ALL k < 2^lo (full circle: an inverse transform indexes it with n - e; no negation logic in the butterflies of
// k_ntt8_cols / k_ntt8_rows).  Keyed like the compact tables, with the order negated.
int pc_circle_roots(vp_ctx *ctx, int lm, int lo, const F **out) {
    const auto key = std::make_pair((const void *) ctx->pc_rt, -lo);
    auto it = ctx->pc_rtc.find(key);
    if (it == ctx->pc_rtc.end()) {
        F *t = nullptr;
        const u32 n = 1u << lo;
        VPCHK(dalloc(ctx, &t, (size_t) n));
        hipLaunchKernelGGL(k_root_circle, dim3(nblk(n)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) ctx->pc_rt, 1u << (lm - 1), 1u << (lm - lo), n, t);
        it = ctx->pc_rtc.emplace(key, t).first;
    }
    *out = it->second;
    return VP_OK;
}

// the pre-split copy of a root table (lz_presplit: what k_ntt8_colsx / k_ntt8_rows multiply with), built once per table
int pc_presplit(vp_ctx *ctx, const F *src, u32 n, const F **out) {
    const auto key = std::make_pair((const void *) src, 7777);
    auto it = ctx->pc_rtc.find(key);
    if (it == ctx->pc_rtc.end()) {
        F *t = nullptr;
        VPCHK(dalloc(ctx, &t, (size_t) n));
        hipLaunchKernelGGL(k_root_presplit, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, src, t, n);
        it = ctx->pc_rtc.emplace(key, t).first;
    }
    *out = it->second;
    return VP_OK;
}

// Transforms of 2^13 .. 2^17 points: N = N1 x 512 as two LDS passes of radix-8 Stockham butterflies (vp_kernels_ntt8.h).  Multiplications per
// transform: pass A's own twiddles (7/8 per point and radix-8 pass after the first, 3/4 or 1/2 for a closing radix-4 / radix-2 pass), one per
// point for w_N^(j2 k1), one per point for the coset twist of the encoder; pass B 2 x 7/8 per point (+ 1 for the 1/N of an inverse).
static inline u64 ntt8_cols_mults(int ln, int twist) {
    const int l1 = ln - 9, nr8 = l1 / 3, rem = l1 - 3 * nr8; const u64 N = 1ull << ln;
    return (u64) (nr8 - 1) * (N / 8 * 7) + (rem == 2 ? N / 4 * 3 : rem == 1 ? N / 2 : 0) + N + (twist ? N : 0);
}
static inline u64 ntt8_rows_mults(int ln, int inverse) { const u64 N = 1ull << ln; return 2 * (N / 8 * 7) + (inverse ? N : 0); }
// The shared scratch of the long transforms grows to the largest request: the new buffer is taken first, pointer and capacity change together, and the
// buffer it replaces is released once the stream has drained (it used to stay allocated until the context went away).
int pc_scratch_reserve(vp_ctx *ctx, size_t total) {
    if (ctx->pc_scr_cap >= total && ctx->pc_scr) return VP_OK;
    F *fresh = nullptr;
    VPCHK(dalloc(ctx, &fresh, total));
    if (ctx->pc_scr) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *) ctx->pc_scr);
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        (void) hipFree(ctx->pc_scr);
    }
    ctx->pc_scr = fresh; ctx->pc_scr_cap = total;
    return VP_OK;
}

// k_ntt8_colsx's chunk rule (pc_launch_ntt8: cosets are dealt to `chunks` workgroups per (row, tile) until the launch has 8192 of them; every chunk reloads the
// row's input): 1 = applied to the row count rounded up to a power of two, so the 57 / 29 rows of the live slices (vp_pc_live.h) chunk like 64 / 32; 0 = applied to
// the rows themselves (twice the chunks at 57 and 29 rows: more input reloads).  1 keeps the chunking every earlier measurement of these encodes was made with;
// the other form is not measured yet (profiles/live_slices_ab.md, section 3), which is what the switch is here for.
#ifndef VP_NTT8X_CHUNK_POW2
#define VP_NTT8X_CHUNK_POW2 1
#endif
#ifndef VP_NTT8X
#define VP_NTT8X 1          // forward encodes of 2^15 .. 2^17 points: pass A with the coset loop inside the workgroup (k_ntt8_colsx); 0: k_ntt8_cols everywhere
#endif
// second-pass roots of k_ntt8_colsx for (order M = 2^lm, N1 = 2^l1, N2 = 512), built once per root table
int pc_ntt8x_t2(vp_ctx *ctx, int lm, int ln, int l1, const F **out) {
    const auto key = std::make_pair((const void *) ctx->pc_rt, 1000 + 32 * ln + l1);
    auto it = ctx->pc_rtc.find(key);
    if (it == ctx->pc_rtc.end()) {
        F *t = nullptr;
        const u32 ncoset = 1u << (lm - ln), n2 = 1u << (ln - l1), total = ncoset * n2 * 64;
        VPCHK(dalloc(ctx, &t, (size_t) total));
        hipLaunchKernelGGL(k_ntt8x_t2, dim3(nblk(total)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) ctx->pc_rt, 1u << (lm - 1), (u32) (11 - l1), n2, total, t);
        it = ctx->pc_rtc.emplace(key, t).first;
    }
    *out = it->second;
    return VP_OK;
}
// pair_rows != 0: rows = pair_rows transforms that carry two real sequences each (Ntt8Args): inverse — row p reads slices p and p + pair_rows of `in`; forward — row p
// writes slices p and p + pair_rows of `out` (and reads E_0 of row p from in[p << ln])
int pc_launch_ntt8(vp_ctx *ctx, const F *in, F *out, int ln, int lm, int inverse, u32 rows, u32 cosets, u32 in_stride, u32 pair_rows = 0) {
    const int l1 = ln - 9;
    const u32 N1 = 1u << l1, nc = inverse ? 1 : cosets;
    const size_t N = (size_t) 1 << ln, total = (size_t) rows * nc * N;
    VPCHK(pc_scratch_reserve(ctx, total));
    const F *rt1 = nullptr, *rt9 = nullptr, *rtm = nullptr;
    VPCHK(pc_circle_roots(ctx, lm, l1, &rt1));
    VPCHK(pc_circle_roots(ctx, lm, 9, &rt9));
    Ntt8Args a{};
    a.in = in; a.out = ctx->pc_scr; a.half_m = 1u << (lm - 1); a.RTn = rt1; a.ln = ln; a.l1 = l1; a.in_stride = in_stride;
    a.ncoset = nc; a.twist = (!inverse && cosets > 1) ? 1 : 0; a.do_scale = 0; a.scale = f_one();
    a.in2 = (pair_rows && inverse) ? in + (size_t) pair_rows * in_stride : nullptr; a.pair_rows = 0; a.e0 = nullptr;
    const u64 tr = (u64) rows * nc;
    const bool colsx = VP_NTT8X && a.twist && l1 >= 6 && l1 <= 8 && cosets == (1u << (lm - ln)) && cosets <= 64;
    // every table of both passes first (built once per root table; vp_warm stops here: ctx->pc_dry)
    Ntt8xArgs x{};
    if (colsx) {
        x.in = in; x.out = ctx->pc_scr; x.RTn = rt1; x.ln = ln; x.in_stride = in_stride; x.ncoset = cosets;
        VPCHK(pc_circle_roots(ctx, lm, l1 + (lm - ln), &x.TW));
        VPCHK(pc_circle_roots(ctx, lm, ln, &x.W1));
        VPCHK(pc_ntt8x_t2(ctx, lm, ln, l1, &x.T2));
        // the kernel multiplies with pre-split roots (lz_mul_ps): packed copies of its four tables
        VPCHK(pc_presplit(ctx, x.TW, 1u << (l1 + (lm - ln)), &x.TW));
        VPCHK(pc_presplit(ctx, x.W1, 1u << ln, &x.W1));
        VPCHK(pc_presplit(ctx, x.T2, (1u << (lm - ln)) * (1u << (ln - l1)) * 64u, &x.T2));
        VPCHK(pc_presplit(ctx, x.RTn, 1u << l1, &x.RTn));
    } else {
        VPCHK(pc_circle_roots(ctx, lm, lm, &rtm));               // all M powers (64 MB at x1024): the gathers of k_ntt8_cols carry no sign logic
        a.RT = rtm;
    }
    const F *rt9p = nullptr;
    VPCHK(pc_presplit(ctx, rt9, 512u, &rt9p));                     // k_ntt8_rows' twiddles, pre-split
    const F *rtz = nullptr;
    const bool pair_fwd = pair_rows && !inverse;
    if (pair_fwd) VPCHK(pc_circle_roots(ctx, lm, lm - ln, &rtz));   // zeta_b = w_ncoset^b: the rows pass reads it from the order-M half table (no 64 MB circle needed for 32 values)
    if (ctx->pc_dry) return VP_OK;
    if (colsx) {
        // the encoder's pass A: one workgroup per (row, tile of 2048 / N1 columns, chunk of cosets)
        const u32 tiles = (512u << l1) / NTT8X_TILE;                  // N2 / columns per tile
        u32 chunks = 1;                                               // enough workgroups for ten rounds of the chip's 768 resident ones, as few input loads as that allows
        // (a row count that is no power of two — the live slices, vp_pc_live.h — chunks like the next power of two: 57 of 64 rows keep the 64 rows' input loads;
        // VP_NTT8X_CHUNK_POW2 = 0 applies the rule to the rows themselves, which doubles the chunks at 57 and 29 rows)
        u32 rows_r = rows;
        if (VP_NTT8X_CHUNK_POW2) { rows_r = 1; while (rows_r < rows) rows_r <<= 1; }
        while (chunks < cosets && (u64) rows_r * tiles * chunks < 8192) chunks <<= 1;
        x.cpw = cosets / chunks;
        const dim3 g(rows, tiles, chunks);
        const int sl_ = prof_begin(ctx, ctx->stream, VP_K_NTT8_COLS, (u32) (g.x * g.y * g.z), (u32) tr, 16ull * N * tr + 16ull * N * rows, tr * (ntt8_cols_mults(ln, 1) + N / 8));
        if (l1 == 6) hipLaunchKernelGGL(k_ntt8_colsx<6>, g, dim3(NTT8X_THREADS), 0, ctx->stream, x);
        else if (l1 == 7) hipLaunchKernelGGL(k_ntt8_colsx<7>, g, dim3(NTT8X_THREADS), 0, ctx->stream, x);
        else hipLaunchKernelGGL(k_ntt8_colsx<8>, g, dim3(NTT8X_THREADS), 0, ctx->stream, x);
        prof_end(ctx, ctx->stream, sl_);
    } else {
        const dim3 g(rows, N1 / 8, nc);                           // 4096 / N1 columns per workgroup: 512 N1 / 4096 tiles per transform; rows fastest
        const int sl_ = prof_begin(ctx, ctx->stream, VP_K_NTT8_COLS, (u32) (g.x * g.y * g.z), (u32) tr, 16ull * N * tr + 16ull * N * rows, tr * ntt8_cols_mults(ln, a.twist));
        if (inverse) hipLaunchKernelGGL(k_ntt8_cols<true>, g, dim3(NTT8_THREADS), NTT8_TILE * sizeof(F), ctx->stream, a);
        else hipLaunchKernelGGL(k_ntt8_cols<false>, g, dim3(NTT8_THREADS), NTT8_TILE * sizeof(F), ctx->stream, a);
        prof_end(ctx, ctx->stream, sl_);
    }
    Ntt8Args b = a;
    b.in = ctx->pc_scr; b.out = out; b.RTn = rt9p; b.do_scale = inverse ? 1 : 0; b.scale = inverse ? host_inv_real(1ull << ln) : f_one();
    b.scale = lz_presplit(b.scale);
    b.in2 = nullptr; b.pair_rows = pair_fwd ? pair_rows : 0; b.e0 = b.pair_rows ? in : nullptr;
    if (b.pair_rows) { b.RT = rtz; b.half_m = nc / 2; }
    {
        const dim3 g(N1 / 8, (u32) tr);
        const int sl_ = prof_begin(ctx, ctx->stream, VP_K_NTT8_ROWS, (u32) (g.x * g.y), (u32) tr, 32ull * N * tr, tr * ntt8_rows_mults(ln, inverse));
        if (inverse) hipLaunchKernelGGL(k_ntt8_rows<true>, g, dim3(NTT8_THREADS), 8 * NTT8_PITCH * sizeof(F), ctx->stream, b);
        else hipLaunchKernelGGL(k_ntt8_rows<false>, g, dim3(NTT8_THREADS), 8 * NTT8_PITCH * sizeof(F), ctx->stream, b);
        prof_end(ctx, ctx->stream, sl_);
    }
    return VP_OK;
}

constexpr int PC_MAX_LN_SPLIT = 17;      // with the register split in front: N1 <= 16; also the largest k_ntt8_cols / k_ntt8_rows pair
constexpr int PC_MAX_LN_LONG = 19;       // one radix-2 / radix-4 step around the 2^17-point pair (pc_launch_ntt_long)
constexpr int PC_MAX_N = 25;             // input layer bit length: slices of 2^19 coefficients

// Transforms of 2^18 / 2^19 points (vp_kernels_ntt_long.h): N = N0 x 2^17.  The input rows are dealt into their N0 interleaved sub-sequences
// (k_ntt_long_split), the unchanged 2^17-point pair transforms rows x N0 of them — forward on the root table of order M / N0, with the same
// cosets — and k_ntt_long_merge combines each (row, coset)'s N0 sub-transforms with one radix-N0 step into natural order.  Scratch: the pair's
// own (rows x cosets x N), the sub-transforms' outputs (the same again; none for one coset: they sit in `out` and the merge runs in place)
// and the dealt input (rows x N).
int pc_launch_ntt_long(vp_ctx *ctx, const F *in, F *out, int ln, int lm, int inverse, u32 rows, u32 cosets, u32 in_stride) {
    const int l0 = ln - PC_MAX_LN_SPLIT, ls = PC_MAX_LN_SPLIT;
    const u32 nc = inverse ? 1 : cosets, N0 = 1u << l0, Ns = 1u << ls;
    const size_t N = (size_t) 1 << ln, total = (size_t) rows * nc * N;
    if ((u64) rows * N0 * nc > 65535) { ctx->err = "transform longer than 2^17 points: more than 65535 sub-transforms in one call"; return VP_ELIMIT; }
    VPCHK(pc_scratch_reserve(ctx, total + (nc > 1 ? total : 0) + (size_t) rows * N));
    F *C = nc > 1 ? ctx->pc_scr + total : out, *D = ctx->pc_scr + total + (nc > 1 ? total : 0);
    const F *rt_sub = nullptr, *W = nullptr;
    VPCHK(pc_compact_roots(ctx, lm, lm - l0, &rt_sub));        // order M / N0, half table
    VPCHK(pc_circle_roots(ctx, lm, ln, &W));                    // w_N^e, e < N
    if (!ctx->pc_dry) {
        const dim3 g(Ns / NTTL_THREADS, rows);
        PC_PROF(VP_K_NTT_LONG_SPLIT, g.x * g.y, rows, 32ull * N * rows, 0,
                if (l0 == 1) hipLaunchKernelGGL(k_ntt_long_split<1>, g, dim3(NTTL_THREADS), 0, ctx->stream, in, D, in_stride, ls);
                else hipLaunchKernelGGL(k_ntt_long_split<2>, g, dim3(NTTL_THREADS), 0, ctx->stream, in, D, in_stride, ls));
    }
    // the sub-transforms: the pair and its tables see the order-M / N0 table as the context's root table (its tables are keyed by that table)
    F *save_rt = ctx->pc_rt; const int save_lm = ctx->pc_lm;
    ctx->pc_rt = const_cast<F *>(rt_sub); ctx->pc_lm = lm - l0;
    const int rc = pc_launch_ntt8(ctx, D, C, ls, lm - l0, inverse, rows * N0, cosets, Ns);
    ctx->pc_rt = save_rt; ctx->pc_lm = save_lm;
    VPCHK(rc);
    if (ctx->pc_dry) return VP_OK;
    NttLongArgs a{};
    a.in = C; a.out = out; a.W = W; a.RT = ctx->pc_rt; a.half_m = 1u << (lm - 1); a.lsub = ls; a.ncoset = nc;
    a.scale = lz_presplit(inverse ? host_inv_real(N0) : f_one());
    const dim3 g(Ns / NTTL_THREADS, rows * nc);
    const u64 tr = (u64) rows * nc;
    PC_PROF(VP_K_NTT_LONG_MERGE, g.x * g.y, tr, 32ull * N * tr, tr * Ns * ((N0 - 1) * (!inverse && nc > 1 ? 2 : 1) + (inverse ? N0 : 0)),
            if (l0 == 1) { if (inverse) hipLaunchKernelGGL((k_ntt_long_merge<1, true>), g, dim3(NTTL_THREADS), 0, ctx->stream, a);
                           else hipLaunchKernelGGL((k_ntt_long_merge<1, false>), g, dim3(NTTL_THREADS), 0, ctx->stream, a); }
            else { if (inverse) hipLaunchKernelGGL((k_ntt_long_merge<2, true>), g, dim3(NTTL_THREADS), 0, ctx->stream, a);
                   else hipLaunchKernelGGL((k_ntt_long_merge<2, false>), g, dim3(NTTL_THREADS), 0, ctx->stream, a); });
    return VP_OK;
}

// butterflies of the register DFT of k_ntt_split that multiply (twiddle neither 1 nor iota), per column
static inline u64 split_dft_mults(int l1) { u64 n = 0; const u32 N1 = 1u << l1; for (int s = l1; s >= 1; --s) for (u32 idx = 0; idx < N1 / 2; ++idx) { const u32 e1 = (idx & ((1u << (s - 1)) - 1)) * (N1 >> s); if (e1 && 4 * e1 != N1) ++n; } return n; }
// F-multiplications of one k_ntt_lds transform of size 2^ln (radix-4 passes: 3 per 4 points, none in a pass whose twiddles are all 1)
static inline u64 ntt_lds_mults(int ln) { const u64 N = 1ull << ln; const int np = (ln & 1) ? (ln - 1) / 2 : std::max(0, ln / 2 - 1); return 3 * (N / 4) * (u64) np; }

// rows transforms of size 2^ln.  forward: `cosets` twisted copies (coset-major output [row][coset][N]); inverse: scaled
// by 1/N.  2^13 .. 2^17: the radix-8 pair (vp_options.ntt_r8, the default) or k_ntt_split -> k_ntt_lds (N1 x 2^13, stored in natural order,
// rows * cosets * N elements of scratch reserved twice); 2^18 / 2^19: pc_launch_ntt_long, whatever ntt_r8 says.
int pc_launch_ntt(vp_ctx *ctx, const F *in, F *out, int ln, int lm, int inverse, u32 rows, u32 cosets, u32 in_stride) {
    if (ln > PC_MAX_LN_SPLIT) {
        if (ln > PC_MAX_LN_LONG) { ctx->err = "transform longer than 2^19 points"; return VP_ELIMIT; }
        return pc_launch_ntt_long(ctx, in, out, ln, lm, inverse, rows, cosets, in_stride);
    }
    if (ctx->opt.ntt_r8 && ln >= 13 && ln <= 17 && (u64) rows * (inverse ? 1 : cosets) <= 65535)
        return pc_launch_ntt8(ctx, in, out, ln, lm, inverse, rows, cosets, in_stride);
    if (ln <= PC_MAX_LN) {
        NttArgs a{};
        a.in = in; a.out = out; a.RT = ctx->pc_rt; a.half_m = 1u << (lm - 1); a.lm = lm; a.ln = ln; a.inverse = inverse;
        a.in_stride = in_stride; a.inv_n = inverse ? host_inv_real(1ull << ln) : f_one();
        VPCHK(pc_compact_roots(ctx, lm, ln, &a.RTp));
        if (ctx->pc_dry) return VP_OK;
        a.half_p = a.RTp == ctx->pc_rt ? a.half_m : 1u << (ln - 1);
        const u32 threads = std::max<u32>(64, std::min<u32>(1024, (1u << ln) / 2));
        const u64 nt = (u64) rows * cosets, Nn = 1ull << ln;
        PC_PROF(VP_K_NTT_LDS, nt, nt, 32 * Nn * nt, nt * (ntt_lds_mults(ln) + (inverse ? Nn : (cosets > 1 ? Nn : 0))),
                hipLaunchKernelGGL(k_ntt_lds, dim3(rows, cosets), dim3(threads), sizeof(F) << ln, ctx->stream, a));
        return VP_OK;
    }
    const int l1 = ln - PC_SPLIT_LN;                     // 2..5 (1..4 with 2^13-point blocks)
    const u32 N = 1u << ln, N2 = 1u << PC_SPLIT_LN, nc = inverse ? 1 : cosets;
    const size_t total = (size_t) rows * nc * N;
    VPCHK(pc_scratch_reserve(ctx, 2 * total));
    if (ctx->pc_dry) { const F *rtp = nullptr; return pc_compact_roots(ctx, lm, PC_SPLIT_LN, &rtp); }
    F *s1 = ctx->pc_scr;
    SplitArgs sa{};
    sa.in = in; sa.out = s1; sa.RT = ctx->pc_rt; sa.half_m = 1u << (lm - 1); sa.ln = ln; sa.l1 = l1; sa.inverse = inverse;
    sa.in_stride = in_stride; sa.ncoset = nc;
    const dim3 g1(nblk(N2), rows, nc);
    {
        const u64 tr = (u64) rows * nc;
        const int sl_ = prof_begin(ctx, ctx->stream, VP_K_NTT_SPLIT, (u32) (nblk(N2) * rows * nc), (u32) tr, 32ull * N * tr,
                                   tr * (split_dft_mults(l1) * (N >> l1) + (N - (N >> l1)) + (!inverse && nc > 1 ? N : 0)));
        if (l1 == 5) hipLaunchKernelGGL(k_ntt_split<5>, g1, dim3(VP_BLOCK), 0, ctx->stream, sa);
        else if (l1 == 1) hipLaunchKernelGGL(k_ntt_split<1>, g1, dim3(VP_BLOCK), 0, ctx->stream, sa);
        else if (l1 == 2) hipLaunchKernelGGL(k_ntt_split<2>, g1, dim3(VP_BLOCK), 0, ctx->stream, sa);
        else if (l1 == 3) hipLaunchKernelGGL(k_ntt_split<3>, g1, dim3(VP_BLOCK), 0, ctx->stream, sa);
        else hipLaunchKernelGGL(k_ntt_split<4>, g1, dim3(VP_BLOCK), 0, ctx->stream, sa);
        prof_end(ctx, ctx->stream, sl_);
    }
    // N1 contiguous N2-point transforms per (row, coset): plain (untwisted, unscaled) forward / inverse kernels
    NttArgs a{};
    a.in = s1; a.RT = ctx->pc_rt; a.half_m = 1u << (lm - 1); a.lm = lm; a.ln = PC_SPLIT_LN; a.inverse = inverse;
    a.in_stride = N2; a.inv_n = f_one();
    VPCHK(pc_compact_roots(ctx, lm, PC_SPLIT_LN, &a.RTp));
    a.half_p = a.RTp == ctx->pc_rt ? a.half_m : 1u << (PC_SPLIT_LN - 1);
    // the sub-transforms store in natural order themselves (NttArgs::scat_l1)
    const u32 long_rows = rows * nc;
    for (u32 r0 = 0; r0 < long_rows; r0 += 1024) {
        NttArgs b = a;
        const u32 nr = std::min<u32>(1024, long_rows - r0);
        b.in = s1 + (size_t) r0 * N; b.out = out + (size_t) r0 * N;
        b.scat_l1 = l1; b.scat_rows = nr; b.scat_do_scale = inverse ? 1 : 0; b.scat_scale = inverse ? host_inv_real(1ull << ln) : f_one();
        const u64 nt = (u64) ((nr + 7) / 8 * 8) << l1;
        PC_PROF(VP_K_NTT_LDS, nt, (u64) nr << l1, 32ull * N2 * ((u64) nr << l1), ((u64) nr << l1) * ntt_lds_mults(PC_SPLIT_LN) + (inverse ? (u64) N * nr : 0),
                hipLaunchKernelGGL(k_ntt_lds, dim3((u32) nt, 1), dim3(1024), sizeof(F) << PC_SPLIT_LN, ctx->stream, b));
    }
    return VP_OK;
}

// Leaf-hash launches: the generated fixed-register chains (vp_keccak_asm.h) or the compiler's form in workgroups of 256 (leaf_asm = 0, small
// trees, and always the checked build, whose index checks the asm block cannot carry).  The asm kernels want exactly ONE workgroup per CU (two
// workgroups would not be in phase with each other) and every CU busy: 1024 threads from 2^18 leaves on, 512 threads (with 96 KB of dynamic LDS asked
// for and never touched, so that a second workgroup does not fit) for 2^17; below that a chain per wave is all a CU gets either way.
static inline u32 pc_leaf_wg(const vp_ctx *ctx, u64 n_leaves) {        // threads per workgroup; 0: the compiler's kernel
#ifdef VP_CHECKED
    (void) ctx; (void) n_leaves; return 0;
#else
    if (!ctx->opt.leaf_asm) return 0;
    return n_leaves >= (1u << 18) ? 1024u : n_leaves >= (1u << 17) ? 512u : 0u;
#endif
}
static inline size_t pc_leaf_lds(u32 wg) { return wg == 1024 ? 0 : 96 * 1024; }
static inline int pc_leaf_prepare(vp_ctx *ctx) {                        // once per context (the attribute belongs to the device the context sits on): the 512-thread form
    if (ctx->leaf_attr_done) return ctx->leaf_attr_done > 0 ? VP_OK : VP_EHIP;     // asks for more dynamic LDS than the default limit
    hipError_t err = hipFuncSetAttribute((const void *) k_leaf_hash<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (err == hipSuccess) err = hipFuncSetAttribute((const void *) k_leaf_hash<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    ctx->leaf_attr_done = err == hipSuccess ? 1 : -1;
    if (err != hipSuccess) { ctx->err = "hipFuncSetAttribute (leaf hash)"; return VP_EHIP; }
    return VP_OK;
}
// THE leaf-hash launch: la.cw / leaves / N / mask / n filled in (N[q] values per coset: 16 N[q] leaves, 16 at the last FRI level's N[q] = 1; one oracle is a
// list of one).  The workgroup form goes by the launch's leaves together (pc_leaf_wg), the mask chain runs iff the entries carry mask codewords (all or none),
// and the launch-table row, when asked for, counts workgroups of the compiler's form whichever kernel runs: what every call site has always recorded.
static int pc_hash_leaves(vp_ctx *ctx, FriLeafArgs &la, bool profiled) {
    if (la.n < 1) return VP_OK;
    u32 blocks = 0, leaves = 0;
    int n_masked = 0;
    for (int q = 0; q < la.n; ++q) {
        const u32 nl = la.N[q] >= 2 ? 16 * la.N[q] : 16u;
        la.blk_start[q] = blocks; la.leaf_start[q] = leaves;
        blocks += nblk(nl); leaves += nl;
        if (la.mask[q]) ++n_masked;
    }
    la.blk_start[la.n] = blocks; la.leaf_start[la.n] = leaves;
    if (n_masked && n_masked != la.n) { ctx->err = "internal: leaf-hash entries with and without a mask slice in one launch"; return VP_EINVAL; }
    u32 wg = pc_leaf_wg(ctx, leaves);
    if (wg && pc_leaf_prepare(ctx) != VP_OK) wg = 0;
    const void *kernel = !wg ? (const void *) k_leaf_hash_c : n_masked ? (const void *) k_leaf_hash<true> : (const void *) k_leaf_hash<false>;
    void *args[] = {&la};
    PC_PROF_IF(profiled, VP_K_LEAF_HASH, blocks, la.n, (u64) leaves * (64 * 32 + 32), (u64) leaves * 65,
               (void) hipLaunchKernel(kernel, dim3(wg ? (leaves + wg - 1) / wg : blocks), dim3(wg ? wg : VP_BLOCK), args, wg ? pc_leaf_lds(wg) : 0, ctx->stream));
    return VP_OK;
}

// Merkle trees over leaves already in place: ma.tree / count / n filled in, count[q] leaves at tree[q][count .. 2 count) (at least 2).  One k_merkle_level
// launch per height while any tree has more than 512 nodes there, then one k_merkle_top launch for all trees; root q also lands in d_roots[q] unless d_roots
// is null.  levels >= 0: exactly that many level launches whatever the width, and no top (the local part of a sharded tree).  ma.count is used up.
// fs (vp_fri_commit_fs, one tree): the top is k_merkle_top_fs, which continues the Fiat-Shamir chain behind the root — D(label, root), then C(counter) into
// *r_next unless that is null; its launch-table row is a k_merkle row with rounds = 1 and first_round = label - 1: the level, 1-based.
struct PcFsTop { Dig *state; u64 label, counter; F *r_next; };
static int pc_merkle_trees(vp_ctx *ctx, MerkleArgs &ma, Dig *d_roots, int levels = -1, const PcFsTop *fs = nullptr) {
    for (int h = 0; levels < 0 || h < levels; ++h) {
        MerkleArgs lv{}; u32 b = 0; u64 hs = 0;
        for (int q = 0; q < ma.n; ++q) {
            const u32 c = ma.count[q] >> 1;
            if (levels < 0 && c <= 512) continue;
            lv.tree[lv.n] = ma.tree[q]; lv.count[lv.n] = c; lv.blk_start[lv.n] = b; b += nblk(c); hs += c; ++lv.n;
            ma.count[q] = c;
        }
        if (!lv.n) break;
        lv.blk_start[lv.n] = b;
        PC_PROF(VP_K_MERKLE, b, lv.n, 96ull * hs, hs, hipLaunchKernelGGL(k_merkle_level, dim3(b), dim3(VP_BLOCK), 0, ctx->stream, lv));
    }
    if (levels >= 0) return VP_OK;
    u64 hs = 0;
    for (int q = 0; q < ma.n; ++q) hs += ma.count[q] - 1;
    if (fs) {
        if (ma.n != 1) { ctx->err = "internal: the drawing tree top takes one tree"; return VP_EINVAL; }
        const int sl_ = prof_begin(ctx, ctx->stream, VP_K_MERKLE, 1, 1, 96ull * hs + 3 * 64, hs + 3, 1, (u32) (fs->label - 1));
        hipLaunchKernelGGL(k_merkle_top_fs, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, ma, d_roots, fs->state, fs->label, fs->counter, fs->r_next);
        prof_end(ctx, ctx->stream, sl_);
        return VP_OK;
    }
    // (the row's bytes: 96 per hash where the roots are collected, 96 per node of the widest level where they are not — the two forms this launch had)
    PC_PROF(VP_K_MERKLE, ma.n, ma.n, 96ull * (d_roots ? hs : hs + ma.n), hs, hipLaunchKernelGGL(k_merkle_top, dim3(ma.n), dim3(VP_BLOCK), 0, ctx->stream, ma, d_roots));
    return VP_OK;
}
int pc_merkle(vp_ctx *ctx, Dig *tree, u32 n_leaves) {    // one tree, leaves already at tree[n_leaves .. 2 n_leaves); the root stays at tree[1]
    MerkleArgs ma{};
    ma.tree[0] = tree; ma.count[0] = n_leaves; ma.n = 1;
    return pc_merkle_trees(ctx, ma, nullptr);
}

// Oracle o (0 = l, 1 = h) hashed now, by a launch of its own: leaf chains (closed by the oracle's mask codeword under a masked commitment), tree, and the
// root on its way to `root` (host memory that outlives the stream's work).  The synchronous commits and whatever vp_pc_hash_late left unhashed come here.
static int pc_hash_oracle(vp_ctx *ctx, int o, void *root) {
    const int n = ctx->L[0].bl;
    const u32 n_leaves = 1u << (n - 2);
    Dig *tree = o ? ctx->pc_tree_h : ctx->pc_tree;
    FriLeafArgs la{};
    la.cw[0] = o ? ctx->pc_hcw : ctx->pc_cw; la.leaves[0] = tree + n_leaves; la.N[0] = 1u << (n - 6); la.n = 1;
    if (ctx->pc_mask_ms) la.mask[0] = o ? ctx->pc_hm_cw : ctx->pc_lm_cw;
    VPCHK(pc_hash_leaves(ctx, la, true));
    VPCHK(pc_merkle(ctx, tree, n_leaves));
    HIPCHK(hipMemcpyAsync(root, tree + 1, 32, hipMemcpyDeviceToHost, ctx->stream));
    return VP_OK;
}

// vp_pc_hash_late: the leaf chains and trees that vp_commit_private / vp_commit_public(_eq) left for vp_fri_commit (vp_ctx::pc_unhashed; which: bit 0 = l,
// bit 1 = h), by the single-oracle launches of the synchronous calls, finished here; each root goes where its call was asked to put it.  Called by everything
// that reads a tree, replaces a codeword or ends the context before a vp_fri_commit has merged them.
int pc_hash_outstanding(vp_ctx *ctx, unsigned which) {
    which &= ctx->pc_unhashed;
    if (!which) return VP_OK;
    if (ctx->L.empty() || !ctx->pc_cw || !ctx->pc_tree) { ctx->pc_unhashed = 0; ctx->err = "internal: unhashed oracle without its codeword"; return VP_EINVAL; }
    uint8_t got[2][32];
    for (int o = 0; o < 2; ++o) if (which >> o & 1) VPCHK(pc_hash_oracle(ctx, o, got[o]));
    ctx->pc_unhashed &= ~which;
    VPCHK(check_stream(ctx));
    for (int o = 0; o < 2; ++o) if ((which >> o & 1) && ctx->late_root[o]) { memcpy(ctx->late_root[o], got[o], 32); ctx->late_root[o] = nullptr; }
    return VP_OK;
}

// the same entry points on a commitment sharded over ranks (vpgpu_pc_shard.inc)
int pcs_commit_private(vp_ctx *ctx, uint8_t root[32]);
int pcs_commit_public(vp_ctx *ctx, const vp_F *pub, uint64_t n_pub, const vp_F *point, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]);
int pcs_fri_commit(vp_ctx *ctx, const vp_F *r, int n_steps, uint8_t *roots);
int pcs_fri_step(vp_ctx *ctx, const vp_F *r, uint8_t root[32]);
bool pcs_private_done(vp_ctx *ctx);
bool pcs_public_done(vp_ctx *ctx);
int pcs_fri_done(vp_ctx *ctx);
bool pcs_fri_one_pass(vp_ctx *ctx);
int pcs_fri_final(vp_ctx *ctx, vp_F *final_code);
int pcs_open_desc(vp_ctx *ctx, int oracle, PcOpenDesc *d);
bool pcs_owns(vp_ctx *ctx, uint64_t leaf);

// ---- the query phase in one device pass (vp_fri_open_many, vp_fri_query; kernel: k_pc_open_many) ----------------------------------------------------------------
// One launch answers up to PC_MANY_PIECE requests into fixed-stride records, one copy brings them to pinned memory, one synchronise follows; the caller's
// layout is written from there.  Every request is validated before anything is launched, by the rules vp_fri_open applies to one.
constexpr int PC_MANY_PIECE = 4096, PC_MANY_MAX = 1 << 16;
static inline size_t pc_many_in_bytes(u32 cap) { return VP_OPEN_MAX_ORACLES * sizeof(PcOpenDesc) + (size_t) cap * sizeof(uint2); }
static int pc_many_reserve(vp_ctx *ctx, u32 want) {        // buffers for `want` requests per launch (two sizes: 1024 covers a protocol run up to 33 x (2 + 19))
    want = std::min<u32>(want, PC_MANY_PIECE);
    if (ctx->pc_many_buf && ctx->pc_many_cap >= want) return VP_OK;
    const u32 cap = want <= 1024 ? 1024 : PC_MANY_PIECE;
    const size_t hb = pc_many_in_bytes(cap) + (size_t) cap * sizeof(PcOpenRec);
    if (ctx->h_many_cap < hb) {
        if (ctx->h_many) (void) hipHostFree(ctx->h_many);
        ctx->h_many = nullptr; ctx->h_many_cap = 0;
        HIPCHK(hipHostMalloc((void **) &ctx->h_many, hb, hipHostMallocDefault));
        ctx->h_many_cap = hb;
    }
    ctx->pc_many_cap = 0;
    VPCHK(dalloc(ctx, &ctx->pc_many_buf, (size_t) cap));   // (a smaller one from before stays in ctx->allocs until the next upload)
    VPCHK(dalloc(ctx, &ctx->pc_many_in, pc_many_in_bytes(cap)));
    ctx->pc_many_cap = cap;
    return VP_OK;
}
// Which buffers an oracle number means (0 = l, 1 = h, 2 + k = FRI level k), or why it cannot be opened: the one place that decides it, for vp_fri_open and
// for every request of vp_fri_open_many / vp_fri_query
static int pc_open_desc(vp_ctx *ctx, int oracle, PcOpenDesc *d) {
    *d = PcOpenDesc{};
    if (oracle < 0 || ctx->L.empty()) return VP_EINVAL;
    if (oracle >= VP_OPEN_MAX_ORACLES) { ctx->err = "FRI level not committed yet"; return VP_EINVAL; }
    if (ctx->pcs) return pcs_open_desc(ctx, oracle, d);
    VPCHK(pc_hash_outstanding(ctx, 3u));
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, M = 1u << lm;
    if (oracle == 0) { if (!ctx->pc_private_done) return VP_EINVAL; d->cw = ctx->pc_cw; d->tree = ctx->pc_tree; d->Nc = N; d->n_leaves = M >> 1; }
    else if (oracle == 1) { if (!ctx->pc_public_done) return VP_EINVAL; d->cw = ctx->pc_hcw; d->tree = ctx->pc_tree_h; d->Nc = N; d->n_leaves = M >> 1; }
    else {
        const int lvl = oracle - 2;
        if (lvl >= ctx->fri_step) { ctx->err = "FRI level not committed yet"; return VP_EINVAL; }
        const FriLayout fl(ln, 0);
        d->cw = ctx->pc_fri_all + fl.cw(lvl); d->tree = ctx->pc_fri_tree + fl.tree(lvl);
        d->Nc = (u32) fl.per_coset(lvl); d->n_leaves = (u32) fl.leaves(lvl);
        if (ctx->pc_mask_ms) d->mask = ctx->pc_fm + fl.mask(lvl);
    }
    if (ctx->pc_mask_ms && oracle < 2) d->mask = oracle == 0 ? ctx->pc_lm_cw : ctx->pc_hm_cw;   // the mask slice's codeword of this oracle (zeros otherwise)
    return VP_OK;
}
static inline int pc_open_depth(u32 n_leaves) { int depth = 0; while ((1u << depth) < n_leaves) ++depth; return depth; }
struct PcManyPlan { PcOpenDesc tab[VP_OPEN_MAX_ORACLES]; std::vector<int> plen, dlen; u64 bytes = 0, layout = 0; };   // plen[i]: digests of request i's path, 0 = another rank's; dlen[i]: whoever answers; bytes: this rank's answers, layout: all
// Validation of a whole list (nothing is launched or written on a refusal).  path_stride < 0: no capacity rule (vp_fri_query packs paths itself).
static int pc_many_plan(vp_ctx *ctx, int n, const int32_t *oracle, const uint64_t *leaf, int path_stride, PcManyPlan &pl) {
    int have[VP_OPEN_MAX_ORACLES]; for (int &h : have) h = 0;       // 0 unknown, 1 described
    pl.plen.assign((size_t) n, 0); pl.dlen.assign((size_t) n, 0); pl.bytes = pl.layout = 0;
    for (auto &t : pl.tab) t = PcOpenDesc{};
    for (int i = 0; i < n; ++i) {
        const int o = oracle[i];
        if (o < 0) return VP_EINVAL;
        if (o >= VP_OPEN_MAX_ORACLES || !have[o]) { VPCHK(pc_open_desc(ctx, o, &pl.tab[std::min(o, VP_OPEN_MAX_ORACLES - 1)])); have[o] = 1; }
        const PcOpenDesc &d = pl.tab[o];
        if (leaf[i] >= d.n_leaves) return VP_EINVAL;
        const int depth = pc_open_depth(d.n_leaves);
        if (depth + 1 > VP_OPEN_MAX_PATH) return VP_ELIMIT;
        if (path_stride >= 0 && path_stride < 32 * (depth + 1)) return VP_EINVAL;
        pl.dlen[i] = depth + 1;
        pl.layout += 130 * sizeof(F) + 32ull * (depth + 1);
        if (d.top && !pcs_owns(ctx, leaf[i])) continue;
        pl.plen[i] = depth + 1;
        pl.bytes += 130 * sizeof(F) + 32ull * (depth + 1);
    }
    return VP_OK;
}
// The launches: sink(i, record) receives the answer of every request this rank owns, in request order.
static int pc_many_run(vp_ctx *ctx, int n, const int32_t *oracle, const uint64_t *leaf, const PcManyPlan &pl, const std::function<void(int, const PcOpenRec &)> &sink) {
    std::vector<int> mine; mine.reserve((size_t) n);
    for (int i = 0; i < n; ++i) if (pl.plen[i]) mine.push_back(i);
    ctx->ev_used = 0;
    if (mine.empty()) { if (ctx->profiling) prof_collect(ctx); return VP_OK; }
    VPCHK(pc_many_reserve(ctx, (u32) std::min<size_t>(mine.size(), PC_MANY_PIECE)));
    const u32 cap = ctx->pc_many_cap;
    PcOpenDesc *h_tab = reinterpret_cast<PcOpenDesc *>(ctx->h_many);
    uint2 *h_req = reinterpret_cast<uint2 *>(ctx->h_many + VP_OPEN_MAX_ORACLES * sizeof(PcOpenDesc));
    const PcOpenRec *h_rec = reinterpret_cast<const PcOpenRec *>(ctx->h_many + pc_many_in_bytes(cap));
    const PcOpenDesc *d_tab = reinterpret_cast<const PcOpenDesc *>(ctx->pc_many_in);
    const uint2 *d_req = reinterpret_cast<const uint2 *>(ctx->pc_many_in + VP_OPEN_MAX_ORACLES * sizeof(PcOpenDesc));
    memcpy(h_tab, pl.tab, sizeof pl.tab);
    for (size_t at = 0; at < mine.size(); at += PC_MANY_PIECE) {
        const u32 cnt = (u32) std::min<size_t>(PC_MANY_PIECE, mine.size() - at);
        u64 bytes = 0;
        for (u32 j = 0; j < cnt; ++j) {
            const int i = mine[at + j];
            h_req[j] = make_uint2((u32) oracle[i], (u32) leaf[i]);
            bytes += 130 * sizeof(F) + 32ull * pl.plen[i];
        }
        HIPCHK(hipMemcpyAsync(ctx->pc_many_in, ctx->h_many, pc_many_in_bytes(cnt), hipMemcpyHostToDevice, ctx->stream));
        PC_PROF(VP_K_PC_OPEN_MANY, cnt, cnt, bytes, 0,
                hipLaunchKernelGGL(k_pc_open_many, dim3(cnt), dim3(128), 0, ctx->stream, d_tab, (u32) VP_OPEN_MAX_ORACLES, d_req, cnt, ctx->pc_many_buf));
        HIPCHK(hipMemcpyAsync(const_cast<PcOpenRec *>(h_rec), ctx->pc_many_buf, (size_t) cnt * sizeof(PcOpenRec), hipMemcpyDeviceToHost, ctx->stream));
        VPCHK(check_stream(ctx));
        for (u32 j = 0; j < cnt; ++j) sink(mine[at + j], h_rec[j]);
    }
    if (ctx->profiling) prof_collect(ctx);
    return VP_OK;
}


// ---- the mask slice with content (round 6; kernels: vp_kernels_pc.h "the mask slice WITH CONTENT") ------------------------------------------------------------
// Geometry of poly_commit.h:55-66: gap = the largest power of two <= slice_size / mask length, padded length ms = slice_size / gap.  What this library takes:
// ms >= 8 (the reference's own transforms of fewer than 8 points read stale scratch, RS_polynomial.cpp:104-133: below that its commitment is not a function of the
// mask), gap >= 2 (poly_commit.h:195 asserts it) and 2 ms <= 2^17 (the quotient's 2 ms-point inverse transform is one of this library's transforms).
static int pc_mask_geometry(vp_ctx *ctx, uint64_t n_mask, u32 *ms_out) {
    const int n = ctx->L[0].bl, lm = n - 1;
    const u64 M = 1ull << lm;
    if (n_mask < 1 || n_mask > M) { ctx->err = "mask longer than a slice"; return VP_EINVAL; }
    u64 gap = 1;
    while (gap * 2 <= M / n_mask) gap *= 2;
    const u64 ms = M / gap;
    if (ms < 8) { ctx->err = "mask pads to fewer than 8 elements: the reference's transforms of that size read stale scratch (RS_polynomial.cpp:104-133), its commitment is not a function of such a mask"; return VP_EINVAL; }
    if (gap < 2) { ctx->err = "mask longer than half a slice (the reference asserts mask_position_gap != 1, poly_commit.h:195)"; return VP_EINVAL; }
    if (2 * ms > (1ull << PC_MAX_LN_SPLIT)) { ctx->err = "mask pads to more than 2^16 elements: its quotient's transform would be longer than 2^17 points (not supported)"; return VP_ELIMIT; }
    *ms_out = (u32) ms;
    return VP_OK;
}
// Scratch of the slice's small transforms, in blocks of B = max(ms, N) elements: [0, B) values / h coefficients, [B, 2B) coefficients, [2B, 4B) l q at 2 ms points,
// [4B, 6B) its coefficients, [6B, 6B + 32 N) the per-coset polynomials of a mask longer than N (k_mask_combine), then S0 of the slice (one element).
static inline F *pc_mask_S0(vp_ctx *ctx) { return ctx->pc_mtmp + ctx->pc_mtmp_cap - 64; }
static int pc_mask_alloc(vp_ctx *ctx, u32 ms) {
    const int n = ctx->L[0].bl;
    const size_t M = (size_t) 1 << (n - 1), N = (size_t) 1 << (n - 6), B = std::max<size_t>(ms, N);
    if (!ctx->pc_lm_cw) { VPCHK(dalloc(ctx, &ctx->pc_lm_cw, M)); VPCHK(dalloc(ctx, &ctx->pc_qm_cw, M)); VPCHK(dalloc(ctx, &ctx->pc_hm_cw, M)); VPCHK(dalloc(ctx, &ctx->pc_fm, M)); }
    const size_t need = 6 * B + 32 * N + 64;
    if (ctx->pc_mtmp_cap < need) {
        F *fresh = nullptr;
        VPCHK(dalloc(ctx, &fresh, need));
        if (ctx->pc_mtmp) {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *) ctx->pc_mtmp);
            if (it != ctx->allocs.end()) ctx->allocs.erase(it);
            (void) hipFree(ctx->pc_mtmp);
        }
        ctx->pc_mtmp = fresh; ctx->pc_mtmp_cap = need;
    }
    ctx->pc_mB = B;
    return VP_OK;
}
// coefficients (ms of them, device, in a buffer of B elements) -> the slice's evaluations on the M-th roots, coset-major.  ms <= N: the slices' own encode
// (pc_launch_ntt, 32 cosets) on the zero-padded array; ms > N: one combined polynomial per coset (k_mask_combine), 32 plain N-point transforms
static int pc_mask_encode(vp_ctx *ctx, F *coef, u32 ms, F *dst) {
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln;
    if (ms <= N) {
        if (ms < N) hipLaunchKernelGGL(k_zero_f, dim3(nblk(N - ms)), dim3(VP_BLOCK), 0, ctx->stream, coef + ms, N - ms);
        return pc_launch_ntt(ctx, coef, dst, ln, lm, 0, 1, 32, N);
    }
    F *rows = ctx->pc_mtmp + 6 * ctx->pc_mB;
    hipLaunchKernelGGL(k_mask_combine, dim3(nblk((u64) 32 * N)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) coef, N, ms / N, (const F *) ctx->pc_rt, 1u << (lm - 1), rows);
    return pc_launch_ntt(ctx, rows, dst, ln, lm, 0, 32, 1, N);
}
// a mask vector of the caller (n_mask elements, padded with zeros to ms: poly_commit.h:68-70,139-141) -> its low-degree extension over the slice's domain
static int pc_mask_lde(vp_ctx *ctx, const vp_F *mask, uint64_t n_mask, u32 ms, F *dst) {
    const int lm = ctx->L[0].bl - 1;
    for (uint64_t i = 0; i < n_mask; ++i) if (mask[i].real >= P61 || mask[i].img >= P61) { ctx->err = "non-canonical mask element"; return VP_EINVAL; }
    F *h = nullptr;                                     // pinned until the stream has taken it (ms <= 2^16: 1 MB): no wait here
    VPCHK(ring_alloc(ctx, (size_t) ms * sizeof(F), (void **) &h));
    for (uint64_t i = 0; i < ms; ++i) h[i] = i < n_mask ? f_make(mask[i].real, mask[i].img) : f_zero();
    F *t = ctx->pc_mtmp;
    HIPCHK(hipMemcpyAsync(t, h, (size_t) ms * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    VPCHK(pc_launch_ntt(ctx, t, t + ctx->pc_mB, ilog2(ms), lm, 1, 1, 1, ms));
    return pc_mask_encode(ctx, t + ctx->pc_mB, ms, dst);
}

// One whole FRI level by launches of its own (vp_fri_step, the tail of a sharded commitment): its leaf chains, which stay out of the launch table
// (Nc == 1: the 16 leaves of the last level; mask: the mask slice's pair closes every chain), and the tree
static int pc_hash_level(vp_ctx *ctx, const F *cw, u32 Nc, const F *mask, Dig *tree) {
    const u32 n_leaves = 16 * Nc;
    FriLeafArgs la{};
    la.cw[0] = cw; la.leaves[0] = tree + n_leaves; la.N[0] = Nc; la.mask[0] = mask; la.n = 1;
    VPCHK(pc_hash_leaves(ctx, la, false));
    return pc_merkle(ctx, tree, n_leaves);
}
// The mask slice (the 65th) in the FRI commit phase, in arrays of its own behind the 64: its virtual oracle in place over its q codeword
// (poly_commit.h:225-245), then one fold per level like the others (fri.cpp:366-374); pc_mask_fold returns level k's codeword, whose pairs close the
// level's leaf chains (fri.cpp:403-411)
static void pc_mask_vo(vp_ctx *ctx, bool profiled) {
    const int n = ctx->L[0].bl;
    const u32 N = 1u << (n - 6), M = 1u << (n - 1);
    PC_PROF_IF(profiled, VP_K_FRI_FOLD, nblk(M), 1, 64ull * M, 4ull * M,
               hipLaunchKernelGGL(k_mask_vo, dim3(nblk(M)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) ctx->pc_lm_cw, (const F *) ctx->pc_qm_cw, (const F *) ctx->pc_hm_cw,
                                  (const F *) pc_mask_S0(ctx), N, ctx->pc_rt, M >> 1, f_make(ctx->pc_mask_ms, 0), ctx->pc_mask_ms, ctx->pc_qm_cw));
}
static const F *pc_mask_fold(vp_ctx *ctx, int k, F r, bool profiled, const F *d_r = nullptr /* the challenge in device memory instead (vp_fri_commit_fs) */) {
    const int n = ctx->L[0].bl;
    const FriLayout fl(n - 6, 0);
    const u32 M = 1u << (n - 1), Nk = (1u << (n - 6)) >> k, No = Nk >> 1;
    const F *in_m = k == 0 ? ctx->pc_qm_cw : ctx->pc_fm + fl.mask(k - 1);
    F *out_m = ctx->pc_fm + fl.mask(k);
    PC_PROF_IF(profiled, VP_K_FRI_FOLD, nblk((u64) 32 * No), 1, 48ull * 32 * No, (u64) 3 * 32 * No,
               if (d_r) hipLaunchKernelGGL(k_fri_fold_one_p, dim3(nblk((u64) 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, in_m, out_m, Nk, k, ctx->pc_rt, M >> 1, d_r, host_inv_real(2));
               else hipLaunchKernelGGL(k_fri_fold_one, dim3(nblk((u64) 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, in_m, out_m, Nk, k, ctx->pc_rt, M >> 1, r, host_inv_real(2)));
    return out_m;
}
// the last level's codeword ([slice][32], one value per coset) in the reference's order: out[(i << 7) | (slice << 1) | hi] = value at position i + 16 hi
static void pc_final_order(const F *cw, vp_F *final_code) {
    F *o = reinterpret_cast<F *>(final_code);
    for (u32 i = 0; i < 16; ++i) for (u32 s = 0; s < 64; ++s) for (u32 hi = 0; hi < 2; ++hi) o[(i << 7) | (s << 1) | hi] = cw[s * 32 + i + 16 * hi];
}

// Live slices (vp_pc_live.h).  vp_commit_private fixes the count for the commitment it starts — the input layer's zero tail is what vp_evaluate and
// vp_pc_load_input leave behind L[0].size — and a commitment with a mask slice runs over all 64.
static inline void pc_live_set(vp_ctx *ctx, bool masked) {
    ctx->pc_lv = masked ? PcLive() : PcLive(ctx->L[0].bl, (uint64_t) ctx->L[0].size, ctx->opt.pc_live != 0);
}
// The dead slices of a buffer of 64 slices x `per` elements must read as zero bytes (leaf hashes, openings and vp_fri_final read all 64).  mark: the slice
// from which on the buffer is known to be zero (64: a fresh allocation).  A smaller live count zeroes the gap here, in stream order; a larger one needs
// nothing, the phase that follows writes every live slice before anything reads the buffer.  (Calls that run over all 64 slices compute the same zeros.)
static int pc_zero_dead(vp_ctx *ctx, F *buf, size_t per, u32 mark, u32 live) {
    if (buf && live < mark) HIPCHK(hipMemsetAsync(buf + (size_t) live * per, 0, (size_t) (mark - live) * per * sizeof(F), ctx->stream));
    return VP_OK;
}
static int pc_live_zero_cw(vp_ctx *ctx, u32 written) {            // `written`: slices the encode writes (the paired encode may write one dead slice)
    const u32 M = 1u << (ctx->L[0].bl - 1);
    VPCHK(pc_zero_dead(ctx, ctx->pc_cw, M, ctx->pc_zf_cw, written));
    ctx->pc_zf_cw = written;
    return VP_OK;
}
static int pc_live_zero_hcw(vp_ctx *ctx) {
    const u32 M = 1u << (ctx->L[0].bl - 1);
    VPCHK(pc_zero_dead(ctx, ctx->pc_hcw, M, ctx->pc_zf_hcw, ctx->pc_lv.live));
    ctx->pc_zf_hcw = ctx->pc_lv.live;
    return VP_OK;
}
static int pc_live_zero_fri(vp_ctx *ctx) {
    if (!ctx->pc_fri_all) return VP_OK;                           // not allocated yet: the mark stays at 64 for the allocation to come
    const int ln = ctx->L[0].bl - 6;
    const FriLayout fl(ln, 0);
    if (ctx->pc_lv.live < ctx->pc_zf_fri)
        for (int k = 0; k < ln; ++k) VPCHK(pc_zero_dead(ctx, ctx->pc_fri_all + fl.cw(k), 32 * fl.per_coset(k), ctx->pc_zf_fri, ctx->pc_lv.live));
    ctx->pc_zf_fri = ctx->pc_lv.live;
    return VP_OK;
}

// buffers of commit_public and of the FRI commit phase (every level's codeword is kept for the openings): allocated with the commitment,
// not inside the first fold step
int pc_public_alloc(vp_ctx *ctx) {
    if (ctx->pc_pub) return VP_OK;
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, M = 1u << lm;
    VPCHK(dalloc(ctx, &ctx->pc_pub, (size_t) 1 << n));
    VPCHK(dalloc(ctx, &ctx->pc_qcw, (size_t) 64 * M));
    VPCHK(dalloc(ctx, &ctx->pc_hcw, (size_t) 64 * M));
    VPCHK(dalloc(ctx, &ctx->pc_tmp, (size_t) 3 * 128 * N));           // products | S,T | H
    VPCHK(dalloc(ctx, &ctx->pc_small, (size_t) 1024 + 160 + 64));    // ... | [1184..1248): qscal of a tensor public vector
    VPCHK(dalloc(ctx, &ctx->pc_q0, (size_t) M));                      // its one encoded slice
    VPCHK(dalloc(ctx, &ctx->pc_flag, (size_t) 1));
    VPCHK(dalloc(ctx, &ctx->pc_eq, (size_t) 32 + 2 * ((size_t) 1 << ((n + 1) / 2))));   // vp_commit_public_eq: point | two eq half tables
    VPCHK(dalloc(ctx, &ctx->pc_cbuf, (size_t) 64));                  // k_fri_fold0_vo: w_M^-b | w_32^b - 1, b < 32
    VPCHK(dalloc(ctx, &ctx->pc_tree_h, (size_t) M));
    VPCHK(dalloc(ctx, &ctx->pc_fri_all, (size_t) 64 * M));
    VPCHK(dalloc(ctx, &ctx->pc_fri_tree, (size_t) M));
    VPCHK(dalloc(ctx, &ctx->pc_fri_roots, (size_t) VP_FRI_MAX));
    return VP_OK;
}

// The slices a context encodes, as the quotient pipeline and the first FRI fold see them: all 64 in the buffers of the context (pc_slices), or a rank's
// 64 / W in the buffers of its PcShard (vpgpu_pc_shard.inc).  A view, not an owner.  Layout of `small`: [0, 1024) partial sums | [1024] inner product |
// [1025, 1090) all_sum | [1105, 1169) S_0 per slice | [1184, 1248) the 64 scalars of a tensor public vector; of `tmp`: products | S, T | H, 2 cap N each.
struct PcSlices {
    u32 first = 0, cap = 64, rows = 64, N = 0;            // global index of the first slice; slices the buffers hold; slices transformed (live ones); slice length
    F *lcw = nullptr, *pub = nullptr, *slice0 = nullptr;  // l codeword; the public vector's slices [first, first + cap); where its slice 0 sits (pub itself, or N in front of it)
    F *coef = nullptr, *qcw = nullptr, *hcw = nullptr, *tmp = nullptr, *small = nullptr, *q0 = nullptr;
    int *flag = nullptr;
    bool tensor = false;                                  // the public vector in flight is encoded as slice 0 alone (q0) and the scalars
    F *P() const { return tmp; }
    F *ST() const { return tmp + (size_t) 2 * cap * N; }
    F *H() const { return tmp + (size_t) 4 * cap * N; }
    F *d_inner() const { return small + 1024; }
    F *d_all() const { return small + 1025; }
    F *S0() const { return small + 1025 + 80; }
    F *qscal() const { return small + 1184; }
    u32 rows_checked() const { return cap + (u32) ((pub - slice0) / N); }      // slices from slice0 to the end of pub: what the tensor check reads
    const F *q0_arg() const { return tensor ? q0 : nullptr; }
    const F *qs_arg() const { return tensor ? qscal() + first : nullptr; }
};
PcSlices pc_slices(vp_ctx *ctx, u32 rows) {
    PcSlices v;
    v.rows = rows; v.N = 1u << (ctx->L[0].bl - 6);
    v.lcw = ctx->pc_cw; v.pub = v.slice0 = ctx->pc_pub; v.coef = ctx->pc_coef; v.qcw = ctx->pc_qcw; v.hcw = ctx->pc_hcw; v.tmp = ctx->pc_tmp;
    v.small = ctx->pc_small; v.q0 = ctx->pc_q0; v.flag = ctx->pc_flag; v.tensor = ctx->pc_q_tensor;
    return v;
}

// Can the one-slice encoding apply at all: the option, and a slice-0 corner that has an inverse
bool pc_tensor_candidate(const vp_ctx *ctx, const F corner[64]) {
    return ctx->opt.pc_tensor_pub && (corner[0].re | corner[0].im) != 0 && corner[0].re < P61 && corner[0].im < P61;
}

// The quotient pipeline over the slices of a view, once their part of the public vector (and slice 0) sits on the device: q encoded like l, h = the quotient
// of l q by x^N - 1 per slice encoded in turn (poly_commit.h:163-176, 264-293), all_sum and S_0 beside them.  corner[i] = pub[i N] (host copies);
// tensor_state: 0 = check the tensor shape on the device, 1 = a tensor by construction (an eq table).
// The protocol's public vector is the eq table of the opening point (src/verifier.cpp:368-369): a tensor, slice i = eq(r_hi, i) * eq(r_lo, .).  Whenever
// the slices in view have that shape against slice 0 (checked exactly on the device: pub[iN + k] pub[0] == pub[iN] pub[k], pub[0] != 0) only slice 0 is
// encoded and q_i = qscal[i] q_0 is formed where it is consumed: the same field elements, 32 forward transforms instead of 32 rows.  Any other vector:
// every slice.  Ranks of a sharded commitment need not agree: either way a rank's slices come out as the same field elements.
int pc_quotient_slices(vp_ctx *ctx, PcSlices &v, const F corner[64], int tensor_state) {
    const int ln = ctx->L[0].bl - 6, lm = ln + 5;
    const u32 N = v.N, M = 32 * N, rows = v.rows;
    v.tensor = false;
    if (pc_tensor_candidate(ctx, corner)) {
        if (tensor_state == 1) v.tensor = true;
        else {
            const u32 chk = v.rows_checked();
            HIPCHK(hipMemsetAsync(v.flag, 0, sizeof(int), ctx->stream));
            PC_PROF(VP_K_PC_POINTWISE, nblk((u64) chk * N), 1, 16ull * chk * N, (u64) 2 * chk * N,
                    hipLaunchKernelGGL(k_pc_rank1_check, dim3(nblk((u64) chk * N)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) v.slice0, N, chk, v.flag));
            int bad = 1;
            HIPCHK(hipMemcpyAsync(&bad, v.flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            v.tensor = bad == 0;
        }
    }
    if (v.tensor) {
        F *sc = nullptr;                                                  // pinned until the stream has taken it: no wait here
        VPCHK(ring_alloc(ctx, 64 * sizeof(F), (void **) &sc));
        const F inv0 = host_pow(corner[0], (unsigned __int128) P61 * P61 - 2);
        for (int i = 0; i < 64; ++i) sc[i] = f_mul(corner[i], inv0);
        HIPCHK(hipMemcpyAsync(v.qscal(), sc, 64 * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        VPCHK(pc_launch_ntt(ctx, v.slice0, v.coef, ln, lm, 1, 1, 1, N));
        VPCHK(pc_launch_ntt(ctx, v.coef, v.q0, ln, lm, 0, 1, 32, N));
    } else {
        // (q of a dead slice is only ever multiplied by zero, and q is no oracle)
        VPCHK(pc_launch_ntt(ctx, v.pub, v.coef, ln, lm, 1, rows, 1, N));
        VPCHK(pc_launch_ntt(ctx, v.coef, v.qcw, ln, lm, 0, rows, 32, N));
    }
    PC_PROF(VP_K_PC_POINTWISE, nblk((u64) 2 * rows * N), 1, 48ull * 2 * rows * N, (u64) 2 * rows * N,
            hipLaunchKernelGGL(k_pc_products, dim3(nblk((u64) 2 * rows * N)), dim3(VP_BLOCK), 0, ctx->stream, v.lcw, v.qcw, N, v.P(), rows, v.q0_arg(), v.qs_arg()));
    VPCHK(pc_launch_ntt(ctx, v.P(), v.ST(), ln, lm, 1, 2 * rows, 1, N));
    hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(256), 0, ctx->stream, v.d_all(), 144u);      // all_sum[65] and S_0 at [80..144): the dead slices' stay zero
    PC_PROF(VP_K_PC_POINTWISE, nblk((u64) rows * N), 1, 48ull * rows * N, (u64) 2 * rows * N,
            hipLaunchKernelGGL(k_pc_quotient, dim3(nblk((u64) rows * N)), dim3(VP_BLOCK), 0, ctx->stream, v.ST(), N, ctx->pc_rt, M >> 1,
                               host_inv_real(2), f_make(N, 0), v.H(), v.d_all(), rows));
    return pc_launch_ntt(ctx, v.H(), v.hcw, ln, lm, 0, rows, 32, N);
}

// vp_commit_public / vp_commit_public_eq once the public vector sits in ctx->pc_pub and ev0 is recorded (corner, tensor_state: pc_quotient_slices)
int pc_commit_public_body(vp_ctx *ctx, hipEvent_t &ev_a, const F corner[64], int tensor_state, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32],
                          const vp_F *pub_mask = nullptr, uint64_t n_pub_mask = 0) {
    const int n = ctx->L[0].bl, lm = n - 1;
    const u32 N = 1u << (n - 6), M = 1u << lm;
    VPCHK(pc_hash_outstanding(ctx, 2u));                  // an h of an earlier call that no vp_fri_commit has hashed: its codeword is replaced below
    VPCHK(pc_live_zero_hcw(ctx));                         // (a masked commitment runs over all 64: nothing to zero, and the mark says so afterwards)
    const bool late = ctx->hash_late && (!pub_mask || ctx->hash_late >= 2);      // vp_pc_hash_late: the transforms only; vp_fri_commit hashes h with its own levels (a masked commit: VP_HASH_LATE_MASKED)
    // slices >= live are zero (vp_pc_live.h): l q, S, T, H, all_sum and h are zero with them
    PcSlices v = pc_slices(ctx, pub_mask ? 64u : ctx->pc_lv.live);
    F *d_inner = v.d_inner(), *d_all = v.d_all();
    // input_0 = <circuitValue[0], pub>
    const u32 used = (u32) ctx->L[0].size, g = std::min<u32>(1024, nblk(used));
    PC_PROF(VP_K_PC_POINTWISE, g, 1, 32ull * used, used, hipLaunchKernelGGL(k_pc_dot, dim3(g), dim3(VP_BLOCK), 0, ctx->stream, ctx->L[0].val, ctx->pc_pub, used, v.small));
    hipLaunchKernelGGL(k_pc_sum_parts, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, v.small, g, d_inner);
    VPCHK(pc_quotient_slices(ctx, v, corner, tensor_state));
    ctx->pc_q_tensor = v.tensor;
    if (pub_mask) {
        // the mask slice (poly_commit.h:150-161,187-247): q = the public mask's low-degree extension; l q at 2 ms points -> its 2 ms coefficients -> h = the upper
        // half, all_sum[64] = (lq_coef[0] + h_coef[0]) ms; h's low-degree extension closes the leaf chains of this oracle
        const u32 ms = ctx->pc_mask_ms, gap = M / ms;
        const size_t B = ctx->pc_mB;
        F *t = ctx->pc_mtmp, *S0m = pc_mask_S0(ctx);
        VPCHK(pc_mask_lde(ctx, pub_mask, n_pub_mask, ms, ctx->pc_qm_cw));
        hipLaunchKernelGGL(k_mask_lq, dim3(nblk(2 * ms)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) ctx->pc_lm_cw, (const F *) ctx->pc_qm_cw, N, gap >> 1, 2 * ms, t + 2 * B);
        VPCHK(pc_launch_ntt(ctx, t + 2 * B, t + 4 * B, ilog2(2 * ms), lm, 1, 1, 1, 2 * ms));
        hipLaunchKernelGGL(k_mask_hcoef, dim3(nblk((u64) B)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) (t + 4 * B), ms, (u32) B, f_make(ms, 0), t, S0m, d_all + 64);
        VPCHK(pc_mask_encode(ctx, t, ms, ctx->pc_hm_cw));
    }
    unsigned char *st = nullptr;                          // root_h | inner | all_sum[65]
    VPCHK(ring_alloc(ctx, 32 + 66 * sizeof(F), (void **) &st));
    // second oracle: leaf chains + tree over h (fri.cpp:36-139 with oracle_indicator = 1)
    if (!late) VPCHK(pc_hash_oracle(ctx, 1, st));
    HIPCHK(hipMemcpyAsync(st + 32, d_inner, 66 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));        // d_all = d_inner + 1
    ctx->pc_public_done = true; ctx->fri_step = -1;
    if (late) { ctx->pc_unhashed |= 2u; ctx->late_root[1] = root_h; }
    return defer_end(ctx, ev_a, VP_PH_PUBLIC, [ctx, st, root_h, inner, all_sum, late](float ms) {
        if (!late) memcpy(root_h, st, 32);
        memcpy(inner, st + 32, sizeof(F)); memcpy(all_sum, st + 32 + sizeof(F), 65 * sizeof(F));
        ctx->commit_ms = ms;
        return VP_OK;
    });
}

}  // namespace

extern "C" {

static int pc_commit_private_body(vp_ctx *ctx, uint8_t root[32], const vp_F *mask, uint64_t n_mask) {
    const int n = ctx->L[0].bl;
    if (n < 7) { ctx->err = "input layer too small for the commitment (bit length < 7)"; return VP_EINVAL; }
    if (ctx->pcs) { if (mask) { ctx->err = "masked commitment: not on a sharded commitment"; return VP_EINVAL; } VPCHK(flush_pending(ctx, (size_t) -1)); return pcs_commit_private(ctx, root); }
    const int ln = n - 6, lm = n - 1;                     // slice_real_ele_cnt = 2^ln, slice_size = 2^lm (poly_commit.h:48-49)
    if (n > PC_MAX_N) { ctx->err = "input layer of more than 2^25 wires: the reference's commitment indexes its codeword with int (poly_commit.h:87-166), "
                                   "which overflows at 2^26 wires"; return VP_ELIMIT; }
    const u32 N = 1u << ln, M = 1u << lm;
    VPCHK(pc_hash_outstanding(ctx, 3u));                  // an earlier commitment under vp_pc_hash_late whose codeword this call replaces
    const bool late = ctx->hash_late && (!mask || ctx->hash_late >= 2);      // vp_pc_hash_late: the transforms only; vp_fri_commit hashes l with h and its own levels (a masked commit: VP_HASH_LATE_MASKED)
    pc_live_set(ctx, mask != nullptr);
    const PcLive &lv = ctx->pc_lv;
    u32 ms = 0;
    if (mask) { VPCHK(pc_mask_geometry(ctx, n_mask, &ms)); VPCHK(flush_pending(ctx, (size_t) -1)); }
    VPCHK(pc_root_table(ctx, lm));
    if (mask) VPCHK(pc_mask_alloc(ctx, ms));
    if (!ctx->pc_coef) {
        VPCHK(dalloc(ctx, &ctx->pc_coef, (size_t) 64 * N));
        VPCHK(dalloc(ctx, &ctx->pc_cw, (size_t) 64 * M));
        VPCHK(dalloc(ctx, &ctx->pc_tree, (size_t) M));    // 2 * (M/2) digests, heap layout
    }
    ctx->ev_used = 0;
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    // l_coef = iFFT of each slice; l_eval = its evaluations on the 2^lm-th roots (poly_commit.h:101-107)
    if (ctx->opt.real_pairs && ctx->vreal == 1 && ctx->opt.ntt_r8 && ln >= 13 && ln <= 17) {
        // a REAL witness (every circuit value real, vp_evaluate): slices p and p + 32 travel as ONE complex sequence through both transforms — half the
        // transforms of this call; the encoder's last store splits a row's values into the two slices' (k_ntt8_rows, Ntt8Args)
        // (PcLive: pair_rows = ceil(live / 2) rows, 32 for a full layer; at odd live the last partner is the first dead slice — zeros in, zeros out)
        VPCHK(pc_live_zero_cw(ctx, lv.pair_end()));
        VPCHK(pc_launch_ntt8(ctx, ctx->L[0].val, ctx->pc_coef, ln, lm, 1, lv.pair_rows, 1, N, lv.pair_rows));
        VPCHK(pc_launch_ntt8(ctx, ctx->pc_coef, ctx->pc_cw, ln, lm, 0, lv.pair_rows, 32, N, lv.pair_rows));
    } else {
        VPCHK(pc_live_zero_cw(ctx, lv.live));
        VPCHK(pc_launch_ntt(ctx, ctx->L[0].val, ctx->pc_coef, ln, lm, 1, lv.live, 1, N));
        VPCHK(pc_launch_ntt(ctx, ctx->pc_coef, ctx->pc_cw, ln, lm, 0, lv.live, 32, N));
    }
    ctx->pc_mask_ms = 0;
    if (mask) {
        // the 65th slice: the padded mask's low-degree extension (poly_commit.h:74-86); its pairs close the leaf chains (fri.cpp:107-122)
        VPCHK(pc_mask_lde(ctx, mask, n_mask, ms, ctx->pc_lm_cw));
        ctx->pc_mask_ms = ms;
    }
    if (late) {
        ctx->pc_unhashed |= 1u; ctx->late_root[0] = root;
        ctx->pc_private_done = true; ++ctx->private_epoch;
        ctx->pc_public_done = false;
        return defer_end(ctx, ev_a, VP_PH_PRIVATE, [ctx](float ms) { ctx->commit_ms = ms; return VP_OK; });
    }
    // leaf chains + tree (fri.cpp:95-127): all 64 slices
    void *st = nullptr;
    VPCHK(ring_alloc(ctx, 32, &st));
    VPCHK(pc_hash_oracle(ctx, 0, st));
    ctx->pc_private_done = true; ++ctx->private_epoch;
    ctx->pc_public_done = false;                          // a commit_public / FRI state of an earlier proof does not belong to this codeword
    return defer_end(ctx, ev_a, VP_PH_PRIVATE, [ctx, root, st](float ms) { memcpy(root, st, 32); ctx->commit_ms = ms; return VP_OK; });
}

int vp_commit_private(vp_ctx *ctx, uint8_t root[32]) {
    if (!ctx || !ctx->evaluated || !root) return VP_EINVAL;
    VP_ENTER_Q(ctx);
    return pc_commit_private_body(ctx, root, nullptr, 0);
}
// commit_private_array with a mask vector (lib/virgo/src/poly_commit.h:41-124): the reference's own prover passes one zero (src/prover.cpp:526) — vp_commit_private
int vp_commit_private_masked(vp_ctx *ctx, const vp_F *mask, uint64_t n_mask, uint8_t root[32]) {
    if (!ctx || !ctx->evaluated || !root || !mask) return VP_EINVAL;
    VP_ENTER(ctx);
    const int keep = ctx->deferred;
    ctx->deferred = 0;                                    // the mask is read during the call: finished here
    const int rc = pc_commit_private_body(ctx, root, mask, n_mask);
    ctx->deferred = keep;
    return rc;
}

// The caller's public vector (pageable memory: the reference hands a std::vector, src/prover.cpp:542) -> ctx->pc_pub.  With the pinned staging of
// vp_warm: four host threads copy it into pinned memory in 4 MB pieces while the copy engine takes the pieces that are ready, in order — the upload
// runs at the bus's speed instead of the pageable path's.  Without it: one hipMemcpyAsync from the caller's memory, as before.
static int pc_upload_pub(vp_ctx *ctx, const vp_F *pub, size_t bytes, F *dst = nullptr) {       // dst: another device array than ctx->pc_pub (vp_pc_public_evals)
    if (!dst) dst = ctx->pc_pub;
    if (!ctx->h_pub || ctx->h_pub_cap < bytes || bytes < ((size_t) 8 << 20)) {
        HIPCHK(hipMemcpyAsync(dst, pub, bytes, hipMemcpyHostToDevice, ctx->stream));
        return VP_OK;
    }
    const size_t piece = (size_t) 4 << 20, n_pieces = (bytes + piece - 1) / piece;
    const int n_thr = 4;
    std::vector<std::atomic<int>> ready(n_pieces);
    for (auto &r : ready) r.store(0, std::memory_order_relaxed);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(pub);
    std::vector<std::thread> thr;
    for (int t = 0; t < n_thr; ++t)
        thr.emplace_back([&, t]() {
            for (size_t q = t; q < n_pieces; q += n_thr) {
                const size_t off = q * piece, len = std::min(piece, bytes - off);
                memcpy(ctx->h_pub + off, src + off, len);
                ready[q].store(1, std::memory_order_release);
            }
        });
    int rc = VP_OK;
    for (size_t q = 0; q < n_pieces && rc == VP_OK; ++q) {
        while (!ready[q].load(std::memory_order_acquire)) std::this_thread::yield();
        const size_t off = q * piece, len = std::min(piece, bytes - off);
        if (hipMemcpyAsync(reinterpret_cast<unsigned char *>(dst) + off, ctx->h_pub + off, len, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { ctx->err = "hipMemcpyAsync (public vector)"; rc = VP_EHIP; }
    }
    for (auto &t : thr) t.join();
    return rc;
}

static int pc_fold0_consts(vp_ctx *ctx, int lm);
// vp_warm (include/vpgpu.h): everything the commitment allocates or builds on first use — the order-M root table, the circles and the T2 table of the
// transforms, their scratch, every codeword / tree / FRI buffer, the fold constants, the pinned staging of the public vector — BEFORE a prover call, where
// the reference has its namespace-scope new[]s (lib/virgo/src/poly_commit.cpp:4-13, fri.cpp:13-34): outside `prove time`.
static int pc_warm(vp_ctx *ctx) {
    const int n = ctx->L[0].bl;
    if (n < 7 || ctx->pcs) return VP_OK;
    const int ln = n - 6, lm = n - 1;
    if (n > PC_MAX_N) return VP_OK;                        // vp_commit_private refuses it
    const u32 N = 1u << ln, M = 1u << lm;
    VPCHK(pc_root_table(ctx, lm));
    if (!ctx->pc_coef) {
        VPCHK(dalloc(ctx, &ctx->pc_coef, (size_t) 64 * N));
        VPCHK(dalloc(ctx, &ctx->pc_cw, (size_t) 64 * M));
        VPCHK(dalloc(ctx, &ctx->pc_tree, (size_t) M));
    }
    VPCHK(pc_public_alloc(ctx));
    struct Dry { vp_ctx *c; ~Dry() { c->pc_dry = false; } } dry{ctx};
    ctx->pc_dry = true;
    // the transform shapes of vp_commit_private (both forms), vp_commit_public / _eq (tensor and general), the quotient
    // (at the full 64 / 32 rows: the scratch then holds every live count, a masked commitment's 64 included)
    if (ctx->opt.real_pairs && ctx->vreal == 1 && ctx->opt.ntt_r8 && ln >= 13 && ln <= 17) {
        VPCHK(pc_launch_ntt8(ctx, ctx->L[0].val, ctx->pc_coef, ln, lm, 1, 32, 1, N, 32));
        VPCHK(pc_launch_ntt8(ctx, ctx->pc_coef, ctx->pc_cw, ln, lm, 0, 32, 32, N, 32));
    }
    VPCHK(pc_launch_ntt(ctx, ctx->L[0].val, ctx->pc_coef, ln, lm, 1, 64, 1, N));
    VPCHK(pc_launch_ntt(ctx, ctx->pc_coef, ctx->pc_cw, ln, lm, 0, 64, 32, N));
    VPCHK(pc_launch_ntt(ctx, ctx->pc_pub, ctx->pc_coef, ln, lm, 1, 1, 1, N));
    VPCHK(pc_launch_ntt(ctx, ctx->pc_coef, ctx->pc_q0, ln, lm, 0, 1, 32, N));
    VPCHK(pc_launch_ntt(ctx, ctx->pc_tmp, ctx->pc_tmp + (size_t) 128 * N, ln, lm, 1, 128, 1, N));
    ctx->pc_dry = false;
    {   // the dead slices' zero bytes (vp_pc_live.h), so that the first commitment does not pay for them
        pc_live_set(ctx, false);
        const bool pairs = ctx->opt.real_pairs && ctx->vreal == 1 && ctx->opt.ntt_r8 && ln >= 13 && ln <= 17;
        VPCHK(pc_live_zero_cw(ctx, pairs ? ctx->pc_lv.pair_end() : ctx->pc_lv.live));
        VPCHK(pc_live_zero_hcw(ctx));
        VPCHK(pc_live_zero_fri(ctx));
    }
    VPCHK(pc_fold0_consts(ctx, lm));
    if (pc_leaf_wg(ctx, (u64) M >> 1)) VPCHK(pc_leaf_prepare(ctx));
    VPCHK(pc_many_reserve(ctx, 33u * (2 + ln)));             // the query phase's records (vp_fri_query)
    if (!ctx->h_pub) {
        const size_t bytes = sizeof(F) << n;
        if (hipHostMalloc((void **) &ctx->h_pub, bytes, hipHostMallocDefault) == hipSuccess) ctx->h_pub_cap = bytes;
        else { ctx->h_pub = nullptr; (void) hipGetLastError(); }      // not fatal: the upload then reads the caller's memory directly
    }
    return VP_OK;
}
static int pc_commit_public_host(vp_ctx *ctx, const vp_F *pub, uint64_t n_pub, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32], const vp_F *pub_mask, uint64_t n_pub_mask) {
    if (ctx->pcs) { if (pub_mask) { ctx->err = "masked commitment: not on a sharded commitment"; return VP_EINVAL; } return pcs_commit_public(ctx, pub, n_pub, nullptr, inner, all_sum, root_h); }
    if (!ctx->pc_private_done) return VP_EINVAL;
    const int n = ctx->L[0].bl;
    if (n_pub != (1ull << n)) return VP_EINVAL;
    const u32 N = 1u << (n - 6);
    VPCHK(pc_public_alloc(ctx));
    VPCHK(pc_upload_pub(ctx, pub, sizeof(F) << n));
    ctx->ev_used = 0;
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    F corner[64];
    for (int i = 0; i < 64; ++i) corner[i] = f_make(pub[(size_t) i * N].real, pub[(size_t) i * N].img);
    const int keep_deferred = ctx->deferred;              // the caller's vector is read during the call and the tensor check reads a flag back: finished here
    ctx->deferred = 0;
    const int rc = pc_commit_public_body(ctx, ev_a, corner, 0, inner, all_sum, root_h, pub_mask, n_pub_mask);
    ctx->deferred = keep_deferred;
    return rc;
}

int vp_commit_public(vp_ctx *ctx, const vp_F *pub, uint64_t n_pub, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]) {
    if (!ctx || !ctx->evaluated || !pub || !inner || !all_sum || !root_h) return VP_EINVAL;
    VP_ENTER(ctx);
    if (ctx->pc_mask_ms) { ctx->err = "vp_commit_public: the private commitment carries a mask (vp_commit_public_masked)"; return VP_EINVAL; }
    return pc_commit_public_host(ctx, pub, n_pub, inner, all_sum, root_h, nullptr, 0);
}
// commit_public_array with a public mask vector (lib/virgo/src/poly_commit.h:126-349) behind vp_commit_private_masked: the mask pads to the private mask's length
int vp_commit_public_masked(vp_ctx *ctx, const vp_F *pub, uint64_t n_pub, const vp_F *pub_mask, uint64_t n_pub_mask, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]) {
    if (!ctx || !ctx->evaluated || !pub || !pub_mask || !inner || !all_sum || !root_h) return VP_EINVAL;
    VP_ENTER(ctx);
    if (!ctx->pc_mask_ms) { ctx->err = "vp_commit_public_masked: vp_commit_private_masked first"; return VP_EINVAL; }
    if (n_pub_mask < 1 || n_pub_mask > ctx->pc_mask_ms) { ctx->err = "public mask longer than the private commitment's padded mask"; return VP_EINVAL; }
    return pc_commit_public_host(ctx, pub, n_pub, inner, all_sum, root_h, pub_mask, n_pub_mask);
}

// vp_commit_public_eq / vp_commit_public_eq_masked behind their checks (unsharded; the point canonical, n coordinates): eq(point, .) built on the device, the 64
// corners on the host, then the quotient pipeline (with the public mask, if there is one)
static int pc_commit_public_eq_body(vp_ctx *ctx, const vp_F *point, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32], const vp_F *pub_mask, uint64_t n_pub_mask) {
    const int n = ctx->L[0].bl;
    VPCHK(pc_public_alloc(ctx));
    // the public vector never crosses PCIe: eq(point, .) is built where it is consumed (two half tables by one workgroup, then one
    // product per entry — initBetaTable, src/utils.cpp:29-45)
    F *dr = ctx->pc_eq, *dbf = ctx->pc_eq + 32, *dbs = dbf + ((size_t) 1 << ((n + 1) / 2));
    F *hr = nullptr;                                       // pinned until the stream has taken it
    VPCHK(ring_alloc(ctx, 32 * sizeof(F), (void **) &hr));
    for (int i = 0; i < n; ++i) hr[i] = f_make(point[i].real, point[i].img);
    hr[n] = f_one();
    ctx->ev_used = 0;
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    HIPCHK(hipMemcpyAsync(dr, hr, (n + 1) * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_beta_half, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, (const F *) dr, n, (const F *) (dr + n), dbf, dbs);
    PC_PROF(VP_K_PC_POINTWISE, grid_for(1ull << n), 1, 16ull << n, 1ull << n,
            hipLaunchKernelGGL(k_beta_expand, dim3(grid_for(1ull << n)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) dbf, (const F *) dbs, n >> 1,
                               (u32) (1u << n), ctx->pc_pub));
    // corner[i] = pub[i N] = eq(point, i N): the host forms these 64 values itself (vp_pc_corners.h: the same field elements as the table's) instead of
    // reading them back — no wait for the device
    F corner[64];
    pc_eq_corners(hr, n, corner);
    return pc_commit_public_body(ctx, ev_a, corner, 1, inner, all_sum, root_h, pub_mask, n_pub_mask);
}
int vp_commit_public_eq(vp_ctx *ctx, const vp_F *point, int n_point, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]) {
    if (!ctx || !ctx->evaluated || !point || !inner || !all_sum || !root_h) return VP_EINVAL;
    VP_ENTER_Q(ctx);
    if (ctx->pc_mask_ms) { ctx->err = "vp_commit_public_eq: the private commitment carries a mask (vp_commit_public_eq_masked, vp_commit_public_masked)"; return VP_EINVAL; }
    if (!(ctx->pcs ? pcs_private_done(ctx) : ctx->pc_private_done)) return VP_EINVAL;
    const int n = ctx->L[0].bl;
    if (n_point != n) return VP_EINVAL;
    for (int i = 0; i < n; ++i) if (point[i].real >= P61 || point[i].img >= P61) { ctx->err = "vp_commit_public_eq: non-canonical coordinate"; return VP_EINVAL; }
    // a sharded commitment: every rank is handed the point and builds what it needs of the table itself (pcs_commit_public)
    if (ctx->pcs) { VPCHK(flush_pending(ctx, (size_t) -1)); return pcs_commit_public(ctx, nullptr, 0, point, inner, all_sum, root_h); }
    return pc_commit_public_eq_body(ctx, point, inner, all_sum, root_h, nullptr, 0);
}
// vp_commit_public_masked on pub = eq(point, .) built on the device: vp_commit_public_eq's table and corners, vp_commit_public_masked's checks and limits.  Every
// refusal comes before the first launch; the mask is copied during the call, so the call may be deferred like its unmasked twin.
int vp_commit_public_eq_masked(vp_ctx *ctx, const vp_F *point, int n_point, const vp_F *pub_mask, uint64_t n_pub_mask, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]) {
    if (!ctx || !ctx->evaluated || !point || !pub_mask || !inner || !all_sum || !root_h) return VP_EINVAL;
    VP_ENTER_Q(ctx);
    if (ctx->pcs) { ctx->err = "masked commitment: not on a sharded commitment"; return VP_EINVAL; }
    if (!ctx->pc_mask_ms || !ctx->pc_private_done) { ctx->err = "vp_commit_public_eq_masked: vp_commit_private_masked first"; return VP_EINVAL; }
    if (n_pub_mask < 1 || n_pub_mask > ctx->pc_mask_ms) { ctx->err = "public mask longer than the private commitment's padded mask"; return VP_EINVAL; }
    const int n = ctx->L[0].bl;
    if (n_point != n) return VP_EINVAL;
    for (int i = 0; i < n; ++i) if (point[i].real >= P61 || point[i].img >= P61) { ctx->err = "vp_commit_public_eq_masked: non-canonical coordinate"; return VP_EINVAL; }
    for (uint64_t i = 0; i < n_pub_mask; ++i) if (pub_mask[i].real >= P61 || pub_mask[i].img >= P61) { ctx->err = "non-canonical mask element"; return VP_EINVAL; }
    return pc_commit_public_eq_body(ctx, point, inner, all_sum, root_h, pub_mask, n_pub_mask);
}

int vp_fri_step(vp_ctx *ctx, const vp_F *r, uint8_t root[32]) {
    if (!ctx || !r || !root) return VP_EINVAL;
    if (ctx->pcs) { VP_ENTER(ctx); return pcs_fri_step(ctx, r, root); }
    if (!ctx->pc_public_done) return VP_EINVAL;
    VP_ENTER(ctx);
    VPCHK(pc_hash_outstanding(ctx, 3u));                  // (vp_pc_hash_late: only the one-pass vp_fri_commit merges)
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, M = 1u << lm;
    if (!ctx->pc_fri_all) {
        VPCHK(dalloc(ctx, &ctx->pc_fri_all, (size_t) 64 * M));            // every level's codeword is kept for the openings
        VPCHK(dalloc(ctx, &ctx->pc_fri_tree, (size_t) M));
    }
    const u32 live = ctx->pc_mask_ms ? 64u : ctx->pc_lv.live;      // slices >= live: a zero oracle and zero levels (vp_pc_live.h), kept as zero bytes
    VPCHK(pc_live_zero_fri(ctx));                                   // (all 64 live under a mask: nothing to zero, and the mark says so afterwards)
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (ctx->fri_step < 0) {
        // virtual oracle in place over the q codeword; S_0 per slice sits behind all_sum in pc_small
        const PcSlices v = pc_slices(ctx, live);
        hipLaunchKernelGGL(k_pc_virtual_oracle, dim3(nblk((u64) live * M)), dim3(VP_BLOCK), 0, ctx->stream, v.lcw, v.qcw, v.hcw, v.S0(), N, ctx->pc_rt, M >> 1,
                           f_make(N, 0), live, v.q0_arg(), v.qs_arg());
        ctx->fri_step = 0;
        if (ctx->pc_mask_ms) pc_mask_vo(ctx, false);
    }
    const int k = ctx->fri_step;
    if (k >= ln) { ctx->err = "FRI commit phase already finished"; return VP_EINVAL; }
    const FriLayout fl(ln, 0);
    const u32 Nk = N >> k, No = Nk >> 1;
    const F *in = k == 0 ? ctx->pc_qcw : ctx->pc_fri_all + fl.cw(k - 1);
    F *out = ctx->pc_fri_all + fl.cw(k);
    F rf; memcpy(&rf, r, sizeof(F));
    hipLaunchKernelGGL(k_fri_fold, dim3(nblk((u64) vp_fold_groups(live, VP_FOLD_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, in, out, Nk, k, ctx->pc_rt, M >> 1, rf,
                       host_inv_real(2), 0, 0u, live);
    // leaves of the folded codeword (M_{k+1} / 2 of them) + tree
    Dig *tree = ctx->pc_fri_tree + fl.tree(k);
    // the mask slice folds like the others (fri.cpp:366-374) and its pair closes every leaf chain of the level (:403-411)
    const F *out_m = ctx->pc_mask_ms ? pc_mask_fold(ctx, k, rf, false) : nullptr;
    VPCHK(pc_hash_level(ctx, out, No, out_m, tree));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(hipMemcpyAsync(root, tree + 1, 32, hipMemcpyDeviceToHost, ctx->stream));
    VPCHK(check_stream(ctx));
    ctx->fri_step = k + 1;
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->commit_ms = ms;
    return VP_OK;
}

// the per-coset constants of the first fold (k_fri_fold0_vo / _vo3): [b] = w_M^-b, [32 + b] = w_32^b - 1
static int pc_fold0_consts(vp_ctx *ctx, int lm) {
    if (ctx->pc_cbuf_lm == lm) return VP_OK;                // once per circuit
    F *cb = nullptr;                                        // pinned until the stream has taken it
    VPCHK(ring_alloc(ctx, 64 * sizeof(F), (void **) &cb));
    const F wM = host_root_of_unity(lm), wMi = host_pow(wM, (unsigned __int128) P61 * P61 - 2), w32 = host_root_of_unity(5);
    F pb = f_one(), pn = f_one();
    for (int b = 0; b < 32; ++b) { cb[b] = pb; cb[32 + b] = f_sub(pn, f_one()); pb = f_mul(pb, wMi); pn = f_mul(pn, w32); }
    HIPCHK(hipMemcpyAsync(ctx->pc_cbuf, cb, 64 * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    ctx->pc_cbuf_lm = lm;
    return VP_OK;
}

int vp_fri_commit(vp_ctx *ctx, const vp_F *r, int n_steps, uint8_t *roots) {
    if (!ctx || !r || !roots || n_steps < 1) return VP_EINVAL;
    VP_ENTER_Q(ctx);
    if (ctx->pcs) { VPCHK(flush_pending(ctx, (size_t) -1)); return pcs_fri_commit(ctx, r, n_steps, roots); }
    if (!ctx->pc_public_done) return VP_EINVAL;
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, M = 1u << lm;
    if (ctx->fri_step >= 0 && ctx->fri_step != 0) { ctx->err = "vp_fri_commit after vp_fri_step"; return VP_EINVAL; }
    if (n_steps > ln || n_steps > VP_FRI_MAX) { ctx->err = "too many FRI steps"; return VP_EINVAL; }
    // A commitment with a mask slice takes the same pass: its 64 slices through the folds below (all live), the 65th in arrays of its own behind them
    // (pc_mask_vo, pc_mask_fold), and its pairs close the chains of the one leaf launch (FriLeafArgs::mask)
    const bool masked = ctx->pc_mask_ms != 0;
    if (!ctx->pc_fri_all) {
        VPCHK(dalloc(ctx, &ctx->pc_fri_all, (size_t) 64 * M));
        VPCHK(dalloc(ctx, &ctx->pc_fri_tree, (size_t) M));
    }
    Dig *d_roots = nullptr;
    if (!ctx->pc_fri_roots) VPCHK(dalloc(ctx, &ctx->pc_fri_roots, (size_t) VP_FRI_MAX));
    d_roots = ctx->pc_fri_roots;
    ctx->ev_used = 0;
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    // the virtual oracle (poly_commit.h:294-318) is consumed by the first fold only: fused into it (k_fri_fold0_vo / k_fri_fold0_vo3)
    ctx->fri_step = 0;
    // slices >= live have a zero oracle and zero levels (vp_pc_live.h): the folds leave them out, the level regions keep their zero bytes for the hashes
    u32 live = ctx->pc_lv.live;
    VPCHK(pc_live_zero_fri(ctx));
    // folds of every level, back to back
    const FriLayout fl(ln, 0);
    const PcSlices v = pc_slices(ctx, live);             // the first fold reads l, q, h, S_0 and the tensor pair through it
    FriLeafArgs la{}; MerkleArgs ma{};
    // vp_pc_hash_late: the oracles whose commit stopped behind its transforms go IN FRONT of the levels in the same lists — an l or h codeword is an entry
    // with N values per coset and 16 N leaves like a level's.  VP_FRI_MAX covers n_steps + 2 (n <= 25: 21 entries) and the u32 leaf offsets 3 x 2^23 leaves.
    if (n_steps + 2 > VP_FRI_MAX) VPCHK(pc_hash_outstanding(ctx, 3u));
    const unsigned merged = ctx->pc_unhashed;
    uint8_t *late_root[2] = {nullptr, nullptr};
    int ne = 0;
    for (int o = 0; o < 2; ++o) {
        if (!(merged >> o & 1)) continue;
        Dig *tree = o ? ctx->pc_tree_h : ctx->pc_tree;
        const u32 n_leaves = M >> 1;
        ma.tree[ne] = tree; ma.count[ne] = n_leaves;
        la.cw[ne] = o ? ctx->pc_hcw : ctx->pc_cw; la.leaves[ne] = tree + n_leaves; la.N[ne] = N;
        if (masked) la.mask[ne] = o ? ctx->pc_hm_cw : ctx->pc_lm_cw;
        late_root[ne] = ctx->late_root[o];
        ++ne;
    }
    const int nt = ne + n_steps;                          // trees of this call
    // folds 0, 1, 2 in one pass (k_fri_fold0_vo3): every challenge is here before the first fold starts
    const bool fold3 = n_steps >= 3 && ln >= 9;       // (E = N / 8 >= 64: a wave per offset)
    for (int k = 0; k < n_steps; ++k) {
        const u32 Nk = N >> k, No = Nk >> 1;
        const F *in = k == 0 ? ctx->pc_qcw : ctx->pc_fri_all + fl.cw(k - 1);
        F *out = ctx->pc_fri_all + fl.cw(k);
        F rf; memcpy(&rf, r + k, sizeof(F));
        if (fold3 && k < 3) {
            if (k == 0) {
                const F *rtn = nullptr;
                VPCHK(pc_circle_roots(ctx, lm, ln, &rtn));
                VPCHK(pc_fold0_consts(ctx, lm));
                F r1, r2; memcpy(&r1, r + 1, sizeof(F)); memcpy(&r2, r + 2, sizeof(F));
                F *o1 = out, *o2 = o1 + (size_t) 64 * 32 * No, *o3 = o2 + (size_t) 64 * 32 * (No >> 1);       // the levels lie end to end (FriLayout::cw)
                const u32 E = N >> 3;
                // VP_VO_GRP slice groups per workgroup where that still leaves >= 2048 workgroups (N >= 2^14), one group per workgroup below
                const bool grouped = (64 / VP_VO_SPT / VP_VO_GRP) * 32 * (E >> 6) >= 2048;
                const u32 grid3 = vp_fold_groups(live, VP_VO_SPT * (grouped ? VP_VO_GRP : 1)) * 32 * (E >> 6);      // the workgroups whose slices include a live one
                const void *fold3 = v.tensor ? (grouped ? (const void *) k_fri_fold0_vo3<true, VP_VO_GRP> : (const void *) k_fri_fold0_vo3<true, 1>)
                                                     : (grouped ? (const void *) k_fri_fold0_vo3<false, VP_VO_GRP> : (const void *) k_fri_fold0_vo3<false, 1>);
                const F *a_lcw = v.lcw, *a_qcw = v.qcw, *a_hcw = v.hcw, *a_S0 = v.S0(), *a_cb = ctx->pc_cbuf, *a_q0 = v.q0_arg(), *a_qs = v.qs_arg();
                u32 a_N = N;
                F a_half = f_mul(f_make(N, 0), host_inv_real(2)), a_inv2 = host_inv_real(2);
                void *args3[] = {&a_lcw, &a_qcw, &a_hcw, &a_S0, &o1, &o2, &o3, &a_N, &rtn, &a_cb, &rf, &r1, &r2, &a_half, &a_inv2, &a_q0, &a_qs, &live};
                PC_PROF(VP_K_FRI_FOLD, grid3, 1, (v.tensor ? 80ull : 112ull) * live * 32 * No + 16ull * live * 32 * ((No >> 1) + (No >> 2)),
                        (u64) (v.tensor ? 9 : 7) * live * 32 * No + 3ull * live * 32 * ((No >> 1) + (No >> 2)),
                        (void) hipLaunchKernel(fold3, dim3(grid3), dim3(256), args3, 0, ctx->stream));
            }
        }
        else if (k == 0)      // algorithmic bytes: l and h at both positions + the output (q is one slice of a tensor vector, or read like l)
        {
            // x^-1 = w_M^-(32 a + b) = w_N^-a . w_M^-b: the a part from the contiguous order-N circle (lanes run along a), the b part and x^N - 1 =
            // w_32^b - 1 from 2 x 32 per-coset constants (before: one gather per output from the 32 MB order-M table at a stride of 512 bytes —
            // PMC: 18.4 GB fetched for 10.7 GB algorithmic)
            const F *rtn = nullptr;
            VPCHK(pc_circle_roots(ctx, lm, ln, &rtn));
            VPCHK(pc_fold0_consts(ctx, lm));
            PC_PROF(VP_K_FRI_FOLD, nblk((u64) vp_fold_groups(live, VP_VO_SPT) * 32 * No), 1, (v.tensor ? 80ull : 112ull) * live * 32 * No, (u64) (v.tensor ? 9 : 7) * live * 32 * No,
                    hipLaunchKernelGGL(k_fri_fold0_vo, dim3(nblk((u64) vp_fold_groups(live, VP_VO_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) v.lcw, (const F *) v.qcw,
                                       (const F *) v.hcw, (const F *) v.S0(), out, N, rtn, (const F *) ctx->pc_cbuf, rf,
                                       f_mul(f_make(N, 0), host_inv_real(2)), v.q0_arg(), v.qs_arg(), live));
        }
        else
        PC_PROF(VP_K_FRI_FOLD, nblk((u64) vp_fold_groups(live, VP_FOLD_SPT) * 32 * No), 1, 48ull * live * 32 * No, (u64) 3 * live * 32 * No,
                hipLaunchKernelGGL(k_fri_fold, dim3(nblk((u64) vp_fold_groups(live, VP_FOLD_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, in, out, Nk, k, ctx->pc_rt, M >> 1, rf,
                                   host_inv_real(2), 0, 0u, live));
        // every level, the single-value last one included, goes into the one leaf-hash launch (the chain of 65 Keccak-f is a fixed ~1 ms latency
        // however few leaves there are)
        const u32 n_leaves = 16 * No;
        Dig *tree = ctx->pc_fri_tree + fl.tree(k);
        ma.tree[ne + k] = tree; ma.count[ne + k] = n_leaves;
        la.cw[ne + k] = out; la.leaves[ne + k] = tree + n_leaves; la.N[ne + k] = No;
    }
    if (masked) {      // the mask slice behind them: what vp_fri_step queues for it, without the waits in between
        pc_mask_vo(ctx, true);
        for (int k = 0; k < n_steps; ++k) {
            F rf; memcpy(&rf, r + k, sizeof(F));
            la.mask[ne + k] = pc_mask_fold(ctx, k, rf, true);
        }
    }
    la.n = ma.n = nt;
    VPCHK(pc_hash_leaves(ctx, la, true));
    if (merged) { ctx->pc_unhashed = 0; ctx->late_root[0] = ctx->late_root[1] = nullptr; }      // queued: whatever follows in stream order finds the trees
    VPCHK(pc_merkle_trees(ctx, ma, d_roots));
    unsigned char *st = nullptr;                          // the merged oracles' roots | the levels' roots: one pinned copy
    VPCHK(ring_alloc(ctx, (size_t) 32 * nt, (void **) &st));
    HIPCHK(hipMemcpyAsync(st, d_roots, (size_t) 32 * nt, hipMemcpyDeviceToHost, ctx->stream));
    ctx->fri_step = n_steps;
    uint8_t *lr0 = late_root[0], *lr1 = late_root[1];
    return defer_end(ctx, ev_a, VP_PH_FRI, [ctx, st, roots, n_steps, ne, lr0, lr1](float ms) {
        if (ne > 0 && lr0) memcpy(lr0, st, 32);
        if (ne > 1 && lr1) memcpy(lr1, st + 32, 32);
        memcpy(roots, st + 32 * (size_t) ne, (size_t) 32 * n_steps);
        ctx->commit_ms = ms;
        return VP_OK;
    });
}

// The commit phase of a NON-INTERACTIVE commitment (steps 8 and 9 of the chain in host/vphost.h): challenge k + 1 is drawn from the root of level k, so the
// levels cannot share a leaf launch or a fused fold as in vp_fri_commit — but nothing of that needs the host.  The state and the challenges live in device
// memory (vp_ctx::pc_fs); k_fs_draw draws r_0, every fold reads its challenge through a pointer (k_fri_fold0_vo_p, k_fri_fold_p, k_fri_fold_one_p: the bodies
// of the by-value kernels), every level is hashed by pc_hash_level's rules and its tree top (k_merkle_top_fs) performs D(2 + k, root) and C(k + 1).  The whole
// phase is queued without a host wait; roots, challenges and the closing state come back in one pinned copy.
int vp_fri_commit_fs(vp_ctx *ctx, const uint8_t state_in[32], uint8_t *roots, vp_F *r_out, uint8_t state_out[32]) {
    if (!ctx) return VP_EINVAL;
    VP_ENTER(ctx);
    // every refusal before anything is queued
    if (!state_in || !roots || !r_out || !state_out) { ctx->err = "vp_fri_commit_fs: a null argument"; return VP_EINVAL; }
    if (ctx->pcs) { ctx->err = "vp_fri_commit_fs: not built for a sharded commitment (vp_pc_set_shard)"; return VP_EINVAL; }
    if (ctx->L.empty() || !ctx->pc_public_done) { ctx->err = "vp_fri_commit_fs: vp_commit_public first"; return VP_EINVAL; }
    if (ctx->fri_step >= 0) { ctx->err = "vp_fri_commit_fs after vp_fri_step or vp_fri_commit of the same commitment"; return VP_EINVAL; }
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    if (ln < 1 || ln > VP_FRI_MAX) { ctx->err = "vp_fri_commit_fs: too many FRI steps"; return VP_ELIMIT; }
    const u32 N = 1u << ln, M = 1u << lm;
    VPCHK(pc_hash_outstanding(ctx, 3u));                  // (vp_pc_hash_late: only the one-pass vp_fri_commit merges)
    const bool masked = ctx->pc_mask_ms != 0;
    if (!ctx->pc_fri_all) {
        VPCHK(dalloc(ctx, &ctx->pc_fri_all, (size_t) 64 * M));
        VPCHK(dalloc(ctx, &ctx->pc_fri_tree, (size_t) M));
    }
    constexpr size_t FS_DIGS = VP_FRI_MAX + VP_FRI_MAX / 2 + 1;          // roots | challenges | state
    if (!ctx->pc_fs) VPCHK(dalloc(ctx, &ctx->pc_fs, FS_DIGS));
    Dig *d_roots = ctx->pc_fs, *d_state = ctx->pc_fs + VP_FRI_MAX + VP_FRI_MAX / 2;
    F *d_r = reinterpret_cast<F *>(ctx->pc_fs + VP_FRI_MAX);
    const F *rtn = nullptr;
    VPCHK(pc_circle_roots(ctx, lm, ln, &rtn));
    VPCHK(pc_fold0_consts(ctx, lm));
    unsigned char *h_in = nullptr, *st = nullptr;         // pinned: the state on its way in, the block on its way out
    VPCHK(ring_alloc(ctx, 32, (void **) &h_in));
    VPCHK(ring_alloc(ctx, FS_DIGS * sizeof(Dig), (void **) &st));
    memcpy(h_in, state_in, 32);
    ctx->ev_used = 0;
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    HIPCHK(hipMemsetAsync(ctx->pc_fs, 0, FS_DIGS * sizeof(Dig), ctx->stream));
    HIPCHK(hipMemcpyAsync(d_state, h_in, 32, hipMemcpyHostToDevice, ctx->stream));
    ctx->fri_step = 0;
    const u32 live = masked ? 64u : ctx->pc_lv.live;     // slices >= live: a zero oracle and zero levels (vp_pc_live.h), kept as zero bytes
    VPCHK(pc_live_zero_fri(ctx));
    const FriLayout fl(ln, 0);
    const PcSlices v = pc_slices(ctx, live);
    hipLaunchKernelGGL(k_fs_draw, dim3(1), dim3(64), 0, ctx->stream, d_state, (const Dig *) nullptr, (u64) 0, (u64) 0, d_r);      // r_0 = C(0)
    if (masked) pc_mask_vo(ctx, true);
    for (int k = 0; k < ln; ++k) {
        const u32 Nk = N >> k, No = Nk >> 1;
        const F *in = k == 0 ? ctx->pc_qcw : ctx->pc_fri_all + fl.cw(k - 1);
        F *out = ctx->pc_fri_all + fl.cw(k);
        const F *rk = d_r + k;
        if (k == 0)       // the virtual oracle is consumed by the first fold only: fused into it, as in vp_fri_commit
            PC_PROF(VP_K_FRI_FOLD, nblk((u64) vp_fold_groups(live, VP_VO_SPT) * 32 * No), 1, (v.tensor ? 80ull : 112ull) * live * 32 * No, (u64) (v.tensor ? 9 : 7) * live * 32 * No,
                    hipLaunchKernelGGL(k_fri_fold0_vo_p, dim3(nblk((u64) vp_fold_groups(live, VP_VO_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) v.lcw, (const F *) v.qcw,
                                       (const F *) v.hcw, (const F *) v.S0(), out, N, rtn, (const F *) ctx->pc_cbuf, rk,
                                       f_mul(f_make(N, 0), host_inv_real(2)), v.q0_arg(), v.qs_arg(), live));
        else
            PC_PROF(VP_K_FRI_FOLD, nblk((u64) vp_fold_groups(live, VP_FOLD_SPT) * 32 * No), 1, 48ull * live * 32 * No, (u64) 3 * live * 32 * No,
                    hipLaunchKernelGGL(k_fri_fold_p, dim3(nblk((u64) vp_fold_groups(live, VP_FOLD_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, in, out, Nk, k, ctx->pc_rt, M >> 1, rk,
                                       host_inv_real(2), 0, 0u, live));
        // the mask slice folds behind the 64 on the same stream, and its pair closes every leaf chain of the level
        const F *out_m = masked ? pc_mask_fold(ctx, k, f_zero(), true, rk) : nullptr;
        const u32 n_leaves = 16 * No;
        Dig *tree = ctx->pc_fri_tree + fl.tree(k);
        FriLeafArgs la{};
        la.cw[0] = out; la.leaves[0] = tree + n_leaves; la.N[0] = No; la.mask[0] = out_m; la.n = 1;
        VPCHK(pc_hash_leaves(ctx, la, true));
        MerkleArgs ma{};
        ma.tree[0] = tree; ma.count[0] = n_leaves; ma.n = 1;
        const PcFsTop top{d_state, (u64) (2 + k), (u64) (k + 1), k + 1 < ln ? d_r + k + 1 : nullptr};
        VPCHK(pc_merkle_trees(ctx, ma, d_roots + k, -1, &top));
    }
    HIPCHK(hipMemcpyAsync(st, ctx->pc_fs, FS_DIGS * sizeof(Dig), hipMemcpyDeviceToHost, ctx->stream));
    ctx->fri_step = ln;
    return defer_end(ctx, ev_a, VP_PH_FRI, [ctx, st, roots, r_out, state_out, ln](float ms) {
        memcpy(roots, st, (size_t) 32 * ln);
        memcpy(r_out, st + 32 * (size_t) VP_FRI_MAX, sizeof(F) * (size_t) ln);
        memcpy(state_out, st + 32 * (size_t) (VP_FRI_MAX + VP_FRI_MAX / 2), 32);
        ctx->commit_ms = ms;
        return VP_OK;
    });
}

// Test hook of the chain's device side.  op 0: one lane performs D(label, root) and C(counter) on `state`: the new state -> state_out, the challenge -> r_out.
// op 1: the reduction alone on raw words: the four words of `root` through fs_limb -> state_out, the first two also -> r_out (state, label, counter unused).
int vp_test_fs_draw(vp_ctx *ctx, int op, const uint8_t state[32], const uint8_t root[32], uint64_t label, uint64_t counter, uint8_t state_out[32], vp_F *r_out) {
    if (!ctx || !root || !state_out || !r_out || (op != 0 && op != 1) || (op == 0 && !state)) return VP_EINVAL;
    VP_ENTER(ctx);
    u64 *d = nullptr;                                      // state | root | out (4 words each) | r (2 words)
    HIPCHK(hipMalloc((void **) &d, 14 * sizeof(u64)));
    u64 h[14] = {0};
    if (op == 0) memcpy(h, state, 32);
    memcpy(h + 4, root, 32);
    int rc = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) == hipSuccess ? VP_OK : VP_EHIP;
    if (rc == VP_OK) {
        if (op == 0) hipLaunchKernelGGL(k_fs_draw, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<Dig *>(d), reinterpret_cast<const Dig *>(d + 4), (u64) label, (u64) counter, reinterpret_cast<F *>(d + 12));
        else hipLaunchKernelGGL(k_test_fs_limbs, dim3(1), dim3(64), 0, ctx->stream, (const u64 *) (d + 4), d + 8, 4u);
        rc = check_stream(ctx);
    }
    if (rc == VP_OK && hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) rc = VP_EHIP;
    (void) hipFree(d);
    if (rc != VP_OK) return rc;
    if (op == 0) { memcpy(state_out, h, 32); memcpy(r_out, h + 12, 16); }
    else { memcpy(state_out, h + 8, 32); memcpy(r_out, h + 8, 16); }
    return VP_OK;
}

// The proof-of-work search (include/vpgpu.h).  Windows ascend and are disjoint: window w holds 2^min(16 + 2 w, 24) nonces (cut at max_tries), so a few bits of
// work cost one short launch and many bits run in launches of 2^24; eight windows are queued behind each other before the host waits and reads the slot (a
// window behind a hit leaves on its first instruction).  The schedule is a function of max_tries alone, so the result is the same on every run — and of the
// internal tuning grind_window_log / grind_batch (24 / 8: profiles/fs_grind.md), which moves the windows and not the answer.
constexpr int FS_GRIND_BATCH_MAX = 64;
int vp_fs_grind(vp_ctx *ctx, const uint8_t state_in[32], int bits, uint64_t first, uint64_t max_tries, uint64_t *nonce, uint8_t state_out[32]) {
    if (!ctx) return VP_EINVAL;
    // every refusal before anything is queued
    if (!state_in || !nonce || !state_out) { ctx->err = "vp_fs_grind: a null argument"; return VP_EINVAL; }
    if (bits < 1 || bits > 48) { ctx->err = "vp_fs_grind: bits outside 1 .. 48"; return VP_EINVAL; }
    if (max_tries == 0 || first + (max_tries - 1) < first) { ctx->err = "vp_fs_grind: an empty range, or one that passes 2^64"; return VP_EINVAL; }
    VP_ENTER(ctx);
    constexpr size_t WORDS = 1 + 4 + 4 + FS_GRIND_BATCH_MAX / 2;  // slot | state out | state in | one 32-bit counter per window of a batch
    const u64 window_log = (u64) ctx->opt.grind_window_log;
    const int batch = ctx->opt.grind_batch;
    if (!ctx->fs_grind_buf) VPCHK(dalloc(ctx, &ctx->fs_grind_buf, WORDS));
    u64 *d = ctx->fs_grind_buf;
    u32 *d_worked = reinterpret_cast<u32 *>(d + 9);
    u64 h[WORDS];
    FsGrindArgs a{};
    memcpy(a.s, state_in, 32);
    a.bits = (u64) bits; a.mask = (1ull << bits) - 1; a.first = first;
    a.slot = reinterpret_cast<unsigned long long *>(d);
    if (ctx->profiling) ensure_event_pool(ctx);
    ctx->ev_used = 0;
    std::vector<std::pair<size_t, u32>> rows;             // per launch: its row of the table (or none) and the workgroups that searched
    std::vector<int> slots;
    u64 base = 0, found = ~0ull;
    for (u64 w = 0; base < max_tries && found == ~0ull;) {
        memset(h, 0, sizeof h);
        h[0] = ~0ull;
        memcpy(h + 5, state_in, 32);
        HIPCHK(hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, ctx->stream));      // (pageable: the copy is staged before the call returns)
        slots.clear();
        for (int q = 0; q < batch && base < max_tries; ++q, ++w) {
            a.base = base; a.count = std::min<u64>(1ull << std::min<u64>(16 + 2 * w, window_log), max_tries - base);
            a.iters = (u32) std::max<u64>(1, a.count / ((u64) VP_FS_GRIND_BLOCK * 4096));
            a.worked = d_worked + q;
            const u64 per = (u64) VP_FS_GRIND_BLOCK * a.iters;
            const u32 grid = (u32) ((a.count + per - 1) / per);
            const int sl = prof_begin(ctx, ctx->stream, VP_K_FS_GRIND, grid, 1, 0, a.count, (u32) a.iters, (u32) w);
            if (bits > 32) hipLaunchKernelGGL(k_fs_grind<true>, dim3(grid), dim3(VP_FS_GRIND_BLOCK), 0, ctx->stream, a);
            else hipLaunchKernelGGL(k_fs_grind<false>, dim3(grid), dim3(VP_FS_GRIND_BLOCK), 0, ctx->stream, a);
            prof_end(ctx, ctx->stream, sl);
            count_launch(ctx);
            slots.push_back(sl);
            base += a.count;
        }
        HIPCHK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        VPCHK(check_stream(ctx));
        found = h[0];
        const u32 *hw = reinterpret_cast<const u32 *>(h + 9);
        for (size_t q = 0; q < slots.size(); ++q) if (slots[q] >= 0) rows.emplace_back((size_t) slots[q], hw[q]);
    }
    if (ctx->profiling) {
        // a row's work: the nonces of the workgroups that searched (the last one may be cut at the window's end) — zero for a window behind a hit
        prof_collect(ctx);
        for (const auto &r : rows) {
            vp_launch_stat &st = ctx->lstats[r.first];
            st.work = std::min<u64>(st.work, (u64) r.second * VP_FS_GRIND_BLOCK * st.rounds);
            st.jobs = r.second;
        }
    }
    if (found == ~0ull) { ctx->err = "vp_fs_grind: no nonce in the range meets the work"; return VP_ELIMIT; }
    hipLaunchKernelGGL(k_fs_work_state, dim3(1), dim3(64), 0, ctx->stream, (const u64 *) (d + 5), (u64) bits, (u64) (first + found), d + 1);
    count_launch(ctx);
    HIPCHK(hipMemcpyAsync(h, d, 5 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    VPCHK(check_stream(ctx));
    if (h[1] & a.mask) { ctx->err = "vp_fs_grind: internal: the nonce found does not meet the work"; return VP_EHIP; }
    *nonce = first + found;
    memcpy(state_out, h + 1, 32);
    return VP_OK;
}

int vp_fri_final(vp_ctx *ctx, vp_F *final_code) {
    if (!ctx || !final_code) return VP_EINVAL;
    VP_ENTER_Q(ctx);
    if (ctx->pcs) { VPCHK(flush_pending(ctx, (size_t) -1)); return pcs_fri_final(ctx, final_code); }
    if (!ctx->pc_public_done) return VP_EINVAL;
    const int ln = ctx->L[0].bl - 6;
    if (ctx->fri_step != ln) { ctx->err = "FRI commit phase not finished"; return VP_EINVAL; }
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    F *cw = nullptr;
    VPCHK(ring_alloc(ctx, 64 * 32 * sizeof(F), (void **) &cw));
    HIPCHK(hipMemcpyAsync(cw, ctx->pc_fri_all + FriLayout(ln, 0).cw(ln - 1), 64 * 32 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    return defer_end(ctx, ev_a, VP_PH_FRI_FINAL, [cw, final_code](float) { pc_final_order(cw, final_code); return VP_OK; });      // (commit_ms stays the commit phase's)
}

// The mask slice's last codeword (fri::cpd.rs_codeword_msk[last], read by vpd_verifier.cpp:321-325): 32 values in the reference's interleaved order
// out[2 i + hi] = value at position i + 16 hi; all zero for the protocol's zero mask.
int vp_fri_final_mask(vp_ctx *ctx, vp_F out[32]) {
    if (!ctx || !out) return VP_EINVAL;
    VP_ENTER(ctx);
    if (ctx->pcs) { ctx->err = "vp_fri_final_mask: not on a sharded commitment"; return VP_EINVAL; }
    if (!ctx->pc_public_done) return VP_EINVAL;
    const int ln = ctx->L[0].bl - 6;
    if (ctx->fri_step != ln) { ctx->err = "FRI commit phase not finished"; return VP_EINVAL; }
    memset(out, 0, 32 * sizeof(vp_F));
    if (!ctx->pc_mask_ms) return VP_OK;
    F v[32];
    HIPCHK(hipMemcpyAsync(v, ctx->pc_fm + FriLayout(ln, 0).mask(ln - 1), sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    VPCHK(check_stream(ctx));
    for (u32 i = 0; i < 16; ++i) for (u32 hi = 0; hi < 2; ++hi) { out[2 * i + hi].real = v[i + 16 * hi].re; out[2 * i + hi].img = v[i + 16 * hi].im; }
    return VP_OK;
}

int vp_fri_open(vp_ctx *ctx, int oracle, uint64_t leaf, vp_F values[130], uint8_t *path, int path_capacity, int *path_len) {
    if (!ctx || !values || !path || !path_len || oracle < 0) return VP_EINVAL;
    VP_ENTER(ctx);
    PcOpenDesc d;
    VPCHK(pc_open_desc(ctx, oracle, &d));
    if (leaf >= d.n_leaves) return VP_EINVAL;
    if (d.top && !pcs_owns(ctx, leaf)) { ctx->err = "this rank does not own the leaf (owner = (leaf >> 5) mod world)"; return VP_EINVAL; }
    const int depth = pc_open_depth(d.n_leaves);
    if (path_capacity < 32 * (depth + 1)) return VP_EINVAL;
    if (!ctx->pc_open_buf) VPCHK(dalloc(ctx, &ctx->pc_open_buf, (size_t) 130 + 2 * 40));
    Dig *dpath = reinterpret_cast<Dig *>(ctx->pc_open_buf + 130);
    hipLaunchKernelGGL(k_pc_open, dim3(1), dim3(128), 0, ctx->stream, d, (u32) oracle, (u32) leaf, ctx->pc_open_buf, dpath);
    HIPCHK(hipMemcpyAsync(values, ctx->pc_open_buf, 130 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(path, dpath, 32 * (size_t) (depth + 1), hipMemcpyDeviceToHost, ctx->stream));
    VPCHK(check_stream(ctx));
    *path_len = depth + 1;
    return VP_OK;
}

int vp_fri_open_many(vp_ctx *ctx, int n, const int32_t *oracle, const uint64_t *leaf, vp_F *values, uint8_t *paths, int path_stride, int32_t *path_len) {
    if (!ctx || n < 0) return VP_EINVAL;
    if (n == 0) return VP_OK;
    if (!oracle || !leaf || !values || !paths || !path_len || path_stride < 0) return VP_EINVAL;
    if (n > PC_MANY_MAX) { ctx->err = "vp_fri_open_many: more than 2^16 requests"; return VP_ELIMIT; }
    VP_ENTER(ctx);
    PcManyPlan pl;
    VPCHK(pc_many_plan(ctx, n, oracle, leaf, path_stride, pl));
    VPCHK(pc_many_run(ctx, n, oracle, leaf, pl, [&](int i, const PcOpenRec &r) {
        memcpy(values + (size_t) 130 * i, r.v, 130 * sizeof(F));
        memcpy(paths + (size_t) path_stride * i, r.path, 32 * (size_t) pl.plen[i]);
    }));
    for (int i = 0; i < n; ++i) path_len[i] = pl.plen[i];
    return VP_OK;
}

// requests of `n_queries` repetitions in vp_fri_query's order: oracle 0, oracle 1, level 0 .. ln - 1 along the leaf chain of host/verifier.cpp
static int pc_query_requests(vp_ctx *ctx, int n_queries, const uint64_t *leaf0, std::vector<int32_t> &oracle, std::vector<uint64_t> &leaf) {
    // a sharded commitment: the drop-in state machine (vp_fri_step) is answered here; after the one-pass vp_fri_commit the calling pattern stays the
    // one-pass one, whose caller merges vp_fri_open_many over the ranks, as before
    if (ctx->pcs && pcs_fri_one_pass(ctx)) { ctx->err = "vp_fri_query: not after vp_fri_commit on a sharded commitment (merge vp_fri_open_many over the ranks)"; return VP_EINVAL; }
    if (ctx->L.empty() || !(ctx->pcs ? pcs_public_done(ctx) : ctx->pc_public_done)) return VP_EINVAL;
    const int ln = ctx->L[0].bl - 6;
    if ((ctx->pcs ? pcs_fri_done(ctx) : ctx->fri_step) != ln) { ctx->err = "FRI commit phase not finished"; return VP_EINVAL; }
    if ((u64) n_queries * (u64) (2 + ln) > (u64) PC_MANY_MAX) { ctx->err = "vp_fri_query: more than 2^16 openings"; return VP_ELIMIT; }
    const u64 M = 1ull << (ctx->L[0].bl - 1);
    oracle.clear(); leaf.clear();
    for (int q = 0; q < n_queries; ++q) {
        const u64 l0 = leaf0 ? leaf0[q] : 0;
        oracle.push_back(0); leaf.push_back(l0);
        oracle.push_back(1); leaf.push_back(l0);
        u64 D = M, t = l0;
        for (int k = 0; k < ln; ++k) { const u64 Dn = D / 2, lf = t % (Dn / 2); oracle.push_back(2 + k); leaf.push_back(lf); t = lf; D = Dn; }
    }
    return VP_OK;
}
int vp_fri_query_bytes(vp_ctx *ctx, int n_queries, uint64_t *bytes) {
    if (!ctx || !bytes || n_queries < 0) return VP_EINVAL;
    VP_ENTER(ctx);
    std::vector<int32_t> oracle; std::vector<uint64_t> leaf;
    VPCHK(pc_query_requests(ctx, n_queries, nullptr, oracle, leaf));
    PcManyPlan pl;
    VPCHK(pc_many_plan(ctx, (int) oracle.size(), oracle.data(), leaf.data(), -1, pl));
    *bytes = pl.layout;
    return VP_OK;
}
int vp_fri_query(vp_ctx *ctx, int n_queries, const uint64_t *leaf0, uint8_t *out, uint64_t capacity, uint64_t *n_written) {
    if (!ctx || n_queries < 0 || !n_written || (n_queries > 0 && (!leaf0 || !out))) return VP_EINVAL;
    VP_ENTER(ctx);
    std::vector<int32_t> oracle; std::vector<uint64_t> leaf;
    VPCHK(pc_query_requests(ctx, n_queries, leaf0, oracle, leaf));
    const int n = (int) oracle.size();
    PcManyPlan pl;
    VPCHK(pc_many_plan(ctx, n, oracle.data(), leaf.data(), -1, pl));
    // the layout is the unsharded one on every rank of a sharded commitment: a rank writes the openings it owns at their places and leaves the
    // other bytes alone (the rule of vp_fri_open_many), so the ranks' buffers merge into one
    if (pl.layout > capacity) { ctx->err = "vp_fri_query: output buffer too small (vp_fri_query_bytes)"; return VP_EINVAL; }
    std::vector<u64> at((size_t) n + 1, 0);
    for (int i = 0; i < n; ++i) at[i + 1] = at[i] + 130 * sizeof(F) + 32ull * pl.dlen[i];
    VPCHK(pc_many_run(ctx, n, oracle.data(), leaf.data(), pl, [&](int i, const PcOpenRec &r) {
        memcpy(out + at[i], r.v, 130 * sizeof(F));
        memcpy(out + at[i] + 130 * sizeof(F), r.path, 32 * (size_t) pl.plen[i]);
    }));
    *n_written = pl.layout;
    return VP_OK;
}

int vp_commit_stats(vp_ctx *ctx, double *commit_ms) {
    if (!ctx || !commit_ms) return VP_EINVAL;
    *commit_ms = ctx->commit_ms;
    return VP_OK;
}

int vp_test_sha3(vp_ctx *ctx, const uint8_t *in, uint8_t *out, uint64_t n) {
    if (!ctx || !in || !out) return VP_EINVAL;
    if (!n) return VP_OK;
    VP_ENTER(ctx);
    u64 *di = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc((void **) &di, n * 64));
    HIPCHK(hipMalloc((void **) &dout, n * 32));
    HIPCHK(hipMemcpy(di, in, n * 64, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_sha3, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, di, dout, (u32) n);
    int rc = check_stream(ctx);
    if (rc == VP_OK && hipMemcpy(out, dout, n * 32, hipMemcpyDeviceToHost) != hipSuccess) rc = VP_EHIP;
    (void) hipFree(di); (void) hipFree(dout);
    return rc;
}

#ifdef VP_LEAF_STAMPS
// Diagnostic build only (tools/leaf_in_step.py): the stamps the leaf-hash workgroups left since the last call (4 words each: memtime, memrealtime before;
// memtime, memrealtime << 1 | kernel after), and the leaf hash of the committed codeword alone, `reps` launches back to back.
int vp_debug_leaf_stamps(vp_ctx *ctx, uint64_t *out, unsigned cap, unsigned *n) {
    if (!ctx || !out || !n) return VP_EINVAL;
    VP_ENTER(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    unsigned cnt = 0;
    HIPCHK(hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(g_leaf_stamp_n), sizeof cnt));
    *n = std::min(std::min(cnt, 65536u), cap);
    if (*n) HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_leaf_stamps), (size_t) *n * 32));
    cnt = 0;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_leaf_stamp_n), &cnt, sizeof cnt));
    return VP_OK;
}
int vp_debug_leaf_only(vp_ctx *ctx, int reps) {
    if (!ctx || !ctx->pc_private_done || ctx->pcs) return VP_EINVAL;
    VP_ENTER(ctx);
    const int n = ctx->L[0].bl;
    FriLeafArgs la{};
    la.cw[0] = ctx->pc_cw; la.leaves[0] = ctx->pc_tree + (1u << (n - 2)); la.N[0] = 1u << (n - 6); la.n = 1;
    for (int i = 0; i < reps; ++i) VPCHK(pc_hash_leaves(ctx, la, false));
    return check_stream(ctx);
}
#endif

int vp_test_fft(vp_ctx *ctx, const vp_F *coefs, int coef_len, int order, int inverse, vp_F *out) {
    if (!ctx || !coefs || !out || coef_len < 1 || (coef_len & (coef_len - 1))) return VP_EINVAL;
    if (order != coef_len && order != 32 * coef_len) return VP_EINVAL;
    if (inverse && order != coef_len) return VP_EINVAL;
    int ln = 0; while ((1 << ln) < coef_len) ++ln;
    if (ln > PC_MAX_LN_LONG) return VP_ELIMIT;
    int lo = 0; while ((1 << lo) < order) ++lo;
    VP_ENTER(ctx);
    // private root table of order max(order, 2)
    const int lm = std::max(lo, 1);
    F *save_rt = ctx->pc_rt; int save_lm = ctx->pc_lm;
    ctx->pc_rt = nullptr; ctx->pc_lm = -1;
    int rc = pc_root_table(ctx, lm);
    F *din = nullptr, *dcw = nullptr;
    const u32 cosets = (u32) (order / coef_len);
    if (rc == VP_OK && hipMalloc((void **) &din, sizeof(F) * coef_len) != hipSuccess) rc = VP_EHIP;
    if (rc == VP_OK && hipMalloc((void **) &dcw, sizeof(F) * order) != hipSuccess) rc = VP_EHIP;
    if (rc == VP_OK && hipMemcpy(din, coefs, sizeof(F) * coef_len, hipMemcpyHostToDevice) != hipSuccess) rc = VP_EHIP;
    std::vector<F> tmp(order);
    if (rc == VP_OK) {
        pc_launch_ntt(ctx, din, dcw, ln, lm, inverse, 1, inverse ? 1 : cosets, coef_len);
        rc = check_stream(ctx);
    }
    if (rc == VP_OK && hipMemcpy(tmp.data(), dcw, sizeof(F) * order, hipMemcpyDeviceToHost) != hipSuccess) rc = VP_EHIP;
    if (rc == VP_OK) {                                    // coset-major -> natural order
        F *o = reinterpret_cast<F *>(out);
        for (u32 b = 0; b < cosets; ++b) for (int a = 0; a < coef_len; ++a) o[(size_t) a * cosets + b] = tmp[(size_t) b * coef_len + a];
        if (inverse) for (int a = 0; a < coef_len; ++a) o[a] = tmp[a];
    }
    if (din) (void) hipFree(din);
    if (dcw) (void) hipFree(dcw);
    ctx->pc_rt = save_rt; ctx->pc_lm = save_lm;           // the temporary table stays in ctx->allocs until the next upload
    return rc;
}

}  // extern "C"
