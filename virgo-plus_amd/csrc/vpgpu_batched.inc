// Part of vpgpu.hip (included at its end): the batched GKR drivers — per-sumcheck lanes, launch plan, hipGraph replay.
// =====================================================================================================
// Batched GKR, fused launches (default path of vp_prove_gkr; VP_GKR_PATH=simple selects the per-round one)
// =====================================================================================================
namespace {

constexpr int SF_BIG_LOG = 17;               // k_sumfold while some lock-step table has >= 2^17 entries
// plan-path parameters (vp_options): fuse the init into the first fold launch from 2^fuse_min_log entries on; rounds per fold launch; fold
// kernel from 2^sf_big_log entries on (14: measured best of 12..17)
// 0 = by circuit size: the largest one or two table sizes of the proof.  Measured (round 2, same-call sweeps, tools/sweep_fuse.sh): x64 (largest
// tables 2^20-2^21) 0.724 ms without fusion, 0.680 with 2^20, 0.690 with 2^21, 0.709 with 2^19; x256 2.00 / 1.947 at 2^22 / 1.965 at 2^21;
// x1024 6.81 / 6.76-6.79 at 2^22 / 6.80 at 2^21; x16: nothing to gain.
#define plan_fuse_min_log() (ctx->opt.fuse_min_log > 0 ? ctx->opt.fuse_min_log : std::min(22, std::max(20, ctx->max_bl - 1)))
#define plan_sf_big_log() (ctx->opt.sf_big_log)
// workgroups of a stand-alone inner-product job (V_u, Vres).  128 was sized for the x64 circuit; on a 2^26-entry layer each thread
// then walks ~1200 elements in one dependent chain (0.46 ms per job at x1024, on the critical path of the largest phase-2 chain)
#define plan_dot_blocks() ((u32) ctx->opt.dot_blocks)
constexpr int SF_MIN_LOG = 9;                // ... and every one of them keeps >= 2^9 after the launch

struct FusedSumcheck {
    int n_tab = 0, rounds = 0, has_a = 1, phase = 0;
    u32 off[VP_MAX_TAB], len0[VP_MAX_TAB], valid0[VP_MAX_TAB];
    const F *V0 = nullptr;                   // round-1 V source (phase 1 / Liu: circuitValue[i-1]; phase 2: tab[0][0])
    const unsigned long long *V0r = nullptr; // the same values as 8-byte reals when V0 is a layer of an all-real circuit (LayerDev::valr)
    const F *r = nullptr;                    // r[k-1] = challenge of round k
    F *poly_out = nullptr, *claims_out = nullptr;
    int exp[VP_MAX_TAB] = {};                // index-split proof: 1 + export slot of a table that is a slice (EmitTab::exp), 0 otherwise
    bool no_drop = false;                    // the rank's sums are partial: the closing kernel must not derive b from the previous claim — with the
                                             // five-product fold on (drop_y) the b of every round >= 2 is restored by split_finish from the ASSEMBLED
                                             // polynomials instead (derive_later), with it off every round computes its own b
};

inline int ilog2(u32 x) { int b = 0; while ((1u << (b + 1)) <= x) ++b; return b; }

// Launch sequence of ONE sumcheck.  Lock-step set = tables that still have more than 2^e entries at round k.
//   throughput regime (some table >= 2^17): the fold kernel (three rounds per launch; k_sumfold3b, its init-generating
//       variant for the first launch of a large phase-1 / Liu sumcheck) on the tables with at
//       least one chunk of entries, and one k_seg launch that finishes the shorter ones (own partial region, same rounds);
//   latency regime: k_seg on the whole set, ten rounds per launch;
//   k_emit closes the sumcheck.
// In record mode (ctx->rec) nothing is launched: the launches are appended to the current chain of the plan.
int run_sumcheck_seg(vp_ctx *ctx, const FusedSumcheck &sc) {
    const int e = sc.n_tab * 64 <= VP_EMIT_CAP ? 6 : sc.n_tab * 32 <= VP_EMIT_CAP ? 5 : 4;
    const u32 E = 1u << e;
    EmitArgs ea{};
    ea.V0 = sc.V0;
    for (int b = 0; b < 2; ++b) for (int t = 0; t < 3; ++t) ea.buf[b][t] = ctx->ln->tab[b][t];
    ea.r = sc.r; ea.part = ctx->ln->part2; ea.part_stride = 0;
    ea.n_tab = sc.n_tab; ea.rounds = sc.rounds; ea.has_a = sc.has_a; ea.emit_log = e;
    ea.poly_out = sc.poly_out; ea.claims_out = sc.claims_out;
    ea.Vu = (sc.phase == 1 && !ctx->rec) ? ctx->ln->Vu : nullptr;      // plan path: V_u is k_dot_multi's
    u32 cur_len[VP_MAX_TAB], cur_valid[VP_MAX_TAB];
    for (int j = 0; j < sc.n_tab; ++j) {
        cur_len[j] = sc.len0[j]; cur_valid[j] = sc.valid0[j];
        EmitTab &t = ea.t[j];
        t.off = sc.off[j]; t.enter = 1; t.len_enter = sc.len0[j]; t.valid_enter = sc.valid0[j];
        t.src = 0; t.v_from_v0 = (sc.phase != 2) ? 1 : 0; t.bl = ilog2(sc.len0[j]);
        t.exp = sc.exp[j];
    }
    ea.exp_out = ctx->d_trs ? ctx->d_trs + ctx->n_tr : nullptr;
    u32 part_used = 0;
    auto new_part = [&](int k0, int nr, u32 nblk) -> F * {
        if (ea.n_pd >= VP_MAX_PD || (size_t) part_used + (size_t) nr * nblk * 3 > (size_t) 16 * MAX_BLOCKS * 3) return nullptr;
        auto &d = ea.pd[ea.n_pd++];
        d.k0 = k0; d.nr = nr; d.nblk = nblk; d.off = part_used;
        part_used += (u32) nr * nblk * 3;
        return ctx->ln->part2 + d.off;
    };
    // Tables that are small from the start (<= 2^e entries) are folded down to one entry by the FIRST k_seg launch of the
    // sumcheck (one segment each, side by side with everything else) instead of round by round in the closing launch, whose
    // rounds with pairs cost ~4 us each on the critical path of the whole proof; k_emit then only retires them.
    const bool seg_tiny = ctx->opt.seg_tiny != 0;
    int k = 1, launch = 0;
    for (;;) {
        int L[VP_MAX_TAB], nL = 0; u32 maxlen = 0;
        for (int j = 0; j < sc.n_tab; ++j)
            if (ea.t[j].enter == k && cur_len[j] > (k == 1 && seg_tiny ? 1u : E)) { L[nL++] = j; maxlen = std::max(maxlen, cur_len[j]); }
        if (!nL) break;
        const F *inV, *inM, *inA;
        if (launch == 0) { inV = sc.V0; inM = ctx->ln->tab[0][1]; inA = ctx->ln->tab[0][2]; }
        else { F **t = ctx->ln->tab[launch & 1]; inV = t[0]; inM = t[1]; inA = t[2]; }
        F **to = ctx->ln->tab[(launch + 1) & 1];
        const bool throughput = maxlen >= (1u << (ctx->rec ? plan_sf_big_log() : SF_BIG_LOG));
        if (!throughput && launch == 0 && ctx->rec && ctx->rec_gen.mode) { ctx->err = "internal: fused init without a fold launch"; return VP_EINVAL; }
        // ---- fold kernel on the long tables ----
        const int SFR = 3;                                   // rounds per fold launch
        const u32 SFC = 64u << SFR;                          // entries per chunk
        if (throughput) {
            SfArgs a{};
            a.inV = inV; a.inM = inM; a.inA = inA; a.outV = to[0]; a.outM = to[1]; a.outA = to[2];
            a.inVr = (launch == 0 && k == 1 && ctx->vreal == 1) ? sc.V0r : nullptr;      // round 1 of phase 1 / Liu: the circuit values as 8-byte reals
            a.r = sc.r + (k - 1); a.has_a = sc.has_a;
            const bool drop_y = ctx->opt.drop_y != 0;
            const bool body3b = true;                                        // the block-cooperative fold kernels honour keep_y0
            const bool drop1 = ctx->rec && ctx->drop_round1;                    // round 1 too: its b comes from k_fixup
            a.keep_y0 = (!drop_y || !body3b) ? 3 : ((k == 1 && !drop1) ? 1 : 0);
            if (k == 1 && launch == 0 && ctx->vreal == 1) a.keep_y0 |= 4;            // V of this round = circuit values, all real: real-V pair step
            if (drop_y && body3b)
                for (int q = 0; q < SFR; ++q) if (k + q >= (drop1 ? 1 : 2) && k + q <= 32) ea.derive_mask |= 1u << (k + q - 1);
            ea.derive_later = (drop1 || sc.no_drop) ? 1 : 0;
            u32 chunks = 0; int nt = 0; u64 bytes = 0, out_bytes = 0, v_bytes = 0, pairs = 0;
            for (int q = 0; q < nL; ++q) {
                const int j = L[q];
                if (cur_len[j] < SFC) continue;
                SfTab &t = a.t[nt++];
                t.off = sc.off[j]; t.len = cur_len[j]; t.valid = cur_valid[j]; t.chunk_start = chunks;
                chunks += (cur_valid[j] + SFC - 1) / SFC;
                const u64 vout = (cur_valid[j] + (1u << SFR) - 1) >> SFR;
                bytes += (u64) (cur_valid[j] + vout) * (sc.has_a ? 48 : 32);
                out_bytes += vout * (sc.has_a ? 48 : 32); v_bytes += (u64) cur_valid[j] * 16;
                for (int q2 = 1; q2 <= SFR; ++q2) pairs += ((u64) cur_valid[j] + (1u << q2) - 1) >> q2;
            }
            a.n_tab = nt; a.total_chunks = chunks;
            const u32 sf3b_grid = (u32) ctx->opt.sf3b_grid;
            const u32 grid = std::max<u32>(1, std::min<u32>(chunks, std::min<u32>(sf3b_grid, MAX_BLOCKS)));
            a.part = new_part(k, SFR, grid); a.part_stride = grid * 3;
            if (!a.part) { ctx->err = "partial buffer exhausted"; return VP_ELIMIT; }
            const int sl = !ctx->rec ? prof_begin(ctx, ctx->ln->stream, VP_K_SF, grid, 1, bytes, pairs, (u32) SFR, (u32) k) : -1;
            if (ctx->rec && launch == 0 && ctx->rec_gen.mode) {
                // the init of this sumcheck runs inside its first fold launch (GenP1 / GenLiu): no mult/add tables at full length
                a.nblk = grid;
                SfGenJob gj = ctx->rec_gen; gj.sf = a;
                if (gj.mode == 1 && gj.dot_part) ctx->rec_dot.nblk = grid;
                // algorithmic bytes of the fused launch: the V table, the contribution lists with their operands (set where the
                // fusion was decided), the folded tables written — the mult/add tables are never read
                ctx->rec->sfgen.push_back(gj); ctx->rec->push(NK_SFGEN, (u32) ctx->rec->sfgen.size() - 1, grid, 0, v_bytes + ctx->rec_gen_bytes + out_bytes, pairs, k, SFR);
                ctx->rec_gen.mode = 0;
            } else if (ctx->rec) { a.nblk = grid; ctx->rec->sf.push_back(a); ctx->rec->push(NK_SF, (u32) ctx->rec->sf.size() - 1, grid, 0, bytes, pairs, k, SFR); }
            else if (sc.has_a) hipLaunchKernelGGL(k_sumfold3b<true>, dim3(grid), dim3(VP_BLOCK), 0, ctx->ln->stream, a);
            else hipLaunchKernelGGL(k_sumfold3b<false>, dim3(grid), dim3(VP_BLOCK), 0, ctx->ln->stream, a);
            prof_end(ctx, ctx->ln->stream, sl);
            count_launch(ctx);
        }
        // ---- k_seg on the rest (all of the set in the latency regime) ----
        SegArgs a{};
        a.inV = inV; a.inM = inM; a.inA = inA; a.outV = to[0]; a.outM = to[1]; a.outA = to[2];
        a.r = sc.r + (k - 1);
        int nt = 0, n_rounds = 0; u32 segs = 0; u64 seg_bytes = 0, seg_pairs = 0;
        int seg_j[VP_MAX_TAB];
        for (int q = 0; q < nL; ++q) {
            const int j = L[q];
            if (throughput && cur_len[j] >= SFC) continue;
            SegTab &t = a.t[nt];
            t.off = sc.off[j]; t.valid = cur_valid[j]; t.seg_start = segs;
            t.seg_log = std::min(VP_SEG_LOG, ilog2(cur_len[j]));
            segs += (cur_valid[j] + (1u << t.seg_log) - 1) >> t.seg_log;
            seg_bytes += ((u64) cur_valid[j] + ((cur_valid[j] + (1u << t.seg_log) - 1) >> t.seg_log)) * (sc.has_a ? 48 : 32);
            seg_pairs += cur_valid[j];
            n_rounds = std::max(n_rounds, t.seg_log);
            seg_j[nt++] = j;
        }
        if (nt) {
            a.total_segs = segs; a.n_tab = nt; a.n_rounds = n_rounds;
            const u32 grid = std::max<u32>(1, std::min<u32>(segs, 512));
            a.part = new_part(k, n_rounds, grid); a.part_stride = grid * 3;
            if (!a.part) { ctx->err = "partial buffer exhausted"; return VP_ELIMIT; }
            a.has_a = sc.has_a; a.nblk = grid;
            if (ctx->rec) { ctx->rec->seg.push_back(a); ctx->rec->push(NK_SEG, (u32) ctx->rec->seg.size() - 1, grid, 0, seg_bytes, seg_pairs, k, n_rounds); }
            else if (sc.has_a) hipLaunchKernelGGL(k_seg<true>, dim3(grid), dim3(VP_SEG_THREADS), 0, ctx->ln->stream, a);
            else hipLaunchKernelGGL(k_seg<false>, dim3(grid), dim3(VP_SEG_THREADS), 0, ctx->ln->stream, a);
            count_launch(ctx);
        }
        // ---- advance ----
        int step = throughput ? SFR : n_rounds;
        for (int q = 0; q < nL; ++q) {
            const int j = L[q];
            const bool via_sf = throughput && cur_len[j] >= SFC;
            const int sl = via_sf ? SFR : std::min(VP_SEG_LOG, ilog2(cur_len[j]));
            cur_len[j] >>= sl;
            cur_valid[j] = (cur_valid[j] + (1u << sl) - 1) >> sl;
            EmitTab &t = ea.t[j];
            t.enter = k + sl; t.len_enter = cur_len[j]; t.valid_enter = cur_valid[j];
            t.src = (launch + 1) & 1; t.v_from_v0 = 0;
        }
        k += step; ++launch;
        if (!throughput && n_rounds < VP_SEG_LOG) break;               // every table of the set is finished
    }
    // rounds in which k_emit has table work: pairs while len >= 2, the retire / claim round when len == 1
    for (int j = 0; j < sc.n_tab; ++j) {
        const EmitTab &t = ea.t[j];
        const int last = t.enter + ilog2(std::max<u32>(1, t.len_enter));
        for (int kk = t.enter; kk <= last && kk <= std::max(sc.rounds, 1); ++kk) {
            ea.work_mask |= 1u << (kk - 1);
            const int sh = kk - t.enter;
            if (kk <= sc.rounds && (sh < 32 ? (t.len_enter >> sh) : 0u) >= 2) ea.pair_mask |= 1u << (kk - 1);
        }
        if (t.enter <= std::max(sc.rounds, 1)) ea.enter_mask |= 1u << (t.enter - 1);
    }
    const size_t lds = ((size_t) 6 * sc.n_tab * E + VP_EMIT_LDS_EXTRA_F) * sizeof(F) + VP_MAX_TAB * sizeof(int);
    if (ctx->rec) {
        u64 eb = 0, ew = 0; int emin = std::max(sc.rounds, 1);
        for (int j = 0; j < sc.n_tab; ++j) { eb += (u64) ea.t[j].valid_enter * (sc.has_a ? 48 : 32); ew += ea.t[j].valid_enter; emin = std::min(emin, ea.t[j].enter); }
        for (int d = 0; d < ea.n_pd; ++d) eb += (u64) ea.pd[d].nr * ea.pd[d].nblk * 48;        // block partials of the earlier launches
        ctx->rec->emit.push_back(ea); ctx->rec->push(NK_EMIT, (u32) ctx->rec->emit.size() - 1, 1, (u32) lds, eb, ew, emin, std::max(0, sc.rounds - emin + 1));
        ctx->rec->chains[ctx->rec->cur].back().rounds = sc.rounds;
    }
    else hipLaunchKernelGGL(k_emit, dim3(1), dim3(VP_EMIT_THREADS), lds, ctx->ln->stream, ea);
    count_launch(ctx);
    ctx->st.rounds += sc.rounds;
    return VP_OK;
}

template <int PHASE>
int run_init2_rows(vp_ctx *ctx, const Csr &c, InitArgs2 &a) {
    a.rowptr = c.rowptr; a.e_g = c.e_g; a.e_x = c.e_x; a.e_tl = c.e_tl; a.n_rows = c.n_rows;
    if (ctx->rec) {
        PlanRec &R = *ctx->rec;
        if (PHASE == 2 && ctx->rec_gen.mode == 3) {      // fused phase 2 (GenP2): the caller adds light-row jobs for the subsets shorter than a chunk
            ctx->rec_gen.a = a;
        } else
        if (PHASE == 1 && ctx->rec_gen.mode == 1) {      // fused: only the heavy rows are summed ahead of the fold launch
            ctx->rec_gen_bytes = 26 * (u64) (c.n_entries - c.n_heavy_entries) + 4 * (u64) c.n_rows + 32 * (u64) c.n_heavy;
            ctx->rec_gen_work = c.n_entries - c.n_heavy_entries;
            ctx->rec_gen.a = a;
            ctx->rec_gen.a.rowptr = c.rowptr; ctx->rec_gen.a.e_g = c.e_g; ctx->rec_gen.a.e_x = c.e_x; ctx->rec_gen.a.e_tl = c.e_tl; ctx->rec_gen.a.n_rows = c.n_rows;
        } else if (c.n_rows) {
            LightJob j{}; j.a = a; j.phase = PHASE;
            u32 rows = c.n_rows;
            if (PHASE == 1 && ctx->rec_dot.part) {              // the launch covers every wire of the layer, not only the rows with contributions
                rows = std::max<u32>(rows, ctx->rec_dot.size);
                j.dot_h = ctx->rec_dot.h; j.dot_val = ctx->rec_dot.val; j.dot_part = ctx->rec_dot.part; j.dot_size = ctx->rec_dot.size;
                ctx->rec_dot.nblk = nblk(rows);
            }
            // Algorithmic bytes, stricter than SURVEY.md §8d (which prices a contribution at 48 B): the 10-byte record (gate, operand index,
            // type/layer) + the 16 B gathered operand — the eq value is the product of two half-table entries that live in L2, not HBM
            // traffic; per row its pointer and the mult/add entries written (phase 2 also gathers and writes V through the slot map);
            // + the V read of a riding inner product
            const u64 light = c.n_entries - c.n_heavy_entries;
            u64 by = 26 * light + (u64) c.n_rows * (4 + 32 + (PHASE == 2 ? 37 : 0));
            if (j.dot_part) by += 16 * (u64) j.dot_size;
            R.light.push_back(j); R.push(NK_LIGHT, (u32) R.light.size() - 1, nblk(rows), 0, by, light);
        }
        if (c.n_chunks) {
            ChunkJob j{}; j.a = a; j.chunk_beg = c.chunk_beg; j.chunk_end = c.chunk_end; j.part = ctx->ln->chunk_part; j.n_chunks = c.n_chunks; j.phase = PHASE;
            if (ctx->opt.fuse_combine) {
                j.fused = 1; j.fuse = ChunkFuse{c.chunk_h, c.heavy_row, c.heavy_cptr, c.heavy_cnt, a.M, a.A};
                R.chunks.push_back(j); R.push(NK_CHUNKS, (u32) R.chunks.size() - 1, (c.n_chunks + 3) / 4, 0, 26 * (u64) c.n_heavy_entries + 40 * (u64) c.n_heavy, c.n_heavy_entries);
                if (ctx->opt.fuse_combine == 2) R.chains[R.cur].push_back(PStep{-1, 0, 0, 0, 0, 0, -1});      // keep the step the combine node had: the alignment of the chains decides which launches share a node
                return VP_OK;
            }
            R.chunks.push_back(j); R.push(NK_CHUNKS, (u32) R.chunks.size() - 1, (c.n_chunks + 3) / 4, 0, 26 * (u64) c.n_heavy_entries + 40 * (u64) c.n_chunks, c.n_heavy_entries);
            CombineJob q{}; q.heavy_row = c.heavy_row; q.heavy_cptr = c.heavy_cptr; q.part = ctx->ln->chunk_part; q.M = a.M; q.A = a.A; q.n_heavy = c.n_heavy;
            R.combine.push_back(q); R.push(NK_COMBINE, (u32) R.combine.size() - 1, (c.n_heavy + 3) / 4, 0, 32 * (u64) c.n_chunks + 40 * (u64) c.n_heavy, c.n_chunks);
        }
        return VP_OK;
    }
    if (c.n_rows) {
        hipLaunchKernelGGL(k_init2_light<PHASE>, dim3(nblk(c.n_rows)), dim3(VP_BLOCK), 0, ctx->ln->stream, a);
        count_launch(ctx);
    }
    if (c.n_chunks) {
        hipLaunchKernelGGL(k_init2_chunks<PHASE>, dim3((c.n_chunks + 3) / 4), dim3(VP_BLOCK), 0, ctx->ln->stream, a,
                           c.chunk_beg, c.chunk_end, c.n_chunks, ctx->ln->chunk_part);
        hipLaunchKernelGGL(k_init_combine, dim3((c.n_heavy + 3) / 4), dim3(VP_BLOCK), 0, ctx->ln->stream, c.heavy_row,
                           c.heavy_cptr, c.n_heavy, ctx->ln->chunk_part, a.M, a.A);
        count_launch(ctx); count_launch(ctx);
    }
    return VP_OK;
}

// ---- the interactive entry points' inits through the kernels above (round 4) ----------------------------------------------------------------
// The per-sumcheck init kernels of round 1 (k_beta_half + k_beta_expand + k_init_light / k_liu_first + k_liu_scatter / k_p2_gather_v) cost 6.4 ms of
// a x1024 interactive proof (rocprofv3, profiles/r04_kernel_stats_interactive_b1024.csv) where the batched plan spends ~3.5 ms on the same work.
// Challenges are already staged in the tape slots the batched kernels read (vp_phase*_init -> stage()).
static int half_tables_of(vp_ctx *ctx, int first_job, int n_jobs) {
    hipLaunchKernelGGL(k_beta_half_direct, dim3((u32) n_jobs * ctx->beta_bpj), dim3(VP_BLOCK), 0, ctx->stream, ctx->all_jobs + first_job, ctx->beta_bpj);
    count_launch(ctx);
    return VP_OK;
}
int do_phase1_init_fast(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
    VPCHK(half_tables_of(ctx, cur.job_hg, 1));
    InitArgs2 a{};
    a.hg = cur.hg; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
    a.M = ctx->tab[0][1]; a.A = ctx->tab[0][2]; a.vreal = ctx->vreal;
    Lane *keep = ctx->ln; ctx->ln = &ctx->lane0;
    const int rc = run_init2_rows<1>(ctx, cur.c1, a);
    ctx->ln = keep;
    VPCHK(rc);
    SumcheckState &s = ctx->sc;
    s.phase = 1; s.layer = i; s.n_tab = 1; s.round = 0; s.total_rounds = pre.bl; s.has_a = 1;
    s.off[0] = 0; s.len0[0] = 1u << pre.bl; s.valid0[0] = (u32) pre.size; s.bl[0] = pre.bl;
    s.V0 = pre.val; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];
    return VP_OK;
}
int do_phase2_init_fast(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i];
    VPCHK(half_tables_of(ctx, cur.job_hu, 1));
    hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(64), 0, ctx->stream, ctx->add_term(), 1u);
    count_launch(ctx);
    InitArgs2 a{};
    a.hg = cur.hg; a.hu = cur.hu; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
    a.Vu = ctx->Vu();
    a.V = ctx->tab[0][0]; a.M = ctx->tab[0][1]; a.A = ctx->tab[0][2];
    a.s_layer = cur.s_layer; a.s_idx = cur.s_idx; a.vreal = ctx->vreal;
    Lane *keep = ctx->ln; ctx->ln = &ctx->lane0;
    const int rc = run_init2_rows<2>(ctx, cur.c2, a);
    ctx->ln = keep;
    VPCHK(rc);
    SumcheckState &s = ctx->sc;
    s.phase = 2; s.layer = i; s.n_tab = i; s.round = 0; s.total_rounds = cur.max_dad_bl; s.has_a = 1;
    for (int j = 0; j < i; ++j) {
        s.off[j] = cur.t_off[j]; s.len0[j] = cur.t_len[j];
        s.valid0[j] = (u32) cur.dad_size[j];
        s.bl[j] = cur.dad_size[j] ? cur.dad_bl[j] : 0;
    }
    s.V0 = ctx->tab[0][0]; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];
    return VP_OK;
}
int do_liu_init_fast(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
    VPCHK(half_tables_of(ctx, cur.job_liu0, cur.job_liun));
    hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(64), 0, ctx->stream, ctx->add_term(), 1u);
    hipLaunchKernelGGL(k_liu_gather, dim3(nblk(pre.size)), dim3(VP_BLOCK), 0, ctx->stream, cur.lrow, cur.l_q, cur.l_g, cur.liu_H, (u32) pre.size, ctx->tab[0][1]);
    count_launch(ctx); count_launch(ctx);
    SumcheckState &s = ctx->sc;
    s.phase = 3; s.layer = i; s.n_tab = 1; s.round = 0; s.total_rounds = pre.bl; s.has_a = 0;
    s.off[0] = 0; s.len0[0] = 1u << pre.bl; s.valid0[0] = (u32) pre.size; s.bl[0] = pre.bl;
    s.V0 = pre.val; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];
    return VP_OK;
}

// ---- round-sharded inits (vp_set_round_shard): the rows of this rank's slices, and the tables built whole on every rank ----------------------------
// Rows [r0, r0 + cnt) of a target-sorted list by direct launches: the light rows on shifted pointers (phase 2: the V gather of those slots only),
// the heavy rows of the range by their share of the chunk list and its combine — the direct-launch form of init_range / light_range above.
template <int PHASE>
int init2_rows_at(vp_ctx *ctx, const Csr &c, InitArgs2 a, u32 r0, u32 cnt) {
    if (!cnt) return VP_OK;
    a.rowptr = c.rowptr; a.e_g = c.e_g; a.e_x = c.e_x; a.e_tl = c.e_tl; a.n_rows = c.n_rows;
    InitArgs2 l = a;
    l.rowptr = c.rowptr + r0; l.n_rows = cnt; l.M = a.M + r0; l.A = a.A + r0;
    if (PHASE == 2) { l.V = a.V + r0; l.s_layer = a.s_layer + r0; l.s_idx = a.s_idx + r0; }
    hipLaunchKernelGGL(k_init2_light<PHASE>, dim3(nblk(cnt)), dim3(VP_BLOCK), 0, ctx->stream, l);
    count_launch(ctx);
    const auto &hr = c.h_heavy_row;
    const u32 h0 = (u32) (std::lower_bound(hr.begin(), hr.end(), r0) - hr.begin()), h1 = (u32) (std::lower_bound(hr.begin(), hr.end(), r0 + cnt) - hr.begin());
    if (h1 > h0) {
        const u32 c0 = c.h_heavy_cptr[h0], c1 = c.h_heavy_cptr[h1];
        hipLaunchKernelGGL(k_init2_chunks<PHASE>, dim3((c1 - c0 + 3) / 4), dim3(VP_BLOCK), 0, ctx->stream, a, c.chunk_beg + c0, c.chunk_end + c0, c1 - c0,
                           ctx->lane0.chunk_part + 2 * (size_t) c0);
        hipLaunchKernelGGL(k_init_combine, dim3((h1 - h0 + 3) / 4), dim3(VP_BLOCK), 0, ctx->stream, c.heavy_row + h0, c.heavy_cptr + h0, h1 - h0,
                           ctx->lane0.chunk_part, a.M, a.A);
        count_launch(ctx); count_launch(ctx);
    }
    return VP_OK;
}
int do_phase1_init_rs(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
    SumcheckState &s = ctx->sc;
    s.phase = 1; s.layer = i; s.n_tab = 1; s.round = 0; s.total_rounds = pre.bl; s.has_a = 1;
    s.off[0] = 0; s.len0[0] = 1u << pre.bl; s.valid0[0] = (u32) pre.size; s.bl[0] = pre.bl;
    unsigned long long split = 0;
    VPCHK(rs_split(ctx, &split));
    if (!split) return do_phase1_init_fast(ctx, i);                 // not split: the ordinary init, on every rank
    VPCHK(half_tables_of(ctx, cur.job_hg, 1));
    InitArgs2 a{};
    a.hg = cur.hg; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
    a.M = ctx->tab[0][1]; a.A = ctx->tab[0][2]; a.vreal = ctx->vreal;
    VPCHK(init2_rows_at<1>(ctx, cur.c1, a, s.off[0], s.valid0[0]));
    s.V0 = pre.val; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];       // the slice's entries sit at its global offset (s.off[0])
    return VP_OK;
}
int do_phase2_init_rs(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i];
    SumcheckState &s = ctx->sc;
    s.phase = 2; s.layer = i; s.n_tab = i; s.round = 0; s.total_rounds = cur.max_dad_bl; s.has_a = 1;
    for (int j = 0; j < i; ++j) {
        s.off[j] = cur.t_off[j]; s.len0[j] = cur.t_len[j];
        s.valid0[j] = (u32) cur.dad_size[j];
        s.bl[j] = cur.dad_size[j] ? cur.dad_bl[j] : 0;
    }
    unsigned long long split = 0;
    VPCHK(rs_split(ctx, &split));
    if (!split) return do_phase2_init_fast(ctx, i);
    VPCHK(half_tables_of(ctx, cur.job_hu, 1));
    hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(64), 0, ctx->stream, ctx->add_term(), 1u);
    count_launch(ctx);
    InitArgs2 a{};
    a.hg = cur.hg; a.hu = cur.hu; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
    a.Vu = ctx->Vu();
    a.V = ctx->tab[0][0]; a.M = ctx->tab[0][1]; a.A = ctx->tab[0][2];
    a.s_layer = cur.s_layer; a.s_idx = cur.s_idx; a.vreal = ctx->vreal;
    // split tables: the slots of this rank's slice; the other tables whole.  Every slot of the range is written, padding included, as the
    // unsharded init does: a table of ONE entry is retired into add_term at round 1 whatever its valid count (round_final_tail)
    // Ranges that meet (whole tables side by side, a slice that ends where the next table begins) go out as one range: a few launches per init.
    u32 r0 = 0, cnt = 0;
    for (int j = 0; j < i; ++j) {
        const u32 b = std::min<u32>(s.off[j], cur.c2.n_rows), n = std::min<u32>(s.len0[j], cur.c2.n_rows - b);
        if (!n) continue;
        if (cnt && b == r0 + cnt) { cnt += n; continue; }
        VPCHK(init2_rows_at<2>(ctx, cur.c2, a, r0, cnt));
        r0 = b; cnt = n;
    }
    VPCHK(init2_rows_at<2>(ctx, cur.c2, a, r0, cnt));
    s.V0 = ctx->tab[0][0]; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];
    return VP_OK;
}
int do_liu_init_rs(vp_ctx *ctx, int i) {
    LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
    SumcheckState &s = ctx->sc;
    s.phase = 3; s.layer = i; s.n_tab = 1; s.round = 0; s.total_rounds = pre.bl; s.has_a = 0;
    s.off[0] = 0; s.len0[0] = 1u << pre.bl; s.valid0[0] = (u32) pre.size; s.bl[0] = pre.bl;
    unsigned long long split = 0;
    VPCHK(rs_split(ctx, &split));
    if (!split) return do_liu_init_fast(ctx, i);
    VPCHK(half_tables_of(ctx, cur.job_liu0, cur.job_liun));
    hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(64), 0, ctx->stream, ctx->add_term(), 1u);
    count_launch(ctx);
    const u32 u0 = s.off[0], n = s.valid0[0];
    if (n) {
        hipLaunchKernelGGL(k_liu_gather_at, dim3(nblk(n)), dim3(VP_BLOCK), 0, ctx->stream, cur.lrow + u0, cur.l_q, cur.l_g, cur.liu_H, n, ctx->tab[0][1] + u0, u0);
        count_launch(ctx);
    }
    s.V0 = pre.val; s.M0 = ctx->tab[0][1]; s.A0 = ctx->tab[0][2];
    return VP_OK;
}

}  // namespace

extern "C" {

// Every launch of the GKR part (all lanes, fork and join included), in submission order.  No host synchronisation and no
// host-dependent argument in here: the same sequence is what the hipGraph of the proof captures.
static int submit_gkr(vp_ctx *ctx, bool serial) {
    const int n = ctx->n_layers;
    // Given the tape, every sumcheck of the proof is independent of the others except phase 1 -> phase 2 of the
    // same layer (V_u).  Layer i's phases 1+2 and its Liu sumcheck each get their own lane (stream + scratch);
    // profiling and VP_GKR_SERIAL=1 run everything on the main lane instead.
    Lane *main_lane = &ctx->lane0;
    ctx->ln = main_lane;
    F *tr = ctx->tr_base();
    // every eq half table of the proof in one launch (they depend on the tape only)
    if (!ctx->rec) {
        hipLaunchKernelGGL(k_beta_half_multi, dim3(ctx->n_all_jobs), dim3(VP_BLOCK), 0, ctx->stream, ctx->all_jobs);
        count_launch(ctx);
        // Vres (verifier.cpp:151): eq(r_0, .) is layer n-1's phase-1 table
        LayerDev &T = ctx->L[n - 1];
        hipLaunchKernelGGL(k_vres2, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, T.hg, T.val, (u32) T.size, tr);
        count_launch(ctx);
    }
    if (!serial && !ctx->rec) {
        HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
        for (int q = 0; q < 2 * (n - 1); ++q) HIPCHK(hipStreamWaitEvent(ctx->lanes[q].stream, ctx->ev_fork, 0));
    }
    // transcript positions (top layer first, as the verifier consumes them)
    std::vector<u64> pos_p1(n), pos_p2(n), pos_liu(n);
    u64 pos = 1;
    for (int i = n - 1; i >= 1; --i) {
        const u64 pbl = ctx->L[i - 1].bl;
        pos_p1[i] = pos; pos += 3 * pbl + 1;
        pos_p2[i] = pos; if (ctx->L[i].max_dad_bl != -1) pos += 3 * (u64) ctx->L[i].max_dad_bl + i;
        pos_liu[i] = pos; pos += 3 * pbl + 1;
    }
    if (pos != ctx->n_tr) { ctx->err = "internal: transcript size"; return VP_EINVAL; }
    // submit the largest layers first so that the long chains start early
    std::vector<int> order;
    for (int i = 1; i < n; ++i) order.push_back(i);
    if (!serial) std::sort(order.begin(), order.end(), [&](int x, int y) { return ctx->L[x - 1].size + ctx->L[x].size > ctx->L[y - 1].size + ctx->L[y].size; });
    else std::reverse(order.begin(), order.end());
    for (int i : order) {
        LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
        const int pbl = pre.bl;
        const int n_lanes_ = 2 * (n - 1);
        // index-split chains (split_layout): every rank below 2^lw runs its slice; the others skip the chain
        auto split_of = [&](int chain) -> const vp_ctx::SplitChain * {
            return (ctx->rec && ctx->split_lw > 0 && ctx->shard_world > 1 && chain < (int) ctx->split.size() && !ctx->split[chain].tabs.empty()) ? &ctx->split[chain] : nullptr;
        };
        const vp_ctx::SplitChain *sp_p1 = split_of(2 * (i - 1)), *sp_liu = split_of(2 * (i - 1) + 1), *sp_p2 = split_of(n_lanes_ + (i - 1));
        const bool in_split = ctx->shard_rank < (1 << ctx->split_lw);
        const bool own_p1 = !ctx->rec || (sp_p1 ? in_split : ctx->owned(2 * (i - 1))), own_liu = !ctx->rec || (sp_liu ? in_split : ctx->owned(2 * (i - 1) + 1)),
                   own_p2 = !ctx->rec || (sp_p2 ? in_split : ctx->owned(n_lanes_ + (i - 1)));
        // the local view of a split chain's tables on this rank: slice `rank` of the split tables, the short tables whole on one rank, empty elsewhere
        auto local_tables = [&](const vp_ctx::SplitChain &sp, FusedSumcheck &sc) {
            const int lw = ctx->split_lw;
            // slice of this rank: rotated from chain to chain — layer sizes are not powers of two, the upper slices of a padded table are
            // short or empty, and they should not all land on the same ranks
            const u32 s_ = (u32) ((ctx->shard_rank + sp.small_owner) & ((1 << lw) - 1));
            sc.no_drop = true;
            for (int j = 0; j < sc.n_tab; ++j) {
                const vp_ctx::SplitTab *st = nullptr;
                for (const auto &t : sp.tabs) if (t.j == j) st = &t;
                if (st) {
                    const u32 S = sc.len0[j] >> lw, lo = s_ * S;
                    sc.off[j] += lo; sc.len0[j] = S;
                    sc.valid0[j] = sc.valid0[j] > lo ? std::min<u32>(S, sc.valid0[j] - lo) : 0u;
                    sc.exp[j] = (int) (st->slot0 + s_) + 1;
                } else if (s_ != 0) { sc.len0[j] = 1; sc.valid0[j] = 0; }      // the short tables ride with slice 0; elsewhere an all-zero single entry
            }
        };
        // row-range init jobs (rows [r0, r0 + cnt) of a target-sorted list): the light rows by a job on shifted pointers, the heavy rows of the range
        // by the chunk / combine jobs of their share of the chunk list
        auto light_range = [&](int PHASE, const Csr &c, InitArgs2 a, u32 r0, u32 cnt) {      // the light rows of [r0, r0 + cnt): a job on shifted pointers
            if (!cnt) return;
            PlanRec &R = *ctx->rec;
            a.rowptr = c.rowptr; a.e_g = c.e_g; a.e_x = c.e_x; a.e_tl = c.e_tl; a.n_rows = c.n_rows;
            LightJob j{}; j.a = a; j.phase = PHASE;
            j.a.rowptr = c.rowptr + r0; j.a.n_rows = cnt; j.a.M = a.M + r0; j.a.A = a.A + r0;
            if (PHASE == 2) { j.a.V = a.V + r0; j.a.s_layer = a.s_layer + r0; j.a.s_idx = a.s_idx + r0; }
            const u64 light = (u64) ((double) (c.n_entries - c.n_heavy_entries) * cnt / std::max<u32>(1, c.n_rows));
            R.light.push_back(j); R.push(NK_LIGHT, (u32) R.light.size() - 1, nblk(cnt), 0, 26 * light + (u64) cnt * (4 + 32 + (PHASE == 2 ? 37 : 0)), light);
        };
        auto init_range = [&](int PHASE, const Csr &c, InitArgs2 a, u32 r0, u32 cnt) {
            if (!cnt) return;
            PlanRec &R = *ctx->rec;
            light_range(PHASE, c, a, r0, cnt);
            a.rowptr = c.rowptr; a.e_g = c.e_g; a.e_x = c.e_x; a.e_tl = c.e_tl; a.n_rows = c.n_rows;
            const auto &hr = c.h_heavy_row;
            const u32 h0 = (u32) (std::lower_bound(hr.begin(), hr.end(), r0) - hr.begin()), h1 = (u32) (std::lower_bound(hr.begin(), hr.end(), r0 + cnt) - hr.begin());
            if (h1 > h0) {
                const u32 c0 = c.h_heavy_cptr[h0], c1 = c.h_heavy_cptr[h1];
                ChunkJob q{}; q.a = a; q.chunk_beg = c.chunk_beg + c0; q.chunk_end = c.chunk_end + c0; q.part = ctx->ln->chunk_part + 2 * (size_t) c0; q.n_chunks = c1 - c0; q.phase = PHASE;
                R.chunks.push_back(q); R.push(NK_CHUNKS, (u32) R.chunks.size() - 1, (q.n_chunks + 3) / 4, 0, 40 * (u64) q.n_chunks, q.n_chunks);
                CombineJob cj{}; cj.heavy_row = c.heavy_row + h0; cj.heavy_cptr = c.heavy_cptr + h0; cj.part = ctx->ln->chunk_part; cj.M = a.M; cj.A = a.A; cj.n_heavy = h1 - h0;
                R.combine.push_back(cj); R.push(NK_COMBINE, (u32) R.combine.size() - 1, (cj.n_heavy + 3) / 4, 0, 32 * (u64) q.n_chunks + 40 * (u64) cj.n_heavy, q.n_chunks);
            }
        };
        // ---- Liu (independent of phases 1 and 2) ----
        if (own_liu && sp_liu) {
            ctx->ln = &ctx->lanes[2 * (i - 1) + 1];
            ctx->rec->cur = 2 * (i - 1) + 1;
            ctx->rec_gen = SfGenJob{};
            FusedSumcheck sc;
            sc.n_tab = 1; sc.rounds = pbl; sc.has_a = 0; sc.phase = 3;
            sc.off[0] = 0; sc.len0[0] = 1u << pbl; sc.valid0[0] = (u32) pre.size;
            local_tables(*sp_liu, sc);
            if (sc.valid0[0]) {                                  // the Liu mult entries of the slice's wires
                LightJob j{}; j.phase = 0;
                j.g.rowptr = cur.lrow + sc.off[0]; j.g.e_q = cur.l_q; j.g.e_g = cur.l_g; j.g.H = cur.liu_H; j.g.M = ctx->ln->tab[0][1] + sc.off[0];
                j.g.size = sc.valid0[0]; j.g.u0 = sc.off[0];
                const u64 ent = (u64) ((double) cur.l_n * sc.valid0[0] / std::max<u64>(1, pre.size));
                ctx->rec->light.push_back(j); ctx->rec->push(NK_LIGHT, (u32) ctx->rec->light.size() - 1, nblk(sc.valid0[0]), 0, 5 * ent + (u64) sc.valid0[0] * (4 + 16), ent);
            }
            sc.V0 = pre.val; sc.V0r = ctx->vreal ? pre.valr : nullptr; sc.r = ctx->d_tape + ctx->rliu_off[i];
            sc.poly_out = tr + pos_liu[i]; sc.claims_out = tr + pos_liu[i] + 3 * (u64) pbl;
            VPCHK(run_sumcheck_seg(ctx, sc));
        } else
        if (own_liu) {
            ctx->ln = serial ? main_lane : &ctx->lanes[2 * (i - 1) + 1];
            const bool fuse_big = ctx->rec && ctx->fuse_init && pbl >= std::max(plan_sf_big_log(), plan_fuse_min_log());      // throughput regime: the first launch is a fold
            ctx->rec_gen = SfGenJob{};
            if (fuse_big) {
                ctx->rec->cur = 2 * (i - 1) + 1;
                ctx->rec_gen.mode = 2;
                if (ctx->gen_rec_ok && (ctx->opt.gen_rec & 2) && cur.l_rec) {      // row records: the first list term's half-table entries by pool index, no descriptor load
                    GenRecArgs &gr = ctx->rec_gen.r;
                    gr.rec = cur.l_rec; gr.l_bf = cur.l_bf; gr.l_bs = cur.l_bs; gr.pool = ctx->half_pool; gr.pool_n = (u32) ctx->pool_n; gr.on = 1;
                }
                ctx->rec_gen.g.rowptr = cur.lrow; ctx->rec_gen.g.e_q = cur.l_q; ctx->rec_gen.g.e_g = cur.l_g; ctx->rec_gen.g.H = cur.liu_H;
                ctx->rec_gen.g.M = nullptr; ctx->rec_gen.g.size = (u32) pre.size;
                ctx->rec_gen_bytes = 5 * (u64) cur.l_n + 4 * (u64) pre.size; ctx->rec_gen_work = cur.l_n;      // 5-byte (subset, position) record per entry; the eq values come from L2-resident half tables
            } else if (ctx->rec) {
                ctx->rec->cur = 2 * (i - 1) + 1;
                LightJob j{}; j.phase = 0;
                j.g.rowptr = cur.lrow; j.g.e_q = cur.l_q; j.g.e_g = cur.l_g; j.g.H = cur.liu_H; j.g.M = ctx->ln->tab[0][1]; j.g.size = (u32) pre.size;
                ctx->rec->light.push_back(j); ctx->rec->push(NK_LIGHT, (u32) ctx->rec->light.size() - 1, nblk(pre.size), 0, 5 * (u64) cur.l_n + (u64) pre.size * (4 + 16), cur.l_n);
            } else
            hipLaunchKernelGGL(k_liu_gather, dim3(nblk(pre.size)), dim3(VP_BLOCK), 0, ctx->ln->stream, cur.lrow, cur.l_q,
                               cur.l_g, cur.liu_H, (u32) pre.size, ctx->ln->tab[0][1]);
            count_launch(ctx);
            FusedSumcheck sc;
            sc.n_tab = 1; sc.rounds = pbl; sc.has_a = 0; sc.phase = 3;
            sc.off[0] = 0; sc.len0[0] = 1u << pbl; sc.valid0[0] = (u32) pre.size;
            sc.V0 = pre.val; sc.V0r = ctx->vreal ? pre.valr : nullptr; sc.r = ctx->d_tape + ctx->rliu_off[i];
            sc.poly_out = tr + pos_liu[i]; sc.claims_out = tr + pos_liu[i] + 3 * (u64) pbl;
            VPCHK(run_sumcheck_seg(ctx, sc));
            if (ctx->rec && ctx->drop_round1) {      // claim: sig[0] * claim_u(i) + sum over later layers k with a subset in layer i-1 of sig[k-i+1] * claims_v[k][i-1]
                FixJob f{}; f.poly_pos = (u32) pos_liu[i]; f.rounds = (u32) pbl; f.derive_mask = ctx->rec->emit.back().derive_mask;
                f.r_off = (u32) ctx->rliu_off[i]; f.kind = 2;
                f.sig[0] = (u32) ctx->sig_off[i]; f.cl[0] = (u32) (pos_p1[i] + 3 * (u64) pbl); f.n_terms = 1;
                for (int k2 = i; k2 < n; ++k2) {
                    if (!ctx->L[k2].dad_size[i - 1]) continue;
                    f.sig[f.n_terms] = (u32) (ctx->sig_off[i] + (k2 - i + 1));
                    f.cl[f.n_terms] = (u32) (pos_p2[k2] + 3 * (u64) ctx->L[k2].max_dad_bl + (i - 1));
                    ++f.n_terms;
                }
                ctx->rec_fix.push_back(f);
            }
        }
        // ---- phase 1 ----
        ctx->ln = serial ? main_lane : &ctx->lanes[2 * (i - 1)];
        if (ctx->rec) ctx->rec->cur = 2 * (i - 1);
        size_t p1_fold_step = 0; bool p1_fused_dot = false;
        ctx->rec_dot = DotJob{};
        if (own_p1 && sp_p1) {
            InitArgs2 a{};
            a.hg = cur.hg; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
            a.M = ctx->ln->tab[0][1]; a.A = ctx->ln->tab[0][2]; a.vreal = ctx->vreal;
            ctx->rec_dot = DotJob{}; ctx->rec_gen = SfGenJob{};
            FusedSumcheck sc;
            sc.n_tab = 1; sc.rounds = pbl; sc.has_a = 1; sc.phase = 1;
            sc.off[0] = 0; sc.len0[0] = 1u << pbl; sc.valid0[0] = (u32) pre.size;
            local_tables(*sp_p1, sc);
            init_range(1, cur.c1, a, sc.off[0], sc.valid0[0]);
            sc.V0 = pre.val; sc.V0r = ctx->vreal ? pre.valr : nullptr; sc.r = ctx->d_tape + ctx->ru_off[i];
            sc.poly_out = tr + pos_p1[i]; sc.claims_out = tr + pos_p1[i] + 3 * (u64) pbl;
            VPCHK(run_sumcheck_seg(ctx, sc));
        } else
        if (own_p1) {
            InitArgs2 a{};
            a.hg = cur.hg; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
            a.M = ctx->ln->tab[0][1]; a.A = ctx->ln->tab[0][2]; a.vreal = ctx->vreal;
            ctx->rec_dot = DotJob{};
            ctx->rec_gen = SfGenJob{};
            const bool fuse_p1 = ctx->rec && ctx->fuse_init && pbl >= std::max(plan_sf_big_log(), plan_fuse_min_log());
            if (fuse_p1) ctx->rec_gen.mode = 1;
            if (fuse_p1 && ctx->gen_rec_ok && (ctx->opt.gen_rec & 1) && ctx->vreal && ctx->valr_arena && cur.c1.rec) {      // row records: operands by arena index (the arena holds real parts: all-real witnesses only)
                GenRecArgs &gr = ctx->rec_gen.r;
                gr.rec = cur.c1.rec; gr.e_xg = cur.c1.e_xg; gr.arena = ctx->valr_arena; gr.arena_n = (u32) ctx->arena_n; gr.on = 1;
            }
            // with the init fused into the first fold launch, V_u riding on it would hold phase 2 back until that launch ends:
            // phase 2 then takes V_u from the separate inner-product pass and starts at step 0 (VP_FUSE_DOT=1: ride anyway)
            const bool fuse_dot = ctx->opt.fuse_dot != 0;
            const bool vu_pre = sp_p2 && ctx->opt.split_vu;      // index-split phase 2: V_u is there before the graph starts (vu_pre_*)
            if (ctx->rec && own_p2 && !vu_pre && cur.max_dad_bl != -1 && cur.c1.n_rows && (!fuse_p1 || fuse_dot)) {      // sharded proof: V_u rides only when this rank runs both phases
                Lane &p2 = ctx->lanes[2 * (n - 1) + (i - 1)];
                ctx->rec_dot.h = cur.hu; ctx->rec_dot.val = pre.val; ctx->rec_dot.part = p2.dot_part;
                ctx->rec_dot.out = p2.Vu; ctx->rec_dot.size = (u32) pre.size; ctx->rec_dot.vreal = ctx->vreal;
            }
            if (fuse_p1 && ctx->rec_dot.part) { ctx->rec_gen.dot_h = ctx->rec_dot.h; ctx->rec_gen.dot_part = ctx->rec_dot.part; }
            VPCHK(run_init2_rows<1>(ctx, cur.c1, a));
            p1_fold_step = ctx->rec ? ctx->rec->chains[ctx->rec->cur].size() : 0;     // local index of the first fold launch
            p1_fused_dot = fuse_p1 && ctx->rec_dot.part;
            FusedSumcheck sc;
            sc.n_tab = 1; sc.rounds = pbl; sc.has_a = 1; sc.phase = 1;
            sc.off[0] = 0; sc.len0[0] = 1u << pbl; sc.valid0[0] = (u32) pre.size;
            sc.V0 = pre.val; sc.V0r = ctx->vreal ? pre.valr : nullptr; sc.r = ctx->d_tape + ctx->ru_off[i];
            sc.poly_out = tr + pos_p1[i]; sc.claims_out = tr + pos_p1[i] + 3 * (u64) pbl;
            VPCHK(run_sumcheck_seg(ctx, sc));
            if (ctx->rec && ctx->drop_round1) {      // claim: Vres for the top layer, vr of the layer above otherwise
                FixJob f{}; f.poly_pos = (u32) pos_p1[i]; f.rounds = (u32) pbl; f.derive_mask = ctx->rec->emit.back().derive_mask;
                f.r_off = (u32) ctx->ru_off[i]; f.kind = 0;
                f.ref0 = i == n - 1 ? 0u : (u32) (pos_liu[i + 1] + 3 * (u64) ctx->L[i].bl);
                ctx->rec_fix.push_back(f);
            }
        }
        // ---- phase 2 (same lane: needs V_u) ----
        const int mdb = cur.max_dad_bl;
        if (mdb != -1 && own_p2) {
            if (ctx->rec) {
                // own chain: V_u comes from an inner product instead of phase 1's last fold
                const int li = 2 * (n - 1) + (i - 1);
                ctx->ln = &ctx->lanes[li]; ctx->rec->cur = li;
                if (sp_p2 && ctx->opt.split_vu) {
                    // index-split chain: every rank has added up its share of the inner product and the shares have been exchanged before the
                    // graph starts (vu_pre_run) — no rank reads the whole layer for a V_u of its own
                } else if (ctx->rec_dot.part && ctx->rec_dot.nblk) {
                    // the phase-1 init launch of this layer left the block partials: wait for it (placeholder step), then combine
                    ctx->rec->dot.push_back(ctx->rec_dot);
                    // the partials come from the phase-1 init launch (step 0) or, when the init is fused, from its first fold launch
                    for (size_t q = 0; q < (p1_fused_dot ? p1_fold_step + 1 : 1); ++q) ctx->rec->chains[li].push_back(PStep{-1, 0, 0, 0, 0, 0, -1});
                    ctx->rec->push(NK_DOTFIN, (u32) ctx->rec->dot.size() - 1, 1);
                    ctx->rec->chains[li].back().xchain = 2 * (i - 1);
                } else {
                    DotJob d{}; d.h = cur.hu; d.val = pre.val; d.part = ctx->ln->part2; d.out = ctx->ln->Vu; d.size = (u32) pre.size; d.vreal = ctx->vreal;
                    d.valr = ctx->vreal ? pre.valr : nullptr;
                    d.nblk = std::max<u32>(1, std::min<u32>(nblk(pre.size), plan_dot_blocks()));
                    ctx->rec->dot.push_back(d);
                    ctx->rec->push(NK_DOT, (u32) ctx->rec->dot.size() - 1, d.nblk, 0, (d.valr ? 8 : 16) * (u64) d.size, d.size);
                    ctx->rec->push(NK_DOTFIN, (u32) ctx->rec->dot.size() - 1, 1, 0, 16 * (u64) d.nblk, d.nblk);
                }
            }
            InitArgs2 a{};
            a.hg = cur.hg; a.hu = cur.hu; a.vals = ctx->d_vals; a.valsr = ctx->vreal ? ctx->d_valsr : nullptr; a.vreal = ctx->vreal; a.gc = cur.gc; a.assert_r = ctx->d_tape + ctx->as_off[i];
            a.Vu = ctx->ln->Vu;
            a.V = ctx->ln->tab[0][0]; a.M = ctx->ln->tab[0][1]; a.A = ctx->ln->tab[0][2];
            a.s_layer = cur.s_layer; a.s_idx = cur.s_idx;
            FusedSumcheck sc;
            sc.n_tab = i; sc.rounds = mdb; sc.has_a = 1; sc.phase = 2;
            for (int j = 0; j < i; ++j) { sc.off[j] = cur.t_off[j]; sc.len0[j] = cur.t_len[j]; sc.valid0[j] = (u32) cur.dad_size[j]; }
            ctx->rec_gen = SfGenJob{};
            if (sp_p2) {
                local_tables(*sp_p2, sc);
                for (int j = 0; j < i; ++j) init_range(2, cur.c2, a, sc.off[j], sc.valid0[j]);     // the slots this rank folds, table by table
            } else {
                // Round 4: like phase 1, the init of the long subsets runs inside the sumcheck's first fold launch (GenP2) — their V / mult / add
                // tables are never written at full length.  A subset shorter than a fold chunk is folded from memory by k_seg / k_emit and
                // keeps its light-row job; the heavy rows are summed ahead by the chunk jobs either way.
                const u32 SFC0 = 512;
                const bool fuse_p2 = ctx->rec && ctx->fuse_init && ctx->opt.fuse_p2 && mdb >= std::max(plan_sf_big_log(), plan_fuse_min_log());
                if (fuse_p2) {
                    ctx->rec_gen.mode = 3;
                    if (ctx->gen_rec_ok && (ctx->opt.gen_rec & 1) && ctx->vreal && ctx->valr_arena && cur.c2.rec && cur.s_gidx) {
                        GenRecArgs &gr = ctx->rec_gen.r;
                        gr.rec = cur.c2.rec; gr.s_gidx = cur.s_gidx; gr.arena = ctx->valr_arena; gr.arena_n = (u32) ctx->arena_n; gr.on = 1;
                    }
                    u64 rows_big = 0;
                    for (int j = 0; j < i; ++j) if (cur.t_len[j] >= SFC0) rows_big += cur.dad_size[j];
                    const Csr &c = cur.c2;
                    const u64 light = (u64) ((double) (c.n_entries - c.n_heavy_entries) * rows_big / std::max<u32>(1, c.n_rows));
                    // records and their half-table operands (L2) as in the light launch; per slot its row pointer, its slot-map entry and the gathered V
                    ctx->rec_gen_bytes = 26 * light + rows_big * (4 + 5 + 16) + 32 * (u64) c.n_heavy; ctx->rec_gen_work = light;
                }
                VPCHK(run_init2_rows<2>(ctx, cur.c2, a));
                if (fuse_p2) {
                    InitArgs2 ar = a;
                    for (int j = 0; j < i; ++j) if (cur.t_len[j] < SFC0) light_range(2, cur.c2, ar, cur.t_off[j], (u32) cur.dad_size[j]);
                }
            }
            sc.V0 = ctx->ln->tab[0][0]; sc.r = ctx->d_tape + ctx->rv_off[i];
            sc.poly_out = tr + pos_p2[i]; sc.claims_out = tr + pos_p2[i] + 3 * (u64) mdb;
            VPCHK(run_sumcheck_seg(ctx, sc));
            if (ctx->rec && ctx->drop_round1) {      // claim: the last phase-1 polynomial at its last challenge (phase 1's own claim if it has no round)
                FixJob f{}; f.poly_pos = (u32) pos_p2[i]; f.rounds = (u32) mdb; f.derive_mask = ctx->rec->emit.back().derive_mask;
                f.r_off = (u32) ctx->rv_off[i];
                if (pbl > 0) { f.kind = 1; f.ref0 = (u32) (pos_p1[i] + 3 * (u64) (pbl - 1)); f.ref1 = (u32) (ctx->ru_off[i] + pbl - 1); }
                else { f.kind = 0; f.ref0 = i == n - 1 ? 0u : (u32) (pos_liu[i + 1] + 3 * (u64) ctx->L[i].bl); }
                ctx->rec_fix.push_back(f);
            }
        }
    }
    ctx->ln = main_lane;
    if (!serial && !ctx->rec) {
        for (int q = 0; q < 2 * (n - 1); ++q) {
            Lane &ln = ctx->lanes[q];
            HIPCHK(hipEventRecord(ln.done, ln.stream));
            HIPCHK(hipStreamWaitEvent(ctx->stream, ln.done, 0));
        }
    }
    return VP_OK;
}

// ---- index-split proof: the large tables of a chain cut into 2^lw slices, one rank each (vp_set_shard_split) ------------------------
// A fold pairs ADJACENT entries (src/prover.cpp:470-487), so rank s can fold slice s = entries [s S, (s+1) S) of a table of 2^bl entries
// through its first bl - lw rounds without seeing the rest, and the coefficient sums of those rounds are sums over the slices: they add up
// in the transcript all-reduce like the disjoint slices of the chain shard.  After bl - lw rounds a slice is one entry (v, m, a); the
// remaining lw rounds pair entries of DIFFERENT ranks: each rank exports its entry to its own slot of an area behind the transcript (zero
// elsewhere, so the same all-reduce gathers it), and split_finish() runs those rounds — 2^lw entries per table — on the host and adds
// their polynomials, claims and add_term contributions to the assembled transcript.  Tables too short to split stay whole on one of the
// participating ranks; ranks beyond 2^lw (a world size that is not a power of two) take whole chains only.
static void chain_costs(vp_ctx *ctx);
static void split_layout(vp_ctx *ctx) {
    const int n = ctx->n_layers, n_lanes = 2 * (n - 1), n_chains = (int) ctx->lanes.size() + 1;
    ctx->split.assign(n_chains, vp_ctx::SplitChain());
    ctx->n_exp = 0;
    if (ctx->split_lw <= 0 || ctx->shard_world <= 1) return;
    const int lw = ctx->split_lw, need = lw + ctx->split_min_log;
    // only the chains that one rank could not absorb are cut (cost above split_cost_percent of a rank's fair share): a split chain costs
    // EVERY rank its closing launches, no fused init and, for a phase 2, its own V_u inner product.  Measured, max over ranks of the per-rank device time (tools/shard_sweep*.sh, W shards on one GPU):
    //   SHA-256 x1024 (43 chains), W = 8: chain shard alone 1.64-1.72 ms; every chain with a long table cut 1.99 ms, the 11 most expensive 1.68 ms,
    //   the 6 above half a rank's fair share 1.46 ms (the default);  randomize(3, 23) (6 chains), W = 8: 0.76 -> 0.53 ms;
    //   randomize(2, 24) (3 chains), W = 4: 1.40 -> 0.83 ms.
    chain_costs(ctx);
    double total = 0;
    for (double c : ctx->chain_cost) total += c;
    const double cut = total / ctx->shard_world * (double) ctx->opt.split_cost_percent / 100.0;
    u64 pos = 1;
    u32 slot = 0;
    for (int i = n - 1; i >= 1; --i) {
        const LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
        const u64 pbl = pre.bl;
        const u64 pos_p1 = pos; pos += 3 * pbl + 1;
        const u64 pos_p2 = pos; if (cur.max_dad_bl != -1) pos += 3 * (u64) cur.max_dad_bl + i;
        const u64 pos_liu = pos; pos += 3 * pbl + 1;
        auto single = [&](int chain, u64 ppos, u64 r_off, int has_a) {
            vp_ctx::SplitChain &sp = ctx->split[chain];
            sp.poly_pos = ppos; sp.claims_pos = ppos + 3 * pbl; sp.r_off = r_off; sp.rounds = (int) pbl; sp.has_a = has_a; sp.n_tab = 1;
            sp.small_owner = chain & ((1 << lw) - 1);
            if ((int) pbl >= need && ctx->chain_cost[chain] > cut) { sp.tabs.push_back({0, (int) pbl, slot}); slot += 1u << lw; }
        };
        single(2 * (i - 1), pos_p1, ctx->ru_off[i], 1);
        single(2 * (i - 1) + 1, pos_liu, ctx->rliu_off[i], 0);
        if (cur.max_dad_bl != -1) {
            vp_ctx::SplitChain &sp = ctx->split[n_lanes + (i - 1)];
            sp.poly_pos = pos_p2; sp.claims_pos = pos_p2 + 3 * (u64) cur.max_dad_bl; sp.r_off = ctx->rv_off[i]; sp.rounds = cur.max_dad_bl; sp.has_a = 1; sp.n_tab = i;
            sp.small_owner = (n_lanes + (i - 1)) & ((1 << lw) - 1);
            if (ctx->chain_cost[n_lanes + (i - 1)] > cut)
                for (int j = 0; j < i; ++j)
                    if (cur.dad_size[j] && cur.dad_bl[j] >= need) { sp.tabs.push_back({j, cur.dad_bl[j], slot}); slot += 1u << lw; }
        }
    }
    ctx->n_exp = slot;
}

// The last lw rounds of every split table, on the host, from the entries the slices ended in (buf: n_tr transcript elements followed by
// 3 * n_exp exported ones, ALREADY summed over the ranks); adds the polynomials of those rounds, the claims and the add_term
// contributions of the rounds after a split table retires (src/prover.cpp:445,462-467) to the transcript part of buf.
static inline u64 host_fold(u64 s) { s = (s & P61) + (s >> 61); s = (s & P61) + (s >> 61); return s >= P61 ? s - P61 : s; }
static void split_finish(const vp_ctx *ctx, F *buf, const F *tape) {
    if (ctx->split_lw <= 0 || !ctx->n_exp) return;
    const int W = 1 << ctx->split_lw;
    const F *ex = buf + ctx->n_tr;
    for (const auto &sp : ctx->split) {
        if (sp.tabs.empty()) continue;
        const F *r = tape + sp.r_off;                                 // r[k-1] = challenge of round k
        std::vector<F> ret(sp.rounds + 2, f_zero());                  // ret[k]: sum of v m + a of the split tables that are down to one entry in round k
        for (const auto &t : sp.tabs) {
            std::vector<F> v(W), m(W), a(W);
            for (int w = 0; w < W; ++w) { const F *e = ex + 3 * (size_t) (t.slot0 + w); v[w] = e[0]; m[w] = e[1]; a[w] = e[2]; }
            int len = W;
            for (int k = t.bl - ctx->split_lw + 1; k <= t.bl; ++k) {   // round k on a table of `len` entries
                F c0 = f_zero(), c1 = f_zero(), c2 = f_zero();
                for (int p = 0; p < len / 2; ++p) {
                    const F dm = f_sub(m[2 * p + 1], m[2 * p]), dv = f_sub(v[2 * p + 1], v[2 * p]);
                    const F qa = f_mul(dm, dv), qc = f_mul(m[2 * p], v[2 * p]), qe = f_mul(m[2 * p + 1], v[2 * p + 1]);
                    c0 = f_add(c0, qa);
                    c1 = f_add(c1, f_add(f_sub(f_sub(qe, qa), qc), f_sub(a[2 * p + 1], a[2 * p])));
                    c2 = f_add(c2, f_add(qc, a[2 * p]));
                }
                F *poly = buf + sp.poly_pos + 3 * (size_t) (k - 1);
                poly[0] = f_add(poly[0], c0); poly[1] = f_add(poly[1], c1); poly[2] = f_add(poly[2], c2);
                const F rk = r[k - 1];
                for (int p = 0; p < len / 2; ++p) {
                    v[p] = f_add(v[2 * p], f_mul(rk, f_sub(v[2 * p + 1], v[2 * p])));
                    m[p] = f_add(m[2 * p], f_mul(rk, f_sub(m[2 * p + 1], m[2 * p])));
                    a[p] = f_add(a[2 * p], f_mul(rk, f_sub(a[2 * p + 1], a[2 * p])));
                }
                len >>= 1;
            }
            // one entry left after round bl: the claim of the table; a table shorter than the sumcheck retires into add_term in round bl + 1
            buf[sp.claims_pos + t.j] = f_add(buf[sp.claims_pos + t.j], v[0]);
            if (t.bl < sp.rounds) ret[t.bl + 1] = f_add(ret[t.bl + 1], f_add(f_mul(v[0], m[0]), a[0]));
        }
        F at = f_zero();                                              // the split tables' share of add_term: linear, so it is added on top
        for (int k = 1; k <= sp.rounds; ++k) {
            if (k >= 2 && !f_is_zero(at)) at = f_mul(at, f_sub(f_one(), r[k - 2]));
            at = f_add(at, ret[k]);
            F *poly = buf + sp.poly_pos + 3 * (size_t) (k - 1);
            poly[1] = f_sub(poly[1], at); poly[2] = f_add(poly[2], at);
        }
        // five-product fold: from round 2 on the fold launches left sum m1 v1 + a1 out and nobody derived b from partial sums; now that a and c
        // are complete, b_k = S_{k-1}(r_{k-1}) - a_k - 2 c_k (src/verifier.cpp:208,249,295), in order.  Round 1 summed everything itself.
        if (ctx->opt.drop_y)
            for (int k = 2; k <= sp.rounds; ++k) {
                const F *pp = buf + sp.poly_pos + 3 * (size_t) (k - 2);
                F *poly = buf + sp.poly_pos + 3 * (size_t) (k - 1);
                const F rr = r[k - 2];
                const F claim = f_add(f_mul(f_add(f_mul(pp[0], rr), pp[1]), rr), pp[2]);
                poly[1] = f_sub(f_sub(claim, poly[0]), f_add(poly[2], poly[2]));
            }
    }
}

// ---- one proof over several GPUs: the sumcheck chains of the plan are dealt out to the ranks -----------
// Given the tape every chain is independent (see above), each writes its own slice of the transcript, and every rank holds
// the circuit and the witness.  So rank r of w records and runs only the chains it owns; the other transcript slots stay
// zero and ONE all-reduce (u64 sum) of the transcript over RCCL assembles the proof (SURVEY.md §8e: "independent sumcheck
// instances shard across the GPUs").  Owners: longest-processing-time greedy on a cost estimate — table entries (x3) plus
// contributions of the init plus a constant for the closing launches; deterministic, identical on all ranks.
static void chain_costs(vp_ctx *ctx);
static void assign_chains(vp_ctx *ctx) {
    const int n_chains = (int) ctx->lanes.size() + 1;
    chain_costs(ctx);
    ctx->chain_owner.assign(n_chains, 0);
    if (ctx->shard_world <= 1) return;
    std::vector<int> order(n_chains);
    for (int c = 0; c < n_chains; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ctx->chain_cost[a] > ctx->chain_cost[b]; });
    std::vector<double> load(ctx->shard_world, 0.0);
    // index-split chains run on every rank below 2^lw, a slice each: their cost is spread before the whole chains are dealt out
    const int n_part = std::min(ctx->shard_world, 1 << ctx->split_lw);
    const int n_ = ctx->n_layers, n_lanes_ = 2 * (n_ - 1);
    for (int c = 0; c < n_chains; ++c)
        if (ctx->split_lw > 0 && c < (int) ctx->split.size() && !ctx->split[c].tabs.empty()) {
            // a rank's share of a split chain: the fixed cost of its closing launches + the chain's variable cost in proportion to the VALID
            // entries of its slices (layer sizes are not powers of two: the upper slices of a padded table are short or empty)
            const vp_ctx::SplitChain &sp = ctx->split[c];
            const int layer = c < n_lanes_ ? c / 2 + 1 : c - n_lanes_ + 1;
            std::vector<double> ent(n_part, 0.0);
            double tot = 0;
            for (const auto &t : sp.tabs) {
                const u64 valid = c < n_lanes_ ? ctx->L[layer - 1].size : ctx->L[layer].dad_size[t.j], S = (1ull << t.bl) >> ctx->split_lw;
                for (int r = 0; r < n_part; ++r) {
                    const u64 s_ = (u64) ((r + sp.small_owner) & (n_part - 1)), lo = s_ * S;
                    const double v = valid > lo ? (double) std::min<u64>(S, valid - lo) : 0.0;
                    ent[r] += v; tot += v;
                }
            }
            const double fixed = 2.0e6, var = std::max(0.0, ctx->chain_cost[c] - fixed);
            for (int r = 0; r < n_part; ++r) load[r] += fixed + (tot > 0 ? var * ent[r] / tot : var / n_part);
            ctx->chain_owner[c] = -1;
        }
    for (int c : order) {
        if (ctx->chain_owner[c] == -1) continue;
        if (ctx->chain_cost[c] == 0.0) { ctx->chain_owner[c] = 0; continue; }      // layers without a phase 2
        int best = 0;
        for (int r = 1; r < ctx->shard_world; ++r) if (load[r] < load[best]) best = r;
        ctx->chain_owner[c] = best; load[best] += ctx->chain_cost[c];
    }
}
static void chain_costs(vp_ctx *ctx) {
    const int n = ctx->n_layers, n_lanes = 2 * (n - 1), n_chains = (int) ctx->lanes.size() + 1;
    ctx->chain_cost.assign(n_chains, 0.0);
    // Weights fitted to the solo device time of every chain (bench.py --shard-sim <number of chains>: one chain per rank; x1024:
    // phase 1 of layer 2 1.43 ms, its phase 2 1.36 ms, its Liu sumcheck 1.19 ms; ~8.7 us per million units; a chain never takes
    // less than ~0.07 ms, the latency of init -> folds -> k_seg -> k_emit, which overlaps with the other chains of its rank).
    const double fixed = 2.0e6;
    for (int i = 1; i < n; ++i) {
        const LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
        u64 liu_contrib = 0;
        for (int k = i; k < n; ++k) liu_contrib += ctx->L[k].dad_size[i - 1];
        ctx->chain_cost[2 * (i - 1)] = fixed + 3.0 * (double) pre.size + 2.0 * (double) cur.c1.n_entries;
        ctx->chain_cost[2 * (i - 1) + 1] = fixed + 3.0 * (double) pre.size + 1.5 * (double) liu_contrib;
        if (cur.max_dad_bl != -1) {
            u64 ent = 0;
            for (int j = 0; j < i; ++j) ent += cur.dad_size[j];
            ctx->chain_cost[n_lanes + (i - 1)] = fixed + 4.0 * (double) ent + 2.0 * (double) cur.c2.n_entries + 1.0 * (double) pre.size;
        }
    }
    ctx->chain_cost[n_chains - 1] = 1.0;                  // Vres
}

// ---- plan: record, merge, upload ---------------------------------------------------------------------
static void free_plan(vp_ctx *ctx) {
    if (!ctx->plan) return;
    for (auto &nd : ctx->plan->nodes) if (nd.ev) (void) hipEventDestroy(nd.ev);
    if (ctx->plan->ev_root) (void) hipEventDestroy(ctx->plan->ev_root);
    for (int q = 0; q < 4; ++q) if (ctx->plan->ev_join[q]) (void) hipEventDestroy(ctx->plan->ev_join[q]);
    for (int q = 1; q < 4; ++q) if (ctx->plan->streams[q]) (void) hipStreamDestroy(ctx->plan->streams[q]);
    for (void *p : ctx->plan->allocs) (void) hipFree(p);      // job descriptors and the block map: a plan is rebuilt on every vp_set_shard
    delete ctx->plan;
    ctx->plan = nullptr;
    ctx->vu_supplied = false;                                 // (the sums lived in the plan's buffers)
}

// Chains = the lanes of the stream path (Liu of layer i; phases 1+2 of layer i).  Step t of the plan holds the t-th launch
// of every chain; launches of one kernel kind inside a step become ONE node.  A node depends on the nodes that hold the
// previous launch of each of its chains, nothing else.
static int build_plan(vp_ctx *ctx) {
    static thread_local bool fixup_refused = false;             // set while a plan is re-recorded without the round-1 variant
    struct Reset { bool &f; bool top; ~Reset() { if (top) f = false; } } reset{fixup_refused, !fixup_refused};
    free_plan(ctx);
    split_layout(ctx);
    assign_chains(ctx);
    if (ctx->n_exp) {                                                // transcript + export area in one buffer (one all-reduce)
        VPCHK(dalloc(ctx, &ctx->d_trs, (size_t) (ctx->n_tr + 3 * ctx->n_exp)));        // (lives until the next circuit upload)
    }
    PlanRec rec;
    rec.chains.assign(ctx->lanes.size() + 1, {});
    ctx->rec = &rec;
    const vp_stats keep = ctx->st;
    ctx->st.rounds = 0;
    // VP_DROP_Y1=1: round 1 of every sumcheck leaves its b to a fix-up pass over the finished transcript as well (k_fixup).  Measured:
    // the fold launches get a little shorter (x1024 146 -> 143 us each, proof 7.11 -> 7.00 ms) but the extra launch behind the join
    // costs ~20 us (x64 0.717 -> 0.738 ms), so it is off by default.  Never for a proof sharded over ranks: the claims live in
    // other ranks' transcript slices.
    {
        ctx->drop_round1 = ctx->opt.drop_y && ctx->opt.drop_y_round1 && ctx->shard_world <= 1 && !fixup_refused;
    }
    ctx->rec_fix.clear();
    int rc = submit_gkr(ctx, false);
    ctx->rec = nullptr;
    if (rc == VP_OK && ctx->drop_round1) {
        // a value another sumcheck starts from must not itself wait for the fix-up: the last polynomial of a phase 1 that feeds a phase 2
        for (const FixJob &f : ctx->rec_fix)
            if (f.rounds && ((f.derive_mask >> (f.rounds - 1)) & 1u)) { fixup_refused = true; break; }
        if (fixup_refused) return build_plan(ctx);               // record again with round 1 kept in the fold launches
    }
    if (ctx->owned((int) ctx->lanes.size())) {   // Vres (verifier.cpp:151) = <eq(r_0, .), output layer>: one more inner-product chain instead of a lone workgroup up front
        LayerDev &T = ctx->L[ctx->n_layers - 1];
        DotJob d{}; d.h = T.hg; d.val = T.val; d.part = ctx->partials; d.out = ctx->tr_base(); d.size = (u32) T.size; d.vreal = ctx->vreal;
        d.valr = ctx->vreal ? T.valr : nullptr;
        d.nblk = std::max<u32>(1, std::min<u32>(nblk(T.size), plan_dot_blocks()));
        rec.dot.push_back(d);
        rec.cur = (int) ctx->lanes.size();
        rec.push(NK_DOT, (u32) rec.dot.size() - 1, d.nblk, 0, 16 * (u64) d.size, d.size);
        rec.push(NK_DOTFIN, (u32) rec.dot.size() - 1, 1, 0, 16 * (u64) d.nblk, d.nblk);
    }
    const u64 rounds = ctx->st.rounds;
    ctx->st = keep;
    if (rc != VP_OK) return rc;
    Plan *P = new Plan();
    ctx->plan = P; ctx->plan_vreal = ctx->vreal;
    P->rounds = rounds;
    static const int kind_stream[NK_COUNT] = {0, 0, 0, 0, 0, 1, 2, 3, 0};     // init kernels and the closing launch | fused init + fold | fold | k_seg
    size_t T = 0;
    for (auto &c : rec.chains) T = std::max(T, c.size());
    P->n_steps = (int) T;
    std::vector<LightJob> light; std::vector<ChunkJob> chunks; std::vector<CombineJob> combine; std::vector<DotJob> dot, dotfin;
    std::vector<SfArgs> sf; std::vector<SfGenJob> sfgen; std::vector<SegArgs> seg; std::vector<EmitArgs> emit;
    std::vector<BlkMap> map;
    // Placement of a chain's launches on the global step axis: its init and fold launches start at step 0 (the throughput
    // work of every chain is available to the device from the beginning), its closing k_seg / k_emit launches are aligned
    // at the END, so that those of all chains fall into the same few steps (one node each instead of a tail of small,
    // serialised ones).  VP_PLAN_ALIGN=left|right: everything at the start / at the end.
    const bool align_left = ctx->opt.plan_align == 1, align_right = ctx->opt.plan_align == 2;
    std::vector<std::vector<size_t>> pos(rec.chains.size());
    for (size_t c = 0; c < rec.chains.size(); ++c) {
        const auto &ch = rec.chains[c];
        size_t suf = ch.size();
        while (suf > 0 && (ch[suf - 1].kind == NK_SEG || ch[suf - 1].kind == NK_EMIT)) --suf;
        if (align_left) suf = ch.size();
        if (align_right) suf = 0;
        pos[c].resize(ch.size());
        for (size_t k = 0; k < ch.size(); ++k) pos[c][k] = k < suf ? k : T - (ch.size() - k);
    }
    std::vector<size_t> cursor(rec.chains.size(), 0);
    std::vector<int> last_node(rec.chains.size(), -1), pending(rec.chains.size(), -1);
    int last_on_stream[4] = {-1, -1, -1, -1};
    for (size_t t = 0; t < T; ++t) {
        for (size_t c = 0; c < rec.chains.size(); ++c)            // placeholder steps only consume their slot
            if (cursor[c] < rec.chains[c].size() && pos[c][cursor[c]] == t && rec.chains[c][cursor[c]].kind < 0) ++cursor[c];
        for (int kind = 0; kind < NK_COUNT; ++kind) {
            PNode nd; nd.kind = kind; nd.step = (int) t; nd.stream = kind_stream[kind]; nd.map_off = (u32) map.size();
            nd.p2 = true;
            u32 first = 0;
            switch (kind) {
                case NK_LIGHT: first = (u32) light.size(); break; case NK_DOT: first = (u32) dot.size(); break; case NK_DOTFIN: first = (u32) dotfin.size(); break;
                case NK_CHUNKS: first = (u32) chunks.size(); break; case NK_COMBINE: first = (u32) combine.size(); break;
                case NK_SF: first = (u32) sf.size(); break; case NK_SFGEN: first = (u32) sfgen.size(); break; case NK_SEG: first = (u32) seg.size(); break;
                default: first = (u32) emit.size(); break;
            }
            nd.first = first;
            for (size_t c = 0; c < rec.chains.size(); ++c) {
                const size_t k = cursor[c];
                if (k >= rec.chains[c].size() || pos[c][k] != t || rec.chains[c][k].kind != kind) continue;
                const PStep &st = rec.chains[c][k];
                const u32 job = first + nd.count;
                nd.p2 = nd.p2 && c >= 2 * (size_t) (ctx->n_layers - 1) && c < ctx->lanes.size();
                switch (kind) {
                    case NK_LIGHT: light.push_back(rec.light[st.idx]); break; case NK_DOT: dot.push_back(rec.dot[st.idx]); break; case NK_DOTFIN: dotfin.push_back(rec.dot[st.idx]); break;
                    case NK_CHUNKS: chunks.push_back(rec.chunks[st.idx]); break; case NK_COMBINE: combine.push_back(rec.combine[st.idx]); break;
                    case NK_SF: sf.push_back(rec.sf[st.idx]); break; case NK_SFGEN: sfgen.push_back(rec.sfgen[st.idx]); break; case NK_SEG: seg.push_back(rec.seg[st.idx]); break;
                    default: emit.push_back(rec.emit[st.idx]); break;
                }
                if (kind != NK_EMIT && kind != NK_DOTFIN) for (u32 b = 0; b < st.grid; ++b) map.push_back(BlkMap{job - first, b});
                nd.grid += st.grid; nd.lds = std::max(nd.lds, st.lds); nd.bytes += st.bytes; nd.work += st.work; ++nd.count;
                if (st.n_rounds) {          // rounds covered by the node: earliest first round .. latest last round over its jobs
                    const int last = std::max(nd.first_round ? nd.first_round + nd.n_rounds - 1 : 0, st.first_round + st.n_rounds - 1);
                    nd.first_round = nd.first_round ? std::min(nd.first_round, st.first_round) : st.first_round;
                    nd.n_rounds = last - nd.first_round + 1;
                }
                if (last_node[c] >= 0 && std::find(nd.deps.begin(), nd.deps.end(), last_node[c]) == nd.deps.end()) nd.deps.push_back(last_node[c]);
                if (st.xchain >= 0) {
                    const int x = last_node[st.xchain];
                    if (x < 0) { ctx->err = "internal: plan cross dependency not placed yet"; return VP_EINVAL; }
                    if (std::find(nd.deps.begin(), nd.deps.end(), x) == nd.deps.end()) nd.deps.push_back(x);
                }
                pending[c] = (int) P->nodes.size();                  // this node (pushed below); becomes last_node at the end of the step
            }
            if (nd.count) {
                // A fold node that does not wait for the fold node before it on the fold stream (the first fold launch of the phase-2
                // sumchecks of the large layers waits for its init, not for the closing fold launches of everything else) must not queue
                // behind it — under stream capture the order on a stream becomes a dependency: it continues on the stream of one of its
                // own fold predecessors if that one is still the last there, else on the (by then idle) stream of the fused launches.
                if (ctx->opt.fold_branches && nd.kind == NK_SF) {
                    auto has = [&](int x) { return std::find(nd.deps.begin(), nd.deps.end(), x) != nd.deps.end(); };
                    const int dflt = nd.stream;
                    if (last_on_stream[dflt] >= 0 && !has(last_on_stream[dflt])) {
                        int pick = -1;
                        for (int q = 1; q < 3 && pick < 0; ++q) if (q != dflt && last_on_stream[q] >= 0 && has(last_on_stream[q]) && P->nodes[last_on_stream[q]].kind == NK_SF) pick = q;
                        nd.stream = pick >= 0 ? pick : 1;
                    }
                }
                last_on_stream[nd.stream] = (int) P->nodes.size();
                P->nodes.push_back(nd);
            }
        }
        // advance the chains placed in this step
        for (size_t c = 0; c < rec.chains.size(); ++c)
            if (pending[c] >= 0) { last_node[c] = pending[c]; pending[c] = -1; ++cursor[c]; }
    }
    if (ctx->opt.debug & 1) {
        static const char *kn[NK_COUNT] = {"light", "chunks", "combine", "dot", "dotfin", "sfgen", "sf", "seg", "emit"};
        for (size_t q = 0; q < P->nodes.size(); ++q) {
            const PNode &nd = P->nodes[q];
            fprintf(stderr, "[vp] plan node %2zu: step %2d %-8s stream %d jobs %3u grid %6u rounds %d+%d work %llu deps", q, nd.step, kn[nd.kind], nd.stream, nd.count, nd.grid,
                    nd.first_round, nd.n_rounds, (unsigned long long) nd.work);
            for (int d : nd.deps) fprintf(stderr, " %d", d);
            fprintf(stderr, "\n");
        }
    }
    for (auto &nd : P->nodes)
        for (int d : nd.deps) if (P->nodes[d].stream != nd.stream) P->nodes[d].record = true;
    for (auto &nd : P->nodes) HIPCHK(hipEventCreateWithFlags(&nd.ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&P->ev_root, hipEventDisableTiming));
    for (int q = 0; q < 4; ++q) HIPCHK(hipEventCreateWithFlags(&P->ev_join[q], hipEventDisableTiming));
    const size_t alloc_mark = ctx->allocs.size();        // the uploads below belong to the plan, not to the circuit
    struct Own { vp_ctx *c; Plan *p; size_t m; ~Own() { if (c->allocs.size() > m) { p->allocs.assign(c->allocs.begin() + m, c->allocs.end()); c->allocs.resize(m); } } } own{ctx, P, alloc_mark};
    VPCHK(dupload(ctx, &P->d_dot, dot)); VPCHK(dupload(ctx, &P->d_dotfin, dotfin));
    VPCHK(dupload(ctx, &P->d_light, light)); VPCHK(dupload(ctx, &P->d_chunks, chunks));
    VPCHK(dupload(ctx, &P->d_combine, combine)); VPCHK(dupload(ctx, &P->d_sf, sf)); VPCHK(dupload(ctx, &P->d_sfgen, sfgen)); VPCHK(dupload(ctx, &P->d_seg, seg));
    VPCHK(dupload(ctx, &P->d_emit, emit)); VPCHK(dupload(ctx, &P->d_map, map));
    for (const SfGenJob &gj : sfgen) ++P->gen_jobs[(gj.mode & 3) + (gj.r.on ? 4 : 0)];
    if (ctx->drop_round1) { VPCHK(dupload(ctx, &P->d_fix, ctx->rec_fix)); P->n_fix = (u32) ctx->rec_fix.size(); }
    if (ctx->split_lw > 0 && ctx->shard_world > 1 && ctx->opt.split_vu) {
        // V_u of the index-split phase-2 chains (same list on every rank: split_layout depends on the circuit and the world size only)
        const int n_lanes_ = 2 * (ctx->n_layers - 1), Wp = 1 << ctx->split_lw;
        const bool in_split = ctx->shard_rank < Wp;
        std::vector<DotJob> js, jw; std::vector<BlkMap> mp; std::vector<F *> dst;
        for (int i = 1; i < ctx->n_layers; ++i) {
            const vp_ctx::SplitChain &sp = ctx->split[n_lanes_ + (i - 1)];
            if (sp.tabs.empty()) continue;
            P->vu_layers.push_back(i);
        }
        F *parts = nullptr;
        const u32 nb_max = plan_dot_blocks();
        if (!P->vu_layers.empty()) VPCHK(dalloc(ctx, &parts, (size_t) nb_max * P->vu_layers.size()));
        for (size_t c = 0; c < P->vu_layers.size(); ++c) {
            const int i = P->vu_layers[c];
            const LayerDev &cur = ctx->L[i], &pre = ctx->L[i - 1];
            const vp_ctx::SplitChain &sp = ctx->split[n_lanes_ + (i - 1)];
            DotJob d{}; d.h = cur.hu; d.val = pre.val; d.part = parts + c * nb_max; d.size = (u32) pre.size; d.vreal = ctx->vreal;
            d.valr = ctx->vreal ? pre.valr : nullptr;
            d.nblk = std::max<u32>(1, std::min<u32>(nblk(pre.size), nb_max));
            jw.push_back(d);
            // this rank's share: whole runs of 2^h1 entries (the unit k_dot_multi walks), dealt in order of the slice the rank folds in this chain
            const u32 H = 1u << d.h.h1, runs = (d.size + H - 1) >> d.h.h1, per = (runs + Wp - 1) / Wp;
            const u32 s_ = (u32) ((ctx->shard_rank + sp.small_owner) & (Wp - 1));
            const u32 r0 = in_split ? std::min(runs, s_ * per) : 0u, r1 = in_split ? std::min(runs, (s_ + 1) * per) : 0u;
            d.beg = r0 << d.h.h1; d.size = (u32) std::min<u64>(pre.size, (u64) r1 << d.h.h1);
            if (d.size < d.beg) d.size = d.beg;
            js.push_back(d);
            for (u32 b = 0; b < d.nblk; ++b) mp.push_back(BlkMap{(u32) c, b});
            dst.push_back(ctx->lanes[n_lanes_ + (i - 1)].Vu);
        }
        if (!P->vu_layers.empty()) {
            VPCHK(dalloc(ctx, &P->d_vu_sum, P->vu_layers.size()));
            for (auto &d : js) d.out = P->d_vu_sum + (&d - js.data());
            for (auto &d : jw) d.out = P->d_vu_sum + (&d - jw.data());
            VPCHK(dupload(ctx, &P->d_vu_slice, js)); VPCHK(dupload(ctx, &P->d_vu_whole, jw)); VPCHK(dupload(ctx, &P->d_vu_map, mp)); VPCHK(dupload(ctx, &P->d_vu_dst, dst));
            P->vu_grid = (u32) mp.size();
        }
    }
    // streams owned by the plan (stream priorities were measured: no effect under hipGraph replay, harmful on direct submission)
    P->streams[0] = ctx->stream;
    for (int q = 1; q < 4; ++q) HIPCHK(hipStreamCreateWithFlags(&P->streams[q], hipStreamNonBlocking));
    return VP_OK;
}

static void launch_node(const Plan &P, const PNode &nd, hipStream_t st) {
    const BlkMap *mp = P.d_map + nd.map_off;
    switch (nd.kind) {
        case NK_LIGHT: hipLaunchKernelGGL(k_light_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_light + nd.first, mp); break;
        case NK_DOT: hipLaunchKernelGGL(k_dot_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_dot + nd.first, mp); break;
        case NK_DOTFIN: hipLaunchKernelGGL(k_dotfin_multi, dim3(nd.count), dim3(VP_BLOCK), 0, st, P.d_dotfin + nd.first); break;
        case NK_CHUNKS: hipLaunchKernelGGL(k_chunks_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_chunks + nd.first, mp); break;
        case NK_COMBINE: hipLaunchKernelGGL(k_combine_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_combine + nd.first, mp); break;
        case NK_SFGEN: hipLaunchKernelGGL(k_sumfold3b_gen_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_sfgen + nd.first, mp); break;
        case NK_SF: hipLaunchKernelGGL(k_sumfold3b_multi, dim3(nd.grid), dim3(VP_BLOCK), 0, st, P.d_sf + nd.first, mp); break;
        case NK_SEG: hipLaunchKernelGGL(k_seg_multi, dim3(nd.grid), dim3(VP_SEG_THREADS), 0, st, P.d_seg + nd.first, mp); break;
        default: hipLaunchKernelGGL(k_emit_multi, dim3(nd.count), dim3(VP_EMIT_THREADS), nd.lds, st, P.d_emit + nd.first); break;
    }
}

// Replays the plan: four streams (init kernels | k_sumfold3b | k_seg | k_emit), events only where a node's predecessor
// ran on another stream.  single = everything on the main stream in step order (profiling: the k_sumfold3b nodes are
// bracketed with events).
static int submit_plan(vp_ctx *ctx, bool single) {
    Plan &P = *ctx->plan;
    {
        const bool profb = single && ctx->profiling;
        const int sl = profb ? prof_begin(ctx, ctx->stream, VP_K_BETA, ctx->n_all_jobs * ctx->beta_bpj, ctx->n_all_jobs, 0, 0) : -1;
        hipLaunchKernelGGL(k_beta_half_direct, dim3(ctx->n_all_jobs * ctx->beta_bpj), dim3(VP_BLOCK), 0, ctx->stream, ctx->all_jobs, ctx->beta_bpj);
        prof_end(ctx, ctx->stream, sl);
    }
    ctx->st.launches += 1 + P.nodes.size();
    ctx->st.rounds += P.rounds;
    if (!single) {
        HIPCHK(hipEventRecord(P.ev_root, ctx->stream));
        for (int q = 1; q < 4; ++q) HIPCHK(hipStreamWaitEvent(P.streams[q], P.ev_root, 0));
    }
    std::vector<std::vector<char>> waited(4, std::vector<char>(P.nodes.size(), 0));       // a stream waits for a node once: later launches on it are ordered behind that wait
    for (auto &nd : P.nodes) {
        hipStream_t st = single ? ctx->stream : P.streams[nd.stream];
        if (!single) for (int d : nd.deps) if (P.nodes[d].stream != nd.stream && !waited[nd.stream][d]) { waited[nd.stream][d] = 1; HIPCHK(hipStreamWaitEvent(st, P.nodes[d].ev, 0)); }
        // profiled replay (single stream): EVERY node is bracketed; the per-launch table is what vp_get_launch_stats returns
        const int sl = (single && ctx->profiling) ? prof_begin(ctx, st, nd.kind + 1 /* NK_* -> VP_K_* */, nd.grid, nd.count, nd.bytes, nd.work, (u32) nd.n_rounds, (u32) nd.first_round) : -1;
        launch_node(P, nd, st);
        prof_end(ctx, st, sl);
        if (!single && nd.record) HIPCHK(hipEventRecord(nd.ev, st));
    }
    if (!single) {
        for (int q = 1; q < 4; ++q) {
            HIPCHK(hipEventRecord(P.ev_join[q], P.streams[q]));
            HIPCHK(hipStreamWaitEvent(ctx->stream, P.ev_join[q], 0));
        }
    }
    if (P.n_fix) {                                               // every sumcheck is closed: restore the b's the fold launches left out
        const int sl = (single && ctx->profiling) ? prof_begin(ctx, ctx->stream, VP_K_FIXUP, (P.n_fix + 63) / 64, P.n_fix, 0, 0) : -1;
        hipLaunchKernelGGL(k_fixup, dim3((P.n_fix + 63) / 64), dim3(64), 0, ctx->stream, P.d_fix, P.n_fix, ctx->d_tape, ctx->d_tr);
        prof_end(ctx, ctx->stream, sl);
        ctx->st.launches += 1;
    }
    return VP_OK;
}

// The same plan as an EXPLICIT graph (graph_explicit): one kernel node per plan node with exactly the plan's dependencies — under stream capture
// the order of unrelated launches on one of the four streams becomes a dependency as well (HISTORY.md section 7, "a false dependency in the replay").
static int plan_graph_explicit(vp_ctx *ctx, hipGraph_t *out) {
    Plan &P = *ctx->plan;
    hipGraph_t g = nullptr;
    HIPCHK(hipGraphCreate(&g, 0));
    struct Free { hipGraph_t *g; bool keep = false; ~Free() { if (!keep && *g) (void) hipGraphDestroy(*g); } } fr{&g};
    auto add = [&](hipGraphNode_t *n, const std::vector<hipGraphNode_t> &deps, void *func, u32 grid, u32 block, u32 lds, void **args) -> hipError_t {
        hipKernelNodeParams kp{};
        kp.func = func; kp.gridDim = dim3(grid); kp.blockDim = dim3(block); kp.sharedMemBytes = lds; kp.kernelParams = args; kp.extra = nullptr;
        return hipGraphAddKernelNode(n, g, deps.empty() ? nullptr : deps.data(), deps.size(), &kp);
    };
    hipGraphNode_t beta = nullptr;
    {
        const void *jobs = ctx->all_jobs; int bpj = ctx->beta_bpj;
        void *args[] = {(void *) &jobs, (void *) &bpj};
        HIPCHK(add(&beta, {}, (void *) k_beta_half_direct, ctx->n_all_jobs * ctx->beta_bpj, VP_BLOCK, 0, args));
    }
    std::vector<hipGraphNode_t> gn(P.nodes.size(), nullptr);
    std::vector<char> has_child(P.nodes.size(), 0);
    // graph_explicit = 2: the captured graph's shape — every node also behind the node before it on its stream — except that the inner products
    // V_u (k_dot / k_dotfin) get a stream of their own: they head the proof's longest chain and depend on nothing but the circuit values
    const bool stream_edges = ctx->opt.graph_explicit >= 2;
    int last_on[6] = {-1, -1, -1, -1, -1, -1};
    for (size_t q = 0; q < P.nodes.size(); ++q) {
        const PNode &nd = P.nodes[q];
        std::vector<hipGraphNode_t> deps;
        for (int d : nd.deps) { deps.push_back(gn[d]); has_child[d] = 1; }
        if (stream_edges) {
            const int vs = (nd.kind == NK_DOT || nd.kind == NK_DOTFIN) ? 4 :
                           (ctx->opt.graph_explicit == 3 && nd.p2 && (nd.kind == NK_LIGHT || nd.kind == NK_CHUNKS || nd.kind == NK_COMBINE)) ? 5 : nd.stream;
            const int pr = last_on[vs];
            if (pr >= 0 && std::find(nd.deps.begin(), nd.deps.end(), pr) == nd.deps.end()) { deps.push_back(gn[pr]); has_child[pr] = 1; }
            last_on[vs] = (int) q;
        }
        if (deps.empty()) deps.push_back(beta);
        const BlkMap *mp = P.d_map + nd.map_off;
        const void *jobs = nullptr; void *func = nullptr; u32 grid = nd.grid, block = VP_BLOCK, lds = 0; bool with_map = true;
        switch (nd.kind) {
            case NK_LIGHT: jobs = P.d_light + nd.first; func = (void *) k_light_multi; break;
            case NK_DOT: jobs = P.d_dot + nd.first; func = (void *) k_dot_multi; break;
            case NK_DOTFIN: jobs = P.d_dotfin + nd.first; func = (void *) k_dotfin_multi; grid = nd.count; with_map = false; break;
            case NK_CHUNKS: jobs = P.d_chunks + nd.first; func = (void *) k_chunks_multi; break;
            case NK_COMBINE: jobs = P.d_combine + nd.first; func = (void *) k_combine_multi; break;
            case NK_SFGEN: jobs = P.d_sfgen + nd.first; func = (void *) k_sumfold3b_gen_multi; break;
            case NK_SF: jobs = P.d_sf + nd.first; func = (void *) k_sumfold3b_multi; break;
            case NK_SEG: jobs = P.d_seg + nd.first; func = (void *) k_seg_multi; block = VP_SEG_THREADS; break;
            default: jobs = P.d_emit + nd.first; func = (void *) k_emit_multi; grid = nd.count; block = VP_EMIT_THREADS; lds = nd.lds; with_map = false; break;
        }
        void *args[] = {(void *) &jobs, (void *) &mp};
        (void) with_map;                                       // kernels without a map take one argument: the second pointer is simply not read
        HIPCHK(add(&gn[q], deps, func, grid, block, lds, args));
    }
    if (P.n_fix) {
        std::vector<hipGraphNode_t> leaves;
        for (size_t q = 0; q < P.nodes.size(); ++q) if (!has_child[q]) leaves.push_back(gn[q]);
        const FixJob *fj = P.d_fix; u32 nf = P.n_fix; const F *tape = ctx->d_tape; F *tr = ctx->d_tr;
        void *args[] = {(void *) &fj, (void *) &nf, (void *) &tape, (void *) &tr};
        hipGraphNode_t fx = nullptr;
        HIPCHK(add(&fx, leaves, (void *) k_fixup, (P.n_fix + 63) / 64, 64, 0, args));
    }
    ctx->st.launches += 1 + P.nodes.size() + (P.n_fix ? 1 : 0);
    ctx->st.rounds += P.rounds;
    fr.keep = true;
    *out = g;
    return VP_OK;
}

bool vp_comm_attached(const vp_ctx *ctx);
int vp_allreduce_u64(vp_ctx *ctx, void *dev_buf, uint64_t count);
// ---- index-split proof: V_u of the split phase-2 chains ahead of the graph -------------------------------------------------------------------
// V_u = <eq(r_u, .), V_{i-1}> depends on the tape and the witness only, so the inner products of ALL split phase-2 chains can stand at the head of
// the proof: every rank adds up 1/W' of each (the previous layer is 2^26 entries at x1024: the whole of it was 0.2 of a rank's 1.32 ms), one
// all-reduce of 16 bytes per chain completes them, and the graph starts with V_u in place.  Without a communicator the caller does the exchange
// (vp_shard_vu_partials / vp_shard_vu_set); a proof with neither adds up the whole layer on every rank, as round 4 did inside the graph.
static u64 tape_tag(const vp_F *tape, u64 n) {                 // FNV-1a over the tape: the sums handed to vp_shard_vu_set belong to ONE tape
    u64 h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(tape);
    for (u64 i = 0; i < n * sizeof(vp_F); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h ? h : 1;
}
static int vu_pre_dots(vp_ctx *ctx, bool slice) {
    Plan &P = *ctx->plan;
    for (int i : P.vu_layers) VPCHK(half_tables_of(ctx, ctx->L[i].job_hu, 1));
    const DotJob *jobs = slice ? P.d_vu_slice : P.d_vu_whole;
    hipLaunchKernelGGL(k_dot_multi, dim3(P.vu_grid), dim3(VP_BLOCK), 0, ctx->stream, jobs, P.d_vu_map);
    hipLaunchKernelGGL(k_dotfin_multi, dim3((u32) P.vu_layers.size()), dim3(VP_BLOCK), 0, ctx->stream, jobs);
    return VP_OK;
}
static int vu_pre_run(vp_ctx *ctx) {
    Plan &P = *ctx->plan;
    const u32 n = (u32) P.vu_layers.size();
    if (vp_comm_attached(ctx)) {
        ctx->vu_supplied = false;                                 // sums a caller handed over (vp_shard_vu_set) are not used beside a communicator
        VPCHK(vu_pre_dots(ctx, true));
        VPCHK(vp_allreduce_u64(ctx, P.d_vu_sum, 2 * (u64) n));    // <= 8 canonical partial sums per limb (vp_set_shard_split refuses more slices): < 2^64
    } else if (ctx->vu_supplied) ctx->vu_supplied = false;       // the caller's sums are in d_vu_sum (vp_shard_vu_set)
    else if (ctx->shard_rank < (1 << ctx->split_lw)) VPCHK(vu_pre_dots(ctx, false));
    hipLaunchKernelGGL(k_vu_place, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const F *) P.d_vu_sum, (F *const *) P.d_vu_dst, n);
    return VP_OK;
}
// ---- the plan tuner's choices, remembered per plan shape for the lifetime of the process ----------------------------------------------------
struct TunedPlan { int fuse_combine, fold_branches, plan_align, fuse_min_log, sf3b_grid, graph_explicit; };
static std::mutex g_tune_mu;
static std::map<u64, TunedPlan> g_tune_cache;
// The same table kept across PROCESSES: a text file named by VP_PLAN_CACHE at vp_create, one line per plan shape ("<key hex> v0 .. v5", the six values of
// vp_plan_tuning_get).  Read once per process and path, appended to when the tuner has run; a line the library does not accept is ignored.  A first proof
// that finds its shape there records ONE plan and captures ONE graph instead of replaying ~14 candidates (x1024: ~1 s).
static std::string g_tune_file_loaded;
static std::set<u64> g_tune_file_keys;          // shapes the file of g_tune_file_loaded is known to hold
static void tune_file_load_locked(const std::string &path) {
    if (path.empty() || g_tune_file_loaded == path) return;
    g_tune_file_loaded = path; g_tune_file_keys.clear();
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return;
    char line[256];
    while (fgets(line, sizeof line, f)) {
        unsigned long long k = 0; int v[6];
        if (sscanf(line, "%llx %d %d %d %d %d %d", &k, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 7 || !k) continue;
        if (v[0] < 0 || v[0] > 2 || v[1] < 0 || v[1] > 1 || v[2] < 0 || v[2] > 2 || v[3] < 0 || v[3] > 30 || v[4] < 1 || v[4] > 2048 || v[5] < 0 || v[5] > 3) continue;
        if (!g_tune_cache.count(k)) g_tune_cache[k] = TunedPlan{v[0], v[1], v[2], v[3], v[4], v[5]};
        g_tune_file_keys.insert(k);
    }
    fclose(f);
}
static void tune_file_append(const std::string &path, u64 key, const TunedPlan &t) {
    if (path.empty() || (g_tune_file_loaded == path && g_tune_file_keys.count(key))) return;
    FILE *f = fopen(path.c_str(), "a");
    if (!f) return;
    if (g_tune_file_loaded == path) g_tune_file_keys.insert(key);
    fprintf(f, "%llx %d %d %d %d %d %d\n", (unsigned long long) key, t.fuse_combine, t.fold_branches, t.plan_align, t.fuse_min_log, t.sf3b_grid, t.graph_explicit);
    fclose(f);
}
// FNV-1a over everything the recorded plan's shape depends on: the layers' sizes and subset sizes, the sizes of the contribution lists, the
// kind of values, the device, and the option fields the tuner does not touch but that change the plan
static u64 plan_shape_key(const vp_ctx *ctx) {
    u64 h = 1469598103934665603ull;
    auto mix = [&](u64 v) { for (int b = 0; b < 8; ++b) { h ^= (v >> (8 * b)) & 0xff; h *= 1099511628211ull; } };
    mix((u64) ctx->n_layers); mix((u64) ctx->device); mix((u64) ctx->vreal); mix((u64) ctx->opt_pinned);
    mix((u64) ctx->opt.fuse_init); mix((u64) ctx->opt.fuse_dot); mix((u64) ctx->opt.drop_y); mix((u64) ctx->opt.drop_y_round1); mix((u64) ctx->opt.seg_tiny);
    mix((u64) ctx->opt.sf_big_log); mix((u64) ctx->opt.dot_blocks);
    mix((u64) ctx->opt.fuse_combine); mix((u64) ctx->opt.fold_branches); mix((u64) ctx->opt.plan_align); mix((u64) ctx->opt.fuse_min_log);
    mix((u64) ctx->opt.sf3b_grid); mix((u64) ctx->opt.graph_explicit);
    for (int i = 0; i < ctx->n_layers; ++i) {
        const LayerDev &L = ctx->L[i];
        mix(L.size); mix((u64) L.bl); mix((u64) (L.max_dad_bl + 2)); mix((u64) L.n_assert); mix((u64) L.l_n);
        mix((u64) L.c1.n_rows); mix((u64) L.c1.n_entries); mix((u64) L.c1.n_heavy); mix((u64) L.c1.n_chunks);
        mix((u64) L.c2.n_rows); mix((u64) L.c2.n_entries); mix((u64) L.c2.n_heavy); mix((u64) L.c2.n_chunks);
        for (u64 d : L.dad_size) mix(d);
    }
    return h ? h : 1;
}

static int prove_gkr_fused(vp_ctx *ctx, const vp_F *tape, uint64_t n_tape, uint8_t *transcript, uint64_t *n_written) {
    VP_ENTER_Q(ctx);
    // a pending proof still owns the pinned staging (h_io): one proof of a context in flight at a time.  What may stay pending here is the commitment
    // of THIS proof (vp_commit_private queued in front of it): the proof does not touch its buffers
    for (const auto &pd : ctx->pending) if (pd.phase == VP_PH_GKR) { VPCHK(flush_pending(ctx, (size_t) -1)); break; }
    const bool dbg_t = (ctx->opt.debug & 1) != 0;
    const auto t_in = std::chrono::steady_clock::now();
    const bool use_plan = ctx->plan_path != 0;
    const bool serial = ctx->serial || ctx->profiling;
    if (use_plan && ctx->plan && ctx->plan_vreal != ctx->vreal) free_plan(ctx);          // the plan's kernels were specialised for the other kind of values
    if (use_plan && !ctx->plan) VPCHK(build_plan(ctx));                                   // (also lays out the export area of an index-split proof)
    F *tr = ctx->tr_base();
    const bool split = ctx->split_lw > 0 && ctx->shard_world > 1 && ctx->n_exp > 0 && use_plan;
    const u64 pos = ctx->n_tr, pos_x = pos + (split ? 3 * ctx->n_exp : 0);               // transcript (+ export area) elements
    ctx->ev_used = 0;
    // pinned staging: pageable copies would be staged synchronously by the runtime on both sides of the proof
    if (ctx->h_io_cap < n_tape + pos_x) {
        if (ctx->h_io) (void) hipHostFree(ctx->h_io);
        ctx->h_io = nullptr; ctx->h_io_cap = 0;
        HIPCHK(hipHostMalloc((void **) &ctx->h_io, (n_tape + pos_x) * sizeof(F), hipHostMallocDefault));
        ctx->h_io_cap = n_tape + pos_x;
    }
    memcpy(ctx->h_io, tape, n_tape * sizeof(F));
    const bool kcopy = ctx->poll && ctx->opt.kernel_copies && n_tape > 0 && pos_x <= (1u << 16);      // small ends: by kernel, not by the copy engine
    if (kcopy) hipLaunchKernelGGL(k_tape_in, dim3((u32) ((n_tape + 255) / 256)), dim3(256), 0, ctx->stream, (const F *) ctx->h_io, ctx->d_tape, (u32) n_tape);
    else HIPCHK(hipMemcpyAsync(ctx->d_tape, ctx->h_io, n_tape * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    // The launch sequence depends on the circuit only (the tape is read on the device), so the concurrent form is
    // captured once per circuit into a hipGraph and replayed: one submission instead of ~170, every lane starts at once.
    const bool dbg = (ctx->opt.debug & 1) != 0;
    auto make_graph = [&]() -> int {
        ctx->st.launches = 0; ctx->st.rounds = 0;
        hipGraph_t g = nullptr;
        int rc = VP_OK;
        if (dbg) fprintf(stderr, "[vp] capture begin\n");
        if (use_plan && ctx->opt.graph_explicit) {
            rc = plan_graph_explicit(ctx, &g);
            if (rc != VP_OK) { g = nullptr; (void) hipGetLastError(); rc = VP_EHIP; }
        } else if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) != hipSuccess) rc = VP_EHIP;
        if (rc == VP_OK && !(use_plan && ctx->opt.graph_explicit)) {
            rc = use_plan ? submit_plan(ctx, false) : submit_gkr(ctx, false);
            if (dbg) fprintf(stderr, "[vp] submitted rc=%d\n", rc);
            if (hipStreamEndCapture(ctx->stream, &g) != hipSuccess || !g) rc = rc == VP_OK ? VP_EHIP : rc;
            if (dbg) fprintf(stderr, "[vp] capture end rc=%d g=%p\n", rc, (void *) g);
        }
        if (rc == VP_OK && hipGraphInstantiate(&ctx->gkr_graph, g, nullptr, nullptr, 0) != hipSuccess) { ctx->gkr_graph = nullptr; rc = VP_EHIP; }
        if (dbg) fprintf(stderr, "[vp] instantiated rc=%d\n", rc);
        if (g) (void) hipGraphDestroy(g);
        if (rc == VP_ELIMIT || rc == VP_EINVAL) return rc;
        if (rc != VP_OK) { (void) hipGetLastError(); ctx->graph_failed = true; }     // run the launches directly instead
        ctx->graph_launches = ctx->st.launches; ctx->graph_rounds = ctx->st.rounds;
        return VP_OK;
    };
    if (ctx->use_graph && !serial && !ctx->gkr_graph && !ctx->graph_failed) {
        // First proof of a circuit: which launches of different chains share a node — and with it what the graph replay overlaps — depends
        // on how the chains are laid along the step axis, and the best layout differs from circuit to circuit (x16: the combine step
        // removed is 10 % faster, x64: 5 % slower).  The few layouts the switches offer are replayed on THIS circuit and the fastest
        // kept (plan_autotune; a one-off cost of the first call: a plan, a capture and six replays per candidate).
        // What the tuner finds depends on the SHAPE of the plan only (layer sizes, contribution-list sizes, the fields the caller pinned): a second
        // context of the same circuit in this process — a second session of a serving prover, the second proof in flight — takes the first
        // one's choice from a process-wide table instead of replaying ~14 candidates again (vp_get_options reads it; a caller that keeps it
        // across processes passes it to vp_create_with_options with plan_autotune = 0).
        const u64 tkey = ctx->opt.plan_autotune && use_plan && ctx->shard_world == 1 && !ctx->plan_tuned ? plan_shape_key(ctx) : 0;
        if (tkey) {
            std::lock_guard<std::mutex> lk(g_tune_mu);
            tune_file_load_locked(ctx->plan_cache_path);
            auto it = g_tune_cache.find(tkey);
            if (it != g_tune_cache.end()) {
                const TunedPlan &t = it->second;
                ctx->opt.fuse_combine = t.fuse_combine; ctx->opt.fold_branches = t.fold_branches; ctx->opt.plan_align = t.plan_align;
                ctx->opt.fuse_min_log = t.fuse_min_log; ctx->opt.sf3b_grid = t.sf3b_grid; ctx->opt.graph_explicit = t.graph_explicit;
                ctx->plan_tuned = true; ctx->plan_tune_cached = true;
                tune_file_append(ctx->plan_cache_path, tkey, t);           // a shape tuned earlier in this process (or under another file) reaches this file too
                if (dbg) fprintf(stderr, "[vp] plan autotune: taken from the process-wide table (same plan shape)\n");
                VPCHK(build_plan(ctx));
            }
        }
        if (ctx->opt.plan_autotune && use_plan && ctx->shard_world == 1 && !ctx->plan_tuned) {
            ctx->plan_tuned = true;
            // one candidate: plan + capture + six replays (the first one not counted); < 0: it does not build or capture here — skipped,
            // never an error of the proof (the settings kept at the end have been replayed)
            auto try_candidate = [&]() -> float {
                if (ctx->gkr_graph) { (void) hipGraphExecDestroy(ctx->gkr_graph); ctx->gkr_graph = nullptr; }
                ctx->graph_failed = false;
                if (build_plan(ctx) != VP_OK || make_graph() != VP_OK || !ctx->gkr_graph) { ctx->graph_failed = false; ctx->err.clear(); (void) hipGetLastError(); return -1.0f; }
                float mn = 1e30f;
                for (int it = 0; it < 6; ++it) {
                    if (hipEventRecord(ctx->ev0, ctx->stream) != hipSuccess || hipGraphLaunch(ctx->gkr_graph, ctx->stream) != hipSuccess ||
                        hipEventRecord(ctx->ev1, ctx->stream) != hipSuccess || hipEventSynchronize(ctx->ev1) != hipSuccess) { (void) hipGetLastError(); return -1.0f; }
                    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
                    if (it) mn = std::min(mn, ms);
                }
                return mn;
            };
            struct Var { int fc, fb, al; };
            static const Var vars[] = {{2, 1, 0}, {1, 1, 0}, {2, 0, 0}, {1, 0, 0}, {0, 1, 0}, {2, 1, 1}};
            const int keep_fc = ctx->opt.fuse_combine, keep_fb = ctx->opt.fold_branches, keep_al = ctx->opt.plan_align;
            float best = 1e30f; int bi = -1;
            const uint32_t pin = ctx->opt_pinned;      // a field the caller set explicitly is not the tuner's to change
            for (int v = 0; v < (int) (sizeof vars / sizeof vars[0]); ++v) {
                if (((pin & 1u) && vars[v].fc != keep_fc) || ((pin & 2u) && vars[v].fb != keep_fb) || ((pin & 4u) && vars[v].al != keep_al)) continue;
                ctx->opt.fuse_combine = vars[v].fc; ctx->opt.fold_branches = vars[v].fb; ctx->opt.plan_align = vars[v].al;
                const float mn = try_candidate();
                if (dbg) fprintf(stderr, "[vp] plan autotune: fuse_combine %d fold_branches %d align %d -> %.4f ms\n", vars[v].fc, vars[v].fb, vars[v].al, mn);
                if (mn > 0 && mn < best) { best = mn; bi = v; }
            }
            if (bi >= 0) { ctx->opt.fuse_combine = vars[bi].fc; ctx->opt.fold_branches = vars[bi].fb; ctx->opt.plan_align = vars[bi].al; }
            else { ctx->opt.fuse_combine = keep_fc; ctx->opt.fold_branches = keep_fb; ctx->opt.plan_align = keep_al; }
            if (dbg) fprintf(stderr, "[vp] plan autotune: kept layout %d\n", bi);
            // second stage, in the kept layout: the size from which an init is generated inside its first fold launch, one step either way
            // (the default rule was fitted to the SHA-256 circuits); third stage: workgroups per fold job (the block partials the closing
            // launch adds up, and how the jobs of a node share the CUs: 384 instead of 512 is ~2 % faster up to x256, ~3 % slower at x1024).
            // A later stage is taken only if clearly (> 1 %) faster.
            if (bi >= 0 && ctx->fuse_init && !(pin & 8u)) {
                const int L0 = plan_fuse_min_log(), keep_fl = ctx->opt.fuse_min_log;
                int best_fl = keep_fl;
                for (int dl = -1; dl <= 1; dl += 2) {
                    ctx->opt.fuse_min_log = L0 + dl;
                    const float mn = try_candidate();
                    if (dbg) fprintf(stderr, "[vp] plan autotune: fuse_min_log %d -> %.4f ms\n", L0 + dl, mn);
                    if (mn > 0 && mn < 0.99f * best) { best = mn; best_fl = L0 + dl; }
                }
                ctx->opt.fuse_min_log = best_fl;
            }
            if (bi >= 0 && !(pin & 16u)) {
                const int keep_g = ctx->opt.sf3b_grid;
                int best_g = keep_g;
                for (int gcand : {384, 320}) {
                    if (gcand == keep_g) continue;
                    ctx->opt.sf3b_grid = gcand;
                    const float mn = try_candidate();
                    if (dbg) fprintf(stderr, "[vp] plan autotune: sf3b_grid %d -> %.4f ms\n", gcand, mn);
                    if (mn > 0 && mn < 0.99f * best) { best = mn; best_g = gcand; }
                }
                ctx->opt.sf3b_grid = best_g;
            }
            // last stage: the graph of the kept plan built node by node with exactly the plan's dependencies instead of captured from the four
            // streams (graph_explicit).  Which one replays faster depends on the circuit: the exact dependencies let the phase-2 chain start
            // earlier, but the runtime's own placement of that graph's branches costs more barriers between its queues — x1024 6.44-6.47 ->
            // 6.26-6.29 ms, x16 0.226 -> 0.211, x64 0.58 -> 0.62 (same call each).
            // (2 = the explicit graph in the captured shape, but with the inner products V_u on a stream of their own: the shape that stream capture
            // could not be trusted with, HISTORY.md section 7; x64 0.585-0.595 -> 0.577-0.595.  3 = the same with the phase-2 init launches on a stream of
            // their own as well, so that they start behind V_u instead of behind the phase-1 heavy rows: x64 0.579-0.584 -> 0.574-0.576.)
            if (bi >= 0 && !(pin & 32u)) {
                int best_ge = ctx->opt.graph_explicit;
                for (int ge = 0; ge <= 3; ++ge) {
                    if (ge == best_ge) continue;
                    const int keep_ge = ctx->opt.graph_explicit;
                    ctx->opt.graph_explicit = ge;
                    const float mn = try_candidate();
                    if (dbg) fprintf(stderr, "[vp] plan autotune: graph_explicit %d -> %.4f ms\n", ge, mn);
                    if (mn > 0 && mn < 0.99f * best) { best = mn; best_ge = ge; }
                    ctx->opt.graph_explicit = keep_ge;
                }
                ctx->opt.graph_explicit = best_ge;
            }
            if (ctx->gkr_graph) { (void) hipGraphExecDestroy(ctx->gkr_graph); ctx->gkr_graph = nullptr; }
            ctx->graph_failed = false;
            VPCHK(build_plan(ctx));
            if (tkey && bi >= 0) {
                std::lock_guard<std::mutex> lk(g_tune_mu);
                g_tune_cache[tkey] = TunedPlan{ctx->opt.fuse_combine, ctx->opt.fold_branches, ctx->opt.plan_align, ctx->opt.fuse_min_log, ctx->opt.sf3b_grid, ctx->opt.graph_explicit};
                tune_file_append(ctx->plan_cache_path, tkey, g_tune_cache[tkey]);
            }
        }
        const int rc = make_graph();
        if (rc != VP_OK) return rc;
    }
    // deferred completion only for the plain case: a replayed graph (or plan) of an unsharded proof, nothing profiled
    const bool can_defer = ctx->deferred && !ctx->profiling && ctx->shard_world <= 1 && !split;
    if (!can_defer && !ctx->pending.empty()) VPCHK(flush_pending(ctx, (size_t) -1));
    if (ctx->vu_supplied && vp_comm_attached(ctx)) ctx->vu_supplied = false;       // unused beside a communicator: never a reason to refuse the proof
    if (ctx->vu_supplied && ctx->vu_tape_tag != tape_tag(tape, n_tape)) {
        ctx->vu_supplied = false;
        ctx->err = "vp_prove_gkr: the V_u sums handed to vp_shard_vu_set were taken on another tape";
        return VP_EINVAL;
    }
    hipEvent_t ev_a = nullptr;
    VPCHK(defer_begin(ctx, &ev_a));
    EvGuard ev_guard{ctx, &ev_a};
    if (ctx->shard_world > 1) HIPCHK(hipMemsetAsync(tr, 0, pos_x * sizeof(F), ctx->stream));    // slots of the other ranks' chains (and export slots) stay zero
    const bool vu_given = ctx->vu_supplied;
    if (split && ctx->plan && !ctx->plan->vu_layers.empty()) VPCHK(vu_pre_run(ctx));
    if (ctx->use_graph && !serial && ctx->gkr_graph) {
        HIPCHK(hipGraphLaunch(ctx->gkr_graph, ctx->stream));
        ctx->st.launches = ctx->graph_launches; ctx->st.rounds = ctx->graph_rounds;
    } else {
        ctx->st.launches = 0; ctx->st.rounds = 0;
        if (use_plan) VPCHK(submit_plan(ctx, serial)); else VPCHK(submit_gkr(ctx, serial));
    }
    // chain-sharded proof with a communicator attached: the one data-path collective — u64 sum of the ranks' disjoint transcript
    // slices over RCCL / xGMI, on the device buffer, before the transcript leaves the GPU (inside the device-time bracket)
    const bool reduced = ctx->shard_world > 1 && vp_comm_attached(ctx);
    if (reduced) VPCHK(vp_allreduce_u64(ctx, tr, 2 * pos_x));
    hipEvent_t ev_b = ev_take(ctx);
    if (!ev_b) { ctx->err = "hipEventCreate"; return VP_EHIP; }
    HIPCHK(hipEventRecord(ev_b, ctx->stream));
    if (kcopy) hipLaunchKernelGGL(k_ship, dim3(1), dim3(1024), 0, ctx->stream, (const F *) tr, ctx->h_io + n_tape, (u32) pos_x, ctx->h_seq, ++ctx->seq);
    else {
        HIPCHK(hipMemcpyAsync(ctx->h_io + n_tape, tr, pos_x * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->poll) hipLaunchKernelGGL(k_ticket, dim3(1), dim3(1), 0, ctx->stream, ctx->h_seq, ++ctx->seq);
    }
    if (can_defer) {
        // the transcript is on its way to pinned memory (k_ship / the copy engine, then the ticket): what is left is the copy into the caller's buffer
        const u64 out_n = pos;
        ctx->st.fold_ms = 0; ctx->st.fold_bytes = 0; ctx->st.fold_launches = 0;
        ctx->ev_spare.push_back(ev_b);                   // (the device time of the deferred form includes the copy out: defer_end records its own end)
        const F *src = ctx->h_io + n_tape;
        return defer_end(ctx, ev_a, VP_PH_GKR, [ctx, transcript, n_written, src, out_n](float ms) {
            memcpy(transcript, src, out_n * sizeof(F));
            ctx->st.gkr_ms = ms;
            if (n_written) *n_written = out_n * sizeof(F);
            return VP_OK;
        });
    }
    const auto t_sub = std::chrono::steady_clock::now();
    VPCHK(wait_ticket(ctx));
    VPCHK(vp_check_collect(ctx));                       // (checked build only: a device-side index check that failed during this proof)
    if (dbg_t) {
        const auto t_done = std::chrono::steady_clock::now();
        fprintf(stderr, "[vp] prove_gkr host: submit %.1f us, wait %.1f us\n", std::chrono::duration<double, std::micro>(t_sub - t_in).count(),
                std::chrono::duration<double, std::micro>(t_done - t_sub).count());
    }
    // index-split proof: with a communicator the sums are complete here and the host finishes the split tables' last rounds; without one the
    // caller adds the ranks' buffers (transcript + export area, vp_gkr_sizes) and calls vp_shard_finish
    if (split && reduced) {
        u64 *w = reinterpret_cast<u64 *>(ctx->h_io + n_tape);
        for (u64 q = 0; q < 2 * pos_x; ++q) w[q] = host_fold(w[q]);                           // u64 sums of < 2^61 addends -> canonical
        split_finish(ctx, ctx->h_io + n_tape, ctx->h_io);
    }
    const u64 out_n = (split && !reduced) ? pos_x : pos;
    if (ctx->opt.debug & 1) fprintf(stderr, "[vp] prove_gkr: n_tr %llu n_exp %llu split %d reduced %d out_n %llu\n", (unsigned long long) pos, (unsigned long long) ctx->n_exp, (int) split, (int) reduced, (unsigned long long) out_n);
    memcpy(transcript, ctx->h_io + n_tape, out_n * sizeof(F));
    float ms = 0;
    hipEventElapsedTime(&ms, ev_a, ev_b);
    ctx->ev_spare.push_back(ev_b);                       // (ev_a goes back with its guard)
    if (vu_given) ms += ctx->vu_pre_ms;                 // the rank's partial inner products ran in vp_shard_vu_partials
    ctx->st.gkr_ms = ms; ctx->phase_ms[VP_PH_GKR] = ms;
    // vp_stats keeps the totals of the plain fold kernel (k_sumfold3b_multi); the whole table goes to vp_get_launch_stats
    ctx->st.fold_ms = 0; ctx->st.fold_bytes = 0; ctx->st.fold_launches = 0;
    if (ctx->profiling) prof_collect(ctx);
    for (size_t e = 0; e < ctx->ev_used; ++e) {
        if (ctx->ev_pool[e].kind != VP_K_SF && ctx->ev_pool[e].kind != -1) continue;
        float t = 0;
        hipEventElapsedTime(&t, ctx->ev_pool[e].a, ctx->ev_pool[e].b);
        ctx->st.fold_ms += t; ctx->st.fold_bytes += ctx->ev_pool[e].bytes; ++ctx->st.fold_launches;
    }
    if (n_written) *n_written = out_n * sizeof(F);
    return VP_OK;
}

// Index-split proof, caller-side exchange of the split phase-2 chains' V_u (include/vpgpu.h): this rank's partial inner products ...
int vp_shard_vu_partials(vp_ctx *ctx, const vp_F *tape_, uint64_t n_tape, vp_F *partials, uint64_t capacity, uint64_t *n_out) {
    if (!ctx || !has_circuit(ctx) || !ctx->evaluated || !n_out || (n_tape && !tape_) || n_tape != ctx->n_tape) return VP_EINVAL;
    if (!pred_canonical(tape_, n_tape)) { ctx->err = "vp_shard_vu_partials: a tape element is not canonical (limb >= 2^61 - 1)"; return VP_EINVAL; }
    VP_ENTER(ctx);
    *n_out = 0;
    ctx->vu_supplied = false;
    if (!(ctx->split_lw > 0 && ctx->shard_world > 1 && ctx->plan_path != 0 && ctx->opt.split_vu)) return VP_OK;       // nothing is split: nothing to exchange
    if (ctx->plan && ctx->plan_vreal != ctx->vreal) free_plan(ctx);
    if (!ctx->plan) VPCHK(build_plan(ctx));
    Plan &P = *ctx->plan;
    const u64 n = P.vu_layers.size();
    *n_out = n;
    if (!n) return VP_OK;
    if (!partials || capacity < n) return VP_EINVAL;
    HIPCHK(hipMemcpyAsync(ctx->d_tape, tape_, n_tape * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    VPCHK(vu_pre_dots(ctx, true));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(hipMemcpyAsync(partials, P.d_vu_sum, n * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->vu_pre_ms = 0;
    (void) hipEventElapsedTime(&ctx->vu_pre_ms, ctx->ev0, ctx->ev1);
    ctx->vu_tape_tag = tape_tag(tape_, n_tape);
    return VP_OK;
}
// ... and their u64 sum over the ranks, for the next vp_prove_gkr of this context (same tape)
int vp_shard_vu_set(vp_ctx *ctx, const vp_F *sums, uint64_t n) {
    if (!ctx || !has_circuit(ctx) || !ctx->evaluated || (n && !sums)) return VP_EINVAL;
    VP_ENTER(ctx);
    if (!(ctx->split_lw > 0 && ctx->shard_world > 1 && ctx->plan_path != 0 && ctx->opt.split_vu)) return n ? VP_EINVAL : VP_OK;
    if (ctx->plan && ctx->plan_vreal != ctx->vreal) free_plan(ctx);
    if (!ctx->plan) VPCHK(build_plan(ctx));
    if (n != ctx->plan->vu_layers.size()) { ctx->err = "vp_shard_vu_set: not the number of split phase-2 chains of this proof"; return VP_EINVAL; }
    if (!n) return VP_OK;
    HIPCHK(hipMemcpyAsync(ctx->plan->d_vu_sum, sums, n * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->vu_supplied = true;
    return VP_OK;
}

// Index-split proof without a communicator (rehearsal of W ranks on one GPU, or a caller with its own transport): `buf` holds the u64 sums
// of the ranks' vp_prove_gkr outputs (transcript + export area, vp_gkr_sizes bytes); reduces them mod p and finishes the split tables' last
// rounds with the tape of this context's last proof.  The first n_tr * 16 bytes of `buf` are then the transcript.
int vp_shard_finish(vp_ctx *ctx, uint8_t *buf, uint64_t n_bytes, uint64_t *n_transcript_bytes) {
    if (!ctx || !has_circuit(ctx) || !buf || !ctx->h_io) return VP_EINVAL;
    split_layout(ctx);
    const u64 n = ctx->n_tr + 3 * ctx->n_exp;
    if (n_bytes < n * sizeof(F)) return VP_EINVAL;
    u64 *w = reinterpret_cast<u64 *>(buf);
    for (u64 q = 0; q < 2 * n; ++q) w[q] = host_fold(w[q]);
    split_finish(ctx, reinterpret_cast<F *>(buf), ctx->h_io);
    if (n_transcript_bytes) *n_transcript_bytes = ctx->n_tr * sizeof(F);
    return VP_OK;
}

}  // extern "C"
