// Part of vpgpu.hip (included at its end): the Virgo commitment sharded over the GPUs of a node, and the RCCL transport.
// =====================================================================================================
// SURVEY.md §8e "PC sharding" / BASELINE.json north_star "FFT subtrees shard across the 8 GPUs".
//
// The 64 data slices of the commitment are independent transforms (lib/virgo/src/poly_commit.h:89-107); a leaf of the
// Merkle tree chains the values of ALL 64 slices at one position pair (lib/virgo/src/fri.cpp:81-124).  With W ranks:
//   * rank r transforms slices [r*64/W, (r+1)*64/W): iNTT + rate-1/32 encoding, everything of vpgpu_pc.inc on 64/W rows — the same code: PcShard
//     holds a PcSlices view of its own buffers (first = r*64/W, cap = rows = 64/W, the context's layout of `small` and `tmp`) and vp_commit_public(_eq)
//     runs pc_quotient_slices over it; this file adds what a shard needs around that: its share of the inner product, slice 0 for the tensor
//     check, the pack, the collectives and the trees;
//   * ONE all-to-all per committed oracle (l, h, and the virtual oracle the FRI folds start from) turns slice ownership
//     into POSITION ownership: rank r' receives, for every slice and coset, the positions a = a'*W + r'.  Ownership by the
//     low bits of a (not a contiguous range) is what keeps every later step local: a leaf pairs (a, a + N/2), a FRI fold
//     pairs (a, a + N_k/2) — partners share their low bits at every level — and locally the data look exactly like an
//     unsharded codeword of N/W positions per coset, so the leaf-hash, fold and tree kernels run unchanged;
//   * a rank hashes its leaves and the five tree levels above them (the 32 cosets of one position are adjacent leaves
//     32a .. 32a+31); the level-5 nodes (1/32 of the leaf digests) are all-gathered and every rank builds the top of the
//     tree: all ranks know the root, any rank can answer the upper part of an opening;
//   * the FRI commit phase folds locally until one position per rank is left, all-gathers that 64 x 32 x W tail together
//     with the level-5 nodes of every level, and finishes the last log2 W levels redundantly on every rank.
//     vp_fri_step takes the challenges one by one instead (pcs_fri_step): the same folds and hashes, one all-gather per local level.
// Bytes on the wire for an input layer of 2^n wires: each all-to-all moves 64*2^(n-1)*16 B in total ((W-1)/W of it leaves
// its GPU): n = 23, W = 8: 4.3 GB per oracle, 67 MB per ordered pair of GPUs; the all-gathers move 2^(n-7)*32 B (2 MB at n = 23).
//
// Transport.  Inside a node the collectives run over RCCL (vp_comm_init; resolved from librccl.so.1 at run time, RTLD_LOCAL: a process
// that imported PyTorch BEFORE this library already holds PyTorch's HIP runtime and RCCL under the same sonames and shares that ONE copy;
// a process that loads this library first and PyTorch afterwards ends up with two ROCm stacks — keeping ours out of the global symbol
// scope stops their same-named globals, e.g. rocm_smi's tables, from being constructed and destroyed twice).  Without a communicator a sharded call stops at each collective and returns
// VP_EXCHANGE; vp_shard_exchange_local performs the pending collectives among W contexts of ONE process (device-to-device copies)
// — how the parity tests run W ranks on the single GPU of the test box.
// Every sharded call is a state machine over stages: a stage ends in pcs_stage_end (collectives done, or pending with the clock paused), a call in pcs_finish.
// =====================================================================================================
#include <dlfcn.h>

struct PcShard {
    int rank = 0, world = 1, lw = 0, S = 64;
    int op = 0, stage = 0;                                  // call in flight: 1 commit_private, 2 commit_public, 3 fri_commit
    // own slices, unsharded layout [S][32][N]: the buffers pc_quotient_slices and the virtual oracle work in (allocated by pcs_alloc, laid out like the
    // context's own; v.slice0 holds slice 0 of the public vector for the tensor check and the one-slice encoding, v.pub sits N behind it)
    PcSlices v;
    // every slice, own positions: [64][32][N/W]
    F *l_loc = nullptr, *h_loc = nullptr, *fri_loc = nullptr;                                   // fri_loc: level 0 input, then every locally folded level
    Dig *tree_l = nullptr, *tree_h = nullptr, *tree_f = nullptr;                                // local leaves + five levels (heap layout of the local leaf order)
    Dig *top_l = nullptr, *top_h = nullptr, *top_f = nullptr;                                   // global trees from level 5 up (every rank holds them)
    F *tail = nullptr; Dig *tail_tree = nullptr;                                                // the last log2 W + 1 FRI levels, whole
    FriLayout fl;                                                                               // where a FRI level sits in fri_loc, tree_f, top_f, tail, tail_tree (vp_pc_set_shard)
    F *send = nullptr; size_t send_cap = 0;
    unsigned char *ag_send = nullptr, *ag_recv = nullptr; size_t ag_cap = 0;
    Dig *d_roots = nullptr;
    int n_steps = 0;
    int f_done = 0, f_mode = 0;                             // FRI levels committed (openable); how: 0 none yet, 1 one pass (vp_fri_commit), 2 step by step (vp_fri_step)
    F step_r;                                               // the vp_fri_step in flight: its challenge
    float acc_ms = 0;                                       // the call in flight: device time of its parts before the collectives it stopped at
    F *eq = nullptr; F pt[32];                              // vp_commit_public_eq: point | two eq half tables on the device; the point of the call in flight
    std::vector<F> fri_r;
    bool private_done = false, public_done = false;
    struct X { int kind; const void *send; void *recv; size_t bytes; } x[2];               // kind 1: all-to-all (bytes per peer), 2: all-gather (bytes per rank)
    int nx = 0;
};
// RCCL communicator of the context (resolved with dlopen at vp_comm_init).  The library is not linked, but the datatype / reduction codes handed to it
// are the enumerators of the RCCL header this library is BUILT against (rccl/rccl.h of the ROCm tree), not literals.
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
constexpr int VP_NCCL_INT8 = (int) ncclInt8, VP_NCCL_UINT64 = (int) ncclUint64, VP_NCCL_SUM = (int) ncclSum;
#else           // a ROCm tree without the RCCL development header: the values of rccl.h 2.x (NCCL's public ABI since 2.0)
constexpr int VP_NCCL_INT8 = 0, VP_NCCL_UINT64 = 5, VP_NCCL_SUM = 0;
#endif
struct VpComm {
    void *lib = nullptr, *comm = nullptr; int rank = 0, world = 1;
    int (*fn_allgather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*fn_allreduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*fn_send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*fn_recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*fn_group_start)() = nullptr;
    int (*fn_group_end)() = nullptr;
    int (*fn_comm_destroy)(void *) = nullptr;
};
extern "C" bool vp_comm_attached(const vp_ctx *ctx) { return ctx && ctx->cm && ctx->cm->comm; }
extern "C" bool vp_comm_matches(const vp_ctx *ctx, int rank, int world) { return ctx && ctx->cm && ctx->cm->comm && ctx->cm->rank == rank && ctx->cm->world == world; }
void vp_free_shard_state(vp_ctx *ctx) { delete ctx->pcs; ctx->pcs = nullptr; }
bool vp_pc_shard_pending(const vp_ctx *ctx) { return ctx->pcs && ctx->pcs->nx; }
void vp_free_comm(vp_ctx *ctx) {
    if (ctx->cm) { if (ctx->cm->comm && ctx->cm->fn_comm_destroy) ctx->cm->fn_comm_destroy(ctx->cm->comm); delete ctx->cm; ctx->cm = nullptr; }
}

namespace {

__global__ void __launch_bounds__(VP_BLOCK) k_pc_pack(const F *__restrict__ in, F *__restrict__ out, u32 N, int lw, u32 rows) {
    // in: [rows][N] (row = own slice * 32 + coset); out: [dest rank][rows][N >> lw] with position a = a' * W + dest
    const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t) rows * N) return;
    const u32 a = (u32) (t % N), row = (u32) (t / N), d = a & ((1u << lw) - 1), al = a >> lw, Nl = N >> lw;
    out[((size_t) d * rows + row) * Nl + al] = in[t];
}
__global__ void __launch_bounds__(VP_BLOCK) k_pc_interleave_dig(const Dig *__restrict__ in, Dig *__restrict__ out, u32 per_rank, int lw) {
    // in: [rank][a'] level-5 nodes as gathered; out[a' * W + rank]: the global order
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (per_rank << lw)) return;
    const u32 r = t / per_rank, al = t % per_rank;
    out[(al << lw) + r] = in[t];
}
__global__ void __launch_bounds__(VP_BLOCK) k_pc_interleave_tail(const F *__restrict__ in, F *__restrict__ out, int lw) {
    // in: [rank][slice*32 + coset] (one position per rank); out: [slice*32 + coset][a = rank]
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (2048u << lw)) return;
    const u32 r = t / 2048, sb = t % 2048;
    out[((size_t) sb << lw) + r] = in[t];
}
__global__ void __launch_bounds__(VP_BLOCK) k_pc_sum_gathered(const F *__restrict__ in, u32 stride, u32 n, F *out) {     // out = sum_r in[r * stride], n ranks
    if (threadIdx.x || blockIdx.x) return;
    F s = f_zero();
    for (u32 r = 0; r < n; ++r) s = f_add(s, in[(size_t) r * stride]);
    *out = s;
}

// vp_commit_public_eq on a shard: entries [base, base + count) of the eq table from its two half tables (k_beta_expand with an offset) ...
__global__ void __launch_bounds__(VP_BLOCK) k_pc_eq_range(const F *__restrict__ bf, const F *__restrict__ bs, int h1, u64 base, u32 count, F *__restrict__ out) {
    const u32 mask = (1u << h1) - 1;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const u64 g = base + i;
        out[i] = f_mul(bf[(u32) g & mask], bs[(u32) (g >> h1)]);
    }
}
// ... and k_pc_dot against that range without storing it: x streams from HBM, the half tables (2^(n/2) entries each) stay in L2
__global__ void __launch_bounds__(VP_BLOCK) k_pc_dot_eq(const F *__restrict__ x, const F *__restrict__ bf, const F *__restrict__ bs, int h1, u64 base, u32 n, F *part) {
    __shared__ F lds[4];
    const u32 mask = (1u << h1) - 1;
    F acc[1] = {f_zero()};
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const u64 g = base + i;
        acc[0] = f_add(acc[0], f_mul(x[i], f_mul(bf[(u32) g & mask], bs[(u32) (g >> h1)])));
    }
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// a pending gather of the round shard (vp_set_round_shard) and a commitment collective cannot both be open on one context
int pcs_guard(vp_ctx *ctx) {
    if (ctx->rsh && ctx->rsh->nx) { ctx->err = "sharded commitment: a round-shard gather is pending on this context"; return VP_EINVAL; }
    return VP_OK;
}

// A call stops at a collective the caller performs (VP_EXCHANGE): the device time of the part that ends here counts towards vp_commit_stats, the wait for
// the exchange (with several ranks on one GPU: the other ranks' work) does not.  pcs_resume starts the next part's clock.
int pcs_pause(vp_ctx *ctx) {
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    VPCHK(check_stream(ctx));
    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1); ctx->pcs->acc_ms += ms;
    return VP_OK;
}
int pcs_resume(vp_ctx *ctx) {
    if (ctx->pcs->stage == 0) ctx->pcs->acc_ms = 0;
    else HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    return VP_OK;
}
int pcs_collectives(vp_ctx *ctx);
// A stage ends: its collectives are performed (VP_OK: the next stage follows) or left pending with the clock paused (VP_EXCHANGE: the caller exchanges)
int pcs_stage_end(vp_ctx *ctx) {
    const int rc = pcs_collectives(ctx);
    if (rc == VP_EXCHANGE) VPCHK(pcs_pause(ctx));
    return rc;
}
// A call ends: the clock stops, the results start their way to the host, the stream drains; device time = the parts before the collectives + this one
struct PcsOut { void *dst; const void *src; size_t bytes; };
int pcs_finish(vp_ctx *ctx, std::initializer_list<PcsOut> outs) {
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    for (const PcsOut &o : outs) HIPCHK(hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
    VPCHK(check_stream(ctx));
    if (ctx->profiling) prof_collect(ctx);
    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1); ctx->commit_ms = ctx->pcs->acc_ms + ms;
    ctx->pcs->op = 0; ctx->pcs->stage = 0;
    return VP_OK;
}

// five tree levels above the local leaves (local leaf order 32a' + b: the 32 cosets of a position are one subtree)
int pcs_local_levels(vp_ctx *ctx, Dig *tree, u32 n_leaves) {
    MerkleArgs ma{};
    ma.tree[0] = tree; ma.count[0] = n_leaves; ma.n = 1;
    return pc_merkle_trees(ctx, ma, nullptr, 5);
}

// the collectives a stage ends with: over RCCL when a communicator is attached, otherwise left pending for vp_shard_exchange_local
int pcs_collectives(vp_ctx *ctx) {
    PcShard &s = *ctx->pcs;
    if (!ctx->cm || !ctx->cm->comm) return VP_EXCHANGE;
    VpComm &c = *ctx->cm;
    if (c.world != s.world || c.rank != s.rank) { ctx->err = "communicator and commitment shard disagree on rank / world"; return VP_EINVAL; }
    for (int i = 0; i < s.nx; ++i) {
        const PcShard::X &x = s.x[i];
        if (x.kind == 2) {
            if (c.fn_allgather(x.send, x.recv, x.bytes, VP_NCCL_INT8, c.comm, ctx->stream)) { ctx->err = "ncclAllGather failed"; return VP_EHIP; }
        } else {
            c.fn_group_start();
            int rc = 0;
            for (int p = 0; p < s.world; ++p) {
                rc |= c.fn_send((const char *) x.send + (size_t) p * x.bytes, x.bytes, VP_NCCL_INT8, p, c.comm, ctx->stream);
                rc |= c.fn_recv((char *) x.recv + (size_t) p * x.bytes, x.bytes, VP_NCCL_INT8, p, c.comm, ctx->stream);
            }
            rc |= c.fn_group_end();
            if (rc) { ctx->err = "RCCL all-to-all failed"; return VP_EHIP; }
        }
    }
    s.nx = 0;
    return VP_OK;
}

int pcs_alloc(vp_ctx *ctx, int ln, int lm) {
    PcShard &s = *ctx->pcs;
    PcSlices &v = s.v;
    if (v.coef) return VP_OK;
    const size_t N = (size_t) 1 << ln, Nl = N >> s.lw, S = s.S;
    v.first = (u32) (s.rank * s.S); v.cap = v.rows = (u32) S; v.N = (u32) N;
    VPCHK(dalloc(ctx, &v.coef, S * N));
    VPCHK(dalloc(ctx, &v.lcw, S * 32 * N)); VPCHK(dalloc(ctx, &v.qcw, S * 32 * N)); VPCHK(dalloc(ctx, &v.hcw, S * 32 * N));
    VPCHK(dalloc(ctx, &v.tmp, 3 * 2 * S * N)); VPCHK(dalloc(ctx, &v.small, (size_t) 1024 + 160 + 64));       // (as pc_public_alloc)
    VPCHK(dalloc(ctx, &v.slice0, (S + 1) * N));               // [slice 0][own slices]
    v.pub = v.slice0 + N;
    VPCHK(dalloc(ctx, &v.q0, 32 * N)); VPCHK(dalloc(ctx, &v.flag, (size_t) 1));
    VPCHK(dalloc(ctx, &s.eq, (size_t) 32 + 2 * ((size_t) 1 << ((ln + 6 + 1) / 2))));       // point | two eq half tables (as pc_public_alloc)
    VPCHK(dalloc(ctx, &s.send, S * 32 * N)); s.send_cap = S * 32 * N;
    VPCHK(dalloc(ctx, &s.l_loc, 64 * 32 * Nl)); VPCHK(dalloc(ctx, &s.h_loc, 64 * 32 * Nl)); VPCHK(dalloc(ctx, &s.fri_loc, 2 * 64 * 32 * Nl));
    VPCHK(dalloc(ctx, &s.tree_l, 32 * Nl)); VPCHK(dalloc(ctx, &s.tree_h, 32 * Nl)); VPCHK(dalloc(ctx, &s.tree_f, 32 * Nl));       // 2 * n_leaves_local, n_leaves_local = 16 Nl
    VPCHK(dalloc(ctx, &s.top_l, N)); VPCHK(dalloc(ctx, &s.top_h, N)); VPCHK(dalloc(ctx, &s.top_f, N));                             // heap over N/2 level-5 nodes (and the shorter FRI levels)
    VPCHK(dalloc(ctx, &s.tail, (size_t) 4 * 2048 << s.lw)); VPCHK(dalloc(ctx, &s.tail_tree, (size_t) 4 * 32 << s.lw));
    VPCHK(dalloc(ctx, &s.d_roots, (size_t) VP_FRI_MAX));
    const size_t ag = std::max<size_t>((N / 2) * 32 * 2 + 2048 * 16 * 4, 4096) * 2;       // level-5 nodes of every level (geometric) + tail + sums
    VPCHK(dalloc(ctx, &s.ag_send, ag)); VPCHK(dalloc(ctx, &s.ag_recv, ag << s.lw)); s.ag_cap = ag;
    return VP_OK;
}

// leaves + five levels on the local codeword, level-5 nodes staged for the all-gather (appended at ag offset `at`)
int pcs_hash_local(vp_ctx *ctx, const F *cw_loc, u32 Nl, Dig *tree, size_t at) {
    PcShard &s = *ctx->pcs;
    const u32 n_leaves = 16 * Nl;                                              // Nl >= 2
    FriLeafArgs la{};
    la.cw[0] = cw_loc; la.leaves[0] = tree + n_leaves; la.N[0] = Nl; la.n = 1;
    VPCHK(pc_hash_leaves(ctx, la, true));
    VPCHK(pcs_local_levels(ctx, tree, n_leaves));
    HIPCHK(hipMemcpyAsync(s.ag_send + at, tree + (Nl >> 1), (size_t) (Nl >> 1) * 32, hipMemcpyDeviceToDevice, ctx->stream));        // level with Nl/2 nodes
    return VP_OK;
}
// gathered level-5 nodes ([rank][Nl/2]) -> global order at the leaves of `top` (N_glob/2 nodes), then the rest of the tree
int pcs_top(vp_ctx *ctx, const unsigned char *gathered, size_t stride, size_t at, u32 Nl, Dig *top) {
    PcShard &s = *ctx->pcs;
    const u32 per = Nl >> 1, n5 = per << s.lw;
    // the all-gather delivers [rank][whole staging buffer]: this level sits at offset `at` inside every rank's part -> compact it first
    Dig *tmpd = reinterpret_cast<Dig *>(s.send);
    for (int r = 0; r < s.world; ++r)
        HIPCHK(hipMemcpyAsync(tmpd + (size_t) r * per, gathered + (size_t) r * stride + at, (size_t) per * 32, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pc_interleave_dig, dim3(nblk(n5)), dim3(VP_BLOCK), 0, ctx->stream, tmpd, top + n5, per, s.lw);
    if (n5 >= 2) VPCHK(pc_merkle(ctx, top, n5));
    return VP_OK;
}

int pcs_commit_private(vp_ctx *ctx, uint8_t root[32]) {
    PcShard &s = *ctx->pcs;
    const int n = ctx->L[0].bl, ln = n - 6, lm = n - 1;
    const u32 N = 1u << ln, Nl = N >> s.lw;
    VPCHK(pcs_guard(ctx));
    if (s.op != 1) { s.op = 1; s.stage = 0; }
    VPCHK(pcs_resume(ctx));
    for (;;) {
        if (s.stage == 0) {
            VPCHK(pc_root_table(ctx, lm));
            VPCHK(pcs_alloc(ctx, ln, lm));
            ctx->ev_used = 0;
            HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
            const F *in = ctx->L[0].val + (size_t) s.rank * s.S * N;
            VPCHK(pc_launch_ntt(ctx, in, s.v.coef, ln, lm, 1, s.S, 1, N));
            VPCHK(pc_launch_ntt(ctx, s.v.coef, s.v.lcw, ln, lm, 0, s.S, 32, N));
            hipLaunchKernelGGL(k_pc_pack, dim3(nblk((u64) s.S * 32 * N)), dim3(VP_BLOCK), 0, ctx->stream, s.v.lcw, s.send, N, s.lw, (u32) s.S * 32);
            s.x[0] = {1, s.send, s.l_loc, (size_t) s.S * 32 * Nl * sizeof(F)}; s.nx = 1;
            s.stage = 1;
            VPCHK(pcs_stage_end(ctx));
        } else if (s.stage == 1) {
            VPCHK(pcs_hash_local(ctx, s.l_loc, Nl, s.tree_l, 0));
            s.x[0] = {2, s.ag_send, s.ag_recv, (size_t) (Nl >> 1) * 32}; s.nx = 1;
            s.stage = 2;
            VPCHK(pcs_stage_end(ctx));
        } else {
            VPCHK(pcs_top(ctx, s.ag_recv, (size_t) (Nl >> 1) * 32, 0, Nl, s.top_l));
            VPCHK(pcs_finish(ctx, {{root, s.top_l + 1, 32}}));
            s.private_done = true;
            return VP_OK;
        }
    }
}

// vp_commit_public (pub: the whole vector on the host) or vp_commit_public_eq (pub == nullptr, point: n coordinates, checked by the caller).  With a point
// nothing of the public vector crosses PCIe and none of it is stored: an eq table is a tensor by construction, so the rank needs slice 0 (the first N
// entries, expanded from the two half tables), the 64 scalars eq(r_hi, i) / eq(r_hi, 0) (formed on the host from the point) and its share of
// <V_0, eq(point, .)>, which k_pc_dot_eq takes from the half tables entry by entry.  The outputs are the field elements vp_commit_public gives for the table.
int pcs_commit_public(vp_ctx *ctx, const vp_F *pub, uint64_t n_pub, const vp_F *point, vp_F *inner, vp_F all_sum[65], uint8_t root_h[32]) {
    PcShard &s = *ctx->pcs;
    const int n = ctx->L[0].bl;
    const u32 N = 1u << (n - 6), Nl = N >> s.lw, S = (u32) s.S;
    if (!s.private_done || (pub && n_pub != (1ull << n))) return VP_EINVAL;
    VPCHK(pcs_guard(ctx));
    if (s.op != 2) { s.op = 2; s.stage = 0; }
    VPCHK(pcs_resume(ctx));
    const size_t sums_at = (size_t) (Nl >> 1) * 32;                      // staging layout of stage 1: [level-5 nodes][66 sums]
    for (;;) {
        if (s.stage == 0) {
            s.f_done = 0; s.f_mode = 0; s.n_steps = 0;                   // the FRI phase of an earlier public vector is gone
            const int h1 = n >> 1;
            F *dr = s.eq, *dbf = s.eq + 32, *dbs = dbf + ((size_t) 1 << ((n + 1) / 2));
            PcSlices &v = s.v;
            const F *hp = reinterpret_cast<const F *>(pub);
            if (pub) HIPCHK(hipMemcpyAsync(v.pub, hp + (size_t) v.first * N, (size_t) S * N * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
            else {
                for (int i = 0; i < n; ++i) s.pt[i] = f_make(point[i].real, point[i].img);
                s.pt[n] = f_one();
                HIPCHK(hipMemcpyAsync(dr, s.pt, (size_t) (n + 1) * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
            }
            ctx->ev_used = 0;
            HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
            // partial inner product over this rank's slices (slice i = input wires [i N, (i+1) N))
            const u64 lo = (u64) v.first * N, used = ctx->L[0].size > lo ? std::min<u64>(ctx->L[0].size - lo, (u64) S * N) : 0;
            const u32 g = std::max<u32>(1, std::min<u32>(1024, nblk(used)));
            if (pub) PC_PROF(VP_K_PC_POINTWISE, g, 1, 32ull * used, used, hipLaunchKernelGGL(k_pc_dot, dim3(g), dim3(VP_BLOCK), 0, ctx->stream, ctx->L[0].val + lo, v.pub, (u32) used, v.small));
            else {
                hipLaunchKernelGGL(k_beta_half, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, (const F *) dr, n, (const F *) (dr + n), dbf, dbs);
                PC_PROF(VP_K_PC_POINTWISE, g, 1, 16ull * used, used,
                        hipLaunchKernelGGL(k_pc_dot_eq, dim3(g), dim3(VP_BLOCK), 0, ctx->stream, ctx->L[0].val + lo, (const F *) dbf, (const F *) dbs, h1, lo, (u32) used, v.small));
            }
            hipLaunchKernelGGL(k_pc_sum_parts, dim3(1), dim3(VP_BLOCK), 0, ctx->stream, v.small, g, v.d_inner());
            // What pc_quotient_slices needs on the device besides the rank's slices: slice 0, if the one-slice encoding can apply (checked there for THIS
            // rank's slices against it).  Of an eq table, a tensor by construction: slice 0 expanded from the half tables and nothing else, or, with
            // the encoding switched off, every slice of this rank as a vector handed in would be.
            F corner[64];                                                // corner[i] = pub[i N]; of an eq table: the host's own product
            if (pub) for (int i = 0; i < 64; ++i) corner[i] = hp[(size_t) i * N];
            else pc_eq_corners(s.pt, n, corner);
            const bool cand = pc_tensor_candidate(ctx, corner);
            if (pub) { if (cand) HIPCHK(hipMemcpyAsync(v.slice0, hp, (size_t) N * sizeof(F), hipMemcpyHostToDevice, ctx->stream)); }
            else if (cand) hipLaunchKernelGGL(k_beta_expand, dim3(grid_for(N)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) dbf, (const F *) dbs, h1, N, v.slice0);
            else PC_PROF(VP_K_PC_POINTWISE, grid_for((u64) S * N), 1, 16ull * S * N, (u64) S * N,
                         hipLaunchKernelGGL(k_pc_eq_range, dim3(grid_for((u64) S * N)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) dbf, (const F *) dbs, h1, lo, S * N, v.pub));
            VPCHK(pc_quotient_slices(ctx, v, corner, pub ? 0 : 1));
            hipLaunchKernelGGL(k_pc_pack, dim3(nblk((u64) S * 32 * N)), dim3(VP_BLOCK), 0, ctx->stream, v.hcw, s.send, N, s.lw, S * 32);
            s.x[0] = {1, s.send, s.h_loc, (size_t) S * 32 * Nl * sizeof(F)}; s.nx = 1;
            s.stage = 1;
            VPCHK(pcs_stage_end(ctx));
        } else if (s.stage == 1) {
            VPCHK(pcs_hash_local(ctx, s.h_loc, Nl, s.tree_h, 0));
            // this rank's all_sum entries and its share of the inner product ride on the same all-gather
            HIPCHK(hipMemcpyAsync(s.ag_send + sums_at, s.v.d_all(), (size_t) S * sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(s.ag_send + sums_at + (size_t) S * sizeof(F), s.v.d_inner(), sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
            s.x[0] = {2, s.ag_send, s.ag_recv, sums_at + (size_t) (S + 1) * sizeof(F)}; s.nx = 1;
            s.stage = 2;
            VPCHK(pcs_stage_end(ctx));
        } else {
            const size_t stride = sums_at + (size_t) (S + 1) * sizeof(F);
            VPCHK(pcs_top(ctx, s.ag_recv, stride, 0, Nl, s.top_h));
            F *g_all = s.v.tmp, *g_inner = s.v.tmp + 80;                   // tmp is free again
            hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(128), 0, ctx->stream, g_all, 66u);
            for (int r = 0; r < s.world; ++r)
                HIPCHK(hipMemcpyAsync(g_all + (size_t) r * S, s.ag_recv + (size_t) r * stride + sums_at, (size_t) S * sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pc_sum_gathered, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const F *>(s.ag_recv + sums_at + (size_t) S * sizeof(F)),
                               (u32) (stride / sizeof(F)), (u32) s.world, g_inner);
            VPCHK(pcs_finish(ctx, {{root_h, s.top_h + 1, 32}, {inner, g_inner, sizeof(F)}, {all_sum, g_all, 65 * sizeof(F)}}));
            s.public_done = true;
            return VP_OK;
        }
    }
}

// Stage 0 of the sharded FRI phase: the virtual oracle of the own slices (in place over q), packed for the all-to-all that turns it into position ownership
void pcs_fri_stage0(vp_ctx *ctx) {
    PcShard &s = *ctx->pcs;
    const u32 N = (u32) s.fl.N, M = 32 * N, Nl = (u32) s.fl.Nl, S = (u32) s.S;
    const PcSlices &v = s.v;
    hipLaunchKernelGGL(k_pc_virtual_oracle, dim3(nblk((u64) S * M)), dim3(VP_BLOCK), 0, ctx->stream, v.lcw, v.qcw, v.hcw, v.S0(), N,
                       ctx->pc_rt, M >> 1, f_make(N, 0), S, v.q0_arg(), v.qs_arg());
    hipLaunchKernelGGL(k_pc_pack, dim3(nblk((u64) S * 32 * N)), dim3(VP_BLOCK), 0, ctx->stream, v.qcw, s.send, N, s.lw, S * 32);
    s.x[0] = {1, s.send, s.fri_loc, (size_t) S * 32 * Nl * sizeof(F)}; s.nx = 1;
    s.stage = 1;
}
// local fold k < n_local: the rank's positions of level k - 1 (k = 0: of the virtual oracle) to its positions of level k; returns them
F *pcs_local_fold(vp_ctx *ctx, int k, F r) {
    PcShard &s = *ctx->pcs;
    const u32 M = 32 * (u32) s.fl.N, Nk = (u32) s.fl.Nl >> k, No = Nk >> 1;
    F *out = s.fri_loc + s.fl.loc_cw(k);
    PC_PROF(VP_K_FRI_FOLD, nblk((u64) 64 * 32 * No), 1, 48ull * 64 * 32 * No, (u64) 3 * 64 * 32 * No,
            hipLaunchKernelGGL(k_fri_fold, dim3(nblk((u64) (64 / VP_FOLD_SPT) * 32 * No)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) (s.fri_loc + s.fl.loc_in(k)), out, Nk, k,
                               ctx->pc_rt, M >> 1, r, host_inv_real(2), s.lw, (u32) s.rank, 64u));
    return out;
}
// One replicated tail step: level k - 1 (whole on every rank) folds to level k > n_local - 1, which is hashed; returns the level's tree (the root is node 1)
int pcs_tail_step(vp_ctx *ctx, int k, F r, Dig **tree_out) {
    PcShard &s = *ctx->pcs;
    const int q = s.fl.tail_q(k);
    const u32 M = 32 * (u32) s.fl.N, Nt = (u32) s.fl.tail_per_coset(q - 1), Nn = Nt >> 1;
    F *out = s.tail + s.fl.tail_cw(q);
    Dig *tree = s.tail_tree + s.fl.tail_tree(q);
    hipLaunchKernelGGL(k_fri_fold, dim3(nblk((u64) (64 / VP_FOLD_SPT) * 32 * Nn)), dim3(VP_BLOCK), 0, ctx->stream, (const F *) (s.tail + s.fl.tail_cw(q - 1)), out, Nt, k, ctx->pc_rt, M >> 1,
                       r, host_inv_real(2), 0, 0u, 64u);
    VPCHK(pc_hash_level(ctx, out, Nn, nullptr, tree));
    *tree_out = tree;
    return VP_OK;
}

int pcs_fri_commit(vp_ctx *ctx, const vp_F *r, int n_steps, uint8_t *roots) {
    PcShard &s = *ctx->pcs;
    const FriLayout &fl = s.fl;
    const int ln = fl.ln, n_local = fl.n_local();                        // n_local: folds whose partners are on this rank: N_k -> N_k/2 while N_k >= 2W
    if (!s.public_done || n_steps != ln) { ctx->err = "sharded vp_fri_commit: all n-6 steps in one call, after vp_commit_public"; return VP_EINVAL; }
    if (s.f_mode == 2) { ctx->err = "vp_fri_commit after vp_fri_step"; return VP_EINVAL; }
    VPCHK(pcs_guard(ctx));
    if (s.op != 3) { s.op = 3; s.stage = 0; }
    VPCHK(pcs_resume(ctx));
    for (;;) {
        if (s.stage == 0) {
            s.fri_r.assign(reinterpret_cast<const F *>(r), reinterpret_cast<const F *>(r) + n_steps);
            s.f_done = 0;
            ctx->ev_used = 0;
            HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
            pcs_fri_stage0(ctx);
            VPCHK(pcs_stage_end(ctx));
        } else if (s.stage == 1) {
            // local folds; level k's output has Nl >> (k+1) positions per coset here
            FriLeafArgs la{};
            for (int k = 0; k < n_local; ++k) {
                F *out = pcs_local_fold(ctx, k, s.fri_r[k]);
                if (!fl.is_tail(k)) {                                      // leaves pair (a', a' + No/2): local
                    const u32 No = (u32) fl.loc_per_coset(k);
                    la.cw[la.n] = out; la.leaves[la.n] = s.tree_f + fl.loc_tree(k) + 16 * No; la.N[la.n] = No; ++la.n;
                }
            }
            VPCHK(pc_hash_leaves(ctx, la, true));
            size_t at = 0;
            for (int q = 0; q < la.n; ++q) {
                const u32 No = la.N[q];
                Dig *tree = s.tree_f + fl.loc_tree(q);
                VPCHK(pcs_local_levels(ctx, tree, 16 * No));
                HIPCHK(hipMemcpyAsync(s.ag_send + at, tree + (No >> 1), (size_t) (No >> 1) * 32, hipMemcpyDeviceToDevice, ctx->stream));
                at += (size_t) (No >> 1) * 32;
            }
            // the one position per coset this rank is left with (output of the last local fold)
            HIPCHK(hipMemcpyAsync(s.ag_send + at, s.fri_loc + fl.loc_cw(n_local - 1), (size_t) 2048 * sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
            at += (size_t) 2048 * sizeof(F);
            s.x[0] = {2, s.ag_send, s.ag_recv, at}; s.nx = 1;
            s.n_steps = n_steps;
            s.stage = 2;
            VPCHK(pcs_stage_end(ctx));
        } else {
            // top trees of the locally hashed levels
            size_t at = 0, stride = 0;
            for (int k = 0; !fl.is_tail(k); ++k) stride += (size_t) (fl.loc_per_coset(k) >> 1) * 32;
            const size_t tail_at = stride;
            stride += (size_t) 2048 * sizeof(F);
            for (int k = 0; !fl.is_tail(k); ++k) {
                const u32 No = (u32) fl.loc_per_coset(k);
                Dig *top = s.top_f + fl.top(k);
                VPCHK(pcs_top(ctx, s.ag_recv, stride, at, No, top));
                HIPCHK(hipMemcpyAsync(s.d_roots + k, top + 1, 32, hipMemcpyDeviceToDevice, ctx->stream));        // heap layout: the root is node 1
                at += (size_t) (No >> 1) * 32;
            }
            // the tail: level n_local-1's output (W positions per coset) and the last lw folds, whole codewords on every rank
            // (gathered rank by rank behind the tail's own levels: the tail buffer has 2048 (2 W + 1) elements to spare there, while the send buffer,
            // 2048 N / W elements, is shorter than the W x 2048 gathered ones once N < W^2)
            F *tmpf = s.tail + fl.tail_gather();
            for (int q = 0; q < s.world; ++q)
                HIPCHK(hipMemcpyAsync(tmpf + (size_t) q * 2048, s.ag_recv + (size_t) q * stride + tail_at, (size_t) 2048 * sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pc_interleave_tail, dim3(nblk(2048u << s.lw)), dim3(VP_BLOCK), 0, ctx->stream, tmpf, s.tail, s.lw);
            Dig *tree = s.tail_tree;
            VPCHK(pc_hash_level(ctx, s.tail, (u32) fl.W, nullptr, tree));
            for (int k = n_local - 1;; ++k) {
                HIPCHK(hipMemcpyAsync(s.d_roots + k, tree + 1, 32, hipMemcpyDeviceToDevice, ctx->stream));
                if (k + 1 == n_steps) break;
                VPCHK(pcs_tail_step(ctx, k + 1, s.fri_r[k + 1], &tree));
            }
            VPCHK(pcs_finish(ctx, {{roots, s.d_roots, (size_t) 32 * n_steps}}));
            s.f_done = n_steps; s.f_mode = 1;
            return VP_OK;
        }
    }
}

// vp_fri_step on a sharded commitment: pcs_fri_commit cut along its levels, one call per fold challenge (the drop-in's commit_phase loop,
// vpd_verifier.cpp:44-74).  Step k commits level k and returns its root, the unsharded one, on every rank:
//   * step 0 begins with the virtual oracle and its all-to-all to position ownership;
//   * a step k < n_local = (n - 6) - log2 W folds locally and ends in ONE all-gather: the level-5 nodes of the level while the rank keeps at least two
//     positions per coset, the 2048 tail elements at the last local step (k = n_local - 1), whose level every rank then holds whole and hashes itself;
//   * a step k >= n_local folds and hashes the replicated tail: no collective.
// 1 + n_local collectives in all (the one-pass form needs 2: it knows every challenge and gathers all levels at once).  Without a communicator the call
// stops at each collective with VP_EXCHANGE and is repeated with the same r after the exchange; a repeat before the exchange changes nothing.
int pcs_fri_step(vp_ctx *ctx, const vp_F *r, uint8_t root[32]) {
    PcShard &s = *ctx->pcs;
    const FriLayout &fl = s.fl;
    const int ln = fl.ln, n_local = fl.n_local();
    if (!s.public_done) { ctx->err = "vp_fri_step: vp_commit_public first"; return VP_EINVAL; }
    if (s.op != 0 && s.op != 4) { ctx->err = "vp_fri_step: another call of the sharded commitment is unfinished"; return VP_EINVAL; }
    if (s.f_mode == 1) { ctx->err = "vp_fri_step after vp_fri_commit"; return VP_EINVAL; }
    VPCHK(pcs_guard(ctx));
    if (s.op == 4 && s.nx) return VP_EXCHANGE;                            // the collective this step waits for has not been performed
    const int k = s.f_done;
    if (s.op != 4) {
        if (k >= ln) { ctx->err = "FRI commit phase already finished"; return VP_EINVAL; }
        memcpy(&s.step_r, r, sizeof(F));
        s.acc_ms = 0; ctx->ev_used = 0;
        if (k == 0) { s.f_mode = 2; s.n_steps = ln; }
        s.op = 4; s.stage = k == 0 ? 0 : k < n_local ? 1 : 3;
    }
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    const u32 No = k < n_local ? (u32) fl.loc_per_coset(k) : 0;           // local step: positions per coset on this rank after the fold
    Dig *tree = nullptr;                                                   // the level's tree (heap layout: the root is node 1)
    for (;;) {
        if (s.stage == 0) {
            pcs_fri_stage0(ctx);
            VPCHK(pcs_stage_end(ctx));
        } else if (s.stage == 1) {
            F *out = pcs_local_fold(ctx, k, s.step_r);
            if (!fl.is_tail(k)) {                                         // leaves pair (a', a' + No/2): local; the level-5 nodes go to every rank
                VPCHK(pcs_hash_local(ctx, out, No, s.tree_f + fl.loc_tree(k), 0));
                s.x[0] = {2, s.ag_send, s.ag_recv, (size_t) (No >> 1) * 32}; s.nx = 1;
            } else {                                                       // the one position per coset this rank is left with
                HIPCHK(hipMemcpyAsync(s.ag_send, out, (size_t) 2048 * sizeof(F), hipMemcpyDeviceToDevice, ctx->stream));
                s.x[0] = {2, s.ag_send, s.ag_recv, (size_t) 2048 * sizeof(F)}; s.nx = 1;
            }
            s.stage = 2;
            VPCHK(pcs_stage_end(ctx));
        } else if (s.stage == 2) {
            if (!fl.is_tail(k)) {
                tree = s.top_f + fl.top(k);
                VPCHK(pcs_top(ctx, s.ag_recv, (size_t) (No >> 1) * 32, 0, No, tree));
            } else {
                // level k = n_local - 1 whole on every rank (W positions per coset): the first level of the replicated tail
                hipLaunchKernelGGL(k_pc_interleave_tail, dim3(nblk(2048u << s.lw)), dim3(VP_BLOCK), 0, ctx->stream, reinterpret_cast<const F *>(s.ag_recv), s.tail, s.lw);
                tree = s.tail_tree;
                VPCHK(pc_hash_level(ctx, s.tail, (u32) fl.W, nullptr, tree));
            }
            break;
        } else {
            VPCHK(pcs_tail_step(ctx, k, s.step_r, &tree));
            break;
        }
    }
    HIPCHK(hipMemcpyAsync(s.d_roots + k, tree + 1, 32, hipMemcpyDeviceToDevice, ctx->stream));
    VPCHK(pcs_finish(ctx, {{root, tree + 1, 32}}));
    s.f_done = k + 1;
    return VP_OK;
}

int pcs_fri_final(vp_ctx *ctx, vp_F *final_code) {
    PcShard &s = *ctx->pcs;
    if (s.n_steps == 0 || s.f_done != s.n_steps) { ctx->err = "FRI commit phase not finished"; return VP_EINVAL; }
    std::vector<F> cw(64 * 32);
    HIPCHK(hipMemcpy(cw.data(), s.tail + s.fl.tail_cw(s.lw), cw.size() * sizeof(F), hipMemcpyDeviceToHost));
    pc_final_order(cw.data(), final_code);
    return VP_OK;
}

// The descriptor of one oracle of a sharded commitment (pc_open_desc).  A position-sharded oracle (l, h, a locally hashed FRI level) is answered by the
// rank that owns position a = leaf >> 5 (pcs_owns): the 65 value pairs from the local codeword, the five lowest siblings from the local tree, the siblings
// above from the replicated top tree.  A tail level is whole on every rank.
int pcs_open_desc(vp_ctx *ctx, int oracle, PcOpenDesc *d) {
    PcShard &s = *ctx->pcs;
    const FriLayout &fl = s.fl;
    const int lvl = oracle - 2;
    if (lvl >= s.f_done) { ctx->err = "FRI level not committed yet"; return VP_EINVAL; }
    if (lvl >= 0 && fl.is_tail(lvl)) {                                     // tail level: whole codeword on every rank
        const int q = fl.tail_q(lvl);
        d->cw = s.tail + fl.tail_cw(q); d->tree = s.tail_tree + fl.tail_tree(q); d->Nc = (u32) fl.tail_per_coset(q); d->n_leaves = (u32) fl.tail_leaves(q);
        return VP_OK;
    }
    if (oracle == 0) { if (!s.private_done) return VP_EINVAL; d->cw = s.l_loc; d->tree = s.tree_l; d->top = s.top_l; d->Nc = (u32) fl.Nl; }
    else if (oracle == 1) { if (!s.public_done) return VP_EINVAL; d->cw = s.h_loc; d->tree = s.tree_h; d->top = s.top_h; d->Nc = (u32) fl.Nl; }
    else { d->cw = s.fri_loc + fl.loc_cw(lvl); d->tree = s.tree_f + fl.loc_tree(lvl); d->top = s.top_f + fl.top(lvl); d->Nc = (u32) fl.loc_per_coset(lvl); }
    d->n_leaves = (16 * d->Nc) << s.lw; d->n5 = (d->Nc >> 1) << s.lw; d->lw = (u32) s.lw;
    return VP_OK;
}
bool pcs_private_done(vp_ctx *ctx) { return ctx->pcs->private_done; }
bool pcs_public_done(vp_ctx *ctx) { return ctx->pcs->public_done; }
int pcs_fri_done(vp_ctx *ctx) { return ctx->pcs->f_done; }
bool pcs_fri_one_pass(vp_ctx *ctx) { return ctx->pcs->f_mode == 1; }
bool pcs_owns(vp_ctx *ctx, uint64_t leaf) { const PcShard &s = *ctx->pcs; return (int) ((leaf >> 5) & (u64) (s.world - 1)) == s.rank; }

}  // namespace

extern "C" {

int vp_pc_load_input(vp_ctx *ctx, const vp_F *inputs, uint64_t n_inputs, int bit_length) {
    if (!ctx || !inputs || bit_length < 7 || bit_length > 30 || n_inputs == 0 || n_inputs > (1ull << bit_length)) return VP_EINVAL;
    VP_ENTER(ctx);
    VPCHK(pc_hash_outstanding(ctx, 3u));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->gkr_graph) { (void) hipGraphExecDestroy(ctx->gkr_graph); ctx->gkr_graph = nullptr; }
    free_plan(ctx);
    free_all(ctx);
    vp_free_shard_state(ctx);
    // the circuit this layer replaces is gone with everything that belonged to it (tables, layouts, an open sumcheck, a commitment): vp_round / vp_finalize and the
    // GKR entry points refuse until a circuit is uploaded again.  vreal = 0: caller data, possibly complex — vp_evaluate's finding about an earlier witness does not
    // hold for it (the paired transforms of vp_commit_private read .re only)
    circuit_forget(ctx);
    ctx->L.assign(1, LayerDev());
    ctx->n_layers = 1;
    ctx->L[0].size = n_inputs; ctx->L[0].bl = bit_length;
    VPCHK(dalloc(ctx, &ctx->L[0].val, (size_t) 1 << bit_length));
    HIPCHK(hipMemsetAsync(ctx->L[0].val, 0, sizeof(F) << bit_length, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->L[0].val, inputs, n_inputs * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    VPCHK(check_stream(ctx));
    ctx->evaluated = true;
    ensure_event_pool(ctx);
    return VP_OK;
}

int vp_pc_set_shard(vp_ctx *ctx, int rank, int world) {
    if (!ctx || world < 1 || rank < 0 || rank >= world || (world & (world - 1)) || world > 64) return VP_EINVAL;
    if (!ctx->evaluated || ctx->L.empty()) { ctx->err = "vp_pc_set_shard: no input layer yet"; return VP_EINVAL; }
    const int ln = ctx->L[0].bl - 6;
    int lw = 0; while ((1 << lw) < world) ++lw;
    if (world > 1 && ln - lw < 1) { ctx->err = "vp_pc_set_shard: slice too short for this many ranks"; return VP_ELIMIT; }
    if (world > 1 && ln > PC_MAX_LN_LONG) { ctx->err = "vp_pc_set_shard: input layer of more than 2^25 wires"; return VP_ELIMIT; }
    VP_ENTER(ctx);
    VPCHK(pc_hash_outstanding(ctx, 3u));        // (vp_pc_hash_late: a sharded commitment hashes at once, and what the unsharded one still owes is hashed first)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    vp_free_shard_state(ctx);                   // its device arrays stay with the context until the next upload
    // world 1 is the unsharded commitment — unless a one-rank communicator is attached: then the sharded code path runs with a single
    // rank and its collectives go through RCCL (self sends), which is how the transport is exercised on a one-GPU box
    if (world == 1 && !(ctx->cm && ctx->cm->comm && ctx->cm->world == 1)) return VP_OK;
    ctx->pcs = new PcShard();
    ctx->pcs->rank = rank; ctx->pcs->world = world; ctx->pcs->lw = lw; ctx->pcs->S = 64 / world;
    ctx->pcs->fl = FriLayout(ln, lw);
    return VP_OK;
}

// the pending collective i of a context: the commitment shard's, else the round shard's gather (vp_set_round_shard)
static bool pending_x(vp_ctx *ctx, int i, int *kind, const void **send, void **recv, size_t *bytes, int *world) {
    if (ctx->pcs && ctx->pcs->nx) {
        if (i < 0 || i >= ctx->pcs->nx) return false;
        const PcShard::X &x = ctx->pcs->x[i];
        *kind = x.kind; *send = x.send; *recv = x.recv; *bytes = x.bytes; *world = ctx->pcs->world;
        return true;
    }
    if (ctx->rsh && ctx->rsh->nx) {
        if (i != 0) return false;
        const RoundShard::X &x = ctx->rsh->x;
        *kind = x.kind; *send = x.send; *recv = x.recv; *bytes = x.bytes; *world = ctx->rsh->world;
        return true;
    }
    return false;
}
// the gather of round-sharded contexts of one process: rank src's block into slot src of every rank's receive buffer, on the receiver's stream
static int rs_exchange_local(vp_ctx **ctxs, int world) {
    vp_ctx *ctx = ctxs[0];
    const int nx = ctx->rsh->nx;
    const size_t bytes = ctx->rsh->x.bytes;
    for (int r = 0; r < world; ++r)
        if (ctxs[r]->rsh->nx != nx || (nx && ctxs[r]->rsh->x.bytes != bytes)) { ctx->err = "vp_shard_exchange_local: ranks are at different gathers"; return VP_EINVAL; }
    if (!nx) return VP_OK;
    for (int dst = 0; dst < world; ++dst) {
        vp_ctx *d = ctxs[dst];
        HIPCHK(hipSetDevice(d->device));
        for (int src = 0; src < world; ++src)
            HIPCHK(hipMemcpyAsync((char *) d->rsh->x.recv + (size_t) src * bytes, ctxs[src]->rsh->x.send, bytes, hipMemcpyDeviceToDevice, d->stream));
    }
    for (int dst = 0; dst < world; ++dst) {
        HIPCHK(hipSetDevice(ctxs[dst]->device));
        HIPCHK(hipStreamSynchronize(ctxs[dst]->stream));
    }
    for (int r = 0; r < world; ++r) ctxs[r]->rsh->nx = 0;
    return VP_OK;
}

int vp_shard_exchange_local(vp_ctx **ctxs, int world) {
    if (!ctxs || world < 1) return VP_EINVAL;
    {   // round-sharded contexts (vp_set_round_shard) with their gather pending and no commitment collective in the way
        bool rs = true;
        for (int r = 0; r < world; ++r)
            if (!ctxs[r] || !ctxs[r]->rsh || ctxs[r]->rsh->world != world || ctxs[r]->rsh->rank != r || (ctxs[r]->pcs && ctxs[r]->pcs->nx)) rs = false;
        if (rs && ctxs[0]->rsh->nx) return rs_exchange_local(ctxs, world);
    }
    for (int r = 0; r < world; ++r) if (!ctxs[r] || !ctxs[r]->pcs || ctxs[r]->pcs->world != world || ctxs[r]->pcs->rank != r) return VP_EINVAL;
    const int nx = ctxs[0]->pcs->nx;
    for (int r = 0; r < world; ++r) if (ctxs[r]->pcs->nx != nx) { ctxs[0]->err = "vp_shard_exchange_local: ranks are at different collectives"; return VP_EINVAL; }
    vp_ctx *ctx = ctxs[0];
    for (int i = 0; i < nx; ++i) {
        const size_t bytes = ctxs[0]->pcs->x[i].bytes;
        const int kind = ctxs[0]->pcs->x[i].kind;
        for (int r = 0; r < world; ++r) if (ctxs[r]->pcs->x[i].bytes != bytes || ctxs[r]->pcs->x[i].kind != kind) { ctx->err = "vp_shard_exchange_local: mismatched collective"; return VP_EINVAL; }
        for (int src = 0; src < world; ++src)
            for (int dst = 0; dst < world; ++dst) {
                const PcShard::X &xs = ctxs[src]->pcs->x[i], &xd = ctxs[dst]->pcs->x[i];
                const char *from = (const char *) xs.send + (kind == 1 ? (size_t) dst * bytes : 0);
                HIPCHK(hipMemcpy((char *) xd.recv + (size_t) src * bytes, from, bytes, hipMemcpyDeviceToDevice));
            }
    }
    for (int r = 0; r < world; ++r) ctxs[r]->pcs->nx = 0;
    HIPCHK(hipDeviceSynchronize());
    return VP_OK;
}

// A caller-supplied transport for the pending collectives (no communicator attached, ranks in DIFFERENT processes): the send side of
// collective i is copied to the host, the caller moves the bytes (torch.distributed over gloo in the rehearsals and the CPU tests), the
// received side is copied back, vp_shard_exchange_done clears the list; then the interrupted entry point is called again, as after
// vp_shard_exchange_local.  kind 1: all-to-all, `bytes` per peer (send / recv = world x bytes, peer-major); kind 2: all-gather, `bytes` per rank
// (send = bytes, recv = world x bytes).
int vp_shard_pending(vp_ctx *ctx, int *n) {
    if (!ctx || !n) return VP_EINVAL;
    VP_LOCK(ctx);
    *n = ctx->pcs ? ctx->pcs->nx : 0;
    if (!*n && ctx->rsh) *n = ctx->rsh->nx;
    return VP_OK;
}
int vp_shard_exchange_info(vp_ctx *ctx, int i, int *kind, uint64_t *bytes) {
    if (!ctx || !kind || !bytes) return VP_EINVAL;
    VP_LOCK(ctx);
    const void *snd; void *rcv; size_t b; int w;
    if (!pending_x(ctx, i, kind, &snd, &rcv, &b, &w)) return VP_EINVAL;
    *bytes = b;
    return VP_OK;
}
int vp_shard_exchange_get(vp_ctx *ctx, int i, void *host_send) {
    if (!ctx || !host_send) return VP_EINVAL;
    int kind, world; const void *snd; void *rcv; size_t bytes;
    { VP_LOCK(ctx); if (!pending_x(ctx, i, &kind, &snd, &rcv, &bytes, &world)) return VP_EINVAL; }
    VP_ENTER(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(host_send, snd, kind == 1 ? (size_t) world * bytes : bytes, hipMemcpyDeviceToHost));
    return VP_OK;
}
int vp_shard_exchange_put(vp_ctx *ctx, int i, const void *host_recv) {
    if (!ctx || !host_recv) return VP_EINVAL;
    int kind, world; const void *snd; void *rcv; size_t bytes;
    { VP_LOCK(ctx); if (!pending_x(ctx, i, &kind, &snd, &rcv, &bytes, &world)) return VP_EINVAL; }
    VP_ENTER(ctx);
    HIPCHK(hipMemcpy(rcv, host_recv, (size_t) world * bytes, hipMemcpyHostToDevice));
    return VP_OK;
}
int vp_shard_exchange_done(vp_ctx *ctx) {
    if (!ctx) return VP_EINVAL;
    VP_LOCK(ctx);
    if (ctx->pcs && ctx->pcs->nx) { ctx->pcs->nx = 0; return VP_OK; }
    if (ctx->rsh) { ctx->rsh->nx = 0; return VP_OK; }
    if (!ctx->pcs) return VP_EINVAL;
    ctx->pcs->nx = 0;
    return VP_OK;
}

// ---- RCCL ------------------------------------------------------------------------------------------------------------------
int vp_comm_unique_id(uint8_t id[128]) {
    RandKeep keep_callers_random_stream;
    void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return VP_EHIP;
    auto fn = (int (*)(void *)) dlsym(lib, "ncclGetUniqueId");
    if (!fn) return VP_EHIP;
    return fn(id) == 0 ? VP_OK : VP_EHIP;
}

int vp_comm_init(vp_ctx *ctx, const uint8_t id[128], int rank, int world) {
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world) return VP_EINVAL;
    RandKeep keep_callers_random_stream;
    VP_ENTER(ctx);
    if (ctx->cm && ctx->cm->comm) { ctx->err = "communicator already attached"; return VP_EINVAL; }
    // a chain-sharded proof all-reduces over THIS communicator: its ranks must be the shard's ranks (a duplicate shard rank would be summed twice)
    if (ctx->shard_world > 1 && (ctx->shard_world != world || ctx->shard_rank != rank)) { ctx->err = "vp_comm_init: communicator rank/world differ from vp_set_shard's"; return VP_EINVAL; }
    if (!ctx->cm) ctx->cm = new VpComm();
    VpComm &s = *ctx->cm;
    s.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!s.lib) s.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!s.lib) { ctx->err = std::string("librccl not found: ") + dlerror(); return VP_EHIP; }
    struct Id { char b[128]; } uid; memcpy(uid.b, id, 128);
    auto init = (int (*)(void **, int, Id, int)) dlsym(s.lib, "ncclCommInitRank");
    s.fn_allgather = (decltype(s.fn_allgather)) dlsym(s.lib, "ncclAllGather");
    s.fn_allreduce = (decltype(s.fn_allreduce)) dlsym(s.lib, "ncclAllReduce");
    s.fn_send = (decltype(s.fn_send)) dlsym(s.lib, "ncclSend");
    s.fn_recv = (decltype(s.fn_recv)) dlsym(s.lib, "ncclRecv");
    s.fn_group_start = (decltype(s.fn_group_start)) dlsym(s.lib, "ncclGroupStart");
    s.fn_group_end = (decltype(s.fn_group_end)) dlsym(s.lib, "ncclGroupEnd");
    s.fn_comm_destroy = (decltype(s.fn_comm_destroy)) dlsym(s.lib, "ncclCommDestroy");
    if (!init || !s.fn_allgather || !s.fn_allreduce || !s.fn_send || !s.fn_recv || !s.fn_group_start || !s.fn_group_end) { ctx->err = "RCCL symbols missing"; return VP_EHIP; }
    if (init(&s.comm, world, uid, rank) != 0) { s.comm = nullptr; ctx->err = "ncclCommInitRank failed"; return VP_EHIP; }
    s.rank = rank; s.world = world;
    return VP_OK;
}

int vp_comm_count(vp_ctx *ctx, int *n_ranks) {
    if (!ctx || !n_ranks || !ctx->cm || !ctx->cm->comm) return VP_EINVAL;
    auto fn = (int (*)(void *, int *)) dlsym(ctx->cm->lib, "ncclCommCount");
    if (!fn || fn(ctx->cm->comm, n_ranks) != 0) { ctx->err = "ncclCommCount failed"; return VP_EHIP; }
    return VP_OK;
}

int vp_comm_destroy(vp_ctx *ctx) {
    if (!ctx) return VP_EINVAL;
    (void) hipStreamSynchronize(ctx->stream);
    vp_free_comm(ctx);
    return VP_OK;
}

// u64 sum of a device buffer over the communicator, in place, on the library stream.  vp_prove_gkr uses it for the ONE data-path
// collective of a chain-sharded proof (the transcript slices of the ranks are disjoint, everything else is zero, so the sum is exact).
int vp_allreduce_u64(vp_ctx *ctx, void *dev_buf, uint64_t count) {
    if (!ctx || !ctx->cm || !ctx->cm->comm || !dev_buf) return VP_EINVAL;
    if (ctx->cm->fn_allreduce(dev_buf, dev_buf, count, VP_NCCL_UINT64, VP_NCCL_SUM, ctx->cm->comm, ctx->stream)) { ctx->err = "ncclAllReduce failed"; return VP_EHIP; }
    return VP_OK;
}

// Opening of a sharded oracle: the rank that owns position a = leaf >> 5 (a mod W) answers — values and the five lowest siblings from
// its local arrays, the upper siblings from the replicated top tree.  Other ranks return VP_EINVAL.  Tail levels: every rank.
int vp_pc_shard_owner(vp_ctx *ctx, int oracle, uint64_t leaf) {
    if (!ctx || !ctx->pcs || ctx->pcs->world <= 1) return 0;
    const PcShard &s = *ctx->pcs;
    if (oracle >= 2 && s.fl.is_tail(oracle - 2)) return -1;                    // tail level: replicated
    return (int) ((leaf >> 5) & (uint64_t) (s.world - 1));
}

}  // extern "C"
