// Device-side construction of the per-layer index structures of vp_circuit_upload (part of the single translation unit vpgpu.hip).
//
// layeredCircuit::subsetInit (src/circuit.cpp:43-80) leaves the gates in layer order; the prover's init passes scatter over them
// (src/prover.cpp:209-272, 314-360, 396-414).  The device inits GATHER instead, so every layer needs its gates listed by target:
//   c1   gates sorted by u                       (phase-1 init: row = wire of layer i-1)
//   c2   gates sorted by (l, lv) slot            (phase-2 init: row = slot of the concatenated subsets)
//   Liu  the later layers' dadId lists inverted  (row = wire of layer i-1, entry = (which later layer, position in its subset))
//   predicate buckets                            (verifier side: gates grouped by type and source layer)
// Round 1 built these with counting sorts on one host core: 0.70 s (x64) / 5.0 s (x1024) per upload.  Here the raw gate arrays are
// copied to HBM as they are and everything per gate happens there: one validation + key kernel, stable LSD radix sorts (rocPRIM
// device primitives: a sort at set-up time is plain library work, the proof's kernels stay hand-written), row pointers by binary search
// in the sorted keys, gathers of the per-entry payload.  Stable sorts reproduce the gate order inside a row, so the lists are the
// same arrays the host version produced.  Only O(layers^2) bookkeeping, the (few) rows with more than VP_LIGHT_MAX contributions and
// the bucket boundaries are finished on the host.
#include <rocprim/rocprim.hpp>

namespace vp {

// error word: min over failing gates of (gate << 8 | code), so that the first failing gate of the layer is the one reported
enum { UP_BAD_TYPE = 1, UP_BAD_U = 2, UP_UNARY_L = 3, UP_BAD_V = 4, UP_BAD_LV = 5, UP_BAD_DAD = 6 };
struct UpLayerArgs {
    u32 n; int layer;
    const uint8_t *ty; const int32_t *l; const u32 *u, *v, *lv; const uint8_t *is_assert;
    const u64 *layer_size;              // [n_layers]
    const u64 *dad_size;                // [layer]
    const u32 *const *dad_id;           // [layer] device pointers
    const u32 *t_off;                   // [layer] phase-2 slot offsets
    uint8_t *o_ty; int16_t *o_gl; u32 *o_gu, *o_gv, *o_glv; uint16_t *o_etl;
    u32 *key1, *key2, *bkey;            // bkey: [2n] predicate bucket of the gate, second half: bucket 4 for Addc gates, ~0 otherwise
    uint8_t *asf;                       // [n] assert flag (select input)
    unsigned long long *err; u32 *need_c;
};
__device__ __forceinline__ bool up_unary(int t) { return t == VP_ADDC || t == VP_MULC || t == VP_COPY || t == VP_NOT; }
__global__ void __launch_bounds__(VP_BLOCK) k_up_prepare(UpLayerArgs a) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const int t = a.ty[g], l = a.l[g], i = a.layer;
    const u32 u = a.u[g], v = a.v[g], lv = a.lv[g];
    int code = 0;
    if (t < 0 || t > VP_COPY || t == VP_INPUT) code = UP_BAD_TYPE;
    else if (u >= a.layer_size[i - 1]) code = UP_BAD_U;
    else if (up_unary(t)) { if (l != -1) code = UP_UNARY_L; }
    else if (l < 0 || l >= i || v >= a.layer_size[l]) code = UP_BAD_V;
    else if (lv >= a.dad_size[l] || a.dad_id[l][lv] != v) code = UP_BAD_LV;
    const bool as = a.is_assert && a.is_assert[g];
    a.asf[g] = as ? 1 : 0;
    if (code) {
        atomicMin(a.err, ((unsigned long long) g << 8) | (unsigned) code);
        a.o_ty[g] = 0; a.o_gl[g] = -1; a.o_gu[g] = 0; a.o_gv[g] = 0; a.o_glv[g] = 0; a.o_etl[g] = 0;
        a.key1[g] = 0; a.key2[g] = 0; a.bkey[g] = 0; a.bkey[a.n + g] = ~0u;
        return;
    }
    const bool un = up_unary(t);
    if (t == VP_ADDC || t == VP_MULC) *a.need_c = 1;             // plain store of the same value from many lanes
    a.o_ty[g] = (uint8_t) t; a.o_gl[g] = (int16_t) l; a.o_gu[g] = u; a.o_gv[g] = un ? 0 : v; a.o_glv[g] = un ? 0 : lv;
    a.o_etl[g] = (uint16_t) ((t << 8) | (l < 0 ? 0xff : l) | (as ? 0x8000 : 0));
    a.key1[g] = u;
    a.key2[g] = un ? a.t_off[i - 1] : a.t_off[l] + lv;           // src/prover.cpp:314,342-353
    // predicate buckets: 0 Copy, 1 Not, 2 Addc, 3 Mulc (x c), 4 bias (Addc x c), 5 + tyidx * i + l for the binary types
    u32 b;
    if (t == VP_COPY) b = 0; else if (t == VP_NOT) b = 1; else if (t == VP_ADDC) b = 2; else if (t == VP_MULC) b = 3;
    else {
        const int tyidx = t == VP_MUL ? 3 : t == VP_ADD ? 0 : t == VP_SUB ? 1 : t == VP_ANTISUB ? 2 : t == VP_NAAB ? 4 : t == VP_ANTINAAB ? 5 : 6;
        b = 5 + (u32) tyidx * (u32) i + (u32) l;
    }
    a.bkey[g] = b;
    a.bkey[a.n + g] = t == VP_ADDC ? 4u : ~0u;
}
__global__ void __launch_bounds__(VP_BLOCK) k_up_iota(u32 *o, u32 n, u32 mod) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = mod ? i % mod : i;
}
// rowptr[r] = first position whose key is >= r  (r = 0..n_rows; sorted keys)
__global__ void __launch_bounds__(VP_BLOCK) k_up_rowptr(const u32 *__restrict__ ks, u32 n, u32 *__restrict__ rowptr, u32 n_rows) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rows) return;
    u32 lo = 0, hi = n;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (ks[mid] < r) lo = mid + 1; else hi = mid; }
    rowptr[r] = lo;
}
__global__ void __launch_bounds__(VP_BLOCK) k_up_gather_entries(const u32 *__restrict__ sg, u32 n, const u32 *__restrict__ ex, const uint16_t *__restrict__ etl,
                                                                u32 *__restrict__ sx, uint16_t *__restrict__ stl) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) { const u32 g = sg[p]; sx[p] = ex[g]; stl[p] = etl[g]; }
}
// rows with more than VP_LIGHT_MAX contributions: (row, begin, end) appended in any order (the host sorts the handful there is)
__global__ void __launch_bounds__(VP_BLOCK) k_up_heavy(const u32 *__restrict__ rowptr, u32 n_rows, u32 *__restrict__ count, u32 *__restrict__ out, u32 cap) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u32 b = rowptr[r], e = rowptr[r + 1];
    if (e - b <= VP_LIGHT_MAX) return;
    const u32 q = atomicAdd(count, 1u);
    if (q < cap) { out[3 * q] = r; out[3 * q + 1] = b; out[3 * q + 2] = e; }
}
// bucket sizes of the sorted predicate list (keys < nbk valid, ~0 = padding): LDS histogram per workgroup
__global__ void __launch_bounds__(VP_BLOCK) k_up_bucket_hist(const u32 *__restrict__ bkey, u32 n2, u32 nbk, u32 *__restrict__ hist) {
    __shared__ u32 h[512];
    for (u32 i = threadIdx.x; i < 512; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += gridDim.x * blockDim.x) { const u32 b = bkey[i]; if (b < nbk) atomicAdd(&h[b], 1u); }
    __syncthreads();
    for (u32 i = threadIdx.x; i < nbk; i += blockDim.x) if (h[i]) atomicAdd(&hist[i], h[i]);
}
__global__ void __launch_bounds__(VP_BLOCK) k_up_pflag(const u32 *__restrict__ sk, const u32 *__restrict__ pidx, u32 n, const uint8_t *__restrict__ asf, uint8_t *__restrict__ pflag) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const u32 b = sk[p];
    const int cls = b >= 5 ? 0 : (b == 3 || b == 4) ? 2 : 1;
    pflag[p] = (uint8_t) ((cls << 1) | asf[pidx[p]]);
}
__global__ void __launch_bounds__(VP_BLOCK) k_up_check_range(const u32 *__restrict__ ids, u32 n, u64 limit, unsigned long long *err) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ids[i] >= limit) atomicMin(err, ((unsigned long long) i << 8) | UP_BAD_DAD);
}
// one subset j of layer i: the gather map of the round-by-round phase-2 init and the per-slot source of the batched one
__global__ void __launch_bounds__(VP_BLOCK) k_up_subset(const u32 *__restrict__ ids, u32 n, u32 slot0, u32 out0, uint8_t j,
                                                        u32 *__restrict__ g_slot, uint8_t *__restrict__ g_layer, u32 *__restrict__ g_idx,
                                                        uint8_t *__restrict__ s_layer, u32 *__restrict__ s_idx) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 x = ids[k];
    g_slot[out0 + k] = slot0 + k; g_layer[out0 + k] = j; g_idx[out0 + k] = x;
    s_layer[slot0 + k] = j; s_idx[slot0 + k] = x;
}
__global__ void k_up_empty_subset(u32 slot0, u32 out0, u32 *g_slot, uint8_t *g_layer, u32 *g_idx, uint8_t *s_layer) {
    g_slot[out0] = slot0; g_layer[out0] = 0xff; g_idx[out0] = 0; s_layer[slot0] = 0xff;
}
// Liu lists: segment q of the concatenation holds positions 0..n-1 of one later layer's subset
__global__ void __launch_bounds__(VP_BLOCK) k_up_liu_fill(u32 *__restrict__ gcat, uint8_t *__restrict__ qcat, u32 at, u32 n, uint8_t q) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) { gcat[at + k] = k; qcat[at + k] = q; }
}
__global__ void __launch_bounds__(VP_BLOCK) k_up_liu_gather(const u32 *__restrict__ sidx, u32 n, const u32 *__restrict__ gcat, const uint8_t *__restrict__ qcat,
                                                            u32 *__restrict__ eg, uint8_t *__restrict__ eq) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) { const u32 s = sidx[p]; eg[p] = gcat[s]; eq[p] = qcat[s]; }
}
// Row records of a target-sorted list (GenP1R / GenP2R, vp_kernels_batch.h): { g, x, tl | count << 16, position of the second entry } of the row's first
// entry; count 0xffff marks a heavy row.  val_off (phase 1 only): x becomes the operand's index in the arena of circuit values, ~0 for a unary entry, and
// every entry's index goes to e_xg.
__global__ void __launch_bounds__(VP_BLOCK) k_up_rowrec(const u32 *__restrict__ rowptr, const u32 *__restrict__ e_g, const u32 *__restrict__ e_x, const uint16_t *__restrict__ e_tl,
                                                        const u32 *__restrict__ val_off, u32 n_rows, u32 n, uint4 *__restrict__ rec, u32 *__restrict__ e_xg) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (val_off && i < n) { const u32 l = e_tl[i] & 0xffu; e_xg[i] = l == 0xffu ? ~0u : val_off[l] + e_x[i]; }
    if (i >= n_rows) return;
    const u32 b = rowptr[i], cnt = rowptr[i + 1] - b;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (cnt > VP_LIGHT_MAX) q.z = 0xffffu << 16;
    else if (cnt) {
        const u32 tl = e_tl[b], l = tl & 0xffu;
        q.x = e_g[b]; q.y = !val_off ? e_x[b] : l == 0xffu ? ~0u : val_off[l] + e_x[b];
        q.z = tl | (cnt << 16); q.w = b + 1;
    }
    rec[i] = q;
}
// phase-2 slot -> arena index of its V entry (~0: an empty subset's slot or a padding slot, both read as zero)
__global__ void __launch_bounds__(VP_BLOCK) k_up_sgidx(const uint8_t *__restrict__ s_layer, const u32 *__restrict__ s_idx, const u32 *__restrict__ val_off, u32 n, u32 *__restrict__ s_gidx) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 l = s_layer[i];
    s_gidx[i] = l >= 0xfeu ? ~0u : val_off[l] + s_idx[i];
}
// Liu row records (GenLiuR): { bf, bs, count, position of the second entry }, bf / bs = where the two factors of eq_q(g) lie in the pool of half
// tables (H[q].h1 depends on bit lengths only); l_bf / l_bs: the same pair for every entry
__global__ void __launch_bounds__(VP_BLOCK) k_up_liu_rec(const u32 *__restrict__ rowptr, const uint8_t *__restrict__ l_q, const u32 *__restrict__ l_g, const Half *__restrict__ H,
                                                         const F *pool, u32 rows, u32 n, uint4 *__restrict__ rec, u32 *__restrict__ l_bf, u32 *__restrict__ l_bs) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const Half h = H[l_q[i]];
        const u32 g = l_g[i];
        l_bf[i] = (u32) (h.bf - pool) + (g & ((1u << h.h1) - 1)); l_bs[i] = (u32) (h.bs - pool) + (g >> h.h1);
    }
    if (i >= rows) return;
    const u32 b = rowptr[i], cnt = rowptr[i + 1] - b;
    uint4 q = make_uint4(0, 0, cnt, b + 1);
    if (cnt) {
        const Half h = H[l_q[b]];
        const u32 g = l_g[b];
        q.x = (u32) (h.bf - pool) + (g & ((1u << h.h1) - 1)); q.y = (u32) (h.bs - pool) + (g >> h.h1);
    }
    rec[i] = q;
}

}  // namespace vp

namespace {

// scratch of one vp_circuit_upload call: freed when the call returns (none of it is referenced by the context afterwards)
struct UpScratch {
    std::vector<void *> tmp;
    void *sort_tmp = nullptr; size_t sort_cap = 0;
    ~UpScratch() { for (void *p : tmp) (void) hipFree(p); if (sort_tmp) (void) hipFree(sort_tmp); }
};
template <class T>
int up_tmp(vp_ctx *ctx, UpScratch &S, T **p, size_t n) {
    *p = nullptr;
    HIPCHK(hipMalloc((void **) p, std::max<size_t>(1, n) * sizeof(T)));
    S.tmp.push_back((void *) *p);
    return VP_OK;
}
template <class T>
int up_h2d(vp_ctx *ctx, UpScratch &S, T **p, const T *h, size_t n) {
    VPCHK(up_tmp(ctx, S, p, n));
    if (n) HIPCHK(hipMemcpyAsync(*p, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return VP_OK;
}
void up_release(UpScratch &S) { for (void *p : S.tmp) (void) hipFree(p); S.tmp.clear(); }

// stable sort of (key, value) pairs on bits [0, bits)
int up_sort_pairs(vp_ctx *ctx, UpScratch &S, const u32 *kin, u32 *kout, const u32 *vin, u32 *vout, u32 n, int bits) {
    if (!n) return VP_OK;
    size_t need = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t) n, 0u, (unsigned) bits, ctx->stream));
    if (need > S.sort_cap) {
        if (S.sort_tmp) (void) hipFree(S.sort_tmp);
        S.sort_tmp = nullptr; S.sort_cap = 0;
        HIPCHK(hipMalloc(&S.sort_tmp, need));
        S.sort_cap = need;
    }
    HIPCHK(rocprim::radix_sort_pairs(S.sort_tmp, need, kin, kout, vin, vout, (size_t) n, 0u, (unsigned) bits, ctx->stream));
    return VP_OK;
}
inline int bits_for(u64 n_values) { int b = 1; while ((1ull << b) < n_values) ++b; return b; }

// Target-sorted contribution list of one layer and one phase, built on the device (the counting sort of round 1, see the file header).
// key / ex / etl: per gate, in gate order.
// d_val_off: phase 1, the layers' offsets in the arena of circuit values (row records with pre-added operand indices); nullptr: phase 2.
int build_csr_dev(vp_ctx *ctx, UpScratch &S, Csr &c, u32 n_rows, u32 n, const u32 *d_key, const u32 *d_iota, const u32 *d_ex, const uint16_t *d_etl, const u32 *d_val_off) {
    c.n_rows = n_rows; c.n_entries = n;
    VPCHK(dalloc(ctx, &c.rowptr, (size_t) n_rows + 1));
    VPCHK(dalloc(ctx, &c.e_g, (size_t) n)); VPCHK(dalloc(ctx, &c.e_x, (size_t) n)); VPCHK(dalloc(ctx, &c.e_tl, (size_t) n));
    u32 *ks = nullptr;
    VPCHK(up_tmp(ctx, S, &ks, (size_t) n));
    VPCHK(up_sort_pairs(ctx, S, d_key, ks, d_iota, c.e_g, n, bits_for(std::max<u64>(2, n_rows))));
    hipLaunchKernelGGL(k_up_rowptr, dim3(nblk((u64) n_rows + 1)), dim3(VP_BLOCK), 0, ctx->stream, ks, n, c.rowptr, n_rows);
    if (n) hipLaunchKernelGGL(k_up_gather_entries, dim3(nblk(n)), dim3(VP_BLOCK), 0, ctx->stream, c.e_g, n, d_ex, d_etl, c.e_x, c.e_tl);
    if (ctx->gen_rec_ok && (ctx->opt.gen_rec & 1)) {
        VPCHK(dalloc(ctx, &c.rec, (size_t) n_rows));
        if (d_val_off) VPCHK(dalloc(ctx, &c.e_xg, (size_t) n));
        const u64 span = std::max<u64>(n_rows, d_val_off ? n : 0);
        if (span) hipLaunchKernelGGL(k_up_rowrec, dim3(nblk(span)), dim3(VP_BLOCK), 0, ctx->stream, c.rowptr, c.e_g, c.e_x, c.e_tl, d_val_off, n_rows, n, c.rec, c.e_xg);
    }
    // heavy rows: count, then fetch (row, begin, end)
    u32 *d_cnt = nullptr, *d_hv = nullptr;
    VPCHK(up_tmp(ctx, S, &d_cnt, 1));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u32), ctx->stream));
    u32 cap = 4096;
    std::vector<u32> hv;
    u32 n_heavy = 0;
    for (int pass = 0; pass < 2; ++pass) {
        VPCHK(up_tmp(ctx, S, &d_hv, (size_t) 3 * cap));
        if (n_rows) hipLaunchKernelGGL(k_up_heavy, dim3(nblk(n_rows)), dim3(VP_BLOCK), 0, ctx->stream, c.rowptr, n_rows, d_cnt, d_hv, cap);
        HIPCHK(hipMemcpyAsync(&n_heavy, d_cnt, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_heavy <= cap) break;
        cap = n_heavy;                                          // more heavy rows than the first buffer holds: once more with the exact size
        HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u32), ctx->stream));
    }
    hv.resize((size_t) 3 * n_heavy);
    if (n_heavy) HIPCHK(hipMemcpy(hv.data(), d_hv, hv.size() * sizeof(u32), hipMemcpyDeviceToHost));
    std::vector<u32> order(n_heavy);
    for (u32 q = 0; q < n_heavy; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), [&](u32 x, u32 y) { return hv[3 * x] < hv[3 * y]; });
    std::vector<u32> heavy_row, heavy_cptr(1, 0), cb, ce, ch;
    c.n_heavy_entries = 0;
    for (u32 q : order) {
        const u32 r = hv[3 * q], b = hv[3 * q + 1], e = hv[3 * q + 2];
        heavy_row.push_back(r);
        for (u32 s = b; s < e; s += VP_CHUNK) { cb.push_back(s); ce.push_back(std::min(e, s + VP_CHUNK)); ch.push_back((u32) heavy_row.size() - 1); }
        heavy_cptr.push_back((u32) cb.size());
        c.n_heavy_entries += e - b;
    }
    c.n_heavy = n_heavy; c.n_chunks = (u32) cb.size();
    c.h_heavy_row = heavy_row; c.h_heavy_cptr = heavy_cptr;
    VPCHK(dupload(ctx, &c.heavy_row, heavy_row)); VPCHK(dupload(ctx, &c.heavy_cptr, heavy_cptr));
    VPCHK(dupload(ctx, &c.chunk_beg, cb)); VPCHK(dupload(ctx, &c.chunk_end, ce)); VPCHK(dupload(ctx, &c.chunk_h, ch));
    { std::vector<u32> zero(std::max<u32>(1, n_heavy), 0); VPCHK(dupload(ctx, &c.heavy_cnt, zero)); }
    ctx->chunk_cap = std::max(ctx->chunk_cap, c.n_chunks);
    return VP_OK;
}

const char *up_error_text(int code) {
    switch (code) {
        case UP_BAD_TYPE: return "bad gate type";
        case UP_BAD_U: return "gate.u out of range";
        case UP_UNARY_L: return "unary gate with l != -1";
        case UP_BAD_V: return "gate.v out of range";
        case UP_BAD_LV: return "gate.lv inconsistent with dadId";
        case UP_BAD_DAD: return "dadId out of range";
        default: return "bad circuit";
    }
}

// Everything per gate of layer i (i >= 1): validation, the arrays the evaluation kernel reads, the two contribution lists, the predicate
// buckets, the assert list, the subset maps.  `d_sizes`: layer sizes on the device.
int upload_layer_dev(vp_ctx *ctx, UpScratch &S, int i, const vp_layer_desc *ld, const u64 *d_sizes) {
    LayerDev &D = ctx->L[i];
    const vp_layer_desc &L = ld[i];
    const u32 n = (u32) L.size;
    // ---- subsets first: the gate check reads dadId ----
    D.dad_size.resize(i); D.dad_bl.resize(i); D.dad_id.assign(i, nullptr); D.t_off.resize(i); D.t_len.resize(i);
    D.max_dad_bl = -1;
    u32 off = 0, n_gather = 0;
    for (int j = 0; j < i; ++j) {
        D.dad_size[j] = L.dad_size[j];
        if (L.dad_size[j] > ld[j].size) { ctx->err = "dadSize too large"; return VP_EINVAL; }
        D.dad_bl[j] = L.dad_size[j] ? ceil_log2(L.dad_size[j]) : 0;
        if (L.dad_size[j]) {
            if (!L.dad_id[j]) { ctx->err = "layer arrays missing"; return VP_EINVAL; }
            if (L.dad_bitlen[j] != D.dad_bl[j]) { ctx->err = "dadBitLength mismatch"; return VP_EINVAL; }
            D.max_dad_bl = std::max(D.max_dad_bl, D.dad_bl[j]);
        }
        D.t_off[j] = off; D.t_len[j] = 1u << D.dad_bl[j];
        off += D.t_len[j];
        n_gather += L.dad_size[j] ? (u32) L.dad_size[j] : 1u;
    }
    D.p2_total = off; D.n_gather = n_gather;
    unsigned long long *d_err = nullptr; u32 *d_needc = nullptr;
    VPCHK(up_tmp(ctx, S, &d_err, 2)); VPCHK(up_tmp(ctx, S, &d_needc, 1));      // [0]: the gates' error word, [1]: the subsets' (reported first: the gate check reads dadId)
    HIPCHK(hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(d_needc, 0, sizeof(u32), ctx->stream));
    VPCHK(dalloc(ctx, &D.g_slot, (size_t) n_gather)); VPCHK(dalloc(ctx, &D.g_layer, (size_t) n_gather)); VPCHK(dalloc(ctx, &D.g_idx, (size_t) n_gather));
    VPCHK(dalloc(ctx, &D.s_layer, (size_t) D.p2_total)); VPCHK(dalloc(ctx, &D.s_idx, (size_t) D.p2_total));
    HIPCHK(hipMemsetAsync(D.s_layer, 0xfe, std::max<size_t>(1, D.p2_total), ctx->stream));
    HIPCHK(hipMemsetAsync(D.s_idx, 0, std::max<size_t>(1, D.p2_total) * sizeof(u32), ctx->stream));
    std::vector<const u32 *> dad_ptrs(i, nullptr);
    u32 gat = 0;
    for (int j = 0; j < i; ++j) {
        if (L.dad_size[j]) {
            const u32 m = (u32) L.dad_size[j];
            VPCHK(dalloc(ctx, &D.dad_id[j], (size_t) m));
            HIPCHK(hipMemcpyAsync(D.dad_id[j], L.dad_id[j], (size_t) m * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_up_check_range, dim3(nblk(m)), dim3(VP_BLOCK), 0, ctx->stream, D.dad_id[j], m, ld[j].size, d_err + 1);
            hipLaunchKernelGGL(k_up_subset, dim3(nblk(m)), dim3(VP_BLOCK), 0, ctx->stream, D.dad_id[j], m, D.t_off[j], gat, (uint8_t) j,
                               D.g_slot, D.g_layer, D.g_idx, D.s_layer, D.s_idx);
            gat += m;
        } else {
            VPCHK(dalloc(ctx, &D.dad_id[j], (size_t) 1));
            hipLaunchKernelGGL(k_up_empty_subset, dim3(1), dim3(1), 0, ctx->stream, D.t_off[j], gat, D.g_slot, D.g_layer, D.g_idx, D.s_layer);
            gat += 1;
        }
        dad_ptrs[j] = D.dad_id[j];
    }
    // ---- raw gate arrays as they are ----
    UpLayerArgs a{};
    a.n = n; a.layer = i;
    uint8_t *r_ty = nullptr, *r_as = nullptr; int32_t *r_l = nullptr; u32 *r_u = nullptr, *r_v = nullptr, *r_lv = nullptr;
    VPCHK(up_h2d(ctx, S, &r_ty, L.ty, (size_t) n)); VPCHK(up_h2d(ctx, S, &r_l, L.l, (size_t) n));
    VPCHK(up_h2d(ctx, S, &r_u, L.u, (size_t) n)); VPCHK(up_h2d(ctx, S, &r_v, L.v, (size_t) n)); VPCHK(up_h2d(ctx, S, &r_lv, L.lv, (size_t) n));
    if (L.is_assert) VPCHK(up_h2d(ctx, S, &r_as, L.is_assert, (size_t) n));
    a.ty = r_ty; a.l = r_l; a.u = r_u; a.v = r_v; a.lv = r_lv; a.is_assert = r_as;
    a.layer_size = d_sizes;
    u64 *d_dsz = nullptr; const u32 **d_dptr = nullptr; u32 *d_toff = nullptr;
    {
        std::vector<u64> dsz(L.dad_size, L.dad_size + i);
        VPCHK(up_h2d(ctx, S, &d_dsz, dsz.data(), (size_t) i));
        VPCHK(up_h2d(ctx, S, &d_dptr, dad_ptrs.data(), (size_t) i));
        VPCHK(up_h2d(ctx, S, &d_toff, D.t_off.data(), (size_t) i));
        HIPCHK(hipStreamSynchronize(ctx->stream));              // the staging vectors above go out of scope
    }
    a.dad_size = d_dsz; a.dad_id = d_dptr; a.t_off = d_toff;
    VPCHK(dalloc(ctx, &D.ty, (size_t) n)); VPCHK(dalloc(ctx, &D.gl, (size_t) n)); VPCHK(dalloc(ctx, &D.gu, (size_t) n));
    VPCHK(dalloc(ctx, &D.gv, (size_t) n)); VPCHK(dalloc(ctx, &D.glv, (size_t) n));
    uint16_t *d_etl = nullptr; u32 *key1 = nullptr, *key2 = nullptr, *bkey = nullptr, *iota2 = nullptr; uint8_t *asf = nullptr;
    VPCHK(up_tmp(ctx, S, &d_etl, (size_t) n)); VPCHK(up_tmp(ctx, S, &key1, (size_t) n)); VPCHK(up_tmp(ctx, S, &key2, (size_t) n));
    VPCHK(up_tmp(ctx, S, &bkey, (size_t) 2 * n)); VPCHK(up_tmp(ctx, S, &iota2, (size_t) 2 * n)); VPCHK(up_tmp(ctx, S, &asf, (size_t) n));
    a.o_ty = D.ty; a.o_gl = D.gl; a.o_gu = D.gu; a.o_gv = D.gv; a.o_glv = D.glv; a.o_etl = d_etl;
    a.key1 = key1; a.key2 = key2; a.bkey = bkey; a.asf = asf; a.err = d_err; a.need_c = d_needc;
    hipLaunchKernelGGL(k_up_prepare, dim3(nblk(n)), dim3(VP_BLOCK), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_up_iota, dim3(nblk((u64) 2 * n)), dim3(VP_BLOCK), 0, ctx->stream, iota2, 2 * n, n);       // g, then g again for the Addc bias entries
    unsigned long long err2[2] = {0, 0}; u32 need_c = 0;
    HIPCHK(hipMemcpyAsync(err2, d_err, sizeof err2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&need_c, d_needc, sizeof need_c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // a subset entry out of range goes first, then the lowest failing gate: a bad dadId entry also fails the lv check of the gate that points at it, and which of
    // the two one shared word reported depended on whether the entry's position or the gate's index was the smaller
    const unsigned long long err = err2[1] != ~0ull ? err2[1] : err2[0];
    if (err != ~0ull) { ctx->err = up_error_text((int) (err & 0xff)); return VP_EINVAL; }
    if (need_c && !L.c) { ctx->err = "Addc/Mulc gates without constants"; return VP_EINVAL; }
    if (need_c) {
        VPCHK(dalloc(ctx, &D.gc, (size_t) n));
        HIPCHK(hipMemcpyAsync(D.gc, L.c, (size_t) n * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
    }
    // ---- assert gates, ascending ----
    {
        u32 *d_sel = nullptr, *d_nsel = nullptr;
        VPCHK(up_tmp(ctx, S, &d_sel, (size_t) n)); VPCHK(up_tmp(ctx, S, &d_nsel, 1));
        size_t need = 0;
        HIPCHK(rocprim::select(nullptr, need, iota2, asf, d_sel, d_nsel, (size_t) n, ctx->stream));
        void *tmp = nullptr;
        VPCHK(up_tmp(ctx, S, (unsigned char **) &tmp, need));
        HIPCHK(rocprim::select(tmp, need, iota2, asf, d_sel, d_nsel, (size_t) n, ctx->stream));
        u32 na = 0;
        HIPCHK(hipMemcpyAsync(&na, d_nsel, sizeof na, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        D.n_assert = na;
        VPCHK(dalloc(ctx, &D.assert_idx, (size_t) na));
        if (na) HIPCHK(hipMemcpyAsync(D.assert_idx, d_sel, (size_t) na * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    }
    // ---- predicate buckets ----
    {
        const u32 nbk = 5 + 7 * (u32) i;
        if (nbk > 512) { ctx->err = "too many layers"; return VP_ELIMIT; }
        u32 *sk = nullptr, *sv = nullptr, *d_hist = nullptr;
        VPCHK(up_tmp(ctx, S, &sk, (size_t) 2 * n)); VPCHK(up_tmp(ctx, S, &sv, (size_t) 2 * n)); VPCHK(up_tmp(ctx, S, &d_hist, (size_t) nbk));
        HIPCHK(hipMemsetAsync(d_hist, 0, nbk * sizeof(u32), ctx->stream));
        VPCHK(up_sort_pairs(ctx, S, bkey, sk, iota2, sv, 2 * n, 10));          // valid buckets < 512, the padding key has bit 9 set
        hipLaunchKernelGGL(k_up_bucket_hist, dim3(grid_for((u64) 2 * n)), dim3(VP_BLOCK), 0, ctx->stream, bkey, 2 * n, nbk, d_hist);
        std::vector<u32> hist(nbk);
        HIPCHK(hipMemcpyAsync(hist.data(), d_hist, nbk * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        std::vector<u32> cbeg, cend, bptr(1, 0);
        u32 tot = 0;
        for (u32 b = 0; b < nbk; ++b) {
            const u32 start = tot; tot += hist[b];
            for (u32 q = start; q < tot; q += 512) { cbeg.push_back(q); cend.push_back(std::min<u32>(tot, q + 512)); }
            bptr.push_back((u32) cbeg.size());
        }
        D.p_chunks = (u32) cbeg.size(); D.p_buckets = nbk;
        VPCHK(dalloc(ctx, &D.p_idx, (size_t) tot)); VPCHK(dalloc(ctx, &D.p_flag, (size_t) tot));
        if (tot) {
            HIPCHK(hipMemcpyAsync(D.p_idx, sv, (size_t) tot * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_up_pflag, dim3(nblk(tot)), dim3(VP_BLOCK), 0, ctx->stream, sk, D.p_idx, tot, asf, D.p_flag);
        }
        VPCHK(dupload(ctx, &D.p_cbeg, cbeg)); VPCHK(dupload(ctx, &D.p_cend, cend)); VPCHK(dupload(ctx, &D.p_bptr, bptr));
    }
    // ---- contribution lists ----
    VPCHK(build_csr_dev(ctx, S, D.c1, (u32) ld[i - 1].size, n, key1, iota2, D.gv, d_etl, ctx->d_val_off));
    VPCHK(build_csr_dev(ctx, S, D.c2, D.p2_total, n, key2, iota2, D.gu, d_etl, nullptr));
    if (ctx->gen_rec_ok && (ctx->opt.gen_rec & 1)) {
        VPCHK(dalloc(ctx, &D.s_gidx, (size_t) D.p2_total));
        if (D.p2_total) hipLaunchKernelGGL(k_up_sgidx, dim3(nblk(D.p2_total)), dim3(VP_BLOCK), 0, ctx->stream, D.s_layer, D.s_idx, ctx->d_val_off, D.p2_total, D.s_gidx);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    up_release(S);
    return VP_OK;
}

// Liu gather lists of layer i over the wires of layer i-1 (dadId[k][i-1] of every later layer k inverted; src/prover.cpp:396,402-414)
int upload_liu_dev(vp_ctx *ctx, UpScratch &S, int i) {
    LayerDev &D = ctx->L[i];
    const u32 rows = (u32) ctx->L[i - 1].size;
    u64 total = 0;
    for (int k = i; k < ctx->n_layers; ++k) total += ctx->L[k].dad_size[i - 1];
    if (total > 0xffffffffull) { ctx->err = "Liu lists too long"; return VP_ELIMIT; }
    const u32 tn = (u32) total;
    u32 *kcat = nullptr, *gcat = nullptr, *iota = nullptr, *ks = nullptr, *sidx = nullptr; uint8_t *qcat = nullptr;
    VPCHK(up_tmp(ctx, S, &kcat, (size_t) tn)); VPCHK(up_tmp(ctx, S, &gcat, (size_t) tn)); VPCHK(up_tmp(ctx, S, &qcat, (size_t) tn));
    VPCHK(up_tmp(ctx, S, &iota, (size_t) tn)); VPCHK(up_tmp(ctx, S, &ks, (size_t) tn)); VPCHK(up_tmp(ctx, S, &sidx, (size_t) tn));
    u32 at = 0; int q = 1;
    for (int k = i; k < ctx->n_layers; ++k) {
        const u32 m = (u32) ctx->L[k].dad_size[i - 1];
        if (!m) continue;
        HIPCHK(hipMemcpyAsync(kcat + at, ctx->L[k].dad_id[i - 1], (size_t) m * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_up_liu_fill, dim3(nblk(m)), dim3(VP_BLOCK), 0, ctx->stream, gcat, qcat, at, m, (uint8_t) q);
        at += m; ++q;
    }
    if (tn) hipLaunchKernelGGL(k_up_iota, dim3(nblk(tn)), dim3(VP_BLOCK), 0, ctx->stream, iota, tn, 0u);
    VPCHK(dalloc(ctx, &D.lrow, (size_t) rows + 1)); VPCHK(dalloc(ctx, &D.l_g, (size_t) tn)); VPCHK(dalloc(ctx, &D.l_q, (size_t) tn));
    VPCHK(up_sort_pairs(ctx, S, kcat, ks, iota, sidx, tn, bits_for(std::max<u64>(2, rows))));
    hipLaunchKernelGGL(k_up_rowptr, dim3(nblk((u64) rows + 1)), dim3(VP_BLOCK), 0, ctx->stream, ks, tn, D.lrow, rows);
    if (tn) hipLaunchKernelGGL(k_up_liu_gather, dim3(nblk(tn)), dim3(VP_BLOCK), 0, ctx->stream, sidx, tn, gcat, qcat, D.l_g, D.l_q);
    D.l_n = tn;
    if (ctx->gen_rec_ok && (ctx->opt.gen_rec & 2)) {
        VPCHK(dalloc(ctx, &D.l_rec, (size_t) rows)); VPCHK(dalloc(ctx, &D.l_bf, (size_t) tn)); VPCHK(dalloc(ctx, &D.l_bs, (size_t) tn));
        hipLaunchKernelGGL(k_up_liu_rec, dim3(nblk(std::max<u64>(rows, tn))), dim3(VP_BLOCK), 0, ctx->stream, D.lrow, D.l_q, D.l_g, D.liu_H, ctx->half_pool, rows, tn,
                           D.l_rec, D.l_bf, D.l_bs);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    up_release(S);
    return VP_OK;
}

}  // namespace
