#include "vphost.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "circuit.hpp"
#include "fft_gkr_fs.hpp"
#include "gkr_fs.hpp"
#include "pc_fs.hpp"
#include "prover.hpp"
#include "verifier.hpp"

struct vph_circuit { layeredCircuit c; };
struct vph_session {
    vph_circuit *circ;
    std::unique_ptr<prover> p;
    std::vector<F> tape;
    std::vector<uint8_t> fri_roots; std::vector<F> fri_final, fri_r;      // FRI commit phase of the last complete-protocol run
    std::vector<uint8_t> full_record;                                     // record of the last accepted complete-protocol run (vph_last_full_record)
    std::vector<F> fft_gkr_msgs; double pc_times[3] = {0, 0, 0};          // fft_gkr messages; {PC prove (reference definition), of which fft_gkr, query answering}
    double verify_split[4] = {0, 0, 0, 0};                               // vph_last_verify_split
    double t_init = 0, t_round = 0, t_fin = 0;
    std::vector<F> last_point;                                           // r_liu after the last Liu sumcheck of the last complete-protocol run
    std::vector<F> ptape_fft, ptape_fri;                                 // vph_draw_protocol_tape: the draws after the GKR tape (fft_gkr, FRI folds)
    // vph_prove_protocol_ex: where the device's results land (the calls of a deferred pass write them when the pass is collected)
    std::vector<uint8_t> pp_gkr, pp_roots; std::vector<F> pp_all, pp_final; F pp_inner; uint64_t pp_written = 0;
    uint8_t pp_root_l[32], pp_root_h[32], pp_root_next[32];
    bool head_queued = false; uint64_t head_epoch = 0;                   // the previous pass queued this one's commit_private (VPH_PASS_QUEUE_NEXT)
};

static void set_err(char *err, int errlen, const std::string &m) {
    if (err && errlen > 0) { strncpy(err, m.c_str(), errlen - 1); err[errlen - 1] = 0; }
}

extern "C" {

vph_circuit *vph_circuit_from_pws(const char *path, int blocks, long seed, char *err, int errlen) {
    if (!path || blocks < 1) { set_err(err, errlen, "bad arguments"); return nullptr; }
    if (seed >= 0) srandom((unsigned) seed);
    std::string e;
    vph_circuit *vc = new vph_circuit();
    const char *route = getenv("VPH_BUILD");                 // "dag": the loader's own route (DAG of all blocks) for any block count
    if (blocks > 1 && !(route && !strcmp(route, "dag"))) {
        if (!vph::build_replicated(path, blocks, vc->c, &e)) { delete vc; set_err(err, errlen, e); return nullptr; }
        return vc;
    }
    std::vector<DAG_gate> dag;
    if (!vph::parse_pws(path, blocks, dag, &e)) { delete vc; set_err(err, errlen, e); return nullptr; }
    vc->c = vph::DAG_to_layered(dag);
    vc->c.subsetInit();
    return vc;
}
vph_circuit *vph_circuit_randomize(int layers, int log_size, long seed) {
    if (layers < 2 || log_size < 0 || log_size > 28) return nullptr;
    if (seed >= 0) srandom((unsigned) seed);
    vph_circuit *vc = new vph_circuit();
    vc->c = layeredCircuit::randomize(layers, log_size);
    vc->c.subsetInit();
    return vc;
}
vph_circuit *vph_circuit_custom(int n_layers, const uint64_t *layer_sizes, const int32_t *ty, const int32_t *l, const uint64_t *u,
                                const uint64_t *v, const uint64_t *c_pairs, const uint8_t *is_assert) {
    vph_circuit *vc = new vph_circuit();
    layeredCircuit &c = vc->c;
    c.size = n_layers;
    c.circuit.resize(n_layers);
    u64 at = 0;
    for (int i = 0; i < n_layers; ++i) {
        layer &L = c.circuit[i];
        L.size = layer_sizes[i];
        L.bitLength = 0;
        while ((1ull << L.bitLength) < L.size) ++L.bitLength;
        L.gates.resize(L.size);
        for (u64 g = 0; g < L.size; ++g, ++at) {
            F cc; cc.real = c_pairs[2 * at]; cc.img = c_pairs[2 * at + 1];
            L.gates[g] = gate((gateType) ty[at], l[at], u[at], v[at], cc, is_assert[at] != 0);
        }
    }
    c.subsetInit();
    return vc;
}
void vph_circuit_free(vph_circuit *c) { delete c; }
int vph_circuit_layers(const vph_circuit *c) { return c->c.size; }
uint64_t vph_circuit_gates(const vph_circuit *c) { u64 n = 0; for (auto &l : c->c.circuit) n += l.size; return n; }
uint64_t vph_circuit_layer_size(const vph_circuit *c, int layer) { return c->c.circuit[layer].size; }
int vph_circuit_layer_bitlen(const vph_circuit *c, int layer) { return c->c.circuit[layer].bitLength; }
void vph_circuit_hash(const vph_circuit *c, uint64_t out[2]) { u64 h[2]; c->c.structuralHash(h); out[0] = h[0]; out[1] = h[1]; }

vph_session *vph_session_create(vph_circuit *c, int device, char *err, int errlen) { return vph_session_create_opts(c, device, nullptr, err, errlen); }
vph_session *vph_session_create_opts(vph_circuit *c, int device, const vp_options *opt, char *err, int errlen) {
    if (!c) { set_err(err, errlen, "null circuit"); return nullptr; }
    try {
        std::unique_ptr<vph_session> s(new vph_session());
        s->circ = c;
        s->p.reset(new prover(c->c, device, opt));
        return s.release();
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return nullptr;
    }
}
vph_session *vph_session_create_round_sharded(vph_circuit *c, const int *devices, int world, int min_log, const vp_options *opt, char *err, int errlen) {
    return vph_session_create_sharded(c, devices, world, min_log, 0, opt, err, errlen);
}
vph_session *vph_session_create_sharded(vph_circuit *c, const int *devices, int world, int min_log, int shard_commitment, const vp_options *opt, char *err, int errlen) {
    if (!c || !devices || world < 1) { set_err(err, errlen, "null circuit / device list"); return nullptr; }
    try {
        std::unique_ptr<vph_session> s(new vph_session());
        s->circ = c;
        s->p.reset(new prover(c->c, std::vector<int>(devices, devices + world), min_log, opt, shard_commitment != 0));
        return s.release();
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return nullptr;
    }
}
void *vph_session_rank_ctx(vph_session *s, int rank) { return s ? (void *) s->p->rankContext(rank) : nullptr; }
int vph_session_world(vph_session *s) { return s ? s->p->world() : 0; }
int vph_session_partials(vph_session *s, vp_F *out, int capacity) {
    if (!s) return -1;
    const auto &pl = s->p->partials();
    for (size_t i = 0; i < pl.size() && (int) i < capacity; ++i)
        for (int q = 0; q < 3; ++q) { out[3 * i + q].real = pl[i][q].real; out[3 * i + q].img = pl[i][q].img; }
    return (int) pl.size();
}
void vph_session_clear_partials(vph_session *s) { if (s) s->p->clearPartials(); }
void vph_session_drop_rank(vph_session *s, int rank) { if (s) s->p->setDropRank(rank); }
double vph_session_gather_sec(vph_session *s) { return s ? s->p->gatherTime() : 0; }
void vph_session_free(vph_session *s) { delete s; }
int vph_set_profiling(vph_session *s, int level) { s->p->setLaunchLog(level != 0); return vp_set_profiling(s->p->context(), level); }
int vph_verifier_launches(vph_session *s, vp_launch_stat *out, int capacity) {
    if (!s || (capacity > 0 && !out)) return -1;
    const auto &v = s->p->verifierLaunches();
    for (int i = 0; i < (int) v.size() && i < capacity; ++i) out[i] = v[i];
    return (int) v.size();
}
void *vph_session_ctx(vph_session *s) { return s ? (void *) s->p->context() : nullptr; }

int vph_layer_values(vph_session *s, int layer, uint64_t *out, uint64_t n) {
    try {
        std::vector<F> v = s->p->layerValues(layer);
        if (n > v.size()) return -1;
        for (u64 i = 0; i < n; ++i) { out[2 * i] = v[i].real; out[2 * i + 1] = v[i].img; }
        return 0;
    } catch (const std::exception &) { return -2; }
}

static void fill(vph_result *res, prover &p, double prove_sec, double verify_sec, bool ok) {
    if (!res) return;
    vp_stats st = p.stats();
    res->prove_sec = prove_sec; res->gkr_device_ms = st.gkr_ms; res->evaluate_ms = st.evaluate_ms;
    res->verify_sec = verify_sec; res->fold_ms = st.fold_ms; res->fold_launches = st.fold_launches;
    res->fold_bytes = st.fold_bytes; res->rounds = st.rounds; res->launches = st.launches;
    res->proof_kb = p.proofSize(); res->verified = ok ? 1 : 0;
}

// seconds the interactive entry points spent in phase inits / round messages / finalize calls during the last vph_prove_interactive
void vph_interactive_breakdown(vph_session *s, double out[3]) { out[0] = s->t_init; out[1] = s->t_round; out[2] = s->t_fin; }

int vph_prove_interactive(vph_session *s, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, vph_result *res,
                          char *err, int errlen) {
    try {
        F::init();
        verifier v(s->p.get(), s->circ->c);
        const double t0 = s->p->proveTime();
        const double i0 = s->p->initTime(), r0 = s->p->roundTime(), f0 = s->p->finalizeTime();
        struct Keep { vph_session *s; double i0, r0, f0; ~Keep() { s->t_init = s->p->initTime() - i0; s->t_round = s->p->roundTime() - r0; s->t_fin = s->p->finalizeTime() - f0; } } keep{s, i0, r0, f0};
        const bool ok = v.verify();
        const auto &tr = v.transcript();
        if (tr.size() > capacity) { set_err(err, errlen, "transcript buffer too small"); return -1; }
        memcpy(transcript, tr.data(), tr.size());
        if (n_written) *n_written = tr.size();
        fill(res, *s->p, s->p->proveTime() - t0, v.verifyTime(), ok);
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_prove_fs(vph_session *s, uint8_t *proof, uint64_t capacity, uint64_t *n_written, vph_result *res, char *err, int errlen) {
    return vph_prove_fs_ex(s, proof, capacity, n_written, res, 0, err, errlen);
}
int vph_prove_fs_ex(vph_session *s, uint8_t *proof, uint64_t capacity, uint64_t *n_written, vph_result *res, int flags, char *err, int errlen) {
    if (flags & VPH_FS_DEVICE_GKR) {       // the prover alone: one device pass, nothing verified (vph_verify_fs is the check)
        if (!s || !proof) { set_err(err, errlen, "vph_prove_fs_ex: a null argument"); return -1; }
        try {
            verifier v(s->p.get(), s->circ->c);
            const double t0 = s->p->proveTime();
            v.proveFSDevice();
            const auto &tr = v.transcript();
            if (tr.size() > capacity) { set_err(err, errlen, "proof buffer too small"); return -1; }
            memcpy(proof, tr.data(), tr.size());
            if (n_written) *n_written = tr.size();
            fill(res, *s->p, s->p->proveTime() - t0, 0, false);
            if (res) res->proof_kb = (double) tr.size() / 1024.0;
            return 0;
        } catch (const std::exception &e) {
            set_err(err, errlen, e.what());
            return -2;
        }
    }
    try {
        verifier v(s->p.get(), s->circ->c);
        const double t0 = s->p->proveTime();
        const bool ok = v.proveFS();
        const auto &tr = v.transcript();
        if (tr.size() > capacity) { set_err(err, errlen, "proof buffer too small"); return -1; }
        memcpy(proof, tr.data(), tr.size());
        if (n_written) *n_written = tr.size();
        fill(res, *s->p, s->p->proveTime() - t0, v.verifyTime(), ok);
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_verify_fs(vph_circuit *c, const uint8_t *proof, uint64_t n) {
    try {
        verifier v(nullptr, c->c);
        std::vector<uint8_t> tr(proof, proof + n);
        return v.checkFS(tr) ? 0 : 1;
    } catch (const std::exception &) { return 1; }
}

int vph_draw_tape(vph_session *s) {
    F::init();
    verifier v(nullptr, s->circ->c);
    s->tape = v.drawTape();
    return 0;
}

// a caller's tape: the layout and length of verifier::drawTape(), canonical limbs
static bool tape_fits(const layeredCircuit &c, const uint64_t *pairs, uint64_t n, std::vector<F> &out) {
    if (!pairs) return false;
    int max_bl = 0;
    for (int i = 0; i < c.size; ++i) max_bl = std::max(max_bl, c.circuit[i].bitLength);
    uint64_t want = c.circuit[c.size - 1].bitLength;
    for (int i = c.size - 1; i; --i) want += 2 * (uint64_t) max_bl + 1 + c.size + (c.circuit[i].maxDadBitLength != -1 ? c.circuit[i].maxDadBitLength : 0);
    if (n != want) return false;
    const uint64_t p = (1ull << 61) - 1;
    for (uint64_t i = 0; i < 2 * n; ++i) if (pairs[i] >= p) return false;
    out.resize(n);
    for (uint64_t i = 0; i < n; ++i) { out[i].real = pairs[2 * i]; out[i].img = pairs[2 * i + 1]; }
    return true;
}

int vph_set_tape(vph_session *s, const uint64_t *tape_pairs, uint64_t n) {
    std::vector<F> t;
    if (!s || !tape_fits(s->circ->c, tape_pairs, n, t)) return -1;
    s->tape.swap(t);
    return 0;
}

int vph_prove_gkr(vph_session *s, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, vph_result *res, char *err,
                  int errlen) {
    try {
        if (s->tape.empty()) vph_draw_tape(s);
        std::vector<uint8_t> tr;
        const double t0 = s->p->proveTime();
        s->p->proveGKR(s->tape, tr);
        if (tr.size() > capacity) { set_err(err, errlen, "transcript buffer too small"); return -1; }
        memcpy(transcript, tr.data(), tr.size());
        if (n_written) *n_written = tr.size();
        fill(res, *s->p, s->p->proveTime() - t0, 0, false);
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

double vph_commit_device_ms(vph_session *s) { double ms = -1; vp_commit_stats(s->p->context(), &ms); return ms; }

int vph_set_shard(vph_session *s, int rank, int world) { return vp_set_shard(s->p->context(), rank, world) == VP_OK ? 0 : -1; }

// index-split proof, caller-side exchange of V_u (include/vpgpu.h: vp_shard_vu_partials / vp_shard_vu_set) on the session's tape; -> n, < 0: refused
int vph_shard_vu_partials(vph_session *s, uint64_t *partials /* 2 per entry */, int capacity) {
    if (s->tape.empty()) vph_draw_tape(s);
    uint64_t n = 0;
    static_assert(sizeof(F) == sizeof(vp_F), "field element layout");
    const int rc = vp_shard_vu_partials(s->p->context(), reinterpret_cast<const vp_F *>(s->tape.data()), s->tape.size(), reinterpret_cast<vp_F *>(partials), (uint64_t) capacity, &n);
    return rc == VP_OK ? (int) n : -1;
}
int vph_shard_vu_set(vph_session *s, const uint64_t *sums, int n) {
    return vp_shard_vu_set(s->p->context(), reinterpret_cast<const vp_F *>(sums), (uint64_t) n) == VP_OK ? 0 : -1;
}

int vph_shard_chains(vph_session *s, int32_t *owner, double *cost, int capacity) {
    int n = 0;
    return vp_shard_chains(s->p->context(), owner, cost, capacity, &n) == VP_OK ? n : -1;
}

int vph_check(vph_session *s, const uint8_t *transcript, uint64_t n, int skip_predicates, double *verify_sec) {
    try {
        verifier v(nullptr, s->circ->c);
        v.skip_predicates = (skip_predicates & 1) != 0;
        if (skip_predicates & 2) v.pred_dev = s->p.get();          // bit 1: predicate loops on the device
        std::vector<uint8_t> tr(transcript, transcript + n);
        timer t; t.start();
        const bool ok = v.check(s->tape, tr);
        t.stop();
        if (verify_sec) *verify_sec = t.elapse_sec();
        return ok ? 0 : 1;
    } catch (const std::exception &) { return -2; }
}

int vph_commit_private(vph_session *s, uint8_t root[32], double *ms, char *err, int errlen) {
    try {
        prover::hhash_digest d = s->p->commit_private();
        memcpy(root, d.b, 32);
        if (ms) *ms = s->p->commitDeviceMs();
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_commit_public(vph_session *s, const uint64_t *pub_pairs, uint64_t n_pub, uint8_t *out, double *ms, char *err, int errlen) {
    try {
        std::vector<F> pub(n_pub), all_sum;
        for (u64 i = 0; i < n_pub; ++i) { pub[i].real = pub_pairs[2 * i]; pub[i].img = pub_pairs[2 * i + 1]; }
        F inner;
        prover::hhash_digest d = s->p->commit_public(pub, inner, all_sum);
        memcpy(out, d.b, 32);
        memcpy(out + 32, &inner, 16);
        memcpy(out + 48, all_sum.data(), 65 * 16);
        if (ms) *ms = s->p->commitDeviceMs();
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_commit_private_masked(vph_session *s, const uint64_t *mask_pairs, uint64_t n_mask, uint8_t root[32], double *ms, char *err, int errlen) {
    try {
        std::vector<F> mask(n_mask);
        for (u64 i = 0; i < n_mask; ++i) { mask[i].real = mask_pairs[2 * i]; mask[i].img = mask_pairs[2 * i + 1]; }
        prover::hhash_digest d = s->p->commit_private(mask);
        memcpy(root, d.b, 32);
        if (ms) *ms = s->p->commitDeviceMs();
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_commit_public_eq(vph_session *s, const uint64_t *point_pairs, int n_point, uint8_t *out, double *ms, char *err, int errlen) {
    try {
        std::vector<F> point((size_t) std::max(0, n_point)), all_sum;
        for (int i = 0; i < n_point; ++i) { point[i].real = point_pairs[2 * i]; point[i].img = point_pairs[2 * i + 1]; }
        F inner;
        prover::hhash_digest d = s->p->commit_public_eq(point, inner, all_sum);
        memcpy(out, d.b, 32);
        memcpy(out + 32, &inner, 16);
        memcpy(out + 48, all_sum.data(), 65 * 16);
        if (ms) *ms = s->p->commitDeviceMs();
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_commit_public_eq_masked(vph_session *s, const uint64_t *point_pairs, int n_point, const uint64_t *mask_pairs, uint64_t n_mask, uint8_t *out, double *ms, char *err, int errlen) {
    try {
        std::vector<F> point((size_t) std::max(0, n_point)), mask(mask_pairs ? n_mask : 0), all_sum;
        for (int i = 0; i < n_point; ++i) { point[i].real = point_pairs[2 * i]; point[i].img = point_pairs[2 * i + 1]; }
        for (u64 i = 0; i < mask.size(); ++i) { mask[i].real = mask_pairs[2 * i]; mask[i].img = mask_pairs[2 * i + 1]; }
        F inner;
        prover::hhash_digest d = s->p->commit_public_eq(point, mask, inner, all_sum);
        memcpy(out, d.b, 32);
        memcpy(out + 32, &inner, 16);
        memcpy(out + 48, all_sum.data(), 65 * 16);
        if (ms) *ms = s->p->commitDeviceMs();
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_fri_open_many(vph_session *s, int n, const int32_t *oracle, const uint64_t *leaf, uint64_t *values_pairs, uint8_t *paths, int path_stride,
                      int32_t *path_len, char *err, int errlen) {
    try {
        if (n < 0 || path_stride < 0 || path_stride % 32) throw std::runtime_error("vph_fri_open_many: path_stride must be a multiple of 32 bytes");
        std::vector<int32_t> o(oracle, oracle + n), len;
        std::vector<u64> lf(leaf, leaf + n);
        std::vector<F> values;
        std::vector<prover::hhash_digest> pt;
        s->p->friOpenMany(o, lf, values, pt, path_stride / 32, len);
        for (int i = 0; i < n; ++i) {
            memcpy(values_pairs + (size_t) 260 * i, values.data() + (size_t) 130 * i, 130 * sizeof(F));
            memcpy(paths + (size_t) path_stride * i, pt.data() + (size_t) (path_stride / 32) * i, 32 * (size_t) len[i]);
            path_len[i] = len[i];
        }
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_fri_query(vph_session *s, int n_queries, const uint64_t *leaf0, uint8_t *out, uint64_t capacity, uint64_t *n_written, char *err, int errlen) {
    try {
        const std::vector<uint8_t> a = s->p->friQuery(std::vector<u64>(leaf0, leaf0 + std::max(0, n_queries)));
        if (n_written) *n_written = a.size();
        if (a.size() > capacity) { set_err(err, errlen, "vph_fri_query: output buffer too small"); return -1; }
        memcpy(out, a.data(), a.size());
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

static std::vector<F> pc_elems(const uint64_t *pairs, uint64_t n_elems);
int vph_prove_and_verify_full(vph_session *s, int reps, uint8_t *transcript, uint64_t capacity, uint64_t *n_written,
                              double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec, char *err, int errlen) {
    return vph_prove_and_verify_full_ex(s, reps, 0, transcript, capacity, n_written, gkr_prove_sec, pc_prove_sec, verify_sec, err, errlen);
}
int vph_prove_and_verify_full_ex(vph_session *s, int reps, int flags, uint8_t *transcript, uint64_t capacity, uint64_t *n_written,
                                 double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec, char *err, int errlen) {
    return vph_prove_and_verify_full_masked(s, reps, flags, nullptr, 0, nullptr, 0, transcript, capacity, n_written, gkr_prove_sec, pc_prove_sec, verify_sec, err, errlen);
}
int vph_prove_and_verify_full_masked(vph_session *s, int reps, int flags, const uint64_t *pri_mask_pairs, uint64_t n_pri, const uint64_t *pub_mask_pairs, uint64_t n_pub,
                                     uint8_t *transcript, uint64_t capacity, uint64_t *n_written, double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec,
                                     char *err, int errlen) {
    try {
        for (uint64_t i = 0; pri_mask_pairs && i < 2 * n_pri; ++i) if (pri_mask_pairs[i] >= F::mod) throw std::runtime_error("vph_prove_and_verify_full_masked: non-canonical mask element");
        for (uint64_t i = 0; pub_mask_pairs && i < 2 * n_pub; ++i) if (pub_mask_pairs[i] >= F::mod) throw std::runtime_error("vph_prove_and_verify_full_masked: non-canonical mask element");
        const std::vector<F> pri_mask = pc_elems(pri_mask_pairs, pri_mask_pairs ? n_pri : 0), pub_mask = pc_elems(pub_mask_pairs, pub_mask_pairs ? n_pub : 0);
        F::init();
        verifier v(s->p.get(), s->circ->c);
        v.batched_openings = (flags & VPH_VERIFY_BATCHED_OPENINGS) != 0;
        if (flags & VPH_VERIFY_DEVICE_LOOPS) { v.pred_dev = s->p.get(); v.poly_dev = s->p.get(); }
        const double t0 = s->p->proveTime();
        const bool ok = v.verifyFull(reps, pri_mask, pub_mask);
        s->full_record = v.fullRecord();
        s->fri_roots = v.friRoots(); s->fri_final = v.friFinalCode(); s->fri_r = v.friChallenges();
        s->fft_gkr_msgs = v.fftGkrMessages();
        s->pc_times[0] = v.polyProveTime(); s->pc_times[1] = v.fftGkrProveTime(); s->pc_times[2] = v.polyOpenTime();
        s->last_point.assign(v.finalPoint().begin(), v.finalPoint().begin() + s->circ->c.circuit[0].bitLength);
        const auto &tr = v.fullTranscript();
        if (tr.size() > capacity) { set_err(err, errlen, "transcript buffer too small"); return -1; }
        memcpy(transcript, tr.data(), tr.size());
        if (n_written) *n_written = tr.size();
        if (gkr_prove_sec) *gkr_prove_sec = s->p->proveTime() - t0;
        if (pc_prove_sec) *pc_prove_sec = v.polyProveTime();
        if (verify_sec) *verify_sec = v.verifyTime() + v.polyVerifyTime();
        s->verify_split[0] = v.verifyTime(); s->verify_split[1] = v.publicEvalTime(); s->verify_split[2] = v.openingDigestTime();
        s->verify_split[3] = v.polyVerifyTime() - v.publicEvalTime() - v.openingDigestTime();
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_last_full_record(vph_session *s, uint8_t *buf, uint64_t cap, uint64_t *n) {
    if (!s || !n) return -1;
    *n = s->full_record.size();
    if (s->full_record.empty() || !buf || cap < s->full_record.size()) return -1;
    memcpy(buf, s->full_record.data(), s->full_record.size());
    return 0;
}
int vph_verify_full_record(vph_circuit *c, const uint8_t *record, uint64_t n) {
    if (!c || !record) return 1;
    try {
        F::init();
        verifier v(nullptr, c->c);
        return v.checkFull(std::vector<uint8_t>(record, record + n)) ? 0 : 1;
    } catch (const std::exception &) { return 1; }
}

int vph_verify_full_record_dev(vph_circuit *c, int device, const uint8_t *record, uint64_t n, char *err, int errlen) {
    if (!c || !record) return 1;
    try { return checkFullOnDevice(c->c, device, std::vector<uint8_t>(record, record + n)) ? 0 : 1; }
    catch (const std::exception &e) { set_err(err, errlen, e.what()); return -2; }
}
void vph_last_verify_split(vph_session *s, double out[4]) { for (int i = 0; i < 4; ++i) out[i] = s ? s->verify_split[i] : 0; }

static bool pc_args_ok(int n, const uint64_t *pairs, uint64_t n_elems, int n_queries, const uint64_t *leaf0) {
    if (n < 7 || n > 25 || n_queries < 1 || n_queries > 4096 || !leaf0) return false;
    for (int q = 0; q < n_queries; ++q) if (leaf0[q] < (1ull << (n - 7)) || leaf0[q] >= (1ull << (n - 2))) return false;
    for (uint64_t i = 0; pairs && i < 2 * n_elems; ++i) if (pairs[i] >= F::mod) return false;
    return true;
}
static std::vector<F> pc_elems(const uint64_t *pairs, uint64_t n_elems) {
    std::vector<F> v(n_elems);
    if (n_elems) memcpy(static_cast<void *>(v.data()), pairs, n_elems * sizeof(F));
    return v;
}
int vph_pc_public_evals_host(int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, int tensor, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs) {
    if (!out_pairs || (point_pairs == nullptr) == (pub_pairs == nullptr) || (tensor && !point_pairs)) return -1;
    if (!pc_args_ok(n, point_pairs ? point_pairs : pub_pairs, point_pairs ? (uint64_t) n : 1ull << n, n_queries, leaf0)) return -1;
    try {
        const std::vector<u64> lf(leaf0, leaf0 + n_queries);
        const std::vector<F> in = pc_elems(point_pairs ? point_pairs : pub_pairs, point_pairs ? (uint64_t) n : 1ull << n);
        const std::vector<F> out = !point_pairs ? pcPublicEvalsHostPub(n, in, lf) : tensor ? pcPublicEvalsHostTensor(n, in, lf) : pcPublicEvalsHost(n, in, lf);
        memcpy(out_pairs, out.data(), out.size() * sizeof(F));
        return 0;
    } catch (const std::exception &) { return -1; }
}
int vph_pc_opening_digests_host(int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out) {
    if (!answer || !out || !pc_args_ok(n, nullptr, 0, n_queries, leaf0)) return -1;
    try {
        const std::vector<uint8_t> d = pcOpeningDigestsHost(n, std::vector<u64>(leaf0, leaf0 + n_queries), answer, n_bytes);
        memcpy(out, d.data(), d.size());
        return 0;
    } catch (const std::exception &) { return -1; }
}
uint64_t vph_pc_query_answer_bytes(int n, int n_queries) { return (n < 7 || n_queries < 0) ? 0 : pcQueryAnswerBytes(n, (u64) n_queries); }
int vph_pc_public_evals(vph_session *s, int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs,
                        char *err, int errlen) {
    // the arguments go to the device library as they are: its refusals are what the caller sees
    vp_ctx *ctx = s->p->context();
    const int rc = vp_pc_public_evals(ctx, n, reinterpret_cast<const vp_F *>(point_pairs), reinterpret_cast<const vp_F *>(pub_pairs), n_queries, leaf0,
                                      reinterpret_cast<vp_F *>(out_pairs));
    if (rc != VP_OK) set_err(err, errlen, std::string("vp_pc_public_evals: ") + vp_last_error(ctx));
    return rc;
}
int vph_fri_query_digests(vph_session *s, int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out, char *err, int errlen) {
    vp_ctx *ctx = s->p->context();
    const int rc = vp_fri_query_digests(ctx, n, n_queries, leaf0, answer, n_bytes, out);
    if (rc != VP_OK) set_err(err, errlen, std::string("vp_fri_query_digests: ") + vp_last_error(ctx));
    return rc;
}

int vph_pc_mask_evals_host(int n, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs) {
    if (!out_pairs || !pub_mask_pairs || ms < 1 || (ms & (ms - 1)) || n_pub_mask < 1 || n_pub_mask > ms || n < 7 || n > 25 || ms > (1ull << (n - 2))) return -1;
    if (!pc_args_ok(n, pub_mask_pairs, n_pub_mask, n_queries, leaf0)) return -1;
    try {
        const std::vector<F> out = pcMaskEvalsHost(n, pc_elems(pub_mask_pairs, n_pub_mask), ms, std::vector<u64>(leaf0, leaf0 + n_queries));
        memcpy(out_pairs, out.data(), out.size() * sizeof(F));
        return 0;
    } catch (const std::exception &) { return -1; }
}
int vph_pc_mask_evals(vph_session *s, int n, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs,
                      char *err, int errlen) {
    vp_ctx *ctx = s->p->context();
    const int rc = vp_pc_mask_evals(ctx, n, reinterpret_cast<const vp_F *>(pub_mask_pairs), n_pub_mask, ms, n_queries, leaf0, reinterpret_cast<vp_F *>(out_pairs));
    if (rc != VP_OK) set_err(err, errlen, std::string("vp_pc_mask_evals: ") + vp_last_error(ctx));
    return rc;
}

int vph_verify_commitment(int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms,
                          const uint64_t *claim_pair, const uint8_t *root_l, const uint8_t *root_h, const uint64_t *all_sum_pairs, const uint64_t *r_pairs,
                          const uint8_t *fri_roots, const uint64_t *final_code_pairs, const uint64_t *final_mask_pairs, int reps, const uint64_t *leaf0,
                          const uint8_t *answer, uint64_t n_bytes, int device, char *err, int errlen) {
    auto bad = [&](const char *m) { set_err(err, errlen, m); return -1; };
    if (n < 7 || n > 25) return bad("vph_verify_commitment: n outside 7 .. 25");
    if ((point_pairs == nullptr) == (pub_pairs == nullptr)) return bad("vph_verify_commitment: exactly one of point and pub");
    if (!claim_pair || !root_l || !root_h || !all_sum_pairs || !r_pairs || !fri_roots || !final_code_pairs || !final_mask_pairs || !leaf0 || !answer)
        return bad("vph_verify_commitment: a null argument");
    if (reps < 1 || reps > 4096) return bad("vph_verify_commitment: 1 .. 4096 repetitions");
    if (pub_mask_pairs && n_pub_mask > ms) return bad("vph_verify_commitment: public mask longer than ms");
    const uint64_t n_mask = pub_mask_pairs ? n_pub_mask : 0;
    const struct { const uint64_t *p; uint64_t n; } elems[] = {{point_pairs, (uint64_t) n}, {pub_pairs, 1ull << n}, {pub_mask_pairs, n_mask}, {claim_pair, 1}, {all_sum_pairs, 65},
                                                                {r_pairs, (uint64_t) (n - 6)}, {final_code_pairs, 2048}, {final_mask_pairs, 32}};
    for (const auto &e : elems)
        for (uint64_t i = 0; e.p && i < 2 * e.n; ++i) if (e.p[i] >= F::mod) return bad("vph_verify_commitment: non-canonical field element in an argument");
    vp_ctx *ctx = nullptr;
    try {
        PcCommitment c;
        c.n = n;
        if (point_pairs) c.point = pc_elems(point_pairs, (uint64_t) n); else c.pub = pc_elems(pub_pairs, 1ull << n);
        c.pub_mask = pc_elems(pub_mask_pairs, n_mask);
        c.ms = ms;
        c.claim = pc_elems(claim_pair, 1)[0];
        memcpy(c.root_l, root_l, 32); memcpy(c.root_h, root_h, 32);
        c.all_sum = pc_elems(all_sum_pairs, 65);
        c.fr = pc_elems(r_pairs, (uint64_t) (n - 6));
        c.fri_roots.assign(fri_roots, fri_roots + 32 * (size_t) (n - 6));
        c.final_code = pc_elems(final_code_pairs, 2048);
        c.final_mask = pc_elems(final_mask_pairs, 32);
        c.leaf0.assign(leaf0, leaf0 + reps);
        c.answer = answer; c.n_bytes = n_bytes;
        if (device >= 0 && vp_create(device, &ctx) != VP_OK) { ctx = nullptr; throw std::runtime_error("vph_verify_commitment: no context on the device"); }
        std::string why;
        const int rc = pcVerifyCommitment(c, why, ctx);
        if (ctx) vp_destroy(ctx);
        if (rc) set_err(err, errlen, why);
        return rc;
    } catch (const std::exception &e) {
        if (ctx) vp_destroy(ctx);
        set_err(err, errlen, e.what());
        return -2;
    }
}

// ---- the non-interactive commitment proof (vphost.h: "The transcript chain", "Proof bytes") ----------------------------------------------------------------
int vph_commit_fs(vph_session *s, const uint64_t *point_pairs, int n_point, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs,
                  uint64_t n_pub_mask, int flags, uint8_t *out, uint64_t cap, uint64_t *len, char *err, int errlen) {
    return vph_commit_fs_pow(s, point_pairs, n_point, reps, mask_pairs, n_mask, pub_mask_pairs, n_pub_mask, flags, 0, out, cap, len, err, errlen);
}
int vph_commit_fs_pow(vph_session *s, const uint64_t *point_pairs, int n_point, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs,
                      uint64_t n_pub_mask, int flags, int pow_bits, uint8_t *out, uint64_t cap, uint64_t *len, char *err, int errlen) {
    if (!s || !point_pairs || n_point < 1 || !len || (n_mask && !mask_pairs) || (n_pub_mask && !pub_mask_pairs)) { set_err(err, errlen, "vph_commit_fs: a null argument"); return -1; }
    if (pow_bits < 0 || pow_bits > PCFS_POW_PROVER_BITS) { set_err(err, errlen, "vph_commit_fs_pow: pow_bits outside 0 .. 32"); return -1; }
    for (uint64_t i = 0; i < 2 * (uint64_t) n_point; ++i) if (point_pairs[i] >= F::mod) { set_err(err, errlen, "vph_commit_fs: non-canonical coordinate"); return -1; }
    try {
        const std::vector<uint8_t> proof = s->p->commitFS(pc_elems(point_pairs, (uint64_t) n_point), reps, pc_elems(mask_pairs, n_mask), pc_elems(pub_mask_pairs, n_pub_mask),
                                                          !(flags & VPH_FS_HOST_DRAWS), pow_bits);
        *len = proof.size();
        if (!out || cap < proof.size()) { set_err(err, errlen, "vph_commit_fs: output buffer too small (*len: the proof's size)"); return -1; }
        memcpy(out, proof.data(), proof.size());
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}
void vph_last_commit_fs_times(vph_session *s, double out[2]) { out[0] = s ? s->p->fsPhaseSec() : 0; out[1] = s ? s->p->fsPhaseDeviceMs() : 0; }
int vph_verify_commitment_fs(const uint8_t *proof, uint64_t len, int device, char *err, int errlen) { return vph_verify_commitment_fs_min(proof, len, device, 0, err, errlen); }
int vph_verify_commitment_fs_min(const uint8_t *proof, uint64_t len, int device, int min_pow_bits, char *err, int errlen) {
    vp_ctx *ctx = nullptr;
    try {
        PcCommitment c;
        std::string why;
        if (pcParseCommitmentFS(proof, len, c, why) != 0) { set_err(err, errlen, why); return -1; }      // malformed: before a context is made
        if (pcCheckWork(c.pow_bits, c.pow_nonce, c.pow_met, min_pow_bits, why)) { set_err(err, errlen, why); return 1; }      // one hash: before a context is made, too
        if (device >= 0 && vp_create(device, &ctx) != VP_OK) { ctx = nullptr; throw std::runtime_error("vph_verify_commitment_fs: no context on the device"); }
        const int rc = pcVerifyCommitment(c, why, ctx);
        if (ctx) vp_destroy(ctx);
        if (rc) set_err(err, errlen, why);
        return rc;
    } catch (const std::exception &e) {
        if (ctx) vp_destroy(ctx);
        set_err(err, errlen, e.what());
        return -2;
    }
}
int vph_commitment_fs_challenges(const uint8_t *proof, uint64_t len, uint64_t *r_pairs, uint64_t *leaf0) {
    try {
        PcCommitment c;
        std::string why;
        if (!r_pairs || !leaf0 || pcParseCommitmentFS(proof, len, c, why) != 0) return -1;
        memcpy(r_pairs, c.fr.data(), c.fr.size() * sizeof(F));
        for (size_t q = 0; q < c.leaf0.size(); ++q) leaf0[q] = c.leaf0[q];
        return 0;
    } catch (const std::exception &) { return -1; }
}

// ---- the joined non-interactive proof of the whole protocol (verifier::proveFullFS / checkFullFS) ----
int vph_prove_full_fs(vph_session *s, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                      uint64_t *len, uint64_t *point_pairs, char *err, int errlen) {
    return vph_prove_full_fs_pow(s, reps, mask_pairs, n_mask, pub_mask_pairs, n_pub_mask, out, cap, len, point_pairs, 0, 0, err, errlen);
}
int vph_prove_full_fs_ex(vph_session *s, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                         uint64_t *len, uint64_t *point_pairs, int flags, char *err, int errlen) {
    return vph_prove_full_fs_pow(s, reps, mask_pairs, n_mask, pub_mask_pairs, n_pub_mask, out, cap, len, point_pairs, flags, 0, err, errlen);
}
int vph_prove_full_fs_pow(vph_session *s, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                          uint64_t *len, uint64_t *point_pairs, int flags, int pow_bits, char *err, int errlen) {
    if (!s || !len || (n_mask && !mask_pairs) || (n_pub_mask && !pub_mask_pairs)) { set_err(err, errlen, "vph_prove_full_fs: a null argument"); return -1; }
    if (pow_bits < 0 || pow_bits > PCFS_POW_PROVER_BITS) { set_err(err, errlen, "vph_prove_full_fs_pow: pow_bits outside 0 .. 32"); return -1; }
    try {
        verifier v(s->p.get(), s->circ->c);
        const std::vector<uint8_t> proof = v.proveFullFS(reps, pc_elems(mask_pairs, n_mask), pc_elems(pub_mask_pairs, n_pub_mask), (flags & VPH_FS_DEVICE_GKR) != 0, pow_bits);
        *len = proof.size();
        if (!out || cap < proof.size()) { set_err(err, errlen, "vph_prove_full_fs: output buffer too small (*len: the proof's size)"); return -1; }
        memcpy(out, proof.data(), proof.size());
        if (point_pairs) memcpy(point_pairs, v.fullFsPoint().data(), v.fullFsPoint().size() * sizeof(F));
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}
int vph_verify_full_fs(vph_circuit *c, const uint8_t *proof, uint64_t len, int device, uint64_t *point_pairs, char *err, int errlen) {
    return vph_verify_full_fs_min(c, proof, len, device, 0, point_pairs, err, errlen);
}
int vph_verify_full_fs_min(vph_circuit *c, const uint8_t *proof, uint64_t len, int device, int min_pow_bits, uint64_t *point_pairs, char *err, int errlen) {
    if (!c) { set_err(err, errlen, "vph_verify_full_fs: no circuit"); return -1; }
    vp_ctx *ctx = nullptr;
    try {
        if (device >= 0 && vp_create(device, &ctx) != VP_OK) { ctx = nullptr; throw std::runtime_error("vph_verify_full_fs: no context on the device"); }
        verifier v(nullptr, c->c);
        std::string why;
        const int rc = v.checkFullFS(proof, len, why, ctx, min_pow_bits);
        if (ctx) vp_destroy(ctx);
        if (rc) set_err(err, errlen, why);
        if (point_pairs && !v.fullFsPoint().empty()) memcpy(point_pairs, v.fullFsPoint().data(), v.fullFsPoint().size() * sizeof(F));
        return rc;
    } catch (const std::exception &e) {
        if (ctx) vp_destroy(ctx);
        set_err(err, errlen, e.what());
        return -2;
    }
}

// ---- the proof of work (vphost.h, "The proof of work"): the host's search, and the two fields of either kind of proof ----
int vph_fs_grind_host(const uint8_t state_in[32], int bits, uint64_t first, uint64_t max_tries, uint64_t *nonce, uint8_t state_out[32]) {
    if (!state_in || !nonce || !state_out || bits < 1 || bits > PCFS_POW_MAX_BITS || max_tries == 0 || first + (max_tries - 1) < first) return -1;
    vph::fs_chain ch;
    memcpy(ch.s.w, state_in, 32);
    uint64_t found = 0;
    if (!vph::fs_grind(ch.s, bits, first, max_tries, &found)) return -5;
    ch.work((uint64_t) bits, found);
    *nonce = found;
    memcpy(state_out, ch.s.w, 32);
    return 0;
}
int vph_fs_pow(const uint8_t *proof, uint64_t len, uint64_t *bits, uint64_t *nonce) {
    if (!proof || !bits || !nonce || len < 32) return -1;
    uint32_t h32[2];
    memcpy(h32, proof, 8);
    if ((h32[0] != PCFS_MAGIC && h32[0] != 0x46465056u) || (h32[1] != PCFS_VERSION && h32[1] != PCFS_VERSION_POW)) return -1;
    PcFsWork w;
    if (h32[1] == PCFS_VERSION_POW && (len < 48 || !pcFsWorkHeader(proof + 32, w))) return -1;
    *bits = w.bits; *nonce = w.nonce;
    return 0;
}

// ---- the GKR part of the chain (vphost.h, "The GKR part on the device"): sizes, the derivation alone (gkr_fs.hpp), the device call ----
int vph_gkr_sizes(const vph_circuit *c, uint64_t *n_tape, uint64_t *n_transcript_bytes) {
    if (!c || c->c.size < 2) return -1;
    const vph::GkrLayout L(c->c);
    if (n_tape) *n_tape = L.n_tape;
    if (n_transcript_bytes) *n_transcript_bytes = L.n_tr * sizeof(F);
    return 0;
}
int vph_gkr_fs_tape(const vph_circuit *c, const uint8_t state_in[32], const uint8_t *transcript, uint64_t n, uint64_t *tape_pairs, uint64_t *n_draws, uint8_t state_out[32]) {
    if (!c || c->c.size < 2 || !state_in || !transcript || !tape_pairs || !n_draws || !state_out) return -1;
    try {
        const vph::GkrLayout L(c->c);
        if (n != L.n_tr * sizeof(F)) return -1;                    // truncated or over-long
        std::vector<F> tr(L.n_tr), tape(L.n_tape);
        memcpy(static_cast<void *>(tr.data()), transcript, n);
        for (const F &x : tr) if (x.real >= F::mod || x.img >= F::mod) return -1;
        vph::fs_chain ch;
        memcpy(ch.s.w, state_in, 32);
        *n_draws = vph::gkrFsTape(c->c, L, ch, tr.data(), tape.data());
        if (L.n_tape) memcpy(tape_pairs, tape.data(), L.n_tape * sizeof(F));
        memcpy(state_out, ch.s.w, 32);
        return 0;
    } catch (const std::exception &) { return -1; }
}
int vph_prove_gkr_fs(vph_session *s, const uint8_t state_in[32], uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint64_t *tape_pairs, uint64_t *n_draws,
                     uint8_t state_out[32], char *err, int errlen) {
    if (!s || !state_in || !transcript || !tape_pairs || !n_draws || !state_out) { set_err(err, errlen, "vph_prove_gkr_fs: a null argument"); return -1; }
    try {
        const vph::GkrLayout L(s->circ->c);
        if (capacity < L.n_tr * sizeof(F)) { set_err(err, errlen, "vph_prove_gkr_fs: transcript buffer size (vph_gkr_sizes)"); return -1; }
        uint8_t st[32];
        memcpy(st, state_in, 32);
        std::vector<F> tape;
        u64 draws = 0;
        const std::vector<uint8_t> tr = s->p->proveGkrFS(st, tape, draws);
        memcpy(transcript, tr.data(), tr.size());
        if (n_written) *n_written = tr.size();
        if (!tape.empty()) memcpy(tape_pairs, tape.data(), tape.size() * sizeof(F));
        *n_draws = draws;
        memcpy(state_out, st, 32);
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

// fft_gkr's part of the chain, the derivation alone (fft_gkr_fs.hpp): the tape and the closing state of vp_fft_gkr_fs from its messages
static bool fgk_pairs_ok(int lg, const uint64_t *pairs, uint64_t n, uint64_t want) {
    if (lg < 1 || lg > 19 || !pairs || n != want) return false;
    for (uint64_t i = 0; i < 2 * n; ++i) if (pairs[i] >= 2305843009213693951ull) return false;
    return true;
}
int vph_fft_gkr_fs_tape(int lg, const uint8_t state_in[32], const uint64_t *msgs_pairs, uint64_t n_msgs, uint64_t *tape_pairs, uint8_t state_out[32]) {
    if (lg < 1 || lg > 19) return -1;
    const vph::FftGkrLayout L(lg);
    if (!state_in || !tape_pairs || !state_out || !fgk_pairs_ok(lg, msgs_pairs, n_msgs, L.n_msgs)) return -1;
    try {
        std::vector<F> msgs(L.n_msgs), tape(L.n_tape);
        memcpy(static_cast<void *>(msgs.data()), msgs_pairs, L.n_msgs * sizeof(F));
        vph::fs_chain ch;
        memcpy(ch.s.w, state_in, 32);
        vph::fftGkrFsTape(lg, ch, msgs.data(), tape.data());
        memcpy(tape_pairs, tape.data(), L.n_tape * sizeof(F));
        memcpy(state_out, ch.s.w, 32);
        return 0;
    } catch (const std::exception &) { return -1; }
}
int vph_fft_gkr_fs(vph_session *s, int lg, const uint8_t state_in[32], uint64_t *msgs_pairs, uint64_t cap_elems, uint64_t *tape_pairs, uint8_t state_out[32],
                   char *err, int errlen) {
    if (!s || !state_in || !msgs_pairs || !tape_pairs || !state_out) { set_err(err, errlen, "vph_fft_gkr_fs: a null argument"); return -1; }
    if (lg < 1 || lg > 19) { set_err(err, errlen, "vph_fft_gkr_fs: lg out of range (1..19)"); return -1; }
    const vph::FftGkrLayout L(lg);
    if (cap_elems < L.n_msgs) { set_err(err, errlen, "vph_fft_gkr_fs: message buffer size"); return -1; }
    try {
        uint8_t st[32];
        memcpy(st, state_in, 32);
        std::vector<F> tape;
        const std::vector<F> msgs = s->p->fftGkrFS(lg, st, tape);
        memcpy(msgs_pairs, msgs.data(), msgs.size() * sizeof(F));
        memcpy(tape_pairs, tape.data(), tape.size() * sizeof(F));
        memcpy(state_out, st, 32);
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}
int vph_fft_gkr_check(int lg, const uint64_t *tape_pairs, uint64_t n_tape, const uint64_t *msgs_pairs, uint64_t n_msgs) {
    if (lg < 1 || lg > 19) return -1;
    const vph::FftGkrLayout L(lg);
    if (!fgk_pairs_ok(lg, tape_pairs, n_tape, L.n_tape) || !fgk_pairs_ok(lg, msgs_pairs, n_msgs, L.n_msgs)) return -1;
    try {
        std::vector<F> msgs(L.n_msgs), tape(L.n_tape);
        memcpy(static_cast<void *>(msgs.data()), msgs_pairs, L.n_msgs * sizeof(F));
        memcpy(static_cast<void *>(tape.data()), tape_pairs, L.n_tape * sizeof(F));
        return vph::fft_gkr_check<F>(lg, tape.data(), tape.size(), msgs.data(), msgs.size(), F::getRootOfUnity(lg).inv()) ? 0 : 1;
    } catch (const std::exception &) { return -1; }
}

// fft_gkr of the last vph_prove_and_verify_full: its messages ({real,img} pairs, layout of vp_fft_gkr); returns their number or -1
int64_t vph_last_fft_gkr(vph_session *s, uint64_t *pairs, uint64_t cap_elems) {
    if (!s || s->fft_gkr_msgs.empty() || cap_elems < s->fft_gkr_msgs.size()) return -1;
    memcpy(pairs, s->fft_gkr_msgs.data(), s->fft_gkr_msgs.size() * sizeof(F));
    return (int64_t) s->fft_gkr_msgs.size();
}
// seconds of the last vph_prove_and_verify_full: [0] "Polynomial commitment: prove time" by the reference's definition (commit_private +
// commit_public + fft_gkr + FRI commit phase), [1] its fft_gkr share, [2] answering the verifier's queries (outside [0], as in the reference)
void vph_last_pc_times(vph_session *s, double out[3]) { for (int i = 0; i < 3; ++i) out[i] = s ? s->pc_times[i] : 0; }

// FRI data of the last vph_prove_and_verify_full on this session: roots (32 bytes per step), final codeword (2048 elements),
// challenges (16 bytes per step); returns the number of fold steps or -1.
int vph_last_fri(vph_session *s, uint8_t *roots, uint64_t roots_cap, uint64_t *final_pairs, uint64_t *r_pairs) {
    if (!s || s->fri_roots.empty()) return -1;
    const int steps = (int) (s->fri_roots.size() / 32);
    if (roots) { if (roots_cap < s->fri_roots.size()) return -1; memcpy(roots, s->fri_roots.data(), s->fri_roots.size()); }
    if (final_pairs) memcpy(final_pairs, s->fri_final.data(), s->fri_final.size() * sizeof(F));
    if (r_pairs) memcpy(r_pairs, s->fri_r.data(), s->fri_r.size() * sizeof(F));
    return steps;
}

// The point the input layer is opened at (r_liu after the last Liu sumcheck) in the last vph_prove_full / vph_prove_and_verify_full:
// the protocol's public vector is its eq table (src/verifier.cpp:368-369).  Returns the number of coordinates or -1.
int vph_last_point(vph_session *s, uint64_t *pairs, int cap) {
    if (!s || s->last_point.empty() || cap < (int) s->last_point.size()) return -1;
    memcpy(pairs, s->last_point.data(), s->last_point.size() * sizeof(F));
    return (int) s->last_point.size();
}

void vph_test_sha3(const uint8_t *in, uint8_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t m[8];
        memcpy(m, in + 64 * i, 64);
        vph::hhash_digest prev; memcpy(prev.w, m + 4, 32);
        vph::hhash_digest d = vph::hhash(m, prev);
        memcpy(out + 32 * i, d.w, 32);
    }
}

// the two FRI commit calls on a session whose commitment is sharded: through the prover, which runs every rank
static int fri_commit_sharded(vph_session *s, const uint64_t *r_pairs, int n_steps, uint8_t *roots, uint64_t *final_pairs, bool batched, char *err, int errlen) {
    try {
        std::vector<F> r((size_t) n_steps);
        for (int k = 0; k < n_steps; ++k) { r[k].real = r_pairs[2 * k]; r[k].img = r_pairs[2 * k + 1]; }
        if (batched) { const auto d = s->p->friCommit(r); memcpy(roots, d.data(), 32 * d.size()); }
        else for (int k = 0; k < n_steps; ++k) { const auto d = s->p->friStep(r[k]); memcpy(roots + 32 * k, d.b, 32); }
        const std::vector<F> fin = s->p->friFinal();
        memcpy(final_pairs, fin.data(), fin.size() * sizeof(F));
        return 0;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

int vph_fri_commit(vph_session *s, const uint64_t *r_pairs, int n_steps, uint8_t *roots, uint64_t *final_pairs, char *err, int errlen) {
    if (s->p->commitmentSharded()) return fri_commit_sharded(s, r_pairs, n_steps, roots, final_pairs, false, err, errlen);
    vp_ctx *ctx = s->p->context();
    for (int k = 0; k < n_steps; ++k) {
        vp_F r; r.real = r_pairs[2 * k]; r.img = r_pairs[2 * k + 1];
        int rc = vp_fri_step(ctx, &r, roots + 32 * k);
        if (rc != VP_OK) { set_err(err, errlen, std::string("vp_fri_step: ") + vp_last_error(ctx)); return rc; }
    }
    int rc = vp_fri_final(ctx, reinterpret_cast<vp_F *>(final_pairs));
    if (rc != VP_OK) { set_err(err, errlen, std::string("vp_fri_final: ") + vp_last_error(ctx)); return rc; }
    return 0;
}

int vph_fri_commit_batched(vph_session *s, const uint64_t *r_pairs, int n_steps, uint8_t *roots, uint64_t *final_pairs, char *err, int errlen) {
    if (s->p->commitmentSharded()) return fri_commit_sharded(s, r_pairs, n_steps, roots, final_pairs, true, err, errlen);
    vp_ctx *ctx = s->p->context();
    int rc = vp_fri_commit(ctx, reinterpret_cast<const vp_F *>(r_pairs), n_steps, roots);
    if (rc != VP_OK) { set_err(err, errlen, std::string("vp_fri_commit: ") + vp_last_error(ctx)); return rc; }
    rc = vp_fri_final(ctx, reinterpret_cast<vp_F *>(final_pairs));
    if (rc != VP_OK) { set_err(err, errlen, std::string("vp_fri_final: ") + vp_last_error(ctx)); return rc; }
    return 0;
}

int vph_prove_full(vph_session *s, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, int batched, char *err, int errlen) {
    try {
        F::init();
        std::vector<uint8_t> out;
        prover::hhash_digest rl = s->p->commit_private();                      // verifier.cpp:137
        out.insert(out.end(), rl.b, rl.b + 32);
        verifier v(batched ? nullptr : s->p.get(), s->circ->c);
        bool ok;
        if (batched) {
            std::vector<F> tape = v.drawTape();
            std::vector<uint8_t> tr;
            s->p->proveGKR(tape, tr);
            v.pred_dev = s->p.get();                 // the verifier's O(|C|) loops on the device (the prover is idle during the replay)
            ok = v.check(tape, tr);
        } else {
            ok = v.verify();
        }
        out.insert(out.end(), v.transcript().begin(), v.transcript().end());
        // verifyPoly (verifier.cpp:363-379): the public vector is eq(r_liu, .) over the input layer
        s->last_point.assign(v.finalPoint().begin(), v.finalPoint().begin() + s->circ->c.circuit[0].bitLength);
        std::vector<F> pub;
        initBetaTable(pub, s->circ->c.circuit[0].bitLength, v.finalPoint().begin(), F_ONE);
        pub.resize(1ull << s->circ->c.circuit[0].bitLength);
        F inner; std::vector<F> all_sum;
        prover::hhash_digest rh = s->p->commit_public(pub, inner, all_sum);
        out.insert(out.end(), rh.b, rh.b + 32);
        const uint8_t *ib = reinterpret_cast<const uint8_t *>(&inner);
        out.insert(out.end(), ib, ib + 16);
        const uint8_t *ab = reinterpret_cast<const uint8_t *>(all_sum.data());
        out.insert(out.end(), ab, ab + 65 * 16);
        if (out.size() > capacity) { set_err(err, errlen, "transcript buffer too small"); return -1; }
        memcpy(transcript, out.data(), out.size());
        if (n_written) *n_written = out.size();
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return -2;
    }
}

// ---- the prover side of the COMPLETE protocol as one pass (the bench's configs[2] step) -----------------------------------------------
// The reference verifier's draws do not depend on the prover's messages (glibc random(), lib/virgo/src/fieldElement.cpp:119-124), so the
// whole tape of verifier::verify() can be drawn first, in its order: F::init(), the GKR draws (src/verifier.cpp:144-279), fft_gkr's
// (lib/virgo/src/fft_circuit_GKR.cpp, count verifier::fftGkrDraws), the FRI fold challenges (vpd_verifier.cpp:57).
int vph_draw_protocol_tape(vph_session *s) {
    const int n = s->circ->c.circuit[0].bitLength;
    if (n < 7) return -1;
    F::init();
    verifier v(nullptr, s->circ->c);
    s->tape = v.drawTape();
    const int ln = n - 6;
    s->ptape_fft.resize((size_t) verifier::fftGkrDraws(ln));
    for (auto &x : s->ptape_fft) x = F::random();
    s->ptape_fri.resize(ln);
    for (auto &x : s->ptape_fri) x = F::random();
    return 0;
}
// commit_private -> GKR (one batched device pass) -> commit_public on eq(r_liu, .) built on the device -> fft_gkr -> FRI commit phase +
// final codeword: every prover call of verifier::verify() except answering the queries, nothing of the verifier.  transcript = the golden
// layout (merkle_root_l | GKR | merkle_root_h | input_0 | all_sum[65]); fri_roots: 32 bytes per fold step; final_pairs: 2048 elements.
// flags (vphost.h): VPH_PASS_DEFERRED — the calls are queued back to back without a host wait between them (vp_set_deferred) and collected at the end;
// VPH_PASS_QUEUE_NEXT — before it waits, the pass queues the HEAD of the next one (commit_private of the same witness) behind its own folds, so
// that the device goes from this proof's last kernel straight into the next proof's first (the next pass finds it and starts at the GKR part).
// The pass hashes once (vphost.h): sec[1] and sec[3] are the transforms of the two commits, sec[5] holds the leaf chains and trees of l, h and the FRI levels.
// sec[6] = whole pass (host wall clock) | commit_private | GKR | commit_public | fft_gkr (host time of its begin + end) | FRI commit phase + final;
// synchronous: host wall clock of each call, deferred: device time of each call (vp_phase_ms).  The fft_gkr messages stay with the session
// (vph_last_fft_gkr), the FRI data too (vph_last_fri).  0 = done, < 0 = error.
// pri_mask / pub_mask: the mask vectors of a hiding commitment (vph_prove_protocol_masked; null or all zero: the reference's own pass, one zero element)
static int prove_protocol_pass(vph_session *s, const uint64_t *pri_mask, uint64_t n_pri, const uint64_t *pub_mask, uint64_t n_pub, uint8_t *transcript, uint64_t capacity,
                               uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap, uint64_t *final_pairs, uint64_t *final_mask_pairs, double sec[6], int flags,
                               char *err, int errlen) {
    if (s->p->commitmentSharded()) { set_err(err, errlen, "vph_prove_protocol: not on a session with a sharded commitment (vph_prove_and_verify_full runs it)"); return -1; }
    vp_ctx *ctx = s->p->context();
    const bool defer = (flags & VPH_PASS_DEFERRED) != 0, queue_next = defer && (flags & VPH_PASS_QUEUE_NEXT) != 0;
    bool with_mask = false;
    for (uint64_t i = 0; pri_mask && i < 2 * n_pri; ++i) with_mask = with_mask || pri_mask[i] != 0;
    // the queued head of the next pass is a vp_commit_private of the same witness: it would have to carry this pass's mask, which the caller owns
    if (with_mask && (flags & VPH_PASS_QUEUE_NEXT)) { set_err(err, errlen, "vph_prove_protocol_masked: VPH_PASS_QUEUE_NEXT is not available with a mask (the queued head is an unmasked commit_private)"); return -1; }
    // a run of fft_gkr that is begun and not collected when this function leaves, for whatever reason, is dropped (it would make every later pass of the
    // session fail with "not collected")
    struct FftGuard { prover *p; bool armed; ~FftGuard() { if (armed) p->fftGkrCancel(); } } fft_guard{s->p.get(), false};
    auto chk = [&](int rc, const char *what) { if (rc != VP_OK) throw std::runtime_error(std::string(what) + ": " + vp_last_error(ctx)); };
    try {
        const layeredCircuit &C = s->circ->c;
        const int n = C.circuit[0].bitLength, ln = n - 6;
        if (s->tape.empty() || (int) s->ptape_fri.size() != ln) { set_err(err, errlen, "vph_draw_protocol_tape first"); return -1; }
        int max_bl = 0;
        for (auto &l : C.circuit) max_bl = std::max(max_bl, l.bitLength);
        using clk = std::chrono::high_resolution_clock;
        auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
        const auto t0 = clk::now();
        static const bool fft_sync = getenv("VPH_FFT_GKR_SYNC") != nullptr;
        static const bool hash_per_call_env = getenv("VPH_HASH_PER_CALL") != nullptr;
        const bool hash_once = !hash_per_call_env && !(flags & VPH_PASS_HASH_PER_CALL);
        u64 nt = 0, nb = 0;
        s->p->gkrSizes(nt, nb);
        if (s->tape.size() != nt) throw std::runtime_error("the tape has the wrong length");
        s->pp_gkr.resize(nb); s->pp_all.resize(65); s->pp_roots.resize((size_t) 32 * ln); s->pp_final.resize(2048);
        chk(vp_set_deferred(ctx, defer ? 1 : 0), "vp_set_deferred");
        // the pass hashes once: commit_private and commit_public_eq stop behind their transforms, vp_fri_commit hashes l, h and its levels in one launch and
        // writes pp_root_l / pp_root_h with its own roots (VPH_PASS_HASH_PER_CALL / VPH_HASH_PER_CALL: every call hashes its own oracle, as before)
        chk(vp_pc_hash_late(ctx, hash_once ? (with_mask ? VP_HASH_LATE_MASKED : 1) : 0), "vp_pc_hash_late");
        // ---- head: fft_gkr (depends on the verifier's draws only: queued on its own stream, its small launches run in the gaps of everything below;
        // VPH_FFT_GKR_SYNC=1: in the reference's place, between commit_public and the FRI folds) and commit_private (src/verifier.cpp:137) —
        // unless the previous pass queued them for this one and that commitment still stands
        uint64_t epoch = 0; int valid = 0;
        chk(vp_commit_private_state(ctx, &epoch, &valid), "vp_commit_private_state");
        const bool have_head = !with_mask && s->head_queued && valid && epoch == s->head_epoch;     // (a masked pass commits anew: the queued head carries no mask)
        s->head_queued = false;
        auto t = clk::now();
        double s_fft = 0, s_priv = 0, s_gkr = 0, s_pub = 0, s_fri = 0;
        if (with_mask) {
            // the 65th slice with content (the call reads the mask and completes at once, whatever the mode; under hash_once its leaf chains wait for vp_fri_commit)
            chk(vp_commit_private_masked(ctx, reinterpret_cast<const vp_F *>(pri_mask), n_pri, s->pp_root_l), "vp_commit_private_masked");
            s->p->setMasked(true);
            s_priv = since(t);
        } else if (!have_head) {
            chk(vp_commit_private(ctx, s->pp_root_l), "vp_commit_private");
            s->p->setMasked(false);
            s_priv = since(t);
        }
        // ---- GKR (src/verifier.cpp:144-169)
        t = clk::now();
        chk(vp_prove_gkr(ctx, reinterpret_cast<const vp_F *>(s->tape.data()), nt, s->pp_gkr.data(), nb, &s->pp_written), "vp_prove_gkr");
        s_gkr = since(t);
        // ---- fft_gkr (vpd_verifier.cpp:92) depends on the verifier's draws only.  It is queued on a stream of its own BEHIND the proof (vp_fft_gkr_begin starts
        // behind what the context has queued so far) and collected last: its ~100 few-workgroup launches then run beside commit_public's transforms, which do not
        // notice them.  Beside a leaf-hash launch they cost that launch a ninth round of workgroups (11.4 instead of 10.2 ms), beside the proof's graph 0.9 ms
        // of its critical path (measured, tools/pass_modes.py / tools/leaf_in_step.py).  VPH_FFT_GKR_SYNC=1: in the reference's place, on the main stream
        t = clk::now();
        if (!fft_sync) { s->p->fftGkrBegin(ln, s->ptape_fft); fft_guard.armed = true; }
        s_fft = since(t);
        // r_liu after the last Liu sumcheck = the last max_bl draws of the GKR tape (verifier::drawTape), its first n coordinates
        s->last_point.assign(s->tape.end() - max_bl, s->tape.end() - max_bl + n);
        // ---- commit_public on eq(r_liu, .) (:368-379)
        t = clk::now();
        if (with_mask) {
            static const uint64_t one_zero[2] = {0, 0};
            const bool have_pub = pub_mask && n_pub;
            chk(vp_commit_public_eq_masked(ctx, reinterpret_cast<const vp_F *>(s->last_point.data()), n, reinterpret_cast<const vp_F *>(have_pub ? pub_mask : one_zero), have_pub ? n_pub : 1,
                                           reinterpret_cast<vp_F *>(&s->pp_inner), reinterpret_cast<vp_F *>(s->pp_all.data()), s->pp_root_h), "vp_commit_public_eq_masked");
        } else
        chk(vp_commit_public_eq(ctx, reinterpret_cast<const vp_F *>(s->last_point.data()), n, reinterpret_cast<vp_F *>(&s->pp_inner),
                                reinterpret_cast<vp_F *>(s->pp_all.data()), s->pp_root_h), "vp_commit_public_eq");
        s_pub = since(t);
        if (fft_sync) { t = clk::now(); s->fft_gkr_msgs = s->p->fftGkr(ln, s->ptape_fft); s_fft = since(t); }
        // ---- FRI commit phase (vpd_verifier.cpp:44-74) + final codeword
        t = clk::now();
        chk(vp_fri_commit(ctx, reinterpret_cast<const vp_F *>(s->ptape_fri.data()), ln, s->pp_roots.data()), "vp_fri_commit");
        chk(vp_fri_final(ctx, reinterpret_cast<vp_F *>(s->pp_final.data())), "vp_fri_final");
        s_fri = since(t);
        chk(vp_pc_hash_late(ctx, 0), "vp_pc_hash_late");      // the mode belongs to this pass's own calls: the next pass's head below is a complete commit_private
        int n_mine = 0;
        chk(vp_pending(ctx, &n_mine), "vp_pending");
        if (queue_next) {
            // the next pass's commit_private, behind this pass's folds in stream order; this pass's results are collected below while the device runs it
            chk(vp_commit_private(ctx, s->pp_root_next), "vp_commit_private (next pass)");
            uint64_t e2 = 0; int v2 = 0;
            chk(vp_commit_private_state(ctx, &e2, &v2), "vp_commit_private_state");
            s->head_queued = true; s->head_epoch = e2;
        }
        if (defer) {
            chk(vp_flush(ctx, n_mine), "vp_flush");
            double ms[5] = {0, 0, 0, 0, 0};
            chk(vp_phase_ms(ctx, ms), "vp_phase_ms");
            s_priv = ms[0] * 1e-3; s_gkr = ms[1] * 1e-3; s_pub = ms[2] * 1e-3; s_fri = (ms[3] + ms[4]) * 1e-3;
        }
        chk(vp_set_deferred(ctx, 0), "vp_set_deferred");      // the mode belongs to this pass: whatever the session calls next waits for its results as usual
        if (final_mask_pairs) {                               // the mask slice's last codeword: zeros without a mask (and a queued head has replaced the commitment by now)
            if (with_mask) chk(vp_fri_final_mask(ctx, reinterpret_cast<vp_F *>(final_mask_pairs)), "vp_fri_final_mask");
            else memset(final_mask_pairs, 0, 32 * sizeof(F));
        }
        // fft_gkr is collected last: its launches had the whole pass to run beside the main stream's
        if (!fft_sync) { t = clk::now(); fft_guard.armed = false; s->fft_gkr_msgs = s->p->fftGkrEnd(ln); s_fft += since(t); }
        const uint64_t total = 32 + s->pp_written + 32 + 16 + 65 * 16;
        if (total > capacity || (fri_roots && roots_cap < s->pp_roots.size())) { set_err(err, errlen, "output buffer too small"); return -1; }
        uint8_t *o = transcript;
        memcpy(o, have_head ? s->pp_root_next : s->pp_root_l, 32); o += 32;      // (a head queued by the previous pass left its root in pp_root_next)
        memcpy(o, s->pp_gkr.data(), s->pp_written); o += s->pp_written;
        memcpy(o, s->pp_root_h, 32); o += 32;
        memcpy(o, &s->pp_inner, 16); o += 16;
        memcpy(o, s->pp_all.data(), 65 * 16);
        if (n_written) *n_written = total;
        s->fri_roots = s->pp_roots;
        s->fri_final = s->pp_final;
        s->fri_r = s->ptape_fri;
        if (fri_roots) memcpy(fri_roots, s->fri_roots.data(), s->fri_roots.size());
        if (final_pairs) memcpy(final_pairs, s->fri_final.data(), s->fri_final.size() * sizeof(F));
        s->p->addProveTime(s_gkr);
        if (sec) { sec[0] = since(t0); sec[1] = s_priv; sec[2] = s_gkr; sec[3] = s_pub; sec[4] = s_fft; sec[5] = s_fri; }
        return 0;
    } catch (const std::exception &e) {
        (void) vp_pc_hash_late(ctx, 0);                  // (first: the flush then also hashes what the failed pass left unhashed)
        (void) vp_flush(ctx, -1);                        // nothing of a failed pass stays queued
        (void) vp_set_deferred(ctx, 0);
        s->head_queued = false;
        set_err(err, errlen, e.what());
        return -2;
    }
}
int vph_prove_protocol_ex(vph_session *s, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap,
                          uint64_t *final_pairs, double sec[6], int flags, char *err, int errlen) {
    return prove_protocol_pass(s, nullptr, 0, nullptr, 0, transcript, capacity, n_written, fri_roots, roots_cap, final_pairs, nullptr, sec, flags, err, errlen);
}
int vph_prove_protocol_masked(vph_session *s, const uint64_t *pri_mask_pairs, uint64_t n_pri, const uint64_t *pub_mask_pairs, uint64_t n_pub, uint8_t *transcript, uint64_t capacity,
                              uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap, uint64_t *final_pairs, uint64_t *final_mask_pairs, double sec[6], int flags,
                              char *err, int errlen) {
    return prove_protocol_pass(s, pri_mask_pairs, n_pri, pub_mask_pairs, n_pub, transcript, capacity, n_written, fri_roots, roots_cap, final_pairs, final_mask_pairs, sec, flags, err, errlen);
}
int vph_prove_protocol(vph_session *s, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap,
                       uint64_t *final_pairs, double sec[6], char *err, int errlen) {
    return vph_prove_protocol_ex(s, transcript, capacity, n_written, fri_roots, roots_cap, final_pairs, sec, 0, err, errlen);
}

int vph_verify_transcript(vph_circuit *c, const uint8_t *transcript, uint64_t n, int skip_predicates) {
    try {
        F::init();
        verifier v(nullptr, c->c);
        const std::vector<F> tape = v.drawTape();
        v.skip_predicates = skip_predicates != 0;
        std::vector<uint8_t> tr(transcript, transcript + n);
        return v.check(tape, tr) ? 0 : 1;
    } catch (const std::exception &) { return 1; }
}

int vph_verify_transcript_tape(vph_circuit *c, const uint64_t *tape_pairs, uint64_t n_tape, const uint8_t *transcript, uint64_t n, int skip_predicates) {
    try {
        std::vector<F> tape;
        if (!c || !tape_fits(c->c, tape_pairs, n_tape, tape)) return -1;
        verifier v(nullptr, c->c);
        v.skip_predicates = skip_predicates != 0;
        std::vector<uint8_t> tr(transcript, transcript + n);
        return v.check(tape, tr) ? 0 : 1;
    } catch (const std::exception &) { return 1; }
}

int vph_last_gkr_failure(int *layer, int *round) {
    const GkrFailure f = lastGkrFailure();
    if (layer) *layer = f.layer;
    if (round) *round = f.round;
    return f.kind;
}

uint64_t vph_transcript_bytes(vph_session *s) {
    u64 a = 0, b = 0;
    s->p->gkrSizes(a, b);
    return b;
}

}  // extern "C"
