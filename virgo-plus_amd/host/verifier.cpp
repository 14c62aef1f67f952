#include "verifier.hpp"
#include "fft_gkr_verify.hpp"
#include "fft_gkr_fs.hpp"
#include "gkr_fs.hpp"
#include "pc_fs.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

void initBetaTable(std::vector<F> &beta, int n, const std::vector<F>::const_iterator &r, const F &init) {
    if (n < 0) return;
    if (beta.size() < (1ull << n)) beta.resize(1ull << n);
    // direct doubling: after step k the first 2^k entries hold init * eq(r[0..k), .)
    beta[0] = init;
    for (int k = 0; k < n; ++k) {
        const u64 half = 1ull << k;
        for (u64 j = 0; j < half; ++j) {
            const F t = beta[j] * r[k];
            beta[j | half] = t;
            beta[j] = beta[j] - t;
        }
    }
}

namespace {
thread_local GkrFailure gkr_failure;
bool gkrFails(int kind, int layer, int round) { gkr_failure.kind = kind; gkr_failure.layer = layer; gkr_failure.round = round; return false; }
}  // namespace
GkrFailure lastGkrFailure() { return gkr_failure; }
const char *gkrCheckName(int kind) {
    static const char *const names[] = {"none", "phase1", "phase2", "semi_final", "liu", "liu_semi_final", "input"};
    return kind >= 0 && kind <= GKR_INPUT ? names[kind] : "?";
}

verifier::verifier(prover *pr, const layeredCircuit &cir) : p(pr), C(cir) {       // verifier.cpp:12-48
    final_claims_v.resize(C.size);
    for (int i = 1; i < C.size; ++i) final_claims_v[i].assign(i, F_ZERO);
    for (auto &v : coeff_r) v.assign(C.size, F_ZERO);
    r_v.resize(C.size + 2);
    if (p) p->init();
    int max_dad_bl = 0;
    for (auto &l : C.circuit) { max_bl = std::max(max_bl, l.bitLength); max_dad_bl = std::max(max_dad_bl, l.maxDadBitLength); }
    beta_g.resize(1ull << std::max(max_bl, max_dad_bl));
    beta_u.resize(1ull << max_bl);
    beta_v.resize(1ull << max_bl);
    r_u.assign(max_bl, F_ZERO);
    r_liu.assign(max_bl, F_ZERO);
    for (int i = 1; i < C.size; ++i)
        if (C.circuit[i].maxDadBitLength != -1) r_v[i].assign(C.circuit[i].maxDadBitLength, F_ZERO);
    sig.assign(C.size, F_ZERO);
}

// ---- Fiat-Shamir: state' = SHA3-256(block || state) over the same 64-byte block function as the commitment (sha3.hpp) ----
// absorb a prover message:  block = {real, img, 0, 0x4d};  squeeze challenge number c:  block = {c, 0, 0, 0x43}, then the two
// limbs are the first two digest words reduced to 61 bits (p itself maps to 0; the bias is 2^-61).
void verifier::fsInit(bool with_inputs) {
    fs_state = vph::fs_chain{};
    fs_ctr = 0;
    // statement: SHA3-256 over the serialised levelised circuit, subset tables and input values (layeredCircuit::statementDigest);
    // the non-cryptographic structuralHash is a test fingerprint only and is not used here
    u64 h[4];
    C.statementDigest(h, with_inputs);
    fs_state.step(h[0], h[1], h[2], h[3]);
    fs_state.step((uint64_t) C.size, 0, 0, 0x53);
}
F verifier::draw() {
    if (fs) {
        uint64_t a, b;
        fs_state.challenge(fs_ctr++, a, b);
        F x; x.real = a; x.img = b;
        tape_.push_back(x);
        return x;
    }
    if (replay) return (*rtape)[tape_pos++];
    F x = F::random();
    tape_.push_back(x);
    return x;
}
void verifier::putF(const F &x) {
    unsigned long long w[2] = {x.real, x.img};
    const uint8_t *b = reinterpret_cast<const uint8_t *>(w);
    tr.insert(tr.end(), b, b + 16);
    if (fs) {
        fs_state.elem(x.real, x.img);
    }
}
F verifier::nextF() {
    F x;
    if (tr_pos + 16 > rtr->size()) throw std::runtime_error("transcript too short");
    unsigned long long w[2];
    memcpy(w, rtr->data() + tr_pos, 16);
    tr_pos += 16;
    // a proof element must be the canonical representative: the host arithmetic (single conditional subtract, 125-bit reduce)
    // is only F_p^2 arithmetic on limbs < p, and every limb would otherwise have up to 8 accepted encodings
    if (w[0] >= F::mod || w[1] >= F::mod) throw std::runtime_error("non-canonical field element in the proof");
    x.real = w[0]; x.img = w[1];
    return x;
}
quadratic_poly verifier::nextPoly(int phase, const F &prev) {
    quadratic_poly q;
    if (replay) { q.a = nextF(); q.b = nextF(); q.c = nextF(); }
    else q = phase == 1 ? p->sumcheckUpdatePhase1(prev) : phase == 2 ? p->sumcheckUpdatePhase2(prev) : p->sumcheckLiuUpdate(prev);
    putF(q.a); putF(q.b); putF(q.c);
    return q;
}

std::vector<F> verifier::drawTape() {           // same draws as run(), without a prover
    std::vector<F> t;
    auto take = [&](size_t n) { for (size_t i = 0; i < n; ++i) t.push_back(F::random()); };
    take(C.circuit[C.size - 1].bitLength);                       // verifier.cpp:144
    for (int i = C.size - 1; i; --i) {
        take(max_bl);                                            // r_u            :196
        take(1);                                                 // assert_random  :202
        if (C.circuit[i].maxDadBitLength != -1) take(C.circuit[i].maxDadBitLength);   // r_v[i] :236
        take(C.size);                                            // sig            :278
        take(max_bl);                                            // r_liu          :279
    }
    return t;
}

bool verifier::verify() {
    if (!p) throw std::runtime_error("verify(): no prover attached");
    replay = false; tape_.clear(); tr.clear();
    return run();
}
bool verifier::proveFS() {
    if (!p) throw std::runtime_error("proveFS(): no prover attached");
    replay = false; fs = true; tape_.clear(); tr.clear();
    fsInit();
    const bool ok = run();
    fs = false;
    return ok;
}
u64 verifier::proveFSDevice() {
    if (!p) throw std::runtime_error("proveFSDevice(): no prover attached");
    replay = false; fs = false; tape_.clear(); tr.clear();
    fsInit();
    uint8_t st[32];
    memcpy(st, fs_state.s.w, 32);
    u64 draws = 0;
    tr = p->proveGkrFS(st, tape_, draws);
    memcpy(fs_state.s.w, st, 32);
    fs_ctr = draws;
    return draws;
}
bool verifier::checkFS(const std::vector<uint8_t> &proof) {
    static const std::vector<F> no_tape;
    replay = true; fs = true; rtape = &no_tape; rtr = &proof; tape_pos = 0; tr_pos = 0; tr.clear(); tape_.clear();
    fsInit();
    bool ok = false;
    try { ok = run(); } catch (const std::exception &) { ok = false; }      // truncated proof
    fs = false;
    return ok && tr_pos == proof.size();
}
bool verifier::check(const std::vector<F> &tape, const std::vector<uint8_t> &transcript) {
    replay = true; rtape = &tape; rtr = &transcript; tape_pos = 0; tr_pos = 0; tr.clear();
    bool ok = false;
    try { ok = run(); } catch (const std::runtime_error &) { ok = false; }      // truncated transcript / non-canonical element
    return ok && tr_pos == transcript.size() && tape_pos == tape.size();
}

bool verifier::run() {                          // verifier.cpp:134-169 (GKR part)
    // a verification starts here: the launch log of the device its loops run on (prover::verifierLaunches) starts with it
    gkr_failure = GkrFailure{};
    if (pred_dev) pred_dev->clearLaunchLog();
    if (poly_dev && poly_dev != pred_dev) poly_dev->clearLaunchLog();
    for (int i = 0; i < C.circuit[C.size - 1].bitLength; ++i) r_liu[i] = draw();
    F previousSum;
    if (replay) previousSum = nextF();
    else {
        previousSum = p->Vres(r_liu.begin(), C.circuit[C.size - 1].bitLength);
        p->sumcheckInitAll(r_liu.begin());
    }
    putF(previousSum);
    for (int i = C.size - 1; i; --i) {
        if (!replay) p->sumcheckInit();
        if (!verifyPhase1(i, previousSum)) return false;
        if (C.circuit[i].maxDadBitLength != -1 && !verifyPhase2(i, previousSum)) return false;
        if (!(replay && skip_predicates)) {
            verify_timer.start();
            const F test_value = getFinalValue(i, final_claim_u, final_claims_v[i]);
            verify_timer.stop();
            if (previousSum != test_value) {
                fprintf(stderr, "Verification fail, semi final, circuit level %d\n", i);
                return gkrFails(GKR_SEMI_FINAL, i, -1);
            }
        }
        if (!verifyLiu(i, previousSum)) return false;
    }
    last_claim = previousSum;
    if (input_check_by_commitment) return true;      // verifyPoly checks the claim against the committed input instead
    return checkInput(previousSum);
}

bool verifier::verifyPhase1(int layer_id, F &previousSum) {      // verifier.cpp:191-229
    const layer &pre = C.circuit[layer_id - 1];
    if (!fs) for (auto &x : r_u) x = draw();
    F previousRandom = F_ZERO;
    assert_random = draw();
    if (!replay) p->sumcheckInitPhase1(assert_random);
    for (int j = 0; j < pre.bitLength; ++j) {
        const quadratic_poly poly = nextPoly(1, previousRandom);
        if (poly.eval(F_ZERO) + poly.eval(F_ONE) != previousSum) {
            fprintf(stderr, "Verification fail, phase1, circuit %d, current bit %d\n", layer_id, j);
            return gkrFails(GKR_PHASE1, layer_id, j);
        }
        if (fs) r_u[j] = draw();                    // Fiat-Shamir: the challenge of round j follows its polynomial
        previousRandom = r_u[j];
        previousSum = poly.eval(r_u[j]);
    }
    if (replay) final_claim_u = nextF(); else p->sumcheckFinalize1(previousRandom, final_claim_u);
    putF(final_claim_u);
    if (!(replay && skip_predicates)) { verify_timer.start(); predicatePhase1(layer_id); verify_timer.stop(); }
    return true;
}

bool verifier::verifyPhase2(int layer_id, F &previousSum) {      // verifier.cpp:231-270
    if (!fs) for (auto &x : r_v[layer_id]) x = draw();
    F previousRandom = F_ZERO;
    if (!replay) p->sumcheckInitPhase2();
    for (int j = 0; j < C.circuit[layer_id].maxDadBitLength; ++j) {
        const quadratic_poly poly = nextPoly(2, previousRandom);
        if (poly.eval(F_ZERO) + poly.eval(F_ONE) != previousSum) {
            fprintf(stderr, "Verification fail, phase2, circuit level %d, current bit %d\n", layer_id, j);
            return gkrFails(GKR_PHASE2, layer_id, j);
        }
        if (fs) r_v[layer_id][j] = draw();
        previousRandom = r_v[layer_id][j];
        previousSum = poly.eval(previousRandom);
    }
    if (replay) for (int j = 0; j < layer_id; ++j) final_claims_v[layer_id][j] = nextF();
    else p->sumcheckFinalize2(previousRandom, final_claims_v[layer_id].begin());
    for (int j = 0; j < layer_id; ++j) putF(final_claims_v[layer_id][j]);
    if (!(replay && skip_predicates)) { verify_timer.start(); predicatePhase2(layer_id); verify_timer.stop(); }
    return true;
}

bool verifier::verifyLiu(int layer_id, F &previousSum) {         // verifier.cpp:272-337
    const int pre_layer_id = layer_id - 1;
    const layer &pre = C.circuit[pre_layer_id];
    for (auto &x : sig) x = draw();
    if (!fs) for (auto &x : r_liu) x = draw();
    previousSum = sig[0] * final_claim_u;
    for (int j = layer_id; j < C.size; ++j)
        if (C.circuit[j].dadSize[pre_layer_id])                  // an empty subset's claim is zero
            previousSum += sig[j - pre_layer_id] * final_claims_v[j][pre_layer_id];
    if (!replay) p->sumcheckInitLiu(sig.begin());
    F previousRandom = F_ZERO;
    for (int j = 0; j < pre.bitLength; ++j) {
        const quadratic_poly poly = nextPoly(3, previousRandom);
        if (poly.eval(F_ZERO) + poly.eval(F_ONE) != previousSum) {
            fprintf(stderr, "Liu fail, circuit %d, current bit %d\n", layer_id, j);
            return gkrFails(GKR_LIU, layer_id, j);
        }
        if (fs) r_liu[j] = draw();
        previousRandom = r_liu[j];
        previousSum = poly.eval(previousRandom);
    }
    F vr;
    if (replay) vr = nextF(); else p->sumcheckLiuFinalize(previousRandom, vr);
    putF(vr);
    verify_timer.start();
    F gr = F_ZERO;
    if (pred_dev) {
        gr = pred_dev->liuGr(layer_id, r_u, r_v, sig, r_liu);          // same sum on the device (vp_liu_gr)
    } else {
    initBetaTable(beta_u, pre.bitLength, r_liu.begin(), F_ONE);
    initBetaTable(beta_g, pre.bitLength, r_u.begin(), sig[0]);
    for (u64 g = 0; g < pre.size; ++g) gr = gr + beta_g[g] * beta_u[g];
    for (int j = layer_id; j < C.size; ++j) {
        const layer &Lj = C.circuit[j];
        if (!Lj.dadSize[pre_layer_id]) continue;
        initBetaTable(beta_g, Lj.dadBitLength[pre_layer_id], r_v[j].begin(), sig[j - pre_layer_id]);
        for (u64 g = 0; g < Lj.dadSize[pre_layer_id]; ++g) gr = gr + beta_g[g] * beta_u[Lj.dadId[pre_layer_id][g]];
    }
    }
    const bool ok = (vr * gr == previousSum);
    verify_timer.stop();
    if (!ok) { fprintf(stderr, "Liu fail, semi final, circuit %d\n", layer_id); return gkrFails(GKR_LIU_SEMI_FINAL, layer_id, -1); }
    previousSum = vr;
    return true;
}

// device version of predicatePhase1 + predicatePhase2: one vp_predicates call per layer
void verifier::predicatesOnDevice(int layer_id, bool with_phase2) {
    const layer &cur = C.circuit[layer_id];
    const int n_v = with_phase2 ? cur.maxDadBitLength : 0;
    std::vector<F> rg(r_liu.begin(), r_liu.begin() + cur.bitLength), ru(r_u.begin(), r_u.begin() + C.circuit[layer_id - 1].bitLength);
    const std::vector<F> out = pred_dev->predicates(layer_id, rg, assert_random, ru, r_v[layer_id], n_v);
    F bv0 = F_ONE;                                   // beta_v[0] = prod (1 - r_v[j]) (verifier.cpp:95-96)
    for (int j = 0; j < n_v; ++j) bv0 = bv0 * (F_ONE - r_v[layer_id][j]);
    coeff_l[Copy] = out[0] * bv0; coeff_l[Not] = out[1] * bv0; coeff_l[Addc] = out[2] * bv0; coeff_l[Mulc] = out[3] * bv0;
    bias = out[4] * bv0;
    static const int order[7] = {(int) Add, (int) Sub, (int) AntiSub, (int) Mul, (int) Naab, (int) AntiNaab, (int) Xor};
    for (int t = 0; t < 7; ++t)
        for (int l = 0; l < layer_id; ++l) coeff_r[order[t]][l] = with_phase2 ? out[5 + (size_t) t * layer_id + l] : F_ZERO;
}

void verifier::predicatePhase1(int layer_id) {                   // verifier.cpp:50-56,63-90
    const layer &cur = C.circuit[layer_id];
    if (pred_dev) { if (cur.maxDadBitLength == -1) predicatesOnDevice(layer_id, false); return; }
    initBetaTable(beta_g, cur.bitLength, r_liu.begin(), F_ONE);
    for (u64 g = 0; g < cur.size; ++g) if (cur.gates[g].is_assert) beta_g[g] *= assert_random;        // verifier.cpp:53-54
    initBetaTable(beta_u, C.circuit[layer_id - 1].bitLength, r_u.begin(), F_ONE);
    for (int t : {(int) Copy, (int) Not, (int) Addc, (int) Mulc}) coeff_l[t] = F_ZERO;
    bias = F_ZERO;
    for (u64 g = 0; g < cur.size; ++g) {
        const gate &G = cur.gates[g];
        switch (G.ty) {
            case Addc:
                bias += beta_g[g] * beta_u[G.u] * G.c;
                coeff_l[G.ty] += beta_g[g] * beta_u[G.u];
                break;
            case Not: case Copy: coeff_l[G.ty] += beta_g[g] * beta_u[G.u]; break;
            case Mulc: coeff_l[G.ty] += beta_g[g] * beta_u[G.u] * G.c; break;
            default: break;
        }
    }
    for (int t : {(int) Add, (int) Sub, (int) AntiSub, (int) Mul, (int) Naab, (int) AntiNaab, (int) Xor})
        std::fill(coeff_r[t].begin(), coeff_r[t].end(), F_ZERO);
}

void verifier::predicatePhase2(int layer_id) {                   // verifier.cpp:58-61,92-113
    const layer &cur = C.circuit[layer_id];
    if (pred_dev) { predicatesOnDevice(layer_id, true); return; }
    initBetaTable(beta_v, cur.maxDadBitLength, r_v[layer_id].begin(), F_ONE);
    for (int t : {(int) Copy, (int) Not, (int) Addc, (int) Mulc}) coeff_l[t] *= beta_v[0];
    bias *= beta_v[0];
    for (u64 g = 0; g < cur.size; ++g) {
        const gate &G = cur.gates[g];
        switch (G.ty) {
            case Add: case Sub: case AntiSub: case Mul: case Naab: case AntiNaab: case Xor:
                coeff_r[G.ty][G.l] += beta_g[g] * beta_u[G.u] * beta_v[G.lv];
                break;
            default: break;
        }
    }
}

F verifier::getFinalValue(int layer_id, const F &cu, const std::vector<F> &cv) {   // verifier.cpp:115-132
    F res = coeff_l[Not] * (F_ONE - cu) + coeff_l[Copy] * cu + coeff_l[Addc] * cu + bias + coeff_l[Mulc] * cu;
    for (int j = 0; j < layer_id; ++j) {
        const F uv = cu * cv[j];
        res = res + coeff_r[Add][j] * (cu + cv[j]) + coeff_r[Sub][j] * (cu - cv[j]) + coeff_r[AntiSub][j] * (cv[j] - cu)
              + coeff_r[Mul][j] * uv + coeff_r[Naab][j] * (cv[j] - uv) + coeff_r[AntiNaab][j] * (cu - uv)
              + coeff_r[Xor][j] * (cu + cv[j] - F(2ll) * uv);
    }
    return res;
}

// With the polynomial commitment off, the last claim is checked directly against the input layer's MLE
// at r_liu (the role of verifyPoly, verifier.cpp:363-389).
bool verifier::checkInput(const F &claim) {
    const layer &L0 = C.circuit[0];
    if (pred_dev) {                                       // the input layer's MLE at r_liu on the device (vp_layer_mle)
        if (pred_dev->layerMle(0, r_liu, L0.bitLength) != claim) { fprintf(stderr, "Verification fail, final input check fail.\n"); return gkrFails(GKR_INPUT, 0, -1); }
        return true;
    }
    std::vector<F> beta;
    initBetaTable(beta, L0.bitLength, r_liu.begin(), F_ONE);
    F acc = F_ZERO;
    for (u64 g = 0; g < L0.size; ++g) acc = acc + beta[g] * F((long long) L0.gates[g].u);
    if (acc != claim) { fprintf(stderr, "Verification fail, final input check fail.\n"); return gkrFails(GKR_INPUT, 0, -1); }
    return true;
}

// ====================================================================================================
// Polynomial-commitment verification (reference: verifier::verifyPoly, src/verifier.cpp:348-389, and
// poly_commit_verifier::verify_poly_commitment, lib/virgo/src/vpd_verifier.cpp:76-328).  Host C++: the verifier is
// not a GPU target; the prover side of every step runs through the C ABI.
// ====================================================================================================
namespace {

void host_fft(std::vector<F> &a, const F &root) {          // in place, natural order, a.size() = 2^k
    const u64 n = a.size();
    for (u64 i = 1, j = 0; i < n; ++i) {
        u64 bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (u64 len = 2; len <= n; len <<= 1) {
        F wl = root;
        for (u64 m = n; m > len; m >>= 1) wl = wl * wl;
        for (u64 i = 0; i < n; i += len) {
            F w = F_ONE;
            for (u64 k = 0; k < len / 2; ++k) {
                const F u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
                w = w * wl;
            }
        }
    }
}
vph::hhash_digest dig(const prover::hhash_digest &d) { vph::hhash_digest r; memcpy(r.w, d.b, 32); return r; }

}  // namespace

struct verifier::RecReader {
    const uint8_t *p; size_t n, at;
    void bytes(void *dst, size_t k) {
        if (k > n - at) throw std::runtime_error("record too short");
        memcpy(dst, p + at, k); at += k;
    }
    F elem() {
        unsigned long long w[2]; bytes(w, 16);
        if (w[0] >= F::mod || w[1] >= F::mod) throw std::runtime_error("non-canonical field element in the record");
        F x; x.real = w[0]; x.img = w[1];
        return x;
    }
};

// ---- the two heavy loops of the commitment verifier (declared in verifier.hpp) ----
std::vector<std::vector<F>> pcPublicCoefsHost(int n, const std::vector<F> &pub) {      // public_array_prepare_generic, verifier.cpp:348-361
    const int ln = n - 6;
    const u64 N = 1ull << ln;
    std::vector<std::vector<F>> q_coef(64, std::vector<F>(N));
    const F inv_root = F::getRootOfUnity(ln).inv();
    const F inv_n = F::fastPow(F((long long) N), (unsigned __int128) F::mod - 2);
    for (int j = 0; j < 64; ++j) {
        std::vector<F> a(pub.begin() + j * N, pub.begin() + (j + 1) * N);
        host_fft(a, inv_root);
        for (u64 k = 0; k < N; ++k) q_coef[j][k] = a[k] * inv_n;
    }
    return q_coef;
}
void pcPublicEvalsAt(const std::vector<std::vector<F>> &q_coef, int n, u64 leaf, F *q0v, F *q1v) {
    const u64 N = 1ull << (n - 6);
    const F x0 = F::fastPow(F::getRootOfUnity(n - 1), leaf), x1 = F_ZERO - x0;
    for (size_t j = 0; j < q_coef.size(); ++j) {
        F q0 = F_ZERO, q1 = F_ZERO;                          // q_j(x) by Horner from the coefficient form
        for (u64 k = N; k-- > 0;) { q0 = q0 * x0 + q_coef[j][k]; q1 = q1 * x1 + q_coef[j][k]; }
        q0v[j] = q0; q1v[j] = q1;
    }
}
std::vector<F> pcPublicEvalsHostPub(int n, const std::vector<F> &pub, const std::vector<u64> &leaf0) {
    if (n < 7 || pub.size() != (1ull << n)) throw std::runtime_error("pcPublicEvalsHost: a public vector of 2^n entries, n >= 7");
    const auto q_coef = pcPublicCoefsHost(n, pub);
    std::vector<F> out(leaf0.size() * 128);
    for (size_t q = 0; q < leaf0.size(); ++q) pcPublicEvalsAt(q_coef, n, leaf0[q], &out[q * 128], &out[q * 128 + 64]);
    return out;
}
std::vector<F> pcPublicEvalsHost(int n, const std::vector<F> &point, const std::vector<u64> &leaf0) {
    if (n < 7 || (int) point.size() < n) throw std::runtime_error("pcPublicEvalsHost: a point of n coordinates, n >= 7");
    std::vector<F> pub;
    initBetaTable(pub, n, point.begin(), F_ONE);
    pub.resize(1ull << n);
    return pcPublicEvalsHostPub(n, pub, leaf0);
}
std::vector<F> pcPublicEvalsHostTensor(int n, const std::vector<F> &point, const std::vector<u64> &leaf0) {
    if (n < 7 || (int) point.size() < n) throw std::runtime_error("pcPublicEvalsHost: a point of n coordinates, n >= 7");
    const int ln = n - 6;
    std::vector<F> lo, hi;                                   // eq(point, j N + i) = hi[j] lo[i]
    initBetaTable(lo, ln, point.begin(), F_ONE);
    initBetaTable(hi, 6, point.begin() + ln, F_ONE);
    lo.resize(1ull << ln);
    host_fft(lo, F::getRootOfUnity(ln).inv());
    const F inv_n = F::fastPow(F((long long) (1ull << ln)), (unsigned __int128) F::mod - 2);
    std::vector<std::vector<F>> q_coef(1, std::vector<F>(lo.size()));
    for (size_t k = 0; k < lo.size(); ++k) q_coef[0][k] = lo[k] * inv_n;
    std::vector<F> out(leaf0.size() * 128);
    for (size_t q = 0; q < leaf0.size(); ++q) {
        F a, b;
        pcPublicEvalsAt(q_coef, n, leaf0[q], &a, &b);
        for (int j = 0; j < 64; ++j) { out[q * 128 + j] = hi[j] * a; out[q * 128 + 64 + j] = hi[j] * b; }
    }
    return out;
}

std::vector<F> pcMaskCoefsHost(const std::vector<F> &pub_mask, u64 ms) {                 // vpd_verifier.cpp:82-87
    if (ms < 1 || (ms & (ms - 1)) || pub_mask.size() > ms) throw std::runtime_error("pcMaskCoefsHost: a power of two ms, at most ms mask elements");
    std::vector<F> a(ms, F_ZERO);
    std::copy(pub_mask.begin(), pub_mask.end(), a.begin());
    if (ms == 1) return a;
    int lg = 0;
    while ((1ull << lg) < ms) ++lg;
    host_fft(a, F::getRootOfUnity(lg).inv());
    const F inv_n = F::fastPow(F((long long) ms), (unsigned __int128) F::mod - 2);
    for (auto &x : a) x = x * inv_n;
    return a;
}
static void pcMaskEvalsAt(const std::vector<F> &coef, int n, u64 leaf, F *out /* 2 */) {
    const F x0 = F::fastPow(F::getRootOfUnity(n - 1), leaf), x1 = F_ZERO - x0;
    F q0 = F_ZERO, q1 = F_ZERO;
    for (size_t k = coef.size(); k-- > 0;) { q0 = q0 * x0 + coef[k]; q1 = q1 * x1 + coef[k]; }
    out[0] = q0; out[1] = q1;
}
std::vector<F> pcMaskEvalsHost(int n, const std::vector<F> &pub_mask, u64 ms, const std::vector<u64> &leaf0) {
    if (n < 7) throw std::runtime_error("pcMaskEvalsHost: n >= 7");
    const std::vector<F> coef = pcMaskCoefsHost(pub_mask, ms);
    std::vector<F> out(leaf0.size() * 2);
    for (size_t q = 0; q < leaf0.size(); ++q) pcMaskEvalsAt(coef, n, leaf0[q], &out[2 * q]);
    return out;
}

u64 pcQueryAnswerBytes(int n, u64 n_queries) {
    u64 per = 2 * (2080 + 32ull * (n - 1));
    for (int k = 0; k < n - 6; ++k) per += 2080 + 32ull * (n - 2 - k);
    return per * n_queries;
}
// Recompute the leaf chain from the opened values (fri.cpp:96-124) and walk the path to the root (vpd_verifier.cpp:9-40).
void pcOpeningDigest(u64 leaf, const uint8_t *values, const uint8_t *path, size_t depth, uint8_t out[64]) {
    vph::hhash_digest h; memset(&h, 0, sizeof h);
    for (int s = 0; s < 65; ++s) {
        uint64_t m[4];
        memcpy(m, values + 32 * s, 32);
        h = vph::hhash(m, h);
    }
    memcpy(out, h.w, 32);
    u64 pos = leaf;
    for (size_t k = 0; k < depth; ++k) {
        vph::hhash_digest sib; memcpy(sib.w, path + 32 * k, 32);
        h = (pos & 1) ? vph::hhash(sib.w, h) : vph::hhash(h.w, sib);
        pos >>= 1;
    }
    memcpy(out + 32, h.w, 32);
}
std::vector<uint8_t> pcOpeningDigestsHost(int n, const std::vector<u64> &leaf0, const uint8_t *answer, u64 n_bytes) {
    if (n < 7 || n_bytes != pcQueryAnswerBytes(n, leaf0.size())) throw std::runtime_error("pcOpeningDigestsHost: not the size of a query answer");
    const int ln = n - 6;
    std::vector<uint8_t> out(leaf0.size() * (size_t) (2 + ln) * 64);
    size_t at = 0, o = 0;
    for (u64 l0 : leaf0) {
        u64 D = 1ull << (n - 1), t = l0;
        for (int oracle = 0; oracle < 2 + ln; ++oracle) {
            u64 leaf = l0;
            if (oracle >= 2) { const u64 Dn = D / 2; leaf = t % (Dn / 2); t = leaf; D = Dn; }
            const size_t plen = (size_t) (oracle < 2 ? n - 1 : n - 2 - (oracle - 2));        // depth + 1 digests; the last is the prover's copy of the leaf digest
            pcOpeningDigest(leaf, answer + at, answer + at + 2080, plen - 1, &out[o]);
            at += 2080 + 32 * plen; o += 64;
        }
    }
    return out;
}

// ---- the algebra of the commitment's verifier over all 65 slices (vpd_verifier.cpp:99-325), shared by verifyPoly and pcVerifyCommitment -------------------
// Slots 0 .. 63 are the witness slices on the N-th roots; slot 64 is the mask slice on the ms-th roots, with the public mask polynomial in q's place, x^ms in
// x^N's and ms in N's (:177-238).  The reference's own protocol is ms = 1 with one zero: q_msk = 0, and every value of slot 64 must then be zero.  Every
// function returns the name of the failed check, or an empty string.
namespace {
struct PcSliceCheck {
    int n, ln;
    u64 N, M, ms;
    const std::vector<F> &all_sum, &fr;
    F w, inv2, Nf, msf;
    std::vector<F> final_val, cur0, cur1;
    u64 D = 0, t = 0;
    PcSliceCheck(int n_, u64 ms_, const std::vector<F> &sums, const std::vector<F> &challenges)
        : n(n_), ln(n_ - 6), N(1ull << (n_ - 6)), M(1ull << (n_ - 1)), ms(ms_), all_sum(sums), fr(challenges), w(F::getRootOfUnity(n_ - 1)), inv2(F(2ll).inv()),
          Nf((long long) N), msf((long long) ms_), final_val(65), cur0(65), cur1(65) {}
    // The 64 witness slices' sums must add up to the claimed inner product.  Slot 64 is no part of it: input_0 is <witness, pub> alone (src/prover.cpp:544), and
    // all_sum[64] = <private mask, public mask> comes on top (poly_commit.h:262).  The sum over all 65 slots that stood here before let claim and all_sum[64]
    // move together; all_sum[64] now meets only the mask slice's own checks below, as in the reference (vpd_verifier.cpp:228-238), and cannot reach the claim.
    std::string sums(const F &claim) const {
        F s = F_ZERO;
        for (int j = 0; j < 64; ++j) s = s + all_sum[j];
        return s == claim ? "" : "commitment: slice sums do not match the inner product";
    }
    // the last codeword must be constant on its 32-point domain, per slice (vpd_verifier.cpp:309-325)
    std::string finalCodes(const std::vector<F> &final_code, const std::vector<F> &final_mask) {
        for (int s = 0; s < 64; ++s) {
            final_val[s] = final_code[(0 << 7) | (s << 1) | 0];
            for (int i = 0; i < 16; ++i)
                for (int hi = 0; hi < 2; ++hi)
                    if (final_code[(i << 7) | (s << 1) | hi] != final_val[s]) return "Fri rs code check fail";
        }
        final_val[64] = final_mask[0];
        for (int j = 1; j < 32; ++j) if (final_mask[j] != final_val[64]) return "Fri msk rs code check fail";
        return "";
    }
    // virtual oracle values at x0 = w^s0 and x1 = -x0 for every slice (poly_commit.h:301-318 on the prover side); q0v / q1v: the 64 public polynomials
    // there, qm: the public mask polynomial at the two points
    void first(u64 s0, const std::vector<F> &vl, const std::vector<F> &vh, const F *q0v, const F *q1v, const F *qm) {
        const F x0 = F::fastPow(w, s0), x1 = F_ZERO - x0;
        const F x0n = F::fastPow(x0, N), x1n = F::fastPow(x1, N), x0m = F::fastPow(x0, ms), x1m = F::fastPow(x1, ms);
        const F inv_x0 = x0.inv(), inv_x1 = F_ZERO - inv_x0;
        for (int j = 0; j < 64; ++j) {
            cur0[j] = ((vl[2 * j] * q0v[j] - (x0n - F_ONE) * vh[2 * j]) * Nf - all_sum[j]) * inv_x0;
            cur1[j] = ((vl[2 * j + 1] * q1v[j] - (x1n - F_ONE) * vh[2 * j + 1]) * Nf - all_sum[j]) * inv_x1;
        }
        cur0[64] = ((vl[128] * qm[0] - (x0m - F_ONE) * vh[128]) * msf - all_sum[64]) * inv_x0;
        cur1[64] = ((vl[129] * qm[1] - (x1m - F_ONE) * vh[129]) * msf - all_sum[64]) * inv_x1;
        D = M; t = s0;                               // D: domain size of the codeword cur0 / cur1 come from; cur0 is its value at index t, cur1 at t + D / 2
    }
    u64 levelLeaf() const { return t % (D / 4); }    // the folded value sits at index t of the next domain (D / 2 points), whose leaves pair i with i + D / 4
    // fold consistency of level k against its opening (vpd_verifier.cpp:167-306)
    std::string level(int k, const std::vector<F> &vb) {
        const F inv_mu = F::fastPow(F::fastPow(w, 1ull << k), t).inv();      // (w_D^t)^-1, w_D = w^(2^k)
        const u64 Dn = D / 2, leaf = t % (Dn / 2);
        const bool upper = t >= Dn / 2;
        for (int j = 0; j < 65; ++j) {
            const F expect = inv2 * ((cur0[j] + cur1[j]) + inv_mu * fr[k] * (cur0[j] - cur1[j]));
            if (expect != vb[2 * j + (upper ? 1 : 0)]) {
                char b[64];
                snprintf(b, sizeof b, j < 64 ? "Fri check consistency %d round fail" : "Fri msk check consistency %d round fail", k);
                return b;
            }
            cur0[j] = vb[2 * j]; cur1[j] = vb[2 * j + 1];
        }
        D = Dn; t = leaf;
        return "";
    }
    std::string last() const {                       // the last level's pairs are the final codewords' constants
        for (int j = 0; j < 65; ++j)
            if (cur0[j] != final_val[j] || cur1[j] != final_val[j]) return j < 64 ? "Fri final codeword mismatch" : "Fri msk final codeword mismatch";
        return "";
    }
};
}  // namespace

// device_digests: the opening's 64 bytes (leaf digest | root) computed elsewhere (poly_dev); the comparisons are the same
bool verifier::checkOpening(const vph::hhash_digest &root, u64 leaf, const std::vector<F> &vals,
                            const std::vector<prover::hhash_digest> &path, const uint8_t *device_digests) {
    if (vals.size() != 130 || path.empty()) return false;
    const size_t depth = path.size() - 1;
    uint8_t d[64];
    if (device_digests) memcpy(d, device_digests, 64);
    else {
        digest_timer.start();
        pcOpeningDigest(leaf, reinterpret_cast<const uint8_t *>(vals.data()), path[0].b, depth, d);
        digest_timer.stop();
    }
    if (memcmp(d, path[depth].b, 32) != 0) return false;
    return memcmp(d + 32, root.w, 32) == 0;
}

bool verifier::verifyPoly(const prover::hhash_digest &root_l_raw, const F &claim, int reps) {
    const int n = C.circuit[0].bitLength;
    if (n < 7) { fprintf(stderr, "commitment needs an input layer of at least 2^7 wires\n"); return false; }
    const int ln = n - 6, lm = n - 1;
    const u64 N = 1ull << ln, M = 1ull << lm;
    const vph::hhash_digest root_l = dig(root_l_raw);
    // public vector = eq(r_liu, .) over the input layer (verifier.cpp:368-369), and its slices in coefficient form
    // (public_array_prepare_generic, verifier.cpp:348-361)
    poly_timer.start();
    prover *const dev = poly_dev;
    std::vector<F> pub;
    if (!(dev && rec)) {                                     // a replay with the device loops needs the point only
        initBetaTable(pub, n, r_liu.begin(), F_ONE);
        pub.resize(1ull << n);
    }
    std::vector<std::vector<F>> q_coef;
    if (!dev) { pub_eval_timer.start(); q_coef = pcPublicCoefsHost(n, pub); pub_eval_timer.stop(); }
    poly_timer.stop();
    // prover: second oracle
    poly_prove_timer.start();
    F input_0;
    std::vector<F> all_sum;
    prover::hhash_digest root_h_raw;
    if (rec) { rec->bytes(root_h_raw.b, 32); input_0 = rec->elem(); all_sum.resize(65); for (auto &x : all_sum) x = rec->elem(); }
    else if (mask_ms > 1) root_h_raw = p->commit_public_eq(std::vector<F>(r_liu.begin(), r_liu.begin() + n), pub_mask_, input_0, all_sum);
    else root_h_raw = p->commit_public(pub, input_0, all_sum);
    poly_prove_timer.stop();
    full_tr.insert(full_tr.end(), root_h_raw.b, root_h_raw.b + 32);
    { const uint8_t *b = reinterpret_cast<const uint8_t *>(&input_0); full_tr.insert(full_tr.end(), b, b + 16); }
    { const uint8_t *b = reinterpret_cast<const uint8_t *>(all_sum.data()); full_tr.insert(full_tr.end(), b, b + 65 * 16); }
    const vph::hhash_digest root_h = dig(root_h_raw);
    poly_timer.start();
    if (claim != input_0) { fprintf(stderr, "Verification fail, final input check fail.\n"); return gkrFails(GKR_INPUT, 0, -1); }   // verifier.cpp:383
    std::vector<F> fr(ln);
    PcSliceCheck chk(n, mask_ms, all_sum, fr);
    auto failed = [&](const std::string &why) { if (why.empty()) return false; fprintf(stderr, "%s\n", why.c_str()); return true; };
    if (failed(chk.sums(input_0))) return false;
    poly_timer.stop();
    // verify_poly_commitment runs fft_circuit_gkr::fft_gkr(ln) here (vpd_verifier.cpp:92): a self-contained GKR over the inverse-FFT +
    // polynomial-evaluation circuit whose verifier draws come from the same glibc stream.  Its prover runs on the device (vp_fft_gkr) on
    // the tape drawn here in the reference's order; its verifier's checks run on the messages (fft_gkr_verify.hpp).  Its prover time is
    // part of the reported "Polynomial commitment: prove time" (vpd_verifier.cpp:94, src/verifier.cpp:183).  The FRI fold challenges
    // below — and the rand() query positions after them — continue the stream exactly where the reference's do (pinned against its
    // recorded challenges).
    {
        std::vector<F> ftape((size_t) fftGkrDraws(ln));
        for (auto &x : ftape) x = F::random();
        poly_prove_timer.start();
        fft_gkr_timer.start();
        std::vector<F> fmsgs;
        if (rec) { fmsgs.resize(vph::FftGkrLayout(ln).n_msgs); for (auto &x : fmsgs) x = rec->elem(); }
        else fmsgs = p->fftGkr(ln, ftape);
        fft_gkr_timer.stop();
        poly_prove_timer.stop();
        fft_gkr_msgs_ = fmsgs;
        poly_timer.start();
        const bool okf = vph::fft_gkr_check<F>(ln, ftape.data(), ftape.size(), fmsgs.data(), fmsgs.size(), F::getRootOfUnity(ln).inv());
        poly_timer.stop();
        if (!okf) { fprintf(stderr, "Error, fft gkr failed\n"); return false; }     // (the reference prints this and carries on, fft_circuit_GKR.cpp:843-844)
    }
    // FRI commit phase (vpd_verifier.cpp:44-74): the fold challenges are drawn here
    std::vector<vph::hhash_digest> roots(ln);
    poly_prove_timer.start();
    std::vector<F> final_code, final_mask(32, F_ZERO);          // the zero mask's last codeword is zero: nothing is asked of the prover
    if (rec) {                  // the same draws; roots and final codeword from the record
        for (int k = 0; k < ln; ++k) fr[k] = F::random();
        for (int k = 0; k < ln; ++k) rec->bytes(roots[k].w, 32);
        final_code.resize(2048); for (auto &x : final_code) x = rec->elem();
        if (mask_ms > 1) {      // version 2: the mask section (its two lengths were read and checked by checkFull, which looked ahead for them)
            uint32_t lens[2]; rec->bytes(lens, sizeof lens);
            if (lens[0] != mask_ms || lens[1] < 1 || lens[1] > mask_ms) throw std::runtime_error("record: mask section");
            pub_mask_.resize(lens[1]); for (auto &x : pub_mask_) x = rec->elem();
            for (auto &x : final_mask) x = rec->elem();
        }
    } else {
    if (fri_batched) {          // same draws in the same order; the device runs the whole commit phase in one pass
        for (int k = 0; k < ln; ++k) fr[k] = F::random();
        const auto ds = p->friCommit(fr);
        for (int k = 0; k < ln; ++k) roots[k] = dig(ds[k]);
    } else
        for (int k = 0; k < ln; ++k) { fr[k] = F::random(); roots[k] = dig(p->friStep(fr[k])); }
    final_code = p->friFinal();
    if (mask_ms > 1) final_mask = p->friFinalMask();
    }
    fri_roots_.clear();
    for (int k = 0; k < ln; ++k) { const uint8_t *b = reinterpret_cast<const uint8_t *>(roots[k].w); fri_roots_.insert(fri_roots_.end(), b, b + 32); }
    fri_final_ = final_code; fri_r_ = fr; fri_final_mask_ = final_mask;
    poly_prove_timer.stop();
    poly_timer.start();
    if (failed(chk.finalCodes(final_code, final_mask))) return false;
    // the public mask polynomial (vpd_verifier.cpp:82-87); the zero mask's is zero
    std::vector<F> mask_coef;
    if (mask_ms > 1 && !dev) { pub_eval_timer.start(); mask_coef = pcMaskCoefsHost(pub_mask_, mask_ms); pub_eval_timer.stop(); }
    std::vector<F> vl, vh, vb;
    std::vector<prover::hhash_digest> pl, ph, pb;
    // query point x0 = w^(pow/2), pow even in [N, M) (vpd_verifier.cpp:119-123); pow / 2 is the leaf of the two first oracles (x1 = -x0 sits in the same leaf)
    auto draw_leaf = [&]() { u64 pw; do { pw = (u64) rand() % M; } while (pw < N || (pw & 1)); return pw / 2; };
    // Where the openings come from: one prover::friOpen each (the default), or a block of bytes in vp_fri_query's layout — the answer of ONE
    // prover::friQuery to all positions (batched_openings), or the record's last section (checkFull).  Either way they are kept for the record.
    const bool positions_first = rec || batched_openings || dev;
    std::vector<u64> leaf0((size_t) reps);
    if (positions_first) for (auto &x : leaf0) x = draw_leaf();
    openings_.clear();
    RecReader answer{nullptr, 0, 0}, *src = rec;
    if (!rec && (batched_openings || dev)) {
        poly_timer.stop(); open_timer.start();
        openings_ = p->friQuery(leaf0);
        open_timer.stop(); poly_timer.start();
        answer = RecReader{openings_.data(), openings_.size(), 0}; src = &answer;
    }
    // poly_dev: the q values of every position and the digests of every opening in two device calls over the whole answer block (the record's
    // remaining bytes, or friQuery's answer); a block that is not the layout's size is rejected here, as the reader below would reject it
    std::vector<F> dev_q, dev_qm;
    std::vector<uint8_t> dev_dig;
    size_t dev_opening = 0;
    if (dev) {
        const uint8_t *blk = src->p + src->at;
        const u64 nb = src->n - src->at;
        if (nb != pcQueryAnswerBytes(n, (u64) reps)) { fprintf(stderr, "commitment: the query answer is not the size of %d repetitions\n", reps); poly_timer.stop(); return false; }
        pub_eval_timer.start();
        dev_q = dev->pcPublicEvals(n, std::vector<F>(r_liu.begin(), r_liu.begin() + n), leaf0);
        if (mask_ms > 1) dev_qm = dev->pcMaskEvals(n, pub_mask_, mask_ms, leaf0);
        pub_eval_timer.stop();
        digest_timer.start();
        dev_dig = dev->pcOpeningDigests(n, leaf0, blk, nb);
        digest_timer.stop();
    }
    auto opening_ok = [&](const vph::hhash_digest &root, u64 leaf, const std::vector<F> &vals, const std::vector<prover::hhash_digest> &path) {
        return checkOpening(root, leaf, vals, path, dev ? &dev_dig[64 * dev_opening++] : nullptr);
    };
    auto open = [&](int oracle, u64 leaf, std::vector<F> &vals, std::vector<prover::hhash_digest> &path) {
        if (src) {
            vals.resize(130); for (auto &x : vals) x = src->elem();
            path.resize((size_t) (oracle < 2 ? n - 1 : n - 2 - (oracle - 2)));
            src->bytes(path.data(), 32 * path.size());
            return;
        }
        poly_timer.stop(); open_timer.start();
        p->friOpen(oracle, leaf, vals, path);
        open_timer.stop(); poly_timer.start();
        const uint8_t *b = reinterpret_cast<const uint8_t *>(vals.data());
        openings_.insert(openings_.end(), b, b + 130 * sizeof(F));
        openings_.insert(openings_.end(), path[0].b, path[0].b + 32 * path.size());
    };
    for (int rep = 0; rep < reps; ++rep) {
        const u64 s0 = positions_first ? leaf0[rep] : draw_leaf();
        open(0, s0, vl, pl);
        open(1, s0, vh, ph);
        if (!opening_ok(root_l, s0, vl, pl) || !opening_ok(root_h, s0, vh, ph)) { fprintf(stderr, "commitment: Merkle opening rejected\n"); return false; }
        // the public polynomials at x0 = w^s0 and x1 = -x0: the 64 slices', and the mask's
        std::vector<F> q0v(64), q1v(64);
        F qm[2] = {F_ZERO, F_ZERO};
        if (dev) {
            std::copy_n(&dev_q[(size_t) rep * 128], 64, q0v.begin()); std::copy_n(&dev_q[(size_t) rep * 128 + 64], 64, q1v.begin());
            if (mask_ms > 1) { qm[0] = dev_qm[2 * (size_t) rep]; qm[1] = dev_qm[2 * (size_t) rep + 1]; }
        } else {
            pub_eval_timer.start();
            pcPublicEvalsAt(q_coef, n, s0, q0v.data(), q1v.data());
            if (mask_ms > 1) pcMaskEvalsAt(mask_coef, n, s0, qm);
            pub_eval_timer.stop();
        }
        chk.first(s0, vl, vh, q0v.data(), q1v.data(), qm);
        for (int k = 0; k < ln; ++k) {
            const u64 leaf = chk.levelLeaf();
            open(2 + k, leaf, vb, pb);
            if (!opening_ok(roots[k], leaf, vb, pb)) { fprintf(stderr, "commitment: FRI Merkle opening rejected (level %d)\n", k); return false; }
            if (failed(chk.level(k, vb))) return false;
        }
        if (failed(chk.last())) return false;
    }
    poly_timer.stop();
    if (src == &answer && answer.at != answer.n) { fprintf(stderr, "commitment: the query answer has bytes left over\n"); return false; }
    return true;
}

// The commitment's verifier on arrays: verifyPoly's checks behind fft_gkr, in its order, with every challenge, position and prover message an argument.
int pcVerifyCommitment(const PcCommitment &c, std::string &why, vp_ctx *dev) {
    const int n = c.n;
    auto bad = [&](const char *m) { why = m; return -1; };
    if (n < 7 || n > 30) return bad("n outside 7 .. 30");
    const int ln = n - 6;
    const u64 reps = c.leaf0.size();
    if (c.point.empty() == c.pub.empty()) return bad("exactly one of point and pub");
    if (!c.point.empty() ? c.point.size() != (size_t) n : c.pub.size() != (1ull << n)) return bad("a point of n coordinates or a public vector of 2^n entries");
    // the padded lengths a commitment can have: the zero mask's 1, or what vp_commit_private_masked takes
    if (c.ms != 1 && (c.ms < 8 || (c.ms & (c.ms - 1)) || c.ms > (1ull << 16) || c.ms > (1ull << (n - 2)))) return bad("ms is neither 1 nor a power of two in [8, min(2^16, 2^(n-2))]");
    if (c.pub_mask.size() > c.ms) return bad("public mask longer than ms");
    if (c.all_sum.size() != 65 || c.fr.size() != (size_t) ln || c.fri_roots.size() != (size_t) 32 * ln || c.final_code.size() != 2048 || c.final_mask.size() != 32)
        return bad("all_sum[65], n - 6 challenges and roots, final_code[2048], final_mask[32]");
    if (reps < 1 || reps > 4096) return bad("1 .. 4096 repetitions");
    for (u64 l : c.leaf0) if (l < (1ull << (n - 7)) || l >= (1ull << (n - 2))) return bad("a leaf outside [N / 2, M / 2)");
    if (!c.answer || c.n_bytes != pcQueryAnswerBytes(n, reps)) return bad("the answer block is not the size of vp_fri_query's answer");
    auto rejected = [&](const std::string &m) { if (m.empty()) return false; why = m; return true; };
    PcSliceCheck chk(n, c.ms, c.all_sum, c.fr);
    if (rejected(chk.sums(c.claim))) return 1;
    if (rejected(chk.finalCodes(c.final_code, c.final_mask))) return 1;
    // the two heavy loops, and the mask row, over all positions: on the device or on the host
    std::vector<F> q, qm(2 * reps, F_ZERO);
    std::vector<uint8_t> dg;
    if (dev) {
        auto call = [&](int rc, const char *what) { if (rc != VP_OK) throw std::runtime_error(std::string(what) + ": " + vp_last_error(dev)); };
        q.resize(128 * reps); dg.resize(reps * (size_t) (n - 4) * 64);
        const uint64_t *lf = reinterpret_cast<const uint64_t *>(c.leaf0.data());
        call(vp_pc_public_evals(dev, n, c.point.empty() ? nullptr : reinterpret_cast<const vp_F *>(c.point.data()), c.pub.empty() ? nullptr : reinterpret_cast<const vp_F *>(c.pub.data()),
                                (int) reps, lf, reinterpret_cast<vp_F *>(q.data())), "vp_pc_public_evals");
        const std::vector<F> one_zero(1, F_ZERO), &pm = c.pub_mask.empty() ? one_zero : c.pub_mask;
        if (c.ms > 1) call(vp_pc_mask_evals(dev, n, reinterpret_cast<const vp_F *>(pm.data()), pm.size(), c.ms, (int) reps, lf, reinterpret_cast<vp_F *>(qm.data())), "vp_pc_mask_evals");
        call(vp_fri_query_digests(dev, n, (int) reps, lf, c.answer, c.n_bytes, dg.data()), "vp_fri_query_digests");
    } else {
        q = c.point.empty() ? pcPublicEvalsHostPub(n, c.pub, c.leaf0) : pcPublicEvalsHostTensor(n, c.point, c.leaf0);
        if (c.ms > 1) qm = pcMaskEvalsHost(n, c.pub_mask, c.ms, c.leaf0);
        dg = pcOpeningDigestsHost(n, c.leaf0, c.answer, c.n_bytes);
    }
    std::vector<F> vl(130), vh(130), vb(130);
    size_t at = 0, opening = 0;                      // (the block has the layout's size: every read below stays inside it)
    // one opening of the block: its values (canonical), then the comparisons of checkOpening on its 64 digest bytes
    auto open = [&](std::vector<F> &vals, size_t plen, const uint8_t *root) {
        for (auto &x : vals) {
            unsigned long long w[2]; memcpy(w, c.answer + at, 16); at += 16;
            if (w[0] >= F::mod || w[1] >= F::mod) throw std::runtime_error("non-canonical field element among the opened values");
            x.real = w[0]; x.img = w[1];
        }
        const uint8_t *path = c.answer + at;
        at += 32 * plen;
        const uint8_t *d = &dg[64 * opening++];
        return memcmp(d, path + 32 * (plen - 1), 32) == 0 && memcmp(d + 32, root, 32) == 0;
    };
    try {
        for (u64 rep = 0; rep < reps; ++rep) {
            const bool okl = open(vl, (size_t) n - 1, c.root_l), okh = open(vh, (size_t) n - 1, c.root_h);
            if (!okl || !okh) { why = "commitment: Merkle opening rejected"; return 1; }
            chk.first(c.leaf0[rep], vl, vh, &q[128 * rep], &q[128 * rep + 64], &qm[2 * rep]);
            for (int k = 0; k < ln; ++k) {
                if (!open(vb, (size_t) (n - 2 - k), &c.fri_roots[32 * (size_t) k])) { why = "commitment: FRI Merkle opening rejected (level " + std::to_string(k) + ")"; return 1; }
                if (rejected(chk.level(k, vb))) return 1;
            }
            if (rejected(chk.last())) return 1;
        }
    } catch (const std::runtime_error &e) { why = e.what(); return 1; }      // a non-canonical element among the opened values
    return 0;
}

// ---- the non-interactive commitment proof: the chain's fixed parts, the parser and the verifier (no algebra here: pcVerifyCommitment decides) ----------------
int pcParseCommitmentFS(const uint8_t *proof, u64 len, PcCommitment &c, std::string &why) {
    auto bad = [&](const char *m) { why = m; return -1; };
    if (!proof) return bad("no proof");
    u64 at = 0;
    auto have = [&](u64 k) { return k <= len - at; };            // (at <= len throughout)
    if (!have(32)) return bad("proof shorter than its header");
    uint32_t h32[4]; u64 h64[2];
    memcpy(h32, proof, 16); memcpy(h64, proof + 16, 16); at = 32;
    if (h32[0] != PCFS_MAGIC) return bad("not a commitment proof (magic)");
    if (h32[1] != PCFS_VERSION && h32[1] != PCFS_VERSION_POW) return bad("a commitment proof of another version");
    PcFsWork work;
    if (h32[1] == PCFS_VERSION_POW) {
        if (!have(16)) return bad("proof shorter than its header");
        if (!pcFsWorkHeader(proof + at, work)) return bad("pow_bits outside 1 .. 48 (no work is version 1)");
        at += 16;
    }
    const u64 n = h32[2], reps = h32[3], ms = h64[0], n_pub = h64[1];
    if (n < 7 || n > 30) return bad("n outside 7 .. 30");
    if (reps < 1 || reps > 4096) return bad("1 .. 4096 repetitions");
    if (ms != 1 && (ms < 8 || (ms & (ms - 1)) || ms > (1ull << 16) || ms > (1ull << (n - 2)))) return bad("ms is neither 1 nor a power of two in [8, min(2^16, 2^(n-2))]");
    if (ms == 1 ? n_pub != 0 : n_pub > ms) return bad("public mask longer than ms (none with the zero mask)");
    const u64 ln = n - 6;
    bool canon = true;
    auto elems = [&](std::vector<F> &v, u64 k) {
        if (!have(16 * k)) return false;
        v.resize(k);
        for (u64 i = 0; i < k; ++i) {
            unsigned long long w[2]; memcpy(w, proof + at, 16); at += 16;
            if (w[0] >= F::mod || w[1] >= F::mod) canon = false;
            v[i].real = w[0]; v[i].img = w[1];
        }
        return true;
    };
    auto bytes = [&](uint8_t *dst, u64 k) { if (!have(k)) return false; memcpy(dst, proof + at, k); at += k; return true; };
    c = PcCommitment{};
    c.n = (int) n; c.ms = ms;
    std::vector<F> claim;
    c.fri_roots.resize(32 * ln);
    if (!elems(c.point, n) || !elems(c.pub_mask, n_pub) || !elems(claim, 1) || !bytes(c.root_l, 32) || !bytes(c.root_h, 32) || !elems(c.all_sum, 65) ||
        !bytes(c.fri_roots.data(), 32 * ln) || !elems(c.final_code, 2048) || !elems(c.final_mask, 32))
        return bad("proof shorter than its sections");
    if (!canon) return bad("non-canonical field element in the proof");
    c.claim = claim[0];
    c.n_bytes = pcQueryAnswerBytes((int) n, reps);
    if (len - at != c.n_bytes) return bad("the proof does not end where the answer ends");
    c.answer = proof + at;
    // the challenges and positions: nobody hands them over
    vph::fs_chain ch;
    pcFsAbsorbHead(ch, (int) n, reps, ms, c.point, c.pub_mask, c.claim, c.root_l, c.root_h, c.all_sum);
    c.fr.resize(ln);
    c.fr[0] = pcFsFirstChallenge(ch);
    for (u64 k = 0; k < ln; ++k) { F next; if (pcFsLevel(ch, (int) k, (int) ln, &c.fri_roots[32 * k], &next)) c.fr[k + 1] = next; }
    c.leaf0 = pcFsPositions(ch, (int) n, reps, c.final_code, c.final_mask, &work);
    c.pow_bits = work.bits; c.pow_nonce = work.nonce; c.pow_met = work.met;
    return 0;
}
int pcCheckWork(u64 pow_bits, u64 pow_nonce, bool met, int min_pow_bits, std::string &why) {
    if (!met) { why = "proof of work not met: W(" + std::to_string(pow_bits) + ", " + std::to_string(pow_nonce) + ") leaves a non-zero bit among the low " + std::to_string(pow_bits); return 1; }
    if (min_pow_bits > 0 && pow_bits < (u64) min_pow_bits) {
        why = "proof of work of " + std::to_string(pow_bits) + " bits, the verifier demands " + std::to_string(min_pow_bits);
        return 1;
    }
    return 0;
}
int pcVerifyCommitmentFS(const uint8_t *proof, u64 len, std::string &why, vp_ctx *dev, int min_pow_bits) {
    PcCommitment c;
    if (pcParseCommitmentFS(proof, len, c, why) != 0) return -1;
    if (pcCheckWork(c.pow_bits, c.pow_nonce, c.pow_met, min_pow_bits, why)) return 1;
    return pcVerifyCommitment(c, why, dev);
}

// F::random() draws of fft_circuit_gkr::fft_gkr(lg) (lib/virgo/src/fft_circuit_GKR.cpp): r[lg] (:840), eval_points[64] (:84),
// r_0 and r_1 of lg + 10 entries (:789-790 via :106), the addition layer's r_u / r_v of lg + 6 (:275-276), the multiplication
// layer's of lg (:394-395), and per iFFT depth (lg of them) r_u / r_v of lg plus alpha and beta (:563-564, :763-764).
int verifier::fftGkrDraws(int lg) { return lg + 64 + 2 * (lg + 10) + 2 * (lg + 6) + 2 * lg + lg * (2 * lg + 2); }

bool verifier::verifyFull(int reps) { return verifyFull(reps, {}, {}); }
bool verifier::verifyFull(int reps, const std::vector<F> &pri_mask, const std::vector<F> &pub_mask) {
    if (!p) throw std::runtime_error("verifyFull(): no prover attached");
    full_tr.clear();
    poly_prove_timer.start();
    const prover::hhash_digest root_l = p->commit_private(pri_mask);       // verifier.cpp:137 (an empty or all-zero mask: commit_private())
    poly_prove_timer.stop();
    mask_ms = 1; pub_mask_.clear();
    if (p->isMasked()) {                                                   // the padded length is public: M / the largest power of two <= M / length (poly_commit.h:55-63)
        const u64 M = 1ull << (C.circuit[0].bitLength - 1);
        u64 gap = 1;
        while (gap * 2 <= M / pri_mask.size()) gap *= 2;
        mask_ms = M / gap;
        pub_mask_ = pub_mask.empty() ? std::vector<F>(1, F_ZERO) : pub_mask;
    }
    full_tr.insert(full_tr.end(), root_l.b, root_l.b + 32);
    replay = false; tape_.clear(); tr.clear();
    input_check_by_commitment = true;
    const bool ok = run();
    input_check_by_commitment = false;
    full_tr.insert(full_tr.end(), tr.begin(), tr.end());
    record_.clear();
    if (!ok) return false;
    if (!verifyPoly(root_l, last_claim, reps)) return false;
    // the record (vphost.h): header, transcript in the golden layout, fft_gkr messages, FRI roots, final codeword, openings
    // (version 2, a masked run: the mask section in front of the openings)
    const bool masked = mask_ms > 1;
    const uint32_t head[4] = {RECORD_MAGIC, masked ? RECORD_VERSION_MASKED : RECORD_VERSION, (uint32_t) C.circuit[0].bitLength, (uint32_t) reps};
    auto put = [&](const void *b, size_t k) { const uint8_t *q = static_cast<const uint8_t *>(b); record_.insert(record_.end(), q, q + k); };
    put(head, sizeof head);
    put(full_tr.data(), full_tr.size());
    put(fft_gkr_msgs_.data(), fft_gkr_msgs_.size() * sizeof(F));
    put(fri_roots_.data(), fri_roots_.size());
    put(fri_final_.data(), fri_final_.size() * sizeof(F));
    if (masked) {
        const uint32_t lens[2] = {(uint32_t) mask_ms, (uint32_t) pub_mask_.size()};
        put(lens, sizeof lens);
        put(pub_mask_.data(), pub_mask_.size() * sizeof(F));
        put(fri_final_mask_.data(), fri_final_mask_.size() * sizeof(F));
    }
    put(openings_.data(), openings_.size());
    return true;
}

bool verifier::checkFull(const std::vector<uint8_t> &record) {
    record_.clear();
    const int n = C.circuit[0].bitLength;
    if (n < 7) return false;
    RecReader r{record.data(), record.size(), 0};
    bool ok = false;
    try {
        uint32_t head[4];
        r.bytes(head, sizeof head);
        if (head[0] != RECORD_MAGIC || (head[1] != RECORD_VERSION && head[1] != RECORD_VERSION_MASKED) || head[2] != (uint32_t) n || head[3] < 1 || head[3] > 4096) return false;
        mask_ms = 1; pub_mask_.clear();
        prover::hhash_digest root_l;
        r.bytes(root_l.b, 32);
        // GKR slice: the replay of check(), on the tape redrawn here; it ends where run() stops reading
        const std::vector<F> tape = drawTape();
        const std::vector<uint8_t> rest(record.begin() + r.at, record.end());
        replay = true; rtape = &tape; rtr = &rest; tape_pos = 0; tr_pos = 0; tr.clear();
        input_check_by_commitment = true;
        ok = run() && tape_pos == tape.size();
        input_check_by_commitment = false;
        if (ok) {
            r.at += tr_pos;
            full_tr.assign(root_l.b, root_l.b + 32);
            full_tr.insert(full_tr.end(), tr.begin(), tr.end());
            if (head[1] == RECORD_VERSION_MASKED) {
                // the mask's padded length decides slot 64's algebra from the first check on: read it ahead, at its place behind the final codeword (the
                // sections in between have fixed sizes), under a masked run's own limits — a power of two in [8, min(2^16, 2^(n-2))]
                RecReader ahead = r;
                ahead.at += 32 + 16 + 65 * 16;
                for (size_t skip : {vph::FftGkrLayout(n - 6).n_msgs * sizeof(F), (size_t) 32 * (n - 6), (size_t) 2048 * sizeof(F)}) {
                    if (skip > ahead.n - std::min(ahead.at, ahead.n)) throw std::runtime_error("record too short");
                    ahead.at += skip;
                }
                uint32_t lens[2]; ahead.bytes(lens, sizeof lens);
                const u64 ms = lens[0];
                if (ms < 8 || (ms & (ms - 1)) || ms > (1ull << 16) || ms > (1ull << (n - 2))) throw std::runtime_error("record: mask length");
                mask_ms = ms;
            }
            rec = &r;
            ok = verifyPoly(root_l, last_claim, (int) head[3]) && r.at == r.n;
        }
    } catch (const std::runtime_error &) { ok = false; }      // short record / non-canonical element
    rec = nullptr; input_check_by_commitment = false;
    return ok;
}

// ---- the joined non-interactive proof (chain and layout: vphost.h, "The joined proof") ------------------------------------------------------------------------
constexpr uint32_t FULLFS_MAGIC = 0x46465056u, FULLFS_VERSION = 1;      // "VPFF", version 1
// steps 1 and 2 of the chain: the statement without the input values, then the head
void verifier::fullFsHead(int n, u64 reps, u64 ms, const std::vector<F> &pub_mask, const uint8_t root_l[32]) {
    fsInit(false);
    const u64 n_pub = ms == 1 ? 0 : pub_mask.size();
    fs_state.param((u64) n, reps, ms, n_pub);
    for (u64 i = 0; i < n_pub; ++i) fs_state.elem(pub_mask[i].real, pub_mask[i].img);
    fs_state.digest(0, root_l);
}
std::vector<uint8_t> verifier::proveFullFS(int reps, const std::vector<F> &pri_mask, const std::vector<F> &pub_mask, bool device_gkr, int pow_bits) {
    if (!p) throw std::runtime_error("proveFullFS(): no prover attached");
    if (p->world() > 1 || p->commitmentSharded()) throw std::runtime_error("proveFullFS: not built for a sharded session");
    if (pow_bits < 0 || pow_bits > PCFS_POW_PROVER_BITS) throw std::invalid_argument("proveFullFS: pow_bits outside 0 .. 32");
    const int n = C.circuit[0].bitLength, ln = n - 6;
    if (n < 7) throw std::runtime_error("proveFullFS: the commitment needs an input layer of at least 2^7 wires");
    if (reps < 1 || reps > 4096) throw std::runtime_error("proveFullFS: 1 .. 4096 repetitions");
    const prover::hhash_digest root_l = p->commit_private(pri_mask);
    u64 ms = 1;
    if (p->isMasked()) {
        const u64 M = 1ull << (n - 1);
        u64 gap = 1;
        while (gap * 2 <= M / pri_mask.size()) gap *= 2;
        ms = M / gap;
    }
    const std::vector<F> pm = ms > 1 ? pub_mask : std::vector<F>();
    // ---- the GKR part: run() in FS mode, the claim left to the commitment
    replay = false; fs = !device_gkr; tape_.clear(); tr.clear();
    fullFsHead(n, (u64) reps, ms, pm, root_l.b);
    if (device_gkr) {
        // the prover alone: every challenge drawn on the device; the point is r_liu of layer 1 in its tape slots, the claim the transcript's last element
        uint8_t st[32];
        memcpy(st, fs_state.s.w, 32);
        u64 draws = 0;
        tr = p->proveGkrFS(st, tape_, draws);
        memcpy(fs_state.s.w, st, 32);
        fs_ctr = draws;
        const vph::GkrLayout L(C);
        for (int j = 0; j < n; ++j) r_liu[j] = tape_[L.rl[1] + j];
        unsigned long long w[2];
        memcpy(w, tr.data() + tr.size() - 16, 16);
        last_claim.real = w[0]; last_claim.img = w[1];
    } else {
    input_check_by_commitment = true;
    bool ok = false;
    try { ok = run(); } catch (...) { fs = false; input_check_by_commitment = false; throw; }
    fs = false; input_check_by_commitment = false;
    if (!ok) throw std::runtime_error("proveFullFS: the GKR part of the prover's own proof is rejected");
    }
    const std::vector<uint8_t> gkr = tr;
    full_fs_point_.assign(r_liu.begin(), r_liu.begin() + n);
    // ---- the commitment head
    F input_0;
    std::vector<F> all_sum;
    const prover::hhash_digest root_h = p->commit_public_eq(full_fs_point_, pm, input_0, all_sum);
    vph::fs_chain ch = fs_state;
    ch.elem(input_0.real, input_0.img);
    for (int i = 0; i < 65; ++i) ch.elem(all_sum[i].real, all_sum[i].img);
    ch.digest(1, root_h.b);
    // ---- fft_gkr, every challenge drawn on the device; fftGkrFS re-derives the tape and the state from the returned messages
    uint8_t st[32];
    memcpy(st, ch.s.w, 32);
    std::vector<F> ftape;
    const std::vector<F> fmsgs = p->fftGkrFS(ln, st, ftape);
    memcpy(ch.s.w, st, 32);
    // ---- the FRI commit phase from that state, checked against the host's chain over the returned roots
    std::vector<uint8_t> roots;
    p->friCommitFS(ch, roots);
    const std::vector<F> fin = p->friFinal(), fm = p->friFinalMask();
    PcFsWork work;
    work.bits = (u64) pow_bits;
    work.find = [&](const vph::hhash_digest &st) { return p->fsGrind(st, pow_bits, true); };
    const std::vector<u64> lf = pcFsPositions(ch, n, (u64) reps, fin, fm, &work);
    if (!work.met) throw std::runtime_error("proveFullFS: the device's nonce does not meet the work");
    const std::vector<uint8_t> ans = p->friQuery(lf);
    std::vector<uint8_t> out;
    auto put = [&](const void *b, size_t k) { const uint8_t *q = static_cast<const uint8_t *>(b); out.insert(out.end(), q, q + k); };
    const uint32_t h32[4] = {FULLFS_MAGIC, pow_bits ? PCFS_VERSION_POW : FULLFS_VERSION, (uint32_t) n, (uint32_t) reps};
    const uint64_t h64[2] = {ms, ms == 1 ? 0 : pm.size()};
    put(h32, sizeof h32); put(h64, sizeof h64);
    if (pow_bits) { const uint64_t hw[2] = {work.bits, work.nonce}; put(hw, sizeof hw); }
    if (ms != 1) put(pm.data(), pm.size() * sizeof(F));
    put(root_l.b, 32);
    put(gkr.data(), gkr.size());
    put(root_h.b, 32);
    put(&input_0, sizeof(F));
    put(all_sum.data(), 65 * sizeof(F));
    put(fmsgs.data(), fmsgs.size() * sizeof(F));
    put(roots.data(), roots.size());
    put(fin.data(), fin.size() * sizeof(F));
    put(fm.data(), fm.size() * sizeof(F));
    put(ans.data(), ans.size());
    return out;
}
int verifier::checkFullFS(const uint8_t *proof, u64 len, std::string &why, vp_ctx *dev, int min_pow_bits) {
    auto bad = [&](const char *m) { why = m; return -1; };
    full_fs_point_.clear();
    full_fs_pow_[0] = full_fs_pow_[1] = 0;
    if (!proof) return bad("no proof");
    u64 at = 0;
    auto have = [&](u64 k) { return k <= len - at; };            // (at <= len throughout)
    if (!have(32)) return bad("proof shorter than its header");
    uint32_t h32[4]; u64 h64[2];
    memcpy(h32, proof, 16); memcpy(h64, proof + 16, 16); at = 32;
    if (h32[0] != FULLFS_MAGIC) return bad("not a joined proof (magic)");
    if (h32[1] != FULLFS_VERSION && h32[1] != PCFS_VERSION_POW) return bad("a joined proof of another version");
    PcFsWork work;
    if (h32[1] == PCFS_VERSION_POW) {
        if (!have(16)) return bad("proof shorter than its header");
        if (!pcFsWorkHeader(proof + at, work)) return bad("pow_bits outside 1 .. 48 (no work is version 1)");
        at += 16;
    }
    const u64 n = h32[2], reps = h32[3], ms = h64[0], n_pub = h64[1];
    if (n < 7 || n > 30 || (int) n != C.circuit[0].bitLength) return bad("n is not the bit length of the circuit's input layer (7 .. 30)");
    if (reps < 1 || reps > 4096) return bad("1 .. 4096 repetitions");
    if (ms != 1 && (ms < 8 || (ms & (ms - 1)) || ms > (1ull << 16) || ms > (1ull << (n - 2)))) return bad("ms is neither 1 nor a power of two in [8, min(2^16, 2^(n-2))]");
    if (ms == 1 ? n_pub != 0 : n_pub > ms) return bad("public mask longer than ms (none with the zero mask)");
    // the verifier's demand is decided by the header: no replay of the GKR part for a proof that carries too little work (the work itself: where the chain reaches it)
    full_fs_pow_[0] = work.bits; full_fs_pow_[1] = work.nonce;
    if (pcCheckWork(work.bits, work.nonce, true, min_pow_bits, why)) return 1;
    const u64 ln = n - 6;
    bool canon = true;
    auto elems = [&](std::vector<F> &v, u64 k) {
        if (!have(16 * k)) return false;
        v.resize(k);
        for (u64 i = 0; i < k; ++i) {
            unsigned long long w[2]; memcpy(w, proof + at, 16); at += 16;
            if (w[0] >= F::mod || w[1] >= F::mod) canon = false;
            v[i].real = w[0]; v[i].img = w[1];
        }
        return true;
    };
    auto bytes = [&](uint8_t *dst, u64 k) { if (!have(k)) return false; memcpy(dst, proof + at, k); at += k; return true; };
    PcCommitment c;
    c.n = (int) n; c.ms = ms;
    if (!elems(c.pub_mask, n_pub) || !bytes(c.root_l, 32)) return bad("proof shorter than its sections");
    if (!canon) return bad("non-canonical field element in the proof");
    // ---- the GKR part: the replay of checkFS on the bytes behind root_l; it ends where run() stops reading
    const std::vector<uint8_t> rest(proof + at, proof + len);
    static const std::vector<F> no_tape;
    replay = true; fs = true; rtape = &no_tape; rtr = &rest; tape_pos = 0; tr_pos = 0; tr.clear(); tape_.clear();
    fullFsHead((int) n, reps, ms, c.pub_mask, c.root_l);
    input_check_by_commitment = true;
    bool ok = false, malformed = false;
    try { ok = run(); } catch (const std::exception &e) { malformed = true; why = e.what(); }      // the proof ends inside the GKR part / a non-canonical element
    fs = false; input_check_by_commitment = false;
    if (malformed) return -1;
    full_fs_point_.assign(r_liu.begin(), r_liu.begin() + n);      // as far as the replay got: a rejected GKR part leaves the coordinates it had derived
    if (!ok) {
        const GkrFailure f = lastGkrFailure();
        why = "the GKR part is rejected (a sumcheck round, a layer's final value or a Liu sumcheck): " + std::string(gkrCheckName(f.kind)) + ", layer " + std::to_string(f.layer) +
              ", round " + std::to_string(f.round);
        return 1;
    }
    at += tr_pos;
    c.point = full_fs_point_;
    // ---- the sections behind it
    std::vector<F> input_0, fmsgs;
    c.fri_roots.resize(32 * ln);
    if (!bytes(c.root_h, 32) || !elems(input_0, 1) || !elems(c.all_sum, 65) || !elems(fmsgs, vph::FftGkrLayout((int) ln).n_msgs) || !bytes(c.fri_roots.data(), 32 * ln) ||
        !elems(c.final_code, 2048) || !elems(c.final_mask, 32))
        return bad("proof shorter than its sections");
    if (!canon) return bad("non-canonical field element in the proof");
    c.n_bytes = pcQueryAnswerBytes((int) n, reps);
    if (len - at != c.n_bytes) return bad("the proof does not end where the answer ends");
    c.answer = proof + at;
    c.claim = input_0[0];
    // ---- the chain behind the GKR part: the commitment head, fft_gkr's tape, the fold challenges, the positions
    vph::fs_chain ch = fs_state;
    ch.elem(c.claim.real, c.claim.img);
    for (int i = 0; i < 65; ++i) ch.elem(c.all_sum[i].real, c.all_sum[i].img);
    ch.digest(1, c.root_h);
    std::vector<F> ftape(vph::FftGkrLayout((int) ln).n_tape);
    vph::fftGkrFsTape((int) ln, ch, fmsgs.data(), ftape.data());
    c.fr.resize(ln);
    c.fr[0] = pcFsFirstChallenge(ch);
    for (u64 k = 0; k < ln; ++k) { F next; if (pcFsLevel(ch, (int) k, (int) ln, &c.fri_roots[32 * k], &next)) c.fr[k + 1] = next; }
    c.leaf0 = pcFsPositions(ch, (int) n, reps, c.final_code, c.final_mask, &work);
    // ---- the checks: the work, then nothing of the joined proof's own beyond the hand-over of the claim
    if (pcCheckWork(work.bits, work.nonce, work.met, min_pow_bits, why)) return 1;
    if (last_claim != c.claim) { gkrFails(GKR_INPUT, 0, -1); why = "the GKR part's claim on the input layer is not input_0 (final input check)"; return 1; }
    if (!vph::fft_gkr_check<F>((int) ln, ftape.data(), ftape.size(), fmsgs.data(), fmsgs.size(), F::getRootOfUnity((int) ln).inv())) { why = "fft_gkr is rejected"; return 1; }
    return pcVerifyCommitment(c, why, dev);
}

// checkFull with the verifier's heavy loops on `device`, on a prover context made for the call (circuit uploaded and evaluated: vp_liu_gr builds its table on an
// evaluated context; nothing is committed and no prover message is asked of it).  Throws when the context cannot be made.
bool checkFullOnDevice(const layeredCircuit &c, int device, const std::vector<uint8_t> &record) {
    prover dev(c, device);
    F::init();
    verifier v(nullptr, c);
    v.pred_dev = &dev; v.poly_dev = &dev;
    return v.checkFull(record);
}
