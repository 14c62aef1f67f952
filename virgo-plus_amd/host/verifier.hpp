// Host verifier: the caller the drop-in prover must satisfy (reference: src/verifier.h, src/verifier.cpp).
// It stays plain host C++ ("OUT OF SCOPE as a GPU target").  Two ways to run it:
//   verify()            interactive, exactly the reference's call sequence into `prover` (verifier.cpp:134-169):
//                       challenges are drawn with F::random() as the prover's messages arrive;
//   drawTape()+check()  the same checks replayed over a recorded transcript produced by
//                       prover::proveGKR from a pre-drawn tape (the challenges do not depend on the
//                       transcript: lib/virgo/src/fieldElement.cpp:119-124).
// Both record the prover's messages in the golden transcript layout (GKR slice).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "circuit.hpp"
#include "polynomial.hpp"
#include "prover.hpp"
#include "sha3.hpp"
#include "pc_fs.hpp"

// The first failed check of the GKR part (run, verifyPhase1, verifyPhase2, verifyLiu, checkInput and the hand-over of the claim to the commitment) in the calling
// thread's last run or replay: kind GKR_NONE when every check held (a malformed transcript is rejected without one).  round: -1 for a closing check.
enum GkrCheck { GKR_NONE = 0, GKR_PHASE1 = 1, GKR_PHASE2 = 2, GKR_SEMI_FINAL = 3, GKR_LIU = 4, GKR_LIU_SEMI_FINAL = 5, GKR_INPUT = 6 };
struct GkrFailure { int kind = GKR_NONE, layer = 0, round = -1; };
GkrFailure lastGkrFailure();
const char *gkrCheckName(int kind);

class verifier {
public:
    verifier(prover *pr, const layeredCircuit &cir);

    bool verify();                                              // interactive GKR (needs pr != nullptr)
    // The complete protocol of the reference's verifier::verify() (src/verifier.cpp:134-189): commit_private, GKR,
    // verifyPoly = commit_public + FRI commit phase + `reps` query repetitions (vpd_verifier.cpp:76-328; the
    // reference hard-codes 33).  fullTranscript() is then merkle_root_l | GKR | merkle_root_h | input_0 | all_sum[65].
    bool verifyFull(int reps = 33);
    // The same with the mask vectors of a hiding commitment: prover::commit_private(pri_mask), and prover::commit_public_eq(r_liu, pub_mask, ..) behind it.  The 65th
    // slice is then verified like the other 64 (verifyPoly; ms = the private mask's padded length, poly_commit.h:55-63) and an accepted run writes a version-2
    // record.  A null or all-zero private mask is verifyFull(reps): the reference's one-element zero mask, ms = 1.  Limits: prover.hpp, at commit_private(mask);
    // a mask the device refuses throws with the library's message.
    bool verifyFull(int reps, const std::vector<F> &pri_mask, const std::vector<F> &pub_mask);
    prover *pred_dev = nullptr;     // when set, the O(|C|) predicate loops run on the device (prover::predicates) instead of the host
    // when set, the commitment verifier's two heavy loops run on the device: the public polynomials' values at the query points
    // (prover::pcPublicEvals) and the digests of every opening (prover::pcOpeningDigests).  All positions are drawn first (the same draws), the
    // device returns values, and every comparison — leaf digest, root, fold consistency, final codeword — stays here.
    prover *poly_dev = nullptr;
    bool fri_batched = true;        // FRI commit phase as one device pass (prover::friCommit) instead of one friStep per challenge
    // The query phase as one device pass: all `reps` positions are drawn first (the loop draws nothing else between two positions, so they are the ones
    // the default path draws), prover::friQuery answers them in one call, the per-repetition checks then run unchanged over the answer.
    bool batched_openings = false;
    // Record of the last accepted verifyFull(): everything the prover handed over, in one block of bytes (layout: vphost.h), and its replay with NO
    // prover: the GKR part as check() does, then verifyPoly reading the prover's side from the record while every challenge and position is drawn
    // from the same seeded generator as the live run (call F::init() first, as for drawTape()).  A record that is short, long, of another version,
    // with a non-canonical element or with any byte changed is rejected.
    const std::vector<uint8_t> &fullRecord() const { return record_; }
    bool checkFull(const std::vector<uint8_t> &record);
    // version 1: the zero mask; version 2: one more section in front of the openings — u32 ms | u32 public mask length | the public mask | the final mask codeword [32]
    static constexpr uint32_t RECORD_MAGIC = 0x52465056u /* "VPFR" */, RECORD_VERSION = 1, RECORD_VERSION_MASKED = 2;
    const std::vector<uint8_t> &fullTranscript() const { return full_tr; }
    // FRI commit phase of the last verifyFull(): Merkle root per fold step (32 bytes each), final codeword (2048), fold challenges
    const std::vector<uint8_t> &friRoots() const { return fri_roots_; }
    const std::vector<F> &friFinalCode() const { return fri_final_; }
    const std::vector<F> &friChallenges() const { return fri_r_; }
    const std::vector<F> &friFinalMask() const { return fri_final_mask_; }      // the mask slice's last codeword (32; zeros for the zero mask)
    static int fftGkrDraws(int lg);
    double polyVerifyTime() const { return poly_timer.elapse_sec(); }
    // "Polynomial commitment: prove time" by the REFERENCE's definition (src/verifier.cpp:183): poly_prover.total_time = commit_private +
    // commit_public + commit_phase (lib/virgo/src/poly_commit.h:43,121,336,345, vpd_verifier.cpp:70) + fft_gkr's prover time (:92-94).
    // Answering the verifier's queries (fri::request_*) is outside that number in the reference and is reported separately here.
    double polyProveTime() const { return poly_prove_timer.elapse_sec(); }
    double polyOpenTime() const { return open_timer.elapse_sec(); }
    // where polyVerifyTime() goes: the public polynomials (interpolation + evaluation at the query points) and the opening digests (leaf chains +
    // Merkle paths), by whichever side computed them
    double publicEvalTime() const { return pub_eval_timer.elapse_sec(); }
    double openingDigestTime() const { return digest_timer.elapse_sec(); }
    // fft_gkr of the last verifyFull(): its share of polyProveTime() (the reference's p_time_fft, vpd_verifier.cpp:92-94) and its messages
    double fftGkrProveTime() const { return fft_gkr_timer.elapse_sec(); }
    const std::vector<F> &fftGkrMessages() const { return fft_gkr_msgs_; }
    // Fiat-Shamir mode (the reference's GKRProof.hpp / transcriptCache.hpp are dead code, so this is a separate
    // mode, not part of the bit-exact parity): every challenge is SHA3-256-derived from the circuit hash and ALL prover messages
    // sent before it, so the transcript is a non-interactive proof.  Differences from the interactive schedule: the challenges of
    // a sumcheck are drawn one per round (after that round's polynomial), not all up front.
    //   proveFS()   runs the prover (interactive entry points, one vp_round per derived challenge); transcript() is the proof;
    //   checkFS()   needs no prover and no tape: re-derives every challenge from the proof and runs the same checks.
    bool proveFS();
    // The same proof with the prover alone (vph_prove_fs_ex, VPH_FS_DEVICE_GKR): prover::proveGkrFS from the state behind fsInit() — the device draws every
    // challenge, one pass, no host round trip per challenge and no verifier sums.  transcript() is the proof, the same bytes as proveFS(); tape() holds the
    // draws in vp_prove_gkr's slots (not in draw order).  Nothing is verified here: checkFS is the check.  Returns the number of draws.
    u64 proveFSDevice();
    bool checkFS(const std::vector<uint8_t> &proof);
    // The joined non-interactive proof of the whole protocol (chain and layout: vphost.h, "The joined proof"): commit_private, the GKR part exactly as run() in
    // FS mode with the input check by commitment, commit_public_eq at the derived point, fft_gkr with its challenges drawn on the device (vp_fft_gkr_fs), the
    // FRI commit phase from the state it leaves (vp_fri_commit_fs), the final codewords, the derived positions and their openings.  Throws on a sharded session,
    // an input layer below 2^7 wires, or a prover whose own proof the checks reject.
    // device_gkr: the GKR part is prover::proveGkrFS from the head's state instead of run() (the point from the tape's r_liu slots of layer 1, the claim from the
    // transcript's last element); the same bytes, and the prover's own GKR proof is not verified here.
    // pow_bits (0 .. 32): the proof of work in front of the positions (prover::fsGrind on the device) and a version-2 proof; 0 is the version-1 proof, byte for byte.
    std::vector<uint8_t> proveFullFS(int reps, const std::vector<F> &pri_mask = {}, const std::vector<F> &pub_mask = {}, bool device_gkr = false, int pow_bits = 0);
    // A verifier that holds only the circuit: parses under checkFull's rules, replays run(), derives every challenge, calls fft_gkr_check and pcVerifyCommitment
    // unchanged (dev: the commitment's heavy loops on a device context).  0 = accepted, 1 = rejected (why: the failed check), -1 = malformed (why).
    // min_pow_bits: the work the verifier demands; a proof that carries less (a version-1 proof carries none) is rejected from its header, before the replay;
    // one whose work is not met, once the chain has reached W.
    int checkFullFS(const uint8_t *proof, u64 len, std::string &why, vp_ctx *dev = nullptr, int min_pow_bits = 0);
    u64 fullFsPowBits() const { return full_fs_pow_[0]; }       // the two fields of the last checkFullFS's header (0, 0: version 1, or malformed before them)
    u64 fullFsPowNonce() const { return full_fs_pow_[1]; }
    const std::vector<F> &fullFsPoint() const { return full_fs_point_; }      // the point the last proveFullFS / checkFullFS derived (checkFullFS: r_liu as far as the replay of the GKR part got)
    std::vector<F> drawTape();                                  // the verifier's draws, in its own order
    bool check(const std::vector<F> &tape, const std::vector<uint8_t> &transcript);   // replay

    const std::vector<uint8_t> &transcript() const { return tr; }
    const std::vector<F> &tape() const { return tape_; }
    const std::vector<F> &finalPoint() const { return r_liu; }     // r_liu after the last Liu sumcheck: where the input MLE is opened
    double verifyTime() const { return verify_timer.elapse_sec(); }
    bool skip_predicates = false;      // replay only: skip the O(|C|) wiring-predicate check (getFinalValue)

private:
    bool run();
    bool verifyPhase1(int layer_id, F &previousSum);
    bool verifyPhase2(int layer_id, F &previousSum);
    bool verifyLiu(int layer_id, F &previousSum);
    void predicatePhase1(int layer_id);
    void predicatePhase2(int layer_id);
    void predicatesOnDevice(int layer_id, bool with_phase2);
    F getFinalValue(int layer_id, const F &claim_u, const std::vector<F> &claim_v);
    bool checkInput(const F &claim);
    bool verifyPoly(const prover::hhash_digest &root_l, const F &claim, int reps);
    bool checkOpening(const vph::hhash_digest &root, u64 leaf, const std::vector<F> &vals, const std::vector<prover::hhash_digest> &path,
                      const uint8_t *device_digests = nullptr);

    F draw();
    quadratic_poly nextPoly(int phase, const F &prev);
    F nextF();
    void putF(const F &x);

    prover *p;
    const layeredCircuit &C;
    bool replay = false;
    bool fs = false;                                   // challenges derived from the transcript
    vph::fs_chain fs_state{};
    uint64_t fs_ctr = 0;
    void fsInit(bool with_inputs = true);
    void fullFsHead(int n, u64 reps, u64 ms, const std::vector<F> &pub_mask, const uint8_t root_l[32]);
    std::vector<F> full_fs_point_;
    u64 full_fs_pow_[2] = {0, 0};
    const std::vector<F> *rtape = nullptr;
    const std::vector<uint8_t> *rtr = nullptr;
    size_t tape_pos = 0, tr_pos = 0;
    std::vector<F> tape_;
    std::vector<uint8_t> tr;

    int max_bl = 0;
    std::vector<F> beta_g, beta_u, beta_v, r_u, r_liu, sig;
    std::vector<std::vector<F>> r_v;
    F coeff_l[(int) gateType::SIZE];
    std::vector<F> coeff_r[(int) gateType::SIZE];
    F bias, final_claim_u, assert_random;
    std::vector<std::vector<F>> final_claims_v;
    timer verify_timer, poly_timer, poly_prove_timer, fft_gkr_timer, open_timer, pub_eval_timer, digest_timer;
    std::vector<F> fft_gkr_msgs_;
    std::vector<uint8_t> full_tr;
    std::vector<uint8_t> fri_roots_; std::vector<F> fri_final_, fri_r_, fri_final_mask_;
    u64 mask_ms = 1;                                   // padded length of the run's mask; 1 = the zero mask (nothing of the prover is asked for slot 64)
    std::vector<F> pub_mask_;                          // the run's public mask (at most mask_ms elements)
    struct RecReader;                                  // bounds- and canonicity-checked cursor over a record (verifier.cpp)
    RecReader *rec = nullptr;                          // checkFull(): where verifyPoly reads the prover's side from
    std::vector<uint8_t> openings_, record_;           // the query phase's answers in vp_fri_query's layout; the whole record
    bool input_check_by_commitment = false;
    F last_claim;
};

// eq table (reference: src/utils.cpp:29-45), host version used by the verifier only
void initBetaTable(std::vector<F> &beta_g, int gLength, const std::vector<F>::const_iterator &r, const F &init);

// ---- the commitment verifier's two heavy loops, as functions that return values (verifier.cpp; verifyPoly calls them) ----
// n = bit length of the input layer (>= 7), N = 2^(n-6), M = 2^(n-1), w = the root of unity of order M.
// pcPublicCoefsHost: the interpolants q_j of the 64 slices of a public vector of 2^n entries, in coefficient form.
std::vector<std::vector<F>> pcPublicCoefsHost(int n, const std::vector<F> &pub);
// q0[j] = q_j(w^leaf), q1[j] = q_j(-w^leaf), j < 64, by Horner.
void pcPublicEvalsAt(const std::vector<std::vector<F>> &q_coef, int n, u64 leaf, F *q0, F *q1);
// Both for a list of leaves: out[(q 2 + 0) 64 + j] = q_j(w^leaf0[q]), out[(q 2 + 1) 64 + j] = q_j(-w^leaf0[q]) (vp_pc_public_evals' layout).
// pcPublicEvalsHost: the public vector is eq(point, .) (n coordinates); ...Pub: a general vector of 2^n entries; ...Tensor: eq(point, .) through
// q_j = eq(point[n-6 .. n), j) q_0' with q_0' the interpolant of eq(point[0 .. n-6), .) — one transform instead of 64, the same values.
std::vector<F> pcPublicEvalsHost(int n, const std::vector<F> &point, const std::vector<u64> &leaf0);
std::vector<F> pcPublicEvalsHostPub(int n, const std::vector<F> &pub, const std::vector<u64> &leaf0);
std::vector<F> pcPublicEvalsHostTensor(int n, const std::vector<F> &point, const std::vector<u64> &leaf0);
// Bytes of vp_fri_query's answer to n_queries positions at input bit length n, and the (oracle, leaf) of every opening in its order.
u64 pcQueryAnswerBytes(int n, u64 n_queries);
// One opening: the leaf-chain digest of its 130 values (65 blocks from the zero state) and the root reached from it through path[0 .. depth).
void pcOpeningDigest(u64 leaf, const uint8_t *values /* 2080 bytes */, const uint8_t *path /* depth x 32 */, size_t depth, uint8_t out[64]);
// All openings of an answer block in vp_fri_query's layout: 64 bytes each (leaf digest | root), in the layout's order.  Bytes are hashed as given.
// Throws std::runtime_error when n_bytes is not the layout's size.
std::vector<uint8_t> pcOpeningDigestsHost(int n, const std::vector<u64> &leaf0, const uint8_t *answer, u64 n_bytes);

// ---- the mask slice (slot 64) --------------------------------------------------------------------------------------------------------------------
// The public mask polynomial: the interpolant of the public mask, zero-padded to ms (a power of two), on the ms-th roots of unity (vpd_verifier.cpp:82-87), in
// coefficient form; and its values at the query points, out[2 q + h] = q_msk((-1)^h w^leaf0[q]) (vp_pc_mask_evals' layout).  ms = 1 with one zero: q_msk = 0.
std::vector<F> pcMaskCoefsHost(const std::vector<F> &pub_mask, u64 ms);
std::vector<F> pcMaskEvalsHost(int n, const std::vector<F> &pub_mask, u64 ms, const std::vector<u64> &leaf0);

// ---- the commitment's verifier by value: everything verifyPoly checks after fft_gkr, on arrays -------------------------------------------------------
struct PcCommitment {
    int n = 0;                                   // bit length of the committed vector (>= 7)
    std::vector<F> point, pub;                   // exactly one: n coordinates (the public vector is eq(point, .)) or 2^n entries
    std::vector<F> pub_mask; u64 ms = 1;         // at most ms elements; ms = 1 (the zero mask) or a power of two in [8, min(2^16, 2^(n-2))]
    F claim;
    uint8_t root_l[32], root_h[32];
    std::vector<F> all_sum;                      // 65
    std::vector<F> fr;                           // n - 6 fold challenges
    std::vector<uint8_t> fri_roots;              // 32 (n - 6)
    std::vector<F> final_code, final_mask;       // 2048, 32
    std::vector<u64> leaf0;                      // one per repetition, in [2^(n-7), 2^(n-2))
    const uint8_t *answer = nullptr; u64 n_bytes = 0;      // vp_fri_query's layout for (n, leaf0.size())
    u64 pow_bits = 0, pow_nonce = 0;             // a non-interactive proof's work (0: none, version 1) and whether W(pow_bits, pow_nonce) met it; pcVerifyCommitment
    bool pow_met = true;                         // does not read them: pcCheckWork decides
};
// The proof of work of a parsed non-interactive proof against the verifier's demand: 0, or 1 with the reason (the work is not met; fewer bits than demanded).
int pcCheckWork(u64 pow_bits, u64 pow_nonce, bool met, int min_pow_bits, std::string &why);
// 0 = accepted, 1 = rejected (why: the failed check), -1 = malformed (why).  dev: a device context for the heavy loops (vp_pc_public_evals, vp_pc_mask_evals,
// vp_fri_query_digests), or null for the host's; a device call that fails throws std::runtime_error.
int pcVerifyCommitment(const PcCommitment &c, std::string &why, vp_ctx *dev = nullptr);

// ---- the non-interactive commitment proof (layout and chain: vphost.h) ---------------------------------------------------------------------------------
// Parses a proof under checkFull's rules (bounds on every read, canonical limbs, the proof ends where the answer ends; ms and n_pub by vph_verify_commitment's
// rules) and derives fr and leaf0 from the chain: c is ready for pcVerifyCommitment, its answer pointing into `proof`.  0, or -1 with the reason.
int pcParseCommitmentFS(const uint8_t *proof, u64 len, PcCommitment &c, std::string &why);
// Parse, derive, pcVerifyCommitment unchanged: no algebra of its own.  0 = accepted, 1 = rejected (why: the failed check), -1 = malformed (why).
int pcVerifyCommitmentFS(const uint8_t *proof, u64 len, std::string &why, vp_ctx *dev = nullptr, int min_pow_bits = 0);

// verifier::checkFull (after F::init()) with pred_dev and poly_dev on a context made for the call on `device`; throws std::runtime_error without a usable device
bool checkFullOnDevice(const layeredCircuit &c, int device, const std::vector<uint8_t> &record);
