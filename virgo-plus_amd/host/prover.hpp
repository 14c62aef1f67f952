// Host mirror of the reference's `class prover` (src/prover.h:12-66): same method names, argument
// meaning and call-order contract, so the verifier below (and the reference's own verifier.cpp, see
// INTEGRATION.md) can drive it unchanged.  Every sumcheck method forwards to the C ABI of
// libvpgpu.so (include/vpgpu.h); no arithmetic on tables happens on the host and there is no CPU
// fallback: construction throws if the device library cannot run.
#pragma once
#include <array>
#include <chrono>
#include <functional>
#include <memory>
#include <stdexcept>
#include <vector>

#include "../../include/vpgpu.h"
#include "circuit.hpp"
#include "polynomial.hpp"
#include "sha3.hpp"

class timer {          // accumulate semantics of lib/virgo/src/timer.hpp:11-25
public:
    void start() { t0 = std::chrono::high_resolution_clock::now(); }
    void stop() { total += std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count(); }
    void clear() { total = 0; }
    void add(double sec) { total += sec; }       // a span measured elsewhere (the GKR part of a protocol pass, in device time when its completion is deferred)
    double elapse_sec() const { return total; }
private:
    std::chrono::high_resolution_clock::time_point t0;
    double total = 0;
};

class prover {
public:
    explicit prover(const layeredCircuit &cir, int device = 0, const vp_options *options = nullptr);   // options: include/vpgpu.h (NULL = shipped defaults)
    // One proof's interactive sumchecks sharded by index over W = devices.size() ranks (vp_set_round_shard, min_log): one context per rank, the same
    // device may be listed several times.  Every sumcheck method runs on all ranks at once (one worker thread per rank), sums the partial round
    // polynomials mod p, performs the gather when a rank stops at it, and checks that the ranks' claims agree.  Vres's message is rank 0's.
    // shard_commitment = false: the commitment runs on rank 0.  true: it is sharded over the same ranks (vp_pc_set_shard) — commit_private, commit_public,
    // commit_public_eq, friStep, friCommit, friFinal and the openings run on every rank through the same worker pool; when all ranks stop at a collective
    // (VP_EXCHANGE) it is performed by vp_shard_exchange_local and the call repeated; roots, input_0 and all_sum must agree across the ranks; friOpen asks
    // the owner of the leaf, friOpenMany and friQuery merge the ranks' answers (friQuery after friCommit: through friOpenMany, since vp_fri_query on a shard
    // serves the step-wise phase only).  Masks are refused on a sharded commitment.  A request that cannot be met
    // (fewer than 2 W positions per slice) throws here with the reason: there is no silent fall-back to rank 0.
    prover(const layeredCircuit &cir, const std::vector<int> &devices, int min_log, const vp_options *options = nullptr, bool shard_commitment = false);
    ~prover();
    prover(const prover &) = delete;
    prover &operator=(const prover &) = delete;

    void evaluate();
    void init();
    void sumcheckInitAll(const std::vector<F>::const_iterator &r_last);
    void sumcheckInit();
    void sumcheckInitPhase1(const F &assert_random);
    void sumcheckInitPhase2();
    void sumcheckInitLiu(std::vector<F>::const_iterator s);

    quadratic_poly sumcheckUpdatePhase1(const F &previousRandom);
    quadratic_poly sumcheckUpdatePhase2(const F &previousRandom);
    quadratic_poly sumcheckLiuUpdate(const F &previousRandom);

    void sumcheckFinalize1(const F &previousRandom, F &claim);
    void sumcheckFinalize2(const F &previousRandom, std::vector<F>::iterator claims);
    void sumcheckLiuFinalize(const F &previousRandom, F &claim);

    F Vres(const std::vector<F>::const_iterator &r_0, int r_0_size);

    // Virgo polynomial commitment (reference: `#ifdef USE_VIRGO` block of src/prover.h:38-43)
    struct hhash_digest { unsigned char b[32]; };
    hhash_digest commit_private();                       // src/prover.cpp:524-530
    // src/prover.cpp:542-546 (the mask argument of the reference is the one-element zero vector and is implied)
    hhash_digest commit_public(std::vector<F> &pub, F &inner_product_sum, std::vector<F> &all_sum);
    // the same two with the mask vectors lib/virgo's commit_private_array / commit_public_array take (poly_commit.h:41-42,126-128; the reference's own
    // prover passes one zero, src/prover.cpp:526, and its commit_public has this signature, src/prover.cpp:542): a non-zero private mask puts content into the
    // 65th slice of every oracle (vp_commit_private_masked / vp_commit_public_masked); an all-zero one is the call above
    // Limits (include/vpgpu.h): the private mask pads to ms = M / gap, M = 2^(n-1), gap = the largest power of two <= M / its length; 8 <= ms <= min(2^16, M / 2);
    // the public mask has at most ms elements; not on a sharded commitment.  The library's refusal is the exception's message.  The verifier (verifier.hpp)
    // accepts such a commitment when ms <= 2^(n-6), a slice's message length, and rejects a longer mask at the final mask codeword, as the reference's does.
    hhash_digest commit_private(const std::vector<F> &mask);
    hhash_digest commit_public(std::vector<F> &pub, F &inner_product_sum, std::vector<F> &mask, std::vector<F> &all_sum);
    std::vector<F> friFinalMask();                       // fri::cpd.rs_codeword_msk[last] (vpd_verifier.cpp:321-325)
    // extension: the protocol's own public vector, pub = eq(point, .) (src/verifier.cpp:368-369), built on the device from the point
    // (vp_commit_public_eq) — same outputs as commit_public on that table, nothing of it crosses PCIe
    hhash_digest commit_public_eq(const std::vector<F> &point, F &inner_product_sum, std::vector<F> &all_sum);
    // the same behind commit_private(mask) with the public mask vector (vp_commit_public_eq_masked); behind a zero private mask it is the call above
    hhash_digest commit_public_eq(const std::vector<F> &point, const std::vector<F> &mask, F &inner_product_sum, std::vector<F> &all_sum);
    void setMasked(bool m) { masked = m; }               // vph_prove_protocol_masked commits through the C ABI itself (its roots are written late)
    bool isMasked() const { return masked; }
    // poly_commit_prover::commit_phase pieces (vpd_verifier.cpp:44-74 -> fri::commit_phase_step / commit_phase_final)
    // verifier-side wiring predicates of one layer on the device (vp_predicates): 5 + 7*layer sums, see include/vpgpu.h
    std::vector<F> predicates(int layer, const std::vector<F> &r_g, const F &assert_random, const std::vector<F> &r_u,
                              const std::vector<F> &r_v, int n_v);
    // the verifier's other O(|C|) loops on the device: gr of verifyLiu (vp_liu_gr) and a layer's MLE at r (vp_layer_mle)
    F liuGr(int layer, const std::vector<F> &r_u, const std::vector<std::vector<F>> &r_v, const std::vector<F> &sig, const std::vector<F> &r_liu);
    F layerMle(int layer, const std::vector<F> &r, int n);
    // the commitment verifier's two heavy loops on the device (vp_pc_public_evals with the point form / with a general vector, vp_fri_query_digests):
    // they read public data only — no witness, no committed oracle — and return values; the verifier compares
    std::vector<F> pcPublicEvals(int n, const std::vector<F> &point, const std::vector<u64> &leaf0);
    std::vector<F> pcPublicEvalsPub(int n, const std::vector<F> &pub, const std::vector<u64> &leaf0);
    std::vector<uint8_t> pcOpeningDigests(int n, const std::vector<u64> &leaf0, const uint8_t *answer, u64 n_bytes);
    // the mask row of pcPublicEvals (vp_pc_mask_evals): out[2 q + h] = the public mask polynomial — the interpolant of pub_mask, zero-padded to ms, on the ms-th
    // roots — at (-1)^h w^leaf0[q].  Limits: ms a power of two in [8, min(2^16, 2^(n-2))], 1 .. ms mask elements (the library refuses anything else)
    std::vector<F> pcMaskEvals(int n, const std::vector<F> &pub_mask, u64 ms, const std::vector<u64> &leaf0);
    // with a launch log on (vph_set_profiling), every verifier-side device call above — predicates, liuGr, layerMle, pcPublicEvals(Pub), pcMaskEvals,
    // pcOpeningDigests — appends the launch table of its call (vp_get_launch_stats), so that a whole verification can be read afterwards
    void setLaunchLog(bool on) { log_launches = on; verifier_launches_.clear(); }
    void clearLaunchLog() { verifier_launches_.clear(); }
    const std::vector<vp_launch_stat> &verifierLaunches() const { return verifier_launches_; }
    // The non-interactive commitment proof (layout and chain: vphost.h): commit_private(pri_mask), commit_public_eq(point[, pub_mask]), the FRI commit phase with
    // every fold challenge drawn from the transcript, the final codewords, the positions drawn from the chain, and their openings (vp_fri_query) — one block
    // of bytes that pcVerifyCommitmentFS checks with no tape and no session.  device_draws: the commit phase is vp_fri_commit_fs, the device drawing each
    // challenge from the root it has just computed (checked here against the host's chain over the returned roots); false: the vp_fri_step loop with the chain on
    // the host, one wait per level — a second implementation with the same bytes.  Throws on a sharded commitment (not built).
    // pow_bits (0 .. 32): the proof of work in front of the positions and a version-2 proof; 0 is the version-1 proof, byte for byte.  The nonce is fsGrind's,
    // on the device with device_draws and on the host without.
    std::vector<uint8_t> commitFS(const std::vector<F> &point, int reps, const std::vector<F> &pri_mask = {}, const std::vector<F> &pub_mask = {}, bool device_draws = true,
                                  int pow_bits = 0);
    // The smallest nonce whose W(bits, nonce) on `state` meets the work, searched from 0 through 64 x 2^bits tries: vp_fs_grind on the context (on_device) or
    // the host's search.  Throws std::invalid_argument for bits outside 1 .. 32 and std::runtime_error when the range holds no such nonce.
    u64 fsGrind(const vph::hhash_digest &state, int bits, bool on_device);
    // vp_fri_commit_fs from the chain's state, the roots returned; the device's challenges and closing state are checked against the chain walked over those
    // roots (steps 8 and 9 of the commitment's chain), which is left behind the last level.  After commit_public_eq.
    void friCommitFS(vph::fs_chain &ch, std::vector<uint8_t> &roots);
    double fsPhaseSec() const { return fs_phase_sec; }      // host wall clock of the last commitFS's commit phase (step 5 alone)
    double fsPhaseDeviceMs() const { return fs_phase_ms; }  // its device time (the levels' sum in the vp_fri_step loop)
    hhash_digest friStep(const F &r);
    std::vector<hhash_digest> friCommit(const std::vector<F> &r);   // every step in one device pass (challenges are transcript-independent)
    std::vector<F> friFinal();                           // 2048 elements, reference layout [i << 7 | slice << 1 | hi]
    // fri::request_init_value_with_merkle (oracle 0 = l, 1 = h) / fri::request_step_commit (oracle 2 + level)
    void friOpen(int oracle, u64 leaf, std::vector<F> &values /* 130 */, std::vector<hhash_digest> &path);
    // the same for a list of requests in one device pass (vp_fri_open_many): values n x 130, paths at a stride of `stride` digests, path_len per request
    void friOpenMany(const std::vector<int32_t> &oracle, const std::vector<u64> &leaf, std::vector<F> &values, std::vector<hhash_digest> &paths, int stride,
                     std::vector<int32_t> &path_len);
    // the whole query phase (vp_fri_query): leaf0[q] = the leaf of l and h of repetition q; per repetition oracle 0, oracle 1, level 0 .. ln - 1, each the
    // 130 values followed by the path at its true length
    std::vector<uint8_t> friQuery(const std::vector<u64> &leaf0);
    // fft_circuit_gkr::fft_gkr (lib/virgo/src/fft_circuit_GKR.cpp:833-849), prover side on the device (vp_fft_gkr): tape = the verifier's
    // draws in the reference's order; returns every prover message (layouts: include/vpgpu.h)
    std::vector<F> fftGkr(int lg, const std::vector<F> &tape);
    // the same in two halves (vp_fft_gkr_begin / _end): queued on a stream of its own, collected later; other prover calls may run in between
    void fftGkrBegin(int lg, const std::vector<F> &tape);
    std::vector<F> fftGkrEnd(int lg);
    void fftGkrCancel() noexcept;                   // drop a begun run (a pass that failed between begin and end)
    // fft_gkr non-interactive (vp_fft_gkr_fs): the device draws the whole tape from the chain, starting at `state` (the chain's text: vphost.h); returns the
    // messages, `tape` = the tape drawn, `state` = the closing state.  The tape and the state are re-derived here from the returned messages
    // (fft_gkr_fs.hpp); throws if either differs from what the device returned.
    std::vector<F> fftGkrFS(int lg, uint8_t state[32], std::vector<F> &tape);
    // The GKR part non-interactive (vp_prove_gkr_fs): Vres and every sumcheck with the device drawing each challenge from the chain that starts at `state`
    // (the schedule: vphost.h, "The GKR part on the device").  Returns the transcript (vp_prove_gkr's layout), `tape` = the draws in vp_prove_gkr's slots,
    // `state` = the closing state, and the number of draws.  Tape, count and state are re-derived here from the returned transcript (gkr_fs.hpp: a walk over
    // the bytes, no verifier sums); throws if any differs from what the device returned.  Throws on a sharded prover (not built).
    std::vector<uint8_t> proveGkrFS(uint8_t state[32], std::vector<F> &tape, u64 &n_draws);
    double commitDeviceMs();

    double proveTime() const { return prove_timer.elapse_sec(); }
    void addProveTime(double sec) { prove_timer.add(sec); }     // vph_prove_protocol_ex calls vp_prove_gkr itself: its GKR span belongs to Prove Time (src/verifier.cpp:177-184)
    // where Prove Time goes on the interactive path: phase inits | round messages | finalize calls | Vres (all inside prove_timer's spans,
    // except sumcheckLiuFinalize, which the reference leaves out of its timer as well)
    double initTime() const { return init_timer.elapse_sec(); }
    double roundTime() const { return round_timer.elapse_sec(); }
    double finalizeTime() const { return fin_timer.elapse_sec(); }
    double proofSize() const { return (double) proof_size / 1024.0; }

    // ---- extensions (not in the reference) ----
    // Whole GKR part in one device pass; tape = the verifier's draws in its own order
    // (layout in include/vpgpu.h).  Appends the messages to `transcript`.
    void proveGKR(const std::vector<F> &tape, std::vector<uint8_t> &transcript);
    void gkrSizes(u64 &n_tape, u64 &n_transcript_bytes);
    std::vector<F> layerValues(int layer);
    vp_ctx *context() { return ctx; }
    int world() const { return (int) rk.size(); }
    bool commitmentSharded() const { return shard_pc; }
    vp_ctx *rankContext(int r) { return (r >= 0 && r < (int) rk.size()) ? rk[r] : nullptr; }
    // round-sharded prover: every rank's partial polynomial of every round since the last clearPartials (test and profiling aid), and a rank whose
    // partial is left out of the sum (-1: none; a test of the verifier's sumcheck check)
    const std::vector<std::array<F, 3>> &partials() const { return part_log; }
    void clearPartials() { part_log.clear(); }
    void setDropRank(int r) { drop_rank = r; }
    double gatherTime() const { return gather_timer.elapse_sec(); }
    vp_stats stats();

private:
    quadratic_poly sumcheckUpdate(const F &previous_random, std::vector<F> &r_arr);
    void check(int rc, const char *what);
    void upload(const std::vector<int> &devices, const vp_options *options);
    // run fn(rank, context) on every rank concurrently and throw on the first failure (VP_EXCHANGE is returned to the caller when every rank stopped there)
    int onRanks(const std::function<int(int, vp_ctx *)> &fn, const char *what);
    void finalizeAll(const F &previousRandom, F *claims, int n, const char *what);
    // a call of the sharded commitment on every rank, repeated after each collective the ranks stop at
    void pcRanks(const std::function<int(int, vp_ctx *)> &fn, const char *what);
    bool shard_pc = false;
    bool fri_one_pass = false;                           // the standing FRI phase came from friCommit: vp_fri_query is not answered on a shard then, friQuery merges friOpenMany
    struct Pool;
    std::unique_ptr<Pool> pool;
    std::vector<vp_ctx *> rk;                            // every rank's context (rk[0] == ctx)
    std::vector<std::array<F, 3>> part_log;
    int drop_rank = -1;
    timer gather_timer;

    const layeredCircuit &C;
    vp_ctx *ctx = nullptr;
    std::vector<F> r_u, r_liu;
    std::vector<std::vector<F>> r_v;
    int round = 0;
    int sumcheckLayerId = 0;
    timer prove_timer, init_timer, round_timer, fin_timer;
    void logLaunches();
    bool log_launches = false;
    std::vector<vp_launch_stat> verifier_launches_;
    bool masked = false;                                 // the standing private commitment carries a non-zero mask slice
    u64 proof_size = 0;
    double fs_phase_sec = 0, fs_phase_ms = 0;
};
