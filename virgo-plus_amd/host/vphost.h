/* vphost.h — C entry points of libvphost.so for the Python harness (tests/, bench.py) and other FFI
 * users: circuit loading, one prover session per GPU, interactive and batched GKR proofs.  Everything
 * here is host orchestration; the arithmetic runs in libvpgpu.so (include/vpgpu.h).                  */
#ifndef VPHOST_H
#define VPHOST_H
#include <stdint.h>
#include "../../include/vpgpu.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vph_circuit vph_circuit;
typedef struct vph_session vph_session;

typedef struct {
    double prove_sec;        /* reference "Prove Time" definition: host wall clock over the prover-method spans */
    double gkr_device_ms;    /* hipEvent time of the batched device pass (0 for interactive)                   */
    double evaluate_ms;      /* device time of circuit evaluation                                              */
    double verify_sec;       /* host verifier time                                                             */
    double fold_ms;          /* profiled dominant-kernel launches: total duration ...                          */
    uint64_t fold_launches;  /* ... count ...                                                                  */
    uint64_t fold_bytes;     /* ... and algorithmic bytes                                      */
    uint64_t rounds;
    uint64_t launches;
    double proof_kb;
    int verified;
} vph_result;

/* seed < 0: keep the process's current glibc random() state (default seed 1 in a fresh process);
 * else srandom(seed) before the witness is drawn (src/main.cpp:188).                                 */
vph_circuit *vph_circuit_from_pws(const char *path, int blocks, long seed, char *err, int errlen);
vph_circuit *vph_circuit_randomize(int layers, int log_size, long seed);
/* Arbitrary layered circuit from flat arrays (all gate types of enum gateType, constants, assert gates); subsetInit runs. */
vph_circuit *vph_circuit_custom(int n_layers, const uint64_t *layer_sizes, const int32_t *ty, const int32_t *l, const uint64_t *u,
                                const uint64_t *v, const uint64_t *c_pairs, const uint8_t *is_assert);
void vph_circuit_free(vph_circuit *);
int vph_circuit_layers(const vph_circuit *);
uint64_t vph_circuit_gates(const vph_circuit *);
uint64_t vph_circuit_layer_size(const vph_circuit *, int layer);
int vph_circuit_layer_bitlen(const vph_circuit *, int layer);
void vph_circuit_hash(const vph_circuit *, uint64_t out[2]);

/* Uploads the circuit to `device` and evaluates it there.  NULL + message on failure (no CPU fallback). */
vph_session *vph_session_create(vph_circuit *, int device, char *err, int errlen);
vph_session *vph_session_create_opts(vph_circuit *, int device, const vp_options *opt /* include/vpgpu.h, NULL = defaults */, char *err, int errlen);
void vph_session_free(vph_session *);
int vph_set_profiling(vph_session *, int level);
/* With profiling on, the launch tables (vp_get_launch_stats) of the VERIFIER-side device calls of the last vph_prove_and_verify_full(_ex) — vp_predicates, vp_liu_gr,
 * vp_layer_mle, vp_pc_public_evals, vp_pc_mask_evals (a masked run), vp_fri_query_digests — one after the other, in call order; every verification (verifier::run) starts the log anew, and
 * vph_set_profiling switches it on and off with the launch tables it reads.  Returns the number of entries (copies up to `capacity`). */
int vph_verifier_launches(vph_session *, vp_launch_stat *out, int capacity);
/* the vp_ctx behind the session's prover (for the measurement calls of include/vpgpu.h: vp_get_launch_stats, ...) */
void *vph_session_ctx(vph_session *);
/* A session whose interactive sumchecks are sharded by index over world = 1, 2, 4 or 8 ranks (vp_set_round_shard, min_log): one context per entry
 * of `devices` (the same device may repeat).  vph_prove_interactive, vph_prove_full and vph_prove_and_verify_full work on it unchanged; the prover
 * sums the ranks' partial round polynomials.  vph_session_ctx is rank 0's context, vph_session_rank_ctx(s, r) rank r's (per-rank stats). */
vph_session *vph_session_create_round_sharded(vph_circuit *, const int *devices, int world, int min_log, const vp_options *opt, char *err, int errlen);
/* The same with a switch for the commitment: shard_commitment = 0 is vph_session_create_round_sharded; non-zero also shards the Virgo commitment
 * over the ranks (vp_pc_set_shard), so that vph_commit_private / vph_commit_public, vph_fri_commit(_batched), vph_prove_full and
 * vph_prove_and_verify_full run commit_private, commit_public, the FRI commit phase and every opening on all ranks (collectives among the
 * contexts by vp_shard_exchange_local).  Fails with the reason when the input layer is too short for the ranks (2^(n-6) < 2 world): there
 * is no fall-back to rank 0.  Masks and the one-pass vph_prove_protocol are not available on such a session.                                  */
vph_session *vph_session_create_sharded(vph_circuit *, const int *devices, int world, int min_log, int shard_commitment, const vp_options *opt,
                                        char *err, int errlen);
void *vph_session_rank_ctx(vph_session *, int rank);
int vph_session_world(vph_session *);
/* round-sharded session: every rank's partial polynomial of every round since the last clear (rank-major per round, 3 elements each; returns the
 * number of entries = rounds x world), a rank whose partial the prover leaves out of the sum (-1: none), host seconds spent in the gathers */
int vph_session_partials(vph_session *, vp_F *out, int capacity);
void vph_session_clear_partials(vph_session *);
void vph_session_drop_rank(vph_session *, int rank);
double vph_session_gather_sec(vph_session *);
/* circuitValue[layer] copied back (tests).                                                             */
int vph_layer_values(vph_session *, int layer, uint64_t *out_pairs, uint64_t n);

/* F::init() (srand(3396)) + verifier::verify(): one device round trip per sumcheck round.              */
int vph_prove_interactive(vph_session *, uint8_t *transcript, uint64_t capacity, uint64_t *n_written,
                          vph_result *res, char *err, int errlen);
/* F::init() + draw the verifier tape once; it stays attached to the session.                           */
int vph_draw_tape(vph_session *);
/* Attach the caller's tape in place of vph_draw_tape's: n elements of {real, img} in the draw order of verifier::drawTape() (the layout of
 * vp_prove_gkr's tape, include/vpgpu.h).  -1, and the attached tape stays as it was, when n is not the circuit's draw count or a limb is >= 2^61 - 1.
 * vph_prove_gkr, vph_check, vph_shard_vu_partials and the sharded proofs of vph_set_shard then run on it.                                             */
int vph_set_tape(vph_session *, const uint64_t *tape_pairs, uint64_t n);
/* One batched GKR proof from the attached tape (a bench "step").                                       */
int vph_prove_gkr(vph_session *, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, vph_result *res,
                  char *err, int errlen);
/* Host verifier replay over a transcript made from the attached tape.  skip_predicates=1 skips the
 * O(|C|) wiring-predicate sums (the sumcheck and Liu checks still run).                                */
int vph_check(vph_session *, const uint8_t *transcript, uint64_t n, int skip_predicates, double *verify_sec);
uint64_t vph_transcript_bytes(vph_session *);
/* prover::commit_private(): Merkle root of the RS-encoded input layer (merkle_root_l); device ms via *ms. */
int vph_commit_private(vph_session *, uint8_t root[32], double *ms, char *err, int errlen);
/* prover::commit_public on a caller-supplied public vector of 2^bit_length(layer 0) elements ({real,img} pairs).
 * out = root_h[32] | input_0[16] | all_sum[65*16]  (the tail of the golden transcript layout).         */
int vph_commit_public(vph_session *, const uint64_t *pub_pairs, uint64_t n_pub, uint8_t out[32 + 16 + 65 * 16], double *ms,
                      char *err, int errlen);
/* The COMPLETE protocol with polynomial-commitment verification (verifier::verify, src/verifier.cpp:134-189):
 * commit_private, interactive GKR, commit_public, FRI commit phase with fresh challenges, `reps` query repetitions
 * answered through vp_fri_open and checked on the host.  Returns 0 = accepted, 1 = rejected.  transcript = the golden
 * layout (identical to the reference's up to all_sum); times in seconds.                                  */
int vph_prove_and_verify_full(vph_session *, int reps, uint8_t *transcript, uint64_t capacity, uint64_t *n_written,
                              double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec, char *err, int errlen);
/* The same with flags.  VPH_VERIFY_BATCHED_OPENINGS: the verifier draws all `reps` query positions first and the prover answers them in ONE device
 * pass (vp_fri_query) instead of 2 + (n - 6) vp_fri_open calls per repetition; same positions, same openings, same checks.                     */
/* VPH_VERIFY_DEVICE_LOOPS: the verifier's heavy loops run on the session's device — the wiring predicates (vp_predicates, vp_liu_gr), the public polynomials'
 * values at the query points (vp_pc_public_evals) and the digests of every opening (vp_fri_query_digests).  Implies positions-first; the device returns values and
 * every comparison stays on the host: transcript, record and verdict are those of the host mode.                                                        */
enum { VPH_VERIFY_BATCHED_OPENINGS = 1, VPH_VERIFY_DEVICE_LOOPS = 2 };
int vph_prove_and_verify_full_ex(vph_session *, int reps, int flags, uint8_t *transcript, uint64_t capacity, uint64_t *n_written,
                                 double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec, char *err, int errlen);
/* The same with the mask vectors of a hiding commitment (flags as _ex): prover::commit_private(pri_mask), commit_public_eq(r_liu, pub_mask; null or n_pub = 0: one
 * zero) behind it, and the verifier checks the 65th slice like the other 64 — the public mask polynomial at the query points, the slice's virtual oracle, its fold
 * consistency on every level, its final codeword (vp_fri_final_mask) constant and equal to the last level's pair.  As the reference's verifier, it accepts a mask
 * that pads to at most 2^(n-6) elements and rejects a longer one at the final mask codeword.  With VPH_VERIFY_DEVICE_LOOPS the mask polynomial's values come from
 * vp_pc_mask_evals.  A null or all-zero private mask is vph_prove_and_verify_full_ex, byte for byte.  A mask the device refuses (lengths: include/vpgpu.h; a sharded
 * commitment) is -2 with the library's message, not a verdict.  An accepted masked run leaves a version-2 record.                                              */
int vph_prove_and_verify_full_masked(vph_session *, int reps, int flags, const uint64_t *pri_mask_pairs, uint64_t n_pri, const uint64_t *pub_mask_pairs, uint64_t n_pub,
                                     uint8_t *transcript, uint64_t capacity, uint64_t *n_written, double *gkr_prove_sec, double *pc_prove_sec, double *verify_sec,
                                     char *err, int errlen);
/* Record of the last ACCEPTED vph_prove_and_verify_full(_ex, _masked) of the session: everything the prover handed over, so that the whole verifier can run
 * again later without a GPU.  All integers little-endian, field elements as {real, img} u64 pairs (canonical), n = bit length of the input layer:
 *     header       16 bytes   u32 magic 0x52465056 ("VPFR") | u32 version = 1, or 2 for a masked run | u32 n | u32 reps (1 .. 4096)
 *     transcript              merkle_root_l[32] | GKR slice | merkle_root_h[32] | input_0[16] | all_sum[65 x 16]      (the golden layout)
 *     fft_gkr      16 x (64 + 3 (2 lg^2 + 2 lg + 6) + 2 + 2 lg) bytes, lg = n - 6                                     (vp_fft_gkr's message layout)
 *     FRI roots    32 x (n - 6) bytes
 *     final code   2048 x 16 bytes                                                                                    (vp_fri_final's layout)
 *     mask         VERSION 2 ONLY: u32 ms (the private mask's padded length, a power of two in [8, min(2^16, 2^(n-2))]) | u32 n_pub (1 .. ms) | the public
 *                  mask, n_pub x 16 bytes | the final mask codeword, 32 x 16 bytes                                    (vp_fri_final_mask's layout)
 *     openings   vp_fri_query's bytes for the `reps` positions the verifier drew: per repetition oracle 0, oracle 1, level 0 .. n - 7, each
 *                  130 values (2080 bytes) + its path at the true length (n - 1 digests for l and h, n - 2 - k for level k)
 * vph_last_full_record: copies it to buf (*n = its size; -1 if there is none or cap is too small, *n still set).
 * vph_verify_full_record: no GPU, no session.  F::init(), then verifier::checkFull: the GKR part as vph_verify_transcript, then the commitment's
 * verifier reading the record while it draws every challenge and query position from the same seeded generator as the live run.  0 = accepted,
 * 1 = rejected (also: short, long, another version, a non-canonical element, any byte changed).                                               */
int vph_last_full_record(vph_session *, uint8_t *buf, uint64_t cap, uint64_t *n);
int vph_verify_full_record(vph_circuit *, const uint8_t *record, uint64_t n);
/* The same replay with the verifier's heavy loops on `device` (VPH_VERIFY_DEVICE_LOOPS), on a context created for the call: the circuit is uploaded and
 * evaluated there (vp_liu_gr builds its table on an evaluated context); nothing is committed on it and no prover message is asked of it.  0 = accepted,
 * 1 = rejected (a device call that fails during the replay rejects, like every other exception of the replay), -2 = the context could not be made (err). */
int vph_verify_full_record_dev(vph_circuit *, int device, const uint8_t *record, uint64_t n, char *err, int errlen);
/* Where the verifier's time of the last vph_prove_and_verify_full(_ex) went, in seconds: [0] the GKR verifier's O(|C|) loops — wiring predicates, the final value
 * they give, Liu gr (verifier::verifyTime; the sumcheck round checks are not timed anywhere), [1] public polynomials (interpolation + evaluation at the query
 * points), [2] opening digests (leaf chains + Merkle paths), [3] the rest of the commitment's verifier. */
void vph_last_verify_split(vph_session *, double out[4]);
/* The commitment verifier's two heavy loops by value, on the host (no GPU, no session): the functions verifier::verifyPoly itself calls.
 * vph_pc_public_evals_host: exactly one of point_pairs (n coordinates: the public vector is eq(point, .)) and pub_pairs (2^n entries); tensor != 0 (point form
 * only): through q_j = eq(point_hi, j) q' (one transform).  out_pairs: n_queries x 2 x 64 elements in vp_pc_public_evals' layout.
 * vph_pc_opening_digests_host: `answer` in vp_fri_query's layout for (n, n_queries) — vph_pc_query_answer_bytes gives its size; out: 64 bytes per opening
 * (recomputed leaf digest | root reached through the path).  0 = done, -1 = refused (sizes, a leaf outside [2^(n-7), 2^(n-2)), a non-canonical limb).     */
int vph_pc_public_evals_host(int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, int tensor, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs);
int vph_pc_opening_digests_host(int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out);
uint64_t vph_pc_query_answer_bytes(int n, int n_queries);
/* The same two on the session's device (vp_pc_public_evals, vp_fri_query_digests on its context, arguments as given). Return the
 * device library's status: VP_OK, or its refusal with the message in err. */
int vph_pc_public_evals(vph_session *, int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs,
                        char *err, int errlen);
int vph_fri_query_digests(vph_session *, int n, int n_queries, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, uint8_t *out, char *err, int errlen);
/* The mask row of the public evaluation (slot 64 of a masked commitment): out_pairs[2 q + h] = the public mask polynomial — the interpolant of the public mask,
 * zero-padded to ms, on the ms-th roots of unity — at (-1)^h w^leaf0[q].  _host: on the host, any power of two ms in 1 .. 2^(n-2), 1 .. ms mask elements; -1 = refused.
 * vph_pc_mask_evals: vp_pc_mask_evals on the session's context, arguments as given; the device library's status, its refusal in err.                             */
int vph_pc_mask_evals_host(int n, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs);
int vph_pc_mask_evals(vph_session *, int n, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms, int n_queries, const uint64_t *leaf0, uint64_t *out_pairs,
                      char *err, int errlen);
/* The commitment's verifier by value (no session, no circuit): everything verifier::verifyPoly checks behind fft_gkr, all 65 slices, on the caller's arrays.
 * n: bit length of the committed vector; exactly one of point_pairs (n coordinates: the public vector is eq(point, .)) and pub_pairs (2^n entries); pub_mask_pairs
 * (n_pub_mask <= ms elements, or null: zeros) and ms, the private mask's padded length — 1 for the zero mask, else a power of two in [8, min(2^16, 2^(n-2))];
 * claim; root_l, root_h; all_sum[65]; the n - 6 fold challenges and FRI roots; final_code[2048] (vp_fri_final), final_mask[32] (vp_fri_final_mask; zeros for the
 * zero mask); reps positions leaf0 in [2^(n-7), 2^(n-2)); answer: n_bytes in vp_fri_query's layout for (n, reps).  device >= 0: the heavy loops (vp_pc_public_evals,
 * vp_pc_mask_evals, vp_fri_query_digests) run there on a context made for the call; -1: on the host.  Same verdict either way.
 * 0 = accepted; 1 = rejected, err names the failed check ("commitment: slice sums ...", "Fri rs code check fail", "Fri msk rs code check fail", "commitment: Merkle
 * opening rejected", "commitment: FRI Merkle opening rejected (level k)", "Fri check consistency k round fail", "Fri msk check consistency k round fail", "Fri final
 * codeword mismatch", "Fri msk final codeword mismatch", a non-canonical opened value); -1 = malformed arguments (err); -2 = the device could not run the loops (err).
 * fft_gkr is not part of it: it is independent of the commitment (vph_prove_and_verify_full covers it).                                                            */
int vph_verify_commitment(int n, const uint64_t *point_pairs, const uint64_t *pub_pairs, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint64_t ms,
                          const uint64_t *claim_pair, const uint8_t root_l[32], const uint8_t root_h[32], const uint64_t *all_sum_pairs /* 65 */,
                          const uint64_t *r_pairs /* n - 6 */, const uint8_t *fri_roots /* 32 (n - 6) */, const uint64_t *final_code_pairs /* 2048 */,
                          const uint64_t *final_mask_pairs /* 32 */, int reps, const uint64_t *leaf0, const uint8_t *answer, uint64_t n_bytes, int device,
                          char *err, int errlen);
/* ---- The non-interactive commitment proof: Fiat-Shamir over the commitment by value ---------------------------------------------------------------------------
 * One block of bytes that anyone checks with no tape and no session: the level of vph_verify_commitment, with the fold challenges and the query positions
 * derived from the prover's own messages instead of handed over.  What it proves: that the committed vector's inner product with eq(point, .) is the claim, with
 * the reference's soundness per repetition (a proof of work on top is the prover's choice: "The proof of work" below); the multiple-of-32 corner of h is what it is for vph_verify_commitment.  Limits: unsharded
 * sessions, the point form of the public vector, masks within vp_commit_private_masked's limits (the verifier accepts ms <= 2^(n-6)).  Joining it to vph_prove_fs
 * and fft_gkr into one proof of the whole protocol is the next step and not part of this.
 *
 * The transcript chain.  The primitive is the one of vph_prove_fs: H(m, s) = SHA3-256 of 64 bytes, four little-endian u64 words m0..m3 followed by the 32-byte
 * state s.  The state starts as 32 zero bytes and every step is s = H(m, s), with m as follows:
 *     P(a, b, c, d)  a parameter block: two steps, {1, 0, 0, 0x50}, then {a, b, c, d}
 *     E(x)           a field element: {x.re, x.im, 0, 0x4d}
 *     D(t, d)        a digest under label t: two steps, {t, 0, 0, 0x44}, then the digest's four words
 *     C(c)           challenge number c: {c, 0, 0, 0x43}; the element is (s.w0 & P, s.w1 & P), P = 2^61 - 1, with a limb equal to P mapped to 0
 *     Q(q)           position number q: {q, 0, 0, 0x51}; leaf0 = 2^(n-7) + (s.w0 mod (2^(n-2) - 2^(n-7))), the range vph_verify_commitment accepts
 *     W(b, nonce)    proof of work: {nonce, b, 0, 0x57}; met when the low b bits of s.w0 are zero ("The proof of work" below)
 * With ln = n - 6 the order is:
 *      1. P(n, reps, ms, n_pub)
 *      2. D(0, root_l)
 *      3. E(point[i]), i < n
 *      4. E(pub_mask[i]), i < n_pub; n_pub = 0 when ms = 1
 *      5. E(claim)
 *      6. E(all_sum[i]), i < 65
 *      7. D(1, root_h)
 *      8. r_0 = C(0)
 *      9. for k = 0 .. ln - 1: fold by r_k, which gives root_k; D(2 + k, root_k); for k + 1 < ln also r_(k+1) = C(k + 1)
 *     10. E over the 2048 elements of vp_fri_final
 *     11. E over the 32 elements of vp_fri_final_mask (zeros for the zero mask)
 *    11w. in a version-2 proof only: W(pow_bits, nonce) ("The proof of work" below); a version-1 proof has no such step
 *     12. Q(q), q < reps, from the state step 11 (version 1) or W (version 2) leaves
 * Positions may repeat.  The point comes after root_l, so the committer cannot choose the witness after seeing it.
 *
 * Proof bytes, little-endian.  Header, 32 bytes: u32 magic 0x46435056 ("VPCF") | u32 version = 1 | u32 n | u32 reps | u64 ms | u64 n_pub.  Then, in this order:
 * the point (16 n bytes) | the public mask (16 n_pub) | the claim (16) | root_l (32) | root_h (32) | all_sum (65 x 16) | the FRI roots (32 ln) | the final codeword
 * (2048 x 16) | the final mask (32 x 16) | the answer in vp_fri_query's layout for (n, reps).
 * Version 2 (a proof with work): the same with version = 2 and 16 bytes behind the header, u64 pow_bits | u64 nonce; everything else keeps its place.
 *
 * vph_commit_fs: prover::commitFS on the session — commit_private(mask; null or all zero: the zero mask), commit_public_eq(point[, pub_mask]), the commit phase,
 * the final codewords, the positions, vp_fri_query.  flags 0: the commit phase is vp_fri_commit_fs (the device draws every challenge from the root it has just
 * computed, no host wait between the levels); VPH_FS_HOST_DRAWS: the vp_fri_step loop with the chain on the host — a second implementation, the same bytes.
 * *len is set to the proof's size whenever it is known.  0 = done; -1 = a bad argument or cap too small (err); -2 = refused or failed (err: a sharded session,
 * the device library's refusal of a mask, ...).  vph_last_commit_fs_times: [0] host seconds, [1] device milliseconds of the last proof's commit phase alone.
 * vph_verify_commitment_fs: parses under vph_verify_full_record's rules (bounds on every read, canonical limbs, the proof ends where the answer ends; ms and
 * n_pub by vph_verify_commitment's rules), derives the challenges and positions from the chain and runs vph_verify_commitment's checks unchanged (device as
 * there).  Return codes of vph_verify_commitment: 0 accepted, 1 rejected (err: the failed check), -1 malformed (err), -2 no device.
 * vph_commitment_fs_challenges: the derivation alone — the n - 6 challenges and the reps positions of a well-formed proof; -1 otherwise.                       */
enum { VPH_FS_HOST_DRAWS = 1 };
int vph_commit_fs(vph_session *, const uint64_t *point_pairs, int n_point, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs,
                  uint64_t n_pub_mask, int flags, uint8_t *out, uint64_t cap, uint64_t *len, char *err, int errlen);
void vph_last_commit_fs_times(vph_session *, double out[2]);
int vph_verify_commitment_fs(const uint8_t *proof, uint64_t len, int device, char *err, int errlen);
int vph_commitment_fs_challenges(const uint8_t *proof, uint64_t len, uint64_t *r_pairs /* n - 6 */, uint64_t *leaf0 /* reps */);
/* The proof of work (grinding) of the commitment proof and of the joined proof.  W(b, nonce) is the chain step state = H({nonce, b, 0, 0x57}, state); the work is
 * met when the low b bits of the new state's first word (little-endian u64, as everywhere in the chain) are zero.  It stands behind the two final codewords and in
 * front of the positions, which are drawn from the state it leaves: the nonce moves every position, so a prover cannot grind after seeing them, and each bit
 * doubles the work of a prover who re-draws the positions of a commitment that would not pass — it buys soundness against the query phase alone, nothing
 * for the GKR and fft_gkr parts.  A proof with work is version 2 of its kind ("VPCF" or "VPFF"): the 32-byte header is followed by u64 pow_bits | u64 nonce.
 * Parser: pow_bits in 1 .. 48, anything else is malformed — a version-2 proof with pow_bits = 0 too: version 1 is the only encoding of "no work"; a version-1
 * body under a version-2 header is 16 bytes short of its answer and malformed by that rule.  Verdicts: work not met is REJECTED (1; err names the proof of
 * work), not malformed; pow_bits below the verifier's demand min_pow_bits is rejected (err names both numbers), and so is a version-1 proof under
 * min_pow_bits >= 1.  In the commitment proof both are decided after the parse and before any other check.  In the joined proof the demand is decided by the
 * header, before the GKR part is replayed (a proof with too little work under a well-formed header is rejected whatever lies behind it), and the work where the
 * chain reaches it: after the replay and the parse of the remaining sections, before fft_gkr's and the commitment's checks.
 * vph_fs_grind_host: the smallest nonce in [first, first + max_tries) that meets `bits` bits of work on state_in, and the state behind W; sha3.hpp on one
 * thread — the second implementation of vp_fs_grind (include/vpgpu.h) and the search of VPH_FS_HOST_DRAWS.  0; -5 (vp_fs_grind's VP_ELIMIT) when the range
 * holds none, outputs untouched; -1 for a null pointer, bits outside 1 .. 48, max_tries = 0, a range that would pass 2^64.
 * vph_commit_fs_pow / vph_prove_full_fs_pow: vph_commit_fs / vph_prove_full_fs_ex with pow_bits.  0 is that call exactly and its version-1 bytes; 1 .. 32 grinds
 * from nonce 0 through 64 x 2^pow_bits tries (failing all of them has probability e^-64) and returns -2 with a reason when none meets the work; anything else is
 * a bad argument (-1).  The nonce is vp_fs_grind's on the session's context, checked against the host's step; under VPH_FS_HOST_DRAWS (commitment proof) it is
 * vph_fs_grind_host's — the same bytes.  Sharded sessions are refused as before.
 * vph_verify_commitment_fs_min / vph_verify_full_fs_min: the verifiers with the demand; vph_verify_commitment_fs / vph_verify_full_fs are these with
 * min_pow_bits = 0 and so accept a well-formed version-2 proof whose work is met.  vph_commitment_fs_challenges reads both versions.
 * vph_fs_pow: the two fields of either kind of proof, from the header alone (the body is not parsed): version 1 gives 0, 0; -1 for a null pointer, fewer bytes
 * than the header, another magic or version, pow_bits outside 1 .. 48.                                                                                      */
int vph_fs_grind_host(const uint8_t state_in[32], int bits, uint64_t first, uint64_t max_tries, uint64_t *nonce, uint8_t state_out[32]);
int vph_commit_fs_pow(vph_session *, const uint64_t *point_pairs, int n_point, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs,
                      uint64_t n_pub_mask, int flags, int pow_bits, uint8_t *out, uint64_t cap, uint64_t *len, char *err, int errlen);
int vph_verify_commitment_fs_min(const uint8_t *proof, uint64_t len, int device, int min_pow_bits, char *err, int errlen);
int vph_fs_pow(const uint8_t *proof, uint64_t len, uint64_t *bits, uint64_t *nonce);
/* The transcript chain: fft_gkr.  vp_fft_gkr_fs (include/vpgpu.h) continues a chain of the steps above from a 32-byte state and draws fft_gkr's whole tape from it
 * on the device.  A slot's counter is its index in the tape layout (r[lg] | x[64] | r_0[lg+10] | r_1[lg+10] | addition layer r_u[lg+6], r_v[lg+6] | multiplication
 * layer r_u[lg], r_v[lg] | per depth r_u[lg], r_v[lg], alpha, beta); messages are in vp_fft_gkr's layout.  The order:
 *      1. r[i] = C(slot), i < lg; x[i] = C(slot), i < 64
 *      2. E(O[i]), i < 64; every slot of r_0, then of r_1 = C(slot)
 *      3. addition layer: per round k < lg + 6: E(a), E(b), E(c), r_u[k] = C(slot); E(v_u); r_v[k] = C(slot), k < lg + 6 (they multiply beta = 0 and are
 *         don't-cares of the prover; fft_gkr_check reads them, so they are drawn)
 *      4. multiplication layer: the same with lg rounds
 *      5. per inverse-FFT depth d < lg: phase 1 per round E(a), E(b), E(c), r_u[k] = C(slot); E(v_u); phase 2 per round E(a), E(b), E(c), r_v[k] = C(slot);
 *         E(v_v); alpha = C(slot), beta = C(slot)
 * A draw never precedes the polynomial it challenges.  fft_gkr is self-contained in the reference: its inputs are draws, and it binds nothing of a commitment —
 * what ties it to one is only the chain state it starts from.
 * vph_fft_gkr_fs_tape: the derivation alone, on the host — the tape (n_tape pairs) and the closing state from state_in and the messages; 0, or -1 (lg outside
 * 1..19, a null pointer, n_msgs not vp_fft_gkr_sizes', a non-canonical limb).  vph_fft_gkr_check: fft_gkr_check (fft_gkr_verify.hpp) on a tape and messages by
 * value: 0 accepted, 1 rejected, -1 malformed by the same rules.  vph_fft_gkr_check and vph_fft_gkr_fs are test and diagnostic entry points: the joined proof
 * calls fft_gkr_check and prover::fftGkrFS itself.                                                                                          */
int vph_fft_gkr_fs_tape(int lg, const uint8_t state_in[32], const uint64_t *msgs_pairs, uint64_t n_msgs, uint64_t *tape_pairs, uint8_t state_out[32]);
int vph_fft_gkr_check(int lg, const uint64_t *tape_pairs, uint64_t n_tape, const uint64_t *msgs_pairs, uint64_t n_msgs);
/* vp_fft_gkr_fs on the session's context (prover::fftGkrFS): messages (cap_elems >= n_msgs), the tape drawn and the closing state; the host re-derives the tape and
 * the state from the returned messages and fails if the device's differ.  0 = done, -1 = a bad argument, -2 = refused or failed (err).                      */
int vph_fft_gkr_fs(vph_session *, int lg, const uint8_t state_in[32], uint64_t *msgs_pairs, uint64_t cap_elems, uint64_t *tape_pairs, uint8_t state_out[32],
                   char *err, int errlen);
/* The GKR part on the device (the transcript chain, continued).  vp_prove_gkr_fs (include/vpgpu.h) continues a chain of the steps above from a 32-byte state and draws every
 * challenge of the GKR part on the device.  The schedule is vph_prove_fs's (verifier::run() in Fiat-Shamir mode), unchanged; the counter of C runs from 0 over the
 * draws in the order below, whatever the slot a draw lands in:
 *      1. r_liu[j] = C, j < the output layer's bit length
 *      2. E(Vres)
 *      3. per layer i from the top:
 *           assert_random = C
 *           phase 1: per round j < bitLength(i - 1): E(a), E(b), E(c), r_u[j] = C; then E(claim_u)
 *           phase 2, if maxDadBitLength(i) != -1: per round j < maxDadBitLength(i): E(a), E(b), E(c), r_v[i][j] = C; then E of each of the i claims
 *           sig[j] = C for all `size` entries
 *           the Liu sumcheck: per round j < bitLength(i - 1): E(a), E(b), E(c), r_liu[j] = C; then E(vr)
 * A draw never precedes the polynomial it challenges.  The draws are returned where vp_prove_gkr reads them (its tape layout: r_0 | per layer r_u[max_bl],
 * assert_random, r_v, sig[size], r_liu[max_bl]); a slot the schedule never draws — the coordinates of r_u / r_liu beyond a layer's bit length — is zero.  The
 * transcript is vp_prove_gkr's, hence vph_prove_fs's proof bytes; vp_prove_gkr on the returned tape returns it again.
 * vph_gkr_sizes: the circuit's tape length (elements) and transcript size (bytes), no GPU.  vph_gkr_fs_tape: the derivation alone, by value, on the host — a walk
 * over the transcript's bytes (no sumcheck is checked): the tape, the number of draws and the closing state from state_in and the n transcript bytes; 0, or -1 (a
 * null pointer, n not the circuit's transcript size, a non-canonical limb).  vph_prove_gkr_fs: vp_prove_gkr_fs on the session's context (prover::proveGkrFS): the
 * host re-derives tape, count and state from the returned transcript with that walk and fails if the device's differ.  0 = done, -1 = a bad argument (err),
 * -2 = refused or failed (err: a sharded session, ...).
 * vph_prove_fs_ex / vph_prove_full_fs_ex: vph_prove_fs / vph_prove_full_fs with flags.  0 is that call exactly.  VPH_FS_DEVICE_GKR: the GKR part is
 * prover::proveGkrFS — the prover without the verifier in its loop: no host round trip per challenge, none of the verifier's O(|C|) sums — and the same bytes.
 * With the flag nothing is verified: vph_prove_fs_ex returns 0 = done (res->verified = 0, res->gkr_device_ms = the call's device time), and vph_verify_fs /
 * vph_verify_full_fs are the check.  In vph_prove_full_fs_ex the point is read from the tape's r_liu slots of layer 1 and the claim is the transcript's last
 * element.                                                                                                                                                       */
enum { VPH_FS_DEVICE_GKR = 2 };
int vph_gkr_sizes(const vph_circuit *, uint64_t *n_tape, uint64_t *n_transcript_bytes);
int vph_gkr_fs_tape(const vph_circuit *, const uint8_t state_in[32], const uint8_t *transcript, uint64_t n, uint64_t *tape_pairs, uint64_t *n_draws, uint8_t state_out[32]);
int vph_prove_gkr_fs(vph_session *, const uint8_t state_in[32], uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint64_t *tape_pairs, uint64_t *n_draws,
                     uint8_t state_out[32], char *err, int errlen);
int vph_prove_fs_ex(vph_session *, uint8_t *proof, uint64_t capacity, uint64_t *n_written, vph_result *res, int flags, char *err, int errlen);
int vph_prove_full_fs_ex(vph_session *, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                         uint64_t *len, uint64_t *point_pairs /* n, or null */, int flags, char *err, int errlen);
/* ---- The joined proof: one block of bytes for the whole protocol, checked by a verifier that holds only the circuit ----------------------------------------------
 * No tape, no session, no input values.  The chain is the one above, in this order:
 *      1. the statement: the four words of layeredCircuit::statementDigest(with_inputs = false) — the digest of vph_prove_fs under another domain tag with the input
 *         layer's values left out (here the input is the witness that root_l commits to) — as one step, then {size, 0, 0, 0x53}
 *      2. the head: P(n, reps, ms, n_pub); E(pub_mask[i]), i < n_pub (n_pub = 0 when ms = 1); D(0, root_l) — before any GKR draw
 *      3. the GKR part: exactly vph_prove_fs's schedule with the input check left to the commitment — every prover element E, every challenge C(counter) with the
 *         counter running from 0; it ends with the point r_liu (the first n coordinates) and the claim on the input layer
 *      4. the commitment head at that point: E(input_0), E(all_sum[i]), i < 65, D(1, root_h)
 *      5. fft_gkr at lg = n - 6 from that state ("The transcript chain: fft_gkr" below)
 *      6. the FRI commit phase from the state fft_gkr leaves, as steps 8 and 9 of the commitment proof: r_0 = C(0); per level D(2 + k, root_k), r_(k+1) = C(k + 1)
 *      7. E over the final codeword (2048), E over the final mask codeword (32), in a version-2 proof W(pow_bits, nonce), then Q(q), q < reps
 * Proof bytes: header u32 magic 0x46465056 ("VPFF") | u32 version = 1 | u32 n | u32 reps | u64 ms | u64 n_pub; then the public mask (16 n_pub) | root_l (32) | the GKR
 * bytes (vph_prove_fs's proof for this chain) | root_h (32) | input_0 (16) | all_sum (65 x 16) | the fft_gkr messages | the FRI roots (32 (n - 6)) | the final codeword |
 * the final mask | the answer in vp_fri_query's layout.  The point is not in the proof: it is derived.  Version 2: version = 2 and u64 pow_bits | u64 nonce behind
 * the header ("The proof of work" above), everything else in its place.
 * vph_verify_full_fs parses under vph_verify_full_record's rules (bounds on every read, canonical limbs, the proof ends where the answer ends; n must be the circuit's
 * input bit length; ms and n_pub by vph_verify_commitment's rules), replays the GKR part, compares its claim with input_0, derives fft_gkr's tape and calls
 * fft_gkr_check unchanged, fills the commitment by value and calls vph_verify_commitment's checks unchanged (device >= 0: their heavy loops on that GPU): no algebra of
 * its own.  0 accepted, 1 rejected (err: the failed check), -1 malformed (err), -2 no device.  point_pairs (may be null): the n derived coordinates, written unless
 * the proof is malformed (a rejected GKR part: as far as its replay got).  vph_prove_full_fs: verifier::proveFullFS on the session (masks as vph_commit_fs); 0 done, -1 a bad argument or cap too small (*len: the
 * size), -2 refused or failed (a sharded session, a mask outside the limits, ...).  Limits: unsharded sessions; masks: ONE rule in two places, as for
 * vph_verify_commitment_fs — the parser takes every ms a prover can commit (1, or a power of two in [8, min(2^16, 2^(n-2))]: anything else is malformed), and the
 * commitment's checks then reject ms > 2^(n-6) as the reference's verifier does ("Fri msk rs code check fail"), so an accepted masked proof has n >= 9.       */
int vph_prove_full_fs(vph_session *, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                      uint64_t *len, uint64_t *point_pairs /* n, or null */, char *err, int errlen);
int vph_verify_full_fs(vph_circuit *, const uint8_t *proof, uint64_t len, int device, uint64_t *point_pairs /* n, or null */, char *err, int errlen);
int vph_prove_full_fs_pow(vph_session *, int reps, const uint64_t *mask_pairs, uint64_t n_mask, const uint64_t *pub_mask_pairs, uint64_t n_pub_mask, uint8_t *out, uint64_t cap,
                          uint64_t *len, uint64_t *point_pairs /* n, or null */, int flags, int pow_bits, char *err, int errlen);
int vph_verify_full_fs_min(vph_circuit *, const uint8_t *proof, uint64_t len, int device, int min_pow_bits, uint64_t *point_pairs /* n, or null */, char *err, int errlen);
/* FRI commit phase of the last vph_prove_and_verify_full: Merkle root per fold step (32 bytes each), final codeword (2048
 * elements), fold challenges (one element per step); any pointer may be NULL.  Returns the number of steps or -1. */
int vph_last_fri(vph_session *, uint8_t *roots, uint64_t roots_cap, uint64_t *final_pairs, uint64_t *r_pairs);
/* fft_gkr of the last vph_prove_and_verify_full (vp_fft_gkr's message layout); returns the element count or -1.  vph_last_pc_times:
 * [0] "Polynomial commitment: prove time" by the reference's definition (src/verifier.cpp:183: commit_private + commit_public +
 * commit_phase + fft_gkr's prover time), [1] the fft_gkr share of it, [2] answering the queries (not part of [0], as in the reference). */
int64_t vph_last_fft_gkr(vph_session *, uint64_t *pairs, uint64_t cap_elems);
void vph_last_pc_times(vph_session *, double out[3]);
/* r_liu after the last Liu sumcheck of the last vph_prove_full / vph_prove_and_verify_full (the protocol's public vector is its eq
 * table, src/verifier.cpp:368-369); returns the number of coordinates or -1. */
int vph_last_point(vph_session *, uint64_t *pairs, int cap);
/* seconds spent in phase inits | round messages | finalize calls by the last vph_prove_interactive */
void vph_interactive_breakdown(vph_session *, double out[3]);
/* my_hhash on the host (verifier side): SHA3-256 of n 64-byte messages.                                   */
void vph_test_sha3(const uint8_t *in, uint8_t *out, uint64_t n);
/* poly_commit_prover::commit_phase (vpd_verifier.cpp:44-74) with caller-supplied fold challenges: n_steps calls of
 * fri::commit_phase_step, then commit_phase_final.  roots: 32 bytes per step; final_code: 2048 {real,img} pairs.
 * commit_public (or vph_prove_full) must have run on this session.                                       */
int vph_fri_commit(vph_session *, const uint64_t *r_pairs, int n_steps, uint8_t *roots, uint64_t *final_pairs, char *err, int errlen);
/* same through vp_fri_commit: every step in one device pass */
int vph_fri_commit_batched(vph_session *, const uint64_t *r_pairs, int n_steps, uint8_t *roots, uint64_t *final_pairs, char *err, int errlen);
/* The commitment calls below go through the session's prover, so on a session with a sharded commitment (vph_session_create_sharded) they run on
 * every rank and return the merged answer; on any other session they are the calls of include/vpgpu.h on its one context.  0 = done, -2 = error (err).
 * vph_commit_private_masked: prover::commit_private(mask) (an all-zero mask is vph_commit_private; a non-zero one is refused on a sharded commitment).
 * vph_commit_public_eq: prover::commit_public_eq, out = root_h | input_0 | all_sum[65].  vph_fri_open_many / vph_fri_query: vp_fri_open_many /
 * vp_fri_query with their layouts (path_stride in bytes, a multiple of 32).                                                                      */
int vph_commit_private_masked(vph_session *, const uint64_t *mask_pairs, uint64_t n_mask, uint8_t root[32], double *ms, char *err, int errlen);
int vph_commit_public_eq(vph_session *, const uint64_t *point_pairs, int n_point, uint8_t out[32 + 16 + 65 * 16], double *ms, char *err, int errlen);
/* prover::commit_public_eq(point, mask, ...): behind vph_commit_private_masked with a non-zero mask, vp_commit_public_eq_masked (mask_pairs null or n_mask = 0: one
 * zero element); behind a zero private mask it is vph_commit_public_eq, whatever the public mask.  Same layout of `out`.                                          */
int vph_commit_public_eq_masked(vph_session *, const uint64_t *point_pairs, int n_point, const uint64_t *mask_pairs, uint64_t n_mask, uint8_t out[32 + 16 + 65 * 16],
                                double *ms, char *err, int errlen);
int vph_fri_open_many(vph_session *, int n, const int32_t *oracle, const uint64_t *leaf, uint64_t *values_pairs, uint8_t *paths, int path_stride,
                      int32_t *path_len, char *err, int errlen);
int vph_fri_query(vph_session *, int n_queries, const uint64_t *leaf0, uint8_t *out, uint64_t capacity, uint64_t *n_written, char *err, int errlen);
/* The whole protocol of verifier::verify() up to commit_public (src/verifier.cpp:134-169,363-379), interactive
 * GKR: writes merkle_root_l | GKR slice | merkle_root_h | input_0 | all_sum[65] — the golden layout.   */
int vph_prove_full(vph_session *, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, int batched, char *err,
                   int errlen);
/* The prover side of the COMPLETE protocol in one pass (bench step of BASELINE configs[2]).  vph_draw_protocol_tape: F::init() and every
 * draw of verifier::verify() in its order — GKR (src/verifier.cpp:144-279), fft_gkr (fft_circuit_GKR.cpp), FRI fold challenges
 * (vpd_verifier.cpp:57) — valid up front because the reference's challenges are glibc random() (fieldElement.cpp:119-124).
 * vph_prove_protocol: commit_private -> batched GKR -> commit_public on eq(r_liu, .) built on the device (vp_commit_public_eq) -> fft_gkr
 * -> FRI commit phase + final codeword; no verifier work inside.  transcript: the golden layout; fri_roots: 32 bytes per step;
 * final_pairs: 2048 elements; sec[6] = whole pass | commit_private | GKR | commit_public | fft_gkr | FRI commit (host wall clock).   */
int vph_draw_protocol_tape(vph_session *);
int vph_prove_protocol(vph_session *, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap,
                       uint64_t *final_pairs, double sec[6], char *err, int errlen);            /* = _ex with flags 0 */
/* flags: 0 = every call waits for its result before the next is made (sec[1..5]: host wall clock per call);
 * VPH_PASS_DEFERRED = the calls are queued back to back and collected at the end (vp_set_deferred, include/vpgpu.h: a device that idles between two calls
 *   runs the following milliseconds at a lower clock); sec[1..5]: device time per call;
 * | VPH_PASS_QUEUE_NEXT = before it waits, the pass queues the next pass's head (commit_private of the same witness) behind its own FRI folds, and
 *   the next vph_prove_protocol_ex of the session starts at its GKR part: no idle device between two proofs of a session that proves back to back.  The
 *   openings of THIS pass's commitment are gone once that head runs (it overwrites the codeword); a pass that will be opened is made without the flag.
 * In every combination the pass hashes ONCE (vp_pc_hash_late, include/vpgpu.h): commit_private and commit_public queue their transforms only, and the FRI
 * commit call hashes the leaves of l, h and all FRI levels in one launch and builds their trees together (a head queued by the previous pass is a complete
 * commit_private: such a pass merges h and the levels).  Same transcript, same layout; sec[1] and sec[3] are then the transforms alone and sec[5] carries
 * all of the hashing — their sum, the reference's "prove time", keeps its meaning.
 * | VPH_PASS_HASH_PER_CALL = the earlier form, every call hashing its own oracle (three leaf-hash launches, three tree chains): the partner of A/B
 *   comparisons in one process (tools/pass_modes.py); the environment variable VPH_HASH_PER_CALL, read once, selects it for every pass. */
enum { VPH_PASS_DEFERRED = 1, VPH_PASS_QUEUE_NEXT = 2, VPH_PASS_HASH_PER_CALL = 4 };
int vph_prove_protocol_ex(vph_session *, uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap,
                          uint64_t *final_pairs, double sec[6], int flags, char *err, int errlen);
/* The same pass with the mask vectors of a hiding commitment (include/vpgpu.h, "the mask slice with CONTENT"): vp_commit_private_masked(pri_mask) ->
 * batched GKR -> vp_commit_public_eq_masked(r_liu, pub_mask; null or n_pub = 0: one zero element) -> fft_gkr -> the one-pass FRI commit phase, whose single leaf
 * launch closes every chain with the mask slice's pair.  Outputs and sec[] as vph_prove_protocol_ex; final_mask_pairs (may be null): the mask slice's last
 * codeword, 32 elements (vp_fri_final_mask).  flags as above, with two differences: the masked commit_private reads the caller's mask and completes at once in
 * every mode (under hash-once its leaf chains still wait for the FRI call), and VPH_PASS_QUEUE_NEXT is refused (-1, message) — the queued head is an unmasked
 * commit_private of the same witness, and a head queued by an earlier pass is not used.  A null or all-zero private mask is vph_prove_protocol_ex, byte for byte
 * (final_mask_pairs: zeros), QUEUE_NEXT included.                                                                                                               */
int vph_prove_protocol_masked(vph_session *, const uint64_t *pri_mask_pairs, uint64_t n_pri, const uint64_t *pub_mask_pairs, uint64_t n_pub, uint8_t *transcript,
                              uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap, uint64_t *final_pairs, uint64_t *final_mask_pairs /* 32 */,
                              double sec[6], int flags, char *err, int errlen);
/* No GPU needed: F::init(), draw the tape for `circuit`, replay the host verifier over `transcript`
 * (GKR slice).  0 = accepted, 1 = rejected.                                                            */
int vph_verify_transcript(vph_circuit *, const uint8_t *transcript, uint64_t n, int skip_predicates);
/* The same replay against the caller's tape (vph_set_tape's conditions: -1 if it does not fit the circuit).  No GPU, no generator.   */
int vph_verify_transcript_tape(vph_circuit *, const uint64_t *tape_pairs, uint64_t n_tape, const uint8_t *transcript, uint64_t n, int skip_predicates);
/* Fiat-Shamir mode: a non-interactive GKR proof.  Every verifier challenge is derived with SHA3-256 from the
 * circuit's structural hash and all prover messages before it (one challenge per sumcheck round, after that round's
 * polynomial); the prover runs through its interactive entry points.  The proof has the transcript layout of vph_prove_gkr.
 * Not comparable with the reference's transcripts (its verifier draws random()).  0 = the built-in verifier accepted.  */
int vph_prove_fs(vph_session *, uint8_t *proof, uint64_t capacity, uint64_t *n_written, vph_result *res, char *err, int errlen);
/* No GPU, no tape: re-derive the challenges from `proof` and run the verifier's checks.  0 = accepted, 1 = rejected.   */
int vph_verify_fs(vph_circuit *, const uint8_t *proof, uint64_t n);
/* Which check of the GKR part rejected: the first failed check of the calling thread's last GKR replay, through vph_verify_transcript(_tape), vph_verify_fs,
 * vph_check, vph_verify_full_record(_dev) and vph_verify_full_fs.  Returns the kind: 0 none (accepted, or rejected without a failed check: a transcript of the
 * wrong length or with a non-canonical element), 1 phase1 / 2 phase2 / 4 liu (a sumcheck round: p(0) + p(1) against the running claim), 3 semi_final (a layer's
 * closing value from the wiring predicates), 5 liu_semi_final (vr * gr against the Liu sumcheck's last value), 6 input (the last claim against the input layer, or
 * against the commitment's input_0 where the commitment takes the claim over: then the replay's other checks all held).  *layer: the layer the check belongs to
 * (0 for input); *round: the round, -1 for a closing check.  Either pointer may be null.  A call that never reaches the replay (a tape that does not fit, a
 * malformed header) leaves the previous answer.                                                                                                                  */
int vph_last_gkr_failure(int *layer, int *round);
/* vp_commit_stats: device milliseconds of the last commit_private / commit_public / FRI call on this session. */
double vph_commit_device_ms(vph_session *);
/* One proof over `world` GPUs (vp_set_shard): vph_prove_gkr on this session then proves only the sumchecks dealt to `rank`
 * and leaves the rest of the transcript zero; the u64 sum of all ranks' transcripts is the proof.      */
int vph_set_shard(vph_session *, int rank, int world);
/* Index-split proof without a communicator: V_u of the split phase-2 chains by a caller-side exchange (include/vpgpu.h: vp_shard_vu_partials /
 * vp_shard_vu_set) on the session's tape.  partials: 2 u64 per entry; returns the number of entries (0: nothing to exchange), < 0: refused.     */
int vph_shard_vu_partials(vph_session *, uint64_t *partials, int capacity);
int vph_shard_vu_set(vph_session *, const uint64_t *sums, int n);
/* vp_shard_chains: owner and cost estimate per sumcheck chain; returns the number of chains (< 0 on error). */
int vph_shard_chains(vph_session *, int32_t *owner, double *cost, int capacity);

#ifdef __cplusplus
}
#endif
#endif
