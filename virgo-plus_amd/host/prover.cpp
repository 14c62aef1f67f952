#include "prover.hpp"
#include "pc_fs.hpp"
#include "fft_gkr_fs.hpp"
#include "gkr_fs.hpp"
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <functional>
#include <memory>
#include <chrono>
#include <thread>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>

#include <cstdio>
#include <cstdlib>
#include <string>

static_assert(sizeof(F) == sizeof(vp_F), "F must be two u64 limbs");
static inline const vp_F *cF(const F *p) { return reinterpret_cast<const vp_F *>(p); }
static inline vp_F *mF(F *p) { return reinterpret_cast<vp_F *>(p); }

void prover::check(int rc, const char *what) {
    if (rc == VP_OK) return;
    throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + vp_last_error(ctx));
}

// src/prover.cpp:14-25.  The circuit tables are flattened to structure-of-arrays and copied to HBM once;
// the constructor then evaluates the circuit on the device like the reference's constructor does on the
// CPU.  A violated assert gate surfaces as an exception instead of the reference's exit(EXIT_FAILURE).
// Worker threads of a round-sharded prover: rank 0 runs on the calling thread, rank r >= 1 on worker r.  A worker spins on the job counter for a
// while after each job (a round is tens of microseconds; waking a blocked thread costs about as much) and then blocks on the condition variable.
struct prover::Pool {
    const int n;
    std::vector<std::thread> th;
    std::mutex mu; std::condition_variable cv;
    std::atomic<unsigned long long> gen{0}; std::atomic<int> left{0};
    const std::function<void(int)> *job = nullptr;
    bool quit = false;
    explicit Pool(int n_) : n(n_) { for (int r = 1; r < n; ++r) th.emplace_back([this, r] { loop(r); }); }
    ~Pool() {
        { std::lock_guard<std::mutex> lk(mu); quit = true; gen.fetch_add(1); }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    void loop(int r) {
        unsigned long long seen = 0;
        for (;;) {
            for (int spin = 0; gen.load(std::memory_order_acquire) == seen; ++spin) {
                if (spin < 20000) { std::this_thread::yield(); continue; }
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return gen.load(std::memory_order_acquire) != seen; });
            }
            seen = gen.load(std::memory_order_acquire);
            if (quit) return;
            (*job)(r);
            left.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    void run(const std::function<void(int)> &fn) {
        job = &fn;
        left.store(n - 1, std::memory_order_release);
        { std::lock_guard<std::mutex> lk(mu); gen.fetch_add(1, std::memory_order_acq_rel); }
        cv.notify_all();
        fn(0);
        while (left.load(std::memory_order_acquire)) std::this_thread::yield();
    }
};

int prover::onRanks(const std::function<int(int, vp_ctx *)> &fn, const char *what) {
    if (rk.size() <= 1) { const int rc = fn(0, ctx); if (rc != VP_EXCHANGE) check(rc, what); return rc; }
    std::vector<int> rc(rk.size(), VP_OK);
    pool->run([&](int r) { rc[r] = fn(r, rk[r]); });
    int n_x = 0;
    for (size_t r = 0; r < rk.size(); ++r) {
        if (rc[r] == VP_EXCHANGE) { ++n_x; continue; }
        if (rc[r] != VP_OK) throw std::runtime_error(std::string(what) + " failed on rank " + std::to_string(r) + " (" + std::to_string(rc[r]) + "): " + vp_last_error(rk[r]));
    }
    if (n_x && n_x != (int) rk.size()) throw std::runtime_error(std::string(what) + ": only some ranks stopped at the gather");
    return n_x ? VP_EXCHANGE : VP_OK;
}

prover::prover(const layeredCircuit &cir, int device, const vp_options *options) : C(cir) { upload({device}, options); }

prover::prover(const layeredCircuit &cir, const std::vector<int> &devices, int min_log, const vp_options *options, bool shard_commitment) : C(cir) {
    if (devices.empty() || devices.size() > 8 || (devices.size() & (devices.size() - 1)))
        throw std::invalid_argument("round-sharded prover: 1, 2, 4 or 8 ranks");
    // Ranks that share a device run without the resident round kernel: it holds the hardware queue it was launched on until its phase ends, and
    // another rank's launches that the runtime put on the same queue would wait behind it while the prover waits for their answer (each such
    // round would stall until the kernel's time-out).  Ranks on GPUs of their own keep it.
    std::vector<int> sorted(devices);
    std::sort(sorted.begin(), sorted.end());
    vp_options shared{};
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
        if (options) shared = *options;
        else vp_options_default(&shared);
        shared.persistent_rounds = 0;
        options = &shared;
    }
    upload(devices, options);
    try {
        for (size_t r = 0; r < rk.size(); ++r) {
            const int rc = vp_set_round_shard(rk[r], (int) r, (int) rk.size(), min_log);
            if (rc != VP_OK) throw std::runtime_error("vp_set_round_shard failed (" + std::to_string(rc) + "): " + vp_last_error(rk[r]));
        }
        if (shard_commitment && rk.size() > 1) {
            const int n = C.circuit[0].bitLength;
            if (n < 7 || (1ull << (n - 6)) < 2 * rk.size())
                throw std::runtime_error("sharded commitment: an input layer of 2^" + std::to_string(n) + " wires has 2^" + std::to_string(n - 6) +
                                         " positions per slice, fewer than the 2 per rank that " + std::to_string(rk.size()) + " ranks need");
            for (size_t r = 0; r < rk.size(); ++r) {
                const int rc = vp_pc_set_shard(rk[r], (int) r, (int) rk.size());
                if (rc != VP_OK) throw std::runtime_error("vp_pc_set_shard failed (" + std::to_string(rc) + "): " + vp_last_error(rk[r]));
            }
            shard_pc = true;
        }
    } catch (...) {
        pool.reset();
        for (vp_ctx *c : rk) vp_destroy(c);
        rk.clear(); ctx = nullptr;
        throw;
    }
}

void prover::upload(const std::vector<int> &devices, const vp_options *options) {
    for (int device : devices) {
        vp_ctx *c = nullptr;
        int rc = vp_create_with_options(device, options, &c);
        if (rc != VP_OK) {
            for (vp_ctx *o : rk) vp_destroy(o);
            rk.clear();
            throw std::runtime_error("vp_create failed (" + std::to_string(rc) + "): no usable MI355X / HIP device");
        }
        rk.push_back(c);
    }
    ctx = rk[0];
    if (rk.size() > 1) pool.reset(new Pool((int) rk.size()));
    const int n = C.size;
    const bool dbg = getenv("VP_DEBUG_UPLOAD") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    std::vector<vp_layer_desc> desc(n);
    // uninitialised arrays (no zero fill, the pages are first touched by the threads that write them)
    struct Flat {
        std::unique_ptr<uint8_t[]> ty, as; std::unique_ptr<int32_t[]> l; std::unique_ptr<uint32_t[]> u, v, lv; std::unique_ptr<vp_F[]> c;
        std::vector<uint64_t> dsz; std::vector<int32_t> dbl; std::vector<std::vector<uint32_t>> did; std::vector<const uint32_t *> dptr;
    };
    std::vector<Flat> flat(n);
    // gate (array of structs, src/circuit.h:11-22) -> the structure-of-arrays view of vp_layer_desc.  Plain copies, split over the host's
    // cores in ranges of 2^20 gates (x1024: 1e8 gates, 0.5 s on one core): pass 1 finds the layers with constants / assert gates, pass 2 copies.
    struct Range { int layer; u64 b, e; };
    std::vector<Range> ranges;
    for (int i = 0; i < n; ++i) {
        const u64 m = C.circuit[i].size;
        for (u64 b = 0; b < m; b += (1u << 20)) ranges.push_back({i, b, std::min<u64>(m, b + (1u << 20))});
    }
    std::vector<std::atomic<char>> c_seen(n), as_seen(n);
    for (int i = 0; i < n; ++i) { c_seen[i] = 0; as_seen[i] = 0; }
    auto run_pool = [&](const std::function<void(const Range &)> &body) {
        std::atomic<size_t> next{0};
        auto work = [&]() { for (;;) { const size_t q = next.fetch_add(1); if (q >= ranges.size()) return; body(ranges[q]); } };
        const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        const unsigned nt = (unsigned) std::min<size_t>(hw, std::max<size_t>(1, ranges.size()));
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    };
    run_pool([&](const Range &r) {
        const layer &L = C.circuit[r.layer];
        bool c = false, as = false;
        for (u64 g = r.b; g < r.e; ++g) { const gate &G = L.gates[g]; c |= (G.ty == Addc || G.ty == Mulc); as |= G.is_assert; }
        if (c) c_seen[r.layer] = 1;
        if (as) as_seen[r.layer] = 1;
    });
    std::vector<char> any_c(n, 0), any_as(n, 0);
    for (int i = 0; i < n; ++i) {
        Flat &f = flat[i];
        const u64 m = C.circuit[i].size;
        any_c[i] = c_seen[i]; any_as[i] = as_seen[i];
        f.ty.reset(new uint8_t[m]); f.as.reset(new uint8_t[m]); f.l.reset(new int32_t[m]);
        f.u.reset(new uint32_t[m]); f.v.reset(new uint32_t[m]); f.lv.reset(new uint32_t[m]);
        if (any_c[i]) f.c.reset(new vp_F[m]);
    }
    run_pool([&](const Range &r) {
        const layer &L = C.circuit[r.layer];
        Flat &f = flat[r.layer];
        const bool has_c = any_c[r.layer];
        for (u64 g = r.b; g < r.e; ++g) {
            const gate &G = L.gates[g];
            f.ty[g] = (uint8_t) G.ty; f.l[g] = G.l;
            f.u[g] = r.layer == 0 ? 0u : (uint32_t) G.u;      // layer 0: u carries the input value, not an index
            f.v[g] = (uint32_t) G.v; f.lv[g] = (uint32_t) G.lv;
            f.as[g] = G.is_assert ? 1 : 0;
            if (has_c) { f.c[g].real = G.c.real; f.c[g].img = G.c.img; }
        }
    });
    {   // the subset lists (u64 in the reference's layout) -> u32, one layer per task
        std::atomic<int> next{0};
        auto work = [&]() {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n) return;
                const layer &L = C.circuit[i];
                Flat &f = flat[i];
                f.did.resize(L.dadId.size());
                for (size_t j = 0; j < L.dadId.size(); ++j) f.did[j].assign(L.dadId[j].begin(), L.dadId[j].end());
            }
        };
        const unsigned nt = std::max(1u, std::min<unsigned>(std::min(16u, std::thread::hardware_concurrency()), (unsigned) n));
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
    for (int i = 0; i < n; ++i) {
        const layer &L = C.circuit[i];
        Flat &f = flat[i];
        f.dsz.assign(L.dadSize.begin(), L.dadSize.end());
        f.dbl.assign(L.dadBitLength.begin(), L.dadBitLength.end());
        f.dptr.resize(L.dadId.size());
        for (size_t j = 0; j < L.dadId.size(); ++j) f.dptr[j] = f.did[j].data();
        vp_layer_desc &d = desc[i];
        d.size = L.size; d.bit_length = L.bitLength;
        d.ty = f.ty.get(); d.l = f.l.get(); d.u = f.u.get(); d.v = f.v.get(); d.lv = f.lv.get();
        d.c = any_c[i] ? f.c.get() : nullptr;
        d.is_assert = any_as[i] ? f.as.get() : nullptr;
        d.dad_size = f.dsz.data(); d.dad_bitlen = f.dbl.data(); d.dad_id = f.dptr.data();
    }
    // the destructor of a partially constructed object never runs: release the context (streams, pinned buffers, the circuit and
    // witness in HBM) before the exception leaves, e.g. when evaluate() reports a violated assert gate (VP_EASSERT)
    try {
        const double t0 = since();
        for (vp_ctx *c : rk) {
            const int rc = vp_circuit_upload(c, n, desc.data());
            if (rc != VP_OK) throw std::runtime_error("vp_circuit_upload failed (" + std::to_string(rc) + "): " + vp_last_error(c));
        }
        const double t1 = since();
        evaluate();
        if (dbg) fprintf(stderr, "[vp upload] flatten %.3f s  vp_circuit_upload %.3f s  evaluate %.3f s\n", t0, t1 - t0, since() - t1);
    } catch (...) {
        pool.reset();
        for (vp_ctx *c : rk) vp_destroy(c);
        rk.clear();
        ctx = nullptr;
        throw;
    }
}

prover::~prover() {
    pool.reset();
    for (vp_ctx *c : rk) vp_destroy(c);
}

void prover::evaluate() {      // src/prover.cpp:27-91
    const layer &L0 = C.circuit[0];
    std::vector<vp_F> in(L0.size);
    for (u64 g = 0; g < L0.size; ++g) { F x((long long) L0.gates[g].u); in[g].real = x.real; in[g].img = x.img; }
    onRanks([&](int, vp_ctx *c) { return vp_evaluate(c, in.data(), in.size()); }, "vp_evaluate");
}

void prover::init() {          // src/prover.cpp:131-155
    int max_bl = 0;
    for (auto &c : C.circuit) max_bl = std::max(max_bl, c.bitLength);
    r_u.assign(max_bl, F_ZERO);
    r_liu.assign(max_bl, F_ZERO);
    r_v.assign(C.size, std::vector<F>());
    for (int i = 1; i < C.size; ++i)
        if (C.circuit[i].maxDadBitLength != -1) r_v[i].assign(C.circuit[i].maxDadBitLength, F_ZERO);
}

F prover::Vres(const std::vector<F>::const_iterator &r_0, int r_0_size) {       // src/prover.cpp:99-129
    prove_timer.start();
    F out;
    // every rank (one small launch): it also starts each rank's log of round stats afresh; rank 0's value is the message
    onRanks([&](int r, vp_ctx *c) { F o; const int rc = vp_vres(c, r_0_size ? cF(&*r_0) : nullptr, r_0_size, mF(&o)); if (r == 0) out = o; return rc; }, "vp_vres");
    prove_timer.stop();
    return out;
}

void prover::sumcheckInitAll(const std::vector<F>::const_iterator &r_last) {     // src/prover.cpp:162-170
    prove_timer.start();
    const int last_bl = C.circuit[C.size - 1].bitLength;
    sumcheckLayerId = C.size;
    for (int i = 0; i < last_bl; ++i) r_liu[i] = r_last[i];
    prove_timer.stop();
}

void prover::sumcheckInit() { --sumcheckLayerId; }                               // src/prover.cpp:177-184

void prover::sumcheckInitPhase1(const F &assert_random) {                        // src/prover.cpp:189-280
    prove_timer.start();
    init_timer.start();
    onRanks([&](int, vp_ctx *c) { return vp_phase1_init(c, sumcheckLayerId, cF(r_liu.data()), cF(&assert_random)); }, "vp_phase1_init");
    init_timer.stop();
    round = 0;
    prove_timer.stop();
}

void prover::sumcheckInitPhase2() {                                              // src/prover.cpp:282-367
    prove_timer.start();
    init_timer.start();
    onRanks([&](int, vp_ctx *c) { return vp_phase2_init(c, sumcheckLayerId, cF(r_u.data())); }, "vp_phase2_init");
    init_timer.stop();
    round = 0;
    prove_timer.stop();
}

void prover::sumcheckInitLiu(std::vector<F>::const_iterator s) {                 // src/prover.cpp:369-420
    prove_timer.start();
    std::vector<const vp_F *> rv(C.size, nullptr);
    for (int k = sumcheckLayerId; k < C.size; ++k) if (!r_v[k].empty()) rv[k] = cF(r_v[k].data());
    init_timer.start();
    onRanks([&](int, vp_ctx *c) { return vp_liu_init(c, sumcheckLayerId, cF(r_u.data()), rv.data(), cF(&*s)); }, "vp_liu_init");
    init_timer.stop();
    round = 0;
    prove_timer.stop();
}

quadratic_poly prover::sumcheckUpdate(const F &previous_random, std::vector<F> &r_arr) {   // src/prover.cpp:436-455
    prove_timer.start();
    if (round) r_arr.at(round - 1) = previous_random;
    ++round;
    F p[3];
    static const bool dbg_rounds = getenv("VP_DEBUG_ROUNDS") != nullptr;      // development aid: per-message latency on stderr
    const auto t_dbg = std::chrono::steady_clock::now();
    round_timer.start();
    if (rk.size() <= 1) check(vp_round(ctx, cF(&previous_random), mF(p)), "vp_round");
    else {
        std::vector<std::array<F, 3>> part(rk.size());
        auto call = [&](int r, vp_ctx *c) { return vp_round(c, cF(&previous_random), mF(part[r].data())); };
        if (onRanks(call, "vp_round") == VP_EXCHANGE) {         // every rank stopped at the gather of its split tables: exchange, same challenge again
            gather_timer.start();
            check(vp_shard_exchange_local(rk.data(), (int) rk.size()), "vp_shard_exchange_local");
            gather_timer.stop();
            if (onRanks(call, "vp_round") != VP_OK) throw std::runtime_error("vp_round: gather still pending after the exchange");
        }
        p[0] = p[1] = p[2] = F_ZERO;
        for (size_t r = 0; r < rk.size(); ++r) {
            part_log.push_back(part[r]);
            if ((int) r == drop_rank) continue;
            for (int q = 0; q < 3; ++q) p[q] = p[q] + part[r][q];
        }
    }
    round_timer.stop();
    if (dbg_rounds) fprintf(stderr, "[round] layer %d round %d: %.2f us\n", sumcheckLayerId, round, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_dbg).count());
    prove_timer.stop();
    proof_size += sizeof(F) * 3;
    return quadratic_poly(p[0], p[1], p[2]);
}
quadratic_poly prover::sumcheckUpdatePhase1(const F &r) { return sumcheckUpdate(r, r_u); }
quadratic_poly prover::sumcheckUpdatePhase2(const F &r) { return sumcheckUpdate(r, r_v[sumcheckLayerId]); }
quadratic_poly prover::sumcheckLiuUpdate(const F &r) { return sumcheckUpdate(r, r_liu); }

void prover::sumcheckFinalize1(const F &previousRandom, F &claim) {              // src/prover.cpp:494-501
    prove_timer.start();
    if (round) r_u[round - 1] = previousRandom;
    fin_timer.start();
    finalizeAll(previousRandom, &claim, 1, "vp_finalize");
    fin_timer.stop();
    prove_timer.stop();
    proof_size += sizeof(F);
}

void prover::sumcheckFinalize2(const F &previousRandom, std::vector<F>::iterator claims) {   // src/prover.cpp:504-516
    prove_timer.start();
    if (round) r_v[sumcheckLayerId][round - 1] = previousRandom;
    std::vector<F> tmp(sumcheckLayerId);
    fin_timer.start();
    finalizeAll(previousRandom, tmp.data(), sumcheckLayerId, "vp_finalize");
    fin_timer.stop();
    for (int i = 0; i < sumcheckLayerId; ++i) claims[i] = tmp[i];
    proof_size += sizeof(F) * sumcheckLayerId;
    prove_timer.stop();
}

void prover::sumcheckLiuFinalize(const F &previousRandom, F &claim) {            // src/prover.cpp:518-521
    if (round) r_liu[round - 1] = previousRandom;
    fin_timer.start();
    finalizeAll(previousRandom, &claim, 1, "vp_finalize");
    fin_timer.stop();
}

// every rank finalizes; a round-sharded proof's ranks must agree on every claim
void prover::finalizeAll(const F &previousRandom, F *claims, int n, const char *what) {
    if (rk.size() <= 1) { check(vp_finalize(ctx, cF(&previousRandom), mF(claims), n), what); return; }
    std::vector<std::vector<F>> cl(rk.size(), std::vector<F>(std::max(1, n)));
    onRanks([&](int r, vp_ctx *c) { return vp_finalize(c, cF(&previousRandom), mF(cl[r].data()), n); }, what);
    for (size_t r = 1; r < rk.size(); ++r)
        for (int q = 0; q < n; ++q)
            if (cl[r][q] != cl[0][q]) throw std::runtime_error(std::string(what) + ": rank " + std::to_string(r) + " returned a different claim than rank 0");
    for (int q = 0; q < n; ++q) claims[q] = cl[0][q];
}

void prover::pcRanks(const std::function<int(int, vp_ctx *)> &fn, const char *what) {
    for (int pass = 0; pass < 8; ++pass) {                 // no call of the commitment stops at more than two collectives
        if (onRanks(fn, what) == VP_OK) return;
        check(vp_shard_exchange_local(rk.data(), (int) rk.size()), "vp_shard_exchange_local");
    }
    throw std::runtime_error(std::string(what) + ": still at a collective after its exchanges");
}
namespace {
struct PubOut { prover::hhash_digest d; F inner; std::vector<F> all = std::vector<F>(65); };
// root_h, input_0 and all_sum of a sharded commit_public: the ranks must agree
void same_public(const std::vector<PubOut> &o, const char *what) {
    for (size_t r = 1; r < o.size(); ++r)
        if (memcmp(o[r].d.b, o[0].d.b, 32) || o[r].inner != o[0].inner || o[r].all != o[0].all)
            throw std::runtime_error(std::string(what) + ": rank " + std::to_string(r) + " returned a different root_h / input_0 / all_sum than rank 0");
}
void same_roots(const std::vector<std::vector<prover::hhash_digest>> &d, const char *what) {
    for (size_t r = 1; r < d.size(); ++r)
        if (memcmp(d[r].data(), d[0].data(), d[0].size() * sizeof(prover::hhash_digest)))
            throw std::runtime_error(std::string(what) + ": rank " + std::to_string(r) + " returned a different root than rank 0");
}
}  // namespace

prover::hhash_digest prover::commit_private() {      // src/prover.cpp:524-530 (mask = one zero element)
    masked = false;
    if (shard_pc) {
        std::vector<std::vector<hhash_digest>> d(rk.size(), std::vector<hhash_digest>(1));
        pcRanks([&](int r, vp_ctx *c) { return vp_commit_private(c, d[r][0].b); }, "vp_commit_private");
        same_roots(d, "vp_commit_private");
        return d[0][0];
    }
    hhash_digest d;
    check(vp_commit_private(ctx, d.b), "vp_commit_private");
    return d;
}
prover::hhash_digest prover::commit_public(std::vector<F> &pub, F &inner_product_sum, std::vector<F> &all_sum) {
    hhash_digest d;
    all_sum.resize(65);
    if (shard_pc) {
        std::vector<PubOut> o(rk.size());
        pcRanks([&](int r, vp_ctx *c) { return vp_commit_public(c, cF(pub.data()), pub.size(), mF(&o[r].inner), mF(o[r].all.data()), o[r].d.b); }, "vp_commit_public");
        same_public(o, "vp_commit_public");
        inner_product_sum = o[0].inner; all_sum = o[0].all;
        return o[0].d;
    }
    check(vp_commit_public(ctx, cF(pub.data()), pub.size(), mF(&inner_product_sum), mF(all_sum.data()), d.b), "vp_commit_public");
    return d;
}
static bool all_zero(const std::vector<F> &v) { for (auto &x : v) if (x.real | x.img) return false; return true; }
prover::hhash_digest prover::commit_private(const std::vector<F> &mask) {      // poly_commit.h:41-124 with its mask argument
    if (mask.empty() || all_zero(mask)) { masked = false; return commit_private(); }
    hhash_digest d;
    // (on a sharded commitment the library refuses the mask: its message is the exception's)
    check(vp_commit_private_masked(ctx, cF(mask.data()), mask.size(), d.b), "vp_commit_private_masked");
    masked = true;
    return d;
}
prover::hhash_digest prover::commit_public(std::vector<F> &pub, F &inner_product_sum, std::vector<F> &mask, std::vector<F> &all_sum) {      // src/prover.cpp:542-546
    if (!masked) return commit_public(pub, inner_product_sum, all_sum);      // behind a zero private mask the public mask's slice is multiplied by zero everywhere
    hhash_digest d;
    all_sum.resize(65);
    std::vector<F> one_zero(1, F_ZERO);
    const std::vector<F> &m = mask.empty() ? one_zero : mask;
    check(vp_commit_public_masked(ctx, cF(pub.data()), pub.size(), cF(m.data()), m.size(), mF(&inner_product_sum), mF(all_sum.data()), d.b), "vp_commit_public_masked");
    return d;
}
std::vector<F> prover::friFinalMask() {
    std::vector<F> out(32);
    check(vp_fri_final_mask(ctx, mF(out.data())), "vp_fri_final_mask");
    return out;
}
prover::hhash_digest prover::commit_public_eq(const std::vector<F> &point, F &inner_product_sum, std::vector<F> &all_sum) {
    hhash_digest d;
    all_sum.resize(65);
    if (shard_pc) {
        std::vector<PubOut> o(rk.size());
        pcRanks([&](int r, vp_ctx *c) { return vp_commit_public_eq(c, cF(point.data()), (int) point.size(), mF(&o[r].inner), mF(o[r].all.data()), o[r].d.b); }, "vp_commit_public_eq");
        same_public(o, "vp_commit_public_eq");
        inner_product_sum = o[0].inner; all_sum = o[0].all;
        return o[0].d;
    }
    check(vp_commit_public_eq(ctx, cF(point.data()), (int) point.size(), mF(&inner_product_sum), mF(all_sum.data()), d.b), "vp_commit_public_eq");
    return d;
}
prover::hhash_digest prover::commit_public_eq(const std::vector<F> &point, const std::vector<F> &mask, F &inner_product_sum, std::vector<F> &all_sum) {
    if (!masked) return commit_public_eq(point, inner_product_sum, all_sum);      // behind a zero private mask the public mask's slice is multiplied by zero everywhere
    hhash_digest d;
    all_sum.resize(65);
    std::vector<F> one_zero(1, F_ZERO);
    const std::vector<F> &m = mask.empty() ? one_zero : mask;
    check(vp_commit_public_eq_masked(ctx, cF(point.data()), (int) point.size(), cF(m.data()), m.size(), mF(&inner_product_sum), mF(all_sum.data()), d.b), "vp_commit_public_eq_masked");
    return d;
}
void prover::logLaunches() {
    if (!log_launches) return;
    int n = 0;
    if (vp_get_launch_stats(ctx, nullptr, 0, &n) != VP_OK || n <= 0) return;
    std::vector<vp_launch_stat> t((size_t) n);
    if (vp_get_launch_stats(ctx, t.data(), n, &n) == VP_OK) verifier_launches_.insert(verifier_launches_.end(), t.begin(), t.end());
}
std::vector<F> prover::predicates(int layer, const std::vector<F> &r_g, const F &assert_random, const std::vector<F> &r_u,
                                  const std::vector<F> &r_v, int n_v) {
    std::vector<F> out(5 + 7 * (size_t) layer);
    check(vp_predicates(ctx, layer, cF(r_g.data()), cF(&assert_random), cF(r_u.data()), n_v ? cF(r_v.data()) : nullptr, n_v,
                        mF(out.data()), out.size()), "vp_predicates");
    logLaunches();
    return out;
}
F prover::liuGr(int layer, const std::vector<F> &ru, const std::vector<std::vector<F>> &rv_all, const std::vector<F> &sig, const std::vector<F> &rliu) {
    std::vector<const vp_F *> rv(C.size, nullptr);
    for (int k = layer; k < C.size; ++k) if (!rv_all[k].empty()) rv[k] = cF(rv_all[k].data());
    F out;
    check(vp_liu_gr(ctx, layer, cF(ru.data()), rv.data(), cF(sig.data()), cF(rliu.data()), mF(&out)), "vp_liu_gr");
    logLaunches();
    return out;
}
F prover::layerMle(int layer, const std::vector<F> &r, int n) {
    F out;
    check(vp_layer_mle(ctx, layer, n ? cF(r.data()) : nullptr, n, mF(&out)), "vp_layer_mle");
    logLaunches();
    return out;
}
std::vector<F> prover::pcPublicEvals(int n, const std::vector<F> &point, const std::vector<u64> &leaf0) {
    std::vector<F> out(leaf0.size() * 128);
    static_assert(sizeof(u64) == sizeof(uint64_t), "leaf indices are passed as they are");
    check(vp_pc_public_evals(ctx, n, cF(point.data()), nullptr, (int) leaf0.size(), reinterpret_cast<const uint64_t *>(leaf0.data()), mF(out.data())), "vp_pc_public_evals");
    logLaunches();
    return out;
}
std::vector<F> prover::pcPublicEvalsPub(int n, const std::vector<F> &pub, const std::vector<u64> &leaf0) {
    if (n < 0 || n > 30 || pub.size() != (1ull << n)) throw std::invalid_argument("pcPublicEvalsPub: a public vector of 2^n entries");
    std::vector<F> out(leaf0.size() * 128);
    check(vp_pc_public_evals(ctx, n, nullptr, cF(pub.data()), (int) leaf0.size(), reinterpret_cast<const uint64_t *>(leaf0.data()), mF(out.data())), "vp_pc_public_evals");
    logLaunches();
    return out;
}
std::vector<uint8_t> prover::pcOpeningDigests(int n, const std::vector<u64> &leaf0, const uint8_t *answer, u64 n_bytes) {
    std::vector<uint8_t> out(leaf0.size() * (size_t) std::max(0, n - 4) * 64);
    check(vp_fri_query_digests(ctx, n, (int) leaf0.size(), reinterpret_cast<const uint64_t *>(leaf0.data()), answer, n_bytes, out.data()), "vp_fri_query_digests");
    logLaunches();
    return out;
}
std::vector<F> prover::pcMaskEvals(int n, const std::vector<F> &pub_mask, u64 ms, const std::vector<u64> &leaf0) {
    std::vector<F> out(leaf0.size() * 2);
    check(vp_pc_mask_evals(ctx, n, cF(pub_mask.data()), pub_mask.size(), ms, (int) leaf0.size(), reinterpret_cast<const uint64_t *>(leaf0.data()), mF(out.data())), "vp_pc_mask_evals");
    logLaunches();
    return out;
}
u64 prover::fsGrind(const vph::hhash_digest &state, int bits, bool on_device) {
    if (bits < 1 || bits > PCFS_POW_PROVER_BITS) throw std::invalid_argument("fsGrind: 1 .. 32 bits");
    const uint64_t tries = 64ull << bits;
    uint64_t nonce = 0;
    if (!on_device) {
        if (!vph::fs_grind(state, bits, 0, tries, &nonce)) throw std::runtime_error("proof of work: no nonce below 64 x 2^" + std::to_string(bits) + " meets " + std::to_string(bits) + " bits");
        return nonce;
    }
    uint8_t st_in[32], st_out[32];
    memcpy(st_in, state.w, 32);
    const int rc = vp_fs_grind(ctx, st_in, bits, 0, tries, &nonce, st_out);
    if (rc == VP_ELIMIT) throw std::runtime_error("proof of work: no nonce below 64 x 2^" + std::to_string(bits) + " meets " + std::to_string(bits) + " bits");
    check(rc, "vp_fs_grind");
    // the host's step on the device's nonce: the work is met and the state is the chain's
    vph::fs_chain ch;
    ch.s = state;
    if (!ch.work((u64) bits, nonce) || memcmp(ch.s.w, st_out, 32)) throw std::runtime_error("vp_fs_grind: the nonce or the state behind it is not the chain's");
    return nonce;
}
std::vector<uint8_t> prover::commitFS(const std::vector<F> &point, int reps, const std::vector<F> &pri_mask, const std::vector<F> &pub_mask, bool device_draws, int pow_bits) {
    if (shard_pc) throw std::runtime_error("commitFS: not built for a sharded commitment");
    if (pow_bits < 0 || pow_bits > PCFS_POW_PROVER_BITS) throw std::invalid_argument("commitFS: pow_bits outside 0 .. 32");
    const int n = C.circuit[0].bitLength, ln = n - 6;
    if (n < 7 || (int) point.size() != n) throw std::runtime_error("commitFS: a point of n >= 7 coordinates, n the input layer's bit length");
    if (reps < 1 || reps > 4096) throw std::runtime_error("commitFS: 1 .. 4096 repetitions");
    const hhash_digest root_l = commit_private(pri_mask);
    u64 ms = 1;
    if (masked) {                                          // the padded length is public: M / the largest power of two <= M / length (poly_commit.h:55-63)
        const u64 M = 1ull << (n - 1);
        u64 gap = 1;
        while (gap * 2 <= M / pri_mask.size()) gap *= 2;
        ms = M / gap;
    }
    const std::vector<F> pm = masked ? pub_mask : std::vector<F>();
    F claim;
    std::vector<F> all_sum;
    const hhash_digest root_h = commit_public_eq(point, pm, claim, all_sum);
    vph::fs_chain ch;
    pcFsAbsorbHead(ch, n, (u64) reps, ms, point, pm, claim, root_l.b, root_h.b, all_sum);
    std::vector<uint8_t> roots(32 * (size_t) ln);
    std::vector<F> fr((size_t) ln);
    fs_phase_ms = 0;
    const auto t0 = std::chrono::high_resolution_clock::now();
    if (device_draws) {
        uint8_t st_in[32], st_out[32];
        memcpy(st_in, ch.s.w, 32);
        check(vp_fri_commit_fs(ctx, st_in, roots.data(), mF(fr.data()), st_out), "vp_fri_commit_fs");
        fs_phase_sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        fs_phase_ms = commitDeviceMs();
        // the host's chain over the returned roots: the device's challenges and closing state must be its own
        F r = pcFsFirstChallenge(ch);
        for (int k = 0; k < ln; ++k) {
            if (memcmp(&r, &fr[k], sizeof(F))) throw std::runtime_error("vp_fri_commit_fs: challenge " + std::to_string(k) + " is not the chain's");
            pcFsLevel(ch, k, ln, &roots[32 * (size_t) k], &r);
        }
        if (memcmp(ch.s.w, st_out, 32)) throw std::runtime_error("vp_fri_commit_fs: the closing state is not the chain's");
    } else {
        F r = pcFsFirstChallenge(ch);
        for (int k = 0; k < ln; ++k) {
            fr[k] = r;
            const hhash_digest d = friStep(r);
            fs_phase_ms += commitDeviceMs();
            memcpy(&roots[32 * (size_t) k], d.b, 32);
            pcFsLevel(ch, k, ln, d.b, &r);
        }
        fs_phase_sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    }
    const std::vector<F> fin = friFinal(), fm = friFinalMask();
    PcFsWork work;
    work.bits = (u64) pow_bits;
    work.find = [&](const vph::hhash_digest &st) { return fsGrind(st, pow_bits, device_draws); };
    const std::vector<u64> lf = pcFsPositions(ch, n, (u64) reps, fin, fm, &work);
    const std::vector<uint8_t> ans = friQuery(lf);
    std::vector<uint8_t> out;
    auto put = [&](const void *b, size_t k) { const uint8_t *q = static_cast<const uint8_t *>(b); out.insert(out.end(), q, q + k); };
    const uint32_t h32[4] = {PCFS_MAGIC, pow_bits ? PCFS_VERSION_POW : PCFS_VERSION, (uint32_t) n, (uint32_t) reps};
    const uint64_t h64[2] = {ms, ms == 1 ? 0 : pm.size()};
    put(h32, sizeof h32); put(h64, sizeof h64);
    if (pow_bits) { const uint64_t hw[2] = {work.bits, work.nonce}; put(hw, sizeof hw); }
    put(point.data(), point.size() * sizeof(F));
    if (ms != 1) put(pm.data(), pm.size() * sizeof(F));
    put(&claim, sizeof(F));
    put(root_l.b, 32); put(root_h.b, 32);
    put(all_sum.data(), 65 * sizeof(F));
    put(roots.data(), roots.size());
    put(fin.data(), fin.size() * sizeof(F));
    put(fm.data(), fm.size() * sizeof(F));
    put(ans.data(), ans.size());
    return out;
}
void prover::friCommitFS(vph::fs_chain &ch, std::vector<uint8_t> &roots) {
    if (shard_pc) throw std::runtime_error("friCommitFS: not built for a sharded commitment");
    const int ln = C.circuit[0].bitLength - 6;
    roots.assign(32 * (size_t) ln, 0);
    std::vector<F> fr((size_t) ln);
    uint8_t st_in[32], st_out[32];
    memcpy(st_in, ch.s.w, 32);
    check(vp_fri_commit_fs(ctx, st_in, roots.data(), mF(fr.data()), st_out), "vp_fri_commit_fs");
    F r = pcFsFirstChallenge(ch);
    for (int k = 0; k < ln; ++k) {
        if (memcmp(&r, &fr[k], sizeof(F))) throw std::runtime_error("vp_fri_commit_fs: challenge " + std::to_string(k) + " is not the chain's");
        pcFsLevel(ch, k, ln, &roots[32 * (size_t) k], &r);
    }
    if (memcmp(ch.s.w, st_out, 32)) throw std::runtime_error("vp_fri_commit_fs: the closing state is not the chain's");
}
prover::hhash_digest prover::friStep(const F &r) {
    hhash_digest d;
    if (shard_pc) {
        std::vector<std::vector<hhash_digest>> ds(rk.size(), std::vector<hhash_digest>(1));
        pcRanks([&](int q, vp_ctx *c) { return vp_fri_step(c, cF(&r), ds[q][0].b); }, "vp_fri_step");
        fri_one_pass = false;
        same_roots(ds, "vp_fri_step");
        return ds[0][0];
    }
    check(vp_fri_step(ctx, cF(&r), d.b), "vp_fri_step");
    return d;
}
std::vector<prover::hhash_digest> prover::friCommit(const std::vector<F> &r) {
    std::vector<hhash_digest> d(r.size());
    if (shard_pc) {
        std::vector<std::vector<hhash_digest>> ds(rk.size(), std::vector<hhash_digest>(std::max<size_t>(1, r.size())));
        pcRanks([&](int q, vp_ctx *c) { return vp_fri_commit(c, cF(r.data()), (int) r.size(), ds[q][0].b); }, "vp_fri_commit");
        fri_one_pass = true;
        same_roots(ds, "vp_fri_commit");
        ds[0].resize(r.size());
        return ds[0];
    }
    check(vp_fri_commit(ctx, cF(r.data()), (int) r.size(), d[0].b), "vp_fri_commit");
    return d;
}
std::vector<F> prover::friFinal() {
    std::vector<F> out(2048);
    if (shard_pc) {                                         // the last codeword is whole on every rank
        std::vector<std::vector<F>> o(rk.size(), std::vector<F>(2048));
        onRanks([&](int r, vp_ctx *c) { return vp_fri_final(c, mF(o[r].data())); }, "vp_fri_final");
        for (size_t r = 1; r < o.size(); ++r) if (o[r] != o[0]) throw std::runtime_error("vp_fri_final: rank " + std::to_string(r) + " returned a different codeword than rank 0");
        return o[0];
    }
    check(vp_fri_final(ctx, mF(out.data())), "vp_fri_final");
    return out;
}
void prover::friOpen(int oracle, u64 leaf, std::vector<F> &values, std::vector<hhash_digest> &path) {
    values.resize(130);
    path.resize(40);
    int len = 0;
    vp_ctx *who = ctx;
    if (shard_pc) { const int owner = vp_pc_shard_owner(ctx, oracle, leaf); who = rk[owner < 0 ? 0 : owner]; }      // -1: a replicated level, any rank answers
    const int rc = vp_fri_open(who, oracle, leaf, mF(values.data()), path[0].b, 40 * 32, &len);
    if (rc != VP_OK) throw std::runtime_error("vp_fri_open failed (" + std::to_string(rc) + "): " + vp_last_error(who));
    path.resize(len);
}
void prover::friOpenMany(const std::vector<int32_t> &oracle, const std::vector<u64> &leaf, std::vector<F> &values, std::vector<hhash_digest> &paths, int stride,
                         std::vector<int32_t> &path_len) {
    if (oracle.size() != leaf.size()) throw std::runtime_error("friOpenMany: oracle and leaf lists differ in length");
    const size_t n = oracle.size();
    values.resize(130 * n); paths.resize((size_t) stride * n); path_len.assign(n, 0);
    if (!n) return;
    std::vector<uint64_t> lf(leaf.begin(), leaf.end());
    if (shard_pc) {
        // every rank answers what it owns into buffers of its own; a request's answer is taken from a rank that reports a path for it
        struct Ans { std::vector<F> v; std::vector<hhash_digest> p; std::vector<int32_t> len; };
        std::vector<Ans> a(rk.size());
        for (auto &x : a) { x.v.resize(130 * n); x.p.resize((size_t) stride * n); x.len.assign(n, 0); }
        onRanks([&](int r, vp_ctx *c) { return vp_fri_open_many(c, (int) n, oracle.data(), lf.data(), mF(a[r].v.data()), a[r].p[0].b, 32 * stride, a[r].len.data()); },
                "vp_fri_open_many");
        for (size_t i = 0; i < n; ++i) {
            size_t r = 0;
            while (r < rk.size() && a[r].len[i] <= 0) ++r;
            if (r == rk.size()) throw std::runtime_error("vp_fri_open_many: no rank answered request " + std::to_string(i));
            std::copy(a[r].v.begin() + 130 * i, a[r].v.begin() + 130 * (i + 1), values.begin() + 130 * i);
            std::copy(a[r].p.begin() + (size_t) stride * i, a[r].p.begin() + (size_t) stride * i + a[r].len[i], paths.begin() + (size_t) stride * i);
            path_len[i] = a[r].len[i];
        }
        return;
    }
    check(vp_fri_open_many(ctx, (int) n, oracle.data(), lf.data(), mF(values.data()), paths[0].b, 32 * stride, path_len.data()), "vp_fri_open_many");
}
std::vector<uint8_t> prover::friQuery(const std::vector<u64> &leaf0) {
    if (shard_pc && fri_one_pass) {
        // after the one-pass friCommit a sharded commitment answers lists of openings only: the same requests in vp_fri_query's order through
        // friOpenMany, packed into its layout (values, then the path at its true length)
        const int n = C.circuit[0].bitLength, ln = n - 6;
        std::vector<int32_t> oracle, len;
        std::vector<u64> leaf;
        for (u64 l0 : leaf0) {
            oracle.push_back(0); leaf.push_back(l0);
            oracle.push_back(1); leaf.push_back(l0);
            u64 D = 1ull << (n - 1), t = l0;
            for (int k = 0; k < ln; ++k) { const u64 Dn = D / 2, lf = t % (Dn / 2); oracle.push_back(2 + k); leaf.push_back(lf); t = lf; D = Dn; }
        }
        std::vector<F> values;
        std::vector<hhash_digest> paths;
        const int stride = n - 1;                           // digests of the longest path
        friOpenMany(oracle, leaf, values, paths, stride, len);
        std::vector<uint8_t> out;
        for (size_t i = 0; i < oracle.size(); ++i) {
            const uint8_t *v = reinterpret_cast<const uint8_t *>(values.data() + 130 * i);
            out.insert(out.end(), v, v + 130 * sizeof(F));
            out.insert(out.end(), paths[(size_t) stride * i].b, paths[(size_t) stride * i].b + 32 * (size_t) len[i]);
        }
        return out;
    }
    uint64_t bytes = 0, written = 0;
    check(vp_fri_query_bytes(ctx, (int) leaf0.size(), &bytes), "vp_fri_query_bytes");
    std::vector<uint8_t> out(bytes);
    std::vector<uint64_t> lf(leaf0.begin(), leaf0.end());
    if (shard_pc) {
        // the layout is the same on every rank and a rank fills in the openings it owns: walk the requests in vp_fri_query's order (host/verifier.cpp's
        // leaf chain) and take each opening from its owner's buffer
        std::vector<std::vector<uint8_t>> o(rk.size(), std::vector<uint8_t>(bytes));
        std::vector<uint64_t> wr(rk.size(), 0);
        onRanks([&](int r, vp_ctx *c) { return vp_fri_query(c, (int) lf.size(), lf.data(), o[r].data(), bytes, &wr[r]); }, "vp_fri_query");
        for (size_t r = 0; r < rk.size(); ++r) if (wr[r] != bytes) throw std::runtime_error("vp_fri_query: rank " + std::to_string(r) + " reports another answer size than vp_fri_query_bytes");
        const int n = C.circuit[0].bitLength, ln = n - 6;
        size_t at = 0;
        auto take = [&](int oracle, uint64_t leaf, int path_digests) {
            const int owner = vp_pc_shard_owner(ctx, oracle, leaf);
            const size_t len = 130 * sizeof(F) + 32 * (size_t) path_digests;
            if (at + len > bytes) throw std::runtime_error("vp_fri_query: the answer is shorter than its layout");
            memcpy(out.data() + at, o[owner < 0 ? 0 : owner].data() + at, len);
            at += len;
        };
        for (uint64_t l0 : lf) {
            take(0, l0, n - 1); take(1, l0, n - 1);
            uint64_t D = 1ull << (n - 1), t = l0;
            for (int k = 0; k < ln; ++k) { const uint64_t Dn = D / 2, leaf = t % (Dn / 2); take(2 + k, leaf, n - 2 - k); t = leaf; D = Dn; }
        }
        if (at != bytes) throw std::runtime_error("vp_fri_query: the answer is longer than its layout");
        return out;
    }
    check(vp_fri_query(ctx, (int) lf.size(), lf.data(), out.data(), bytes, &written), "vp_fri_query");
    out.resize(written);
    return out;
}
std::vector<F> prover::fftGkr(int lg, const std::vector<F> &tape) {
    uint64_t nt = 0, nm = 0;
    check(vp_fft_gkr_sizes(lg, &nt, &nm), "vp_fft_gkr_sizes");
    if (tape.size() != nt) throw std::runtime_error("fftGkr: tape has the wrong length");
    std::vector<F> msgs(nm);
    uint64_t written = 0;
    check(vp_fft_gkr(ctx, lg, cF(tape.data()), nt, mF(msgs.data()), nm, &written), "vp_fft_gkr");
    msgs.resize(written);
    return msgs;
}
void prover::fftGkrBegin(int lg, const std::vector<F> &tape) {
    check(vp_fft_gkr_begin(ctx, lg, cF(tape.data()), tape.size()), "vp_fft_gkr_begin");
}
std::vector<F> prover::fftGkrEnd(int lg) {
    uint64_t nt = 0, nm = 0;
    check(vp_fft_gkr_sizes(lg, &nt, &nm), "vp_fft_gkr_sizes");
    std::vector<F> msgs(nm);
    uint64_t written = 0;
    check(vp_fft_gkr_end(ctx, mF(msgs.data()), nm, &written), "vp_fft_gkr_end");
    msgs.resize(written);
    return msgs;
}
void prover::fftGkrCancel() noexcept { (void) vp_fft_gkr_cancel(ctx); }
std::vector<F> prover::fftGkrFS(int lg, uint8_t state[32], std::vector<F> &tape) {
    uint64_t nt = 0, nm = 0;
    check(vp_fft_gkr_sizes(lg, &nt, &nm), "vp_fft_gkr_sizes");
    std::vector<F> msgs(nm);
    tape.assign(nt, F_ZERO);
    uint8_t st_out[32];
    uint64_t written = 0;
    check(vp_fft_gkr_fs(ctx, lg, state, mF(msgs.data()), nm, &written, mF(tape.data()), st_out), "vp_fft_gkr_fs");
    if (written != nm) throw std::runtime_error("vp_fft_gkr_fs: message count");
    vph::fs_chain ch;
    memcpy(ch.s.w, state, 32);
    std::vector<F> want(nt);
    vph::fftGkrFsTape(lg, ch, msgs.data(), want.data());
    for (uint64_t i = 0; i < nt; ++i)
        if (memcmp(&want[i], &tape[i], sizeof(F))) throw std::runtime_error("vp_fft_gkr_fs: tape slot " + std::to_string(i) + " is not the chain's");
    if (memcmp(ch.s.w, st_out, 32)) throw std::runtime_error("vp_fft_gkr_fs: the closing state is not the chain's");
    memcpy(state, st_out, 32);
    return msgs;
}
std::vector<uint8_t> prover::proveGkrFS(uint8_t state[32], std::vector<F> &tape, u64 &n_draws) {
    if (world() > 1) throw std::runtime_error("proveGkrFS: not built for a sharded session");
    const vph::GkrLayout L(C);
    u64 nt = 0, nb = 0;
    gkrSizes(nt, nb);
    if (nt != L.n_tape || nb != L.n_tr * sizeof(F)) throw std::runtime_error("proveGkrFS: the device's tape / transcript sizes are not the circuit's");
    std::vector<uint8_t> tr(nb);
    tape.assign(nt, F_ZERO);
    uint8_t st_out[32];
    uint64_t written = 0, draws = 0;
    prove_timer.start();
    const int rc = vp_prove_gkr_fs(ctx, state, tr.data(), nb, &written, mF(tape.data()), &draws, st_out);
    prove_timer.stop();
    check(rc, "vp_prove_gkr_fs");
    if (written != nb) throw std::runtime_error("vp_prove_gkr_fs: transcript size");
    std::vector<F> elems(L.n_tr), want(nt);
    memcpy(static_cast<void *>(elems.data()), tr.data(), nb);
    vph::fs_chain ch;
    memcpy(ch.s.w, state, 32);
    const u64 want_draws = vph::gkrFsTape(C, L, ch, elems.data(), want.data());
    for (u64 i = 0; i < nt; ++i)
        if (memcmp(&want[i], &tape[i], sizeof(F))) throw std::runtime_error("vp_prove_gkr_fs: tape slot " + std::to_string(i) + " is not the chain's");
    if (draws != want_draws) throw std::runtime_error("vp_prove_gkr_fs: the number of draws is not the schedule's");
    if (memcmp(ch.s.w, st_out, 32)) throw std::runtime_error("vp_prove_gkr_fs: the closing state is not the chain's");
    memcpy(state, st_out, 32);
    n_draws = draws;
    return tr;
}
double prover::commitDeviceMs() { double ms = 0; check(vp_commit_stats(ctx, &ms), "vp_commit_stats"); return ms; }

void prover::gkrSizes(u64 &n_tape, u64 &n_bytes) {
    uint64_t a = 0, b = 0;
    check(vp_gkr_sizes(ctx, &a, &b), "vp_gkr_sizes");
    n_tape = a; n_bytes = b;
}

void prover::proveGKR(const std::vector<F> &tape, std::vector<uint8_t> &transcript) {
    u64 nt, nb;
    gkrSizes(nt, nb);
    if (tape.size() != nt) throw std::runtime_error("proveGKR: tape has the wrong length");
    const size_t at = transcript.size();
    transcript.resize(at + nb);
    uint64_t written = 0;
    prove_timer.start();
    check(vp_prove_gkr(ctx, cF(tape.data()), nt, transcript.data() + at, nb, &written), "vp_prove_gkr");
    prove_timer.stop();
    transcript.resize(at + written);
}

std::vector<F> prover::layerValues(int layer) {
    std::vector<F> out(C.circuit[layer].size);
    check(vp_layer_values(ctx, layer, mF(out.data()), out.size()), "vp_layer_values");
    return out;
}

vp_stats prover::stats() {
    vp_stats s{};
    check(vp_get_stats(ctx, &s), "vp_get_stats");
    return s;
}
