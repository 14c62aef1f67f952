#!/usr/bin/env python3
"""Same-process A/B of the complete protocol's verifier:  python tools/pc_verify_ab.py [BLOCKS ...]   (default: 64 1024)

Per size, in ONE process and ONE session: the SHA-256 x BLOCKS circuit, one warm-up run of the complete protocol in each mode, then
Session.prove_and_verify_full(reps=33) alternately in host mode (every verifier loop on one host core) and with device_verifier=True (wiring
predicates, public polynomial values and opening digests on the device; every comparison on the host), five times each, profiling off.  Prints
verify_sec of every run, the host mode's split into the GKR verifier's O(|C|) loops (wiring predicates, their final value, Liu gr: verifier::verifyTime) |
public evaluation | opening digests | the rest (timers around the factored functions, host/verifier.cpp), the device mode's split, and — from one more device-mode run with vp_set_profiling(1) — the device times of
k_pc_poly_eval (+ its closing launch) and k_pc_opening_digests with the evaluation kernel's F-multiply rate against DESIGN.md section 4's
7.0e11 / s and its bytes against HBM — for the protocol's own call (the point form: ONE row of coefficients) and for the same 33 positions on a
general vector of the same size (64 rows: the kernel under load, which is where a bound can be named).  The claim checked: every device-mode run is below the smallest host-mode run.  Output is Markdown."""
import gzip
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, RUNS = 33, 5
FMUL_PER_SEC, HBM_BYTES_PER_SEC = 7.0e11, 8.0e12         # measured chip-wide F_p^2 multiply rate; the HBM roofline bench.py uses
SPLIT = ("verify_predicates_sec", "verify_public_eval_sec", "verify_digests_sec", "verify_rest_sec")


def main():
    sys.path.insert(0, ROOT)
    import vp_loader
    vp = vp_loader.load()
    vp.lib_host()
    sizes = [int(x) for x in sys.argv[1:]] or [64, 1024]
    print("# The verifier's heavy loops: host vs. device (tools/pc_verify_ab.py)\n")
    print("`verify_sec` of `Session.prove_and_verify_full(reps=%d)`: host wall clock of the verifier's own work (GKR checks and predicates + the commitment's verifier)," % REPS)
    print("device calls included in device mode.  Same process, same session, alternating, profiling off; one warm-up run of each mode first.\n")
    verdicts = []
    with tempfile.TemporaryDirectory() as tmp:
        pws = os.path.join(tmp, "s.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as o:
            o.write(f.read())
        for blocks in sizes:
            c = vp.Circuit.from_pws(pws, blocks, seed=1)
            n = c.layer_bitlen(0)
            s = vp.Session(c)
            s.warm()
            ref = None
            for dev in (False, True):                            # warm-up
                tr, ok, _ = s.prove_and_verify_full(reps=REPS, device_verifier=dev)
                assert ok and (ref is None or tr == ref)
                ref = tr
            rec0 = s.last_full_record()
            t = {False: [], True: []}
            for _ in range(RUNS):
                for dev in (False, True):
                    tr, ok, times = s.prove_and_verify_full(reps=REPS, device_verifier=dev)
                    assert ok and tr == ref and s.last_full_record() == rec0
                    t[dev].append(times)
            s.set_profiling(1)
            _, ok, _ = s.prove_and_verify_full(reps=REPS, device_verifier=True)
            st = s.verifier_launch_stats()
            s.set_profiling(0)
            assert ok
            print("## SHA-256 x%d (n = %d, slices of 2^%d coefficients, %d openings)\n" % (blocks, n, n - 6, REPS * (n - 4)))
            print("| run | host mode verify_sec | device mode verify_sec |\n|---|---|---|")
            for i in range(RUNS):
                print("| %d | %.6f | %.6f |" % (i + 1, t[False][i]["verify_sec"], t[True][i]["verify_sec"]))
            v = {d: [x["verify_sec"] for x in t[d]] for d in t}
            print("| min | %.6f | %.6f |\n| max | %.6f | %.6f |\n" % (min(v[False]), min(v[True]), max(v[False]), max(v[True])))
            for d, name in ((False, "host"), (True, "device")):
                best = min(t[d], key=lambda x: x["verify_sec"])
                print("- %s mode, its fastest run: GKR predicate loops (wiring predicates, Liu gr) %.6f s | public evaluation %.6f s | opening digests %.6f s | the rest %.6f s"
                      % ((name,) + tuple(best[k] for k in SPLIT)))
            ev = [e for e in st if e["kernel"] == "k_pc_poly_eval"]
            fin = [e for e in st if e["kernel"] == "k_pc_poly_eval_fin"]
            dg = [e for e in st if e["kernel"] == "k_pc_opening_digests"]
            assert len(ev) == 1 and len(fin) == 1 and len(dg) == 1, [e["kernel"] for e in st]
            import numpy as np
            rng = np.random.default_rng(blocks)
            vec = rng.integers(0, (1 << 61) - 1, size=(1 << n, 2), dtype=np.uint64)
            lf = rng.integers(1 << (n - 7), 1 << (n - 2), size=REPS, dtype=np.uint64)
            s.pc_public_evals(lf, pub=vec)                       # warm-up (tables, first launches)
            s.set_profiling(1)
            s.pc_public_evals(lf, pub=vec)
            gen = [e for e in s.launch_stats() if e["kernel"] == "k_pc_poly_eval"]
            s.set_profiling(0)
            del vec
            assert len(gen) == 1
            for what, e in (("the protocol's call (point form, 1 row)", ev[0]), ("a general vector (64 rows), same positions", gen[0])):
                rate, bw = e["work"] / (e["us"] * 1e-6), e["bytes"] / (e["us"] * 1e-6)
                print("- `k_pc_poly_eval`, %s: 1 launch, %d workgroups, %.1f us, %d F-multiplications = %.3g / s (%.1f %% of %.1e / s), %d coefficient bytes = %.3g B/s (%.2f %% of HBM's %.1e B/s)"
                      % (what, e["workgroups"], e["us"], e["work"], rate, 100 * rate / FMUL_PER_SEC, FMUL_PER_SEC, e["bytes"], bw, 100 * bw / HBM_BYTES_PER_SEC, HBM_BYTES_PER_SEC))
            print("  - under load (64 rows) the nearer bound is **%s**; the protocol's one-row call is tens of microseconds of launch and dependent-chain latency, far from both"
                  % ("the multiplier" if rate / FMUL_PER_SEC > bw / HBM_BYTES_PER_SEC else "HBM"))
            print("- `k_pc_poly_eval_fin`: %.1f us; `k_pc_opening_digests`: 1 launch, %d single-wave workgroups, %.1f us for %d Keccak-f (%d openings)"
                  % (fin[0]["us"], dg[0]["workgroups"], dg[0]["us"], dg[0]["work"], dg[0]["jobs"]))
            held = max(v[True]) < min(v[False])
            verdicts.append(held)
            print("- every device-mode run below the smallest host-mode run: **%s** (largest device %.6f s, smallest host %.6f s, ratio of the minima %.1fx)\n"
                  % ("yes" if held else "NO", max(v[True]), min(v[False]), min(v[False]) / min(v[True])))
            s.close(); c.close()
    return 0 if all(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
