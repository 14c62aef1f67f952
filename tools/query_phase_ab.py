#!/usr/bin/env python3
"""Same-process A/B of the commitment's query phase:  python tools/query_phase_ab.py [BLOCKS ...]   (default: 1024 64)

Per size, in ONE process: the SHA-256 x BLOCKS circuit, one warm-up run of the complete protocol in each form, then
Session.prove_and_verify_full(reps=33) alternately with batched_openings off (one vp_fri_open per opening: a launch, two copies and a
synchronise each) and on (vp_fri_query: one launch, one copy, one synchronise), five times each, profiling off.  Prints pc_query_answer_sec of
every run, then — from one more batched run with vp_set_profiling(1) — the device time of the k_pc_open_many launch, the bytes it gathers and
the bytes the one copy moves, and whether every batched run was below the smallest one-by-one run.  Output is Markdown."""
import gzip
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, RUNS, RECORD_STRIDE = 33, 5, 130 * 16 + 26 * 32        # RECORD_STRIDE: sizeof(PcOpenRec), csrc/vp_kernels_pc.h


def main():
    sys.path.insert(0, ROOT)
    import vp_loader
    vp = vp_loader.load()
    vp.lib_host()
    sizes = [int(x) for x in sys.argv[1:]] or [1024, 64]
    print("# Query phase: one vp_fri_open per opening vs. one vp_fri_query (tools/query_phase_ab.py)\n")
    print("`pc_query_answer_sec` of `Session.prove_and_verify_full(reps=%d)`: host wall clock around the prover's answers to the verifier's queries." % REPS)
    print("Same process, same session, alternating, profiling off; one warm-up run of each form first.\n")
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
            for batched in (False, True):                        # warm-up
                tr, ok, _ = s.prove_and_verify_full(reps=REPS, batched_openings=batched)
                assert ok and (ref is None or tr == ref)
                ref = tr
            rec0 = s.last_full_record()
            t = {False: [], True: []}
            for _ in range(RUNS):
                for batched in (False, True):
                    tr, ok, times = s.prove_and_verify_full(reps=REPS, batched_openings=batched)
                    assert ok and tr == ref and s.last_full_record() == rec0
                    t[batched].append(times["pc_query_answer_sec"])
            s.set_profiling(1)
            _, ok, _ = s.prove_and_verify_full(reps=REPS, batched_openings=True)
            st = s.launch_stats()
            s.set_profiling(0)
            assert ok and [e["kernel"] for e in st] == ["k_pc_open_many"]
            n_open = REPS * (2 + n - 6)
            print("## SHA-256 x%d (n = %d, %d FRI levels, %d openings)\n" % (blocks, n, n - 6, n_open))
            print("| run | one by one (s) | batched (s) |\n|---|---|---|")
            for i in range(RUNS):
                print("| %d | %.6f | %.6f |" % (i + 1, t[False][i], t[True][i]))
            print("| min | %.6f | %.6f |\n| max | %.6f | %.6f |\n" % (min(t[False]), min(t[True]), max(t[False]), max(t[True])))
            print("- `k_pc_open_many`: 1 launch, %d workgroups, device time %.1f us, gathers %d bytes (= `vp_fri_query_bytes`)" % (st[0]["workgroups"], st[0]["us"], st[0]["bytes"]))
            print("- copied device to host: %d bytes (%d records of %d bytes), host to device: %d bytes (descriptor table + requests)"
                  % (n_open * RECORD_STRIDE, n_open, RECORD_STRIDE, 21 * 48 + 8 * n_open))
            held = max(t[True]) < min(t[False])
            verdicts.append(held)
            print("- every batched run below the smallest one-by-one run: **%s** (largest batched %.6f s, smallest one-by-one %.6f s, ratio of the minima %.1fx)\n"
                  % ("yes" if held else "NO", max(t[True]), min(t[False]), min(t[False]) / min(t[True])))
            s.close(); c.close()
    return 0 if all(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
