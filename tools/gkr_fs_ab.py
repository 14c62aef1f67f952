#!/usr/bin/env python3
"""The GKR part with its challenges drawn on the device against the host-driven loop, alternated in one process:
    python tools/gkr_fs_ab.py BLOCKS RUNS [--host-runs K] [--cold]
On the SHA-256 x BLOCKS circuit: Session.prove_fs() against prove_fs(device_draws=True), and Session.prove_full_fs() against prove_full_fs(device_gkr=True), RUNS
times each in turn after one warm-up of each; host wall clock per run, and the device milliseconds of the new call (vp_prove_gkr_fs, HIP events).  Beside them
vp_prove_gkr on the tape the device drew, in the same run: the tape-form floor (the same sumchecks as one batched pass; it draws nothing).  The number of chain
steps (every transcript element absorbed once, every challenge drawn once) gives microseconds per step.
--host-runs K: the host-driven forms only in the first K runs (a host-driven proof of a large circuit takes most of a minute); --cold: no warm-up of the
host-driven forms.  The bytes of the two forms are compared on every run.  Prints markdown, each row as soon as it is measured."""
import gzip
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(blocks, runs, host_runs, cold):
    sys.path.insert(0, ROOT)
    import vp_loader
    vp = vp_loader.load()
    with tempfile.TemporaryDirectory() as tmp:
        pws = os.path.join(tmp, "s.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as o:
            o.write(f.read())
        c = vp.Circuit.from_pws(pws, blocks, seed=1)
    n_tape, n_bytes = c.gkr_sizes()
    s = vp.Session(c)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return out, 1e3 * (time.perf_counter() - t)

    tr, tape, draws, _ = s.prove_gkr_fs(bytes(32))
    steps = n_bytes // 16 + draws
    s.set_tape(tape)
    assert s.prove_gkr()[0] == tr, "vp_prove_gkr on the drawn tape gives other bytes"
    s.prove_fs(device_draws=True); s.prove_full_fs(device_gkr=True)
    if not cold:
        s.prove_fs(); s.prove_full_fs()
    print("## x%d (%d layers, transcript %d elements, %d draws: %d chain steps), %d alternated runs%s\n" % (blocks, c.layers, n_bytes // 16, draws, steps, runs,
                                                                                                           ", host-driven forms in the first %d" % host_runs if host_runs < runs else ""))
    print("| run | prove_fs host ms | prove_fs(device_draws) host ms | its device ms | us per chain step | vp_prove_gkr on that tape, device ms | prove_full_fs host ms | prove_full_fs(device_gkr) host ms |")
    print("|---|---|---|---|---|---|---|---|", flush=True)
    rows = []
    for i in range(runs):
        host = i < host_runs
        (p_h, _, _), t_h = timed(lambda: s.prove_fs()) if host else ((None, None, None), float("nan"))
        (p_d, res, _), t_d = timed(lambda: s.prove_fs(device_draws=True))
        assert p_h is None or p_h == p_d, "prove_fs: the two forms give other bytes"
        dev_ms = res["gkr_device_ms"]
        floor_ms = s.prove_gkr()[1]["gkr_device_ms"]
        f_h, tf_h = timed(lambda: s.prove_full_fs()) if host else (None, float("nan"))
        f_d, tf_d = timed(lambda: s.prove_full_fs(device_gkr=True))
        assert f_h is None or f_h == f_d, "prove_full_fs: the two forms give other bytes"
        rows.append((t_h, t_d, dev_ms, 1e3 * dev_ms / steps, floor_ms, tf_h, tf_d))
        print("| %d | %.2f | %.2f | %.3f | %.2f | %.3f | %.2f | %.2f |" % ((i,) + rows[-1]), flush=True)
    med = lambda k: statistics.median([r[k] for r in rows if r[k] == r[k]])
    spread = lambda k: max(r[k] for r in rows if r[k] == r[k]) - min(r[k] for r in rows if r[k] == r[k])
    print("\nmedian: prove_fs host-driven %.2f ms (spread %.2f), device draws %.2f ms (spread %.2f): %.1f x; device time %.3f ms = %.2f us per chain step, %.1f x the "
          "tape form's %.3f ms; prove_full_fs %.2f ms (spread %.2f) against %.2f ms (spread %.2f)\n"
          % (med(0), spread(0), med(1), spread(1), med(0) / med(1), med(2), med(3), med(2) / med(4), med(4), med(5), spread(5), med(6), spread(6)), flush=True)
    if not cold:
        assert c.verify_fs(p_d), "the device form's proof is rejected"
    s.close()
    c.close()


if __name__ == "__main__":
    argv, hr = sys.argv[1:], None
    if "--host-runs" in argv:
        k = argv.index("--host-runs")
        hr = int(argv[k + 1])
        del argv[k:k + 2]
    args = [a for a in argv if not a.startswith("--")]
    runs = int(args[1]) if len(args) > 1 else 5
    main(int(args[0]), runs, runs if hr is None else hr, "--cold" in argv)
