"""Round-sharded drop-in proof at x1024 on ONE GPU (include/vpgpu.h: vp_set_round_shard): wall time of the interactive proof with one context
against W = 4 and W = 8 ranks as contexts of the same GPU, the host time of the gathers, and the per-round fan-out overhead (round time of the
sharded prover minus the slowest rank's own vp_round time, per round).  No speedup is expected on one GPU: the ranks share its bandwidth.

    python tools/round_shard_x1024.py [--blocks 1024] [--reps 3] [--min-log 11] [--out FILE.json]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-log", type=int, default=11)
    ap.add_argument("--worlds", default="4,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import vp_loader
    vp = vp_loader.load()
    pws = os.path.join(tempfile.mkdtemp(), "SHA256_64.pws")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as g:
        g.write(f.read())
    c = vp.Circuit.from_pws(pws, a.blocks, seed=1)
    out = {"blocks": a.blocks, "min_log": a.min_log, "runs": []}

    def run(world):
        try:
            s = vp.Session(c) if world == 1 else vp.Session(c, devices=[0] * world, round_shard_min_log=a.min_log)
        except RuntimeError as e:                    # W whole circuits in one GPU's memory: the largest W may not fit
            rec = {"world": world, "error": str(e)}
            print(json.dumps(rec), flush=True)
            out["runs"].append(rec)
            return
        tr0, _, ok = s.prove_interactive()           # warm-up (first-touch allocations, resident kernel images)
        assert ok
        walls, rounds, gathers = [], [], []
        fan = []
        for _ in range(a.reps):
            g0 = s.gather_sec() if world > 1 else 0.0
            tr, res, ok = s.prove_interactive()
            assert ok and tr == tr0
            walls.append(res["prove_sec"]); rounds.append(res["round_sec"])
            gathers.append((s.gather_sec() - g0) if world > 1 else 0.0)
            if world > 1:
                st = [s.round_stats(rank=r) for r in range(world)]
                own = sum(max(st[r][i]["us"] for r in range(world)) for i in range(len(st[0]))) * 1e-6
                fan.append((res["round_sec"] - gathers[-1] - own) / max(1, len(st[0])) * 1e6)
        n_rounds = len(s.round_stats())
        s.close()
        rec = {"world": world, "prove_sec_median": statistics.median(walls), "round_sec_median": statistics.median(rounds),
               "rounds": n_rounds, "gather_sec_median": statistics.median(gathers)}
        if fan:
            rec["fanout_us_per_round_median"] = statistics.median(fan)
        print(json.dumps(rec), flush=True)
        out["runs"].append(rec)

    run(1)
    for w in (int(x) for x in a.worlds.split(",")):
        run(w)
    c.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
