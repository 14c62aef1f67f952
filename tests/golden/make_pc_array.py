#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator, like make_golden.py): runs the oracle; nothing in the product imports this.
The ORACLE's whole commitment (orc_commitment_array) on the "uniform" input set of tests/pc_array_inputs.py at the two recorded sizes of
tests/test_gpu_commitment_ladder.py, n = 18 and n = 20: root_l | root_h | inner | all_sum[65] | roots[n - 6] | final[2048] per size
(pc_array_n18.bin, pc_array_n20.bin, about 34 KB each) and pc_array.json with the seeds, n_used and the SHA-256 of the generated input, public
and challenge bytes.  CPU only, a few minutes and a few GB at n = 20; rerunning reproduces the committed files byte for byte.

    python tests/golden/make_pc_array.py [OUT_DIR]
"""
import hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = (18, 20)


def main():
    import oracle_binding as ob
    import pc_array_inputs as pai
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    L = ob.lib()
    meta = {}
    for n in SIZES:
        t0 = time.time()
        x = pai.inputs("uniform", n)
        rec = pai.oracle_record(L, x["values"], x["n_used"], x["pub"], n, x["r"])
        name = "pc_array_n%d.bin" % n
        open(os.path.join(out, name), "wb").write(rec)
        meta["n%d" % n] = dict({"n": n, "set": "uniform", "seed": pai.seed_of("uniform", n), "n_used": x["n_used"], "record": name,
                                "record_sha256": hashlib.sha256(rec).hexdigest()}, **pai.digests(x))
        print("n = %d: %d bytes, %.0f s" % (n, len(rec), time.time() - t0), flush=True)
    with open(os.path.join(out, "pc_array.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
