#!/usr/bin/env python3
"""Write tests/golden/full_fs_rand3_7.bin and full_fs_rand3_9_ms8.bin: joined non-interactive proofs (host/vphost.h, "The joined proof") of
Circuit.randomize(3, 7, seed=11) — the smallest circuit with an input layer of 2^7 wires, the zero mask — and of Circuit.randomize(3, 9, seed=12) with ms = 8, 3
repetitions each.  The candidate bytes come from Session.prove_full_fs on the GPU; a record is written only if it equals, byte for byte, the record that
tests/full_fs_ref.py assembles from the oracle alone on the hashlib-derived challenges (the same code tests/test_full_fs_host.py runs without a GPU), and the host
verifier accepts it.

    python tests/golden/make_full_fs.py [--out DIR]      (default: this directory)
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    import full_fs_ref as ff
    import oracle_binding as ob
    import vp_loader
    vp = vp_loader.load()
    vp.build()
    os.makedirs(a.out, exist_ok=True)
    f = ff.masked_family()
    for name, fix, kw, okw in (("full_fs_rand3_7", ff.FIXTURE, {}, {}),
                               ("full_fs_rand3_9_ms8", ff.FIXTURE_MASKED, {"mask": f["pri_mask"], "pub_mask": f["pub_mask"]},
                                {"pri_mask": f["pri_mask"], "oracle_pub_mask": f["pub_mask"]})):
        _, layers, log_size, seed, reps = fix
        c = vp.Circuit.randomize(layers, log_size, seed=seed)
        s = vp.Session(c)
        proof = s.prove_full_fs(reps=reps, **kw)
        # the reference: the same record assembled from the oracle alone on the hashlib-derived challenges (tests/full_fs_ref.py)
        want, _ = ff.assemble(ob.Circuit.randomize(layers, log_size, seed=seed), proof, **okw)
        if want != proof:
            sys.exit("refused: %s is not the record the oracle assembles" % name)
        ok, why = c.verify_full_fs(proof)
        if not ok:
            sys.exit("refused: the host verifier rejects %s: %s" % (name, why))
        assert len(proof) < 200 * 1024 and ff.sections(proof)["end"] == len(proof)
        open(os.path.join(a.out, name + ".bin"), "wb").write(proof)
        meta = {"circuit": "Circuit.randomize(%d, %d, seed=%d)" % (layers, log_size, seed), "circuit_hash": c.hash(), "n": c.layer_bitlen(0), "reps": reps,
                "ms": 8 if kw else 1, "bytes": len(proof), "sha256": hashlib.sha256(proof).hexdigest(),
                "origin": "tests/golden/make_full_fs.py on the GPU box: Session.prove_full_fs, equal to full_fs_ref.assemble (the oracle) before it is written"}
        json.dump(meta, open(os.path.join(a.out, name + ".json"), "w"), indent=1, sort_keys=True)
        print("wrote", name, len(proof), "bytes", meta["sha256"])
        s.close(); c.close()


if __name__ == "__main__":
    main()
