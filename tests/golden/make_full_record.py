#!/usr/bin/env python3
"""Write tests/golden/full_record_custom_a.bin: the record of ONE complete-protocol run (vphost.h: vph_last_full_record) of the custom_a
circuit on the GPU — n = 10, 4 FRI levels, 2 query repetitions, answered in one device pass.  tests/test_query_record_host.py replays the
host verifier over it without a GPU.  Needs the GPU box; refuses to write a record whose transcript section is not the real reference's
transcript_custom_a.bin or whose FRI roots / final codeword are not those of fri_custom_a.bin.

    python tests/golden/make_full_record.py [--out DIR]      (default: this directory)
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
NAME, REPS = "custom_a", 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    import custom_circuits as cc
    import vp_loader
    vp = vp_loader.load()
    vp.build()
    g = json.load(open(os.path.join(HERE, "golden.json")))[NAME]
    c = vp.Circuit.custom(*cc.make(g["custom"]["seed"], g["custom"]["sizes"]))
    assert c.hash() == g["circuit_hash"]
    s = vp.Session(c)
    tr, ok, _ = s.prove_and_verify_full(reps=REPS, batched_openings=True)
    assert ok, "the host verifier rejected the run"
    rec = s.last_full_record()
    gold = open(os.path.join(HERE, g["transcript"]), "rb").read()
    if tr != gold or rec[16:16 + len(gold)] != gold:
        sys.exit("refused: the transcript section differs from " + g["transcript"])
    fri = open(os.path.join(HERE, g["fri"]), "rb").read()
    st = g["fri_steps"]
    roots = b"".join(fri[48 * k + 16:48 * k + 48] for k in range(st))
    final = fri[48 * st:48 * st + 2048 * 16]
    n = c.layer_bitlen(0)
    per_query = 2 * (2080 + 32 * (n - 1)) + sum(2080 + 32 * (n - 2 - k) for k in range(n - 6))
    at = len(rec) - REPS * per_query - len(final) - len(roots)
    if rec[at:at + len(roots)] != roots or rec[at + len(roots):at + len(roots) + len(final)] != final:
        sys.exit("refused: FRI roots / final codeword differ from " + g["fri"])
    assert c.verify_full_record(rec), "the host replay rejected the record"
    assert len(rec) < 100 * 1024
    os.makedirs(a.out, exist_ok=True)
    open(os.path.join(a.out, "full_record_%s.bin" % NAME), "wb").write(rec)
    meta = {"circuit": NAME, "custom": g["custom"], "circuit_hash": g["circuit_hash"], "n": n, "fri_steps": st, "reps": REPS, "batched_openings": True,
            "bytes": len(rec), "sha256": hashlib.sha256(rec).hexdigest(), "transcript": g["transcript"], "fri": g["fri"],
            "origin": "tests/golden/make_full_record.py on the GPU box: Session.prove_and_verify_full(reps=2, batched_openings=True), Session.last_full_record()"}
    json.dump(meta, open(os.path.join(a.out, "full_record_%s.json" % NAME), "w"), indent=1, sort_keys=True)
    print("wrote", len(rec), "bytes", meta["sha256"])
    s.close(); c.close()


if __name__ == "__main__":
    main()
