"""Times of a complete masked verification (Session.prove_and_verify_full(mask=, pub_mask=)) in the three verifier modes, beside the unmasked run, on
SHA-256 x BLOCKS (x64: an input layer of 2^19 wires).  For information (profiles/masked_verifier.md): the mask row is at most 2^16 coefficients.

    python tools/masked_verifier_times.py [--blocks 64] [--mask 3000] [--runs 5]"""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import vp_loader  # noqa: E402

KEYS = ("verify_sec", "verify_public_eval_sec", "verify_digests_sec", "verify_rest_sec", "verify_predicates_sec", "pc_prove_sec", "pc_query_answer_sec")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--mask", type=int, default=3000)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    vp = vp_loader.load()
    vp.build()
    with tempfile.TemporaryDirectory() as d:
        pws = os.path.join(d, "SHA256_64.pws")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "SHA256_64.pws.gz"), "rb") as f, open(pws, "wb") as g:
            g.write(f.read())
        c = vp.Circuit.from_pws(pws, a.blocks, seed=1)
    n = c.layer_bitlen(0)
    rng = np.random.default_rng(1)
    P = (1 << 61) - 1
    pri, pub = rng.integers(0, P, size=(a.mask, 2), dtype=np.uint64), rng.integers(0, P, size=(a.mask, 2), dtype=np.uint64)
    s = vp.Session(c)
    out = {"n": n, "mask_elements": a.mask, "runs": a.runs}
    for masked in (False, True):
        for mode, kw in (("default", {}), ("batched_openings", {"batched_openings": True}), ("device_verifier", {"device_verifier": True})):
            rows = []
            for i in range(a.runs + 1):
                _, ok, t = s.prove_and_verify_full(**kw, **({"mask": pri, "pub_mask": pub} if masked else {}))
                assert ok
                if i:                                # the first run of a mode warms its paths
                    rows.append(t)
            out[("masked " if masked else "unmasked ") + mode] = {k: round(1e3 * statistics.median(r[k] for r in rows), 3) for k in KEYS}
    rec = s.last_full_record()
    out["record_version"], out["record_bytes"] = int.from_bytes(rec[4:8], "little"), len(rec)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
