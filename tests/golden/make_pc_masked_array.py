#!/usr/bin/env python3
"""Recorded runs of the oracle's masked commitment (orc_commitment_array_masked) at the sizes the suite does not compute live (minutes of CPU):
n = 18 with a 40000-element mask (pads to 2^16, 16 blocks of a slice's message, a 2^17-point quotient transform — the longest mask the device takes) and
n = 20 with a 2^14-element mask of edge limbs (exactly a slice's message) under edge challenges.

    python tests/golden/make_pc_masked_array.py   -> tests/golden/pc_masked_array_<case>.bin (root_l | root_h | inner | all_sum[65] | roots | final | final_mask),
                                                     pc_masked_array.json (seeds come from tests/pc_masked_inputs.py; the inputs' sha256 are in the index)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_binding as ob
import pc_masked_inputs as pmi


def main():
    meta = {}
    for name, (n, kind, fam, ms, m) in pmi.ARRAY_CASES.items():
        x = pmi.array_case(name)
        rec, _ = pmi.oracle_masked(ob.lib(), x["values"], x["n_used"], x["pub"], n, x["r"], x["pri_mask"], x["pub_mask"])
        out = "pc_masked_array_%s.bin" % name
        open(os.path.join(HERE, out), "wb").write(rec)
        meta[name] = dict(pmi.array_digests(x), n=n, set=kind, family=fam, ms=ms, m=m, n_used=x["n_used"], record=out, record_sha256=hashlib.sha256(rec).hexdigest(),
                          origin="oracle: orc_commitment_array_masked (oracle/vp_oracle.cpp) on tests/pc_masked_inputs.array_case")
        print(name, len(rec), meta[name]["record_sha256"])
    json.dump(meta, open(os.path.join(HERE, "pc_masked_array.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
