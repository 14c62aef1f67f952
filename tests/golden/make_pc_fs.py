"""Writes tests/golden/pc_fs.json: the fixed point of the non-interactive commitment (tests/pc_fs_ref.py: the Python chain over the oracle's commitment, ln + 1
runs) at the sizes where it takes the CPU too long for a test — pc_fs_ref.RECORDED.  Run from the repository root after __graft_entry__.build():
    python tests/golden/make_pc_fs.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_binding as ob
import pc_fs_ref as fs

if __name__ == "__main__":
    L = ob.lib()
    out = {}
    for name, (kind, n, fam, ms) in fs.RECORDED.items():
        x, point, f = fs.case(kind, n, fam, ms)
        fp = fs.fixed_point(L, n, x["values"], x["n_used"], point, f)
        fp["values"] = x["values"]
        out[name] = fs.record_of(fp)
        print(name, out[name]["state_out"], flush=True)
    json.dump(out, open(fs.GOLDEN, "w"), indent=1, sort_keys=True)
