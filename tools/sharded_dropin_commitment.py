"""The drop-in commitment on a shard, on ONE GPU (include/vpgpu.h: vp_pc_set_shard with vp_fri_step / vp_commit_public_eq): per-rank device time
(vp_commit_stats) of commit_private, commit_public, commit_public_eq and the sum of the n - 6 FRI steps for W ranks as contexts of one GPU, called
one after the other from one thread so that a rank's time is its own; beside them the one-pass vp_fri_commit, the host wall time of a rank's
commit_public / commit_public_eq (the first includes the copy of its slices of the public vector), and the bytes a rank sends per collective.
W = 1 is the unsharded context.  The input layer has the size of the SHA-256 circuit of `blocks` blocks (2^19 wires at x64, 2^23 at x1024) and
random values: no kernel's time here depends on the values (an unsharded context with a REAL witness would halve commit_private's transforms, the
sharded one does not take that path).  No speed-up is expected on one GPU; wall clock across several GPUs is not measured by this tool.

    python tools/sharded_dropin_commitment.py [--blocks 64,1024] [--worlds 1,2,4,8] [--reps 5] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VP_EXCHANGE = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="64,1024")
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import vp_loader
    vp = vp_loader.load()
    L = vp.lib_gpu()
    L.vp_shard_exchange_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
    P = (1 << 61) - 1
    out = {"runs": []}

    def run(blocks, world):
        n = 13 + (blocks.bit_length() - 1)                 # input layer of the SHA-256 circuit: 2^13 wires per block
        rng = np.random.default_rng(blocks)
        inputs = rng.integers(0, P, size=(1 << n, 2), dtype=np.uint64)
        point = rng.integers(0, P, size=(n, 2), dtype=np.uint64)
        r = rng.integers(0, P, size=(n - 6, 2), dtype=np.uint64)
        ctx = []
        for q in range(world):
            c = ctypes.c_void_p()
            assert L.vp_create(0, ctypes.byref(c)) == 0
            assert L.vp_pc_load_input(c, inputs.ctypes.data, inputs.shape[0], n) == 0
            assert L.vp_pc_set_shard(c, q, world) == 0
            ctx.append(c)
        arr = (ctypes.c_void_p * world)(*[c.value for c in ctx])
        # the table for commit_public: built once on rank 0's device (vp_test_beta), as the protocol's caller would hold it
        one = np.array([1, 0], dtype=np.uint64)
        pub = np.zeros((1 << n, 2), dtype=np.uint64)
        assert L.vp_test_beta(ctx[0], point.ctypes.data, n, one.ctypes.data, pub.ctypes.data) == 0
        root = ctypes.create_string_buffer(32 * 32)
        inner = np.zeros(2, np.uint64); alls = np.zeros((65, 2), np.uint64)
        rootp = ctypes.cast(root, ctypes.c_void_p)

        def call(fn):
            """fn(ctx) on every rank in turn until all are done: per-rank (device ms, host wall ms), and what a rank sends per collective"""
            wall = [0.0] * world
            sent = []
            while True:
                rcs = []
                for q in range(world):
                    t0 = time.perf_counter()
                    rcs.append(fn(ctx[q]))
                    wall[q] += (time.perf_counter() - t0) * 1e3
                assert all(rc >= 0 for rc in rcs), (rcs, L.vp_last_error(ctx[0]))
                if all(rc == 0 for rc in rcs):
                    break
                assert all(rc == VP_EXCHANGE for rc in rcs), rcs
                kind = ctypes.c_int(0); nb = ctypes.c_uint64(0)
                assert L.vp_shard_exchange_info(ctx[0], 0, ctypes.byref(kind), ctypes.byref(nb)) == 0
                sent.append({"kind": "all-to-all" if kind.value == 1 else "all-gather", "bytes_sent_per_rank": int(nb.value) * ((world - 1) if kind.value == 1 else 1)})
                assert L.vp_shard_exchange_local(arr, world) == 0
            dev = []
            for q in range(world):
                ms = ctypes.c_double(0)
                L.vp_commit_stats(ctx[q], ctypes.byref(ms))
                dev.append(ms.value)
            return dev, wall, sent

        def one_pass(stepwise, eq):
            rec = {}
            rec["commit_private"] = call(lambda c: L.vp_commit_private(c, rootp))
            if eq:
                rec["commit_public_eq"] = call(lambda c: L.vp_commit_public_eq(c, point.ctypes.data, n, inner.ctypes.data, alls.ctypes.data, rootp))
            else:
                rec["commit_public"] = call(lambda c: L.vp_commit_public(c, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data, rootp))
            if stepwise:
                dev = [0.0] * world; wall = [0.0] * world; sent = []
                for k in range(n - 6):
                    d, w, s = call(lambda c: L.vp_fri_step(c, r[k:].ctypes.data, rootp))
                    dev = [x + y for x, y in zip(dev, d)]; wall = [x + y for x, y in zip(wall, w)]; sent += s
                rec["fri_steps"] = (dev, wall, sent)
            else:
                rec["fri_commit"] = call(lambda c: L.vp_fri_commit(c, r.ctypes.data, n - 6, rootp))
            return rec

        modes = [(True, True), (False, False)]            # step-wise after the eq point; one pass after the table
        one_pass(*modes[0]); one_pass(*modes[1])           # warm-up: first-touch allocations, root tables, code objects
        acc = {}
        collectives = {}
        for _ in range(a.reps):
            for m in modes:
                for name, (dev, wall, sent) in one_pass(*m).items():
                    key = name + ("" if name != "commit_private" else ("" if m[0] else "#2"))
                    acc.setdefault(key, {"dev": [], "wall": []})
                    acc[key]["dev"].append(dev); acc[key]["wall"].append(wall)
                    collectives[key] = sent
        res = {"blocks": blocks, "n": n, "world": world, "reps": a.reps, "calls": {}}
        for key, v in acc.items():
            if key.endswith("#2"):
                continue
            dev = [statistics.median(x[q] for x in v["dev"]) for q in range(world)]
            wall = [statistics.median(x[q] for x in v["wall"]) for q in range(world)]
            res["calls"][key] = {"device_ms_per_rank": [round(x, 3) for x in dev], "device_ms_max": round(max(dev), 3),
                                 "host_wall_ms_max": round(max(wall), 3), "collectives": collectives[key]}
        for c in ctx:
            L.vp_destroy(c)
        print(json.dumps(res), flush=True)
        out["runs"].append(res)

    for b in (int(x) for x in a.blocks.split(",")):
        for w in (int(x) for x in a.worlds.split(",")):
            run(b, w)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
