#!/bin/bash
# Rehearsal of bench.py's multi-rank modes on a ONE-GPU box (both ranks on the same card; timings are meaningless, the
# code path — rendezvous, barrier, max-over-ranks, sharded proof + transcript all-reduce, JSON line — is what is exercised).
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; O=bench_out; mkdir -p "$O"
python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29541 bench.py --gpus 2 --steps 5 --warmup 2 --blocks 16 --no-pc --full > $O/rehearse_weak.json 2> $O/rehearse_weak.err || { tail -20 $O/rehearse_weak.err; exit 1; }
VP_BENCH_BACKEND=gloo python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29542 bench.py --gpus 2 --steps 5 --warmup 2 --blocks 16 --no-pc --shard-chains --full > $O/rehearse_shard.json 2> $O/rehearse_shard.err || { tail -20 $O/rehearse_shard.err; exit 1; }
python3 - "$O" <<'PY'
import json, sys
for f in ("rehearse_weak","rehearse_shard"):
    d=json.loads(open("%s/%s.json"%(sys.argv[1], f)).read().strip().splitlines()[-1])
    print(f, d["n_gpus"], d["ranks"], d["scaling"], d["config"]["proofs_per_step"], "bit-exact", d["bit_exact"], "verifier", d.get("host_verifier_accepts"), d.get("sharded_proof"))
PY
