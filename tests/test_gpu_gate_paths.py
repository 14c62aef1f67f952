"""GPU (-m gpu): every gate type through the kernels that carry the per-type switch — the generators of the fused init (GenP1 / GenLiu / GenP2 inside
the first fold launch), the chunk kernels of the heavy rows with their ChunkFuse and combine forms, and the row-range init jobs of a sharded proof.
The circuits come from custom_circuits.make_skewed (tests/test_skewed_circuits_host.py asserts their shape); the reference is the real reference's
record of one of them (tests/golden: custom_c) or the oracle's transcript of the same arrays.  Bar: byte for byte.  Every test asserts through the
profiled launch table that the path it names ran."""
import os
import subprocess
import sys

import pytest

import custom_circuits as cc
from conftest import GOLDEN as GOLDEN_DIR
from test_gpu_parity import _both_modes, _engagement, _kind, _sharded_parts, _split_parts
from test_skewed_circuits_host import NAMES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSE = {"VP_FUSE_MIN_LOG": "14"}      # tables of bit length 14 fuse at the shipped sf_big_log; setting it pins the field against the plan tuner


def _run(vp, c, monkeypatch, env):
    """A fresh session under `env` (the library reads the switches when the context is created): _engagement of its proof."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        s = vp.Session(c)
        s.draw_tape()
        out = _engagement(vp, s)
        tr2, _ = s.prove_gkr()          # the unprofiled replay
        assert tr2 == out[0]
        s.close()
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return out


@pytest.fixture(scope="module")
def custom_c(vp, golden):
    g = golden["custom_c"]
    c = vp.Circuit.custom(*cc.from_golden(g["custom"]))
    assert c.hash() == g["circuit_hash"]
    gold = open(os.path.join(GOLDEN_DIR, g["transcript"]), "rb").read()[g["gkr_slice"][0]:g["gkr_slice"][1]]
    yield c, gold
    c.close()


def test_fused_init_every_gate_type_vs_reference(vp, custom_c, monkeypatch):
    """custom_c with the init of every table of bit length >= 14 generated inside its first fold launch: phase 1 (GenP1), Liu (GenLiu) and the long
    subsets of phase 2 (GenP2), all eleven gate types and assert gates in light and heavy rows.  The real reference's transcript in both modes; fewer
    generating jobs without the phase-2 generator and none without the fused init, the same bytes each time."""
    c, gold = custom_c
    monkeypatch.setenv("VP_FUSE_MIN_LOG", "14")
    _both_modes(vp, c, gold)
    monkeypatch.delenv("VP_FUSE_MIN_LOG")
    tr, _, jobs = _run(vp, c, monkeypatch, FUSE)
    tr_p1, _, jobs_p1 = _run(vp, c, monkeypatch, dict(FUSE, VP_FUSE_P2="0"))
    tr_no, _, jobs_no = _run(vp, c, monkeypatch, dict(FUSE, VP_FUSE_INIT="0"))
    print("fused jobs: %d, without VP_FUSE_P2 %d, without VP_FUSE_INIT %d" % (jobs, jobs_p1, jobs_no))
    assert tr == gold and tr_p1 == gold and tr_no == gold
    assert jobs > 0 and jobs_p1 > 0 and jobs_p1 <= jobs - 1 and jobs_no == 0


@pytest.mark.parametrize("env", [{"VP_FUSE_DOT": "1"}, {"VP_FUSE_COMBINE": "0"}, {"VP_FUSE_COMBINE": "1"}, {"VP_FUSE_COMBINE": "2"}, {"VP_DROP_Y": "0"},
                                 {"VP_DROP_Y1": "1"}, {"VP_REAL_V": "0"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_fused_init_every_gate_type_under_each_switch(vp, custom_c, monkeypatch, env):
    """The same proof with V_u riding on the fused launch, each form of the heavy-row sums (0: chunk partials + k_init_combine, 1 / 2: the chunk launch
    finishes its rows itself — ChunkFuse, whose last-arrival loop takes two passes on the rows of 33000 gates), every round summing its own b, round 1
    leaving b to the fix-up pass, and the complex product on real values.  (VP_FUSE_COMBINE=2 is the default, which the environment cannot pin: the plan
    tuner is switched off for these three, so that the launch table shows the form that was asked for.)"""
    c, gold = custom_c
    if "VP_FUSE_COMBINE" in env:
        env = dict(env, VP_PLAN_AUTOTUNE="0")
    tr, launches, jobs = _run(vp, c, monkeypatch, dict(FUSE, **env))
    chunks, combine = launches.get(_kind(vp, "CHUNKS"), 0), launches.get(_kind(vp, "COMBINE"), 0)
    print("%s: fused jobs %d, chunk launches %d, combine launches %d" % (env, jobs, chunks, combine))
    assert tr == gold
    assert jobs > 0 and chunks > 0
    if "VP_FUSE_COMBINE" in env:
        assert (combine > 0) == (env["VP_FUSE_COMBINE"] == "0")


def test_fused_init_real_values_vs_oracle(vp, ob, monkeypatch):
    """A second skewed circuit with real constants: every circuit value is real, so the generators take the half-price products and the dense arrays
    of real parts (mul_val, valsr)."""
    args = cc.make_skewed(104, real_consts=True)
    c, oc = vp.Circuit.custom(*args), ob.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    gold, st = oc.prove_gkr()
    assert st["verified"] == 1
    monkeypatch.setenv("VP_FUSE_MIN_LOG", "14")
    _both_modes(vp, c, gold)
    monkeypatch.delenv("VP_FUSE_MIN_LOG")
    tr, _, jobs = _run(vp, c, monkeypatch, FUSE)
    tr_c, _, jobs_c = _run(vp, c, monkeypatch, dict(FUSE, VP_REAL_V="0"))
    assert tr == gold and tr_c == gold and jobs > 0 and jobs_c > 0
    c.close(); oc.close()


@pytest.mark.parametrize("t", sorted(NAMES), ids=lambda t: NAMES[t])
def test_fused_init_one_gate_type(vp, ob, monkeypatch, t):
    """Every gate of one type (and the Sub assert gate that closes each layer), the same fan-outs: a wrong arm of a generator's switch fails under its own
    name.  The unary types have no subsets, so their phase 2 is one heavy row that holds the whole layer."""
    args = cc.make_skewed(200 + t, only_type=t)
    c, oc = vp.Circuit.custom(*args), ob.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    gold, st = oc.prove_gkr()
    assert st["verified"] == 1
    monkeypatch.setenv("VP_FUSE_MIN_LOG", "14")
    _both_modes(vp, c, gold)
    monkeypatch.delenv("VP_FUSE_MIN_LOG")
    tr, launches, jobs = _run(vp, c, monkeypatch, FUSE)
    assert tr == gold and jobs > 0 and launches.get(_kind(vp, "CHUNKS"), 0) > 0
    c.close(); oc.close()


def test_heavy_rows_without_fusing_and_device_predicates(vp, custom_c):
    """Default switches: nothing of this size fuses, every init is a light-row launch plus the chunk kernels of the heavy rows.  The real reference's
    transcript; the device predicates accept it and reject it with one bit of the last claim flipped."""
    c, gold = custom_c
    s = vp.Session(c)
    s.draw_tape()
    tr, launches, jobs = _engagement(vp, s)
    assert tr == gold and jobs == 0
    assert launches.get(_kind(vp, "CHUNKS"), 0) > 0 and launches.get(_kind(vp, "LIGHT"), 0) > 0
    ok_host, _ = s.check(tr)
    ok_dev, _ = s.check(tr, device_predicates=True)
    assert ok_host and ok_dev
    bad = bytearray(tr); bad[-8] ^= 1
    assert not s.check(bytes(bad))[0] and not s.check(bytes(bad), device_predicates=True)[0]
    s.close()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_chain_sharded_fused_init_every_gate_type(vp, custom_c, monkeypatch, world):
    """The sumcheck chains of custom_c dealt to `world` ranks, fused init forced on: the ranks' transcripts add up to the real reference's, and the
    generating fold launches ran on the ranks' plans."""
    c, gold = custom_c
    monkeypatch.setenv("VP_FUSE_MIN_LOG", "14")
    s = vp.Session(c)
    monkeypatch.delenv("VP_FUSE_MIN_LOG")
    s.draw_tape()
    assert vp.sum_transcripts(_sharded_parts(vp, s, world)) == gold
    jobs = 0
    for r in range(world):
        s.set_shard(r, world)
        jobs += _engagement(vp, s)[2]
    s.set_shard(0, 1)
    assert jobs > 0
    s.close()


@pytest.mark.parametrize("world", [2, 4])
def test_index_split_heavy_rows_at_the_slice_edges(vp, custom_c, monkeypatch, world):
    """Every table of bit length >= log2(world) + 11 cut by index: the row-range init jobs of a rank (light rows on shifted pointers, its share of the chunk
    list, the combine job) with heavy rows at rows 0 / 1, at 2^13 - 1 and 2^13 — the slice edge of two ranks — and at the last valid row."""
    c, gold = custom_c
    monkeypatch.setenv("VP_SPLIT_COST_PERCENT", "0")
    s = vp.Session(c)
    monkeypatch.delenv("VP_SPLIT_COST_PERCENT")
    s.draw_tape()
    s.set_shard(0, world); s.set_shard_split(11)
    owner, _ = s.shard_chains()
    assert (owner == -1).any(), "nothing was split"
    assert _split_parts(vp, s, world) == gold
    assert _split_parts(vp, s, world, exchange=False) == gold
    chunks = combine = 0
    for r in range(world):
        s.set_shard(r, world); s.set_shard_split(11)
        launches = _engagement(vp, s)[1]
        chunks += launches.get(_kind(vp, "CHUNKS"), 0); combine += launches.get(_kind(vp, "COMBINE"), 0)
    s.set_shard(0, 1)
    assert chunks > 0 and combine > 0
    tr, _ = s.prove_gkr()
    assert tr == gold
    s.close()


@pytest.mark.parametrize("world", [2, 4])
def test_round_sharded_every_gate_type_heavy_rows(vp, custom_c, world):
    """The interactive sumchecks sharded by index over `world` contexts: the real reference's transcript."""
    c, gold = custom_c
    s = vp.Session(c, devices=[0] * world, round_shard_min_log=2)
    assert s.world() == world
    tr, _, ok = s.prove_interactive()
    assert ok and tr == gold
    s.close()


_CHECKED_WORKER = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import vp_loader
import custom_circuits as cc
vp = vp_loader.load()
vp.lib_host()
assert vp.lib_gpu().vp_checked_build() == 1, "VP_LIBGPU did not select the checked library"
g = json.load(open(sys.argv[1]))["custom_c"]
gold = open(os.path.join(os.path.dirname(sys.argv[1]), g["transcript"]), "rb").read()[g["gkr_slice"][0]:g["gkr_slice"][1]]
c = vp.Circuit.custom(*cc.from_golden(g["custom"]))
s = vp.Session(c)
s.draw_tape()
tr, _ = s.prove_gkr()                    # a fired check makes this raise
assert tr == gold, "checked build: batched transcript differs"
s.set_profiling(1)
tr2, _ = s.prove_gkr()
jobs = sum(e["jobs"] for e in s.launch_stats() if e["kernel"] == sys.argv[2])
assert tr2 == gold and jobs > 0, "checked build: no generating fold launch ran"
print("CHECKED OK", jobs, flush=True)
"""


def test_checked_build_fused_init_every_gate_type(vp, custom_c):
    """The -DVP_CHECKED library in a fresh process on custom_c with the fused init forced on: the index checks inside the generators (contrib2, p1_gather,
    GenP2::vrow) are compiled in and run, none fires, and the transcript is the real reference's."""
    assert os.path.exists(vp.LIB_GPU_CHECKED), "vp.build() did not produce the checked library"
    env = dict(os.environ, VP_LIBGPU=vp.LIB_GPU_CHECKED, VP_FUSE_MIN_LOG="14")
    r = subprocess.run([sys.executable, "-c", _CHECKED_WORKER % (ROOT, ROOT), os.path.join(GOLDEN_DIR, "golden.json"), _kind(vp, "SFGEN")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2000:])
    assert "CHECKED OK" in r.stdout
