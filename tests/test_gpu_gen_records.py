"""GPU (-m gpu): the row records of the fused inits (VP_GEN_REC; csrc/vp_kernels_batch.h GenP1R / GenLiuR / GenP2R, built at upload by k_up_rowrec /
k_up_sgidx / k_up_liu_rec).  A fused init generates the mult / add entries of a sumcheck's first fold launch from the target-sorted contribution lists;
with records it reads one 16-byte record per row and gathers through indices into one arena of circuit values and the pool of half tables, instead of
row pointers -> entry arrays -> layer pointers -> values.  No field operation changes, so the bar is byte equality: with the records against without
them, against the real reference's transcripts where the repository holds one, and against the oracle on a circuit built for the row shapes.  Every
test asserts from the plan (Session.gen_jobs) and the profiled launch table that the generators it names ran in the form it names."""
import os
import subprocess
import sys

import pytest

import custom_circuits as cc
import gen_record_circuits as grc
from conftest import GOLDEN as GOLDEN_DIR
from test_gpu_parity import _engagement, _kind, _sharded_parts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tables of 2^10 entries take the fold kernel and fuse their inits; the plan tuner is off so that the launch table shows the plan that was asked for
SMALL = {"VP_FUSE_MIN_LOG": "10", "VP_SF_BIG_LOG": "10", "VP_PLAN_AUTOTUNE": "0"}


def _prove(vp, c, monkeypatch, env, shard_world=0):
    """A fresh session under `env`: (transcript, {mode: (row-pointer jobs, record jobs)}, jobs of the generating fold launches that ran).  shard_world: also
    the summed transcripts of a chain-sharded rehearsal on this GPU."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        s = vp.Session(c)
        s.draw_tape()
        tr, _, ran = _engagement(vp, s)
        modes = s.gen_jobs()
        tr2, _ = s.prove_gkr()                  # the unprofiled replay
        assert tr2 == tr
        summed = vp.sum_transcripts(_sharded_parts(vp, s, shard_world)) if shard_world else None
        if shard_world:                          # the ranks' own plans: their jobs, summed over the ranks, in place of the unsharded plan's
            modes = {m: (0, 0) for m in (1, 2, 3)}
            for r in range(shard_world):
                s.set_shard(r, shard_world)
                s.prove_gkr()
                g = s.gen_jobs()
                modes = {m: (modes[m][0] + g[m][0], modes[m][1] + g[m][1]) for m in modes}
            s.set_shard(0, 1)
        s.close()
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return tr, modes, ran, summed


def _ab(vp, c, monkeypatch, env, gold, want_rec, shard_world=0, real=True):
    """VP_GEN_REC=3 (both bits: the default) against VP_GEN_REC=0 under `env`, both against gold.  want_rec: the modes that must run, from records, when they are on.  real: the
    witness is real, so every fused job must take its record form; otherwise phases 1 and 2 (modes 1, 3) must keep the row-pointer form.  With the records
    off every job runs from row pointers, and the same sumchecks fuse either way."""
    tr1, m1, ran1, sum1 = _prove(vp, c, monkeypatch, dict(env, VP_GEN_REC="3"), shard_world)
    tr0, m0, ran0, sum0 = _prove(vp, c, monkeypatch, dict(env, VP_GEN_REC="0"), shard_world)
    print("fused jobs by mode (row pointers, records): VP_GEN_REC=3 %s, VP_GEN_REC=0 %s; ran %d / %d" % (m1, m0, ran1, ran0))
    assert tr1 == tr0, "the transcript changes with VP_GEN_REC"
    if gold is not None:
        assert tr1 == gold, "transcript differs from the reference"
    if shard_world:
        assert sum1 == tr1 and sum0 == tr1, "the sharded ranks do not add up to the unsharded transcript"
    assert ran1 == ran0
    for mode in (1, 2, 3):
        assert m0[mode][1] == 0, "VP_GEN_REC=0 ran a record job"
        assert sum(m1[mode]) == m0[mode][0], "VP_GEN_REC changed which sumchecks fuse"
        if mode in want_rec:
            assert m1[mode][1] > 0 and ran1 > 0, "mode %d did not run from records" % mode
        if real or mode == 2:
            assert m1[mode][0] == 0, "mode %d: a job kept the row-pointer form" % mode
        else:
            assert m1[mode][1] == 0, "mode %d ran from records on a complex witness" % mode
    return m1, m0


def _gold(golden, name):
    g = golden[name]
    return open(os.path.join(GOLDEN_DIR, g["transcript"]), "rb").read()[g["gkr_slice"][0]:g["gkr_slice"][1]]


@pytest.mark.parametrize("name", ["custom_a", "custom_b", "custom_c", "custom_d"])
def test_records_custom_circuits_vs_reference(vp, golden, monkeypatch, name):
    """The four custom circuits of the real reference's records, every table of 2^10 entries or more fused.  Their Mulc / Addc constants are complex, so
    the witness is: phases 1 and 2 keep the row-pointer generators (the arena holds real parts), the Liu gathers run from records wherever one fuses.
    custom_a and custom_d have one table of 2^10 entries (600 inputs): one phase-1 and one Liu job fuse there, nothing else does — these two cases mostly
    pin the switch, and the records built at upload, as harmless on circuits that hardly use them."""
    c = vp.Circuit.custom(*cc.from_golden(golden[name]["custom"]))
    assert c.hash() == golden[name]["circuit_hash"]
    m1, m0 = _ab(vp, c, monkeypatch, SMALL, _gold(golden, name), want_rec=(2,), real=False)
    assert m0[1][0] > 0 and m0[2][0] > 0
    c.close()


@pytest.mark.parametrize("name", ["randomize_8_12", "sha256_x1"])
def test_records_small_real_circuits_vs_reference(vp, golden, pws_path, monkeypatch, name):
    """randomize(8, 12) and SHA-256 x1: real witnesses, tables of 2^10 entries or more fused — phase 1 and the Liu gathers from records."""
    c = vp.Circuit.randomize(8, 12, seed=1) if name == "randomize_8_12" else vp.Circuit.from_pws(pws_path, 1, seed=1)
    assert c.hash() == golden[name]["circuit_hash"]
    _ab(vp, c, monkeypatch, SMALL, _gold(golden, name), want_rec=(1, 2))
    c.close()


def test_records_all_three_modes_at_the_shipped_thresholds(vp, golden, monkeypatch):
    """randomize(16, 20): the one fixture whose tables (2^20 entries) fuse phase 1, Liu and phase 2 at the threshold its own size resolves to
    (VP_FUSE_MIN_LOG=20; setting it pins the field against the plan tuner)."""
    c = vp.Circuit.randomize(16, 20, seed=1)
    assert c.hash() == golden["randomize_16_20"]["circuit_hash"]
    _ab(vp, c, monkeypatch, {"VP_FUSE_MIN_LOG": "20", "VP_PLAN_AUTOTUNE": "0"}, _gold(golden, "randomize_16_20"), want_rec=(1, 2, 3))
    c.close()


# ---- row shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_real(vp, ob):
    args = grc.make_rows(5, real=True)
    c, oc = vp.Circuit.custom(*args), ob.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    gold, st = oc.prove_gkr()
    assert st["verified"] == 1
    oc.close()
    yield args, c, gold
    c.close()


def test_row_shape_circuit_has_the_shapes():
    """From the arrays: phase-1 rows of 0, 1, 2, VP_LIGHT_MAX and VP_LIGHT_MAX + 1 contributions over an odd number of wires that is two fold chunks and a
    partial third; phase-2 slots of 1, 2, VP_LIGHT_MAX and more; unary entries, assert gates, operands in a layer other than i - 1."""
    args = grc.make_rows(5)
    rows, slots, unary, asserts, operand_layers = grc.shape(args)
    m = int(args[0][1])
    assert m % 2 == 1 and m > 1024 and m % 512 != 0
    assert {0, 1, 2, grc.LIGHT_MAX, grc.LIGHT_MAX + 1} <= rows
    assert {1, 2, grc.LIGHT_MAX, grc.LIGHT_MAX + 1} <= slots
    assert unary > grc.LIGHT_MAX and asserts == 3 and operand_layers == {0, 1}


def test_records_row_shapes_vs_oracle(vp, rows_real, monkeypatch):
    """The shaped circuit with a real witness, every init fused: all three generators from records, the oracle's transcript on the same tape."""
    args, c, gold = rows_real
    _ab(vp, c, monkeypatch, SMALL, gold, want_rec=(1, 2, 3))


@pytest.mark.parametrize("level,forms", [("1", {1: 1, 2: 0, 3: 1}), ("2", {1: 0, 2: 1, 3: 0})])
def test_records_row_shapes_one_bit_of_the_switch(vp, rows_real, monkeypatch, level, forms):
    """VP_GEN_REC=1: records for the phase-1 and phase-2 inits only; VP_GEN_REC=2: for the Liu gathers only.  The oracle's transcript either way."""
    args, c, gold = rows_real
    tr, m, ran, _ = _prove(vp, c, monkeypatch, dict(SMALL, VP_GEN_REC=level))
    assert tr == gold and ran > 0
    for mode, rec in forms.items():
        assert m[mode][rec] > 0 and m[mode][1 - rec] == 0, (mode, m)


def test_records_row_shapes_without_fused_phase2(vp, rows_real, monkeypatch):
    """VP_FUSE_P2=0: phase 2 keeps its init launches, phase 1 and Liu run from records."""
    args, c, gold = rows_real
    m1, m0 = _ab(vp, c, monkeypatch, dict(SMALL, VP_FUSE_P2="0"), gold, want_rec=(1, 2))
    assert sum(m1[3]) == 0 and sum(m0[3]) == 0


def test_records_row_shapes_chain_sharded(vp, rows_real, monkeypatch):
    """A 2-way chain-sharded rehearsal on one GPU: each rank's plan holds its share of the generating jobs, the ranks' transcripts add up to the oracle's."""
    args, c, gold = rows_real
    _ab(vp, c, monkeypatch, SMALL, gold, want_rec=(1, 2, 3), shard_world=2)


def test_records_complex_witness_keeps_the_row_pointer_generators(vp, ob, monkeypatch):
    """The same gates with complex Mulc / Addc constants: the arena holds real parts only, so phases 1 and 2 must run from row pointers (and do fuse); the
    Liu gather reads no circuit value and runs from records.  The oracle's transcript."""
    args = grc.make_rows(5, real=False)
    c, oc = vp.Circuit.custom(*args), ob.Circuit.custom(*args)
    assert c.hash() == oc.hash()
    gold, st = oc.prove_gkr()
    assert st["verified"] == 1
    m1, m0 = _ab(vp, c, monkeypatch, SMALL, gold, want_rec=(2,), real=False)
    assert m1[1][0] > 0 and m1[3][0] > 0
    c.close(); oc.close()


_CHECKED_WORKER = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import vp_loader
import gen_record_circuits as grc
vp = vp_loader.load()
vp.lib_host()
assert vp.lib_gpu().vp_checked_build() == 1, "VP_LIBGPU did not select the checked library"
for real in (True, False):
    c = vp.Circuit.custom(*grc.make_rows(5, real=real))
    out = []
    for rec in ("3", "0"):
        os.environ["VP_GEN_REC"] = rec
        s = vp.Session(c)
        s.draw_tape()
        tr, _ = s.prove_gkr()                # a fired check makes this raise
        out.append((tr, s.gen_jobs()))
        s.close()
    assert out[0][0] == out[1][0], "checked build: the transcript changes with VP_GEN_REC"
    open(sys.argv[1 if real else 2], "wb").write(out[0][0])
    want = (1, 2, 3) if real else (2,)
    assert all(out[0][1][m][1] > 0 for m in want) and all(out[1][1][m][1] == 0 for m in (1, 2, 3)), out
print("CHECKED OK", flush=True)
"""


def test_records_checked_build(vp, ob, rows_real, tmp_path):
    """The -DVP_CHECKED library in a fresh process on the shaped circuit, real and complex witness: the checks of the record forms (arena and pool bounds, a
    record's count against the row pointers) are compiled in and none fires; its transcripts are the product build's, byte for byte."""
    assert os.path.exists(vp.LIB_GPU_CHECKED), "vp.build() did not produce the checked library"
    env = dict(os.environ, VP_LIBGPU=vp.LIB_GPU_CHECKED, **SMALL)
    f_real, f_cplx = str(tmp_path / "real.bin"), str(tmp_path / "cplx.bin")
    r = subprocess.run([sys.executable, "-c", _CHECKED_WORKER % (ROOT, ROOT), f_real, f_cplx], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2000:])
    assert "CHECKED OK" in r.stdout
    assert open(f_real, "rb").read() == rows_real[2]
    s = vp.Session(vp.Circuit.custom(*grc.make_rows(5, real=False)))
    s.draw_tape()
    assert open(f_cplx, "rb").read() == s.prove_gkr()[0]
    s.close()
