"""CPU: the oracle's masked commitment (orc_commitment_array_masked, oracle/vp_oracle.cpp) against a definition-level reference of the mask slice in Python
integers (tests/pc_mask_ref.py) — all_sum[64], the mask pair of openings of l, h and every FRI level, the final mask codeword — at n = 7 .. 10 for every
padded mask length the device takes (8 .. M/2, up to 256) and every mask family of tests/pc_masked_inputs.py; the families' own properties; the entry's
refusals; the zero-mask composition; and the recorded sizes' index.  (The oracle against the real reference's records: tests/test_oracle_golden.py.)"""
import hashlib
import json
import os

import numpy as np
import pytest

import pc_array_inputs as pai
import pc_mask_ref as ref
import pc_masked_inputs as pmi
from conftest import GOLDEN

P = pmi.P61
_RUNS = {}


def _pairs(a):
    return [(int(x), int(y)) for x, y in a]


def _open_leaves(n):
    """(oracle, leaf) of l, h and every FRI level: the first leaf, the last and one inside"""
    out = []
    for o in range(2 + n - 6):
        leaves = 1 << (n - 2) if o < 2 else 1 << (n - 2 - (o - 1))
        out += [(o, lf) for lf in sorted({0, leaves - 1, leaves // 3 + 1})]
    return out


def _run(ob, n, ms, fam):
    """one oracle run and one Python reference per (n, ms, family), shared by the tests below"""
    if (n, ms, fam) not in _RUNS:
        x, f = pai.inputs("uniform", n), pmi.family(fam, n, ms)
        opens = _open_leaves(n)
        rec, vals = pmi.oracle_masked(ob.lib(), x["values"], x["n_used"], x["pub"], n, f["r"], f["pri_mask"], f["pub_mask"], opens)
        py = ref.MaskSlice(n, _pairs(f["pri_mask"]), _pairs(f["pub_mask"]), _pairs(f["r"]), ob.root_of_unity(n - 1))
        _RUNS[(n, ms, fam)] = (x, f, pmi.split_masked_record(rec, n), opens, vals, py)
    return _RUNS[(n, ms, fam)]


CASES = [(n, ms) for n in (7, 8, 9, 10) for ms in pmi.accepted_ms(n, cap=256)]


def test_the_cases_are_every_accepted_mask_length():
    assert CASES == [(7, 8), (7, 16), (7, 32), (8, 8), (8, 16), (8, 32), (8, 64), (9, 8), (9, 16), (9, 32), (9, 64), (9, 128),
                     (10, 8), (10, 16), (10, 32), (10, 64), (10, 128), (10, 256)]
    assert all(ms > (1 << (n - 6)) for n, ms in CASES if n <= 8)          # at n = 7 and 8 every accepted mask is longer than a slice's message


@pytest.mark.parametrize("fam", pmi.FAMILIES)
@pytest.mark.parametrize("n,ms", CASES)
def test_oracle_mask_slice_equals_the_python_reference(ob, n, ms, fam):
    """all_sum[64], the mask pairs of 3 openings of l, of h and of every FRI level, and the 32 values of the final mask codeword: the oracle's transforms and
    folds against polynomials in Python integers.  The final mask codeword is constant exactly when the mask pads to no more than a slice's message."""
    x, f, got, opens, vals, py = _run(ob, n, ms, fam)
    assert py.ms == ms
    assert got["public"][16 + 64 * 16:] == np.array(py.all_sum, np.uint64).tobytes(), "all_sum[64]"
    for (o, lf), v in zip(opens, vals):
        assert _pairs(v[128:130]) == list(py.pair(o, lf)), "mask pair of oracle %d at leaf %d" % (o, lf)
    fm = py.final_mask()
    assert got["final_mask"] == np.array(fm, np.uint64).tobytes(), "final mask codeword"
    if fam in pmi.NONZERO_FAMILIES:
        assert (len(set(fm)) == 1) == (ms <= (1 << (n - 6)))


@pytest.mark.parametrize("fam", pmi.FAMILIES)
@pytest.mark.parametrize("n,ms", CASES)
def test_mask_families_are_what_they_name(ob, n, ms, fam):
    """every family other than pub_zero and pri_zero has all_sum[64] != 0 and a final mask codeword that is not all zero; the zero families have both zero; the
    masks pad to ms; edges holds its special challenges"""
    x, f, got, opens, vals, py = _run(ob, n, ms, fam)
    pri, pub, r = f["pri_mask"], f["pub_mask"], f["r"]
    assert pmi.padded_length(n, pri.shape[0])[1] == ms and 1 <= pub.shape[0] <= ms
    alls64, fm = got["public"][16 + 64 * 16:], got["final_mask"]
    if fam in pmi.NONZERO_FAMILIES:
        assert alls64 != bytes(16) and fm != bytes(32 * 16)
    else:
        assert alls64 == bytes(16) and fm == bytes(32 * 16)
        assert (pri.any(), pub.any()) == ((True, False) if fam == "pub_zero" else (False, True))
    if fam == "edges":
        assert set(np.unique(pri)) <= set(pai.EDGES) and set(np.unique(pub)) <= set(pai.EDGES) and pri.shape[0] < ms
        rs = _pairs(r)
        want = [lambda c: c[0] == 0 and c[1] != 0, lambda c: c == (0, 0), lambda c: c == (P - 1, P - 1)][:n - 6]
        assert all(any(w(c) for c in rs) for w in want)
    if fam == "short_pub":
        assert pub.shape[0] < pri.shape[0] < ms
    if fam == "one_hot":
        assert pri.shape[0] == ms and pri[-1].all() and not pri[:-1].any() and pub[-1].all() and not pub[:-1].any()


@pytest.mark.parametrize("n", [7, 9, 12])
@pytest.mark.parametrize("kind", pai.SETS)
def test_zero_masks_are_the_unmasked_entry(ob, n, kind):
    """orc_commitment_array and orc_commitment_array_masked with zero masks (any accepted length) return the same bytes, and a zero final mask codeword: one code"""
    x = pai.inputs(kind, n)
    want = pai.oracle_record(ob.lib(), x["values"], x["n_used"], x["pub"], n, x["r"])
    for m, q in ((8, 1), (1 << (n - 2), 5)):
        rec, _ = pmi.oracle_masked(ob.lib(), x["values"], x["n_used"], x["pub"], n, x["r"], np.zeros((m, 2), np.uint64), np.zeros((q, 2), np.uint64))
        assert rec[:-32 * 16] == want and rec[-32 * 16:] == bytes(32 * 16)


def test_oracle_entry_refuses_what_the_device_refuses(ob):
    """a mask that pads to fewer than 8 elements, one that pads to the whole slice (gap 1), one longer than a slice, an empty one; a public mask longer than the
    padded private one or empty; a non-canonical limb in either mask or a challenge: -1 each.  The neighbours of each are taken."""
    n = 10
    M = 1 << (n - 1)
    x, f = pai.inputs("uniform", n), pmi.family("uniform", n, 16)
    pri, pub = np.array(f["pri_mask"]), np.array(f["pub_mask"])
    call = lambda pm, qm, r=f["r"], **kw: pmi.oracle_masked_rc(ob.lib(), x["values"], x["n_used"], x["pub"], n, r, pm, qm, **kw)[0]
    big = np.random.default_rng(1).integers(0, P, size=(M + 1, 2), dtype=np.uint64)
    assert call(pri, pub) == 0
    assert call(big[:M // 128 + 1], big[:1]) == 0 and call(big[:M // 128], big[:1]) == -1          # pads to 8 / to 4
    assert call(big[:M // 4], big[:M // 4]) == 0 and call(big[:M // 4 + 1], big[:1]) == 0            # pads to M/4 / to M/2: gap 4, 2
    assert call(big[:M // 2 + 1], big[:1]) == -1 and call(big[:M], big[:1]) == -1                    # gap 1
    assert call(big, big[:1]) == -1 and call(big, big[:1], n_pri=0) == -1                            # longer than a slice; empty
    assert call(pri, big[:16]) == 0 and call(pri, big[:17]) == -1 and call(pri, big, n_pub=0) == -1  # pri pads to 16
    for which in range(3):
        for limb in range(2):
            pm, qm, r = pri.copy(), pub.copy(), np.array(f["r"])
            (pm, qm, r)[which][-1, limb] = P
            assert call(pm, qm, r) == -1
            (pm, qm, r)[which][-1, limb] = P - 1
            assert call(pm, qm, r) == 0


def test_opening_requests_outside_the_commitment_are_refused(ob):
    n = 7
    x, f = pai.inputs("uniform", n), pmi.family("uniform", n, 8)
    call = lambda opens: pmi.oracle_masked_rc(ob.lib(), x["values"], x["n_used"], x["pub"], n, f["r"], f["pri_mask"], f["pub_mask"], opens)[0]
    assert call([(0, 31), (1, 31), (2, 15)]) == 0
    assert call([(0, 32)]) == -2 and call([(2, 16)]) == -2 and call([(3, 0)]) == -2 and call([(-1, 0)]) == -2 and call([(0, -1)]) == -2


def test_masked_array_goldens_are_the_recorded_files():
    """tests/golden/pc_masked_array_*.bin (the oracle's masked entry at n = 18 with a mask that pads to 2^16 and at n = 20 with edge limbs and ms = N,
    make_pc_masked_array.py): the files are the ones the index was written for and the inputs regenerate to the recorded digests."""
    meta = json.load(open(os.path.join(GOLDEN, "pc_masked_array.json")))
    assert set(meta) == set(pmi.ARRAY_CASES)
    for name, m in meta.items():
        n, kind, fam, ms, cnt = pmi.ARRAY_CASES[name]
        rec = open(os.path.join(GOLDEN, m["record"]), "rb").read()
        assert hashlib.sha256(rec).hexdigest() == m["record_sha256"] and len(rec) == pmi.masked_record_bytes(n)
        x = pmi.array_case(name)
        assert (m["n"], m["ms"], m["m"], m["n_used"]) == (n, ms, cnt, x["n_used"]) and pmi.padded_length(n, x["pri_mask"].shape[0])[1] == ms
        for k, v in pmi.array_digests(x).items():
            assert m[k] == v, "input generator differs: " + k
        f = pmi.split_masked_record(rec, n)
        assert f["public"][-16:] != bytes(16) and f["final_mask"] != bytes(32 * 16)
        fm = np.frombuffer(f["final_mask"], np.uint64).reshape(32, 2)
        assert (fm == fm[0]).all() == (ms <= (1 << (n - 6)))                   # constant exactly when the mask fits a slice's message
    assert pmi.ARRAY_CASES["n18_m40000"][3] == 1 << 16 and pmi.ARRAY_CASES["n20_edges_m16384"][3] == 1 << (20 - 6)
