"""fft_gkr off the seeded tapes, CPU side: the oracle's tape entry (orc_fft_gkr_tape) against its seeded entry and the real reference's records, the
Python-integer prover (fft_gkr_ref.py) against the oracle byte for byte on every tape family (fft_gkr_cases.py) at lg 1 .. 6, and the oracle's embedded
verifier on every (family, lg) tests/test_gpu_fft_gkr.py hands to the device — completeness holds for any tape, so a rejected one is a broken test input."""
import numpy as np
import pytest

import fft_gkr_cases as fc
import fft_gkr_ref as ref

P = ref.P


@pytest.mark.parametrize("lg", [1, 2, 3, 6, 7, 10, 13, 17])
def test_tape_entry_on_the_seeded_draws_returns_the_seeded_record(ob, lg):
    """orc_fft_gkr_tape fed orc_f_random_seq(3396) = orc_fft_gkr(lg, 3396); at lg 7 / 13 / 17 that is the real reference's record on file (lg 17 is compared
    with the file alone: tests/test_oracle_golden.py pins the seeded entry to it)."""
    assert ob.lib().orc_fft_gkr_draws(lg) == ref.n_tape(lg) == fc.Offsets(lg).n and ob.fft_gkr_msgs(lg) == ref.n_msgs(lg)
    got, ok = fc.oracle("uniform", lg)
    assert ok == 1
    if lg in (7, 13, 17):
        assert fc.first_difference(lg, got, fc.golden(lg)) is None
    if lg != 17:
        assert (got, 1) == ob.fft_gkr_seeded(lg, fc.SEED)
        again, ok = ob.fft_gkr_tape(lg, ob.random_seq(77, ref.n_tape(lg)))
        assert (again, ok) == ob.fft_gkr_seeded(lg, 77) and again != got


def test_tape_entry_refusals(ob):
    lg = 4
    t = np.array(fc.tape("uniform", lg))
    n, full = t.shape[0], 16 * ref.n_msgs(lg)
    assert ob.fft_gkr_tape_rc(lg, t)[0] == full
    assert ob.fft_gkr_tape_rc(0, t)[0] == -2 and ob.fft_gkr_tape_rc(25, t)[0] == -2
    assert ob.fft_gkr_tape_rc(lg, t, n_tape=n - 1)[0] == -3                        # a short count, a long count, another size's count: an error of its own
    assert ob.fft_gkr_tape_rc(lg, np.concatenate([t, t[:1]]))[0] == -3
    assert ob.fft_gkr_tape_rc(lg + 1, t)[0] == -3
    assert ob.lib().orc_fft_gkr_tape(lg, None, n, None, 0, None) == -3
    assert ob.fft_gkr_tape_rc(lg, t, capacity=full - 1)[0] == -1
    for at, limb, v in ((0, 0, P), (n - 1, 1, P), (n // 2, 0, 2 ** 64 - 1), (fc.Offsets(lg).r1, 1, P)):      # a don't-care position is checked too
        bad = t.copy()
        bad[at, limb] = v
        assert ob.fft_gkr_tape_rc(lg, bad)[0] == -4
        bad[at, limb] = P - 1
        assert ob.fft_gkr_tape_rc(lg, bad)[0] == full


def test_families_are_what_they_say():
    for lg in (1, 4, 9):
        o, u = fc.Offsets(lg), fc.tape("uniform", lg)
        assert set(np.unique(fc.tape("corner_pattern", lg))) == {0, 1} and not fc.tape("corner_pattern", lg)[:, 1].any()
        assert not fc.tape("zero", lg).any() and (fc.tape("one", lg) == [1, 0]).all() and (fc.tape("minus_one_limbs", lg) == P - 1).all()
        assert set(np.unique(fc.tape("edge_both", lg))) <= set(fc.EDGE) and not fc.tape("edge_real", lg)[:, 1].any() and fc.tape("edge_both", lg)[:, 1].any()
        d = fc._mid(lg)
        for name, za, zb in (("weights_zero", True, True), ("alpha_zero", True, False), ("beta_zero", False, True)):
            t = fc.tape(name, lg)
            assert (not t[o.alpha_d(d)].any()) == za and (not t[o.beta_d(d)].any()) == zb
            assert (np.flatnonzero((t != u).any(axis=1)) >= o.alpha_d(d)).all()
        x = fc.tape("points", lg)[o.x:o.x + 64]
        assert [tuple(int(v) for v in e) for e in x[:4]] == [(0, 0), (1, 0), (P - 1, 0), (0, 1)] and (x[6] == x[14]).all() and (x[7] != x[15]).any()
        assert ref.mul(tuple(int(v) for v in x[4]), tuple(int(v) for v in x[5])) == ref.ONE
        moved = np.flatnonzero((fc.tape("dont_care", lg) != u).any(axis=1))
        for a in (o.r1, o.rv_a, o.rv_m, o.r0 + 6, o.alpha_d(lg - 1)):
            assert a in moved
        keep = set(range(o.r0 + 6)) | set(range(o.ru_a, o.rv_a)) | set(range(o.ru_m, o.rv_m)) | set(range(o.dep0, o.alpha_d(lg - 1)))
        assert not keep & set(moved.tolist())
    assert fc.locate(3, 0) == "output 0" and fc.locate(3, 64) == "addition layer, round 1, coefficient a"
    assert fc.locate(3, 64 + 27) == "addition layer, claimed value" and fc.locate(3, 64 + 28 + 10 + 10 + 4) == "inverse FFT depth 0 phase 2, round 2, coefficient b"
    assert fc.locate(3, ref.n_msgs(3) - 1) == "inverse FFT depth 2 phase 2, claimed value"
    with pytest.raises(IndexError):
        fc.locate(3, ref.n_msgs(3))


def test_outputs_known_without_running_anything(ob):
    """With r in {0,1}^lg the expansion E is a unit vector: S[j] = N^-1 w^(-jm) for its index m, so the output at x_i = 1 is sum_j S[j] = E[0] in {0, 1} and the
    output at x_i = 0 is S[0] = N^-1 (0^0 = 1).  Both records carry exactly that."""
    for lg in fc.REF_LGS:
        inv_n = ref.inv((1 << lg, 0))
        for family in ("zero", "one", "corner_pattern"):
            t = fc.tape(family, lg)
            e0 = (1, 0) if t[:lg, 0].all() else (0, 0)                            # E[0] = prod_i r[i]
            for rec in (fc.python_reference(family, lg), fc.oracle(family, lg)[0]):
                for i in range(64):
                    out = (int.from_bytes(rec[16 * i:16 * i + 8], "little"), int.from_bytes(rec[16 * i + 8:16 * i + 16], "little"))
                    assert out == (e0 if t[lg + i, 0] else inv_n)


@pytest.mark.parametrize("family", list(fc.FAMILIES))
@pytest.mark.parametrize("lg", fc.REF_LGS)
def test_python_reference_vs_oracle(ob, lg, family):
    """Byte for byte, whole record; the Python prover's own checks (the two sums over S, q(0) + q(1) = claim in every round) run inside prove()."""
    got, (want, ok) = fc.python_reference(family, lg), fc.oracle(family, lg)
    assert ok == 1
    assert fc.first_difference(lg, got, want) is None, fc.first_difference(lg, got, want)
    assert fc.first_difference(lg, got, fc.expected(family, lg)) is None


@pytest.mark.parametrize("lg", sorted({lg for lg, _ in fc.GPU_ORACLE_CASES}))
def test_oracle_accepts_every_tape_the_gpu_tests_use(ob, lg):
    for family in sorted({f for l, f in fc.GPU_ORACLE_CASES if l == lg}):
        rec, ok = fc.oracle(family, lg)
        assert ok == 1, family
        assert len(rec) == 16 * ref.n_msgs(lg)
        if family == "dont_care":
            assert not np.array_equal(fc.tape(family, lg), fc.tape("uniform", lg))
            assert fc.first_difference(lg, rec, fc.oracle("uniform", lg)[0]) is None, "the oracle's messages moved with a draw they do not depend on"
