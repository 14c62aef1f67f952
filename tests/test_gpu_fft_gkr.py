"""vp_fft_gkr on arbitrary tapes, in both of its forms, at every size where its launch sequence changes.  Every comparison is bit-exact on the whole message
buffer: against the Python-integer prover (fft_gkr_ref.py) at lg 1 .. 6, against the oracle on the caller's tape (orc_fft_gkr_tape) above that, and the two
forms against each other.  Tapes: fft_gkr_cases.py (uniform, constant, corner challenges, edge limbs, zero weights, special evaluation points, changed
don't-care draws); tests/test_fft_gkr_host.py has checked every expectation used here on the CPU.

The two forms (fft_gkr_batched, VP_FFT_GKR_BATCHED, read in vp_create):
  1  the 2 lg inverse-FFT sumchecks as one batch: k_fg_gtab_multi, k_fg_dot_multi (v_u as an inner product), k_fg_ifft_multi, then the RECORDED launches of
     run_sumcheck_seg merged step by step (k_sumfold3b_multi, k_seg_multi, k_emit_multi); fold kernel from 2^sf_big_log (14) entries on.
  0  depth by depth: k_fg_gtab, k_fg_ifft_p1, a DIRECT run_sumcheck_seg with an add table (k_sumfold3b<true>, k_seg<true>, k_emit), v_u read from that
     sumcheck's closing kernel, k_fg_ifft_p2, the second sumcheck; fold kernel from 2^SF_BIG_LOG (17) entries on.
The addition layer (2^(lg+6) entries, no add table) and the multiplication layer (2^lg, none) run directly in both forms.

What each size is there for, read from run_sumcheck_seg (csrc/vpgpu_batched.inc) and fg_lb (csrc/vp_kernels_fftgkr.h).  A sumcheck over 2^n entries runs
fold launches (3 rounds each) while the table has >= 2^T entries, then k_seg launches of min(10, log2 len) rounds, then k_emit on what is left.  With seg_tiny
(default 1) the first launch of a sumcheck is a k_seg even for a table k_emit could hold (2^6), so below n = 10 k_emit only retires a one-entry table — the
2^6 capacity of k_emit is reached from above (n = 16: segment -> 64 entries), not at lg = 6 as a stand-alone closing launch.

  lg   2^lg-entry sumchecks (T = 14 recorded / 17 direct)            addition layer, n = lg + 6 (direct, T = 17)       power tables (fg_lb)
  1-5  one k_seg of lg rounds, one segment -> k_emit retires          seg(7..10 rounds) -> k_emit on 1 .. 2 entries       one table
  6    seg(6) -> 1                                                    seg(10) -> 4 entries in k_emit                      one table
  8    seg(8) -> 1                                                    seg(10) -> 16                                       one table
  9    seg(9) -> 1: the last size with one segment of < 2^10          seg(10) -> 32                                       lb = 9 = lg: last one-table size
  10   seg(10) -> 1: a full segment, the loop ends by length          seg(10) -> 64: k_emit at its capacity               first size with a Q table (2 entries per point)
  11   seg(10) -> 2 entries in k_emit (two segments)                  fold -> 2^14 -> seg(10) -> 16: first fold launch    Q: 4
  13   seg(10) -> 8                                                   fold -> 2^16 -> seg -> 64
  14   recorded: fold -> 2^11 -> seg -> 2; direct: seg -> 16          fold, fold -> 2^14 -> seg -> 16
  15   recorded: fold -> 2^12 -> seg -> 4; direct: seg -> 32          fold, fold -> 2^15 -> seg -> 32
  16   recorded: fold -> 2^13 -> seg -> 8; direct: seg -> 64          fold, fold -> 2^16 -> seg -> 64
  17   recorded: fold, fold -> 2^11 -> seg -> 2; direct: fold -> 2^14 -> seg -> 16 — k_sumfold3b<true> (form 0) and, for the multiplication layer,
       k_sumfold3b<false> at its smallest table
  12, 13 with VP_SF_BIG_LOG = 12 (batched): fold -> 2^9 -> seg(9) -> 1 and fold -> 2^10 -> seg(10) -> 1: the merged fold launch on its smallest table,
       leaving 2^9 entries (SF_MIN_LOG)."""
import ctypes

import numpy as np
import pytest

import fft_gkr_cases as fc
import fft_gkr_ref as ref

pytestmark = pytest.mark.gpu


class Stats(ctypes.Structure):
    _fields_ = [("gkr_ms", ctypes.c_double), ("evaluate_ms", ctypes.c_double), ("fold_ms", ctypes.c_double), ("fold_launches", ctypes.c_uint64),
                ("fold_bytes", ctypes.c_uint64), ("rounds", ctypes.c_uint64), ("launches", ctypes.c_uint64)]


class Ctx:
    """A context created under the tuning switches given (the library reads them in vp_create, nowhere else)."""

    def __init__(self, vp, **tuning):
        self.L = L = vp.lib_gpu()
        vpt, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.vp_fft_gkr_sizes.argtypes = [ctypes.c_int, vpt, vpt]
        L.vp_fft_gkr.argtypes = [vpt, ctypes.c_int, vpt, u64, vpt, u64, vpt]
        L.vp_fft_gkr_begin.argtypes = [vpt, ctypes.c_int, vpt, u64]
        L.vp_fft_gkr_end.argtypes = [vpt, vpt, u64, vpt]
        L.vp_tuning_get.argtypes = [vpt, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
        L.vp_get_stats.argtypes = [vpt, ctypes.POINTER(Stats)]
        L.vp_last_error.restype = ctypes.c_char_p
        L.vp_last_error.argtypes = [vpt]
        self.c = ctypes.c_void_p()
        with pytest.MonkeyPatch.context() as mp:
            for k, v in vp.Options(**tuning).tuning_env().items():
                mp.setenv(k, v)
            assert L.vp_create_with_options(0, None, ctypes.byref(self.c)) == 0, "vp_create failed: the HIP extension must run on the GPU box"
        for k, v in tuning.items():
            assert self.tuning(k) == v

    def tuning(self, name):
        v = ctypes.c_int32(-1)
        assert self.L.vp_tuning_get(self.c, name.encode(), ctypes.byref(v)) == 0
        return v.value

    def sizes(self, lg):
        nt, nm = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert self.L.vp_fft_gkr_sizes(lg, ctypes.byref(nt), ctypes.byref(nm)) == 0
        assert (nt.value, nm.value) == (ref.n_tape(lg), ref.n_msgs(lg))
        return nt.value, nm.value

    def run(self, lg, tape):
        nt, nm = self.sizes(lg)
        tape = np.ascontiguousarray(tape, np.uint64)
        assert tape.shape == (nt, 2)
        msgs, nw = np.zeros((nm, 2), np.uint64), ctypes.c_uint64(0)
        rc = self.L.vp_fft_gkr(self.c, lg, tape.ctypes.data, nt, msgs.ctypes.data, nm, ctypes.byref(nw))
        assert rc == 0, self.L.vp_last_error(self.c)
        assert nw.value == nm
        return msgs.tobytes()

    def begin(self, lg, tape):
        tape = np.array(tape, np.uint64)
        assert self.L.vp_fft_gkr_begin(self.c, lg, tape.ctypes.data, tape.shape[0]) == 0, self.L.vp_last_error(self.c)
        tape[:] = 0                                            # the call keeps its own copy

    def end(self, lg):
        nm = ref.n_msgs(lg)
        msgs, nw = np.zeros((nm, 2), np.uint64), ctypes.c_uint64(0)
        assert self.L.vp_fft_gkr_end(self.c, msgs.ctypes.data, nm, ctypes.byref(nw)) == 0, self.L.vp_last_error(self.c)
        assert nw.value == nm
        return msgs.tobytes()

    def rounds(self):
        st = Stats()
        assert self.L.vp_get_stats(self.c, ctypes.byref(st)) == 0
        return st.rounds

    def close(self):
        if self.c:
            self.L.vp_destroy(self.c)
            self.c = None


@pytest.fixture(scope="module")
def forms(vp):
    """One context per form: {1: batched (the default), 0: the per-depth loop}."""
    f = {b: Ctx(vp, fft_gkr_batched=b) for b in (1, 0)}
    yield f
    for c in f.values():
        c.close()


def check(lg, got, want, what):
    d = fc.first_difference(lg, got, want)
    assert d is None, "%s: %s" % (what, d)


def check_both_forms(forms, lg, family, want, against):
    t = fc.tape(family, lg)
    got = {b: forms[b].run(lg, t) for b in (1, 0)}
    for b in (1, 0):
        check(lg, got[b], want, "%s tape, fft_gkr_batched=%d, against %s" % (family, b, against))
    check(lg, got[0], got[1], "%s tape, per-depth loop against the batch" % family)


def test_switch_in_effect(forms):
    """fft_gkr_batched = 0 runs the per-depth loop: the context says so (vp_tuning_get), and its sumcheck rounds say so — the per-depth loop drives 2 lg
    sumchecks of lg rounds through run_sumcheck_seg in every call, the batch replays recorded launches (run_sumcheck_seg runs for them once per size, when the
    batch is recorded).  The two buffers are the same bytes."""
    assert forms[1].tuning("fft_gkr_batched") == 1 and forms[0].tuning("fft_gkr_batched") == 0
    assert forms[1].tuning("sf_big_log") == 14
    lg, t = 7, fc.tape("edge_both", 7)
    got = {}
    for b in (1, 0):
        forms[b].run(lg, t)
        got[b] = forms[b].run(lg, t)                         # the second call at this size: nothing is recorded in it
    assert forms[1].rounds() == (lg + 6) + lg
    assert forms[0].rounds() == (lg + 6) + lg + 2 * lg * lg
    check(lg, got[0], got[1], "per-depth loop against the batch")
    check(lg, got[1], fc.oracle("edge_both", lg)[0], "batch against the oracle")


@pytest.mark.parametrize("family", list(fc.FAMILIES))
@pytest.mark.parametrize("lg", fc.REF_LGS)
def test_device_vs_python_reference(forms, lg, family):
    want = fc.python_reference("uniform" if family == "dont_care" else family, lg)
    check_both_forms(forms, lg, family, want, "the Python reference")


@pytest.mark.parametrize("lg,family", fc.ORACLE_CASES)
def test_device_vs_oracle(forms, ob, lg, family):
    check_both_forms(forms, lg, family, fc.expected(family, lg), "the oracle")


def test_lowered_fold_threshold(vp, ob):
    """VP_SF_BIG_LOG = 12 on a batched context: the merged fold launch at lg 12 (2^12 -> 2^9, its floor) and 13 (-> 2^10, one full segment)."""
    c = Ctx(vp, fft_gkr_batched=1, sf_big_log=12)
    try:
        for lg, family in fc.LOW_FOLD_CASES:
            check(lg, c.run(lg, fc.tape(family, lg)), fc.expected(family, lg), "%s tape, sf_big_log=12" % family)
    finally:
        c.close()


def test_one_context_many_shapes(forms, ob):
    """Sizes 14, 3, 14, 9 on one context: the buffers are re-allocated and the batch is recorded again at every change of size."""
    for b in (1, 0):
        for lg, family in fc.SHAPES_CASES:
            check(lg, forms[b].run(lg, fc.tape(family, lg)), fc.expected(family, lg), "%s tape, fft_gkr_batched=%d" % (family, b))


def test_asynchronous_form(forms, ob):
    """vp_fft_gkr_begin / vp_fft_gkr_end return the bytes of the synchronous call; a synchronous call at another size follows on the same context."""
    (lg, f1), (_, f2), (lg2, f3) = fc.ASYNC_CASES
    for b in (1, 0):
        c = forms[b]
        for family in (f1, f2):
            t = fc.tape(family, lg)
            sync = c.run(lg, t)
            c.begin(lg, t)
            check(lg, c.end(lg), sync, "%s tape, begin / end against the one-call form, fft_gkr_batched=%d" % (family, b))
            check(lg, sync, fc.expected(family, lg), "%s tape, fft_gkr_batched=%d" % (family, b))
        check(lg2, c.run(lg2, fc.tape(f3, lg2)), fc.expected(f3, lg2), "%s tape after the asynchronous runs, fft_gkr_batched=%d" % (f3, b))
