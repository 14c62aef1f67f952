"""vp_fft_gkr_fs (include/vpgpu.h): fft_gkr with every challenge drawn on the device from the Fiat-Shamir chain.  Every comparison is bit-exact.

The reference at any size needs no second implementation of the interleaving (tests/fft_gkr_fs_ref.py): if msgs = P(tape) for a prover P that takes its tape up
front and tape = derive(msgs) with hashlib, the pair is the one Fiat-Shamir transcript from that state.  So every case checks
  - tape_out and state_out are the hashlib derivation's from msgs,
  - msgs = vp_fft_gkr(tape_out) in both of its forms (fft_gkr_batched 1 and 0), at every size,
  - msgs = orc_fft_gkr_tape(tape_out) up to lg 13, and the oracle's embedded verifier accepts,
  - msgs, tape and state equal the Python non-interactive prover's at lg <= 6 (tests/test_fft_gkr_fs_host.py has checked those records on the CPU),
  - the launch table says which form ran: per sumcheck of R rounds max(0, R - T) round launches with their closing launches, then one tail.

Sizes, with T = VP_FFT_GKR_FS_TAIL_LOG = 11:  1 .. 4 tail only, tables of 2 .. 2^10 entries;  5 = T - 6: the addition layer (lg + 6 rounds) exactly fills the
tail;  6 = T - 5: its first round above the tail (one round launch, no fold in it, the tail folds on load);  11 = T: the 2^lg-entry sumchecks exactly fill the
tail, the addition layer runs six rounds above it (folds between the lane's two table sets);  12 = T + 1: every sumcheck has a round above the tail, with an add
table in the inverse-FFT layers;  13;  17 = x1024's size.
Refusals that can be reached from outside: null arguments, lg out of range, a short message buffer, a pending vp_fft_gkr_begin (a recording plan exists only
inside a library call)."""
import ctypes

import numpy as np
import pytest

import fft_gkr_fs_cases as fc
import fft_gkr_fs_ref as fr
import fft_gkr_ref as ref

pytestmark = pytest.mark.gpu

T = fc.tail_log()
SIZES = [1, 2, 3, 4, T - 6, T - 5, T, T + 1, 13, 17]
ORACLE_MAX = 13


class Ctx:
    def __init__(self, vp, **tuning):
        self.vp, self.L = vp, vp.lib_gpu()
        L = self.L
        vpt, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.vp_fft_gkr.argtypes = [vpt, ctypes.c_int, vpt, u64, vpt, u64, vpt]
        L.vp_fft_gkr_begin.argtypes = [vpt, ctypes.c_int, vpt, u64]
        L.vp_fft_gkr_end.argtypes = [vpt, vpt, u64, vpt]
        L.vp_fft_gkr_fs.argtypes = [vpt, ctypes.c_int, vpt, vpt, u64, vpt, vpt, vpt]
        L.vp_set_profiling.argtypes = [vpt, ctypes.c_int]
        L.vp_get_launch_stats.argtypes = [vpt, ctypes.POINTER(vp.LaunchStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.vp_last_error.restype = ctypes.c_char_p
        L.vp_last_error.argtypes = [vpt]
        self.c = ctypes.c_void_p()
        with pytest.MonkeyPatch.context() as mp:
            for k, v in vp.Options(**tuning).tuning_env().items():
                mp.setenv(k, v)
            assert L.vp_create_with_options(0, None, ctypes.byref(self.c)) == 0, "vp_create failed: the HIP extension must run on the GPU box"

    def fs_rc(self, lg, state, null=None, capacity=None):
        """vp_fft_gkr_fs as it is: (return code, msgs, tape, state_out); null: the argument passed as a null pointer"""
        msgs, tape = np.zeros((ref.n_msgs(max(1, min(lg, 19))), 2), np.uint64), np.zeros((ref.n_tape(max(1, min(lg, 19))), 2), np.uint64)
        si, so, nw = ctypes.create_string_buffer(bytes(state), 32), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        arg = {"state_in": ctypes.cast(si, ctypes.c_void_p), "msgs": msgs.ctypes.data, "tape_out": tape.ctypes.data, "state_out": ctypes.cast(so, ctypes.c_void_p)}
        if null:
            arg[null] = None
        rc = self.L.vp_fft_gkr_fs(self.c, lg, arg["state_in"], arg["msgs"], msgs.shape[0] if capacity is None else capacity, ctypes.byref(nw), arg["tape_out"],
                                  arg["state_out"])
        assert rc != 0 or nw.value == msgs.shape[0]
        return rc, msgs, tape, so.raw

    def fs(self, lg, state):
        rc, msgs, tape, so = self.fs_rc(lg, state)
        assert rc == 0, self.L.vp_last_error(self.c)
        return msgs, tape, so

    def tape_form(self, lg, tape):
        msgs, nw = np.zeros((ref.n_msgs(lg), 2), np.uint64), ctypes.c_uint64(0)
        t = np.ascontiguousarray(tape, np.uint64)
        assert self.L.vp_fft_gkr(self.c, lg, t.ctypes.data, t.shape[0], msgs.ctypes.data, msgs.shape[0], ctypes.byref(nw)) == 0, self.L.vp_last_error(self.c)
        return msgs

    def profiling(self, on):
        assert self.L.vp_set_profiling(self.c, 1 if on else 0) == 0

    def rows(self):
        n = ctypes.c_int(0)
        arr = (self.vp.LaunchStat * 1024)()
        assert self.L.vp_get_launch_stats(self.c, arr, 1024, ctypes.byref(n)) == 0
        return [(self.L.vp_kernel_name(e.kind).decode(), e.rounds, e.first_round, e.workgroups, e.work) for e in arr[:n.value]]

    def close(self):
        if self.c:
            self.L.vp_destroy(self.c)
            self.c = None


@pytest.fixture(scope="module")
def forms(vp):
    """One context per form of vp_fft_gkr: {1: batched (the default), 0: the per-depth loop}; vp_fft_gkr_fs runs on [1] unless a test says otherwise."""
    f = {b: Ctx(vp, fft_gkr_batched=b) for b in (1, 0)}
    yield f
    for c in f.values():
        c.close()


def check_run(forms, ob, lg, state_name, ctx=None):
    c = ctx or forms[1]
    s0 = fr.START_STATES[state_name]
    c.profiling(True)
    msgs, tape, so = c.fs(lg, s0)
    rows = c.rows()
    c.profiling(False)
    fc.assert_honest(lg, s0, msgs, tape, so)
    for b in (1, 0):
        assert forms[b].tape_form(lg, tape).tobytes() == msgs.tobytes(), "lg %d: vp_fft_gkr(tape_out), fft_gkr_batched=%d: other messages" % (lg, b)
    if lg <= ORACLE_MAX:
        raw, verified = ob.fft_gkr_tape(lg, tape)
        assert raw == msgs.tobytes() and verified, "lg %d: the oracle on tape_out" % lg
    if lg <= ref.MAX_LG:
        m_py, t_py, s_py = fc.python_fs(lg, state_name)
        assert msgs.tobytes() == m_py.tobytes() and tape.tobytes() == t_py.tobytes() and so == s_py, "lg %d: the Python non-interactive prover" % lg
    # which form ran
    want = fc.expected_rows(lg, T)
    assert [r[:3] for r in rows] == want, "lg %d: launch table" % lg
    assert all(r[3] == 1 for r in rows if r[0] != "k_round") and all(r[3] >= 1 and r[4] == 1 << (R - k) for r, (R, k) in
                                                                     zip([r for r in rows if r[0] == "k_round"],
                                                                         [(R, k) for R in fc.sumcheck_rounds(lg) for k in range(1, max(0, R - T) + 1)]))
    # chain steps by row: every message absorbed once, every slot drawn once
    assert sum(r[4] for r in rows if r[0] != "k_round") == fr.chain_steps(lg)
    return msgs, tape, so


@pytest.mark.parametrize("lg", SIZES)
def test_sizes_from_a_random_state(forms, ob, lg):
    check_run(forms, ob, lg, "random")


@pytest.mark.parametrize("state", ["zero", "ones"])
@pytest.mark.parametrize("lg", [2, T - 5, T + 1])
def test_start_states(forms, ob, lg, state):
    a = check_run(forms, ob, lg, state)
    b = forms[1].fs(lg, fr.START_STATES["random"])
    assert a[1].tobytes() != b[1].tobytes() and a[2] != b[2]


def test_per_depth_context_runs_the_same_entry_point(forms, ob):
    """vp_fft_gkr_fs on the context created with fft_gkr_batched = 0: the switch does not apply to it, the bytes are the same"""
    for lg in (3, T + 1):
        a = check_run(forms, ob, lg, "random", ctx=forms[0])
        b = forms[1].fs(lg, fr.START_STATES["random"])
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:2], b[:2])) and a[2] == b[2]


def test_determinism_and_order_on_one_context(forms, ob):
    """a second call gives the same bytes; sizes T + 1, 3, T + 1, T - 5, 1 on one context (the buffers are re-allocated at every change); a vp_fft_gkr runs
    before and after"""
    c = forms[1]
    s0 = fr.START_STATES["ones"]
    seen = {}
    t0 = np.array(fc.python_fs(4, "zero")[1])
    before = c.tape_form(4, t0)
    for lg in (T + 1, 3, T + 1, T - 5, 1):
        m, t, so = c.fs(lg, s0)
        m2, t2, so2 = c.fs(lg, s0)
        assert m.tobytes() == m2.tobytes() and t.tobytes() == t2.tobytes() and so == so2, "lg %d: a second call" % lg
        fc.assert_honest(lg, s0, m, t, so)
        if lg in seen:
            assert seen[lg] == (m.tobytes(), t.tobytes(), so), "lg %d: after other sizes" % lg
        seen[lg] = (m.tobytes(), t.tobytes(), so)
        assert c.tape_form(lg, t).tobytes() == m.tobytes()
    after = c.tape_form(4, t0)
    assert before.tobytes() == after.tobytes() == fc.python_fs(4, "zero")[0].tobytes()


def test_refusals_leave_the_context_as_it_was(forms):
    c = forms[1]
    s0 = fr.START_STATES["random"]
    lg = T - 5
    honest = c.fs(lg, s0)
    same = lambda: all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(c.fs(lg, s0)[:2], honest[:2])) and c.fs(lg, s0)[2] == honest[2]
    refused = []
    for null in ("state_in", "msgs", "tape_out", "state_out"):
        refused.append(("null " + null, c.fs_rc(lg, s0, null=null)[0]))
        assert same(), "after a null " + null
    for bad_lg in (0, -3, 20, 64):
        refused.append(("lg = %d" % bad_lg, c.fs_rc(bad_lg, s0)[0]))
        assert same(), "after lg = %d" % bad_lg
    refused.append(("a short message buffer", c.fs_rc(lg, s0, capacity=ref.n_msgs(lg) - 1)[0]))
    assert same()
    # a pending asynchronous run
    t = np.ascontiguousarray(honest[1])
    assert c.L.vp_fft_gkr_begin(c.c, lg, t.ctypes.data, t.shape[0]) == 0
    refused.append(("a pending vp_fft_gkr_begin", c.fs_rc(lg, s0)[0]))
    msgs, nw = np.zeros((ref.n_msgs(lg), 2), np.uint64), ctypes.c_uint64(0)
    assert c.L.vp_fft_gkr_end(c.c, msgs.ctypes.data, msgs.shape[0], ctypes.byref(nw)) == 0
    assert msgs.tobytes() == honest[0].tobytes(), "the pending run was disturbed by the refused call"
    assert same()
    assert all(rc != 0 for _, rc in refused), refused
    lims = dict(refused)
    assert lims["lg = 0"] == lims["lg = 20"] != lims["null msgs"], "lg out of range is VP_ELIMIT, a null argument VP_EINVAL"


def test_session_entry_point(vp, ob):
    """Session.fft_gkr_fs / Circuit.fft_gkr_fs_tape: the Python API over vph_fft_gkr_fs, whose host side re-derives the tape and the state"""
    c = vp.Circuit.randomize(3, 7, seed=1)
    s = vp.Session(c, device=0)
    try:
        for lg, state in ((3, "zero"), (T - 5, "random")):
            msgs, tape, so = s.fft_gkr_fs(lg, fr.START_STATES[state])
            m_py, t_py, s_py = fc.python_fs(lg, state)
            assert msgs.tobytes() == m_py.tobytes() and tape.tobytes() == t_py.tobytes() and so == s_py
            t2, s2 = vp.Circuit.fft_gkr_fs_tape(lg, fr.START_STATES[state], msgs)
            assert t2.tobytes() == tape.tobytes() and s2 == so and vp.Circuit.fft_gkr_check(lg, tape, msgs)
        with pytest.raises(ValueError):
            s.fft_gkr_fs(20, bytes(32))
    finally:
        s.close()
        c.close()
