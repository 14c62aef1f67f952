"""Shared by tests/test_fft_gkr_fs_host.py (CPU) and tests/test_gpu_fft_gkr_fs.py (GPU): the Python non-interactive prover's records (fft_gkr_fs_ref.prove, lg <= 6),
computed once per process and never modified, so that the GPU file compares against nothing the CPU suite has not checked."""
import functools
import os
import re

import numpy as np

import fft_gkr_fs_ref as fr
import fft_gkr_ref as ref

REF_LGS = (1, 2, 3, 4, 5, 6)
STATES = tuple(fr.START_STATES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def python_fs(lg, state_name):
    """(msgs, tape) as read-only (n, 2) uint64 arrays and the closing state"""
    import oracle_binding as ob
    msgs, tape, st = fr.prove(lg, fr.START_STATES[state_name], ob.root_of_unity(lg))
    m, t = np.array(msgs, np.uint64).reshape(-1, 2), np.array(tape, np.uint64).reshape(-1, 2)
    m.setflags(write=False)
    t.setflags(write=False)
    return m, t, st


def tail_log():
    """VP_FFT_GKR_FS_TAIL_LOG as include/vpgpu.h exports it"""
    hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    return int(re.search(r"^#define VP_FFT_GKR_FS_TAIL_LOG (\d+)$", hdr, flags=re.M).group(1))


def sumcheck_rounds(lg):
    """rounds of every sumcheck of fft_gkr(lg), in order: addition, multiplication, then per depth phase 1 and phase 2"""
    return [lg + 6, lg] + [lg] * (2 * lg)


def expected_rows(lg, T):
    """The launch table of vp_fft_gkr_fs by the header's rules, as (vp_kernel_name of the row's id, rounds, first_round) in order: two drawing launches, then per sumcheck of R
    rounds max(0, R - T) times (round, closing launch) and one tail of min(R, T) rounds."""
    rows = [("k_merkle", 0, 0), ("k_merkle", 0, 0)]
    for R in sumcheck_rounds(lg):
        above = max(0, R - T)
        for k in range(1, above + 1):
            rows += [("k_round", 1, k), ("k_emit_multi", 1, k)]
        rows.append(("k_seg_multi", R - above, above + 1))
    return rows


def assert_honest(lg, state, msgs, tape, state_out):
    """what every honest run satisfies, whatever computed it: the tape and the closing state are the hashlib derivation's from the messages"""
    t, s = fr.derive(lg, state, msgs)
    got = np.ascontiguousarray(tape, np.uint64)
    want = np.array(t, np.uint64).reshape(-1, 2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "lg %d: tape slot %d is not the chain's" % (lg, bad[0])
    assert bytes(state_out) == s, "lg %d: the closing state is not the chain's" % lg
    assert got.shape == (ref.n_tape(lg), 2) and int(got.max()) < ref.P
