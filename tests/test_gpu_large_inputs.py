"""Input layers of 2^24 and 2^25 wires: the commitment's transforms of 2^18 / 2^19 points (vp_kernels_ntt_long.h), the commitment, FRI and
openings sized from n up to 25, and the limit above it (the reference's commitment indexes its codeword with int: poly_commit.h:87-166)."""
import ctypes

import numpy as np
import pytest

import test_gpu_parity as parity
from test_gpu_parity import _sharded_commitment_case

pytestmark = pytest.mark.gpu
P = (1 << 61) - 1
VP_ELIMIT = -5


@pytest.fixture(scope="module")
def ctx(vp):
    lib = vp.lib_gpu()
    h = ctypes.c_void_p()
    assert lib.vp_create(0, ctypes.byref(h)) == 0, "vp_create failed: the HIP extension must run on the GPU box"
    yield h
    lib.vp_destroy(h)


@pytest.mark.parametrize("ln,ratio", [(18, 1), (18, 32), (19, 1), (19, 32)])
def test_long_fft_vs_oracle(vp, ob, ctx, ln, ratio):
    """fast_fourier_transform / its inverse (RS_polynomial.cpp:26-220) at 2^18 and 2^19 points: the sizes of the slices of n = 24 / 25."""
    rng = np.random.default_rng(1000 + ln * 7 + ratio)
    n = 1 << ln
    c = rng.integers(0, P, size=(n, 2), dtype=np.uint64)
    out = np.zeros((n * ratio, 2), dtype=np.uint64)
    exp = np.zeros_like(out)
    lib = vp.lib_gpu()
    assert lib.vp_test_fft(ctx, c.ctypes.data, n, n * ratio, 0, out.ctypes.data) == 0
    ob.lib().orc_fft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    ob.lib().orc_fft(c.ctypes.data, n, n * ratio, exp.ctypes.data)
    assert np.array_equal(out, exp)
    if ratio == 1:
        back = np.zeros_like(c)
        assert lib.vp_test_fft(ctx, out.ctypes.data, n, n, 1, back.ctypes.data) == 0
        assert np.array_equal(back, c)
    assert lib.vp_test_fft(ctx, c.ctypes.data, 1 << 20, 1 << 20, 0, out.ctypes.data) == VP_ELIMIT     # 2^20 points: above any slice


@pytest.mark.parametrize("mode", [1, 32, 0])
@pytest.mark.parametrize("ln", [18, 19])
def test_long_fft_structured_inputs_vs_oracle(vp, ob, ctx, ln, mode):
    """The radix-2 (2^18) and radix-4 (2^19) merges of vp_kernels_ntt_long.h on constant / spike / alternating / real / imaginary vectors (the lazy
    butterflies at differences of exactly 2p: tests/test_gpu_field_edges.py), forward at ratio 1 and 32 and the inverse against orc_ifft on the same input."""
    from test_gpu_field_edges import structured_fft_case
    structured_fft_case(vp, ob, ctx, ln, mode)


@pytest.mark.parametrize("lg", [18, 19])
def test_fft_gkr_long_vs_oracle(vp, ob, ctx, lg):
    """fft_gkr (fft_circuit_GKR.cpp:833-849) at lg = n - 6 of the n = 24 / 25 commitments, against the oracle's restatement (same checks as at lg <= 17)."""
    parity.test_fft_gkr_vs_reference_record_and_oracle(vp, ob, ctx, lg)


def test_commitment_refuses_more_than_2_25_wires(vp):
    """n = 26 is VP_ELIMIT with a message (the reference's int index overflows there); n = 25 commits."""
    lib = vp.lib_gpu()
    inputs = np.random.default_rng(3).integers(0, P, size=(4096, 2), dtype=np.uint64)
    for bits, want in ((26, VP_ELIMIT), (25, 0)):
        h = ctypes.c_void_p()
        assert lib.vp_create(0, ctypes.byref(h)) == 0
        try:
            assert lib.vp_pc_load_input(h, inputs.ctypes.data, inputs.shape[0], bits) == 0
            root = ctypes.create_string_buffer(32)
            rc = lib.vp_commit_private(h, ctypes.cast(root, ctypes.c_void_p))
            assert rc == want, lib.vp_last_error(h)
            if want:
                assert b"2^25" in lib.vp_last_error(h)
            else:
                assert root.raw != bytes(32)
        finally:
            lib.vp_destroy(h)


def test_random_circuit_n25_complete_protocol_and_sharded_commitment(vp):
    """A random circuit with an input layer of 2^25 wires: the complete protocol (commitment, GKR, fft_gkr at lg 19, FRI over 19 levels, 33 query
    openings) accepted by the host verifier; then the commitment of the same input layer sharded over 2 ranks gives the same roots, sums and final
    codeword, and the owners' openings verify."""
    c = vp.Circuit.randomize(2, 25, seed=5)
    n = c.layer_bitlen(0)
    assert n == 25
    s = vp.Session(c)
    trf, ok, _ = s.prove_and_verify_full(reps=33)
    assert ok, "host verifier rejected the n = 25 proof"
    roots, fin, r = s.last_fri()
    st = n - 6
    assert len(roots) == 32 * st and r.shape == (st, 2)
    tail = trf[-(32 + 16 + 65 * 16):]
    inputs = s.layer_values(0)
    pub = s.eq_table(s.last_point())
    s.close(); c.close()            # the unsharded commitment's device memory goes before the two ranks take theirs
    _sharded_commitment_case(vp, inputs, n, pub, r, 2, trf[:32], tail, roots, fin)


def test_sha256_x2048_vs_oracle(vp, pws_path):
    """SHA-256 x2048: input layer 2^24 (65 slices of 2^23 code symbols, transforms of 2^18 points).  GKR transcript and commitment outputs against
    the oracle's (tests/golden/make_oracle_fixture_gkr.py oracle 2048, make_oracle_fixture_pc.py 2048); the complete protocol with 33 query
    repetitions accepted by the host verifier; the commitment sharded over 8 ranks equals the unsharded one (roots, sums, FRI roots, final codeword)."""
    import json
    import os
    from conftest import GOLDEN
    gold_gkr = open(os.path.join(GOLDEN, "oracle_sha256_x2048_gkr.bin"), "rb").read()
    meta = json.load(open(os.path.join(GOLDEN, "oracle_sha256_x2048_gkr.bin.json")))
    exp = open(os.path.join(GOLDEN, "oracle_sha256_x2048_pc.bin"), "rb").read()
    c = vp.Circuit.from_pws(pws_path, 2048, seed=1)
    assert c.hash() == meta["circuit_hash"]
    n = c.layer_bitlen(0)
    assert n == 24
    s = vp.Session(c)
    s.draw_tape()
    tr, res = s.prove_gkr()
    assert tr == gold_gkr and res["rounds"] == meta["rounds"]
    root, _ = s.commit_private()
    assert root == exp[:32]
    pub = np.random.default_rng(8).integers(0, P, size=(1 << n, 2), dtype=np.uint64)
    root_h, inner, all_sum, _ = s.commit_public(pub)
    assert root_h == exp[32:64] and inner == exp[64:80] and all_sum == exp[80:]
    del pub
    trf, ok, _ = s.prove_and_verify_full(reps=33)
    assert ok, "host verifier rejected the x2048 proof"
    roots, fin, r = s.last_fri()
    assert len(roots) == 32 * (n - 6)
    inputs = s.layer_values(0)
    pub = s.eq_table(s.last_point())
    s.close(); c.close()
    _sharded_commitment_case(vp, inputs, n, pub, r, 8, trf[:32], trf[-(32 + 16 + 65 * 16):], roots, fin)
