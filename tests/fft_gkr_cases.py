"""The tapes of tests/test_fft_gkr_host.py (CPU: the Python reference against the oracle, the oracle's verifier on every tape) and tests/test_gpu_fft_gkr.py
(GPU: vp_fft_gkr against both).  One list, so that the GPU file adds no expectation the CPU suite has not checked.  A family is a function of (lg, seed) that
returns a canonical tape as an (n, 2) uint64 array in draw order (fft_gkr_ref.py); everything is seeded, and every tape, Python-reference record and oracle
record is computed once per process and never modified."""
import functools
import os

import numpy as np

import fft_gkr_ref as ref

P = ref.P
EDGE = (0, 1, 2, P - 2, P - 1)
SEED = 3396                  # the seed of tests/golden/fftgkr_lg{7,13,17}.bin: the uniform tape at those sizes is the real reference's own
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Offsets:
    """Where each draw sits on the tape (csrc/vpgpu_fftgkr.inc, FgkOffsets)."""

    def __init__(self, lg):
        self.lg = lg
        self.r, self.x = 0, lg
        self.r0 = self.x + 64
        self.r1 = self.r0 + lg + 10
        self.ru_a = self.r1 + lg + 10
        self.rv_a = self.ru_a + lg + 6
        self.ru_m = self.rv_a + lg + 6
        self.rv_m = self.ru_m + lg
        self.dep0 = self.rv_m + lg
        self.n = self.dep0 + lg * (2 * lg + 2)
        assert self.n == ref.n_tape(lg)

    def ru_d(self, d):
        return self.dep0 + d * (2 * self.lg + 2)

    def rv_d(self, d):
        return self.ru_d(d) + self.lg

    def alpha_d(self, d):
        return self.rv_d(d) + self.lg

    def beta_d(self, d):
        return self.alpha_d(d) + 1


def _rng(lg, seed, *key):
    return np.random.default_rng([int(seed), int(lg)] + [int(k) for k in key])


def _const(lg, re, im):
    t = np.zeros((ref.n_tape(lg), 2), np.uint64)
    t[:, 0], t[:, 1] = re, im
    return t


def uniform(lg, seed):
    import oracle_binding as ob
    return ob.random_seq(seed, ref.n_tape(lg))


def zero(lg, seed):
    """All zero: what vp_warm runs and throws away; as challenges, the corner 0...0."""
    return _const(lg, 0, 0)


def one(lg, seed):
    """All one: as challenges, the corner 1...1."""
    return _const(lg, 1, 0)


def minus_one(lg, seed):
    return _const(lg, P - 1, 0)


def minus_one_limbs(lg, seed):
    return _const(lg, P - 1, P - 1)


def corner_pattern(lg, seed):
    """Every element 0 or 1: eq tables are unit vectors, folds are selections, x_i in {0, 1}."""
    t = _const(lg, 0, 0)
    t[:, 0] = _rng(lg, seed, 1).integers(0, 2, ref.n_tape(lg))
    return t


def edge_real(lg, seed):
    t = _const(lg, 0, 0)
    t[:, 0] = np.array(EDGE, np.uint64)[_rng(lg, seed, 2).integers(0, 5, ref.n_tape(lg))]
    return t


def edge_both(lg, seed):
    return np.array(EDGE, np.uint64)[_rng(lg, seed, 3).integers(0, 5, (ref.n_tape(lg), 2))]


def _mid(lg):
    return (lg - 1) // 2     # a depth whose weights the next depth uses, as soon as there is one (lg >= 2)


def weights_zero(lg, seed):
    """alpha = beta = 0 after one middle depth: every later claim and g table is zero."""
    t, o = uniform(lg, seed), Offsets(lg)
    t[o.alpha_d(_mid(lg))] = 0
    t[o.beta_d(_mid(lg))] = 0
    return t


def alpha_zero(lg, seed):
    t, o = uniform(lg, seed), Offsets(lg)
    t[o.alpha_d(_mid(lg))] = 0
    return t


def beta_zero(lg, seed):
    t, o = uniform(lg, seed), Offsets(lg)
    t[o.beta_d(_mid(lg))] = 0
    return t


def points(lg, seed):
    """x_i cycling through 0 (0^0 = 1 in both tables of the two-table power form), 1, -1, i, the 2^lg-th root of unity, its inverse, a value that occurs
    many times, and one uniform value per cycle."""
    import oracle_binding as ob
    t, o = uniform(lg, seed), Offsets(lg)
    w = ob.root_of_unity(lg)
    dup = (int(t[o.x + 6, 0]), int(t[o.x + 6, 1]))
    cyc = [(0, 0), (1, 0), (P - 1, 0), (0, 1), w, ref.inv(w), dup, None]
    for i in range(64):
        if cyc[i % 8] is not None:
            t[o.x + i] = cyc[i % 8]
    return t


def dont_care(lg, seed):
    """The uniform tape with every draw the prover's messages do not depend on replaced: r_1[] (beta = 0 until the first depth has run), r_v of the addition
    and the multiplication layer (one-phase sumchecks), r_0[6..] (the outputs are 64), and the weights drawn after the last depth."""
    t, o = uniform(lg, seed), Offsets(lg)
    other = edge_both(lg, seed + 1)
    for a, n in ((o.r1, lg + 10), (o.rv_a, lg + 6), (o.rv_m, lg), (o.r0 + 6, lg + 4), (o.alpha_d(lg - 1), 2)):
        first = (int(t[a, 0]) + 1) % P              # differs from the uniform tape whatever the edge draw is
        t[a:a + n] = other[a:a + n]
        t[a, 0] = first
    return t


FAMILIES = {f.__name__: f for f in (uniform, zero, one, minus_one, minus_one_limbs, corner_pattern, edge_real, edge_both, weights_zero, alpha_zero,
                                    beta_zero, points, dont_care)}
CORNER_AND_EDGE = ("uniform", "zero", "one", "corner_pattern", "edge_real", "edge_both")

# The sizes of the GPU file, and which families run at each (tests/test_gpu_fft_gkr.py carries the table of what each size is there for)
REF_LGS = (1, 2, 3, 4, 5, 6)
ORACLE_CASES = ([(lg, f) for lg in (8, 9, 10, 14) for f in FAMILIES] + [(lg, f) for lg in (6, 11, 13, 15, 16) for f in CORNER_AND_EDGE] + [(17, "uniform")])
LOW_FOLD_CASES = [(lg, f) for lg in (12, 13) for f in ("uniform", "corner_pattern", "edge_both")]
SHAPES_CASES = [(14, "edge_both"), (3, "points"), (14, "corner_pattern"), (9, "weights_zero")]
ASYNC_CASES = [(9, "corner_pattern"), (9, "edge_both"), (5, "edge_real")]
GPU_ORACLE_CASES = sorted(set(ORACLE_CASES + LOW_FOLD_CASES + SHAPES_CASES + ASYNC_CASES))


@functools.lru_cache(maxsize=None)
def tape(family, lg):
    t = np.ascontiguousarray(FAMILIES[family](lg, SEED), np.uint64)
    assert t.shape == (ref.n_tape(lg), 2) and int(t.max()) < P
    t.setflags(write=False)
    return t


def golden(lg):
    return open(os.path.join(GOLDEN, "fftgkr_lg%d.bin" % lg), "rb").read()


@functools.lru_cache(maxsize=None)
def oracle(family, lg):
    """(message bytes, verified) of orc_fft_gkr_tape on the family's tape."""
    import oracle_binding as ob
    return ob.fft_gkr_tape(lg, tape(family, lg))


@functools.lru_cache(maxsize=None)
def expected(family, lg):
    """What the device must return.  dont_care: the uniform tape's record.  The uniform tape at lg 7 / 13 / 17 is the real reference's own draw sequence:
    its record is on file (tests/test_fft_gkr_host.py pins orc_fft_gkr_tape to it), and the oracle is not run again."""
    if family == "dont_care":
        return expected("uniform", lg)
    if family == "uniform" and lg in (7, 13, 17):
        return golden(lg)
    return oracle(family, lg)[0]


@functools.lru_cache(maxsize=None)
def python_reference(family, lg):
    import oracle_binding as ob
    return ref.to_bytes(ref.prove(lg, [(int(a), int(b)) for a, b in tape(family, lg)], ob.root_of_unity(lg)))


def locate(lg, idx):
    """Message element idx in words: output / layer / depth / phase / round."""
    if idx < 64:
        return "output %d" % idx
    idx -= 64
    for name, rounds in [("addition layer", lg + 6), ("multiplication layer", lg)] + [("inverse FFT depth %d phase %d" % (d, ph), lg) for d in range(lg) for ph in (1, 2)]:
        if idx < 3 * rounds:
            return "%s, round %d, coefficient %s" % (name, idx // 3 + 1, "abc"[idx % 3])
        if idx == 3 * rounds:
            return "%s, claimed value" % name
        idx -= 3 * rounds + 1
    raise IndexError("message element out of range")


def first_difference(lg, got, want):
    """None, or a description of the first message element in which two records differ."""
    if got == want:
        return None
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    i = next(i for i in range(len(got) // 16) if got[16 * i:16 * i + 16] != want[16 * i:16 * i + 16])
    pair = lambda b: (int.from_bytes(b[16 * i:16 * i + 8], "little"), int.from_bytes(b[16 * i + 8:16 * i + 16], "little"))
    return "fft_gkr(lg=%d): first differing message element %d of %d (%s): %r, expected %r" % (lg, i, len(got) // 16, locate(lg, i), pair(got), pair(want))
