"""The challenge tapes of tests/test_gkr_tape_host.py (CPU: the oracle's prover and verifier and the host verifier on every tape, the zero shares) and
tests/test_gpu_gkr_tapes.py (GPU: every device path of the GKR sumcheck against the oracle on the same tape).  One list, so that the GPU file adds no
expectation the CPU suite has not checked.  A family is a function of (Offsets, seed) that returns a canonical tape as an (n, 2) uint64 array in the draw
order of include/vpgpu.h (vp_prove_gkr); everything is seeded, and every circuit, tape and oracle transcript is computed once per process and never modified.

VALUE families (the oracle's transcript is at most half zero elements, asserted per (circuit, family) in test_gkr_tape_host.py; measured 0.00 - 0.40):
    uniform, sprinkle, stripes_{k}_{val} (12), edge_limbs_real, edge_limbs_complex, uv_corners, sig_zero_mid, sig_first_only, assert_0, assert_1, assert_m1,
    dont_care (whose transcript is uniform's).
DEGENERATE families (compared byte for byte as well, but most of their transcript is zero — measured 0.65 - 1.00 — so a match there is weak evidence):
    zero, one, minus_one, minus_one_limbs, corner_pattern."""
import functools

import numpy as np

import custom_circuits as cc

P = cc.P
SEED = 3396                   # F::init(): the uniform tape is the draw sequence of the real reference, so its transcripts are the golden records
EDGE_VALUES = (0, 1, 2, P - 2, P - 1)                                                   # the witness values of tests/test_gpu_field_edges.py
EDGE_LIMBS = (0, 1, 2, (1 << 31) - 1, (1 << 31) + 1, 1 << 60, P - 2, P - 1)
SPRINKLE = ((0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (P - 1, P - 1))
STRIPE_VALUES = {"zero": (0, 0), "one": (1, 0), "m1": (P - 1, 0), "m1m1": (P - 1, P - 1)}


class Offsets:
    """Where each draw sits on the tape and each message in the transcript.  bl[i]: bit length of layer i; mdb[i]: maxDadBitLength of layer i (-1: no
    binary gate, no phase 2; mdb[0] unused).  Every slot is (start, used, drawn): `drawn` elements are on the tape, the prover reads the first `used`."""

    def __init__(self, bl, mdb):
        self.bl, self.mdb, self.n_layers = list(bl), list(mdb), len(bl)
        n, mx = self.n_layers, max(bl)
        self.max_bl = mx
        self.r0 = (0, bl[n - 1], bl[n - 1])
        at = bl[n - 1]
        self.ru, self.ar, self.rv, self.sig, self.rl = {}, {}, {}, {}, {}
        for i in range(n - 1, 0, -1):
            self.ru[i] = (at, bl[i - 1], mx); at += mx
            self.ar[i] = (at, 1, 1); at += 1
            k = max(0, mdb[i]) if mdb[i] != -1 else 0
            self.rv[i] = (at, k, k); at += k
            self.sig[i] = (at, n - i + 1, n); at += n
            self.rl[i] = (at, bl[i - 1], mx); at += mx
        self.n = at
        # transcript: Vres | per layer i = n-1 .. 1: phase 1 (3 per round, claim_u), phase 2 if any (3 per round, i claims), Liu (3 per round, vr)
        self.parts = [("Vres", n - 1, 0, 0, 1)]
        t = 1
        for i in range(n - 1, 0, -1):
            self.parts.append(("phase 1", i, t, bl[i - 1], 1)); t += 3 * bl[i - 1] + 1
            if mdb[i] != -1:
                self.parts.append(("phase 2", i, t, mdb[i], i)); t += 3 * mdb[i] + i
            self.parts.append(("Liu", i, t, bl[i - 1], 1)); t += 3 * bl[i - 1] + 1
        self.n_tr = t

    @classmethod
    def of(cls, oc):
        """From a circuit of oracle_binding (its layer bit lengths and subsets())."""
        n = oc.layers
        return cls([oc.layer_bitlen(i) for i in range(n)], [-1] + [oc.subsets(i)[2] for i in range(1, n)])

    def claim_index(self, phase, layer):
        """Transcript element index of the first claim of a sumcheck (claim_u, claims_v[0], vr)."""
        for name, i, start, rounds, _ in self.parts:
            if name == phase and i == layer:
                return start + 3 * rounds
        raise KeyError((phase, layer))

    def locate(self, idx):
        """Transcript element idx in words: layer / phase / round / coefficient or claim."""
        for name, i, start, rounds, claims in self.parts:
            if name == "Vres":
                if idx == 0:
                    return "Vres (output layer %d)" % i
                continue
            if idx < start + 3 * rounds:
                return "layer %d, %s, round %d of %d, coefficient %s" % (i, name, (idx - start) // 3 + 1, rounds, "abc"[(idx - start) % 3])
            if idx < start + 3 * rounds + claims:
                return "layer %d, %s, claim %d of %d" % (i, name, idx - start - 3 * rounds, claims)
        raise IndexError("transcript element out of range")

    def vectors(self):
        """The slots that hold sumcheck challenges: r_0 (the r_liu of the output layer) and every r_u, r_v, r_liu."""
        out = [self.r0]
        for i in range(self.n_layers - 1, 0, -1):
            out += [self.ru[i], self.rv[i], self.rl[i]]
        return out

    def unused(self):
        """Index of every drawn slot the prover never reads."""
        idx = []
        for i in range(self.n_layers - 1, 0, -1):
            for s, used, drawn in (self.ru[i], self.sig[i], self.rl[i]):
                idx += list(range(s + used, s + drawn))
        return np.array(idx, np.int64)


def _rng(off, seed, *key):
    return np.random.default_rng([int(seed), off.n] + [int(k) for k in key])


def _const(off, re, im):
    t = np.zeros((off.n, 2), np.uint64)
    t[:, 0], t[:, 1] = re, im
    return t


def uniform(off, seed):
    import oracle_binding as ob
    return ob.random_seq(SEED, off.n)


def sprinkle(off, seed):
    """Uniform, each element replaced with probability 1/4 by one of SPRINKLE."""
    t, rng = uniform(off, seed), _rng(off, seed, 1)
    hit = rng.random(off.n) < 0.25
    t[hit] = np.array(SPRINKLE, np.uint64)[rng.integers(0, len(SPRINKLE), int(hit.sum()))]
    return t


def _stripes(k, val):
    def f(off, seed):
        t = uniform(off, seed)
        for s, _, drawn in off.vectors():
            t[s + k:s + drawn:3] = val
        return t
    return f


def edge_limbs_real(off, seed):
    t = _const(off, 0, 0)
    t[:, 0] = np.array(EDGE_LIMBS, np.uint64)[_rng(off, seed, 2).integers(0, len(EDGE_LIMBS), off.n)]
    return t


def edge_limbs_complex(off, seed):
    return np.array(EDGE_LIMBS, np.uint64)[_rng(off, seed, 3).integers(0, len(EDGE_LIMBS), (off.n, 2))]


def uv_corners(off, seed):
    """r_u and r_v are 0 / 1 patterns, everything else uniform: claim_u and every claims_v[j] is then one witness value (or zero)."""
    t, rng = uniform(off, seed), _rng(off, seed, 4)
    for i in range(off.n_layers - 1, 0, -1):
        for s, _, drawn in (off.ru[i], off.rv[i]):
            t[s:s + drawn, 0] = rng.integers(0, 2, drawn)
            t[s:s + drawn, 1] = 0
    return t


def _mid(off):
    return (off.n_layers + 1) // 2     # a layer with layers above and below it as soon as there are three gate layers


def sig_zero_mid(off, seed):
    """sig all zero at a middle layer: its Liu sumcheck runs on all-zero tables and a zero claim."""
    t = uniform(off, seed)
    s, _, drawn = off.sig[_mid(off)]
    t[s:s + drawn] = 0
    return t


def sig_first_only(off, seed):
    """Only sig[0] non-zero at the same layer: the later layers' subsets add nothing to the Liu tables."""
    t = uniform(off, seed)
    s, _, drawn = off.sig[_mid(off)]
    t[s + 1:s + drawn] = 0
    return t


def _assert(val):
    def f(off, seed):
        t = uniform(off, seed)
        for i in range(1, off.n_layers):
            t[off.ar[i][0]] = val
        return t
    return f


def dont_care(off, seed):
    """The uniform tape with every drawn slot the prover never reads changed: the transcript is uniform's."""
    t = uniform(off, seed)
    idx = off.unused()
    other = edge_limbs_complex(off, seed + 1)
    same = (other[idx] == t[idx]).all(axis=1)
    t[idx] = other[idx]
    t[idx[same], 0] = (t[idx[same], 0] + np.uint64(1)) % np.uint64(P)
    return t


def zero(off, seed):
    return _const(off, 0, 0)


def one(off, seed):
    return _const(off, 1, 0)


def minus_one(off, seed):
    return _const(off, P - 1, 0)


def minus_one_limbs(off, seed):
    return _const(off, P - 1, P - 1)


def corner_pattern(off, seed):
    """Every challenge 0 or 1."""
    t = _const(off, 0, 0)
    t[:, 0] = _rng(off, seed, 5).integers(0, 2, off.n)
    return t


STRIPES = {"stripes_%d_%s" % (k, name): _stripes(k, val) for k in range(3) for name, val in STRIPE_VALUES.items()}
VALUE = dict({"uniform": uniform, "sprinkle": sprinkle}, **STRIPES, edge_limbs_real=edge_limbs_real, edge_limbs_complex=edge_limbs_complex, uv_corners=uv_corners,
             sig_zero_mid=sig_zero_mid, sig_first_only=sig_first_only, assert_0=_assert((0, 0)), assert_1=_assert((1, 0)), assert_m1=_assert((P - 1, 0)),
             dont_care=dont_care)
DEGENERATE = {f.__name__: f for f in (zero, one, minus_one, minus_one_limbs, corner_pattern)}
FAMILIES = dict(VALUE, **DEGENERATE)
EDGE_FAMILIES = ("sprinkle",) + tuple(STRIPES) + ("edge_limbs_real", "edge_limbs_complex")        # the families of the non-default switches
LIMB_M1_FAMILIES = ("sprinkle", "stripes_0_m1m1", "stripes_1_m1m1", "stripes_2_m1m1", "edge_limbs_complex", "minus_one_limbs")   # limbs of p - 1: all 61 low bits set
MAX_ZERO_SHARE = 0.5

# ---- circuits: name -> (builder of the seven arrays or None for randomize, environment of the session) ------------------------------------------------------
# tests/test_gpu_gkr_tapes.py carries the table of what each is there for; the small ones are also the circuits of the Python prover (test_gkr_tape_host.py)
CIRCUITS = {
    "S": (lambda: cc.make(12, [40, 33, 50, 17]), {}),
    "M": (lambda: cc.make(11, [1500, 2100, 900, 4100, 700]), {}),
    "E_real": (lambda: cc.make(13, [4096, 1024, 3000], values=EDGE_VALUES, real_consts=True), {}),
    "E_complex": (lambda: cc.make(13, [4096, 1024, 3000], values=EDGE_VALUES, real_consts=False), {}),
    "R": (None, {"VP_SF_BIG_LOG": "12"}),
    "K_skewed": (lambda: cc.make_skewed(104, real_consts=True), {"VP_FUSE_MIN_LOG": "14"}),
    "K_custom_c": (lambda: cc.make_skewed(103, [12001, 16383, 9001, 16384, 49153, 16001]), {"VP_FUSE_MIN_LOG": "14"}),
    "tiny": (lambda: cc.make(4, [5, 3, 2, 1]), {}),
    "zero_var": (lambda: cc.make_zero_var(21), {}),
    "unary_mid": (lambda: cc.make_unary_mid(104), {}),
    "edge_small": (lambda: cc.make(14, [64, 40, 64, 23], values=EDGE_VALUES, real_consts=False), {}),
}
GPU_CIRCUITS = ("S", "M", "E_real", "E_complex", "R", "K_skewed", "K_custom_c")
SMALL_CIRCUITS = ("S", "tiny", "zero_var", "unary_mid", "edge_small")
RANDOMIZE = (4, 12, 1)          # layers, log size, seed of R


@functools.lru_cache(maxsize=None)
def arrays(name):
    mk = CIRCUITS[name][0]
    return mk() if mk is not None else None


def env(name):
    return dict(CIRCUITS[name][1])


def build(mod, name):
    """The circuit in `mod` (oracle_binding or the package: both have Circuit.custom and Circuit.randomize)."""
    a = arrays(name)
    return mod.Circuit.custom(*a) if a is not None else mod.Circuit.randomize(RANDOMIZE[0], RANDOMIZE[1], seed=RANDOMIZE[2])


@functools.lru_cache(maxsize=None)
def oracle_circuit(name):
    import oracle_binding as ob
    return build(ob, name)


@functools.lru_cache(maxsize=None)
def offsets(name):
    off = Offsets.of(oracle_circuit(name))
    assert off.n == oracle_circuit(name).gkr_draws()
    return off


@functools.lru_cache(maxsize=None)
def tape(name, family):
    off = offsets(name)
    t = np.ascontiguousarray(FAMILIES[family](off, SEED), np.uint64)
    assert t.shape == (off.n, 2) and int(t.max()) < P
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle(name, family):
    """(transcript bytes, verified) of orc_prove_gkr_tape on the family's tape."""
    tr, st = oracle_circuit(name).prove_gkr_tape(tape(name, family))
    assert len(tr) == 16 * offsets(name).n_tr
    return tr, st["verified"]


def expected(name, family):
    """What the device must return: the oracle's transcript on the same arrays and the same tape (dont_care: on the uniform tape)."""
    return oracle(name, "uniform" if family == "dont_care" else family)[0]


@functools.lru_cache(maxsize=None)
def subset_wires(name, layer):
    """dadId of the layer from its exported gates: for every j < layer the wires of layer j that the layer's binary gates read, by subset slot (lv)."""
    e = oracle_circuit(name).export_layer(layer)
    binary = np.isin(e["ty"], cc.BINARY)
    out = []
    for j in range(layer):
        m = binary & (e["l"] == j)
        wires = np.zeros(int(e["lv"][m].max()) + 1 if m.any() else 0, np.int64)
        wires[e["lv"][m].astype(np.int64)] = e["v"][m].astype(np.int64)
        out.append(wires)
    return out


def corner_claims(name, values):
    """On the uv_corners tape every r_u and r_v coordinate is 0 or 1, so claim_u and claims_v[j] are single witness values: {transcript element index: (re, im)}
    looked up in `values` (values[i][wire] = (re, im) of layer i) without any arithmetic.  claim_u of layer i is the value of the wire of layer i - 1 whose index has
    the bits of r_u (bit 0 with r_u[0]: verifier_sums.eq_table), zero past the end of the layer; claims_v[j] the value of the wire in the subset slot given by the
    first dadBitLength[i][j] bits of r_v, zero past the end of the subset (an empty subset: zero)."""
    off, t = offsets(name), tape(name, "uv_corners")
    idx = lambda bits: sum(int(b) << k for k, b in enumerate(bits))
    at = lambda i, w: (int(values[i][w][0]), int(values[i][w][1]))
    want = {}
    for i in range(off.n_layers - 1, 0, -1):
        s, used, _ = off.ru[i]
        k = idx(t[s:s + used, 0])
        want[off.claim_index("phase 1", i)] = at(i - 1, k) if k < len(values[i - 1]) else (0, 0)
        if off.mdb[i] == -1:
            continue
        wires, dad_bl = subset_wires(name, i), oracle_circuit(name).subsets(i)[1]
        s = off.rv[i][0]
        for j in range(i):
            k = idx(t[s:s + (dad_bl[j] if len(wires[j]) else 0), 0])
            want[off.claim_index("phase 2", i) + j] = at(j, int(wires[j][k])) if k < len(wires[j]) else (0, 0)
    return want


def zero_share(tr):
    w = np.frombuffer(tr, np.uint64).reshape(-1, 2)
    return float((~w.any(axis=1)).mean())


def elements(tr):
    return [(int(a), int(b)) for a, b in np.frombuffer(tr, np.uint64).reshape(-1, 2)]


def first_difference(name, family, got, want):
    """None, or a description of the first transcript element in which two transcripts differ."""
    if got == want:
        return None
    if len(got) != len(want):
        return "%s / %s: lengths %d and %d" % (name, family, len(got), len(want))
    g, w = elements(got), elements(want)
    bad = [i for i in range(len(g)) if g[i] != w[i]]
    i = bad[0]
    return "%s / %s: %d of %d transcript elements differ, the first is %d (%s): %r, expected %r" % (name, family, len(bad), len(g), i, offsets(name).locate(i), g[i], w[i])
