"""ctypes binding of the oracle (oracle/_build/libvp_oracle.so).  TEST INFRASTRUCTURE: imported only by
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_build", "libvp_oracle.so")


class Stats(ctypes.Structure):
    _fields_ = [("prove_sec", ctypes.c_double), ("evaluate_sec", ctypes.c_double), ("verify_sec", ctypes.c_double),
                ("mult_count", ctypes.c_uint64), ("add_count", ctypes.c_uint64), ("rounds", ctypes.c_uint64),
                ("pairs", ctypes.c_uint64), ("proof_kb", ctypes.c_double), ("verified", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        src = [os.path.join(ROOT, "oracle", f) for f in ("vp_oracle.cpp", "vp_oracle.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in src):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"], check=True, stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(LIB)
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.orc_circuit_from_pws.restype = vp
        L.orc_circuit_from_pws.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_long]
        L.orc_circuit_randomize.restype = vp
        L.orc_circuit_randomize.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long]
        L.orc_circuit_custom.restype = vp
        L.orc_circuit_custom.argtypes = [ctypes.c_int] + [vp] * 7
        L.orc_circuit_free.argtypes = [vp]
        L.orc_circuit_layers.argtypes = [vp]
        L.orc_circuit_layer_size.restype = u64
        L.orc_circuit_layer_size.argtypes = [vp, ctypes.c_int]
        L.orc_circuit_layer_bitlen.argtypes = [vp, ctypes.c_int]
        L.orc_circuit_gates.restype = u64
        L.orc_circuit_gates.argtypes = [vp]
        L.orc_circuit_hash.argtypes = [vp, ctypes.POINTER(u64)]
        L.orc_circuit_inputs.argtypes = [vp, vp]
        L.orc_prove_gkr.restype = ctypes.c_int64
        L.orc_prove_gkr.argtypes = [vp, vp, ctypes.c_int64, ctypes.POINTER(Stats)]
        L.orc_gkr_draws.restype = ctypes.c_int64
        L.orc_gkr_draws.argtypes = [vp]
        L.orc_prove_gkr_tape.restype = ctypes.c_int64
        L.orc_prove_gkr_tape.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.POINTER(Stats)]
        L.orc_prove_fs.restype = ctypes.c_int64
        L.orc_prove_fs.argtypes = [vp, vp, ctypes.c_int64, ctypes.POINTER(Stats)]
        for f in ("orc_f_add", "orc_f_sub", "orc_f_mul"):
            getattr(L, f).argtypes = [vp, vp, vp]
        L.orc_f_neg.argtypes = [vp, vp]
        L.orc_f_inv.argtypes = [vp, vp]
        L.orc_f_root_of_unity.argtypes = [ctypes.c_int, vp]
        L.orc_f_random_seq.argtypes = [ctypes.c_uint, ctypes.c_int, vp]
        L.orc_fft_gkr_draws.argtypes = [ctypes.c_int]
        L.orc_fft_gkr.restype = ctypes.c_int64
        L.orc_fft_gkr.argtypes = [ctypes.c_int, ctypes.c_long, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
        L.orc_fft_gkr_tape.restype = ctypes.c_int64
        L.orc_fft_gkr_tape.argtypes = [ctypes.c_int, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]
        L.orc_beta_table.argtypes = [vp, ctypes.c_int, vp, vp]
        L.orc_update_each.argtypes = [vp, vp, vp, u64, u64, vp, vp]
        L.orc_circuit_export_layer.argtypes = [vp, ctypes.c_int] + [vp] * 5
        L.orc_circuit_subsets.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        L.orc_predicates.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp]
        L.orc_liu_gr.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp]
        L.orc_layer_mle.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, vp]
        _lib = L
    return _lib


def fft_gkr_msgs(lg):
    """Message elements of fft_gkr(lg): the 64 outputs, then per sumcheck three per round and the claimed value."""
    return 64 + 3 * (2 * lg * lg + 2 * lg + 6) + 2 + 2 * lg


def random_seq(seed, n):
    """orc_f_random_seq: srand(seed), then n draws of F::random(), as an (n, 2) uint64 array."""
    import numpy as np
    out = np.zeros((n, 2), np.uint64)
    lib().orc_f_random_seq(seed, n, out.ctypes.data)
    return out


def root_of_unity(log_order):
    out = (ctypes.c_uint64 * 2)()
    lib().orc_f_root_of_unity(log_order, out)
    return (int(out[0]), int(out[1]))


def fft_gkr_seeded(lg, seed):
    """orc_fft_gkr: (message bytes, verified)."""
    buf = ctypes.create_string_buffer(16 * fft_gkr_msgs(lg))
    ok = ctypes.c_int(0)
    n = lib().orc_fft_gkr(lg, seed, buf, len(buf), None, ctypes.byref(ok))
    if n != len(buf):
        raise RuntimeError("orc_fft_gkr: %d" % n)
    return buf.raw, ok.value


def fft_gkr_tape_rc(lg, tape, n_tape=None, capacity=None):
    """orc_fft_gkr_tape as it is: (return code, message buffer, verified).  tape: (n, 2) uint64 array in draw order."""
    import numpy as np
    t = np.ascontiguousarray(tape, np.uint64)
    buf = ctypes.create_string_buffer(16 * fft_gkr_msgs(lg))
    ok = ctypes.c_int(0)
    rc = lib().orc_fft_gkr_tape(lg, t.ctypes.data, t.shape[0] if n_tape is None else n_tape, buf, len(buf) if capacity is None else capacity, ctypes.byref(ok))
    return rc, buf.raw, ok.value


def fft_gkr_tape(lg, tape):
    """The oracle's fft_gkr on the caller's tape: (message bytes, verified)."""
    rc, raw, ok = fft_gkr_tape_rc(lg, tape)
    if rc != len(raw):
        raise RuntimeError("orc_fft_gkr_tape: %d" % rc)
    return raw, ok


class Circuit:
    def __init__(self, h):
        if not h:
            raise RuntimeError("oracle circuit construction failed")
        self.h = h

    @classmethod
    def from_pws(cls, path, blocks=1, seed=-1):
        return cls(lib().orc_circuit_from_pws(os.fsencode(path), blocks, seed))

    @classmethod
    def randomize(cls, layers, log_size, seed=-1):
        return cls(lib().orc_circuit_randomize(layers, log_size, seed))

    @classmethod
    def custom(cls, layer_sizes, ty, l, u, v, c_pairs, is_assert):
        import numpy as np
        a = [np.ascontiguousarray(layer_sizes, np.uint64), np.ascontiguousarray(ty, np.int32), np.ascontiguousarray(l, np.int32),
             np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(v, np.uint64), np.ascontiguousarray(c_pairs, np.uint64),
             np.ascontiguousarray(is_assert, np.uint8)]
        return cls(lib().orc_circuit_custom(len(a[0]), *[x.ctypes.data for x in a]))

    @property
    def layers(self):
        return lib().orc_circuit_layers(self.h)

    @property
    def gates(self):
        return lib().orc_circuit_gates(self.h)

    def layer_size(self, i):
        return lib().orc_circuit_layer_size(self.h, i)

    def hash(self):
        out = (ctypes.c_uint64 * 2)()
        lib().orc_circuit_hash(self.h, out)
        return "%016x%016x" % (out[0], out[1])

    def prove_gkr(self, capacity=1 << 20):
        """F::init() + the reference's GKR protocol on the CPU: (transcript bytes, stats dict)."""
        buf = ctypes.create_string_buffer(capacity)
        st = Stats()
        n = lib().orc_prove_gkr(self.h, ctypes.cast(buf, ctypes.c_void_p), capacity, ctypes.byref(st))
        if n < 0:
            raise RuntimeError("oracle prove failed")
        return buf.raw[:n], st.as_dict()

    def gkr_draws(self):
        """Number of challenges orc_prove_gkr's verifier draws: the tape length of vp_prove_gkr."""
        return lib().orc_gkr_draws(self.h)

    def prove_gkr_tape_rc(self, tape, n_tape=None, capacity=1 << 20):
        """orc_prove_gkr_tape as it is: (return code, buffer, stats dict).  tape: (n, 2) uint64 array in draw order."""
        import numpy as np
        t = np.ascontiguousarray(tape, np.uint64)
        buf = ctypes.create_string_buffer(max(capacity, 1))
        st = Stats()
        rc = lib().orc_prove_gkr_tape(self.h, t.ctypes.data, t.shape[0] if n_tape is None else n_tape, ctypes.cast(buf, ctypes.c_void_p),
                                      capacity, ctypes.byref(st))
        return rc, buf.raw, st.as_dict()

    def prove_gkr_tape(self, tape, capacity=1 << 20):
        """The oracle's GKR proof on the caller's tape: (transcript bytes, stats dict)."""
        rc, raw, st = self.prove_gkr_tape_rc(tape, capacity=capacity)
        if rc < 0:
            raise RuntimeError("orc_prove_gkr_tape: %d" % rc)
        return raw[:rc], st

    def prove_fs(self, capacity=1 << 20):
        """The same proof in Fiat-Shamir mode (orc_prove_fs): (proof bytes, stats dict)."""
        buf = ctypes.create_string_buffer(capacity)
        st = Stats()
        n = lib().orc_prove_fs(self.h, ctypes.cast(buf, ctypes.c_void_p), capacity, ctypes.byref(st))
        if n < 0:
            raise RuntimeError("oracle FS prove failed")
        return buf.raw[:n], st.as_dict()

    def layer_bitlen(self, i):
        return lib().orc_circuit_layer_bitlen(self.h, i)

    def export_layer(self, layer):
        """The layer's gate table after subsetInit: dict of numpy arrays ty, l, u, v, lv (lv: the gate's slot in the subset of layer l)."""
        import numpy as np
        n = self.layer_size(layer)
        a = {"ty": np.zeros(n, np.int32), "l": np.zeros(n, np.int32), "u": np.zeros(n, np.uint64), "v": np.zeros(n, np.uint64), "lv": np.zeros(n, np.uint64)}
        lib().orc_circuit_export_layer(self.h, layer, *[a[k].ctypes.data for k in ("ty", "l", "u", "v", "lv")])
        return a

    def subsets(self, layer):
        """(dadSize[j] for j < layer, dadBitLength[j] for j < layer, maxDadBitLength) of the layer."""
        import numpy as np
        ds, db, mx = np.zeros(max(layer, 1), np.int64), np.zeros(max(layer, 1), np.int32), ctypes.c_int32(0)
        if lib().orc_circuit_subsets(self.h, layer, ds.ctypes.data, db.ctypes.data, ctypes.byref(mx)):
            raise RuntimeError("orc_circuit_subsets: bad layer")
        return [int(x) for x in ds[:layer]], [int(x) for x in db[:layer]], mx.value

    # ---- the verifier's loops by value: points are lists of (re, im) pairs of Python ints, results likewise -------------------------------
    @staticmethod
    def _pts(p):
        import numpy as np
        return np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in p], dtype=np.uint64).reshape(-1, 2))

    def predicates(self, layer, r_g, assert_random, r_u, r_v):
        import numpy as np
        g, a, u, v = self._pts(r_g), self._pts([assert_random]), self._pts(r_u), self._pts(r_v)
        out = np.zeros((5 + 7 * layer, 2), np.uint64)
        if lib().orc_predicates(self.h, layer, g.ctypes.data, a.ctypes.data, u.ctypes.data, v.ctypes.data, len(r_v), out.ctypes.data):
            raise RuntimeError("orc_predicates: arguments do not fit the circuit")
        return [(int(x), int(y)) for x, y in out]

    def liu_gr(self, layer, r_u, r_v, sig, r_liu):
        """r_v: dict or list indexed by layer j >= layer (missing / empty where the subset is empty)."""
        import numpy as np
        n = self.layers
        keep = [self._pts(r_v[j]) if (j >= layer and len(r_v[j])) else None for j in range(n)]
        ptrs = (ctypes.c_void_p * n)(*[k.ctypes.data if k is not None else None for k in keep])
        u, s, rl = self._pts(r_u), self._pts(sig), self._pts(r_liu)
        out = np.zeros((1, 2), np.uint64)
        if lib().orc_liu_gr(self.h, layer, u.ctypes.data, ctypes.cast(ptrs, ctypes.c_void_p), s.ctypes.data, rl.ctypes.data, out.ctypes.data):
            raise RuntimeError("orc_liu_gr: arguments do not fit the circuit")
        return (int(out[0, 0]), int(out[0, 1]))

    def layer_mle(self, layer, r):
        import numpy as np
        rr = self._pts(r)
        out = np.zeros((1, 2), np.uint64)
        if lib().orc_layer_mle(self.h, layer, rr.ctypes.data, len(r), out.ctypes.data):
            raise RuntimeError("orc_layer_mle: arguments do not fit the circuit")
        return (int(out[0, 0]), int(out[0, 1]))

    def close(self):
        if self.h:
            lib().orc_circuit_free(self.h)
            self.h = None
