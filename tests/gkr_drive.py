"""The verifier's side of one GKR proof, message by message through the C ABI (include/vpgpu.h: vp_vres, vp_phase1_init, vp_round, vp_finalize,
vp_phase2_init, vp_liu_init) on a caller's tape, assembling the transcript in the golden layout.  The host's prove_interactive draws its challenges from
random() and cannot take a tape; this driver does what host/verifier.cpp's run() does with the prover, and nothing of the verifier's checks.

`ctxs` is one context, or the contexts of all ranks of a round-sharded proof (vp_set_round_shard): every rank is called with the same arguments, the
partial polynomials are summed mod p in Python integers, VP_EXCHANGE is served with vp_shard_exchange_local, and the ranks' claims must agree."""
import ctypes

import numpy as np

P = (1 << 61) - 1
VP_EXCHANGE = 1


def _bind(lib):
    vp_, i = ctypes.c_void_p, ctypes.c_int
    lib.vp_vres.argtypes = [vp_, vp_, i, vp_]
    lib.vp_phase1_init.argtypes = [vp_, i, vp_, vp_]
    lib.vp_phase2_init.argtypes = [vp_, i, vp_]
    lib.vp_liu_init.argtypes = [vp_, i, vp_, vp_, vp_]
    lib.vp_round.argtypes = [vp_] * 3
    lib.vp_finalize.argtypes = [vp_] * 3 + [i]


class Drive:
    def __init__(self, vp, ctxs, off, tape):
        self.lib = vp.lib_gpu()
        _bind(self.lib)
        self.ctxs = list(ctxs) if isinstance(ctxs, (list, tuple)) else [ctxs]
        self.off = off
        self.tape = np.ascontiguousarray(tape, np.uint64)
        self.msgs = []
        self.exchanges = 0          # gathers served
        self.partial_rounds = 0     # rounds in which some rank's polynomial was not the sum

    def _ok(self, rc, what):
        assert rc == 0, "%s: %d (%s)" % (what, rc, self.lib.vp_last_error(self.ctxs[0]))

    def _slot(self, slot, width):
        """The used part of a tape slot in an array of `width` elements (at least one, so that there is a pointer to pass)."""
        s, used, _ = slot
        a = np.zeros((max(width, used, 1), 2), np.uint64)
        a[:used] = self.tape[s:s + used]
        return a

    def _round(self, prev):
        polys = []
        for attempt in range(2):
            polys, rcs = [], []
            for x in self.ctxs:
                poly = np.zeros((3, 2), np.uint64)
                rcs.append(self.lib.vp_round(x, prev.ctypes.data, poly.ctypes.data))
                polys.append(poly)
            if rcs[0] == VP_EXCHANGE and attempt == 0:
                assert all(rc == VP_EXCHANGE for rc in rcs), "the ranks disagree on the gather round: %r" % rcs
                arr = (ctypes.c_void_p * len(self.ctxs))(*[x.value for x in self.ctxs])
                self._ok(self.lib.vp_shard_exchange_local(arr, len(self.ctxs)), "vp_shard_exchange_local")
                self.exchanges += 1
                continue
            assert all(rc == 0 for rc in rcs), "vp_round: %r (%s)" % (rcs, self.lib.vp_last_error(self.ctxs[0]))
            break
        total = np.array([[sum(int(p[q, k]) for p in polys) % P for k in range(2)] for q in range(3)], dtype=np.uint64)
        if not np.array_equal(polys[0], total):
            self.partial_rounds += 1
        self.msgs.append(total.tobytes())

    def _sumcheck(self, challenges, rounds, n_claims):
        prev = np.zeros((1, 2), np.uint64)
        for j in range(rounds):
            self._round(prev)
            prev = challenges[j:j + 1].copy()
        claims = []
        for x in self.ctxs:
            cl = np.zeros((max(n_claims, 1), 2), np.uint64)
            self._ok(self.lib.vp_finalize(x, prev.ctypes.data, cl.ctypes.data, n_claims), "vp_finalize")
            claims.append(cl[:n_claims])
        assert all(np.array_equal(cl, claims[0]) for cl in claims), "the ranks return different claims"
        self.msgs.append(claims[0].tobytes())

    def run(self):
        off, lib = self.off, self.lib
        n, mx = off.n_layers, off.max_bl
        r_liu = self._slot(off.r0, mx)
        out = np.zeros((1, 2), np.uint64)
        for k, x in enumerate(self.ctxs):
            o = np.zeros((1, 2), np.uint64)
            self._ok(lib.vp_vres(x, r_liu.ctypes.data, off.bl[n - 1], o.ctypes.data), "vp_vres")
            if k == 0:
                out = o
        self.msgs.append(out.tobytes())
        rv = {}
        for i in range(n - 1, 0, -1):
            ru, ar, sig, rl = self._slot(off.ru[i], mx), self._slot(off.ar[i], 1), self._slot(off.sig[i], n), self._slot(off.rl[i], mx)
            rv[i] = self._slot(off.rv[i], 0)
            for x in self.ctxs:
                self._ok(lib.vp_phase1_init(x, i, r_liu.ctypes.data, ar.ctypes.data), "vp_phase1_init(%d)" % i)
            self._sumcheck(ru, off.bl[i - 1], 1)
            if off.mdb[i] != -1:
                for x in self.ctxs:
                    self._ok(lib.vp_phase2_init(x, i, ru.ctypes.data), "vp_phase2_init(%d)" % i)
                self._sumcheck(rv[i], off.mdb[i], i)
            ptrs = (ctypes.c_void_p * n)(*[rv[k].ctypes.data if (k >= i and off.mdb[k] > 0) else None for k in range(n)])
            for x in self.ctxs:
                self._ok(lib.vp_liu_init(x, i, ru.ctypes.data, ctypes.cast(ptrs, ctypes.c_void_p), sig.ctypes.data), "vp_liu_init(%d)" % i)
            self._sumcheck(rl, off.bl[i - 1], 1)
            r_liu = rl
        return b"".join(self.msgs)


def prove(vp, ctxs, off, tape):
    """The transcript of one interactive proof on `tape`; returns (bytes, Drive) — the Drive carries the gather and partial-round counts."""
    d = Drive(vp, ctxs, off, tape)
    return d.run(), d
