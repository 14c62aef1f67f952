"""fft_gkr's part of the Fiat-Shamir chain in Python, written from the text in host/vphost.h ("The transcript chain" and "The transcript chain: fft_gkr"):

  derive(lg, state, msgs)   the tape and the closing state from the messages alone, with hashlib: what a verifier does.  Any lg.
  prove(lg, state, root)    a complete non-interactive prover for lg <= 6 in Python integers: the circuit, the tables and the sumchecks of tests/fft_gkr_ref.py
                            (its field helpers, butterfly_gates, expansion and weights by import), every challenge taken from a draw callback at the moment the
                            schedule allows it.  Returns (msgs, tape, state_out).

Why the pair is a reference at any size: if msgs = P(tape) for a prover P that takes its tape up front (vp_fft_gkr, orc_fft_gkr_tape, fft_gkr_ref.prove) and
tape = derive(msgs), then by induction over the schedule — a slot's draw depends only on messages before it, a message only on slots before it — (msgs, tape) is
THE Fiat-Shamir transcript from that state: no second implementation of the interleaving is needed above lg = 6.

A step is state = SHA3-256(m0 | m1 | m2 | m3 | state), four little-endian u64 words and the 32-byte state.  E(x) = {x.re, x.im, 0, 0x4d}; C(c) = {c, 0, 0, 0x43}
and the challenge is (w0 & p, w1 & p) of the new state with a limb equal to p mapped to 0.  A slot's counter is its index in the tape layout."""
import hashlib
import struct

import fft_gkr_ref as ref
from fft_gkr_ref import ONE, ZERO, add, mul, sub

P = ref.P


class Chain:
    def __init__(self, state):
        self.s = bytes(state)
        assert len(self.s) == 32

    def _step(self, a, b, c, d):
        self.s = hashlib.sha3_256(struct.pack("<4Q", a, b, c, d) + self.s).digest()

    def E(self, x):
        self._step(int(x[0]), int(x[1]), 0, 0x4d)

    def C(self, counter):
        self._step(counter, 0, 0, 0x43)
        w = struct.unpack("<4Q", self.s)
        return tuple(0 if (v & P) == P else v & P for v in w[:2])


class Layout:
    """tape slots, in draw order (include/vpgpu.h)"""

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


def chain_steps(lg):
    """E and C steps of one run: every message absorbed once, every slot drawn once"""
    return ref.n_msgs(lg) + ref.n_tape(lg)


def schedule(lg):
    """The chain's steps in order: ("C", slot) draws a tape slot, ("E", i) absorbs message element i."""
    L = Layout(lg)
    pos = [0]

    def draw(slot, n=1):
        return [("C", s) for s in range(slot, slot + n)]

    def absorb(n):
        pos[0] += n
        return [("E", i) for i in range(pos[0] - n, pos[0])]

    def sumcheck(rounds, slot0):
        ops = []
        for k in range(rounds):
            ops += absorb(3) + draw(slot0 + k)
        return ops + absorb(1)

    ops = draw(L.r, lg) + draw(L.x, 64) + absorb(64) + draw(L.r0, lg + 10) + draw(L.r1, lg + 10)
    ops += sumcheck(lg + 6, L.ru_a) + draw(L.rv_a, lg + 6)
    ops += sumcheck(lg, L.ru_m) + draw(L.rv_m, lg)
    for d in range(lg):
        ops += sumcheck(lg, L.ru_d(d)) + sumcheck(lg, L.rv_d(d)) + draw(L.alpha_d(d), 2)
    assert pos[0] == ref.n_msgs(lg) and sorted(s for k, s in ops if k == "C") == list(range(L.n))
    return ops


def derive(lg, state, msgs):
    """msgs: a sequence of n_msgs(lg) pairs.  Returns (tape as a list of pairs, closing state)."""
    msgs = [(int(a), int(b)) for a, b in msgs]
    assert len(msgs) == ref.n_msgs(lg)
    ch = Chain(state)
    tape = [None] * ref.n_tape(lg)
    for kind, i in schedule(lg):
        if kind == "C":
            tape[i] = ch.C(i)
        else:
            ch.E(msgs[i])
    return tape, ch.s


def slots_after(lg, i):
    """the tape slots drawn after message element i is absorbed"""
    ops = schedule(lg)
    at = ops.index(("E", i))
    return [s for k, s in ops[at:] if k == "C"]


def _sumcheck(V, M, A, rounds, claim, msgs, absorb, draw, slot0):
    """fft_gkr_ref.sumcheck with the round's challenge drawn behind its polynomial; returns (v, claim left, the challenges)"""
    V, M, A = list(V), list(M), list(A)
    assert len(V) == len(M) == len(A) == 1 << rounds
    ch = []
    for k in range(rounds):
        a = b = c = ZERO
        for i in range(len(V) // 2):
            v0, m0, a0 = V[2 * i], M[2 * i], A[2 * i]
            dv, dm, da = sub(V[2 * i + 1], v0), sub(M[2 * i + 1], m0), sub(A[2 * i + 1], a0)
            a = add(a, mul(dm, dv))
            b = add(b, add(add(mul(dm, v0), mul(m0, dv)), da))
            c = add(c, add(mul(m0, v0), a0))
        assert add(add(add(a, b), c), c) == claim, "round check q(0) + q(1) = claim"
        for x in (a, b, c):
            msgs.append(x)
            absorb(x)
        r = draw(slot0 + k)
        ch.append(r)
        claim = add(mul(add(mul(a, r), b), r), c)
        V, M, A = ([add(T[2 * i], mul(r, sub(T[2 * i + 1], T[2 * i]))) for i in range(len(T) // 2)] for T in (V, M, A))
    msgs.append(V[0])
    absorb(V[0])
    return V[0], claim, ch


def prove(lg, state, root):
    """The non-interactive prover, lg <= 6.  root = the 2^lg-th root of unity of the field library (orc_f_root_of_unity(lg))."""
    assert 1 <= lg <= ref.MAX_LG
    L, chain = Layout(lg), Chain(state)
    tape = [None] * L.n

    def draw(slot):
        assert tape[slot] is None
        tape[slot] = chain.C(slot)
        return tape[slot]

    def draws(slot, n):
        return [draw(s) for s in range(slot, slot + n)]

    absorb = chain.E
    N = 1 << lg
    inv_root, inv_n = ref.inv(root), ref.inv((N, 0))
    # ---- the circuit
    r = draws(L.r, lg)
    xs = draws(L.x, 64)
    B, layer_gates = [ref.expansion(r)], []
    for dep in range(lg - 1, -1, -1):
        gates = ref.butterfly_gates(lg, dep, inv_root)
        cur = [None] * N
        for g, u, v, c in gates:
            cur[g] = add(B[-1][u], mul(c, B[-1][v]))
        layer_gates.append(gates)
        B.append(cur)
    S = [mul(x, inv_n) for x in B[lg]]
    coef = []
    for x in xs:
        p = ONE
        for _ in range(N):
            coef.append(p)
            p = mul(p, x)
    Pm = [mul(S[t & (N - 1)], coef[t]) for t in range(64 * N)]
    O = [ref.fsum(Pm[i << lg:(i + 1) << lg]) for i in range(64)]
    msgs = list(O)
    for x in O:
        absorb(x)
    r0, r1 = draws(L.r0, lg + 10), draws(L.r1, lg + 10)
    alpha, beta = ONE, ZERO
    claim = ref.fsum(mul(ref.eq_at(r0[:6], i), O[i]) for i in range(64))
    # ---- addition layer
    wg = ref.weights(r0, r1, alpha, beta, 6)
    M = [wg[t >> lg] for t in range(64 * N)]
    vu, _, ru = _sumcheck(Pm, M, [ZERO] * (64 * N), lg + 6, claim, msgs, absorb, draw, L.ru_a)
    rv = draws(L.rv_a, lg + 6)
    r0[:lg + 6], r1[:lg + 6] = ru, rv
    claim = mul(alpha, vu)
    # ---- multiplication layer
    wg = ref.weights(r0, r1, alpha, beta, lg + 6)
    M = [ZERO] * N
    for t in range(64 * N):
        M[t & (N - 1)] = add(M[t & (N - 1)], mul(wg[t], coef[t]))
    vu, _, ru = _sumcheck(S, M, [ZERO] * N, lg, claim, msgs, absorb, draw, L.ru_m)
    rv = draws(L.rv_m, lg)
    r0[:lg], r1[:lg] = ru, rv
    claim = mul(mul(alpha, vu), (N, 0))
    # ---- the inverse FFT, last butterfly layer first
    for d in range(lg):
        pre, gates = B[lg - d - 1], layer_gates[lg - d - 1]
        wg = ref.weights(r0, r1, alpha, beta, lg)
        M, A = [ZERO] * N, [ZERO] * N
        for g, u, v, c in gates:
            M[u] = add(M[u], wg[g])
            A[u] = add(A[u], mul(mul(wg[g], c), pre[v]))
        vu, claim, ru = _sumcheck(pre, M, A, lg, claim, msgs, absorb, draw, L.ru_d(d))
        M, A = [ZERO] * N, [ZERO] * N
        for g, u, v, c in gates:
            e = mul(wg[g], ref.eq_at(ru, u))
            M[v] = add(M[v], mul(e, c))
            A[v] = add(A[v], mul(e, vu))
        vv, _, rv = _sumcheck(pre, M, A, lg, claim, msgs, absorb, draw, L.rv_d(d))
        r0[:lg], r1[:lg] = ru, rv
        alpha, beta = draws(L.alpha_d(d), 2)
        claim = add(mul(alpha, vu), mul(beta, vv))
    assert all(t is not None for t in tape) and len(msgs) == ref.n_msgs(lg)
    return msgs, tape, chain.s


START_STATES = {"zero": bytes(32), "ones": b"\xff" * 32, "random": hashlib.sha3_256(b"fft_gkr_fs start state").digest()}
