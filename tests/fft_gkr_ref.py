"""fft_gkr (lib/virgo's fft_circuit_gkr::fft_gkr, fft_circuit_GKR.cpp:22-849), prover side, in plain Python integers: the reference vp_fft_gkr and the
oracle's orc_fft_gkr_tape are compared with off the seeded tapes, for lg <= 6.  F_p^2 is a pair (re, im) of Python ints, p = 2^61 - 1, i^2 = -1; no numpy
arithmetic, no ctypes.  Written from the protocol, not from either C++ reading of it:

  circuit   r[lg] -> E (eq expansion, by its product) -> lg butterfly layers of the inverse FFT (gate lists) -> S = B / N -> the 64 * N products
            S[j] * x_i^j -> the 64 sums O[i].
  GKR       every layer is a list of gates; the claim on a layer is  sum_g w(g) * gate_g(inputs),  w = alpha * eq(r_0, .) + beta * eq(r_1, .).  The tables of
            a sumcheck are that sum regrouped by the variable summed over:  M[u] = what multiplies V[u], A[u] = what does not depend on V[u] — one pass over
            the gate list each, no closed forms.  A sumcheck folds the pairs (2i, 2i + 1): round polynomial q(t) = sum_i M_i(t) V_i(t) + A_i(t) as (a, b, c) of
            a t^2 + b t + c.

Messages (the layout of vp_fft_gkr and of tests/golden/fftgkr_*.bin): O[64], then per sumcheck the (a, b, c) of every round and the value V is left with —
addition layer (lg + 6 rounds), multiplication layer (lg rounds), per inverse-FFT depth phase 1 and phase 2 (lg rounds each): 84 + 6 lg^2 + 8 lg elements.
Tape (draw order): r[lg] | x[64] | r_0[lg+10] | r_1[lg+10] | r_u[lg+6] r_v[lg+6] | r_u[lg] r_v[lg] | per depth r_u[lg] r_v[lg] alpha beta.

The prover checks itself where the wiring has no say: sum_j S[j] = E[0] and S[0] = (1/N) sum_m E[m] (any inverse DFT, in any output order that keeps index
0), and q(0) + q(1) = the running claim in every round of every sumcheck (the verifier's round check, fft_circuit_GKR.cpp:264-266)."""
P = (1 << 61) - 1
ZERO, ONE = (0, 0), (1, 0)
MAX_LG = 6


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def inv(a):
    """1 / (x + i y) = (x - i y) / (x^2 + y^2)."""
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    assert n, "no inverse of zero"
    return (a[0] * n % P, -a[1] * n % P)


def fsum(xs):
    re = im = 0
    for x in xs:
        re += x[0]
        im += x[1]
    return (re % P, im % P)


def n_tape(lg):
    return 2 * lg * lg + 9 * lg + 96


def n_msgs(lg):
    return 84 + 6 * lg * lg + 8 * lg


def eq_at(r, x):
    """eq(r, x) = prod_b (bit b of x ? r[b] : 1 - r[b])."""
    acc = ONE
    for b, rb in enumerate(r):
        acc = mul(acc, rb if (x >> b) & 1 else sub(ONE, rb))
    return acc


def weights(r0, r1, alpha, beta, n):
    """w(g) = alpha * eq(r_0[0..n), g) + beta * eq(r_1[0..n), g) for g < 2^n."""
    return [add(mul(alpha, eq_at(r0[:n], g)), mul(beta, eq_at(r1[:n], g))) for g in range(1 << n)]


def expansion(r):
    """E[g] = prod_i (bit (lg - 1 - i) of g ? 1 - r[i] : r[i])  (csrc/vp_kernels_fftgkr.h, k_fg_expand; fft_circuit_GKR.cpp:24-32)."""
    lg = len(r)
    out = []
    for g in range(1 << lg):
        acc = ONE
        for i in range(lg):
            acc = mul(acc, sub(ONE, r[i]) if (g >> (lg - 1 - i)) & 1 else r[i])
        out.append(acc)
    return out


def butterfly_gates(lg, dep, inv_root):
    """Gates (g, u, v, c) of one butterfly layer, out[g] = pre[u] + c * pre[v]  (csrc/vp_kernels_fftgkr.h, k_fg_butterfly): for k < 2^(lg-dep-1), j < 2^dep
    u = k << (dep + 1) | j, v = u | 2^dep, x = inv_root^(k 2^dep):  out[k << dep | j] = pre[u] + x pre[v],  out[(k + half) << dep | j] = pre[u] - x pre[v]."""
    half, J = 1 << (lg - dep - 1), 1 << dep
    w = inv_root
    for _ in range(dep):
        w = mul(w, w)
    gates, x = [], ONE
    for k in range(half):
        for j in range(J):
            u = k << (dep + 1) | j
            v = u | J
            gates.append((k << dep | j, u, v, x))
            gates.append(((k + half) << dep | j, u, v, sub(ZERO, x)))
        x = mul(x, w)
    return gates


def sumcheck(V, M, A, ch, claim, msgs):
    """sum_i M[i] V[i] + A[i] over len(ch) rounds; appends the round polynomials and V's last value to msgs; returns (that value, the claim left)."""
    V, M, A = list(V), list(M), list(A)
    assert len(V) == len(M) == len(A) == 1 << len(ch)
    for r in ch:
        a = b = c = ZERO
        for i in range(len(V) // 2):
            v0, m0, a0 = V[2 * i], M[2 * i], A[2 * i]
            dv, dm, da = sub(V[2 * i + 1], v0), sub(M[2 * i + 1], m0), sub(A[2 * i + 1], a0)
            a = add(a, mul(dm, dv))                                     # (m0 + t dm)(v0 + t dv) + a0 + t da
            b = add(b, add(add(mul(dm, v0), mul(m0, dv)), da))
            c = add(c, add(mul(m0, v0), a0))
        assert add(add(add(a, b), c), c) == claim, "round check q(0) + q(1) = claim"
        msgs += [a, b, c]
        claim = add(mul(add(mul(a, r), b), r), c)
        V, M, A = ([add(T[2 * i], mul(r, sub(T[2 * i + 1], T[2 * i]))) for i in range(len(T) // 2)] for T in (V, M, A))
    msgs.append(V[0])
    return V[0], claim


def prove(lg, tape, root):
    """The message list of fft_gkr(lg) on `tape` (n_tape(lg) pairs); root = the 2^lg-th root of unity the field library uses (orc_f_root_of_unity(lg))."""
    assert 1 <= lg <= MAX_LG and len(tape) == n_tape(lg)
    tape = [(int(a), int(b)) for a, b in tape]
    assert all(0 <= a < P and 0 <= b < P for a, b in tape)
    pos = [0]

    def take(n):
        pos[0] += n
        return tape[pos[0] - n:pos[0]]

    N = 1 << lg
    w = root
    for _ in range(lg):
        w = mul(w, w)
    assert w == ONE and (lg == 0 or root != ONE), "not a 2^lg-th root of unity"
    inv_root, inv_n = inv(root), inv((N, 0))
    # ---- the circuit
    r = take(lg)
    B = [expansion(r)]
    layer_gates = []
    for dep in range(lg - 1, -1, -1):
        gates = butterfly_gates(lg, dep, inv_root)
        cur = [None] * N
        for g, u, v, c in gates:
            assert cur[g] is None
            cur[g] = add(B[-1][u], mul(c, B[-1][v]))
        layer_gates.append(gates)
        B.append(cur)
    S = [mul(x, inv_n) for x in B[lg]]
    assert fsum(S) == B[0][0], "sum_j S[j] = E[0]"
    assert S[0] == mul(inv_n, fsum(B[0])), "S[0] = (1/N) sum_m E[m]"
    xs = take(64)
    coef = []                                                            # coef[i << lg | j] = x_i^j, 0^0 = 1
    for x in xs:
        p = ONE
        for _ in range(N):
            coef.append(p)
            p = mul(p, x)
    Pm = [mul(S[t & (N - 1)], coef[t]) for t in range(64 * N)]
    O = [fsum(Pm[i << lg:(i + 1) << lg]) for i in range(64)]
    msgs = list(O)
    # ---- the claim on the outputs
    r0, r1 = take(lg + 10), take(lg + 10)
    alpha, beta = ONE, ZERO
    claim = fsum(mul(eq_at(r0[:6], i), O[i]) for i in range(64))
    # ---- addition layer: output i = sum of the products i << lg | j
    wg = weights(r0, r1, alpha, beta, 6)
    M = [ZERO] * (64 * N)
    for i in range(64):
        for j in range(N):
            M[i << lg | j] = add(M[i << lg | j], wg[i])
    ru, rv = take(lg + 6), take(lg + 6)
    vu, _ = sumcheck(Pm, M, [ZERO] * (64 * N), ru, claim, msgs)
    r0[:lg + 6], r1[:lg + 6] = ru, rv
    claim = mul(alpha, vu)
    # ---- multiplication layer: product i << lg | j = S[j] * x_i^j
    wg = weights(r0, r1, alpha, beta, lg + 6)
    M = [ZERO] * N
    for t in range(64 * N):
        M[t & (N - 1)] = add(M[t & (N - 1)], mul(wg[t], coef[t]))
    ru, rv = take(lg), take(lg)
    vu, _ = sumcheck(S, M, [ZERO] * N, ru, claim, msgs)
    r0[:lg], r1[:lg] = ru, rv
    claim = mul(mul(alpha, vu), (N, 0))                                  # S = B[lg] / N
    # ---- the inverse FFT, last butterfly layer first: layer B[lg - d] from pre = B[lg - d - 1], gate g = pre[u] + c pre[v]
    for d in range(lg):
        pre, gates = B[lg - d - 1], layer_gates[lg - d - 1]
        wg = weights(r0, r1, alpha, beta, lg)
        ru, rv = take(lg), take(lg)
        M, A = [ZERO] * N, [ZERO] * N                                    # phase 1, over u: sum_g w(g) (V[u] + c V[v])
        for g, u, v, c in gates:
            M[u] = add(M[u], wg[g])
            A[u] = add(A[u], mul(mul(wg[g], c), pre[v]))
        vu, claim = sumcheck(pre, M, A, ru, claim, msgs)
        M, A = [ZERO] * N, [ZERO] * N                                    # phase 2, over v: sum_g w(g) eq(r_u, u) (v_u + c V[v])
        for g, u, v, c in gates:
            e = mul(wg[g], eq_at(ru, u))
            M[v] = add(M[v], mul(e, c))
            A[v] = add(A[v], mul(e, vu))
        vv, _ = sumcheck(pre, M, A, rv, claim, msgs)
        r0[:lg], r1[:lg] = ru, rv
        alpha, beta = take(2)
        claim = add(mul(alpha, vu), mul(beta, vv))
    assert pos[0] == len(tape) and len(msgs) == n_msgs(lg)
    return msgs


def to_bytes(msgs):
    return b"".join(int(a).to_bytes(8, "little") + int(b).to_bytes(8, "little") for a, b in msgs)
