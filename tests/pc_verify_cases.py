"""Inputs shared by tests/test_pc_verifier_loops_host.py and tests/test_gpu_pc_verifier_loops.py: opening points, public vectors and query leaves
of the commitment verifier's two loops.  Points and vectors are (k, 2) uint64 arrays of canonical limbs."""
import numpy as np

P = (1 << 61) - 1
EDGE = (P - 1, 1 << 60, (1 << 31) + 1, (1 << 31) - 1, 0, 1)


def points(n, seed=0):
    """name -> (n, 2) uint64: a uniform point, the 0/1 corners (eq(point, .) is then a unit vector: all-zero, all-one, alternating), edge limbs."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    out = {"uniform": rng.integers(0, P, size=(n, 2), dtype=np.uint64)}
    out["corner 0"] = np.zeros((n, 2), dtype=np.uint64)
    one = np.zeros((n, 2), dtype=np.uint64); one[:, 0] = 1
    out["corner 1"] = one
    alt = np.zeros((n, 2), dtype=np.uint64); alt[::2, 0] = 1
    out["corner 0101"] = alt
    edge = np.array([[EDGE[(2 * i) % 4], EDGE[(2 * i + 1 + i // 4) % 4]] for i in range(n)], dtype=np.uint64)
    out["edge limbs"] = edge
    return out


def general_vector(n, seed=0):
    """A public vector that is no tensor: uniform entries with edge limbs sprinkled in (first, last and every 37th entry)."""
    rng = np.random.default_rng(2000 + 17 * n + seed)
    v = rng.integers(0, P, size=(1 << n, 2), dtype=np.uint64)
    for k, i in enumerate(list(range(0, 1 << n, 37)) + [(1 << n) - 1]):
        v[i] = (EDGE[k % 4], EDGE[(k + 1) % 4])
    return v


def leaves(n, seed=0):
    """The smallest leaf N / 2, the largest M / 2 - 1, one drawn, and a pair whose level chains take the upper half at one level and the lower at another:
    M / 4 + 1 (upper at level 0, lower at level 1) and M / 8 + 3 (lower at level 0, upper at level 1)."""
    N, M = 1 << (n - 6), 1 << (n - 1)
    rng = np.random.default_rng(3000 + n + seed)
    return [N // 2, M // 2 - 1, int(rng.integers(N // 2, M // 2)), M // 4 + 1, M // 8 + 3]


def leaves_33(n, seed=0):
    """33 positions as a protocol run draws them, with two repeats."""
    N, M = 1 << (n - 6), 1 << (n - 1)
    rng = np.random.default_rng(4000 + n + seed)
    lf = [int(x) for x in rng.integers(N // 2, M // 2, size=33)]
    lf[7] = lf[3]
    lf[32] = lf[0]
    return lf
