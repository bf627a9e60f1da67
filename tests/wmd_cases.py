"""Cases and the oracle shared by tests/test_wmd.py and tests/test_wmd_gpu.py.

The oracle is ``scipy.optimize.linear_sum_assignment`` on the cost matrix with every row
repeated m/g times and every column n/g times (g = gcd(n, m)): the transport problem in unit
masses, solved combinatorially, its cost divided by L = n m / g.  The bound on |value - oracle|
is the worst-case rounding of the two sums, (L + n m + 4) 2^-52 max c: the oracle adds L costs,
the solver n m products, each to half an ulp of a partial sum <= L max c.
"""
import functools
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = 2.0 ** -52
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (7, 7), (12, 9), (64, 64), (65, 13), (13, 65), (72, 64),
          (66, 64), (129, 43), (130, 130), (512, 512), (512, 256)]
CPU_SHAPES = [s for s in SHAPES if max(s) <= 130]
DIM = 20


def oracle(c):
    n, m = c.shape
    g = math.gcd(n, m)
    big = np.repeat(np.repeat(c, m // g, axis=0), n // g, axis=1)
    r, k = linear_sum_assignment(big)
    return float(big[r, k].sum() / big.shape[0])


def bound(c):
    n, m = c.shape
    return (n * m // math.gcd(n, m) + n * m + 4) * EPS * float(c.max())


@functools.lru_cache(maxsize=None)
def vectors(n, m):
    """Unit vectors of the n + m words of a case; half of min(n, m) words are shared (the
    second list's first words are the first list's), so exact-zero costs occur."""
    rng = np.random.default_rng(1000 * n + m)
    va, vb = rng.standard_normal((n, DIM)), rng.standard_normal((m, DIM))
    va /= np.linalg.norm(va, axis=1, keepdims=True)
    vb /= np.linalg.norm(vb, axis=1, keepdims=True)
    vb[:min(n, m) // 2] = va[:min(n, m) // 2]
    va.setflags(write=False)
    vb.setflags(write=False)
    return va, vb


@functools.lru_cache(maxsize=None)
def integer_cases():
    """200 cost matrices with n, m <= 8 and entries in 0..3 (ties everywhere), and the exact
    optimum of each as the integer cost of the expanded assignment."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(200):
        n, m = (int(v) for v in rng.integers(1, 9, 2))
        c = rng.integers(0, 4, (n, m)).astype(np.float64)
        g = math.gcd(n, m)
        big = np.repeat(np.repeat(c, m // g, axis=0), n // g, axis=1)
        r, k = linear_sum_assignment(big)
        c.setflags(write=False)
        out.append((c, int(big[r, k].sum()), n * m // g))
    return out


def stacked(costs):
    """Cost matrices on the diagonal of one ground-distance matrix: (D, row lists, column lists)
    with problem (k, k) the k-th matrix."""
    R, Cc = sum(c.shape[0] for c in costs), sum(c.shape[1] for c in costs)
    D = np.zeros((R, Cc))
    la, lb, r0, c0 = [], [], 0, 0
    for c in costs:
        n, m = c.shape
        D[r0:r0 + n, c0:c0 + m] = c
        la.append(list(range(r0, r0 + n)))
        lb.append(list(range(c0, c0 + m)))
        r0, c0 = r0 + n, c0 + m
    return D, la, lb
