"""NumPy restatement of the Nash-welfare lottery solver and the induced policy, as the
gfx950 kernels (csrc/lottery.hip) state them: Frank-Wolfe towards the vertex of largest
gradient with a golden-section line search, ``a = U p`` carried incrementally between
iterations, sums over the agents taken in index order.  Host fp64; the expected values of
tests/test_lottery_host.py and tests/test_lottery_gpu.py, and the host side of
tools/lottery_bench.py."""
from __future__ import annotations

import math

import numpy as np

GOLDEN = (np.sqrt(5.0) - 1.0) / 2.0
ROUNDS = 80
BRACKET = 1e-9


def _sum_log(x) -> float:
    """sum_i log x_i added left to right (np.sum is pairwise from 8 terms on); plain floats,
    which also keeps the 100k evaluations of a long solve quick."""
    s = 0.0
    for v in x:
        s += math.log(v) if v > 0.0 else -math.inf
    return s


def gradient(U, a):
    """g_j = sum_i U[i, j] / a_i, the agents added in index order."""
    g = np.zeros(U.shape[1])
    for i in range(U.shape[0]):
        g = g + U[i] / a[i]
    return g


def solve(U, max_iters=1000, tol=1e-10):
    """Returns a dict of p, a, F, gap, iters and the per-iteration F increments.  A problem
    with a negative or non-finite entry or an all-zero agent row: iters = -1 and NaN."""
    U = np.asarray(U, dtype=np.float64)
    n, m = U.shape
    nan = float("nan")
    p = np.full(m, 1.0 / m)
    a = U @ p
    if not (np.all(np.isfinite(U)) and np.all(U >= 0) and np.all(a > 0) and np.all(np.isfinite(a))):
        return {"p": np.full(m, nan), "a": np.full(n, nan), "F": nan, "gap": nan, "iters": -1,
                "increments": np.zeros(0)}
    f_prev = _sum_log(a.tolist())
    iters, incs = 0, []
    for it in range(max_iters):
        j = int(np.argmax(gradient(U, a)))
        b = U[:, j]
        al, bl = a.tolist(), b.tolist()

        def f_gamma(gamma):
            return _sum_log([(1.0 - gamma) * x + gamma * y for x, y in zip(al, bl)])

        lo, hi = 0.0, 1.0
        c = hi - GOLDEN * (hi - lo)
        d = lo + GOLDEN * (hi - lo)
        fc, fd = f_gamma(c), f_gamma(d)
        for _ in range(ROUNDS):
            if fc < fd:
                lo, c, fc = c, d, fd
                d = lo + GOLDEN * (hi - lo)
                fd = f_gamma(d)
            else:
                hi, d, fd = d, c, fc
                c = hi - GOLDEN * (hi - lo)
                fc = f_gamma(c)
            if hi - lo < BRACKET:
                break
        gamma = 0.5 * (lo + hi)
        a = (1.0 - gamma) * a + gamma * b
        f_new = _sum_log(a.tolist())
        p = (1.0 - gamma) * p
        p[j] += gamma
        iters = it + 1
        incs.append(f_new - f_prev)
        if f_new - f_prev < tol:
            break
        f_prev = f_new
    a = U @ p
    return {"p": p, "a": a, "F": float(np.sum(np.log(a))),
            "gap": float(gradient(U, a).max() - n), "iters": iters,
            "increments": np.array(incs)}


def policy(p, B, L):
    """Per-level tables [B^t, B] of pi(b | s) = mass(s + b) / mass(s) from fp64 block sums of
    p over the leaves under each prefix; a prefix of mass <= 0 has the uniform 1/B."""
    p = np.asarray(p, dtype=np.float64)
    tables = []
    for t in range(L):
        child = p.reshape(B ** (t + 1), -1).sum(axis=1).reshape(B ** t, B)
        parent = p.reshape(B ** t, -1).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            pi = child / parent[:, None]
        pi[parent <= 0] = 1.0 / B
        tables.append(pi)
    return tables
