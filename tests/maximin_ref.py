"""NumPy restatement of the maximin-lottery / coalition-improvement solver as the gfx950 kernel
(csrc/lottery.hip, ``cs_maximin_lottery``) states it: the matrix game
``value(M) = max_q min_{i in S} (M q)_i`` with ``M[i, j] = U[i, j] / base[i]`` solved as
``min 1.x  s.t.  M x >= 1, x >= 0`` by a revised dual simplex from the all-slack basis.

Same pivot choice and tie rule as the kernel, and the same fp64 operations in the same order
(every dot product runs over the coalition's rows in index order, multiply then add), so the
pivot paths are equal and the results agree to the last bits.  Host fp64; the expected values of
tests/test_maximin_host.py and tests/test_maximin_gpu.py.

State per problem, r = |S|: the basis inverse Binv [r, r], the basic values xB [r], the dual
weights w [r] (the slack columns' reduced costs) and which column is basic in each row.
A pivot:
  1. leaving row k: the most negative xB, lowest row on ties; none negative: optimal;
  2. pivot row over the nonbasic columns: a_j = -sum_l Binv[k, l] M[l, j] for a lottery column,
     Binv[k, l] for slack l; reduced cost d_j = max(1 - sum_l w[l] M[l, j], 0), w[l] for a slack;
     entering column e = argmin d_j / -a_j over a_j < 0, lowest index on ties (the m lottery
     columns first, then the slacks);
  3. t = Binv A_e; row k of Binv is divided by t[k], the other rows, xB and w are eliminated.
At the end x is read off the basis: q = x / sum x, value = 1 / sum x, lam = w / sum w."""
from __future__ import annotations

import itertools

import numpy as np

MAX_PIVOTS = 4096          # CS_MAXIMIN_MAX_PIVOTS


def coalition_masks(n):
    """All 2^n - 1 nonempty coalitions as bit masks, in the reference's order
    (itertools.combinations by size, core.py:230-232)."""
    out = []
    for r in range(1, n + 1):
        for S in itertools.combinations(range(n), r):
            out.append(sum(1 << i for i in S))
    return np.array(out, dtype=np.uint64)


def members(mask, A):
    return [i for i in range(A) if (int(mask) >> i) & 1]


def _failed(A, m, status):
    nan = float("nan")
    return {"alpha": nan, "value": nan, "q": np.full(m, nan), "lam": np.full(A, nan),
            "pivots": status}


def solve(U, base=None, mask=None, max_pivots=MAX_PIVOTS):
    """One (problem, coalition): {"alpha", "value", "q" [m], "lam" [A], "pivots"}.
    pivots = -1 (and NaN) for a negative or non-finite utility anywhere in U, a member whose
    base is not finite and positive, or a member whose row of M is not finite or all zero;
    -2 (and NaN) when max_pivots is exhausted or the pivot row has no negative entry."""
    U = np.asarray(U, dtype=np.float64)
    A, m = U.shape
    S = members((1 << A) - 1 if mask is None else mask, A)
    r = len(S)
    b = np.ones(A) if base is None else np.asarray(base, dtype=np.float64)
    if not (np.all(np.isfinite(U)) and np.all(U >= 0)):
        return _failed(A, m, -1)
    if not np.all(np.isfinite(b[S]) & (b[S] > 0)):
        return _failed(A, m, -1)
    with np.errstate(over="ignore"):
        M = U[S] / b[S, None]
    if not (np.all(np.isfinite(M)) and np.all(M.max(axis=1) > 0)):
        return _failed(A, m, -1)
    if m == 1:          # one lottery: no pivots; the weight on the lowest row of the minimum
        kmin = int(np.argmin(M[:, 0]))
        lam = np.zeros(A)
        lam[S[kmin]] = 1.0
        value = float(M[kmin, 0])
        return {"alpha": (float(r) / float(A)) * value, "value": value, "q": np.ones(1),
                "lam": lam, "pivots": 0}

    Binv = np.eye(r)
    xB = np.full(r, -1.0)
    w = np.zeros(r)
    basis = np.arange(m, m + r)                 # the slack of every row
    basic = np.zeros(m + r, dtype=bool)
    basic[m:] = True
    pivots = 0
    while True:
        k = int(np.argmin(xB))                  # first minimum: the lowest row on ties
        if not xB[k] < 0.0:
            break
        if pivots >= max_pivots:
            return _failed(A, m, -2)
        rho = Binv[k].copy()
        acc_a = np.zeros(m)
        acc_d = np.zeros(m)
        for l in range(r):
            acc_a = acc_a + rho[l] * M[l]
            acc_d = acc_d + w[l] * M[l]
        a = np.concatenate([-acc_a, rho])
        d = np.concatenate([np.maximum(1.0 - acc_d, 0.0), w])
        ok = (a < 0.0) & ~basic
        if not ok.any():
            return _failed(A, m, -2)
        ratio = np.full(m + r, np.inf)
        ratio[ok] = d[ok] / -a[ok]
        e = int(np.argmin(ratio))               # first minimum: the lowest column on ties
        if not ok[e]:                           # every candidate's ratio is inf
            e = int(np.flatnonzero(ok)[0])
        col = -M[:, e] if e < m else np.eye(r)[:, e - m]
        t = np.zeros(r)
        for l in range(r):
            t = t + Binv[:, l] * col[l]
        piv = t[k]
        row = Binv[k] / piv
        theta = xB[k] / piv
        for i in range(r):
            if i != k:
                Binv[i] = Binv[i] - t[i] * row
                xB[i] = xB[i] - t[i] * theta
        Binv[k] = row
        xB[k] = theta
        w = np.maximum(w - d[e] * row, 0.0)
        basic[basis[k]] = False
        basic[e] = True
        basis[k] = e
        pivots += 1

    sx = 0.0
    for i in range(r):
        if basis[i] < m:
            sx = sx + xB[i]
    sw = 0.0
    for i in range(r):
        sw = sw + w[i]
    value = 1.0 / sx
    q = np.zeros(m)
    for i in range(r):
        if basis[i] < m:
            q[basis[i]] = xB[i] / sx
    lam = np.zeros(A)
    lam[S] = w / sw
    return {"alpha": (float(r) / float(A)) * value, "value": value, "q": q, "lam": lam,
            "pivots": pivots}


def certificate(U, q, lam, mask=None, base=None):
    """(lower, upper) = (min_{i in S} (M q)_i, max_j (lam M)_j): lower <= value(M) <= upper for
    any lottery q and any weights lam on S that sum to 1 (weak duality)."""
    U = np.asarray(U, dtype=np.float64)
    A = U.shape[0]
    S = members((1 << A) - 1 if mask is None else mask, A)
    b = np.ones(A) if base is None else np.asarray(base, dtype=np.float64)
    M = U[S] / b[S, None]
    return float((M @ np.asarray(q)).min()), float((np.asarray(lam)[S] @ M).max())
