"""NumPy restatement of the clustering step (scikit-learn's StandardScaler, KMeans with
k-means++ and Lloyd's iteration, pairwise_distances_argmin_min) as csrc/cluster.hip computes it:
the expected values of the GPU tests, itself pinned to scikit-learn and to the reference's
data/cluster_habermas_issues.py by tests/golden/cluster_golden.npz (tests/test_cluster_host.py).

Distances are the plain ((x - c) ** 2).sum(), not the GEMM form scikit-learn uses; every random
number is drawn up front from numpy's RandomState in the pattern scikit-learn consumes it.  Each
run also reports its narrowest decisions, relative, so that a case in which fp64 summation order
could change a decision is refused when the fixtures are made:
  seed_draw   distance of a draw u * pot to the nearest cumulative-sum boundary, over pot
  seed_cand   gap of the best two (different) candidate potentials, over the best
  label       gap of the best two distances of a point, over the second, all iterations
  select      gap of two inertias compared at the selection (different partitions), over the best
"""
from __future__ import annotations

import numpy as np

MAX_K, MAX_D, MAX_N, MAX_R = 64, 4096, 1 << 20, 1024
TILE, CHUNK, SEG = 64, 32, 128            # csrc/cluster.hip: point tile, feature chunk, sum segment
EPS = float(np.finfo(np.float64).eps)


def standardize(X):
    """StandardScaler().fit_transform: (Z, mean, scale), ddof 0, constant features scale 1."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    t = X - mean
    var = ((t ** 2).sum(axis=0) - t.sum(axis=0) ** 2 / n) / n
    constant = var <= n * EPS * var + (n * mean * EPS) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return (X - mean) / scale, mean, scale


def n_trials(k: int) -> int:
    return 2 + int(np.log(k))


def predraw(seed, n: int, k: int, n_init: int):
    """Every random number KMeans(random_state=seed, n_init=n_init).fit consumes, in its order:
    per restart one choice(n, p=uniform) and k - 1 calls of uniform(size=T)."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    T = n_trials(k)
    first = np.zeros(n_init, dtype=np.int32)
    u = np.zeros((n_init, max(k - 1, 0), T), dtype=np.float64)
    w = np.ones(n, dtype=np.float64)
    for r in range(n_init):
        first[r] = rs.choice(n, p=w / w.sum())
        for c in range(k - 1):
            u[r, c] = rs.uniform(size=T)
    return first, u


def _d2(Z, c):
    return ((Z - c) ** 2).sum(axis=1)


def seed_one(Z, k: int, first: int, u):
    """k-means++ of one restart from its draws: (centers [k, d], indices [k], margins)."""
    n = Z.shape[0]
    idx = np.zeros(k, dtype=np.int32)
    idx[0] = first
    closest = _d2(Z, Z[first])
    pot = closest.sum()
    m_draw = m_cand = np.inf
    for c in range(1, k):
        vals = u[c - 1] * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, vals, side="left"), n - 1)
        if pot > 0:
            for v, i in zip(vals, cand):
                below = cum[i - 1] if i > 0 else -np.inf
                m_draw = min(m_draw, (cum[i] - v) / pot if cum[i] >= v else np.inf,
                             (v - below) / pot)
        mins = [np.minimum(closest, _d2(Z, Z[i])) for i in cand]
        pots = np.array([m.sum() for m in mins])
        b = int(np.argmin(pots))
        others = [p for p, i in zip(pots, cand) if i != cand[b] and p != pots[b]]
        if others and pots[b] > 0:
            m_cand = min(m_cand, (min(others) - pots[b]) / pots[b])
        idx[c] = cand[b]
        closest, pot = mins[b], pots[b]
    return Z[idx].copy(), idx, {"seed_draw": m_draw, "seed_cand": m_cand}


def relocate(Z, labels, dist, sums, counts):
    """scikit-learn's _relocate_empty_clusters_dense on the sums; the lower index among equal
    distances (scikit-learn's argpartition leaves that order unspecified)."""
    empty = np.where(counts == 0)[0]
    if len(empty) == 0 or dist.max() == 0:
        return
    order = np.lexsort((np.arange(len(dist)), -dist))[:len(empty)]
    for e, f in zip(empty, order):
        o = labels[f]
        sums[o] -= Z[f]
        sums[e] = Z[f]
        counts[e] = 1
        counts[o] -= 1


def lloyd_step(Z, C):
    """One iteration from the centres C: (labels, new centres, shift, label margin)."""
    k = C.shape[0]
    D = np.stack([_d2(Z, C[c]) for c in range(k)], axis=1)
    labels = D.argmin(axis=1).astype(np.int32)
    dist = D[np.arange(len(Z)), labels]
    margin = np.inf
    if k > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        ok = two[:, 1] > 0
        if ok.any():
            margin = float(((two[ok, 1] - two[ok, 0]) / two[ok, 1]).min())
    sums = np.zeros_like(C)
    np.add.at(sums, labels, Z)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    relocate(Z, labels, dist, sums, counts)
    amax = int(np.argmax(counts))
    new = sums
    for c in range(k):                     # scikit-learn's _average_centers, in its order
        if counts[c] > 0:
            new[c] = new[c] * (1.0 / counts[c])
        else:
            new[c] = new[amax]
    shift = float(sum(np.sqrt(((new[c] - C[c]) ** 2).sum()) ** 2 for c in range(k)))
    return labels, new, shift, margin


def labels_for(Z, C):
    D = np.stack([_d2(Z, C[c]) for c in range(C.shape[0])], axis=1)
    return D.argmin(axis=1).astype(np.int32)


def lloyd(Z, C0, max_iter: int, tol_abs: float):
    """One restart: dict(labels, centers, n_iter, done (1 labels repeated, 2 tolerance or
    max_iter), inertia, label margin)."""
    C = np.array(C0, dtype=np.float64)
    old = np.full(len(Z), -1, dtype=np.int32)
    margin = np.inf
    done = 2
    it = 0
    for it in range(1, max_iter + 1):
        labels, C, shift, m = lloyd_step(Z, C)
        margin = min(margin, m)
        if np.array_equal(labels, old):
            done = 1
            break
        if shift <= tol_abs:
            break
        old = labels
    if done != 1:
        labels = labels_for(Z, C)
    inertia = float(((Z - C[labels]) ** 2).sum(axis=1).sum())
    return {"labels": labels, "centers": C, "n_iter": it, "done": done, "inertia": inertia,
            "label": margin}


def same_clustering(l1, l2, k: int) -> bool:
    """scikit-learn's _is_same_clustering: one mapping of l1's names onto l2's."""
    mapping = np.full(k, -1, dtype=np.int64)
    for a, b in zip(l1, l2):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


def select(runs, k: int):
    """The sequential choice among restarts: (best index, selection margin)."""
    best, margin = 0, np.inf
    for r in range(1, len(runs)):
        a, b = runs[r]["inertia"], runs[best]["inertia"]
        if same_clustering(runs[r]["labels"], runs[best]["labels"], k):
            continue
        if b > 0:
            margin = min(margin, abs(a - b) / b)
        if a < b:
            best = r
    return best, margin


def tolerance(Zs, tol: float) -> float:
    return float(np.mean(np.var(Zs, axis=0)) * tol)


def fit(Zs, k: int, seed=42, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4, init=None):
    """KMeans(k, random_state=seed, n_init=n_init, max_iter=max_iter, tol=tol[, init=init]).fit(Zs)
    on fp64 data: labels, centers (uncentred), inertia [R], n_iter [R], best, indices [R, k],
    done [R] and the narrowest margins."""
    Zs = np.asarray(Zs, dtype=np.float64)
    n = Zs.shape[0]
    if n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
    mean = Zs.mean(axis=0)
    Z = Zs - mean
    tol_abs = tolerance(Zs, tol)
    margins = {"seed_draw": np.inf, "seed_cand": np.inf, "label": np.inf, "select": np.inf}
    runs, indices = [], []
    if init is not None:
        starts = [(np.asarray(init, dtype=np.float64) - mean, np.full(k, -1, dtype=np.int32))]
    else:
        first, u = predraw(seed, n, k, n_init)
        starts = []
        for r in range(n_init):
            C0, idx, m = seed_one(Z, k, int(first[r]), u[r])
            for key, v in m.items():
                margins[key] = min(margins[key], v)
            starts.append((C0, idx))
    for C0, idx in starts:
        run = lloyd(Z, C0, max_iter, tol_abs)
        margins["label"] = min(margins["label"], run["label"])
        runs.append(run)
        indices.append(idx)
    best, margins["select"] = select(runs, k)
    return {"labels": runs[best]["labels"], "centers": runs[best]["centers"] + mean,
            "inertia": np.array([r["inertia"] for r in runs]),
            "n_iter": np.array([r["n_iter"] for r in runs], dtype=np.int32),
            "done": np.array([r["done"] for r in runs], dtype=np.int32),
            "best": best, "indices": np.array(indices, dtype=np.int32), "mean": mean,
            "margins": margins, "narrowest": float(min(margins.values()))}


def nearest_rows(Q, X):
    """(index of the nearest row of X, Euclidean distance) per row of Q; first lowest on ties."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    idx = np.zeros(len(Q), dtype=np.int32)
    dist = np.zeros(len(Q))
    for i, q in enumerate(Q):
        d = _d2(X, q)
        idx[i] = int(np.argmin(d))
        dist[i] = np.sqrt(d[idx[i]])
    return idx, dist


def center_bound(Z) -> float:
    """Summation-order bound on a centre's entry: 8 n 2^-53 max|Z|."""
    return 8.0 * Z.shape[0] * 2.0 ** -53 * float(np.abs(Z).max())


def inertia_bound(Z) -> float:
    """Summation-order bound on the inertia, relative: 4 n d 2^-53."""
    return 4.0 * Z.shape[0] * Z.shape[1] * 2.0 ** -53
