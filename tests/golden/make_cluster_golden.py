"""Generate tests/golden/cluster_golden.npz by RUNNING scikit-learn and the reference's
data/cluster_habermas_issues.py (cluster_embeddings, find_cluster_centroids,
save_cluster_results) on small seeded inputs.  Nothing of the reference is copied, only input /
output DATA is written:

  x_<name>            the raw inputs: a 40 x 3, b 300 x 32, c 97 x 33 (c has a constant feature)
  z_<name>, mean_<name>, scale_<name>   StandardScaler().fit_transform and its statistics
  cases               the number of KMeans cases; per case i:
    c<i>_input / _k / _seed / _n_init / _max_iter / _tol    the call (seed -1: init given)
    c<i>_init         the explicit starting centres (planted-empty-cluster cases), else absent
    c<i>_labels / _centers / _inertia / _n_iter             what KMeans(...).fit(z) holds
    c<i>_indices      [n_init][k] the rows k-means++ chose, from scikit-learn's own seeding
                      run on the same RandomState stream (Lloyd's iteration draws nothing)
    c<i>_narrowest    the narrowest decision margin of the case (tests/kmeans_ref.py)
  ref_<name>_labels / _centers / _centroids / _csv          the reference's
                      cluster_embeddings(x, 5, 43), find_cluster_centroids (as row numbers) and
                      the text save_cluster_results wrote

A case whose narrowest margin is below 1e-9 is refused: fp64 summation order can move a sum of
n <= 1e4 terms by about n 2^-53 ~ 1e-12 relative, and inside that the reference alone is
ambiguous.  Such a case moves on to seed + 100 (the seed used is stored); the bound is not lowered.

Usage:  python tests/golden/make_cluster_golden.py [--reference /root/reference]
        python tests/golden/make_cluster_golden.py --parity profiles/cluster_parity.jsonl
            (no scikit-learn needed: the restatement against the stored file, one JSON line per case)
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_ref as kr  # noqa: E402

MIN_MARGIN = 1e-9
SEEDS, KS = (42, 43, 7), (3, 5, 8)


def import_reference(ref: str):
    sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
    loader = types.ModuleType("data.load_habermas_data")
    loader.get_data_for_issue = lambda issue: None
    sys.modules.setdefault("data.load_habermas_data", loader)
    if ref not in sys.path:
        sys.path.insert(0, ref)
    return importlib.import_module("data.cluster_habermas_issues")


def inputs():
    rng = np.random.default_rng(20261)
    a = rng.normal(size=(40, 3))
    centres = rng.normal(size=(5, 32)) * 1.5
    b = centres[rng.integers(0, 5, 300)] + rng.normal(size=(300, 32))
    low = rng.normal(size=(97, 6)) @ rng.normal(size=(6, 33)) + 0.3 * rng.normal(size=(97, 33))
    c = low / np.linalg.norm(low, axis=1, keepdims=True)
    c[:, 11] = 0.125                                      # a constant feature
    return {"a": a, "b": b, "c": c}


def sk_indices(z, k, seed, n_init):
    """The rows scikit-learn's k-means++ picks for each of the n_init restarts of one fit."""
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    zc = z - z.mean(axis=0)
    rs = np.random.RandomState(seed)
    norms = row_norms(zc, squared=True)
    w = np.ones(len(zc), dtype=zc.dtype)
    out = []
    for _ in range(n_init):
        _, idx = _kmeans_plusplus(zc, k, x_squared_norms=norms, sample_weight=w, random_state=rs)
        out.append(idx)
    return np.array(out, dtype=np.int32)


def write_parity(path: str) -> None:
    import json
    g = np.load(os.path.join(HERE, "cluster_golden.npz"))
    with open(path, "w") as f:
        for i in range(int(g["cases"])):
            z = g[f"z_{str(g[f'c{i}_input'])}"]
            init = g[f"c{i}_init"] if f"c{i}_init" in g else None
            mine = kr.fit(z, int(g[f"c{i}_k"]), int(g[f"c{i}_seed"]), int(g[f"c{i}_n_init"]),
                          int(g[f"c{i}_max_iter"]), float(g[f"c{i}_tol"]), init=init)
            b = mine["best"]
            row = {"what": "restatement vs scikit-learn (host)", "case": i,
                   "input": str(g[f"c{i}_input"]), "n": int(z.shape[0]), "d": int(z.shape[1]),
                   "k": int(g[f"c{i}_k"]), "seed": int(g[f"c{i}_seed"]),
                   "labels_equal": bool(np.array_equal(mine["labels"], g[f"c{i}_labels"])),
                   "n_iter_equal": int(mine["n_iter"][b]) == int(g[f"c{i}_n_iter"]),
                   "centers_abs": float(np.abs(mine["centers"] - g[f"c{i}_centers"]).max()),
                   "centers_bound": kr.center_bound(z),
                   "inertia_rel": abs(mine["inertia"][b] - float(g[f"c{i}_inertia"]))
                   / float(g[f"c{i}_inertia"]),
                   "inertia_bound": kr.inertia_bound(z), "narrowest_margin": mine["narrowest"]}
            f.write(json.dumps(row) + "\n")
    print(f"wrote {path}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    if args.parity:
        write_parity(args.parity)
        return
    from sklearn.cluster import KMeans
    from sklearn.preprocessing import StandardScaler
    warnings.filterwarnings("ignore")
    ref = import_reference(args.reference)
    out = {}
    xs = inputs()
    zs = {}
    for name, x in xs.items():
        sc = StandardScaler()
        zs[name] = sc.fit_transform(x)
        out[f"x_{name}"], out[f"z_{name}"] = x, zs[name]
        out[f"mean_{name}"], out[f"scale_{name}"] = sc.mean_, sc.scale_

    cases = []
    for name in xs:
        for seed in SEEDS:
            for k in KS:
                # the reference's own call (k 5, seed 43) keeps its seed; the others move on
                cases.append(dict(input=name, k=k, seed=seed, n_init=10, max_iter=300, tol=1e-4,
                                  free_seed=(k, seed) != (5, 43)))
    cases.append(dict(input="b", k=5, seed=42, n_init=10, max_iter=300, tol=0.5))
    cases.append(dict(input="b", k=5, seed=42, n_init=10, max_iter=2, tol=1e-4))
    # planted far-off starting centres: one and two empty clusters in the first iteration
    for name, k, n_far in (("b", 5, 1), ("b", 5, 2), ("a", 3, 1), ("c", 8, 2)):
        z = zs[name]
        rng = np.random.default_rng(77 + n_far + k)
        init = z[rng.choice(len(z), k, replace=False)].copy()
        for j in range(n_far):
            init[k - 1 - 2 * j] = 50.0 + 7.0 * j + rng.normal(size=z.shape[1])
        cases.append(dict(input=name, k=k, seed=-1, n_init=1, max_iter=300, tol=1e-4, init=init))

    for i, c in enumerate(cases):
        z = zs[c["input"]]
        init = c.get("init")
        mine = kr.fit(z, c["k"], c["seed"], c["n_init"], c["max_iter"], c["tol"], init=init)
        while mine["narrowest"] < MIN_MARGIN and c.get("free_seed"):
            print(f"case {i} {c['input']} k {c['k']} seed {c['seed']}: narrowest margin "
                  f"{mine['narrowest']:.2e} is below {MIN_MARGIN:.0e}, refused: next seed")
            c["seed"] += 100
            mine = kr.fit(z, c["k"], c["seed"], c["n_init"], c["max_iter"], c["tol"])
        if mine["narrowest"] < MIN_MARGIN:
            raise SystemExit(f"case {i} {c}: narrowest margin {mine['narrowest']:.2e} is below "
                             f"{MIN_MARGIN:.0e}: choose another seed")
        km = KMeans(n_clusters=c["k"], n_init=c["n_init"], max_iter=c["max_iter"], tol=c["tol"],
                    **(dict(init=init) if init is not None else dict(random_state=c["seed"])))
        km.fit(z)
        for key in ("input", "k", "seed", "n_init", "max_iter", "tol"):
            out[f"c{i}_{key}"] = c[key]
        if init is not None:
            out[f"c{i}_init"] = init
            first = kr.lloyd_step(z - z.mean(axis=0), init - z.mean(axis=0))[0]
            assert c["k"] - len(set(first.tolist())) >= 1, "the planted centre is not empty"
        else:
            out[f"c{i}_indices"] = sk_indices(z, c["k"], c["seed"], c["n_init"])
        out[f"c{i}_labels"] = km.labels_.astype(np.int32)
        out[f"c{i}_centers"] = km.cluster_centers_
        out[f"c{i}_inertia"] = km.inertia_
        out[f"c{i}_n_iter"] = km.n_iter_
        out[f"c{i}_narrowest"] = mine["narrowest"]
        print(f"case {i}: {c['input']} k {c['k']} seed {c['seed']} n_iter {km.n_iter_} "
              f"narrowest {mine['narrowest']:.1e}")
    out["cases"] = len(cases)

    for name, x in xs.items():
        info = [{"issue": f"issue {j}: {'yes, no' if j % 7 == 0 else 'plain'}",
                 "num_opinions": j % 5 + 1} for j in range(len(x))]
        with contextlib.redirect_stdout(io.StringIO()):
            labels, centers = ref.cluster_embeddings(x, n_clusters=5, seed=43)
            cents = ref.find_cluster_centroids(x, info, labels, centers)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "clusters.csv")
                ref.save_cluster_results(info, labels, cents, path)
                with open(path) as f:
                    text = f.read()
        out[f"ref_{name}_labels"] = labels.astype(np.int32)
        out[f"ref_{name}_centers"] = centers
        out[f"ref_{name}_centroids"] = np.array([info.index(c) for c in cents], dtype=np.int32)
        out[f"ref_{name}_csv"] = text
    path = os.path.join(HERE, "cluster_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
