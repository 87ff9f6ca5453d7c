#!/usr/bin/env python3
"""The clustering step on the reference's workload at the bge-large width: n = 4096 issues,
d = 1024, k = 5, n_init = 10, seed 43 (the seed of data/cluster_habermas_issues.py's __main__),
on seeded unit-norm low-rank "embedding-like" data.

  single    clustering.cluster_embeddings(E, 5, 43): the whole call (host clock around a call that
            ends in device-to-host copies), median of --reps after --warmup calls, and its parts
            from one more call with a device synchronise after each: scaler, seeding, iterations
            (with their polls of `live`), finish
  batch     cluster_embeddings_batch over ten seeds (R = 100 restarts iterating together)
  host      scikit-learn's StandardScaler + KMeans on THIS box's CPU with the thread count the box
            sets (OMP_NUM_THREADS), if scikit-learn is importable here; labelled a host figure.
            Where it is not importable the record says so and the labels are checked against the
            NumPy restatement (tests/kmeans_ref.py) instead.

The work is small (about 0.8 GFLOP per iteration for all ten restarts): the figures include every
launch and every poll.  Writes one JSON line:

  python tools/cluster_bench.py [--out profiles/cluster_bench.jsonl]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
PKG = "generating-fair-consensus-statements-with-social-choice-on-token-level-mdps_amd"
ops = importlib.import_module(PKG + ".ops")
cl = importlib.import_module(PKG + ".clustering")

N, D, K, N_INIT, SEED = 4096, 1024, 5, 10, 43
BATCH_SEEDS = list(range(43, 53))


def embeddings(n=N, d=D):
    rng = np.random.default_rng(20262)
    e = rng.normal(size=(n, 32)) @ rng.normal(size=(32, d)) + 0.5 * rng.normal(size=(n, d))
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cluster_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--d", type=int, default=D)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    E = embeddings(args.n, args.d)
    Et = torch.from_numpy(E).to(dev)
    line = {"bench": "cluster", "device": torch.cuda.get_device_name(dev), "n": args.n, "d": args.d,
            "k": K, "n_init": N_INIT, "seed": SEED, "warmup": args.warmup, "reps": args.reps}

    res = {}

    def single():
        res["out"] = cl.cluster_embeddings(Et, K, SEED, return_info=True)

    med, lo, hi = wall_ms(single, args.warmup, args.reps)
    labels, centers, info = res["out"]
    line["single"] = {"ms": med, "ms_min": lo, "ms_max": hi, "n_iter": info["n_iter"].tolist(),
                      "best": info["best"], "inertia_best": float(info["inertia"][info["best"]])}
    # the parts, each ended by a device synchronise (so their sum exceeds the whole call a little)
    torch.cuda.synchronize()
    t = time.perf_counter()
    Z, _, _ = ops.standardize(Et)
    torch.cuda.synchronize()
    parts = {"scaler_ms": (time.perf_counter() - t) * 1e3}
    first, u = cl.predraw(SEED, args.n, K, N_INIT)
    fit = ops.kmeans(Z, K, first, u, timings=parts)
    line["single"]["parts"] = {k: round(v, 3) for k, v in parts.items()}
    line["single"]["iterations_enqueued"] = fit["iterations"]
    iters = int(sum(info["n_iter"]))
    line["single"]["gflop_distances"] = round(2.0 * args.n * args.d * K * iters / 1e9, 3)

    def batch():
        res["batch"] = cl.cluster_embeddings_batch(Et, K, BATCH_SEEDS, return_info=True)

    med, lo, hi = wall_ms(batch, 1, max(3, args.reps // 2))
    line["batch"] = {"seeds": len(BATCH_SEEDS), "restarts": len(BATCH_SEEDS) * N_INIT, "ms": med,
                     "ms_min": lo, "ms_max": hi, "ms_per_seed": round(med / len(BATCH_SEEDS), 3),
                     "equals_single": bool(np.array_equal(res["batch"][0][0], labels))}

    try:
        from sklearn.cluster import KMeans
        from sklearn.preprocessing import StandardScaler
    except ImportError:
        line["host"] = "scikit-learn is not importable on this box: no host figure"
        import kmeans_ref as kr
        want = kr.fit(kr.standardize(E)[0], K, SEED, N_INIT)
        line["single"]["labels_equal_restatement"] = bool(np.array_equal(want["labels"], labels))
        line["single"]["narrowest_margin"] = want["narrowest"]
    else:
        times = []
        for _ in range(3):
            t = time.perf_counter()
            zs = StandardScaler().fit_transform(E)
            km = KMeans(n_clusters=K, random_state=SEED, n_init=N_INIT).fit(zs)
            times.append((time.perf_counter() - t) * 1e3)
        line["host"] = {"what": "scikit-learn StandardScaler + KMeans on this box's CPU (a HOST figure)",
                        "threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                        "ms": round(statistics.median(times), 1), "n_iter": int(km.n_iter_)}
        line["single"]["labels_equal_sklearn"] = bool(np.array_equal(km.labels_, labels))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
