"""Choosing the scenario issues: the drop-ins of the reference's data/embed_habermas_issues.py and
data/cluster_habermas_issues.py.  Every unique issue is embedded (utils.get_embeddings), the
embeddings are standardised and clustered with k-means, and the issue nearest each centre is the
scenario set.  The scaler, KMeans and the nearest-row search run on the GPU in fp64
(csrc/cluster.hip through ops.standardize / ops.kmeans / ops.nearest_rows) and restate
scikit-learn's decisions: every random number is drawn on the host from numpy's RandomState in
the pattern ``KMeans(random_state=seed)`` consumes it, so the labels are scikit-learn's.

Precision: everything is computed in fp64.  A float32 input is widened, so it is NOT
scikit-learn's float32 path.  Empty-cluster relocation takes the lower index among points at equal
distance, where scikit-learn's argpartition leaves the order unspecified: parity is claimed only
when those distances are distinct.

The Habermas dataset loader is out of scope: what the reference reads from it is passed in as an
``opinions_for_issue`` callable.
"""
from __future__ import annotations

import csv
import json
import logging
import os
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from . import utils

logger = logging.getLogger(__name__)

EMBEDDINGS_JSON = "habermas_issue_embeddings.json"
ISSUES_CSV = "habermas_issues.csv"
CLUSTERS_CSV = "habermas_issue_clusters.csv"
CENTROIDS_CSV = "centroid_issues.csv"
CENTROIDS_TXT = "centroid_issues.txt"
NO_OPINION = "No opinion was provided."


# --- k-means -----------------------------------------------------------------------------------
def predraw(seed, n: int, k: int, n_init: int):
    """Every random number ``KMeans(n_clusters=k, random_state=seed, n_init=n_init).fit`` consumes
    on n samples, in its order: per restart one ``choice(n, p=uniform)`` (the first centre) and
    k - 1 calls of ``uniform(size=2 + int(log k))`` (the candidates' draws).  Lloyd's iteration
    draws nothing.  ``seed`` is an int or a RandomState (which is advanced, as scikit-learn
    advances it).  Returns (first int32 [n_init], u float64 [n_init, k - 1, T])."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    T = ops.kmeans_trials(k)
    first = np.zeros(n_init, dtype=np.int32)
    u = np.zeros((n_init, k - 1, T), dtype=np.float64)
    w = np.ones(n, dtype=np.float64)
    p = w / w.sum()
    for r in range(n_init):
        first[r] = rs.choice(n, p=p)
        for c in range(k - 1):
            u[r, c] = rs.uniform(size=T)
    return first, u


def _device_rows(embeddings, k: Optional[int] = None, n_init: int = 1) -> torch.Tensor:
    """The embeddings as a 2-D device tensor; with k, scikit-learn's checks of the fit first."""
    if isinstance(embeddings, torch.Tensor):
        E = embeddings
    else:
        E = torch.from_numpy(np.ascontiguousarray(np.asarray(embeddings)))
    if E.dim() != 2 or not E.is_floating_point():
        raise ValueError(f"embeddings must be a 2-D floating-point array, got {tuple(E.shape)}")
    if k is not None:
        _check_fit(E.shape[0], k, n_init)
    if E.is_cuda:
        return E
    return E.to(ops.default_device("clustering runs on the GPU; there is no CPU path"))


def _check_fit(n: int, k: int, n_init: int) -> None:
    if k < 1 or n_init < 1:
        raise ValueError("n_clusters and n_init must be >= 1")
    if n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")


def _info(fit, g: int, n_init: int, mean, scale) -> dict:
    sl = slice(g * n_init, (g + 1) * n_init)
    return {"inertia": fit["inertia"][sl].cpu().numpy(), "n_iter": fit["n_iter"][sl].cpu().numpy(),
            "best": int(fit["best"][g]), "indices": fit["indices"][sl].cpu().numpy(),
            "done": fit["done"][sl].cpu().numpy(), "mean": mean.cpu().numpy(),
            "scale": scale.cpu().numpy()}


def cluster_embeddings(embeddings, n_clusters: int = 5, seed=42, *, n_init: int = 10,
                       max_iter: int = 300, tol: float = 1e-4, init=None, poll_every: int = 8,
                       return_info: bool = False):
    """The reference's cluster_embeddings: StandardScaler, then
    ``KMeans(n_clusters, random_state=seed, n_init=10)``.  Returns (labels int32 [n], centers
    float64 [k, d]); the centres live in the STANDARDISED space.  ``seed`` is an int or a
    ``np.random.RandomState``.  ``init`` is an explicit [k, d] array of starting centres in the
    standardised space (one restart, as scikit-learn's ``init=ndarray``).  ``return_info=True``
    adds a dict: inertia and n_iter per restart, the chosen restart, the seeds' row indices, done
    (1 the labels repeated, 2 tolerance or max_iter), the scaler's mean and scale.
    fp64 throughout (a float32 input is widened: not scikit-learn's float32 path)."""
    E = _device_rows(embeddings, n_clusters, n_init)
    n = E.shape[0]
    Z, mean, scale = ops.standardize(E)
    if init is not None:
        C0 = torch.as_tensor(np.asarray(init, dtype=np.float64)).to(Z.device)
        if tuple(C0.shape) != (n_clusters, Z.shape[1]):
            raise ValueError(f"init must be [{n_clusters}, {Z.shape[1]}], got {tuple(C0.shape)}")
        fit = ops.kmeans(Z, n_clusters, init=C0, max_iter=max_iter, tol=tol, poll_every=poll_every)
        n_init = 1
    else:
        first, u = predraw(seed, n, n_clusters, n_init)
        fit = ops.kmeans(Z, n_clusters, first, u, max_iter=max_iter, tol=tol, poll_every=poll_every)
    labels, centers = fit["labels"][0].cpu().numpy(), fit["centers"][0].cpu().numpy()
    if return_info:
        return labels, centers, _info(fit, 0, n_init, mean, scale)
    return labels, centers


def cluster_embeddings_batch(embeddings, n_clusters: int, seeds: Sequence, *, n_init: int = 10,
                             max_iter: int = 300, tol: float = 1e-4, poll_every: int = 8,
                             return_info: bool = False) -> list:
    """cluster_embeddings for every seed of ``seeds`` in one batch: the len(seeds) * n_init
    restarts iterate together and one restart is chosen per seed.  Each entry of the returned list
    is what the single call returns for that seed."""
    E = _device_rows(embeddings, n_clusters, n_init)
    n = E.shape[0]
    seeds = list(seeds)
    if not seeds:
        return []
    Z, mean, scale = ops.standardize(E)
    draws = [predraw(s, n, n_clusters, n_init) for s in seeds]
    first = np.concatenate([f for f, _ in draws])
    u = np.concatenate([x for _, x in draws])
    fit = ops.kmeans(Z, n_clusters, first, u, n_init=n_init, max_iter=max_iter, tol=tol,
                     poll_every=poll_every)
    labels, centers = fit["labels"].cpu().numpy(), fit["centers"].cpu().numpy()
    out = []
    for g in range(len(seeds)):
        row = (labels[g], centers[g])
        out.append(row + (_info(fit, g, n_init, mean, scale),) if return_info else row)
    return out


def find_cluster_centroids(embeddings, issue_info, cluster_labels, cluster_centers, *,
                           space: str = "raw"):
    """The issue nearest each cluster centre (the reference's find_cluster_centroids,
    pairwise_distances_argmin_min).  The reference compares the centres, which live in the
    standardised space, with the RAW embeddings; ``space="raw"`` (the default) reproduces that.
    ``space="standardized"`` standardises the embeddings first, so that both sides live in the
    same space.  Returns one entry of ``issue_info`` per cluster."""
    if space not in ("raw", "standardized"):
        raise ValueError("space must be 'raw' or 'standardized'")
    E = _device_rows(embeddings)
    if space == "standardized":
        E = ops.standardize(E)[0]
    C = torch.as_tensor(np.asarray(cluster_centers, dtype=np.float64)).to(E.device)
    idx, _ = ops.nearest_rows(C, E)
    return [issue_info[int(i)] for i in idx.cpu().tolist()]


# --- files -------------------------------------------------------------------------------------
def _write_table(path: str, rows: List[dict]) -> None:
    """A list of dicts as pandas' DataFrame(rows).to_csv(path, index=False) writes it: the columns
    in order of first appearance, minimal quoting, True / False, an empty field where missing."""
    cols: List[str] = []
    for r in rows:
        for key in r:
            if key not in cols:
                cols.append(key)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f, lineterminator="\n")
        wr.writerow(cols)
        for r in rows:
            wr.writerow(["" if r.get(c) is None else r[c] for c in cols])


def load_issue_embeddings(json_file: str = EMBEDDINGS_JSON) -> list:
    """The list of {"issue", "embedding"} written by embed_issues; [] if it cannot be read."""
    try:
        with open(json_file, "r") as f:
            data = json.load(f)
    except (FileNotFoundError, json.JSONDecodeError) as e:
        logger.error("Error loading embeddings: %s", e)
        return []
    valid = sum(1 for item in data if item.get("embedding") is not None)
    logger.info("Loaded embeddings for %d issues (%d with valid embeddings)", len(data), valid)
    return data


def _opinions(opinions_for_issue: Callable, issue: str):
    """(the distinct opinions that say something, the consensus statement or None)"""
    got = opinions_for_issue(issue)
    consensus = None
    if isinstance(got, tuple):
        got, consensus = got
    seen, out = set(), []
    for op in got:
        if op is None or (isinstance(op, float) and op != op) or op == NO_OPINION or op in seen:
            continue
        seen.add(op)
        out.append(op)
    return out, consensus


def extract_embeddings(issue_data, max_opinions: int = 5, *, opinions_for_issue: Callable):
    """The embeddings of the issues with at most ``max_opinions`` distinct opinions (issues with
    more are left out whole) and their info: (float64 [m, d], [{"issue", "num_opinions"}]).
    ``opinions_for_issue(issue)`` returns the issue's opinions (or (opinions, consensus))."""
    embeddings, issue_info, excluded = [], [], 0
    for item in issue_data:
        if not item.get("embedding"):
            continue
        text = item.get("issue", "")
        ops_, _ = _opinions(opinions_for_issue, text)
        if len(ops_) <= max_opinions:
            embeddings.append(np.asarray(item["embedding"]))
            issue_info.append({"issue": text, "num_opinions": len(ops_)})
        else:
            excluded += 1
    logger.info("Selected %d issues with %d or fewer opinions, excluded %d", len(embeddings),
                max_opinions, excluded)
    return np.array(embeddings), issue_info


def save_cluster_results(issue_info, cluster_labels, centroid_issues, output_file) -> None:
    """The reference's cluster CSV: issue_info's columns, then cluster and is_centroid (True for
    every row whose issue text is a centroid's)."""
    centroid_texts = {c["issue"] for c in centroid_issues}
    rows = []
    for info, lab in zip(issue_info, np.asarray(cluster_labels).tolist()):
        row = dict(info)
        row["cluster"] = int(lab)
        row["is_centroid"] = info["issue"] in centroid_texts
        rows.append(row)
    _write_table(output_file, rows)
    logger.info("Saved clustering results to %s", output_file)
    counts = np.bincount(np.asarray(cluster_labels, dtype=np.int64))
    logger.info("Cluster distribution: %s", {c: int(m) for c, m in enumerate(counts)})
    for i, c in enumerate(centroid_issues):
        logger.info("Cluster %d: (%s opinions) %s...", i, c.get("num_opinions", "unknown"),
                    c["issue"][:100])


def save_centroid_issues_to_file(centroid_issues, output_file: str = CENTROIDS_CSV,
                                 txt_output_file: str = CENTROIDS_TXT, *,
                                 opinions_for_issue: Callable) -> None:
    """The centroid issues as a CSV (cluster, issue) and as the reference's text file: per
    cluster the issue, its opinions and, where the callable returns one, the consensus."""
    _write_table(output_file, [{"cluster": i, "issue": c["issue"]}
                               for i, c in enumerate(centroid_issues)])
    logger.info("Saved %d centroid issues to %s", len(centroid_issues), output_file)
    with open(txt_output_file, "w") as f:
        for i, c in enumerate(centroid_issues):
            opinions, consensus = _opinions(opinions_for_issue, c["issue"])
            f.write(f"CLUSTER {i + 1}\n{'=' * 50}\n\nISSUE:\n{c['issue']}\n\n")
            f.write(f"OPINIONS ({len(opinions)}):\n")
            for j, op in enumerate(opinions, 1):
                f.write(f"{j}. {op}\n\n")
            if consensus is not None:
                f.write(f"CONSENSUS STATEMENT:\n{consensus}\n\n")
            f.write("\n\n")
    logger.info("Saved detailed centroid issues with opinions to %s", txt_output_file)


def save_progress(results, json_output, csv_output) -> None:
    with open(json_output, "w") as f:
        json.dump(results, f)
    _write_table(csv_output, [{"issue": r["issue"], "has_embedding": r["embedding"] is not None}
                              for r in results])
    logger.info("Saved embeddings to %s and issue text to %s", json_output, csv_output)


def embed_issues(issues: Sequence[str], model: str = "BAAI/bge-large-en-v1.5",
                 json_output: str = EMBEDDINGS_JSON, csv_output: str = ISSUES_CSV) -> list:
    """The resumable embedding step of the reference's embed_habermas_issues.main: issues already
    in ``json_output`` are kept, all missing ones are embedded in ONE utils.get_embeddings pass,
    and the same JSON ([{"issue", "embedding"}]) and CSV (issue, has_embedding) are written."""
    try:
        with open(json_output, "r") as f:
            results = json.load(f)
    except (FileNotFoundError, json.JSONDecodeError):
        results = []
    have = {r["issue"] for r in results}
    todo = []
    for issue in issues:
        if issue not in have:
            have.add(issue)
            todo.append(issue)
    if not todo:
        logger.info("All %d issues already embedded", len(results))
        return results
    embs = utils.get_embeddings(todo, model=model)
    for issue, e in zip(todo, embs):
        results.append({"issue": issue, "embedding": e})
    save_progress(results, json_output, csv_output)
    valid = sum(1 for r in results if r["embedding"] is not None)
    logger.info("Successfully embedded %d/%d issues", valid, len(results))
    return results


def main(n_clusters: int = 5, seed: int = 42, max_opinions: int = 5, *,
         opinions_for_issue: Callable, json_file: str = EMBEDDINGS_JSON, out_dir: str = "."):
    """The reference's clustering pipeline: load the embeddings, keep the issues with at most
    ``max_opinions`` opinions, cluster, and write habermas_issue_clusters.csv,
    centroid_issues.csv and centroid_issues.txt into ``out_dir``.  Returns the centroid issues
    (None where the reference returns early)."""
    issue_data = load_issue_embeddings(json_file)
    if not issue_data:
        logger.error("No embeddings found. Run embed_issues first.")
        return None
    embeddings, issue_info = extract_embeddings(issue_data, max_opinions=max_opinions,
                                                opinions_for_issue=opinions_for_issue)
    if len(embeddings) < n_clusters:
        n_clusters = max(2, len(embeddings))
        logger.warning("Not enough issue embeddings (%d): reducing to %d clusters",
                       len(embeddings), n_clusters)
    if len(embeddings) == 0:
        logger.error("No issues found with the specified number of opinions.")
        return None
    labels, centers = cluster_embeddings(embeddings, n_clusters=n_clusters, seed=seed)
    centroid_issues = find_cluster_centroids(embeddings, issue_info, labels, centers)
    save_cluster_results(issue_info, labels, centroid_issues, os.path.join(out_dir, CLUSTERS_CSV))
    save_centroid_issues_to_file(centroid_issues, os.path.join(out_dir, CENTROIDS_CSV),
                                 os.path.join(out_dir, CENTROIDS_TXT),
                                 opinions_for_issue=opinions_for_issue)
    return centroid_issues
