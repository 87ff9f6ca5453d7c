"""NumPy restatement of Schulze rank aggregation as the Habermas Machine runs it
(src/methods/habermas_machine.py:992-1024, 1048-1160 of the reference): the source of the
expected values of the cs_schulze GPU tests.  tests/test_schulze_host.py pins it to what the
reference's own functions returned (tests/golden/schulze_golden.npz).

Two forms of the three stages:
  loops   the reference's loop order, literally (slow: three nested Python loops per stage)
  fast    one vectorised update per pivot, which keeps row k, column k and the diagonal
Both are exact integer arithmetic, so every comparison against them is with zero tolerance.
Scores mode, ``valid``, the ballot untie, the winner and the statuses follow the contract in
include/consensus_scoring.h."""
from __future__ import annotations

import numpy as np

TILE = 32          # kSchTile of csrc/schulze.hip: the voters staged per pass
NARROW_C = 16      # kSchNarrowC: one wave per workgroup up to this many candidates
MAX_C, MAX_R = 128, 65536


# --- stage 1 ------------------------------------------------------------------------------
def defeats_loops(rankings):
    R, C = rankings.shape
    d = np.zeros((C, C), dtype=np.int32)
    for r in range(R):
        for i in range(C):
            for j in range(C):
                if i == j:
                    continue
                if rankings[r, i] < rankings[r, j]:
                    d[i, j] += 1
    return d


def defeats_fast(rankings):
    x = np.asarray(rankings)
    d = (x[:, :, None] < x[:, None, :]).sum(axis=0).astype(np.int32)
    np.fill_diagonal(d, 0)
    return d


def defeats_scores(scores):
    """Higher is better; a NaN compares false both ways; -0.0 == 0.0."""
    x = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d = (x[:, :, None] > x[:, None, :]).sum(axis=0).astype(np.int32)
    np.fill_diagonal(d, 0)
    return d


# --- stage 2 ------------------------------------------------------------------------------
def _initial_strengths(d):
    p = np.where(d > d.T, d, 0).astype(np.int32)
    np.fill_diagonal(p, 0)
    return p


def strengths_loops(d):
    d = np.asarray(d, dtype=np.int32)
    C = d.shape[0]
    p = _initial_strengths(d)
    for i in range(C):
        for j in range(C):
            if i == j:
                continue
            for k in range(C):
                if i == k or j == k:
                    continue
                p[j, k] = max(p[j, k], min(p[j, i], p[i, k]))
    return p


def strengths_fast(d):
    d = np.asarray(d, dtype=np.int32)
    C = d.shape[0]
    p = _initial_strengths(d)
    off = ~np.eye(C, dtype=bool)
    for k in range(C):
        via = np.minimum(p[:, k][:, None], p[k, :][None, :])
        keep = off.copy()
        keep[k, :] = False
        keep[:, k] = False
        p = np.where(keep, np.maximum(p, via), p)
    return p


# --- stage 3 ------------------------------------------------------------------------------
def ranking_loops(p):
    C = p.shape[0]
    count = [sum(1 for j in range(C) if p[i, j] >= p[j, i]) for i in range(C)]
    distinct = sorted(set(count), reverse=True)
    return np.array([distinct.index(c) for c in count], dtype=np.intp)


def ranking_fast(p):
    p = np.asarray(p)
    count = (p >= p.T).sum(axis=1)
    return np.unique(-count, return_inverse=True)[1].reshape(-1).astype(np.intp)


# --- tie-break and winner -----------------------------------------------------------------
def dense_rank(v):
    """The number of distinct values below each entry (np.unique's inverse, written out)."""
    v = [int(x) for x in v]
    distinct = sorted(set(v))
    return np.array([distinct.index(x) for x in v], dtype=np.intp)


def untie(ranking, ballot):
    C = len(ranking)
    key = dense_rank(ranking) * C + dense_rank(ballot)
    return dense_rank(key)


def winner(ranking):
    return int(np.where(np.asarray(ranking) == 0)[0][0])


# --- the whole election as cs_schulze answers it ------------------------------------------
def solve(x, kind="rankings", valid=None, ballot=None, form="fast"):
    """One election.  Returns {"status", "defeats", "strengths", "ranking", "untied", "winner"};
    "defeats" is None where stage 1 is skipped, "strengths" where stage 2 is, "untied" without a
    ballot.  status -1 / -2: every other entry present is filled with -1."""
    f_def = defeats_fast if form == "fast" else defeats_loops
    f_str = strengths_fast if form == "fast" else strengths_loops
    f_rank = ranking_fast if form == "fast" else ranking_loops
    x = np.asarray(x)
    C = x.shape[-1]
    status, d, p = 0, None, None
    if kind in ("rankings", "scores"):
        rows = x if valid is None else x[np.asarray(valid).astype(bool)]
        if rows.shape[0] == 0:
            status = -2
        elif kind == "rankings":
            if np.any(rows < 0) or np.any(rows >= C):
                status = -1
            else:
                d = f_def(rows)
        else:
            d = defeats_scores(rows)
        if status == 0:
            p = f_str(d)
    elif kind == "defeats":
        if np.any(np.diag(x) != 0):
            status = -1
        else:
            p = f_str(x)
    elif kind == "strengths":
        if np.any(np.diag(x) != 0):
            status = -1
    else:
        raise ValueError(kind)
    has_d, has_p = kind in ("rankings", "scores"), kind != "strengths"
    if status != 0:
        minus = np.full((C, C), -1, dtype=np.int32)
        return {"status": status, "defeats": minus if has_d else None,
                "strengths": minus.copy() if has_p else None,
                "ranking": np.full(C, -1, dtype=np.intp),
                "untied": None if ballot is None else np.full(C, -1, dtype=np.intp), "winner": -1}
    tied = f_rank(p if has_p else x)
    unt = None if ballot is None else untie(tied, ballot)
    return {"status": 0, "defeats": d, "strengths": p if has_p else None, "ranking": tied,
            "untied": unt, "winner": winner(tied if unt is None else unt)}


def dense_ranks_of_scores(scores):
    """Per voter, the dense ranks (0 = best) of finite-or-infinite scores: the ranking whose
    comparisons are the scores' (no NaN)."""
    s = np.asarray(scores)
    return np.stack([dense_rank_float(-row) for row in s]).astype(np.int32)


def dense_rank_float(v):
    distinct = sorted(set(float(x) for x in v))
    return np.array([distinct.index(float(x)) for x in v], dtype=np.intp)


def random_election(rng, R, C, kind="ties"):
    """The golden file's two generators: ranks drawn with ties, or one permutation per voter."""
    if kind == "ties":
        return rng.integers(0, C, (R, C)).astype(np.int32)
    return np.stack([rng.permutation(C) for _ in range(R)]).astype(np.int32)
