"""Schulze rank aggregation, the Habermas Machine's choice among candidate statements
(src/methods/habermas_machine.py:992-1261), on the GPU.

This is the AGGREGATION half of the reference module, as drop-ins: the names, arguments,
return values, ``None`` cases and ``ValueError`` cases are the reference's, NumPy in and NumPy
out.  The three stages run in cs_schulze (ops.schulze), each reference function through the
kernel's own entry stage:

  _schulze_compute_pairwise_defeats           kind "rankings"  (stage 1)
  _schulze_compute_strongest_path_strengths   kind "defeats"   (stage 2)
  _schulze_rank_candidates                    kind "strengths" (stage 3)
  _schulze_aggregate_with_ties                kind "rankings", all stages in one launch
  _aggregate_schulze                          the same launch with the random ballot's tie-break
  aggregate_schulze_batch                     many elections in one launch (not in the reference)

_hm_normalize_ranking, _hm_is_untied_ranking, _hm_untie_ranking_with_ballot and
_schulze_check_rankings are host functions, as in the reference.  Dimension and type errors are
raised on the host before any launch; the kernel's status -1 (a rank outside [0, C - 1], a
nonzero diagonal) becomes the reference's ValueError.  The reference's ``print``s are ``logger``
calls here.

The random ballot is ``np.random.default_rng(seed).permutation(C).astype(np.int32)`` on the
host, exactly as the reference draws it.  The reference draws it only when the ranking is tied;
the generator is fresh per call, so drawing it always gives the same ballot, and untying an
untied ranking is the identity, so the kernel always applies it.

NOT here: the LLM-prompted generator (candidate generation, ranking prompts and their parsing,
critique rounds; about 1,200 lines of text handling in the reference).  No parity test of it is
possible on the fixture models, whose text is noise, so ``habermas_machine`` is not registered
in GENERATOR_MAP.  Best-of-N's ``selection: "schulze"`` (methods/best_of_n.py) is the selection
rule on this build's own candidates.
"""
from __future__ import annotations

import logging
from typing import Dict, Optional

import numpy as np
import torch

from .. import ops

logger = logging.getLogger(__name__)

MAX_CANDIDATES = 128     # cs_schulze: C <= 128
MAX_VOTERS = 65536       # cs_schulze: R <= 65536


# --- host helpers (src/methods/habermas_machine.py:992-1045) ------------------------------
def _hm_normalize_ranking(ranking: np.ndarray) -> np.ndarray:
    """Normalizes ranking so e.g. [0, 2, 5, 5] -> [0, 1, 2, 2]."""
    if ranking.ndim != 1:
        raise ValueError("The input array should be a single ranking so `ndim=1`")
    _, normalized_ranking = np.unique(ranking, return_inverse=True)
    return normalized_ranking


def _hm_is_untied_ranking(ranking: np.ndarray) -> bool:
    """Checks if the ranking is untied."""
    if ranking.ndim != 1:
        raise ValueError("The input array should be a single ranking so `ndim=1`")
    return np.unique(ranking).size == ranking.size


def _hm_untie_ranking_with_ballot(ranking: np.ndarray, ballot: np.ndarray) -> np.ndarray:
    """Unties ranking with extra ballot and renormalizes rankings."""
    if ranking.ndim != 1:
        raise ValueError("The input array should be a single ranking so `ndim=1`")
    if ranking.shape != ballot.shape:
        raise ValueError("The ranking and ballot should have the same shape.")
    untied = _hm_normalize_ranking(ranking) * len(ranking) + _hm_normalize_ranking(ballot)
    return _hm_normalize_ranking(untied)


def _schulze_check_rankings(rankings: np.ndarray):
    """Basic checks for the rankings array format."""
    _check_rankings_format(rankings)
    num_candidates = rankings.shape[1]
    if np.any(rankings < 0) or np.any(rankings >= num_candidates):
        raise ValueError(_bad_rank_message(rankings))


def _check_rankings_format(rankings: np.ndarray) -> None:
    if rankings.ndim != 2:
        raise ValueError(
            f"Rankings should be 2D [num_citizens, num_candidates], got shape {rankings.shape}")
    if not np.issubdtype(rankings.dtype, np.integer):
        raise ValueError(f"Rankings should be integers, got {rankings.dtype}")


def _bad_rank_message(rankings: np.ndarray) -> str:
    num_candidates = rankings.shape[-1]
    invalid_rank = rankings[(rankings < 0) | (rankings >= num_candidates)][0]
    return f"Ranks must be between 0 and {num_candidates - 1}. Found invalid rank: {invalid_rank}"


# --- the launches ---------------------------------------------------------------------------
def _device() -> torch.device:
    return ops.default_device("Schulze aggregation runs on the GPU (cs_schulze); there is no CPU path")


def _check_limits(R: Optional[int], C: int) -> None:
    if not 1 <= C <= MAX_CANDIDATES:
        raise ops.CSError(f"cs_schulze takes 1 to {MAX_CANDIDATES} candidates, got {C}")
    if R is not None and not 1 <= R <= MAX_VOTERS:
        raise ops.CSError(f"cs_schulze takes 1 to {MAX_VOTERS} voters, got {R}")


def _ranks_int32(rankings: np.ndarray) -> np.ndarray:
    """Integer ranks as int32 without wrapping: a rank out of range stays out of range."""
    C = rankings.shape[-1]
    if rankings.dtype == np.uint64:            # no signed type holds all of it
        rankings = np.minimum(rankings, np.uint64(C))
    return np.ascontiguousarray(np.clip(rankings.astype(np.int64), -1, C).astype(np.int32))


def _run(x: np.ndarray, kind: str, ballot: Optional[np.ndarray] = None,
         valid: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """ops.schulze on host arrays with a leading batch dimension; host arrays back."""
    dev = _device()
    res = ops.schulze(torch.as_tensor(x, device=dev), kind=kind,
                      valid=None if valid is None else torch.as_tensor(valid, device=dev),
                      ballot=None if ballot is None else torch.as_tensor(ballot, device=dev))
    return {k: v.cpu().numpy() for k, v in res.items()}


def _square_or_raise(a: np.ndarray, name: str) -> None:
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"{name} should be a square array, got shape {a.shape}")


def _matrix_int32(a: np.ndarray, name: str) -> np.ndarray:
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} should be integers, got {a.dtype}")
    info = np.iinfo(np.int32)
    if a.size and (a.min() < info.min or a.max() > info.max):
        raise ValueError(f"{name} entries must fit int32")
    return np.ascontiguousarray(a.astype(np.int32))


def _schulze_compute_pairwise_defeats(rankings: np.ndarray) -> np.ndarray:
    """d[i, j] = the number of voters who prefer candidate i to candidate j (lower rank is
    better), int32 [num_candidates, num_candidates].  Like the reference's loop it only compares
    ranks, so it accepts any values: rows that are not ranks in [0, C - 1] are replaced by their
    dense ranks, which compare the same."""
    rankings = np.asarray(rankings)
    if rankings.ndim != 2:
        raise ValueError(
            f"Rankings should be 2D [num_citizens, num_candidates], got shape {rankings.shape}")
    R, C = rankings.shape
    if R == 0 or C == 0:
        return np.zeros((C, C), dtype=np.int32)
    _check_limits(R, C)
    in_range = (np.issubdtype(rankings.dtype, np.integer)
                and not (np.any(rankings < 0) or np.any(rankings >= C)))
    if not in_range:
        rankings = np.stack([np.unique(row, return_inverse=True)[1].reshape(-1)
                             for row in rankings])
    return _run(_ranks_int32(rankings)[None], "rankings")["defeats"][0]


def _schulze_compute_strongest_path_strengths(pairwise_defeats: np.ndarray) -> np.ndarray:
    """p[i, j] = the strength of the strongest path from candidate i to candidate j."""
    pairwise_defeats = np.asarray(pairwise_defeats)
    _square_or_raise(pairwise_defeats, "pairwise_defeats")
    d = _matrix_int32(pairwise_defeats, "pairwise_defeats")
    if d.shape[0] == 0:
        return d
    _check_limits(None, d.shape[0])
    res = _run(d[None], "defeats")
    if res["status"][0] == -1:
        raise ValueError("pairwise_defeats should have an all zero diagonal.")
    return res["strengths"][0]


def _schulze_rank_candidates(path_strengths: np.ndarray) -> np.ndarray:
    """The social rank of each candidate from the strongest-path strengths (lower is better,
    ties possible), intp [num_candidates]."""
    path_strengths = np.asarray(path_strengths)
    _square_or_raise(path_strengths, "path_strengths")
    p = _matrix_int32(path_strengths, "path_strengths")
    if p.shape[0] == 0:
        return np.zeros(0, dtype=np.intp)
    _check_limits(None, p.shape[0])
    res = _run(p[None], "strengths")
    if res["status"][0] == -1:
        raise ValueError("path_strengths should have an all zero diagonal.")
    return res["ranking"][0].astype(np.intp)


def _schulze_aggregate_with_ties(rankings: np.ndarray) -> np.ndarray:
    """Aggregates rankings into a single social ranking with potential ties using Schulze."""
    rankings = np.asarray(rankings)
    _check_rankings_format(rankings)
    _check_limits(*rankings.shape)
    res = _run(_ranks_int32(rankings)[None], "rankings")
    if res["status"][0] == -1:
        raise ValueError(_bad_rank_message(rankings))
    return res["ranking"][0].astype(np.intp)


def _aggregate_schulze(agent_rankings: dict, num_candidates: int, seed: Optional[int] = None,
                       tie_breaking_method: str = "random") -> Optional[np.ndarray]:
    """Prepares rankings, calls the Schulze method, and handles tie-breaking.

    agent_rankings maps agent ids to ranking arrays (lower is better) or None where ranking
    failed.  Returns the final social ranking (untied under 'random'), or None where the
    reference returns None: no valid ranking, a shape mismatch, or a ValueError of the checks."""
    valid_rankings_list = [r for r in agent_rankings.values() if r is not None]
    if not valid_rankings_list:
        logger.warning("Schulze Aggregation Warning: No valid agent rankings provided.")
        return None
    try:
        rankings_arr = np.stack(valid_rankings_list, axis=0)
        if rankings_arr.ndim < 2 or rankings_arr.shape[1] != num_candidates:
            logger.error("Schulze Aggregation Error: Ranking shape mismatch. Expected %s "
                         "candidates, found %s.", num_candidates, rankings_arr.shape[1:2])
            return None
    except ValueError as e:
        logger.error("Schulze Aggregation Error: Could not stack rankings. %s", e)
        logger.error("Individual ranking shapes: %s", [np.shape(r) for r in valid_rankings_list])
        return None
    logger.info("Aggregating %d valid rankings using Schulze...", rankings_arr.shape[0])
    try:
        _check_rankings_format(rankings_arr)
        _check_limits(*rankings_arr.shape)
        ballot = np.random.default_rng(seed).permutation(num_candidates).astype(np.int32)
        res = _run(_ranks_int32(rankings_arr)[None], "rankings", ballot=ballot[None])
        if res["status"][0] == -1:
            raise ValueError(_bad_rank_message(rankings_arr))
        tied = res["ranking"][0].astype(np.intp)
        if tie_breaking_method == "ties_allowed" or _hm_is_untied_ranking(tied):
            logger.info("No ties detected or ties allowed. Returning Schulze ranking.")
            return tied
        if tie_breaking_method == "random":
            untied = res["untied"][0].astype(np.intp)
            logger.info("Ties detected. Applied random tie-breaking: tied %s, ballot %s, final %s",
                        tied, ballot, untied)
            return untied
        logger.warning("Unsupported tie_breaking_method '%s'. Returning tied ranking.",
                       tie_breaking_method)
        return tied
    except ValueError as e:
        logger.error("Schulze Aggregation Error: %s", e)
        return None


def aggregate_schulze_batch(rankings: np.ndarray, seeds=None, tie_breaking_method: str = "random",
                            valid: Optional[np.ndarray] = None) -> np.ndarray:
    """Many elections in ONE launch: rankings int [E, R, C]; seeds None, one seed for all, or one
    per election (each election's ballot is default_rng(its seed).permutation(C), as
    _aggregate_schulze draws it); valid bool [E, R] (optional) names the voters that count, the
    single call's non-None rankings.  Returns intp [E, C]: row e is what
    _aggregate_schulze(election e, C, seed, tie_breaking_method) returns; an election for which
    that call returns None (a rank out of range, no voter left) is a row of -1."""
    rankings = np.asarray(rankings)
    if rankings.ndim != 3:
        raise ValueError(f"Rankings should be 3D [elections, num_citizens, num_candidates], "
                         f"got shape {rankings.shape}")
    if not np.issubdtype(rankings.dtype, np.integer):
        raise ValueError(f"Rankings should be integers, got {rankings.dtype}")
    E, R, C = rankings.shape
    if E == 0:
        return np.zeros((0, C), dtype=np.intp)
    _check_limits(R, C)
    if seeds is None or np.ndim(seeds) == 0:
        per = [seeds] * E
    else:
        per = list(seeds)
        if len(per) != E:
            raise ValueError(f"need one seed per election ({E}), got {len(per)}")
    ballots = np.stack([np.random.default_rng(s).permutation(C).astype(np.int32) for s in per])
    if valid is not None:
        valid = np.ascontiguousarray(np.asarray(valid, dtype=bool))
        if valid.shape != (E, R):
            raise ValueError(f"valid should be [elections, num_citizens] = {(E, R)}, "
                             f"got {valid.shape}")
    res = _run(_ranks_int32(rankings), "rankings", ballot=ballots, valid=valid)
    if tie_breaking_method == "random":
        return res["untied"].astype(np.intp)
    if tie_breaking_method != "ties_allowed":
        logger.warning("Unsupported tie_breaking_method '%s'. Returning tied rankings.",
                       tie_breaking_method)
    return res["ranking"].astype(np.intp)
