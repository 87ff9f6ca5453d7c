"""Generate tests/golden/schulze_golden.npz FROM THE REFERENCE ITSELF: what the Schulze
functions of its Habermas Machine (src/methods/habermas_machine.py:992-1261) return, and the
known-answer cases of its own test file (src/methods/tests/test_habermas_schulze.py).

The reference's modules are imported with ``together`` and ``dotenv`` stubbed (as
make_method_traces.py does; no model is called: the aggregation is pure NumPy).  Nothing of the
reference is copied, only input / output DATA is written:

  known     the five known-answer cases: k<i>_rankings / _defeats / _strengths / _ranking as the
            test file states them, and k<i>_ref_* as the reference's functions return them
            (stage by stage from the stated inputs, as its test runs them)
  fig1      the two Figure-1 cases: f<i>_rankings, f<i>_ranking (stated), f<i>_ref_ranking
  tiebreak  the six seeded random-tie-break cases: t<i>_rankings, t<i>_seed, t<i>_untied
            (stated), t<i>_ref_untied (what _aggregate_schulze returned)
  random    elections drawn here, rng.integers(0, C, (R, C)) ("ties") and one permutation per
            voter ("perm"), at (R, C) = (1, 1), (2, 2), (4, 5) x 32, (8, 16) x 8, (16, 48),
            (5, 65), (16, 128): r<i>_rankings, r<i>_defeats, r<i>_strengths, r<i>_ranking from
            the reference's three functions, r<i>_ballot (a seeded ballot with repeated values on
            odd cases) and r<i>_untied from _hm_untie_ranking_with_ballot
``known``, ``fig1``, ``tiebreak`` and ``random`` hold the case counts; ``random_kind`` the
generator of each random case.

Usage:  python tests/golden/make_schulze_golden.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1, 1), (2, 2, 1), (4, 5, 32), (8, 16, 8), (16, 48, 1), (5, 65, 1), (16, 128, 1)]
SEED = 20251


def import_reference(ref: str):
    sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
    tog = types.ModuleType("together")
    tog.Together = type("Together", (), {"__init__": lambda self, *a, **k: None})
    sys.modules.setdefault("together", tog)
    dot = types.ModuleType("dotenv")
    dot.load_dotenv = lambda *a, **k: False
    sys.modules.setdefault("dotenv", dot)
    if ref not in sys.path:
        sys.path.insert(0, ref)
    hm = importlib.import_module("src.methods.habermas_machine")
    cases = importlib.import_module("src.methods.tests.test_habermas_schulze")
    return hm, cases


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    hm, cases = import_reference(args.reference)
    out = {}

    known = cases.SCHULZE_TEST_CASES
    out["known"] = len(known)
    for i, k in enumerate(known):
        out[f"k{i}_rankings"] = np.asarray(k.rankings, dtype=np.int32)
        out[f"k{i}_defeats"] = np.asarray(k.pairwise_defeats, dtype=np.int32)
        out[f"k{i}_strengths"] = np.asarray(k.strongest_path_strengths, dtype=np.int32)
        out[f"k{i}_ranking"] = np.asarray(k.social_ranking, dtype=np.int32)
        out[f"k{i}_ref_defeats"] = hm._schulze_compute_pairwise_defeats(k.rankings)
        out[f"k{i}_ref_strengths"] = hm._schulze_compute_strongest_path_strengths(k.pairwise_defeats)
        out[f"k{i}_ref_ranking"] = hm._schulze_rank_candidates(k.strongest_path_strengths)
        out[f"k{i}_ref_aggregate"] = hm._schulze_aggregate_with_ties(k.rankings)

    out["fig1"] = len(cases.figure_1_cases)
    for i, f in enumerate(cases.figure_1_cases):
        out[f"f{i}_rankings"] = np.asarray(f["rankings"], dtype=np.int32)
        out[f"f{i}_ranking"] = np.asarray(f["expected_social_ranking"], dtype=np.int32)
        out[f"f{i}_ref_ranking"] = hm._schulze_aggregate_with_ties(f["rankings"])

    out["tiebreak"] = len(cases.aggregate_random_params)
    for i, t in enumerate(cases.aggregate_random_params):
        out[f"t{i}_rankings"] = np.asarray(t["rankings"], dtype=np.int32)
        out[f"t{i}_seed"] = t["seed"]
        out[f"t{i}_untied"] = np.asarray(t["target_untied_ranking"], dtype=np.int32)
        with contextlib.redirect_stdout(io.StringIO()):
            got = hm._aggregate_schulze({f"agent_{a}": r for a, r in enumerate(t["rankings"])},
                                        t["num_candidates"], seed=t["seed"],
                                        tie_breaking_method="random")
        out[f"t{i}_ref_untied"] = got

    rng = np.random.default_rng(SEED)
    kinds, n = [], 0
    for R, C, count in SHAPES:
        for kind in ("ties", "perm"):
            for _ in range(count):
                if kind == "ties":
                    x = rng.integers(0, C, (R, C)).astype(np.int32)
                else:
                    x = np.stack([rng.permutation(C) for _ in range(R)]).astype(np.int32)
                d = hm._schulze_compute_pairwise_defeats(x)
                p = hm._schulze_compute_strongest_path_strengths(d)
                tied = hm._schulze_rank_candidates(p)
                assert np.array_equal(tied, hm._schulze_aggregate_with_ties(x))
                ballot = rng.permutation(C).astype(np.int32)
                if n % 2:                      # repeated and negative ballot values
                    ballot = (ballot // 2 - 3).astype(np.int32)
                out[f"r{n}_rankings"], out[f"r{n}_defeats"], out[f"r{n}_strengths"] = x, d, p
                out[f"r{n}_ranking"], out[f"r{n}_ballot"] = tied, ballot
                out[f"r{n}_untied"] = hm._hm_untie_ranking_with_ballot(tied, ballot)
                kinds.append(kind)
                n += 1
        print(f"R {R} C {C}: {2 * count} elections")
    out["random"] = n
    out["random_kind"] = np.array(kinds)
    path = os.path.join(HERE, "schulze_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {n} random elections, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
