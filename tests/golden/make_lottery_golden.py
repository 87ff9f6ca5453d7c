"""Generate tests/golden/lottery_golden.npz FROM THE REFERENCE ITSELF: the Nash-welfare
lotteries of its ``FW_nash_welfare`` and one ``induced_policy_rollout`` result.

The reference is imported exactly as make_golden.py imports it (stub modules for its
network-only dependencies); nothing of it is copied, only input / output DATA is written.
Its ``F_val`` is wrapped while a solve runs, which yields the welfare after every iteration
without touching the solver: the first call is F at the uniform lottery, every later one the
F_new of an iteration (core.py:123, 161).

Per case ``<name>``:  U_<name>, p_<name> (the reference's lottery), iters_<name> (iterations
run), inc_<name> (every iteration's F increment).  ``cases`` lists the names; max_iters and
tol are those of the reference's sweep (core.py:369).  A case with an increment inside
(tol / 2, 2 * tol) is refused: a 1-ulp difference could move its stopping iteration.

Usage:  python tests/golden/make_lottery_golden.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from make_golden import import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ITERS, TOL = 1500, 1e-11


def solve_recorded(core, U):
    """The reference's lottery, its iteration count and per-iteration F increments."""
    seen = []
    plain = core.F_val

    def recording(U_, p_):
        f = plain(U_, p_)
        seen.append(f)
        return f

    core.F_val = recording
    try:
        p = core.FW_nash_welfare(U, max_iters=MAX_ITERS, tol=TOL)
    finally:
        core.F_val = plain
    inc = np.diff(np.array(seen))
    return p, len(seen) - 1, inc


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    core = import_reference(args.reference)

    rho_grid = np.linspace(0.6, 5.0, 20)      # core.py:348
    problems = []                             # (name, B, L, d, n, seed, rho)
    for seed in (42, 43, 44):
        for ri in (0, 9, 19):
            problems.append((f"{seed}_{ri}", 3, 4, 8, 6, seed, float(rho_grid[ri])))   # core.py:342-344
    # two tiny trees; at d = 4 the four-leaf problem has an interior optimum (1500 iterations)
    problems.append(("b2l2", 2, 2, 4, 2, 43, 5.0))
    problems.append(("b2l1", 2, 1, 4, 1, 43, 5.0))

    stored = np.load(os.path.join(HERE, "core_golden.npz"))
    out = {"cases": np.array([p[0] for p in problems]), "max_iters": MAX_ITERS, "tol": TOL}
    for name, B, L, d, n, seed, rho in problems:
        v, w = core.generate_params(B, L, d, n, seed=seed)
        U, leaves = core.compute_utilities(v, w, rho)
        if f"U_{name}" in stored.files:
            assert np.array_equal(U, stored[f"U_{name}"]), name
        p, iters, inc = solve_recorded(core, U)
        near = inc[(inc > TOL / 2) & (inc < 2 * TOL)]
        if near.size:
            raise SystemExit(f"case {name}: increments {near} lie within a factor 2 of tol; "
                             "its stopping iteration is not robust to rounding")
        print(f"{name}: {U.shape[0]} x {U.shape[1]}, {iters} iterations, "
              f"last increment {inc[-1] if inc.size else float('nan'):.3e}")
        out[f"U_{name}"] = U
        out[f"p_{name}"] = p
        out[f"iters_{name}"] = iters
        out[f"inc_{name}"] = inc
        if name == "42_9":
            assert np.array_equal(p, stored["p_nw_42_9"])
            p_hat, tv = core.induced_policy_rollout(p, leaves, B, L, num_samples=2000, seed=7)
            out["rollout_case"] = name
            out["rollout_B"], out["rollout_L"] = B, L
            out["rollout_samples"], out["rollout_seed"] = 2000, 7
            out["rollout_p_hat"], out["rollout_tv"] = p_hat, tv
    np.savez_compressed(os.path.join(HERE, "lottery_golden.npz"), **out)
    print("wrote lottery_golden.npz")


if __name__ == "__main__":
    main()
