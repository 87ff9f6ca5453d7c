"""Generate tests/golden/maximin_golden.npz FROM THE REFERENCE ITSELF: what its
``max_coalition_improvement`` and ``egalitarian_lottery`` (the HiGHS LPs, core.py:171-279)
return on the problems of lottery_golden.npz.

The reference is imported exactly as make_golden.py imports it; nothing of it is copied, only
input / output DATA is written.  ``linprog`` is wrapped in the imported module's namespace
while a call runs, which yields every coalition's own optimum and ``success`` flag without
touching the function: the calls come in the order of its loop (itertools.combinations by
size, core.py:230-232).

The problems are the U_<name> of lottery_golden.npz (nine 6 x 81 and two tiny trees); the
lotteries, in the order of ``lotteries``: the reference's Nash lottery p_<name> of that file,
the utilitarian point mass on argmax_j sum_i U[i, j] (core.py:374-376) and the uniform
lottery.  Per case ``<name>``:
  maxalpha_<name> [3]      the returned max alpha per lottery (it starts from 1.0)
  alpha_<name>    [3][C]   every coalition's res.x[-1] (NaN where success is false)
  success_<name>  [3][C]   res.success
  egal_p_<name>   [m]      egalitarian_lottery(U)
  egal_value_<name>        min_i U_i . egal_p

Usage:  python tests/golden/make_maximin_golden.py --reference <checkout of the reference>
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from make_golden import import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
LOTTERIES = ("nash", "utilitarian", "uniform")


def improvement_recorded(core, U, p):
    """The reference's max alpha, and every coalition's own (alpha, success)."""
    seen = []
    plain = core.linprog

    def recording(*a, **k):
        res = plain(*a, **k)
        seen.append((float(res.x[-1]) if res.success else float("nan"), bool(res.success)))
        return res

    core.linprog = recording
    try:
        top = core.max_coalition_improvement(U, p)
    finally:
        core.linprog = plain
    return top, np.array([s[0] for s in seen]), np.array([s[1] for s in seen])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository")
    args = ap.parse_args()
    core = import_reference(args.reference)

    stored = np.load(os.path.join(HERE, "lottery_golden.npz"))
    names = [str(n) for n in stored["cases"]]
    out = {"cases": np.array(names), "lotteries": np.array(LOTTERIES)}
    for name in names:
        U = stored[f"U_{name}"]
        n, m = U.shape
        p_util = np.zeros(m)
        p_util[int(np.argmax(U.sum(axis=0)))] = 1.0
        tops, alphas, oks = [], [], []
        for p in (stored[f"p_{name}"], p_util, np.ones(m) / m):
            top, alpha, ok = improvement_recorded(core, U, p)
            assert alpha.size == 2 ** n - 1
            assert top == max(1.0, np.nanmax(np.where(ok, alpha, np.nan)))
            tops.append(top)
            alphas.append(alpha)
            oks.append(ok)
        p_eg = core.egalitarian_lottery(U)
        out[f"maxalpha_{name}"] = np.array(tops)
        out[f"alpha_{name}"] = np.stack(alphas)
        out[f"success_{name}"] = np.stack(oks)
        out[f"egal_p_{name}"] = p_eg
        out[f"egal_value_{name}"] = float((U @ p_eg).min())
        print(f"{name}: {n} x {m}, max alpha {tops}, solved {[int(o.sum()) for o in oks]} of "
              f"{alphas[0].size}, egalitarian value {out[f'egal_value_{name}']:.6e}")
    np.savez_compressed(os.path.join(HERE, "maximin_golden.npz"), **out)
    print("wrote maximin_golden.npz")


if __name__ == "__main__":
    main()
