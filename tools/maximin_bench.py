#!/usr/bin/env python3
"""cs_maximin_lottery on the shapes of the reference's coalition-blocking experiment.

  sweep   the experiment of core.main as ONE launch: 60 problems (3 seeds x 20 rho, 6 agents x
          81 leaves) x 3 lotteries (Nash, utilitarian point mass, uniform) x 63 coalitions =
          11,340 LPs
  wide    a scaling point: one 16-agent x 81-leaf problem, all 65,535 coalitions

GPU times are HIP events around --inner back-to-back launches (per launch: the median of
--reps such windows after --warmup launches), with and without the q / lambda outputs.  Every
timed result is certified by its own duality gap (from q and lambda, fp64 on the host) before
its time is reported, and the pivot counts are histogrammed.  The comparison is the LP of the
reference's max_coalition_improvement solved one coalition at a time by scipy's HiGHS on this
box's CPU (the same LP, stated here from its formula: maximise alpha s.t. U_i . p' >= alpha *
base_i for i in S, sum p' = |S| / n, p' >= 0), timed over --host-calls calls of 63 LPs, and the NumPy restatement tests/maximin_ref.py over
the same calls.  Without scipy the HiGHS figure is "not measured".  Writes one JSON line:

  python tools/maximin_bench.py [--out profiles/maximin_bench.jsonl]
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
core = importlib.import_module(PKG + ".core")
import maximin_ref  # noqa: E402

MAX_ITERS, TOL = 1500, 1e-11      # the reference's sweep (core.py:369)


def gpu_ms(fn, warmup, reps, inner):
    """ms per launch: `reps` event windows of `inner` back-to-back launches each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / inner)
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def worst_gap(U3, base, masks, res, stride):
    """The largest (upper - lower) / upper over every stride-th LP of a result (host fp64)."""
    U3, base = U3.cpu().numpy(), base.cpu().numpy()
    q, lam = res["q"].cpu().numpy(), res["lam"].cpu().numpy()
    worst, n = 0.0, 0
    for k in range(U3.shape[0]):
        for ci in range(k % stride, masks.size, stride):
            lo, up = maximin_ref.certificate(U3[k], q[k, ci], lam[k, ci], int(masks[ci]), base[k])
            worst = max(worst, (up - lo) / up)
            n += 1
    return worst, n


def run(name, U3, base, masks, args, gap_stride):
    res = ops.maximin_lottery(U3, base, masks)
    piv = res["pivots"].cpu().numpy()
    if piv.min() < 0:
        raise SystemExit(f"{name}: a problem failed (status {piv.min()})")
    gap, checked = worst_gap(U3, base, masks, res, gap_stride)
    rec = {"problems": int(U3.shape[0]), "A": int(U3.shape[1]), "m": int(U3.shape[2]),
           "coalitions": int(masks.size), "lps": int(piv.size),
           "worst_duality_gap": gap, "gap_checked_lps": checked,
           "pivots_total": int(piv.sum()), "pivots_max": int(piv.max()),
           "pivot_histogram": {str(k): int(v) for k, v in enumerate(np.bincount(piv.ravel())) if v},
           "alpha_max": float(res["alpha"].max())}
    rec["ms_all_outputs"] = gpu_ms(lambda: ops.maximin_lottery(U3, base, masks),
                                   args.warmup, args.reps, args.inner)
    rec["ms_alpha_only"] = gpu_ms(lambda: ops.maximin_lottery(U3, base, masks, with_q=False,
                                                              with_lam=False),
                                  args.warmup, args.reps, args.inner)
    rec["us_per_lp_alpha_only"] = round(rec["ms_alpha_only"][0] * 1e3 / piv.size, 4)
    print(f"{name}: {rec}", file=sys.stderr, flush=True)
    return rec, res


def highs_alpha(linprog, U, base, S):
    """One coalition's LP as the reference poses it, by HiGHS; None when it does not solve."""
    n, m = U.shape
    c = np.zeros(m + 1)
    c[-1] = -1.0
    A_ub = np.hstack([-U[S], base[S, None]])
    A_eq = np.concatenate([np.ones(m), [0.0]])[None]
    res = linprog(c, A_ub=A_ub, b_ub=np.zeros(len(S)), A_eq=A_eq, b_eq=[len(S) / n],
                  bounds=[(0.0, None)] * m + [(None, None)], method="highs")
    return float(res.x[-1]) if res.success else None


def host_compare(U3, base, masks, res, calls):
    """HiGHS and the restatement over `calls` (problem, lottery) pairs spread over the sweep."""
    U3, base = U3.cpu().numpy(), base.cpu().numpy()
    alpha = res["alpha"].cpu().numpy()
    picks = np.linspace(0, U3.shape[0] - 1, calls).astype(int)
    members = [maximin_ref.members(int(mk), U3.shape[1]) for mk in masks]
    out = {"calls": int(calls), "lps": int(calls * masks.size)}
    t = time.perf_counter()
    worst = 0.0
    for k in picks:
        for ci, mk in enumerate(masks):
            r = maximin_ref.solve(U3[k], base[k], int(mk))
            worst = max(worst, abs(r["alpha"] - alpha[k, ci]) / r["alpha"])
    out["restatement_s_per_call"] = round((time.perf_counter() - t) / calls, 4)
    out["restatement_vs_gpu_max_rel"] = worst
    try:
        from scipy.optimize import linprog
    except ImportError:
        out["highs_s_per_call"] = "not measured (no scipy on this box)"
        return out
    t = time.perf_counter()
    worst = 0.0
    for k in picks:
        for ci, S in enumerate(members):
            a = highs_alpha(linprog, U3[k], base[k], S)
            if a is not None:
                worst = max(worst, abs(a - alpha[k, ci]) / abs(a))
    out["highs_s_per_call"] = round((time.perf_counter() - t) / calls, 4)
    out["highs_vs_gpu_max_rel"] = worst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "maximin_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window")
    ap.add_argument("--host-calls", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maximin_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    rho = np.linspace(0.6, 5.0, 20)                                  # core.py:348

    Us = torch.cat([core.compute_utilities_fp64(*core.generate_params(3, 4, 8, 6, seed=42 + i), rho)
                    for i in range(3)]).contiguous()                 # core.py:342-366
    U3, base = core.sweep_lotteries(Us, MAX_ITERS, TOL)
    sweep, res = run("sweep", U3, base, core.coalition_masks(6), args, 1)
    sweep["host"] = host_compare(U3, base, core.coalition_masks(6), res, args.host_calls)
    sweep["host"]["highs_sweep_s_extrapolated"] = (
        round(sweep["host"]["highs_s_per_call"] * 180, 1)
        if isinstance(sweep["host"]["highs_s_per_call"], float) else "not measured")

    Uw = core.compute_utilities_fp64(*core.generate_params(3, 4, 8, 16, seed=42), rho[[9]])
    Uw3, basew = core.sweep_lotteries(Uw.contiguous(), MAX_ITERS, TOL)
    wide, _ = run("wide", Uw3[2:], basew[2:], core.coalition_masks(16), args, 97)   # the uniform one

    line = {"bench": "maximin_lottery", "device": torch.cuda.get_device_name(dev),
            "warmup": args.warmup, "reps": args.reps, "inner": args.inner,
            "ms": "per launch [median, min, max] over the windows",
            "sweep": sweep, "wide": wide}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
