#!/usr/bin/env python3
"""cs_nash_lottery against the host restatement (tests/lottery_ref.py) on the same box.

  sweep   the 60 problems of the reference's core.main (3 seeds x 20 rho, 6 agents x 81 leaves,
          max_iters 1500, tol 1e-11) as ONE launch, in each variant
  mid     one 16 x 1000 problem, the largest of the tests that both variants take
  big     one 32 x 16384 problem: 4 MiB of utilities, so the global variant only (the staged
          one is rejected there; that rejection is checked)

GPU times are HIP events around the launch (median of --reps after --warmup launches); the
host time is a wall clock around lottery_ref.solve over the same problems.  Every timed
result is compared with the host's p.  Writes one JSON line:

  python tools/lottery_bench.py [--out profiles/lottery_bench.jsonl]
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
import lottery_ref  # noqa: E402

MAX_ITERS, TOL = 1500, 1e-11      # the reference's sweep (core.py:369)


def gpu_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return statistics.median(out), min(out), max(out)


def host_s(Us):
    t = time.perf_counter()
    res = [lottery_ref.solve(U, max_iters=MAX_ITERS, tol=TOL) for U in Us]
    return time.perf_counter() - t, res


def run(name, Us, variants, host, args, dev):
    Ut = torch.as_tensor(np.ascontiguousarray(Us), device=dev)
    rec = {"problems": int(Us.shape[0]), "A": int(Us.shape[1]), "m": int(Us.shape[2])}
    if host:
        secs, refs = host_s(Us)
        rec["host_s"] = round(secs, 3)
    for v in variants:
        res = {}

        def launch():
            res.update(ops.nash_lottery(Ut, max_iters=MAX_ITERS, tol=TOL, variant=v))

        med, lo, hi = gpu_ms(launch, args.warmup, args.reps)
        r = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
             "iters_total": int(res["iters"].sum()),
             "gap_max": float(res["gap"].max())}
        if host:
            p = res["p"].cpu().numpy()
            r["max_abs_p_vs_host"] = float(max(np.abs(p[k] - refs[k]["p"]).max()
                                               for k in range(len(refs))))
            r["iters_equal_host"] = bool(all(int(res["iters"][k]) == refs[k]["iters"]
                                             for k in range(len(refs))))
            r["host_over_gpu"] = round(rec["host_s"] * 1e3 / med, 1)
        rec[f"variant{v}"] = r
        print(f"{name} variant {v}: {r}", file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lottery_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement's runs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lottery_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())

    sweep = []
    for run_i in range(3):                                   # core.py:356-366
        v, w = core.generate_params(3, 4, 8, 6, seed=42 + run_i)
        for rho in np.linspace(0.6, 5.0, 20):
            sweep.append(core.compute_utilities(v, w, rho)[0])
    rng = np.random.default_rng(0)
    mid = np.exp(rng.normal(size=(1, 16, 1000)))
    big = np.exp(rng.normal(size=(1, 32, 16384)))
    host = not args.no_host
    line = {"bench": "nash_lottery", "device": torch.cuda.get_device_name(dev),
            "max_iters": MAX_ITERS, "tol": TOL, "warmup": args.warmup, "reps": args.reps,
            "sweep": run("sweep", np.stack(sweep), (0, 1, 2), host, args, dev),
            "mid": run("mid", mid, (1, 2), host, args, dev),
            "big": run("big", big, (0, 2), host, args, dev)}
    try:
        ops.nash_lottery(torch.as_tensor(big[0], device=dev), max_iters=1, variant=1)
        line["big"]["variant1"] = "accepted"
    except ops.CSError:
        line["big"]["variant1"] = "rejected (A * m * 8 exceeds the LDS)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
