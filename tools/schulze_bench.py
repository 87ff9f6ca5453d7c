#!/usr/bin/env python3
"""cs_schulze on the shapes the Habermas Machine's aggregation meets here.

  one       one election of 5 voters x 4 candidates (the reference's Figure-1 size)
  sweep     4,096 elections of 16 x 16 in ONE launch (issues x seeds, bootstrap resamples)
  c2        one election of 8 x 64 from float scores (BASELINE C2's agent x candidate matrix)
  wide      one election of 16 x 128 (the kernel's candidate limit)
  host      the reference's three nested Python loops per stage, restated literally
            (tests/schulze_ref.py, form "loops"), on the same box's CPU for the sizes where
            they end within a few seconds: HOST figures, a wall clock around one call

GPU times are HIP events around ops.schulze (the launch and the allocation of its outputs;
median of --reps after --warmup launches).  Every timed result is compared with the vectorised
restatement (form "fast").  Writes one JSON line:

  python tools/schulze_bench.py [--out profiles/schulze_bench.jsonl]
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
import schulze_ref as sr  # noqa: E402

SHAPES = [("one", 1, 5, 4, "rankings"), ("sweep", 4096, 16, 16, "rankings"),
          ("c2", 1, 8, 64, "scores"), ("wide", 1, 16, 128, "rankings")]
HOST_LOOP_MAX_C = 64          # the loops take about 2 s at 128 candidates


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


def run(name, E, R, C, kind, dev, args):
    rng = np.random.default_rng(E * 1000 + C)
    if kind == "scores":
        x = rng.standard_normal((E, R, C)).astype(np.float32)
    else:
        x = rng.integers(0, C, (E, R, C)).astype(np.int32)
    ballots = np.stack([rng.permutation(C) for _ in range(E)]).astype(np.int32)
    xt, bt = torch.as_tensor(x, device=dev), torch.as_tensor(ballots, device=dev)
    res = {}

    def launch():
        res.update(ops.schulze(xt, kind=kind, ballot=bt))

    med, lo, hi = gpu_ms(launch, args.warmup, args.reps)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    checked = list(range(E)) if E <= 64 else list(range(0, E, E // 64))
    equal = True
    for e in checked:
        want = sr.solve(x[e], kind, ballot=ballots[e])
        equal &= all(np.array_equal(got[k][e], want[k])
                     for k in ("defeats", "strengths", "ranking", "untied"))
        equal &= int(got["winner"][e]) == want["winner"] and int(got["status"][e]) == 0
    rec = {"elections": E, "voters": R, "candidates": C, "kind": kind, "ms": round(med, 4),
           "ms_min": round(lo, 4), "ms_max": round(hi, 4), "us_per_election": round(med * 1e3 / E, 3),
           "checked": len(checked), "equal_restatement": bool(equal)}
    if C <= HOST_LOOP_MAX_C:
        t = time.perf_counter()
        want = sr.solve(x[0], kind, ballot=ballots[0], form="loops") if kind != "scores" else \
            sr.solve(sr.dense_ranks_of_scores(x[0]), ballot=ballots[0], form="loops")
        rec["host_loops_s_per_election"] = round(time.perf_counter() - t, 4)
        rec["host_loops_equal"] = bool(np.array_equal(want["untied"], got["untied"][0]))
    print(f"{name}: {rec}", file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "schulze_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("schulze_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    line = {"bench": "schulze", "device": torch.cuda.get_device_name(dev), "warmup": args.warmup,
            "reps": args.reps}
    for name, E, R, C, kind in SHAPES:
        line[name] = run(name, E, R, C, kind, dev, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
