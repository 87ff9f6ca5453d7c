#!/usr/bin/env python3
"""cs_policy_rollout on the shapes of the reference's policy-lottery equivalence check.

  one     the Nash-welfare lottery of seed 42 at the middle rho (6 agents x 81 leaves, B, L =
          3, 4), 200,000 samples, seed 7: the reference's own check (core.py:437-444)
  sweep   the 60 lotteries of the reference's sweep (3 seeds x 20 rho), 200,000 samples each,
          as ONE launch
  host    the host loop this kernel replaced (tests/rollout_ref.host_loop: num_samples * L calls
          of rng.choice over the GPU's policy tables) on the same box at 20,000 samples; its
          200,000-sample figure is that time x 10 and labelled as extrapolated

GPU times are HIP events around cs_lottery_policy + cs_policy_rollout (tables, cdf, walk and the
zeroing of the counts; median of --reps after --warmup launches); ``wall_ms`` is a wall clock
around core.induced_policy_rollout, host copies and the p_hat / tv arithmetic included.  The
20,000-sample counts of the kernel are compared with the host loop's.  Writes one JSON line:

  python tools/rollout_bench.py [--out profiles/rollout_bench.jsonl]
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
import rollout_ref  # noqa: E402

B, L, D, AGENTS = 3, 4, 8, 6          # core.py:342-344
SAMPLES, SEED = 200_000, 7            # core.py:441
HOST_SAMPLES = 20_000


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


def run(name, pt, args):
    states = torch.as_tensor(np.tile(ops.pcg64_state(SEED), (pt.shape[0], 1)).view(np.int64),
                             device=pt.device)
    res = {}

    def launch():
        res.update(ops.policy_rollout(ops.lottery_policy(pt, B, L, flat=True), B, L, states,
                                      SAMPLES))

    med, lo, hi = gpu_ms(launch, args.warmup, args.reps)
    counts = res["counts"].cpu().numpy()
    ps = pt.cpu().numpy()
    tv = [0.5 * np.sum(np.abs(counts[k] / counts[k].sum() - ps[k])) for k in range(len(ps))]
    rec = {"lotteries": int(pt.shape[0]), "samples": SAMPLES, "draws": int(pt.shape[0]) * SAMPLES * L,
           "ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
           "status_ok": bool((res["status"] == 0).all()),
           "samples_counted": bool((counts.sum(axis=1) == SAMPLES).all()),
           "tv_max": float(max(tv))}
    print(f"{name}: {rec}", file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())

    rho_grid = np.linspace(0.6, 5.0, 20)                     # core.py:348
    Us = []
    for run_i in range(3):                                   # core.py:356-366
        v, w = core.generate_params(B, L, D, AGENTS, seed=42 + run_i)
        Us.append(core.compute_utilities_fp64(v, w, rho_grid))
    sweep = ops.nash_lottery(torch.cat(Us).contiguous(), max_iters=1500, tol=1e-11)["p"]
    mid = len(rho_grid) // 2                                 # core.py:438, seed 42
    one = sweep[mid:mid + 1].contiguous()

    line = {"bench": "policy_rollout", "device": torch.cuda.get_device_name(dev), "B": B, "L": L,
            "seed": SEED, "warmup": args.warmup, "reps": args.reps,
            "one": run("one", one, args), "sweep": run("sweep", sweep, args)}

    p_one = one[0].cpu().numpy()
    leaves = core.enumerate_leaves(B, L)
    core.induced_policy_rollout(p_one, leaves, B, L, num_samples=SAMPLES, seed=SEED)   # warm
    t = time.perf_counter()
    core.induced_policy_rollout(p_one, leaves, B, L, num_samples=SAMPLES, seed=SEED)
    line["one"]["wall_ms"] = round((time.perf_counter() - t) * 1e3, 3)

    tables = core.induced_policy(p_one, B, L)
    t = time.perf_counter()
    host_counts = rollout_ref.host_loop(tables, B, L, SEED, HOST_SAMPLES)
    host_s = time.perf_counter() - t
    flat = ops.lottery_policy(one[0], B, L, flat=True)
    gpu_counts = ops.policy_rollout(flat, B, L, ops.pcg64_state(SEED), HOST_SAMPLES)["counts"]
    line["host"] = {"samples": HOST_SAMPLES, "host_s": round(host_s, 3),
                    "host_s_at_200000_extrapolated": round(host_s * SAMPLES / HOST_SAMPLES, 2),
                    "counts_equal_gpu": bool(np.array_equal(gpu_counts.cpu().numpy(), host_counts))}
    line["host_extrapolated_over_gpu_one"] = round(
        line["host"]["host_s_at_200000_extrapolated"] * 1e3 / line["one"]["ms"], 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
