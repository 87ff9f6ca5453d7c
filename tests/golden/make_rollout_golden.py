"""Generate tests/golden/rollout_golden.npz FROM THE REFERENCE ITSELF: results of its
``induced_policy_rollout`` (core.py:297-332), the host loop of ``rng.choice`` calls.

The reference is imported exactly as make_golden.py imports it; nothing of it is copied, only
input / output DATA is written.  Per case ``<name>``: p_<name> (the lottery), B_<name>, L_<name>,
seed_<name>, n_<name> (the samples), p_hat_<name> and tv_<name> (what the reference returned).
``cases`` lists the names.

  ref         the reference's own check (core.py:437-444): the Nash-welfare lottery of seed 42 at
              the middle rho (p_42_9 of lottery_golden.npz), B, L = 3, 4, seed 7, 200,000 samples
  z<B>_<L>_<seed>   a random lottery with the whole subtree under first action 0 zeroed and a
              deeper one under (B-1, B-1), 5,000 samples
  one_leaf    B, L = 1, 3: a single leaf
  point       all mass on one leaf: every sample must reach it

Usage:  python tests/golden/make_rollout_golden.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import itertools
import os

import numpy as np

from make_golden import import_reference

HERE = os.path.dirname(os.path.abspath(__file__))


def zeroed_lottery(B, L, seed):
    m = B ** L
    p = np.random.default_rng(1000 * B + 10 * L + seed % 7).random(m)
    p[: m // B] = 0.0
    p[-(m // B // B):] = 0.0
    return p / p.sum()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    core = import_reference(args.reference)

    lot = np.load(os.path.join(HERE, "lottery_golden.npz"))
    cases = [("ref", lot["p_42_9"], 3, 4, 7, 200_000)]
    for (B, L), seed in itertools.product([(2, 6), (5, 2), (3, 4)], [0, 7, 12345]):
        cases.append((f"z{B}_{L}_{seed}", zeroed_lottery(B, L, seed), B, L, seed, 5000))
    cases.append(("one_leaf", np.ones(1), 1, 3, 7, 5000))
    point = np.zeros(81)
    point[40] = 1.0
    cases.append(("point", point, 3, 4, 7, 5000))

    out = {"cases": np.array([c[0] for c in cases])}
    for name, p, B, L, seed, n in cases:
        leaves = list(itertools.product(range(B), repeat=L))
        p_hat, tv = core.induced_policy_rollout(p, leaves, B, L, num_samples=n, seed=seed)
        print(f"{name}: B {B} L {L} seed {seed} samples {n} tv {tv:.6f}")
        out[f"p_{name}"] = p
        out[f"B_{name}"], out[f"L_{name}"] = B, L
        out[f"seed_{name}"], out[f"n_{name}"] = seed, n
        out[f"p_hat_{name}"], out[f"tv_{name}"] = p_hat, tv
    np.savez_compressed(os.path.join(HERE, "rollout_golden.npz"), **out)
    print("wrote rollout_golden.npz")


if __name__ == "__main__":
    main()
