"""Host restatement of the induced-policy rollout as the gfx950 kernels (csrc/lottery.hip,
``cs_policy_rollout``) state it: numpy's PCG64 stream in Python integers, one double per draw,
and Generator.choice's rule cdf = cumsum(p); cdf /= cdf[-1]; a = searchsorted(cdf, u, "right").
The expected values of tests/test_rollout_host.py and tests/test_rollout_gpu.py, and the host
side of tools/rollout_bench.py."""
from __future__ import annotations

import numpy as np

MULT = 0x2360ED051FC65DA44385DF649FCCF645     # PCG64's 128-bit LCG multiplier
MASK128 = (1 << 128) - 1
MASK64 = (1 << 64) - 1


def seed_state(seed):
    """(state, inc) of np.random.default_rng(seed), two 128-bit integers."""
    st = np.random.PCG64(seed).state["state"]
    return int(st["state"]), int(st["inc"])


def step(state, inc):
    return (state * MULT + inc) & MASK128


def output(state):
    """XSL-RR: high word ^ low word, rotated right by the state's top six bits."""
    x = (state >> 64) ^ (state & MASK64)
    rot = state >> 122
    return ((x >> rot) | (x << ((64 - rot) & 63))) & MASK64


def advance(state, inc, delta):
    """The state after ``delta`` steps, O(log delta): square-and-multiply on (MULT, inc)."""
    acc_mult, acc_plus, cur_mult, cur_plus = 1, 0, MULT, inc
    while delta > 0:
        if delta & 1:
            acc_mult = (acc_mult * cur_mult) & MASK128
            acc_plus = (acc_plus * cur_mult + cur_plus) & MASK128
        cur_plus = ((cur_mult + 1) * cur_plus) & MASK128
        cur_mult = (cur_mult * cur_mult) & MASK128
        delta >>= 1
    return (acc_mult * state + acc_plus) & MASK128


def uniforms(seed, first_draw, count):
    """Draws first_draw .. first_draw + count - 1 (0-based) of default_rng(seed).random():
    draw k is the output of the state advanced k + 1 times, (out >> 11) * 2^-53."""
    state, inc = seed_state(seed)
    state = advance(state, inc, first_draw)
    words = np.empty(count, dtype=np.uint64)
    for k in range(count):
        state = (state * MULT + inc) & MASK128
        x = (state >> 64) ^ (state & MASK64)           # output(state), inlined: this loop is
        rot = state >> 122                             # the restatement's whole cost
        words[k] = ((x >> rot) | (x << (64 - rot))) & MASK64
    return (words >> np.uint64(11)) * (1.0 / 9007199254740992.0)


def cdf_tables(policy_levels):
    """Per level the rows' cdf: np.cumsum, then divided by the last entry, row by row."""
    tables = []
    for level in policy_levels:
        level = np.asarray(level, dtype=np.float64)
        cdf = np.empty_like(level)
        for s in range(level.shape[0]):
            c = level[s].cumsum()
            c /= c[-1]
            cdf[s] = c
        tables.append(cdf)
    return tables


def walk(policy_levels, B, L, seed, first_sample, num_samples):
    """The leaves (prefix index in base B, int64 [num_samples]) of the samples first_sample ..
    first_sample + num_samples - 1: sample i takes the draws i * L .. i * L + L - 1.  A level's
    samples are searched row by row (np.searchsorted, side "right")."""
    cdf = cdf_tables(policy_levels)
    u = uniforms(seed, first_sample * L, num_samples * L).reshape(num_samples, L)
    s = np.zeros(num_samples, dtype=np.int64)
    for t in range(L):
        a = np.empty(num_samples, dtype=np.int64)
        for row in np.unique(s):
            at = s == row
            a[at] = np.searchsorted(cdf[t][row], u[at, t], side="right")
        s = s * B + a
    return s


def host_loop(policy_levels, B, L, seed, num_samples):
    """The reference's loop (core.py:313-328) over the tables: num_samples * L calls of
    ``rng.choice(B, p=row)``; returns the counts per leaf."""
    rng = np.random.default_rng(seed)
    counts = np.zeros(B ** L, dtype=np.int64)
    for _ in range(num_samples):
        s = 0                      # the prefix's index in base B
        for t in range(L):
            s = s * B + int(rng.choice(B, p=policy_levels[t][s]))
        counts[s] += 1
    return counts
