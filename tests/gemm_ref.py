"""Exact cases for cs_gemm_bf16 / cs_gemm_bf16_packed (csrc/gemm.hip): operands, references,
a Python restatement of the host dispatch, and the list of GPU cases.  No GPU needed here;
tests/test_gemm_cases_host.py checks the cases, tests/test_gemm_exact_gpu.py runs them.

Why the cases need no tolerance.  X and W hold integers |v| <= 15 (bf16-exact); W is then
scaled by a power of two 2^e (still exact).  Every product is an integer of magnitude
<= 225 times 2^e, and every partial sum over K <= 64 * 49 elements, in ANY association
order, is an integer below 225 * K < 2^24 times 2^e: fp32 holds it exactly.  So whatever
the MFMA's internal order, the K split, the wave fold or the weight packing, the fp32
accumulator holds the exact sum and the only rounding left is the last one to bf16.  The
expected output is bf16_rne(exact integer sum * 2^e), computed on the CPU in fp64 (exact
below 2^53) and rounded by torch; a K split's partial p is the exact sum over its own K
slice as fp32.

All cases of one (M, N) share one pair of integer operands of MAX_STEPS K steps; a case
with K = 64 * n takes their first K columns, so the per-step products are computed once
(prefix_products) and every expectation is a difference of two prefix sums."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

BK = 64                       # kGemmBK
AMAX = 15                     # |x|, |w| <= 15
NK = (1, 2, 3, 4, 5, 7)       # K steps per split: the ws loop runs 3 steps + a 1- or 2-step
                              # tail, ws2 a ring of 3 with `if (t + r < nk)`
SPLITS = (1, 2, 3)
ZERO_STEPS = (5, 16, 20)      # K / 64 run with splits = 0: cs_gemm_splits picks 1, 2, 2
THIN_NSTEPS = (1, 7, 8, 9, 17, 25, 33, 49)
MAX_STEPS = 21                # 7 steps x 3 splits
THIN_MAX_STEPS = 49
THIN_MAX_ROWS = 80
ACTS = ("silu", "gelu_tanh")


# --- operands and references ---------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def operands(M, N, steps, seed):
    """Integer operands (int64) X [M, 64 * steps], W [N, 64 * steps] in [-15, 15]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    xi = torch.randint(-AMAX, AMAX + 1, (M, steps * BK), generator=g, dtype=torch.int64)
    wi = torch.randint(-AMAX, AMAX + 1, (N, steps * BK), generator=g, dtype=torch.int64)
    return xi, wi


@functools.lru_cache(maxsize=4)
def prefix_products(M, N, steps, seed):
    """C [steps + 1, M, N] fp64: C[t] = the exact integer product over K steps [0, t)."""
    xi, wi = operands(M, N, steps, seed)
    x, w = xi.double(), wi.double()
    C = torch.zeros(steps + 1, M, N, dtype=torch.float64)
    for t in range(steps):
        C[t + 1] = C[t] + x[:, t * BK:(t + 1) * BK] @ w[:, t * BK:(t + 1) * BK].t()
    return C


def to_bf16(v64, e=0):
    """bf16_rne(v * 2^e): torch's round-to-nearest-even conversion of an fp32-exact value."""
    return (v64 * 2.0 ** e).to(torch.bfloat16)


def bits(t):
    """The bit patterns of a bf16 / fp32 tensor as integers (NaN payloads and signs of zero
    compare like everything else)."""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@dataclass(frozen=True)
class Case:
    family: str          # "ws" (variant 1), "ws2" (2-4), "thin" (5-7)
    variant: int
    gated: bool
    packed: bool
    M: int
    N: int = 512         # W rows (gated: 2F)

    @property
    def id(self):
        return (f"{self.family}-v{self.variant}-{'gated' if self.gated else 'plain'}-"
                f"{'packed' if self.packed else 'rowmajor'}-M{self.M}-N{self.N}")

    __repr__ = __str__ = lambda self: self.id

    @property
    def e(self):
        """W scale exponent.  Gated: 2^-10 keeps the gate values (|sum| of a few thousand)
        where SiLU / tanh-GeLU are not saturated."""
        return -10 if self.gated else (-20, 0, 20)[(self.M + self.variant) % 3]

    @property
    def seed(self):
        return 7000 + self.M + self.N

    @property
    def steps(self):
        return THIN_MAX_STEPS if self.family == "thin" else MAX_STEPS

    def shapes(self):
        """(nk, splits) pairs, K = 64 * nk * max(splits, 1); splits = 0: the library's choice."""
        if self.family == "thin":
            return [(n, 1) for n in THIN_NSTEPS]
        if self.gated:
            return [(nk, 1) for nk in NK]
        return [(nk, s) for nk in NK for s in SPLITS] + [(n, 0) for n in ZERO_STEPS]

    def operands(self):
        return operands(self.M, self.N, self.steps, self.seed)

    def prefix(self):
        return prefix_products(self.M, self.N, self.steps, self.seed)

    def x_bf16(self):
        return self.operands()[0].to(torch.bfloat16)

    def w_bf16(self):
        return to_bf16(self.operands()[1].double(), self.e)

    def expected(self, n_steps):
        """bf16 [M, N] of the first 64 * n_steps columns (gated: the rounded gate | up halves)."""
        return to_bf16(self.prefix()[n_steps], self.e)

    def expected_partials(self, nk, splits):
        """fp32 [splits, M, N]: partial p is the exact product over K steps [p nk, (p + 1) nk)."""
        C = self.prefix()
        return torch.stack([(C[(p + 1) * nk] - C[p * nk]) * 2.0 ** self.e
                            for p in range(splits)]).float()


def gated_expected(ops, gu_bf16, act, dev):
    """act(gate) * up of the host-computed, RNE-rounded exact halves through cs_gated_act
    (itself pinned element by element in tests/test_row_kernels_gpu.py)."""
    F = gu_bf16.shape[1] // 2
    gu = gu_bf16.to(dev)
    return ops.gated_act(gu[:, :F], gu[:, F:], act)


# --- selector cases ------------------------------------------------------------------------------

SEL_STRIDE = 5                # coprime to 192 = 2^6 * 3 and to 448 = 2^6 * 7


def selector_w(N, K):
    """W[n][k] = ((131 n + 7 k) mod 251) - 125: |v| <= 125, bf16-exact."""
    n = torch.arange(N, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    return (n * 131 + k * 7) % 251 - 125


def selector_shifts(M, K):
    """Shifts under which rows m = 0..M-1 with k(m) = (5 m + shift) mod K visit every k: with
    shift = 5 j M the rows of shift j stand for m' = m + j M, and 5 m' mod K runs over all of
    0..K-1 as m' does (5 is coprime to K) -- every K step, both 32-halves, every 8-chunk and
    every element inside a chunk."""
    return [SEL_STRIDE * j * M for j in range(-(-K // M))]


def selector_k(M, K, shift):
    return (torch.arange(M, dtype=torch.int64) * SEL_STRIDE + shift) % K


def selector_x(M, K, shift):
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), selector_k(M, K, shift)] = 1.0
    return x


def selector_expected(wi, M, K, shift):
    """Y[m][n] = W[n][k(m)] exactly."""
    return wi[:, selector_k(M, K, shift)].t().contiguous()


def selector_decode(wi, got, want, M, K, shift, limit=6):
    """Which W element each wrong output actually holds: the (n, k) candidates of its value in
    its own W row (a wrong k: K step, half, chunk, lane) and in its own K column (a wrong n)."""
    ks = selector_k(M, K, shift)
    bad = (got != want).nonzero()
    lines = [f"{len(bad)} of {got.numel()} outputs wrong"]
    for m, n in bad[:limit].tolist():
        v = float(got[m, n])
        k_same_row = (wi[n].double() == v).nonzero().flatten().tolist()
        n_same_col = (wi[:, ks[m]].double() == v).nonzero().flatten().tolist()
        k = int(ks[m])
        lines.append(f"  y[{m}][{n}] = {v:g}, want W[{n}][{k}] = {float(want[m, n]):g} (step "
                     f"{k // 64}, half {k % 64 // 32}, chunk {k % 32 // 8}, elem {k % 8}); that "
                     f"value is W[{n}][k] at k = {k_same_row[:8]} and W[n][{k}] at n = {n_same_col[:8]}")
    return "\n".join(lines)


# --- the host dispatch of gemm.hip, restated -----------------------------------------------------

WS2_MT = (2, 4, 5, 8, 9, 12, 17, 18)     # kWs2MT
WS_MAX_MW = 9                            # kGemmMaxMW
# kGemmVariants: variant -> (family, W rows per workgroup, most row tiles per workgroup)
VARIANTS = {1: ("ws", 128, 18), 2: ("ws2", 256, 18), 3: ("ws2", 128, 18), 4: ("ws2", 256, 9),
            5: ("thin", 16, 5), 6: ("thin", 32, 5), 7: ("thin", 16, 5)}


def thin_variant(variant):
    return VARIANTS.get(variant or 2, ("",))[0] == "thin"


def resolve_variant(variant, N, gated):
    variant = variant or 2
    if VARIANTS[variant][1] == 256 and N % 256:
        return 1 if gated else 3
    return variant


def ws_mw(M):
    tiles = (M + 15) // 16
    return min((tiles + 1) // 2, WS_MAX_MW)


def ws2_rows(M, max_tiles=18, packed=False):
    """(row tiles per workgroup, row blocks)"""
    tiles = (M + 15) // 16
    mb = (tiles + max_tiles - 1) // max_tiles
    per = (tiles + mb - 1) // mb
    mt = next((c for c in WS2_MT if (c != 5 or packed) and c >= per), 18)
    return mt, (tiles + mt - 1) // mt


def gemm_tiles(variant, M, N):
    """workgroups per K split: column tiles x row blocks (the same on a packed weight)"""
    _, bn, max_tiles = VARIANTS[variant]
    if variant == 1:
        mw = ws_mw(M)
        return (N // bn) * ((M + 32 * mw - 1) // (32 * mw))
    return (N // bn) * ws2_rows(M, max_tiles)[1]


def ws2_grid(cells, mblocks):
    return (cells + 7) // 8 * 8 * mblocks if mblocks > 1 else cells


def gemm_splits(M, N, K, gated, variant):
    """cs_gemm_splits (1 for a call cs_gemm_bf16 rejects: here a variant outside 0..7)"""
    if M <= 0 or N <= 0 or K <= 0 or N % 128:
        return 0
    if gated or thin_variant(variant) or (variant or 2) not in VARIANTS:
        return 1
    tiles = gemm_tiles(resolve_variant(variant, N, gated), M, N)
    s = 1
    while tiles * s < 256 and K % (BK * s * 2) == 0 and K // (BK * s * 2) >= 8:
        s *= 2
    return s


def thin_slices(nsteps, waves):
    """K steps per wave: wave w runs [w n / WAVES, (w + 1) n / WAVES)"""
    return [(w + 1) * nsteps // waves - w * nsteps // waves for w in range(waves)]


def launch(variant, M, N, K, gated=False, packed=False, splits=1):
    """What one cs_gemm_bf16(_packed) call launches (gemm_plan): {"name": the template
    instantiation, "nk", "splits", "grid"} and, thin, "waves", "ring", "slices"."""
    gated, packed = int(bool(gated)), bool(packed)
    variant = resolve_variant(variant, N, gated)
    family, bn, max_tiles = VARIANTS[variant]
    assert N % 128 == 0 and K % BK == 0 and not (packed and family != "ws2")
    if splits <= 0:
        splits = gemm_splits(M, N, K, gated, variant)
    assert K % (BK * splits) == 0 and not (gated and splits > 1)
    if family == "thin":
        assert M <= THIN_MAX_ROWS and splits == 1
        mt = (M + 15) // 16
        if gated:         # gemm_form: one gate + one up tile; 16 waves up to 3 row tiles
            ft, waves, ring = (2, 16, 2) if variant == 7 and mt <= 3 else (2, 8, 3)
        else:
            ft, waves, ring = {5: (1, 8, 3), 6: (2, 8, 3), 7: (1, 16, 2)}[variant]
        n_out = N // 2 if gated else N
        return {"name": f"thin<{mt},{ft},{gated},{waves},{ring}>", "nk": K // BK, "splits": 1,
                "grid": n_out // 16 if gated else n_out // (16 * ft), "waves": waves,
                "ring": ring, "slices": thin_slices(K // BK, waves)}
    nk = K // (BK * splits)
    if family == "ws":
        return {"name": f"ws<{ws_mw(M)},{gated}>", "nk": nk, "splits": splits,
                "grid": gemm_tiles(1, M, N) * splits}
    mt, mb = ws2_rows(M, max_tiles, packed)
    if gated and packed and bn == 256 and M <= 80 and N % 224 == 0:     # gemm_form: 7 waves
        mt = mt if mt in (2, 4) else 5
        return {"name": f"ws2<{mt},2,1,7,1>", "nk": nk, "splits": 1, "grid": N // 224}
    nt, waves = (2, 4) if variant == 3 and gated else (bn // 128, 8)
    cells = (N // bn) * splits
    return {"name": f"ws2<{mt},{nt},{gated},{waves},{int(packed)}>", "nk": nk, "splits": splits,
            "grid": ws2_grid(cells, mb), "cells": cells, "mblocks": mb}


def all_instantiations():
    """Every template instantiation gemm_compiled admits, so gemm_launch can reach (104)."""
    out = [f"ws<{mw},{g}>" for g in (0, 1) for mw in range(1, WS_MAX_MW + 1)]
    # ws2<.., NT, GATED, WAVES, PACKED>: gated variant 3, gated, variant 3, the default;
    # the 5-tile row block on packed weights only (ws2_rows)
    for nt, g, waves in ((2, 1, 4), (2, 1, 8), (1, 0, 8), (2, 0, 8)):
        for p in (0, 1):
            out += [f"ws2<{mt},{nt},{g},{waves},{p}>" for mt in WS2_MT if mt != 5 or p]
    out += [f"ws2<{mt},2,1,7,1>" for mt in (2, 4, 5)]                  # the 7-wave form
    out += [f"thin<{mt},2,1,16,2>" for mt in (1, 2, 3)]                # gated variant 7
    for ft, g, waves, ring in ((2, 1, 8, 3), (1, 0, 8, 3), (2, 0, 8, 3), (1, 0, 16, 2)):
        out += [f"thin<{mt},{ft},{g},{waves},{ring}>" for mt in range(1, 6)]
    return out


# --- the GPU cases -------------------------------------------------------------------------------

WS_M = sorted({m for mw in range(1, 10) for m in (32 * mw, 32 * (mw - 1) + 1)} | {289})
WS2_M = (1, 16, 17, 32, 33, 64, 65, 80, 81, 128, 129, 144, 145, 192, 193, 272, 273, 288, 289,
         304, 577)
WS2_V4_M = (144, 145, 288, 289, 433)
THIN_M = (1, 16, 17, 32, 33, 48, 49, 64, 65, 80)
GATED7_M = (1, 17, 32, 33, 64, 65, 80)
GATED7_N = 1792               # 2F = 8 x 224: the 7-wave packed gated form


@functools.lru_cache(maxsize=None)
def cases():
    """The exact GPU cases: (family, variant, gated, packed, M) at the smallest row counts
    that reach each tile count with a full and with a ragged last tile."""
    out = []
    for gated in (False, True):
        out += [Case("ws", 1, gated, False, M) for M in WS_M]
        for variant in (2, 3):
            for packed in (False, True):
                out += [Case("ws2", variant, gated, packed, M) for M in WS2_M]
        for packed in (False, True):
            out += [Case("ws2", 4, gated, packed, M) for M in WS2_V4_M]
        for variant in (5, 6, 7):
            out += [Case("thin", variant, gated, False, M) for M in THIN_M]
    out += [Case("ws2", 2, True, True, M, GATED7_N) for M in GATED7_M]
    out += [Case("ws2", 4, True, True, 49, GATED7_N)]
    # N % 256 != 0: resolve_variant sends variant 2 to 3 (gated: to 1), the default 0 likewise
    out += [Case("ws2", 2, False, False, 33, 384), Case("ws2", 2, True, False, 33, 384),
            Case("ws2", 0, False, True, 17, 384)]
    return tuple(out)


def case_launches(c):
    return [launch(c.variant, c.M, c.N, BK * nk * max(s, 1), c.gated, c.packed, s)
            for nk, s in c.shapes()]


def instantiation_of(c):
    names = {l["name"] for l in case_launches(c)}
    assert len(names) == 1, (c, names)
    return names.pop()


@functools.lru_cache(maxsize=None)
def guard_cases():
    """One case per instantiation for the guarded-output and poisoned-padding tests: the
    smallest M with a ragged last row tile (M % 16 != 0) that reaches it."""
    best = {}
    for c in cases():
        name = instantiation_of(c)
        key = (c.M % 16 == 0, c.M)
        if name not in best or key < best[name][0]:
            best[name] = (key, c)
    return tuple((name, best[name][1]) for name in sorted(best))


# --- mutants of the expectation (the power of a case, on the CPU) --------------------------------

def f32_bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def round_rne(v):
    """bf16 bits of fp32 values, round to nearest even (finite inputs)."""
    u = f32_bits(v).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_trunc(v):
    return (f32_bits(v) >> 16).astype(np.uint16)


def round_half_away(v):
    u = f32_bits(v).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


def rounding_profile(v):
    """Shares of fp32 values that are not bf16-representable, that are exact ties, and of the
    ties that round up / down (in magnitude) to even."""
    u = f32_bits(v)
    low = u & 0xffff
    tie = low == 0x8000
    odd = ((u >> 16) & 1) == 1
    n = float(u.size)
    return {"inexact": float((low != 0).sum()) / n, "ties": float(tie.sum()) / n,
            "ties_up": int((tie & odd).sum()), "ties_down": int((tie & ~odd).sum())}


# --- overflow at the output rounding -------------------------------------------------------------

OVERFLOW_E = 118


def overflow_operands(M, N, K, seed=99):
    """Non-negative integers (x in [0, 3], w in [0, 11]) with W scaled by 2^118: every term is
    non-negative, so a partial sum never exceeds the final one in any order, and a final sum
    S 2^118 is finite in fp32 for S < 1024 and +inf from 1024 on whatever the order.  bf16's
    largest finite value is 1020 * 2^118: S = 1022 (a tie, to even) and 1023 round to +inf.
    At K = 128 the sums centre on 1056 with a spread of about 100: both outcomes are common."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    xi = torch.randint(0, 4, (M, K), generator=g, dtype=torch.int64)
    wi = torch.randint(0, 12, (N, K), generator=g, dtype=torch.int64)
    return xi, wi
