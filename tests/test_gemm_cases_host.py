"""The exact GEMM cases (tests/gemm_ref.py) on the CPU: these tests check the CASES that
tests/test_gemm_exact_gpu.py runs, and the restated dispatch, not the kernels.

Exactness: every sum stays below 2^24 (fp32-exact in any order), the fp64 prefix sums the
expectations are taken from equal the int64 product, and so does torch's fp32 product.
Power: every (operand set, K) has >= 25 % outputs that are not bf16-representable before
rounding, >= 3 % exact ties, and ties that round up and ties that round down to even, so
the output rounding mode decides bits in every case.  Mutants of the expectation
(truncation, round-half-away, last K step dropped, a K step used twice in place of the
next, one 8-element chunk dropped, split bases swapped, one wave's slice missing from the
thin fold) each change >= 1 % of the rounded outputs; the row mutant (row M - 1 in place
of row M - 2) can only touch one row, so it must change >= 50 % of THAT row.
Coverage: the restated dispatch, applied to the case list, reaches every template
instantiation gemm.hip can launch, the ws / ws2 ones at nk 1, 2, 3, 4, 5 and 7, the thin
ones at per-wave slice lengths 0, 1, RING - 1, RING, RING + 1 and >= 2 RING.  The
restatement is pinned against the library's own cs_gemm_splits (a pure host function: the
split of gemm_plan, which depends on kGemmVariants, resolve_variant, ws_mw and ws2_rows)."""
import importlib
import re

import numpy as np
import pytest
import torch

import gemm_ref as R

CASES = R.cases()


def _sets():
    """operand set (M, N, steps, seed) -> the cases that share it"""
    out = {}
    for c in CASES:
        out.setdefault((c.M, c.N, c.steps, c.seed), []).append(c)
    return out


SETS = _sets()
SET_IDS = [f"M{k[0]}-N{k[1]}-steps{k[2]}" for k in SETS]


def _totals(cs):
    """K / 64 of every launch of these cases"""
    return sorted({nk * max(s, 1) for c in cs for nk, s in c.shapes()})


def _changed(a, b):
    return float((R.round_rne(a) != R.round_rne(b)).mean())


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
def test_operands_are_exact_in_fp32_and_the_prefix_sums_are_the_int64_product(key):
    M, N, steps, seed = key
    assert 225 * R.BK * steps < 2 ** 24
    xi, wi = R.operands(*key)
    assert int(xi.abs().max()) <= R.AMAX and int(wi.abs().max()) <= R.AMAX
    assert torch.equal(xi.to(torch.bfloat16).long(), xi) and torch.equal(wi.to(torch.bfloat16).long(), wi)
    C = R.prefix_products(*key)
    x32, w32 = xi.float(), wi.float()
    xn, wn = xi.numpy(), wi.numpy()
    acc = np.zeros((M, N), dtype=np.int64)
    totals = set(_totals(SETS[key]))
    for t in range(steps):
        acc += xn[:, t * R.BK:(t + 1) * R.BK] @ wn[:, t * R.BK:(t + 1) * R.BK].T
        assert np.array_equal(C[t + 1].numpy(), acc.astype(np.float64)), t
        if t + 1 in totals:
            K = (t + 1) * R.BK
            assert np.array_equal((x32[:, :K] @ w32[:, :K].t()).numpy().astype(np.int64), acc), K
    for c in SETS[key]:
        # the scaled operands and every scaled sum are exact too: a power of two, in range
        assert torch.equal(c.w_bf16().double(), wi.double() * 2.0 ** c.e)
        assert 2.0 ** -100 < 2.0 ** c.e and 225 * R.BK * steps * 2.0 ** c.e < 2.0 ** 100


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
def test_every_case_exercises_the_rounding_mode_and_catches_the_mutants(key):
    M, N, steps, seed = key
    cs = SETS[key]
    xi, wi = R.operands(*key)
    C = R.prefix_products(*key).numpy()
    for n in _totals(cs):
        ref = C[n]
        p = R.rounding_profile(ref)
        assert p["inexact"] >= 0.25 and p["ties"] >= 0.03, (n, p)
        assert p["ties_up"] > 0 and p["ties_down"] > 0, (n, p)
        want = R.round_rne(ref)
        # torch's conversion is the RNE the mutants are measured against
        assert np.array_equal(want, R.to_bf16(torch.from_numpy(ref)).view(torch.int16).numpy().view(np.uint16))
        assert float((R.round_trunc(ref) != want).mean()) >= 0.01, n
        assert float((R.round_half_away(ref) != want).mean()) >= 0.01, n
        assert _changed(C[n - 1], ref) >= 0.01, ("last K step dropped", n)
        if n >= 2:      # step n - 2 used twice in place of step n - 1
            assert _changed(C[n - 1] + (C[n - 1] - C[n - 2]), ref) >= 0.01, ("K step doubled", n)
        k0 = (n - 1) * R.BK + 8 * (n * 3 % 8)       # one 8-element chunk of the last step
        chunk = (xi[:, k0:k0 + 8].double() @ wi[:, k0:k0 + 8].double().t()).numpy()
        assert _changed(ref - chunk, ref) >= 0.01, ("chunk dropped", n)
        if M >= 2:
            assert float((want[M - 1] != want[M - 2]).mean()) >= 0.5, ("row M - 1 for M - 2", n)
    for nk, s in sorted({sh for c in cs for sh in c.shapes() if sh[1] >= 2}):
        a, b = C[nk] - C[0], C[2 * nk] - C[nk]
        assert float((a != b).mean()) >= 0.01, ("split bases swapped", nk, s)
    for waves in sorted({l["waves"] for c in cs if c.family == "thin" for l in R.case_launches(c)}):
        for n in R.THIN_NSTEPS:
            for w in range(waves):
                s0, s1 = w * n // waves, (w + 1) * n // waves
                if s1 > s0:
                    assert _changed(C[n] - (C[s1] - C[s0]), C[n]) >= 0.01, ("wave dropped", waves, n, w)


def test_the_cases_reach_every_instantiation():
    reached = {}
    for c in CASES:
        for l in R.case_launches(c):
            reached.setdefault(l["name"], []).append(l)
    want = R.all_instantiations()
    assert len(want) == len(set(want)) == 104
    missing = [n for n in want if n not in reached]
    assert not missing, f"instantiations no case launches: {missing}"
    assert set(reached) == set(want), sorted(set(reached) - set(want))
    weak = []
    for name, ls in reached.items():
        if name.startswith("thin"):
            ring = ls[0]["ring"]
            lens = {v for l in ls for v in l["slices"]}
            need = {0, 1, ring - 1, ring, ring + 1}
            if not need <= lens or max(lens) < 2 * ring:
                weak.append((name, sorted(need - lens), max(lens)))
        elif not set(R.NK) <= {l["nk"] for l in ls}:
            weak.append((name, sorted(set(R.NK) - {l["nk"] for l in ls})))
    assert not weak, f"instantiations not reached at every pipeline length: {weak}"
    # plain ws / ws2 instantiations also run split (partials + fold), the library's own
    # choice of a split included, and a grid padded to whole groups of 8 cells
    for name in R.all_instantiations():
        if not name.startswith("thin") and re.fullmatch(r"ws<\d+,0>|ws2<\d+,\d,0,8,[01]>", name):
            assert {1, 2, 3} <= {l["splits"] for l in reached[name]}, name
    assert any(l.get("mblocks", 1) > 1 and l["cells"] % 8 and l["grid"] > l["cells"] * l["mblocks"]
               for ls in reached.values() for l in ls)


def test_zero_splits_reaches_a_library_chosen_split():
    got = {R.launch(2, 33, 512, 64 * n, splits=0)["splits"] for n in R.ZERO_STEPS}
    assert got == {1, 2}


def test_guard_cases_cover_every_instantiation_with_a_ragged_tile():
    g = R.guard_cases()
    assert [n for n, _ in g] == sorted(R.all_instantiations())
    for name, c in g:
        assert R.instantiation_of(c) == name and c.M % 16 != 0, (name, c)


@pytest.mark.parametrize("N", [128, 256, 384, 1792])
def test_restated_dispatch_matches_cs_gemm_splits(pkg, N):
    """cs_gemm_splits = f(gemm_plan) = f(kGemmVariants, resolve_variant, ws_mw, ws2_rows): with K
    so large that only the tile count bounds the split, every row count's tile count shows.
    N = 384 takes the N % 256 fallback; 1792 = 8 x 224 is the 7-wave form's N."""
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    K = 1 << 20
    rows = {}
    for variant in range(8):
        for M in range(1, 601):
            want = int(L.cs_gemm_splits(M, N, K, 0, variant))
            assert R.gemm_splits(M, N, K, 0, variant) == want, (variant, M)
            rows.setdefault(variant, []).append(want)
    # it discriminates: the split drops where a variant takes a second or third row block
    # (289 rows; variant 4: 145 and 433), and where N % 256 == 0 the 128- and 256-column
    # variants differ; the thin variants never split
    assert all(len(set(rows[v])) >= 2 for v in range(5)) and all(set(rows[v]) == {1} for v in (5, 6, 7))
    assert len({tuple(rows[v]) for v in range(5)}) >= (3 if N % 256 == 0 else 1)
    if N % 256:
        assert rows[0] == rows[2] == rows[4] == rows[3]
    for K in (64, 512, 1024, 1280, 1344, 2048, 14336):
        for variant in (0, 1, 3, 5, 7):
            for gated in (0, 1):
                for M in (1, 33, 289):
                    assert R.gemm_splits(M, N, K, gated, variant) == \
                        int(L.cs_gemm_splits(M, N, K, gated, variant)), (M, K, gated, variant)
    assert R.gemm_splits(4, 100, 64, 0, 0) == int(L.cs_gemm_splits(4, 100, 64, 0, 0)) == 0
    assert R.gemm_splits(4, N, 1 << 20, 0, 8) == int(L.cs_gemm_splits(4, N, 1 << 20, 0, 8)) == 1


def test_restated_row_blocks():
    assert [R.ws_mw(M) for M in (1, 32, 33, 64, 257, 288, 289, 600)] == [1, 1, 2, 2, 9, 9, 9, 9]
    assert R.ws2_rows(72) == (8, 1) and R.ws2_rows(72, packed=True) == (5, 1)
    assert R.ws2_rows(289) == (12, 2) and R.ws2_rows(289, 9) == (8, 3) and R.ws2_rows(577) == (17, 3)
    assert R.ws2_grid(6, 2) == 16 and R.ws2_grid(6, 1) == 6
    assert R.resolve_variant(0, 384, 0) == 3 and R.resolve_variant(4, 384, 1) == 1
    assert R.launch(2, 72, 1792, 128, True, True)["name"] == "ws2<5,2,1,7,1>"
    assert R.launch(7, 49, 512, 128, True)["name"] == "thin<4,2,1,8,3>"
    assert R.launch(7, 48, 512, 128, True)["name"] == "thin<3,2,1,16,2>"


@pytest.mark.parametrize("M,K", [(80, 192), (80, 448), (289, 192), (289, 448)])
def test_selector_rows_visit_every_k_and_decode(M, K):
    hit = torch.cat([R.selector_k(M, K, s) for s in R.selector_shifts(M, K)])
    assert set(hit.tolist()) == set(range(K))
    wi = R.selector_w(256, K)
    assert int(wi.abs().max()) <= 125 and torch.equal(wi.to(torch.bfloat16).long(), wi)
    s = R.selector_shifts(M, K)[-1]
    want = R.selector_expected(wi, M, K, s)
    assert torch.equal(want.double(), R.selector_x(M, K, s).double() @ wi.double().t())
    got = want.clone()
    m, n = 3, 7
    k = int(R.selector_k(M, K, s)[m])
    got[m, n] = wi[n, (k + 8) % K]                  # the neighbouring 8-chunk delivered
    msg = R.selector_decode(wi, got.double(), want.double(), M, K, s)
    assert "1 of" in msg and f"{(k + 8) % K}" in msg


def test_overflow_operands_reach_both_sides_of_the_bf16_maximum():
    xi, wi = R.overflow_operands(33, 512, 128)
    S = xi.double() @ wi.double().t()
    assert int((xi < 0).sum()) == 0 and int((wi < 0).sum()) == 0
    y = R.to_bf16(S, R.OVERFLOW_E)
    assert torch.equal(torch.isinf(y), S >= 1022)
    assert int(torch.isinf(y).sum()) > 100 and int(torch.isfinite(y).sum()) > 100
    # fp32 holds every sum below 1024 exactly and overflows from 1024 on
    f = (S * 2.0 ** R.OVERFLOW_E).float()
    assert torch.equal(torch.isinf(f), S >= 1024)
    assert torch.equal(R.to_bf16(wi.double(), R.OVERFLOW_E).double(), wi.double() * 2.0 ** R.OVERFLOW_E)
