"""CPU tests: the C oracle is pinned to golden vectors produced by the reference
itself (tests/golden/core_golden.npz via make_golden.py) and to the reference's
published evaluation CSVs (tests/golden/eval_welfare_published.csv)."""
import os

import numpy as np
import pandas as pd
import pytest


@pytest.fixture(scope="module")
def core_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "core_golden.npz"))


@pytest.mark.parametrize("name", ["ls_small", "ls_wide", "ls_big"])
def test_oracle_log_softmax_rows_matches_reference(orc, core_golden, name):
    M = core_golden[f"{name}_in"]
    ref = core_golden[f"{name}_out"]
    n, B = M.shape
    tgt = np.tile(np.arange(B, dtype=np.int32), (n, 1))
    # oracle reads f32; compare the f32-rounded input through the fp64 numpy formula too
    tok, lse = orc.logsoftmax_gather(M.astype(np.float32), tgt)
    np.testing.assert_allclose(tok, ref, atol=1e-5)
    np.testing.assert_allclose(tok, orc.log_softmax_rows_np(M.astype(np.float32)), atol=1e-12)


def _utilities_via_oracle(orc, v, w, rho):
    """core.compute_utilities restated as rows -> oracle log-softmax/gather -> segment sums."""
    L, B, d = v.shape
    n = w.shape[0]
    import itertools
    leaves = np.array(list(itertools.product(range(B), repeat=L)))
    m = len(leaves)
    chosen = v[np.arange(L)[None, :], leaves]            # [m, L, d]
    z = np.cumsum(chosen, axis=1) - chosen
    X = z[:, :, None, :] + v[None]                       # [m, L, B, d]
    logits = rho * np.einsum("id,mtbd->imtb", w, X)      # [n, m, L, B]
    rows = np.ascontiguousarray(logits.reshape(-1, B), dtype=np.float32)
    tgt = np.broadcast_to(leaves[None], (n, m, L)).reshape(-1, 1).astype(np.int32)
    tok, _ = orc.logsoftmax_gather(rows, tgt)
    seg = orc.segment_reduce(tok, np.arange(0, n * m * L + 1, L))
    logu = seg["sum_lp"].reshape(n, m)
    return np.exp(logu - logu.max(axis=1, keepdims=True)) + 1e-300


def test_oracle_compute_utilities_matches_reference(orc, core_golden):
    for s in core_golden["seeds"]:
        v, w = core_golden[f"v_{s}"], core_golden[f"w_{s}"]
        for ri, rho in zip((0, 9, 19), core_golden["rho"]):
            U = _utilities_via_oracle(orc, v, w, rho)
            np.testing.assert_allclose(U, core_golden[f"U_{s}_{ri}"], rtol=1e-5, atol=1e-12)


def test_oracle_point_mass_welfare_and_selection(orc, core_golden):
    for s in core_golden["seeds"]:
        for ri in (0, 9, 19):
            U = core_golden[f"U_{s}_{ri}"]
            F = orc.welfare(U, orc.SUMLOG, eps=1e-320)
            np.testing.assert_allclose(F, core_golden[f"Fpoint_{s}_{ri}"], rtol=1e-12)
            assert orc.topk(orc.welfare(U, orc.SUM), 1)[0, 0] == core_golden[f"jutil_{s}_{ri}"]
            assert orc.topk(orc.welfare(U, orc.MIN), 1)[0, 0] == core_golden[f"jegal_{s}_{ri}"]
            assert orc.topk(F, 1)[0, 0] == core_golden[f"jnash_{s}_{ri}"]


def test_oracle_perplexity_welfare_matches_published_results(orc, golden_dir):
    """src/evaluation.py:367-381 identities on all 749 published rows."""
    df = pd.read_csv(os.path.join(golden_dir, "eval_welfare_published.csv"))
    assert len(df) == 749
    for n_agents, g in df.groupby("n_agents"):
        lp = g[[f"avg_logprob_{j}" for j in range(n_agents)]].to_numpy().T   # [A, rows]
        ppl = np.exp(-lp)
        np.testing.assert_allclose(ppl, g[[f"perplexity_{j}" for j in range(n_agents)]].to_numpy().T,
                                   rtol=1e-12)
        np.testing.assert_allclose(orc.welfare(ppl, orc.MAX),
                                   g["egalitarian_welfare_perplexity"], rtol=1e-12)
        np.testing.assert_allclose(orc.welfare(ppl, orc.SUM),
                                   g["utilitarian_welfare_perplexity"], rtol=1e-12)
        inv = 1.0 / np.maximum(ppl, 1e-9)
        np.testing.assert_allclose(orc.welfare(inv, orc.SUMLOG, eps=1e-300),
                                   g["log_nash_welfare_perplexity"], rtol=1e-10, atol=1e-12)


def test_oracle_topk_is_python_stable_sort(orc):
    rng = np.random.default_rng(3)
    for _ in range(20):
        W = rng.integers(-3, 3, size=37).astype(np.float64)   # many ties
        W[rng.integers(0, 37, size=3)] = np.nan
        idx = orc.topk(W, 37)[0]
        finite = [i for i in range(37) if not np.isnan(W[i])]
        expect = sorted(finite, key=lambda i: W[i], reverse=True)
        expect += [i for i in range(37) if np.isnan(W[i])]
        assert list(idx) == expect


def test_oracle_segment_reduce_skips_none(orc):
    lp = np.array([-1.0, np.nan, -2.0, -0.5, np.nan], dtype=np.float64)
    out = orc.segment_reduce(lp, np.array([0, 3, 3, 5]))
    np.testing.assert_allclose(out["sum_lp"], [-3.0, 0.0, -0.5])
    assert list(out["count"]) == [2, 0, 1]
    np.testing.assert_allclose(out["sum_p"], [np.exp(-1) + np.exp(-2), 0.0, np.exp(-0.5)])
    assert out["last"][0] == -2.0 and np.isnan(out["last"][1]) and np.isnan(out["last"][2])


def test_oracle_welfare_nonfinite_modes(orc):
    U = np.array([[1.0, np.nan, -np.inf], [2.0, 3.0, np.inf]])
    np.testing.assert_allclose(orc.welfare(U, orc.MIN), [1.0, 3.0, np.nan])  # all-non-finite column -> NaN
    W = orc.welfare(U, orc.MIN, nonfinite=1, nan_val=-10, posinf_val=20, neginf_val=-20)
    np.testing.assert_allclose(W, [1.0, -10.0, -20.0])


def test_oracle_bf16_and_f16_decoding(orc):
    rng = np.random.default_rng(5)
    x = (rng.normal(size=(3, 300)) * 4).astype(np.float32)
    tgt = rng.integers(0, 300, size=(3, 2)).astype(np.int32)
    bits = orc.bf16_bits(x)
    tok_b, _ = orc.logsoftmax_gather(bits, tgt, bf16=True)
    tok_ref, _ = orc.logsoftmax_gather(orc.bf16_to_f32(bits), tgt)
    np.testing.assert_allclose(tok_b, tok_ref, atol=1e-12)
    tok_h, _ = orc.logsoftmax_gather(x.astype(np.float16), tgt)
    tok_h_ref, _ = orc.logsoftmax_gather(x.astype(np.float16).astype(np.float32), tgt)
    np.testing.assert_allclose(tok_h, tok_h_ref, atol=1e-12)


def test_oracle_softcap_and_out_of_range(orc):
    rng = np.random.default_rng(6)
    x = (rng.normal(size=(2, 50)) * 40).astype(np.float32)
    tgt = np.array([[3, -1], [50, 7]], dtype=np.int32)
    tok, _ = orc.logsoftmax_gather(x, tgt, softcap=30.0)
    capped = 30.0 * np.tanh(x.astype(np.float64) / 30.0)
    ref = orc.log_softmax_rows_np(capped)
    assert abs(tok[0, 0] - ref[0, 3]) < 1e-12 and abs(tok[1, 1] - ref[1, 7]) < 1e-12
    assert np.isnan(tok[0, 1]) and np.isnan(tok[1, 0])


def test_oracle_uniform_is_strictly_inside_unit_interval(orc):
    u = orc.cs_uniform(123456789, np.arange(1 << 20))
    assert u.dtype == np.float32 and u.min() > 0 and u.max() < 1
    assert abs(float(u.mean()) - 0.5) < 2e-3
    assert np.array_equal(u, orc.cs_uniform(123456789, np.arange(1 << 20)))
    assert not np.array_equal(u[:100], orc.cs_uniform(123456790, np.arange(100)))


# --- the seeded Gumbel-max sampler's oracle (the contract of cs_vocab_sample) -----------------
def _gumbel_manual(x, seed, T, cap):
    x = np.asarray(x, dtype=np.float64)
    y = (cap * np.tanh(x / cap) if cap else x) / T
    u = np.asarray(__import__("oracle").cs_uniform(seed, np.arange(x.size)), dtype=np.float64)
    return y, y - np.log(-np.log(u))


def test_oracle_gumbel_softcap_is_applied_before_the_temperature(orc):
    rng = np.random.default_rng(21)
    x = (rng.normal(size=500) * 40).astype(np.float32)
    for seed in (3, 2 ** 63 + 11, -5):
        i, lp, s = orc.gumbel_sample(x, seed, 0.5, 30.0, scores=True)
        y, s_ref = _gumbel_manual(x, seed, 0.5, 30.0)
        np.testing.assert_array_equal(s, s_ref)
        assert i == int(np.argmax(s_ref))
        assert abs(lp - orc.log_softmax_rows_np(y[None])[0, i]) < 1e-12
        # cap(x) / T, not cap(x / T): the two orders disagree on this row
        wrong = 30.0 * np.tanh(x.astype(np.float64) / 0.5 / 30.0)
        assert np.max(np.abs(wrong - y)) > 1.0
    assert orc.gumbel_sample(x, 7, 0.7) == orc.gumbel_sample(x, 7, 0.7, 0.0)


def test_oracle_gumbel_scores_and_candidate_margin(orc):
    rng = np.random.default_rng(22)
    x = rng.normal(size=300).astype(np.float32)
    i, lp, s = orc.gumbel_sample(x, 99, 2.5, scores=True)
    assert s.shape == (300,) and s.dtype == np.float64 and i == int(np.argmax(s))
    for c in (0, 17, 299, i):
        i2, lp2, m = orc.gumbel_sample(x, 99, 2.5, candidate=c)
        assert (i2, lp2) == (i, lp) and m == s[i] - s[c] and m >= 0.0
    assert orc.gumbel_sample(x, 99, 2.5, candidate=i)[2] == 0.0
    assert np.isnan(orc.gumbel_sample(x, 99, 2.5, candidate=300)[2])
    assert np.isnan(orc.gumbel_sample(x, 99, 2.5, candidate=-1)[2])


def test_oracle_gumbel_masked_nan_and_no_candidate_rows(orc):
    rng = np.random.default_rng(23)
    x = (rng.normal(size=400) * 3).astype(np.float32)
    masked = x.copy()
    masked[100:] = -np.inf
    nan3 = x.copy()
    nan3[::3] = np.nan
    single = np.full(400, -np.inf, dtype=np.float32)
    single[222] = -7.5
    for seed in range(40):
        i, lp, s = orc.gumbel_sample(masked, seed, scores=True)
        assert 0 <= i < 100 and np.isfinite(lp) and np.all(s[100:] == -np.inf)
        ref = orc.log_softmax_rows_np(x[None, :100].astype(np.float64))[0, i]
        assert abs(lp - ref) < 1e-12
        i, lp = orc.gumbel_sample(nan3, seed)
        assert i % 3 != 0 and np.isnan(lp)                  # never a NaN token; NaN poisons lp
        assert orc.gumbel_sample(single, seed) == (222, 0.0)
        # a masked candidate has no margin
        assert np.isnan(orc.gumbel_sample(masked, seed, candidate=250)[2])
    for dead in (np.full(50, -np.inf, dtype=np.float32), np.full(50, np.nan, dtype=np.float32),
                 np.array([np.nan, -np.inf] * 25, dtype=np.float32)):
        i, lp, s, m = orc.gumbel_sample(dead, 5, 0.7, scores=True, candidate=3)
        assert i == -1 and np.isnan(lp) and np.all(s == -np.inf) and np.isnan(m)
    # selectability is judged on x': a soft-cap maps -inf to -cap (tanh(-inf) = -1), a token
    # like any other, and leaves NaN a NaN
    i, lp = orc.gumbel_sample(np.full(50, -np.inf, dtype=np.float32), 5, 0.7, 30.0)
    assert 0 <= i < 50 and abs(lp + np.log(50.0)) < 1e-12
    assert orc.gumbel_sample(np.full(50, np.nan, dtype=np.float32), 5, 0.7, 30.0)[0] == -1
    # one NaN anywhere (first, last) poisons the log-prob but not the selection
    for at in (0, 399):
        one = x.copy()
        one[at] = np.nan
        i, lp = orc.gumbel_sample(one, 4)
        assert i != at and np.isnan(lp)


def _tie_rows(orc, rows=64, n_draw=16, vocab=256000):
    seeds = (np.arange(rows * n_draw, dtype=np.int64) * 2654435761 + 12345).reshape(rows, n_draw)
    x = np.full((rows, vocab), 1.25, dtype=np.float32)
    return x, seeds, orc.gumbel_sample_rows(x, seeds)


def test_oracle_gumbel_exact_ties_go_to_the_lowest_id_and_the_rule_is_observable(orc):
    """Constant rows at vocab 256,000: the 23-bit uniform repeats at the top in ~3 % of the
    draws.  The oracle returns the lowest tied id; an oracle variant in which the highest id
    wins disagrees on every tied draw, so a comparison on these rows is not vacuous."""
    x, seeds, o = _tie_rows(orc)
    tied = np.argwhere(o["ties"] > 1)
    assert len(tied) >= 10
    assert np.all(o["gap"][o["ties"] > 1] == 0.0) and np.all(o["gap"][o["ties"] == 1] > 0.0)
    differ = 0
    for r, d in tied:
        i, _, s = orc.gumbel_sample(x[r], int(seeds[r, d]), scores=True)
        assert i == o["id"][r, d]
        top = np.flatnonzero(s == s.max())
        assert len(top) == o["ties"][r, d] and i == top[0]
        highest_wins = x.shape[1] - 1 - int(np.argmax(s[::-1]))      # the broken variant
        assert highest_wins == top[-1]
        differ += int(highest_wins != i)
        # the variant's pick has margin exactly 0: the comparison rule never excuses it
        assert orc.gumbel_sample(x[r], int(seeds[r, d]), candidate=highest_wins)[2] == 0.0
    assert differ == len(tied)


def test_oracle_gumbel_c_layer_matches_numpy(orc):
    rng = np.random.default_rng(24)
    seeds = np.array([[0, -1, -2 ** 63, 2 ** 63 - 1, 77, 77]], dtype=np.int64).repeat(5, 0)
    seeds[1:] += np.arange(1, 5, dtype=np.int64)[:, None] * 1000003 * np.array([0, 0, 1, -1, 1, 1])
    for dtype, T, cap in (("f32", 1.0, 0.0), ("bf16", 0.3, 30.0), ("f16", 2.5, 0.0),
                          ("f32", 0.7, 50.0)):
        x = (rng.normal(size=(5, 1037)) * 4).astype(np.float32)
        x = np.round(x * 2) / 2 if dtype == "f16" else x        # heavy value ties
        x[1, 100:] = -np.inf
        x[2, ::3] = np.nan
        x[3, :] = -np.inf
        x[4, :] = np.nan
        if dtype == "bf16":
            host = orc.bf16_bits(x)
            xf = orc.bf16_to_f32(host)
        elif dtype == "f16":
            host = x.astype(np.float16)
            xf = host.astype(np.float32)
        else:
            host = xf = x
        wide = np.zeros((5, 1040), dtype=host.dtype)            # ld > vocab
        wide[:, :1037] = host
        cand = rng.integers(0, 1037, size=seeds.shape).astype(np.int32)
        o = orc.gumbel_sample_rows(wide, seeds, T, cap, bf16=dtype == "bf16", vocab=1037,
                                   candidates=cand)
        for r in range(5):
            for d in range(seeds.shape[1]):
                i, lp, s, m = orc.gumbel_sample(xf[r], int(seeds[r, d]), T, cap, scores=True,
                                                candidate=int(cand[r, d]))
                assert o["id"][r, d] == i
                np.testing.assert_allclose(o["lp"][r, d], lp, atol=1e-12, equal_nan=True)
                np.testing.assert_allclose(o["margin"][r, d], m, atol=1e-12, equal_nan=True)
                if i >= 0:
                    top2 = np.sort(s)[-2:]
                    np.testing.assert_allclose(o["gap"][r, d], top2[1] - top2[0], atol=1e-12)
                    assert o["ties"][r, d] == int((s == s.max()).sum())
                else:
                    assert o["ties"][r, d] == 0 and np.isnan(o["gap"][r, d])
        assert np.array_equal(o["id"][:, 4], o["id"][:, 5])     # a duplicated seed
        assert np.all(o["scale"] >= 1.0)
