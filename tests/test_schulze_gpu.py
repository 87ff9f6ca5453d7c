"""GPU tests of Schulze rank aggregation (cs_schulze) through ops.schulze, the drop-ins of
methods/habermas_machine.py and Best-of-N's ``selection: "schulze"``.

Expected values: what the reference's own functions returned (tests/golden/schulze_golden.npz)
and the NumPy restatement tests/schulze_ref.py, which tests/test_schulze_host.py pins to those
recordings.  The aggregation is integer arithmetic: every comparison is exact, no tolerance
anywhere.

The kernel stages the voters 32 at a time (kSchTile) and runs one wave per election up to 16
candidates, four above (kSchNarrowC); the shape tests sit on those boundaries."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import schulze_ref as sr

pytestmark = pytest.mark.gpu

T = sr.TILE
KEYS = ("defeats", "strengths", "ranking", "untied")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "schulze_golden.npz"))


@pytest.fixture(scope="module")
def hm(pkg, dev):
    return import_module(pkg.__name__ + ".methods.habermas_machine")


def run(ops, dev, x, kind="rankings", valid=None, ballot=None):
    """ops.schulze on host arrays [E, ...]; host arrays back."""
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt),  # noqa: E731
                                                                device=dev)
    res = ops.schulze(t(x, np.float32 if kind == "scores" else np.int32), kind=kind,
                      valid=t(valid, np.uint8), ballot=t(ballot, np.int32))
    assert all(v.dtype == torch.int32 and v.is_cuda for v in res.values())
    return {k: v.cpu().numpy() for k, v in res.items()}


def check(got, e, want, where):
    """Election e of a launch against one restatement result: every output present, exactly."""
    assert int(got["status"][e]) == want["status"], where
    assert int(got["winner"][e]) == want["winner"], where
    for k in KEYS:
        if want[k] is None:
            continue
        assert np.array_equal(got[k][e], want[k]), (where, k)


def elections(seed, E, R, C):
    """E elections of one shape: ranks drawn with ties and permutations alternate; ballots with
    repeated values on every third."""
    rng = np.random.default_rng(seed)
    xs = np.stack([sr.random_election(rng, R, C, "ties" if e % 2 == 0 else "perm") for e in range(E)])
    bs = np.stack([rng.permutation(C) // (2 if e % 3 == 0 else 1) - 1 for e in range(E)])
    return xs, bs.astype(np.int32)


# 1 ---------------------------------------------------------------------------------------
def test_every_golden_case(ops, dev, golden):
    cases = []   # (name, rankings, ballot or None, expected by key)
    for i in range(int(golden["known"])):
        cases.append((f"k{i}", golden[f"k{i}_rankings"], None,
                      {k: golden[f"k{i}_{k}"] for k in ("defeats", "strengths", "ranking")}))
    for i in range(int(golden["fig1"])):
        cases.append((f"f{i}", golden[f"f{i}_rankings"], None, {"ranking": golden[f"f{i}_ranking"]}))
    for i in range(int(golden["tiebreak"])):
        x = golden[f"t{i}_rankings"]
        ballot = np.random.default_rng(int(golden[f"t{i}_seed"])).permutation(x.shape[1])
        cases.append((f"t{i}", x, ballot, {"untied": golden[f"t{i}_untied"]}))
    for i in range(int(golden["random"])):
        cases.append((f"r{i}", golden[f"r{i}_rankings"], golden[f"r{i}_ballot"],
                      {k: golden[f"r{i}_{k}"] for k in KEYS}))
    by_shape = {}
    for c in cases:
        by_shape.setdefault(c[1].shape, []).append(c)
    seen = 0
    for (R, C), group in by_shape.items():
        x = np.stack([c[1] for c in group])
        ballots = np.stack([np.arange(C) if c[2] is None else c[2] for c in group])
        got = run(ops, dev, x, ballot=ballots)            # one launch per shape
        assert (got["status"] == 0).all(), (R, C)
        for e, (name, _, ballot, want) in enumerate(group):
            for k, v in want.items():
                assert np.array_equal(got[k][e], v), (name, k)
            final = got["untied"][e]
            assert np.array_equal(final, sr.untie(got["ranking"][e], ballots[e])), name
            assert int(got["winner"][e]) == int(np.where(final == 0)[0][0]), name
            seen += 1
        # stage by stage, as the reference's own test runs them: each stage from recorded input
        with_d = [(e, c) for e, c in enumerate(group) if "strengths" in c[3]]
        if with_d:
            d = np.stack([c[3]["defeats"] for _, c in with_d])
            p = np.stack([c[3]["strengths"] for _, c in with_d])
            g2 = run(ops, dev, d, "defeats")
            g3 = run(ops, dev, p, "strengths")
            assert "defeats" not in g2 and "defeats" not in g3 and "strengths" not in g3
            for n, (e, c) in enumerate(with_d):
                assert np.array_equal(g2["strengths"][n], c[3]["strengths"]), c[0]
                assert np.array_equal(g2["ranking"][n], c[3]["ranking"]), c[0]
                assert np.array_equal(g3["ranking"][n], c[3]["ranking"]), c[0]
                assert g2["winner"][n] == g3["winner"][n] == int(np.where(c[3]["ranking"] == 0)[0][0])
    assert seen == 5 + 2 + 6 + 90


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128])
def test_shape_edges(ops, dev, C):
    for R in (1, 2, T - 1, T, T + 1, 3 * T + 1):
        xs, bs = elections(1000 * C + R, 3, R, C)
        got = run(ops, dev, xs, ballot=bs)
        for e in range(3):
            check(got, e, sr.solve(xs[e], ballot=bs[e]), (C, R, e))


def test_thirty_three_mixed_elections_in_one_launch(ops, dev):
    E, R, C = 33, T + 1, 17
    xs, bs = elections(33, E, R, C)
    rng = np.random.default_rng(34)
    valid = rng.random((E, R)) < 0.7
    valid[::4] = True
    valid[5] = False                       # no voter
    xs[9, R - 1, 3] = C                    # malformed, in the second tile
    valid[9, R - 1] = True
    xs[13, 0, 0] = -1                      # out of range but not counted: solved
    valid[13, 0] = False
    got = run(ops, dev, xs, valid=valid, ballot=bs)
    want = [sr.solve(xs[e], valid=valid[e], ballot=bs[e]) for e in range(E)]
    assert [w["status"] for w in want] == [-2 if e == 5 else -1 if e == 9 else 0 for e in range(E)]
    for e in range(E):
        check(got, e, want[e], e)


# 3 ---------------------------------------------------------------------------------------
def _chain(order):
    """One chain of wins order[0] -> order[1] -> ... with strictly decreasing margins; the
    expected strengths: the last (smallest) margin on the way forwards, 0 backwards."""
    C = len(order)
    margin = [2 * C - t for t in range(C - 1)]
    d = np.zeros((C, C), dtype=np.int32)
    p = np.zeros((C, C), dtype=np.int32)
    for t in range(C - 1):
        d[order[t], order[t + 1]] = margin[t]
    for s in range(C):
        for t in range(s + 1, C):
            p[order[s], order[t]] = margin[t - 1]
    return d, p


@pytest.mark.parametrize("C", [17, 128])
def test_planted_chains(ops, dev, C):
    orders = [np.arange(C), np.arange(C)[::-1], np.random.default_rng(C).permutation(C)]
    ds, ps = zip(*[_chain(o) for o in orders])
    got = run(ops, dev, np.stack(ds), "defeats")
    assert (got["status"] == 0).all()
    for n, o in enumerate(orders):
        assert np.array_equal(got["strengths"][n], ps[n]), n
        assert np.array_equal(ps[n], sr.strengths_fast(ds[n])), n     # the expectation itself
        # the chain's order is the social ranking, untied
        rank = np.empty(C, dtype=np.int64)
        rank[o] = np.arange(C)
        assert np.array_equal(got["ranking"][n], rank), n
        assert int(got["winner"][n]) == int(o[0])


@pytest.mark.parametrize("C", [5, 17, 128])
def test_defeat_matrices_of_any_integers(ops, dev, C):
    rng = np.random.default_rng(7 * C)
    neg = rng.integers(-9, 10, (3, C, C)).astype(np.int32)
    big = rng.integers(-2 ** 31, 2 ** 31, (1, C, C), dtype=np.int64).astype(np.int32)
    flat = np.full((1, C, C), 3, dtype=np.int32)          # all equal: nobody beats anybody
    ds = np.concatenate([neg, big, flat])
    for d in ds:
        np.fill_diagonal(d, 0)
    got = run(ops, dev, ds, "defeats")
    for n, d in enumerate(ds):
        check(got, n, sr.solve(d, "defeats"), (C, n))
        if C == 5:
            assert np.array_equal(got["strengths"][n], sr.strengths_loops(d)), n
    assert not got["strengths"][4].any() and not got["ranking"][4].any() and got["winner"][4] == 0


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(8, 16), (T + 3, 65)])
def test_scores_equal_rankings_of_their_dense_ranks(ops, dev, R, C):
    rng = np.random.default_rng(R * C)
    s = rng.integers(-3, 4, (4, R, C)).astype(np.float32) * 0.25       # many equal scores
    s[1] = rng.standard_normal((R, C)).astype(np.float32)              # none
    ballots = np.stack([rng.permutation(C) for _ in range(4)])
    ranks = np.stack([sr.dense_ranks_of_scores(e) for e in s])
    a = run(ops, dev, s, "scores", ballot=ballots)
    b = run(ops, dev, ranks, "rankings", ballot=ballots)
    assert (a["status"] == 0).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for e in range(4):
        check(a, e, sr.solve(s[e], "scores", ballot=ballots[e]), e)


def test_scores_special_values(ops, dev):
    nan, inf = np.nan, np.inf
    s = np.float32([
        [[nan, 1.0, -inf, inf], [-0.0, 0.0, 1.0, 1.0], [nan, nan, nan, nan]],
        [[inf, inf, -inf, -inf], [0.0, -0.0, 0.0, -0.0], [1e-45, 0.0, -1e-45, 3e38]],
        [[2.0, 2.0, 2.0, 2.0], [nan, 5.0, nan, 5.0], [-1.0, -1.0, nan, -2.0]],
    ])
    got = run(ops, dev, s, "scores", ballot=np.tile(np.arange(4), (3, 1)))
    for e in range(3):
        check(got, e, sr.solve(s[e], "scores", ballot=np.arange(4)), e)
    assert got["defeats"][0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [1, 2, 1, 0]]


# 5 ---------------------------------------------------------------------------------------
def test_valid_equals_the_election_without_those_rows(ops, dev):
    R, C = 2 * T + 5, 17
    xs, bs = elections(55, 4, R, C)
    rng = np.random.default_rng(56)
    valid = rng.random((4, R)) < 0.5
    valid[1] = False                                        # no voter at all
    valid[2, :T] = False                                    # a whole tile left out
    got = run(ops, dev, xs, valid=valid, ballot=bs)
    assert got["status"].tolist() == [0, -2, 0, 0]
    for k in KEYS:
        assert (got[k][1] == -1).all(), k
    assert got["winner"][1] == -1
    for e in (0, 2, 3):
        alone = run(ops, dev, xs[e][valid[e]][None], ballot=bs[e][None])
        for k in got:
            assert np.array_equal(got[k][e], alone[k][0]), (e, k)
        check(got, e, sr.solve(xs[e], valid=valid[e], ballot=bs[e]), e)
    # scores mode takes valid too
    s = np.random.default_rng(57).standard_normal((4, R, C)).astype(np.float32)
    gs = run(ops, dev, s, "scores", valid=valid, ballot=bs)
    for e in range(4):
        check(gs, e, sr.solve(s[e], "scores", valid=valid[e], ballot=bs[e]), ("scores", e))


# 6 ---------------------------------------------------------------------------------------
def test_malformed_elections_inside_a_batch(ops, dev):
    R, C = T + 2, 16
    xs, bs = elections(66, 5, R, C)
    xs[1, 3, 7] = C                                        # a rank of C
    xs[3, R - 1, 0] = -1                                   # a rank of -1, in the second tile
    got = run(ops, dev, xs, ballot=bs)
    assert got["status"].tolist() == [0, -1, 0, -1, 0]
    for e in (1, 3):
        assert all((got[k][e] == -1).all() for k in KEYS) and got["winner"][e] == -1
    for e in (0, 2, 4):
        alone = run(ops, dev, xs[e][None], ballot=bs[e][None])
        for k in got:
            assert np.array_equal(got[k][e], alone[k][0]), (e, k)
        check(got, e, sr.solve(xs[e], ballot=bs[e]), e)
    # a nonzero diagonal, kinds defeats and strengths
    d = np.stack([sr.defeats_fast(x) for x in xs[[0, 2, 4]]])
    d[1, 5, 5] = 2
    for kind in ("defeats", "strengths"):
        m = d if kind == "defeats" else np.stack([sr.strengths_fast(x) if n != 1 else d[1]
                                                  for n, x in enumerate(d)])
        gm = run(ops, dev, m, kind, ballot=bs[:3])
        assert gm["status"].tolist() == [0, -1, 0], kind
        for n in range(3):
            check(gm, n, sr.solve(m[n], kind, ballot=bs[n]), (kind, n))
        assert (gm["ranking"][1] == -1).all() and gm["winner"][1] == -1


# 7 ---------------------------------------------------------------------------------------
def test_drop_ins_follow_the_reference(hm, golden):
    for i in range(int(golden["known"])):
        g = lambda k: golden[f"k{i}_{k}"]                  # noqa: E731
        d = hm._schulze_compute_pairwise_defeats(g("rankings"))
        p = hm._schulze_compute_strongest_path_strengths(g("defeats"))
        t = hm._schulze_rank_candidates(g("strengths"))
        a = hm._schulze_aggregate_with_ties(g("rankings"))
        assert d.dtype == np.int32 and p.dtype == np.int32
        assert t.dtype == np.intp and a.dtype == np.intp
        assert np.array_equal(d, g("defeats")) and np.array_equal(p, g("strengths"))
        assert np.array_equal(t, g("ranking")) and np.array_equal(a, g("ranking"))
    for i in range(int(golden["fig1"])):
        got = hm._schulze_aggregate_with_ties(golden[f"f{i}_rankings"])
        assert np.array_equal(got, golden[f"f{i}_ranking"])
    # the six seeded tie-break cases
    for i in range(int(golden["tiebreak"])):
        x = golden[f"t{i}_rankings"]
        got = hm._aggregate_schulze({f"agent_{a}": r for a, r in enumerate(x)}, x.shape[1],
                                    seed=int(golden[f"t{i}_seed"]), tie_breaking_method="random")
        assert got is not None and got.dtype == np.intp
        assert np.array_equal(got, golden[f"t{i}_untied"]), i
        assert np.unique(got).size == got.size
    # ranks that only compare: the defeats are those of the rows' dense ranks
    odd = np.array([[10, -3, 10, 99], [5, 5, 5, 7]])
    assert np.array_equal(hm._schulze_compute_pairwise_defeats(odd), sr.defeats_fast(odd))


def test_aggregate_schulze_none_and_tie_cases(hm, golden):
    x = golden["k3_rankings"]                              # A = D > B > C
    tied, untied = golden["k3_ranking"], golden["t1_untied"]
    rankings = {"a": x[0], "gone": None, "b": x[1], "c": x[2], "lost": None, "d": x[3], "e": x[4]}
    assert np.array_equal(hm._aggregate_schulze(rankings, 4, seed=1), untied)
    assert np.array_equal(hm._aggregate_schulze(rankings, 4, seed=1,
                                                tie_breaking_method="ties_allowed"), tied)
    assert np.array_equal(hm._aggregate_schulze(rankings, 4, seed=1,
                                                tie_breaking_method="tbrc"), tied)   # unsupported
    assert hm._aggregate_schulze({"a": None, "b": None}, 4, seed=1) is None
    assert hm._aggregate_schulze(rankings, 5, seed=1) is None                        # shape mismatch
    bad = dict(rankings, a=np.array([0, 1, 4, 2]))
    assert hm._aggregate_schulze(bad, 4, seed=1) is None       # the check's ValueError -> None


@pytest.mark.parametrize("fn,arg", [
    ("_schulze_compute_strongest_path_strengths", np.int32([[0, 1, 1], [1, 1, 1], [1, 1, 0]])),
    ("_schulze_compute_strongest_path_strengths", np.int32([[0, 1, 1], [1, 0, 1]])),
    ("_schulze_rank_candidates", np.int32([[0, 1, 1], [1, 1, 1], [1, 1, 0]])),
    ("_schulze_rank_candidates", np.int32([[0, 1, 1], [1, 0, 1]])),
])
def test_the_references_four_value_errors(hm, fn, arg):
    with pytest.raises(ValueError):
        getattr(hm, fn)(arg)


def test_aggregate_with_ties_raises_on_a_bad_rank(hm):
    with pytest.raises(ValueError, match="Ranks must be between 0 and 3. Found invalid rank: 4"):
        hm._schulze_aggregate_with_ties(np.array([[0, 1, 2, 3], [0, 4, 2, 1]]))


def test_batch_rows_equal_the_single_calls(hm):
    E, R, C = 12, 5, 6
    xs, _ = elections(77, E, R, C)
    xs[4, 2, 1] = C                                        # the single call returns None
    valid = np.random.default_rng(78).random((E, R)) < 0.8
    valid[:, 0] = True
    valid[4, 2] = True                                     # the bad rank counts
    valid[7] = False                                       # no ranking left: None
    seeds = list(range(100, 100 + E))

    def single(e, seed, method):
        agents = {a: (xs[e, a] if valid[e, a] else None) for a in range(R)}
        return hm._aggregate_schulze(agents, C, seed=seed, tie_breaking_method=method)

    for method in ("random", "ties_allowed"):
        for sd in (seeds, 5):
            got = hm.aggregate_schulze_batch(xs, seeds=sd, tie_breaking_method=method, valid=valid)
            assert got.shape == (E, C) and got.dtype == np.intp
            for e in range(E):
                want = single(e, sd[e] if isinstance(sd, list) else sd, method)
                if e in (4, 7):
                    assert want is None and (got[e] == -1).all()
                else:
                    assert np.array_equal(got[e], want), (method, e)
    assert hm.aggregate_schulze_batch(xs[:0]).shape == (0, C)


# 8 ---------------------------------------------------------------------------------------
ISSUE = "How should the city spend its budget?"
OPINIONS = {"Agent 1": "We should fund public transit first.",
            "Agent 2": "Lower the city's taxes before anything else."}
# two agents and twelve candidates: the agents' orders of the fixture's candidates differ in a
# few pairs, which Schulze leaves tied (with six candidates they agree and nothing is tied)
BON_CFG = {"n": 12, "max_tokens": 12, "seed": 5}


@pytest.fixture(scope="module")
def bon_runs(pkg, dev):
    """Best-of-N on a seeded fixture engine with no selection key, "egalitarian" and "schulze"."""
    R = import_module(pkg.__name__ + ".runtime")
    methods = import_module(pkg.__name__ + ".methods")
    # no prefix reuse: a reused prefill rounds its bf16 differently from a fresh one, and the
    # three runs must draw and score the same candidates
    eng, tok = R.random_engine("tiny-llama", dev, dtype=torch.bfloat16, seed=3, reuse_caches=0)
    R.register_engine("test/schulze-bon", eng, tok)
    runs = {}
    try:
        for name, extra in (("none", {}), ("egalitarian", {"selection": "egalitarian"}),
                            ("schulze", {"selection": "schulze"})):
            gen = methods.get_method_generator("best_of_n", dict(BON_CFG, **extra), "test/schulze-bon")
            runs[name] = (gen.generate_statement(ISSUE, OPINIONS), gen)
        bad = methods.get_method_generator("best_of_n", dict(BON_CFG, selection="borda"),
                                           "test/schulze-bon")
        with pytest.raises(ValueError, match="selection"):
            bad.generate_statement(ISSUE, OPINIONS)
    finally:
        R.clear_engines()
    return runs


def test_best_of_n_schulze_selection(bon_runs):
    text, gen = bon_runs["schulze"]
    cands = gen.last_candidates
    U = np.array([gen.last_agent_rewards[a] for a in OPINIONS], dtype=np.float64)
    assert U.shape == (2, len(cands)) and len(cands) >= 2
    U = np.nan_to_num(U, nan=gen.DEFAULT_REWARD, posinf=gen.REWARD_CLIP_MAX,
                      neginf=gen.REWARD_CLIP_MIN).astype(np.float32)
    ballot = np.random.default_rng(BON_CFG["seed"]).permutation(len(cands)).astype(np.int32)
    want = sr.solve(U, "scores", ballot=ballot)
    # the condition that makes the ballot matter: the restatement's tied ranking has a tie
    assert len(set(want["ranking"].tolist())) < len(cands), want["ranking"]
    assert gen.last_social_ranking == want["untied"].tolist()
    assert text == cands[want["winner"]]
    assert np.array_equal(np.array(gen.last_welfare, dtype=np.float32), U.min(axis=0))


def test_best_of_n_default_selection_is_unchanged(bon_runs):
    (t0, g0), (t1, g1) = bon_runs["none"], bon_runs["egalitarian"]
    assert t0 == t1 and g0.last_candidates == g1.last_candidates
    assert g0.last_welfare == g1.last_welfare and g0.last_social_ranking == []
    # today's rule: the first maximum of the egalitarian welfare
    assert t0 == g0.last_candidates[int(np.argmax(np.array(g0.last_welfare)))]
    assert bon_runs["schulze"][1].last_candidates == g0.last_candidates
    assert bon_runs["schulze"][1].last_welfare == g0.last_welfare
