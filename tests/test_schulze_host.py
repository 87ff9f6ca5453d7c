"""CPU tests of the Schulze path: the NumPy restatement (tests/schulze_ref.py, the expected
values of the GPU tests) in both its forms is pinned to what the reference's functions returned
(tests/golden/schulze_golden.npz, written by tests/golden/make_schulze_golden.py), and
cs_schulze rejects bad arguments with a status and a message before any launch.

Everything here is integer arithmetic: every comparison is exact."""
import ctypes
import os
from importlib import import_module

import numpy as np
import pytest

import schulze_ref as sr


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "schulze_golden.npz"))


def _stages(form):
    if form == "loops":
        return sr.defeats_loops, sr.strengths_loops, sr.ranking_loops
    return sr.defeats_fast, sr.strengths_fast, sr.ranking_fast


def test_loops_equal_fast_on_random_tied_elections():
    rng = np.random.default_rng(11)
    tied = 0
    for n in range(240):
        C = int(rng.integers(1, 13))
        R = int(rng.integers(1, 9))
        x = sr.random_election(rng, R, C, "ties" if n % 4 else "perm")
        d = sr.defeats_loops(x)
        assert np.array_equal(d, sr.defeats_fast(x)), n
        p = sr.strengths_loops(d)
        assert np.array_equal(p, sr.strengths_fast(d)), n
        t = sr.ranking_loops(p)
        assert np.array_equal(t, sr.ranking_fast(p)), n
        tied += len(set(t.tolist())) < C
        # stage 2 on matrices that are no defeat counts: any integers, negative ones included
        g = rng.integers(-5, 6, (C, C)).astype(np.int32)
        np.fill_diagonal(g, 0)
        assert np.array_equal(sr.strengths_loops(g), sr.strengths_fast(g)), n
    assert tied >= 120


@pytest.mark.parametrize("form", ["loops", "fast"])
def test_restatement_equals_every_golden_entry(golden, form):
    f_def, f_str, f_rank = _stages(form)
    for i in range(int(golden["known"])):
        g = lambda k: golden[f"k{i}_{k}"]                     # noqa: E731
        # what the reference's test file states is what its functions return
        assert np.array_equal(g("ref_defeats"), g("defeats"))
        assert np.array_equal(g("ref_strengths"), g("strengths"))
        assert np.array_equal(g("ref_ranking"), g("ranking"))
        assert np.array_equal(g("ref_aggregate"), g("ranking"))
        # stage by stage from the stated inputs, as the reference's own test runs them
        assert np.array_equal(f_def(g("rankings")), g("defeats")), i
        assert np.array_equal(f_str(g("defeats")), g("strengths")), i
        assert np.array_equal(f_rank(g("strengths")), g("ranking")), i
        assert np.array_equal(sr.solve(g("rankings"), form=form)["ranking"], g("ranking")), i
    for i in range(int(golden["fig1"])):
        assert np.array_equal(golden[f"f{i}_ref_ranking"], golden[f"f{i}_ranking"])
        got = sr.solve(golden[f"f{i}_rankings"], form=form)
        assert got["status"] == 0 and np.array_equal(got["ranking"], golden[f"f{i}_ranking"]), i
    for i in range(int(golden["random"])):
        x = golden[f"r{i}_rankings"]
        if form == "loops" and x.shape[1] > 48:
            continue                                          # seconds per election; fast covers them
        got = sr.solve(x, ballot=golden[f"r{i}_ballot"], form=form)
        assert got["status"] == 0
        for k in ("defeats", "strengths", "ranking", "untied"):
            assert np.array_equal(got[k], golden[f"r{i}_{k}"]), (i, k)
        assert got["winner"] == int(np.where(golden[f"r{i}_untied"] == 0)[0][0]), i


def test_golden_random_elections_are_mostly_tied(golden):
    """The condition that keeps the golden comparison honest: a tied social ranking in at least
    half of the random (4, 5) elections, judged on the recorded reference results."""
    shapes = {}
    for i in range(int(golden["random"])):
        R, C = golden[f"r{i}_rankings"].shape
        t = golden[f"r{i}_ranking"]
        n, k = shapes.get((R, C), (0, 0))
        shapes[(R, C)] = (n + 1, k + (len(set(t.tolist())) < C))
    assert set(shapes) == {(1, 1), (2, 2), (4, 5), (8, 16), (16, 48), (5, 65), (16, 128)}
    n, k = shapes[(4, 5)]
    assert n == 64 and 2 * k >= n, shapes
    kinds = [str(s) for s in golden["random_kind"]]
    assert kinds.count("ties") == kinds.count("perm") == 45


def test_ballot_untie(golden):
    # the six seeded cases: the ballot is default_rng(seed).permutation(C), as the reference draws
    assert int(golden["tiebreak"]) == 6
    for i in range(6):
        x, seed = golden[f"t{i}_rankings"], int(golden[f"t{i}_seed"])
        assert np.array_equal(golden[f"t{i}_ref_untied"], golden[f"t{i}_untied"])
        ballot = np.random.default_rng(seed).permutation(x.shape[1]).astype(np.int32)
        got = sr.solve(x, ballot=ballot)
        assert np.array_equal(got["untied"], golden[f"t{i}_untied"]), i
        assert len(set(got["untied"].tolist())) == x.shape[1]
    # ballots with repeated values: _hm_untie_ranking_with_ballot's rule, written with np.unique
    rng = np.random.default_rng(5)
    for _ in range(100):
        C = int(rng.integers(1, 10))
        ranking = rng.integers(0, 3, C)
        ballot = rng.integers(-4, 4, C).astype(np.int32)
        nr = np.unique(ranking, return_inverse=True)[1].reshape(-1)
        nb = np.unique(ballot, return_inverse=True)[1].reshape(-1)
        want = np.unique(nr * C + nb, return_inverse=True)[1].reshape(-1)
        assert np.array_equal(sr.untie(ranking, ballot), want)
    assert sr.untie([0, 0, 1], [7, 7, -2]).tolist() == [0, 0, 1]      # a ballot that cannot untie
    assert sr.untie([0, 0, 0], [2 ** 31 - 1, -2 ** 31, 0]).tolist() == [2, 0, 1]


def test_restatement_statuses_and_modes():
    x = np.int32([[0, 1, 2], [2, 1, 0], [0, 0, 1]])
    for bad in (3, -1):
        y = x.copy()
        y[1, 2] = bad
        got = sr.solve(y, ballot=[0, 1, 2])
        assert got["status"] == -1 and got["winner"] == -1
        assert all((got[k] == -1).all() for k in ("defeats", "strengths", "ranking", "untied"))
        # an uncounted voter's rank is not looked at
        assert sr.solve(y, valid=[1, 0, 1])["status"] == 0
    assert sr.solve(x, valid=[0, 0, 0])["status"] == -2
    got = sr.solve(x, valid=[1, 0, 1])
    want = sr.solve(x[[0, 2]])
    assert all(np.array_equal(got[k], want[k]) for k in ("defeats", "strengths", "ranking"))
    diag = np.int32([[0, 1, 1], [1, 1, 1], [1, 1, 0]])                 # the reference's own case
    assert sr.solve(diag, "defeats")["status"] == -1
    assert sr.solve(diag, "strengths")["status"] == -1
    assert sr.solve(diag, "strengths")["strengths"] is None
    # scores: higher is better, NaN prefers nothing, -0.0 == 0.0, infinities compare as usual
    s = np.float32([[np.nan, 1.0, -np.inf, np.inf], [-0.0, 0.0, 1.0, 1.0]])
    d = sr.defeats_scores(s)
    assert d.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [1, 2, 1, 0]]
    fin = np.float32([[0.5, -1.0, 0.5, 3.0], [2.0, 2.0, -7.0, 0.0]])
    assert np.array_equal(sr.defeats_scores(fin), sr.defeats_fast(sr.dense_ranks_of_scores(fin)))


def _lib(pkg):
    return import_module(pkg.__name__ + "._lib").load()


def test_schulze_rejects_bad_arguments(pkg):
    L = _lib(pkg)
    d, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def call(kind=0, E=2, R=5, C=4, x=d, valid=None, ballot=None, defeats=None, strengths=None,
             ranking=d, untied=None, winner=None, status=d):
        return L.cs_schulze(x, kind, E, R, C, valid, ballot, defeats, strengths, ranking, untied,
                            winner, status, None)

    for bad in (dict(E=-1), dict(C=0), dict(C=129), dict(R=0), dict(R=65537), dict(kind=-1),
                dict(kind=4), dict(kind=1, R=0), dict(kind=2, C=129),
                dict(untied=d),                                   # out_untied without ballot
                dict(E=0, untied=d),                              # ... even for an empty batch
                dict(x=None), dict(ranking=None), dict(status=None),
                dict(x=odd), dict(ballot=odd), dict(defeats=odd), dict(strengths=odd),
                dict(ranking=odd), dict(ballot=d, untied=odd), dict(winner=odd),
                dict(status=odd)):
        assert call(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_schulze: "), bad
    # an empty batch is a no-op before any pointer check, at either workgroup size
    assert call(E=0) == 0
    assert call(E=0, x=None, ranking=None, status=None) == 0
    assert call(E=0, C=128, R=65536, x=None, ranking=None, status=None) == 0
    # R is not looked at where stage 1 is skipped
    assert call(E=0, kind=2, R=0) == 0 and call(E=0, kind=3, R=-7) == 0
    lib = import_module(pkg.__name__ + "._lib")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include",
                               "consensus_scoring.h")).read()
    for name in ("RANKINGS", "SCORES", "DEFEATS", "STRENGTHS"):
        assert f"CS_SCHULZE_{name} = {getattr(lib, 'SCHULZE_' + name)}" in header
    assert (lib.SCHULZE_MAX_C, lib.SCHULZE_MAX_R, lib.SCHULZE_TILE) == (sr.MAX_C, sr.MAX_R, sr.TILE)
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "schulze.hip")).read()
    assert f"kSchTile = {sr.TILE};" in src and f"kSchNarrowC = {sr.NARROW_C};" in src


def test_ops_and_drop_ins_check_their_arguments(pkg, ops):
    import torch
    hm = import_module(pkg.__name__ + ".methods.habermas_machine")
    methods = import_module(pkg.__name__ + ".methods")
    assert "habermas_machine" not in methods.GENERATOR_MAP
    with pytest.raises(ops.CSError, match="no CPU path"):
        ops.schulze(torch.zeros(1, 3, 4, dtype=torch.int32))
    with pytest.raises(ops.CSError):
        ops.schulze(torch.zeros(1, 3, 4, dtype=torch.int64))
    with pytest.raises(ops.CSError):
        ops.schulze(torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ops.CSError):
        ops.schulze(torch.zeros(1, 3, 4, dtype=torch.int32), kind="borda")
    with pytest.raises(ops.CSError):
        ops.schulze(torch.zeros(1, 3, 4), kind="rankings")
    # the host helpers are the reference's
    assert hm._hm_normalize_ranking(np.array([0, 2, 5, 5])).tolist() == [0, 1, 2, 2]
    assert hm._hm_is_untied_ranking(np.array([3, 1, 2])) and not hm._hm_is_untied_ranking(
        np.array([1, 1, 2]))
    got = hm._hm_untie_ranking_with_ballot(np.array([0, 1, 2, 0]), np.array([3, 2, 1, 0]))
    assert got.tolist() == sr.untie([0, 1, 2, 0], [3, 2, 1, 0]).tolist() == [1, 2, 3, 0]
    for bad in (lambda: hm._hm_normalize_ranking(np.zeros((2, 2), dtype=int)),
                lambda: hm._hm_is_untied_ranking(np.zeros((2, 2), dtype=int)),
                lambda: hm._hm_untie_ranking_with_ballot(np.zeros(3, dtype=int), np.zeros(4, dtype=int)),
                lambda: hm._schulze_check_rankings(np.zeros(3, dtype=int)),
                lambda: hm._schulze_check_rankings(np.zeros((2, 3))),
                lambda: hm._schulze_check_rankings(np.array([[0, 1, 3]])),
                lambda: hm._schulze_check_rankings(np.array([[0, -1, 2]])),
                # dimension and type errors are raised on the host, before any launch
                lambda: hm._schulze_compute_strongest_path_strengths(np.int32([[0, 1, 1], [1, 0, 1]])),
                lambda: hm._schulze_rank_candidates(np.int32([[0, 1, 1], [1, 0, 1]])),
                lambda: hm._schulze_aggregate_with_ties(np.zeros(3, dtype=int)),
                lambda: hm._schulze_aggregate_with_ties(np.zeros((2, 3))),
                lambda: hm.aggregate_schulze_batch(np.zeros((2, 3), dtype=int)),
                lambda: hm.aggregate_schulze_batch(np.zeros((2, 2, 3), dtype=int), seeds=[1])):
        with pytest.raises(ValueError):
            bad()
    assert hm._schulze_check_rankings(np.array([[0, 1, 2], [2, 2, 0]])) is None
    # the None cases that need no launch
    assert hm._aggregate_schulze({}, 3) is None
    assert hm._aggregate_schulze({"a": None, "b": None}, 3) is None
    assert hm._aggregate_schulze({"a": np.array([0, 1]), "b": np.array([1, 0])}, 3) is None
    assert hm._aggregate_schulze({"a": np.array([0, 1]), "b": np.array([1, 0, 2])}, 3) is None
