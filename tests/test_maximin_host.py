"""CPU tests of the maximin-lottery / coalition-improvement path: the NumPy restatement
(tests/maximin_ref.py, the expected values of the GPU tests) is pinned to what the reference's
HiGHS LPs returned (tests/golden/maximin_golden.npz), and the entry point, ops and core reject
bad arguments before any launch.

ALPHA_TOL = 1e-6 relative: HiGHS's own feasibility and optimality tolerances are 1e-7, so the
recorded optimum is no surer than that, and this is ten times it.  Measured: 2.8e-11 over the
1,713 LPs, 6.0e-15 over the eleven egalitarian values; the restatement's worst duality gap there
is 7.4e-15 and its longest solve 19 pivots (printed below; GAP_TOL of the GPU tests is taken from
such figures)."""
import ctypes
import itertools
import os
from importlib import import_module

import numpy as np
import pytest

import maximin_ref

ALPHA_TOL = 1e-6
NAN = float("nan")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "maximin_golden.npz"))


@pytest.fixture(scope="module")
def problems(golden_dir):
    return np.load(os.path.join(golden_dir, "lottery_golden.npz"))


def lotteries(problems, name):
    """The fixture's three lotteries of a problem, in the order of golden["lotteries"]."""
    U = problems[f"U_{name}"]
    m = U.shape[1]
    p_util = np.zeros(m)
    p_util[int(np.argmax(U.sum(axis=0)))] = 1.0
    return [problems[f"p_{name}"], p_util, np.ones(m) / m]


def test_fixture_shape(golden, problems):
    assert [str(x) for x in golden["lotteries"]] == ["nash", "utilitarian", "uniform"]
    assert [str(x) for x in golden["cases"]] == [str(x) for x in problems["cases"]]
    assert len(golden["cases"]) == 11
    for name in golden["cases"]:
        n = problems[f"U_{name}"].shape[0]
        assert golden[f"alpha_{name}"].shape == (3, 2 ** n - 1)
        ok = golden[f"success_{name}"]
        top = np.where(ok, golden[f"alpha_{name}"], 1.0).max(axis=1)
        assert np.array_equal(np.maximum(top, 1.0), golden[f"maxalpha_{name}"])


def test_restatement_matches_the_reference(golden, problems):
    worst_alpha = worst_gap = worst_egal = 0.0
    most_pivots = solved = 0
    for name in [str(x) for x in golden["cases"]]:
        U = problems[f"U_{name}"]
        masks = maximin_ref.coalition_masks(U.shape[0])
        for li, p in enumerate(lotteries(problems, name)):
            base = U @ p
            tops = [1.0]
            for ci, mask in enumerate(masks):
                if not golden[f"success_{name}"][li, ci]:
                    continue
                r = maximin_ref.solve(U, base, mask)
                assert r["pivots"] >= 0, (name, li, ci)
                want = golden[f"alpha_{name}"][li, ci]
                err = abs(r["alpha"] - want) / abs(want)
                assert err <= ALPHA_TOL, (name, li, ci, r["alpha"], want)
                lo, up = maximin_ref.certificate(U, r["q"], r["lam"], mask, base)
                worst_alpha = max(worst_alpha, err)
                worst_gap = max(worst_gap, (up - lo) / up)
                most_pivots = max(most_pivots, r["pivots"])
                solved += 1
                assert r["q"].min() >= 0.0 and abs(r["q"].sum() - 1.0) <= 1e-12
                assert r["lam"].min() >= 0.0 and abs(r["lam"].sum() - 1.0) <= 1e-12
                tops.append(r["alpha"])
            want = golden[f"maxalpha_{name}"][li]
            assert abs(max(tops) - want) <= ALPHA_TOL * want, (name, li)
        r = maximin_ref.solve(U)
        want = float(golden[f"egal_value_{name}"])
        worst_egal = max(worst_egal, abs(r["value"] - want) / want)
        assert abs(r["value"] - want) <= ALPHA_TOL * want, name
        assert abs((U @ r["q"]).min() - want) <= ALPHA_TOL * want, name
    print(f"{solved} LPs: worst relative alpha error {worst_alpha:.3e}, worst egalitarian value "
          f"error {worst_egal:.3e}, worst duality gap {worst_gap:.3e}, most pivots {most_pivots}")
    assert solved == 9 * 3 * 63 + 3 * 3 + 3 * 1


def test_restatement_edges():
    # a single agent: the point mass on the lowest-index maximum of its row, one pivot
    U = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 1.0, 1.0]])
    r = maximin_ref.solve(U, mask=1)
    assert r["pivots"] == 1 and np.array_equal(r["q"], [0.0, 1.0, 0.0, 0.0])
    assert r["alpha"] == 0.5 * 3.0 and np.array_equal(r["lam"], [1.0, 0.0])
    # one column: min_i M[i, 0] without a pivot, the weight on the lowest row of the minimum
    r = maximin_ref.solve(np.array([[4.0], [2.0], [2.0]]), base=np.array([2.0, 1.0, 1.0]))
    assert r["pivots"] == 0 and r["value"] == 2.0 and np.array_equal(r["lam"], [1.0, 0.0, 0.0])
    # all equal: value exactly 1
    r = maximin_ref.solve(np.ones((6, 81)), mask=0b101101)
    assert r["value"] == 1.0 and r["alpha"] == 4.0 / 6.0
    # a 2 x 2 game against its closed form: the optimal q equalises the two agents
    U = np.array([[1.0, 0.2], [0.1, 1.0]])
    r = maximin_ref.solve(U)
    q0 = 0.8 / 1.7                                   # equalises 1 q0 + 0.2 (1 - q0) = 0.1 q0 + (1 - q0)
    assert abs(r["q"][0] - q0) <= 1e-15 and abs(r["value"] - (0.2 + 0.8 * q0)) <= 1e-15
    # statuses
    for defect in (NAN, float("inf"), -1.0):
        V = np.ones((3, 4))
        V[2, 1] = defect
        r = maximin_ref.solve(V, mask=0b011)          # anywhere in the problem, member or not
        assert r["pivots"] == -1 and np.isnan(r["alpha"]) and np.isnan(r["q"]).all()
    V = np.ones((3, 4))
    V[2] = 0.0
    assert maximin_ref.solve(V)["pivots"] == -1 and maximin_ref.solve(V, mask=0b011)["pivots"] == 1
    for b in (0.0, -1.0, NAN, float("inf")):
        base = np.array([1.0, b, 1.0])
        assert maximin_ref.solve(np.ones((3, 4)), base)["pivots"] == -1
        assert maximin_ref.solve(np.ones((3, 4)), base, mask=0b101)["pivots"] == 1
    r = maximin_ref.solve(U, max_pivots=0)
    assert r["pivots"] == -2 and np.isnan(r["alpha"]) and np.isnan(r["lam"]).all()
    assert maximin_ref.solve(U, max_pivots=1)["pivots"] == -2
    assert maximin_ref.solve(U, max_pivots=2)["pivots"] == 2


def _lib(pkg):
    return import_module(pkg.__name__ + "._lib").load()


def test_maximin_lottery_rejects_bad_arguments(pkg):
    L = _lib(pkg)
    d = ctypes.c_void_p(256)
    good = np.array([0b000001, 0b111111, 0b100000], dtype=np.uint64)

    def call(P=2, A=6, m=81, ldu=81, ldp=None, base=None, mh=good, md=d, C=3, max_pivots=10, U=d,
             alpha=d, q=None, lam=None, piv=d):
        ldp = A * ldu if ldp is None else ldp
        mh = mh.ctypes.data if isinstance(mh, np.ndarray) else mh
        return L.cs_maximin_lottery(U, P, A, m, ldu, ldp, base, mh, md, C, max_pivots, alpha, q,
                                    lam, piv, None)

    u64 = lambda *xs: np.array(xs, dtype=np.uint64)      # noqa: E731
    for bad in (dict(A=0), dict(A=65), dict(m=0), dict(m=16385, ldu=16385), dict(ldu=80),
                dict(max_pivots=-1), dict(P=-1), dict(C=0), dict(ldp=5 * 81 + 80),
                dict(mh=u64(1, 0, 3)),                    # an empty coalition
                dict(mh=u64(1, 1 << 6, 3)),               # agent 6 of 6
                dict(mh=u64(1, 1 << 63, 3)),
                dict(mh=None), dict(md=None),             # one copy without the other
                dict(mh=None, md=None, C=2),              # no masks: one coalition
                dict(P=1 << 20, C=1 << 12, mh=np.ones(1 << 12, dtype=np.uint64)),   # grid
                dict(U=None), dict(alpha=None), dict(piv=None),
                dict(U=ctypes.c_void_p(260)), dict(base=ctypes.c_void_p(260)),
                dict(md=ctypes.c_void_p(260)), dict(q=ctypes.c_void_p(260)),
                dict(lam=ctypes.c_void_p(260)), dict(piv=ctypes.c_void_p(258))):
        assert call(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_maximin_lottery: "), bad
    # an empty batch is a no-op, with or without masks, at either side of the LDS limit
    assert call(P=0) == 0
    assert call(P=0, mh=None, md=None, C=1) == 0
    assert call(P=0, A=64, m=16384, ldu=16384, mh=u64(1 << 63), C=1) == 0
    lib = import_module(pkg.__name__ + "._lib")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include",
                               "consensus_scoring.h")).read()
    assert f"#define CS_MAXIMIN_MAX_PIVOTS {lib.MAXIMIN_MAX_PIVOTS}\n" in header
    assert maximin_ref.MAX_PIVOTS == lib.MAXIMIN_MAX_PIVOTS


def test_ops_and_core_check_their_arguments(pkg, ops):
    import torch
    core = import_module(pkg.__name__ + ".core")
    for name in ("egalitarian_lottery", "max_coalition_improvement",
                 "max_coalition_improvement_batch", "maximin_certificate", "coalition_sweep"):
        assert callable(getattr(core, name, None)), name
    # the reference's order of coalitions
    want = [sum(1 << i for i in S) for r in range(1, 5) for S in itertools.combinations(range(4), r)]
    assert core.coalition_masks(4).tolist() == want
    assert np.array_equal(core.coalition_masks(6), maximin_ref.coalition_masks(6))
    assert core.coalition_masks(6).size == 63 and core.MAX_COALITION_AGENTS == 16
    U, p = np.ones((17, 4)), np.full(4, 0.25)
    with pytest.raises(ops.CSError, match="at most 16 agents"):
        core.max_coalition_improvement(U, p)
    for bad in ([[]], [[0, 0]], [[17]], [[-1]], []):
        with pytest.raises(ops.CSError):
            core.max_coalition_improvement(U, p, coalitions=bad)
    with pytest.raises(ops.CSError):
        core.max_coalition_improvement(np.ones(4), p)
    with pytest.raises(ops.CSError):
        core.max_coalition_improvement(np.ones((3, 5)), p)
    with pytest.raises(ops.CSError):
        core.egalitarian_lottery(np.ones(4))
    assert ops.coalition_masks([1, 0b110], 3).tolist() == [1, 6]
    assert ops.coalition_masks(np.array([1 << 63], dtype=np.uint64), 64).tolist() == [1 << 63]
    for bad, A in (([0], 3), ([8], 3), ([-1], 3), ([], 3), ([1.5], 3), (["a"], 3)):
        with pytest.raises(ops.CSError):
            ops.coalition_masks(bad, A)
    with pytest.raises(ops.CSError, match="no CPU path"):
        ops.maximin_lottery(torch.ones(3, 4, dtype=torch.float64))
    with pytest.raises(ops.CSError):
        ops.maximin_lottery(torch.ones(3, 4))                      # fp32
    with pytest.raises(ops.CSError):
        ops.maximin_lottery(torch.ones(4, dtype=torch.float64))
    # the certificate is host arithmetic: the 2 x 2 game's optimum has equal bounds
    U = np.array([[1.0, 0.2], [0.1, 1.0]])
    r = maximin_ref.solve(U)
    lo, up = core.maximin_certificate(U, r["q"], r["lam"])
    assert abs(lo - r["value"]) <= 1e-15 and abs(up - r["value"]) <= 1e-15
    lo, up = core.maximin_certificate(U, [0.5, 0.5], [1.0, 0.0], S=[0], base=[2.0, 1.0])
    assert lo == 0.3 and up == 0.5
    assert (lo, up) == maximin_ref.certificate(U, [0.5, 0.5], [1.0, 0.0], 1, [2.0, 1.0])
