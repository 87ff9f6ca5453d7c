"""CPU tests of the Nash-welfare lottery path: the NumPy restatement (tests/lottery_ref.py,
the expected values of the GPU tests) is pinned to the reference's own lotteries
(tests/golden/lottery_golden.npz), and the two entry points reject bad arguments with a
status and a message before any launch."""
import ctypes
import os

import numpy as np
import pytest

import lottery_ref

NAN = float("nan")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lottery_golden.npz"))


def test_fixture_cases_are_robust_to_rounding(golden):
    """No recorded increment lies within a factor 2 of tol, so the stopping iteration of a
    case cannot move with a 1-ulp difference."""
    tol = float(golden["tol"])
    assert len(golden["cases"]) == 11
    for name in golden["cases"]:
        inc = golden[f"inc_{name}"]
        assert inc.size == int(golden[f"iters_{name}"])
        assert not np.any((inc > tol / 2) & (inc < 2 * tol)), name


def test_restatement_matches_the_reference(golden):
    max_iters, tol = int(golden["max_iters"]), float(golden["tol"])
    for name in golden["cases"]:
        r = lottery_ref.solve(golden[f"U_{name}"], max_iters=max_iters, tol=tol)
        err = np.abs(r["p"] - golden[f"p_{name}"]).max()
        print(f"{name}: iters {r['iters']} (reference {int(golden[f'iters_{name}'])}), "
              f"max |p - p_ref| {err:.3e}")
        assert r["iters"] == int(golden[f"iters_{name}"]), name
        assert err <= 1e-6, name
        assert abs(r["p"].sum() - 1.0) <= 1e-12 and r["p"].min() >= 0.0


def test_restatement_edges():
    r = lottery_ref.solve(np.ones((3, 5)), max_iters=0)
    assert r["iters"] == 0 and np.array_equal(r["p"], np.full(5, 0.2))
    U = np.ones((2, 4))
    U[1, 2] = NAN
    assert lottery_ref.solve(U)["iters"] == -1
    U[1] = 0.0
    r = lottery_ref.solve(U)
    assert r["iters"] == -1 and np.isnan(r["p"]).all()
    # the certificate bounds the distance to the optimum: a solved case has a small gap
    r = lottery_ref.solve(np.array([[1.0, 0.2], [0.1, 1.0]]), max_iters=200)
    assert 0.0 <= r["gap"] < 1e-6


def test_policy_restatement_is_a_policy():
    p = np.random.default_rng(3).random(81)
    p /= p.sum()
    p[27:54] = 0.0                      # the subtree under first action 1
    tables = lottery_ref.policy(p, 3, 4)
    assert [t.shape for t in tables] == [(1, 3), (3, 3), (9, 3), (27, 3)]
    for t in tables:
        assert np.abs(t.sum(axis=1) - 1.0).max() <= 1e-12
    assert tables[0][0, 1] == 0.0 and np.array_equal(tables[1][1], np.full(3, 1 / 3))
    # the chain of step probabilities of a leaf multiplies back to its mass
    leaf = (2, 0, 1, 2)
    s, prob = 0, p.sum()
    for t, a in enumerate(leaf):
        prob *= tables[t][s, a]
        s = s * 3 + a
    assert abs(prob - p[s]) <= 1e-15


def _lib(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + "._lib").load()


def test_nash_lottery_rejects_bad_arguments(pkg):
    L = _lib(pkg)
    d = ctypes.c_void_p(256)

    def call(P=2, A=6, m=81, ldu=81, ldp=None, max_iters=10, tol=1e-10, variant=0, U=d, p=d):
        ldp = A * ldu if ldp is None else ldp
        return L.cs_nash_lottery(U, P, A, m, ldu, ldp, max_iters, tol, variant, p, None, None,
                                 None, None, None)

    for bad in (dict(A=0), dict(A=65), dict(m=0), dict(m=16385, ldu=16385), dict(ldu=80),
                dict(max_iters=-1), dict(tol=NAN), dict(tol=float("inf")), dict(P=-1),
                dict(variant=3), dict(ldp=5 * 81 + 80), dict(U=ctypes.c_void_p(260)),
                dict(U=None), dict(p=None),
                # staged U that cannot fit the LDS: 16 x 4096 x 8 = 512 KiB
                dict(variant=1, A=16, m=4096, ldu=4096)):
        assert call(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_nash_lottery: "), bad
    # the same shape is fine for the library's choice and the global variant up to the launch;
    # an empty batch is a no-op
    assert call(P=0) == 0
    assert call(P=0, variant=2, A=16, m=4096, ldu=4096) == 0
    assert call(P=0, variant=1, A=16, m=1000, ldu=1000) == 0


def test_lottery_policy_rejects_bad_arguments(pkg):
    L = _lib(pkg)
    d = ctypes.c_void_p(256)
    for bad in ((2, 0, 3), (2, 3, 0), (2, 2, 15), (2, 129, 2), (2, 16385, 1), (2, 1, 65),
                (-1, 3, 4)):
        assert L.cs_lottery_policy(d, *bad, d, None) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_lottery_policy: "), bad
    assert L.cs_lottery_policy(None, 1, 3, 4, d, None) == -1
    assert L.cs_lottery_policy(d, 1, 3, 4, ctypes.c_void_p(260), None) == -1
    assert L.cs_lottery_policy(d, 0, 128, 2, d, None) == 0
    assert L.cs_lottery_policy(d, 0, 2, 14, d, None) == 0


def test_core_module_names_the_lottery_entry_points(pkg):
    """The drop-in module provides the lottery API (it once ended at the utilities)."""
    from importlib import import_module
    core = import_module(pkg.__name__ + ".core")
    for name in ("FW_nash_welfare", "FW_nash_welfare_batch", "nash_lottery_certificate",
                 "induced_policy", "build_prefix_index", "induced_policy_rollout"):
        assert callable(getattr(core, name, None)), name
    # host pieces: the prefix table of the reference's contract, and the certificate
    idx = core.build_prefix_index(core.enumerate_leaves(2, 2))
    assert idx[()] == [0, 1, 2, 3] and idx[(1,)] == [2, 3] and idx[(1, 0)] == [2]
    U = np.array([[1.0, 0.2], [0.1, 1.0]])
    r = lottery_ref.solve(U, max_iters=200)
    F, gap = core.nash_lottery_certificate(U, r["p"])
    assert abs(F - r["F"]) <= 1e-12 and abs(gap - r["gap"]) <= 1e-12
