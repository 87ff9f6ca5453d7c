"""GPU tests of the Nash-welfare lottery solver (cs_nash_lottery) and the induced token policy
(cs_lottery_policy) through ops.py and the core.py drop-ins.

Expected values: the reference's own lotteries (tests/golden/lottery_golden.npz) and the NumPy
restatement tests/lottery_ref.py, which tests/test_lottery_host.py pins to that fixture.

Tolerance on p: 1e-6.  The restatement, run for 1500 iterations with sequential sums and an
incrementally carried ``a``, stays within 1.0e-7 of the reference's p (accumulated 1e-9
golden-section slack, also with a 1e-15 relative perturbation of ``a`` per iteration, which
stands in for a GPU log or division that is an ulp off); 1e-6 is ten times that.  Iteration
counts must be equal: no case has an F increment within a factor 2 of tol (checked below for
the cases made here, by the generator for the fixture)."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import lottery_ref

pytestmark = pytest.mark.gpu

P_TOL = 1e-6


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lottery_golden.npz"))


@pytest.fixture(scope="module")
def core(pkg):
    return import_module(pkg.__name__ + ".core")


def _cuda(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _robust(ref, tol):
    """The expected solve's stopping iteration cannot move with a 1-ulp difference."""
    inc = ref["increments"]
    return not np.any((inc > tol / 2) & (inc < 2 * tol))


def _rand_u(seed, A, m, sigma=1.0):
    return np.exp(np.random.default_rng(seed).normal(size=(A, m)) * sigma)


def _check_against(res, ref, what):
    err = np.abs(res["p"] - ref["p"]).max()
    print(f"{what}: iters {int(res['iters'])} (expected {ref['iters']}), max |p - p_ref| {err:.3e}")
    assert int(res["iters"]) == ref["iters"], what
    assert err <= P_TOL, what


# 1 ---------------------------------------------------------------------------------------
def test_fixture_lotteries(core, ops, dev, golden, golden_dir):
    max_iters, tol = int(golden["max_iters"]), float(golden["tol"])
    names = [str(n) for n in golden["cases"]]
    for name in names:
        U = golden[f"U_{name}"]
        p = core.FW_nash_welfare(U, max_iters=max_iters, tol=tol)
        res = _np(ops.nash_lottery(_cuda(U, dev), max_iters=max_iters, tol=tol))
        assert np.array_equal(p, res["p"]), name
        _check_against(res, {"p": golden[f"p_{name}"], "iters": int(golden[f"iters_{name}"])}, name)
        assert p.min() >= 0.0 and abs(p.sum() - 1.0) <= 1e-12, name
    nine = [n for n in names if golden[f"U_{n}"].shape == (6, 81)]
    assert len(nine) == 9
    Us = np.stack([golden[f"U_{n}"] for n in nine])
    pb = core.FW_nash_welfare_batch(Us, max_iters=max_iters, tol=tol)
    rb = _np(ops.nash_lottery(_cuda(Us, dev), max_iters=max_iters, tol=tol))
    assert np.array_equal(pb, rb["p"])
    for k, n in enumerate(nine):
        _check_against({"p": pb[k], "iters": rb["iters"][k]},
                       {"p": golden[f"p_{n}"], "iters": int(golden[f"iters_{n}"])}, f"batch {n}")
        assert pb[k].min() >= 0.0 and abs(pb[k].sum() - 1.0) <= 1e-12
    # the lottery make_golden.py recorded "for the lottery API"
    stored = np.load(os.path.join(golden_dir, "core_golden.npz"))
    assert np.abs(pb[nine.index("42_9")] - stored["p_nw_42_9"]).max() <= P_TOL


# 2 ---------------------------------------------------------------------------------------
def test_certificate_is_recomputed_from_p(core, ops, dev, golden):
    cases = [golden["U_42_9"], golden["U_44_0"], _rand_u(11, 16, 1000, 2.0), _rand_u(12, 64, 100)]
    for U in cases:
        res = _np(ops.nash_lottery(_cuda(U, dev), max_iters=300, tol=1e-11))
        a = U @ res["p"]
        F = float(np.sum(np.log(a)))
        gap = float((U / a[:, None]).sum(0).max() - U.shape[0])
        print(f"{U.shape}: |a| {np.abs(res['a'] - a).max():.2e} |F| {abs(res['F'] - F):.2e} "
              f"|gap| {abs(res['gap'] - gap):.2e} gap {gap:.3e}")
        assert np.abs(res["a"] - a).max() <= 1e-9
        assert abs(float(res["F"]) - F) <= 1e-9
        assert abs(float(res["gap"]) - gap) <= 1e-9
        assert gap >= -1e-9                     # F* - F(p) <= gap, and F* >= F(p)
        Fh, gh = core.nash_lottery_certificate(U, res["p"])
        assert Fh == F and gh == gap


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,m", [(6, 81), (1, 1), (1, 2), (64, 100), (16, 1000),
                                 (2, 4097)])   # m > 4096: the 1024-thread launch, 16 waves
def test_variants_are_bitwise_equal(ops, dev, A, m):
    U = _cuda(_rand_u(100 * A + m, A, m, 2.0), dev)
    r1 = ops.nash_lottery(U, max_iters=100, variant=1)
    r2 = ops.nash_lottery(U, max_iters=100, variant=2)
    r0 = ops.nash_lottery(U, max_iters=100)
    again = ops.nash_lottery(U, max_iters=100, variant=1)
    for k in ("p", "a", "F", "gap", "iters"):
        assert torch.equal(r1[k], r2[k]), k
        assert torch.equal(r1[k], r0[k]), k
        assert torch.equal(r1[k], again[k]), k
    assert int(r1["iters"]) >= 1 and bool(torch.isfinite(r1["p"]).all())


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,m,pad", [
    (3, 1, 0), (5, 63, 0), (5, 64, 0), (5, 65, 0), (4, 255, 0), (4, 257, 0),
    (16, 4096, 0),              # 512 KiB of utilities: the library's choice is the global path
    (1, 10, 0), (63, 50, 0), (64, 50, 0),
    (6, 81, 3),                 # ldu = m + 3
    (2, 4097, 0),               # m > 4096: the 1024-thread launch
])
def test_shapes_against_restatement(ops, dev, A, m, pad):
    tol = 1e-10
    U = _rand_u(7 * A + m, A, m)
    ref = lottery_ref.solve(U, max_iters=200, tol=tol)
    assert _robust(ref, tol)
    wide = torch.full((A, m + pad), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :m] = _cuda(U, dev)
    res = _np(ops.nash_lottery(wide[:, :m], max_iters=200, tol=tol))
    _check_against(res, ref, f"{A} x {m} (+{pad})")
    assert abs(res["p"].sum() - 1.0) <= 1e-12 and res["p"].min() >= 0.0
    if A * m * 8 > 147456:
        with pytest.raises(ops.CSError):
            ops.nash_lottery(wide[:, :m], max_iters=1, variant=1)
        g = ops.nash_lottery(wide[:, :m], max_iters=200, tol=tol, variant=2)
        assert np.array_equal(g["p"].cpu().numpy(), res["p"])


def test_batch_problems_stop_independently(ops, dev, golden):
    tol = float(golden["tol"])
    names = ["42_9", "43_0", "42_19", "44_9", "43_19"]    # the second stops after 3 iterations
    Us = np.stack([golden[f"U_{n}"] for n in names])
    refs = [lottery_ref.solve(U, max_iters=200, tol=tol) for U in Us]
    assert [r["iters"] for r in refs] == [200, 3, 200, 200, 200]
    assert all(_robust(r, tol) for r in refs)
    res = _np(ops.nash_lottery(_cuda(Us, dev), max_iters=200, tol=tol))
    for k, ref in enumerate(refs):
        _check_against({"p": res["p"][k], "iters": res["iters"][k]}, ref, names[k])
    # a strided batch (every other problem of a larger stack) gives the same bits
    big = torch.zeros((10, 6, 81), dtype=torch.float64, device=dev)
    big[::2] = _cuda(Us, dev)
    strided = ops.nash_lottery(big[::2], max_iters=200, tol=tol)
    assert np.array_equal(strided["p"].cpu().numpy(), res["p"])


# 5 ---------------------------------------------------------------------------------------
def test_ties_take_the_lowest_index(ops, dev):
    U = _rand_u(5, 6, 81)
    top = int(np.argmax(lottery_ref.solve(U, max_iters=50)["p"]))     # a column of the support
    assert top > 40
    U[:, 5] = U[:, top]                  # columns 5, 40 and `top` tie wherever one is the best
    U[:, 40] = U[:, 5]
    ref = lottery_ref.solve(U, max_iters=200)
    assert _robust(ref, 1e-10) and ref["p"][5] > 0.1 > ref["p"][40]
    res = _np(ops.nash_lottery(_cuda(U, dev), max_iters=200))
    _check_against(res, ref, "duplicate column")
    # columns 40 and `top` only ever decay, with the columns that are never chosen
    assert res["p"][40] == res["p"].min() == res["p"][top] and res["p"][40] < res["p"][5]
    # m > 4096, the 1024-thread launch: the best column of the first iteration copied to columns
    # 5 and 1000, which threads of the first and the last of the 16 waves hold; the first vertex
    # is the lower index, so after one iteration every other column still has (1 - gamma) / m
    U = _rand_u(5, 6, 4097)
    g = (U / U.mean(axis=1)[:, None]).sum(axis=0)
    top = int(np.argmax(g))
    assert top > 5
    U[:, 5] = U[:, top]
    U[:, 1000] = U[:, top]
    g = (U / U.mean(axis=1)[:, None]).sum(axis=0)
    assert g[5] == g[1000] == g.max() and np.sort(g)[-4] < g.max() - 1.0   # a clear margin
    ref = lottery_ref.solve(U, max_iters=1)
    res = _np(ops.nash_lottery(_cuda(U, dev), max_iters=1))
    _check_against(res, ref, "duplicate column, 16 waves")
    assert int(np.argmax(res["p"])) == 5 and res["p"][5] > 0.1
    assert res["p"][1000] == res["p"].min() == res["p"][top]


def test_all_equal_utilities_and_zero_iterations(ops, dev):
    # all ones: every evaluation of the line search is log(1) or log(1 - ulp) in the same fp64
    # arithmetic as the restatement, so the bracket closes on gamma < 1e-9 on both sides and p
    # moves from uniform by less than the bracket
    U = np.ones((6, 81))
    ref = lottery_ref.solve(U, max_iters=200)
    res = _np(ops.nash_lottery(_cuda(U, dev), max_iters=200))
    _check_against(res, ref, "all equal")
    assert np.abs(res["p"] - 1.0 / 81).max() <= 1e-9
    Ur = _cuda(_rand_u(1, 4, 33), dev)
    z = ops.nash_lottery(Ur, max_iters=0)
    assert int(z["iters"]) == 0
    assert torch.equal(z["p"], torch.full((33,), 1.0 / 33, dtype=torch.float64, device=dev))
    assert abs(float(z["F"]) - float(torch.log(Ur.mean(dim=1)).sum())) <= 1e-12


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["nan", "zero_row", "negative", "inf"])
def test_bad_problem_does_not_disturb_its_neighbours(ops, dev, defect):
    Us = np.stack([_rand_u(s, 6, 81) for s in (21, 22, 23)])
    if defect == "nan":
        Us[1, 3, 17] = float("nan")
    elif defect == "zero_row":
        Us[1, 4, :] = 0.0
    elif defect == "negative":
        Us[1, 0, 80] = -1e-3
    else:
        Us[1, 5, 0] = float("inf")
    Ut = _cuda(Us, dev)
    for variant in (1, 2):
        res = ops.nash_lottery(Ut, max_iters=50, variant=variant)     # raises unless CS_OK
        assert int(res["iters"][1]) == -1
        assert bool(torch.isnan(res["p"][1]).all()) and bool(torch.isnan(res["a"][1]).all())
        assert bool(torch.isnan(res["F"][1])) and bool(torch.isnan(res["gap"][1]))
        for k in (0, 2):
            alone = ops.nash_lottery(Ut[k], max_iters=50, variant=variant)
            for key in ("p", "a", "F", "gap", "iters"):
                assert torch.equal(res[key][k], alone[key]), (key, k)
            assert int(alone["iters"]) == 50
    # the process is healthy afterwards
    torch.cuda.synchronize()
    assert float((Ut[0] * 2).sum()) > 0


# 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 4), (2, 1), (1, 3), (4, 7), (128, 2)])
def test_induced_policy_tables(core, ops, dev, B, L):
    m = B ** L
    p = np.random.default_rng(B * 31 + L).random(m)
    if B > 1:
        p[: m // B] = 0.0                  # the whole subtree under first action 0
        if L > 1:
            p[-(m // B // B):] = 0.0       # and a deeper one under (B-1, B-1)
    p /= p.sum()
    tables = core.induced_policy(p, B, L)
    want = lottery_ref.policy(p, B, L)
    assert len(tables) == L
    for t in range(L):
        assert tables[t].shape == (B ** t, B)
        assert np.abs(tables[t] - want[t]).max() <= 1e-10, t
        assert np.abs(tables[t].sum(axis=1) - 1.0).max() <= 1e-12, t
    if B > 1:
        assert tables[0][0, 0] == 0.0
        if L > 1:
            assert np.array_equal(tables[1][0], np.full(B, 1.0 / B))      # zero-mass prefix (0,)
            if L > 2:
                assert np.array_equal(tables[2][B * B - 1], np.full(B, 1.0 / B))
    # a batch through ops gives every problem the table it has alone
    pt = _cuda(np.stack([p, np.full(m, 1.0 / m)]), dev)
    both = ops.lottery_policy(pt, B, L)
    for t in range(L):
        assert both[t].shape == (2, B ** t, B)
        assert np.array_equal(both[t][0].cpu().numpy(), tables[t])
        assert float((both[t][1] - 1.0 / B).abs().max()) <= 1e-15


# 8 ---------------------------------------------------------------------------------------
def test_rollout_reproduces_the_reference_draws(core, golden):
    name = str(golden["rollout_case"])
    B, L = int(golden["rollout_B"]), int(golden["rollout_L"])
    p = golden[f"p_{name}"]
    p_hat, tv = core.induced_policy_rollout(p, core.enumerate_leaves(B, L), B, L,
                                            num_samples=int(golden["rollout_samples"]),
                                            seed=int(golden["rollout_seed"]))
    assert np.array_equal(p_hat, golden["rollout_p_hat"])
    assert tv == float(golden["rollout_tv"])
