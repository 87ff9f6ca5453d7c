"""GPU tests of the maximin-lottery / coalition-improvement solver (cs_maximin_lottery) through
ops.py and the core.py drop-ins.

Expected values: what the reference's HiGHS LPs returned (tests/golden/maximin_golden.npz) and
the NumPy restatement tests/maximin_ref.py, which tests/test_maximin_host.py pins to that
fixture.  Every result is also certified without any reference: from the returned q and lam,
lower = min_{i in S} (M q)_i <= value <= upper = max_j (lam M)_j by weak duality, so
(upper - lower) / upper bounds the distance to the optimum.

ALPHA_TOL = 1e-6 relative against the reference (ten times HiGHS's 1e-7 tolerances).
GAP_TOL = 1000 x the restatement's worst duality gap on the inputs used here, computed on the
CPU: GAP_MEASURED below is that gap, 7.4e-15 over the fixture's 1,713 LPs and 8.02e-15 over the
cases of tests 3 and 4 (the 64-agent egalitarian problems; _worst_restatement_gap() recomputes
it and test_gap_tol_is_as_measured checks the constant against it every run), so GAP_TOL is
8.1e-12.  The margin of 1000 is for a GPU division or a
different but valid pivot path that ends on a differently conditioned basis; it is not taken
from the kernel's output.

Pivot counts must equal the restatement's: it performs the kernel's fp64 operations in the
kernel's order (no contraction to FMA on either side, correctly rounded division), so every
comparison of the ratio test sees the same bits."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import maximin_ref

pytestmark = pytest.mark.gpu

ALPHA_TOL = 1e-6
GAP_MEASURED = 8.1e-15
GAP_TOL = 1000 * GAP_MEASURED


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "maximin_golden.npz"))


@pytest.fixture(scope="module")
def problems(golden_dir):
    return np.load(os.path.join(golden_dir, "lottery_golden.npz"))


@pytest.fixture(scope="module")
def core(pkg):
    return import_module(pkg.__name__ + ".core")


def _cuda(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _lotteries(problems, name):
    U = problems[f"U_{name}"]
    m = U.shape[1]
    p_util = np.zeros(m)
    p_util[int(np.argmax(U.sum(axis=0)))] = 1.0
    return [problems[f"p_{name}"], p_util, np.ones(m) / m]


def _rand_u(seed, A, m, sigma=1.0):
    return np.exp(np.random.default_rng(seed).normal(size=(A, m)) * sigma)


def _certify(U, base, mask, alpha, q, lam, what):
    """The returned (q, lam) prove alpha optimal to GAP_TOL; returns the relative gap."""
    A = U.shape[0]
    S = maximin_ref.members((1 << A) - 1 if mask is None else mask, A)
    lo, up = maximin_ref.certificate(U, q, lam, mask, base)
    value = alpha * A / len(S)
    assert q.min() >= 0.0 and abs(q.sum() - 1.0) <= 1e-12, what
    assert lam.min() >= 0.0 and abs(lam.sum() - 1.0) <= 1e-12, what
    assert not lam[[i for i in range(A) if i not in S]].any(), what
    assert np.count_nonzero(q) <= len(S), what              # exact zeros off the basis
    assert lo <= value * (1 + GAP_TOL) and value <= up * (1 + GAP_TOL), (what, lo, value, up)
    assert (up - lo) / up <= GAP_TOL, (what, lo, up)
    return (up - lo) / up


# the cases of test 3: (A, m, sigma, column padding); each runs the full coalition, the last
# agent alone and (from three agents on) a coalition drawn from the seed, with base = U p for a
# random lottery p
SHAPES = [
    (1, 1, 1.0, 0), (1, 2, 1.0, 0), (3, 1, 1.0, 0), (5, 63, 1.0, 0), (5, 64, 1.0, 0),
    (5, 65, 1.0, 0), (4, 128, 1.0, 0), (4, 129, 1.0, 0),       # 64- / 256-thread workgroups
    (4, 255, 1.0, 0), (4, 257, 1.0, 0), (6, 81, 2.0, 3),        # ldu = m + 3, NaN padding
    (64, 50, 1.0, 0),               # the 64-agent coalition and agent 63 alone
    (16, 4096, 1.0, 0),             # 512 KiB of utilities: past the LDS limit, 256 threads
    (2, 4097, 1.0, 0),              # 1024 threads, staged
    (16, 4097, 0.5, 0),             # 1024 threads, past the LDS limit
    (64, 300, 1.0, 0),              # (64 * 65 + 64 * 300) * 8 = 186,880 B: just past the limit
]


def _shape_case(A, m, sigma):
    rng = np.random.default_rng(1000 * A + m)
    U = np.exp(rng.normal(size=(A, m)) * sigma)
    base = U @ rng.dirichlet(np.ones(m))
    masks = [(1 << A) - 1, 1 << (A - 1)]
    if A >= 3:
        masks.append(int(sum(1 << int(i) for i in rng.choice(A, size=max(2, A // 2), replace=False))))
    return U, base, masks


_REF = {}


def _ref(key, U, base, mask, **kw):
    """The restatement's solve, computed once per case and shared."""
    if key not in _REF:
        _REF[key] = maximin_ref.solve(U, base, mask, **kw)
    return _REF[key]


def _degenerate_cases():
    """The cases of test 4: (name, U, base, masks)."""
    U = _rand_u(5, 6, 81)
    dup = U.copy()
    dup[:, 5] = dup[:, 40] = dup[:, 70]            # three equal columns
    twin = U.copy()
    twin[4] = twin[1]                               # two identical agents
    return [("ones", np.ones((6, 81)), None, [0b111111, 0b101101, 0b000100]),
            ("duplicate columns", dup, None, [0b111111, 0b011011]),
            ("identical agents", twin, twin @ np.full(81, 1 / 81), [0b111111, 0b010010, 0b010011])]


def _worst_restatement_gap():
    """The restatement's worst duality gap over every case of tests 3 and 4 (CPU)."""
    worst = 0.0
    cases = [(f"{A}x{m}", *_shape_case(A, m, s)) for A, m, s, _ in SHAPES] + _degenerate_cases()
    for name, U, base, masks in cases:
        for mask in masks:
            r = _ref((name, mask), U, base, mask)
            lo, up = maximin_ref.certificate(U, r["q"], r["lam"], mask, base)
            worst = max(worst, (up - lo) / up)
    for A, m, s, _ in SHAPES:
        U = _shape_case(A, m, s)[0]
        r = _ref((f"{A}x{m}", "egalitarian"), U, None, None)
        lo, up = maximin_ref.certificate(U, r["q"], r["lam"])
        worst = max(worst, (up - lo) / up)
    return worst


def test_gap_tol_is_as_measured():
    worst = _worst_restatement_gap()
    print(f"restatement's worst duality gap over the cases of tests 3 and 4: {worst:.3e}")
    # the certificate's own matrix product may round differently on another host
    assert GAP_MEASURED / 2 <= worst <= GAP_MEASURED * 1.25


# 1, 2 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_runs(ops, dev, golden, problems):
    """Every (problem, lottery) of the fixture through ops, all coalitions in one launch each."""
    runs = {}
    for name in [str(x) for x in golden["cases"]]:
        U = problems[f"U_{name}"]
        masks = maximin_ref.coalition_masks(U.shape[0])
        for li, p in enumerate(_lotteries(problems, name)):
            base = U @ p
            runs[name, li] = (U, base, masks,
                              _np(ops.maximin_lottery(_cuda(U, dev), _cuda(base, dev), masks)))
    return runs


def test_fixture_alphas(core, ops, dev, golden, problems, fixture_runs):
    worst = 0.0
    for (name, li), (U, base, masks, res) in fixture_runs.items():
        ok = golden[f"success_{name}"][li]
        want = golden[f"alpha_{name}"][li]
        assert res["alpha"].shape == (masks.size,) and (res["pivots"][ok] >= 0).all(), name
        err = np.abs(res["alpha"][ok] - want[ok]) / np.abs(want[ok])
        worst = max(worst, err.max())
        assert err.max() <= ALPHA_TOL, (name, li)
        top = core.max_coalition_improvement(U, _lotteries(problems, name)[li])
        want_top = golden[f"maxalpha_{name}"][li]
        assert isinstance(top, float) and abs(top - want_top) <= ALPHA_TOL * want_top, (name, li)
        assert top == max(1.0, res["alpha"][ok].max())
    print(f"worst relative alpha error against the reference: {worst:.3e}")
    for name in [str(x) for x in golden["cases"]]:
        U = problems[f"U_{name}"]
        p = core.egalitarian_lottery(U)
        want = float(golden[f"egal_value_{name}"])
        assert abs((U @ p).min() - want) <= ALPHA_TOL * want, name
        assert p.min() >= 0.0 and abs(p.sum() - 1.0) <= 1e-12, name
    # an explicit coalition is that coalition's own LP
    U = problems["U_42_19"]
    p = _lotteries(problems, "42_19")[1]
    masks = maximin_ref.coalition_masks(6).tolist()
    for S in ([0, 3], [5], [0, 1, 2, 3, 4, 5]):
        ci = masks.index(sum(1 << i for i in S))
        a = core.max_coalition_improvement(U, p, coalitions=[S])
        assert a == max(1.0, fixture_runs["42_19", 1][3]["alpha"][ci])


def test_fixture_batch_is_bitwise_the_single_calls(core, ops, dev, golden, problems, fixture_runs):
    nine = [str(n) for n in golden["cases"] if problems[f"U_{n}"].shape == (6, 81)]
    assert len(nine) == 9
    masks = maximin_ref.coalition_masks(6)
    for li in range(3):
        Us = np.stack([problems[f"U_{n}"] for n in nine])
        ps = np.stack([_lotteries(problems, n)[li] for n in nine])
        base = np.stack([problems[f"U_{n}"] @ _lotteries(problems, n)[li] for n in nine])
        res = _np(ops.maximin_lottery(_cuda(Us, dev), _cuda(base, dev), masks))
        for k, n in enumerate(nine):
            for key in ("alpha", "q", "lam", "pivots"):
                assert np.array_equal(res[key][k], fixture_runs[n, li][3][key]), (n, li, key)
        tops = core.max_coalition_improvement_batch(Us, ps)
        assert tops.shape == (9,)
        assert np.array_equal(tops, np.maximum(res["alpha"].max(axis=1), 1.0))


def test_fixture_results_certify_themselves(fixture_runs):
    worst = 0.0
    for (name, li), (U, base, masks, res) in fixture_runs.items():
        for ci, mask in enumerate(masks):
            worst = max(worst, _certify(U, base, int(mask), res["alpha"][ci], res["q"][ci],
                                        res["lam"][ci], (name, li, ci)))
    print(f"worst duality gap over the fixture's LPs: {worst:.3e} (GAP_TOL {GAP_TOL:.1e})")


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,m,sigma,pad", SHAPES)
def test_shapes_against_restatement(ops, dev, A, m, sigma, pad):
    U, base, masks = _shape_case(A, m, sigma)
    wide = torch.full((A, m + pad), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :m] = _cuda(U, dev)
    res = _np(ops.maximin_lottery(wide[:, :m], _cuda(base, dev), masks))
    for ci, mask in enumerate(masks):
        what = f"{A} x {m} (+{pad}) mask {mask:#x}"
        ref = _ref((f"{A}x{m}", mask), U, base, mask)
        gap = _certify(U, base, mask, res["alpha"][ci], res["q"][ci], res["lam"][ci], what)
        err = abs(res["alpha"][ci] - ref["alpha"]) / ref["alpha"]
        print(f"{what}: pivots {res['pivots'][ci]} (expected {ref['pivots']}), alpha error "
              f"{err:.2e}, gap {gap:.2e}")
        assert res["pivots"][ci] == ref["pivots"], what
        assert err <= GAP_TOL, what
    # the last agent alone: the point mass on the lowest-index maximum of its row
    q = res["q"][1]
    j = int(np.argmax(U[A - 1]))
    assert q[j] == 1.0 and np.count_nonzero(q) == 1
    assert res["pivots"][1] == (0 if m == 1 else 1)
    if m == 1:       # one column: min_i M[i, 0], no pivots
        assert res["alpha"][0] == (U[:, 0] / base).min() and res["pivots"][0] == 0
    # without base and masks: the egalitarian problem, one result per problem
    one = _np(ops.maximin_lottery(wide[:, :m]))
    assert one["alpha"].shape == () and one["q"].shape == (m,) and one["lam"].shape == (A,)
    ref = _ref((f"{A}x{m}", "egalitarian"), U, None, None)
    assert one["pivots"] == ref["pivots"]
    assert abs(one["alpha"] - ref["alpha"]) <= GAP_TOL * ref["alpha"]
    _certify(U, None, None, float(one["alpha"]), one["q"], one["lam"], f"{A} x {m} egalitarian")


def test_strided_batch_gives_the_same_bits(ops, dev, problems):
    names = ["42_9", "43_0", "42_19", "44_9", "43_19"]
    Us = np.stack([problems[f"U_{n}"] for n in names])
    base = Us.mean(axis=2)
    masks = maximin_ref.coalition_masks(6)[::5]
    res = ops.maximin_lottery(_cuda(Us, dev), _cuda(base, dev), masks)
    big = torch.zeros((10, 8, 90), dtype=torch.float64, device=dev)
    big[::2, :6, :81] = _cuda(Us, dev)
    strided = ops.maximin_lottery(big[::2, :6, :81], _cuda(base, dev), masks)
    for key in ("alpha", "q", "lam", "pivots"):
        assert torch.equal(res[key], strided[key]), key
    assert int(res["pivots"].min()) >= 1


# 4 ---------------------------------------------------------------------------------------
def test_degenerate_cases_terminate(ops, dev):
    for name, U, base, masks in _degenerate_cases():
        res = _np(ops.maximin_lottery(_cuda(U, dev), None if base is None else _cuda(base, dev),
                                      masks))
        for ci, mask in enumerate(masks):
            what = f"{name} mask {mask:#x}"
            ref = _ref((name, mask), U, base, mask)
            assert 0 <= res["pivots"][ci] == ref["pivots"], what
            assert abs(res["alpha"][ci] - ref["alpha"]) <= GAP_TOL * ref["alpha"], what
            _certify(U, base, mask, res["alpha"][ci], res["q"][ci], res["lam"][ci], what)
            if name == "ones":          # value exactly 1
                assert res["alpha"][ci] == bin(mask).count("1") / 6.0, what
    # no pivots allowed: -2 and NaN wherever one is needed
    U = _cuda(_rand_u(9, 4, 33), dev)
    z = ops.maximin_lottery(U, masks=[0b1111, 0b0001], max_pivots=0)
    assert z["pivots"].tolist() == [-2, -2]
    assert bool(torch.isnan(z["alpha"]).all()) and bool(torch.isnan(z["q"]).all())
    assert bool(torch.isnan(z["lam"]).all())
    one = ops.maximin_lottery(U, masks=[0b1111, 0b0001], max_pivots=1)
    assert one["pivots"].tolist() == [-2, 1]            # a single agent needs exactly one
    best = 0.25 * float(U[0].max())                      # 1 / (1 / max) may be an ulp off
    assert bool(torch.isnan(one["alpha"][0])) and abs(float(one["alpha"][1]) - best) <= 4.5e-16 * best
    col = ops.maximin_lottery(U[:, :1], max_pivots=0)    # one column needs none
    assert int(col["pivots"]) == 0 and float(col["alpha"]) == float(U[:, 0].min())


# 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["nan", "inf", "negative", "zero_row", "zero_base", "nan_base"])
def test_bad_problem_does_not_disturb_its_neighbours(ops, dev, defect):
    Us = np.stack([_rand_u(s, 6, 81) for s in (21, 22, 23)])
    base = Us.mean(axis=2)
    masks = maximin_ref.coalition_masks(6)
    agent = None                                     # None: every coalition of problem 1 fails
    if defect == "nan":
        Us[1, 3, 17] = float("nan")
    elif defect == "inf":
        Us[1, 5, 0] = float("inf")
    elif defect == "negative":
        Us[1, 0, 80] = -1e-3
    elif defect == "zero_row":
        Us[1, 4, :] = 0.0
        agent = 4
    elif defect == "zero_base":
        base[1, 2] = 0.0
        agent = 2
    else:
        base[1, 2] = float("nan")
        agent = 2
    Ut, bt = _cuda(Us, dev), _cuda(base, dev)
    res = ops.maximin_lottery(Ut, bt, masks)                       # raises unless CS_OK
    hit = np.array([agent is None or bool((int(mk) >> agent) & 1) for mk in masks])
    assert 0 < hit.sum() and (agent is None or hit.sum() == 32)
    piv = res["pivots"][1].cpu().numpy()
    assert np.array_equal(piv == -1, hit) and (piv[~hit] >= 1).all()
    hit_t = torch.as_tensor(hit, device=dev)
    assert bool(torch.isnan(res["alpha"][1][hit_t]).all())
    assert bool(torch.isnan(res["q"][1][hit_t]).all()) and bool(torch.isnan(res["lam"][1][hit_t]).all())
    if agent is not None:
        # the coalitions without that agent are solved, with the bits they get alone
        rest = masks[~hit]
        alone = ops.maximin_lottery(Ut[1], bt[1], rest)
        for key in ("alpha", "q", "lam", "pivots"):
            assert torch.equal(res[key][1][~hit_t], alone[key]), key
        ci = int(np.flatnonzero(~hit)[-1])
        a, q, lam = (res[k][1, ci].cpu().numpy() for k in ("alpha", "q", "lam"))
        _certify(np.where(np.isfinite(Us[1]), Us[1], 0.0), np.where(base[1] > 0, base[1], 1.0),
                 int(masks[ci]), float(a), q, lam, defect)
    for k in (0, 2):
        alone = ops.maximin_lottery(Ut[k], bt[k], masks)
        for key in ("alpha", "q", "lam", "pivots"):
            assert torch.equal(res[key][k], alone[key]), (key, k)
        assert int(alone["pivots"].min()) >= 1
    # the process is healthy afterwards
    torch.cuda.synchronize()
    assert float((Ut[0] * 2).sum()) > 0


# 6 ---------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(ops, dev, golden, problems):
    nine = [str(n) for n in golden["cases"] if problems[f"U_{n}"].shape == (6, 81)]
    Us = _cuda(np.stack([problems[f"U_{n}"] for n in nine]), dev)
    base = Us.mean(dim=2)
    masks = maximin_ref.coalition_masks(6)
    a = ops.maximin_lottery(Us, base, masks)
    b = ops.maximin_lottery(Us, base, masks)
    for key in ("alpha", "q", "lam", "pivots"):
        assert torch.equal(a[key], b[key]), key
    assert int(a["pivots"].min()) >= 1
    big = _cuda(_rand_u(77, 16, 4096), dev)
    a, b = ops.maximin_lottery(big), ops.maximin_lottery(big)
    for key in ("alpha", "q", "lam", "pivots"):
        assert torch.equal(a[key], b[key]), key


# 7 ---------------------------------------------------------------------------------------
def test_sweep_is_one_launch_of_each_solver(core, ops, golden, monkeypatch):
    calls = {"nash_lottery": 0, "maximin_lottery": 0}
    for fn in calls:
        def counted(*a, _plain=getattr(ops, fn), _fn=fn, **k):
            calls[_fn] += 1
            return _plain(*a, **k)
        monkeypatch.setattr(ops, fn, counted)
    rho = np.linspace(0.6, 5.0, 20)[[0, 19]]                  # core.py:348
    table = core.coalition_sweep(3, 4, 8, 6, (42, 43), rho)   # core.py:342-344
    assert calls == {"nash_lottery": 1, "maximin_lottery": 1}
    for key in ("nash", "utilitarian", "uniform"):
        assert table[key].shape == (2, 2)
    for si, seed in enumerate((42, 43)):
        for ri, r in enumerate((0, 19)):
            want = golden[f"maxalpha_{seed}_{r}"]
            got = [table[k][si, ri] for k in ("nash", "utilitarian", "uniform")]
            print(f"seed {seed} rho {rho[ri]:.2f}: {got} (reference {want.tolist()})")
            assert (np.abs(np.array(got) - want) <= ALPHA_TOL * want).all(), (seed, r)
