"""The power of the attention edge cases (tests/attention_ref.py), on the CPU: these tests
check the CASES that tests/test_attention_edges_gpu.py runs, not the kernel.

Every planted-key and staircase case names the mutants it is aimed at.  A mask mutant
(limit +- 1, window edge +- 1, the neighbour streams' history or a future slot made
visible) is applied to the fp64 reference; an arithmetic mutant (no rescale, the rescale
applied to l only, combine weight 1 everywhere) to the NumPy restatement of the kernel's
order of operations, under every block order of the four routes it is meant for.  Each
must move the targeted output row by >= 16 x the bound the GPU test holds the kernel to,
so a kernel with that fault cannot pass.  The unmutated restatement must stay inside the
bound.  No case is skipped or filtered: a case that cannot discriminate fails here."""
import numpy as np
import pytest

import attention_ref as R

FAMILIES = ("a", "b", "c", "d", "e", "f")
ALL = [c for f in FAMILIES for c in R.cases(f)]
ORDERS = ("lds", "plan", "plan1")


@pytest.mark.parametrize("c", ALL, ids=repr)
def test_case_splits_and_restatement_stays_within_bound(c):
    plan = R.plan_cells(c)
    assert plan is not None and plan[2] > 0 and max(plan[0].values()) > 1    # a split plan
    ref, A = R.reference(c)
    assert np.isfinite(ref).all()
    for order in ORDERS:
        out = R.emulate(c, order)
        assert np.isfinite(out).all()
        worst = float(R.err_over_bound(out, ref, A).max())
        assert worst <= 1.0, f"{c} [{order}]: restatement at {worst:.2f} x the bound"


@pytest.mark.parametrize("c", [c for c in ALL if c.family in "abcd"], ids=repr)
def test_case_catches_its_mutants(c):
    ref, A = R.reference(c)
    assert c.checks, f"{c}: a case with nothing to catch"
    for chk in c.checks:
        mut, tok, head = chk[:3]
        bound = R.bound_of(A[tok, head])
        if mut in R.REF_MUTANTS:
            got = [("fp64", R.reference(c, mut)[0])]
        else:
            got = [(o, R.emulate(c, o, mut).astype(np.float64)) for o in (chk[3] if len(chk) > 3 else ORDERS)]
        for what, out in got:
            ratio = float((np.abs(out[tok, head] - ref[tok, head]) / bound).max())
            assert ratio >= 16.0, f"{c}: mutant {mut} [{what}] moves row ({tok}, {head}) by " \
                                  f"{ratio:.1f} x the bound only"


def test_every_mutant_has_a_case():
    used = {chk[0] for c in ALL for chk in c.checks}
    assert used == set(R.REF_MUTANTS) | set(R.EMU_MUTANTS)


def test_planted_key_decides_the_row():
    """a visible plant gives the planted V row, an invisible one leaves the background
    average: the first prefix-limit case with both"""
    c = next(c for c in R.cases("a") if len(c.checks) == 2)
    ref, _ = R.reference(c)
    (_, tok, h_vis), (_, _, h_inv) = c.checks
    p = c.prefix_of(tok // c.T)
    v_vis = c.vflat[0, c.off[p] + c.plens[p] - 1].float().numpy()
    assert np.abs(ref[tok, h_vis] - v_vis).max() < 1e-6 * np.abs(v_vis).max()
    assert np.abs(ref[tok, h_inv]).max() < 1.0 < np.abs(v_vis).mean()


def test_reference_matches_the_fp32_torch_reference():
    """the vectorised fp64 reference against a direct per-row softmax (window, cap, map)"""
    c = R.cases("c")[1]
    ref, _ = R.reference(c)
    q, kf, vf, kh, vh = (x.double().numpy() for x in (c.q, c.kflat, c.vflat, c.kh, c.vh))
    for tok, head in [(0, 0), (c.S * c.T - 1, c.H - 1), (c.checks[0][1], c.checks[0][2])]:
        s, t, g = tok // c.T, tok % c.T, head // c.rep
        p = c.prefix_of(s)
        P = c.plens[p]
        keys = [(kf[g, c.off[p] + j], vf[g, c.off[p] + j], j) for j in range(P)]
        keys += [(kh[s, g, j], vh[s, g, j], P + j) for j in range(c.hb + t + 1)]
        qpos = P + c.hb + t
        sc, vs = [], []
        for k, v, pos in keys:
            if c.window > 0 and qpos - pos >= c.window:
                continue
            x = float(q[tok, head] @ k) * c.scale
            sc.append(c.cap * np.tanh(x / c.cap) if c.cap > 0 else x)
            vs.append(v)
        w = np.exp(np.array(sc) - max(sc))
        want = (w[:, None] * np.array(vs)).sum(0) / w.sum()
        assert np.abs(want - ref[tok, head]).max() <= 1e-9 * max(1.0, np.abs(want).max())
