"""cs_prefix_attention at its mask edges and through its softmax rescale, on inputs whose
answer ONE key decides (tests/attention_ref.py; tests/test_attention_cases_host.py proves on
the CPU that every case here would catch the mutant it is aimed at).

Every case runs through four routes and each is held to |out - ref| <= 2^-7 A + 1e-30
against the fp64 reference (A = sum p |v|, derivation in attention_ref.py):
  plain      no plan (prefix_attn_lds_kernel)
  split      a work plan with key splits (prefix_attn_plan_lds_kernel + attn_merge_kernel)
  rows+plan  the row-layout history behind a slot table, the same plan
  rows       the row-layout history, no plan
The split plans come from exact host lengths with 64 query rows per cell, or from inflated
host bounds (most splits then hold no key at all: empty partials the merge must weight 0);
each test asserts the plan it got is the one the planner restatement predicts.

Families: a. prefix limit, b. history limit (own key, next token's key, the neighbour
stream in the same tile), c. window edge and two exact window identities, d. staircases
(rescale, wave combine, split merge), e. invisible slots are inert (zeros vs +-1e30 there:
bitwise equal outputs), f. scores around -200 / +200 nats.  Every case also asserts a
bit-identical relaunch.  Each test prints its worst err / bound per route (pytest -s)."""
import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

ROUTES = ("plain", "split", "rows+plan", "rows")


class Routes:
    """The case's tensors on the device and the four launches."""

    def __init__(self, ops, dev, c, bufs=None):
        self.ops, self.c = ops, c
        lay = R.rows_layout(c)
        kf, vf, kh, vh, kr, vr = bufs(lay) if bufs else (c.kflat, c.vflat, c.kh, c.vh, lay[0], lay[1])
        self.q = c.q.to(dev)
        self.kflat, self.vtflat = kf.to(dev), ops.blocked_vt(vf.to(dev))
        self.kh, self.vth = kh.to(dev), ops.blocked_vt(vh.to(dev))
        self.kr, self.vr, self.table = kr.to(dev), vr.to(dev), lay[2].to(dev)
        self.offt = torch.tensor(c.off, dtype=torch.int64, device=dev)
        self.plen = torch.tensor(c.plens, dtype=torch.int32, device=dev)
        self.hbt = torch.tensor([c.hb], dtype=torch.int32, device=dev)
        self.gp = None if c.gmap is None else torch.tensor(c.gmap, dtype=torch.int32, device=dev)
        self.mpl = max(c.plens)
        # the split plan, and that it is the plan meant: the planner restatement's splits
        self.plan = ops.attention_plan(c.host_lens, c.gmap, c.n_grp, c.n_str, c.T, c.H, c.Hkv, c.D,
                                       c.ldh, dev)
        assert self.plan.entries is not None and self.plan.n_merge > 0
        cells, na, nm = R.plan_cells(c)
        assert (self.plan.n_attn, self.plan.n_merge) == (na, nm)
        ent = self.plan.entries.cpu().numpy()[:na]
        got = {(int(e[0]) // c.Hkv, int(e[1])): int(e[2]) >> 8 for e in ent}
        assert got == cells
        self.plain = ops.AttnPlan(None, 0, 0, None)
        assert self.plain.entries is None
        self.shape = f"n_attn {na} n_merge {nm} splits/cell {sorted(set(cells.values()))}"

    def run(self, route, window=None):
        c = self.c
        rows = route.startswith("rows")
        return self.ops.prefix_attention(
            self.q, self.kflat, self.vtflat, self.offt, self.plen, self.mpl,
            self.kr if rows else self.kh, self.vr if rows else self.vth, self.hbt, c.n_str, c.T,
            scale=c.scale, softcap=c.cap, window=c.window if window is None else window,
            group_prefix=self.gp, plan=self.plan if route in ("split", "rows+plan") else self.plain,
            hist_rows=self.table if rows else None)


def _hold_to_bound(ops, dev, c):
    ref, A = R.reference(c)
    r = Routes(ops, dev, c)
    outs = {route: r.run(route) for route in ROUTES}
    again = {route: r.run(route) for route in ROUTES}
    torch.cuda.synchronize()
    worst = {}
    for route in ROUTES:
        o = outs[route].cpu()
        assert bool(torch.isfinite(o.float()).all()), f"{c} [{route}]: non-finite output"
        worst[route] = float(R.err_over_bound(o, ref, A).max())
    print(f"\n[attn-edges] {c.family} {c.name}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" | {r.shape}")
    for route in ROUTES:
        assert worst[route] <= 1.0, f"{c} [{route}]: {worst[route]:.2f} x the bound"
        assert torch.equal(outs[route], again[route]), f"{c} [{route}]: relaunch differs"
    return outs


@pytest.mark.parametrize("c", R.cases("a"), ids=repr)
def test_prefix_limit(ops, dev, c):
    outs = _hold_to_bound(ops, dev, c)
    mut, tok, head = c.checks[0]
    if mut != "limit-1":                              # the empty prefix: no visible plant
        return
    p = c.prefix_of(tok // c.T)                       # the visible plant: out is its V row
    v = c.vflat[0, c.off[p] + c.plens[p] - 1].float()
    for route in ROUTES:
        assert float((outs[route][tok, head].cpu().float() - v).abs().max()) <= 2.0 ** -7 * float(v.abs().max())


@pytest.mark.parametrize("c", R.cases("b"), ids=repr)
def test_history_limit(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", R.cases("c"), ids=repr)
def test_window_edge(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", R.cases("ci"), ids=repr)
def test_window_of_one_returns_the_own_value_row(ops, dev, c):
    """window = 1: only the token's own key is visible, p = 1 and l = 1 exactly, so the
    output is V_hist[s, h // rep, hb + t] bit for bit"""
    r = Routes(ops, dev, c)
    want = torch.empty_like(c.q)
    for s in range(c.S):
        for t in range(c.T):
            want[s * c.T + t] = c.vh[s, :, c.hb + t].repeat_interleave(c.rep, dim=0)
    for route in ROUTES:
        out = r.run(route, window=1)
        assert torch.equal(out.cpu(), want), route
        assert torch.equal(out, r.run(route, window=1)), route
    print(f"\n[attn-edges] c {c.name} window=1: exact | {r.shape}")


@pytest.mark.parametrize("c", R.cases("ci"), ids=repr)
def test_window_over_every_position_is_no_window(ops, dev, c):
    r = Routes(ops, dev, c)
    full = max(c.plens) + c.hb + c.T
    for route in ROUTES:
        base = r.run(route, window=0)
        for w in (full, full + 1000, 2 ** 31 - 1):
            assert torch.equal(r.run(route, window=w), base), (route, w)
    # one position short hides prefix key 0 from the longest prefix's last token: not equal
    assert not torch.equal(r.run("plain", window=full - 1), r.run("plain", window=0))
    print(f"\n[attn-edges] c {c.name} window>=all: exact | {r.shape}")


@pytest.mark.parametrize("c", R.cases("d"), ids=repr)
def test_staircase(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", R.cases("e"), ids=repr)
def test_invisible_slots_are_inert(ops, dev, c):
    """zeros against +-1e30 (finite bf16) in every K / V slot no query may see: bitwise the
    same output on every route, finite, and within the bound"""
    ref, A = R.reference(c)
    runs = {}
    for value in (0.0, 1e30):
        r = Routes(ops, dev, c, bufs=lambda lay, v=value: R.fill_invisible(c, lay, v))
        runs[value] = {route: r.run(route) for route in ROUTES}
        again = {route: r.run(route) for route in ROUTES}
        for route in ROUTES:
            assert torch.equal(runs[value][route], again[route]), (route, value)
    torch.cuda.synchronize()
    worst = {}
    for route in ROUTES:
        z, h = runs[0.0][route], runs[1e30][route]
        assert bool(torch.isfinite(h.float()).all()), f"{c} [{route}]: non-finite output"
        assert torch.equal(z, h), f"{c} [{route}]: an invisible slot reached the output"
        worst[route] = float(R.err_over_bound(h.cpu(), ref, A).max())
    print(f"\n[attn-edges] e {c.name}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" | {r.shape}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("c", R.cases("f"), ids=repr)
def test_score_offsets(ops, dev, c):
    _hold_to_bound(ops, dev, c)
