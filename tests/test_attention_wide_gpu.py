"""cs_prefix_attention's wide tile (prefix_attn_wide_kernel: 32 query rows per wave over
64-key blocks) at its mask edges, its missing second tiles and through its softmax rescale,
on the cases of tests/attention_wide_cases.py (tests/test_attention_wide_cases_host.py proves
on the CPU that every planted case would catch the mask mutants it is aimed at).

Every case runs the plain route (no plan) and is held to |out - ref| <= 2^-7 A + 1e-30 against
the fp64 reference (A = sum p |v|, derivation in attention_ref.py), and to a bit-identical
relaunch.  Each test prints its worst err / bound (pytest -s)."""
import numpy as np
import pytest
import torch

import attention_ref as R
import attention_wide_cases as W

pytestmark = pytest.mark.gpu


class Plain:
    """The case's tensors on the device and the no-plan launch."""

    def __init__(self, ops, dev, c, bufs=None):
        self.ops, self.c = ops, c
        kf, vf, kh, vh = bufs if bufs else (c.kflat, c.vflat, c.kh, c.vh)
        self.q = c.q.to(dev)
        self.kflat, self.vtflat = kf.to(dev), ops.blocked_vt(vf.to(dev))
        self.kh, self.vth = kh.to(dev), ops.blocked_vt(vh.to(dev))
        self.offt = torch.tensor(c.off, dtype=torch.int64, device=dev)
        self.plen = torch.tensor(c.plens, dtype=torch.int32, device=dev)
        self.hbt = torch.tensor([c.hb], dtype=torch.int32, device=dev)
        self.gp = None if c.gmap is None else torch.tensor(c.gmap, dtype=torch.int32, device=dev)
        self.plan = ops.AttnPlan(None, 0, 0, None)

    def run(self):
        c = self.c
        return self.ops.prefix_attention(
            self.q, self.kflat, self.vtflat, self.offt, self.plen, max(c.plens), self.kh, self.vth,
            self.hbt, c.n_str, c.T, scale=c.scale, softcap=0.0, window=0, group_prefix=self.gp,
            plan=self.plan)


def _hold_to_bound(ops, dev, c, bufs=None):
    ref, A = R.reference(c)
    r = Plain(ops, dev, c, bufs)
    out, again = r.run(), r.run()
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool(torch.isfinite(o.float()).all()), f"{c}: non-finite output"
    worst = float(R.err_over_bound(o, ref, A).max())
    print(f"\n[attn-wide] {c.family} {c.name}: {worst:.3f} x the bound")
    assert worst <= 1.0, f"{c}: {worst:.2f} x the bound"
    assert torch.equal(out, again), f"{c}: relaunch differs"
    return out


@pytest.mark.parametrize("c", W.cases("prefix"), ids=repr)
def test_prefix_edges(ops, dev, c):
    out = _hold_to_bound(ops, dev, c)
    if c.checks[0][0] != "limit-1":                   # the empty prefix: no visible plant
        return
    _, tok, head = c.checks[0]                        # the visible plant: out is its V row
    v = c.vflat[0, c.off[1] + c.plens[1] - 1].float()
    assert float((out[tok, head].cpu().float() - v).abs().max()) <= 2.0 ** -7 * float(v.abs().max())


def test_missing_second_tile(ops, dev):
    """the last prefix padded to 96 keys and ld_hist = 96: zeros against +-1e30 (finite bf16)
    in every K / V slot no query may see give bitwise the same finite output, in the bound"""
    c = W.cases("missing")[0]
    lay = R.rows_layout(c)
    outs = {v: _hold_to_bound(ops, dev, c, R.fill_invisible(c, lay, v)[:4]) for v in (0.0, 1e30)}
    assert torch.equal(outs[0.0], outs[1e30]), f"{c}: an invisible slot reached the output"


@pytest.mark.parametrize("c", W.cases("history"), ids=repr)
def test_history_edges(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", W.cases("span"), ids=repr)
def test_tiles_that_span_streams(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", W.cases("stairs"), ids=repr)
def test_rescale_staircase(ops, dev, c):
    _hold_to_bound(ops, dev, c)


@pytest.mark.parametrize("c", W.cases("offset"), ids=repr)
def test_score_offsets(ops, dev, c):
    _hold_to_bound(ops, dev, c)


def test_both_sides_of_the_rule_agree(ops, dev):
    """T = 31 (the narrow tile) against T = 32 (the wide one) on the 31 tokens per stream they
    share: each within the bound of its reference, and of each other"""
    c31, c32 = W.cases("rule")
    o31 = _hold_to_bound(ops, dev, c31).cpu()
    o32 = _hold_to_bound(ops, dev, c32).cpu()
    _, A = R.reference(c31)
    shared = o32.reshape(c32.S, 32, c32.H, c32.D)[:, :31].reshape(-1, c32.H, c32.D)
    worst = float(R.err_over_bound(o31, shared.float().numpy().astype(np.float64), A).max())
    print(f"\n[attn-wide] rule T31 vs T32: {worst:.3f} x the bound")
    assert worst <= 1.0, f"T = 31 and T = 32 differ by {worst:.2f} x the bound"
