"""cs_rope_place, cs_rope_place_rows, cs_rope_place_splitk and cs_rope_place_splitk_rows
(csrc/attn.hip) against the float64 reference of tests/rope_ref.py, per item path, slot and
split count.  tests/test_rope_cases_host.py shows on the CPU what these checks are worth: the
rounding windows are one value on all but 0.26 % of the elements at most, the kernel's own
arithmetic with sin / cos 2 fp32 ulps off stays inside them, and each of ten subtly wrong
kernels is rejected by a case that runs here.

Every launch writes into q_out, k_hist and vt_hist views that start 16 bytes (not 32) past a
guard inside larger buffers filled with 0x5A5A: slots [hb, hb + T) must hold the expected
values and every other element, inside the views and in the guards, must still be the
sentinel.  V is any 16-bit pattern and is compared as bits.

  random_cases        the real tables (llama-3.1-8b D 128, gemma-2-9b D 256, tiny-llama):
                      8-pair items with 1 and 2 workgroups per token, 4-pair items by a
                      4-element column offset (up to 5 workgroups per token) and by head_dim
                      8 / 24 / 40, per-token slots across the 32-slot V tile boundary in both V
                      layouts, the tile path with ragged and aligned 8-slot groups, T >= 32 on
                      the per-token path, positions 0 .. 2^17 + 44, group maps
  zero / quarter      planted tables, bit for bit; a failing quarter-turn family names the
                      frequency index each pair used
  fold                splits 1 .. 17 (every surplus-lane count of the 2-, 4- and 8-wide chunks,
                      a second and third chunk): windows on a real table, bits on the zero
                      table, and bitwise cs_rope_place of the folded projection
  tile == per-token   (hb, T) = (5, 40): the same bits by tiles, by 8-pair items (rows V) and
                      by 4-pair items (column offset 4, ld_qkv % 8 == 4)"""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import rope_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096 + 8          # elements: the views are 16-byte, not 32-byte, aligned


def _guarded(dev, shape):
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), R.SENT16, dtype=torch.int16, device=dev)
    view = buf[GUARD:GUARD + n].view(torch.bfloat16).view(shape)
    assert view.data_ptr() % 32 == 16
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _launch(ops, dev, c, x=None):
    """One launch of case c (x: other projection bits [n_tok, nh, D], as a bf16 projection in
    c's buffer layout).  Returns the uint16 (q_out, k_hist, vt_hist); the guards are checked."""
    cx, part = c.inputs()
    if x is not None:
        cx, part = x, None
    if part is not None:
        src = ops.SplitPartials(torch.from_numpy(part.copy()).to(dev))
    else:
        buf = torch.full((c.n_tok, c.width + c.ldpad), R.SENT16, dtype=torch.int16, device=dev)
        buf[:, c.col0:c.col0 + c.width] = torch.from_numpy(
            np.array(cx).reshape(c.n_tok, c.width).view(np.int16)).to(dev)
        src = buf.view(torch.bfloat16)[:, c.col0:c.col0 + c.width]
        if c.n_tok == 1:
            src = src.contiguous()
        assert src.data_ptr() % 16 == 2 * c.col0 % 16
    inv = torch.from_numpy(c.inv_freq()).to(dev)
    plen = torch.tensor(c.plen, dtype=torch.int32, device=dev)
    hb = torch.tensor([c.hb], dtype=torch.int32, device=dev)
    gp = None if c.gp is None else torch.tensor(c.gp, dtype=torch.int32, device=dev)
    bufs = [_guarded(dev, s) for s in ((c.n_tok, c.H, c.D), (c.S, c.Hkv, c.ldh, c.D), R.v_shape(c))]
    (_, q), (_, kh), (_, vh) = bufs
    ops.rope_place(src, inv, plen, hb, c.n_str, c.T, c.H, c.Hkv, c.D, q, kh, vh, group_prefix=gp,
                   v_rows=c.v_rows)
    torch.cuda.synchronize()
    for what, (buf, view) in zip(("q_out", "k_hist", "vt_hist"), bufs):
        n = view.numel()
        assert bool((buf[:GUARD] == R.SENT16).all()) and bool((buf[GUARD + n:] == R.SENT16).all()), \
            f"{c}: a store outside the {what} buffer"
    return _bits(q), _bits(kh), _bits(vh)


def _same(a, b, what):
    for name, x, y in zip(("q_out", "k_hist", "vt_hist"), a, b):
        if not np.array_equal(x, y.reshape(x.shape)):
            bad = np.argwhere(x != y.reshape(x.shape))
            pytest.fail(f"{what}: {name} differs in {len(bad)} elements, first at {tuple(bad[0])}")


def _run(ops, dev, c):
    out = _launch(ops, dev, c)
    errs = R.check(c, *out)
    assert not errs, "\n".join(errs)
    _same(out, _launch(ops, dev, c), f"{c}: relaunch")
    return out


@pytest.mark.parametrize("c", R.random_cases(), ids=str)
def test_real_tables_round_correctly_into_the_right_slots(ops, dev, c):
    _run(ops, dev, c)


@pytest.mark.parametrize("c", R.zero_cases(), ids=str)
def test_zero_table_returns_the_input_bits(ops, dev, c):
    _run(ops, dev, c)


@pytest.mark.parametrize("fam", R.quarter_families(), ids=lambda f: f[-1].name)
def test_quarter_turns_tell_every_frequency_index_apart(ops, dev, fam):
    outs = [_launch(ops, dev, c) for c in fam]
    errs = [e for c, o in zip(fam, outs) for e in R.check(c, *o)]
    if errs:
        used = R.decode_freq_index(fam, [o[0] for o in outs])
        wrong = np.argwhere(used != np.arange(fam[0].half))
        if len(wrong):
            tok, h, j = wrong[0]
            errs.append(f"q_out token {tok} head {h}: pair {j} was turned by frequency index "
                        f"{used[tok, h, j]} ({len(wrong)} pairs used another index than their own)")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c", R.fold_cases(), ids=str)
def test_fold_sums_the_splits_in_order_and_no_surplus_lane(ops, dev, c):
    out = _run(ops, dev, c)                           # the windows, on the case's real table
    z = R.zero_table(c)
    zout = _launch(ops, dev, z)                       # bit for bit the fp32 fold, rounded
    errs = R.check(z, *zout)
    assert not errs, "\n".join(errs)
    x, _ = c.inputs()
    folded = replace(c, name=c.name + "-folded", splits=0, plant="")
    _same(out, _launch(ops, dev, folded, x=x), f"{c}: cs_rope_place of the folded projection")


@pytest.mark.parametrize("item", R.ITEMS8, ids=lambda it: f"D{it[0]}H{it[1]}k{it[2]}")
def test_tile_path_and_per_token_paths_give_the_same_bits(ops, dev, item):
    D, H, Hkv, table = item
    c = [c for c in R.random_cases() if c.name == f"tile-D{D}H{H}k{Hkv}-hb5T40ld64"][0]
    assert c.path()[2]
    x, _ = c.inputs()
    out = _launch(ops, dev, c)
    assert not R.check(c, *out)
    for tag, kw in (("4-pair items, column offset 4", dict(col0=4, ldpad=8)),
                    ("4-pair items, ld_qkv % 8 == 4", dict(ldpad=4))):
        other = replace(c, name=f"{c.name} ({tag})", **kw)
        assert other.path()[0] == 4 and not other.path()[2]
        _same(out, _launch(ops, dev, other, x=x), str(other))
    rows = replace(c, name=c.name + " (rows V)", v_rows=True)
    rq, rk, rv = _launch(ops, dev, rows, x=x)
    assert not R.check(rows, rq, rk, rv)
    blocked = out[2].reshape(c.S, c.Hkv, c.ldh // 32, c.D, 32).transpose(0, 1, 2, 4, 3).reshape(rv.shape)
    _same((out[0], out[1], blocked), (rq, rk, rv), str(rows))
