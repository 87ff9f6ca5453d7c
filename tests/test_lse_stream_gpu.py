"""The vocab log-sum-exp stream (block_lse_partial and the split merge behind
cs_logsoftmax_gather, cs_beam_step) pinned with planted rows at every position class.

Every row of a launch is one probe of tests/lse_ref.py: a counting row, a one-hot row, a
late maximum, a saturated plant under the soft-cap, a NaN, or a random row, with the plant at a
position where one of the kernel's code paths begins or ends.  References are float64, windows
are derived in lse_ref.py from the kernel's arithmetic (tests/test_lse_cases_host.py shows that
an fp32 restatement fits them and that they reject ten wrong kernels).  Logits live in a larger
buffer whose pad columns and bands hold NaN (or a huge finite value), outputs in 0x5A-filled
buffers whose surroundings must not change.

Measured on an MI355X: the file's 171 tests (2,678 planted launches and the dense ones) take
11 s, the slowest 0.7 s (the dense random rows of the widest unsplit case, most of it the float64
reference on the host); the kernels use at most 0.57 of a planted row's window and 0.19 of a
random row's."""
import numpy as np
import pytest
import torch

import lse_ref as R

pytestmark = pytest.mark.gpu

TORCH = {R.F32: torch.float32, R.BF16: torch.bfloat16, R.F16: torch.float16}
CASES = {c.name: c for c in R.all_cases()}
SWEPT = ("onehot0", "latemax", ("nan_inf", 0.0))          # planted at every class of every row
TWICE = ("onehot3.5", "onehot-80", "sat30+", "sat30-", "sat75+", "sat75-", ("nan_inf", 30.0),
         ("nan_inf", 75.0))


def _logits(L, dev):
    """The launch's logits on the device: a [rows, ld] view into the poisoned buffer."""
    c = L.case
    dt = TORCH[c.dtype]
    nbuf, first = max(c.view_of, c.rows), c.first
    start = R.BAND + (c.base_off if c.pad else 0)
    poison = L.poison if np.isnan(L.poison) or c.dtype != R.F16 else 65504.0
    flat = torch.full((start + nbuf * c.ld + R.BAND + c.epv,), poison, dtype=dt, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[start:start + nbuf * c.ld].view(nbuf, c.ld)[first:first + c.rows]
    if L.dense is not None:
        view[:, :c.V] = torch.from_numpy(L.dense).to(dev)
    else:
        view[:, :c.V] = torch.from_numpy(L.bg.astype(np.float32)).to(dev)[:, None]
    for col, val in ((L.plant_col, L.plant_val), (L.nan_col, np.full(c.rows, np.nan))):
        r = np.nonzero(col >= 0)[0]
        if len(r):
            view[torch.from_numpy(r).to(dev), torch.from_numpy(col[r]).to(dev)] = \
                torch.from_numpy(val[r].astype(np.float32)).to(dev).to(dt)
    return view


def _guarded(n, dev):
    """n float32 inside a 0x5A-filled byte buffer: (the buffer, the contiguous slice)."""
    buf = torch.full((2 * R.GUARD + 4 * n,), R.FILL, dtype=torch.uint8, device=dev)
    return buf, buf[R.GUARD:R.GUARD + 4 * n].view(torch.float32)


def _untouched(buf, n):
    g = torch.cat([buf[:R.GUARD], buf[R.GUARD + 4 * n:]])
    return bool((g == R.FILL).all())


def _run(ops, dev, L):
    """The launch through ops.logsoftmax_gather: (failures, share of the window used)."""
    c = L.case
    x = _logits(L, dev)
    tgt = torch.from_numpy(L.targets).to(dev) if c.k else None
    obuf, out = _guarded(c.rows * c.k, dev)
    lbuf, lse = _guarded(c.rows, dev)
    tok, lse2 = ops.logsoftmax_gather(x, tgt, vocab=c.V, softcap=L.cap, lse_out=lse,
                                      out=out.view(c.rows, c.k) if c.k else None)
    assert lse2.data_ptr() == lse.data_ptr()
    bad, frac = R.check(L, lse.cpu().numpy(), tok.cpu().numpy())
    if not (_untouched(obuf, c.rows * c.k) and _untouched(lbuf, c.rows)):
        bad.append(f"{c.name}/{L.kind}: bytes around out= or lse_out= changed")
    return bad, frac


def _kind(k):
    return k if isinstance(k, tuple) else (k, None)


@pytest.mark.parametrize("name", list(CASES))
def test_planted_rows(ops, dev, name):
    """Counting rows, then every planted kind: one-hot (c = 0), late-maximum and NaN rows at
    every class of every alignment, the other kinds over two stretches of the class list."""
    c = CASES[name]
    n = R.n_shifts(c) if c.rows >= 64 else 3
    if c.k > 65:
        n = min(n, 2)
    todo = [("count", None, 0)]
    todo += [(*_kind(k), s) for k in SWEPT for s in range(n)]
    todo += [(*_kind(k), s + i) for i, k in enumerate(TWICE) for s in range(min(n, 2))
             if c.k <= 65]
    bad, worst = [], 0.0
    for kind, cap, shift in todo:
        b, f = _run(ops, dev, R.make_launch(c, kind, shift, cap=cap))
        bad += b
        worst = max(worst, f)
    print(f"{name}: {len(todo)} launches, worst share of a window {worst:.2f}")
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:20])


DENSE = [(f"{dt}-{nm}", full) for dt in R.DTYPES for nm, full in
         (("u-nvec1", True), ("u-nvec1025", True), ("u-nvec4097", False), ("u-view300", False),
          ("u-aligned", False), ("u-V7", True),
          (f"s-V{R.SPLIT_V[dt][0]}-r3", True), (f"s-V{R.SPLIT_V[dt][2]}-r3", True),
          (f"s-V{R.SPLIT_V[dt][-1]}-r64", False), ("s-aligned", False), ("s-k65", False))]


@pytest.mark.parametrize("name,full", DENSE, ids=[d[0] for d in DENSE])
def test_random_rows_in_a_derived_window(ops, dev, name, full):
    """randn * 3 rows, rows with a 100-wide -inf mask and rows with one NaN (every second row
    clean) against the float64 reference, inside the derived window instead of 1e-3; once more
    with a huge finite value instead of NaN in the pad columns and bands."""
    c = CASES[name]
    todo = [("random", 0.0, float("nan")), ("random", 0.0, 3e38), ("nan_randn", 0.0, float("nan"))]
    if full:
        todo += [(k, cap, float("nan")) for k in ("random", "masked", "nan_randn")
                 for cap in R.CAPS if (k, cap) not in (("random", 0.0), ("nan_randn", 0.0))]
    bad, worst = [], 0.0
    for kind, cap, poison in todo:
        L = R.make_launch(c, kind, 1, cap=cap, poison=poison)
        assert L.win_lse[~L.nan_row].max() < (3e-5 if cap == 0.0 else 2e-4)
        b, f = _run(ops, dev, L)
        bad += b
        worst = max(worst, f)
    print(f"{name}: worst share of a window {worst:.2f}")
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("name", [f"{dt}-{nm}" for dt in R.DTYPES for nm in
                                  ("u-nvec1025", "u-V3", f"s-V{R.SPLIT_V[dt][2]}-r3")])
def test_all_minus_inf_rows_give_minus_inf_and_nan(ops, dev, name):
    """The kernel's answer for a row without a finite element, like torch.logsumexp:
    lse = -inf and NaN tok_lp (the fp64 oracle returns NaN for such a row)."""
    L = R.make_launch(CASES[name], "allinf")
    assert np.isneginf(L.ref_lse).all() and np.isnan(L.ref_tok).all()
    bad, _ = _run(ops, dev, L)
    assert not bad, "\n".join(bad[:20])
    x = _logits(L, dev)
    assert torch.isneginf(torch.logsumexp(x[:, :L.case.V].float(), dim=1)).all()


BEAM = [(dt, cap, form) for dt in R.DTYPES for cap in R.CAPS for form in ("unsplit", "split")]


@pytest.mark.parametrize("dt,cap,form", BEAM, ids=[f"{d}-cap{c:g}-{f}" for d, c, f in BEAM])
def test_beam_step_agent_rows_are_the_same_stream(ops, dev, dt, cap, form):
    """cs_beam_step over counting, one-hot and NaN agent rows, in its unsplit and split forms:
    out_U is rewards_in + tok_lp of cs_logsoftmax_gather bit for bit, NaN pattern included, and
    that tok_lp is inside the windows."""
    A, B, K = (32, 8, 5) if form == "unsplit" else (2, 3, 7)
    V = 1025 * R.EPV[dt] + 3 if form == "unsplit" else R.SPLIT_V[dt][2]
    c = R.Case(f"{dt}-beam-{form}", dt, V, A * B, k=K, base_off=3)
    assert c.path == form
    for shift in (0, 1):
        L = R.beam_launch(c, cap, B, K, shift)
        x = _logits(L, dev)
        tg = torch.from_numpy(L.targets[:B]).to(dev)
        g = torch.Generator().manual_seed(A + shift)
        rew = (-torch.rand(A, B, generator=g) * 20.0).to(dev)
        tok, lse = ops.logsoftmax_gather(x, tg.repeat(A, 1), vocab=V, softcap=cap, want_lse=True)
        bad, _ = R.check(L, lse.cpu().numpy(), tok.cpu().numpy())
        assert not bad, "\n".join(bad[:20])
        U, W, _, _ = ops.beam_step(x, tg, rew, "min", n_order=0, vocab=V, softcap=cap)
        want = (rew[:, :, None] + tok.view(A, B, K)).reshape(A, B * K)
        assert torch.equal(torch.isnan(U), torch.isnan(want))
        assert torch.isnan(want).any() and not torch.isnan(want).all()
        assert torch.equal(torch.nan_to_num(U, nan=7.0).view(torch.int32),
                           torch.nan_to_num(want, nan=7.0).view(torch.int32))
