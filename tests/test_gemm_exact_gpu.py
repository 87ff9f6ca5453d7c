"""cs_gemm_bf16 / cs_gemm_bf16_packed (csrc/gemm.hip) bit for bit, on integer operands whose
fp32 sums are exact in any order (tests/gemm_ref.py; tests/test_gemm_cases_host.py proves
on the CPU that every case exercises the output rounding and would catch a dropped, doubled
or misplaced K element).  No tolerance anywhere: the expected output is
bf16_rne(int64 product * 2^e) computed on the host, the expected K-split partial the exact
product over its own K slice, the expected gated output cs_gated_act of the host-computed
rounded halves.

  every_split_and_pipeline_length   each (family, variant, gated, packed, M) case at nk = 1,
                                    2, 3, 4, 5, 7 K steps per split and splits 1, 2, 3 and
                                    0 (the library's choice), thin nsteps 1..49: output,
                                    partials, both activations, a bit-identical relaunch
  guarded_output                    per template instantiation (ragged M): out a window of a
                                    sentinel-filled buffer (ld % 8 == 0, and == 4 unsplit),
                                    the partials workspace with sentinel slack through the
                                    C ABI -- nothing outside the window may change
  poisoned_padding                  per instantiation: X and W windows of NaN-filled buffers
                                    (rows past M, columns outside [0, K))
  nan_and_inf / overflow            special values stay in their row; sums beyond the bf16
                                    maximum round to inf as torch rounds them
  selector                          one-hot X rows: Y[m][n] = W[n][k(m)], every k visited;
                                    a failure names the (n, k) the kernel delivered"""
import importlib

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
GUARD = R.guard_cases()
SENT16 = 0x5A5A
SENT32 = 0x5A5A5A5A


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    gb, wb = R.bits(got), R.bits(want)
    if torch.equal(gb, wb):
        return
    bad = (gb != wb).nonzero()
    i = tuple(bad[0].tolist())
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: "
                f"got {got[i].item()!r}, want {want[i].item()!r}")


def _run(ops, c, x, w, pw, *, splits=1, act="silu", out=None):
    if c.packed:
        return ops.gemm_packed(x, pw, gated=c.gated, act=act, splits=splits, variant=c.variant, out=out)
    return ops.gemm(x, w, gated=c.gated, act=act, splits=splits, variant=c.variant, out=out)


def _partials(ops, c, x, w, pw, splits):
    if c.packed:
        return ops.gemm_packed_partials(x, pw, splits=splits, variant=c.variant).part
    return ops.gemm_partials(x, w, splits=splits, variant=c.variant).part


class Operands:
    """A case's operands on the device; the first 64 n columns as contiguous tensors (and the
    packed copy of W), made once per n."""

    def __init__(self, ops, dev, c):
        self.ops, self.c = ops, c
        self.x, self.w = c.x_bf16().to(dev), c.w_bf16().to(dev)
        self.made = {}

    def __call__(self, n):
        if n not in self.made:
            K = R.BK * n
            x, w = self.x[:, :K].contiguous(), self.w[:, :K].contiguous()
            self.made[n] = (x, w, self.ops.gemm_pack(w) if self.c.packed else None)
        return self.made[n]


def _name(c, n, s=1):
    return R.launch(c.variant, c.M, c.N, R.BK * n, c.gated, c.packed, s)["name"]


def _check_case(ops, dev, c, opnd, nk, s, run=_run):
    """One (nk, splits) shape of a case against the host expectation; `run` launches."""
    n = nk * max(s, 1)
    x, w, pw = opnd(n)
    gu = c.expected(n)
    what = f"{c} [{_name(c, n, s)}] nk {nk} splits {s}"
    if c.gated:
        for act in R.ACTS:
            want = R.gated_expected(ops, gu, act, dev)
            got = run(ops, c, x, w, pw, act=act)
            _same(got, want, f"{what} {act}")
            _same(run(ops, c, x, w, pw, act=act), got, f"{what} {act}: relaunch")
    else:
        got = run(ops, c, x, w, pw, splits=s)
        _same(got, gu.to(dev), what)
        _same(run(ops, c, x, w, pw, splits=s), got, f"{what}: relaunch")


@pytest.mark.parametrize("c", CASES, ids=str)
def test_every_split_and_pipeline_length_is_bit_exact(ops, dev, c):
    opnd = Operands(ops, dev, c)
    for nk, s in c.shapes():
        _check_case(ops, dev, c, opnd, nk, s)
        if s >= 2:
            x, w, pw = opnd(nk * s)
            _same(_partials(ops, c, x, w, pw, s), c.expected_partials(nk, s).to(dev),
                  f"{c} [{_name(c, nk * s, s)}] nk {nk} splits {s}: partials")


# --- guarded output ------------------------------------------------------------------------------

def _window(dev, M, n_out, extra, r0, c0):
    buf = torch.full((M + r0 + 3, n_out + extra), SENT16, dtype=torch.int16, device=dev)
    return buf, buf.view(torch.bfloat16)[r0:r0 + M, c0:c0 + n_out]


def _untouched_outside(buf, M, n_out, r0, c0):
    b = buf.clone()
    b[r0:r0 + M, c0:c0 + n_out] = SENT16
    return bool((b == SENT16).all())


@pytest.mark.parametrize("name,c", GUARD, ids=[n for n, _ in GUARD])
def test_guarded_output_window_only_is_written(ops, dev, name, c):
    """out = buf[r0 : r0 + M, c0 : c0 + N] of a sentinel-filled buffer: the window holds the
    exact result and no element outside it changes (a store for a padded row m >= M, or into
    the next column window, would show).  ld % 8 == 0 with every split, ld % 8 == 4 unsplit."""
    opnd = Operands(ops, dev, c)
    n_out = c.N // 2 if c.gated else c.N
    split = c.family != "thin" and not c.gated
    runs = [(2, 1, 24, 2, 8), (2, 1, 20, 1, 4)] + ([(2, 2, 24, 2, 8), (1, 3, 24, 2, 8)] if split else [])
    for nk, s, extra, r0, c0 in runs:
        assert _name(c, nk * s, s) == name
        assert (n_out + extra) % 8 == (0 if extra == 24 else 4)
        bufs = []

        def run(ops, c, x, w, pw, **kw):
            buf, win = _window(dev, c.M, n_out, extra, r0, c0)
            bufs.append(buf)
            out = _run(ops, c, x, w, pw, out=win, **kw)
            assert out.data_ptr() == win.data_ptr()
            return out

        _check_case(ops, dev, c, opnd, nk, s, run)
        for buf in bufs:
            assert _untouched_outside(buf, c.M, n_out, r0, c0), \
                f"{c} [{name}] nk {nk} splits {s} ld {n_out + extra}: a store outside the out window"


@pytest.mark.parametrize("name,c", [(n, c) for n, c in GUARD if c.family != "thin" and not c.gated],
                         ids=[n for n, c in GUARD if c.family != "thin" and not c.gated])
def test_guarded_partials_workspace(ops, pkg, dev, name, c):
    """The K-split partials through the C ABI into a workspace with sentinel slack before and
    after its splits * M * N floats: exact partials, slack unchanged."""
    lib = importlib.import_module(pkg.__name__ + "._lib")
    L = lib.load()
    opnd = Operands(ops, dev, c)
    slack = 1024
    for nk, s in ((2, 3), (1, 2)):
        x, w, pw = opnd(nk * s)
        M, N, K = c.M, c.N, R.BK * nk * s
        size = s * M * N
        ws = torch.full((slack + size + slack,), SENT32, dtype=torch.int32, device=dev)
        ptr = ws.data_ptr() + 4 * slack
        if c.packed:
            rc = L.cs_gemm_bf16_packed(x.data_ptr(), K, pw.data.data_ptr(), None, 0, M, N, K, s, 0, 0,
                                       c.variant, ptr, ops._stream())
        else:
            rc = L.cs_gemm_bf16(x.data_ptr(), K, w.data_ptr(), K, None, 0, M, N, K, s, 0, 0,
                                c.variant, ptr, ops._stream())
        lib.check(rc, "cs_gemm_bf16")
        torch.cuda.synchronize()
        _same(ws[slack:slack + size].view(torch.float32).view(s, M, N),
              c.expected_partials(nk, s).to(dev), f"{c} [{name}] nk {nk} splits {s}: partials")
        assert bool((ws[:slack] == SENT32).all()) and bool((ws[slack + size:] == SENT32).all()), \
            f"{c} [{name}] nk {nk} splits {s}: a store outside the partials"


# --- poisoned padding ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,c", GUARD, ids=[n for n, _ in GUARD])
def test_poisoned_padding_is_never_read_into_a_result(ops, dev, name, c):
    """X [M, K] and W [N, K] are windows of NaN-filled buffers: NaN rows before and after the
    M rows of X, NaN columns on both sides of [0, K) in both.  A read past a K split's slice
    (kbase, the kt < nk clamp, the thin slices' `last`) or of a row past M - 1 (the padded
    rows re-read row M - 1) would put a NaN into a result."""
    full = Operands(ops, dev, c)
    nan = float("nan")

    def poisoned(n):
        x, w, _ = full(n)
        K = R.BK * n
        xb = torch.full((c.M + 4, K + 16), nan, dtype=torch.bfloat16, device=dev)
        wb = torch.full((c.N + 2, K + 16), nan, dtype=torch.bfloat16, device=dev)
        xb[2:2 + c.M, 8:8 + K] = x
        wb[1:1 + c.N, 8:8 + K] = w
        xw, ww = xb[2:2 + c.M, 8:8 + K], wb[1:1 + c.N, 8:8 + K]
        return xw, ww, (ops.gemm_pack(ww) if c.packed else None)

    shapes = [(17, 1), (8, 1)] if c.family == "thin" else [(2, 1), (5, 1)] if c.gated else \
        [(2, 1), (2, 2), (1, 3)]
    for nk, s in shapes:
        assert _name(c, nk * s, s) == name
        _check_case(ops, dev, c, poisoned, nk, s)
        if s >= 2:
            x, w, pw = poisoned(nk * s)
            _same(_partials(ops, c, x, w, pw, s), c.expected_partials(nk, s).to(dev),
                  f"{c} [{name}] nk {nk} splits {s}: partials")


# --- special values ------------------------------------------------------------------------------

SPECIAL = [("ws", 1, False), ("ws2", 2, False), ("ws2", 3, True), ("thin", 5, False), ("thin", 7, False)]
SPECIAL_IDS = [f"{f}-v{v}-{'packed' if p else 'rowmajor'}" for f, v, p in SPECIAL]


@pytest.mark.parametrize("nan_last", [False, True], ids=["nan-row-7", "nan-row-last"])
@pytest.mark.parametrize("family,variant,packed", SPECIAL, ids=SPECIAL_IDS)
def test_nan_and_inf_stay_in_their_rows(ops, dev, family, variant, packed, nan_last):
    """One X row holds +inf at one k, another NaN (nan_last: row M - 1, the row every padded
    row re-reads).  The NaN / inf pattern equals that of torch's fp32 product; every other row
    is still bit-exact."""
    c = R.Case(family, variant, False, packed, 33)
    n, K = 3, 192
    r_inf, r_nan = 3, (c.M - 1 if nan_last else 7)
    x = c.x_bf16()[:, :K].clone()
    w = c.w_bf16()[:, :K].contiguous()
    x[r_inf, 70] = float("inf")
    x[r_nan, 130] = float("nan")
    ref32 = x.float() @ w.float().t()
    want = c.expected(n)
    xd, wd = x.to(dev), w.to(dev)
    got = _run(ops, c, xd, wd, ops.gemm_pack(wd) if packed else None).cpu()
    clean = torch.ones(c.M, dtype=torch.bool)
    clean[[r_inf, r_nan]] = False
    _same(got[clean], want[clean], f"{c}: rows without a special value")
    assert bool(torch.isnan(ref32[r_nan]).all()) and bool(torch.isnan(got[r_nan]).all())
    isn = torch.isnan(ref32[r_inf])
    assert bool(isn.any()) and bool((~isn).any())          # inf * 0 where W holds a zero
    assert torch.equal(torch.isnan(got[r_inf]), isn)
    assert bool(torch.isinf(ref32[r_inf][~isn]).all())
    _same(got[r_inf][~isn], ref32[r_inf][~isn].to(torch.bfloat16), f"{c}: the inf row")


@pytest.mark.parametrize("family,variant,packed", SPECIAL, ids=SPECIAL_IDS)
def test_sums_beyond_the_bf16_maximum_round_to_inf(ops, dev, family, variant, packed):
    """Non-negative operands with W scaled by 2^118 (gemm_ref.overflow_operands): sums of
    1022 * 2^118 and more round to +inf, smaller ones stay finite, as torch rounds them."""
    c = R.Case(family, variant, False, packed, 33)
    xi, wi = R.overflow_operands(c.M, c.N, 128)
    x, w = xi.to(torch.bfloat16), R.to_bf16(wi.double(), R.OVERFLOW_E)
    want = R.to_bf16(xi.double() @ wi.double().t(), R.OVERFLOW_E)
    assert torch.equal(R.bits(want), R.bits((x.float() @ w.float().t()).to(torch.bfloat16)))
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
    xd, wd = x.to(dev), w.to(dev)
    got = _run(ops, c, xd, wd, ops.gemm_pack(wd) if packed else None)
    _same(got, want.to(dev), f"{c}: overflow at the output rounding")


# --- selector ------------------------------------------------------------------------------------

SELECT = [(v, False) for v in range(1, 8)] + [(v, True) for v in (2, 3, 4)]


@pytest.mark.parametrize("K", [192, 448])
@pytest.mark.parametrize("variant,packed", SELECT,
                         ids=[f"v{v}-{'packed' if p else 'rowmajor'}" for v, p in SELECT])
def test_selector_rows_deliver_their_own_k(ops, dev, variant, packed, K):
    """Row m of X is one-hot at k(m): Y[m][n] must be W[n][k(m)].  Over the shifts the rows
    visit every k.  On failure the message decodes which W element arrived instead."""
    thin = variant >= 5
    c = R.Case("thin" if thin else "ws" if variant == 1 else "ws2", variant, False, packed,
               80 if thin else 289)
    wi = R.selector_w(c.N, K)
    w = wi.to(torch.bfloat16).to(dev)
    pw = ops.gemm_pack(w) if packed else None
    for shift in R.selector_shifts(c.M, K):
        x = R.selector_x(c.M, K, shift).to(dev)
        want = R.selector_expected(wi, c.M, K, shift).double()
        for s in ((1,) if thin else (1, K // R.BK if K == 448 else 3)):
            got = _run(ops, c, x, w, pw, splits=s).cpu().double()
            if not torch.equal(got, want):
                pytest.fail(f"{c} [{_name(c, K // R.BK, s)}] K {K} shift {shift} splits {s}: " +
                            R.selector_decode(wi, got, want, c.M, K, shift))
