"""cs_gemm_bf16_w8 (csrc/gemm_w8.hip) bit for bit, with no tolerance anywhere, on the operands
and helpers of tests/gemm_ref.py and the cases of tests/w8_ref.py (whose exactness
tests/test_w8_host.py proves on the CPU):

  every_code        W holds each of the 254 finite e4m3 codes, rows scaled by 2^-20, 1, 2^20;
                    one-hot X rows select W[n][k(m)]: Y must be value(code) * 2^e[n] for every
                    K step, half, chunk and element (a failure names the element delivered)
  integer cases     |v| <= 15 operands (exact as codes, sums exact in fp32 in any order): the
                    folded output is bf16_rne(exact sum * 2^e[n]), the unfolded partials the
                    exact sums of their K slices, for every tail length of the register ring,
                    splits 1, 2, 3 and the library's choice, and a bit-identical relaunch
  gated             both activations against cs_gated_act of the host-computed rounded halves
                    and against the plain w8 GEMM followed by cs_gated_act
  overflow          sums beyond the bf16 maximum round to inf as torch rounds them (the scale
                    2^118 is the row exponent)
  guards            ragged last row tile in NaN-poisoned X padding, an out window inside a
                    sentinel-filled tensor, max_rows + 1 refused with nothing written"""
import importlib

import numpy as np
import pytest
import torch

import gemm_ref as R
import w8_ref as W

pytestmark = pytest.mark.gpu
SENT16 = 0x5A5A


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    gb, wb = R.bits(got), R.bits(want)
    if torch.equal(gb, wb):
        return
    bad = (gb != wb).nonzero()
    i = tuple(bad[0].tolist())
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: "
                f"got {got[i].item()!r}, want {want[i].item()!r}")


def _fp8(ops, dev, wi, exps):
    """The Fp8Weight of integer (or any on-grid) values wi [N, K] with row exponents exps."""
    codes = W.encode_rne(np.asarray(wi, dtype=np.float64))
    assert np.array_equal(W.code_value(codes), np.asarray(wi, dtype=np.float64))
    return ops.gemm_w8_from_codes(torch.from_numpy(codes).to(dev),
                                  torch.from_numpy(np.asarray(exps)).to(torch.int8).to(dev))


class Operands:
    """The operands of one (M, N, gated): X and the Fp8Weight of the first 64 n columns."""

    def __init__(self, ops, dev, M, N, gated):
        self.ops, self.dev, self.M, self.N, self.gated = ops, dev, M, N, gated
        self.xi, self.wi = W.case_operands(M, N)
        self.exps = W.case_exps(N, gated)
        self.C = W.case_prefix(M, N)
        self.made = {}

    def __call__(self, n):
        if n not in self.made:
            K = R.BK * n
            x = self.xi[:, :K].to(torch.bfloat16).to(self.dev)
            self.made[n] = (x, _fp8(self.ops, self.dev, self.wi[:, :K].numpy(), self.exps))
        return self.made[n]

    def expected(self, n):
        return W.scale_rows(self.C[n], self.exps).to(torch.bfloat16)

    def expected_partials(self, nk, s):
        return torch.stack([W.scale_rows(self.C[(p + 1) * nk] - self.C[p * nk], self.exps)
                            for p in range(s)]).float()


# --- every code ----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [192, 448])
@pytest.mark.parametrize("M", [16, 80])
def test_every_code_and_every_k_position(ops, dev, M, K):
    N = 256
    codes = W.every_code_matrix(N, K)
    assert set(codes.ravel().tolist()) == set(W.FINITE_CODES.tolist())
    exps = np.array(W.ROW_E)[np.arange(N) % 3]
    fw = ops.gemm_w8_from_codes(torch.from_numpy(codes).to(dev), torch.from_numpy(exps).to(torch.int8).to(dev))
    wv = torch.from_numpy(W.twin_of(codes, exps))                    # fp64 [N, K]
    assert torch.equal(wv.to(torch.bfloat16).double(), wv)           # every expected output is a bf16 number
    for shift in R.selector_shifts(M, K):
        x = R.selector_x(M, K, shift).to(dev)
        want = R.selector_expected(wv, M, K, shift)
        for s in (1, K // R.BK if K == 448 else 3):
            got = ops.gemm_w8(x, fw, splits=s).cpu().double()
            # (-0 codes: value -0 * 2^e + the other products' +0 = +0 in fp32, as in `want == got`)
            if not torch.equal(got, want):
                pytest.fail(f"M {M} K {K} shift {shift} splits {s}: " +
                            R.selector_decode(wv, got, want, M, K, shift))


# --- integer cases -------------------------------------------------------------------------------

@pytest.mark.parametrize("N", W.CASE_N)
@pytest.mark.parametrize("M", W.CASE_M)
def test_integer_cases_are_bit_exact(ops, pkg, dev, M, N):
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    opnd = Operands(ops, dev, M, N, False)
    for nk, s in W.case_shapes(False):
        n = nk * max(s, 1)
        x, fw = opnd(n)
        what = f"M {M} N {N} nk {nk} splits {s}"
        got = ops.gemm_w8(x, fw, splits=s)
        _same(got, opnd.expected(n).to(dev), what)
        _same(ops.gemm_w8(x, fw, splits=s), got, what + ": relaunch")
        chosen = s if s else int(L.cs_gemm_w8_splits(M, N, R.BK * n, 0))
        assert chosen == (s or W.splits(M, N, R.BK * n))
        if chosen >= 2:
            part = ops.gemm_w8_partials(x, fw, splits=chosen).part
            _same(part, opnd.expected_partials(n // chosen, chosen).to(dev), what + ": partials")


@pytest.mark.parametrize("N", W.CASE_N)
@pytest.mark.parametrize("M", W.CASE_M)
def test_gated_cases_are_bit_exact(ops, dev, M, N):
    opnd = Operands(ops, dev, M, N, True)
    F = N // 2
    for nk, s in W.case_shapes(True):
        x, fw = opnd(nk)
        gu = opnd.expected(nk)
        plain = ops.gemm_w8(x, fw, splits=1)
        _same(plain, gu.to(dev), f"M {M} N {N} nk {nk}: the plain halves")
        for act in R.ACTS:
            what = f"M {M} N {N} nk {nk} {act}"
            got = ops.gemm_w8(x, fw, gated=True, act=act)
            _same(got, R.gated_expected(ops, gu, act, dev), what)
            _same(got, ops.gated_act(plain[:, :F], plain[:, F:], act), what + ": plain + cs_gated_act")
            _same(ops.gemm_w8(x, fw, gated=True, act=act), got, what + ": relaunch")


# --- overflow ------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 2])
def test_sums_beyond_the_bf16_maximum_round_to_inf(ops, dev, splits):
    M, N, K = 33, 512, 128
    xi, wi = R.overflow_operands(M, N, K)
    want = R.to_bf16(xi.double() @ wi.double().t(), R.OVERFLOW_E)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
    fw = _fp8(ops, dev, wi.numpy(), np.full(N, R.OVERFLOW_E))
    got = ops.gemm_w8(xi.to(torch.bfloat16).to(dev), fw, splits=splits)
    _same(got, want.to(dev), f"overflow at the output rounding, splits {splits}")


# --- guards --------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 17, 33, 49, 65])
def test_ragged_rows_in_poisoned_padding_and_a_guarded_out_window(ops, dev, M):
    """X is a window of a NaN-filled buffer (NaN rows around its M rows, NaN columns around
    [0, K)); out is a window of a sentinel-filled tensor.  The window holds the exact result,
    nothing outside it changes."""
    N = 384
    opnd = Operands(ops, dev, M, N, False)
    gopnd = Operands(ops, dev, M, N, True)
    for nk, s, gated in ((2, 1, False), (7, 1, False), (2, 2, False), (1, 3, False), (5, 1, True)):
        o = gopnd if gated else opnd
        n = nk * s
        K = R.BK * n
        x, fw = o(n)
        xb = torch.full((M + 4, K + 16), float("nan"), dtype=torch.bfloat16, device=dev)
        xb[2:2 + M, 8:8 + K] = x
        n_out = N // 2 if gated else N
        for extra, r0, c0 in ((24, 2, 8), (20, 1, 4)):
            if s > 1 and extra != 24:
                continue
            buf = torch.full((M + r0 + 3, n_out + extra), SENT16, dtype=torch.int16, device=dev)
            win = buf.view(torch.bfloat16)[r0:r0 + M, c0:c0 + n_out]
            out = ops.gemm_w8(xb[2:2 + M, 8:8 + K], fw, gated=gated, splits=s, out=win)
            assert out.data_ptr() == win.data_ptr()
            what = f"M {M} nk {nk} splits {s} gated {gated} ld {n_out + extra}"
            want = R.gated_expected(ops, o.expected(n), "silu", dev) if gated else o.expected(n).to(dev)
            _same(win, want, what)
            b = buf.clone()
            b[r0:r0 + M, c0:c0 + n_out] = SENT16
            assert bool((b == SENT16).all()), what + ": a store outside the out window"


def test_more_than_max_rows_is_refused_and_nothing_is_written(ops, pkg, dev):
    lib = importlib.import_module(pkg.__name__ + "._lib")
    L = lib.load()
    assert ops.gemm_w8_max_rows() == W.MAX_ROWS == L.cs_gemm_w8_max_rows()
    M, N, K = W.MAX_ROWS + 1, 384, 128
    fw = _fp8(ops, dev, np.ones((N, K)), np.zeros(N))
    x = torch.ones(M, K, dtype=torch.bfloat16, device=dev)
    y = torch.full((M, N), SENT16, dtype=torch.int16, device=dev)
    ws = torch.full((2 * M * N,), SENT16, dtype=torch.int16, device=dev)
    for s in (1, 2, 0):
        rc = L.cs_gemm_bf16_w8(x.data_ptr(), K, fw.data.data_ptr(), fw.exps.data_ptr(), y.data_ptr(), N,
                               M, N, K, s, 0, 0, ws.data_ptr(), ops._stream())
        assert rc != 0 and b"max_rows" in L.cs_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENT16).all()) and bool((ws == SENT16).all())
    with pytest.raises(ops.CSError):
        ops.gemm_w8(x, fw)
    # the last served row count, on the same weight
    got = ops.gemm_w8(x[:W.MAX_ROWS], fw)
    assert bool((got == float(K)).all())
    # other refusals of the entry point
    with pytest.raises(ops.CSError):
        ops.gemm_w8(x[:8, :64].contiguous(), fw)         # K of x is not the weight's
    with pytest.raises(ops.CSError):
        ops.gemm_w8(x[:8], fw, splits=4)                 # K = 128: not a multiple of 64 * 4


# --- the partials' consumers ---------------------------------------------------------------------

def test_unfolded_partials_feed_the_residual_add_and_linear_routes_them(ops, dev):
    """ops.linear(fold=False) on an Fp8Weight whose shape takes a K split returns the unfolded
    partials, and cs_add_rms_norm_splitk folds them bitwise as the GEMM's own fold + the add."""
    M, N, K = 33, 384, 1024
    assert W.splits(M, N, K) == 2
    g = torch.Generator(device="cpu").manual_seed(3)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    fw = ops.gemm_w8_pack(w, twin_out=w)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    h = (torch.randn(M, N, generator=g) * 2).to(torch.bfloat16).to(dev)
    wt = (torch.randn(N, generator=g) * 0.1 + 1.0).to(torch.bfloat16).to(dev)
    p = ops.linear(x, w, fold=False, packed=fw)
    assert isinstance(p, ops.SplitPartials) and tuple(p.part.shape) == (2, M, N)
    y = ops.linear(x, w, packed=fw)
    _same(y, ops.gemm_w8(x, fw, splits=2), "linear on an Fp8Weight")
    _same(p.part, ops.gemm_w8_partials(x, fw, splits=2).part, "linear(fold=False)")
    h_p, h_f = h.clone(), h.clone()
    x_p = ops.add_rms_norm(h_p, wt, 1e-6, b=p, s_out=h_p)
    x_f = ops.add_rms_norm(h_f, wt, 1e-6, b=y, s_out=h_f)
    _same(h_p, h_f, "residual stream")
    _same(x_p, x_f, "normed rows")
    # against the bf16 route on the twin: the accumulation order alone differs
    ref = x.float() @ w.float().t()
    tol = ref.abs() * 2.0 ** -7 + 1e-3 * ref.abs().max()
    assert bool(((y.float() - ref).abs() <= tol).all())
    assert bool(((ops.linear(x, w).float() - ref).abs() <= tol).all())


# --- the residual form ---------------------------------------------------------------------------

@pytest.mark.parametrize("M", [17, 80])
def test_residual_form_adds_before_the_one_rounding(ops, dev, M):
    """cs_gemm_bf16_w8_add on the integer cases: h = hi * 2^e[n] with |hi| <= 100 is exact in
    bf16 and (sum + hi) * 2^e[n] exact in fp32, so h must come back as bf16_rne((sum + hi) * 2^e[n])
    -- and that differs from rounding the product first in a share of the elements."""
    N = 384
    opnd = Operands(ops, dev, M, N, False)
    g = torch.Generator(device="cpu").manual_seed(M)
    hi = torch.randint(-100, 101, (M, N), generator=g, dtype=torch.int64).double()
    h0 = W.scale_rows(hi, opnd.exps).to(torch.bfloat16)
    assert torch.equal(h0.double(), W.scale_rows(hi, opnd.exps))
    twice = 0
    for nk, s in [(2, 1), (7, 1), (25, 1), (2, 2), (5, 3), (16, 0), (32, 0)]:
        n = nk * max(s, 1)
        x, fw = opnd(n)
        want = W.scale_rows(opnd.C[n] + hi, opnd.exps).to(torch.bfloat16)
        buf = torch.full((M + 3, N + 24), SENT16, dtype=torch.int16, device=dev)
        win = buf.view(torch.bfloat16)[2:2 + M, 8:8 + N]
        win.copy_(h0)
        out = ops.gemm_w8_add(x, fw, win, splits=s)
        assert out.data_ptr() == win.data_ptr()
        _same(win, want.to(dev), f"M {M} nk {nk} splits {s}: h + product, one rounding")
        b = buf.clone()
        b[2:2 + M, 8:8 + N] = SENT16
        assert bool((b == SENT16).all()), "a store outside h"
        two = (opnd.expected(n).float() + h0.float()).to(torch.bfloat16)
        twice += int((R.bits(two) != R.bits(want)).sum())
    assert twice > 0                     # the cases tell one rounding from two
    x, fw = opnd(2)
    with pytest.raises(ops.CSError):
        ops.gemm_w8_add(x, fw, torch.zeros(M, N - 8, dtype=torch.bfloat16, device=dev))
