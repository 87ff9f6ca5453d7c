"""The FP8 weight form on the CPU: tests/w8_ref.py (the restated quantiser, layout and split)
against torch.float8_e4m3fn and against its own definitions, the `@fp8` identifier, the new
entry points' declarations, and the exactness precondition of the integer GPU cases
(tests/test_w8_gemm_exact_gpu.py).  No kernel runs here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as R
import w8_ref as W
from conftest import REPO

F8 = torch.float8_e4m3fn


def _all_finite_bf16():
    bits = torch.arange(0x10000, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16)
    return v[torch.isfinite(v.float())]


def test_code_values_are_torchs_and_exact_in_bf16():
    codes = torch.from_numpy(W.FINITE_CODES.copy())
    assert len(codes) == 254
    want = codes.view(F8).float()
    got = torch.from_numpy(W.code_value(W.FINITE_CODES))
    assert torch.equal(got, want.double())
    assert torch.equal(want.to(torch.bfloat16).float(), want)          # all 254 exact in bf16
    assert float(want.max()) == 448.0 and float(want[want > 0].min()) == 2.0 ** -9
    assert np.isnan(W.code_value(np.array([0x7f, 0xff]))).all()


def test_rne_equals_torch_over_every_finite_bf16_input_at_e0():
    v = _all_finite_bf16()
    small = v[v.float().abs() <= 448]
    assert len(small) > 30000
    got = W.encode_rne(small.double().numpy())
    want = small.float().to(F8).view(torch.uint8).numpy()
    assert np.array_equal(got, want)
    assert not (got & 0x7f == 0x7f).any()                    # NaN codes are never produced
    assert (got & 0x78 == 0).sum() > 1000                    # subnormal codes are kept
    # a one-element row: e = 0 exactly for 224 < |v| <= 448, below for smaller, above for larger
    a = v.double().abs().numpy()
    e = np.array([W.row_exponent(x) for x in a])
    assert ((e == 0) == ((a == 0) | ((a > 224) & (a <= 448)))).all()
    assert (e[a > 448] > 0).all() and (e[(a > 0) & (a <= 224)] < 0).all()
    nz = a > 0
    scaled = a[nz] * 2.0 ** -e[nz].astype(np.float64)
    assert (scaled <= 448).all() and (scaled > 224).all()    # the smallest such exponent


@pytest.mark.parametrize("e", [-128, -20, 0, 7, 119])
def test_row_amax_edges(e):
    top = 448.0 * 2.0 ** e
    w = torch.tensor([[top, -top / 448, 0.0, -0.0] + [0.0] * 60,
                      [0.0] * 64], dtype=torch.float64).to(torch.bfloat16)
    assert float(w[0, 0]) == top
    codes, exps, twin, status = W.quantise(w)
    assert status == 0 and list(exps) == [e, 0]
    assert list(codes[0, :4]) == [0x7e, 0x80 | 0x38, 0x00, 0x80]      # 448, -1, +0, -0
    assert not codes[1].any()
    assert torch.equal(R.bits(twin), R.bits(w))
    # one bf16 ulp above 448 * 2^e: the exponent steps up, the top value rounds onto the coarser grid
    up = (R.bits(w[0, :1]) + 1).view(torch.bfloat16)
    w2 = w.clone()
    w2[0, 0] = up[0]
    codes2, exps2, twin2, status2 = W.quantise(w2)
    if e == 119:      # 450 * 2^119 -> e = 120, fine; bf16's own maximum is the overflow case below
        assert status2 == 0
    assert exps2[0] == e + 1
    assert codes2[0, 0] == W.encode_rne(np.array([225.0]))[0] == 0x76          # 225 -> 224
    assert float(twin2[0, 0]) == 224.0 * 2.0 ** (e + 1)


def test_subnormal_range_inputs_round_to_nearest_even():
    # a row with amax 448 (e = 0) and elements around the subnormal grid (spacing 2^-9)
    u = 2.0 ** -9
    vals = [448.0, u, 1.5 * u, 2.5 * u, 0.5 * u, 0.75 * u, 0.25 * u, 7.5 * u, 8 * u, -0.5 * u, -1.5 * u]
    w = torch.tensor([vals + [0.0] * (64 - len(vals))], dtype=torch.float64).to(torch.bfloat16)
    assert torch.equal(w.double()[0, :len(vals)], torch.tensor(vals, dtype=torch.float64))
    codes, exps, twin, status = W.quantise(w)
    assert status == 0 and exps[0] == 0
    assert list(codes[0, :len(vals)]) == [0x7e, 1, 2, 2, 0, 1, 0, 8, 8, 0x80, 0x82]
    assert np.array_equal(codes, w.float().to(F8).view(torch.uint8).numpy())
    assert float(twin[0, 4]) == 0.0 and float(twin[0, 2]) == 2 * u


def test_refused_rows():
    ok = torch.ones(16, 64, dtype=torch.bfloat16)
    for bad in (float("nan"), float("inf"), float("-inf")):
        w = ok.clone()
        w[3, 5] = bad
        assert W.quantise(w)[3] == W.STATUS_NONFINITE
    w = ok.clone()
    w[2, 0] = torch.finfo(torch.bfloat16).max          # 255 * 2^120 -> code 256 * 2^120: overflow
    assert W.quantise(w)[3] == W.STATUS_ROW_RANGE
    w = ok.clone()
    w[2] = 0
    w[2, 1] = 2.0 ** -125                               # e = -133: no int8
    assert W.quantise(w)[3] == W.STATUS_ROW_RANGE
    # the lowest exponent int8 holds, with a bf16-subnormal input beside the row's amax
    w = ok.clone()
    w[2] = 0
    w[2, :2] = torch.tensor([1.75 * 2.0 ** -120, 2.0 ** -127])
    codes, exps, twin, status = W.quantise(w)
    assert status == 0 and exps[2] == -128 and list(codes[2, :2]) == [0x7e, 0x40]      # 448, 2
    assert torch.equal(R.bits(twin), R.bits(w))


def test_twin_requantises_to_itself():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 128, generator=g) * 0.05).to(torch.bfloat16)
    w[1, 0] = 224.0            # the row's amax lands on 224 * 2^e: the second exponent is one less
    w[1, 1:] *= 0.01
    codes, exps, twin, status = W.quantise(w)
    assert status == 0
    codes2, exps2, twin2, status2 = W.quantise(twin)
    assert status2 == 0 and torch.equal(R.bits(twin2), R.bits(twin))
    assert np.array_equal(W.twin_of(codes, exps), twin.double().numpy())


@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (128, 448)])
def test_layout_is_a_permutation_and_the_documented_formula(N, K):
    idx = W.packed_index(N, K)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(N * K))
    # the header's formula, element by element on a sample
    for n, k in [(0, 0), (N - 1, K - 1), (5, 37), (N // 2 + 3, K // 2 + 9), (15, 63), (N - 16, 32)]:
        T, s, h, l, j = n // 16, k // 64, k % 64 // 32, 16 * (k % 32 // 8) + n % 16, k % 8
        assert idx[n, k] == (T * (K // 64) + s) * 1024 + 16 * l + 8 * h + j
    codes = np.random.default_rng(0).integers(0, 256, (N, K), dtype=np.uint8)
    assert np.array_equal(W.unpack(W.pack(codes), N, K), codes)
    # one lane's 16 bytes: one row, the two halves' 8 k each
    p = W.pack(np.arange(N * K, dtype=np.int64).reshape(N, K) % 251).reshape(-1, 64, 16)
    lane = W.pack(np.repeat(np.arange(N)[:, None], K, 1).astype(np.uint8)).reshape(-1, 64, 16)
    assert (lane == lane[:, :, :1]).all()
    assert p.shape[0] == N // 16 * (K // 64)


def test_fp8_identifier_parsing(pkg):
    rt = importlib.import_module(pkg.__name__ + ".runtime")
    assert rt.split_fp8_id("meta-llama/Meta-Llama-3.1-8B-Instruct-Turbo@fp8") == \
        ("meta-llama/Meta-Llama-3.1-8B-Instruct-Turbo", True)
    assert rt.split_fp8_id("random:tiny-llama@fp8") == ("random:tiny-llama", True)
    assert rt.split_fp8_id("random:tiny-llama") == ("random:tiny-llama", False)
    assert rt.split_fp8_id("@fp8") == ("@fp8", False)
    assert rt.split_fp8_id("x@fp8@fp8") == ("x@fp8", True)
    assert rt.split_fp8_id("x@FP8") == ("x@FP8", False)
    assert rt.resolve_preset(rt.split_fp8_id("meta-llama/Meta-Llama-3.1-8B-Instruct-Turbo@fp8")[0]) == \
        "llama-3.1-8b"


_CTYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int8_t*": ctypes.c_void_p,
           "int8_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "cs_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}
W8_ENTRIES = ("cs_gemm_w8_pack", "cs_gemm_w8_pack_codes", "cs_gemm_bf16_w8", "cs_gemm_bf16_w8_add", "cs_gemm_w8_splits",
              "cs_gemm_w8_max_rows")


def test_header_and_ctypes_agree_on_the_w8_entries(pkg):
    lib = importlib.import_module(pkg.__name__ + "._lib")
    L = lib.load()
    text = open(os.path.join(REPO, "include", "consensus_scoring.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in W8_ENTRIES:
        assert name in lib.EXPORTED
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(2).split(",")]
        types = [] if params == ["void"] else [_CTYPES[re.sub(r"\s*\w+$", "", p).replace(" *", "*")]
                                               for p in params]
        fn = getattr(L, name)
        assert list(fn.argtypes) == types, (name, fn.argtypes, types)
        assert fn.restype == (ctypes.c_int if m.group(1) == "int" else ctypes.c_int64), name


def test_splits_restatement_is_the_librarys(pkg):
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    assert L.cs_gemm_w8_max_rows() == W.MAX_ROWS
    for N in (128, 384, 512, 4096, 6144, 28672, 128256, 100):
        for K in (64, 320, 1024, 2048, 4096, 14336, 8192, 100):
            for gated in (0, 1):
                for M in (0, 1, 48, 80):
                    assert L.cs_gemm_w8_splits(M, N, K, gated) == W.splits(M, N, K, bool(gated)), (M, N, K)
    assert [W.splits(48, 512, 64 * n) for n in W.ZERO_STEPS] == [1, 2, 2, 4]
    assert W.splits(48, 4096, 14336) == 8 and W.splits(48, 28672, 4096, True) == 1


def test_integer_cases_are_exact_as_codes_and_in_fp32():
    """|v| <= 15 is an e4m3 value (so the codes hold the operands exactly), every sum of the
    integer products stays below 2^24 in any order (fp32-exact), and the row scale is a power
    of two applied to that exact sum: the only rounding left is the output's."""
    ints = np.arange(-R.AMAX, R.AMAX + 1, dtype=np.float64)
    assert np.array_equal(W.code_value(W.encode_rne(ints)), ints)
    assert R.AMAX * R.AMAX * R.BK * W.MAX_STEPS < 2 ** 24
    for gated in (False, True):
        for nk, s in W.case_shapes(gated):
            assert nk * max(s, 1) <= W.MAX_STEPS
    M, N = 17, 384
    xi, wi = W.case_operands(M, N)
    assert int(xi.abs().max()) <= R.AMAX and int(wi.abs().max()) <= R.AMAX
    C = W.case_prefix(M, N)
    n = 7
    assert torch.equal(C[n], (xi[:, :64 * n].double() @ wi[:, :64 * n].double().t()))
    assert float(C.abs().max()) < 2 ** 24
    for e in W.ROW_E + (W.GATED_E,):
        assert -100 < e < 100                       # the scaled sums stay normal fp32 numbers
    # the overflow operands are codes too
    xo, wo = R.overflow_operands(33, 128, 128)
    assert np.array_equal(W.code_value(W.encode_rne(wo.double().numpy())), wo.double().numpy())
    # every tail length of the six-step ring is reached, with and without a whole ring before it
    assert {nk % 6 for nk, s in W.case_shapes(False)} >= {1, 2, 3, 4, 5}
    assert {nk % 6 for nk, s in W.case_shapes(False) if nk > 6} >= {1, 2, 3, 5}
