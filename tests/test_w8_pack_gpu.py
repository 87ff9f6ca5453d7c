"""cs_gemm_w8_pack / cs_gemm_w8_pack_codes (csrc/gemm_w8.hip) against the CPU restatement
tests/w8_ref.py, bit for bit: the codes after un-permuting, the row exponents and the twin;
refused weights (NaN, Inf, a row whose twin overflows bf16) set the status and write nothing."""
import importlib

import numpy as np
import pytest
import torch

import gemm_ref as R
import w8_ref as W

pytestmark = pytest.mark.gpu

SHAPES = [(N, K) for N in (128, 384) for K in (64, 192)]


def _weight(N, K):
    """Random rows of mixed magnitudes plus planted edge rows, as a window of a wider buffer."""
    g = torch.Generator(device="cpu").manual_seed(31 * N + K)
    w = torch.randn(N, K, generator=g) * (10.0 ** torch.randint(-4, 3, (N, 1), generator=g).float())
    w = w.to(torch.bfloat16)
    w[3] = 0                                             # an all-zero row: e = 0
    w[4, :4] = torch.tensor([448.0, -0.0, 2.0 ** -9, 1.5 * 2.0 ** -9])   # e = 0, subnormal codes
    w[5, 0] = 448.0 * 2.0 ** -30                        # amax exactly 448 * 2^e
    w[6, 0] = 450.0 * 2.0 ** 7                          # one bf16 ulp above 448 * 2^7
    w[7] = 0
    w[7, :3] = torch.tensor([1.75 * 2.0 ** -120, 2.0 ** -127, -2.0 ** -130])   # bf16 subnormal inputs
    w[8] *= 1e-3
    w[8, 0] = 100.0                                      # most of the row far below its amax
    buf = torch.full((N + 2, K + 24), float("nan"), dtype=torch.bfloat16)
    buf[1:1 + N, 8:8 + K] = w
    return w, buf


@pytest.mark.parametrize("N,K", SHAPES)
def test_pack_equals_the_restatement_bitwise(ops, dev, N, K):
    w, buf = _weight(N, K)
    codes, exps, twin, status = W.quantise(w)
    assert status == 0 and exps[7] == -128 and exps[3] == 0 and exps[6] == 8
    win = buf.to(dev)[1:1 + N, 8:8 + K]                  # strided: ld = K + 24
    assert win.stride(0) == K + 24
    tw = torch.full((N, K + 8), 7.0, dtype=torch.bfloat16, device=dev)
    fw = ops.gemm_w8_pack(win, twin_out=tw[:, :K])
    assert fw.shape == (N, K) and fw.data.dtype == torch.uint8 and fw.exps.dtype == torch.int8
    got = W.unpack(fw.data.cpu().numpy(), N, K)
    bad = np.argwhere(got != codes)
    assert not len(bad), (len(bad), bad[:4], got[tuple(bad[0])], codes[tuple(bad[0])])
    assert np.array_equal(fw.exps.cpu().numpy().astype(np.int64), exps)
    assert torch.equal(R.bits(tw[:, :K].cpu()), R.bits(twin))
    assert bool((tw[:, K:] == 7.0).all())
    # no twin asked for; and in place (the model's way)
    fw2 = ops.gemm_w8_pack(win)
    assert torch.equal(fw2.data, fw.data) and torch.equal(fw2.exps, fw.exps)
    inplace = win.clone()
    fw3 = ops.gemm_w8_pack(inplace, twin_out=inplace)
    assert torch.equal(fw3.data, fw.data) and torch.equal(R.bits(inplace.cpu()), R.bits(twin))
    # the twin packs to values equal to itself
    again = torch.empty_like(inplace)
    ops.gemm_w8_pack(inplace, twin_out=again)
    assert torch.equal(R.bits(again), R.bits(inplace))
    # the permutation alone
    fc = ops.gemm_w8_from_codes(torch.from_numpy(codes).to(dev), torch.from_numpy(exps).to(torch.int8).to(dev))
    assert torch.equal(fc.data, fw.data) and torch.equal(fc.exps, fw.exps)


@pytest.mark.parametrize("what", ["nan", "inf", "overflow", "exponent"])
def test_refused_weight_sets_status_and_writes_nothing(ops, pkg, dev, what):
    lib = importlib.import_module(pkg.__name__ + "._lib")
    L = lib.load()
    N, K = 128, 192
    w, _ = _weight(N, K)
    if what == "nan":
        w[77, 100] = float("nan")
    elif what == "inf":
        w[0, 191] = float("-inf")
    elif what == "overflow":
        w[127, 5] = torch.finfo(torch.bfloat16).max      # 255 * 2^120 rounds to 256 * 2^120
    else:
        w[40] = 0
        w[40, 9] = 2.0 ** -125                           # e = -133
    want = W.STATUS_NONFINITE if what in ("nan", "inf") else W.STATUS_ROW_RANGE
    assert W.quantise(w)[3] == want
    wd = w.to(dev)
    data = torch.full((N * K,), 0x5A, dtype=torch.uint8, device=dev)
    exps = torch.full((N,), 0x5A, dtype=torch.int8, device=dev)
    twin = torch.full((N, K), 7.0, dtype=torch.bfloat16, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = L.cs_gemm_w8_pack(wd.data_ptr(), K, N, K, data.data_ptr(), exps.data_ptr(), twin.data_ptr(), K,
                           status.data_ptr(), ops._stream())
    lib.check(rc, "cs_gemm_w8_pack")
    assert int(status.item()) == want
    assert bool((data == 0x5A).all()) and bool((exps == 0x5A).all()) and bool((twin == 7.0).all())
    keep = wd.clone()
    with pytest.raises(ops.CSError, match="refused"):
        ops.gemm_w8_pack(wd, twin_out=wd)
    assert torch.equal(R.bits(wd), R.bits(keep))


def test_pack_rejects_bad_arguments(ops, dev):
    w = torch.zeros(24, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ops.CSError):
        ops.gemm_w8_pack(w)                              # N % 16
    with pytest.raises(ops.CSError):
        ops.gemm_w8_pack(torch.zeros(16, 96, dtype=torch.bfloat16, device=dev))     # K % 64
    with pytest.raises(ops.CSError):
        ops.gemm_w8_pack(torch.zeros(16, 64, dtype=torch.float16, device=dev))
