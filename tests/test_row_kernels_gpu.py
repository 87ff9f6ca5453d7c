"""cs_add_rms_norm and cs_gated_act (csrc/norm.hip) element by element against fp64 torch on the
same bf16 inputs, at the widths where the launch changes shape (d / 8 = 256, 512, 1024 threads
per row, the 16-vectors-per-thread loop above 8192), the model widths 2304 / 4608, d = 8 and
the limit 32768; strided operands and outputs with guard columns; every s_out mode.

The reference emulates exactly the roundings include/consensus_scoring.h defines -- s =
bf16(a + b), bf16(act(gate)) before the product -- and everything else is fp64.

Bounds (per element, derived from the arithmetic; measured maxima are printed under -s and
recorded in DESIGN.md):

* cs_add_rms_norm: s_out is bit-exact (the fp32 sum of two bf16 values rounds to bf16 as the
  exact sum does: it is inexact only when the smaller operand is below 2^-16 of the larger,
  far from a bf16 midpoint).  y is one bf16 rounding of an fp32 result:
  |y - ref| <= 2^-8 |ref| + 2^-20 rms(ref row).
* cs_gated_act: the fp32 activation may flip the rounding of bf16(act(gate)) by one bf16 ulp
  (2^-7 relative) and the product is rounded once more (2^-9): 2^-6 |ref|, plus an absolute
  floor for what fp32 cannot hold: 2^-121 max(1, |up|) (fp32 exp(-x) overflows at 2^128, so
  SiLU of a gate below -88.7 comes out as -0 where the true value is up to 88.7 * 2^-128 <
  2^-121; below the smallest normal 2^-126 only absolute precision exists anyway), and for
  tanh-GeLU 2^-23 |gate up| -- the kernel evaluates 0.5 x (1 + tanh(u)) in fp32 as PyTorch
  does, and 1 + tanh(u) near tanh(u) = -1 is known only to an ulp of 1 (2^-24, two ulps of
  tanhf allowed), so for gates in about [-5.6, -3.5] the activation carries an absolute error of
  up to 2^-23 |x| that no relative bound covers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = -777.0                     # exactly representable in bf16
EPS = 1e-6


def _strided(rows, d, ld, off, dev, fill=None):
    """A [rows, d] column slice at column ``off`` of a [rows, ld] buffer of GUARD."""
    buf = torch.full((rows, ld), GUARD, dtype=BF, device=dev)
    view = buf[:, off:off + d]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf, off, d):
    return bool((buf[:, :off] == GUARD).all()) and bool((buf[:, off + d:] == GUARD).all())


LAYOUTS = [("contiguous", 0, 0), ("ld=d+8", 8, 0), ("ld=d+264", 264, 128)]   # name, pad, offset


def _norm_inputs(rows, d, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(rows, d, generator=g) * 2
    b = torch.randn(rows, d, generator=g)
    if rows >= 3:
        a[1] = 0.0                                   # an all-zero row (a and b)
        b[1] = 0.0
        a[2, (d * 5) // 8] = 1e4                     # an outlier two thirds into the row
    else:
        a[0, d - 1] = 1e4
    w = torch.randn(d, generator=g) * 0.1
    return a.to(BF).to(dev), b.to(BF).to(dev), w.to(BF).to(dev)


def _norm_ref(a, b, w, plus_one):
    """(s bf16, y fp64, per-row rms of y fp64) with the header's roundings."""
    s = a if b is None else (a.double() + b.double()).to(BF)
    S = s.double()
    g = (1.0 + w.double()) if plus_one else w.double()
    y = S * torch.rsqrt((S * S).mean(-1, keepdim=True) + EPS) * g
    return s, y, y.pow(2).mean(-1, keepdim=True).sqrt()


def _norm_excess(y, y_ref, rms):
    """max over elements of |y - ref| / (2^-8 |ref| + 2^-20 rms): <= 1 passes."""
    tol = 2.0 ** -8 * y_ref.abs() + 2.0 ** -20 * rms
    err = (y.double() - y_ref).abs()
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    return bool(ok.all()), float(ratio.max())


NORM_D = [8, 248, 2048, 2056, 2304, 4096, 4104, 4608, 8192, 8200, 32760, 32768]


@pytest.mark.parametrize("d", NORM_D)
def test_add_rms_norm_per_element(ops, dev, d):
    worst = 0.0
    for rows in (1, 3):
        a, b, w = _norm_inputs(rows, d, dev, seed=d + rows)
        for plus_one in (False, True):
            for with_b in (False, True):
                s_ref, y_ref, rms = _norm_ref(a, b if with_b else None, w, plus_one)
                for lname, pad, off in LAYOUTS:
                    ld = d + pad
                    for s_mode in ("none", "alias", "separate"):
                        tag = (d, rows, plus_one, with_b, lname, s_mode)
                        abuf, av = _strided(rows, d, ld, off, dev, a)
                        bbuf, bv = _strided(rows, d, ld, off, dev, b)
                        obuf, ov = _strided(rows, d, ld, off, dev)
                        sbuf, sv = (abuf, av) if s_mode == "alias" else _strided(rows, d, ld, off, dev)
                        y = ops.add_rms_norm(av, w, EPS, b=bv if with_b else None,
                                             plus_one=plus_one, out=ov,
                                             s_out=None if s_mode == "none" else sv)
                        assert y.data_ptr() == ov.data_ptr()
                        ok, ratio = _norm_excess(ov, y_ref, rms)
                        worst = max(worst, ratio)
                        assert ok, (tag, ratio)
                        assert _guards_intact(obuf, off, d), tag
                        assert _guards_intact(abuf, off, d) and _guards_intact(bbuf, off, d), tag
                        assert torch.equal(bv, b), tag
                        if s_mode == "none":
                            assert torch.equal(av, a), tag
                        else:
                            assert torch.equal(sv, s_ref), tag          # bit-exact
                            assert _guards_intact(sbuf, off, d), tag
                            if s_mode == "separate":
                                assert torch.equal(av, a), tag
    print(f"add_rms_norm d={d}: max |y - ref| / bound = {worst:.3f}")


def test_add_rms_norm_per_element_70000_rows(ops, dev):
    """More rows than a 16-bit grid index holds, d = 256, every row checked."""
    rows, d = 70000, 256
    g = torch.Generator(device=dev).manual_seed(70000)
    a = (torch.randn(rows, d, generator=g, device=dev) * 2).to(BF)
    b = torch.randn(rows, d, generator=g, device=dev).to(BF)
    w = (torch.randn(d, generator=g, device=dev) * 0.1).to(BF)
    a[12345] = 0.0
    b[12345] = 0.0
    a[69999, 100] = 1e4
    s_ref, y_ref, rms = _norm_ref(a, b, w, True)
    a2 = a.clone()
    obuf, ov = _strided(rows, d, d + 8, 0, dev)
    ops.add_rms_norm(a2, w, EPS, b=b, plus_one=True, s_out=a2, out=ov)
    ok, ratio = _norm_excess(ov, y_ref, rms)
    print(f"add_rms_norm 70000 x 256: max |y - ref| / bound = {ratio:.3f}")
    assert ok, ratio
    assert torch.equal(a2, s_ref)
    assert _guards_intact(obuf, 0, d)


def test_add_rms_norm_splitk_refusals(ops, dev):
    """Split partials are refused (CS_ERR_INVALID = -1, nothing launched) above d = 8192 and
    for splits outside 1..16."""
    L = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream

    def call(d, splits, n_part):
        rows = 2
        a = torch.zeros(rows, d, dtype=BF, device=dev)
        w = torch.ones(d, dtype=BF, device=dev)
        y = torch.full((rows, d), GUARD, dtype=BF, device=dev)
        part = torch.zeros(n_part, rows, d, dtype=torch.float32, device=dev)
        rc = L.cs_add_rms_norm_splitk(a.data_ptr(), d, part.data_ptr(), splits, None, None, 0,
                                      w.data_ptr(), rows, d, EPS, 0, y.data_ptr(), d, st)
        torch.cuda.synchronize()
        assert bool((y == GUARD).all()) or rc == 0
        return rc

    assert call(8192, 2, 2) == 0
    assert call(8200, 2, 2) == -1
    assert call(32768, 2, 2) == -1
    assert call(256, 0, 1) == -1
    assert call(256, 17, 17) == -1
    assert call(256, 16, 16) == 0
    part = ops.SplitPartials(torch.zeros(2, 2, 8200, dtype=torch.float32, device=dev))
    with pytest.raises(ops.CSError, match=r"status -1"):
        ops.add_rms_norm(torch.zeros(2, 8200, dtype=BF, device=dev),
                         torch.ones(8200, dtype=BF, device=dev), EPS, b=part)


# ------------------------------------------------------------------------------------------
def _act64(x, act):
    if act == "silu":
        return x * torch.sigmoid(x)
    k0, k1 = 0.7978845608028654, 0.044715
    return 0.5 * x * (1.0 + torch.tanh(k0 * (x + k1 * x * x * x)))


def _gated_ref(gate, up, act):
    a = _act64(gate.double(), act).to(BF)              # the header's rounding
    return a.double() * up.double()


def _gated_excess(out, ref, gate, up, act):
    G, U = gate.double().abs(), up.double().abs()
    tol = 2.0 ** -6 * ref.abs() + 2.0 ** -121 * U.clamp_min(1.0)
    if act == "gelu_tanh":
        tol = tol + 2.0 ** -23 * G * U
    err = (out.double() - ref).abs()
    rel = err / ref.abs().clamp_min(1e-300)
    big = ref.abs() >= 2.0 ** -6 * U            # where the relative term governs
    return bool((err <= tol).all()), float((err / tol).max()), \
        float(rel[big].max()) if bool(big.any()) else 0.0


@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
@pytest.mark.parametrize("F", [8, 2040, 2048, 2056, 14336])
def test_gated_act_per_element(ops, dev, F, act):
    worst = worst_rel = 0.0
    for rows in (1, 29):
        g = torch.Generator(device="cpu").manual_seed(F + rows)
        gu = (torch.randn(rows, 2 * F, generator=g) * 3).to(BF).to(dev)
        gate, up = gu[:, :F], gu[:, F:]                 # halves of one buffer (ld = 2F)
        ref = _gated_ref(gate, up, act)
        for layout in ("halves", "separate"):
            for lname, pad, off in LAYOUTS:
                tag = (F, act, rows, layout, lname)
                if layout == "halves":
                    gv, uv = gate, up
                else:                                   # separate buffers, different strides
                    _, gv = _strided(rows, F, F + 8, 0, dev, gate)
                    _, uv = _strided(rows, F, F + 264, 128, dev, up)
                obuf, ov = _strided(rows, F, F + pad, off, dev)
                out = ops.gated_act(gv, uv, act, out=ov)
                assert out.data_ptr() == ov.data_ptr()
                ok, ratio, rel = _gated_excess(ov, ref, gate, up, act)
                worst, worst_rel = max(worst, ratio), max(worst_rel, rel)
                assert ok, (tag, ratio)
                assert _guards_intact(obuf, off, F), tag
        assert torch.equal(ops.gated_act(gate, up, act), ov), (F, act, rows)   # out=None path
    print(f"gated_act {act} F={F}: max err / bound = {worst:.3f}, "
          f"max relative error where |ref| >= 2^-6 |up| = {worst_rel:.2e}")


@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_gated_act_sweeps_every_finite_gate_in_range(ops, dev, act):
    """Every finite bf16 gate in [-100, 100] (both zeros, subnormals) against up = 1, -3, 2^-100:
    within the bound, never NaN, and large negative gates give a zero of either sign."""
    gates = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)
    gates = gates[torch.isfinite(gates.float()) & (gates.float().abs() <= 100.0)]
    n = gates.numel()
    assert n > 34000
    F = (n + 7) // 8 * 8
    gate = torch.zeros(3, F, dtype=BF)
    gate[:, :n] = gates
    up = torch.ones(3, F, dtype=BF)
    up[1] = -3.0
    up[2] = 2.0 ** -100
    gate, up = gate.to(dev), up.to(dev)
    out = ops.gated_act(gate, up, act)
    assert not bool(torch.isnan(out).any())
    ref = _gated_ref(gate, up, act)
    ok, ratio, rel = _gated_excess(out, ref, gate, up, act)
    print(f"gated_act {act} gate sweep ({n} patterns): max err / bound = {ratio:.3f}, "
          f"max relative error where |ref| >= 2^-6 |up| = {rel:.2e}")
    assert ok, ratio
    far = gate[0].float() <= -90.0
    assert bool(far.any()) and bool((out[0][far] == 0).all())      # -0 or 0, not NaN
    # positive gates pass through: act(x) -> x
    big = gate[0].float() >= 20.0
    assert torch.equal(out[0][big], gate[0][big])
