"""Model.quantize_fp8 and the `@fp8` model identifier end to end: the bf16 weights become the
restatement's twins (tests/w8_ref.py) bit for bit, the decode-step GEMMs run on the FP8 copies
and agree with the bf16 routes on the same twins within the bound of the existing route
comparisons (tests/test_gemm_gpu.py `_tol`: only the accumulation order differs), row counts
above the kernel's range stay bitwise on the bf16 routes, and a graph replay equals the eager
step.

The residual adds matter for this: Llama's twin adds the output and down projections to the
residual stream inside hipBLASLt's epilogue (ops.linear_into_residual: the fp32 product added,
one rounding), so the FP8 route adds them in its own kernel's epilogue (cs_gemm_bf16_w8_add)
where the twin takes that route, and leaves them to the residual add's launch (product
rounded, then the sum) where the twin does.  Rounding the product first instead puts the
tiny-llama hidden states 5 to 10 times over the bound (the test prints that figure for two
bf16 routes of the twin itself, for scale).  Measured on an MI355X: both configs agree
bitwise in every forward_streams case; generation log-probs within 0.001 of the bound."""
import importlib

import numpy as np
import pytest
import torch

import gemm_ref as R
import w8_ref as W
from conftest import PKG_DIR as PKG

pytestmark = pytest.mark.gpu

OVERRIDES = dict(d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512)


def _tol(ref):                # tests/test_gemm_gpu.py
    return ref.abs() * 2.0 ** -7 + 1e-3 * ref.abs().max()


def _mods():
    return (importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".engine"),
            importlib.import_module(PKG + ".runtime"), importlib.import_module(PKG + ".tokenizer"))


def _engine(preset, dev, seed=3, overrides=OVERRIDES, weights=None):
    M, E, _, _ = _mods()
    cfg = M.preset(preset, **overrides)
    return E.ScoringEngine(M.Model(cfg, dev, torch.bfloat16, seed=seed, weights=weights), reuse_caches=0)


def _twin_engine(eng):
    """The same (already rounded) bf16 weights in a model without FP8 copies."""
    M, E, _, _ = _mods()
    w = {k: v.clone() for k, v in eng.model.w.items()}
    model = M.Model(eng.model.cfg, eng.device, torch.bfloat16, weights=w)
    assert not model.w8
    return E.ScoringEngine(model, reuse_caches=0)


@pytest.fixture(scope="module", params=["tiny-llama", "tiny-gemma"])
def pair(request, dev):
    """(FP8 engine, twin engine, the weights before rounding) of the all-eligible config."""
    eng = _engine(request.param, dev)
    before = {n: w.clone() for n, (w, _) in eng.model.decode_weights().items()}
    eng.model.quantize_fp8()
    return eng, _twin_engine(eng), before


def test_every_decode_weight_becomes_its_twin_and_keeps_an_fp8_copy(pair):
    eng, _, before = pair
    m = eng.model
    names = set(m.decode_weights())
    assert set(m.w8) == names                            # every projection is eligible here
    assert ("lm_head" in names) and len(names) == 1 + 4 * m.cfg.n_layers
    for name, (w, _) in m.decode_weights().items():
        codes, exps, twin, status = W.quantise(before[name].cpu())
        assert status == 0
        assert torch.equal(R.bits(w.cpu()), R.bits(twin)), name
        fw = m.w8[name]
        assert np.array_equal(W.unpack(fw.data.cpu().numpy(), *w.shape), codes), name
        assert np.array_equal(fw.exps.cpu().numpy().astype(np.int64), exps), name
        assert not torch.equal(w, before[name]), name    # the rounding did change the weight
    # the separate q / k / v and gate / up weights are views of the fused, rounded ones
    assert m.w["l0.wq"].data_ptr() == m.wf["l0.qkv"].data_ptr()
    # the norms are left alone; a second call is the identity on the weights
    snap = {k: v.clone() for k, v in m.w.items()}
    m.quantize_fp8()
    for k, v in m.w.items():
        assert torch.equal(R.bits(v), R.bits(snap[k])), k
    assert set(m.w8) == names


def test_ineligible_shapes_are_rounded_and_fall_through(ops, dev):
    """Unmodified tiny-llama: wo and w_down have 64 output rows (N % 128 != 0): rounded to the
    twin all the same, no FP8 copy; ops.linear with an Fp8Weight above the kernel's row range
    is the bf16 route, bitwise."""
    eng = _engine("tiny-llama", dev, overrides={})
    m = eng.model
    before = {n: w.clone() for n, (w, _) in m.decode_weights().items()}
    m.quantize_fp8()
    assert "l0.wo" not in m.w8 and "l1.w_down" not in m.w8 and "l0.qkv" in m.w8 and "l0.gate_up" in m.w8
    for name, (w, _) in m.decode_weights().items():
        assert torch.equal(R.bits(w.cpu()), R.bits(W.quantise(before[name].cpu())[2])), name
    fw, w = m.w8["l0.gate_up"], m.wf["l0.gate_up"]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(W.MAX_ROWS + 1, w.shape[1], generator=g).to(dev, torch.bfloat16)
    for gated in (False, True):
        assert not ops.gemm_w8_serves(x.shape[0], *w.shape, gated)
        assert torch.equal(ops.linear(x, w, gated=gated, packed=fw), ops.linear(x, w, gated=gated))
        y = ops.linear(x[:7], w, gated=gated, packed=fw)
        assert ops.gemm_w8_serves(7, *w.shape, gated)
        assert torch.equal(y, ops.gemm_w8(x[:7], fw, gated=gated))
    # the residual route of a served shape: the FP8 kernel's own epilogue, h + product rounded once
    g2 = torch.Generator().manual_seed(2)
    h0 = torch.randn(7, w.shape[0], generator=g2).to(dev, torch.bfloat16)
    h = h0.clone()
    assert ops.gemm_choice(7, *w.shape) is None          # (the twin takes hipBLASLt's epilogue here)
    assert ops.linear_into_residual(x[:7], w, h, packed=fw) is True
    want = (h0.double() + x[:7].double() @ w.double().t())
    err = (h.double() - want).abs()
    assert bool((err <= 2.0 ** -8 * want.abs() + 1e-3 * want.abs().max()).all())
    assert torch.equal(h, ops.gemm_w8_add(x[:7], fw, h0.clone()))
    # above the kernel's range the call is the twin's: hipBLASLt's epilogue, bitwise
    big = torch.randn(x.shape[0], w.shape[0], generator=g2).to(dev, torch.bfloat16)
    a, b = big.clone(), big.clone()
    assert ops.linear_into_residual(x, w, a, packed=fw) is True and ops.linear_into_residual(x, w, b) is True
    assert torch.equal(a, b)


def _streams(eng, prefixes, n_str, T, toks):
    E = _mods()[1]
    m, c, dev = eng.model, eng.model.cfg, eng.device
    S = len(prefixes) * n_str
    pfx = E.fused_prefix(eng.prefill(prefixes))
    hk = [torch.zeros(S, c.n_kv_heads, 32, c.head_dim, dtype=torch.bfloat16, device=dev)
          for _ in range(c.n_layers)]
    hv = [torch.zeros(S, c.n_kv_heads, 1, c.head_dim, 32, dtype=torch.bfloat16, device=dev)
          for _ in range(c.n_layers)]
    hb = torch.zeros(1, dtype=torch.int32, device=dev)
    return m.forward_streams(toks.reshape(-1), pfx, hk, hv, hb, n_str, T)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("P,n_str", [(1, 5), (3, 16), (3, 27)], ids=["S5", "S48", "S81"])
def test_forward_streams_on_fp8_copies_against_the_twin_routes(ops, pair, P, n_str, T):
    eng, twin, _ = pair
    dev = eng.device
    S = P * n_str
    g = torch.Generator().manual_seed(100 * S + T)
    prefixes = [torch.randint(5, 380, (n,), generator=g).tolist() for n in (30, 52, 41)[:P]]
    toks = torch.randint(5, 380, (S, T), generator=g).to(dev)
    calls = []
    orig = ops.gemm_w8, ops.gemm_w8_partials, ops.gemm_w8_add
    ops.gemm_w8 = lambda *a, **k: (calls.append("y"), orig[0](*a, **k))[1]
    ops.gemm_w8_partials = lambda *a, **k: (calls.append("p"), orig[1](*a, **k))[1]
    ops.gemm_w8_add = lambda *a, **k: (calls.append("a"), orig[2](*a, **k))[1]
    try:
        h8 = _streams(eng, prefixes, n_str, T, toks)
    finally:
        ops.gemm_w8, ops.gemm_w8_partials, ops.gemm_w8_add = orig
    ref = _streams(twin, prefixes, n_str, T, toks)
    assert h8.shape == ref.shape == (S * T, eng.model.cfg.d_model)
    if S * T > W.MAX_ROWS:
        assert not calls                                  # every projection stayed on the twin
        assert torch.equal(h8, ref)
        return
    assert len(calls) == 4 * eng.model.cfg.n_layers, calls
    err = (h8.float() - ref.float()).abs()
    tol = _tol(ref.float())
    # for scale (printed, not asserted): the twin model on another of its own bf16 routes,
    # cs_gemm_bf16 variant 1 unsplit in place of hipBLASLt for every projection
    choice = ops.gemm_choice
    ops.gemm_choice = lambda *a, **k: {"variant": 1, "splits": 1, "packed": False}
    try:
        alt = _streams(twin, prefixes, n_str, T, toks)
    finally:
        ops.gemm_choice = choice
    e_alt = (alt.float() - ref.float()).abs()
    print(f"S {S} T {T}: fp8 vs twin max err / bound {float((err / tol).max()):.3f} (max err "
          f"{float(err.max()):.5f}, {float((err > tol).float().mean()):.2%} of elements over); two bf16 "
          f"routes of the twin {float((e_alt / tol).max()):.3f} (max err {float(e_alt.max()):.5f})")
    assert bool((err <= tol).all()), float((err / tol).max())


def test_graph_replay_equals_the_eager_step(pair):
    eng, _, _ = pair
    E = _mods()[1]
    g = torch.Generator().manual_seed(11)
    prefixes = [torch.randint(5, 380, (n,), generator=g).tolist() for n in (40, 23, 61)]
    B, steps = 4, 5
    cache = eng.prefill(prefixes)
    fus = E.DecodeState(eng, cache, n_prefix=3, n_beams=B, max_steps=steps)
    eag = E.DecodeState(eng, cache, n_prefix=3, n_beams=B, max_steps=steps, use_graphs=False)
    for step in range(steps):
        parent = [0] * B if step == 0 else torch.randint(0, B, (B,), generator=g).tolist()
        toks = torch.randint(5, 380, (B,), generator=g).tolist()
        fus.advance(parent, toks)
        eag.advance(parent, toks)
        torch.cuda.synchronize()
        assert torch.equal(fus.hidden, eag.hidden), step
    fus.release()


def test_fp8_identifier_engines(pair, dev):
    """The engine registered under an `@fp8` id against its twin engine: prompt log-probs
    bitwise (prefill and the head run on the twin: more rows than the FP8 kernel serves), the
    step log-probs of generate_streams within the route bound where both drew the same tokens."""
    eng, twin, _ = pair
    M, E, rt, T = _mods()
    utils = importlib.import_module(PKG + ".utils")
    fam = "gemma2" if eng.model.cfg.family == "gemma2" else "llama3"
    tok = T.CharTokenizer(fam, vocab_size=eng.model.cfg.vocab)
    ids = {"w8-fixture@fp8": eng, "w8-fixture-twin": twin}
    try:
        for k, e in ids.items():
            rt.register_engine(k, e, tok)
        assert rt.get_engine("w8-fixture@fp8")[0] is eng
        with pytest.raises(rt.ops.CSError, match="registered engine object"):
            rt.register_engine("w8-plain", twin, tok)
            rt.get_engine("w8-plain@fp8")
        user = "Should the town build a new library? " * 4
        a = utils.get_prompt_logprobs("w8-fixture@fp8", "You are helpful.", user)
        b = utils.get_prompt_logprobs("w8-fixture-twin", "You are helpful.", user)
        assert len(a[1]) > W.MAX_ROWS and a[0] == b[0] and a[1] == b[1]
        assert all(isinstance(v, float) and np.isfinite(v) for v in a[1][1:])

        prompts = [tok.render_chat(None, q)[0] for q in ("Parks or roads?", "A longer question about buses.")]
        seeds = [[1, 2, 3, 4], [5, 6, 7, 8]]
        t8, l8 = rt.generate_streams(eng, tok, prompts, seeds, max_tokens=12, return_logprobs=True)
        tt, lt = rt.generate_streams(twin, tok, prompts, seeds, max_tokens=12, return_logprobs=True)
        ref, got, total = [], [], 0
        for p in range(2):
            for i in range(4):
                total += min(len(t8[p][i]), len(tt[p][i]))
                assert len(l8[p][i]) >= 1 and len(lt[p][i]) >= 1
                ref.append(lt[p][i][0])                   # the first step has the same history in both
                got.append(l8[p][i][0])
                for s in range(1, min(len(t8[p][i]), len(tt[p][i]))):
                    if t8[p][i][:s] != tt[p][i][:s]:
                        break
                    ref.append(lt[p][i][s])
                    got.append(l8[p][i][s])
        ref, got = torch.tensor(ref, dtype=torch.float64), torch.tensor(got, dtype=torch.float64)
        share = len(ref) / max(total, 1)
        err, tol = (got - ref).abs(), _tol(ref)
        msg = (f"{len(ref)} of {total} steps compared ({share:.0%}), max err / bound "
               f"{float((err / tol).max()):.3f}, max err {float(err.max()):.5f}")
        print(msg)
        assert len(ref) >= 8 and bool((err <= tol).all()), msg
    finally:
        with rt._lock:
            for k in list(ids) + ["w8-plain"]:
                rt._ENGINES.pop(k, None)


def test_random_preset_with_and_without_the_suffix(dev):
    M, E, rt, T = _mods()
    ident = "random:tiny-llama"
    try:
        e16, _ = rt.get_engine(ident)                                # (cached under the plain id first)
        e8, _ = rt.get_engine(ident + "@fp8")
        assert e8 is not e16 and e8.model.w8 and not e16.model.w8
        assert rt.get_engine(ident + "@fp8")[0] is e8                # cached under the full id
        fresh = M.Model(M.preset("tiny-llama"), dev, torch.bfloat16, seed=0)
        for name, (w, _) in e16.model.decode_weights().items():      # the plain id is unrounded
            assert torch.equal(w, fresh.decode_weights()[name][0]), name
            twin = W.quantise(w.cpu())[2]
            assert torch.equal(R.bits(e8.model.decode_weights()[name][0].cpu()), R.bits(twin)), name
        e32 = E.ScoringEngine(M.Model(M.preset("tiny-llama"), dev, torch.float32, seed=0), reuse_caches=0)
        with pytest.raises(rt.ops.CSError):
            e32.model.quantize_fp8()
    finally:
        with rt._lock:
            rt._ENGINES.pop(ident + "@fp8", None)
            rt._ENGINES.pop(ident, None)
