"""GPU tests of the text encoder's kernels, each against the fp64 restatement
(tests/encoder_ref.py) on identical bf16 inputs, and each relaunched for bit identity.

Bounds (none is taken from what the kernels give):
  LayerNorm   |out - ref| <= 2^-8 |ref| + 1e-5 (|w xhat| + |b|): one bf16 rounding of the
              output plus fp32 arithmetic on the two terms.  bf16 keeps 8 significant bits, so
              one rounding to nearest is up to 2^-8 of the value just above a power of two: the
              first term is one rounding with nothing to spare (measured on MI355X: up to 0.992
              of the bound), and a second rounding anywhere would exceed it.
  GELU        2^-8 |ref| + 1e-6 (measured: up to 0.967 of the bound).
  attention   tests/attention_ref.py's 2^-7 A + 1e-30, A = sum_i p_i |v_i|.
  cosine      1e-13 against scipy's formula (fp64 both sides, d <= 1024 products of O(1/d)),
              1e-12 against the published rows.
"""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import attention_ref as ar
import encoder_ref as er

pytestmark = pytest.mark.gpu


def to_dev(x, dev):
    """bf16-representable float32 array -> bf16 device tensor, bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(er.bf16_round(x), x)
    return torch.from_numpy(er.bf16_bits(x)).view(torch.bfloat16).to(dev)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def rnd(rng, *shape, std=1.0, mean=0.0):
    return er.bf16_round((rng.standard_normal(shape) * std + mean).astype(np.float32))


def check_ln(out, ref, wx, b):
    bound = 2.0 ** -8 * np.abs(ref) + 1e-5 * (np.abs(wx) + np.abs(b))
    err = np.abs(out - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"LayerNorm max err / bound = {worst:.3f}")
    assert (err <= bound).all(), worst


# --- LayerNorm kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 1024])
@pytest.mark.parametrize("rows", [1, 65])
def test_add_layer_norm(ops, dev, d, rows):
    rng = np.random.default_rng(100 + d + rows)
    x, r = rnd(rng, rows, d, std=2.0, mean=0.5), rnd(rng, rows, d)
    x[rows // 2], r[rows // 2] = 1.5, 0.25          # a constant row: variance 0, eps decides
    w, b = rnd(rng, d, std=0.3, mean=1.0), rnd(rng, d, std=0.5)
    X, R, W, B = (to_dev(a, dev) for a in (x, r, w, b))
    out = ops.add_layer_norm(X, R, W, B, er.LN_EPS)
    ref, wx = er.layer_norm(x.astype(np.float64) + r, w, b)
    check_ln(host(out), ref, wx, b.astype(np.float64))
    assert np.array_equal(host(out)[rows // 2], b.astype(np.float64))
    assert torch.equal(out, ops.add_layer_norm(X, R, W, B, er.LN_EPS))
    # no residual, and in place over x
    ref1, wx1 = er.layer_norm(x, w, b)
    o1 = ops.add_layer_norm(X, None, W, B, er.LN_EPS)
    check_ln(host(o1), ref1, wx1, b.astype(np.float64))
    X2 = X.clone()
    assert ops.add_layer_norm(X2, R, W, B, er.LN_EPS, out=X2) is X2 and torch.equal(X2, out)


@pytest.mark.parametrize("d", [64, 128, 1024])
@pytest.mark.parametrize("lens", [[1], [1, 31, 33]])
def test_embed_layer_norm(ops, dev, d, lens):
    rng = np.random.default_rng(200 + d + len(lens))
    vocab, n_pos = 97, 40
    word, pos, typ = rnd(rng, vocab, d), rnd(rng, n_pos, d), rnd(rng, 2, d)
    word[5], pos[0], typ[0] = 0.5, 0.25, 0.125      # id 5 at offset 0: a constant row
    w, b = rnd(rng, d, std=0.3, mean=1.0), rnd(rng, d, std=0.5)
    ids = [rng.integers(0, vocab, size=n) for n in lens]
    ids[-1][-1] = vocab - 1
    ids[-1][0] = 5
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    flat = torch.from_numpy(np.concatenate(ids).astype(np.int32)).to(dev)
    cu_d = torch.from_numpy(cu).to(dev)
    tabs = [to_dev(a, dev) for a in (word, pos, typ, w, b)]
    out = ops.embed_layer_norm(flat, cu_d, max(lens), *tabs, er.LN_EPS)
    x = np.concatenate([word[i].astype(np.float64) + pos[:len(i)] + typ[0] for i in ids])
    ref, wx = er.layer_norm(x, w, b)
    check_ln(host(out), ref, wx, b.astype(np.float64))
    assert np.array_equal(host(out)[cu[-2]], b.astype(np.float64))
    assert torch.equal(out, ops.embed_layer_norm(flat, cu_d, max(lens), *tabs, er.LN_EPS))


def test_embed_layer_norm_reports_bad_ids_and_long_texts(ops, dev):
    rng = np.random.default_rng(3)
    d, vocab, n_pos = 64, 50, 8
    tabs = [to_dev(rnd(rng, *s), dev) for s in ((vocab, d), (n_pos, d), (2, d), (d,), (d,))]
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device=dev)
    for bad in (vocab, -1):
        ids = torch.tensor([1, 2, 3, 4, bad, 6, 7, 8], dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = ops.embed_layer_norm(ids, cu, 5, *tabs, 1e-12, status=status)
        assert int(status.item()) == -1
        assert not out[4].any() and out[3].any() and out[5].any()
        with pytest.raises(ops.CSError, match="status -1"):
            ops.embed_layer_norm(ids, cu, 5, *tabs, 1e-12)
    # a text longer than the position table: refused before any launch
    ids = torch.ones(9, dtype=torch.int32, device=dev)
    with pytest.raises(ops.CSError, match="position table"):
        ops.embed_layer_norm(ids, torch.tensor([0, 9], dtype=torch.int32, device=dev), 9, *tabs, 1e-12)
    # ... and one the host's max_seqlen understates: reported by the device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.embed_layer_norm(ids, torch.tensor([0, 9], dtype=torch.int32, device=dev), 8, *tabs, 1e-12,
                         status=status)
    assert int(status.item()) == -1


# --- GELU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F", [(1, 16), (65, 2056)])
def test_gelu(ops, dev, rows, F):
    rng = np.random.default_rng(rows)
    x = rnd(rng, rows, F, std=2.0)
    pts = er.bf16_round(np.float32([0.0, 1e-3, 1.0, 6.0, 40.0]))
    x[0, :10] = np.concatenate([pts, -pts])
    x[-1, -10:] = np.concatenate([-pts, pts])
    X = to_dev(x, dev)
    out = ops.gelu(X)
    ref = er.gelu(x)
    err = np.abs(host(out) - ref)
    bound = 2.0 ** -8 * np.abs(ref) + 1e-6
    print(f"GELU max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert host(out)[0, 4] == 40.0 and host(out)[0, 9] == 0.0 and host(out)[0, 0] == 0.0
    assert torch.equal(out, ops.gelu(X))
    X2 = X.clone()
    ops.gelu(X2, out=X2)
    assert torch.equal(X2, out)


# --- attention ---------------------------------------------------------------------------------
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512]


def run_attn(ops, dev, qkv, cu, H):
    Q = to_dev(qkv, dev)
    cu_d = torch.from_numpy(np.asarray(cu, dtype=np.int32)).to(dev)
    mx = int(np.diff(cu).max())
    out = ops.encoder_attention(Q, cu_d, mx, H)
    assert torch.equal(out, ops.encoder_attention(Q, cu_d, mx, H)), "relaunch differs"
    return host(out)


def check_attn(out, qkv, cu, H, what=""):
    ref, A = er.ragged_attention(qkv, cu, H)
    worst = float((np.abs(out - ref) / ar.bound_of(A)).max())
    print(f"attention {what}: max err / bound = {worst:.3f}")
    assert (np.abs(out - ref) <= ar.bound_of(A)).all(), worst
    return ref


@pytest.mark.parametrize("H", [2, 16])
def test_attention_every_length(ops, dev, H):
    rng = np.random.default_rng(300 + H)
    lens = list(rng.permutation(LENGTHS))
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = rnd(rng, cu[-1], 3 * H * 64)
    qkv[:, :H * 64] *= np.float32(2.0)            # scores of a few nats: a peaked softmax
    check_attn(run_attn(ops, dev, qkv, cu, H), qkv, cu, H, f"H={H}")


@pytest.mark.parametrize("H", [2, 16])
def test_attention_planted_key(ops, dev, H):
    """One key per text scores 128 nats above the rest: the output is that key's V row, wherever
    the key sits (first and last of a block, of a text, alone in the last block)."""
    rng = np.random.default_rng(400 + H)
    plan = [(1, 0), (2, 1), (31, 30), (32, 31), (33, 32), (33, 0), (63, 31), (64, 32), (65, 64),
            (127, 95), (128, 127), (129, 128), (129, 96), (511, 510), (512, 511), (512, 255)]
    lens = [n for n, _ in plan]
    cu = np.concatenate([[0], np.cumsum(lens)])
    HD = H * 64
    qkv = rnd(rng, cu[-1], 3 * HD, std=0.25)
    u = np.zeros(64, np.float32)
    u[::4] = 8.0                                   # u.u = 1024: 128 nats at scale 1/8
    for t, (n, j) in enumerate(plan):
        a = cu[t]
        for h in range(H):
            qkv[a:a + n, h * 64:(h + 1) * 64] = u
            qkv[a:a + n, HD + h * 64:HD + (h + 1) * 64] *= np.float32(0.125)
            qkv[a + j, HD + h * 64:HD + (h + 1) * 64] = u
    out = run_attn(ops, dev, qkv, cu, H)
    check_attn(out, qkv, cu, H, f"planted H={H}")
    for t, (n, j) in enumerate(plan):
        a = cu[t]
        want = qkv[a + j, 2 * HD:].astype(np.float64)
        assert np.abs(out[a:a + n] - want).max() <= 2.0 ** -8 * np.abs(want).max() + 1e-30, (n, j)


@pytest.mark.parametrize("H", [2, 16])
def test_attention_staircase_and_extremes(ops, dev, H):
    """Scores that rise (or fall) by half a nat per key -- every key block moves the running
    maximum by 16 nats, so each one rescales, and the waves that share a short text's query
    tile combine partial sums whose maxima differ by tens of nats -- and scores at +-200 nats."""
    rng = np.random.default_rng(500 + H)
    HD = H * 64
    lens = [129, 80, 96, 512, 33, 129, 80, 96, 512, 64, 40]
    kinds = ["up"] * 5 + ["down"] * 4 + ["pm200", "all-200"]
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = rnd(rng, cu[-1], 3 * HD)
    one = np.ones(64, np.float32)
    for t, (n, kind) in enumerate(zip(lens, kinds)):
        a = cu[t]
        for h in range(H):
            q = slice(h * 64, (h + 1) * 64)
            k = slice(HD + h * 64, HD + (h + 1) * 64)
            if kind in ("up", "down"):
                # q.k / 8 = 8 k_j: k_j = j / 16 gives steps of half a nat
                j = np.arange(n, dtype=np.float32) if kind == "up" else np.arange(n, 0, -1, dtype=np.float32)
                qkv[a:a + n, q] = one * er.bf16_round(1.0 + 0.25 * rng.random((n, 1)).astype(np.float32))
                qkv[a:a + n, k] = er.bf16_round(j[:, None] / 16.0 * one)
            else:
                sign = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
                if kind == "all-200":
                    sign[:] = -1.0
                qkv[a:a + n, q] = 5.0 * one                       # 25 * 64 / 8 = 200 nats
                qkv[a:a + n, k] = 5.0 * sign[:, None] * one
    check_attn(run_attn(ops, dev, qkv, cu, H), qkv, cu, H, f"staircase H={H}")


@pytest.mark.parametrize("H", [2, 16])
def test_attention_ignores_the_neighbouring_texts(ops, dev, H):
    rng = np.random.default_rng(600 + H)
    lens = [33, 65, 31]
    cu = np.concatenate([[0], np.cumsum(lens)])
    base = rnd(rng, cu[-1], 3 * H * 64)
    outs = []
    for fill in (1e30, -1e30, 0.0):
        qkv = base.copy()
        qkv[:cu[1]] = er.bf16_round(np.float32(fill))
        qkv[cu[2]:] = er.bf16_round(np.float32(fill))
        Q = to_dev(qkv, dev)
        o = ops.encoder_attention(Q, torch.from_numpy(cu.astype(np.int32)).to(dev), 65, H)
        outs.append(o[cu[1]:cu[2]].clone())
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    ref, A = er.ragged_attention(base[cu[1]:cu[2]], [0, 65], H)
    assert (np.abs(host(outs[2]) - ref) <= ar.bound_of(A)).all()
    # a malformed cu_seqlens touches nothing
    out = torch.full((int(cu[-1]), H * 64), 7.0, dtype=torch.bfloat16, device=dev)
    bad = torch.tensor([0, 500, 400, 129], dtype=torch.int32, device=dev)
    ops.encoder_attention(to_dev(base, dev), bad, 65, H, out=out)
    assert bool((out == 7.0).all())


# --- cs_cosine_welfare ---------------------------------------------------------------------
@pytest.mark.parametrize("S,A,d", [(7, 5, 1024), (1, 1, 3), (70, 4, 257)])
def test_cosine_welfare_matches_scipy(ops, dev, S, A, d):
    from scipy.spatial.distance import cosine

    rng = np.random.default_rng(S + d)
    Es = rng.standard_normal((S, d)).astype(np.float32)
    Ea = rng.standard_normal((A, d)).astype(np.float32)
    Es /= np.linalg.norm(Es, axis=1, keepdims=True)
    Ea[0] = Es[0] * np.float32(3.0)                 # a similarity of 1
    Es_d, Ea_d = torch.from_numpy(Es).to(dev), torch.from_numpy(Ea).to(dev)
    cos, wel = ops.cosine_welfare(Es_d, Ea_d)
    want = np.array([[1.0 - cosine(Es[s].astype(np.float64), Ea[a].astype(np.float64))
                      for s in range(S)] for a in range(A)])
    assert np.abs(cos.cpu().numpy() - want).max() <= 1e-13
    rc, rw = er.cosine_welfare(Es, Ea)
    assert np.abs(cos.cpu().numpy() - rc).max() <= 1e-13
    assert np.abs(wel.cpu().numpy() - rw).max() <= 1e-12
    c2, w2 = ops.cosine_welfare(Es_d, Ea_d)
    assert torch.equal(cos, c2) and torch.equal(wel, w2)


def _pair_with_cosine(c):
    """float32 vectors u, v (8 wide) whose exact cosine is c to ~1e-15: u = (1, 2^-12, 0 ...),
    v carries c split in two float32 words and three words that bring |u| |v| to 1."""
    f32 = lambda x: float(np.float32(float(x)))   # noqa: E731
    u = [1.0, 2.0 ** -12, 0, 0, 0, 0, 0, 0]
    hi = f32(c)
    lo = f32((Fraction(c) - Fraction(hi)) * 2 ** 12)
    v = [hi, lo, 0, 0, 0, 0, 0, 0]
    rest = 1 / (1 + Fraction(2) ** -24) - Fraction(hi) ** 2 - Fraction(lo) ** 2
    for i in (2, 3, 4):
        if rest <= 0:
            break
        y = f32(float(rest) ** 0.5)
        while Fraction(y) ** 2 > rest:
            y = float(np.nextafter(np.float32(y), np.float32(0)))
        v[i] = y
        rest -= Fraction(y) ** 2
    return u, v


def test_cosine_welfare_matches_published_rows(ops, dev, golden_dir):
    import pandas as pd

    df = pd.read_csv(os.path.join(golden_dir, "eval_cosine_published.csv"))
    cols = ["egalitarian_welfare_cosine", "utilitarian_welfare_cosine", "log_nash_welfare_cosine"]
    Es, Ea, want_c, want_w = [], [], [], []
    for _, r in df.iterrows():
        A = int(r.n_agents)
        cs = [float(r[f"cosine_similarity_{j}"]) for j in range(A)]
        pairs = [_pair_with_cosine(c) for c in cs]
        Es.append(pairs[0][0])
        Ea.append([p[1] for p in pairs] + [[0.0] * 8] * (5 - A))
        want_c.append(cs + [np.nan] * (5 - A))
        want_w.append([r[c] for c in cols])
    Es_d = torch.tensor(Es, dtype=torch.float32, device=dev)          # [750, 8]
    Ea_d = torch.tensor(Ea, dtype=torch.float32, device=dev)          # [750, 5, 8]
    got = [ops.cosine_welfare(Es_d[i:i + 1], Ea_d[i, :int(df.n_agents[i])]) for i in range(len(df))]
    worst_c = worst_w = 0.0
    for i, (cos, wel) in enumerate(got):
        A = int(df.n_agents[i])
        worst_c = max(worst_c, float(np.abs(cos.cpu().numpy()[:, 0] - np.array(want_c[i][:A])).max()))
        worst_w = max(worst_w, float(np.abs(wel.cpu().numpy()[:, 0] - np.array(want_w[i])).max()))
    print(f"published rows: max |cos - published| = {worst_c:.2e}, welfare {worst_w:.2e}")
    assert worst_c <= 1e-12 and worst_w <= 1e-12


def test_cosine_welfare_invalid_zero_and_empty_columns(ops, dev):
    rng = np.random.default_rng(9)
    d = 32
    Es = rng.standard_normal((5, d)).astype(np.float32)
    Ea = rng.standard_normal((4, d)).astype(np.float32)
    Es[1] = 0.0                                    # zero-norm statement: every similarity 0.0
    Ea[2] = 0.0                                    # zero-norm opinion
    Ea[3, 7] = np.nan                              # a NaN embedding: None in the reference
    Es[4, 0] = np.inf
    vs = np.array([1, 1, 0, 1, 1], dtype=bool)     # statement 2 has no embedding
    va = np.array([1, 0, 1, 1], dtype=bool)        # opinion 1 has none
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    cos, wel = ops.cosine_welfare(t(Es), t(Ea), t(vs), t(va))
    cos, wel = cos.cpu().numpy(), wel.cpu().numpy()
    rc, rw = er.cosine_welfare(Es, Ea, vs, va)
    assert np.array_equal(np.isnan(cos), np.isnan(rc)) and np.array_equal(np.isnan(wel), np.isnan(rw))
    assert np.nanmax(np.abs(cos - rc)) <= 1e-13 and np.nanmax(np.abs(wel - rw)) <= 1e-12
    assert np.isnan(cos[:, 2]).all() and np.isnan(wel[:, 2]).all()       # all-invalid column
    assert np.isnan(cos[1]).all() and np.isnan(cos[0, 4]) and cos[2, 4] == 0.0
    assert cos[0, 1] == 0.0 and cos[2, 1] == 0.0 and cos[2, 0] == 0.0
    assert cos[3, 1] == 0.0 and np.isnan(cos[3, 0])     # zero vector first, then the NaN
    assert wel[0, 1] == 0.0 and wel[1, 1] == 0.0
    assert wel[2, 1] == pytest.approx(3 * np.log(1e-9), abs=1e-12)
    # uint8 masks and no masks agree with bool / all-valid
    c2, _ = ops.cosine_welfare(t(Es), t(Ea), t(vs.astype(np.uint8)), t(va.astype(np.uint8)))
    assert np.array_equal(np.isnan(c2.cpu().numpy()), np.isnan(cos))
