"""CPU tests of the text encoder's oracle and host side: the fp64 restatement against Hugging
Face's fp64 forward, the cosine / welfare rules against the published evaluation rows, the
reference's None / zero-vector / NaN cases, the C-ABI's argument checks (no launch) and the
WordPiece tokenizer's truncation."""
import ctypes
import math
import os
from importlib import import_module

import numpy as np
import pytest

import encoder_ref as er
from conftest import PKG_DIR


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "encoder_golden.npz"))


@pytest.fixture(scope="module")
def published(golden_dir):
    import pandas as pd

    return pd.read_csv(os.path.join(golden_dir, "eval_cosine_published.csv"))


def _texts(golden, m):
    cu = golden[f"{m}_cu"]
    return [golden[f"{m}_ids"][cu[i]:cu[i + 1]] for i in range(len(cu) - 1)]


def test_weight_recipe_is_bf16_representable():
    w = er.make_weights("tiny")
    assert set(w) == {n for n, _ in er.param_names(er.SHAPES["tiny"]["layers"])}
    for k, v in w.items():
        assert v.dtype == np.float32
        assert np.array_equal(er.bf16_round(v), v), k
    x = np.float32([1.0, 1.00390625, 1.01171875, -3.0e38, 1e-40])
    # ties to even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert er.bf16_round(x)[1] == 1.0 and er.bf16_round(x)[2] == np.float32(1.015625)


def test_restatement_matches_hf_fp64(golden):
    # both fp64: only summation order differs
    ids = _texts(golden, "tiny")
    assert [len(t) for t in ids] == [1, 2, 5, 31, 33, 64, 65, 130]
    e = er.forward(er.make_weights("tiny"), "tiny", ids)
    assert np.abs(e - golden["tiny_emb_f64"]).max() <= 1e-10
    assert np.abs(np.linalg.norm(e, axis=1) - 1.0).max() <= 1e-12


def test_golden_layout(golden):
    for m, lens in (("tiny", [1, 2, 5, 31, 33, 64, 65, 130]), ("bge-large", [2, 33, 128, 512])):
        assert list(np.diff(golden[f"{m}_cu"])) == lens
        n, h = len(lens), er.SHAPES[m]["hidden"]
        assert golden[f"{m}_emb_f32"].shape == (n, h) and golden[f"{m}_emb_f32"].dtype == np.float32
        assert golden[f"{m}_cos_f32"].shape == (n, n)
        err = golden[f"{m}_bf16_eager_err"]
        assert err.shape == (2,) and (err > 0).all() and (err < 0.05).all()
        # the stored cosines are the rules applied to the stored embeddings
        cos, _ = er.cosine_welfare(golden[f"{m}_emb_f32"], golden[f"{m}_emb_f32"])
        assert np.abs(cos - golden[f"{m}_cos_f32"]).max() <= 1e-15
        assert np.abs(golden[f"{m}_emb_f32"] - golden[f"{m}_emb_f64"]).max() < 1e-4


def test_rules_match_published_rows(published):
    assert len(published) == 750 and set(published.n_agents) == {4, 5}
    worst = 0.0
    for _, r in published.iterrows():
        sims = [r[f"cosine_similarity_{j}"] for j in range(int(r.n_agents))]
        assert all(np.isfinite(s) for s in sims)
        got = er.welfare_folds(sims)
        want = (r.egalitarian_welfare_cosine, r.utilitarian_welfare_cosine, r.log_nash_welfare_cosine)
        worst = max(worst, max(abs(g - w) for g, w in zip(got, want)))
    assert worst <= 1e-12


def test_rules_match_scipy():
    from scipy.spatial.distance import cosine

    rng = np.random.default_rng(5)
    for d in (3, 64, 1024):
        u, v = rng.normal(size=d), rng.normal(size=d)
        assert abs(er.cosine_similarity(u, v) - (1 - cosine(u, v))) <= 1e-13
    assert er.cosine_similarity(u, u) == pytest.approx(1.0, abs=1e-15)
    assert er.cosine_similarity(u, -u) == pytest.approx(-1.0, abs=1e-15)


def test_none_zero_and_nan_cases():
    u, z = np.array([1.0, 2.0, 2.0]), np.zeros(3)
    n = np.array([1.0, np.nan, 0.0])
    assert er.cosine_similarity(None, u) is None and er.cosine_similarity(u, None) is None
    assert er.cosine_similarity(z, u) == 0.0 and er.cosine_similarity(u, z) == 0.0
    assert er.cosine_similarity(z, n) == 0.0        # the zero check comes first
    assert er.cosine_similarity(u, n) is None
    # None and non-finite entries are left out of the folds; nothing left: NaN
    eg, ut, ln = er.welfare_folds([0.5, None, float("nan"), 0.25, float("inf")])
    assert (eg, ut) == (0.25, 0.75) and ln == pytest.approx(math.log(0.5) + math.log(0.25), abs=1e-15)
    assert all(math.isnan(x) for x in er.welfare_folds([None, float("nan")]))
    # a zero or negative similarity enters the log fold as log(1e-9)
    assert er.welfare_folds([0.0, -0.5])[2] == pytest.approx(2 * math.log(1e-9), abs=1e-12)
    cos, wel = er.cosine_welfare(np.stack([u, z, u]), np.stack([u, n]), valid_s=[1, 1, 0])
    assert cos[0, 0] == pytest.approx(1.0, abs=1e-15) and np.isnan(cos[1, 0])
    assert (cos[:, 1] == 0.0).all() and np.isnan(cos[:, 2]).all()
    assert wel[1, 0] == cos[0, 0] and wel[1, 1] == 0.0 and np.isnan(wel[:, 2]).all()


# --- the C-ABI's argument checks: status -1 and a message, nothing launched ---------------
P = ctypes.c_void_p(4096)     # never dereferenced: every call below is refused first


def _embed(L, **kw):
    a = dict(ids=P, cu=P, n_text=2, n_tok=8, max_seqlen=4, word=P, vocab=512, pos=P, n_pos=512,
             typ=P, w=P, b=P, d=128, eps=1e-12, y=P, ldy=128, status=P)
    a.update(kw)
    return L.cs_embed_layer_norm(a["ids"], a["cu"], a["n_text"], a["n_tok"], a["max_seqlen"], a["word"],
                                 a["vocab"], a["pos"], a["n_pos"], a["typ"], a["w"], a["b"], a["d"],
                                 a["eps"], a["y"], a["ldy"], a["status"], None)


def _addln(L, **kw):
    a = dict(x=P, ldx=128, r=P, ldr=128, w=P, b=P, rows=4, d=128, eps=1e-12, y=P, ldy=128)
    a.update(kw)
    return L.cs_add_layer_norm(a["x"], a["ldx"], a["r"], a["ldr"], a["w"], a["b"], a["rows"], a["d"],
                               a["eps"], a["y"], a["ldy"], None)


def _gelu(L, **kw):
    a = dict(x=P, ldx=512, rows=4, F=512, y=P, ldy=512)
    a.update(kw)
    return L.cs_gelu(a["x"], a["ldx"], a["rows"], a["F"], a["y"], a["ldy"], None)


def _attn(L, **kw):
    a = dict(qkv=P, ld=384, cu=P, n_text=2, n_tok=8, max_seqlen=4, H=2, D=64, scale=0.125, out=P)
    a.update(kw)
    return L.cs_encoder_attention(a["qkv"], a["ld"], a["cu"], a["n_text"], a["n_tok"], a["max_seqlen"],
                                  a["H"], a["D"], a["scale"], a["out"], None)


def _cosw(L, **kw):
    a = dict(Es=P, lds=128, Ea=P, lda=128, vs=None, va=None, S=3, A=2, d=128, eps=1e-9, cos=P, wel=P)
    a.update(kw)
    return L.cs_cosine_welfare(a["Es"], a["lds"], a["Ea"], a["lda"], a["vs"], a["va"], a["S"], a["A"],
                               a["d"], a["eps"], a["cos"], a["wel"], None)


BAD = [
    (_embed, dict(max_seqlen=513), "position table"),      # a text longer than the table
    (_embed, dict(n_tok=-1), "bad shape"), (_embed, dict(d=132), "multiple of 8"),
    (_embed, dict(d=4096, ldy=4096), "2048"), (_embed, dict(ids=None), "NULL"),
    (_embed, dict(status=None), "NULL"), (_embed, dict(vocab=0), "vocabulary"),
    (_embed, dict(ldy=120), "ldy"), (_embed, dict(word=ctypes.c_void_p(4098)), "aligned"),
    (_embed, dict(n_text=0), "without a text"), (_embed, dict(eps=float("nan")), "eps"),
    (_addln, dict(rows=-1), "bad shape"), (_addln, dict(d=0), "bad shape"),
    (_addln, dict(d=2056, ldx=2056, ldy=2056, ldr=2056), "2048"), (_addln, dict(x=None), "NULL"),
    (_addln, dict(ldr=64), "leading"), (_addln, dict(y=ctypes.c_void_p(4104)), "aligned"),
    (_gelu, dict(F=0), "bad shape"), (_gelu, dict(F=500), "multiples of 8"),
    (_gelu, dict(ldy=256), "multiples of 8"), (_gelu, dict(y=None), "NULL"),
    (_attn, dict(D=128), "head_dim"), (_attn, dict(H=0), "H must"), (_attn, dict(max_seqlen=513), "512"),
    (_attn, dict(ld=383), "ld_qkv"), (_attn, dict(ld=256), "ld_qkv"), (_attn, dict(scale=0.0), "scale"),
    (_attn, dict(cu=None), "NULL"), (_attn, dict(n_tok=-1), "negative"),
    (_attn, dict(out=ctypes.c_void_p(4100)), "aligned"),
    (_cosw, dict(S=-1), "bad shape"), (_cosw, dict(d=0), "bad shape"), (_cosw, dict(Es=None), "NULL"),
    (_cosw, dict(wel=None), "NULL"), (_cosw, dict(lda=64), "leading"), (_cosw, dict(eps=0.0), "eps"),
    (_cosw, dict(cos=ctypes.c_void_p(4100)), "misaligned"),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_abi_rejects_bad_arguments(pkg, i):
    L = import_module(PKG_DIR + "._lib").load()
    call, kw, msg = BAD[i]
    assert call(L, **kw) == -1
    assert msg in L.cs_last_error().decode()


def test_abi_empty_batches_are_ok(pkg):
    L = import_module(PKG_DIR + "._lib").load()
    assert _embed(L, n_tok=0, n_text=0, max_seqlen=0) == 0
    assert _addln(L, rows=0) == 0 and _gelu(L, rows=0) == 0
    assert _attn(L, n_text=0, n_tok=0, max_seqlen=0) == 0 and _cosw(L, S=0) == 0


# --- tokenizer, presets, get_embedding's contract ----------------------------------------
def test_wordpiece_keeps_sep_when_truncating(pkg, golden_dir):
    T = import_module(PKG_DIR + ".tokenizer").WordPieceTokenizer
    tok = T(os.path.join(golden_dir, "wordpiece_fixture"))
    ids = tok.encode("Cleaner AIR matters to everyone.")
    assert ids[0] == tok.cls_id and ids[-1] == tok.sep_id and tok.sep_id not in ids[1:-1]
    assert tok.tokens(ids)[1] == "cleaner"          # the normaliser lower-cases
    long = tok.encode("safer streets and cleaner air " * 300)
    assert len(long) == 512 and long[0] == tok.cls_id and long[-1] == tok.sep_id
    assert tok.sep_id not in long[1:-1]
    body = tok.tk.encode("safer streets and cleaner air " * 300, add_special_tokens=False).ids
    assert len(body) > 510 and long[1:-1] == body[:510]
    assert tok.encode_many(["a b", "safer streets and cleaner air " * 300]) == [tok.encode("a b"), long]
    assert tok.encode("") == [tok.cls_id, tok.sep_id]


def test_presets(pkg):
    enc = import_module(PKG_DIR + ".encoder")
    lg, bs = enc.preset("BAAI/bge-large-en-v1.5"), enc.preset("bge-base-en-v1.5")
    assert (lg.n_layers, lg.d_model, lg.n_heads, lg.d_ff, lg.vocab, lg.n_pos) == (24, 1024, 16, 4096, 30522, 512)
    assert (bs.n_layers, bs.d_model, bs.n_heads, bs.d_ff) == (12, 768, 12, 3072)
    assert lg.ln_eps == 1e-12 and lg.head_dim == bs.head_dim == 64
    with pytest.raises(ValueError):
        enc.preset("bge-small")


def test_get_embedding_never_raises(pkg):
    utils = import_module(PKG_DIR + ".utils")
    assert utils.get_embedding("some text", model="no/such-embedding-model") is None
    assert utils.get_embedding(None, model="no/such-embedding-model") is None
    assert utils.get_embeddings(["a", "b"], model="no/such-embedding-model") == [None, None]
