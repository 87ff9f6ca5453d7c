"""fp64 NumPy restatement of the text encoder (BERT-style, post-LayerNorm, erf-GELU, CLS pooling,
L2 normalisation: BAAI/bge-*-en-v1.5) and of the evaluator's cosine / welfare rules
(src/evaluation.py:239-307 of the reference), plus the seeded weight recipe the tests and
tests/golden/make_encoder_golden.py share.

Nothing here rounds: the kernels are compared against these values on identical bf16 inputs,
and the restatement itself is pinned to Hugging Face's ``BertModel`` in fp64
(tests/golden/encoder_golden.npz, 1e-10: only summation order differs).
"""
from __future__ import annotations

import math

import numpy as np

EPS_WELFARE = 1e-9

# (layers, hidden, heads, ffn, vocab, positions); head_dim is 64 everywhere
SHAPES = {
    "tiny": dict(layers=2, hidden=128, heads=2, ffn=512, vocab=512, n_pos=512),
    "bge-large": dict(layers=24, hidden=1024, heads=16, ffn=4096, vocab=30522, n_pos=512),
}
LN_EPS = 1e-12
SEEDS = {"tiny": 20240611, "bge-large": 20240612}


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bf16-representable float32 (ties to even)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """The int16 bit patterns of bf16-representable float32 values (torch: .view(bfloat16))."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def param_names(layers: int):
    """Hugging Face BertModel parameter names with their roles, in the recipe's fixed order."""
    out = [("embeddings.word_embeddings.weight", "word"),
           ("embeddings.position_embeddings.weight", "pos"),
           ("embeddings.token_type_embeddings.weight", "type"),
           ("embeddings.LayerNorm.weight", "ln_w"), ("embeddings.LayerNorm.bias", "ln_b")]
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for nm in ("attention.self.query", "attention.self.key", "attention.self.value",
                   "attention.output.dense"):
            out += [(p + nm + ".weight", "hh"), (p + nm + ".bias", "bias_h")]
        out += [(p + "attention.output.LayerNorm.weight", "ln_w"),
                (p + "attention.output.LayerNorm.bias", "ln_b"),
                (p + "intermediate.dense.weight", "fh"), (p + "intermediate.dense.bias", "bias_f"),
                (p + "output.dense.weight", "hf"), (p + "output.dense.bias", "bias_h"),
                (p + "output.LayerNorm.weight", "ln_w"), (p + "output.LayerNorm.bias", "ln_b")]
    return out


def make_weights(shape: str) -> dict:
    """The seeded weights of ``shape``: float32 arrays holding bf16-representable values, keyed
    by Hugging Face's parameter names.  Projections N(0, 1/fan_in) (attention scores and FFN
    activations of order one), embeddings N(0, 1), LayerNorm weights 1 + N(0, 0.1^2), biases
    N(0, 0.1^2)."""
    c = SHAPES[shape]
    h, f = c["hidden"], c["ffn"]
    rng = np.random.default_rng(SEEDS[shape])
    dims = {"word": ((c["vocab"], h), 1.0, 0.0), "pos": ((c["n_pos"], h), 1.0, 0.0),
            "type": ((2, h), 1.0, 0.0), "ln_w": ((h,), 0.1, 1.0), "ln_b": ((h,), 0.1, 0.0),
            "hh": ((h, h), h ** -0.5, 0.0), "fh": ((f, h), h ** -0.5, 0.0),
            "hf": ((h, f), f ** -0.5, 0.0), "bias_h": ((h,), 0.1, 0.0), "bias_f": ((f,), 0.1, 0.0)}
    w = {}
    for name, role in param_names(c["layers"]):
        shp, std, mean = dims[role]
        x = rng.standard_normal(shp, dtype=np.float32) * np.float32(std) + np.float32(mean)
        w[name] = bf16_round(x)
    return w


def make_ids(shape: str, lengths, seed: int = 0):
    """Seeded token ids for texts of the given lengths (id 1 first, as a [CLS] would be)."""
    rng = np.random.default_rng(SEEDS[shape] + 1000 + seed)
    out = []
    for n in lengths:
        ids = rng.integers(2, SHAPES[shape]["vocab"], size=n).astype(np.int64)
        ids[0] = 1
        out.append(ids)
    return out


# --- the encoder, fp64 ----------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps=LN_EPS):
    """LayerNorm rows of x (biased variance); also returns w * xhat for the tests' bound."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    wx = (x - mu) / np.sqrt(var + eps) * np.asarray(w, dtype=np.float64)
    return wx + np.asarray(b, dtype=np.float64), wx


def attention(q, k, v, scale):
    """softmax(scale q k^T) v of one text and head (fp64); also A = sum_i p_i |v_i|, the scale
    of tests/attention_ref.py's bound."""
    s = (np.asarray(q, np.float64) @ np.asarray(k, np.float64).T) * scale
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    v = np.asarray(v, np.float64)
    return p @ v, p @ np.abs(v)


def ragged_attention(qkv, cu, H, D=64, scale=None):
    """out [n_tok, H D] and the bound's A for a fused projection [n_tok, 3 H D]."""
    qkv = np.asarray(qkv, np.float64)
    scale = D ** -0.5 if scale is None else scale
    out = np.zeros((qkv.shape[0], H * D))
    A = np.zeros_like(out)
    for t in range(len(cu) - 1):
        a, b = int(cu[t]), int(cu[t + 1])
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            o, aa = attention(qkv[a:b, sl], qkv[a:b, H * D + h * D:H * D + (h + 1) * D],
                              qkv[a:b, 2 * H * D + h * D:2 * H * D + (h + 1) * D], scale)
            out[a:b, sl] = o
            A[a:b, sl] = aa
    return out, A


def embed(w, ids_list):
    W = {k: np.asarray(v, np.float64) for k, v in w.items() if k.startswith("embeddings.")}
    rows = []
    for ids in ids_list:
        ids = np.asarray(ids)
        rows.append(W["embeddings.word_embeddings.weight"][ids]
                    + W["embeddings.position_embeddings.weight"][:len(ids)]
                    + W["embeddings.token_type_embeddings.weight"][0])
    x = np.concatenate(rows, axis=0)
    return layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"])[0]


def forward(w, shape: str, ids_list):
    """CLS-pooled, L2-normalised embeddings [n, hidden] (fp64) of the texts."""
    c = SHAPES[shape]
    H = c["heads"]
    cu = np.concatenate([[0], np.cumsum([len(i) for i in ids_list])])
    x = embed(w, ids_list)
    g = lambda n: np.asarray(w[n], np.float64)   # noqa: E731
    for i in range(c["layers"]):
        p = f"encoder.layer.{i}."
        qkv = np.concatenate([x @ g(p + f"attention.self.{n}.weight").T + g(p + f"attention.self.{n}.bias")
                              for n in ("query", "key", "value")], axis=1)
        ctx, _ = ragged_attention(qkv, cu, H)
        ao = ctx @ g(p + "attention.output.dense.weight").T + g(p + "attention.output.dense.bias")
        x = layer_norm(ao + x, g(p + "attention.output.LayerNorm.weight"),
                       g(p + "attention.output.LayerNorm.bias"))[0]
        hdn = gelu(x @ g(p + "intermediate.dense.weight").T + g(p + "intermediate.dense.bias"))
        fo = hdn @ g(p + "output.dense.weight").T + g(p + "output.dense.bias")
        x = layer_norm(fo + x, g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"))[0]
    cls = x[cu[:-1]]
    return cls / np.linalg.norm(cls, axis=1, keepdims=True)


# --- the evaluator's rules ------------------------------------------------------------
def cosine_similarity(u, v):
    """One pair by the reference's rules (src/evaluation.py:239-261): None if either embedding
    is missing or the value is NaN, 0.0 for a zero vector, else 1 - scipy's cosine distance
    (1 - clip(1 - u.v / sqrt(u.u v.v), 0, 2), scipy.spatial.distance.cosine)."""
    if u is None or v is None:
        return None
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    if np.linalg.norm(u) == 0 or np.linalg.norm(v) == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = 1.0 - np.dot(u, v) / math.sqrt(np.dot(u, u) * np.dot(v, v)) \
            if np.isfinite(np.dot(u, u) * np.dot(v, v)) else float("nan")
    sim = 1.0 - float(np.clip(dist, 0.0, 2.0))
    return None if math.isnan(sim) else sim


def welfare_folds(sims, eps=EPS_WELFARE):
    """(egalitarian, utilitarian, log_nash) over the finite similarities, in order
    (src/evaluation.py:278-307); NaN each when there is none."""
    ok = [s for s in sims if s is not None and np.isfinite(s)]
    if not ok:
        return float("nan"), float("nan"), float("nan")
    return min(ok), sum(ok), sum(np.log([max(s, eps) for s in ok]))


def cosine_welfare(E_s, E_a, valid_s=None, valid_a=None):
    """cos [A, S] (NaN where the reference has None) and welfare [3, S], as cs_cosine_welfare."""
    S, A = len(E_s), len(E_a)
    cos = np.full((A, S), np.nan)
    wel = np.full((3, S), np.nan)
    for s in range(S):
        u = None if valid_s is not None and not valid_s[s] else E_s[s]
        sims = []
        for a in range(A):
            v = None if valid_a is not None and not valid_a[a] else E_a[a]
            c = cosine_similarity(u, v)
            sims.append(c)
            if c is not None:
                cos[a, s] = c
        wel[:, s] = welfare_folds(sims)
    return cos, wel


# --- the encoder under test on the seeded weights ---------------------------------------
def build_encoder(shape: str, dev, dtype=None):
    """The package's TextEncoder of ``shape`` on make_weights(shape) (bf16 unless ``dtype``)."""
    from importlib import import_module

    import torch

    from conftest import PKG_DIR

    enc = import_module(PKG_DIR + ".encoder")
    c = SHAPES[shape]
    cfg = enc.EncoderConfig(shape, vocab=c["vocab"], d_model=c["hidden"], n_layers=c["layers"],
                            n_heads=c["heads"], d_ff=c["ffn"], n_pos=c["n_pos"], ln_eps=LN_EPS)
    dtype = torch.bfloat16 if dtype is None else dtype
    sd = {k: torch.from_numpy(v).to(device=dev, dtype=dtype) for k, v in make_weights(shape).items()}
    return enc.TextEncoder(cfg, dev, weights=enc.fuse_hf_weights(sd, cfg))
