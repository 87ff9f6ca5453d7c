"""The text encoder behind ``utils.get_embedding``: a BERT-style bidirectional encoder
(BAAI/bge-large-en-v1.5 and bge-base-en-v1.5: learned positions, post-LayerNorm, erf-GELU,
CLS pooling, L2-normalised output) run on the device over a RAGGED batch -- the texts'
tokens back to back, no padding, text boundaries in ``cu_seqlens``.

The reference gets its embeddings from a hosted API (src/utils.py:376-407).  Here a layer is

    qkv = x Wqkv^T + b            F.linear (hipBLASLt), rounded to bf16 once
    ctx = cs_encoder_attention    bidirectional, per text, bf16 MFMA, fp32 online softmax
    x   = cs_add_layer_norm(ctx Wo^T + b, x)
    h   = cs_gelu(x Wi^T + b)
    x   = cs_add_layer_norm(h Wo2^T + b, x)

after cs_embed_layer_norm.  bf16 weights and activations only: another dtype raises CSError.
Texts are sorted by length and run in passes of at most ``max_tokens`` tokens; a text's
embedding does not depend on what shares its pass (every kernel works row by row or text by
text, and the GEMMs' rows are independent).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import ops
from ._lib import CSError


@dataclass(frozen=True)
class EncoderConfig:
    name: str
    vocab: int = 30522
    d_model: int = 1024
    n_layers: int = 24
    n_heads: int = 16
    d_ff: int = 4096
    n_pos: int = 512
    n_types: int = 2
    ln_eps: float = 1e-12
    head_dim: int = 64


PRESETS: Dict[str, EncoderConfig] = {
    "bge-large-en-v1.5": EncoderConfig("bge-large-en-v1.5"),
    "bge-base-en-v1.5": EncoderConfig("bge-base-en-v1.5", d_model=768, n_layers=12, n_heads=12,
                                      d_ff=3072),
}


def preset(name: str, **overrides) -> EncoderConfig:
    key = name.split("/")[-1].lower()
    if key not in PRESETS:
        raise ValueError(f"no encoder preset {name!r} (one of {sorted(PRESETS)})")
    c = PRESETS[key]
    return EncoderConfig(**{**c.__dict__, **overrides}) if overrides else c


def weight_names(cfg: EncoderConfig) -> List[str]:
    """The encoder's weight names (q | k | v fused): what ``TextEncoder`` takes."""
    out = ["word", "pos", "type", "emb_ln_w", "emb_ln_b"]
    for i in range(cfg.n_layers):
        out += [f"l{i}.{n}" for n in ("wqkv", "bqkv", "wo", "bo", "ln1_w", "ln1_b", "wi", "bi",
                                      "wo2", "bo2", "ln2_w", "ln2_b")]
    return out


def random_weights(cfg: EncoderConfig, device, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random bf16 weights of the architecture (benchmarks: the embeddings mean nothing)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    d, f = cfg.d_model, cfg.d_ff

    def rnd(*shape, std=1.0, mean=0.0):
        return (torch.randn(*shape, generator=g) * std + mean).to(torch.bfloat16).to(device)

    w = {"word": rnd(cfg.vocab, d), "pos": rnd(cfg.n_pos, d), "type": rnd(cfg.n_types, d),
         "emb_ln_w": rnd(d, std=0.1, mean=1.0), "emb_ln_b": rnd(d, std=0.1)}
    for i in range(cfg.n_layers):
        p = f"l{i}."
        w.update({p + "wqkv": rnd(3 * d, d, std=d ** -0.5), p + "bqkv": rnd(3 * d, std=0.1),
                  p + "wo": rnd(d, d, std=d ** -0.5), p + "bo": rnd(d, std=0.1),
                  p + "ln1_w": rnd(d, std=0.1, mean=1.0), p + "ln1_b": rnd(d, std=0.1),
                  p + "wi": rnd(f, d, std=d ** -0.5), p + "bi": rnd(f, std=0.1),
                  p + "wo2": rnd(d, f, std=f ** -0.5), p + "bo2": rnd(d, std=0.1),
                  p + "ln2_w": rnd(d, std=0.1, mean=1.0), p + "ln2_b": rnd(d, std=0.1)})
    return w


class TextEncoder:
    """``embed_ids(list of id lists) -> float32 [n, d_model]`` on the device."""

    def __init__(self, cfg: EncoderConfig, device, weights: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 0, max_tokens: int = 16384):
        self.cfg = cfg
        self.device = torch.device(device)
        if cfg.head_dim != 64 or cfg.n_heads * cfg.head_dim != cfg.d_model:
            raise CSError(f"encoder {cfg.name}: the attention kernel serves heads of 64 "
                          f"(d_model = 64 n_heads), got {cfg.n_heads} x {cfg.head_dim} for {cfg.d_model}")
        if cfg.d_model % 8 or cfg.d_model > 2048 or cfg.d_ff % 8:
            raise CSError(f"encoder {cfg.name}: d_model must be a multiple of 8, <= 2048")
        if weights is None:
            weights = random_weights(cfg, self.device, seed)
        self.w: Dict[str, torch.Tensor] = {}
        for n in weight_names(cfg):
            if n not in weights:
                raise CSError(f"encoder {cfg.name}: missing weight {n!r}")
            t = weights[n]
            if t.dtype != torch.bfloat16:
                raise CSError(f"encoder {cfg.name}: weight {n!r} is {t.dtype}; the encoder is "
                              "bf16 only (cast the checkpoint, the numerics are bf16's)")
            self.w[n] = t.to(self.device).contiguous()
        self.max_tokens = max(int(max_tokens), cfg.n_pos)

    @property
    def dtype(self):
        return torch.bfloat16

    def _check_ids(self, ids_list: Sequence[Sequence[int]]) -> List[List[int]]:
        out = []
        for i, ids in enumerate(ids_list):
            ids = [int(t) for t in ids]
            if not 1 <= len(ids) <= self.cfg.n_pos:
                raise CSError(f"text {i} has {len(ids)} tokens; the encoder takes 1 .. {self.cfg.n_pos}")
            if min(ids) < 0 or max(ids) >= self.cfg.vocab:
                raise CSError(f"text {i} has a token id outside [0, {self.cfg.vocab})")
            out.append(ids)
        return out

    @torch.no_grad()
    def hidden(self, ids: torch.Tensor, cu: torch.Tensor, max_len: int) -> torch.Tensor:
        """Last hidden states bf16 [n_tok, d_model] of one ragged pass."""
        c, w = self.cfg, self.w
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        x = ops.embed_layer_norm(ids, cu, max_len, w["word"], w["pos"], w["type"], w["emb_ln_w"],
                                 w["emb_ln_b"], c.ln_eps, status=status)
        for i in range(c.n_layers):
            p = f"l{i}."
            qkv = F.linear(x, w[p + "wqkv"], w[p + "bqkv"])
            ctx = ops.encoder_attention(qkv, cu, max_len, c.n_heads, c.head_dim)
            x = ops.add_layer_norm(F.linear(ctx, w[p + "wo"], w[p + "bo"]), x, w[p + "ln1_w"],
                                   w[p + "ln1_b"], c.ln_eps)
            h = ops.gelu(F.linear(x, w[p + "wi"], w[p + "bi"]))
            x = ops.add_layer_norm(F.linear(h, w[p + "wo2"], w[p + "bo2"]), x, w[p + "ln2_w"],
                                   w[p + "ln2_b"], c.ln_eps)
        return x

    @torch.no_grad()
    def embed_ids(self, ids_list: Sequence[Sequence[int]]) -> torch.Tensor:
        """CLS-pooled, L2-normalised float32 [n, d_model] embeddings, in the order given."""
        texts = self._check_ids(ids_list)
        n = len(texts)
        out = torch.empty(n, self.cfg.d_model, dtype=torch.float32, device=self.device)
        order = sorted(range(n), key=lambda i: len(texts[i]))
        a = 0
        while a < n:
            b, tot = a, 0
            while b < n and (b == a or tot + len(texts[order[b]]) <= self.max_tokens):
                tot += len(texts[order[b]])
                b += 1
            idx = order[a:b]
            lens = [len(texts[i]) for i in idx]
            cu_h = [0]
            for ln in lens:
                cu_h.append(cu_h[-1] + ln)
            flat = [t for i in idx for t in texts[i]]
            ids = torch.tensor(flat, dtype=torch.int32, device=self.device)
            cu = torch.tensor(cu_h, dtype=torch.int32, device=self.device)
            x = self.hidden(ids, cu, max(lens))
            cls = x[cu[:-1].long()].float()
            emb = cls / cls.norm(dim=1, keepdim=True)
            out[torch.tensor(idx, dtype=torch.long, device=self.device)] = emb
            a = b
        return out


def fuse_hf_weights(sd: Dict[str, torch.Tensor], cfg: EncoderConfig) -> Dict[str, torch.Tensor]:
    """Hugging Face ``BertModel`` parameters (optionally prefixed ``bert.``) -> the encoder's
    names, q | k | v fused.  Tensors keep their dtype and device."""
    def g(name):
        for pre in ("", "bert."):
            if pre + name in sd:
                return sd[pre + name]
        raise ValueError(f"checkpoint lacks {name!r}")

    w = {"word": g("embeddings.word_embeddings.weight"), "pos": g("embeddings.position_embeddings.weight"),
         "type": g("embeddings.token_type_embeddings.weight"),
         "emb_ln_w": g("embeddings.LayerNorm.weight"), "emb_ln_b": g("embeddings.LayerNorm.bias")}
    for i in range(cfg.n_layers):
        q, p = f"encoder.layer.{i}.", f"l{i}."
        w[p + "wqkv"] = torch.cat([g(q + f"attention.self.{n}.weight") for n in ("query", "key", "value")], 0)
        w[p + "bqkv"] = torch.cat([g(q + f"attention.self.{n}.bias") for n in ("query", "key", "value")], 0)
        w[p + "wo"], w[p + "bo"] = g(q + "attention.output.dense.weight"), g(q + "attention.output.dense.bias")
        w[p + "ln1_w"], w[p + "ln1_b"] = g(q + "attention.output.LayerNorm.weight"), g(q + "attention.output.LayerNorm.bias")
        w[p + "wi"], w[p + "bi"] = g(q + "intermediate.dense.weight"), g(q + "intermediate.dense.bias")
        w[p + "wo2"], w[p + "bo2"] = g(q + "output.dense.weight"), g(q + "output.dense.bias")
        w[p + "ln2_w"], w[p + "ln2_b"] = g(q + "output.LayerNorm.weight"), g(q + "output.LayerNorm.bias")
    return w
