#!/usr/bin/env python3
"""The evaluator's embedding pass at the published sweep's size: 750 statements plus 5 opinions
on the bge-large-en-v1.5 shape with random weights.

  ragged    encoder.TextEncoder.embed_ids: texts back to back with no padding (sorted by
            length, at most --max-tokens tokens per pass), the HIP kernels + hipBLASLt GEMMs
  eager     the same weights in torch eager bf16 on the same box: texts sorted the same way,
            each pass PADDED to its longest text (at most --max-tokens padded tokens per pass),
            F.layer_norm / F.gelu / F.scaled_dot_product_attention with a key-padding mask
  per_op    one layer's launches of the ragged path on its largest pass, each timed alone

The texts are random ids with the published statements' lengths: tests/golden/
eval_statement_words.json holds their word counts, taken as 1.3 WordPiece tokens per word plus
[CLS] and [SEP] (the real tokenizer's vocabulary is not needed for a throughput figure).
Times are HIP events around a whole call, median of --reps after --warmup.  Writes one JSON line:

  python tools/encoder_bench.py [--out profiles/encoder_bench.jsonl]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "generating-fair-consensus-statements-with-social-choice-on-token-level-mdps_amd"
ops = importlib.import_module(PKG + ".ops")
encoder = importlib.import_module(PKG + ".encoder")


def gpu_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def texts(cfg):
    with open(os.path.join(REPO, "tests", "golden", "eval_statement_words.json")) as f:
        d = json.load(f)
    rng = np.random.default_rng(0)
    lens = [min(cfg.n_pos, int(round(1.3 * w)) + 2) for w in d["statement_words"] + d["opinion_words"]]
    return [rng.integers(1000, cfg.vocab, size=n).tolist() for n in lens]


def passes(ids, cap, padded):
    """Texts sorted by length, cut into passes of at most ``cap`` (padded) tokens."""
    order = sorted(range(len(ids)), key=lambda i: len(ids[i]))
    out, cur = [], []
    for i in order:
        n = len(ids[i])
        size = (len(cur) + 1) * n if padded else sum(len(ids[j]) for j in cur) + n
        if cur and size > cap:
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


@torch.no_grad()
def eager_embed(enc, ids, cap):
    c, w, dev = enc.cfg, enc.w, enc.device
    res = torch.empty(len(ids), c.d_model, dtype=torch.float32, device=dev)
    for idx in passes(ids, cap, padded=True):
        L = max(len(ids[i]) for i in idx)
        tok = torch.zeros(len(idx), L, dtype=torch.long)
        keep = torch.zeros(len(idx), L, dtype=torch.bool)
        for r, i in enumerate(idx):
            tok[r, :len(ids[i])] = torch.tensor(ids[i])
            keep[r, :len(ids[i])] = True
        tok, keep = tok.to(dev), keep.to(dev)
        x = w["word"][tok] + w["type"][0] + w["pos"][:L]
        x = F.layer_norm(x, (c.d_model,), w["emb_ln_w"], w["emb_ln_b"], c.ln_eps)
        mask = keep[:, None, None, :]
        B = len(idx)
        for li in range(c.n_layers):
            p = f"l{li}."
            qkv = F.linear(x, w[p + "wqkv"], w[p + "bqkv"]).view(B, L, 3, c.n_heads, c.head_dim)
            q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
            ctx = ctx.transpose(1, 2).reshape(B, L, c.d_model)
            x = F.layer_norm(F.linear(ctx, w[p + "wo"], w[p + "bo"]) + x, (c.d_model,),
                             w[p + "ln1_w"], w[p + "ln1_b"], c.ln_eps)
            h = F.gelu(F.linear(x, w[p + "wi"], w[p + "bi"]))
            x = F.layer_norm(F.linear(h, w[p + "wo2"], w[p + "bo2"]) + x, (c.d_model,),
                             w[p + "ln2_w"], w[p + "ln2_b"], c.ln_eps)
        cls = x[:, 0].float()
        res[torch.tensor(idx, device=dev)] = cls / cls.norm(dim=1, keepdim=True)
    return res


def per_op(enc, ids, cap, warmup, reps):
    """One layer's launches on the largest ragged pass, each alone (median ms)."""
    c, w, dev = enc.cfg, enc.w, enc.device
    idx = max(passes(ids, cap, padded=False), key=lambda p: sum(len(ids[i]) for i in p))
    lens = [len(ids[i]) for i in idx]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    flat = torch.tensor([t for i in idx for t in ids[i]], dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mx = max(lens)
    x = ops.embed_layer_norm(flat, cu, mx, w["word"], w["pos"], w["type"], w["emb_ln_w"], w["emb_ln_b"],
                             c.ln_eps, status=status)
    qkv = F.linear(x, w["l0.wqkv"], w["l0.bqkv"])
    ctx = ops.encoder_attention(qkv, cu, mx, c.n_heads)
    h = F.linear(x, w["l0.wi"], w["l0.bi"])
    t = lambda fn: gpu_ms(fn, warmup, reps)[0]   # noqa: E731
    return {
        "tokens": int(flat.numel()), "texts": len(idx), "longest": mx,
        "embed_layer_norm": t(lambda: ops.embed_layer_norm(flat, cu, mx, w["word"], w["pos"], w["type"],
                                                           w["emb_ln_w"], w["emb_ln_b"], c.ln_eps,
                                                           status=status)),
        "gemm_qkv": t(lambda: F.linear(x, w["l0.wqkv"], w["l0.bqkv"])),
        "encoder_attention": t(lambda: ops.encoder_attention(qkv, cu, mx, c.n_heads)),
        "gemm_attn_out": t(lambda: F.linear(ctx, w["l0.wo"], w["l0.bo"])),
        "add_layer_norm": t(lambda: ops.add_layer_norm(ctx, x, w["l0.ln1_w"], w["l0.ln1_b"], c.ln_eps)),
        "gemm_ffn_in": t(lambda: F.linear(x, w["l0.wi"], w["l0.bi"])),
        "gelu": t(lambda: ops.gelu(h)),
        "gemm_ffn_out": t(lambda: F.linear(h, w["l0.wo2"], w["l0.bo2"])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "encoder_bench.jsonl"))
    ap.add_argument("--preset", default="bge-large-en-v1.5")
    ap.add_argument("--max-tokens", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_bench needs the GPU (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = encoder.preset(args.preset)
    enc = encoder.TextEncoder(cfg, dev, seed=0, max_tokens=args.max_tokens)
    ids = texts(cfg)
    n_tok = sum(len(t) for t in ids)
    pad_tok = sum(len(p) * max(len(ids[i]) for i in p) for p in passes(ids, args.max_tokens, True))
    out = {}

    def ragged():
        out["r"] = enc.embed_ids(ids)

    def eager():
        out["e"] = eager_embed(enc, ids, args.max_tokens)

    r_ms = gpu_ms(ragged, args.warmup, args.reps)
    e_ms = gpu_ms(eager, args.warmup, args.reps)
    diff = float((out["r"] - out["e"]).abs().max())
    line = {"bench": "encoder", "device": torch.cuda.get_device_name(dev), "preset": cfg.name,
            "texts": len(ids), "tokens": n_tok, "padded_tokens_eager": pad_tok,
            "longest": max(len(t) for t in ids), "max_tokens": args.max_tokens,
            "warmup": args.warmup, "reps": args.reps,
            "ragged_ms": r_ms[0], "ragged_ms_min": r_ms[1], "ragged_ms_max": r_ms[2],
            "eager_ms": e_ms[0], "eager_ms_min": e_ms[1], "eager_ms_max": e_ms[2],
            "ragged_over_eager": round(r_ms[0] / e_ms[0], 3),
            "max_abs_diff_ragged_eager": diff,
            "per_op_one_layer_ms": per_op(enc, ids, args.max_tokens, args.warmup, max(args.reps, 11))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
