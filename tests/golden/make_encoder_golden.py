"""Generate the text encoder's stored vectors (CPU only; needs ``transformers``, ``tokenizers``).

  encoder_golden.npz         Hugging Face ``BertModel(add_pooling_layer=False)`` on the seeded
                             weights of tests/encoder_ref.py, one text per forward (no padding),
                             CLS-pooled and L2-normalised, in fp64, fp32 and eager bf16.  Per
                             model m in (tiny, bge-large):
                               m_ids, m_cu           the texts' token ids, concatenated
                               m_emb_f64, m_emb_f32  embeddings [n, hidden]
                               m_cos_f32             1 - cosine distance of every pair of the
                                                     fp32 embeddings [n, n] (fp64 arithmetic)
                               m_bf16_eager_err      [max |eager bf16 - fp32| over embedding
                                                     entries, the same over the cosines]: the
                                                     unit of the GPU tests' bound
  wordpiece_fixture/tokenizer.json   a small BERT WordPiece tokenizer trained here on a few lines
  eval_cosine_published.csv  (with --reference DIR) per-agent cosine similarities and the three
                             cosine welfare columns of every row of the reference's published
                             results/appendix/*/evaluation/*/seed_*/evaluation_results.csv

Usage:  python tests/golden/make_encoder_golden.py [--reference DIR] [--only tiny]
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import encoder_ref as er  # noqa: E402

LENGTHS = {"tiny": [1, 2, 5, 31, 33, 64, 65, 130], "bge-large": [2, 33, 128, 512]}


def _pair_cos(E):
    E = np.asarray(E, np.float64)
    n = len(E)
    return np.array([[er.cosine_similarity(E[i], E[j]) for j in range(n)] for i in range(n)])


def run_model(shape: str) -> dict:
    import torch
    from transformers import BertConfig, BertModel

    c = er.SHAPES[shape]
    cfg = BertConfig(vocab_size=c["vocab"], hidden_size=c["hidden"], num_hidden_layers=c["layers"],
                     num_attention_heads=c["heads"], intermediate_size=c["ffn"],
                     max_position_embeddings=c["n_pos"], type_vocab_size=2, hidden_act="gelu",
                     layer_norm_eps=er.LN_EPS, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    w = er.make_weights(shape)
    ids = er.make_ids(shape, LENGTHS[shape])
    embs = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32), ("bf16", torch.bfloat16)):
        model = BertModel(cfg, add_pooling_layer=False).eval()
        missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        assert not missing.unexpected_keys and all("position_ids" in k or "token_type_ids" in k
                                                   for k in missing.missing_keys), missing
        model = model.to(dt)
        rows = []
        with torch.no_grad():
            for t in ids:
                h = model(input_ids=torch.from_numpy(t)[None]).last_hidden_state[0, 0]
                h = h.to(torch.float64 if dt == torch.float64 else torch.float32)
                rows.append((h / h.norm()).numpy())
        embs[name] = np.stack(rows)
        del model
        print(f"{shape}: {name} done", flush=True)
    cos32, cosb = _pair_cos(embs["f32"]), _pair_cos(embs["bf16"])
    err = np.array([np.abs(embs["bf16"].astype(np.float64) - embs["f32"]).max(),
                    np.abs(cosb - cos32).max()])
    print(f"{shape}: bf16_eager_err = {err}")
    return {f"{shape}_ids": np.concatenate(ids).astype(np.int32),
            f"{shape}_cu": np.concatenate([[0], np.cumsum(LENGTHS[shape])]).astype(np.int32),
            f"{shape}_emb_f64": embs["f64"], f"{shape}_emb_f32": embs["f32"].astype(np.float32),
            f"{shape}_cos_f32": cos32, f"{shape}_bf16_eager_err": err}


def make_wordpiece() -> None:
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers

    tok = Tokenizer(models.WordPiece(unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    corpus = ["We should invest in public transport and cycling lanes.",
              "Taxes on fuel are unfair to people who live in the countryside.",
              "A consensus statement balances every opinion fairly.",
              "The council agrees that cleaner air matters to everyone.",
              "Opinions differ, yet most people want safer streets."] * 4
    trainer = trainers.WordPieceTrainer(vocab_size=300, min_frequency=1,
                                        special_tokens=["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    tok.train_from_iterator(corpus, trainer)
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", tok.token_to_id("[CLS]")), ("[SEP]", tok.token_to_id("[SEP]"))])
    tok.decoder = decoders.WordPiece()
    d = os.path.join(HERE, "wordpiece_fixture")
    os.makedirs(d, exist_ok=True)
    tok.save(os.path.join(d, "tokenizer.json"))
    print("wrote wordpiece_fixture/tokenizer.json", tok.get_vocab_size(), "tokens")


def make_published(ref: str) -> None:
    import pandas as pd

    files = sorted(glob.glob(os.path.join(ref, "results", "appendix", "*", "evaluation", "*",
                                          "seed_*", "evaluation_results.csv")))
    rows = []
    for f in files:
        df = pd.read_csv(f)
        agents = [c[len("cosine_similarity_"):] for c in df.columns if c.startswith("cosine_similarity_")]
        for i, r in df.iterrows():
            rec = {"source": os.path.relpath(f, ref), "row": i, "n_agents": len(agents)}
            for j, a in enumerate(agents):
                rec[f"cosine_similarity_{j}"] = r[f"cosine_similarity_{a}"]
            for c in ("egalitarian_welfare_cosine", "utilitarian_welfare_cosine", "log_nash_welfare_cosine"):
                rec[c] = r[c]
            rows.append(rec)
    out = pd.DataFrame(rows)
    out.to_csv(os.path.join(HERE, "eval_cosine_published.csv"), index=False, float_format="%.17g")
    print(f"wrote eval_cosine_published.csv ({len(out)} rows from {len(files)} files)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--only", default=None, choices=list(LENGTHS))
    a = ap.parse_args()
    if a.reference:
        make_published(a.reference)
    make_wordpiece()
    path = os.path.join(HERE, "encoder_golden.npz")
    out = dict(np.load(path)) if a.only and os.path.exists(path) else {}
    for shape in ([a.only] if a.only else list(LENGTHS)):
        out.update(run_model(shape))
    np.savez_compressed(path, **out)
    print("wrote encoder_golden.npz", os.path.getsize(path), "bytes")
