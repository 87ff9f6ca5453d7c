"""GPU tests of the whole text encoder against Hugging Face's ``BertModel`` on the same seeded
weights (tests/golden/encoder_golden.npz, made on the CPU by make_encoder_golden.py).

Bound: 3 x the stored ``bf16_eager_err`` -- the max |eager bf16 - fp32| HF itself shows on the
CPU, over the embedding entries and over the pairwise cosines.  The encoder rounds where
eager does (each projection once, each LayerNorm output once) or less often, and only
summation orders differ, so the max over a few thousand entries of two such runs differs by
well under 3x.  Each test prints its figures; with CS_ENCODER_PARITY_OUT=<file> they are
appended there as JSON lines (profiles/encoder_parity.jsonl holds the MI355X run).
"""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import encoder_ref as er
from encoder_ref import build_encoder
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "encoder_golden.npz"))


@pytest.fixture(scope="module")
def tiny(dev):
    return build_encoder("tiny", dev)


def texts_of(golden, m):
    cu = golden[f"{m}_cu"]
    return [golden[f"{m}_ids"][cu[i]:cu[i + 1]].tolist() for i in range(len(cu) - 1)]


def parity(enc, golden, m, ops):
    ids = texts_of(golden, m)
    E = enc.embed_ids(ids)
    assert E.dtype == torch.float32 and tuple(E.shape) == golden[f"{m}_emb_f32"].shape
    assert torch.equal(E, enc.embed_ids(ids)), "a second pass differs"
    cos, _ = ops.cosine_welfare(E, E)
    e_err = float(np.abs(E.cpu().numpy().astype(np.float64) - golden[f"{m}_emb_f32"]).max())
    c_err = float(np.abs(cos.cpu().numpy() - golden[f"{m}_cos_f32"]).max())
    unit = golden[f"{m}_bf16_eager_err"]
    rec = {"model": m, "texts": [len(t) for t in ids], "emb_err": e_err, "cos_err": c_err,
           "bf16_eager_emb_err": float(unit[0]), "bf16_eager_cos_err": float(unit[1]),
           "emb_ratio": e_err / float(unit[0]), "cos_ratio": c_err / float(unit[1])}
    print(json.dumps(rec))
    out = os.environ.get("CS_ENCODER_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert e_err <= 3 * unit[0], rec
    assert c_err <= 3 * unit[1], rec


def test_tiny_forward_matches_hf(tiny, golden, ops):
    parity(tiny, golden, "tiny", ops)


def test_bge_large_shape_forward_matches_hf(dev, golden, ops):
    parity(build_encoder("bge-large", dev), golden, "bge-large", ops)


def test_batching_invariance(tiny, golden):
    """A text's embedding is bitwise the same alone, in a mixed batch, in another order and
    when the pass is cut into several by the token cap."""
    ids = texts_of(golden, "tiny")
    E = tiny.embed_ids(ids)
    for i, t in enumerate(ids):
        assert torch.equal(tiny.embed_ids([t])[0], E[i]), f"text {i} ({len(t)} tokens) alone"
    rev = tiny.embed_ids(ids[::-1])
    assert torch.equal(rev.flip(0), E)
    small = import_module(PKG_DIR + ".encoder").TextEncoder(tiny.cfg, tiny.device, weights=tiny.w,
                                                            max_tokens=1)   # floor: n_pos per pass
    assert small.max_tokens == tiny.cfg.n_pos
    many = ids * 5                                   # 1655 tokens: four passes
    Em = small.embed_ids(many)
    assert torch.equal(Em, E.repeat(5, 1))


def test_only_bf16_and_only_valid_ids(tiny, dev, ops):
    with pytest.raises(ops.CSError, match="bf16 only"):
        build_encoder("tiny", dev, dtype=torch.float32)
    with pytest.raises(ops.CSError, match="1 .. 512"):
        tiny.embed_ids([[1] * 513])
    with pytest.raises(ops.CSError, match="1 .. 512"):
        tiny.embed_ids([[]])
    with pytest.raises(ops.CSError, match="outside"):
        tiny.embed_ids([[1, 512]])
    assert tuple(tiny.embed_ids([]).shape) == (0, 128)


def test_load_encoder_reads_a_bert_checkpoint(tiny, dev, golden, golden_dir, tmp_path):
    """config.json + safetensors under HF's names + tokenizer.json -> the same encoder."""
    import shutil

    from safetensors.numpy import save_file

    c = er.SHAPES["tiny"]
    conf = {"model_type": "bert", "architectures": ["BertModel"], "vocab_size": c["vocab"],
            "hidden_size": c["hidden"], "num_hidden_layers": c["layers"],
            "num_attention_heads": c["heads"], "intermediate_size": c["ffn"],
            "max_position_embeddings": c["n_pos"], "type_vocab_size": 2, "hidden_act": "gelu",
            "layer_norm_eps": er.LN_EPS, "position_embedding_type": "absolute"}
    (tmp_path / "config.json").write_text(json.dumps(conf))
    save_file(er.make_weights("tiny"), str(tmp_path / "model.safetensors"))
    shutil.copy(os.path.join(golden_dir, "wordpiece_fixture", "tokenizer.json"), tmp_path / "tokenizer.json")
    R = import_module(PKG_DIR + ".runtime")
    try:
        enc, tok = R.get_encoder(str(tmp_path))
        ids = texts_of(golden, "tiny")
        assert torch.equal(enc.embed_ids(ids), tiny.embed_ids(ids))
        assert tok.max_len == 512 and tok.encode("safer streets")[0] == tok.cls_id
        assert R.get_encoder(str(tmp_path))[0] is enc
    finally:
        R.clear_encoders()
