"""The evaluator's embedding block on the MI355X (src/evaluation.py:166-174, 232-307): with a
registered text encoder ``evaluate_statements_batched`` fills every cosine key from one
encoder pass and one cs_cosine_welfare launch; the values are the reference's arithmetic
(1 - scipy cosine distance, min / sum / sum-log folds) on ``get_embedding``'s lists to 1e-12;
the rows feed the CSV writer.  With nothing registered the rows are what they were."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import encoder_ref as er
import method_parity as mp
from encoder_ref import build_encoder

pytestmark = pytest.mark.gpu

MODEL = "google/gemma-2-9b-it"
EMB = "BAAI/bge-large-en-v1.5"
ISSUE = "Should the city invest in cycling lanes?"
OPINIONS = {"Agent 1": "Cleaner air matters to everyone, so the council should invest.",
            "Agent 2": "Taxes on fuel are unfair to people who live in the countryside.",
            "Agent 3": "Most people want safer streets."}
STATEMENTS = ["We should invest in public transport and cycling lanes.",
              "A consensus statement balances every opinion fairly.",
              "Most people want safer streets.",       # an opinion verbatim: similarity 1
              "Opinions differ, yet the council agrees that cleaner air matters."]


@pytest.fixture(scope="module")
def evaluator(dev):
    R = importlib.import_module(mp.PKG + ".runtime")
    mp.register_fixture_engine(mp.load_traces("method_traces_wide.json"), dev, dtype=torch.bfloat16,
                               model_id=MODEL)
    ev_mod = importlib.import_module(mp.PKG + ".evaluation")
    yield ev_mod.StatementEvaluator(MODEL, include_comparative_ranking=False, verbose=False), R
    R.clear_engines()
    R.clear_encoders()


@pytest.fixture(scope="module")
def baseline(evaluator):
    """The rows with no encoder registered (computed first, once)."""
    ev, R = evaluator
    R.clear_encoders()
    return ev.evaluate_statements_batched(STATEMENTS, ISSUE, OPINIONS)


@pytest.fixture(scope="module")
def with_encoder(evaluator, baseline, dev, golden_dir):
    ev, R = evaluator
    T = importlib.import_module(mp.PKG + ".tokenizer")
    tok = T.WordPieceTokenizer(os.path.join(golden_dir, "wordpiece_fixture"))
    R.register_encoder(EMB, build_encoder("tiny", dev), tok)
    rows = ev.evaluate_statements_batched(STATEMENTS, ISSUE, OPINIONS)
    return rows


def test_rows_without_an_encoder_are_todays(baseline):
    assert len(baseline) == len(STATEMENTS)
    for r in baseline:
        assert r["statement_embedding"] is None
        for a in OPINIONS:
            assert r[f"cosine_similarity_{a}"] is None and r[f"utility_cosine_similarity_{a}"] is None
            assert f"avg_logprob_{a}" in r
        for kind in ("egalitarian", "utilitarian", "log_nash"):
            assert math.isnan(r[f"{kind}_welfare_cosine"]) and math.isnan(r[f"utility_{kind}_welfare_cosine"])


def test_every_cosine_key_is_filled(with_encoder, baseline):
    for r, b in zip(with_encoder, baseline):
        assert list(r) == list(b), "same keys, same order"
        assert isinstance(r["statement_embedding"], list) and len(r["statement_embedding"]) == 128
        for a in OPINIONS:
            c = r[f"cosine_similarity_{a}"]
            assert isinstance(c, float) and -1.0 <= c <= 1.0
            assert r[f"utility_cosine_similarity_{a}"] == c
        for kind in ("egalitarian", "utilitarian", "log_nash"):
            assert math.isfinite(r[f"{kind}_welfare_cosine"])
            assert r[f"utility_{kind}_welfare_cosine"] == r[f"{kind}_welfare_cosine"]
    assert with_encoder[2]["cosine_similarity_Agent 3"] == pytest.approx(1.0, abs=1e-12)


def test_values_are_the_references_arithmetic_on_get_embedding(with_encoder):
    from scipy.spatial.distance import cosine

    utils = importlib.import_module(mp.PKG + ".utils")
    op_emb = {a: utils.get_embedding(o, model=EMB) for a, o in OPINIONS.items()}
    batch = utils.get_embeddings(STATEMENTS, model=EMB)
    for s, r in zip(STATEMENTS, with_encoder):
        e = utils.get_embedding(s, model=EMB)
        assert isinstance(e, list) and len(e) == 128 and all(isinstance(x, float) for x in e)
        assert e == r["statement_embedding"] and e == batch[STATEMENTS.index(s)]
        assert abs(np.linalg.norm(e) - 1.0) < 1e-6
        sims = [1 - cosine(np.array(e), np.array(op_emb[a])) for a in OPINIONS]
        for a, c in zip(OPINIONS, sims):
            assert abs(r[f"cosine_similarity_{a}"] - c) <= 1e-12
        eg, ut, ln = er.welfare_folds(sims)
        assert abs(r["egalitarian_welfare_cosine"] - eg) <= 1e-12
        assert abs(r["utilitarian_welfare_cosine"] - ut) <= 1e-12
        assert abs(r["log_nash_welfare_cosine"] - ln) <= 1e-12
    assert utils.get_embedding("text", model="no/such-model") is None


def test_rows_feed_the_csv_writer(evaluator, with_encoder, tmp_path):
    import pandas as pd

    ev, _ = evaluator
    df = ev.evaluate_statements({f"method {i}": s for i, s in enumerate(STATEMENTS)}, ISSUE, OPINIONS)
    assert "statement_embedding" not in df.columns
    ev_mod = importlib.import_module(mp.PKG + ".evaluation")
    ev_mod.write_results_csv(df.to_dict("records"), tmp_path / "evaluation_results.csv")
    back = pd.read_csv(tmp_path / "evaluation_results.csv")
    for i, r in enumerate(with_encoder):
        for a in OPINIONS:
            assert back[f"cosine_similarity_{a}"][i] == pytest.approx(r[f"cosine_similarity_{a}"], abs=1e-15)
        for kind in ("egalitarian", "utilitarian", "log_nash"):
            assert back[f"{kind}_welfare_cosine"][i] == pytest.approx(r[f"{kind}_welfare_cosine"], abs=1e-15)
            assert back[f"utility_{kind}_welfare_cosine"][i] == back[f"{kind}_welfare_cosine"][i]
