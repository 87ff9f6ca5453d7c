"""§8(f) row 4 — output formats: the evaluator's file-level path writes
evaluation_results.csv in the reference's layout (column schema of the published
file), and it still carries what the reference's own improved_aggregation consumed from
it (checked against the table that aggregator wrote, stored with the fixture).  Kernels
are emulated by the oracle here (host logic only); tests/test_methods_gpu.py covers the
same evaluator on the MI355X."""
import importlib
import math
import os
import re
import shutil

import pandas as pd
import pytest
import torch

import method_parity as mp

PKG = mp.PKG
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "results_fixture")


@pytest.fixture(scope="module")
def evaluated(tmp_path_factory, orc):
    import cpu_emulation
    R = importlib.import_module(PKG + ".runtime")
    saved = cpu_emulation.install()
    traces = mp.load_traces()
    eng, tok = mp.register_fixture_engine(traces, torch.device("cpu"))
    R.register_engine("google/gemma-2-9b-it", eng, tok)
    run = tmp_path_factory.mktemp("run")
    shutil.copy(os.path.join(FIX, "results.csv"), run / "results.csv")
    shutil.copy(os.path.join(FIX, "config.yaml"), run / "config.yaml")
    ev_mod = importlib.import_module(PKG + ".evaluation")
    ev = ev_mod.StatementEvaluator("google/gemma-2-9b-it", include_comparative_ranking=False,
                                   verbose=False)
    out = run / "evaluation" / "google_gemma-2-9b-it" / "seed_0"
    combined = ev.evaluate_results_file(run / "results.csv", output_dir=out, is_seed_specific=True)
    yield run, out, combined
    cpu_emulation.uninstall(saved)
    R.clear_engines()


def test_evaluation_csv_schema_matches_published(evaluated):
    run, out, combined = evaluated
    ours = pd.read_csv(out / "evaluation_results.csv")
    published = open(os.path.join(FIX, "published_evaluation_header.csv")).readline().strip().split(",")
    assert list(ours.columns) == published
    assert len(ours) == len(pd.read_csv(os.path.join(FIX, "results.csv")))
    assert (combined["evaluation_status"] == "completed").all()


def test_evaluation_csv_welfare_identities(evaluated):
    run, out, _ = evaluated
    df = pd.read_csv(out / "evaluation_results.csv")
    agents = [c[len("avg_logprob_"):] for c in df.columns if c.startswith("avg_logprob_")]
    for _, r in df.iterrows():
        ppl = [math.exp(-r[f"avg_logprob_{a}"]) for a in agents]
        assert abs(r["egalitarian_welfare_perplexity"] - max(ppl)) <= 1e-3 * max(ppl)
        assert abs(r["utilitarian_welfare_perplexity"] - sum(ppl)) <= 1e-3 * sum(ppl)
        assert abs(r["log_nash_welfare_perplexity"] - sum(r[f"avg_logprob_{a}"] for a in agents)) < 1e-3


def test_reference_improved_aggregation_consumes_our_output(evaluated):
    """golden/results_fixture/reference_aggregated_metrics.csv is the table the reference's
    improved_aggregation wrote when it was run on this fixture's evaluation_results.csv
    (one row per method key, mean and population std over the seeds of every perplexity
    column it picked up).  What it consumed must still be in our file: the same method
    keys from ``method`` / ``method_with_params``, every column it aggregated, and values
    that fold to the recorded numbers.  Tolerance: the fixture model's fp32 CPU forward
    moves a mean log-prob by ~1e-6 with the summation order (thread count), i.e. a
    perplexity by ~1e-6 relative; 1e-4 of the column's mean is far above that and far
    below the seed-to-seed spread the std columns measure."""
    run, out, _ = evaluated
    ours = pd.read_csv(out / "evaluation_results.csv")
    ref = pd.read_csv(os.path.join(FIX, "reference_aggregated_metrics.csv"))
    assert len(ref) >= 1
    metrics = [c[:-len("_mean")] for c in ref.columns if c.endswith("_mean")]
    assert metrics and all("perplexity" in m for m in metrics)
    assert all(m in ours.columns and m + "_std" in ref.columns for m in metrics)
    # the aggregator's method key: method_with_params without its "[seed=...]" suffix
    key = ours["method_with_params"].str.replace(r"\s*\[seed=\d+\]$", "", regex=True)
    assert sorted(key.unique()) == sorted(ref["method_with_params"])
    for _, r in ref.iterrows():
        rows = ours[key == r["method_with_params"]]
        assert (rows["method"] == r["method"]).all()
        assert re.search(r"beam_width=(\d+)", r["method_with_params"]).group(1) == \
            str(r["param_beam_width"])
        for m in metrics:
            tol = 1e-4 * abs(r[m + "_mean"])
            assert abs(rows[m].mean() - r[m + "_mean"]) <= tol, (r["method_with_params"], m)
            assert abs(rows[m].std(ddof=0) - r[m + "_std"]) <= tol, (r["method_with_params"], m)
