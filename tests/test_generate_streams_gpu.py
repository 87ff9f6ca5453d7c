"""runtime.generate_streams (device-closed sampling loop: DecodeState graph replays ending in
the LM head + cs_sample_step) against a reference loop written here on the SAME
prefill_streams + DecodeState forward with the control on the host (lm_head, apply_bias,
ops.vocab_sample with draw_seed, the state machine of tests/sample_step_ref.py, the next
tokens uploaded and the step advanced) -- every token equal.

The engines are the tiny-llama / tiny-gemma presets with the head shapes the stream kernels
serve (head_dim 64 / 128; the presets' own head_dim 16 has no DecodeState), as the other
stream-decode tests build them; tiny-gemma keeps its final soft-cap of 30.

Token equality with runtime.generate is deliberately not asserted: it runs other forward
kernels in bf16, and a near-tie may fall either way.
"""
import warnings
from importlib import import_module

import pytest
import torch

from conftest import PKG_DIR
from sample_step_ref import StepState

pytestmark = pytest.mark.gpu

SEEDS = [11, (1 << 63) + 5]
ISSUE = "How should the city spend its budget?"
OPINIONS = {"Agent 1": "We should fund public transit first.",
            "Agent 2": "Lower the city's taxes before anything else."}


@pytest.fixture(scope="module")
def mods(pkg):
    return {n: import_module(f"{pkg.__name__}.{n}")
            for n in ("model", "engine", "runtime", "tokenizer", "utils", "methods", "ops")}


def _engine(mods, family, dev, dtype=torch.bfloat16):
    M, E, T = mods["model"], mods["engine"], mods["tokenizer"]
    if family == "llama3":
        cfg = M.preset("tiny-llama", vocab=512, d_model=256, n_heads=8, n_kv_heads=2, head_dim=64,
                       d_ff=512, n_layers=3, init_std=0.05)
    else:
        cfg = M.preset("tiny-gemma", vocab=512, d_model=256, n_heads=4, n_kv_heads=2,
                       head_dim=128, d_ff=512, n_layers=3, sliding_window=4096,
                       query_pre_attn_scalar=128.0, init_std=0.05)
    eng = E.ScoringEngine(M.Model(cfg, dev, dtype, seed=3), reuse_caches=0)
    return eng, T.CharTokenizer(family, vocab_size=cfg.vocab)


@pytest.fixture(scope="module")
def engines(mods, dev):
    return {f: _engine(mods, f, dev) for f in ("llama3", "gemma2")}


def prompts(tok, lens=(5, 33, 64)):
    """Prompts either side of the 32-key prefix padding."""
    g = torch.Generator().manual_seed(7)
    return [[tok.bos_id] + [int(x) for x in torch.randint(40, 300, (n - 1,), generator=g)]
            for n in lens]


def ref_loop(mods, eng, tok, prefixes, per_seeds, max_tokens, *, temperature=1.0, bias=(),
             bias_value=-1e6, stop=None, use_graphs=True):
    """Host-controlled generation on the stream decode -> (tokens, lps, advances), [prompt][seed]."""
    R, E, ops = mods["runtime"], mods["engine"], mods["ops"]
    P, B = len(prefixes), max(len(r) for r in per_seeds)
    S = P * B
    dev = eng.device
    stop = list(tok.eos_ids if stop is None else stop)
    pad = tok.eos_ids[0]
    done0 = [0 if b < len(r) else 1 for r in per_seeds for b in range(B)]
    base = [r[b] if b < len(r) else 0 for r in per_seeds for b in range(B)]
    state = StepState(S, max_tokens, pad, stop_ids=stop, done=done0)
    sp = eng.prefill_streams(prefixes)
    st = E.DecodeState(eng, sp, n_prefix=P, n_beams=B, max_steps=max(1, max_tokens - 1),
                       use_graphs=use_graphs)
    try:
        for t in range(max_tokens):
            logits = R.apply_bias(eng.model.lm_head(st.hidden).float(), list(bias), bias_value)
            sd = torch.tensor([[R.to_i64(R.draw_seed(b, t))] for b in base], dtype=torch.int64,
                              device=dev)
            ids, lp = ops.vocab_sample(logits, sd, temperature=temperature, softcap=eng.softcap)
            state.step(t, lambda _t: (ids[:, 0].tolist(), lp[:, 0].tolist()))
            if state.n_alive == 0 or t + 1 == max_tokens:
                break
            st.tok.copy_(torch.tensor(state.next_tok, dtype=torch.long, device=dev))
            st.advance_device()                      # src stays the identity
        torch.cuda.synchronize()
        advances = st.steps
    finally:
        st.release()
    seqs = state.sequences()
    toks = [[seqs[p * B + b] for b in range(len(r))] for p, r in enumerate(per_seeds)]
    lps = [[state.out_lp[p * B + b][:state.out_len[p * B + b]] for b in range(len(r))]
           for p, r in enumerate(per_seeds)]
    return toks, lps, advances


@pytest.fixture(scope="module")
def base_runs(mods, engines):
    """Per family: generate_streams and the graph reference, 3 prompts x 2 seeds x 12 tokens,
    no stop ids (shared by the tests below; never modified)."""
    out = {}
    for fam, (eng, tok) in engines.items():
        pf = prompts(tok)
        got = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 12, stop_ids=[])
        ref, _, _ = ref_loop(mods, eng, tok, pf, [SEEDS] * 3, 12, stop=[])
        out[fam] = (pf, got, ref)
    return out


@pytest.mark.parametrize("fam", ["llama3", "gemma2"])
def test_every_token_equals_the_reference_loop(mods, engines, base_runs, fam):
    eng, tok = engines[fam]
    pf, got, ref_graph = base_runs[fam]
    ref_eager, _, _ = ref_loop(mods, eng, tok, pf, [SEEDS] * 3, 12, stop=[], use_graphs=False)
    if ref_eager != ref_graph:       # a finding about the existing decode path, not this one
        warnings.warn(f"{fam}: the reference loop differs between graph replay and eager steps")
    assert [len(r) for r in got] == [2, 2, 2]
    assert all(len(s) == 12 for r in got for s in r)
    assert got == ref_graph
    # default stop ids (tok.eos_ids) against the same reference rule
    got_eos = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 12)
    assert got_eos == ref_loop(mods, eng, tok, pf, [SEEDS] * 3, 12)[0]


def test_stop_id_cuts_streams_at_its_first_occurrence(mods, engines, base_runs):
    eng, tok = engines["llama3"]
    pf, got, _ = base_runs["llama3"]
    stop = got[0][0][3]
    cut = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 12, stop_ids=[stop])
    first = got[0][0].index(stop)
    assert first <= 3 and len(cut[0][0]) == first
    if first == 3:
        assert len(cut[0][0]) == 3
    for p in range(3):
        for b in range(2):
            want = got[p][b][:got[p][b].index(stop)] if stop in got[p][b] else got[p][b]
            assert cut[p][b] == want, (p, b)


def test_lengths_one_and_past_the_history_tile(mods, engines, monkeypatch):
    eng, tok = engines["llama3"]
    E, R = mods["engine"], mods["runtime"]
    pf = prompts(tok)[:2]
    calls = []
    real = E.DecodeState.advance_device
    monkeypatch.setattr(E.DecodeState, "advance_device",
                        lambda self, post=None: (calls.append(1), real(self, post=post))[1])
    one = R.generate_streams(eng, tok, pf, SEEDS, 1, stop_ids=[])
    assert calls == [] and [[len(s) for s in r] for r in one] == [[1, 1], [1, 1]]
    long = R.generate_streams(eng, tok, pf, SEEDS, 33, stop_ids=[])
    assert len(calls) == 32 and all(len(s) == 33 for r in long for s in r)
    monkeypatch.undo()
    ref, _, adv = ref_loop(mods, eng, tok, pf, [SEEDS] * 2, 33, stop=[])
    assert adv == 32 and long == ref
    assert [[s[:1] for s in r] for r in long] == one


def test_polling_interval_changes_nothing(mods, engines, base_runs):
    eng, tok = engines["gemma2"]
    pf, got, _ = base_runs["gemma2"]
    # a stop id some streams draw, so streams end at different steps
    stop = [got[1][0][5]]
    runs = [mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 12, stop_ids=stop, poll_every=k)
            for k in (1, 8, 1000)]
    assert runs[0] == runs[1] == runs[2]
    assert len(runs[0][1][0]) <= 5


def test_ragged_seed_lists(mods, engines):
    eng, tok = engines["llama3"]
    pf = prompts(tok)[:2]
    seeds = [[1, 2, 3], [4]]
    got = mods["runtime"].generate_streams(eng, tok, pf, seeds, 6, stop_ids=[])
    assert [len(r) for r in got] == [3, 1]
    assert got == ref_loop(mods, eng, tok, pf, seeds, 6, stop=[])[0]
    assert all(len(s) == 6 for r in got for s in r)


def test_bias_changes_the_draw_as_apply_bias_does(mods, engines, base_runs):
    eng, tok = engines["llama3"]
    pf, got, _ = base_runs["llama3"]
    first = got[0][0][0]
    bias = [first, first]                            # listed twice: counted once
    out = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 12, bias_ids=bias,
                                           bias_value=-1e6, stop_ids=[])
    assert out[0][0][0] != first and all(first not in s for r in out for s in r)
    assert out == ref_loop(mods, eng, tok, pf, [SEEDS] * 3, 12, bias=bias, stop=[])[0]


def test_logprobs_equal_the_reference_loop(mods, engines):
    eng, tok = engines["gemma2"]
    pf = prompts(tok)
    toks, lps = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, 6, temperature=0.7,
                                                 stop_ids=[], return_logprobs=True)
    rt, rl, _ = ref_loop(mods, eng, tok, pf, [SEEDS] * 3, 6, temperature=0.7, stop=[])
    assert toks == rt
    assert lps == rl
    assert all(v <= 0.0 for r in lps for s in r for v in s)


def test_fp32_engine_is_refused(mods, pkg, dev):
    eng, tok = mods["runtime"].random_engine("tiny-llama", dev, dtype=torch.float32, seed=1)
    with pytest.raises(pkg.CSError, match="float32"):
        mods["runtime"].generate_streams(eng, tok, [[tok.bos_id, 50]], [1], 4)


@pytest.fixture
def registered(mods, engines):
    R = mods["runtime"]
    eng, tok = engines["llama3"]
    R.register_engine("test/streams", eng, tok)
    yield "test/streams", eng, tok
    R.clear_engines()


def test_generate_texts(mods, registered):
    name, eng, tok = registered
    U, R = mods["utils"], mods["runtime"]
    users, systems = ["Name a colour.", "Name a much longer list of animals, please."], "Be brief."
    texts = U.generate_texts(name, users, systems, n_per_prompt=2, max_tokens=10, seeds=[3, 4],
                             terminators=("e",))
    idss = [tok.render_chat(systems, u)[0] for u in users]
    want = [[tok.decode(o) for o in row] for row in R.generate_streams(eng, tok, idss, [3, 4], 10)]
    want = [[t[:t.find("e")] if "e" in t else t for t in row] for row in want]
    assert texts == want and [len(r) for r in texts] == [2, 2]
    bad = U.generate_texts("test/unknown-model", users, n_per_prompt=2, max_tokens=4)
    assert [len(r) for r in bad] == [2, 2]
    assert all(t.startswith("[ERROR: ") and t.endswith("]") for r in bad for t in r)


def test_best_of_n_on_the_device_path(mods, registered, monkeypatch):
    name, eng, tok = registered
    R = mods["runtime"]
    bon = import_module(PKG_DIR + ".methods.best_of_n")
    cfg = {"n": 4, "max_tokens": 8, "seed": 5}
    host_calls = []
    real = R.generate
    monkeypatch.setattr(R, "generate", lambda *a, **k: (host_calls.append(1), real(*a, **k))[1])
    gen = mods["methods"].get_method_generator("best_of_n", dict(cfg, generation="device"), name)
    text = gen.generate_statement(ISSUE, OPINIONS)
    assert host_calls == []                          # the device path never enters generate
    assert gen.last_candidates and text in gen.last_candidates
    ref_user = bon.BON["ref_user"].format(issue=ISSUE, opinions_text=bon.opinions_text(OPINIONS))
    ref_ids, _ = tok.render_chat(bon.BON["ref_system"], ref_user)
    outs = R.generate_streams(eng, tok, [ref_ids], [5 + i for i in range(4)], 8)[0]
    want = [c for c in (bon.clean_generated_text(tok.decode(o)) for o in outs) if c]
    assert gen.last_candidates == want
    again = mods["methods"].get_method_generator("best_of_n", dict(cfg, generation="device"), name)
    assert again.generate_statement(ISSUE, OPINIONS) == text
    # the default configuration still generates through runtime.generate
    default = mods["methods"].get_method_generator("best_of_n", dict(cfg), name)
    default.generate_statement(ISSUE, OPINIONS)
    assert host_calls == [1]
