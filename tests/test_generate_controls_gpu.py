"""temperature 0, repetition_penalty and stop strings through runtime.generate (host loop),
runtime.generate_streams (device loop, cs_sample_step_ex) and utils.generate_text(s), on the
3-layer random engines and the prompt lengths of tests/test_generate_streams_gpu.py.

Figures printed under -s: the number of streams compared per case, and the decode steps with
and without the device's stop-string test."""
from importlib import import_module

import pytest
import torch

import sample_controls_ref as R
from test_generate_streams_gpu import SEEDS, _engine, prompts

pytestmark = pytest.mark.gpu

N_TOK = 8


@pytest.fixture(scope="module")
def mods(pkg):
    return {n: import_module(f"{pkg.__name__}.{n}")
            for n in ("model", "engine", "runtime", "tokenizer", "utils", "ops")}


@pytest.fixture(scope="module")
def engines(mods, dev):
    return {f: _engine(mods, f, dev) for f in ("llama3", "gemma2")}


def host_loop(mods, eng, tok, pf, seeds, n, **kw):
    """runtime.generate stream by stream: [prompt][seed] token lists."""
    return [[mods["runtime"].generate(eng, tok, p, [s], n, **kw)[0] for s in seeds] for p in pf]


MODES = {
    "greedy": dict(temperature=0.0),
    "penalty": dict(temperature=1.0, repetition_penalty=1.3),
    "greedy_penalty": dict(temperature=0.0, repetition_penalty=1.3),
}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("fam", ["llama3", "gemma2"])
def test_streams_equal_the_host_loop(mods, engines, fam, mode):
    eng, tok = engines[fam]
    pf = prompts(tok)
    got = mods["runtime"].generate_streams(eng, tok, pf, SEEDS, N_TOK, stop_ids=[], **MODES[mode])
    want = host_loop(mods, eng, tok, pf, SEEDS, N_TOK, stop_ids=[], **MODES[mode])
    same = sum(g == w for rg, rw in zip(got, want) for g, w in zip(rg, rw))
    print(f"{fam} {mode}: {same} of {len(pf) * len(SEEDS)} streams equal")
    assert all(len(s) == N_TOK for r in got for s in r)
    assert got == want


@pytest.mark.parametrize("fam", ["llama3", "gemma2"])
def test_greedy_ignores_the_seed(mods, engines, fam):
    eng, tok = engines[fam]
    pf = prompts(tok)
    a = mods["runtime"].generate_streams(eng, tok, pf, [1], N_TOK, temperature=0.0, stop_ids=[])
    b = mods["runtime"].generate_streams(eng, tok, pf, [2 ** 40 + 7], N_TOK, temperature=0.0,
                                         stop_ids=[])
    assert a == b
    sampled = mods["runtime"].generate_streams(eng, tok, pf, [1], N_TOK, stop_ids=[])
    assert sampled != a                                       # and it is not the sampled text


@pytest.mark.parametrize("fam", ["llama3", "gemma2"])
def test_defaults_spelled_out_change_no_token(mods, engines, fam):
    eng, tok = engines[fam]
    pf = prompts(tok)
    Rt = mods["runtime"]
    plain = Rt.generate_streams(eng, tok, pf, SEEDS, N_TOK, temperature=0.7)
    assert Rt.generate_streams(eng, tok, pf, SEEDS, N_TOK, temperature=0.7,
                               repetition_penalty=1.0, stop_strings=()) == plain
    host = Rt.generate(eng, tok, pf[1], SEEDS, N_TOK, temperature=0.7)
    assert Rt.generate(eng, tok, pf[1], SEEDS, N_TOK, temperature=0.7, repetition_penalty=1.0,
                       stop_strings=None) == host


@pytest.fixture
def registered(mods, engines):
    Rt = mods["runtime"]
    eng, tok = engines["llama3"]
    Rt.register_engine("test/controls", eng, tok)
    yield "test/controls", eng, tok
    Rt.clear_engines()


def _ascii_terminator(tok, rows):
    """A printable ASCII character some stream generates after its first token."""
    for row in rows:
        for seq in row:
            for v in seq[1:]:
                s = tok.token_str(v)
                if len(s) == 1 and s.isascii() and s.isprintable() and s != "<":
                    return s
    raise AssertionError("no ASCII character in any stream: other seeds")


def test_ascii_terminator_ends_streams_early_and_keeps_the_texts(mods, registered, monkeypatch):
    name, eng, tok = registered
    U, Rt = mods["utils"], mods["runtime"]
    users, systems = ["Name a colour.", "Name a much longer list of animals, please."], "Be brief."
    seeds, n = [3, 4, 5], 12
    idss = [tok.render_chat(systems, u)[0] for u in users]
    steps = []
    real = mods["engine"].DecodeState.advance_device
    monkeypatch.setattr(mods["engine"].DecodeState, "advance_device",
                        lambda self, post=None: (steps.append(1), real(self, post=post))[1])
    full = Rt.generate_streams(eng, tok, idss, seeds, n)
    full_steps, steps[:] = 1 + len(steps), []
    term = _ascii_terminator(tok, full)
    assert Rt.early_stop_strings((term,)) == [term.encode()]
    table = Rt.stop_token_table(tok, eng.model.cfg.vocab)
    cut = Rt.generate_streams(eng, tok, idss, seeds, n, stop_strings=(term,))
    cut_steps = 1 + len(steps)
    ended = 0
    for p in range(len(users)):
        for b in range(len(seeds)):
            k = R.run_window(table, full[p][b], [term.encode()])
            if all(v >= len(tok.special_ids) for v in full[p][b]):
                # one character per token: the restatement's step is str.find's place
                at = tok.decode(full[p][b]).find(term)
                assert k == (None if at < 0 else at)
            want = full[p][b] if k is None else full[p][b][:k + 1]
            assert cut[p][b] == want, (p, b)
            ended += k is not None
    print(f"terminator {term!r}: {ended} of {len(users) * len(seeds)} streams ended early, "
          f"{cut_steps} decode steps against {full_steps}")
    assert ended >= 1 and cut_steps <= full_steps
    texts = U.generate_texts(name, users, systems, max_tokens=n, seeds=seeds, terminators=(term,))
    monkeypatch.setattr(Rt, "early_stop_strings", lambda s: [])       # device stop disabled
    assert U.generate_texts(name, users, systems, max_tokens=n, seeds=seeds,
                            terminators=(term,)) == texts
    assert all(term not in t and not t.startswith("[ERROR") for r in texts for t in r)


def test_generate_text_at_temperature_zero(mods, registered):
    name, eng, tok = registered
    U = mods["utils"]
    a = U.generate_text(name, "Name a colour.", max_tokens=N_TOK, temperature=0, seed=1)
    b = U.generate_text(name, "Name a colour.", max_tokens=N_TOK, temperature=0, seed=99)
    assert isinstance(a, str) and not a.startswith("[ERROR") and a == b
    many = U.generate_texts(name, ["Name a colour."], max_tokens=N_TOK, temperature=0, seeds=[5])
    assert not many[0][0].startswith("[ERROR")


def test_generate_text_repetition_penalty_changes_a_repeating_continuation(mods, registered):
    name, eng, tok = registered
    U, Rt = mods["utils"], mods["runtime"]
    n = 16
    for user in ("Name a colour.", "aaaa", "List three animals.", "Why?", "1 2 3 4 5 6"):
        ids, _ = tok.render_chat(None, user)
        base = Rt.generate(eng, tok, ids, [1], n, temperature=0.0)[0]
        if len(set(base)) < len(base):
            break
    else:
        raise AssertionError("no prompt whose greedy continuation repeats a token")
    pen = Rt.generate(eng, tok, ids, [1], n, temperature=0.0, repetition_penalty=1.3)[0]
    assert pen != base                                        # the host loop alone shows it
    plain = U.generate_text(name, user, max_tokens=n, temperature=0, seed=1)
    again = U.generate_text(name, user, max_tokens=n, temperature=0, seed=1, repetition_penalty=1.0)
    penalised = U.generate_text(name, user, max_tokens=n, temperature=0, seed=1,
                                repetition_penalty=1.3)
    assert plain == again == tok.decode(base)
    assert penalised == tok.decode(pen) and penalised != plain
