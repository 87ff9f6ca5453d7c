"""runtime.generate / generate_streams / utils.generate_text(s) under a constraint
(runtime.compile_constraint), on the 3-layer random engines of tests/test_generate_streams_gpu.py
(character tokenizer) and of tests/test_text_path_gpu.py (the byte-level BPE fixture).

A random model never writes a format by itself, so every property here is the constraint's:
finished texts match, texts cut at max_tokens are live prefixes, the device loop equals the
host loop token for token, and each prompt of a batch follows its own pattern."""
import json
import re
from importlib import import_module

import pytest

import test_text_path_gpu as bpe_engines
from conftest import PKG_DIR
from test_generate_streams_gpu import SEEDS, _engine, prompts

pytestmark = pytest.mark.gpu

C = import_module(PKG_DIR + ".constrain")
BOUNDED = r'\{"score": (10|[1-9]), "ok": (true|false)\}'
WORDS = r"(yes|no|maybe)( [a-c]{1,3})?"
LONGEST = 26                        # bytes of the longest text BOUNDED matches


@pytest.fixture(scope="module")
def mods(pkg):
    return {n: import_module(f"{pkg.__name__}.{n}")
            for n in ("model", "engine", "runtime", "tokenizer", "utils", "ops")}


@pytest.fixture(scope="module")
def engines(mods, dev):
    out = {("char", f): _engine(mods, f, dev) for f in ("llama3", "gemma2")}
    out.update({("bpe", f): bpe_engines._engine(dev, f) for f in ("llama3", "gemma2")})
    return out


def text_bytes(con, ids):
    return b"".join(con.token_bytes(v) for v in ids)


def check_rows(con, dfa, pattern, rows, max_tokens, start=None):
    """Every stream: finished -> its text matches; cut at max_tokens -> a live prefix."""
    n_done = 0
    for row in rows:
        for ids in row:
            text = text_bytes(con, ids)
            q = dfa.walk(dfa.start if start is None else start, text)
            assert q >= 0, text                                 # never a dead text
            if len(ids) < max_tokens:
                n_done += 1
                assert dfa.accept[q] and re.fullmatch(pattern, text.decode("utf-8")), text
    return n_done


CASES = [(k, f) for k in ("char", "bpe") for f in ("llama3", "gemma2")]


@pytest.mark.parametrize("kind,fam", CASES)
def test_streams_follow_the_pattern_and_equal_the_host_loop(mods, engines, kind, fam):
    R = mods["runtime"]
    eng, tok = engines[(kind, fam)]
    con = R.compile_constraint(tok, BOUNDED)
    assert R.compile_constraint(tok, BOUNDED) is con            # built once
    dfa = C.compile_regex(BOUNDED)
    pf = prompts(tok)
    n = LONGEST + 2                                             # room for every match
    got = R.generate_streams(eng, tok, pf, SEEDS, n, constraint=con)
    assert check_rows(con, dfa, BOUNDED, got, n) == len(pf) * len(SEEDS)
    free = R.generate_streams(eng, tok, pf, SEEDS, 4)
    assert all(not dfa.accepts(text_bytes(con, s)) for r in free for s in r)   # not by itself
    short = R.generate_streams(eng, tok, pf, SEEDS, 5, constraint=con)
    assert check_rows(con, dfa, BOUNDED, short, 5) == 0     # all cut: live prefixes
    host = [[R.generate(eng, tok, p, [s], n, constraint=con)[0] for s in SEEDS] for p in pf]
    assert got == host
    # temperature 0 and a penalty ride along
    kw = dict(temperature=0.0, repetition_penalty=1.3)
    g0 = R.generate_streams(eng, tok, pf[:2], [1], n, constraint=con, **kw)
    assert check_rows(con, dfa, BOUNDED, g0, n) == 2
    assert g0 == [[R.generate(eng, tok, p, [1], n, constraint=con, **kw)[0]] for p in pf[:2]]


@pytest.mark.parametrize("kind", ["char", "bpe"])
def test_each_prompt_follows_its_own_pattern(mods, engines, kind):
    R = mods["runtime"]
    eng, tok = engines[(kind, "llama3")]
    pats = [BOUNDED, WORDS]
    con = R.compile_constraint(tok, pats)
    assert len(con.starts) == 2 and con.starts[0] != con.starts[1]
    pf = prompts(tok)[:2]
    n = LONGEST + 2
    got = R.generate_streams(eng, tok, pf, SEEDS, n, constraint=con)
    for p, pat in enumerate(pats):
        assert check_rows(con, con.dfa, pat, [got[p]], n, start=con.starts[p]) == len(SEEDS)
        assert got[p] == [R.generate(eng, tok, pf[p], [s], n, constraint=con.select(p))[0]
                          for s in SEEDS]
    with pytest.raises(ValueError, match="2 patterns for 3 prompts"):
        R.generate_streams(eng, tok, prompts(tok), SEEDS, 4, constraint=con)
    with pytest.raises(mods["ops"].CSError, match="stop ids"):
        R.generate_streams(eng, tok, pf, SEEDS, 4, constraint=con, stop_ids=[])


@pytest.fixture
def registered(mods, engines):
    R = mods["runtime"]
    eng, tok = engines[("char", "llama3")]
    R.register_engine("test/constrained", eng, tok)
    yield "test/constrained", eng, tok
    R.clear_engines()


def test_generate_texts_with_a_pattern_and_a_response_format(mods, registered):
    name, eng, tok = registered
    U, R = mods["utils"], mods["runtime"]
    users = ["Rate this statement.", "Rate this much longer statement, please."]
    seeds, n = [3, 4], LONGEST + 2
    texts = U.generate_texts(name, users, max_tokens=n, seeds=seeds, pattern=BOUNDED)
    idss = [tok.render_chat(None, u)[0] for u in users]
    want = R.generate_streams(eng, tok, idss, seeds, n,
                              constraint=R.compile_constraint(tok, BOUNDED))
    assert texts == [[tok.decode(o) for o in row] for row in want]
    for row in texts:
        for t in row:
            obj = json.loads(t)
            assert re.fullmatch(BOUNDED, t) and 1 <= obj["score"] <= 10 and obj["ok"] in (True, False)
    per = U.generate_texts(name, users, max_tokens=n, seeds=seeds, pattern=[WORDS, BOUNDED])
    assert all(re.fullmatch(WORDS, t) for t in per[0]) and per[1] == texts[1]
    one = U.generate_text(name, users[0], max_tokens=n, seed=3, pattern=BOUNDED)
    assert re.fullmatch(BOUNDED, one)
    # the hosted API's spelling: one JSON object, or a live prefix of one at max_tokens
    dfa = C.json_object(2)
    js = U.generate_texts(name, users, max_tokens=24, seeds=seeds,
                          response_format={"type": "json_object"})
    con = R.compile_constraint(tok, {"type": "json_object"})
    raw = R.generate_streams(eng, tok, idss, seeds, 24, constraint=con)
    assert js == [[tok.decode(o) for o in row] for row in raw]
    for row, ids_row in zip(js, raw):
        for t, ids in zip(row, ids_row):
            assert not t.startswith("[ERROR") and t.startswith("{")
            assert dfa.walk(dfa.start, t.encode("utf-8")) >= 0
            if len(ids) < 24:
                assert isinstance(json.loads(t), dict)
    j1 = U.generate_text(name, users[0], max_tokens=8, seed=3,
                         response_format={"type": "json_object"})
    assert j1.startswith("{") and dfa.walk(dfa.start, j1.encode("utf-8")) >= 0


@pytest.mark.parametrize("kw", [
    dict(response_format={"type": "xml"}),
    dict(response_format="json_object"),
    dict(pattern=BOUNDED, response_format={"type": "json_object"}),
    dict(pattern=r"^anchored$"),
])
def test_bad_formats_fill_the_error_slots(mods, registered, kw):
    name, _, _ = registered
    U = mods["utils"]
    out = U.generate_texts(name, ["a", "b"], n_per_prompt=2, max_tokens=4, **kw)
    assert out == [["[ERROR: ValueError]"] * 2] * 2
    assert U.generate_text(name, "a", max_tokens=4, **kw) == "[ERROR: ValueError]"


def test_a_tokenizer_without_a_byte_table_is_refused(mods, pkg):
    R = mods["runtime"]

    class NoTable:
        eos_ids = (1,)

    class EmptyTable(NoTable):
        def token_bytes(self):
            return None

    for tok in (NoTable(), EmptyTable(), mods["tokenizer"].RandomIdTokenizer(64, 16)):
        with pytest.raises(pkg.CSError, match="token_bytes"):
            R.compile_constraint(tok, BOUNDED)
