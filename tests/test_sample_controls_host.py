"""CPU tests around cs_vocab_sample_ex / cs_sample_step_ex: the restatement of
tests/sample_controls_ref.py pinned against transformers' repetition penalty and str.find,
the tokenizers' token_bytes() tables, the host-side stop helpers of runtime, and the ABI text."""
import os
import random
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import sample_controls_ref as R
from conftest import PKG_DIR, REPO

assert "cs_sample_step_ex" in import_module(PKG_DIR + "._lib").EXPORTED

NEW = ("cs_vocab_sample_ex_workspace_size", "cs_vocab_sample_ex",
       "cs_sample_step_ex_workspace_size", "cs_sample_step_ex")


# --- the penalty rule ------------------------------------------------------------------------

def test_penalty_on_the_documented_row():
    got = R.penalise(np.array([2, -1.5, 0, 3], dtype=np.float32), [0, 1, 2], 1.3)
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, [1.5385, -1.95, 0, 3], atol=5e-5)


@pytest.mark.parametrize("penalty", [1.3, 0.7, 2.0, 1.0])
def test_penalty_is_transformers_rule_bit_for_bit(penalty):
    from transformers import RepetitionPenaltyLogitsProcessor

    rng = np.random.default_rng(int(penalty * 10))
    V = 97
    for case in range(12):
        x = (rng.standard_normal(V) * 4).astype(np.float32)
        x[rng.integers(0, V, 6)] = 0.0
        x[rng.integers(0, V, 4)] = -np.inf
        x[3], x[4] = -0.0, np.float32(1e-42)                 # a signed zero and a subnormal
        n = (0, 1, 5, 40)[case % 4]
        seen = [int(i) for i in rng.integers(0, V, n)]
        seen += seen[:2]                                      # duplicates count once
        if case % 3 == 0 and n:
            seen += [int(np.argmax(x == -np.inf)), 3, 4]      # a seen -inf, -0.0, subnormal
        if penalty == 1.0:
            want = x.copy()
        else:
            proc = RepetitionPenaltyLogitsProcessor(penalty=float(penalty))
            want = proc(torch.tensor([seen], dtype=torch.long).reshape(1, len(seen)),
                        torch.from_numpy(x.copy())[None])[0].numpy()
        got = R.penalise(x, seen, penalty)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case, seen)
        # ids outside [0, V) are ignored, NaN stays NaN
        y = x.copy()
        y[7] = np.nan
        wide = R.penalise(y, seen + [V, V + 40, -1, 1 << 30, 7], penalty)
        keep = np.arange(V) != 7
        assert np.array_equal(wide[keep].view(np.int32), got[keep].view(np.int32))
        assert np.isnan(wide[7])


def test_transform_order_is_bias_cap_penalty():
    x = np.array([40.0, -40.0, 1.0, 0.5], dtype=np.float32)
    t = R.transform(x, bias_ids=[0, 0, 9], bias_value=-10.0, softcap=30.0, seen=[0, 1], penalty=2.0)
    want0 = 30.0 * np.tanh((40.0 - 10.0) / 30.0) / 2.0
    want1 = 30.0 * np.tanh(-40.0 / 30.0) * 2.0
    np.testing.assert_allclose(t, [want0, want1, 30 * np.tanh(1 / 30), 30 * np.tanh(0.5 / 30)],
                               rtol=1e-12)


def test_greedy_is_the_first_argmax_over_drawable_tokens():
    assert R.greedy(np.array([1.0, 3.0, 3.0, -np.inf]))[0] == 1
    assert R.greedy(np.array([np.nan, 2.0, 5.0]))[0] == 2 and np.isnan(R.greedy([np.nan, 2.0])[1])
    i, lp = R.greedy(np.array([-np.inf, -np.inf]))
    assert i == -1 and np.isnan(lp)
    i, lp = R.greedy(np.array([0.0, np.log(3.0)]))
    assert i == 1 and abs(lp - np.log(0.75)) < 1e-12


# --- the stop window -------------------------------------------------------------------------

def _random_case(rng, alphabet, n_tok, max_len):
    toks = [bytes(rng.choice(alphabet) for _ in range(rng.randint(0 if v % 7 == 0 else 1, max_len)))
            for v in range(n_tok)]
    ids = [rng.randrange(n_tok) for _ in range(rng.randint(1, 60))]
    return toks, ids


def test_stop_window_is_str_find_on_random_ascii_tables():
    rng = random.Random(5)
    hits = spans = 0
    for case in range(600):
        alphabet = b"ab" if case % 2 else b"abc\n#"
        toks, ids = _random_case(rng, alphabet, rng.randint(2, 12), rng.choice((1, 2, 5, 40)))
        text = b"".join(toks[i] for i in ids)
        stops = []
        for _ in range(rng.randint(1, 8)):
            n = rng.choice((1, 2, 3, 5, 32))
            if text and rng.random() < 0.7 and len(text) >= n:     # planted: it does occur
                at = rng.randrange(len(text) - n + 1)
                stops.append(text[at:at + n])
            else:
                stops.append(bytes(rng.choice(alphabet) for _ in range(n)))
        want = R.first_stop_step(toks, ids, stops)
        assert R.run_window(toks, ids, stops) == want, (case, toks, ids, stops)
        hits += want is not None
        spans += want is not None and any(len(s) > len(toks[ids[want]]) for s in stops)
    assert hits > 200 and spans > 50


def test_stop_window_named_cases():
    toks = [b"a", b"b", b"ab", b"", b"q" * 20, b"q" * 12, b"xaabx"]
    assert R.run_window(toks, [0, 0, 0, 1], [b"aab"]) == 3            # "aab" in "aaab"
    assert R.run_window(toks, [6], [b"aab"]) == 0                     # inside one token
    assert R.run_window(toks, [0, 3, 0, 3, 3, 1], [b"aab"]) == 5      # three tokens, empties between
    assert R.run_window(toks, [4, 5], [b"q" * 32]) == 1               # the longest stop string
    assert R.run_window(toks, [5, 5, 3], [b"q" * 32]) is None         # 24 bytes only
    assert R.run_window(toks, [5, 5, 5], [b"q" * 32]) == 2
    assert R.run_window(toks, [1, 1, 0], [b"a"]) == 2                 # one byte
    w = R.StopWindow([b"zz"])
    for i in (4, 5, 4):
        w.push(toks[i])
    assert len(w.tail) == R.TAIL_MAX
    before = w.tail
    assert w.push(b"") is False and w.tail == before                  # a special token


def test_control_state_ends_on_the_completing_token():
    toks = [b"a", b"b", b"", b"c"]
    st = R.ControlState(3, 4, 9, tok_bytes=toks, stop_seqs=[b"ab"], stop_ids=[3])
    script = [[0, 1, 0, 0], [0, 2, 1, 0], [0, 3, 1, 0]]
    for t in range(4):
        st.step(t, lambda tt: ([r[tt] for r in script], [0.0] * 3))
    assert st.sequences() == [[0, 1], [0, 2, 1], [0]]
    assert st.done == [1, 1, 1] and st.n_alive == 0
    assert [w.tail for w in st.win] == [b"ab", b"ab", b"a"]           # a stop ID leaves the window


# --- token bytes -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    return import_module(PKG_DIR + ".tokenizer")


def _bytes_of(tb, i):
    data, off = tb
    return data[off[i]:off[i + 1]]


@pytest.mark.parametrize("family,vocab", [("llama3", 0), ("gemma2", 2048)])
def test_char_tokenizer_token_bytes_are_exact(T, family, vocab):
    tok = T.CharTokenizer(family, vocab_size=vocab)
    tb = tok.token_bytes()
    assert len(tb[1]) == tok.vocab_size + 1 and tb[1][-1] == len(tb[0])
    assert tok.token_bytes() is tb                                     # built once
    for i in tok.special_ids.values():
        assert _bytes_of(tb, i) == b""
    rng = random.Random(3)
    plain = [i for i in range(tok.vocab_size) if i not in set(tok.special_ids.values())]
    multi = [tok.char_to_id[c] for c in ("é", "€", "’")] + [tok.vocab_size - 1]
    for _ in range(50):
        ids = [rng.choice(plain) for _ in range(rng.randint(1, 30))] + [rng.choice(multi)]
        rng.shuffle(ids)
        joined = b"".join(_bytes_of(tb, i) for i in ids)
        assert joined.decode("utf-8", errors="replace") == tok.decode(ids)
    assert len(_bytes_of(tb, tok.char_to_id["€"])) == 3


def test_bpe_fixture_token_bytes_are_exact(T):
    tok = T.BPETokenizer(os.path.join(REPO, "tests", "golden", "bpe_fixture"), "llama3")
    tb = tok.token_bytes()
    assert tb is not None          # the fixture is byte-level: losing its table loses the early stop
    assert len(tb[1]) == tok.vocab_size + 1
    added = set(tok.tk.get_added_tokens_decoder())
    assert all(_bytes_of(tb, i) == b"" for i in added)
    rng = random.Random(4)
    plain = [i for i in range(tok.n_table) if i not in added]
    texts = ["café €5 — naïve", "你好, world!\n\n  tabs\tand spaces  "]
    seqs = [tok.encode(t) for t in texts]
    seqs += [[rng.choice(plain) for _ in range(rng.randint(1, 40))] for _ in range(200)]
    for ids in seqs:
        joined = b"".join(_bytes_of(tb, i) for i in ids)
        assert joined.decode("utf-8", errors="replace") == tok.decode(ids), ids
    assert b"".join(_bytes_of(tb, i) for i in seqs[0]).decode("utf-8") == texts[0]


def test_a_tokenizer_that_is_not_byte_level_has_no_table(T, tmp_path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers

    words = ["<|begin_of_text|>", "<|eot_id|>", "<|end_of_text|>", "[UNK]", "fair", "share", "café"]
    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.add_special_tokens(words[:3])
    path = str(tmp_path / "tokenizer.json")
    tk.save(path)
    assert T.BPETokenizer(path, "llama3", use_config=False).token_bytes() is None   # no decoder
    tk.decoder = decoders.WordPiece()
    tk.save(path)
    assert T.BPETokenizer(path, "llama3", use_config=False).token_bytes() is None
    # a ByteLevel decoder over a vocabulary that is not spelled in its alphabet: "é" is, " " is not
    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words + ["a b"])}, unk_token="[UNK]"))
    tk.add_special_tokens(words[:3])
    tk.decoder = decoders.ByteLevel()
    tk.save(path)
    assert T.BPETokenizer(path, "llama3", use_config=False).token_bytes() is None


# --- runtime's host helpers --------------------------------------------------------------------

@pytest.fixture(scope="module")
def runtime():
    return import_module(PKG_DIR + ".runtime")


def test_early_stop_strings_keeps_only_what_the_device_can_test(runtime):
    f = runtime.early_stop_strings
    assert f(None) == [] and f(()) == [] and f("###") == [b"###"]
    assert f(("\n\n", "###", "", "###")) == [b"\n\n", b"###"]
    assert f(("café", "end")) == [b"end"]                         # ASCII only
    assert f(("x" * 33, "y" * 32)) == [b"y" * 32]
    assert len(f([chr(65 + i) * 2 for i in range(12)])) == 8
    # strings that can overlap each other in a text: none is used
    assert f(("ab", "xaby")) == [] and f(("bcd", "ab")) == [] and f(("\n", "\n\n")) == []
    assert f(("aa",)) == [b"aa"]                                       # itself is no rival


def _cut(text, terms):
    for term in terms:
        at = text.find(term)
        if at != -1:
            text = text[:at]
    return text


def test_stopping_early_never_changes_the_cut_text(runtime):
    """The caller's cut (utils.generate_text) on the whole text and on the text ended by the
    window rule at the first completed stop string agree, for whatever early_stop_strings
    lets through."""
    rng = random.Random(11)
    used = 0
    for case in range(3000):
        alphabet = "ab" if case % 3 else "abc"
        terms = tuple("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 3)))
                      for _ in range(rng.randint(1, 3)))
        stops = runtime.early_stop_strings(terms)
        if not stops:
            continue
        used += 1
        text = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 14)))
        tail, ended = b"", text
        for k, ch in enumerate(text):                                  # one character per token
            hit, tail = runtime.stop_window_push(tail, ch.encode(), stops)
            if hit:
                ended = text[:k + 1]
                break
        assert _cut(ended, terms) == _cut(text, terms), (terms, text)
    assert used > 300


def test_stop_window_push_is_the_restatement(runtime):
    rng = random.Random(2)
    for _ in range(300):
        toks, ids = _random_case(rng, b"ab#", 6, 40)
        stops = [bytes(rng.choice(b"ab#") for _ in range(rng.choice((1, 2, 4, 32)))) for _ in range(3)]
        w, tail = R.StopWindow(stops), b""
        for i in ids:
            hit, tail = runtime.stop_window_push(tail, toks[i], stops)
            assert hit == w.push(toks[i]) and tail == w.tail


def test_stop_token_table_pads_with_a_barrier(runtime, T):
    tok = T.CharTokenizer("llama3")
    table = runtime.stop_token_table(tok, tok.vocab_size + 5)
    assert len(table) == tok.vocab_size + 5
    assert table[tok.eos_id] == b"\xff" and table[-1] == b"\xff"
    assert table[tok.char_to_id["a"]] == b"a"
    assert runtime.stop_token_table(tok, tok.vocab_size + 5) is table


# --- the ABI text ------------------------------------------------------------------------------

def _prototype(text, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree():
    header = open(os.path.join(REPO, "include", "consensus_scoring.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib_src = open(os.path.join(REPO, PKG_DIR, "_lib.py")).read()
    for name in NEW:
        args = _prototype(header, name)
        assert f'"{name}"' in lib_src, f"{name} missing from _lib.EXPORTED"
        m = re.search(r"L\." + name + r"\.argtypes\s*=\s*\[(.*?)\]", lib_src, flags=re.S)
        assert m, f"{name} has no argtypes"
        bound = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert len(bound) == len(args), (name, len(bound), len(args))
        for b, a in zip(bound, args):
            assert (b == "vp") == ("*" in a or a.startswith("cs_stream_t")), (name, b, a)
    old = _prototype(header, "cs_sample_step")
    new = _prototype(header, "cs_sample_step_ex")
    assert len(old) == 25 and len(new) == 35 and set(old) <= set(new)
    assert set(_prototype(header, "cs_vocab_sample")) <= set(_prototype(header, "cs_vocab_sample_ex"))
