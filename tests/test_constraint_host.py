"""constrain.py on the CPU: compile_regex against Python's ``re``, json_object against
``json.loads``, the limits, ``union`` and the token-mask rule of tests/constraint_ref.py.

The shorthands \\d \\w \\s are ASCII in the subset (documented in constrain.py), so a pattern
that uses one is compared with ``re.fullmatch(p, s, re.ASCII)``; every other pattern with
plain ``re.fullmatch(p, s)``.  A byte string that is not well-formed UTF-8 is no text at all
and must be rejected by every automaton."""
import json
import random
import re
from importlib import import_module

import numpy as np
import pytest

import constraint_ref as CR
from conftest import PKG_DIR

C = import_module(PKG_DIR + ".constrain")
CSError = import_module(PKG_DIR + "._lib").CSError

BOUNDED = r'\{"score": (10|[1-9]), "ok": (true|false)\}'
PATTERNS = [
    r"abc",
    r"",
    r"a|b|cd",
    r"(ab)*c+",
    r"(?:ab|c)?d",
    r"a?b?c?",
    r"[a-c]{2,3}",
    r"[abc]{2}",
    r"x{2,}y",
    r"a{,2}b",
    r"a{0}b",
    r".",
    r".*",
    r"a.c",
    r"[^a]",
    r"[^a-y]+",
    r'"[^"\\]*"',
    r"[]a]+",
    r"[a\-z]+",
    r"[-a]b",
    r"\d+\.\d*",
    r"\w+@\w+",
    r"a\sb\s*c",
    r"\D\W\S",
    r"[\d_a-f]+",
    r"\.\*\+\?\(\)\[\]\{\}\|\\",
    r"a{b",
    r"\n\t\r\x41\u00e9\U0001F600",
    r"é+|ü",
    r"[α-ω]+",
    r"[^é€]x",
    r"(a|b)*abb",
    r"<answer>[^<]{0,4}<sep>[A-D]( (>|=) [A-D])*</answer>",
    BOUNDED,
]
USES_SHORTHAND = re.compile(r"\\[dwsDWS]")
ALPHABET = "abcdxyz.*+01 9_@\n\t\"\\<>=/{}[]()|-AD,:stepanwrouflk" + "éüαω€😀\x7f\x1c\xa0٣"


def py_match(p, data: bytes) -> bool:
    try:
        s = data.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return re.fullmatch(p, s, re.ASCII if USES_SHORTHAND.search(p) else 0) is not None


def dist_to_accept(d):
    """Per state: the fewest bytes to an accepting state (every state has one: trimmed)."""
    n = d.n_states
    dist = np.where(d.accept, 0, n + 1)
    for _ in range(n):
        succ = np.concatenate([dist, [n + 1]])[d.trans.astype(np.int64)]
        new = np.minimum(dist, succ.min(axis=1) + 1)
        if (new == dist).all():
            break
        dist = new
    assert (dist <= n).all(), "a state that cannot reach an accepting one"
    return dist


def random_walk(d, rng, dist, wander: int, start=None, max_len=400) -> bytes:
    """Bytes of a walk that wanders for about ``wander`` steps, then heads for an accepting
    state; it may also stop early in one."""
    q, out = d.start if start is None else start, bytearray()
    while len(out) < max_len:
        if d.accept[q] and (len(out) >= wander or rng.random() < 0.2):
            break
        live = np.flatnonzero(d.trans[q] >= 0)
        if len(live) == 0:
            break
        if len(out) >= wander:
            live = [b for b in live if dist[d.trans[q, b]] < dist[q]]
        b = int(rng.choice(list(live)))
        out.append(b)
        q = int(d.trans[q, b])
    return bytes(out)


@pytest.mark.parametrize("p", PATTERNS)
def test_compile_regex_agrees_with_re(p):
    d = C.compile_regex(p)
    assert d.trans.dtype == np.int16 and d.trans.shape == (d.n_states, 256)
    assert d.accept.dtype == bool and d.n_states <= 1024
    dist = dist_to_accept(d)                                  # trimmed
    rng = random.Random(len(p) * 7919 + sum(map(ord, p)))
    cases = []
    for _ in range(150):                                      # random texts and random bytes
        cases.append("".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 8))).encode())
        cases.append(bytes(rng.randrange(256) for _ in range(rng.randint(1, 5))))
    accepted = []
    for _ in range(120):                                      # walks of the automaton
        w = random_walk(d, rng, dist, rng.randint(0, 12))
        cases.append(w)
        if d.accepts(w):
            accepted.append(w)
        cases.append(w[:rng.randint(0, len(w))])
    assert accepted, "no accepted walk"
    for w in accepted[:60]:                                   # one-byte mutations
        if w:
            k = rng.randrange(len(w))
            cases.append(w[:k] + bytes([rng.randrange(256)]) + w[k + 1:])
            cases.append(w[:k] + w[k + 1:])
        cases.append(w + bytes([rng.choice(w or b"a")]))
    n_yes = 0
    for data in cases:
        want = py_match(p, data)
        n_yes += want
        assert d.accepts(data) == want, (p, data)
    assert n_yes >= len(accepted)
    # minimal: no two states agree on accept and on every successor
    sig = np.concatenate([d.accept[:, None].astype(np.int16), d.trans], axis=1)
    assert len(np.unique(sig, axis=0)) == d.n_states


def test_walk_and_accepts():
    d = C.compile_regex(r"ab+")
    q = d.walk(d.start, b"ab")
    assert q >= 0 and d.accept[q] and d.walk(q, b"bb") == q
    assert d.walk(d.start, b"b") == -1 and d.walk(d.start, b"ba") == -1
    assert d.walk(d.start, b"") == d.start and not d.accepts(b"") and d.accepts(b"abbb")


@pytest.mark.parametrize("p,what", [
    (r"^a", "anchor"), (r"a$", "anchor"), (r"\bword", "anchor"), (r"a\B", "anchor"),
    (r"\Aa", "anchor"), (r"a\Z", "anchor"),
    (r"(a)\1", "backreference"), (r"(?P<n>a)(?P=n)", "named group"),
    (r"(?=a)a", "lookaround"), (r"(?!a)b", "lookaround"), (r"(?<=a)b", "lookaround"),
    (r"(?<!a)b", "lookaround"),
    (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a??", "lazy"), (r"a{1,2}?", "lazy"),
    (r"a*+", "possessive"), (r"(?i)a", "flags"), (r"[\D]", "negated shorthand"),
    (r"[[:alpha:]]", "POSIX"), (r"\p", "escape"), (r"a**", "multiple repeat"),
    (r"(a", "parenthesis"), (r"a)", "parenthesis"), (r"[a", "unterminated"), (r"*a", "repeat"),
    (r"a{3,2}", "n < m"), (r"[z-a]", "reversed"), ("a\\", "backslash"),
])
def test_unsupported_constructs_raise(p, what):
    with pytest.raises(ValueError, match=what):
        C.compile_regex(p)


def test_empty_language_raises():
    with pytest.raises(ValueError, match="matches nothing"):
        C.compile_regex(r"[^\x00-\U0010FFFF]")


def test_state_limit():
    d = C.compile_regex(r"a{1023}")
    assert d.n_states == 1024 and d.accepts(b"a" * 1023) and not d.accepts(b"a" * 1022)
    with pytest.raises(CSError, match="1025"):
        C.compile_regex(r"a{1024}")
    with pytest.raises(CSError):
        C.Dfa(np.full((1025, 256), -1, dtype=np.int16), np.ones(1025, dtype=bool), 0)


# --- JSON ---------------------------------------------------------------------------------

def rand_value(rng, depth):
    """A random JSON value nesting ``depth`` more container levels at the most."""
    kinds = ["str", "int", "float", "lit"] + (["obj", "arr"] * 2 if depth > 0 else [])
    k = rng.choice(kinds)
    if k == "str":
        return "".join(rng.choice('ab "\\/\n\t\x08é€😀{}[],:') for _ in range(rng.randint(0, 5)))
    if k == "int":
        return rng.choice([0, -0, 7, -12, 10 ** 12, -305])
    if k == "float":
        return rng.choice([0.5, -2.25, 1e-7, 3.0e20, -1.5e-9, 100.0])
    if k == "lit":
        return rng.choice([True, False, None])
    if k == "arr":
        return [rand_value(rng, depth - 1) for _ in range(rng.randint(0, 3))]
    return rand_object(rng, depth - 1)


def rand_object(rng, depth):
    return {"k%d" % i + rng.choice(["", " é", '"']): rand_value(rng, depth)
            for i in range(rng.randint(0, 3))}


def nested(levels):
    """An object whose innermost value sits ``levels`` levels deep, through arrays and objects."""
    v = 1
    for k in range(levels - 1):
        v = [v] if k % 2 == 0 else {"a": v}
    return {"a": v}


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_json_object_accepts_what_json_dumps_writes(max_depth):
    d = C.json_object(max_depth)
    assert d.n_states <= 1024
    rng = random.Random(max_depth)
    for _ in range(150):
        obj = rand_object(rng, max_depth - 1)
        for kw in (dict(separators=(",", ":")), dict(), dict(ensure_ascii=False),
                   dict(separators=(", ", ": "))):
            text = json.dumps(obj, **kw)
            assert d.accepts(text.encode("utf-8")), text
    assert d.accepts(json.dumps(nested(max_depth)).encode())
    assert not d.accepts(json.dumps(nested(max_depth + 1)).encode())
    assert d.accepts(b'{ \n"a"\n\n:  1 ,\n "b" : [ ]}') == (max_depth >= 2)
    assert d.accepts(b'{"a": -0.0e+10, "b": 1E5, "c": "\\u00e9\\n"}')


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_json_object_walks_parse_to_dicts(max_depth):
    d = C.json_object(max_depth)
    dist = dist_to_accept(d)
    rng = random.Random(100 + max_depth)
    n = 0
    for _ in range(300):
        w = random_walk(d, rng, dist, rng.randint(0, 60))
        if d.accepts(w):
            n += 1
            assert isinstance(json.loads(w.decode("utf-8")), dict), w
    assert n >= 250


@pytest.mark.parametrize("text", [
    b'[1]', b'[]', b'"a"', b'1', b'', b' {}', b'{} ', b'{}{}',
    b'{"a":1,}', b'{"a":[1,]}', b'{,}', b'{"a"}', b'{"a":}', b'{a:1}', b"{'a':1}",
    b'{"a":"\x01"}', b'{"a":"\n"}', b'{"a":"\x7f"}', b'{"a":"\\x41"}', b'{"a":"\\u12g4"}',
    b'{"a":   1}', b'{   }', b'{"a":1   }', b'{"a":\t1}', b'{"a":\r1}',
    b'{"a":01}', b'{"a":1.}', b'{"a":.5}', b'{"a":+1}', b'{"a":1e}', b'{"a":-}', b'{"a":0x1}',
    b'{"a":tru}', b'{"a":True}', b'{"a":nul}', b'{"a":NaN}',
    b'{"a":"\xc3"}', b'{"a":"\xc0\x80"}', b'{"a":"\xed\xa0\x80"}', b'{"a":"\xf4\x90\x80\x80"}',
    b'{"a":"\xe9"}',
])
def test_json_object_rejects(text):
    for k in (1, 2, 3):
        assert not C.json_object(k).accepts(text), (k, text)


def test_json_object_depth_argument():
    for bad in (0, 4):
        with pytest.raises(ValueError):
            C.json_object(bad)
    # the judges' objects are depth 2
    d = C.json_object()
    assert d.accepts(b'{"score": 7, "reasoning": "ok"}')
    assert d.accepts(b'{"ranking": [2, 1, 3], "method_ranking": {"a": 1}, "reasoning": "x"}')
    assert not d.accepts(b'{"ranking": [[2], 1]}')


# --- union ----------------------------------------------------------------------------------

def test_union_keeps_the_languages_apart():
    pats = [r"ab*", r"(true|false)", BOUNDED, r"ab*"]
    dfas = [C.compile_regex(p) for p in pats]
    u, starts = C.union(dfas)
    assert len(starts) == 4 and starts[0] == starts[3] == u.start       # equal automata share
    assert u.n_states == sum(d.n_states for d in dfas[:3])
    dist_to_accept(u)
    rng = random.Random(5)
    texts = [random_walk(d, rng, dist_to_accept(d), rng.randint(0, 6)) for d in dfas
             for _ in range(30)]
    texts += [b"", b"a", b"tru", b"abtrue"]
    for k, d in enumerate(dfas):
        for t in texts:
            q = u.walk(starts[k], t)
            assert (q >= 0 and bool(u.accept[q])) == d.accepts(t), (k, t)
            assert (q >= 0) == (d.walk(d.start, t) >= 0)
    big = C.compile_regex(r"a{600}")
    with pytest.raises(CSError, match="limit"):
        C.union([big, C.compile_regex(r"b{600}")])
    with pytest.raises(ValueError):
        C.union([])


# --- the mask rule --------------------------------------------------------------------------

def test_token_mask_rule_on_a_hand_made_vocabulary():
    d = C.compile_regex(r'ab*(cd)?"?')
    tok = [b"", b"a", b"b", b"ab", b"abbbbbbc", b"c", b"d", b"cd", b'"', b"bb", b"", b"x",
           b"<eos>", b"bbbbbbbb", b"dc", b"abcd"] + [b"b"] * 20 + [b"a"]
    vocab, stop = len(tok), [12, 10]
    assert vocab == 37                                         # a partial second word
    m = CR.token_masks(d.trans, d.accept, tok, stop)
    assert m.dtype == np.uint32 and m.shape == (d.n_states, 2)
    q_a = d.walk(d.start, b"a")
    q_c = d.walk(d.start, b"ac")
    q_end = d.walk(d.start, b'ab"')
    start = CR.allowed(m, d.start, vocab)
    assert np.flatnonzero(start).tolist() == [1, 3, 4, 15, 36]           # "a..." only
    assert not start[0] and not start[10] and not start[12]   # empty, empty stop id, stop id
    after_a = CR.allowed(m, q_a, vocab)
    assert after_a[2] and after_a[9] and after_a[13] and after_a[5] and after_a[7] and after_a[8]
    assert after_a[12] and after_a[10]                         # accepting: the stop ids are on
    assert not after_a[1] and not after_a[6] and not after_a[14] and not after_a[11]
    assert CR.allowed(m, q_c, vocab)[6] and not CR.allowed(m, d.start, vocab)[6]   # "d"
    assert not CR.allowed(m, q_c, vocab)[12]                   # not accepting: no stop id
    assert np.flatnonzero(CR.allowed(m, q_end, vocab)).tolist() == [10, 12]
    assert (m[:, 1] >> 5 == 0).all()                           # pad bits
    assert not CR.allowed(m, -1, vocab).any() and not CR.allowed(m, d.n_states, vocab).any()
    # the rule agrees with the automaton token by token
    for q in range(d.n_states):
        for v, data in enumerate(tok):
            want = bool(d.accept[q]) if v in stop else (len(data) > 0 and d.walk(q, data) >= 0)
            assert bool(CR.allowed(m, q, vocab)[v]) == want
