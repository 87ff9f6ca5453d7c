"""cs_dfa_token_masks, cs_vocab_sample_dfa and cs_sample_step_dfa (csrc/proposer.hip).

* The masks equal the NumPy rule of tests/constraint_ref.py bit for bit.
* The constrained draw is the EXISTING draw on the row whose forbidden tokens are -inf: the
  reference transforms the row outside the kernel under test (bias in fp32, the soft-cap by the
  library's own soft-cap as cs_vocab_topk returns it, the penalty by torch on the host, then
  -inf under every clear bit) and draws from it with ops.vocab_sample / the greedy
  ops.vocab_sample_ex without any control.  Ids, log-probabilities and states are compared
  exactly.
* With masks = None the entries are their *_ex siblings in every output array.
* A 40-step loop, eager and as one captured graph, follows the NumPy state machine step by
  step, for a bounded regex and for json_object(2).

Every comparison is exact."""
import json
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import constraint_ref as CR
from conftest import PKG_DIR
from test_sample_controls_gpu import DevX, i32, ragged_dev, rand_logits, seeds_for
from test_sample_step_gpu import SENT_LP, SENT_TOK

pytestmark = pytest.mark.gpu

C = import_module(PKG_DIR + ".constrain")
BOUNDED = r'\{"score": (10|[1-9]), "ok": (true|false)\}'
NEG_INF = float("-inf")


# --- helpers ----------------------------------------------------------------------------------

def dev_table(dev, tok_bytes):
    """(tok_bytes uint8, tok_off int32 [vocab + 1]) device tensors of a list of byte strings."""
    off = np.zeros(len(tok_bytes) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b) for b in tok_bytes])
    data = np.frombuffer(b"".join(tok_bytes) + b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)


def dev_dfa(dev, trans, accept):
    return (torch.from_numpy(np.ascontiguousarray(trans, dtype=np.int16).copy()).to(dev),
            torch.from_numpy(np.asarray(accept).astype(np.uint8)).to(dev))


def build_masks(ops, dev, trans, accept, tok_bytes, stop):
    tb, to = dev_table(dev, tok_bytes)
    t, a = dev_dfa(dev, trans, accept)
    return ops.dfa_token_masks(t, a, tb, to, i32(dev, stop) if len(stop) else None)


def as_u32(masks):
    return masks.cpu().numpy().view(np.uint32)


def bits_of(x):
    return x.detach().cpu().numpy().view(np.int32)


# --- the masks ----------------------------------------------------------------------------------

def random_vocab(rng, vocab, n_distinct=1500):
    """``vocab`` byte strings of 0 to 8 bytes over a small alphabet, drawn from a pool of
    distinct ones (the reference walks each distinct string once)."""
    pool = [bytes(rng.integers(97, 103, size=int(rng.integers(1, 9))).astype(np.uint8))
            for _ in range(n_distinct)] + [b"", b"a", b"f", b"abcdefab"]
    return [pool[k] for k in rng.integers(0, len(pool), size=vocab)]


def random_dfa(rng, n):
    """An arbitrary (untrimmed) table over bytes a..f: about a third of the arcs are dead."""
    trans = np.full((n, 256), -1, dtype=np.int16)
    arcs = rng.integers(0, n, size=(n, 6)).astype(np.int16)
    arcs[rng.random((n, 6)) < 0.33] = -1
    trans[:, 97:103] = arcs
    return trans, rng.random(n) < 0.4


@pytest.mark.parametrize("n_states", [1, 7, 1024])
@pytest.mark.parametrize("vocab", [33, 1000, 128256])
def test_token_masks_equal_the_numpy_rule(ops, dev, vocab, n_states):
    rng = np.random.default_rng(vocab + n_states)
    tok = random_vocab(rng, vocab)
    tok[0], tok[vocab - 1] = b"", b"ab"
    trans, accept = random_dfa(rng, n_states)
    accept[0] = True
    # stop ids: an empty token, the last id, an ordinary one, a duplicate
    stop = [0, vocab - 1, 17, 17]
    got = build_masks(ops, dev, trans, accept, tok, stop)
    want = CR.token_masks(trans, accept, tok, stop)
    assert tuple(got.shape) == want.shape == (n_states, (vocab + 31) // 32)
    assert np.array_equal(as_u32(got), want)
    if vocab % 32:
        assert (want[:, -1] >> (vocab % 32) == 0).all()                    # pad bits
    if n_states > 1:                                           # neither empty nor full
        on = sum(int(CR.allowed(want, q, vocab).sum()) for q in range(min(n_states, 7)))
        assert 0 < on < min(n_states, 7) * vocab
    if n_states * vocab < 10 ** 7:                             # and with no stop id at all
        none = build_masks(ops, dev, trans, accept, tok, [])
        assert np.array_equal(as_u32(none), CR.token_masks(trans, accept, tok, []))


@pytest.fixture(scope="module")
def tokenizers(pkg):
    import os
    T = import_module(pkg.__name__ + ".tokenizer")
    here = os.path.dirname(os.path.abspath(__file__))
    return {"char": T.CharTokenizer("llama3", vocab_size=512),
            "bpe": T.BPETokenizer(os.path.join(here, "golden", "bpe_fixture"), "llama3",
                                  vocab_size=4096)}


@pytest.mark.parametrize("which", ["char", "bpe"])
@pytest.mark.parametrize("spec", ["bounded", "json"])
def test_token_masks_on_the_tokenizers_own_tables(ops, dev, tokenizers, which, spec):
    tok = tokenizers[which]
    data, off = tok.token_bytes()
    table = [bytes(data[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    d = C.compile_regex(BOUNDED) if spec == "bounded" else C.json_object(2)
    stop = list(tok.eos_ids)
    got = build_masks(ops, dev, d.trans, d.accept, table, stop)
    want = CR.token_masks(d.trans, d.accept, table, stop)
    assert np.array_equal(as_u32(got), want)
    first = CR.allowed(want, d.start, len(table))
    assert first.any() and all(table[v].startswith(b"{") for v in np.flatnonzero(first))
    assert not any(first[s] for s in stop)


# --- the draw -----------------------------------------------------------------------------------

# the planted automaton: 0 general (a b c stay, d -> 1, e -> 2), 1 allows only "zq" (through 4),
# 2 allows nothing and does not accept, 3 accepts and allows nothing but the stop ids
def planted_dfa():
    trans = np.full((5, 256), -1, dtype=np.int16)
    trans[0, [97, 98, 99]] = 0
    trans[0, 100], trans[0, 101] = 1, 2
    trans[1, ord("z")], trans[4, ord("q")] = 4, 3
    return trans, np.asarray([False, False, False, True, False])


def planted_vocab(V):
    """a b c d e x x by id modulo 7 ("x" is dead everywhere); ONE is the only token that state 1
    allows; the stop ids spell "a", which state 0 would allow by its bytes."""
    tok = [b"abcdexx"[v % 7:v % 7 + 1] for v in range(V)]
    one, stops = V - 3, [V - 2, 40]
    tok[one] = b"zq"
    tok[9], tok[V - 1] = b"", b"aab"                                       # special, multi-byte
    for s in stops:
        tok[s] = b"a"
    return tok, one, stops


def device_softcap(ops, rows, cap):
    """softcap(rows) with the library's own bits: cs_vocab_topk with k = the row width returns
    every soft-capped value of 256-wide rows, which are scattered back to their places."""
    flat = rows.reshape(-1)
    pad = (-flat.numel()) % 256
    m = torch.cat([flat, flat.new_zeros(pad)]).view(-1, 256).contiguous()
    ids, vals = ops.vocab_topk(m, 256, softcap=cap)
    out = torch.empty_like(m)
    out.scatter_(1, ids.long(), vals)
    return out.reshape(-1)[:flat.numel()].view_as(rows)


def reference_rows(ops, dev, lg, allow, *, bias=(), bias_value=0.0, cap=0.0, seen=None, penalty=1.0):
    """The transformed fp32 rows with -inf under every clear bit (allow: bool [S, V])."""
    rows = torch.nan_to_num(lg.float(), nan=0.0).cpu()      # a NaN sits under a clear bit only
    V = rows.shape[1]
    keep = sorted({int(i) for i in bias if 0 <= int(i) < V})
    if keep:
        rows[:, keep] = rows[:, keep] + torch.tensor(bias_value, dtype=torch.float32)
    if cap > 0.0:
        rows = device_softcap(ops, rows.to(dev), cap).cpu()
    if penalty != 1.0:
        p = torch.tensor(penalty, dtype=torch.float32)
        for r, ids in enumerate(seen):
            idx = sorted({int(i) for i in ids if 0 <= int(i) < V})
            if idx:
                x = rows[r, idx]
                rows[r, idx] = torch.where(x < 0, x * p, x / p)
    rows[~torch.from_numpy(allow)] = NEG_INF
    return rows.to(dev)


def reference_draw(ops, rows, seeds, T):
    if T == 0.0:
        return ops.vocab_sample_ex(rows, None, temperature=0.0, n_draw=seeds.shape[1])
    return ops.vocab_sample(rows, seeds, temperature=T)


class DevD(DevX):
    """DevX calling ops.sample_step_dfa with the automaton's tensors."""

    def __init__(self, ops, dev, S, max_tokens, pad, base, *, masks, trans, states, **kw):
        super().__init__(ops, dev, S, max_tokens, pad, base, **kw)
        self.masks, self.trans = masks, trans
        self.dfa_state = i32(dev, states)

    def call(self, logits, **over):
        kw = dict(self.kw, bias_ids=self.bias, stop_ids=self.stop, out_lp=self.out_lp,
                  workspace=self.ws, repetition_penalty=self.penalty, seen_ids=self.seen_ids,
                  seen_off=self.seen_off, stop_seqs=self.stop_seqs, tok_bytes=self.tok_bytes,
                  tok_off=self.tok_off, tail=self.tail, tail_len=self.tail_len, masks=self.masks,
                  trans=self.trans, dfa_state=self.dfa_state)
        kw.update(over)
        self.ops.sample_step_dfa(logits, self.base, self.step, self.done, self.out_len,
                                 self.out_tokens, self.next_tok, self.n_alive, **kw)

    def snapshot(self):
        snap = super().snapshot()
        snap["dfa_state"] = self.dfa_state.tolist()
        return snap


CONTROLS = [(cap, T, biased, penalty) for cap in (0.0, 30.0) for T in (0.0, 0.7)
            for biased in (False, True) for penalty in (1.0, 1.3)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [1000, 256000])
def test_constrained_draw_is_the_existing_draw_on_the_masked_row(ops, dev, V, dtype):
    trans, accept = planted_dfa()
    tok, one, stops = planted_vocab(V)
    masks = build_masks(ops, dev, trans, accept, tok, stops)
    want_masks = CR.token_masks(trans, accept, tok, stops)
    assert np.array_equal(as_u32(masks), want_masks)
    states = [0, 1, 2, 3, 0, 0]
    S = len(states)
    allow = np.stack([CR.allowed(want_masks, q, V) for q in states])
    assert allow[1].sum() == 1 and allow[1][one] and not allow[2].any()
    assert sorted(np.flatnonzero(allow[3])) == sorted(stops)
    lg = rand_logits(S, V, dtype, dev, seed=V % 97)
    lg[4, stops[0]] = 60.0                    # a stop id leads where the text cannot end
    lg[5, 6] = float("nan")                   # "x": a NaN under a clear bit poisons nothing
    lg[0, 13] = 55.0                          # another "x", far ahead, never drawn
    assert not allow[5][6] and not allow[0][13]
    trans_t, _ = dev_dfa(dev, trans, accept)
    tb, to = dev_table(dev, tok)
    states_t = i32(dev, states)
    base = [101 + s for s in range(S)]
    seeds = torch.cat([seeds_for(dev, base, 0), seeds_for(dev, base, 5)], dim=1)
    allowed_tok, forbidden_tok = 0, 20        # "a" in state 0; "x"
    assert allow[0][allowed_tok] and not allow[0][forbidden_tok]
    seen = [[allowed_tok, 1, 13, forbidden_tok, one, V + 4], [one], [], [stops[0]], [2, 3], [7]]
    sid, soff = ragged_dev(dev, seen)
    for cap, T, biased, penalty in CONTROLS:
        what = f"cap {cap} T {T} bias {biased} penalty {penalty}"
        bias = [allowed_tok, forbidden_tok, forbidden_tok] if biased else []
        kw = dict(temperature=T, softcap=cap, bias_ids=i32(dev, bias) if bias else None,
                  bias_value=6.0, repetition_penalty=penalty, seen_ids=sid, seen_off=soff)
        rows = reference_rows(ops, dev, lg, allow, bias=bias, bias_value=6.0, cap=cap, seen=seen,
                              penalty=penalty)
        want_ids, want_lp = reference_draw(ops, rows, seeds, T)
        ids, lp = ops.vocab_sample_dfa(lg, None if T == 0.0 else seeds, n_draw=2, masks=masks,
                                       dfa_state=states_t, **kw)
        assert torch.equal(ids, want_ids), what
        assert np.array_equal(bits_of(lp), bits_of(want_lp)), what
        got = ids.tolist()
        assert got[1] == [one, one] and got[2] == [-1, -1], what
        assert all(v in stops for v in got[3]) and all(v not in stops for v in got[4]), what
        assert all(allow[r][v] for r in (0, 4, 5) for v in got[r]), what
        assert torch.isfinite(lp[[0, 1, 3, 4, 5]]).all() and torch.isnan(lp[2]).all(), what
        # one call of the step entry: the same draw (column 0), then the state machine
        d = DevD(ops, dev, S, 3, 9, base, masks=masks, trans=trans_t, states=states, stop=stops,
                 bias=bias, bias_value=6.0, temperature=T, softcap=cap, penalty=penalty, seen=seen,
                 tok_bytes=tok)
        ref = CR.DfaState(S, 3, 9, trans=trans, starts=states, tok_bytes=tok, stop_ids=stops,
                          sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
        d.call(lg)
        ref.step(0, lambda t: (want_ids[:, 0].tolist(), want_lp[:, 0].tolist()))
        snap = d.snapshot()
        for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "dfa_state"):
            assert snap[k] == getattr(ref, k), (what, k)
        assert np.array_equal(snap["out_lp"].view(np.int32),
                              np.asarray(ref.out_lp, dtype=np.float32).view(np.int32)), what
        assert snap["done"][1:4] == [0, 1, 1] and snap["out_len"][1:4] == [1, 0, 0], what
        assert snap["dfa_state"][1:4] == [3, 2, 3] and snap["done"][4] == 0, what


# --- masks = None ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_without_masks_the_entries_are_their_ex_siblings(ops, dev, dtype):
    S, V = 3, 8269
    lg = rand_logits(S, V, dtype, dev, seed=4)
    tok = [bytes([97 + v % 3]) for v in range(V)]
    seen = [[1, 2, 3], [], [V - 1]]
    sid, soff = ragged_dev(dev, seen)
    seeds = seeds_for(dev, [5, 6, 7], 0)
    for T, cap, pen in ((0.0, 0.0, 1.0), (0.7, 30.0, 1.3), (1.0, 0.0, 1.0)):
        kw = dict(temperature=T, softcap=cap, bias_ids=i32(dev, [4, 9]), bias_value=-2.0,
                  repetition_penalty=pen, seen_ids=sid, seen_off=soff)
        a = ops.vocab_sample_ex(lg, seeds, **kw)
        b = ops.vocab_sample_dfa(lg, seeds, masks=None, **kw)
        assert torch.equal(a[0], b[0]) and np.array_equal(bits_of(a[1]), bits_of(b[1]))
        mk = dict(stop=[17], bias=[4, 9], bias_value=-2.0, temperature=T, softcap=cap, penalty=pen,
                  seen=seen, stop_seqs=[b"cc", b"abca"], tok_bytes=tok)
        old = DevX(ops, dev, S, 6, 1, [5, 6, 7], **mk)
        new = DevD(ops, dev, S, 6, 1, [5, 6, 7], masks=None, trans=None, states=[0, 0, 0], **mk)
        for _ in range(6):
            old.call(lg)
            new.call(lg)
            old.step += 1
            new.step += 1
        so, sn = old.snapshot(), new.snapshot()
        for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "step", "tail",
                  "tail_len"):
            assert so[k] == sn[k], (T, k)
        assert np.array_equal(so["out_lp"].view(np.int32), sn["out_lp"].view(np.int32))
        assert sn["dfa_state"] == [0, 0, 0]                                # never written


# --- the 40-step loop -----------------------------------------------------------------------------

STRUCT = [b'{"', b'": ', b'", "', b'"}', b'"', b"}", b"{", b": ", b", ", b":", b",", b"true",
          b"false", b"null", b"score", b"ok", b"10", b" ", b"\n", b"[", b"]", b'\\"', b"\\u00e9",
          "é".encode(), "€".encode(), b"1.5e3", b"-0"]


def loop_vocab():
    """301 tokens: specials without bytes, printable ASCII one by one, JSON pieces, letters."""
    tok = [b"", b""] + [bytes([c]) for c in range(0x20, 0x7F)] + STRUCT
    tok += [bytes([97 + k % 26, 97 + (k // 26) % 26]) for k in range(301 - len(tok))]
    assert len(tok) == 301
    return tok, [0]                                        # token 0 is the end-of-text id


def loop_logits(dev, tok, S, bonus):
    g = torch.Generator().manual_seed(77)
    lg = torch.randn(S, len(tok), generator=g) * 2.0
    closing = [v for v, b in enumerate(tok) if b in (b'"', b"}", b'"}', b'": ', b":", b"1", b"true")]
    lg[:, closing] += bonus
    return lg.to(torch.bfloat16).to(dev)


def run_loop(ops, dev, d, steps, max_tokens, bonus):
    """The NumPy state machine driven by the existing draw on masked rows, and the device
    eager, compared after every step -> (reference, per-step snapshots, what a graph needs)."""
    tok, stops = loop_vocab()
    S = 8
    masks = build_masks(ops, dev, d.trans, d.accept, tok, stops)
    want_masks = CR.token_masks(d.trans, d.accept, tok, stops)
    assert np.array_equal(as_u32(masks), want_masks)
    trans_t, _ = dev_dfa(dev, d.trans, d.accept)
    lg = loop_logits(dev, tok, S, bonus)
    base = [1000 + 7 * s for s in range(S)]
    mk = lambda: DevD(ops, dev, S, max_tokens, 1, base, masks=masks, trans=trans_t,
                      states=[d.start] * S, stop=stops, temperature=0.8, tok_bytes=tok)
    ref = CR.DfaState(S, max_tokens, 1, trans=d.trans, starts=[d.start] * S, tok_bytes=tok,
                      stop_ids=stops, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    eager, snaps = mk(), []
    for t in range(steps):
        allow = np.stack([CR.allowed(want_masks, q, len(tok)) for q in ref.dfa_state])
        rows = reference_rows(ops, dev, lg, allow)

        def draw(tt):
            ids, lp = ops.vocab_sample(rows, seeds_for(dev, base, tt), temperature=0.8)
            return ids[:, 0].tolist(), lp[:, 0].tolist()

        eager.call(lg)
        ref.step(t, draw)
        snap = eager.snapshot()
        for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "dfa_state"):
            assert snap[k] == getattr(ref, k), (t, k)
        snaps.append(snap)
        eager.step += 1
    # one captured step, replayed: step 0 eager, then 39 replays
    g = mk()
    g.ws = eager.ws
    g.call(lg)
    g.step += 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.call(lg)
        g.step += 1
    for t in range(1, steps):
        graph.replay()
        snap = g.snapshot()
        for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "dfa_state"):
            assert snap[k] == snaps[t][k], (t, k)
        assert np.array_equal(snap["out_lp"].view(np.int32), snaps[t]["out_lp"].view(np.int32))
    texts = [b"".join(tok[v] for v in seq) for seq in ref.sequences()]
    return ref, texts


def test_forty_steps_under_a_bounded_regex(ops, dev):
    d = C.compile_regex(BOUNDED)
    ref, texts = run_loop(ops, dev, d, steps=40, max_tokens=40, bonus=0.0)
    # every path of the pattern ends within 27 tokens, so every stream ended by a stop id
    assert ref.done == [1] * 8 and all(n < 40 for n in ref.out_len)
    for s, text in enumerate(texts):
        assert d.accept[ref.dfa_state[s]] and re.fullmatch(BOUNDED, text.decode()), text
    assert len(set(texts)) > 1


def test_forty_steps_under_the_json_automaton(ops, dev):
    d = C.json_object(2)
    ref, texts = run_loop(ops, dev, d, steps=40, max_tokens=40, bonus=4.5)
    finished = [s for s in range(8) if ref.out_len[s] < 40]
    print(f"json loop: {len(finished)} of 8 streams ended by a stop id, lengths {ref.out_len}")
    assert ref.done == [1] * 8
    assert len(finished) >= 4                              # stated on the reference alone
    for s in range(8):
        if s in finished:
            assert isinstance(json.loads(texts[s].decode("utf-8")), dict), texts[s]
        else:                                              # cut at max_tokens: a live prefix
            assert d.walk(d.start, texts[s]) == ref.dfa_state[s] >= 0


# --- argument checks ------------------------------------------------------------------------------

def test_bad_automaton_arguments_return_a_status_and_launch_nothing(ops, pkg, dev):
    CSError = pkg.CSError
    trans, accept = planted_dfa()
    V = 1000
    tok, one, stops = planted_vocab(V)
    masks = build_masks(ops, dev, trans, accept, tok, stops)
    trans_t, accept_t = dev_dfa(dev, trans, accept)
    lg = rand_logits(2, V, torch.float32, dev, seed=1)
    seeds = seeds_for(dev, [1, 2], 0)
    st = i32(dev, [0, 0])
    plain = [dict(n_states=0), dict(n_states=1025), dict(masks=masks[:, :-1].contiguous()),
             dict(dfa_state=None)]
    for over in plain:
        kw = dict(masks=masks, dfa_state=st)
        kw.update(over)
        with pytest.raises(CSError, match="cs_vocab_sample_dfa"):
            ops.vocab_sample_dfa(lg, seeds, **kw)
    d = DevD(ops, dev, 2, 3, 9, [1, 2], masks=masks, trans=trans_t, states=[0, 0], stop=stops,
             tok_bytes=tok)
    before = d.snapshot()
    for over in plain + [dict(trans=None), dict(tok_bytes=None), dict(tok_off=None)]:
        with pytest.raises(CSError, match="cs_sample_step_dfa"):
            d.call(lg, **over)
    after = d.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    d.call(lg)                                             # and the workspace is still good
    assert d.snapshot()["out_len"] == [1, 1]
    tb, to = dev_table(dev, tok)
    with pytest.raises(CSError, match="cs_dfa_token_masks"):
        ops.dfa_token_masks(torch.zeros(1025, 256, dtype=torch.int16, device=dev),
                            torch.zeros(1025, dtype=torch.uint8, device=dev), tb, to)
    with pytest.raises(CSError, match="n_stop"):
        ops.dfa_token_masks(trans_t, accept_t, tb, to, i32(dev, range(17)))
