"""cs_vocab_sample_ex and cs_sample_step_ex (csrc/proposer.hip): the two identities of their
contract bit for bit, the repetition penalty against ops.vocab_sample on rows penalised on
the host, greedy against numpy's argmax, the stop-string window against the restatement of
tests/sample_controls_ref.py after every step, graph replay, one real-width vocabulary and
the argument checks.

V_SPLIT is cut into two slices at every row count used here ([0, 5120) and [5120, 8269):
test_split_vocabulary_is_split reads the count back), and is no multiple of 32, so the last
bitmap word of the second slice is partial."""
from importlib import import_module

import numpy as np
import pytest
import torch

import sample_controls_ref as R
from sample_step_ref import as_i64, seed_of, vocab_sample_draw
from test_sample_step_gpu import SENT_LP, SENT_TOK, Dev, assert_same, n_splits, planted
from test_sampler_gpu import LP_TOL

pytestmark = pytest.mark.gpu

V_SMALL, V_SPLIT, SLICE = 64, 8269, 5120
DTYPES = [torch.float32, torch.bfloat16]


def i32(dev, xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int32, device=dev)


def ragged_dev(dev, lists):
    flat, off = R.ragged(lists)
    # one spare element keeps the (possibly empty) id tensor's pointer non-NULL
    return torch.from_numpy(np.append(flat, 0).astype(np.int32)).to(dev)[:len(flat)], \
        torch.from_numpy(off).to(dev)


def seeds_for(dev, base, t):
    return torch.tensor([[as_i64(seed_of(b, t))] for b in base], dtype=torch.int64, device=dev)


def rand_logits(S, V, dtype, dev, seed, ld=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S, ld or V, generator=g) * 3.0).to(dtype).to(dev)


class DevX(Dev):
    """Dev of test_sample_step_gpu.py calling ops.sample_step_ex, with the extra state."""

    def __init__(self, ops, dev, S, max_tokens, pad, base, *, penalty=1.0, seen=None,
                 stop_seqs=(), tok_bytes=None, **kw):
        super().__init__(ops, dev, S, max_tokens, pad, base, **kw)
        self.penalty, self.stop_seqs = penalty, list(stop_seqs)
        self.seen_ids, self.seen_off = (None, None) if seen is None else ragged_dev(dev, seen)
        self.tail = torch.zeros(S, 32, dtype=torch.uint8, device=dev)
        self.tail_len = torch.zeros(S, dtype=torch.int32, device=dev)
        self.tok_bytes = self.tok_off = None
        if tok_bytes is not None:
            off = np.zeros(len(tok_bytes) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(b) for b in tok_bytes])
            self.tok_off = torch.from_numpy(off).to(dev)
            self.tok_bytes = torch.tensor(list(b"".join(tok_bytes)) + [0], dtype=torch.uint8,
                                          device=dev)

    def call(self, logits, **over):
        kw = dict(self.kw, bias_ids=self.bias, stop_ids=self.stop, out_lp=self.out_lp,
                  workspace=self.ws, repetition_penalty=self.penalty, seen_ids=self.seen_ids,
                  seen_off=self.seen_off, stop_seqs=self.stop_seqs, tok_bytes=self.tok_bytes,
                  tok_off=self.tok_off, tail=self.tail, tail_len=self.tail_len)
        kw.update(over)
        self.ops.sample_step_ex(logits, self.base, self.step, self.done, self.out_len,
                                self.out_tokens, self.next_tok, self.n_alive, **kw)

    def snapshot(self):
        snap = super().snapshot()
        snap["tail"] = self.tail.tolist()
        snap["tail_len"] = self.tail_len.tolist()
        return snap


def test_split_vocabulary_is_split(pkg):
    assert [n_splits(pkg, S, V_SPLIT) for S in (1, 3, 5)] == [2, 2, 2]
    assert [n_splits(pkg, S, V_SMALL) for S in (1, 5)] == [1, 1]


# --- identity 1: off means old --------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(1, V_SMALL), (5, V_SMALL), (3, V_SPLIT)])
def test_plain_entry_with_every_control_off_is_vocab_sample(ops, dev, S, V, dtype):
    lg = rand_logits(S, V, dtype, dev, seed=S + V)
    g = torch.Generator().manual_seed(1)
    seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (S, 3), generator=g, dtype=torch.int64).to(dev)
    seen_ids, seen_off = ragged_dev(dev, [[1, 2, 3]] * S)
    for cap, T in ((0.0, 1.0), (30.0, 0.7)):
        want = ops.vocab_sample(lg, seeds, temperature=T, softcap=cap)
        for kw in (dict(), dict(repetition_penalty=1.0, seen_ids=seen_ids, seen_off=seen_off),
                   dict(repetition_penalty=1.3)):            # a penalty with no list: off
            got = ops.vocab_sample_ex(lg, seeds, temperature=T, softcap=cap, **kw)
            assert torch.equal(got[0], want[0])
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def _run_pair(make_old, make_new, lg, n_steps):
    old, new = make_old(), make_new()
    for _ in range(n_steps):
        old.call(lg)
        new.call(lg)
        old.step += 1
        new.step += 1
    return old.snapshot(), new.snapshot()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(1, V_SMALL), (5, V_SMALL), (3, V_SPLIT)])
def test_step_entry_with_every_control_off_is_sample_step(ops, dev, S, V, dtype):
    lg = rand_logits(S, V, dtype, dev, seed=7 * S + V)
    base = list(range(11, 11 + S))
    kw = dict(stop=[5, 9], bias=[4, 4, 9, V + 1], bias_value=-3.0, softcap=30.0, temperature=0.7)
    old, new = _run_pair(lambda: Dev(ops, dev, S, 3, 1, base, **kw),
                         lambda: DevX(ops, dev, S, 3, 1, base, seen=[[0, 1, 2]] * S, **kw), lg, 4)
    for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive"):
        assert old[k] == new[k], k
    assert np.array_equal(old["out_lp"].view(np.int32), new["out_lp"].view(np.int32))
    assert new["tail_len"] == [0] * S                        # no stop strings: never written


def test_step_entry_off_under_graph_replay(ops, dev):
    S, V = 5, V_SPLIT
    lg = rand_logits(S, V, torch.bfloat16, dev, seed=3)
    base = [3, 1 << 63, 5, 6, 7]
    kw = dict(done=[0, 0, 1, 0, 0], stop=[17, 400, 8000], bias=[4, 4, 9], bias_value=-3.0,
              softcap=30.0, temperature=0.7)
    eager = Dev(ops, dev, S, 2, 1, base, **kw)
    for _ in range(3):
        eager.call(lg)
        eager.step += 1
    want = eager.snapshot()
    d = DevX(ops, dev, S, 2, 1, base, **kw)
    d.ws = eager.ws
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.call(lg)
        d.step += 1
    for _ in range(3):
        graph.replay()
    got = d.snapshot()
    for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "step"):
        assert got[k] == want[k], k
    assert np.array_equal(got["out_lp"].view(np.int32), want["out_lp"].view(np.int32))


# --- identity 2: the step entry is the plain entry ------------------------------------------

SETTINGS = {
    "greedy": dict(temperature=0.0),
    "penalty": dict(temperature=0.7, penalty=1.3),
    "greedy_penalty_cap": dict(temperature=0.0, penalty=1.7, softcap=30.0),
    "penalty_bias_cap": dict(temperature=1.0, penalty=0.6, softcap=20.0, bias=[3, 40, 40, -1],
                             bias_value=-2.5),
    "bias_stop_strings_only": dict(temperature=0.9, bias=[2, 7], bias_value=-1.5, stops=True),
}


@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(1, V_SMALL), (4, V_SMALL), (2, V_SPLIT)])
def test_step_entry_is_the_plain_entry(ops, dev, S, V, dtype, name):
    cfg = dict(SETTINGS[name])
    penalty, stops = cfg.pop("penalty", 1.0), cfg.pop("stops", False)
    bias, bias_value = cfg.get("bias", ()), cfg.get("bias_value", 0.0)
    T, cap = cfg.get("temperature", 1.0), cfg.get("softcap", 0.0)
    g = torch.Generator().manual_seed(S * 1000 + V)
    prompts = [[int(x) for x in torch.randint(0, V, (3 + 2 * s,), generator=g)] + [V + 9, -4]
               for s in range(S)]
    base = [int(x) for x in torch.randint(0, 1 << 62, (S,), generator=g)]
    tok_bytes = [b"ab"] * V
    d = DevX(ops, dev, S, 4, 0, base, penalty=penalty, seen=prompts,
             stop_seqs=[b"zzzz"] if stops else (), tok_bytes=tok_bytes, **cfg)
    ref = R.ControlState(S, 4, 0, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    bias_t = i32(dev, bias) if len(bias) else None
    for t in range(4):
        lg = rand_logits(S, V, dtype, dev, seed=t + 31 * V)
        # the plain entry takes the same seen list with the generated tokens appended
        sid, soff = ragged_dev(dev, [prompts[s] + ref.out_tokens[s][:ref.out_len[s]]
                                     for s in range(S)])

        def draw(tt):
            ids, lp = ops.vocab_sample_ex(
                lg, None if T == 0 else seeds_for(dev, base, tt), temperature=T, softcap=cap,
                bias_ids=bias_t, bias_value=bias_value, repetition_penalty=penalty, seen_ids=sid,
                seen_off=soff)
            return ids[:, 0].tolist(), lp[:, 0].tolist()

        d.call(lg)
        ref.step(t, draw)
        assert_same(d.snapshot(), ref, f"{name} step {t}")
        d.step += 1


# --- the penalty, soft-cap off: the bits of vocab_sample on rows penalised on the host -----

def host_penalised(lg, seen, penalty, bias=(), bias_value=0.0):
    """fp32 rows with the bias added and the seen tokens penalised by torch on the host."""
    rows = lg.float().cpu().clone()
    V = rows.shape[1]
    keep = sorted({int(i) for i in bias if 0 <= int(i) < V})
    if keep:
        rows[:, keep] = rows[:, keep] + torch.tensor(bias_value, dtype=torch.float32)
    p = torch.tensor(penalty, dtype=torch.float32)
    for r, ids in enumerate(seen):
        idx = sorted({int(i) for i in ids if 0 <= int(i) < V})
        if idx:
            x = rows[r, idx]
            rows[r, idx] = torch.where(x < 0, x * p, x / p)
    return rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(1, V_SMALL), (5, V_SMALL), (3, V_SPLIT)])
def test_penalty_is_vocab_sample_on_host_penalised_rows(ops, dev, S, V, dtype):
    lg = rand_logits(S, V, dtype, dev, seed=5 * S + V)
    edge = [0, V - 1, V - 2, 31, 32] + ([SLICE - 1, SLICE, 8256, 8268] if V == V_SPLIT else [])
    seen = [edge + [V, V + 31, -1, 1 << 30] + edge[:2] if s % 2 == 0 else [] for s in range(S)]
    lg[0, 5] = float("-inf")
    lg[0, 6] = float("nan") if S > 1 else lg[0, 6]           # S == 1 keeps its log-prob finite
    seen[0] += [5, 6, 9]
    bias = [9, 11, V - 1]                                     # 9 and V - 1: biased AND seen
    g = torch.Generator().manual_seed(2)
    seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (S, 4), generator=g, dtype=torch.int64).to(dev)
    sid, soff = ragged_dev(dev, seen)
    for penalty, T in ((1.3, 1.0), (0.5, 0.7)):
        rows = host_penalised(lg, seen, penalty, bias, -2.0).to(dev)
        want = ops.vocab_sample(rows, seeds, temperature=T)
        got = ops.vocab_sample_ex(lg, seeds, temperature=T, bias_ids=i32(dev, bias), bias_value=-2.0,
                                  repetition_penalty=penalty, seen_ids=sid, seen_off=soff)
        assert torch.equal(got[0], want[0])
        assert np.array_equal(got[1].cpu().numpy().view(np.int32),
                              want[1].cpu().numpy().view(np.int32))
        assert not (got[0][0] == 5).any() and not (got[0][0] == 6).any()
    if S > 1:
        assert torch.isnan(got[1][0]).all() and torch.isfinite(got[1][1:]).all()


def test_penalty_reaches_a_token_listed_only_through_out_tokens(ops, dev):
    S, V, A, B = 2, V_SPLIT, 8268, 100
    lg = planted(S, V, dev, {A: 80.0, B: 50.0})
    d = DevX(ops, dev, S, 3, 0, [5, 6], penalty=2.0, seen=[[], []])
    ref = R.ControlState(S, 3, 0, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    for t in range(3):
        gen = [ref.out_tokens[s][:ref.out_len[s]] for s in range(S)]
        rows = host_penalised(lg, gen, 2.0).to(dev)
        d.call(lg)
        ref.step(t, vocab_sample_draw(ops, rows, [5, 6]))
        assert_same(d.snapshot(), ref, f"step {t}")
        d.step += 1
    # A leads at 80, then falls to 40 behind B's 50, then B at 25 falls behind A again
    assert d.snapshot()["out_tokens"] == [[A, B, A]] * S


# --- the penalty under a soft-cap: planted rows, fp64 restatement ---------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(2, V_SMALL), (3, V_SPLIT)])
def test_penalty_after_the_soft_cap_on_planted_rows(ops, dev, S, V, dtype):
    cap, penalty, T = 30.0, 10.0, 0.25
    lead, second = V - 1, 17
    # capped: lead 30 * tanh(3) = 29.9, second 30 * tanh(0.5) = 13.9, the rest in [-1, 0]: the
    # lead stands 16 / T = 64 ahead.  The penalty takes it to 3.0, and `second` then stands
    # 10.9 / T = 43 ahead of it; Gumbel terms of fp32 uniforms span less than 20
    lg = planted(S, V, dev, {lead: 90.0, second: 15.0}, dtype=dtype)
    seen = [[lead, lead, V + 2]] * S
    sid, soff = ragged_dev(dev, seen)
    base = [3 + s for s in range(S)]
    free, _ = ops.vocab_sample_ex(lg, seeds_for(dev, base, 0), temperature=T, softcap=cap)
    assert free[:, 0].tolist() == [lead] * S
    ids, lp = ops.vocab_sample_ex(lg, seeds_for(dev, base, 0), temperature=T, softcap=cap,
                                  repetition_penalty=penalty, seen_ids=sid, seen_off=soff)
    host = lg.float().cpu().numpy()
    for s in range(S):
        x = R.transform(host[s], softcap=cap, seen=seen[s], penalty=penalty)
        want, want_lp, gap, scale = R.gumbel64(x, seed_of(base[s], 0), T)
        tol = 2.0 * (8.0 * 2.0 ** -23 * scale + 1e-5 / T)    # test_sampler_gpu._oracle_side
        assert want == second and gap > tol
        assert int(ids[s, 0]) == want
        print(f"capped penalty S={S} V={V} row {s}: |dlp| {abs(float(lp[s, 0]) - want_lp):.2e}")
        assert abs(float(lp[s, 0]) - want_lp) < LP_TOL


# --- greedy ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,V", [(1, V_SMALL), (5, V_SMALL), (3, V_SPLIT)])
def test_greedy_is_the_first_argmax_of_the_transformed_row(ops, dev, S, V, dtype):
    lg = rand_logits(S, V, dtype, dev, seed=9 * S + V)
    lg[0, 3] = float("nan") if S > 1 else lg[0, 3]
    lg[-1, 8] = float("-inf")
    seen = [[int(torch.argmax(torch.nan_to_num(lg[s].float(), nan=-1e9))), 8, 3] for s in range(S)]
    sid, soff = ragged_dev(dev, seen)
    bias = [1, 2]
    host = lg.float().cpu().numpy()
    outs = []
    for seed in (1, 2):
        seeds = torch.full((S, 2), seed, dtype=torch.int64, device=dev)
        outs.append(ops.vocab_sample_ex(lg, seeds, temperature=0.0, bias_ids=i32(dev, bias),
                                        bias_value=-1.0, repetition_penalty=3.0, seen_ids=sid,
                                        seen_off=soff))
    outs.append(ops.vocab_sample_ex(lg, None, temperature=0.0, bias_ids=i32(dev, bias), n_draw=2,
                                    bias_value=-1.0, repetition_penalty=3.0, seen_ids=sid,
                                    seen_off=soff))
    for o in outs[1:]:                                        # seeds are not read
        assert torch.equal(o[0], outs[0][0])
        assert np.array_equal(o[1].cpu().numpy().view(np.int32),
                              outs[0][1].cpu().numpy().view(np.int32))
    ids, lp = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    for s in range(S):
        x32 = R.transform(host[s], bias_ids=bias, bias_value=-1.0, seen=seen[s], penalty=3.0,
                          dtype=np.float32)
        want, want_lp = R.greedy(x32)
        assert ids[s].tolist() == [want, want], s
        assert want != seen[s][0]                             # the penalty demoted the leader
        if np.isnan(want_lp):
            assert np.isnan(lp[s]).all()
        else:
            assert np.abs(lp[s] - want_lp).max() < LP_TOL


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_ties_go_to_the_lowest_id(ops, dev, dtype):
    # one thread (5, 261), one wave (3, 7), two waves (10, 100), two slices (200, 6000)
    pairs = [(5, 261), (3, 7), (10, 100), (200, 6000), (SLICE - 1, SLICE)]
    S, V = len(pairs), V_SPLIT
    lg = planted(S, V, dev, {}, dtype=dtype)
    for s, (a, b) in enumerate(pairs):
        lg[s, a] = lg[s, b] = 8.0
    ids, lp = ops.vocab_sample_ex(lg, None, temperature=0.0)
    assert ids[:, 0].tolist() == [a for a, _ in pairs]
    st = DevX(ops, dev, S, 1, 0, [1] * S, temperature=0.0)
    st.call(lg)
    assert st.snapshot()["out_tokens"] == [[a] for a, _ in pairs]
    host = lg.float().cpu().numpy()
    for s in range(S):
        assert R.greedy(host[s])[0] == pairs[s][0]
        assert abs(float(lp[s, 0]) - R.greedy(host[s])[1]) < LP_TOL


def test_greedy_with_nothing_drawable(ops, dev):
    S, V = 2, V_SMALL
    lg = planted(S, V, dev, {})
    lg[0] = float("-inf")
    ids, lp = ops.vocab_sample_ex(lg, None, temperature=0.0)
    assert int(ids[0, 0]) == -1 and bool(torch.isnan(lp[0, 0])) and int(ids[1, 0]) >= 0
    st = DevX(ops, dev, S, 2, 4, [1, 2], temperature=0.0)
    st.call(lg)
    snap = st.snapshot()
    assert snap["done"] == [1, 0] and snap["out_len"] == [0, 1] and snap["next_tok"][0] == 4


# --- stop strings ---------------------------------------------------------------------------

def force(S, V, dev, toks, dtype=torch.float32):
    """Rows whose draw is forced: token toks[s] stands 40 ahead in row s."""
    lg = planted(S, V, dev, {}, dtype=dtype)
    for s, t in enumerate(toks):
        lg[s, t] = 40.0
    return lg


TOKS = [b"a", b"b", b"ab", b"", b"xyz", b"###", b"\n\n", b"q" * 20, b"q" * 12, b"end"]


@pytest.mark.parametrize("temperature", [1.0, 0.0])
def test_stop_strings_follow_the_restatement_step_by_step(ops, dev, temperature):
    V = V_SMALL
    tok_bytes = TOKS + [bytes([65 + v % 26]) for v in range(len(TOKS), V)]
    stops = [b"aab", b"###", b"\n\n\n", b"q" * 32, b"aend"]
    scripts = [
        [0, 0, 0, 1, 4, 4],        # "aaab": the overlapping prefix, complete at step 3
        [4, 5, 4, 4, 4, 4],        # "###" inside one token, step 1
        [6, 3, 6, 4, 4, 4],        # "\n\n" + special + "\n\n": spans tokens across an empty one
        [7, 8, 4, 4, 4, 4],        # 20 + 12 bytes: the 32-byte stop string, step 1
        [2, 1, 2, 1, 2, 0],        # "ababab" then "a": "aab"? no: runs to max_tokens, no hit
        # token 9 ("end") is a stop ID and, after "aa", its bytes would complete "aend" too:
        # the stop id wins, nothing is appended and the tail stands at "aa"
        [0, 0, 9, 1, 4, 4],
        [4, 4, 4, 0, 0, 1],        # "aab" completes on the step that reaches max_tokens
        [30, 9 + 21, 4, 4, 4, 4],  # single letters only
    ]
    S, max_tokens = len(scripts), 6
    done0 = [0] * S
    done0[7] = 1                                              # a finished stream is untouched
    d = DevX(ops, dev, S, max_tokens, 63, list(range(1, S + 1)), done=done0, stop=[9],
             stop_seqs=stops, tok_bytes=tok_bytes, temperature=temperature)
    d.tail[7, :3] = torch.tensor([7, 7, 7], dtype=torch.uint8)
    ref = R.ControlState(S, max_tokens, 63, tok_bytes=tok_bytes, stop_seqs=stops, stop_ids=[9],
                         done=done0, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    for t in range(max_tokens):
        col = [sc[t] for sc in scripts]
        d.call(force(S, V, dev, col))
        ref.step(t, lambda tt: (col, [0.0] * S))
        snap = d.snapshot()
        what = f"step {t}"
        for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive"):
            assert snap[k] == getattr(ref, k), (what, k)
        for s in range(S - 1):
            assert snap["tail_len"][s] == len(ref.win[s].tail), (what, s)
            assert bytes(snap["tail"][s][:snap["tail_len"][s]]) == ref.win[s].tail, (what, s)
        assert snap["tail"][7][:3] == [7, 7, 7] and snap["tail_len"][7] == 0
        d.step += 1
    assert ref.out_len == [4, 2, 3, 2, 6, 2, 6, 0]
    assert ref.done == [1] * S
    # the coincidence is real: had token 9 been appended, the window would have hit "aend"
    assert R.run_window(tok_bytes, [0, 0, 9], stops) == 2
    assert ref.win[5].tail == b"aa" and snap["tail_len"][5] == 2 and snap["out_len"][5] == 2
    assert snap["out_tokens"][5][2] == SENT_TOK


# --- graph replay with the controls on ------------------------------------------------------

def test_graph_replay_with_penalty_and_stop_strings(ops, dev):
    S, V = 4, V_SPLIT
    tok_bytes = [bytes([97 + v % 3]) for v in range(V)]        # "a", "b", "c"
    lg = rand_logits(S, V, torch.bfloat16, dev, seed=12) * 4.0  # peaked: repeats without a penalty
    prompts = [[int(torch.argmax(lg[s].float()))] for s in range(S)]
    mk = lambda: DevX(ops, dev, S, 8, 1, [21, 22, 23, 24], penalty=1.8, seen=prompts,
                      stop_seqs=[b"cc", b"abca"], tok_bytes=tok_bytes, temperature=0.3, softcap=30.0)
    eager = mk()
    snaps = []
    for _ in range(8):
        eager.call(lg)
        eager.step += 1
        snaps.append(eager.snapshot())
    want = snaps[-1]
    d = mk()
    d.ws = eager.ws
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.call(lg)
        d.step += 1
    for _ in range(8):
        graph.replay()
    got = d.snapshot()
    for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "step", "tail_len"):
        assert got[k] == want[k], k
    for s in range(S):
        assert got["tail"][s][:got["tail_len"][s]] == want["tail"][s][:want["tail_len"][s]]
    assert np.array_equal(got["out_lp"].view(np.int32), want["out_lp"].view(np.int32))
    assert want["n_alive"] == 0


# --- one real-width vocabulary --------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 3, 256])
def test_real_width_vocabulary(ops, dev, S):
    """V = 256,000 with bias and penalty on and a seen id at V - 1.  S = 256 rows are not
    split: one workgroup holds both bitmaps of the whole row (64,000 bytes of LDS)."""
    V = 256000
    lead, mid, low = 1000, V - 1, 77
    lg = torch.zeros(S, V, dtype=torch.bfloat16, device=dev)
    lg[:, lead], lg[:, mid], lg[:, low] = 200.0, 160.0, 120.0
    sid, soff = ragged_dev(dev, [[mid, 5, V]] * S)
    bias = i32(dev, [lead])
    kw = dict(bias_ids=bias, bias_value=-1e6, repetition_penalty=4.0, seen_ids=sid, seen_off=soff)
    # lead is biased away, mid falls to 40, low stands 80 ahead
    ids, _ = ops.vocab_sample_ex(lg, None, temperature=0.0, **kw)
    assert ids[:, 0].tolist() == [low] * S
    seeds = torch.arange(S, dtype=torch.int64, device=dev).reshape(S, 1)
    ids, _ = ops.vocab_sample_ex(lg, seeds, temperature=1.0, **kw)
    assert ids[:, 0].tolist() == [low] * S
    ids, _ = ops.vocab_sample_ex(lg, None, temperature=0.0, bias_ids=bias, bias_value=-1e6)
    assert ids[:, 0].tolist() == [mid] * S
    if S <= 3:
        d = DevX(ops, dev, S, 2, 0, list(range(S)), penalty=4.0, seen=[[5]] * S, bias=[lead],
                 bias_value=-1e6, temperature=0.0)
        d.call(lg)                                            # mid is not seen yet
        d.call(lg)                                            # now it is, through out_tokens
        assert d.snapshot()["out_tokens"] == [[mid, low]] * S


# --- bad arguments --------------------------------------------------------------------------

BAD = {
    "temperature_negative": dict(temperature=-0.5),
    "temperature_inf": dict(temperature=float("inf")),
    "temperature_nan": dict(temperature=float("nan")),
    "penalty_zero": dict(repetition_penalty=0.0),
    "penalty_negative": dict(repetition_penalty=-1.3),
    "penalty_inf": dict(repetition_penalty=float("inf")),
    "penalty_nan": dict(repetition_penalty=float("nan")),
    "nine_stop_strings": dict(stop_seqs=[b"a"] * 9),
    "empty_stop_string": dict(stop_seqs=[b"ab", b""]),
    "long_stop_string": dict(stop_seqs=[b"x" * 33]),
    "stop_strings_without_token_bytes": dict(stop_seqs=[b"ab"], tok_bytes=None),
    "stop_strings_without_tail": dict(stop_seqs=[b"ab"], tail=None),
    "softcap_negative": dict(softcap=-1.0),
    "pad_at_vocab": dict(pad_id=64),
    "max_tokens_zero": dict(max_tokens=0),
}


@pytest.mark.parametrize("case", sorted(BAD) + ["n_bias", "seen_off_without_ids"])
def test_bad_arguments_raise_and_change_nothing(ops, pkg, dev, case):
    CSError = pkg.CSError
    S, V = 2, V_SMALL
    lg = planted(S, V, dev, {3: 40.0})
    d = DevX(ops, dev, S, 3, 0, [1, 2], tok_bytes=[b"ab"] * V, seen=[[1], [2]])
    before = d.snapshot()
    if case in BAD:
        with pytest.raises(CSError):
            d.call(lg, **BAD[case])
    elif case == "n_bias":
        with pytest.raises(CSError, match="n_bias"):
            d.call(lg, bias_ids=torch.zeros(1025, dtype=torch.int32, device=dev))
    else:
        L = import_module(pkg.__name__ + "._lib").load()
        need = L.cs_sample_step_ex_workspace_size(S, V)
        assert need == L.cs_sample_step_workspace_size(S, V)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        rc = L.cs_sample_step_ex(
            lg.data_ptr(), 0, S, V, V, 1.0, 0.0, d.base.data_ptr(), d.step.data_ptr(), None, 0, 0.0,
            1.3, None, d.seen_off.data_ptr(), None, 0, None, None, None, None, 0, None, None, 3, 0,
            d.done.data_ptr(), d.out_len.data_ptr(), d.out_tokens.data_ptr(), d.out_lp.data_ptr(),
            d.next_tok.data_ptr(), d.n_alive.data_ptr(), ws.data_ptr(), need,
            torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"NULL" in L.cs_last_error()
    after = d.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    d.call(lg)
    assert d.snapshot()["next_tok"] == [3, 3]


@pytest.mark.parametrize("kw", [dict(temperature=-1.0), dict(temperature=float("nan")),
                                dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf")),
                                dict(softcap=float("inf"))])
def test_plain_entry_bad_arguments(ops, pkg, dev, kw):
    lg = planted(2, V_SMALL, dev, {3: 40.0})
    seeds = torch.zeros(2, 1, dtype=torch.int64, device=dev)
    with pytest.raises(pkg.CSError):
        ops.vocab_sample_ex(lg, seeds, **kw)
    with pytest.raises(pkg.CSError):                          # Gumbel draws need their seeds
        ops.vocab_sample_ex(lg, None, temperature=1.0, bias_ids=i32(dev, [1]))
