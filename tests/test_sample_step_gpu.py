"""cs_sample_step (csrc/proposer.hip) against the state machine's restatement driven by
ops.vocab_sample on the biased fp32 rows (tests/sample_step_ref.py): ids, log-probs, lengths,
done flags, next tokens and n_alive after every step, zero tolerance."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import PKG_DIR
from sample_step_ref import StepState, as_i64, vocab_sample_draw

pytestmark = pytest.mark.gpu

SENT_TOK, SENT_LP, SENT_NEXT = -7, -777.0, -99
# the two vocabularies that plan_split cuts into several splits at 3 rows (8 and 7 splits:
# test_split_vocabularies_are_split reads the counts back from the workspace size)
SPLIT_VOCABS = (32768, 32768 + 77)


class Dev:
    """The device side of one run: every state tensor pre-filled with its sentinel."""

    def __init__(self, ops, dev, S, max_tokens, pad, base, *, done=None, stop=(), bias=(),
                 bias_value=0.0, temperature=1.0, softcap=0.0, with_lp=True, vocab=None):
        self.ops, self.S, self.max_tokens, self.pad = ops, S, max_tokens, pad
        self.base = torch.tensor([as_i64(b) for b in base], dtype=torch.int64, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.done = torch.tensor([0] * S if done is None else done, dtype=torch.int32, device=dev)
        self.out_len = torch.zeros(S, dtype=torch.int32, device=dev)
        self.out_tokens = torch.full((S, max_tokens), SENT_TOK, dtype=torch.int32, device=dev)
        self.out_lp = torch.full((S, max_tokens), SENT_LP, dtype=torch.float32, device=dev) \
            if with_lp else None
        self.next_tok = torch.full((S,), SENT_NEXT, dtype=torch.int64, device=dev)
        self.n_alive = torch.full((1,), -5, dtype=torch.int32, device=dev)
        self.stop = torch.tensor(list(stop), dtype=torch.int32, device=dev) if stop else None
        self.bias = torch.tensor(list(bias), dtype=torch.int32, device=dev) if bias else None
        self.kw = dict(pad_id=pad, temperature=temperature, softcap=softcap,
                       bias_value=bias_value, vocab=vocab)
        self.ws = ops.Workspace(zeroed=True)

    def call(self, logits, **over):
        kw = dict(self.kw, bias_ids=self.bias, stop_ids=self.stop, out_lp=self.out_lp,
                  workspace=self.ws)
        kw.update(over)
        self.ops.sample_step(logits, self.base, self.step, self.done, self.out_len,
                             self.out_tokens, self.next_tok, self.n_alive, **kw)

    def snapshot(self):
        torch.cuda.synchronize()
        return dict(done=self.done.tolist(), out_len=self.out_len.tolist(),
                    out_tokens=self.out_tokens.tolist(),
                    out_lp=None if self.out_lp is None else self.out_lp.cpu().numpy().copy(),
                    next_tok=self.next_tok.tolist(), n_alive=int(self.n_alive.item()),
                    step=int(self.step.item()))


def assert_same(snap, ref: StepState, what=""):
    assert snap["done"] == ref.done, what
    assert snap["out_len"] == ref.out_len, what
    assert snap["out_tokens"] == ref.out_tokens, what
    assert snap["next_tok"] == ref.next_tok, what
    assert snap["n_alive"] == ref.n_alive, what
    if snap["out_lp"] is not None:
        want = np.asarray(ref.out_lp, dtype=np.float32)
        assert np.array_equal(snap["out_lp"], want, equal_nan=True), what


def n_splits(pkg, rows, vocab):
    L = import_module(pkg.__name__ + "._lib").load()
    # cs_vocab_sample with one draw keeps 16 bytes per (row, split)
    return L.cs_vocab_sample_workspace_size(rows, vocab, 1) // (16 * rows)


def run_steps(ops, dev, S, V, ld, dtype, softcap, temperature, seed, n_steps=5, max_tokens=4,
              done=None):
    """Five steps on fresh random logits per step (written into ONE buffer), ``step``
    incremented on the device; stops, a duplicated bias list and max_tokens all bite."""
    g = torch.Generator().manual_seed(seed)
    pad = V - 1
    base = [int(x) for x in torch.randint(0, 1 << 62, (S,), generator=g)]
    base[0] = (1 << 64) - 1 - seed              # high bit set: the uint64 word, not its int64
    stop = sorted({int(x) for x in torch.randint(0, V, (max(1, V // 6),), generator=g)})[:16]
    bias = [int(x) for x in torch.randint(0, V, (min(5, V),), generator=g)]
    bias = bias + bias[:2] + [V + 3, -2]        # duplicates and out-of-range ids
    d = Dev(ops, dev, S, max_tokens, pad, base, done=done, stop=stop, bias=bias, bias_value=-4.0,
            temperature=temperature, softcap=softcap, vocab=V)
    ref = StepState(S, max_tokens, pad, stop_ids=stop, done=done, sentinel_tok=SENT_TOK,
                    sentinel_lp=SENT_LP)
    buf = torch.zeros(S, ld, dtype=dtype, device=dev)
    snaps = []
    for t in range(n_steps):
        fresh = (torch.randn(S, ld, generator=g) * 3.0).to(dtype)
        if done is not None:
            fresh[torch.tensor(done, dtype=torch.bool)] = float("nan")
        buf.copy_(fresh.to(dev))
        d.call(buf)
        ref.step(t, vocab_sample_draw(ops, buf, base, temperature=temperature, softcap=softcap,
                                      bias_ids=bias, bias_value=-4.0, vocab=V))
        snap = d.snapshot()
        assert_same(snap, ref, f"S={S} V={V} step {t}")
        assert snap["step"] == t
        snaps.append(snap)
        d.step += 1                              # on the device; no host argument changes
    assert ref.n_alive == 0                      # max_tokens < n_steps: every stream ended
    return snaps, ref


CASES = [(S, V) for S in (1, 3, 65) for V in (1, 255, 257, 384)]


@pytest.mark.parametrize("i,S,V", [(i, S, V) for i, (S, V) in enumerate(CASES)])
def test_steps_match_reference(ops, dev, i, S, V):
    # dtype, soft-cap and temperature cycle with different periods over the 12 shapes
    dtype = (torch.bfloat16, torch.float32)[i % 2]
    softcap = (0.0, 30.0)[(i // 2) % 2]
    temperature = (1.0, 0.7)[(i // 4) % 2 if i < 8 else i % 2]
    run_steps(ops, dev, S, V, V, dtype, softcap, temperature, seed=100 + i)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", SPLIT_VOCABS)
def test_split_vocabularies(ops, pkg, dev, V, dtype):
    assert n_splits(pkg, 3, V) > 1
    run_steps(ops, dev, 3, V, V, dtype, 30.0 if dtype == torch.bfloat16 else 0.0,
              0.7 if V % 2 else 1.0, seed=V)


def test_split_vocabularies_are_split(pkg):
    assert [n_splits(pkg, 3, V) for V in SPLIT_VOCABS] == [8, 7]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_row_stride_wider_than_vocab(ops, dev, dtype):
    run_steps(ops, dev, 3, 257, 300, dtype, 30.0, 0.7, seed=9)


def test_streams_that_start_done(ops, dev):
    S, V = 7, 384
    done = [1, 0, 0, 1, 1, 0, 1]
    snaps, ref = run_steps(ops, dev, S, V, V, torch.bfloat16, 0.0, 1.0, seed=4, done=done)
    # the same run with the done streams live instead (same row count, so the same plan):
    # the live streams' results do not depend on their neighbours
    snaps_all, ref_all = run_steps(ops, dev, S, V, V, torch.bfloat16, 0.0, 1.0, seed=4)
    for s, dn in enumerate(done):
        if dn:   # NaN rows, never read: everything but next_tok keeps its sentinel
            assert snaps[-1]["out_tokens"][s] == [SENT_TOK] * 4
            assert (snaps[-1]["out_lp"][s] == SENT_LP).all()
            assert snaps[-1]["out_len"][s] == 0 and snaps[0]["next_tok"][s] == V - 1
        else:
            assert snaps[-1]["out_tokens"][s] == snaps_all[-1]["out_tokens"][s]
            assert np.array_equal(snaps[-1]["out_lp"][s], snaps_all[-1]["out_lp"][s])
    assert snaps[0]["n_alive"] <= 3


def planted(S, V, dev, plants, dtype=torch.float32, seed=0):
    """Logits in [-1, 0] with the given {token: value} planted in every row."""
    g = torch.Generator().manual_seed(seed)
    x = -torch.rand(S, V, generator=g)
    for tok, val in plants.items():
        x[:, tok] = val
    return x.to(dtype).to(dev)


def test_planted_stop_at_step_two(ops, dev):
    S, V, pad = 2, 300, 0
    d = Dev(ops, dev, S, 6, pad, [11, 12], stop=[77, V + 5])
    seq = [10, 20, 77, 30, 40]                       # the forced token per step
    for t, tok in enumerate(seq):
        d.call(planted(S, V, dev, {tok: 40.0}, seed=t))
        d.step += 1
        snap = d.snapshot()
        if t < 2:
            assert snap["next_tok"] == [tok] * S and snap["n_alive"] == S
        else:
            assert snap["next_tok"] == [pad] * S and snap["n_alive"] == 0
    assert snap["out_len"] == [2, 2] and snap["done"] == [1, 1]
    assert snap["out_tokens"] == [[10, 20] + [SENT_TOK] * 4] * 2   # the stop id is not appended
    assert (snap["out_lp"][:, 2:] == SENT_LP).all() and (snap["out_lp"][:, :2] > -1e-6).all()


def test_planted_bias_moves_the_draw_to_the_runner_up(ops, dev):
    S, V = 3, 257
    lg = planted(S, V, dev, {100: 40.0, 200: 30.0}, dtype=torch.bfloat16)
    free = Dev(ops, dev, S, 2, 0, [1, 2, 3])
    free.call(lg)
    assert free.snapshot()["next_tok"] == [100] * S
    d = Dev(ops, dev, S, 2, 0, [1, 2, 3], bias=[100], bias_value=-1e6)
    d.call(lg)
    assert d.snapshot()["next_tok"] == [200] * S


def test_duplicate_bias_counts_once(ops, dev):
    S, V, A, B = 2, 384, 5, 300
    lg = planted(S, V, dev, {A: 200.0, B: 110.0})
    # ids past the vocabulary and negative ones are ignored (V + B % V would alias B)
    d = Dev(ops, dev, S, 1, 0, [5, 6], bias=[A, A, V + 1, -1, 1 << 30], bias_value=-60.0)
    d.call(lg)
    snap = d.snapshot()
    assert snap["out_tokens"] == [[A]] * S           # 140 beats 110; 80 would not
    ref = StepState(S, 1, 0, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    ref.step(0, vocab_sample_draw(ops, lg, [5, 6], bias_ids=[A, A, V + 1, -1, 1 << 30],
                                  bias_value=-60.0))
    assert_same(snap, ref)


def test_degenerate_rows(ops, dev):
    S, V = 3, 255
    lg = planted(S, V, dev, {})
    lg[0] = float("-inf")                            # nothing drawable: the stream just ends
    lg[1, 17] = float("nan")                         # a NaN token: the id of vocab_sample, lp NaN
    d = Dev(ops, dev, S, 3, 4, [7, 8, 9])
    ref = StepState(S, 3, 4, sentinel_tok=SENT_TOK, sentinel_lp=SENT_LP)
    d.call(lg)
    ref.step(0, vocab_sample_draw(ops, lg, [7, 8, 9]))
    snap = d.snapshot()
    assert_same(snap, ref)
    assert snap["done"] == [1, 0, 0] and snap["out_len"] == [0, 1, 1]
    assert snap["out_tokens"][0] == [SENT_TOK] * 3 and snap["next_tok"][0] == 4
    assert np.isnan(snap["out_lp"][1, 0]) and snap["out_tokens"][1][0] != 17
    assert np.isfinite(snap["out_lp"][2, 0])


def test_without_logprobs(ops, dev):
    S, V = 3, 257
    lg = planted(S, V, dev, {9: 40.0})
    d = Dev(ops, dev, S, 2, 0, [1, 2, 3], with_lp=False)
    d.call(lg)
    snap = d.snapshot()
    assert snap["out_tokens"] == [[9, SENT_TOK]] * S and snap["n_alive"] == S


def test_graph_replay_equals_eager_calls(ops, dev):
    S, V = 5, SPLIT_VOCABS[1]
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(S, V, generator=g) * 3.0).to(torch.bfloat16).to(dev)
    base = [3, 1 << 63, 5, 6, 7]
    stop = [int(x) for x in torch.randint(0, V, (16,), generator=g)]
    mk = lambda: Dev(ops, dev, S, 2, 1, base, done=[0, 0, 1, 0, 0], stop=stop, bias=[4, 4, 9],
                     bias_value=-3.0, softcap=30.0, temperature=0.7)
    eager = mk()
    for _ in range(3):
        eager.call(lg)
        eager.step += 1
    want = eager.snapshot()
    assert want["n_alive"] == 0 and want["step"] == 3     # max_tokens 2 < 3 steps
    d = mk()
    d.ws = eager.ws                                  # allocated, and left zeroed where it counts
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.call(lg)                                   # one chain: the two launches, then step += 1
        d.step += 1
    got = []
    for _ in range(3):
        graph.replay()                               # nothing is cleared in between
        got.append(d.snapshot())
    assert [s["n_alive"] for s in got][-1] == 0 and got[0]["n_alive"] > 0
    for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive", "step"):
        assert got[-1][k] == want[k], k
    assert np.array_equal(got[-1]["out_lp"], want["out_lp"], equal_nan=True)


BAD = {
    "temperature_zero": dict(temperature=0.0),
    "temperature_inf": dict(temperature=float("inf")),
    "temperature_nan": dict(temperature=float("nan")),
    "softcap_negative": dict(softcap=-1.0),
    "pad_negative": dict(pad_id=-1),
    "pad_at_vocab": dict(pad_id=64),
    "max_tokens_zero": dict(max_tokens=0),
    "vocab_wider_than_row": dict(vocab=65),
}


@pytest.mark.parametrize("case", sorted(BAD) + ["n_stop", "n_bias", "dtype", "null", "short_ws",
                                                "misaligned_ws"])
def test_bad_arguments_raise_and_launch_nothing(ops, pkg, dev, case):
    CSError = pkg.CSError
    S, V = 2, 64
    lg = planted(S, V, dev, {3: 40.0})
    d = Dev(ops, dev, S, 3, 0, [1, 2])
    before = d.snapshot()
    if case in BAD:
        with pytest.raises(CSError):
            d.call(lg, **BAD[case])
    elif case == "n_stop":
        with pytest.raises(CSError, match="n_stop"):
            d.call(lg, stop_ids=torch.arange(17, dtype=torch.int32, device=dev))
    elif case == "n_bias":
        with pytest.raises(CSError, match="n_bias"):
            d.call(lg, bias_ids=torch.zeros(1025, dtype=torch.int32, device=dev))
    elif case == "dtype":
        with pytest.raises(CSError):
            d.call(lg.to(torch.float64))
    else:
        # straight through the C ABI: what ops cannot express
        L = import_module(pkg.__name__ + "._lib").load()
        need = L.cs_sample_step_workspace_size(S, V)
        ws = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 8 == 0

        def abi(dtype=0, done_ptr=d.done.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need):
            return L.cs_sample_step(
                lg.data_ptr(), dtype, S, V, V, 1.0, 0.0, d.base.data_ptr(), d.step.data_ptr(),
                None, 0, 0.0, None, 0, 3, 0, done_ptr, d.out_len.data_ptr(),
                d.out_tokens.data_ptr(), d.out_lp.data_ptr(), d.next_tok.data_ptr(),
                d.n_alive.data_ptr(), ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)

        if case == "null":
            assert abi(done_ptr=None) == -1 and b"NULL" in L.cs_last_error()
            assert abi(dtype=7) == -1
        elif case == "short_ws":
            assert abi(ws_bytes=need - 1) < 0 and abi(ws_ptr=None) < 0
        else:
            assert abi(ws_ptr=ws.data_ptr() + 4) < 0
        assert L.cs_sample_step(None, 0, 0, V, V, 1.0, 0.0, None, None, None, 0, 0.0, None, 0, 3,
                                0, None, None, None, None, None, None, None, 0, None) == 0  # S = 0
    after = d.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    d.call(lg)                                       # and the same state still takes a good call
    assert d.snapshot()["next_tok"] == [3, 3]
