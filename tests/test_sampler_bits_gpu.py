"""The output bits of the four sampling entries (ops.vocab_sample, sample_step, vocab_sample_ex,
sample_step_ex; csrc/proposer.hip) against tests/golden/sampler_bits.npz, with no tolerance.

What this pins: THIS TOOLCHAIN'S bits for these entries, so that a change of the sampler that
is meant to leave every output bit alone can show that it did.  The other sampler tests say
whether the bits are right; this one only says that they are the recorded ones.  If a ROCm
upgrade moves logf, rewrite the fixture on the GPU, from a commit whose other sampler tests
pass:

  python tests/test_sampler_bits_gpu.py --write

The fixture holds outputs only: per case one int32 vector (ids, lengths, flags, tail bytes)
and one uint32 vector (the log-probs' bit patterns), the fields concatenated in the order the
case lists them.  The inputs are integer formulas written here, every logit a multiple of 1/4
below 256 in magnitude and so exact in bf16: no random generator enters them."""
import os
import sys

import numpy as np
import pytest
import torch

from test_sample_controls_gpu import V_SMALL, V_SPLIT, DevX, i32, ragged_dev
from test_sample_step_gpu import Dev

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_bits.npz")
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
S_STEP, MAX_TOKENS, PAD = 3, 4, 1
FORCED = 200.0                                   # stands ahead of every other logit at any setting


def logits(rows, V, t, dtype, dev, force=()):
    """Row r, token v at step t: ((37 v + 101 r + 53 t) mod 61 - 30) / 4, two planted peaks per
    row (12 and 10, the second in the last slice of a split row), and `force` = (row, token)
    pairs that take FORCED."""
    v = torch.arange(V, dtype=torch.int64).reshape(1, V)
    r = torch.arange(rows, dtype=torch.int64).reshape(rows, 1)
    x = (((37 * v + 101 * r + 53 * t) % 61 - 30).to(torch.float32) * 0.25)
    for row in range(rows):
        x[row, (7 * row + 3 + 11 * t) % V] = 12.0
        x[row, V - 1 - row - t] = 10.0
    for row, tok in force:
        x[row, tok] = FORCED
    assert torch.equal(x.to(torch.bfloat16).to(torch.float32), x)
    return x.to(dtype).to(dev)


def seeds(rows, n_draw, dev):
    r = torch.arange(rows, dtype=torch.int64).reshape(rows, 1)
    d = torch.arange(n_draw, dtype=torch.int64).reshape(1, n_draw)
    return (r * 1000003 + d * 7919 + 12345).to(dev)


def seen_lists(rows, V):
    """Per row: both planted peaks of step 0, ids at the slice and word edges, one past the row."""
    return [[(7 * r + 3) % V, V - 1 - r, 0, 31, 32, V - 2, V + 5] + [5120 % V] * (r % 2)
            for r in range(rows)]


def draw_fields(out):
    ids, lp = out
    return [("ids", ids.cpu().numpy()), ("lp", lp.cpu().numpy().view(np.uint32))]


def state_fields(d, t, tail=False):
    snap = d.snapshot()
    f = [(f"t{t}/{k}", np.asarray(snap[k], dtype=np.int32).reshape(-1))
         for k in ("done", "out_len", "out_tokens", "next_tok", "n_alive")]
    if tail:
        f += [(f"t{t}/tail", d.tail.cpu().numpy().astype(np.int32).reshape(-1)),
              (f"t{t}/tail_len", d.tail_len.cpu().numpy())]
    return f + [(f"t{t}/out_lp", snap["out_lp"].view(np.uint32).reshape(-1))]


# --- the cases: name -> function (ops, dev) -> [(field name, int32 or uint32 array)] ----------

def plain_case(dtype, V, cap, rows, n_draw):
    def run(ops, dev):
        return draw_fields(ops.vocab_sample(logits(rows, V, 0, dtype, dev), seeds(rows, n_draw, dev),
                                            temperature=0.7 if cap else 1.0, softcap=cap))
    return run


STOP_TOK = 9


def step_case(dtype, V, biased):
    def run(ops, dev):
        d = Dev(ops, dev, S_STEP, MAX_TOKENS, PAD, [11, (1 << 63) + 5, 13], stop=[STOP_TOK],
                bias=[3, 3, V - 1, V + 7] if biased else (), bias_value=-3.0, temperature=0.7,
                softcap=30.0)
        fields = []
        for t in range(3):
            d.call(logits(S_STEP, V, t, dtype, dev, force=[(0, STOP_TOK)] if t == 1 else ()))
            fields += state_fields(d, t)
            d.step += 1
        assert d.snapshot()["done"][0] == 1 and d.snapshot()["out_len"][0] == 1   # the stop id
        return fields
    return run


EX = {
    "penalty": dict(temperature=0.7, repetition_penalty=1.3),
    "greedy": dict(temperature=0.0),
    "bias_penalty_cap": dict(temperature=0.7, repetition_penalty=1.3, softcap=30.0, bias=True),
}


def plain_ex_case(dtype, V, name, n_draw, rows=3):
    def run(ops, dev):
        kw = dict(EX[name])
        if kw.pop("bias", False):
            kw.update(bias_ids=i32(dev, [(7 * 1 + 3) % V, 4, V - 3]), bias_value=-2.5)
        if "repetition_penalty" in kw:
            kw["seen_ids"], kw["seen_off"] = ragged_dev(dev, seen_lists(rows, V))
        sd = None if kw["temperature"] == 0.0 else seeds(rows, n_draw, dev)
        return draw_fields(ops.vocab_sample_ex(logits(rows, V, 0, dtype, dev), sd, n_draw=n_draw,
                                               **kw))
    return run


STOP_SEQ, TOK_B, TOK_C = b"bc", 6, 7             # token v's byte is "a" + v mod 5


def step_ex_case(dtype, V, name):
    def run(ops, dev):
        kw = dict(temperature=0.7)
        force = {}
        if name == "penalty":
            # the same row at every step and a sharp draw: without the penalty a stream would
            # repeat its first token, which joins the seen set through out_tokens
            kw.update(temperature=0.05, penalty=1.3, seen=[[0, 31, V + 5]] * S_STEP)
        elif name == "greedy":
            kw.update(temperature=0.0)
        else:
            kw.update(stop_seqs=[STOP_SEQ], tok_bytes=[bytes([97 + v % 5]) for v in range(V)])
            force = {1: [(0, TOK_B)], 2: [(0, TOK_C)]}
        d = DevX(ops, dev, S_STEP, MAX_TOKENS, PAD, [21, 22, (1 << 63) + 23], **kw)
        fields = []
        for t in range(3):
            d.call(logits(S_STEP, V, 0 if name == "penalty" else t, dtype, dev, force.get(t, ())))
            fields += state_fields(d, t, tail=True)
            d.step += 1
        snap = d.snapshot()
        if name == "stop_string":                # row 0 ended on the step that completed "bc"
            assert snap["done"][0] == 1 and snap["out_tokens"][0][1:3] == [TOK_B, TOK_C]
        if name == "penalty":                    # the penalty kept step 1 off step 0's token
            assert all(row[0] != row[1] for row in snap["out_tokens"])
        return fields
    return run


CASES = {}
for _dn, _dt in DTYPES.items():
    for _V in (V_SMALL, V_SPLIT):
        for _cap in (0.0, 30.0):
            for _rows in (1, 3):
                for _n in (1, 16):
                    CASES[f"vocab_sample/{_dn}/V{_V}/cap{_cap:g}/rows{_rows}/n{_n}"] = \
                        plain_case(_dt, _V, _cap, _rows, _n)
        for _b in (False, True):
            CASES[f"sample_step/{_dn}/V{_V}/{'bias' if _b else 'nobias'}"] = step_case(_dt, _V, _b)
        for _name in EX:
            for _n in (1, 16):
                CASES[f"vocab_sample_ex/{_dn}/V{_V}/{_name}/n{_n}"] = plain_ex_case(_dt, _V, _name, _n)
        for _name in ("penalty", "greedy", "stop_string"):
            CASES[f"sample_step_ex/{_dn}/V{_V}/{_name}"] = step_ex_case(_dt, _V, _name)


def pack(fields):
    ints = [a.reshape(-1) for _, a in fields if a.dtype == np.int32]
    lps = [a.reshape(-1) for _, a in fields if a.dtype == np.uint32]
    assert len(ints) + len(lps) == len(fields)
    return np.concatenate(ints), np.concatenate(lps)


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_these_cases(golden):
    assert sorted(golden) == sorted(f"{c}/{kind}" for c in CASES for kind in ("i32", "lp"))
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert all(golden[f"{c}/i32"].dtype == np.int32 and golden[f"{c}/lp"].dtype == np.uint32
               for c in CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bits(ops, dev, golden, case):
    fields = CASES[case](ops, dev)
    want = {np.dtype(np.int32): golden[case + "/i32"], np.dtype(np.uint32): golden[case + "/lp"]}
    at = {k: 0 for k in want}
    for name, a in fields:                       # field by field, so that a failure names one
        w = want[a.dtype][at[a.dtype]:at[a.dtype] + a.size]
        at[a.dtype] += a.size
        assert np.array_equal(a.reshape(-1), w), (case, name)
    assert all(at[k] == want[k].size for k in want), case


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_sampler_bits_gpu.py --write   (on the GPU)")
    from importlib import import_module
    from conftest import PKG_DIR
    if not torch.cuda.is_available():
        raise SystemExit("the fixture is written on the GPU (no CPU path)")
    _ops, _dev, _out = import_module(PKG_DIR + ".ops"), torch.device("cuda:0"), {}
    for _case in sorted(CASES):
        _out[_case + "/i32"], _out[_case + "/lp"] = pack(CASES[_case](_ops, _dev))
    np.savez_compressed(FIXTURE, **_out)
    print(f"wrote {FIXTURE}: {len(CASES)} cases, {os.path.getsize(FIXTURE)} bytes")
