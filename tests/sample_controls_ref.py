"""Plain-Python / numpy restatement of what cs_vocab_sample_ex and cs_sample_step_ex add to
their siblings (include/consensus_scoring.h): the row transform (bias, soft-cap, repetition
penalty), the greedy draw, the stop-string window and the step's state machine with it.

The fp32 pieces restate the kernel's arithmetic operation for operation (numpy float32 is
IEEE: the division is correctly rounded); the ``*64`` pieces are the fp64 statement of the
same contract, for the cases where a soft-cap's tanh keeps the fp32 bits from being pinned.
"""
from __future__ import annotations

import numpy as np

from sample_step_ref import StepState

TAIL_MAX = 31          # bytes of window kept between steps (one less than the longest stop string)
MAX_STOP_SEQ, MAX_STOP_LEN = 8, 32


def seen_mask(vocab: int, seen) -> np.ndarray:
    """bool [vocab]: the seen set; ids outside [0, vocab) are ignored, duplicates count once."""
    m = np.zeros(vocab, dtype=bool)
    for i in seen:
        if 0 <= int(i) < vocab:
            m[int(i)] = True
    return m


def penalise(x: np.ndarray, seen, penalty: float) -> np.ndarray:
    """The penalty rule on a row, in the row's own dtype (float32: the kernel's bits)."""
    x = np.array(x, copy=True)
    if penalty == 1.0:
        return x
    m = seen_mask(x.shape[0], seen)
    p = x.dtype.type(penalty)
    with np.errstate(invalid="ignore", over="ignore"):
        x[m] = np.where(x[m] < 0, x[m] * p, x[m] / p)
    return x


def transform(x: np.ndarray, *, bias_ids=(), bias_value=0.0, softcap=0.0, seen=(), penalty=1.0,
              dtype=np.float64) -> np.ndarray:
    """The transformed row in ``dtype``: bias (once per listed token), soft-cap, penalty."""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    b = seen_mask(x.shape[0], bias_ids)
    with np.errstate(invalid="ignore", over="ignore"):
        x[b] = x[b] + dtype(bias_value)
        if softcap > 0.0:
            x = (dtype(softcap) * np.tanh(x / dtype(softcap))).astype(dtype)
    return penalise(x, seen, penalty)


def log_softmax_at(x: np.ndarray, i: int) -> float:
    """fp64 log-probability of token i under softmax(x); NaN if the row holds a NaN."""
    x = np.asarray(x, dtype=np.float64)
    if i < 0 or np.isnan(x).any():
        return float("nan")
    ok = x != -np.inf
    mx = x[ok].max()
    with np.errstate(over="ignore"):
        return float(x[i] - (mx + np.log(np.exp(x[ok] - mx).sum())))


def greedy(x: np.ndarray):
    """(id, fp64 log-prob at temperature 1) of the greedy draw on a transformed row: numpy's
    first-index argmax over the drawable tokens (not -inf, not NaN); (-1, NaN) if there is none."""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x) & (x != -np.inf)
    if not ok.any():
        return -1, float("nan")
    i = int(np.argmax(np.where(ok, x, -np.inf)))
    return i, log_softmax_at(x, i)


def gumbel64(x: np.ndarray, seed: int, temperature: float):
    """(id, log-prob, gap to the runner-up, largest magnitude) of the Gumbel-max draw on a
    transformed fp64 row, with the product's counter-based uniforms (oracle.cs_uniform)."""
    import oracle

    x = np.asarray(x, dtype=np.float64)
    y = x / temperature
    ok = ~np.isnan(y) & (y != -np.inf)
    u = oracle.cs_uniform(seed, np.arange(y.shape[0])).astype(np.float64)
    g = -np.log(-np.log(u))
    s = np.where(ok, y + g, -np.inf)
    if not ok.any():
        return -1, float("nan"), float("nan"), 1.0
    i = int(np.argmax(s))
    rest = np.delete(s, i)
    gap = float(s[i] - rest.max()) if rest.size else float("inf")
    scale = max(1.0, float(np.abs(y[ok]).max()), float(np.abs(g[ok]).max()))
    return i, log_softmax_at(y, i), gap, scale


class StopWindow:
    """The per-stream byte window of cs_sample_step_ex."""

    def __init__(self, stops):
        self.stops = [bytes(s) for s in stops]
        assert len(self.stops) <= MAX_STOP_SEQ
        assert all(1 <= len(s) <= MAX_STOP_LEN for s in self.stops)
        self.tail = b""

    def push(self, tok: bytes) -> bool:
        """Append a token's bytes; True if a stop string occurs in tail ++ tok ending inside
        tok.  The tail becomes the last min(31, len) bytes.  No bytes: nothing changes."""
        if not tok:
            return False
        w = self.tail + bytes(tok)
        hit = False
        for e in range(len(self.tail) + 1, len(w) + 1):        # e: one past the last byte
            for s in self.stops:
                if len(s) <= e and w[e - len(s):e] == s:
                    hit = True
        self.tail = w[-TAIL_MAX:]
        return hit


class ControlState(StepState):
    """StepState plus the stop-string window: ``tok_bytes[v]`` are token v's bytes."""

    def __init__(self, S, max_tokens, pad_id, *, tok_bytes=None, stop_seqs=(), **kw):
        super().__init__(S, max_tokens, pad_id, **kw)
        self.tok_bytes = tok_bytes
        self.win = [StopWindow(stop_seqs) for _ in range(S)]
        self.has_stop = len(stop_seqs) > 0

    def step(self, t: int, draw) -> None:
        before = list(self.out_len)
        was_done = list(self.done)
        super().step(t, draw)
        if not self.has_stop:
            return
        for s in range(self.S):
            if was_done[s] or self.out_len[s] == before[s]:
                continue                                    # nothing appended: the window stands
            tok = self.out_tokens[s][before[s]]
            if self.win[s].push(self.tok_bytes[tok]):
                self.done[s] = 1
                self.next_tok[s] = self.pad_id
        self.n_alive = sum(1 for d in self.done if not d)

    def tails(self):
        """(tail [S][32] zero-padded lists, tail_len [S]) as the device holds them; bytes past
        tail_len are not compared by the tests."""
        return [list(w.tail) for w in self.win], [len(w.tail) for w in self.win]


def first_stop_step(tok_bytes, ids, stops):
    """From the decoded text alone: the index of the token that completes the first
    occurrence (by its end) of any stop string, or None.  Tokens are ASCII here, so the text
    is the concatenation of their strings and str.find sees what the bytes hold."""
    text = "".join(tok_bytes[i].decode("ascii") for i in ids)
    ends = []
    for s in stops:
        at = text.find(s.decode("ascii"))
        if at >= 0:
            ends.append(at + len(s))
    if not ends:
        return None
    end, n = min(ends), 0
    for k, i in enumerate(ids):
        n += len(tok_bytes[i])
        if n >= end:
            return k
    raise AssertionError("unreachable")


def run_window(tok_bytes, ids, stops):
    """The step at which the restatement's window ends a stream fed ``ids``, or None."""
    w = StopWindow(stops)
    for k, i in enumerate(ids):
        if w.push(tok_bytes[i]):
            return k
    return None


def ragged(lists):
    """(ids, offsets) int32 arrays of a list of per-row id lists."""
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in lists])
    flat = np.asarray([int(i) for r in lists for i in r], dtype=np.int32)
    return flat, off
