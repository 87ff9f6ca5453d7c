"""NumPy / plain-Python restatement of the constrained sampling contract
(include/consensus_scoring.h: cs_dfa_token_masks, cs_vocab_sample_dfa, cs_sample_step_dfa):
the token-mask rule, the set of tokens a state allows, the state walk of an appended token and
the step's state machine with the automaton state beside it.

The draw itself stays a callable, as in tests/sample_step_ref.py: the GPU tests pass the
EXISTING draw (ops.vocab_sample / ops.vocab_sample_ex without masks) on rows whose forbidden
tokens were set to -inf after the row transform, so the constrained entries are pinned bit
for bit to the unconstrained ones.
"""
from __future__ import annotations

import numpy as np

from sample_controls_ref import ControlState


def walk(trans: np.ndarray, q: int, data: bytes) -> int:
    """The state after ``data`` from q; -1 once a byte is dead or q is no state."""
    n = trans.shape[0]
    for b in bytes(data):
        if not 0 <= q < n:
            return -1
        q = int(trans[q, b])
    return q if 0 <= q < n else -1


def token_masks(trans: np.ndarray, accept: np.ndarray, tok_bytes, stop_ids=()) -> np.ndarray:
    """uint32 [n_states, ceil(vocab / 32)]: bit (q, v) set iff token v has at least one byte
    and its bytes walked from q never die; for a listed stop id the bit is accept[q]; bits
    past the vocabulary are 0."""
    n, vocab = trans.shape[0], len(tok_bytes)
    # every state walks every DISTINCT byte string at once, one byte position per round
    distinct = sorted(set(bytes(b) for b in tok_bytes))
    index = {b: k for k, b in enumerate(distinct)}
    lens = np.asarray([len(b) for b in distinct])
    grid = np.zeros((len(distinct), max(1, int(lens.max()))), dtype=np.int64)
    for k, b in enumerate(distinct):
        grid[k, :len(b)] = list(b)
    table = np.concatenate([trans.astype(np.int64), np.full((1, 256), -1)])   # row -1: dead
    table[(table < 0) | (table >= n)] = -1
    q = np.repeat(np.arange(n)[:, None], len(distinct), axis=1)
    for j in range(grid.shape[1]):
        q = np.where(j < lens, table[q, grid[:, j]], q)
    alive = (q >= 0) & (lens > 0)
    bits = np.zeros((n, (vocab + 31) // 32 * 32), dtype=bool)
    bits[:, :vocab] = alive[:, [index[bytes(b)] for b in tok_bytes]]
    for v in {int(i) for i in stop_ids}:
        if 0 <= v < vocab:
            bits[:, v] = np.asarray(accept, dtype=bool)
    packed = np.packbits(bits.reshape(n, -1, 32), axis=-1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4").reshape(n, -1)


def allowed(masks: np.ndarray, q: int, vocab: int) -> np.ndarray:
    """bool [vocab]: the tokens state q may draw (none if q is no state)."""
    if not 0 <= q < masks.shape[0]:
        return np.zeros(vocab, dtype=bool)
    bits = np.unpackbits(np.ascontiguousarray(masks[q]).view(np.uint8), bitorder="little")
    return bits[:vocab].astype(bool)


class DfaState(ControlState):
    """ControlState plus one automaton state per stream, advanced by every appended token."""

    def __init__(self, S, max_tokens, pad_id, *, trans, starts, tok_bytes, **kw):
        super().__init__(S, max_tokens, pad_id, tok_bytes=tok_bytes, **kw)
        self.trans = trans
        self.dfa_state = [int(q) for q in starts]

    def step(self, t: int, draw) -> None:
        before = list(self.out_len)
        was_done = list(self.done)
        super().step(t, draw)
        for s in range(self.S):
            if was_done[s] or self.out_len[s] == before[s]:
                continue
            tok = self.out_tokens[s][before[s]]
            if len(self.tok_bytes[tok]):
                self.dfa_state[s] = walk(self.trans, self.dfa_state[s], self.tok_bytes[tok])
