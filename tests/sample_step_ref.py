"""Plain-Python restatement of cs_sample_step's state machine (include/consensus_scoring.h).

The draw itself is a callable passed in: ``draw(t) -> (ids, lps)``, one entry per stream.
The CPU tests script it; the GPU tests pass ``vocab_sample_draw``: ops.vocab_sample on the
fp32 rows with the bias added by indexed assignment (runtime.apply_bias: duplicates count
once), seeded with draw_seed(base, t).
"""
from __future__ import annotations

M64 = (1 << 64) - 1
SEED_MUL = 1000003


def seed_of(base: int, t: int) -> int:
    """(base * 1000003 + t) mod 2^64 on Python integers."""
    return (int(base) * SEED_MUL + int(t)) % (1 << 64)


def as_i64(u: int) -> int:
    u &= M64
    return u - (1 << 64) if u >> 63 else u


class StepState:
    """done / out_len / out_tokens / out_lp / next_tok / n_alive of S streams."""

    def __init__(self, S: int, max_tokens: int, pad_id: int, stop_ids=(), done=None,
                 sentinel_tok: int = -7, sentinel_lp: float = -777.0):
        self.S, self.max_tokens, self.pad_id = S, max_tokens, pad_id
        self.stop = set(int(s) for s in stop_ids)
        self.done = [0] * S if done is None else [int(d) for d in done]
        self.out_len = [0] * S
        self.out_tokens = [[sentinel_tok] * max_tokens for _ in range(S)]
        self.out_lp = [[sentinel_lp] * max_tokens for _ in range(S)]
        self.next_tok = [None] * S      # unwritten until the first step
        self.n_alive = None

    def step(self, t: int, draw) -> None:
        ids, lps = draw(t)
        for s in range(self.S):
            if self.done[s]:
                self.next_tok[s] = self.pad_id
                continue
            i = int(ids[s])
            if i == -1 or i in self.stop:
                self.done[s] = 1
            else:
                n = self.out_len[s]
                self.out_tokens[s][n] = i
                self.out_lp[s][n] = float(lps[s])
                self.out_len[s] = n + 1
                if n + 1 == self.max_tokens:
                    self.done[s] = 1
            self.next_tok[s] = self.pad_id if self.done[s] else i
        self.n_alive = sum(1 for d in self.done if not d)

    def sequences(self):
        return [self.out_tokens[s][:self.out_len[s]] for s in range(self.S)]


def vocab_sample_draw(ops, logits, base_seeds, *, temperature=1.0, softcap=0.0, bias_ids=(),
                      bias_value=0.0, vocab=None):
    """draw(t) for StepState.step on the GPU: ops.vocab_sample of every row (the row count
    is the kernel's, so both split the vocabulary alike) on the fp32 copy with the bias added
    by indexed assignment; ids outside [0, vocab) are dropped as the kernel ignores them."""
    import torch

    V = logits.shape[1] if vocab is None else vocab
    rows = logits.float().clone()
    keep = [int(i) for i in bias_ids if 0 <= int(i) < V]
    if keep:
        idx = torch.as_tensor(keep, dtype=torch.long, device=rows.device)
        rows[:, idx] = rows[:, idx] + bias_value
    base = [int(b) & M64 for b in base_seeds]

    def draw(t):
        sd = torch.tensor([[as_i64(seed_of(b, t))] for b in base], dtype=torch.int64,
                          device=rows.device)
        ids, lp = ops.vocab_sample(rows, sd, temperature=temperature, softcap=softcap, vocab=V)
        return ids[:, 0].tolist(), lp[:, 0].tolist()

    return draw
