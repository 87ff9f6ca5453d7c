"""Torch-tensor front end of the C-ABI (``include/consensus_scoring.h``).

Every function here launches a hand-written gfx950 kernel through
``libconsensus_scoring.so`` on torch's *current* HIP stream and returns device
tensors.  Inputs must already live on the GPU; nothing is copied to the host and
nothing falls back to a CPU path (a missing library raises ``CSError``).

Reference semantics each op restates are cited on the op.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import json
import operator
import os
import threading
import time
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import CSError

WELFARE = {"min": _lib.WELFARE_MIN, "egalitarian": _lib.WELFARE_MIN,
           "sum": _lib.WELFARE_SUM, "utilitarian": _lib.WELFARE_SUM,
           "sumlog": _lib.WELFARE_SUMLOG, "nash": _lib.WELFARE_SUMLOG,
           "max": _lib.WELFARE_MAX}

# CS_DEBUG_TABLES=1: the row-layout history's slot tables are checked on the host against
# the K / V buffer they index before every (uncaptured) launch that reads them (read once)
_DEBUG_TABLES = os.environ.get("CS_DEBUG_TABLES") == "1"
_DTYPE = {torch.float32: _lib.CS_F32, torch.bfloat16: _lib.CS_BF16, torch.float16: _lib.CS_F16}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """The tensor's address; None or an empty tensor gives NULL."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def default_device(who: str) -> torch.device:
    """The current HIP device; without one, CSError(who): there is no CPU path."""
    if not torch.cuda.is_available():
        raise CSError(who)
    return torch.device("cuda", torch.cuda.current_device())


def _require_cuda(*ts: torch.Tensor) -> None:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise CSError("consensus_scoring ops take device tensors (got a CPU tensor); "
                          "there is no CPU path")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise CSError(f"tensors on different devices: {dev} vs {t.device}")


class Workspace:
    """Grow-only device scratch for split-V partials (allocation happens here, never
    inside a launch, so a captured graph can reuse a pre-sized workspace).

    ``zeroed=True`` allocates zero-filled memory: cs_beam_step keeps arrival counters in
    its workspace that must start at zero (every call leaves them at zero again)."""

    def __init__(self, zeroed: bool = False) -> None:
        self.buf: Optional[torch.Tensor] = None
        self.zeroed = zeroed

    def get(self, nbytes: int, device: torch.device) -> Optional[torch.Tensor]:
        if nbytes == 0:
            return None
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            alloc = torch.zeros if self.zeroed else torch.empty
            self.buf = alloc(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return self.buf

    def reset(self) -> None:
        """Zero a zeroed workspace again (its arrival counters), e.g. after a failed launch
        that may have stopped with counters half-counted."""
        if self.zeroed and self.buf is not None and not torch.cuda.is_current_stream_capturing():
            self.buf.zero_()


_default_ws: dict = {}
_beam_ws: dict = {}
_decode_ws: dict = {}


def _workspace_args(workspace: Optional[Workspace], pool: dict, nbytes: int, device: torch.device,
                    counters_of: Optional[str] = None):
    """The workspace arguments of an entry point: (workspace, pointer or None, byte size), from
    the caller's Workspace or the device's default in ``pool``.  ``counters_of`` names an op that
    keeps arrival counters there and so needs a zeroed Workspace."""
    if workspace is None:
        workspace = pool.setdefault(device, Workspace(zeroed=counters_of is not None))
    if counters_of is not None and not workspace.zeroed:
        raise CSError(f"{counters_of} needs a Workspace(zeroed=True) of its own (arrival counters)")
    buf = workspace.get(nbytes, device)
    if buf is None:
        return workspace, None, 0
    return workspace, buf.data_ptr(), buf.numel()


def _logits_args(logits: torch.Tensor, vocab: Optional[int]):
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise CSError("logits must be 2-D with unit column stride")
    if logits.dtype not in _DTYPE:
        raise CSError(f"unsupported logits dtype {logits.dtype}")
    rows = logits.shape[0]
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    vocab = logits.shape[1] if vocab is None else int(vocab)
    if vocab > logits.shape[1]:
        raise CSError("vocab exceeds logits width")
    return rows, ld, vocab


def workspace_size(rows: int, vocab: int, k: int = 1) -> int:
    return int(_lib.load().cs_workspace_size(rows, vocab, k))


def logsoftmax_gather(logits: torch.Tensor, targets: Optional[torch.Tensor], *, vocab: Optional[int] = None,
                      softcap: float = 0.0, out: Optional[torch.Tensor] = None,
                      lse_out: Optional[torch.Tensor] = None, want_lse: bool = False,
                      workspace: Optional[Workspace] = None):
    """Fused log-softmax over the vocab + gather at ``targets``.

    logits  [rows, ld] bf16/f16/f32 with unit column stride (only the first
            ``vocab`` columns are used); targets [rows, k] int32 (ids outside
            [0, vocab) give NaN, the reference's ``None``).
    Returns (tok_lp [rows, k] f32, lse [rows] f32 or None).

    Restates: remote echo=True prompt log-probs read by get_prompt_logprobs
    (src/utils.py:249-263); core.log_softmax_rows + gather (core.py:64-68, 89-90).
    """
    L = _lib.load()
    rows, ld, vocab = _logits_args(logits, vocab)
    if targets is None:
        k = 0
        targets = torch.empty((rows, 0), dtype=torch.int32, device=logits.device)
    else:
        if targets.dtype != torch.int32:
            raise CSError("targets must be int32")
        if targets.dim() != 2 or targets.shape[0] != rows:
            if rows == 0 or targets.numel() % rows != 0:
                raise CSError("targets must be [rows, k]")
            targets = targets.reshape(rows, -1)
        if not targets.is_contiguous():
            targets = targets.contiguous()
        k = targets.shape[1]
    _require_cuda(logits, targets, out, lse_out)
    if out is None:
        out = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * k:
        raise CSError("out must be contiguous float32 with rows*k elements")
    if lse_out is None and want_lse:
        lse_out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _, ws_ptr, ws_bytes = _workspace_args(workspace, _default_ws, workspace_size(rows, vocab, k),
                                          logits.device)
    rc = L.cs_logsoftmax_gather(
        logits.data_ptr(), _DTYPE[logits.dtype], rows, vocab, ld,
        targets.data_ptr() if k else None, k, float(softcap), out.data_ptr() if k else None,
        lse_out.data_ptr() if lse_out is not None else None, ws_ptr, ws_bytes, _stream())
    _lib.check(rc, "cs_logsoftmax_gather")
    return out, lse_out


def segment_reduce(tok_lp: torch.Tensor, offsets: torch.Tensor):
    """Per-segment Σlp, Σexp(lp), count of non-NaN, last value (fp64 accumulation).

    Restates best_of_n.py:303-305, finite_lookahead.py:508-520, evaluation.py:203-213,
    beam_search.py:389-390 and core.py:90.
    """
    L = _lib.load()
    tok = tok_lp.reshape(-1)
    if tok.dtype != torch.float32 or not tok.is_contiguous():
        raise CSError("tok_lp must be contiguous float32")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or not offsets.is_contiguous():
        raise CSError("offsets must be a contiguous 1-D int32 tensor")
    _require_cuda(tok, offsets)
    n_seg = offsets.numel() - 1
    dev = tok.device
    sum_lp = torch.empty(n_seg, dtype=torch.float32, device=dev)
    sum_p = torch.empty(n_seg, dtype=torch.float32, device=dev)
    cnt = torch.empty(n_seg, dtype=torch.int32, device=dev)
    last = torch.empty(n_seg, dtype=torch.float32, device=dev)
    rc = L.cs_segment_reduce(tok.data_ptr(), tok.numel(), offsets.data_ptr(), n_seg,
                             sum_lp.data_ptr(), sum_p.data_ptr(), cnt.data_ptr(), last.data_ptr(),
                             _stream())
    _lib.check(rc, "cs_segment_reduce")
    return {"sum_lp": sum_lp, "sum_p": sum_p, "count": cnt, "last": last}


def welfare(U: torch.Tensor, kind, *, eps: float = 1e-9, nonfinite: str = "skip",
            nan_val: float = -10.0, posinf_val: float = 20.0, neginf_val: float = -20.0,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Welfare over agents (rows of U [A, C]) for every candidate column.

    kind: 'min'|'egalitarian', 'sum'|'utilitarian', 'sumlog'|'nash', 'max'.
    Restates evaluation.py:337-381, beam_search.py:558-560, best_of_n.py:384-408,
    core.py:108-113 (point mass) and core.py:374.
    """
    L = _lib.load()
    if isinstance(kind, str):
        kind = WELFARE[kind]
    if U.dim() != 2 or U.dtype != torch.float32 or (U.stride(1) != 1 and U.shape[1] > 1):
        raise CSError("U must be 2-D float32 with unit column stride")
    _require_cuda(U, out)
    A, C = U.shape
    ldu = U.stride(0) if A > 1 else C
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=U.device)
    mode = {"skip": _lib.NONFINITE_SKIP, "replace": _lib.NONFINITE_REPLACE}[nonfinite]
    rc = L.cs_welfare_reduce(U.data_ptr(), A, C, ldu, int(kind), float(eps), mode, float(nan_val),
                             float(posinf_val), float(neginf_val), out.data_ptr(), _stream())
    _lib.check(rc, "cs_welfare_reduce")
    return out


def topk(W: torch.Tensor, k: int, *, with_values: bool = True):
    """Stable descending top-k per row of W [n_seg, seg_len] (value desc, index asc;
    NaN last).  Restates beam_search.py:558-560 (stable sorted, reverse=True),
    best_of_n.py:198 (np.argmax) and finite_lookahead.py:527 (max, first wins)."""
    L = _lib.load()
    W2 = W.reshape(1, -1) if W.dim() == 1 else W
    if W2.dim() != 2 or W2.dtype != torch.float32 or W2.stride(1) != 1:
        raise CSError("W must be float32 with unit column stride")
    _require_cuda(W2)
    n_seg, seg_len = W2.shape
    ld = W2.stride(0) if n_seg > 1 else seg_len
    idx = torch.empty((n_seg, k), dtype=torch.int32, device=W.device)
    val = torch.empty((n_seg, k), dtype=torch.float32, device=W.device) if with_values else None
    rc = L.cs_segmented_topk(W2.data_ptr(), n_seg, seg_len, ld, int(k), idx.data_ptr(),
                             val.data_ptr() if val is not None else None, _stream())
    _lib.check(rc, "cs_segmented_topk")
    if W.dim() == 1:
        return idx[0], (val[0] if val is not None else None)
    return idx, val


UNFILL = {None: 0, "none": 0, "+inf": 1, "min": 1, "-inf": 2, "max": 2}


def beam_select(W: torch.Tensor, n_order: int, *, U: Optional[torch.Tensor] = None,
                unfill=None, kept_out: Optional[torch.Tensor] = None, W_out: Optional[torch.Tensor] = None,
                with_values: bool = False):
    """Selection half of an agent-sharded beam step, one launch (cs_beam_select).

    W [C] float32 all-reduced welfare (C <= 1024); unfill '+inf'/'min' maps +inf back to
    NaN (the MIN combine's fill for columns without a usable utility), '-inf'/'max' -inf.
    Returns (order [n_order] int32 by (W desc, index asc), NaN last; values or None).
    With U [A, C] (this rank's agents) and kept_out [A, n_order]: kept_out[a, r] =
    U[a, order[r]], the kept beams' cumulative rewards.  W_out (nullable) receives W after
    unfill.  Bit-identical to topk(W) + U.index_select(1, order).
    Restates the stable sort + keep of beam_search.py:558-593 on one agent shard."""
    L = _lib.load()
    if W.dim() != 1 or W.dtype != torch.float32 or not W.is_contiguous():
        raise CSError("W must be a contiguous 1-D float32 tensor")
    _require_cuda(W)
    C = W.shape[0]
    A = 0
    if kept_out is not None:
        if U is None or U.dtype != torch.float32 or not U.is_contiguous() or U.dim() != 2 \
                or U.shape[1] != C:
            raise CSError("kept_out needs U [A, C] contiguous float32")
        A = U.shape[0]
        if kept_out.shape != (A, n_order) or kept_out.dtype != torch.float32 \
                or not kept_out.is_contiguous():
            raise CSError("kept_out must be [A, n_order] contiguous float32")
    order = torch.empty(n_order, dtype=torch.int32, device=W.device)
    val = torch.empty(n_order, dtype=torch.float32, device=W.device) if with_values else None
    rc = L.cs_beam_select(W.data_ptr(), C, UNFILL[unfill], U.data_ptr() if A else None, A,
                          int(n_order), W_out.data_ptr() if W_out is not None else None,
                          order.data_ptr(), val.data_ptr() if val is not None else None,
                          kept_out.data_ptr() if kept_out is not None else None, _stream())
    _lib.check(rc, "cs_beam_select")
    return order, val


def _beam_outputs(A: int, C: int, n_order: int, dev: torch.device, out_U, out_W, kept_out,
                  out_order=None):
    """(U, W, order, order_val) of a beam step: the caller's tensors, validated, or new ones."""
    U = torch.empty((A, C), dtype=torch.float32, device=dev) if out_U is None else out_U
    W = torch.empty(C, dtype=torch.float32, device=dev) if out_W is None else out_W
    if (U.shape != (A, C) or W.shape != (C,) or U.dtype != torch.float32 or
            W.dtype != torch.float32 or not U.is_contiguous() or not W.is_contiguous()):
        raise CSError(f"out_U / out_W must be contiguous float32 [{A}, {C}] / [{C}]")
    order = (torch.empty(max(n_order, 0), dtype=torch.int32, device=dev) if out_order is None
             else out_order)
    if order.shape != (max(n_order, 0),) or order.dtype != torch.int32 or not order.is_contiguous():
        raise CSError(f"out_order must be a contiguous int32 [{n_order}] tensor")
    oval = torch.empty(max(n_order, 0), dtype=torch.float32, device=dev)
    if kept_out is not None:
        if (kept_out.dtype != torch.float32 or not kept_out.is_contiguous()
                or tuple(kept_out.shape) != (A, n_order)):
            raise CSError(f"kept_out must be a contiguous float32 [{A}, {n_order}] tensor")
        _require_cuda(kept_out)
    return U, W, order, oval


def beam_step(logits: torch.Tensor, targets: torch.Tensor, rewards: torch.Tensor, kind="min", *,
              n_order: Optional[int] = None, vocab: Optional[int] = None, softcap: float = 0.0,
              eps: float = 1e-9, workspace: Optional[Workspace] = None,
              kept_out: Optional[torch.Tensor] = None,
              out_U: Optional[torch.Tensor] = None, out_W: Optional[torch.Tensor] = None):
    """One beam-search scoring step after the LM head, fused into one launch.

    logits  [A*B, ld] agent rows (row a*B + b = agent a, beam b);
    targets [B, K] int32 candidate tokens per beam (ids outside [0, vocab) = padding);
    rewards [A, B] float32 cumulative per-agent rewards of the beams.
    Returns (U [A, B*K], W [B*K], order [n_order] int32, order_val [n_order]) with
    U = rewards + log p(token), W = welfare over agents, order = stable descending
    (n_order defaults to B*K; 0 skips the sort and returns (U, W, None, None); up to 256
    the launch selects the n_order best without sorting the rest).
    kept_out [A, n_order] float32 (optional) receives U[:, order]: the cumulative rewards
    of the kept beams when the first n_order ranks are kept (B*K <= 1024).

    Restates beam_search.py:495-560 (per-candidate agent log-probs :335-404,
    cumulative rewards :534-536, stable sort by min over agents :558-560).
    """
    L = _lib.load()
    rows, ld, vocab = _logits_args(logits, vocab)
    if targets.dim() != 2 or targets.dtype != torch.int32:
        raise CSError("targets must be [B, K] int32")
    if rewards.dim() != 2 or rewards.dtype != torch.float32:
        raise CSError("rewards must be [A, B] float32")
    targets, rewards = targets.contiguous(), rewards.contiguous()
    A, B = rewards.shape
    K = targets.shape[1]
    if targets.shape[0] != B or rows != A * B:
        raise CSError(f"shape mismatch: logits rows {rows}, rewards {tuple(rewards.shape)}, "
                      f"targets {tuple(targets.shape)}")
    _require_cuda(logits, targets, rewards)
    if isinstance(kind, str):
        kind = WELFARE[kind]
    C = B * K
    n_order = C if n_order is None else int(n_order)
    dev = logits.device
    U, W, order, oval = _beam_outputs(A, C, n_order, dev, out_U, out_W, kept_out)
    workspace, ws_ptr, ws_bytes = _workspace_args(
        workspace, _beam_ws, int(L.cs_beam_step_workspace_size(rows, vocab)), dev, "beam_step")
    rc = L.cs_beam_step(logits.data_ptr(), _DTYPE[logits.dtype], A, B, vocab, ld,
                        targets.data_ptr(), K, rewards.data_ptr(), float(softcap), int(kind),
                        float(eps), U.data_ptr(), W.data_ptr(), n_order,
                        order.data_ptr() if n_order else None, oval.data_ptr() if n_order else None,
                        kept_out.data_ptr() if kept_out is not None else None,
                        ws_ptr, ws_bytes, _stream())
    if rc != 0:
        workspace.reset()
    _lib.check(rc, "cs_beam_step")
    if n_order == 0:
        return U, W, None, None
    return U, W, order, oval


def beam_decode_step(ref_logits: torch.Tensor, logits: torch.Tensor, rewards: torch.Tensor,
                     k: int, kind="min", *, n_order: Optional[int] = None,
                     vocab: Optional[int] = None, softcap: float = 0.0, eps: float = 1e-9,
                     workspace: Optional[Workspace] = None,
                     kept_out: Optional[torch.Tensor] = None,
                     out_U: Optional[torch.Tensor] = None, out_W: Optional[torch.Tensor] = None,
                     out_ids: Optional[torch.Tensor] = None,
                     out_order: Optional[torch.Tensor] = None):
    """Proposer + scoring of one beam decode step in ONE launch (cs_beam_decode_step).

    ref_logits [B, ld_ref] reference-policy rows; logits [A*B, ld] agent rows (row a*B+b);
    rewards [A, B] float32.  Returns (ids [B, k] int32, U [A, B*k], W [B*k], order, order_val)
    — identical to ``ids, _ = vocab_topk(ref_logits, k)`` followed by
    ``beam_step(logits, ids, rewards, ...)``.  Restates beam_search.py:439-560.
    """
    L = _lib.load()
    rows, ld, vocab = _logits_args(logits, vocab)
    B_ref, ld_ref, _ = _logits_args(ref_logits, vocab)
    if rewards.dim() != 2 or rewards.dtype != torch.float32:
        raise CSError("rewards must be [A, B] float32")
    if ref_logits.dtype != logits.dtype:
        raise CSError("ref_logits and logits must share a dtype")
    rewards = rewards.contiguous()
    A, B = rewards.shape
    if B_ref != B or rows != A * B:
        raise CSError(f"shape mismatch: ref rows {B_ref}, agent rows {rows}, rewards {tuple(rewards.shape)}")
    _require_cuda(ref_logits, logits, rewards, out_ids, out_order)
    if isinstance(kind, str):
        kind = WELFARE[kind]
    k = int(k)
    C = B * k
    n_order = C if n_order is None else int(n_order)
    dev = logits.device
    ids = torch.empty((B, k), dtype=torch.int32, device=dev) if out_ids is None else out_ids
    if ids.shape != (B, k) or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise CSError(f"out_ids must be a contiguous int32 [{B}, {k}] tensor")
    U, W, order, oval = _beam_outputs(A, C, n_order, dev, out_U, out_W, kept_out, out_order)
    workspace, ws_ptr, ws_bytes = _workspace_args(
        workspace, _decode_ws, int(L.cs_beam_decode_workspace_size(A, B, vocab, k)), dev,
        "beam_decode_step")
    rc = L.cs_beam_decode_step(ref_logits.data_ptr(), ld_ref, logits.data_ptr(), ld,
                               _DTYPE[logits.dtype], A, B, vocab, k, float(softcap),
                               rewards.data_ptr(), int(kind), float(eps), ids.data_ptr(),
                               U.data_ptr(), W.data_ptr(), n_order,
                               order.data_ptr() if n_order else None,
                               oval.data_ptr() if n_order else None,
                               kept_out.data_ptr() if kept_out is not None else None,
                               ws_ptr, ws_bytes, _stream())
    if rc != 0:
        workspace.reset()
    _lib.check(rc, "cs_beam_decode_step")
    if n_order == 0:
        return ids, U, W, None, None
    return ids, U, W, order, oval


def vocab_topk(logits: torch.Tensor, k: int, *, vocab: Optional[int] = None, softcap: float = 0.0,
               workspace: Optional[Workspace] = None):
    """Top-k token ids (value desc, id asc) of every logits row -> (ids [rows, k] int32,
    values [rows, k] f32).  The deterministic beam-candidate proposer replacing the
    reference's repeated one-token sampling (beam_search.py:199-333)."""
    L = _lib.load()
    rows, ld, vocab = _logits_args(logits, vocab)
    _require_cuda(logits)
    ids = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    vals = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    _, ws_ptr, ws_bytes = _workspace_args(workspace, _default_ws,
                                          int(L.cs_vocab_topk_workspace_size(rows, vocab, k)),
                                          logits.device)
    rc = L.cs_vocab_topk(logits.data_ptr(), _DTYPE[logits.dtype], rows, vocab, ld, int(k),
                         float(softcap), ids.data_ptr(), vals.data_ptr(), ws_ptr, ws_bytes, _stream())
    _lib.check(rc, "cs_vocab_topk")
    return ids, vals


def _vocab_sample(entry: str, logits, seeds, n_draw, temperature, vocab, softcap, workspace,
                  lists=(), controls=lambda rows: ()):
    """The body of vocab_sample and vocab_sample_ex around the C entry point ``entry``:
    ``controls(rows)`` gives the arguments that entry takes between n_draw and out_ids, from
    the device tensors ``lists``."""
    L = _lib.load()
    rows, ld, vocab = _logits_args(logits, vocab)
    if seeds is None:
        n_draw = 1 if n_draw is None else int(n_draw)
    else:
        seeds = seeds.reshape(rows, -1)
        if seeds.dtype != torch.int64 or not seeds.is_contiguous():
            raise CSError("seeds must be a contiguous int64 tensor [rows, n_draw]")
        n_draw = seeds.shape[1]
    _require_cuda(logits, seeds, *lists)
    extra = controls(rows)
    ids = torch.empty((rows, n_draw), dtype=torch.int32, device=logits.device)
    lp = torch.empty((rows, n_draw), dtype=torch.float32, device=logits.device)
    _, ws_ptr, ws_bytes = _workspace_args(
        workspace, _default_ws, int(getattr(L, entry + "_workspace_size")(rows, vocab, n_draw)),
        logits.device)
    rc = getattr(L, entry)(logits.data_ptr(), _DTYPE[logits.dtype], rows, vocab, ld,
                           float(temperature), float(softcap), _ptr(seeds), n_draw, *extra,
                           ids.data_ptr(), lp.data_ptr(), ws_ptr, ws_bytes, _stream())
    _lib.check(rc, entry)
    return ids, lp


def vocab_sample(logits: torch.Tensor, seeds: torch.Tensor, *, temperature: float = 1.0,
                 vocab: Optional[int] = None, softcap: float = 0.0,
                 workspace: Optional[Workspace] = None):
    """Seeded Gumbel-max draws: seeds [rows, n_draw] int64 (bit pattern used as uint64) ->
    (ids [rows, n_draw] int32, log-probs [rows, n_draw] f32)."""
    return _vocab_sample("cs_vocab_sample", logits, seeds, None, temperature, vocab, softcap,
                         workspace)


_sample_ws: dict = {}


def _state_ptr(t: Optional[torch.Tensor], name: str, dtype: torch.dtype, shape: tuple):
    """Pointer of one of sample_step's state tensors (None stays NULL for the library to judge)."""
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise CSError(f"{name} must be a contiguous {dtype} tensor of shape {list(shape)}")
    return t.data_ptr()


def _id_list(t: Optional[torch.Tensor], name: str):
    """(pointer or None, count) of an optional 1-D int32 device list."""
    n = 0 if t is None else t.numel()
    if n and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
        raise CSError(f"{name} must be a contiguous 1-D int32 tensor")
    return (t.data_ptr() if n else None), n


def _sample_step(entry: str, logits, base_seeds, step, done, out_len, out_tokens, next_tok, n_alive,
                 pad_id, temperature, softcap, bias_ids, bias_value, stop_ids, out_lp, max_tokens,
                 vocab, workspace, tensors=(), penalty=lambda S: (), stop_seqs=lambda S, vocab: ()):
    """The body of sample_step and sample_step_ex around the C entry point ``entry``:
    ``penalty(S)`` gives the arguments that entry takes between bias_value and stop_ids,
    ``stop_seqs(S, vocab)`` those between n_stop and max_tokens, from the device ``tensors``."""
    L = _lib.load()
    S, ld, vocab = _logits_args(logits, vocab)
    _require_cuda(logits, base_seeds, step, done, out_len, out_tokens, next_tok, n_alive,
                  bias_ids, stop_ids, out_lp, *tensors)
    if max_tokens is None:
        if out_tokens is None or out_tokens.dim() != 2:
            raise CSError("out_tokens must be [S, max_tokens] int32")
        max_tokens = out_tokens.shape[1]
    max_tokens = int(max_tokens)
    bias = _id_list(bias_ids, "bias_ids")
    stop = _id_list(stop_ids, "stop_ids")
    seen = penalty(S)
    workspace, ws_ptr, ws_bytes = _workspace_args(
        workspace, _sample_ws, int(getattr(L, entry + "_workspace_size")(S, vocab)), logits.device,
        "sample_step")
    rc = getattr(L, entry)(
        logits.data_ptr(), _DTYPE[logits.dtype], S, vocab, ld, float(temperature), float(softcap),
        _state_ptr(base_seeds, "base_seeds", torch.int64, (S,)),
        _state_ptr(step, "step", torch.int32, (1,)), *bias, float(bias_value), *seen, *stop,
        *stop_seqs(S, vocab), max_tokens, int(pad_id),
        _state_ptr(done, "done", torch.int32, (S,)),
        _state_ptr(out_len, "out_len", torch.int32, (S,)),
        _state_ptr(out_tokens, "out_tokens", torch.int32, (S, max_tokens)),
        _state_ptr(out_lp, "out_lp", torch.float32, (S, max_tokens)),
        _state_ptr(next_tok, "next_tok", torch.int64, (S,)),
        _state_ptr(n_alive, "n_alive", torch.int32, (1,)), ws_ptr, ws_bytes, _stream())
    if rc != 0:
        workspace.reset()
    _lib.check(rc, entry)


def sample_step(logits: torch.Tensor, base_seeds: torch.Tensor, step: torch.Tensor,
                done: torch.Tensor, out_len: torch.Tensor, out_tokens: torch.Tensor,
                next_tok: torch.Tensor, n_alive: torch.Tensor, *, pad_id: int,
                temperature: float = 1.0, softcap: float = 0.0,
                bias_ids: Optional[torch.Tensor] = None, bias_value: float = -1e6,
                stop_ids: Optional[torch.Tensor] = None, out_lp: Optional[torch.Tensor] = None,
                max_tokens: Optional[int] = None, vocab: Optional[int] = None,
                workspace: Optional[Workspace] = None) -> None:
    """One generation step of S streams in place (cs_sample_step): the draw of
    ``vocab_sample`` with seed draw_seed(base_seeds[s], step[0]) on the biased row, the stop
    test, the append to out_tokens [S, max_tokens] / out_lp / out_len, the next input token
    (next_tok [S] int64: the id, or pad_id once the stream is done) and n_alive [1].

    Every argument that changes between steps (step [1] int32, done / out_len [S] int32) lives
    on the device and nothing is allocated here, so the call replays inside a captured graph.
    bias_ids / stop_ids: int32 device tensors (None or empty: none).  The workspace is a
    Workspace(zeroed=True) used by this op alone."""
    _sample_step("cs_sample_step", logits, base_seeds, step, done, out_len, out_tokens, next_tok,
                 n_alive, pad_id, temperature, softcap, bias_ids, bias_value, stop_ids, out_lp,
                 max_tokens, vocab, workspace)


def _seen_args(seen_ids: Optional[torch.Tensor], seen_off: Optional[torch.Tensor], rows: int):
    """Pointers of the ragged seen list (both None: no list).  seen_off is int32 [rows + 1]."""
    if seen_off is None:
        if seen_ids is not None:
            raise CSError("seen_ids needs seen_off")
        return None, None
    if seen_off.dtype != torch.int32 or tuple(seen_off.shape) != (rows + 1,) \
            or not seen_off.is_contiguous():
        raise CSError(f"seen_off must be a contiguous int32 tensor of shape [{rows + 1}]")
    if seen_ids is None or seen_ids.dtype != torch.int32 or seen_ids.dim() != 1 \
            or not seen_ids.is_contiguous():
        raise CSError("seen_ids must be a contiguous 1-D int32 tensor")
    # an empty tensor's pointer may be NULL: the library wants one whenever offsets are given
    return (seen_ids.data_ptr() or seen_off.data_ptr()), seen_off.data_ptr()


def vocab_sample_ex(logits: torch.Tensor, seeds: Optional[torch.Tensor], *,
                    temperature: float = 1.0, vocab: Optional[int] = None, softcap: float = 0.0,
                    bias_ids: Optional[torch.Tensor] = None, bias_value: float = -1e6,
                    repetition_penalty: float = 1.0, seen_ids: Optional[torch.Tensor] = None,
                    seen_off: Optional[torch.Tensor] = None, n_draw: Optional[int] = None,
                    workspace: Optional[Workspace] = None):
    """``vocab_sample`` with the controls of cs_vocab_sample_ex: bias_ids take bias_value
    before the soft-cap, the tokens of seen_ids[seen_off[r]:seen_off[r+1]] (int32 device
    tensors) take the repetition penalty after it, and temperature 0 is greedy (seeds may then
    be None, with n_draw giving the number of columns, default 1)."""
    def controls(rows):
        return (*_id_list(bias_ids, "bias_ids"), float(bias_value), float(repetition_penalty),
                *_seen_args(seen_ids, seen_off, rows))

    return _vocab_sample("cs_vocab_sample_ex", logits, seeds, n_draw, temperature, vocab, softcap,
                         workspace, (bias_ids, seen_ids, seen_off), controls)


MAX_STOP_SEQ, MAX_STOP_LEN = 8, 32     # cs_sample_step_ex


def sample_step_ex(logits: torch.Tensor, base_seeds: Optional[torch.Tensor], step: torch.Tensor,
                   done: torch.Tensor, out_len: torch.Tensor, out_tokens: torch.Tensor,
                   next_tok: torch.Tensor, n_alive: torch.Tensor, *, pad_id: int,
                   temperature: float = 1.0, softcap: float = 0.0,
                   bias_ids: Optional[torch.Tensor] = None, bias_value: float = -1e6,
                   repetition_penalty: float = 1.0, seen_ids: Optional[torch.Tensor] = None,
                   seen_off: Optional[torch.Tensor] = None,
                   stop_ids: Optional[torch.Tensor] = None, stop_seqs=(),
                   tok_bytes: Optional[torch.Tensor] = None,
                   tok_off: Optional[torch.Tensor] = None, tail: Optional[torch.Tensor] = None,
                   tail_len: Optional[torch.Tensor] = None,
                   out_lp: Optional[torch.Tensor] = None, max_tokens: Optional[int] = None,
                   vocab: Optional[int] = None, workspace: Optional[Workspace] = None,
                   _dfa=None) -> None:
    """``sample_step`` with the controls of cs_sample_step_ex: temperature 0 is greedy, the
    tokens of seen_ids[seen_off[s]:seen_off[s+1]] and the stream's own out_tokens take the
    repetition penalty, and stop_seqs (a sequence of bytes objects, held by the host) end a
    stream whose decoded bytes complete one: tok_bytes (uint8) / tok_off (int32 [vocab + 1])
    are the tokens' bytes, tail (uint8 [S, 32]) / tail_len (int32 [S]) the per-stream window,
    zero at the start.  With every control off this is ``sample_step``, bit for bit.
    (``_dfa`` is sample_step_dfa's way in: the same body around cs_sample_step_dfa.)"""
    entry = "cs_sample_step_ex" if _dfa is None else "cs_sample_step_dfa"
    dfa_tensors = () if _dfa is None else _dfa[:3]
    stop_seqs = [bytes(b) for b in stop_seqs]
    offs = [0]
    for b in stop_seqs:
        offs.append(offs[-1] + len(b))
    stop_bytes = ctypes.create_string_buffer(b"".join(stop_seqs), max(1, offs[-1]))
    stop_off = (ctypes.c_int32 * len(offs))(*offs)

    def penalty(S):
        return (float(repetition_penalty), *_seen_args(seen_ids, seen_off, S))

    def seq_args(S, vocab):
        return (_state_ptr(tok_bytes, "tok_bytes", torch.uint8,
                           tuple(tok_bytes.shape[:1]) if tok_bytes is not None else ()),
                _state_ptr(tok_off, "tok_off", torch.int32, (vocab + 1,)),
                ctypes.cast(stop_bytes, ctypes.c_void_p), ctypes.cast(stop_off, ctypes.c_void_p),
                len(stop_seqs), _state_ptr(tail, "tail", torch.uint8, (S, MAX_STOP_LEN)),
                _state_ptr(tail_len, "tail_len", torch.int32, (S,)), *dfa_args(S))

    def dfa_args(S):
        # cs_sample_step_dfa: masks, mask_words, trans, n_states, dfa_state
        if _dfa is None:
            return ()
        masks, trans, dfa_state, n_states = _dfa
        mp, words, n, sp = _mask_args(masks, dfa_state, S, n_states)
        return mp, words, _ptr(trans) if masks is not None else None, n, sp

    _sample_step(entry, logits, base_seeds, step, done, out_len, out_tokens, next_tok,
                 n_alive, pad_id, temperature, softcap, bias_ids, bias_value, stop_ids, out_lp,
                 max_tokens, vocab, workspace,
                 (seen_ids, seen_off, tok_bytes, tok_off, tail, tail_len, *dfa_tensors),
                 penalty, seq_args)


MAX_DFA_STATES = 1024                  # cs_dfa_token_masks, cs_vocab_sample_dfa, cs_sample_step_dfa


def dfa_token_masks(trans: torch.Tensor, accept: torch.Tensor, tok_bytes: torch.Tensor,
                    tok_off: torch.Tensor, stop_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-state token masks of a byte automaton (cs_dfa_token_masks): trans int16
    [n_states, 256] (-1 dead), accept uint8 [n_states], tok_bytes uint8 / tok_off int32
    [vocab + 1] the tokens' bytes, stop_ids int32 -> int32 [n_states, ceil(vocab / 32)] whose
    bit (q, v) says that token v may be drawn in state q (a stop id: in accepting states)."""
    L = _lib.load()
    _require_cuda(trans, accept, tok_bytes, tok_off, stop_ids)
    if trans.dtype != torch.int16 or trans.dim() != 2 or trans.shape[1] != 256 \
            or not trans.is_contiguous():
        raise CSError("trans must be a contiguous int16 [n_states, 256] tensor")
    n_states = trans.shape[0]
    if accept.dtype != torch.uint8 or tuple(accept.shape) != (n_states,) \
            or not accept.is_contiguous():
        raise CSError(f"accept must be a contiguous uint8 tensor of shape [{n_states}]")
    if tok_off.dtype != torch.int32 or tok_off.dim() != 1 or tok_off.numel() < 2 \
            or not tok_off.is_contiguous():
        raise CSError("tok_off must be a contiguous int32 [vocab + 1] tensor")
    if tok_bytes.dtype != torch.uint8 or tok_bytes.dim() != 1 or not tok_bytes.is_contiguous():
        raise CSError("tok_bytes must be a contiguous 1-D uint8 tensor")
    vocab = tok_off.numel() - 1
    masks = torch.empty((n_states, (vocab + 31) // 32), dtype=torch.int32, device=trans.device)
    rc = L.cs_dfa_token_masks(trans.data_ptr(), accept.data_ptr(), n_states, tok_bytes.data_ptr(),
                              tok_off.data_ptr(), vocab, *_id_list(stop_ids, "stop_ids"),
                              masks.data_ptr(), _stream())
    _lib.check(rc, "cs_dfa_token_masks")
    return masks


def _mask_args(masks: Optional[torch.Tensor], dfa_state: Optional[torch.Tensor], rows: int,
               n_states: Optional[int]):
    """(masks pointer, mask_words, n_states, dfa_state pointer) of the *_dfa entries; masks
    None: all NULL / 0, which makes the entry its *_ex sibling."""
    if masks is None:
        return None, 0, 0, None
    if masks.dtype != torch.int32 or masks.dim() != 2 or not masks.is_contiguous():
        raise CSError("masks must be a contiguous int32 [n_states, mask_words] tensor")
    return (masks.data_ptr(), masks.shape[1], masks.shape[0] if n_states is None else int(n_states),
            _state_ptr(dfa_state, "dfa_state", torch.int32, (rows,)))


def vocab_sample_dfa(logits: torch.Tensor, seeds: Optional[torch.Tensor], *,
                     masks: Optional[torch.Tensor] = None,
                     dfa_state: Optional[torch.Tensor] = None, n_states: Optional[int] = None,
                     temperature: float = 1.0, vocab: Optional[int] = None, softcap: float = 0.0,
                     bias_ids: Optional[torch.Tensor] = None, bias_value: float = -1e6,
                     repetition_penalty: float = 1.0, seen_ids: Optional[torch.Tensor] = None,
                     seen_off: Optional[torch.Tensor] = None, n_draw: Optional[int] = None,
                     workspace: Optional[Workspace] = None):
    """``vocab_sample_ex`` on rows held to an automaton (cs_vocab_sample_dfa): row r may draw
    the tokens whose bit is set in masks[dfa_state[r]] (``dfa_token_masks``; dfa_state int32
    [rows]); the others are out of the draw and of the log-probabilities' normaliser.  A row
    whose state allows nothing yields id -1.  masks None: ``vocab_sample_ex``, bit for bit."""
    def controls(rows):
        return (*_id_list(bias_ids, "bias_ids"), float(bias_value), float(repetition_penalty),
                *_seen_args(seen_ids, seen_off, rows), *_mask_args(masks, dfa_state, rows, n_states))

    return _vocab_sample("cs_vocab_sample_dfa", logits, seeds, n_draw, temperature, vocab, softcap,
                         workspace, (bias_ids, seen_ids, seen_off, masks, dfa_state), controls)


def sample_step_dfa(logits: torch.Tensor, base_seeds: Optional[torch.Tensor], step: torch.Tensor,
                    done: torch.Tensor, out_len: torch.Tensor, out_tokens: torch.Tensor,
                    next_tok: torch.Tensor, n_alive: torch.Tensor, *, pad_id: int,
                    masks: Optional[torch.Tensor] = None, trans: Optional[torch.Tensor] = None,
                    dfa_state: Optional[torch.Tensor] = None, n_states: Optional[int] = None,
                    **kw) -> None:
    """``sample_step_ex`` (whose keywords it takes) with every stream held to an automaton
    (cs_sample_step_dfa): the draw is ``vocab_sample_dfa``'s in state dfa_state[s] (int32
    [S], device, the start states before the first step), and an appended token's bytes
    (tok_bytes / tok_off, needed here with or without stop strings) are walked through trans
    (int16 [n_states, 256]) to the stream's next state, inside the same two launches.
    masks None: ``sample_step_ex``, bit for bit."""
    if masks is not None and trans is not None and (
            trans.dtype != torch.int16 or trans.dim() != 2 or trans.shape[1] != 256
            or not trans.is_contiguous()):
        raise CSError("trans must be a contiguous int16 [n_states, 256] tensor")
    if masks is not None and trans is not None and n_states is None \
            and trans.shape[0] != masks.shape[0]:
        raise CSError("trans and masks disagree on the number of states")
    sample_step_ex(logits, base_seeds, step, done, out_len, out_tokens, next_tok, n_alive,
                   pad_id=pad_id, _dfa=(masks, trans, dfa_state, n_states), **kw)


class AttnPlan:
    """A cs_prefix_attention work plan on the device (entries, counts) and the split
    partials' workspace it needs; built once per (prefix-length bounds, shape) and reused by
    every launch (and graph replay) of that shape."""

    def __init__(self, entries: Optional[torch.Tensor], n_attn: int, n_merge: int,
                 workspace: Optional[torch.Tensor]) -> None:
        self.entries, self.n_attn, self.n_merge, self.workspace = entries, n_attn, n_merge, workspace


_attn_plans: "collections.OrderedDict" = collections.OrderedDict()
_ATTN_PLAN_CACHE = 64
_plan_sinks = threading.local()


@contextlib.contextmanager
def retain_plans(holder: dict):
    """Every AttnPlan handed out inside the block is also stored in ``holder`` (keyed by
    id).  A captured graph keeps the raw device pointers of its plans' entries and
    workspace; the owner of the graph keeps the plans alive through ``holder`` so that
    an eviction from the LRU cache above cannot free memory a later replay uses."""
    stack = getattr(_plan_sinks, "stack", None)
    if stack is None:
        stack = _plan_sinks.stack = []
    stack.append(holder)
    try:
        yield holder
    finally:
        stack.pop()


def _retain(plan: "AttnPlan") -> "AttnPlan":
    for holder in getattr(_plan_sinks, "stack", ()):
        holder[id(plan)] = plan
    return plan


def attention_plan(prefix_len_host: Sequence[int], group_prefix_host: Optional[Sequence[int]],
                   n_groups: int, n_str: int, T: int, H: int, Hkv: int, D: int, ld_hist: int,
                   device) -> AttnPlan:
    """The work plan of cs_prefix_attention_plan for host bounds of the prefix lengths
    (cached; the device copy is made outside any graph capture)."""
    key = (tuple(int(x) for x in prefix_len_host),
           None if group_prefix_host is None else tuple(int(x) for x in group_prefix_host),
           n_groups, n_str, T, H, Hkv, D, ld_hist, str(device))
    plan = _attn_plans.get(key)
    if plan is not None:
        _attn_plans.move_to_end(key)
        return _retain(plan)
    if torch.cuda.is_current_stream_capturing():
        raise CSError("cs_prefix_attention: the work plan of this shape must be built before "
                      "graph capture (run the step once eagerly)")
    L = _lib.load()
    lens = np.ascontiguousarray(np.asarray(key[0], dtype=np.int32))
    gp = None if key[1] is None else np.ascontiguousarray(np.asarray(key[1], dtype=np.int32))
    n_a, n_m = ctypes.c_int32(0), ctypes.c_int32(0)
    wsb = ctypes.c_size_t(0)
    args = (lens.ctypes.data, lens.size, None if gp is None else gp.ctypes.data, n_groups, n_str,
            T, H, Hkv, D, ld_hist)
    total = int(L.cs_prefix_attention_plan(*args, None, 0, ctypes.byref(n_a), ctypes.byref(n_m),
                                           ctypes.byref(wsb)))
    if total < 0:
        _lib.check(total, "cs_prefix_attention_plan")
    if total == 0:
        plan = AttnPlan(None, 0, 0, None)
    else:
        host = np.zeros((total, 4), dtype=np.int32)
        rc = int(L.cs_prefix_attention_plan(*args, host.ctypes.data, total, ctypes.byref(n_a),
                                            ctypes.byref(n_m), ctypes.byref(wsb)))
        if rc != total:
            _lib.check(rc if rc < 0 else -1, "cs_prefix_attention_plan")
        plan = AttnPlan(torch.from_numpy(host).to(device), n_a.value, n_m.value,
                        torch.empty(max(int(wsb.value), 16), dtype=torch.uint8, device=device))
    _attn_plans[key] = plan
    while len(_attn_plans) > _ATTN_PLAN_CACHE:
        _attn_plans.popitem(last=False)
    return _retain(plan)


def prefix_attention(q: torch.Tensor, k_prefix: torch.Tensor, vt_prefix: torch.Tensor,
                     prefix_off: torch.Tensor, prefix_len: torch.Tensor, max_prefix_len: int,
                     k_hist: torch.Tensor, vt_hist: torch.Tensor, hist_base: torch.Tensor,
                     n_str: int, T: int, *, scale: float, softcap: float = 0.0, window: int = 0,
                     group_prefix: Optional[torch.Tensor] = None,
                     prefix_len_host: Optional[Sequence[int]] = None,
                     group_prefix_host: Optional[Sequence[int]] = None,
                     out: Optional[torch.Tensor] = None, plan: Optional[AttnPlan] = None,
                     hist_rows: Optional[torch.Tensor] = None):
    """Cascade attention of candidate streams over shared per-agent prefix K/V
    (cs_prefix_attention; layouts in include/consensus_scoring.h).  hist_rows [S, ldh] int32:
    the history is row-layout (vt_hist is V [S, Hkv, ldh, D] like k_hist) and slot j of
    stream s lives in row hist_rows[s, j] (cs_prefix_attention_rows: beams without copies).

    q [n_groups*n_str*T, H, D] bf16; k_prefix [Hkv, Lp, D], vt_prefix [Hkv, Lp/32, D, 32]
    (ragged prefixes: prefix p's keys are rows prefix_off[p] ..; V transposed in 32-key
    tiles, see blocked_vt); prefix_off [n_prefix] int64, prefix_len [n_prefix] int32
    (device), max_prefix_len >= every prefix_len (host); k_hist [S, Hkv, ldh, D], vt_hist
    [S, Hkv, ldh/32, D, 32] (S = n_groups*n_str); hist_base [1] int32 (device).
    prefix_len_host (per prefix) / group_prefix_host: host bounds that size the key splits
    of the work plan (default: max_prefix_len everywhere); ``plan`` overrides them.
    Returns out [n_tok, H, D] bf16.  Replaces the per-call prompt re-encoding of
    src/utils.py:249-259."""
    L = _lib.load()
    if q.dim() != 3 or q.dtype != torch.bfloat16 or not q.is_contiguous():
        raise CSError("q must be a contiguous [n_tok, H, D] bfloat16 tensor")
    n_tok, H, D = q.shape
    Hkv, Lp, Dk = k_prefix.shape
    S, Hkv2, ldh, Dh = k_hist.shape
    if Dk != D or Dh != D or Hkv2 != Hkv:
        raise CSError("head layout mismatch between q, k_prefix and k_hist")
    if hist_rows is not None:
        # the buffers may hold more rows than query streams (a token tree's earlier levels)
        if tuple(vt_hist.shape) != (S, Hkv, ldh, D):
            raise CSError("row-layout history: V [R, Hkv, ldh, D] like K expected")
        if hist_rows.dtype != torch.int32 or hist_rows.dim() != 2 or hist_rows.shape[1] != ldh or \
                hist_rows.shape[0] > S or not hist_rows.is_contiguous():
            raise CSError("hist_rows must be a contiguous int32 [S, ldh] tensor (S <= buffer rows)")
        if _DEBUG_TABLES and hist_rows.numel() and not torch.cuda.is_current_stream_capturing():
            if int(hist_rows.min()) < 0 or int(hist_rows.max()) >= S:
                raise CSError("hist_rows names a row outside the K / V buffer")
        S = hist_rows.shape[0]
    if tuple(vt_prefix.shape) != (Hkv, Lp // 32, D, 32) or \
            (hist_rows is None and tuple(vt_hist.shape) != (S, Hkv, ldh // 32, D, 32)):
        raise CSError("vt_prefix [Hkv, Lp/32, D, 32] / vt_hist [S, Hkv, ldh/32, D, 32] "
                      "(V^T in 32-key tiles) expected")
    for t in (k_prefix, vt_prefix, k_hist, vt_hist):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise CSError("K/V buffers must be contiguous bfloat16")
    if n_str <= 0 or T <= 0 or S % n_str != 0 or n_tok != S * T:
        raise CSError(f"n_tok {n_tok} != streams {S} x T {T} (n_str {n_str})")
    n_groups = S // n_str
    n_prefix = prefix_len.numel()
    if group_prefix is None and n_groups != n_prefix:
        raise CSError("n_groups must equal n_prefix without group_prefix")
    if group_prefix is not None and (group_prefix.dtype != torch.int32 or group_prefix.numel() != n_groups):
        raise CSError("group_prefix must be int32 [n_groups]")
    if prefix_len.dtype != torch.int32 or prefix_off.dtype != torch.int64 or \
            prefix_off.numel() != n_prefix:
        raise CSError("prefix_len must be int32 [n_prefix] and prefix_off int64 [n_prefix]")
    if hist_base.dtype != torch.int32 or hist_base.numel() != 1:
        raise CSError("hist_base must be a one-element int32 device tensor")
    _require_cuda(q, k_prefix, vt_prefix, prefix_off, prefix_len, k_hist, vt_hist, hist_base,
                  group_prefix, out, hist_rows)
    if out is None:
        out = torch.empty_like(q)
    mpl = int(max_prefix_len)
    if plan is None:
        if prefix_len_host is None or (group_prefix is not None and group_prefix_host is None):
            # no host lengths: every group bounded by max_prefix_len
            lens_h, gp_h = [mpl], [0] * n_groups
        else:
            lens_h = [min(int(x), mpl) for x in prefix_len_host]
            gp_h = None if group_prefix is None else list(group_prefix_host)
            if len(lens_h) != n_prefix or (gp_h is not None and len(gp_h) != n_groups):
                raise CSError("prefix_len_host / group_prefix_host sizes do not match")
        plan = attention_plan(lens_h, gp_h, n_groups, n_str, T, H, Hkv, D, ldh, q.device)
    else:
        _retain(plan)
    ws = plan.workspace
    gp = group_prefix.data_ptr() if group_prefix is not None else None
    pe = plan.entries.data_ptr() if plan.entries is not None else None
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    if hist_rows is not None:
        rc = L.cs_prefix_attention_rows(q.data_ptr(), k_prefix.data_ptr(), vt_prefix.data_ptr(), Lp,
                                        prefix_off.data_ptr(), prefix_len.data_ptr(), mpl, gp,
                                        n_groups, k_hist.data_ptr(), vt_hist.data_ptr(),
                                        hist_rows.data_ptr(), ldh, hist_base.data_ptr(), n_str, T,
                                        H, Hkv, D, float(scale), float(softcap), int(window), pe,
                                        plan.n_attn, plan.n_merge, out.data_ptr(), wsp, wsn,
                                        _stream())
        _lib.check(rc, "cs_prefix_attention_rows")
        return out
    rc = L.cs_prefix_attention(q.data_ptr(), k_prefix.data_ptr(), vt_prefix.data_ptr(), Lp,
                               prefix_off.data_ptr(), prefix_len.data_ptr(), mpl, gp,
                               n_groups, k_hist.data_ptr(), vt_hist.data_ptr(), ldh,
                               hist_base.data_ptr(), n_str, T, H, Hkv, D, float(scale),
                               float(softcap), int(window), pe, plan.n_attn, plan.n_merge,
                               out.data_ptr(), wsp, wsn, _stream())
    _lib.check(rc, "cs_prefix_attention")
    return out


def rope_place(qkv: "torch.Tensor | SplitPartials", inv_freq: torch.Tensor, prefix_len: torch.Tensor,
               hist_base: torch.Tensor, n_str: int, T: int, H: int, Hkv: int, D: int,
               q_out: torch.Tensor, k_hist: torch.Tensor, vt_hist: torch.Tensor, *,
               group_prefix: Optional[torch.Tensor] = None, v_rows: bool = False) -> torch.Tensor:
    """RoPE of the fused projection + placement of q / the new K, V (cs_rope_place).  qkv
    may be a K-split GEMM's unfolded SplitPartials (T < 32): folded inside the launch
    (cs_rope_place_splitk), bitwise the folded projection.  v_rows: vt_hist is a row-layout
    V [S, Hkv, ldh, D] (cs_rope_place_rows, the cs_prefix_attention_rows history)."""
    L = _lib.load()
    vshape = (lambda S, ldh: (S, Hkv, ldh, D)) if v_rows else (lambda S, ldh: (S, Hkv, ldh // 32, D, 32))
    split = isinstance(qkv, SplitPartials)
    name = "cs_rope_place" + ("_splitk" if split else "") + ("_rows" if v_rows else "")
    if split:
        src = qkv.part
        if (src.dim() != 3 or src.dtype != torch.float32 or not src.is_contiguous()
                or src.shape[2] != (H + 2 * Hkv) * D):
            raise CSError("qkv partials must be contiguous float32 [splits, n_tok, (H + 2 Hkv) D]")
        n_tok = src.shape[1]
        head = (src.data_ptr(), src.shape[0])
    else:
        src = qkv
        if src.dim() != 2 or src.dtype != torch.bfloat16 or src.stride(1) != 1:
            raise CSError("qkv must be a 2-D bfloat16 tensor with unit column stride")
        n_tok = src.shape[0]
        ld = src.stride(0) if n_tok > 1 else src.shape[1]
        if src.data_ptr() % 8 or ld % 4 != 0:
            raise CSError(f"{name}: qkv must be 8-byte aligned, ld_qkv a multiple of 4")
        head = (src.data_ptr(), ld)
    S, Hkv2, ldh, Dk = k_hist.shape
    if not v_rows and ldh % 32 != 0:
        raise CSError(f"{name}: ld_hist must be a multiple of 32 (V^T tiles)")
    if Hkv2 != Hkv or Dk != D or tuple(vt_hist.shape) != vshape(S, ldh):
        raise CSError("k_hist [S, Hkv, ldh, D] / vt_hist [S, Hkv, ldh/32, D, 32] layout mismatch")
    if n_tok != S * T or S % n_str != 0:
        raise CSError("qkv rows must be streams x T")
    if tuple(q_out.shape) != (n_tok, H, D) or q_out.dtype != torch.bfloat16 or not q_out.is_contiguous():
        raise CSError("q_out must be a contiguous [n_tok, H, D] bfloat16 tensor")
    if inv_freq.dtype != torch.float32 or inv_freq.numel() != D // 2:
        raise CSError("inv_freq must be float32 [D/2]")
    if q_out.data_ptr() % 16 or k_hist.data_ptr() % 16 or vt_hist.data_ptr() % 16:
        raise CSError(f"{name}: q_out, k_hist and vt_hist must be 16-byte aligned")
    _require_cuda(src, inv_freq, prefix_len, hist_base, q_out, k_hist, vt_hist, group_prefix)
    rc = getattr(L, name)(*head, inv_freq.data_ptr(), prefix_len.data_ptr(),
                          group_prefix.data_ptr() if group_prefix is not None else None,
                          S // n_str, hist_base.data_ptr(), n_str, T, H, Hkv, D, q_out.data_ptr(),
                          k_hist.data_ptr(), vt_hist.data_ptr(), ldh, _stream())
    _lib.check(rc, name)
    return q_out


def _rows2d(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.dtype != torch.bfloat16 or t.stride(1) != 1:
        raise CSError(f"{name} must be a 2-D bfloat16 tensor with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


class SplitPartials(NamedTuple):
    """A K-split GEMM's unfolded fp32 partials [splits, M, N] (cs_gemm_bf16 with y = NULL),
    folded by the add_rms_norm that consumes them (cs_add_rms_norm_splitk)."""
    part: torch.Tensor


def add_rms_norm(a: torch.Tensor, weight: torch.Tensor, eps: float, *,
                 b: "Optional[torch.Tensor | SplitPartials]" = None,
                 b_weight: Optional[torch.Tensor] = None, plus_one: bool = False,
                 s_out: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = RMSNorm(a + b) (cs_add_rms_norm); the bf16 sum a + b is also written to s_out.
    a, b, s_out, out [rows, d] bf16; weight [d] bf16 (Gemma-2: plus_one, 1 + weight).
    b_weight: b is RMS-normalised first with that weight (Gemma-2's post norms), bitwise as
    add_rms_norm(b, b_weight) followed by this call.  b may be a SplitPartials (linear(...,
    fold=False)): folded inside this launch, bitwise as the GEMM's own fold then this call."""
    L = _lib.load()
    lda = _rows2d(a, "a")
    rows, d = a.shape
    if isinstance(b, SplitPartials):
        return _add_rms_norm_splitk(L, a, lda, weight, eps, b.part, b_weight, plus_one, s_out, out)
    ldb = _rows2d(b, "b") if b is not None else 0
    lds = _rows2d(s_out, "s_out") if s_out is not None else 0
    if (b is not None and b.shape != a.shape) or (s_out is not None and s_out.shape != a.shape):
        raise CSError("a, b and s_out must share one shape")
    if weight.dtype != torch.bfloat16 or weight.numel() != d or not weight.is_contiguous():
        raise CSError("weight must be a contiguous bfloat16 [d] tensor")
    if b_weight is not None and (b is None or b_weight.dtype != torch.bfloat16 or
                                 b_weight.numel() != d or not b_weight.is_contiguous()):
        raise CSError("b_weight must be a contiguous bfloat16 [d] tensor and needs b")
    if out is None:
        out = torch.empty_like(a, memory_format=torch.contiguous_format)
    ldy = _rows2d(out, "out")
    _require_cuda(a, b, s_out, weight, out)
    rc = L.cs_add_rms_norm(a.data_ptr(), lda, b.data_ptr() if b is not None else None, ldb,
                           b_weight.data_ptr() if b_weight is not None else None,
                           s_out.data_ptr() if s_out is not None else None, lds, weight.data_ptr(),
                           rows, d, float(eps), int(bool(plus_one)), out.data_ptr(), ldy, _stream())
    _lib.check(rc, "cs_add_rms_norm")
    return out


def _add_rms_norm_splitk(L, a, lda, weight, eps, part, b_weight, plus_one, s_out, out):
    rows, d = a.shape
    if part.dim() != 3 or part.dtype != torch.float32 or not part.is_contiguous() or \
            tuple(part.shape[1:]) != (rows, d):
        raise CSError("split partials must be a contiguous float32 [splits, rows, d] tensor")
    lds = _rows2d(s_out, "s_out") if s_out is not None else 0
    if s_out is not None and s_out.shape != a.shape:
        raise CSError("a and s_out must share one shape")
    if weight.dtype != torch.bfloat16 or weight.numel() != d or not weight.is_contiguous():
        raise CSError("weight must be a contiguous bfloat16 [d] tensor")
    if b_weight is not None and (b_weight.dtype != torch.bfloat16 or b_weight.numel() != d or
                                 not b_weight.is_contiguous()):
        raise CSError("b_weight must be a contiguous bfloat16 [d] tensor")
    if out is None:
        out = torch.empty_like(a, memory_format=torch.contiguous_format)
    ldy = _rows2d(out, "out")
    _require_cuda(a, part, s_out, weight, out)
    rc = L.cs_add_rms_norm_splitk(a.data_ptr(), lda, part.data_ptr(), int(part.shape[0]),
                                  b_weight.data_ptr() if b_weight is not None else None,
                                  s_out.data_ptr() if s_out is not None else None, lds,
                                  weight.data_ptr(), rows, d, float(eps), int(bool(plus_one)),
                                  out.data_ptr(), ldy, _stream())
    _lib.check(rc, "cs_add_rms_norm_splitk")
    return out


_ACT = {"silu": 0, "gelu_tanh": 1}      # the `act` argument of cs_gated_act and cs_gemm_bf16


def gated_act(gate: torch.Tensor, up: torch.Tensor, act: str = "silu",
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(gate) * up (cs_gated_act): SiLU (Llama-3) or tanh-GeLU (Gemma-2); [rows, F] bf16."""
    L = _lib.load()
    ldg = _rows2d(gate, "gate")
    ldu = _rows2d(up, "up")
    if gate.shape != up.shape:
        raise CSError("gate and up must share one shape")
    rows, F = gate.shape
    if out is None:
        out = torch.empty(rows, F, dtype=torch.bfloat16, device=gate.device)
    ldo = _rows2d(out, "out")
    _require_cuda(gate, up, out)
    rc = L.cs_gated_act(gate.data_ptr(), ldg, up.data_ptr(), ldu, rows, F, _ACT[act],
                        out.data_ptr(), ldo, _stream())
    _lib.check(rc, "cs_gated_act")
    return out


GEMM_DISPATCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned",
                             "gemm_dispatch_mi355x.json")
_gemm_table: Optional[dict] = None


def gemm_choice(M: int, N: int, K: int, gated: bool = False,
                packed: bool = False) -> Optional[dict]:
    """The cs_gemm_bf16 tile variant and K split measured faster than hipBLASLt for this
    exact shape on MI355X (tools/tune_gemm_dispatch.py -> tuned/gemm_dispatch_mi355x.json,
    read only), or None: the shape stays on hipBLASLt.  packed: the caller holds the weight's
    cs_gemm_pack'ed copy, so the packed form's entry counts too ({"packed": True, ...} when it
    is the fastest).  CS_GEMM_DISPATCH=0 turns the table off, CS_GEMM_DISPATCH=<file> reads
    another one."""
    global _gemm_table
    if _gemm_table is None:
        env = os.environ.get("CS_GEMM_DISPATCH", "")
        path = GEMM_DISPATCH if env in ("", "1") else env
        table = {}
        if env != "0" and os.path.exists(path):
            with open(path) as f:
                table = json.load(f).get("table", {})
        _gemm_table = table
    e = _gemm_table.get(f"{M},{N},{K},{int(bool(gated))}")
    if e is None:
        return None
    if packed and "packed" in e:
        return {"variant": int(e["packed"]["variant"]), "splits": int(e["packed"]["splits"]),
                "packed": True}
    if "variant" in e:
        return {"variant": int(e["variant"]), "splits": int(e["splits"]), "packed": False}
    return None


def gemm_pack_gain(N: int, K: int, gated: bool = False) -> float:
    """The largest time (µs) the packed form saves on an [N, K] weight at any row count the
    dispatch table measured (against the faster of hipBLASLt and the unpacked cs_gemm_bf16);
    0 when no row count runs it packed.  A model keeps cs_gemm_pack'ed copies of the weights
    with a gain, the most per byte first."""
    gemm_choice(1, N, K, gated)                 # loads the table
    if hasattr(_gemm_table, "packs"):           # a computed table (tests)
        return 1.0 if _gemm_table.packs(N, K, gated) else 0.0
    tail = f",{N},{K},{int(bool(gated))}"
    gain = 0.0
    for k, v in _gemm_table.items():
        if k.endswith(tail) and "packed" in v:
            ref = min(float(v.get("us", float("inf"))), float(v.get("torch_us", float("inf"))))
            gain = max(gain, ref - float(v["packed"]["us"]) if ref < float("inf") else 1.0)
    return gain


def gemm_packs(N: int, K: int, gated: bool = False) -> bool:
    """Whether the dispatch table runs an [N, K] weight packed at some row count."""
    return gemm_pack_gain(N, K, gated) > 0.0


def linear(x: torch.Tensor, w: torch.Tensor, *, gated: bool = False, act: str = "silu",
           out: Optional[torch.Tensor] = None, fold: bool = True,
           packed: Optional["PackedWeight"] = None):
    """y = x @ w.T (gated: act(gate) * up of the fused gate|up weight) on whichever GEMM the
    dispatch table measured faster for this shape: cs_gemm_bf16 (on the packed copy
    ``packed`` of w when given and fastest) or hipBLASLt (+ cs_gated_act).
    fold=False: a K-split cs_gemm_bf16 returns its unfolded SplitPartials (for an
    add_rms_norm to fold); every other path returns the bf16 tensor as usual.
    packed an Fp8Weight (w is then its bf16 twin): a row count and shape cs_gemm_bf16_w8 serves
    (gemm_w8_serves) runs on the 1-byte codes; every other call continues below on the twin."""
    if isinstance(packed, Fp8Weight):
        fw, packed = packed, packed.fallback
        if x.dim() == 2 and gemm_w8_serves(x.shape[0], fw.N, fw.K, gated) and _w8_operands(x, fw):
            if not fold and not gated and out is None:
                splits = int(_lib.load().cs_gemm_w8_splits(x.shape[0], fw.N, fw.K, 0))
                if splits > 1:
                    return gemm_w8_partials(x, fw, splits=splits)
            return gemm_w8(x, fw, gated=gated, act=act, out=out)
    if x.is_cuda and x.dim() == 2:
        ch = gemm_choice(x.shape[0], w.shape[0], w.shape[1], gated, packed=packed is not None)
        if ch is not None:
            # through the public names (a test counts the calls by replacing them); their
            # body checks the operands, once per call, and what it refuses goes to hipBLASLt
            wt = packed if ch["packed"] else w
            try:
                if not fold and not gated and out is None and ch["splits"] > 1:
                    part = gemm_packed_partials if ch["packed"] else gemm_partials
                    return part(x, wt, splits=ch["splits"], variant=ch["variant"])
                run = gemm_packed if ch["packed"] else gemm
                return run(x, wt, gated=gated, act=act, splits=ch["splits"], variant=ch["variant"],
                           out=out)
            except _OperandsRefused:
                pass
    if gated:          # the plain GEMM (on whichever form is faster) + cs_gated_act
        F = w.shape[0] // 2
        y = linear(x, w, packed=packed)
        return gated_act(y[:, :F], y[:, F:], act, out=out)
    if out is not None:
        return torch.matmul(x, w.t(), out=out)
    return x @ w.t()


def linear_into_residual(x: torch.Tensor, w: torch.Tensor, h: torch.Tensor, *,
                         packed: Optional["PackedWeight"] = None) -> bool:
    """h += x @ w.T in the GEMM's own epilogue (hipBLASLt, beta = 1: the product is added in
    fp32 and rounded once) when the dispatch table leaves this shape on hipBLASLt; returns
    False (nothing done) otherwise, and the caller takes ``linear`` + the residual add.
    For the many-row scoring forward: the residual add's launch then only normalises (one
    read and one write of the rows instead of two and two).  packed an Fp8Weight: a shape
    cs_gemm_bf16_w8 serves adds its product in that kernel's own epilogue (gemm_w8_add: fp32
    sum + h, rounded once -- the rounding of the epilogue the bf16 twin takes here, so the FP8
    engine differs from the twin's by accumulation order alone); otherwise as without it, on
    the twin w."""
    if isinstance(packed, Fp8Weight):
        fw, packed = packed, packed.fallback
        if (x.dim() == 2 and h.dim() == 2 and h.is_contiguous() and h.dtype == torch.bfloat16
                and h.shape == (x.shape[0], fw.N) and h.is_cuda
                and gemm_w8_serves(x.shape[0], fw.N, fw.K, False) and _w8_operands(x, fw)):
            if gemm_choice(x.shape[0], fw.N, fw.K, False, packed=packed is not None) is not None:
                return False      # the twin folds this shape in the residual add: so does the FP8 route
            gemm_w8_add(x, fw, h)
            return True
    if not (x.is_cuda and x.dim() == 2 and h.dim() == 2 and h.is_contiguous() and
            h.dtype == x.dtype == w.dtype == torch.bfloat16 and h.shape == (x.shape[0], w.shape[0])):
        return False
    if gemm_choice(x.shape[0], w.shape[0], w.shape[1], False, packed=packed is not None) is not None:
        return False
    h.addmm_(x, w.t())
    return True


class PackedWeight:
    """A [N, K] bf16 weight in cs_gemm_pack's fragment-major layout: each 16-row tile's
    64-deep K step is 2 KB of lane-ordered MFMA fragments, so cs_gemm_bf16_packed reads its
    weight stream in contiguous 1 KB pieces.  ``data`` is the packed [N * K] tensor."""

    def __init__(self, data: torch.Tensor, N: int, K: int):
        self.data, self.N, self.K = data, int(N), int(K)

    @property
    def shape(self):
        return (self.N, self.K)


def gemm_pack(w: torch.Tensor) -> PackedWeight:
    """The packed copy of w [N, K] (cs_gemm_pack; N % 16 == 0, K % 64 == 0)."""
    L = _lib.load()
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.stride(1) != 1:
        raise CSError("gemm_pack needs a bf16 [N, K] tensor with unit column stride")
    N, K = w.shape
    _require_cuda(w)
    out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    rc = L.cs_gemm_pack(w.data_ptr(), w.stride(0), N, K, out.data_ptr(), _stream())
    _lib.check(rc, "cs_gemm_pack")
    return PackedWeight(out, N, K)


class _OperandsRefused(CSError):
    """Operands cs_gemm_bf16 does not take (gemm_ok): ``linear`` then runs hipBLASLt."""


def _gemm_operands(x: torch.Tensor, w: "torch.Tensor | PackedWeight"):
    """(the weight's tensor, its row stride, N, K) when cs_gemm_bf16 takes y = x @ w.T (see
    gemm_ok), else None."""
    packed = isinstance(w, PackedWeight)
    wt = w.data if packed else w
    if x.dim() != 2 or wt.dim() != (1 if packed else 2):
        return None
    if x.dtype != torch.bfloat16 or wt.dtype != torch.bfloat16:
        return None
    (M, Kx), (ldx, col_x) = x.shape, x.stride()
    (N, K), (ldw, col_w) = ((w.N, w.K), (w.K, 1)) if packed else (wt.shape, wt.stride())
    if Kx != K or N % 128 or K % 64 or col_x != 1 or col_w != 1 or (ldx % 8 and M > 1) or ldw % 8:
        return None
    return (wt, ldw, N, K) if x.data_ptr() % 16 == 0 and wt.data_ptr() % 16 == 0 else None


def gemm_ok(x: torch.Tensor, w: "torch.Tensor | PackedWeight", gated: bool = False) -> bool:
    """Whether cs_gemm_bf16 takes y = x @ w.T: bf16 2-D operands with unit column stride,
    N a multiple of 128, K of 64, 16-byte aligned rows (a PackedWeight: its K-long rows)."""
    return _gemm_operands(x, w) is not None


def _gemm(who: str, x: torch.Tensor, w: "torch.Tensor | PackedWeight", gated: bool = False,
          act: str = "silu", splits: int = 0, variant: int = 0, out: Optional[torch.Tensor] = None,
          partials: bool = False):
    """The body of gemm, gemm_packed, gemm_partials and gemm_packed_partials: cs_gemm_bf16 on
    a tensor w, cs_gemm_bf16_packed on a PackedWeight; the bf16 result, or (partials, y =
    NULL) the K split's unfolded SplitPartials."""
    L = _lib.load()
    operands = _gemm_operands(x, w)
    if operands is None:
        raise _OperandsRefused(f"{who} needs bf16 x [M, K], w [N, K] with N % 128 == 0, K % 64 == 0")
    if partials and splits < 2:
        raise CSError(f"{who} needs splits >= 2")
    wt, ldw, N, K = operands
    packed = wt is not w
    M = x.shape[0]
    n_out = N // 2 if gated else N
    if out is None and not partials:
        out = torch.empty(M, n_out, dtype=torch.bfloat16, device=x.device)
    if out is not None and (out.shape != (M, n_out) or out.dtype != torch.bfloat16 or out.stride(1) != 1):
        raise CSError("out must be a bf16 [M, N] tensor with unit column stride")
    _require_cuda(x, wt, out)
    if gated:
        splits = 1
    elif splits <= 0:
        splits = int(L.cs_gemm_splits(M, N, K, 0, variant))
    ldx = x.stride(0) if M > 1 else K
    ldy = 0 if out is None else out.stride(0) if M > 1 else n_out
    if out is not None and splits > 1 and (ldy % 8 or out.data_ptr() % 16):
        # the split-K fold stores 16-byte vectors: fold into an aligned tensor, then copy
        out.copy_(_gemm(who, x, w, splits=splits, variant=variant))
        return out
    part = torch.empty(splits, M, N, dtype=torch.float32, device=x.device) if splits > 1 else None
    ws = (wt.data_ptr(),) if packed else (wt.data_ptr(), ldw)
    entry = L.cs_gemm_bf16_packed if packed else L.cs_gemm_bf16
    rc = entry(x.data_ptr(), ldx, *ws, None if out is None else out.data_ptr(), ldy, M, N, K, splits,
               int(bool(gated)), _ACT[act], variant, None if part is None else part.data_ptr(),
               _stream())
    _lib.check(rc, "cs_gemm_bf16_packed" if packed else "cs_gemm_bf16")
    return SplitPartials(part) if partials else out


def gemm(x: torch.Tensor, w: torch.Tensor, *, gated: bool = False, act: str = "silu",
         splits: int = 0, variant: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T (cs_gemm_bf16): x [M, K], w [N, K] bf16, y [M, N] bf16, fp32 accumulation.
    gated: w is the fused gate|up weight [2F, K] and y [M, F] = act(gate) * up (the rounding
    of cs_gated_act).  splits: K split (0 = the library's choice); the fp32 partials are a
    per-call tensor (inside a capture it belongs to the graph's pool)."""
    return _gemm("cs_gemm_bf16", x, w, gated, act, splits, variant, out)


def gemm_packed(x: torch.Tensor, pw: PackedWeight, *, gated: bool = False, act: str = "silu",
                splits: int = 0, variant: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.gemm on a packed weight (cs_gemm_bf16_packed, variants 0 / 2 / 3 / 4): bitwise the
    unpacked result."""
    return _gemm("gemm_packed", x, pw, gated, act, splits, variant, out)


def gemm_packed_partials(x: torch.Tensor, pw: PackedWeight, *, splits: int,
                         variant: int = 0) -> SplitPartials:
    """gemm_partials on a packed weight (cs_gemm_bf16_packed with y = NULL)."""
    return _gemm("gemm_packed_partials", x, pw, splits=splits, variant=variant, partials=True)


def gemm_partials(x: torch.Tensor, w: torch.Tensor, *, splits: int, variant: int = 0) -> SplitPartials:
    """The fp32 partials [splits, M, N] of cs_gemm_bf16 with a K split, unfolded (y = NULL)."""
    return _gemm("gemm_partials", x, w, splits=splits, variant=variant, partials=True)


class Fp8Weight:
    """A [N, K] weight as OCP e4m3fn codes with one power-of-two scale per row, in
    cs_gemm_w8_pack's fragment-major layout: ``data`` the packed codes (uint8 [N * K]), ``exps``
    the row exponents (int8 [N]).  ``fallback``: the cs_gemm_pack'ed copy of its bf16 twin, if
    one is kept, for the calls that stay on the bf16 routes."""

    def __init__(self, data: torch.Tensor, exps: torch.Tensor, N: int, K: int,
                 fallback: Optional[PackedWeight] = None):
        self.data, self.exps, self.N, self.K, self.fallback = data, exps, int(N), int(K), fallback

    @property
    def shape(self):
        return (self.N, self.K)


GEMM_W8_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned",
                             "gemm_w8_mi355x.json")
_w8_excluded: Optional[frozenset] = None
_w8_max_rows: Optional[int] = None


def gemm_w8_max_rows() -> int:
    """The largest row count cs_gemm_bf16_w8 takes (cs_gemm_w8_max_rows)."""
    global _w8_max_rows
    if _w8_max_rows is None:
        _w8_max_rows = int(_lib.load().cs_gemm_w8_max_rows())
    return _w8_max_rows


def gemm_w8_serves(M: int, N: int, K: int, gated: bool = False) -> bool:
    """Whether ``linear`` runs an Fp8Weight of this shape on cs_gemm_bf16_w8 at M rows: M within
    the kernel's range, N % 128 == 0, K % 64 == 0, and "M,N,K,gated" not in the exclusion list
    tuned/gemm_w8_mi355x.json (tools/w8_bench.py: the shapes measured no faster than the bf16
    route of the twin; read only)."""
    global _w8_excluded
    if _w8_excluded is None:
        ex = []
        if os.path.exists(GEMM_W8_TABLE):
            with open(GEMM_W8_TABLE) as f:
                ex = json.load(f).get("exclude", [])
        _w8_excluded = frozenset(ex)
    if M < 1 or M > gemm_w8_max_rows() or N % 128 or K % 64:
        return False
    return f"{M},{N},{K},{int(bool(gated))}" not in _w8_excluded


def _w8_operands(x: torch.Tensor, fw: Fp8Weight) -> bool:
    """Whether cs_gemm_bf16_w8 takes x: bf16 [M, K] on the GPU, unit column stride, 16-byte
    aligned rows."""
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] == fw.K
            and x.stride(1) == 1 and (x.stride(0) % 8 == 0 or x.shape[0] <= 1)
            and x.data_ptr() % 16 == 0)


def gemm_w8_pack(w: torch.Tensor, twin_out: Optional[torch.Tensor] = None) -> Fp8Weight:
    """The FP8 copy of w [N, K] bf16 (cs_gemm_w8_pack; N % 16 == 0, K % 64 == 0): codes =
    e4m3_rne(w * 2^-e[n]) with e[n] the smallest exponent that brings the row's amax to <= 448.
    twin_out (bf16 [N, K]; may be w itself) receives the twin value(code) * 2^e[n], the bf16
    weight every other route then computes on.  A non-finite input or a row whose twin is no
    bf16 number raises CSError and leaves twin_out untouched (reads the status: a host sync)."""
    L = _lib.load()
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.stride(1) != 1:
        raise CSError("gemm_w8_pack needs a bf16 [N, K] tensor with unit column stride")
    N, K = w.shape
    if twin_out is not None and (twin_out.shape != w.shape or twin_out.dtype != torch.bfloat16
                                 or twin_out.stride(1) != 1):
        raise CSError("twin_out must be a bf16 [N, K] tensor with unit column stride")
    _require_cuda(w, twin_out)
    data = torch.empty(N * K, dtype=torch.uint8, device=w.device)
    exps = torch.empty(N, dtype=torch.int8, device=w.device)
    status = torch.empty(1, dtype=torch.int32, device=w.device)
    rc = L.cs_gemm_w8_pack(w.data_ptr(), w.stride(0), N, K, data.data_ptr(), exps.data_ptr(),
                           _ptr(twin_out), 0 if twin_out is None else twin_out.stride(0),
                           status.data_ptr(), _stream())
    _lib.check(rc, "cs_gemm_w8_pack")
    st = int(status.item())
    if st:
        why = " and ".join(t for b, t in ((1, "an Inf or NaN input"),
                                          (2, "a row whose FP8 twin is no bf16 number")) if st & b)
        raise CSError(f"gemm_w8_pack refused the weight (status {st}): {why}")
    return Fp8Weight(data, exps, N, K)


def gemm_w8_from_codes(codes: torch.Tensor, exps: torch.Tensor) -> Fp8Weight:
    """An Fp8Weight of given e4m3fn codes (uint8 [N, K]) and row exponents (int8 [N]):
    cs_gemm_w8_pack_codes, the layout permutation alone."""
    L = _lib.load()
    if codes.dim() != 2 or codes.dtype != torch.uint8 or not codes.is_contiguous():
        raise CSError("gemm_w8_from_codes needs contiguous uint8 codes [N, K]")
    N, K = codes.shape
    if exps.shape != (N,) or exps.dtype != torch.int8:
        raise CSError("exps must be int8 [N]")
    _require_cuda(codes, exps)
    data = torch.empty(N * K, dtype=torch.uint8, device=codes.device)
    rc = L.cs_gemm_w8_pack_codes(codes.data_ptr(), N, K, data.data_ptr(), _stream())
    _lib.check(rc, "cs_gemm_w8_pack_codes")
    return Fp8Weight(data, exps.contiguous().clone(), N, K)


def _gemm_w8(x: torch.Tensor, fw: Fp8Weight, gated: bool = False, act: str = "silu",
             splits: int = 0, out: Optional[torch.Tensor] = None, partials: bool = False):
    L = _lib.load()
    if not _w8_operands(x, fw):
        raise CSError("gemm_w8 needs bf16 x [M, K] with unit column stride and 16-byte aligned rows")
    if partials and splits < 2:
        raise CSError("gemm_w8_partials needs splits >= 2")
    M, N, K = x.shape[0], fw.N, fw.K
    n_out = N // 2 if gated else N
    if out is None and not partials:
        out = torch.empty(M, n_out, dtype=torch.bfloat16, device=x.device)
    if out is not None and (out.shape != (M, n_out) or out.dtype != torch.bfloat16 or out.stride(1) != 1):
        raise CSError("out must be a bf16 [M, N] tensor with unit column stride")
    _require_cuda(x, fw.data, fw.exps, out)
    if gated:
        splits = 1
    elif splits <= 0:
        splits = max(1, int(L.cs_gemm_w8_splits(M, N, K, 0)))
    ldx = x.stride(0) if M > 1 else K
    ldy = 0 if out is None else out.stride(0) if M > 1 else n_out
    if out is not None and splits > 1 and (ldy % 8 or out.data_ptr() % 16):
        # the split-K fold stores 16-byte vectors: fold into an aligned tensor, then copy
        out.copy_(_gemm_w8(x, fw, splits=splits))
        return out
    part = torch.empty(splits, M, N, dtype=torch.float32, device=x.device) if splits > 1 else None
    rc = L.cs_gemm_bf16_w8(x.data_ptr(), ldx, fw.data.data_ptr(), fw.exps.data_ptr(), _ptr(out), ldy,
                           M, N, K, splits, int(bool(gated)), _ACT[act], _ptr(part), _stream())
    _lib.check(rc, "cs_gemm_bf16_w8")
    return SplitPartials(part) if partials else out


def gemm_w8(x: torch.Tensor, fw: Fp8Weight, *, gated: bool = False, act: str = "silu",
            splits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = bf16(2^e[n] * sum_k x[m][k] * value(code[n][k])) (cs_gemm_bf16_w8): ops.gemm on an
    Fp8Weight, M <= gemm_w8_max_rows().  It differs from ops.gemm on the weight's bf16 twin only
    by the accumulation order.  gated, act, splits, out as ops.gemm."""
    return _gemm_w8(x, fw, gated, act, splits, out)


def gemm_w8_add(x: torch.Tensor, fw: Fp8Weight, h: torch.Tensor, *, splits: int = 0) -> torch.Tensor:
    """h += x @ w.T in place (cs_gemm_bf16_w8_add): h [M, N] bf16; the fp32 product (a K split:
    its fold) is added to h before the one rounding to bf16."""
    L = _lib.load()
    if not _w8_operands(x, fw):
        raise CSError("gemm_w8_add needs bf16 x [M, K] with unit column stride and 16-byte aligned rows")
    M, N, K = x.shape[0], fw.N, fw.K
    if h.shape != (M, N) or h.dtype != torch.bfloat16 or h.stride(1) != 1:
        raise CSError("h must be a bf16 [M, N] tensor with unit column stride")
    _require_cuda(x, fw.data, fw.exps, h)
    if splits <= 0:
        splits = max(1, int(L.cs_gemm_w8_splits(M, N, K, 0)))
    ldh = h.stride(0) if M > 1 else N
    if splits > 1 and (ldh % 8 or h.data_ptr() % 16):
        raise CSError("gemm_w8_add with a K split needs h 16-byte aligned with a row stride % 8 == 0")
    part = torch.empty(splits, M, N, dtype=torch.float32, device=x.device) if splits > 1 else None
    rc = L.cs_gemm_bf16_w8_add(x.data_ptr(), x.stride(0) if M > 1 else K, fw.data.data_ptr(),
                               fw.exps.data_ptr(), _ptr(h), ldh, M, N, K, splits, _ptr(part), _stream())
    _lib.check(rc, "cs_gemm_bf16_w8_add")
    return h


def gemm_w8_partials(x: torch.Tensor, fw: Fp8Weight, *, splits: int) -> SplitPartials:
    """The fp32 partials [splits, M, N] of cs_gemm_bf16_w8 with a K split, unfolded (y = NULL)."""
    return _gemm_w8(x, fw, splits=splits, partials=True)


def hist_rows_update(src_rows: torch.Tensor, dst_rows: torch.Tensor, parent: torch.Tensor,
                     hist_base: torch.Tensor, *, n_rows: int, row_base: int = 0) -> None:
    """dst_rows[s, j] = src_rows[parent[s], j] for j < hist_base, else row_base + s
    (cs_hist_rows_update): a row-layout history's beam / tree step, no K / V moved.
    src_rows [S_src, ldh], dst_rows [S, ldh], parent [S] indexes src_rows; n_rows = the
    K / V buffer's row count (row_base + S beyond it is rejected).  With CS_DEBUG_TABLES=1
    the parents and the source table's entries are checked on the host as well."""
    L_ = _lib.load()
    if src_rows.dtype != torch.int32 or dst_rows.dtype != torch.int32 or \
            src_rows.dim() != 2 or dst_rows.dim() != 2 or src_rows.shape[1] != dst_rows.shape[1] or \
            not src_rows.is_contiguous() or not dst_rows.is_contiguous():
        raise CSError("slot tables must be contiguous int32 [S, ldh] tensors of one ldh")
    S, ldh = dst_rows.shape
    if parent.dtype != torch.int64 or parent.numel() != S or hist_base.dtype != torch.int32:
        raise CSError("parent must be int64 [S], hist_base int32 [1]")
    _require_cuda(src_rows, dst_rows, parent, hist_base)
    if _DEBUG_TABLES and S and not torch.cuda.is_current_stream_capturing():
        if int(parent.min()) < 0 or int(parent.max()) >= src_rows.shape[0]:
            raise CSError("hist_rows_update: a parent does not index the source table")
        if int(src_rows.min()) < 0 or int(src_rows.max()) >= int(n_rows):
            raise CSError("hist_rows_update: the source table names a row past n_rows")
    rc = L_.cs_hist_rows_update(src_rows.data_ptr(), dst_rows.data_ptr(), parent.data_ptr(),
                                hist_base.data_ptr(), S, ldh, int(row_base), int(n_rows),
                                _stream())
    _lib.check(rc, "cs_hist_rows_update")


def blocked_vt(v: torch.Tensor) -> torch.Tensor:
    """V rows [..., keys, D] (keys a multiple of 32) -> the kernels' V^T in 32-key tiles
    [..., keys/32, D, 32] (contiguous)."""
    *lead, n, D = v.shape
    return v.reshape(*lead, n // 32, 32, D).transpose(-1, -2).contiguous()


def rows_from_blocked(vt: torch.Tensor) -> torch.Tensor:
    """Inverse of blocked_vt: [..., nb, D, 32] -> [..., nb * 32, D]."""
    *lead, nb, D, w = vt.shape
    return vt.transpose(-1, -2).reshape(*lead, nb * w, D)


def _problem_args(U: torch.Tensor, *others: Optional[torch.Tensor]):
    """The solvers' problems U [A, m] or [P, A, m] as (batched, P, A, m, ldu, ldp, device)."""
    if U.dim() not in (2, 3) or U.dtype != torch.float64 or (U.stride(-1) != 1 and U.shape[-1] > 1):
        raise CSError("U must be [A, m] or [P, A, m] float64 with unit column stride")
    _require_cuda(U, *others)
    batched = U.dim() == 3
    P = U.shape[0] if batched else 1
    A, m = U.shape[-2], U.shape[-1]
    ldu = U.stride(-2) if A > 1 else m
    ldp = U.stride(0) if batched and P > 1 else max(A, 1) * ldu
    return batched, P, A, m, ldu, ldp, U.device


def nash_lottery(U: torch.Tensor, max_iters: int = 1000, tol: float = 1e-10,
                 variant: int = 0) -> Dict[str, torch.Tensor]:
    """The Nash-welfare lottery of every problem of U in one launch (cs_nash_lottery).

    U [A, m] or [P, A, m] float64 utilities with unit column stride (A <= 64, m <= 16384).
    Returns {"p": [.., m] the lottery, "a": [.., A] = U p, "F": [..] = sum_i log a_i,
    "gap": [..] the Frank-Wolfe certificate max_j g_j - A, "iters": [..] int32}; a problem with
    a negative or non-finite utility or an all-zero agent row gets iters = -1 and NaN.
    variant: 0 the library's choice, 1 U staged in LDS, 2 U read from global memory (bitwise
    equal outputs).  Restates FW_nash_welfare (core.py:116-168)."""
    L = _lib.load()
    batched, P, A, m, ldu, ldp, dev = _problem_args(U)
    p = torch.empty((P, m), dtype=torch.float64, device=dev)
    a = torch.empty((P, A), dtype=torch.float64, device=dev)
    F = torch.empty(P, dtype=torch.float64, device=dev)
    gap = torch.empty(P, dtype=torch.float64, device=dev)
    iters = torch.empty(P, dtype=torch.int32, device=dev)
    rc = L.cs_nash_lottery(U.data_ptr(), P, A, m, ldu, ldp, int(max_iters), float(tol), int(variant),
                           p.data_ptr(), a.data_ptr(), F.data_ptr(), gap.data_ptr(),
                           iters.data_ptr(), _stream())
    _lib.check(rc, "cs_nash_lottery")
    out = {"p": p, "a": a, "F": F, "gap": gap, "iters": iters}
    return out if batched else {k: v[0] for k, v in out.items()}


MAXIMIN_MAX_PIVOTS = _lib.MAXIMIN_MAX_PIVOTS
_mask_cache: "collections.OrderedDict" = collections.OrderedDict()   # (device, bytes) -> device copy


def coalition_masks(masks, A: int) -> np.ndarray:
    """masks (ints, or a uint64 / int64 array) as the uint64 array the entry point takes, checked:
    every mask is a nonempty set of agents below A."""
    try:
        ints = [operator.index(x) for x in np.asarray(masks, dtype=object).reshape(-1)]
    except (TypeError, ValueError) as e:
        raise CSError(f"coalition masks must be integers: {e}") from e
    if not ints:
        raise CSError("need at least one coalition mask")
    if any(x <= 0 or x >> A for x in ints):
        raise CSError(f"every coalition mask must be a nonempty set of agents below {A}")
    return np.array(ints, dtype=np.uint64)


def _masks_on(device: torch.device, host: np.ndarray) -> torch.Tensor:
    key = (str(device), host.tobytes())
    t = _mask_cache.get(key)
    if t is None:
        t = torch.as_tensor(host.view(np.int64), device=device)
        _mask_cache[key] = t
        while len(_mask_cache) > 8:
            _mask_cache.popitem(last=False)
    else:
        _mask_cache.move_to_end(key)
    return t


def maximin_lottery(U: torch.Tensor, base: Optional[torch.Tensor] = None, masks=None,
                    max_pivots: int = MAXIMIN_MAX_PIVOTS, *, with_q: bool = True,
                    with_lam: bool = True) -> Dict[str, torch.Tensor]:
    """The matrix game max_q min_{i in S} (U_i . q) / base_i of every (problem, coalition) in one
    launch (cs_maximin_lottery): the maximin lottery and the coalition-improvement factor.

    U [A, m] or [P, A, m] float64 with unit column stride (A <= 64, m <= 16384); base [A] or
    [P, A] float64 (None: ones); masks: C coalition bit masks (bit i = agent i) as host integers,
    shared by all problems (None: one coalition of all agents).
    Returns {"alpha": |S| / A * value, "q": the optimal lottery [.., m], "lam": the dual weights
    on the agents [.., A], "pivots": int32}, each with leading dimensions [P] (batched U) and [C]
    (masks given).  pivots = -1 and NaN: a negative or non-finite utility in the problem, a
    member's base not finite and positive, or a member's row all zero; -2 and NaN: max_pivots
    exhausted.  with_q / with_lam = False leave that output out.
    Restates the LPs of egalitarian_lottery and max_coalition_improvement (core.py:171-279)."""
    L = _lib.load()
    batched, P, A, m, ldu, ldp, dev = _problem_args(U, base)
    if base is not None:
        if base.dtype != torch.float64 or tuple(base.shape) != ((P, A) if batched else (A,)):
            raise CSError("base must be float64 of shape [A] (or [P, A] for batched U)")
        base = base.contiguous()
    if masks is None:
        C, mh, md = 1, None, None
    else:
        host = coalition_masks(masks, A)
        C, mh, md = host.size, host.ctypes.data, _masks_on(dev, host).data_ptr()
    alpha = torch.empty((P, C), dtype=torch.float64, device=dev)
    q = torch.empty((P, C, m), dtype=torch.float64, device=dev) if with_q else None
    lam = torch.empty((P, C, A), dtype=torch.float64, device=dev) if with_lam else None
    pivots = torch.empty((P, C), dtype=torch.int32, device=dev)
    rc = L.cs_maximin_lottery(U.data_ptr(), P, A, m, ldu, ldp, _ptr(base), mh, md, C,
                              int(max_pivots), alpha.data_ptr(), _ptr(q), _ptr(lam),
                              pivots.data_ptr(), _stream())
    _lib.check(rc, "cs_maximin_lottery")
    out = {"alpha": alpha, "pivots": pivots}
    if with_q:
        out["q"] = q
    if with_lam:
        out["lam"] = lam
    if masks is None:
        out = {k: v[:, 0] for k, v in out.items()}
    return out if batched else {k: v[0] for k, v in out.items()}


def _tree_sizes(B: int, L: int) -> list:
    """A token tree's level sizes B^(t+1); [0] for a shape the entry points reject (unallocated)."""
    sizes = [B ** (t + 1) for t in range(L)] if 1 <= B and 1 <= L <= 64 else [0]
    return sizes if sizes[-1] <= 16384 else [0]


def lottery_policy(p: torch.Tensor, B: int, L: int, *, flat: bool = False):
    """The token policy a lottery over the B^L leaves (lexicographic order) induces
    (cs_lottery_policy): a list over the levels t = 0..L-1 of pi[t][s, b] = mass(s + b) / mass(s),
    [B^t, B] float64 (with a leading P for p [P, m]), views of one output; a prefix of mass <= 0
    has the uniform 1/B.  flat=True returns that one output instead, [sum_t B^(t+1)] (or with a
    leading P): the levels concatenated, what policy_rollout takes.  Restates the masses and
    step probabilities of induced_policy_rollout (core.py:303-325)."""
    L_ = _lib.load()
    B, L = int(B), int(L)
    if p.dim() not in (1, 2) or p.dtype != torch.float64 or not p.is_contiguous():
        raise CSError("p must be a contiguous float64 [m] or [P, m] tensor")
    _require_cuda(p)
    batched = p.dim() == 2
    P = p.shape[0] if batched else 1
    sizes = _tree_sizes(B, L)
    if sizes[-1] and p.shape[-1] != sizes[-1]:
        raise CSError(f"p has {p.shape[-1]} leaves, B^L is {sizes[-1]}")
    out = torch.empty((P, sum(sizes)), dtype=torch.float64, device=p.device)
    rc = L_.cs_lottery_policy(p.data_ptr(), P, B, L, out.data_ptr(), _stream())
    _lib.check(rc, "cs_lottery_policy")
    if flat:
        return out if batched else out[0]
    levels, at = [], 0
    for n in sizes:
        blk = out[:, at:at + n].view(P, n // B, B)
        levels.append(blk if batched else blk[0])
        at += n
    return levels


def pcg64_state(seed) -> np.ndarray:
    """The stream of ``np.random.default_rng(seed)`` as policy_rollout takes it: uint64 [4], the
    PCG64 state's high and low word, then the increment's high and low word."""
    st = np.random.PCG64(seed).state["state"]
    lo64 = (1 << 64) - 1
    return np.array([st["state"] >> 64, st["state"] & lo64, st["inc"] >> 64, st["inc"] & lo64],
                    dtype=np.uint64)


def _rng_words(rng_state, P: int, batched: bool, device: torch.device) -> torch.Tensor:
    """rng_state as the int64 bit patterns [P, 4] on the device."""
    if isinstance(rng_state, torch.Tensor):
        t = rng_state
        if t.dtype == torch.uint64:
            t = t.view(torch.int64)
        if t.dtype != torch.int64:
            raise CSError("rng_state must hold 64-bit words (uint64, or int64 bit patterns)")
        _require_cuda(t)
        if t.device != device:
            raise CSError(f"tensors on different devices: {device} vs {t.device}")
    else:
        host = np.ascontiguousarray(rng_state)
        if host.dtype != np.uint64 and host.dtype != np.int64:
            raise CSError("rng_state must hold 64-bit words (uint64, or int64 bit patterns)")
        t = torch.as_tensor(host.view(np.int64), device=device)
    if tuple(t.shape) != ((P, 4) if batched else (4,)):
        raise CSError("rng_state must be [4] (or [P, 4] for a batched policy): "
                      "state high, state low, increment high, increment low")
    return t.reshape(P, 4).contiguous()


def policy_rollout(policy, B: int, L: int, rng_state, num_samples: int, first_sample: int = 0,
                   counts: Optional[torch.Tensor] = None,
                   with_leaves: bool = False) -> Dict[str, torch.Tensor]:
    """Leaves sampled step by step from a token policy with numpy's own draws, counted per leaf
    (cs_policy_rollout): sample i takes the draws i * L .. i * L + L - 1 of
    ``default_rng(seed)``, each step is ``rng.choice(B, p=policy row)``.

    policy: lottery_policy's result, either its list of levels or its flat=True tensor
    [sum_t B^(t+1)] (or [P, ...]), float64; any token policy in that layout.
    rng_state: pcg64_state(seed), [4] or [P, 4] (one stream per problem): a host uint64 array, or
    a device tensor of uint64 / int64 bit patterns.
    This call does the samples first_sample .. first_sample + num_samples - 1 and ADDS their
    counts to ``counts`` (int64 [m] or [P, m]; None: fresh zeros), so a split rollout
    accumulates to the counts of one call.
    Returns {"counts", "status": int32 [..], "leaves": int32 [.., num_samples] with with_leaves}.
    status -1: the problem's policy holds a negative or non-finite entry or a row that does not
    sum to 1 within 2^-26 (where numpy's choice raises); its counts and leaves are untouched.
    Restates the sampling loop of induced_policy_rollout (core.py:313-332)."""
    L_ = _lib.load()
    B, L = int(B), int(L)
    num_samples, first_sample = int(num_samples), int(first_sample)
    if isinstance(policy, (list, tuple)):
        if not policy or any(not isinstance(t, torch.Tensor) for t in policy):
            raise CSError("policy levels must be a non-empty list of tensors")
        lead = policy[0].dim() == 3
        policy = torch.cat([t.reshape(t.shape[0], -1) if lead else t.reshape(-1) for t in policy],
                           dim=-1)
    if policy.dim() not in (1, 2) or policy.dtype != torch.float64:
        raise CSError("policy must be float64 [sum_t B^(t+1)] or [P, sum_t B^(t+1)] "
                      "(or lottery_policy's list of levels)")
    _require_cuda(policy, counts)
    policy = policy.contiguous()
    batched = policy.dim() == 2
    P = policy.shape[0] if batched else 1
    sizes = _tree_sizes(B, L)
    m = sizes[-1]
    if m and policy.shape[-1] != sum(sizes):
        raise CSError(f"policy has {policy.shape[-1]} entries per problem, "
                      f"sum_t B^(t+1) is {sum(sizes)}")
    dev = policy.device
    rng = _rng_words(rng_state, P, batched, dev)
    if counts is None:
        counts = torch.zeros((P, m) if batched else (m,), dtype=torch.int64, device=dev)
    elif (counts.dtype != torch.int64 or not counts.is_contiguous()
          or tuple(counts.shape) != ((P, m) if batched else (m,))):
        raise CSError("counts must be a contiguous int64 [m] (or [P, m]) tensor")
    if with_leaves and P * num_samples >= 2 ** 31:
        raise CSError("with_leaves needs P * num_samples <= 2^31 - 1")
    work = torch.empty_like(policy)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    leaves = None
    if with_leaves:      # -1: the leaves of a problem of status -1 stay untouched
        leaves = torch.full((P, max(num_samples, 0)), -1, dtype=torch.int32, device=dev)
    rc = L_.cs_policy_rollout(policy.data_ptr(), P, B, L, rng.data_ptr(), first_sample, num_samples,
                              work.data_ptr(), counts.data_ptr(), _ptr(leaves), status.data_ptr(),
                              _stream())
    _lib.check(rc, "cs_policy_rollout")
    out = {"counts": counts, "status": status if batched else status[0]}
    if with_leaves:
        out["leaves"] = leaves if batched else leaves[0]
    return out


def _valid_u8(v: Optional[torch.Tensor], shape: tuple, name: str, dims: Optional[str] = None):
    """An optional bool / uint8 mask of ``shape`` as uint8; ``dims`` spells it in the message."""
    if v is None:
        return None
    if v.dtype not in (torch.bool, torch.uint8) or tuple(v.shape) != tuple(shape):
        raise CSError(f"{name} must be a bool or uint8 {dims or list(shape)} tensor")
    return v.to(torch.uint8).contiguous()


SCHULZE_KINDS = {"rankings": _lib.SCHULZE_RANKINGS, "scores": _lib.SCHULZE_SCORES,
                 "defeats": _lib.SCHULZE_DEFEATS, "strengths": _lib.SCHULZE_STRENGTHS}


def schulze(x: torch.Tensor, kind: str = "rankings", valid: Optional[torch.Tensor] = None,
            ballot: Optional[torch.Tensor] = None, *, with_defeats: bool = True,
            with_strengths: bool = True) -> Dict[str, torch.Tensor]:
    """Schulze rank aggregation of a batch of elections in one launch (cs_schulze), one workgroup
    per election.

    x by ``kind``: "rankings" int32 [E, R, C] (lower is better, ties allowed), "scores" float32
    [E, R, C] (higher is better; a NaN prefers nothing), "defeats" int32 [E, C, C] (skips the
    pairwise count), "strengths" int32 [E, C, C] (skips the path strengths too).  C <= 128,
    R <= 65536.  valid [E, R] (bool or uint8; rankings and scores only): the voters that count.
    ballot int32 [E, C]: the tie-breaking ballot (any values, repeats allowed).
    Returns {"defeats" [E, C, C] (rankings / scores, with_defeats), "strengths" [E, C, C] (all
    but kind "strengths", with_strengths), "ranking" [E, C] the tied social ranking, "untied"
    [E, C] (ballot given), "winner" [E] the lowest index of rank 0 (of "untied" when there is
    one), "status" [E]}, all int32.  status -1: a counted rank outside [0, C - 1] or a nonzero
    diagonal (the reference's ValueErrors), -2: valid leaves no voter; that election's other
    outputs are -1, the rest of the batch is unaffected.
    Restates _schulze_compute_pairwise_defeats, _schulze_compute_strongest_path_strengths,
    _schulze_rank_candidates and _hm_untie_ranking_with_ballot
    (src/methods/habermas_machine.py:992-1160)."""
    L = _lib.load()
    if kind not in SCHULZE_KINDS:
        raise CSError(f"unknown kind {kind!r} (one of {sorted(SCHULZE_KINDS)})")
    k = SCHULZE_KINDS[kind]
    voters = k <= _lib.SCHULZE_SCORES
    want = torch.float32 if k == _lib.SCHULZE_SCORES else torch.int32
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != want:
        raise CSError(f"x must be a {want} tensor [E, R, C] (rankings, scores) or [E, C, C] "
                      f"(defeats, strengths) for kind {kind!r}")
    _require_cuda(x, valid, ballot)
    if not voters and x.shape[1] != x.shape[2]:
        raise CSError(f"{kind} must be square per election, got {tuple(x.shape)}")
    if not voters and valid is not None:
        raise CSError("valid applies to rankings and scores only")
    x = x.contiguous()
    E, R, C = x.shape
    dev = x.device
    valid = _valid_u8(valid, (E, R), "valid", "[E, R]")
    if ballot is not None:
        if ballot.dtype != torch.int32 or tuple(ballot.shape) != (E, C):
            raise CSError("ballot must be an int32 [E, C] tensor")
        ballot = ballot.contiguous()

    def new(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    defeats = new(E, C, C) if voters and with_defeats else None
    strengths = new(E, C, C) if k != _lib.SCHULZE_STRENGTHS and with_strengths else None
    ranking, winner, status = new(E, C), new(E), new(E)
    untied = new(E, C) if ballot is not None else None
    rc = L.cs_schulze(x.data_ptr(), k, E, R, C, _ptr(valid), _ptr(ballot), _ptr(defeats),
                      _ptr(strengths), ranking.data_ptr(), _ptr(untied), winner.data_ptr(),
                      status.data_ptr(), _stream())
    _lib.check(rc, "cs_schulze")
    out = {"ranking": ranking, "winner": winner, "status": status}
    for name, t in (("defeats", defeats), ("strengths", strengths), ("untied", untied)):
        if t is not None:
            out[name] = t
    return out


# --- text encoder (csrc/encoder.hip, encoder_attn_kernel in csrc/attn.hip) ----------------
def _vec_bf16(t: torch.Tensor, d: int, name: str) -> None:
    if t.dtype != torch.bfloat16 or t.numel() != d or not t.is_contiguous():
        raise CSError(f"{name} must be a contiguous bfloat16 [{d}] tensor")


def _out_like(out: Optional[torch.Tensor], shape: tuple, device: torch.device, what: str):
    """(out, row stride): a fresh bf16 ``shape`` when None, else bf16 rows of it or CSError(what)."""
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=device)
    ld = _rows2d(out, "out")
    if tuple(out.shape) != tuple(shape):
        raise CSError(what)
    return out, ld


def _ragged_args(cu_seqlens: torch.Tensor, n_tok: int, max_seqlen: int):
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1 or \
            not cu_seqlens.is_contiguous():
        raise CSError("cu_seqlens must be a contiguous int32 [n_text + 1] tensor")
    if max_seqlen < 0 or max_seqlen > n_tok:
        raise CSError("max_seqlen must be the longest text's length")
    return int(cu_seqlens.numel()) - 1


def embed_layer_norm(ids: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int,
                     word_emb: torch.Tensor, pos_emb: torch.Tensor, type_emb: torch.Tensor,
                     weight: torch.Tensor, bias: torch.Tensor, eps: float,
                     status: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm(word_emb[ids] + pos_emb[offset within the text] + type_emb[0]) of a ragged batch
    (cs_embed_layer_norm): ids int32 [n_tok], cu_seqlens int32 [n_text + 1], tables bf16
    [vocab | n_pos | >= 1, d]; returns bf16 [n_tok, d].  A text longer than the position table
    raises; ``status`` (int32 [1], zeroed by the caller) receives -1 if an id is outside the
    vocabulary (that row is zeros) -- without it the check is made here, with a sync."""
    L = _lib.load()
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise CSError("ids must be a contiguous int32 [n_tok] tensor")
    n_tok = int(ids.numel())
    n_text = _ragged_args(cu_seqlens, n_tok, int(max_seqlen))
    for t, name in ((word_emb, "word_emb"), (pos_emb, "pos_emb"), (type_emb, "type_emb")):
        if t.dim() != 2 or t.dtype != torch.bfloat16 or not t.is_contiguous() or \
                t.shape[1] != word_emb.shape[1] or t.shape[0] < 1:
            raise CSError(f"{name} must be a contiguous bfloat16 [n, d] tensor")
    d = int(word_emb.shape[1])
    _vec_bf16(weight, d, "weight")
    _vec_bf16(bias, d, "bias")
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=ids.device)
    elif status.dtype != torch.int32 or status.numel() != 1:
        raise CSError("status must be an int32 [1] tensor")
    out, ldy = _out_like(out, (n_tok, d), ids.device, "out must be [n_tok, d]")
    _require_cuda(ids, cu_seqlens, word_emb, pos_emb, type_emb, weight, bias, status, out)
    rc = L.cs_embed_layer_norm(ids.data_ptr(), cu_seqlens.data_ptr(), n_text, n_tok, int(max_seqlen),
                               word_emb.data_ptr(), int(word_emb.shape[0]), pos_emb.data_ptr(),
                               int(pos_emb.shape[0]), type_emb.data_ptr(), weight.data_ptr(),
                               bias.data_ptr(), d, float(eps), out.data_ptr(), ldy,
                               status.data_ptr(), _stream())
    _lib.check(rc, "cs_embed_layer_norm")
    if own and n_tok and int(status.item()) != 0:
        raise CSError("cs_embed_layer_norm failed (status -1): a token id outside the vocabulary "
                      "or a token outside every text")
    return out


def add_layer_norm(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor,
                   bias: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm(x + residual) * weight + bias (cs_add_layer_norm): [rows, d] bf16, fp32 sum and
    statistics, one rounding."""
    L = _lib.load()
    ldx = _rows2d(x, "x")
    rows, d = x.shape
    ldr = _rows2d(residual, "residual") if residual is not None else 0
    if residual is not None and residual.shape != x.shape:
        raise CSError("x and residual must share one shape")
    _vec_bf16(weight, d, "weight")
    _vec_bf16(bias, d, "bias")
    out, ldy = _out_like(out, (rows, d), x.device, "out must have x's shape")
    _require_cuda(x, residual, weight, bias, out)
    rc = L.cs_add_layer_norm(x.data_ptr(), ldx, _ptr(residual), ldr, weight.data_ptr(),
                             bias.data_ptr(), rows, d, float(eps), out.data_ptr(), ldy, _stream())
    _lib.check(rc, "cs_add_layer_norm")
    return out


def gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """erf-GELU in fp32 on bf16 rows [rows, F] (cs_gelu)."""
    L = _lib.load()
    ldx = _rows2d(x, "x")
    rows, F = x.shape
    out, ldy = _out_like(out, (rows, F), x.device, "out must have x's shape")
    _require_cuda(x, out)
    rc = L.cs_gelu(x.data_ptr(), ldx, rows, F, out.data_ptr(), ldy, _stream())
    _lib.check(rc, "cs_gelu")
    return out


def encoder_attention(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int, n_heads: int,
                      head_dim: int = 64, scale: Optional[float] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bidirectional attention of a ragged batch (cs_encoder_attention): qkv bf16 [n_tok, 3 H D]
    the fused projection (q | k | v), cu_seqlens int32 [n_text + 1]; returns bf16 [n_tok, H D].
    A token attends to its own text's keys only.  D = 64, texts of 1 .. 512 tokens."""
    L = _lib.load()
    ld = _rows2d(qkv, "qkv")
    n_tok = int(qkv.shape[0])
    n_text = _ragged_args(cu_seqlens, n_tok, int(max_seqlen))
    H, D = int(n_heads), int(head_dim)
    if qkv.shape[1] != 3 * H * D:
        raise CSError("qkv must be [n_tok, 3 * n_heads * head_dim]")
    if out is None:
        out = torch.empty(n_tok, H * D, dtype=torch.bfloat16, device=qkv.device)
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (n_tok, H * D) or not out.is_contiguous():
        raise CSError("out must be a contiguous bfloat16 [n_tok, H * D] tensor")
    _require_cuda(qkv, cu_seqlens, out)
    rc = L.cs_encoder_attention(qkv.data_ptr(), ld, cu_seqlens.data_ptr(), n_text, n_tok,
                                int(max_seqlen), H, D,
                                float(D ** -0.5 if scale is None else scale), out.data_ptr(),
                                _stream())
    _lib.check(rc, "cs_encoder_attention")
    return out


def cosine_welfare(E_s: torch.Tensor, E_a: torch.Tensor, valid_s: Optional[torch.Tensor] = None,
                   valid_a: Optional[torch.Tensor] = None, eps: float = 1e-9):
    """The evaluator's embedding utilities in one launch (cs_cosine_welfare), fp64 arithmetic:
    E_s float32 [S, d] statement embeddings, E_a float32 [A, d] opinion embeddings, valid_* bool
    or uint8 [S] / [A] (False: the embedding is missing).  Returns (cos [A, S], welfare [3, S])
    float64: 1 - scipy's cosine distance (0.0 for a zero vector, NaN for a missing or non-finite
    pair) and min / sum / sum log(max(c, eps)) over each statement's finite similarities (NaN
    when there is none) -- src/evaluation.py:239-307."""
    L = _lib.load()
    for t, name in ((E_s, "E_s"), (E_a, "E_a")):
        if t.dim() != 2 or t.dtype != torch.float32 or (t.numel() and t.stride(1) != 1):
            raise CSError(f"{name} must be a 2-D float32 tensor with unit column stride")
    S, d = E_s.shape
    A = E_a.shape[0]
    if E_a.shape[1] != d:
        raise CSError("E_s and E_a must share the embedding width")
    valid_s, valid_a = _valid_u8(valid_s, (S,), "valid_s"), _valid_u8(valid_a, (A,), "valid_a")
    _require_cuda(E_s, E_a, valid_s, valid_a)
    cos = torch.empty(A, S, dtype=torch.float64, device=E_s.device)
    wel = torch.empty(3, S, dtype=torch.float64, device=E_s.device)
    rc = L.cs_cosine_welfare(_ptr(E_s), E_s.stride(0) if S > 1 else d, _ptr(E_a),
                             E_a.stride(0) if A > 1 else d, _ptr(valid_s), _ptr(valid_a), S, A, d,
                             float(eps), _ptr(cos), _ptr(wel), _stream())
    _lib.check(rc, "cs_cosine_welfare")
    return cos, wel


# --- clustering (csrc/cluster.hip): StandardScaler, KMeans, nearest rows, all fp64 -----------
def _f64_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """A 2-D device tensor as contiguous float64 rows (a float32 input is widened)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point():
        raise CSError(f"{name} must be a 2-D floating-point tensor")
    _require_cuda(t)
    return t.to(torch.float64).contiguous()


def _kmeans_limits(n: int, d: int, k: int = 1, R: int = 1) -> None:
    if not (1 <= n <= _lib.KMEANS_MAX_N and 1 <= d <= _lib.KMEANS_MAX_D):
        raise CSError(f"need 1 <= n <= {_lib.KMEANS_MAX_N} and 1 <= d <= {_lib.KMEANS_MAX_D}, "
                      f"got n {n}, d {d}")
    if not (1 <= k <= _lib.KMEANS_MAX_K and 1 <= R <= _lib.KMEANS_MAX_R):
        raise CSError(f"need 1 <= k <= {_lib.KMEANS_MAX_K} and 1 <= restarts <= "
                      f"{_lib.KMEANS_MAX_R}, got k {k}, restarts {R}")
    if k > n:
        raise CSError(f"need k <= n, got k {k}, n {n}")


def _scratch(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def standardize(X: torch.Tensor):
    """StandardScaler().fit_transform on the device (cs_standardize), fp64: returns (Z, mean,
    scale) with the population variance and scale 1 for a constant feature (scikit-learn's rule,
    var <= n eps var + (n mean eps)^2).  A float32 X is widened first."""
    L = _lib.load()
    X = _f64_rows(X, "X")
    n, d = X.shape
    _kmeans_limits(n, d)
    Z = torch.empty_like(X)
    mean = torch.empty(d, dtype=torch.float64, device=X.device)
    scale = torch.empty_like(mean)
    ws = _scratch(L.cs_standardize_workspace_size(n, d), X.device)
    rc = L.cs_standardize(X.data_ptr(), d, n, d, Z.data_ptr(), d, mean.data_ptr(), scale.data_ptr(),
                          ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "cs_standardize")
    return Z, mean, scale


def kmeans_trials(k: int) -> int:
    """k-means++ candidates per centre, scikit-learn's 2 + int(log k)."""
    return 2 + int(np.log(k))


def _seed_draws(first, u, k: int):
    first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    R, T = first.size, kmeans_trials(k)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.shape != (R, k - 1, T):
        raise CSError(f"u must be [{R}, {k - 1}, {T}] (restarts, k - 1, 2 + int(log k)), got "
                      f"{u.shape}")
    return first, u, R, T


def kmeans_seed(Z: torch.Tensor, k: int, first, u, *, _ws: Optional[torch.Tensor] = None):
    """k-means++ of R restarts at once (cs_kmeans_seed) from numpy's draws: Z float64 [n, d]
    (centred), first [R] the first centres' rows, u [R, k - 1, T] uniforms in [0, 1) (host
    arrays).  Returns (centers [R, k, d] float64, indices [R, k] int32) on the device."""
    L = _lib.load()
    Z = _f64_rows(Z, "Z")
    n, d = Z.shape
    first, u, R, T = _seed_draws(first, u, k)
    _kmeans_limits(n, d, k, R)
    dev = Z.device
    ws = _ws if _ws is not None else _scratch(L.cs_kmeans_workspace_size(n, d, k, R), dev)
    first_d = torch.from_numpy(first).to(dev)
    u_d = torch.from_numpy(u).to(dev) if u.size else None
    centers = torch.empty(R, k, d, dtype=torch.float64, device=dev)
    indices = torch.empty(R, k, dtype=torch.int32, device=dev)
    rc = L.cs_kmeans_seed(Z.data_ptr(), d, n, d, k, R, T, first.ctypes.data,
                          u.ctypes.data if u.size else None, first_d.data_ptr(),
                          None if u_d is None else u_d.data_ptr(), centers.data_ptr(),
                          indices.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "cs_kmeans_seed")
    return centers, indices


def kmeans(Zs: torch.Tensor, k: int, first=None, u=None, *, n_init: Optional[int] = None,
           init: Optional[torch.Tensor] = None, max_iter: int = 300, tol: float = 1e-4,
           poll_every: int = 8, timings: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """The whole fit of KMeans on the device, fp64: Zs [n, d] is centred by its column mean,
    R = len(first) restarts are seeded (kmeans_seed) or started from ``init`` ([k, d] or
    [R, k, d], uncentred), iterated together (cs_kmeans_iterate: a finished restart's workgroups
    exit; ``live`` is read back every ``poll_every`` iterations, the only host syncs), and one
    restart is chosen per group of ``n_init`` consecutive restarts (default: all of them) by
    scikit-learn's sequential rule (cs_kmeans_finish).
    Returns labels [G, n] int32, centers [G, k, d] (uncentred), best [G], inertia [R],
    n_iter [R], done [R] (1 labels repeated, 2 tolerance or max_iter), indices [R, k] (-1 with
    init), mean [d], iterations (enqueued per restart).  ``timings`` (a dict) asks for the wall
    clock of each phase in ms, taken with a device synchronise at each phase's end."""
    L = _lib.load()
    Zs = _f64_rows(Zs, "Zs")
    n, d = Zs.shape
    dev = Zs.device
    if max_iter < 1 or poll_every < 1:
        raise CSError("need max_iter >= 1 and poll_every >= 1")
    if init is not None:
        C0 = init.to(torch.float64)
        _require_cuda(C0)
        if C0.dim() == 2:
            C0 = C0[None]
        if C0.dim() != 3 or tuple(C0.shape[1:]) != (k, d):
            raise CSError(f"init must be [{k}, {d}] or [R, {k}, {d}]")
        R = C0.shape[0]
    else:
        if first is None or (u is None and k > 1):
            raise CSError("kmeans needs the draws (first, u) or init")
        if u is None:
            u = np.zeros((len(first), 0, kmeans_trials(k)))
        first, u, R, _ = _seed_draws(first, u, k)
    _kmeans_limits(n, d, k, R)
    n_init = R if n_init is None else int(n_init)
    if n_init < 1 or R % n_init:
        raise CSError(f"the restarts ({R}) must be a multiple of n_init ({n_init})")
    G = R // n_init
    clock = [0.0]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            if name:
                timings[name] = timings.get(name, 0.0) + (now - clock[0]) * 1e3
            clock[0] = now

    lap(None)
    mean = Zs.mean(dim=0)
    Z = (Zs - mean).contiguous()
    ws = _scratch(L.cs_kmeans_workspace_size(n, d, k, R), dev)
    if init is not None:
        centers = (C0 - mean).contiguous()
        indices = torch.full((R, k), -1, dtype=torch.int32, device=dev)
    else:
        centers, indices = kmeans_seed(Z, k, first, u, _ws=ws)
    lap("seed_ms")
    state = torch.empty(2 * R + 1, dtype=torch.int32, device=dev)
    st = _stream()
    wsa = (ws.data_ptr(), ws.numel(), st)
    _lib.check(L.cs_kmeans_init(Z.data_ptr(), d, n, d, k, R, float(tol), state.data_ptr(), *wsa),
               "cs_kmeans_init")
    enq = 0
    while enq < max_iter:
        steps = min(poll_every, max_iter - enq)
        _lib.check(L.cs_kmeans_iterate(Z.data_ptr(), d, n, d, k, R, centers.data_ptr(),
                                       state.data_ptr(), steps, max_iter, *wsa), "cs_kmeans_iterate")
        enq += steps
        if int(state[2 * R].item()) == 0:
            break
    lap("iterate_ms")
    best = torch.empty(G, dtype=torch.int32, device=dev)
    labels = torch.empty(G, n, dtype=torch.int32, device=dev)
    out_c = torch.empty(G, k, d, dtype=torch.float64, device=dev)
    inertia = torch.empty(R, dtype=torch.float64, device=dev)
    n_iter = torch.empty(R, dtype=torch.int32, device=dev)
    rc = L.cs_kmeans_finish(Z.data_ptr(), d, n, d, k, R, n_init, centers.data_ptr(), mean.data_ptr(),
                            state.data_ptr(), best.data_ptr(), labels.data_ptr(), out_c.data_ptr(),
                            inertia.data_ptr(), n_iter.data_ptr(), *wsa)
    _lib.check(rc, "cs_kmeans_finish")
    lap("finish_ms")
    return {"labels": labels, "centers": out_c, "best": best, "inertia": inertia, "n_iter": n_iter,
            "done": state[:R].clone(), "indices": indices, "mean": mean, "iterations": enq}


def nearest_rows(Q: torch.Tensor, X: torch.Tensor):
    """For each row of Q the index of the nearest row of X (fp64 squared distance, the first
    lowest index on ties) and the Euclidean distance (cs_nearest_rows): (int32 [q], float64 [q]).
    sklearn.metrics.pairwise_distances_argmin_min(Q, X)."""
    L = _lib.load()
    Q, X = _f64_rows(Q, "Q"), _f64_rows(X, "X")
    q, d = Q.shape
    n = X.shape[0]
    if X.shape[1] != d:
        raise CSError("Q and X must share the feature width")
    _kmeans_limits(n, d)
    if not 1 <= q <= _lib.KMEANS_MAX_N:
        raise CSError(f"need 1 <= q <= {_lib.KMEANS_MAX_N}")
    idx = torch.empty(q, dtype=torch.int32, device=X.device)
    dist = torch.empty(q, dtype=torch.float64, device=X.device)
    ws = _scratch(L.cs_nearest_rows_workspace_size(q, n), X.device)
    rc = L.cs_nearest_rows(Q.data_ptr(), d, q, X.data_ptr(), d, n, d, idx.data_ptr(),
                           dist.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "cs_nearest_rows")
    return idx, dist
