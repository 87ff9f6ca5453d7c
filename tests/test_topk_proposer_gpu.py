"""The two vocab top-k proposers (cs_vocab_topk, and the proposer half of cs_beam_decode_step)
pinned with planted winners at every position class, and the top of the documented ranges.

Every row of a launch is one probe of tests/topk_ref.py: K winners and one first loser at the
elements where a chunk, a lane, a slot, a wave, a lane group or a packed word begins or ends, on
a flat or a stairs background, plus the families (all winners in one chunk, one per chunk, ties
across a chunk edge, +-inf / +-0 / NaN / saturated values, a partly filled output).  Expected
ids are (float64 capped value descending, id ascending, NaN last) and are met with no tolerance,
under a soft-cap as well; values are bit-exact without a cap and within
C_CAP * cap * 2^-24 + 2^-24 |ref| of cap * tanh(x / cap) with one.  Rows are views of a buffer
whose pad columns and bands hold the dtype's largest finite value.  tests/test_topk_cases_host.py
shows on the CPU that the cases reach every class in every role and reject thirteen wrong
proposers.

Measured on an MI355X: the file's 275 tests (6,768 cs_vocab_topk and 2,747 decode launches,
each run twice) take 33 s, the slowest 0.54 s; under a cap the device's values use at most 0.108
of their window; no planted case exposed a wrong id.  The launches of the last three tests ask
for 128 KiB of dynamic LDS and pass through launch_big_lds ("The vocab top-k
proposers at every position")."""
import numpy as np
import pytest
import torch

import topk_ref as T

pytestmark = pytest.mark.gpu

TORCH = {T.F32: torch.float32, T.BF16: torch.bfloat16, T.F16: torch.float16}
CASES = {c.name: c for c in T.all_cases()}
_worst = {}


def _rows(Ln, dev):
    """The launch's rows on the device: a [rows, V] view (row stride ld) of the poisoned buffer."""
    c = Ln.case
    flat, start = Ln.buffer()
    t = torch.from_numpy(flat).to(dev).to(TORCH[c.dtype])
    assert t.data_ptr() % 16 == 0
    return t[start:start + c.rows * c.ld].view(c.rows, c.ld)[:, :c.V]


def _bits(t):
    return torch.nan_to_num(t, nan=7.0).view(torch.int32)


def _note(cap, worst):
    _worst[cap] = max(_worst.get(cap, 0.0), worst)


TOPK_PARAMS = [(K, lb) for K in T.TOPK_K for lb in T.topk_vocabs(K)]


@pytest.mark.parametrize("K,label", TOPK_PARAMS, ids=[f"K{K}-V{lb}" for K, lb in TOPK_PARAMS])
def test_vocab_topk_planted_rows(ops, dev, K, label):
    """cs_vocab_topk at 1, 3 and 300 rows, three dtypes, three cap modes: the backgrounds at
    every row count, the families at 1 and 3 rows; every launch twice, bit for bit."""
    bad, n = [], 0
    for rows in T.TOPK_ROWS:
        for kind in (T.KINDS if rows < 300 else T.BACKGROUNDS):
            for ci, cap in enumerate(T.CAPS):
                for dt in T.DTYPES:
                    c = CASES[f"{dt}-topk-V{label}-K{K}-r{rows}"]
                    Ln = T.make_launch(c, kind, ci if rows < 300 else 0, cap)
                    x = _rows(Ln, dev)
                    assert x.stride(0) == c.ld or rows == 1
                    ids, vals = ops.vocab_topk(x, K, softcap=cap)
                    ids2, vals2 = ops.vocab_topk(x, K, softcap=cap)
                    b, w = T.check(Ln, ids.cpu().numpy(), vals.cpu().numpy())
                    if not (torch.equal(ids, ids2) and torch.equal(_bits(vals), _bits(vals2))):
                        b.append(f"{c.name}/{kind} cap {cap:g}: a relaunch gave other bits")
                    bad += b
                    _note(cap, w)
                    n += 1
    print(f"K {K} V {label}: {n} launches (each twice)")
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:20])


def _agents(c, dev, cache={}):
    """Agent logits and rewards of a decode case (random; shared by the case's launches)."""
    key = (c.dtype, c.A, c.rows, c.V)
    if key not in cache:
        cache.clear()
        g = torch.Generator(device=dev).manual_seed(c.A * 131 + c.rows * 7 + c.V)
        x = (torch.randn(c.A * c.rows, c.V, generator=g, device=dev) * 3.0).to(TORCH[c.dtype])
        R = -torch.rand(c.A, c.rows, generator=g, device=dev) * 20.0
        cache[key] = (x, R)
    return cache[key]


def _decode_once(ops, dev, ws, Ln):
    """One planted launch through cs_beam_decode_step, twice on one workspace: out_ids are the
    expected ids and cs_vocab_topk's; U, W and order are cs_beam_step's on the expected ids."""
    c = Ln.case
    ref = _rows(Ln, dev)
    assert (ref.data_ptr() % 16 == 0 and c.ld * T.ELT[c.dtype] % 16 == 0) == c.ref_vec
    x, R = _agents(c, dev)
    want = torch.from_numpy(Ln.exp_ids).to(dev)
    t_ids, t_vals = ops.vocab_topk(ref, c.K, softcap=Ln.cap)
    bad, w = T.check(Ln, t_ids.cpu().numpy(), t_vals.cpu().numpy())
    bad = ["cs_vocab_topk: " + b for b in bad]
    _note(Ln.cap, w)
    U, W, o, _ = ops.beam_step(x, want, R, "min", softcap=Ln.cap)
    for rep in range(2):
        ids, U2, W2, o2, _ = ops.beam_decode_step(ref, x, R, c.K, "min", softcap=Ln.cap, workspace=ws)
        b, _ = T.check(Ln, ids.cpu().numpy())
        bad += [f"cs_beam_decode_step (launch {rep}): " + s for s in b]
        head = f"{c.name}/{Ln.kind} cap {Ln.cap:g} launch {rep}: "
        if not torch.equal(ids, t_ids):
            bad.append(head + "out_ids differ from cs_vocab_topk's")
        if not (torch.equal(_bits(U), _bits(U2)) and torch.equal(_bits(W), _bits(W2))):
            bad.append(head + "U or W differ from cs_beam_step on the expected ids")
        if not torch.equal(o, o2):
            bad.append(head + "order differs from cs_beam_step on the expected ids")
    return bad


def _grid_orders(dev):
    """{rows first?} over the decode cases, from the device's CU count."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    return {T.decode_rows_first(T.decode_layout(c.A, c.rows, c.V, c.K, c.dtype)["row_blocks"], n_cu)
            for c in T.all_cases() if c.path == "decode"}


DECODE_PARAMS = [c.name for dt in T.DTYPES for c in T.decode_cases(dt)]


@pytest.mark.parametrize("name", DECODE_PARAMS)
def test_decode_proposer_planted_rows(ops, dev, name):
    """The decode proposer's four index maps (4 and 8 / 16 keys per lane, vector and scalar
    loads of full chunks, RAW words), its tail chunks, its cached and uncached merge and both
    grid orders: every family on the K = 10 aligned shapes and the uncached and 512-row shapes,
    the backgrounds and the special rows elsewhere, in three cap modes; the 2-beam shapes with a
    257-element tail sweep their whole class list."""
    assert _grid_orders(dev) == {True, False}
    ws = ops.Workspace(zeroed=True)
    c = CASES[name]
    full = "-K10-aligned" in name or "uncached" in name or "rows512" in name
    todo = [(k, ci, cap) for k in (T.KINDS if full else ("flat", "stairs", "special"))
            for ci, cap in enumerate(T.CAPS)]
    if "-kp4-r257-K10" in name:
        todo += [("flat", s, T.CAPS[s % 3]) for s in range(3, T.n_shifts(c))]
    bad = []
    for kind, shift, cap in todo:
        bad += _decode_once(ops, dev, ws, T.make_launch(c, kind, shift, cap))
    assert int(ws.buf[:4096].count_nonzero()) == 0          # the counters are left at zero
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:20])


def test_report_the_worst_share_of_a_cap_window(ops, dev):
    """What the device's fp32 cap used of its window, over the planted tests that ran before
    (and over one case's launches here)."""
    for dt in T.DTYPES:
        for cap in T.CAPS[1:]:
            Ln = T.make_launch(CASES[f"{dt}-topk-V4097-K50-r3"], "stairs", 2, cap)
            ids, vals = ops.vocab_topk(_rows(Ln, dev), 50, softcap=cap)
            bad, w = T.check(Ln, ids.cpu().numpy(), vals.cpu().numpy())
            assert not bad, "\n".join(bad[:20])
            _note(cap, w)
    print("worst |value - cap * tanh(x / cap)| as a share of its window: "
          + ", ".join(f"cap {c:g}: {w:.3f}" for c, w in sorted(_worst.items()) if c > 0))
    assert all(w <= 1.0 for w in _worst.values())


# --- the top of the documented ranges: launches with 128 KiB of dynamic LDS ------------------
@pytest.mark.parametrize("dt,V,rows", [(T.F32, 131073, 2), (T.BF16, 256000, 1)])
def test_vocab_topk_merge_of_more_than_8192_chunk_winners(ops, orc, dev, dt, V, rows):
    """nchunk * k = 8448 and 16128 keys: the merge kernel asks for 128 KiB of dynamic LDS."""
    c = T.Case(f"{dt}-topk-top-V{V}", "topk", dt, V, 256, rows, layout="aligned")
    assert 8192 < T.topk_nchunk(V) * 256 <= T.TOPK_MAX_KEYS
    for kind, cap in (("flat", 0.0), ("perchunk", 30.0), ("edge_ties", 0.0), ("special", 0.0)):
        Ln = T.make_launch(c, kind, 1, cap)
        with np.errstate(invalid="ignore"):
            o_ids, _ = orc.vocab_topk(np.ascontiguousarray(T.softcap64(Ln.x.astype(np.float64), cap)), 256)
        assert np.array_equal(o_ids, Ln.exp_ids)
        ids, vals = ops.vocab_topk(_rows(Ln, dev), 256, softcap=cap)
        bad, _ = T.check(Ln, ids.cpu().numpy(), vals.cpu().numpy())
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("k", [16384, 300])
def test_segmented_topk_sorts_16384_keys(ops, orc, dev, k):
    """seg_len = 16384 with k > 256: topk_kernel sorts 16384 keys in 128 KiB of dynamic LDS."""
    rng = np.random.default_rng(k)
    W = rng.integers(-40, 40, size=(2, 16384 + 3)).astype(np.float32) / 4        # heavy ties
    W[:, rng.integers(0, 16384, size=300)] = np.nan
    W[0, 1], W[0, 2], W[1, 16383] = -0.0, 0.0, np.inf
    W[1, 7] = -np.inf
    Wt = torch.as_tensor(W, device=dev)[:, :16384]
    idx, val = ops.topk(Wt, k)
    ref = orc.topk(W[:, :16384].astype(np.float64), k)
    assert np.array_equal(idx.cpu().numpy(), ref)
    v, r = val.cpu().numpy(), np.take_along_axis(W[:, :16384], ref, 1)
    assert np.array_equal(np.isnan(v), np.isnan(r)) and np.array_equal(v[~np.isnan(v)], r[~np.isnan(r)])


def test_beam_step_orders_8400_candidates(ops, orc, dev):
    """B * K = 8400: the order comes from topk_kernel behind the launch, over 16384 keys."""
    A, B, K, V = 2, 2, 4200, 5000
    g = torch.Generator().manual_seed(8400)
    logits = torch.round(torch.randn(A * B, V, generator=g) * 3.0)              # ties in W
    tgt = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(B)]).to(torch.int32)
    tgt[0, 5] = tgt[1, 4199] = -1
    R = -torch.rand(A, B, generator=g) * 20.0
    U, W, order, oval = ops.beam_step(logits.to(dev), tgt.to(dev), R.to(dev), "min")
    w = W.cpu().numpy()
    ref = orc.topk(w.astype(np.float64), B * K)[0]
    assert np.array_equal(order.cpu().numpy(), ref)
    assert torch.equal(_bits(oval), _bits(W[order.long()]))
    tok, _ = ops.logsoftmax_gather(logits.to(dev), tgt.to(dev).repeat(A, 1))
    U2 = (R.to(dev)[:, :, None] + tok.view(A, B, K)).reshape(A, B * K)
    assert torch.equal(_bits(U), _bits(U2))
