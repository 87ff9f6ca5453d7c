"""cs_vocab_sample (csrc/proposer.hip) against the fp64 Gumbel-max oracle at the edges: the
soft-capped instantiation, fp16, padded rows, n_draw 1 / 16, split and unsplit vocabularies,
masked and NaN tokens, rows with no selectable token, extreme seeds and exact ties.

Comparison rule, applied to every draw of every case (``_check``):

* the GPU id equals the oracle id, or the oracle margin m = s[best] - s[gpu id] satisfies
  0 < m <= tol.  An exact oracle tie (m == 0) is never excused: the lowest id must win.
* tol is twice the fp32 evaluation error of one perturbed score: 8 ulp of the largest
  magnitude M >= 1 among |x'/T| and the Gumbel term of the row (8 * 2^-23 * M), plus, under a
  soft-cap, 1e-5 / T (the bound the fp32 soft-capped values are held to in
  test_proposer_gpu.py).
* where the ids agree, |lp_gpu - lp_oracle| < 1e-3 (LP_TOL), and NaN where the oracle's is NaN.
* at most 1 % of a case's draws may be excused, and the case is first shown -- from the oracle
  alone, before the GPU output is looked at -- to have at most 1 % of its draws at risk
  (runner-up margin in (0, tol]).

Measured on the MI355X (printed under -s): 0 excused draws in every case; see DESIGN.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LP_TOL = 1e-3
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _host(t):
    """CPU tensor -> the array the oracle reads (bf16 as uint16 bit patterns), bf16 flag."""
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16), True
    return t.numpy(), False


def _oracle_side(orc, full, vocab, seeds, T, cap):
    """The oracle's draws and each draw's tolerance; asserts (from the oracle alone) that at
    most 1 % of the draws have their runner-up within the tolerance."""
    host, bf = _host(full)
    o = orc.gumbel_sample_rows(host, seeds.numpy(), T, cap, bf16=bf, vocab=vocab)
    tol = 2.0 * (8.0 * 2.0 ** -23 * o["scale"] + (1e-5 / T if cap else 0.0))
    at_risk = int(((o["gap"] > 0) & (o["gap"] <= tol)).sum())
    assert at_risk <= 0.01 * o["id"].size, f"{at_risk} of {o['id'].size} draws at risk: other seeds"
    return o, tol


def _check(ops, orc, dev, full, seeds, T=1.0, cap=0.0, vocab=None, narrow=False, label=""):
    """full [rows, ld] CPU logits, seeds [rows, n_draw] int64.  The kernel reads the first
    ``vocab`` columns: as a column slice (row stride ld), or with narrow=True as the whole
    tensor and vocab=.  Returns (ids, lp, oracle dict) as numpy."""
    vocab = full.shape[1] if vocab is None else vocab
    o, tol = _oracle_side(orc, full, vocab, seeds, T, cap)
    fd = full.to(dev)
    if narrow:
        ids, lp = ops.vocab_sample(fd, seeds.to(dev), temperature=T, softcap=cap, vocab=vocab)
    else:
        ids, lp = ops.vocab_sample(fd[:, :vocab], seeds.to(dev), temperature=T, softcap=cap)
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
    assert ids.shape == o["id"].shape and ids.dtype == np.int32
    differ = ids != o["id"]
    excused = int(differ.sum())
    if excused:
        host, bf = _host(full)
        m = orc.gumbel_sample_rows(host, seeds.numpy(), T, cap, bf16=bf, vocab=vocab,
                                   candidates=ids)["margin"][differ]
        # NaN (an id that is no selectable token) and 0 (an exact tie lost) both fail here
        assert np.all((m > 0) & (m <= tol[differ])), (label, ids[differ], o["id"][differ], m)
    assert excused <= 0.01 * ids.size, (label, excused)
    same = ~differ
    want_nan = np.isnan(o["lp"]) & same
    assert np.all(np.isnan(lp[want_nan])), label
    fin = same & ~np.isnan(o["lp"])
    err = float(np.max(np.abs(lp[fin] - o["lp"][fin]))) if fin.any() else 0.0
    print(f"sampler {label}: draws {ids.size} excused {excused} max|dlp| {err:.2e}")
    assert err < LP_TOL, (label, err)
    return ids, lp, o


def _seeds(g, rows, n_draw):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (rows, n_draw), generator=g, dtype=torch.int64)


TABLE = [
    # dtype, rows, vocab, ld_pad, n_draw, T, softcap
    ("f32", 4, 256000, 0, 16, 1.0, 30.0),     # Gemma-2's final soft-cap: the CAP instantiation
    ("bf16", 2, 256000, 8, 16, 0.7, 30.0),
    ("f16", 3, 32000, 3, 2, 1.0, 0.0),
    ("bf16", 256, 4097, 5, 1, 2.5, 50.0),     # unsplit rows, one draw
    ("f32", 1, 1, 0, 16, 1.0, 0.0),           # a one-token vocabulary
    ("f32", 300, 2, 1, 16, 0.3, 0.0),
    ("f16", 255, 8193, 7, 16, 0.3, 0.0),      # one row short of the unsplit plan
]


def _fuzz(n=24, seed=91):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        dtype = ["f32", "bf16", "f16"][rng.integers(0, 3)]
        rows = int(rng.choice([1, 3, 255, 256, 300]))
        vocab = int(rng.choice([1, 2, 77, 4097, 8193, 32000, 128256]))
        if rows * vocab > 4_000_000:
            rows = max(1, 4_000_000 // vocab)
        out.append((dtype, rows, vocab, int(rng.integers(0, 9)), int(rng.choice([1, 2, 16])),
                    float(rng.choice([0.3, 0.7, 1.0, 2.5])),
                    float(rng.choice([0.0, 30.0, 50.0])) if dtype != "f16" else 0.0))
    return out


@pytest.mark.parametrize("dtype,rows,vocab,ld_pad,n_draw,T,softcap", TABLE + _fuzz())
def test_vocab_sample_matches_oracle_at_shapes(ops, orc, dev, dtype, rows, vocab, ld_pad, n_draw,
                                               T, softcap):
    g = torch.Generator().manual_seed(rows * 131 + vocab + n_draw)
    full = (torch.randn(rows, vocab + ld_pad, generator=g) * 3.0).to(DT[dtype])
    ids, _, _ = _check(ops, orc, dev, full, _seeds(g, rows, n_draw), T, softcap, vocab=vocab,
                       label=f"{dtype} {rows}x{vocab}+{ld_pad} n{n_draw} T{T} cap{softcap}")
    assert ids.min() >= 0 and ids.max() < vocab


def test_vocab_sample_split_and_unsplit_plans_draw_the_same_tokens(ops, orc, dev):
    """3 rows x 8193 f32 split the vocabulary in two (5120 + a ragged 3073); 256 rows leave it
    unsplit.  Same logits, same seeds: the same ids, and the oracle's."""
    g = torch.Generator().manual_seed(8193)
    full = torch.randn(256, 8193, generator=g) * 3.0
    seeds = _seeds(g, 256, 16)
    a, _, _ = _check(ops, orc, dev, full[:3].contiguous(), seeds[:3].contiguous(), label="split 3x8193")
    b, _, o = _check(ops, orc, dev, full, seeds, label="unsplit 256x8193")
    assert np.array_equal(a, b[:3])
    assert np.array_equal(b, o["id"])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_vocab_sample_exact_ties_go_to_the_lowest_id(ops, orc, dev, dtype):
    """Constant rows at vocab 256,000: the 23-bit uniform repeats at the top in ~3 % of the
    draws, and the winner is then decided by the order in which lanes, waves and splits are
    merged.  The documented rule is the lowest id; an exact tie is never excused."""
    rows, n_draw, vocab = 64, 16, 256000
    seeds = torch.from_numpy((np.arange(rows * n_draw, dtype=np.int64) * 2654435761 + 12345)
                             .reshape(rows, n_draw))
    full = torch.full((rows, vocab), 1.25).to(DT[dtype])
    ids, _, o = _check(ops, orc, dev, full, seeds, label=f"constant rows {dtype}")
    tied = o["ties"] > 1
    assert int(tied.sum()) >= 10                      # the case is not vacuous
    print(f"sampler constant rows {dtype}: {int(tied.sum())} exactly tied draws")
    assert np.array_equal(ids[tied], o["id"][tied])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_vocab_sample_quantised_rows(ops, orc, dev, dtype):
    """round(2x) / 2: every score class holds thousands of tokens with the same logit."""
    g = torch.Generator().manual_seed(55)
    full = (torch.round(torch.randn(4, 128256, generator=g) * 6.0) / 2).to(DT[dtype])
    _check(ops, orc, dev, full, _seeds(g, 4, 16), label=f"quantised rows {dtype}")


def test_vocab_sample_masked_and_nan_tokens(ops, orc, dev):
    g = torch.Generator().manual_seed(20000)
    rows, V = 4, 20000
    x = torch.randn(rows, V, generator=g) * 3.0
    seeds = _seeds(g, rows, 16)
    masked = x.clone()
    masked[:, 100:] = float("-inf")                  # a logit-bias mask
    masked[3] = float("-inf")
    masked[3, 12345] = -7.5                          # a single finite token
    ids, lp, _ = _check(ops, orc, dev, masked, seeds, T=0.7, label="masked")
    assert ids[:3].max() < 100 and ids[:3].min() >= 0
    assert np.all(ids[3] == 12345)
    print(f"sampler single finite token: max|lp| {np.abs(lp[3]).max():.2e}")
    assert np.abs(lp[3]).max() < LP_TOL              # log-prob 0
    nan3 = x.clone()
    nan3[:, ::3] = float("nan")
    ids, lp, _ = _check(ops, orc, dev, nan3, seeds, label="every third NaN")
    assert np.all(ids % 3 != 0) and np.all(np.isnan(lp))


@pytest.mark.parametrize("rows,V", [(5, 77), (3, 8193), (256, 300)])
def test_vocab_sample_one_nan_anywhere_poisons_the_row(ops, orc, dev, rows, V):
    """A single NaN token makes the row's log-probs NaN wherever it sits -- also as the first
    element a thread reads, where the running (max, sum) is still empty."""
    g = torch.Generator().manual_seed(rows + V)
    x = torch.randn(rows, V, generator=g) * 3.0
    at = [0, V - 1, V // 2, min(255, V - 1), min(256, V - 1)]
    for r in range(rows):
        if r % 2 == 0:
            x[r, at[(r // 2) % len(at)]] = float("nan")
    ids, lp, _ = _check(ops, orc, dev, x, _seeds(g, rows, 4), label=f"one NaN {rows}x{V}")
    assert np.all(np.isnan(lp[0::2])) and np.all(np.isfinite(lp[1::2]))
    assert np.all(ids >= 0)


@pytest.mark.parametrize("rows,V,dead_inf,dead_nan", [(5, 20000, 1, 3), (260, 77, 5, 200)])
def test_vocab_sample_rows_without_a_candidate_give_minus_one(ops, orc, dev, rows, V, dead_inf,
                                                              dead_nan):
    """A row with no finite logit yields id -1 and NaN (nothing is read at the sentinel index);
    the normal rows of the same launch are unaffected.  Split and unsplit plans."""
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, V, generator=g) * 3.0
    seeds = _seeds(g, rows, 16)
    want, _, _ = _check(ops, orc, dev, x, seeds, label=f"all rows alive {rows}x{V}")
    x[dead_inf] = float("-inf")
    x[dead_nan] = float("nan")
    ids, lp, _ = _check(ops, orc, dev, x, seeds, label=f"two dead rows {rows}x{V}")
    for r in (dead_inf, dead_nan):
        assert np.all(ids[r] == -1) and np.all(np.isnan(lp[r]))
    alive = np.ones(rows, dtype=bool)
    alive[[dead_inf, dead_nan]] = False
    assert np.array_equal(ids[alive], want[alive]) and np.all(np.isfinite(lp[alive]))


def test_vocab_sample_extreme_and_duplicated_seeds(ops, orc, dev):
    g = torch.Generator().manual_seed(31)
    full = (torch.randn(2, 32000, generator=g) * 3.0).to(torch.bfloat16)
    row = [0, -1, -2 ** 63, 2 ** 63 - 1, 5, 5]
    seeds = torch.tensor([row, [s ^ 0x5555 for s in row]], dtype=torch.int64)
    ids, lp, _ = _check(ops, orc, dev, full, seeds, T=0.7, label="extreme seeds")
    assert np.array_equal(ids[:, 4], ids[:, 5])
    assert np.array_equal(lp[:, 4].view(np.int32), lp[:, 5].view(np.int32))
    assert len(set(ids[0, :5].tolist())) > 1          # the seeds do matter


def test_vocab_sample_vocab_narrower_than_the_tensor(ops, orc, dev):
    g = torch.Generator().manual_seed(5000)
    rows, V, W = 3, 5000, 5008
    full = torch.randn(rows, W, generator=g) * 3.0
    full[:, V:] = 1000.0                              # a maximum the draws must never see
    ids, _, _ = _check(ops, orc, dev, full, _seeds(g, rows, 16), vocab=V, narrow=True,
                       label="vocab= narrower")
    assert ids.max() < V and ids.min() >= 0


def test_vocab_sample_is_bitwise_deterministic(ops, dev):
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(7, 50001, generator=g) * 3.0).to(torch.bfloat16).to(dev)
    seeds = _seeds(g, 7, 16).to(dev)
    a_ids, a_lp = ops.vocab_sample(x, seeds, temperature=0.7, softcap=30.0)
    b_ids, b_lp = ops.vocab_sample(x, seeds, temperature=0.7, softcap=30.0)
    assert torch.equal(a_ids, b_ids)
    assert torch.equal(a_lp.view(torch.int32), b_lp.view(torch.int32))


def test_vocab_sample_distribution_with_softcap_and_temperature(ops, dev):
    """Draws follow softmax(cap * tanh(x / cap) / T): empirical frequencies over many seeds."""
    V, T, cap = 16, 0.5, 2.5
    x = torch.linspace(-2, 2, V)
    rows = 4096
    seeds = torch.arange(rows * 16, dtype=torch.int64).reshape(rows, 16)
    ids, _ = ops.vocab_sample(x.repeat(rows, 1).to(dev), seeds.to(dev), temperature=T, softcap=cap)
    freq = torch.bincount(ids.reshape(-1).long().cpu(), minlength=V).double() / ids.numel()
    p = torch.softmax(cap * torch.tanh(x.double() / cap) / T, 0)
    err = torch.max(torch.abs(freq - p)).item()
    print(f"sampler distribution T{T} cap{cap}: max|freq - p| {err:.4f}")
    assert err < 0.01


def test_vocab_sample_refuses_bad_arguments(ops, dev):
    x = torch.zeros(2, 64, device=dev)
    with pytest.raises(ops.CSError):
        ops.vocab_sample(x, torch.zeros(2, 17, dtype=torch.int64, device=dev))     # n_draw > 16
    for T in (0.0, float("inf"), float("nan")):
        with pytest.raises(ops.CSError):
            ops.vocab_sample(x, torch.zeros(2, 1, dtype=torch.int64, device=dev), temperature=T)
