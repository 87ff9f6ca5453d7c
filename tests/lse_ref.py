"""Reference, planted cases and checker for the vocab log-sum-exp stream
(block_lse_partial, csrc/cs_kernels.cuh) behind cs_logsoftmax_gather and the beam kernels.

Three parts:

* the kernel's GEOMETRY restated in Python (plan_split, and per split head / nvec / tail0,
  which loop and which lane take each 16-byte vector) and, from it, the POSITION CLASSES of a
  row: the element positions at which one of the kernel's code paths begins or ends;
* a float64 REFERENCE (max-shifted log-sum-exp of cap * tanh(x / cap), and the gather) with a
  WINDOW per row derived from the kernel's arithmetic (below), never from its output;
* the case builders (every row of a launch is one probe: a row of known content with one
  plant at a class position), a checker, and an fp32 numpy RESTATEMENT of the kernel's order of
  operations with its transcendentals pushed +-1 ulp, which tests/test_lse_cases_host.py keeps
  inside the windows and whose MUTANTS (wrong kernels) the checker must reject.

The windows
-----------
u = 2^-24 is the relative rounding of one fp32 operation.  Write x' for the soft-capped logit,
m* for the row maximum of x', d_i = m* - x'_i >= 0 and w_i = exp(-d_i) for element i's share of
the sum.  The kernel returns lse = fl(m + logf(s)) with (m, s) built by lse_accum (per lane, T
calls), wave_lse_reduce and lse_merge (G merges from a lane to the row).  Element i's term is
wrong by a relative eps_i made of:

  arguments   Every exp2 argument on the term's way is (a - b) * log2(e) for two successive
              running maxima (or the element and its first maximum); they telescope to d_i.
              Each is rounded once in lse_accum (one fma) and twice in lse_merge (fl(m - mn),
              then the product), and kLog2e itself is off by 0.23 u relative:
              at most 2.23 u * d_i.
  offsets     lse_accum subtracts off = fl(mn * kLog2e) inside the fma, so even the maximum's
              own argument is the rounding residue of off, up to |mn| * u in nats, once per
              call while the sum is carried: T * M * u with M = max |x'| over finite elements.
              (lse_merge has no such residue: m - mn is exactly 0 for the larger operand.)
  exp2        v_exp_f32 is good to 1 ulp = 2 u (AMD's CDNA ISA guide; the microarchitecture
              guide gives its cost only): the term's own and one per carry and merge,
              2 u * (1 + T + G).  exp2 of 0 is exactly 1.
  sums        N sequential adds in one lse_accum (N = elements per call; 6 through the bf16
              table's four chains), one fma per later call, a product and an add per merge:
              u * (N + T + 2 G).
  soft-cap    softcap_fn / softcap_exp: c = fl(fl(2 log2e) * fl(1 / cap)) is 3 u off, x * c one
              more; with a = x c and r = 1 / (2^a + 1) the error of 2^a reaches r through
              2^a r <= min(1, 2^a): |a| * 2^-|a| <= 0.54 bounds the argument part, then 2 u
              (exp2), u (the add), 2 u (v_rcp_f32, 1 ulp) relative in r <= 1, times 2 cap,
              plus the fma's own rounding of a result <= cap:
              2 cap (0.54 ln2 * 4 + 2 + 1 + 2) u + cap u < 14 cap u.  The fixed-offset form
              (cap <= 60) feeds r to exp2 through one more fma and two rounded constants
              (3 cap u more): C_CAP = 18 cap u covers both.

so |s - s*| / s* <= sum_i w_i eps_i / sum_i w_i
                 =  u * (2.23 E_w[d] + T M + 2 (1 + T + G) + N + T + 2 G + C_CAP cap),
with E_w[d] the w-weighted mean of d, computed in float64 from the row itself.  The
fixed-offset paths keep m = 0 (every merge factor is exp2(0) = 1), so their argument and offset
terms vanish.  Then one logf (1 ulp documented for HIP's logf; 2 ulps of |log s| allowed) and the
final add (half an ulp of |lse|).  tok_lp = fl(x' - lse) adds the gather's own soft-cap error
and half an ulp of |tok_lp|.

Counting rows (all zeros, no cap) are exact up to the logf: every exp2 argument is 0, every
sum an integer below 2^24, so s = V and lse = logf(V).  The device's logf is not pinned to a
bit pattern, so the window is 2 ulps of log V (1.9e-6 for 2981 <= V < 2^16) -- one dropped or
doubled element moves lse by log(V / (V - 1)) >= 2.4e-5 at V <= 41,000, more than 12 windows.
One-hot rows with c = 0 are exact outright: s = exp2(0) = 1 and logf(1) = 0.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

F32, BF16, F16 = "f32", "bf16", "f16"
DTYPES = (BF16, F16, F32)
EPV = {F32: 4, BF16: 8, F16: 8}          # elements per 16-byte vector
K_BLOCK, K_UNROLL, K_TARGET_WGS = 256, 4, 256          # plan_split's constants
STREAM_BLOCK, STREAM_UNROLL = 1024, 2                  # unsplit rows
SPLIT_SUB, SPLIT_UNROLL, SPLIT_QUAD = 256, 2, 4        # split rows
MERGE_LANES = 64
FIXED_CAP_MAX = 60.0
U = 2.0 ** -24
LOG2E32 = np.float32(1.4426950408889634)
LOGF_ULPS = 2.0
C_CAP = 18.0
BAND = 64               # poisoned elements before the first and after the last row
GUARD = 64              # 0x5A bytes either side of out= / lse_out=
FILL = 0x5A


# ---------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------
def plan_split(rows: int, vocab: int, dtype: str):
    """(nsplit, split_len) of cs_kernels.cuh's plan_split."""
    if rows <= 0 or vocab <= 0 or rows >= K_TARGET_WGS:
        return 1, vocab
    grain = K_BLOCK * EPV[dtype]
    min_len = grain * K_UNROLL
    want = (K_TARGET_WGS * SPLIT_QUAD + rows - 1) // rows
    want = min(want, max(vocab // min_len, 1))
    if want <= 1:
        return 1, vocab
    length = -(-vocab // want)
    length = -(-length // grain) * grain
    nsplit = -(-vocab // length)
    return (1, vocab) if nsplit <= 1 else (nsplit, length)


def workspace_bytes(rows: int, vocab: int) -> int:
    """cs_workspace_size: 8 bytes per (row, split) of the larger of the bf16 and f32 plans."""
    ns = max(plan_split(rows, vocab, BF16)[0], plan_split(rows, vocab, F32)[0])
    return 0 if ns <= 1 else rows * ns * 8


@dataclass(frozen=True)
class Split:
    """block_lse_partial's view of logits[v0, v0 + n) of a row whose first element sits `off`
    elements past a 16-byte boundary.  head / tail0 are relative to v0."""
    index: int
    v0: int
    n: int
    head: int
    nvec: int
    tail0: int
    block: int
    unroll: int
    epv: int

    def lane_of(self, j):
        return j % self.block

    def wave_of(self, j):
        return (j % self.block) // 64

    def in_sweep(self, j):
        """Whether vector j (array or int) is taken by the unrolled sweep (else the remainder
        loop): lane t's r-th sweep needs t + (unroll r + unroll - 1) block < nvec."""
        j = np.asarray(j)
        r = (j // self.block) // self.unroll
        return (j % self.block) + (self.unroll * r + self.unroll - 1) * self.block < self.nvec

    def calls(self):
        """T: the most lse_accum calls one lane makes (scalar, sweeps, remainder trips)."""
        if self.nvec == 0:
            return 1
        j = np.arange(0, self.nvec, self.block)        # lane 0's vectors
        sw = int(self.in_sweep(j).sum())
        return 1 + sw // self.unroll + (len(j) - sw)


def geometry(dtype: str, off: int, vocab: int, plan) -> list:
    nsplit, split_len = plan
    epv = EPV[dtype]
    block = STREAM_BLOCK if nsplit == 1 else SPLIT_SUB
    unroll = STREAM_UNROLL if nsplit == 1 else SPLIT_UNROLL
    out = []
    for i in range(nsplit):
        v0 = i * split_len
        n = min(vocab, v0 + split_len) - v0
        head = min((epv - (off + v0) % epv) % epv, n)
        nvec = (n - head) // epv
        out.append(Split(i, v0, n, head, nvec, head + nvec * epv, block, unroll, epv))
    return out


N_RANDOM = 32
VEC_MARKS = (("v63", lambda b: 63), ("v64", lambda b: 64), ("vB-1", lambda b: b - 1),
             ("vB", lambda b: b), ("v2B-1", lambda b: 2 * b - 1), ("v2B", lambda b: 2 * b))


def split_classes(sp: Split) -> list:
    """[(class name, position in the row)] of one split: where its paths begin and end."""
    out = []
    if sp.head > 0:
        out.append(("head_last", sp.head - 1))
    if sp.head < sp.n:
        out.append(("after_head", sp.head))
    if sp.tail0 > 0:
        out.append(("tail_prev", sp.tail0 - 1))
    if sp.tail0 < sp.n:
        out.append(("tail_first", sp.tail0))
        out.append(("tail_last", sp.n - 1))
    marks = [(nm, f(sp.block)) for nm, f in VEC_MARKS]
    if sp.nvec > 0:
        js = np.arange(sp.nvec)
        sw = sp.in_sweep(js)
        if sw.any():
            marks.append(("sweep_last", int(js[sw].max())))
        if (~sw).any():
            marks.append(("rem_first", int(js[~sw].min())))
        marks.append(("vec_last", sp.nvec - 1))
    for nm, j in marks:
        if j < sp.nvec:
            out.append((nm + "_first", sp.head + j * sp.epv))
            out.append((nm + "_last", sp.head + j * sp.epv + sp.epv - 1))
    return [(nm, sp.v0 + p) for nm, p in out]


def row_classes(dtype: str, off: int, vocab: int, plan, seed: int = 0) -> list:
    """The position classes of a row: [(name, position)], structural ones first, then
    N_RANDOM seeded positions (a position may carry several names).  Split rows
    carry the per-split classes of splits 0, 1, the first split of the second quad item
    ("q2.") and the last split ("sl."), and the two elements at every split edge."""
    geo = geometry(dtype, off, vocab, plan)
    ns = len(geo)
    named = [("elem0", 0), ("elem_last", vocab - 1)]
    if ns == 1:
        named += split_classes(geo[0])
    else:
        tags = {0: "s0.", 1: "s1."}
        if ns > SPLIT_QUAD:
            tags[SPLIT_QUAD] = "q2."
        tags[ns - 1] = "sl."
        for i, tag in tags.items():
            named += [(tag + nm, p) for nm, p in split_classes(geo[i])]
        for sp in geo[1:]:
            named += [("edge_prev", sp.v0 - 1), ("edge", sp.v0)]
        if ns > SPLIT_QUAD:
            named.append(("quad2_first", geo[SPLIT_QUAD].v0))
        named.append(("last_split", geo[-1].v0 + geo[-1].n // 2))
    rng = np.random.default_rng([vocab, off, seed, 0xC1A55])
    named += [("random", int(p)) for p in rng.integers(0, vocab, N_RANDOM)]
    assert all(0 <= p < vocab for _, p in named), named
    return list(dict.fromkeys(named))


def class_kind(name: str) -> str:
    return name.split(".", 1)[-1]


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    dtype: str
    V: int
    rows: int
    pad: bool = True        # ld = 1 (mod EPV) with poisoned pad columns; else ld = V, aligned
    base_off: int = 0       # elements between a 16-byte boundary and row 0 (pad cases)
    k: int = 3
    view_of: int = 0        # rows of the buffer the launch is a view of (0: all of them)

    @property
    def epv(self):
        return EPV[self.dtype]

    @property
    def ld(self):
        if not self.pad:
            return self.V
        ld = self.V + self.epv + 1
        return ld + (1 - ld) % self.epv

    @property
    def plan(self):
        return plan_split(self.rows, self.V, self.dtype)

    @property
    def path(self):
        return "unsplit" if self.plan[0] == 1 else "split"

    @property
    def first(self):
        """The launch's row 0 in the buffer's rows (a view of a larger buffer starts later)."""
        return (max(self.view_of, self.rows) - self.rows) // 2

    def off(self, row: int) -> int:
        """Elements between a 16-byte boundary and the row's first element."""
        return (self.base_off + (self.first + row) * self.ld) % self.epv if self.pad else 0

    def classes(self, row: int) -> list:
        return row_classes(self.dtype, self.off(row), self.V, self.plan)


UNSPLIT_NVEC = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4097)
SPLIT_V = {BF16: (16384, 16385, 40961, 40967, 40969), F16: (16384, 16385, 40961, 40967, 40969),
           F32: (8192, 20481, 20485, 40961)}
# the plans the split shapes must get at 1, 3 and 64 rows: (nsplit, split_len, last split)
SPLIT_PLANS = {(BF16, 16384): (2, 8192, 8192), (BF16, 16385): (2, 10240, 6145),
               (BF16, 40961): (5, 10240, 1), (BF16, 40967): (5, 10240, 7),
               (BF16, 40969): (5, 10240, 9), (F32, 8192): (2, 4096, 4096),
               (F32, 20481): (5, 5120, 1), (F32, 20485): (5, 5120, 5),
               (F32, 40961): (9, 5120, 1)}


def unsplit_cases() -> tuple:
    out = []
    for dt in DTYPES:
        e = EPV[dt]
        for nv in UNSPLIT_NVEC:
            out.append(Case(f"{dt}-u-nvec{nv}", dt, nv * e if nv else e - 1, 256))
        for v in (1, 2, 3, 7):
            out.append(Case(f"{dt}-u-V{v}", dt, v, 256))
        out.append(Case(f"{dt}-u-view300", dt, 1025 * e + 3, 300, view_of=311))
        out.append(Case(f"{dt}-u-aligned", dt, 1025 * e, 256, pad=False))
        out.append(Case(f"{dt}-u-k1025", dt, 1025 * e + 5, 256, k=1025))
        out.append(Case(f"{dt}-u-k1", dt, 2049 * e + 1, 256, k=1))
        out.append(Case(f"{dt}-u-k0", dt, 1023 * e + 2, 256, k=0))
    return tuple(out)


def split_cases() -> tuple:
    out = []
    for dt in DTYPES:
        for v in SPLIT_V[dt]:
            for rows in (1, 3, 64):
                out.append(Case(f"{dt}-s-V{v}-r{rows}", dt, v, rows, base_off=(v + rows) % EPV[dt]))
        v = SPLIT_V[dt][2]
        out.append(Case(f"{dt}-s-aligned", dt, SPLIT_V[dt][0], 64, pad=False))
        out.append(Case(f"{dt}-s-k65", dt, v, 64, k=65))
        out.append(Case(f"{dt}-s-k1", dt, v, 3, k=1, base_off=3))
        out.append(Case(f"{dt}-s-k0", dt, v, 3, k=0, base_off=2))
    return tuple(out)


def all_cases() -> tuple:
    return unsplit_cases() + split_cases()


# ---------------------------------------------------------------------------------------
# launches: every row is one probe
# ---------------------------------------------------------------------------------------
KINDS_NOCAP = ("count", "onehot0", "onehot3.5", "onehot-80", "latemax")
SAT = (("sat30+", 30.0, 1000.0), ("sat30-", 30.0, -1000.0), ("sat75+", 75.0, 1000.0),
       ("sat75-", 75.0, -1000.0))
CAPS = (0.0, 30.0, 75.0)


@dataclass
class Launch:
    case: Case
    kind: str
    cap: float
    bg: np.ndarray                      # [rows] background value of columns [0, V)
    plant_col: np.ndarray               # [rows] or -1
    plant_val: np.ndarray
    nan_col: np.ndarray                 # [rows] or -1
    targets: np.ndarray                 # [rows, k] int32
    dense: Optional[np.ndarray] = None  # [rows, V] float32 background instead of bg
    poison: float = float("nan")
    cls: list = field(default_factory=list)   # the class name each row's position came from
    # expectations (fill_expected)
    ref_lse: np.ndarray = None
    ref_tok: np.ndarray = None
    win_lse: np.ndarray = None
    win_tok: np.ndarray = None
    nan_row: np.ndarray = None
    exact: np.ndarray = None            # rows whose lse is exact (window 0)

    def values(self) -> np.ndarray:
        """[rows, V] float32: what the rows' first V columns hold."""
        c = self.case
        x = (self.dense.copy() if self.dense is not None
             else np.repeat(self.bg.astype(np.float32)[:, None], c.V, axis=1))
        r = np.nonzero(self.plant_col >= 0)[0]
        x[r, self.plant_col[r]] = self.plant_val[r]
        r = np.nonzero(self.nan_col >= 0)[0]
        x[r, self.nan_col[r]] = np.nan
        return x

    def buffer(self):
        """(flat float32 buffer, start of row 0, rows of the buffer): bands and pad columns
        poisoned.  The launch reads rows [first, first + rows) of the buffer's rows."""
        c = self.case
        nbuf, first = max(c.view_of, c.rows), c.first
        start = BAND + (c.base_off if c.pad else 0)
        flat = np.full(start + nbuf * c.ld + BAND + c.epv, self.poison, dtype=np.float32)
        rows = flat[start:start + nbuf * c.ld].reshape(nbuf, c.ld)
        rows[first:first + c.rows, :c.V] = self.values()
        return flat, start + first * c.ld, nbuf


def softcap64(x, cap):
    x = np.asarray(x, dtype=np.float64)
    return x if cap <= 0 else cap * np.tanh(x / cap)


def reference(x, targets, cap, vocab):
    """float64 (lse [rows], tok_lp [rows, k]) of x [rows, >= vocab]: plain max-shifted
    log-sum-exp of the soft-capped logits and the gather; ids outside [0, vocab) give NaN; a
    row without a finite element gives lse = -inf (NaN tok_lp), one with a NaN gives NaN."""
    xc = softcap64(np.asarray(x)[:, :vocab], cap)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = xc.max(axis=1)
        ms = np.where(np.isfinite(m), m, 0.0)
        lse = ms + np.log(np.exp(xc - ms[:, None]).sum(axis=1))
        t = np.asarray(targets).reshape(len(xc), -1)
        ok = (t >= 0) & (t < vocab)
        tok = np.take_along_axis(xc, np.where(ok, t, 0).astype(np.int64), axis=1) - lse[:, None]
        tok = np.where(ok, tok, np.nan)
    return lse, tok


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    x = np.where(np.isfinite(x), x, 0.0)
    return np.spacing(np.maximum(x, 2.0 ** -126).astype(np.float32)).astype(np.float64)


def path_counts(case: Case, dtype_cap_table: bool):
    """(T, G, N) of the window: lse_accum calls per lane, merges lane -> row, adds per call."""
    ns, _ = case.plan
    T = max(sp.calls() for r in range(min(case.rows, case.epv))
            for sp in geometry(case.dtype, case.off(r), case.V, case.plan))
    if ns == 1:
        G = 6 + STREAM_BLOCK // 64 - 1
        N = STREAM_UNROLL * case.epv
    else:
        G = 6 + SPLIT_SUB // 64 - 1 + -(-ns // MERGE_LANES) + 6
        N = SPLIT_UNROLL * case.epv
    if dtype_cap_table:
        N = 6
    return T, G, N


def _contents(L: Launch):
    """(values [rows, J], counts [rows, J], target values [rows, k]) in float64: what each row
    holds besides its NaN.  Planted rows are a background value and one plant (J = 2), so their
    reference is a closed form; dense rows are summed element by element."""
    c = L.case
    t = L.targets.astype(np.int64)
    ok = (t >= 0) & (t < c.V)
    if L.dense is not None:
        x = L.values().astype(np.float64)
        xt = np.take_along_axis(x, np.where(ok, t, 0), axis=1)
        return np.where(np.isnan(x), -np.inf, x), np.ones_like(x), np.where(ok, xt, np.nan)
    has_p = (L.plant_col >= 0) & (L.plant_col != L.nan_col)
    vals = np.stack([L.bg.astype(np.float64), L.plant_val.astype(np.float64)], axis=1)
    cnt = np.stack([c.V - has_p - (L.nan_col >= 0), has_p], axis=1).astype(np.float64)
    xt = np.where(t == L.plant_col[:, None], L.plant_val[:, None], L.bg[:, None]).astype(np.float64)
    xt = np.where((t == L.nan_col[:, None]) | ~ok, np.nan, xt)
    return vals, cnt, xt


def fill_expected(L: Launch) -> Launch:
    """Reference and windows of every row, from the row's content (see the module docstring)."""
    c, cap = L.case, float(L.cap)
    vals, cnt, xt = _contents(L)
    L.nan_row = L.nan_col >= 0
    fixed = 0.0 < cap <= FIXED_CAP_MAX
    T, G, N = path_counts(c, fixed and c.dtype == BF16)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        xc = softcap64(vals, cap)
        fin = np.isfinite(xc) & (cnt > 0)
        mstar = np.where(fin, xc, -np.inf).max(axis=1)
        ms = np.where(np.isfinite(mstar), mstar, 0.0)
        d = np.where(fin, ms[:, None] - xc, 0.0)
        w = np.where(fin, cnt * np.exp(-d), 0.0)
        L.ref_lse = ms + np.log(w.sum(axis=1))
        L.ref_tok = softcap64(xt, cap) - L.ref_lse[:, None]
        Ed = (w * d).sum(axis=1) / np.maximum(w.sum(axis=1), 1e-300)
        M = np.where(fin, np.abs(xc), 0.0).max(axis=1)
    if fixed:
        rel = U * (2.0 + N + T + 2 * G + C_CAP * cap)
        log_s = L.ref_lse
    else:
        rel = U * (2.23 * Ed + T * M + 2.0 * (1 + T + G) + N + T + 2 * G + C_CAP * cap)
        with np.errstate(invalid="ignore"):
            log_s = L.ref_lse - mstar
    L.win_lse = rel + LOGF_ULPS * _ulp32(log_s) + 0.5 * _ulp32(L.ref_lse)
    L.exact = np.zeros(c.rows, dtype=bool)
    if cap == 0.0 and L.dense is None:
        zero_bg = (L.bg == 0.0) & (L.plant_col < 0) & (L.nan_col < 0)          # counting rows
        L.win_lse = np.where(zero_bg, LOGF_ULPS * _ulp32(math.log(c.V)), L.win_lse)
        L.exact = np.isneginf(L.bg) & (L.plant_col >= 0) & (L.plant_val == 0.0) & ~L.nan_row
        L.win_lse = np.where(L.exact, 0.0, L.win_lse)
    L.win_tok = (L.win_lse[:, None] + C_CAP * cap * U
                 + 0.5 * _ulp32(np.nan_to_num(L.ref_tok, nan=0.0, posinf=0.0, neginf=0.0)))
    return L


def _round_to(dtype: str, x: np.ndarray) -> np.ndarray:
    """x (float32) rounded to the values `dtype` holds, as float32."""
    if dtype == F32:
        return x.astype(np.float32)
    if dtype == F16:
        return x.astype(np.float16).astype(np.float32)
    b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def targets_for(case: Case, cols: np.ndarray, shift: int = 0) -> np.ndarray:
    """[rows, k] ids: the plant first, then 0, V - 1, the three out-of-range ids (-1, V and
    ld - 1: a poisoned pad column), duplicates and seeded in-range ids."""
    V, k = case.V, case.k
    t = np.empty((case.rows, k), dtype=np.int32)
    rng = np.random.default_rng([V, k, shift, 7])
    menu = [0, V - 1, -1, V, max(case.ld - 1, V), 0, V - 1]
    for r in range(case.rows):
        p = int(cols[r]) if cols[r] >= 0 else (r * 7919) % V
        row = [p] + [menu[(r + shift + j) % len(menu)] for j in range(min(k, 8))]
        row += [p, p]                                                   # duplicates
        if k > len(row):
            row += list(rng.integers(-1, V + 1, k - len(row)))
        t[r] = row[:k]
    return t


def probe_cols(case: Case, shift: int):
    """One class position per row, and the class names taken: the rows of one alignment walk
    their class list, and each further `shift` takes the next stretch of it."""
    cols = np.empty(case.rows, dtype=np.int64)
    names = []
    cache = {}
    div = case.epv if case.pad else 1
    per = max(case.rows // div, 1)
    for r in range(case.rows):
        o = case.off(r)
        if o not in cache:
            cache[o] = case.classes(r)
        cl = cache[o]
        nm, p = cl[(r // div + shift * per) % len(cl)]
        cols[r] = p
        names.append(nm)
    return cols, names


def n_shifts(case: Case) -> int:
    """Launches after which every row alignment has planted every class of its list."""
    per = max(case.rows // (case.epv if case.pad else 1), 1)
    longest = max(len(case.classes(r)) for r in range(min(case.rows, case.epv)))
    return -(-longest // per)


def make_launch(case: Case, kind: str, shift: int = 0, cap: Optional[float] = None,
                poison: float = float("nan")) -> Launch:
    """The launch of `kind` on `case`; `shift` moves every row to its next classes."""
    R, V = case.rows, case.V
    cols, names = probe_cols(case, shift)
    none = np.full(R, -1, dtype=np.int64)
    z = np.zeros(R)
    rng = np.random.default_rng([V, R, shift, sum(map(ord, kind))])
    kw = dict(case=case, kind=kind, cls=names, poison=poison)
    if kind == "count":
        L = Launch(cap=0.0, bg=z, plant_col=none, plant_val=z, nan_col=none,
                   targets=targets_for(case, none, shift), **kw)
    elif kind.startswith("onehot"):
        c = float(kind[6:])
        L = Launch(cap=0.0, bg=np.full(R, -np.inf), plant_col=cols, plant_val=np.full(R, c),
                   nan_col=none, targets=targets_for(case, cols, shift), **kw)
    elif kind == "latemax":
        L = Launch(cap=0.0, bg=z, plant_col=cols, plant_val=np.full(R, 40.0), nan_col=none,
                   targets=targets_for(case, cols, shift), **kw)
    elif kind.startswith("sat"):
        _, c, v = next(s for s in SAT if s[0] == kind)
        L = Launch(cap=c, bg=z, plant_col=cols, plant_val=np.full(R, v), nan_col=none,
                   targets=targets_for(case, cols, shift), **kw)
    elif kind == "allinf":
        L = Launch(cap=0.0, bg=np.full(R, -np.inf), plant_col=none, plant_val=z, nan_col=none,
                   targets=targets_for(case, cols, shift), **kw)
    elif kind == "nan_inf":
        # -inf background.  Even rows: clean one-hot (plant 0 at a seeded position).  Odd rows:
        # a NaN at the class position, and every other odd row has no finite element at all
        # (every partner of the NaN's lane is empty).
        r = np.arange(R)
        pc = rng.integers(0, V, R)
        pc = np.where((r % 4 == 3) | ((pc == cols) & (r % 2 == 1)), -1, pc)
        L = Launch(cap=cap or 0.0, bg=np.full(R, -np.inf), plant_col=pc, plant_val=z,
                   nan_col=np.where(r % 2 == 1, cols, -1), targets=targets_for(case, cols, shift),
                   **kw)
    elif kind in ("nan_randn", "random", "masked"):
        dense = _round_to(case.dtype, (rng.standard_normal((R, V)) * 3.0).astype(np.float32))
        nan_col = none
        if kind == "nan_randn":
            nan_col = np.where(np.arange(R) % 2 == 1, cols, -1)
        if kind == "masked":
            for r in range(R):
                dense[r, cols[r]:cols[r] + 100] = -np.inf
        L = Launch(cap=cap or 0.0, bg=z, plant_col=none, plant_val=z, nan_col=nan_col,
                   targets=targets_for(case, cols, shift), dense=dense, **kw)
    else:
        raise ValueError(kind)
    return fill_expected(L)


def beam_launch(case: Case, cap: float, B: int, K: int, shift: int = 0) -> Launch:
    """The agent rows of a beam step (row a * B + b: agent a, beam b) as probes: by row a
    counting row, a one-hot row (c = 0, 3.5, -80 in turn), a NaN beside one finite element on a
    -inf background, and a NaN in a counting row.  A beam's candidates are shared by the agents:
    the class position of the beam's first row, 0, V - 1 and out-of-range ids."""
    R, V = case.rows, case.V
    assert R % B == 0
    cols, names = probe_cols(case, shift)
    r = np.arange(R)
    kind = r % 4
    hot = np.array([0.0, 3.5, -80.0])[(r // 4) % 3]
    other = (cols + 1 + (r * 7919) % max(V - 1, 1)) % V          # a position that is not cols
    tb = np.stack([[int(cols[b]), 0, V - 1, -1, V, int(cols[b]), case.ld - 1 if case.pad else V]
                   for b in range(B)])[:, :K].astype(np.int32)
    L = Launch(case=case, kind="beam", cap=cap, cls=names,
               bg=np.where((kind == 0) | (kind == 3), 0.0, -np.inf),
               plant_col=np.where(kind == 1, cols, np.where((kind == 2) & (V > 1), other, -1)),
               plant_val=np.where(kind == 1, hot, 0.0),
               nan_col=np.where(kind >= 2, cols, -1), targets=np.tile(tb, (R // B, 1)))
    return fill_expected(L)


def check(L: Launch, lse, tok, rows=None):
    """(failures, worst share of a window used) of a result against the launch's expectations.
    lse [rows] and tok [rows, k] as the kernel (or a restatement) returned them; `rows` limits
    the check to those rows (lse / tok then hold only them)."""
    idx = np.arange(L.case.rows) if rows is None else np.asarray(rows)
    k = L.targets.shape[1]
    lse = np.asarray(lse, dtype=np.float64).reshape(len(idx))
    tok = np.asarray(tok, dtype=np.float64).reshape(len(idx), k)
    want, wtok = L.ref_lse[idx], L.ref_tok[idx]
    win, wint = L.win_lse[idx], L.win_tok[idx]
    nanr, exact = L.nan_row[idx], L.exact[idx]
    with np.errstate(invalid="ignore"):
        err, errt = np.abs(lse - want), np.abs(tok - wtok)
        # a NaN row: NaN lse and all-NaN tok_lp.  A clean row: the infinite and the exact
        # expectations bit for bit, the others inside their windows.
        same = np.isinf(want) | exact
        bad_lse = np.where(nanr, ~np.isnan(lse), np.where(same, lse != want, ~(err <= win)))
        bad_tok = np.where(nanr[:, None] | np.isnan(wtok), ~np.isnan(tok),
                           np.where(np.isinf(wtok), tok != wtok, ~(errt <= wint)))
        used = np.where(nanr | same | bad_lse, 0.0, err / np.where(win > 0, win, 1.0))
        usedt = np.where(nanr[:, None] | ~np.isfinite(wtok) | bad_tok, 0.0, errt / wint)
    bad = []
    for i in np.nonzero(bad_lse | bad_tok.any(axis=1))[0]:
        r = idx[i]
        head = (f"{L.case.name}/{L.kind} cap {L.cap:g} row {r} ({L.cls[r]}, plant "
                f"{L.plant_col[r]}, nan {L.nan_col[r]}, off {L.case.off(int(r))}): ")
        if bad_lse[i]:
            bad.append(head + (f"lse {lse[i]!r} of a row with a NaN" if nanr[i] else
                               f"lse {lse[i]!r}, want {want[i]!r} +- {win[i]:.3g}"))
        for j in np.nonzero(bad_tok[i])[0][:3]:
            bad.append(head + f"tok_lp[{j}] (id {L.targets[r, j]}) {tok[i, j]!r}, want "
                              f"{'NaN' if nanr[i] else repr(wtok[i, j])} +- {wint[i, j]:.3g}")
    worst = max(float(used.max(initial=0.0)), float(usedt.max(initial=0.0)))
    return bad, worst


# ---------------------------------------------------------------------------------------
# fp32 restatement of the kernel's order of operations (and its mutants)
# ---------------------------------------------------------------------------------------
MUTANTS = ("drop_head", "drop_tail", "drop_rem", "double_first", "no_rescale", "nan_drop",
           "read_past", "lose_last_split", "merge_ignores_m", "gather_first_lanes")
_f32 = np.float32
_NINF = _f32(-np.inf)


class Restated:
    """The kernels in numpy fp32, lane by lane in the device's order.  push = +1 / -1 moves
    every inexact exp2, reciprocal and logf one ulp up / down, 0 leaves them correctly
    rounded, "mix" picks per call from a seeded stream.  mutant: one of MUTANTS."""

    def __init__(self, push=0, mutant: Optional[str] = None, seed: int = 1):
        assert mutant is None or mutant in MUTANTS
        self.push, self.mutant = push, mutant
        self.rng = np.random.default_rng(seed)

    # -- transcendentals ------------------------------------------------------------
    def _pushed(self, r, exact):
        r = r.astype(_f32)
        if self.push == 0:
            return r
        if self.push == "mix":
            up = self.rng.integers(0, 2, r.shape).astype(bool)
        else:
            up = np.full(r.shape, self.push > 0)
        with np.errstate(invalid="ignore", over="ignore"):
            moved = np.where(up, np.nextafter(r, _f32(np.inf)), np.nextafter(r, _f32(0)))
        keep = exact | ~np.isfinite(r) | (r == 0)
        return np.where(keep, r, moved).astype(_f32)

    def exp2(self, a):
        a = np.asarray(a, dtype=_f32)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            r = np.exp2(a.astype(np.float64))
            r = np.where(r < 2.0 ** -126, 0.0, r)          # v_exp_f32 flushes denormal results
            return self._pushed(r, a == np.floor(a))

    def rcp(self, a):
        a = np.asarray(a, dtype=_f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            m, _ = np.frexp(a)
            return self._pushed(1.0 / a.astype(np.float64), np.abs(m) == 0.5)

    def logf(self, a):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._pushed(np.log(np.asarray(a, dtype=np.float64)), a == 1)

    @staticmethod
    def fma(a, b, c):
        # the product of two fp32 values is exact in float64; one rounding of the sum to 53
        # bits, then to 24 (a double rounding in about one case in 2^29)
        with np.errstate(invalid="ignore", over="ignore"):
            return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
                    + np.asarray(c, np.float64)).astype(_f32)

    # -- soft-cap -------------------------------------------------------------------
    def softcap_rcp(self, x, inv_cap):
        c = _f32(_f32(2.0) * LOG2E32) * inv_cap
        with np.errstate(invalid="ignore", over="ignore"):
            return self.rcp(self.exp2(x * c) + _f32(1.0))

    def softcap_fn(self, x, cap):
        cap = _f32(cap)
        return self.fma(_f32(-2.0) * cap, self.softcap_rcp(x, _f32(1.0) / cap), cap)

    def softcap_exp(self, x, cap):
        cap = _f32(cap)
        return self.exp2(self.fma(_f32(_f32(-2.0) * LOG2E32) * cap,
                                  self.softcap_rcp(x, _f32(1.0) / cap), LOG2E32 * cap))

    def table(self, x, cap):
        """cap_lookup of bf16 values x: the entry (softcap_exp of the clamped value) and
        whether the element is a NaN (tracked beside the sum)."""
        nan = np.isnan(x)
        a = np.abs(x)
        with np.errstate(invalid="ignore"):
            y = np.where(a < _f32(2.0 ** -24), np.copysign(_f32(0), x),
                         np.where(a > _f32(1020.0), np.copysign(_f32(1020.0), x), x))
        y = np.where(nan, _f32(1020.0), y).astype(_f32)
        return self.softcap_exp(y, cap), nan

    # -- (m, s) ---------------------------------------------------------------------
    def accum(self, m, s, v, act):
        """lse_accum<N> of v [..., N] into the lanes where act."""
        with np.errstate(invalid="ignore", over="ignore"):
            cm = v[..., 0]
            for i in range(1, v.shape[-1]):
                cm = np.fmax(cm, v[..., i])
            mn = np.fmax(m, cm)
            empty = mn == _NINF
            t = v.sum(axis=-1, dtype=_f32)
            poison = act & empty & np.isnan(t) & (self.mutant != "nan_drop")
            go = act & ~empty
            off = mn * LOG2E32
            acc = np.zeros_like(m)
            for i in range(v.shape[-1]):
                acc = acc + self.exp2(self.fma(v[..., i], LOG2E32, -off))
            if self.mutant == "no_rescale":
                s2 = s + acc
            else:
                s2 = self.fma(s, self.exp2(self.fma(m, LOG2E32, -off)), acc)
        m = np.where(go, mn, np.where(poison, _f32(0), m))
        s = np.where(go, s2, np.where(poison, _f32(np.nan), s))
        return m.astype(_f32), s.astype(_f32)

    def merge(self, m, s, m2, s2):
        with np.errstate(invalid="ignore", over="ignore"):
            mn = np.fmax(m, m2)
            empty = mn == _NINF
            if self.mutant == "merge_ignores_m":
                sn = s + s2
            else:
                sn = (s * self.exp2((m - mn) * LOG2E32) + s2 * self.exp2((m2 - mn) * LOG2E32))
        return np.where(empty, m, mn).astype(_f32), np.where(empty, s, sn).astype(_f32)

    def wave_reduce(self, m, s):
        """wave_lse_reduce over the last axis (64 lanes); every lane ends with the result."""
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            m, s = self.merge(m, s, m[..., lanes ^ o], s[..., lanes ^ o])
        return m, s

    def partial(self, x, sp: Split, dtype, cap):
        """block_lse_partial over x [R, >= v0 + n (+ 1)] of rows sharing sp: (m, s) [R]."""
        R, B, E, UN = x.shape[0], sp.block, sp.epv, sp.unroll
        fixed = 0.0 < cap <= FIXED_CAP_MAX
        tab = fixed and dtype == BF16
        n = sp.n + (1 if self.mutant == "read_past" and sp.v0 + sp.n < x.shape[1] else 0)
        head, nvec = sp.head, (n - sp.head) // E
        tail0 = head + nvec * E
        seg = x[:, sp.v0:sp.v0 + n]
        m = np.full((R, B), 0.0 if fixed else -np.inf, dtype=_f32)
        s = np.zeros((R, B), dtype=_f32)
        nan = np.zeros((R, B), dtype=bool)
        lane = np.arange(B)
        # scalar head (lanes < head) and tail (lanes 64 ...)
        xs = np.full((R, B), -np.inf, dtype=_f32)
        have = np.zeros(B, dtype=bool)
        if head and self.mutant != "drop_head":
            xs[:, :head] = seg[:, :head]
            have[:head] = True
        nt = n - tail0
        if nt and self.mutant != "drop_tail":
            xs[:, 64:64 + nt] = seg[:, tail0:n]
            have[64:64 + nt] = True
        have = np.broadcast_to(have, (R, B))
        if tab:
            e, isn = self.table(xs, cap)
            s = np.where(have, s + e, s).astype(_f32)
            nan |= have & isn
        elif fixed:
            s = np.where(have, s + self.softcap_exp(xs, cap), s).astype(_f32)
        else:
            if cap > 0:
                xs = self.softcap_fn(xs, cap)
            m, s = self.accum(m, s, xs[..., None], have & (xs != _NINF))
        # vectors
        vec = seg[:, head:tail0].reshape(R, nvec, E)

        def consume(m, s, nan, js, act):
            """the lanes where act take vectors js [B, q] (q vectors each) in one call"""
            v = vec[:, np.where(act[:, None], js, 0)].reshape(R, B, -1)
            a = np.broadcast_to(act, (R, B))
            if tab:
                e, isn = self.table(v, cap)
                ch = [e[..., c] for c in range(4)]
                for i in range(4, e.shape[-1]):
                    ch[i & 3] = ch[i & 3] + e[..., i]
                s = np.where(a, s + ((ch[0] + ch[1]) + (ch[2] + ch[3])), s).astype(_f32)
                nan = nan | (a & isn.any(axis=-1))
            elif fixed:
                acc = np.zeros((R, B), dtype=_f32)
                e = self.softcap_exp(v, cap)
                for i in range(e.shape[-1]):
                    acc = acc + e[..., i]
                s = np.where(a, s + acc, s).astype(_f32)
            else:
                if cap > 0:
                    v = self.softcap_fn(v, cap)
                m, s = self.accum(m, s, v, a)
            return m, s, nan

        if nvec:
            i = lane.copy()
            first = True
            while (i + (UN - 1) * B < nvec).any():
                act = i + (UN - 1) * B < nvec
                js = i[:, None] + np.arange(UN)[None, :] * B
                m, s, nan = consume(m, s, nan, js, act)
                if first and self.mutant == "double_first":
                    m, s, nan = consume(m, s, nan, js, act & (lane == 0))
                first = False
                i = np.where(act, i + UN * B, i)
            while (i < nvec).any():
                act = i < nvec
                if self.mutant != "drop_rem":
                    m, s, nan = consume(m, s, nan, i[:, None], act)
                    if first and self.mutant == "double_first":
                        m, s, nan = consume(m, s, nan, i[:, None], act & (lane == 0))
                    first = False
                i = np.where(act, i + B, i)
        if tab:
            s = np.where(nan, _f32(np.nan), s)
        m, s = self.wave_reduce(m.reshape(R, B // 64, 64), s.reshape(R, B // 64, 64))
        mm, ss = m[:, 0, 0], s[:, 0, 0]
        for w in range(1, B // 64):
            mm, ss = self.merge(mm, ss, m[:, w, 0], s[:, w, 0])
        return mm, ss

    def rows(self, x, dtype, off, vocab, plan, cap, targets, fill=None):
        """(lse [R], tok_lp [R, k]) of rows x [R, >= vocab] that share the offset `off`, the
        way cs_logsoftmax_gather computes them under `plan`."""
        x = np.asarray(x, dtype=_f32)
        R = x.shape[0]
        geo = geometry(dtype, off, vocab, plan)
        parts = [self.partial(x, sp, dtype, cap) for sp in geo]
        if len(geo) == 1:
            m, s = parts[0]
            nl = STREAM_BLOCK
        else:
            nl = MERGE_LANES
            if self.mutant == "lose_last_split":
                parts = parts[:-1]
            m = np.full((R, 64), -np.inf, dtype=_f32)
            s = np.zeros((R, 64), dtype=_f32)
            for j, (pm, ps) in enumerate(parts):
                lm, ls = self.merge(m[:, j % 64], s[:, j % 64], pm, ps)
                m[:, j % 64], s[:, j % 64] = lm, ls
            m, s = self.wave_reduce(m, s)
            m, s = m[:, 0], s[:, 0]
        with np.errstate(invalid="ignore"):
            lse = (m + self.logf(s)).astype(_f32)
        t = np.asarray(targets).reshape(R, -1)
        ok = (t >= 0) & (t < vocab)
        xt = np.take_along_axis(x, np.where(ok, t, 0).astype(np.int64), axis=1)
        if cap > 0:
            xt = self.softcap_fn(xt, cap)
        with np.errstate(invalid="ignore"):
            tok = np.where(ok, xt - lse[:, None], _f32(np.nan)).astype(_f32)
        if self.mutant == "gather_first_lanes":
            tok[:, nl:] = _f32(1.5e16) if fill is None else fill      # what the buffer held
        return lse, tok

    def launch(self, L: Launch, rows=None):
        """(lse, tok_lp) of the launch's rows (or of `rows`), grouped by alignment."""
        c = L.case
        idx = np.arange(c.rows) if rows is None else np.asarray(rows)
        flat, start, _ = L.buffer()
        lse = np.empty(len(idx), dtype=_f32)
        tok = np.empty((len(idx), c.k), dtype=_f32)
        offs = np.array([c.off(int(r)) for r in idx])
        for o in np.unique(offs):
            sel = np.nonzero(offs == o)[0]
            x = np.stack([flat[start + int(idx[i]) * c.ld:start + int(idx[i]) * c.ld + c.ld]
                          for i in sel])
            lse[sel], tok[sel] = self.rows(x, c.dtype, int(o), c.V, c.plan, L.cap,
                                           L.targets[idx[sel]])
        return lse, tok
