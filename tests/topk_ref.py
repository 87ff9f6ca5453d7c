"""Geometry, planted cases, reference and wrong kernels for the two vocab top-k proposers:
cs_vocab_topk (csrc/proposer.hip) and the proposer half of cs_beam_decode_step (csrc/beam.hip,
beam_decode_kernel).

Four parts:

* the GEOMETRY restated from the sources: cs_vocab_topk's 4096-element chunks (256 lanes x 16
  slots, lane t slot j holds chunk element t + 256 j, each chunk hands over k keys, the merge
  sees nchunk * k), and the decode proposer's decode_kp / decode_layout, its chunks of
  KP * 1024 elements, its four element-to-(lane, slot) maps, ref_vec, the cached
  (nchunk_p * K <= 4096) and uncached merge and decode_rows_first; from it the POSITION
  CLASSES of a row: the elements at which a chunk, a lane, a slot, a wave, a lane group or a
  packed word begins or ends;
* PLANTED ROWS (every row of a launch is one probe): K winners at class positions, one first
  loser one step below the K-th winner at a class position, on a flat or a stairs background,
  and the extra families (one chunk, one per chunk, ties across a chunk edge, +-inf / +-0 /
  NaN, saturated values under a soft-cap, a partly filled output);
* the REFERENCE: ids by (float64 capped value descending, id ascending, NaN last), by
  selection around the k-th largest value (tests/test_topk_cases_host.py holds it to the
  oracle's sort); never derived from device output;
* a numpy RESTATEMENT of the proposers, lane by lane through the maps above, whose MUTANTS
  (thirteen wrong proposers) the checker must reject on named cases.

Planted values are multiples of 0.25 between -8 and 64 (exact in bf16 and fp16), so without a
cap every dtype holds the same row and values come back bit for bit.  Under a cap the builder
asserts that two distinct values of a row differ, after the float64 cap, by more than
2 * C_CAP * cap * 2^-24 (C_CAP: lse_ref.py's bound for softcap_fn), so the device's fp32 cap
cannot reorder them; values at or above 40 * cap and +inf saturate to exactly cap in fp32 and
in float64 and tie by id.

Rows are views of a wider buffer whose pad columns and bands before and after hold the dtype's
largest finite value: a read outside [0, vocab) of a row wins and shows as a wrong id, and the
poison lies inside the allocation.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

import lse_ref as L

F32, BF16, F16, DTYPES = L.F32, L.BF16, L.F16, L.DTYPES
EPV = L.EPV
ELT = {F32: 4, BF16: 2, F16: 2}
C_CAP, U = L.C_CAP, L.U
CAPS = (0.0, 30.0, 75.0)
POISON = {F32: 3.4028234663852886e38, BF16: 3.3895313892515355e38, F16: 65504.0}
BAND = 64

TOPK_CHUNK, TOPK_LANES, TOPK_MAX_KEYS = 4096, 256, 16384
DECODE_BLOCK = 1024
MERGE_CACHED = 4 * DECODE_BLOCK          # chunk winners the decode merge keeps in registers
BEAM_MAX_ROWS, BEAM_MAX_CAND, BEAM_MAX_BEAMS = 65536, 16384, 4096
BEAM_COUNTER_BYTES = 64 + 4 * BEAM_MAX_ROWS + 4 * BEAM_MAX_CAND


def _dt(dtype) -> str:
    """'f32' / 'bf16' / 'f16' of a name or a torch dtype."""
    return {"torch.float32": F32, "torch.bfloat16": BF16, "torch.float16": F16}.get(str(dtype), dtype)


# ---------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------
def plan_nsplit(rows: int, vocab: int, dtype) -> int:
    """The library's split plan (cs_kernels.cuh plan_split)."""
    return L.plan_split(rows, vocab, _dt(dtype))[0]


def decode_kp(B: int, vocab: int, K: int, dtype) -> int:
    """Elements per lane of a proposer chunk (beam.hip decode_kp)."""
    big = 8 if _dt(dtype) == F32 else 16
    nbig = B * -(-vocab // (big * DECODE_BLOCK))
    return 4 if nbig < 128 and -(-vocab // (4 * DECODE_BLOCK)) * K <= 16384 else big


def pad_line(n: int, elt_bytes: int) -> int:
    return (n * elt_bytes + 127) // 128 * 128 // elt_bytes


def decode_layout(A: int, B: int, vocab: int, K: int, dtype) -> dict:
    """beam.hip decode_layout: keys per lane, proposer chunks, split plan, row blocks, bytes."""
    rows = A * B
    nsplit = plan_nsplit(rows, vocab, dtype)
    kp = decode_kp(B, vocab, K, dtype)
    nchunk = -(-vocab // (kp * DECODE_BLOCK))
    total = BEAM_COUNTER_BYTES + 2 * 4 * BEAM_MAX_BEAMS
    total += 4 * B * pad_line(A, 4) + 4 * B * pad_line(K, 4)
    total += 8 * B * pad_line(nchunk * K, 8) + 8 * rows * pad_line(nsplit, 8)
    return dict(kp=kp, nchunk=nchunk, nsplit=nsplit, total=total, cached=nchunk * K <= MERGE_CACHED,
                row_blocks=rows * (-(-nsplit // L.SPLIT_QUAD) if nsplit > 1 else 1))


def decode_workspace_bytes(A: int, B: int, vocab: int, K: int) -> int:
    """cs_beam_decode_workspace_size: the larger of the bf16 and the f32 layout."""
    if min(A, B, vocab, K) <= 0:
        return 0
    return max(decode_layout(A, B, vocab, K, d)["total"] for d in (BF16, F32))


def decode_rows_first(row_blocks: int, n_cu: int) -> bool:
    """Agent-row blocks first in the grid while they leave workgroup slots free."""
    return row_blocks < 2 * n_cu


def topk_nchunk(vocab: int) -> int:
    return -(-vocab // TOPK_CHUNK)


def topk_workspace_bytes(rows: int, vocab: int, k: int) -> int:
    return 0 if min(rows, vocab, k) <= 0 else rows * topk_nchunk(vocab) * k * 8


@dataclass(frozen=True)
class Geo:
    """How one chunk's elements sit in (lane, slot): lane t holds `per` elements in groups of
    `group` consecutive ones, slot j being element (j // group * lanes + t) * group + j % group
    (group 1: t + lanes * j).  raw: 16-bit values, two slots per register."""
    name: str
    lanes: int
    per: int
    group: int
    raw: bool = False

    @property
    def CH(self):
        return self.lanes * self.per

    def elem(self, t, j):
        return (j // self.group * self.lanes + t) * self.group + j % self.group

    def table(self) -> np.ndarray:
        """[lanes, per]: the chunk element of every (lane, slot)."""
        t = np.arange(self.lanes)[:, None]
        j = np.arange(self.per)[None, :]
        return self.elem(t, j)


TOPK_GEO = Geo("topk", TOPK_LANES, TOPK_CHUNK // TOPK_LANES, 1)


def decode_geo(dtype: str, kp: int, vec: bool) -> Geo:
    """The decode proposer's four maps: fp32 vector (j/4*1024+tid)*4 + j%4, fp32 scalar
    tid + 1024 j, RAW with 4 keys per lane tid*4 + j, RAW with 16 (j/8*1024+tid)*8 + j%8."""
    if dtype == F32:
        return Geo(f"f32-kp{kp}-{'vec' if vec else 'scalar'}", DECODE_BLOCK, kp, 4 if vec else 1)
    return Geo(f"raw-kp{kp}", DECODE_BLOCK, kp, min(kp, EPV[dtype]), raw=True)


def chunk_classes(g: Geo, n: int) -> list:
    """[(class, chunk element)] of a chunk holding n <= CH elements: where its paths begin
    and end.  Names are unique; elements may repeat."""
    G, Ln, mid = g.group, g.lanes, 5
    out = [("first", 0), ("last", n - 1),
           ("lane_lo", g.elem(0, G - 1)), ("lane_hi", g.elem(1, 0)),
           ("wave_lo", g.elem(63, G - 1)), ("wave_hi", g.elem(64, 0)),
           ("slot_lo", g.elem(mid, 0)), ("slot_hi", g.elem(mid, min(1, g.per - 1))),
           ("lanes_lo", g.elem(Ln - 1, G - 1)), ("lanes_hi", g.elem(0, min(G, g.per - 1))),
           ("lastslot_lo", g.elem(0, g.per - 1)), ("lastslot_hi", g.elem(Ln - 1, g.per - 1))]
    if g.raw:
        out += [("half0", g.elem(7, 2)), ("half1", g.elem(7, 3))]
    if G > 1 and g.per > G:          # the same lane's next group
        out += [("group_lo", g.elem(3, G - 1)), ("group_hi", g.elem(3, G))]
    return [(nm, int(p)) for nm, p in out if 0 <= p < n]


CLASS_KINDS = {"first", "last", "lane_lo", "lane_hi", "wave_lo", "wave_hi", "slot_lo", "slot_hi",
               "lanes_lo", "lanes_hi", "lastslot_lo", "lastslot_hi"}
RAW_KINDS = {"half0", "half1"}
GROUP_KINDS = {"group_lo", "group_hi"}
ROW_KINDS = {"edge_lo", "edge_hi", "vocab_last", "tail_last"}


def class_kind(name: str) -> str:
    return name.split(".", 1)[-1]


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
LAYOUTS = ("aligned", "odd", "off1", "dense")


@dataclass(frozen=True)
class Case:
    """One launch shape.  path 'topk': rows x V through cs_vocab_topk.  path 'decode': B = rows
    reference rows (and A agents) through cs_beam_decode_step.
    layout: 'aligned' ld > V with ld * elt % 16 == 0; 'odd' ld * elt % 16 != 0; 'off1' aligned
    ld, row 0 one element past a 16-byte boundary; 'dense' ld == V."""
    name: str
    path: str
    dtype: str
    V: int
    K: int
    rows: int
    A: int = 0
    layout: str = "aligned"

    @property
    def ld(self):
        if self.layout == "dense":
            return self.V
        e = EPV[self.dtype]
        ld = (self.V // e + 1) * e
        return ld + 1 if self.layout == "odd" else ld

    @property
    def base_off(self):
        return 1 if self.layout == "off1" else 0

    @property
    def ref_vec(self):
        """beam.hip's ref_vec for a buffer that starts 16-byte aligned."""
        e = ELT[self.dtype]
        return self.base_off * e % 16 == 0 and self.ld * e % 16 == 0

    @property
    def kp(self):
        return decode_kp(self.rows, self.V, self.K, self.dtype) if self.path == "decode" else 16

    @property
    def CH(self):
        return TOPK_CHUNK if self.path == "topk" else self.kp * DECODE_BLOCK

    @property
    def nchunk(self):
        return -(-self.V // self.CH)

    def chunk_n(self, c: int) -> int:
        return min(self.CH, self.V - c * self.CH)

    def geo(self, c: int) -> Geo:
        if self.path == "topk":
            return TOPK_GEO
        vec = self.dtype == F32 and self.ref_vec and self.chunk_n(c) == self.CH
        return decode_geo(self.dtype, self.kp, vec)

    @property
    def geo_name(self):
        """The path a coverage table files this case under."""
        return "topk" if self.path == "topk" else self.geo(0).name

    @property
    def geokey(self):
        """What a row's content depends on (not the dtype, unless the geometry does)."""
        return (self.path, self.V, self.K, self.rows) + \
            ((self.dtype, self.ref_vec) if self.path == "decode" else ())

    def classes(self) -> list:
        """[(name, position)] of a row: chunk 0 ('c0.'), the tail chunk ('t.'), both sides of
        every chunk edge, the tail's last element and vocab - 1."""
        nc = self.nchunk
        out = [("c0." + nm, p) for nm, p in chunk_classes(self.geo(0), self.chunk_n(0))]
        if nc > 1:
            v0 = (nc - 1) * self.CH
            out += [("t." + nm, v0 + p) for nm, p in chunk_classes(self.geo(nc - 1), self.chunk_n(nc - 1))]
            out.append(("tail_last", self.V - 1))
            for b in range(1, nc):
                out += [(f"b{b}.edge_lo", b * self.CH - 1), (f"b{b}.edge_hi", b * self.CH)]
        out.append(("vocab_last", self.V - 1))
        assert all(0 <= p < self.V for _, p in out)
        return out


TOPK_K = (1, 10, 50, 256)
TOPK_ROWS = (1, 3, 300)
TAIL_N = ("1", "K-1", "K", "K+1", "255", "256", "257", "13")     # 13: no multiple of a group


def tail_n(label: str, K: int) -> int:
    return {"K-1": K - 1, "K": K, "K+1": K + 1}.get(label) if "K" in label else int(label)


def topk_vocabs(K: int) -> dict:
    """{label: V} of cs_vocab_topk's shapes for one K (V >= K; equal V keep the first label)."""
    out = {"K": K, "4095": 4095, "4096": 4096, "4097": 4097, "8192": 8192}
    out.update({"8192+" + lb: 8192 + tail_n(lb, K) for lb in TAIL_N})
    seen, keep = set(), {}
    for lb, v in out.items():
        if v >= K and v not in seen:
            keep[lb] = v
            seen.add(v)
    return keep


@lru_cache(maxsize=None)
def topk_cases(dtype: str) -> tuple:
    out = []
    for K in TOPK_K:
        for i, (lb, V) in enumerate(topk_vocabs(K).items()):
            for j, rows in enumerate(TOPK_ROWS):
                out.append(Case(f"{dtype}-topk-V{lb}-K{K}-r{rows}", "topk", dtype, V, K, rows,
                                layout=LAYOUTS[(i + j + TOPK_K.index(K)) % len(LAYOUTS)]))
    return tuple(out)


def decode_base(dtype: str, big: bool) -> int:
    """V - r of the decode shapes: two 4096-element chunks, or one chunk of 8 / 16 keys per lane."""
    return (8192 if dtype == F32 else 16384) if big else 2 * 4096


@lru_cache(maxsize=None)
def decode_cases(dtype: str) -> tuple:
    """The decode proposer's shapes: 4 keys per lane (B = 2, A = 2, V = 8192 + r), 8 / 16 keys
    per lane (B = 64, A = 1, V = 8192 + r or 16384 + r: 128 proposer workgroups), each with
    aligned rows (the vector path on full chunks) and with a misaligned base (the scalar path on
    the same chunks), the uncached merge and the 512-row grid."""
    out = []
    for big in (False, True):
        B, A = (64, 1) if big else (2, 2)
        base = decode_base(dtype, big)
        tag = "big" if big else "kp4"
        shapes = [(10, lb) for lb in TAIL_N] + [(K, lb) for K in (1, 50, 256) for lb in ("K+1", "257")]
        if not big:
            shapes += [(K, "0") for K in TOPK_K]
        for K, lb in shapes:
            r = 0 if lb == "0" else tail_n(lb, K)
            if r == 0 and lb != "0":
                continue
            for layout in ("aligned", "off1") + (("odd",) if lb == "257" else ()):
                out.append(Case(f"{dtype}-dec-{tag}-r{lb}-K{K}-{layout}", "decode", dtype, base + r,
                                K, B, A, layout))
    out.append(Case(f"{dtype}-dec-uncached", "decode", dtype, 69637, 256, 2, 2, "odd"))
    out.append(Case(f"{dtype}-dec-rows512", "decode", dtype, decode_base(dtype, True) + 257, 10, 64, 8,
                    "aligned"))
    return tuple(out)


def all_cases() -> tuple:
    return tuple(c for dt in DTYPES for c in topk_cases(dt) + decode_cases(dt))


# ---------------------------------------------------------------------------------------
# launches: every row is one probe
# ---------------------------------------------------------------------------------------
BACKGROUNDS = ("flat", "stairs")
FAMILIES = ("fill", "onechunk", "perchunk", "edge_ties", "special")
KINDS = BACKGROUNDS + FAMILIES
FLAT = -8.0
SAT = (4096.0, 8192.0)           # >= 40 * cap for every cap used here


def stairs(V: int) -> np.ndarray:
    return (-8.0 - 0.5 * (np.arange(V) // 512)).astype(np.float32)


@dataclass
class Launch:
    case: Case
    kind: str
    cap: float
    shift: int
    x: np.ndarray                                   # [rows, V] float32
    roles: list = field(default_factory=list)       # per row {position: (role, class names)}
    exp_ids: np.ndarray = None                      # [rows, K] int32
    exp_vals: np.ndarray = None                     # [rows, K] float64 (capped; zeros +0.0)

    def buffer(self):
        """(flat float32 buffer, element offset of row 0): bands and pad columns poisoned."""
        c = self.case
        start = BAND + c.base_off
        flat = np.full(start + c.rows * c.ld + BAND, POISON[c.dtype], dtype=np.float32)
        flat[start:start + c.rows * c.ld].reshape(c.rows, c.ld)[:, :c.V] = self.x
        return flat, start

    def describe(self, r: int, pos: int) -> str:
        c = self.case
        if not 0 <= pos < c.V:
            return "outside [0, vocab)"
        ch = pos // c.CH
        role, names = self.roles[r].get(pos, ("background", ()))
        return f"{role}, class {' '.join(names) or '-'}, chunk {ch} element {pos - ch * c.CH}"


def softcap64(x, cap):
    return L.softcap64(x, cap)


def expected_topk(xc: np.ndarray, K: int) -> np.ndarray:
    """ids [rows, K] by (value descending, id ascending, NaN last) of xc [rows, V] float64:
    everything above the K-th largest value, then the lowest ids that hold it."""
    rows, V = xc.shape
    nan = np.isnan(xc)
    v = np.where(nan, -np.inf, xc)
    kth = np.partition(v, V - K, axis=1)[:, V - K]
    ids = np.empty((rows, K), dtype=np.int32)
    for r in range(rows):
        gt = np.nonzero(v[r] > kth[r])[0]
        gt = gt[np.lexsort((gt, -v[r, gt]))]
        eq = np.nonzero(v[r] == kth[r])[0]
        eq = np.concatenate([eq[~nan[r, eq]], eq[nan[r, eq]]])
        ids[r] = np.concatenate([gt, eq])[:K]
    return ids


def assert_unambiguous(vals: np.ndarray, cap: float, what: str = ""):
    """Two distinct values of a row differ, after the float64 cap, by more than twice the
    fp32 cap's error bound, or are saturated to exactly the cap."""
    if cap <= 0:
        return
    v = np.unique(vals[~np.isnan(vals)].astype(np.float64))
    c = softcap64(v, cap)
    d = np.diff(c)
    sat = np.abs(v) >= 40.0 * cap
    ok = (d > 2.0 * C_CAP * cap * U) | ((d == 0) & sat[:-1] & sat[1:])
    assert ok.all(), (what, cap, v[:-1][~ok], v[1:][~ok])


def _extras(rng, V: int, taken: list, need: int, lo: int = 0, hi: Optional[int] = None) -> list:
    """`taken` filled up to `need` distinct positions with seeded ones from [lo, hi)."""
    hi = V if hi is None else hi
    out, have = list(taken), set(taken)
    while len(out) < need:
        for p in rng.integers(lo, hi, 2 * (need - len(out)) + 4):
            if int(p) not in have and len(out) < need:
                have.add(int(p))
                out.append(int(p))
    return out


def n_shifts(case: Case) -> int:
    """Launches after which every class position has been first loser, rank 0 and rank K - 1."""
    P = len(dict.fromkeys(p for _, p in case.classes()))
    return -(-P // case.rows)


@lru_cache(maxsize=6)
def _content(case: Case, kind: str, shift: int):
    """(x [rows, V] float32, roles) of a launch; depends on case.geokey only."""
    V, K, R = case.V, case.K, case.rows
    cl = case.classes()
    names = {}
    for nm, p in cl:
        names.setdefault(p, []).append(nm)
    cp = list(names)
    P = len(cp)
    bg = stairs(V) if kind == "stairs" else np.full(V, FLAT, dtype=np.float32)
    x = np.repeat(bg[None, :], R, axis=0)
    roles = []
    rng = np.random.default_rng([V, K, R, shift, sum(map(ord, kind))])

    def tag(p, role):
        return role, tuple(names.get(p, ()))

    for r in range(R):
        q = shift * R + r
        rot = [cp[(q + i) % P] for i in range(P)]
        role = {}
        if kind in ("flat", "stairs", "fill", "onechunk", "perchunk"):
            nw = K if kind != "fill" else K // 2
            lose = 1 if V > nw else 0
            need = nw + lose
            if kind == "onechunk":
                c = q % case.nchunk
                if case.chunk_n(c) < need:
                    c = 0
                lo, hi = c * case.CH, c * case.CH + case.chunk_n(c)
                pos = _extras(rng, V, [p for p in rot if lo <= p < hi][:need], need, lo, hi)
            elif kind == "perchunk":
                per = [[p for p in rot if p // case.CH == c][::-1] for c in range(case.nchunk)]
                pos, used, held = [], set(), [0] * case.nchunk
                for i in range(need):
                    c = (q + i) % case.nchunk
                    if held[c] >= case.chunk_n(c):
                        c = 0
                    lo, hi = c * case.CH, c * case.CH + case.chunk_n(c)
                    p = per[c].pop() if per[c] else -1
                    while p < 0 or p in used:
                        p = int(rng.integers(lo, hi))
                    pos.append(p)
                    used.add(p)
                    held[c] += 1
            else:
                pos = _extras(rng, V, rot[:need], need)
            w = pos[lose:]
            ranks = [0] + ([nw - 1] if nw > 1 else []) + [int(i) for i in rng.permutation(np.arange(1, max(nw - 1, 1)))]
            top = -7.5 + 0.25 * (K - 1)
            for p, k in zip(w, ranks):
                x[r, p] = top - 0.25 * k
                role[p] = tag(p, f"rank {k}")
            if lose:
                x[r, pos[0]] = top - 0.25 * nw
                role[pos[0]] = tag(pos[0], "first loser" if kind != "fill" else f"rank {nw}")
        elif kind == "edge_ties":
            T = [p for b in range(1, case.nchunk) for p in range(b * case.CH - 2, b * case.CH + 2)]
            if not T or q % 2:
                T += [0, 1, V - 2, V - 1]
            for p in sorted({p for p in T if 0 <= p < V}):
                x[r, p] = 5.0
                role[p] = tag(p, "tie")
        elif kind == "special":
            x[r] = (np.nan, -np.inf, -1.0)[q % 3]
            vals = [np.inf, 2.0, None, None, -np.inf, np.nan, np.nan, SAT[0], SAT[1]]
            pos = _extras(rng, V, rot[:min(len(vals), V)], min(len(vals), V))
            if len(pos) > 3:
                z = sorted(pos[2:4])
                pos[2:4] = z if q % 2 == 0 else z[::-1]
                vals[2:4] = [-0.0, 0.0]          # q even: -0.0 holds the lower id
            for p, v in zip(pos, vals):
                if v is not None:
                    x[r, p] = v
                    role[p] = tag(p, f"plant {v!r}")
        else:
            raise ValueError(kind)
        roles.append(role)
    x.setflags(write=False)
    return x, roles


@lru_cache(maxsize=96)
def _expected(case: Case, kind: str, shift: int, cap: float):
    x, _ = _content(case, kind, shift)
    for r in range(min(case.rows, 4)):
        assert_unambiguous(x[r], cap, (case.name, kind, r))
    with np.errstate(invalid="ignore"):
        xc = softcap64(x.astype(np.float64), cap)
    ids = expected_topk(xc, case.K)
    vals = np.take_along_axis(xc, ids.astype(np.int64), axis=1)
    return ids, np.where(vals == 0, 0.0, vals)


def _key_case(case: Case) -> Case:
    """The case that stands for every case of the same geometry in the content caches."""
    if case.path == "topk":
        return Case("", "topk", F32, case.V, case.K, case.rows)
    return Case("", "decode", case.dtype, case.V, case.K, case.rows, 0, case.layout)


def make_launch(case: Case, kind: str, shift: int = 0, cap: float = 0.0) -> Launch:
    kc = _key_case(case)
    assert kc.classes() == case.classes()
    x, roles = _content(kc, kind, shift)
    ids, vals = _expected(kc, kind, shift, float(cap))
    return Launch(case, kind, float(cap), shift, x, roles, ids, vals)


def cap_window(ref: np.ndarray, cap: float) -> np.ndarray:
    """|device value - cap * tanh(x / cap)| allowed: softcap_fn's bound and the last rounding."""
    return C_CAP * cap * U + U * np.abs(np.where(np.isfinite(ref), ref, 0.0))


def check(Ln: Launch, ids, vals=None, rows=None):
    """(failures, worst share of a cap window used) of a proposer's output: ids exactly, values
    bit for bit without a cap, inside cap_window with one."""
    c = Ln.case
    idx = np.arange(c.rows) if rows is None else np.asarray(rows)
    ids = np.asarray(ids).reshape(len(idx), c.K)
    want = Ln.exp_ids[idx]
    bad, worst = [], 0.0
    head = f"{c.name}/{Ln.kind} cap {Ln.cap:g} shift {Ln.shift}"
    for i in np.nonzero((ids != want).any(axis=1))[0]:
        r = int(idx[i])
        j = int(np.nonzero(ids[i] != want[i])[0][0])
        bad.append(f"{head} row {r} rank {j}: id {ids[i, j]} ({Ln.describe(r, int(ids[i, j]))}), want "
                   f"{want[i, j]} ({Ln.describe(r, int(want[i, j]))})")
    if vals is not None:
        vals = np.asarray(vals, dtype=np.float64).reshape(len(idx), c.K)
        ref = Ln.exp_vals[idx]
        with np.errstate(invalid="ignore"):
            if Ln.cap <= 0:
                off = ~((vals == ref) & (np.signbit(vals) == np.signbit(ref)) | (np.isnan(vals) & np.isnan(ref)))
            else:
                err = np.abs(vals - ref)
                win = cap_window(ref, Ln.cap)
                same = ~np.isfinite(ref)
                off = np.where(same, ~((vals == ref) | (np.isnan(vals) & np.isnan(ref))), ~(err <= win))
                worst = float(np.where(same | off, 0.0, err / win).max(initial=0.0))
        for i, j in zip(*np.nonzero(off)):
            if len(bad) < 40:
                bad.append(f"{head} row {idx[i]} rank {j}: value {vals[i, j]!r}, want {ref[i, j]!r}")
    return bad, worst


# ---------------------------------------------------------------------------------------
# restatement of the proposers (and their mutants)
# ---------------------------------------------------------------------------------------
MUTANTS = ("tail_drops_last", "tail_reads_past", "raw_halves_swapped", "vec_ids_on_scalar",
           "scalar_ids_on_vec", "wrong_v0", "chunk_keeps_k_minus_1", "merge_first_4096",
           "ties_desc_id", "nan_first", "negzero_below", "padding_real", "stride_ignored")
_M32 = np.uint64(0xFFFFFFFF)


class Restated:
    """Both proposers in numpy: every (lane, slot) loads its element through the chunk's map,
    builds the (order key, ~id) composite key, each chunk hands over its K largest, the merge
    takes the K largest of those.  mutant: one of MUTANTS."""

    def __init__(self, mutant: Optional[str] = None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.cap32 = L.Restated()

    def order_key(self, x: np.ndarray) -> np.ndarray:
        x = x.astype(np.float32)
        z = x if self.mutant == "negzero_below" else np.where(x == 0, np.float32(0), x)
        u = z.view(np.uint32)
        k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
        return np.where(np.isnan(x), np.uint32(0xFFFFFFFF if self.mutant == "nan_first" else 0), k)

    @staticmethod
    def key_to_float(k: np.ndarray) -> np.ndarray:
        k = k.astype(np.uint32)
        u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
        return np.where(k == 0, np.float32(np.nan), u.view(np.float32))

    def _keys(self, x32, ids):
        lo = ids.astype(np.uint64) if self.mutant == "ties_desc_id" else _M32 - ids.astype(np.uint64)
        return (self.order_key(x32).astype(np.uint64) << np.uint64(32)) | lo

    def launch(self, Ln: Launch, rows=None):
        """(ids [n, K] int32, values [n, K] float32) of the launch's rows (or of `rows`)."""
        c, m = Ln.case, self.mutant
        idx = np.arange(c.rows) if rows is None else np.asarray(rows)
        flat, start = Ln.buffer()
        ld = c.V if m == "stride_ignored" else c.ld
        CH, K, nc = c.CH, c.K, c.nchunk
        step = CH // 2 if m == "wrong_v0" else CH
        parts = np.zeros((len(idx), nc, K), dtype=np.uint64)
        for ch in range(nc):
            g = c.geo(ch)
            v0 = ch * step
            n = min(CH, c.V - v0)
            if ch == nc - 1:
                if m == "tail_drops_last":
                    n -= 1
                if m == "tail_reads_past" and n < CH:
                    n += 1
            la = g.table()                           # the element each (lane, slot) loads
            lb = la                                  # ... and the element its id names
            if m == "raw_halves_swapped" and g.raw:
                la = la.reshape(g.lanes, g.per // 2, 2)[:, :, ::-1].reshape(g.lanes, g.per)
            if c.dtype == F32 and c.path == "decode":
                other = decode_geo(F32, c.kp, g.group == 1).table()
                if (m == "vec_ids_on_scalar" and g.group == 1) or (m == "scalar_ids_on_vec" and g.group > 1):
                    lb = other
            la, lb = la.reshape(-1), lb.reshape(-1)
            base = start + idx[:, None] * ld + v0
            with np.errstate(invalid="ignore"):
                x = np.where(la[None, :] < n, flat[np.minimum(base + la[None, :], len(flat) - 1)],
                             np.float32(0))
                if Ln.cap > 0:
                    x = self.cap32.softcap_fn(x, Ln.cap)
            key = self._keys(x, v0 + np.broadcast_to(lb[None, :], x.shape))
            if m != "padding_real":
                key = np.where(lb[None, :] < n, key, np.uint64(0))
            key = np.sort(key, axis=1)[:, ::-1]
            keep = K - 1 if m == "chunk_keeps_k_minus_1" else K
            top = key[:, :keep]
            parts[:, ch, :top.shape[1]] = top
        allk = parts.reshape(len(idx), nc * K)
        if m == "merge_first_4096":
            allk = allk[:, :MERGE_CACHED]
        srt = np.sort(allk, axis=1)[:, ::-1][:, :K]
        if srt.shape[1] < K:
            srt = np.concatenate([srt, np.zeros((len(idx), K - srt.shape[1]), np.uint64)], axis=1)
        low = srt & _M32
        ids = (low if m == "ties_desc_id" else _M32 - low).astype(np.int64)
        return np.where(srt == 0, np.int64(-1), ids).astype(np.int32), self.key_to_float(srt >> np.uint64(32))
