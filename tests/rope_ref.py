"""Reference, cases and checker for cs_rope_place and its three siblings (csrc/attn.hip), in
numpy alone: no device, no import of the package.

Reference (float64).  Token (s, t) of group i = s // n_str sits at position
plen[gp[i]] + hb + t (gp the identity when None).  The angle of pair j is the FP32 product
float32(pos) * inv_freq[j], widened to float64 -- the entry point's documented contract,
"angle = position * inv_freq[i]", fp32 rotation -- and
    y1 = x1 cos a - x2 sin a,   y2 = x2 cos a + x1 sin a      pairs (j, j + D/2)
in float64.  q lands at [s*T + t][h], K at [s][g][hb + t], V's bits unchanged at
[s][g][hb + t] of the row layout or of the blocked [S][Hkv][ldh/32][D][32] layout.

Rounding window.  rne_bf16 rounds a float64 to bf16 (nearest, ties to even) with
frexp / rint, never through fp32.  A bf16 output `got` for reference `ref` passes iff
    rne(ref - delta) <= got <= rne(ref + delta),     delta = (|x1| + |x2|) 2^-21.
delta is derived, not measured: sincosf is within 2 fp32 ulps (<= 2^-23 absolute, |sin|,
|cos| <= 1), the kernel rounds one fp32 product (<= |x2| 2^-24) and one fp32 fma
(<= (|x1| + |x2|) 2^-24): together at most (|x1| + |x2|) (2^-23 + 2^-24) < (|x1| + |x2|)
2^-22 from ref, and delta doubles that.  Where ref is not within delta of a bf16 tie the
window is one value: the correctly rounded result.  tests/test_rope_cases_host.py asserts
that the window is open on at most 1 % of a random case's elements, that an fp32
restatement of the kernel's arithmetic with sin / cos pushed 2 ulps either way stays inside
every window, and that the checker rejects each of a list of subtly wrong kernels.

Planted tables need no window: inv_freq == 0 returns the input bits, and a quarter turn
(pos a power of two, inv_freq[j] = float32(pi/2) / pos, integer operands 1 .. 15) returns
y1 = -x2, y2 = x1 exactly (|x1 cos| < 2^-20 vanishes in the bf16 rounding).  Launch b of a
quarter-turn family turns the pairs whose index has bit b set and leaves the others, a last
launch turns every pair: ceil(log2(D/2)) + 1 launches tell every frequency index from every
other, and decode_freq_index names the index a failing kernel used."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

SENT16 = 0x5A5A
DELTA_SCALE = 2.0 ** -21
F32_HALF_PI = np.float32(math.pi / 2)

LLAMA31_ROPE = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                "original_max_position_embeddings": 8192}
# preset -> (rope_theta, rope_scaling, head_dim): the configs alone, no weights
ROPE_CFG = {"llama-3.1-8b": (500000.0, LLAMA31_ROPE, 128),
            "gemma-2-9b": (10000.0, None, 256),
            "tiny-llama": (500000.0, LLAMA31_ROPE, 16)}


def table_inv_freq(preset: str, D: int) -> np.ndarray:
    """The preset's rope_inv_freq at head_dim D (model.rope_inv_freq restated in numpy)."""
    theta, rs, _ = ROPE_CFG[preset]
    inv = 1.0 / (theta ** (np.arange(0, D, 2, dtype=np.float64) / D))
    if rs:
        factor, lo, hi = rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"]
        old = rs["original_max_position_embeddings"]
        wavelen = 2 * math.pi / inv
        scaled = np.where(wavelen > old / lo, inv / factor, inv)
        smooth = (old / wavelen - lo) / (hi - lo)
        smoothed = (1 - smooth) * scaled / factor + smooth * scaled
        medium = (wavelen >= old / hi) & (wavelen <= old / lo)
        inv = np.where(medium, smoothed, scaled)
    return inv.astype(np.float32)


# --- bf16 ------------------------------------------------------------------------------------------

def bf16_value(bits) -> np.ndarray:
    """uint16 bf16 bit patterns -> their float64 values."""
    b = np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)
    with np.errstate(invalid="ignore"):             # V's signalling NaN patterns
        return b.view(np.float32).astype(np.float64)


def rne_bf16(x) -> np.ndarray:
    """float64 -> bf16 bit patterns, round to nearest even, exactly: the 8-bit significand
    by frexp / rint (subnormals on the fixed 2^-133 grid, overflow to inf)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    e = np.maximum(e, -125)
    q = np.rint(np.ldexp(x, 8 - e))                 # an integer, |q| <= 256: exact
    v = np.ldexp(q, e - 8)                          # a bf16 value or +-2^128
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)                    # exact; 2^128 -> inf
    return (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def fold_f32(part: np.ndarray, order=None) -> np.ndarray:
    """fp32 sum of the splits in split order (IEEE adds, as the kernel's)."""
    idx = list(range(part.shape[0])) if order is None else list(order)
    acc = part[idx[0]].astype(np.float32).copy()
    for sp in idx[1:]:
        acc = (acc + part[sp]).astype(np.float32)
    return acc


# --- cases -----------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    D: int
    H: int
    Hkv: int
    hb: int
    T: int
    ldh: int
    table: str = "tiny-llama"      # a ROPE_CFG preset | "zero" | "quarter:<bit>" | "quarter:all"
    col0: int = 0                  # qkv = buf[:, col0 : col0 + width] of a [n_tok, width + ldpad] buffer
    ldpad: int = 0
    v_rows: bool = False
    plen: Tuple[int, ...] = (0, 131071, 1000)
    gp: Optional[Tuple[int, ...]] = None
    n_str: int = 2
    splits: int = 0                # > 0: the projection arrives as fp32 K-split partials
    plant: str = ""                # partials: "big_last" the last split of magnitude 1e30;
                                   # "cancel" splits 0 and 1 are B and -B, |B| ~ 2^20 (only the
                                   # kernel's own order, (B - B) + rest, keeps the rest)
    ints: bool = False             # q / k operands integers 1 .. 15
    seed: int = 0

    def __str__(self):
        return self.name

    @property
    def n_groups(self):
        return len(self.gp) if self.gp is not None else len(self.plen)

    @property
    def S(self):
        return self.n_groups * self.n_str

    @property
    def n_tok(self):
        return self.S * self.T

    @property
    def nh(self):
        return self.H + 2 * self.Hkv

    @property
    def width(self):
        return self.nh * self.D

    @property
    def half(self):
        return self.D // 2

    @property
    def random(self):
        return self.table in ROPE_CFG

    def path(self):
        """The launch csrc/attn.hip's rope_place_impl picks: (pairs per item, workgroups per
        token, V by tiles)."""
        if self.splits:
            p8 = True
        else:
            p8 = (self.width + self.ldpad) % 8 == 0 and self.col0 % 8 == 0 and self.D % 16 == 0
        items = self.nh * self.half // (8 if p8 else 4)
        tiles = (not self.splits and not self.v_rows and self.T >= 32
                 and (self.width + self.ldpad) % 8 == 0 and self.col0 % 8 == 0)
        return (8 if p8 else 4), -(-items // 256), tiles

    def inv_freq(self) -> np.ndarray:
        if self.table == "zero":
            return np.zeros(self.half, dtype=np.float32)
        if self.table.startswith("quarter:"):
            pos = self.positions()
            assert len(set(pos.tolist())) == 1 and pos[0] & (pos[0] - 1) == 0 and pos[0] > 0
            q = np.float32(F32_HALF_PI / np.float32(pos[0]))            # exact: a power of two
            assert np.float32(pos[0]) * q == F32_HALF_PI
            bit = self.table.split(":")[1]
            j = np.arange(self.half)
            on = np.ones(self.half, bool) if bit == "all" else ((j >> int(bit)) & 1).astype(bool)
            return np.where(on, q, np.float32(0)).astype(np.float32)
        return table_inv_freq(self.table, self.D)

    def turned(self) -> np.ndarray:
        """quarter-turn tables: which pairs are turned."""
        return self.inv_freq() != 0

    def positions(self, gp_ignored=False, shift=0) -> np.ndarray:
        """[n_tok] int64, token (s, t) at s * T + t."""
        s = np.repeat(np.arange(self.S), self.T)
        t = np.tile(np.arange(self.T), self.S)
        gi = s // self.n_str
        p = np.asarray(self.gp)[gi] if self.gp is not None and not gp_ignored else \
            np.minimum(gi, len(self.plen) - 1)
        return np.asarray(self.plen, dtype=np.int64)[p] + self.hb + t + shift

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        """(x bits [n_tok, nh, D] uint16 -- the bf16 projection, folded where the case has
        partials --, part float32 [splits, n_tok, width] or None).  q / k finite and non-zero;
        V any 16-bit pattern (-0, subnormals, Inf, NaN payloads) where the input is bf16."""
        rng = np.random.default_rng(1000 + self.seed)
        n_tok, nh, D = self.n_tok, self.nh, self.D
        if self.splits:
            part = (rng.standard_normal((self.splits, n_tok, self.width)) * 2).astype(np.float32)
            if self.plant == "big_last":
                part[-1] = (rng.standard_normal((n_tok, self.width)) * 1e30).astype(np.float32)
            if self.plant == "cancel":
                part[0] = np.ldexp(np.float32(1) + rng.random((n_tok, self.width), dtype=np.float32), 20)
                part[1] = -part[0]
            x = rne_bf16(fold_f32(part).astype(np.float64)).reshape(n_tok, nh, D)
            part.setflags(write=False)
            x.setflags(write=False)
            return x, part
        if self.ints:
            val = rng.integers(1, 16, size=(n_tok, nh, D)).astype(np.float64)
        else:
            val = rng.standard_normal((n_tok, nh, D)) * 2
        x = rne_bf16(val)
        x[(x & 0x7FFF) == 0] = 0x3F80
        v = rng.integers(0, 65536, size=(n_tok, self.Hkv, D)).astype(np.uint16)
        special = np.array([0x8000, 0x0001, 0x8001, 0x007F, 0x7F80, 0xFF80, 0x7FC1, 0xFFFF, 0x7F81],
                           dtype=np.uint16)
        flat = v.reshape(-1)
        flat[rng.choice(flat.size, size=min(flat.size, 4 * special.size), replace=False)] = \
            np.tile(special, 4)[:min(flat.size, 4 * special.size)]
        x[:, self.H + self.Hkv:] = v
        x.setflags(write=False)
        return x, None


@dataclass
class Expect:
    q_ref: np.ndarray      # float64 [n_tok, H, D]
    k_ref: np.ndarray      # float64 [S, Hkv, T, D]
    q_lo: np.ndarray       # bf16 bits of rne(ref - delta), rne(ref + delta)
    q_hi: np.ndarray
    k_lo: np.ndarray
    k_hi: np.ndarray
    q_delta: np.ndarray
    k_delta: np.ndarray
    v_full: np.ndarray     # uint16, the whole V buffer: sentinel but for the placed slots

    def open_share(self) -> float:
        n = self.q_lo.size + self.k_lo.size
        return float(((self.q_lo != self.q_hi).sum() + (self.k_lo != self.k_hi).sum()) / n)


def rotate_f64(x_bits: np.ndarray, inv: np.ndarray, pos: np.ndarray):
    """x bits [n_tok, heads, D] -> (ref float64 [n_tok, heads, D], delta)."""
    half = x_bits.shape[-1] // 2
    ang = (pos.astype(np.float32)[:, None] * inv.astype(np.float32)[None, :]).astype(np.float32)
    a = ang.astype(np.float64)
    c, s = np.cos(a)[:, None, :], np.sin(a)[:, None, :]
    x = bf16_value(x_bits)
    x1, x2 = x[..., :half], x[..., half:]
    ref = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)
    d = (np.abs(x1) + np.abs(x2)) * DELTA_SCALE
    return ref, np.concatenate([d, d], axis=-1)


def v_shape(c: Case):
    return (c.S, c.Hkv, c.ldh, c.D) if c.v_rows else (c.S, c.Hkv, c.ldh // 32, c.D, 32)


@functools.lru_cache(maxsize=None)
def expected(c: Case) -> Expect:
    x, _ = c.inputs()
    H, Hkv, T, S, D = c.H, c.Hkv, c.T, c.S, c.D
    ref, delta = rotate_f64(x[:, :H + Hkv], c.inv_freq(), c.positions())
    q_ref, q_d = ref[:, :H], delta[:, :H]
    k_ref = ref[:, H:].reshape(S, T, Hkv, D).transpose(0, 2, 1, 3)
    k_d = delta[:, H:].reshape(S, T, Hkv, D).transpose(0, 2, 1, 3)
    v = x[:, H + Hkv:].reshape(S, T, Hkv, D)
    v_full = np.full(v_shape(c), SENT16, dtype=np.uint16)
    for t in range(T):
        slot = c.hb + t
        if c.v_rows:
            v_full[:, :, slot, :] = v[:, t]
        else:
            v_full[:, :, slot // 32, :, slot % 32] = v[:, t]
    return Expect(q_ref, k_ref, rne_bf16(q_ref - q_d), rne_bf16(q_ref + q_d), rne_bf16(k_ref - k_d),
                  rne_bf16(k_ref + k_d), q_d, k_d, v_full)


def planted_expected(c: Case):
    """Exact q [n_tok, H, D] and K [S, Hkv, T, D] bits of a planted table ("zero": the input;
    "quarter:*": turned pairs y1 = -x2, y2 = x1)."""
    assert not c.random
    x, _ = c.inputs()
    H, Hkv, half = c.H, c.Hkv, c.half
    qk = x[:, :H + Hkv].copy()
    if c.table != "zero":
        on = c.turned()
        x1, x2 = x[:, :H + Hkv, :half], x[:, :H + Hkv, half:]
        qk[..., :half] = np.where(on, x2 ^ np.uint16(0x8000), x1)
        qk[..., half:] = np.where(on, x1, x2)
    k = qk[:, H:].reshape(c.S, c.T, Hkv, c.D).transpose(0, 2, 1, 3)
    return qk[:, :H], k


# --- checker ---------------------------------------------------------------------------------------

def _first(mask, what, got, lo, hi):
    i = tuple(int(v) for v in np.argwhere(mask)[0])
    return (f"{what}: {int(mask.sum())} of {mask.size} elements wrong, first at {i}: got "
            f"{bf16_value(got[i])!r} (0x{int(got[i]):04x}), want [{bf16_value(lo[i])!r}, {bf16_value(hi[i])!r}]")


def _outside(got, lo, hi):
    g = bf16_value(got)
    return ~((bf16_value(lo) <= g) & (g <= bf16_value(hi)))      # a NaN is outside


def check(c: Case, q, kh, vh) -> list:
    """Every complaint about one launch's outputs (uint16 views of q_out [n_tok, H, D], k_hist
    [S, Hkv, ldh, D] and vt_hist in its layout, each pre-filled with SENT16): [] when slots
    [hb, hb + T) hold the expected values and every other element is still the sentinel."""
    out = []
    q, kh, vh = (np.asarray(a).view(np.uint16) for a in (q, kh, vh))
    kw = kh[:, :, c.hb:c.hb + c.T]
    if c.random:
        e = expected(c)
        bad = _outside(q, e.q_lo, e.q_hi)
        if bad.any():
            out.append(_first(bad, f"{c} q_out", q, e.q_lo, e.q_hi))
        bad = _outside(kw, e.k_lo, e.k_hi)
        if bad.any():
            out.append(_first(bad, f"{c} k_hist[s][g][hb + t]", kw, e.k_lo, e.k_hi))
    else:
        pq, pk = planted_expected(c)
        for what, got, want in ((f"{c} q_out", q, pq), (f"{c} k_hist[s][g][hb + t]", kw, pk)):
            if not np.array_equal(got, want):
                msg = _first(got != want, what, got, want, want)
                if c.table.startswith("quarter:"):
                    msg += " (decode_freq_index over the family's launches names the index used)"
                out.append(msg)
    rest = kh.copy()
    rest[:, :, c.hb:c.hb + c.T] = SENT16
    if (rest != SENT16).any():
        i = tuple(int(v) for v in np.argwhere(rest != SENT16)[0])
        out.append(f"{c} k_hist: {int((rest != SENT16).sum())} elements outside slots "
                   f"[{c.hb}, {c.hb + c.T}) written, first at [s, g, slot, d] = {i}")
    vf = expected(c).v_full
    if vh.shape != vf.shape or not np.array_equal(vh, vf):
        bad = vh.reshape(vf.shape) != vf
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        out.append(f"{c} v{'' if c.v_rows else 't'}_hist: {int(bad.sum())} elements differ (placed "
                   f"bits or sentinel), first at {i}: got 0x{int(vh.reshape(vf.shape)[i]):04x}, "
                   f"want 0x{int(vf[i]):04x}")
    return out


def decode_freq_index(family, q_outs) -> np.ndarray:
    """The frequency index each pair of q_out used, read off a quarter-turn family's bit
    launches (a turned pair has y1 < 0): [n_tok, H, D/2] int."""
    idx = 0
    for c, q in zip(family, q_outs):
        bit = c.table.split(":")[1]
        if bit == "all":
            continue
        y1 = np.asarray(q).view(np.uint16)[..., :c.half]
        idx = idx + (((y1 >> 15) & 1).astype(np.int64) << int(bit))
    return idx


# --- the kernel's arithmetic, restated in numpy fp32 (for the host tests) ---------------------------

MUTANTS = ("pos_off_by_one", "interleaved_pairs", "sine_sign", "freq_index_shift", "bf16_truncate",
           "group_prefix_ignored", "v_slot_off_by_one", "v_tile_ignored", "surplus_split_summed",
           "splits_reversed")


def _nudge(x, k):
    """k fp32 ulps up (k > 0) or down."""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def emulate(c: Case, mut=(), ulps: Tuple[int, int] = (0, 0)):
    """rope_place_kernel's arithmetic in fp32 (fp32 angle, sin / cos rounded to fp32 and moved
    by ulps = (sin, cos) fp32 ulps, one rounded product, one fma, bf16 RNE), with the wrong
    kernels of MUTANTS on request.  Returns uint16 (q, k_hist, v_hist) in the launch's layouts,
    sentinel-filled, and the fp32 values before rounding [n_tok, H + Hkv, D]."""
    mut = frozenset(mut)
    assert mut <= set(MUTANTS)
    x, part = c.inputs()
    H, Hkv, T, S, D, half = c.H, c.Hkv, c.T, c.S, c.D, c.half
    if part is not None:
        order = list(range(c.splits))
        if "splits_reversed" in mut:
            order = order[::-1]
        if "surplus_split_summed" in mut:
            nsp = 2 if c.splits <= 2 else (4 if c.splits <= 4 else 8)
            order += [c.splits - 1] * (-c.splits % nsp)
        x = rne_bf16(fold_f32(part, order).astype(np.float64)).reshape(c.n_tok, c.nh, D)
    pos = c.positions(gp_ignored="group_prefix_ignored" in mut, shift=int("pos_off_by_one" in mut))
    inv = c.inv_freq()
    if "freq_index_shift" in mut:
        inv = np.roll(inv, -1)
    ang = (pos.astype(np.float32)[:, None] * inv[None, :]).astype(np.float32)
    a = ang.astype(np.float64)
    sn = _nudge(np.sin(a).astype(np.float32), ulps[0])[:, None, :]
    cs = _nudge(np.cos(a).astype(np.float32), ulps[1])[:, None, :]
    if "sine_sign" in mut:
        sn = -sn
    xv = bf16_value(x[:, :H + Hkv]).astype(np.float32)
    if "interleaved_pairs" in mut:
        x1, x2 = xv[..., 0::2], xv[..., 1::2]
    else:
        x1, x2 = xv[..., :half], xv[..., half:]
    # fma(x1, cs, -(x2 * sn)): the bf16 x fp32 products are exact in float64, the sum rounded
    # once more on the way to fp32 (a second rounding of at most 2^-53 relative)
    p1, p2 = (x2 * sn).astype(np.float32), (x1 * sn).astype(np.float32)
    y1 = (x1.astype(np.float64) * cs - p1.astype(np.float64)).astype(np.float32)
    y2 = (x2.astype(np.float64) * cs + p2.astype(np.float64)).astype(np.float32)
    y = np.empty_like(xv)
    if "interleaved_pairs" in mut:
        y[..., 0::2], y[..., 1::2] = y1, y2
    else:
        y[..., :half], y[..., half:] = y1, y2
    if "bf16_truncate" in mut:
        yb = (y.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    else:
        yb = rne_bf16(y.astype(np.float64))
    q = yb[:, :H].copy()
    kh = np.full((S, Hkv, c.ldh, D), SENT16, dtype=np.uint16)
    kh[:, :, c.hb:c.hb + T] = yb[:, H:].reshape(S, T, Hkv, D).transpose(0, 2, 1, 3)
    v = x[:, H + Hkv:].reshape(S, T, Hkv, D)
    vflat = np.full(S * Hkv * c.ldh * D + 32 * D, SENT16, dtype=np.uint16)   # room for a slot too far
    sg = (np.arange(S)[:, None] * Hkv + np.arange(Hkv)[None, :])[:, :, None]
    d = np.arange(D)[None, None, :]
    for t in range(T):
        slot = c.hb + t + int("v_slot_off_by_one" in mut)
        if c.v_rows:
            idx = (sg * c.ldh + slot) * D + d
        else:
            tile = 0 if "v_tile_ignored" in mut else slot & ~31
            idx = (sg * c.ldh + tile) * D + d * 32 + (slot & 31)
        vflat[idx] = v[:, t]
    vh = vflat[:S * Hkv * c.ldh * D].reshape(v_shape(c))
    return q, kh, vh, y


# --- case lists ------------------------------------------------------------------------------------

ITEMS8 = ((64, 8, 2, "tiny-llama"), (128, 32, 8, "llama-3.1-8b"), (256, 16, 8, "gemma-2-9b"))
ITEMS4_OFFSET = ((64, 8, 2, "tiny-llama"), (128, 64, 8, "llama-3.1-8b"), (256, 16, 8, "gemma-2-9b"))
ITEMS4_HEAD_DIM = ((8, 6, 2, "tiny-llama"), (24, 4, 2, "tiny-llama"), (40, 6, 3, "tiny-llama"))
SLOTS_TOKEN = ((0, 1, 64), (5, 3, 64), (31, 2, 64), (32, 1, 64), (37, 2, 64), (63, 1, 64), (37, 2, 96))
SLOTS_TILE = ((0, 32, 32), (5, 40, 64), (8, 33, 64), (29, 35, 64), (24, 64, 96))
PLENS = ((0, 131071, 1000), (17, 0, 131071), (131071, 1000, 0))
GROUP_MAPS = (((0, 17, 1000, 131071), (3, 1, 3), 2), ((0, 17, 1000, 131071), (2, 0, 3, 1, 2), 1))
FOLD_SPLITS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17)


def _ceil32(n):
    return -(-n // 32) * 32


def _mk(tag, item, hb, T, ldh, seed, **kw):
    D, H, Hkv, table = item
    kw.setdefault("table", table)
    kw.setdefault("plen", PLENS[seed % len(PLENS)])
    name = f"{tag}-D{D}H{H}k{Hkv}-hb{hb}T{T}ld{ldh}" + ("-rows" if kw.get("v_rows") else "")
    if kw.get("gp"):
        name += f"-g{len(kw['gp'])}"
    return Case(name, D, H, Hkv, hb, T, ldh, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def random_cases():
    """bf16-input cases on the real tables: every item path x both V layouts at (hb, T) =
    (5, 3); every per-token slot case x both V layouts on an 8-pair and a 4-pair shape; every
    tile-path slot case on the three 8-pair shapes and D = 24; T >= 32 on the per-token path;
    the group maps."""
    out, seed = [], 0

    def add(*a, **kw):
        nonlocal seed
        out.append(_mk(*a, seed=seed, **kw))
        seed += 1

    for rows in (False, True):
        for it in ITEMS8:
            add("p8", it, 5, 3, 64, v_rows=rows)
        for it in ITEMS4_OFFSET:
            add("p4off", it, 5, 3, 64, v_rows=rows, col0=4, ldpad=8)
        for it in ITEMS4_HEAD_DIM:
            add("p4dim", it, 5, 3, 64, v_rows=rows)
        for hb, T, ldh in SLOTS_TOKEN:
            add("slot", ITEMS8[0], hb, T, ldh, v_rows=rows)
            add("slot", ITEMS4_HEAD_DIM[2], hb, T, ldh, v_rows=rows)
    for hb, T, ldh in SLOTS_TILE:
        for it in ITEMS8 + (ITEMS4_HEAD_DIM[1],):
            add("tile", it, hb, T, ldh)
    add("long-p4off", ITEMS8[1], 5, 40, 64, col0=4, ldpad=8)
    add("long-p4off", ITEMS8[1], 5, 40, 64, col0=4, ldpad=8, v_rows=True)
    add("long", ITEMS8[1], 5, 40, 64, v_rows=True)
    add("long-ld4", ITEMS8[0], 5, 40, 64, ldpad=4)
    for plen, gp, n_str in GROUP_MAPS:
        add("gmap", ITEMS8[0], 5, 3, 64, plen=plen, gp=gp, n_str=n_str)
        add("gmap", ITEMS8[0], 5, 3, 64, plen=plen, gp=gp, n_str=n_str, v_rows=True)
        add("gmap-tile", ITEMS8[1], 8, 33, 64, plen=plen, gp=gp, n_str=n_str)
    for c in out:
        p, _, tiles = c.path()
        assert p == (4 if c.name.startswith(("p4", "long-p4", "long-ld4")) or c.D % 16 else 8), c
        assert tiles == c.name.startswith(("tile", "gmap-tile")), c
    assert {1, 2, 5} <= {c.path()[1] for c in out}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def zero_cases():
    """inv_freq == 0 on every item path and both routes of V: q and K are the input bits."""
    out = []
    for i, it in enumerate(ITEMS8 + ITEMS4_HEAD_DIM):
        out.append(_mk("zero", it, 37, 2, 64, 100 + i, table="zero", v_rows=bool(i % 2)))
        out.append(_mk("zero-tile", it, 29, 35, 64, 110 + i, table="zero"))
    for i, it in enumerate(ITEMS4_OFFSET):
        out.append(_mk("zero-p4off", it, 31, 2, 64, 120 + i, table="zero", col0=4, ldpad=8))
    return tuple(out)


def quarter_family(item, hb, log2pos, seed, **kw):
    """ceil(log2(D/2)) + 1 launches on the same operands (T = 1, every token at position
    2^log2pos): bit b of the pair index for each b, then every pair."""
    D = item[0]
    nb = max(1, math.ceil(math.log2(D // 2)))
    plen = ((1 << log2pos) - hb,) * 3
    fam = [_mk(f"quarter{b}", item, hb, 1, 64, seed, table=f"quarter:{b}", plen=plen, ints=True, **kw)
           for b in list(range(nb)) + ["all"]]
    assert len(fam) <= math.ceil(math.log2(D // 2)) + 1 or D // 2 == 1
    return tuple(fam)


@functools.lru_cache(maxsize=None)
def quarter_families():
    out = []
    for i, it in enumerate(ITEMS8 + ITEMS4_HEAD_DIM):
        out.append(quarter_family(it, 5 + 32 * (i % 2), 6 + 2 * i, 200 + i, v_rows=bool(i % 2)))
    for i, it in enumerate(ITEMS4_OFFSET):
        out.append(quarter_family(it, 31, 17 - i, 210 + i, col0=4, ldpad=8))
    return tuple(out)


def fold_shape(splits, T):
    if splits == 9 and T == 1:
        return ITEMS8[2]
    return ITEMS8[1] if T == 1 else ITEMS8[0]


@functools.lru_cache(maxsize=None)
def fold_cases():
    """Every split count x T in {1, 3} x both V layouts, on a real table and on the zero table
    (same operands); two more with a last split of magnitude 1e30 and two whose first two
    splits cancel."""
    out = []
    for i, sp in enumerate(FOLD_SPLITS):
        for T in (1, 3):
            for rows in (False, True):
                seed = 300 + 4 * i + 2 * (T == 3) + rows
                out.append(_mk(f"fold{sp}", fold_shape(sp, T), 30, T, 64, seed, splits=sp, v_rows=rows))
    out.append(_mk("fold5-big", ITEMS8[0], 30, 3, 64, 399, splits=5, plant="big_last"))
    out.append(_mk("fold17-big", ITEMS8[0], 30, 3, 64, 398, splits=17, plant="big_last", v_rows=True))
    out.append(_mk("fold5-cancel", ITEMS8[0], 30, 3, 64, 397, splits=5, plant="cancel"))
    out.append(_mk("fold12-cancel", ITEMS8[1], 30, 1, 64, 396, splits=12, plant="cancel", v_rows=True))
    return tuple(out)


def zero_table(c: Case) -> Case:
    return replace(c, name=c.name + "-zero", table="zero")

