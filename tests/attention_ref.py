"""fp64 reference, error bound, case builders and a NumPy restatement of cs_prefix_attention
(csrc/attn.hip) for tests/test_attention_cases_host.py and tests/test_attention_edges_gpu.py.

Random q / K / V cannot see a wrong mask edge or a missing softmax rescale (the outputs are
averages of hundreds of V rows, and the running max never jumps after the first key
block).  The cases built here have answers that ONE key decides:

  planted key   K[slot] = c q_row / (scale |q_row|^2): its score is c nats above a small
                random background for the target row, ~0 for every other row that reads
                the same K row (their q is made orthogonal to the target's).  V[slot] is a
                distinctive row (mean 8, sigma 4): visible -> the output is that row,
                invisible -> the output is the background average.
  staircase     the keys of key block j score level[j] log2 units above block 0 (a few "hot"
                ones a little more), V means alternate in sign and grow: every block moves
                the running max, and a missing / doubled rescale or a wrong combine weight
                changes the output by far more than the bound.

The bound, for out (bf16) against the fp64 reference over the SAME bf16 inputs:
    |out - ref| <= 2^-7 A + 1e-30,   A = sum_i p_i |v_i|
(2^-9 A for the bf16 rounding of the output, 2^-9 A for the bf16 rounding of P before the
P.V MFMA, a factor 2 for the fp32 accumulation and the exp2 / rcp approximations).

``reference`` also takes mask mutants, ``emulate`` restates attend_block's order of
operations (32-key blocks, wave-striped blocks, the lazy rescale behind a wave-wide
ballot, a bf16 P, the wave combine and the split merge) and takes arithmetic mutants; the
host test uses both to prove that every case would catch the mutant it is aimed at."""
import math
import zlib

import numpy as np
import torch

BF = torch.bfloat16
LOG2E = 1.4426950408889634
LAZY = 8.0            # kLazyRescale
GROUP_ROWS = 64       # kGroupRows
MERGE_ROWS = 8        # kMergeRows
MAX_SPLIT = 32        # kMaxSplit
PLAN_MIN_BASE = 1024
PLAN_TARGET = 512
PLAN_MIN_ITEMS = 3

REF_MUTANTS = ("limit+1", "limit-1", "window+1", "window-1", "neighbour", "future")
EMU_MUTANTS = ("norescale", "rescale_l_only", "combine1")


def ceil32(n):
    return max(32, (n + 31) // 32 * 32)


def bound_of(A):
    return 2.0 ** -7 * A + 1e-30


def _f64(x):
    return x.float().numpy().astype(np.float64)


def _bf16_round(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, NumPy."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


class Case:
    """One attention problem (CPU bf16 tensors in the kernel's logical layouts: V row-major,
    the history as the copied history a slot table describes) and the rows it is aimed at.

    checks: [(mutant, tok, head)]: the mutant must move out[tok, head] by >= 16 x the bound.
    """

    def __init__(self, name, family, D, rep, n_str, T, plens, gmap, hb, cap, window, host_lens,
                 Hkv=2, sigma=0.5, scale=None, ldh=None):
        self.name, self.family = name, family
        self.D, self.rep, self.Hkv, self.H = D, rep, Hkv, rep * Hkv
        self.n_str, self.T = n_str, T
        self.plens, self.gmap = list(plens), (None if gmap is None else list(gmap))
        self.n_grp = len(plens) if gmap is None else len(gmap)
        self.S = self.n_grp * n_str
        self.hb, self.ldh = hb, ceil32(hb + T) if ldh is None else ldh
        self.cap, self.window = float(cap), int(window)
        self.scale = float(D ** -0.5 if scale is None else scale)
        self.host_lens = list(plens if host_lens is None else host_lens)
        self.checks = []
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        self.gen = g

        def rnd(*shape, s=sigma):
            return (torch.randn(*shape, generator=g) * s).to(BF)

        self.off, o = [], 0
        for n in self.plens:
            self.off.append(o)
            o += ceil32(n)
        self.Lp = o
        self.q = rnd(self.S * T, self.H, D)
        # every slot random, the invisible ones (prefix padding, history slots >= hb + T)
        # included: finite garbage that no query may see
        self.kflat, self.vflat = rnd(Hkv, o, D), rnd(Hkv, o, D)
        self.kh, self.vh = rnd(self.S, Hkv, self.ldh, D), rnd(self.S, Hkv, self.ldh, D)
        self._ref = {}

    def prefix_of(self, s):
        gi = s // self.n_str
        return gi if self.gmap is None else self.gmap[gi]

    def tok(self, gi, b, t):
        return (gi * self.n_str + b) * self.T + t

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------ reference

def reference(c, mutant=None):
    """(ref, A) in fp64, [n_tok, H, D] each.  Mask mutants: limit+1 / limit-1 (the prefix
    length and the history limit hb + t), window+1 / window-1 (the first visible position),
    neighbour (the history of the streams next to it in the group visible too), future
    (every history slot up to ld_hist visible)."""
    if mutant in c._ref:
        return c._ref[mutant]
    assert mutant is None or mutant in REF_MUTANTS, mutant
    dl = {"limit+1": 1, "limit-1": -1}.get(mutant, 0)
    dk = {"window+1": 1, "window-1": -1}.get(mutant, 0)
    q, kf, vf, kh, vh = (_f64(x) for x in (c.q, c.kflat, c.vflat, c.kh, c.vh))
    ref = np.zeros((c.S * c.T, c.H, c.D))
    A = np.zeros_like(ref)
    for s in range(c.S):
        p = c.prefix_of(s)
        P, o = c.plens[p], c.off[p]
        Pv = max(0, min(P + dl, c.Lp - o))
        for t in range(c.T):
            nh = c.ldh if mutant == "future" else max(0, min(c.hb + t + 1 + dl, c.ldh))
            ks, vs = [kf[:, o:o + Pv], kh[s, :, :nh]], [vf[:, o:o + Pv], vh[s, :, :nh]]
            pos = [np.arange(Pv), P + np.arange(nh)]
            if mutant == "neighbour":
                b = s % c.n_str
                for b2 in sorted({(b + 1) % c.n_str, (b - 1) % c.n_str} - {b}):
                    s2 = s - b + b2
                    ks.append(kh[s2, :, :nh])
                    vs.append(vh[s2, :, :nh])
                    pos.append(P + np.arange(nh))
            K, V, pos = np.concatenate(ks, 1), np.concatenate(vs, 1), np.concatenate(pos)
            qq = q[s * c.T + t].reshape(c.Hkv, c.rep, c.D)
            sc = np.einsum("grd,gnd->grn", qq, K) * c.scale
            if c.cap > 0:
                sc = c.cap * np.tanh(sc / c.cap)
            if c.window > 0:
                kmin = P + c.hb + t - c.window + 1 + dk
                sc = np.where((pos >= kmin)[None, None], sc, -np.inf)
            sc = sc - sc.max(-1, keepdims=True)
            pr = np.exp(sc)
            pr /= pr.sum(-1, keepdims=True)
            ref[s * c.T + t] = np.einsum("grn,gnd->grd", pr, V).reshape(c.H, c.D)
            A[s * c.T + t] = np.einsum("grn,gnd->grd", pr, np.abs(V)).reshape(c.H, c.D)
    c._ref[mutant] = (ref, A)
    return ref, A


def err_over_bound(out, ref, A):
    """max |out - ref| / bound per (tok, head) row; out: bf16 tensor or fp array."""
    o = _f64(out.cpu()) if isinstance(out, torch.Tensor) else np.asarray(out, dtype=np.float64)
    return (np.abs(o - ref) / bound_of(A)).max(-1)


# --------------------------------------------------------------------- the planner, restated

def plan_cells(c):
    """cs_prefix_attention_plan restated for the case's host bounds: ({(gi, qg): splits},
    n_attn, n_merge), or None when the planner asks for the plain grid."""
    M = c.n_str * c.T * c.rep
    n_qg = -(-M // GROUP_ROWS)
    base = c.n_grp * c.Hkv * n_qg
    if base >= PLAN_MIN_BASE:
        return None                     # not restated: the cases here are small
    nbh_max = c.ldh // 32
    cells = []
    for gi in range(c.n_grp):
        p = gi if c.gmap is None else c.gmap[gi]
        nbp = -(-c.host_lens[p] // 32)
        for qg in range(n_qg):
            r0 = qg * GROUP_ROWS
            nrows = min(GROUP_ROWS, M - r0)
            n_qt = -(-nrows // 16)
            kw = 4 if n_qt == 1 else (2 if n_qt == 2 else 1)
            items = 0
            for qt in range(n_qt):
                rt0 = r0 + 16 * qt
                rt1 = min(rt0 + 15, M - 1)
                streams = (rt1 // c.rep) // c.T - (rt0 // c.rep) // c.T + 1
                items = max(items, nbp + streams * nbh_max)
            cells.append((gi, qg, items, kw, nrows))
    work = sum(-(-it // kw) for _, _, it, kw, _ in cells) * c.Hkv
    qb = max(PLAN_MIN_ITEMS, -(-work // PLAN_TARGET))
    out, na, nm = {}, 0, 0
    for gi, qg, items, kw, nrows in cells:
        s = max(1, min(MAX_SPLIT, -(-items // (qb * kw))))
        out[(gi, qg)] = s
        na += s * c.Hkv
        if s > 1:
            nm += -(-nrows // MERGE_ROWS) * c.Hkv
    return (out, na, nm) if nm else None


# ------------------------------------------------------------------ the kernel, restated

def _attend(c, qt_rows, Kb, Vb, vis, st, mutant):
    """attend_block for one 16-column wave: scores in log2 units, mask, the wave-wide lazy
    rescale ballot, p = 2^(y - m) rounded to bf16 for the P.V product (l sums the fp32 p)."""
    m, l, o = st
    f32 = np.float32
    s = (qt_rows @ Kb.T).astype(f32)
    if c.cap > 0:
        x = s * f32(c.scale)
        y = (f32(c.cap) * np.tanh(x / f32(c.cap))).astype(f32) * f32(LOG2E)
    else:
        y = s * f32(f32(c.scale) * f32(LOG2E))
    y = np.where(vis, y, -np.inf).astype(f32)
    bm = y.max(1)
    mn = m
    with np.errstate(invalid="ignore"):
        if np.any(bm > m + f32(LAZY)):
            mn = np.maximum(m, bm)
            alpha = np.where(mn == -np.inf, f32(1), np.exp2(m - mn)).astype(f32)
            if mutant != "norescale":
                l = l * alpha
            if mutant not in ("norescale", "rescale_l_only"):
                o = o * alpha[:, None]
        p = np.where((mn == -np.inf)[:, None], f32(0), np.exp2(y - mn[:, None])).astype(f32)
    l = l + p.sum(1, dtype=f32)
    o = o + (_bf16_round(p) @ Vb).astype(f32)
    return mn, l, o


def _fold(parts, mutant):
    """the wave combine / split merge: weights 2^(m_k - max m), 0 for an empty partial"""
    f32 = np.float32
    mt = np.max([p[0] for p in parts], axis=0)
    l = np.zeros_like(parts[0][1])
    o = np.zeros_like(parts[0][2])
    for m, lk, ok in parts:
        with np.errstate(invalid="ignore"):
            w = np.where(mt == -np.inf, f32(0), np.exp2(m - mt)).astype(f32)
        if mutant == "combine1":
            w = np.ones_like(w)
        l = l + lk * w
        o = o + ok * w[:, None]
    return mt, l, o


def emulate(c, order, mutant=None):
    """The kernels' arithmetic in fp32 NumPy.  order "lds": prefix_attn_lds_kernel (no plan,
    one block list per workgroup); "plan": prefix_attn_plan_lds_kernel with the splits of
    plan_cells (both history layouts: they differ only in where the keys come from);
    "plan1": that kernel unsplit (the row-layout history without a plan).  Returns out as
    fp32 [n_tok, H, D] holding bf16 values."""
    assert mutant is None or mutant in EMU_MUTANTS
    f32 = np.float32
    q, kf, vf, kh, vh = (x.float().numpy() for x in (c.q, c.kflat, c.vflat, c.kh, c.vh))
    M = c.n_str * c.T * c.rep
    n_qg = -(-M // GROUP_ROWS)
    splits = plan_cells(c)[0] if order == "plan" else None
    out = np.zeros((c.S * c.T, c.H, c.D), f32)
    for gi in range(c.n_grp):
        p = gi if c.gmap is None else c.gmap[gi]
        pl, po = c.plens[p], c.off[p]
        nbp = -(-pl // 32)
        for g in range(c.Hkv):
            for qg in range(n_qg):
                r0 = qg * GROUP_ROWS
                nrows = min(GROUP_ROWS, M - r0)
                n_qt = -(-nrows // 16)
                kw = 4 if n_qt == 1 else (2 if n_qt == 2 else 1)
                n_used = splits[(gi, qg)] if splits else 1
                rw1 = r0 + nrows - 1
                for qt in range(n_qt):
                    rows = r0 + qt * 16 + np.arange(16)
                    ok = rows < M
                    rr = np.minimum(rows, M - 1)
                    jh, bt = rr % c.rep, rr // c.rep
                    t, b = bt % c.T, bt // c.T
                    tok = (gi * c.n_str + b) * c.T + t
                    head = g * c.rep + jh
                    Q = np.where(ok[:, None], q[tok, head], f32(0)).astype(f32)
                    hv = np.minimum(c.hb + t + 1, c.ldh)
                    kmin = pl + c.hb + t - c.window + 1 if c.window > 0 else np.full(16, -2 ** 31)
                    if order == "lds":           # the workgroup's streams
                        lo, hi = r0, rw1
                    else:                        # the tile's streams
                        lo, hi = r0 + qt * 16, min(r0 + qt * 16 + 15, M - 1)
                    b_lo, b_hi = (lo // c.rep) // c.T, (hi // c.rep) // c.T
                    t_hi = (hi // c.rep) % c.T if b_lo == b_hi else c.T - 1
                    nbh = -(-min(c.hb + t_hi + 1, c.ldh) // 32)
                    n_hist = (b_hi - b_lo + 1) * nbh

                    def block(it):
                        if it < nbp:
                            kb = it * 32
                            keys = kb + np.arange(32)
                            a0 = po + kb
                            vis = ok[:, None] & (keys[None] < pl) & (keys[None] >= kmin[:, None])
                            return kf[g, a0:a0 + 32], vf[g, a0:a0 + 32], vis
                        ih = it - nbp
                        bb, kb = b_lo + ih // nbh, (ih % nbh) * 32
                        keys = kb + np.arange(32)
                        sg = gi * c.n_str + bb
                        vis = (ok & (b == bb))[:, None] & (keys[None] < hv[:, None]) & \
                            (pl + keys[None] >= kmin[:, None])
                        return kh[sg, g, kb:kb + 32], vh[sg, g, kb:kb + 32], vis

                    parts = []
                    for sp in range(n_used):
                        waves = []
                        for ks in range(kw):
                            if order == "lds":
                                its = [it for it in range(nbp + n_hist) if it % kw == ks]
                            else:
                                npi = -(-(nbp - sp) // n_used) if nbp > sp else 0
                                its = [sp + j * n_used for j in range(npi) if j % kw == ks]
                                its += [nbp + ih for ih in range(sp * kw + ks, n_hist, n_used * kw)]
                            st = (np.full(16, -np.inf, f32), np.zeros(16, f32), np.zeros((16, c.D), f32))
                            for it in its:
                                st = _attend(c, Q, *block(it), st, mutant)
                            waves.append(st)
                        parts.append(_fold(waves, mutant) if kw > 1 else waves[0])
                    m, l, o = _fold(parts, mutant) if n_used > 1 else parts[0]
                    with np.errstate(divide="ignore"):
                        inv = np.where(l > 0, f32(1) / l, f32(0)).astype(f32)
                    res = _bf16_round(o * inv[:, None])
                    out[tok[ok], head[ok]] = res[ok]
    return out


# -------------------------------------------------------------------------------- builders

def plant(c, where, g, slot, target, aligned=(), nats=None, v_seed=0):
    """Plant a key in K/V head g: where = ("prefix", p) or ("hist", s); slot the key slot
    (a prefix padding row or a history slot past the visible range is allowed: that is the
    point).  target = (tok, jh) gives the direction; the rows in ``aligned`` get the target's
    q; every other row that reads this K row is made orthogonal to it (controls)."""
    tok0, jh0 = target
    h0 = g * c.rep + jh0
    nats = (45.0 if c.cap > 0 else 40.0) if nats is None else nats
    qd = c.q[tok0, h0].double()
    n2 = float(qd @ qd)
    krow = (nats / (c.scale * n2) * qd).to(BF)
    gv = torch.Generator().manual_seed(1000 + v_seed)
    vrow = (8.0 + 4.0 * torch.randn(c.D, generator=gv)).to(BF)
    if where[0] == "prefix":
        p = where[1]
        readers = [s for s in range(c.S) if c.prefix_of(s) == p]
        c.kflat[g, c.off[p] + slot] = krow
        c.vflat[g, c.off[p] + slot] = vrow
    else:
        readers = [where[1]]
        c.kh[where[1], g, slot] = krow
        c.vh[where[1], g, slot] = vrow
    keep = {(tok0, h0)} | {(tk, g * c.rep + jh) for tk, jh in aligned}
    for tk, h in keep:
        c.q[tk, h] = c.q[tok0, h0]
    for s in readers:
        for t in range(c.T):
            for jh in range(c.rep):
                tk, h = s * c.T + t, g * c.rep + jh
                if (tk, h) in keep:
                    continue
                x = c.q[tk, h].double()
                c.q[tk, h] = (x - (x @ qd) / n2 * qd).to(BF)
    c._ref.clear()
    return vrow


HOT = (32, 8, 2, 1)
HOT_BOOST = 3.0       # log2 units
BETAS = (1.0, 0.5, -1.0)


def staircase(c, levels_prefix, levels_hist, qnorm=4.0):
    """Staircase in every K/V head and group.  All query rows lie along one direction qhat:
    row r of a cell (r = (b T + t) rep + jh) has q = BETAS[r % 3] * qnorm * qhat plus a little
    noise, so inside one 16-row tile one column climbs the stairs, its neighbour climbs half
    as fast and the next one descends: the wave-wide rescale ballot fires for all of them.
    Every key of block j of a prefix (levels_prefix[j]) and of every stream's history
    (levels_hist[j]) scores beta * level log2 units above block 0's background, so a
    beta = -1 row climbs a descending staircase; HOT[j] keys of the block (fewer with j, 1
    from j = 3 on) score beta * HOT_BOOST more and carry most of the block's weight for a
    beta = 1 row, so earlier blocks keep a few per cent of its output.  The block's V rows
    have mean (-1)^j (1 + j / 2)."""
    g = c.gen
    D = c.D
    qhat = torch.randn(D, generator=g).double()
    qhat /= qhat.norm()
    M = c.n_str * c.T * c.rep
    for gi in range(c.n_grp):
        for r in range(M):
            jh, bt = r % c.rep, r // c.rep
            t, b = bt % c.T, bt // c.T
            for gg in range(c.Hkv):
                noise = 0.05 * torch.randn(D, generator=g).double()
                c.q[c.tok(gi, b, t), gg * c.rep + jh] = (BETAS[r % 3] * qnorm * qhat + noise).to(BF)

    def fill(K, V, j, level, nvis):
        """K, V: [Hkv, 32, D] views of block j (nvis visible keys)"""
        n_hot = min(HOT[min(j, len(HOT) - 1)], nvis)
        hot = sorted({(5 * i + 3) % nvis for i in range(n_hot)}) if n_hot < nvis else list(range(nvis))
        # level log2 units = level ln2 nats = scale * qnorm * kappa
        unit = math.log(2.0) / (c.scale * qnorm)
        for k in range(nvis):
            K[:, k] = (K[:, k].double() + (level + (HOT_BOOST if k in hot else 0.0)) * unit * qhat).to(BF)
        mean = (-1.0) ** j * (1.0 + 0.5 * j)
        V[:, :nvis] = (mean + 0.25 * torch.randn(c.Hkv, nvis, D, generator=g)).to(BF)

    nbp_all = []
    for p, pl in enumerate(c.plens):
        nbp = -(-pl // 32)
        nbp_all.append(nbp)
        for j in range(nbp):
            a = c.off[p] + 32 * j
            fill(c.kflat[:, a:a + 32], c.vflat[:, a:a + 32], j, levels_prefix[j], min(32, pl - 32 * j))
    n_vis = c.hb + c.T
    for s in range(c.S):
        nbp = nbp_all[c.prefix_of(s)]
        for j in range(-(-n_vis // 32)):
            fill(c.kh[s, :, 32 * j:32 * j + 32], c.vh[s, :, 32 * j:32 * j + 32], nbp + j,
                 levels_hist[j], min(32, n_vis - 32 * j))
    c._ref.clear()


# ------------------------------------------------------------- device tensors for the routes

def rows_layout(c, extra_rows=2):
    """The row-layout history behind a slot table that describes c.kh / c.vh: inherited
    slots j < hb live in OTHER rows (a random injective map per slot into S + extra_rows
    buffer rows), the step's own slots j >= hb in the stream's own row.  Returns (k, v
    [R, Hkv, ldh, D], table [S, ldh] int32, named [R, ldh] bool: buffer slots that a table
    entry of a visible slot (j < hb + T) names); unnamed slots hold random finite values."""
    g = torch.Generator().manual_seed(zlib.crc32((c.name + "/rows").encode()))
    R = c.S + extra_rows
    k = (torch.randn(R, c.Hkv, c.ldh, c.D, generator=g) * 0.5).to(BF)
    v = (torch.randn(R, c.Hkv, c.ldh, c.D, generator=g) * 0.5).to(BF)
    table = torch.arange(c.S, dtype=torch.int32)[:, None].repeat(1, c.ldh)
    named = torch.zeros(R, c.ldh, dtype=torch.bool)
    for j in range(c.ldh):
        if j < c.hb:
            table[:, j] = torch.randperm(R, generator=g)[:c.S].to(torch.int32)
        idx = table[:, j].long()
        k[idx, :, j] = c.kh[:, :, j]
        v[idx, :, j] = c.vh[:, :, j]
        if j < c.hb + c.T:
            named[idx, j] = True
    return k, v, table, named


def fill_invisible(c, layout, value):
    """Copies of the K / V buffers with every slot that no query may see set to +-value
    (random signs; 0 gives zeros): prefix padding rows, history slots >= hb + T, and the
    row-layout buffer slots no visible table entry names.  Returns (kflat, vflat, kh, vh,
    k_rows, v_rows)."""
    g = torch.Generator().manual_seed(77)

    def junk(shape):
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        return (sign * value).to(BF) if value else torch.zeros(shape, dtype=BF)

    kf, vf, kh, vh = c.kflat.clone(), c.vflat.clone(), c.kh.clone(), c.vh.clone()
    pad = torch.ones(c.Lp, dtype=torch.bool)
    for p, pl in enumerate(c.plens):
        pad[c.off[p]:c.off[p] + pl] = False
    n = int(pad.sum())
    kf[:, pad] = junk((c.Hkv, n, c.D))
    vf[:, pad] = junk((c.Hkv, n, c.D))
    nv = c.hb + c.T
    kh[:, :, nv:] = junk(tuple(kh[:, :, nv:].shape))
    vh[:, :, nv:] = junk(tuple(vh[:, :, nv:].shape))
    kr, vr, _, named = layout
    kr, vr = kr.clone().transpose(1, 2), vr.clone().transpose(1, 2)      # [R, ldh, Hkv, D]
    n = int((~named).sum())
    kr[~named] = junk((n, c.Hkv, c.D))
    vr[~named] = junk((n, c.Hkv, c.D))
    return kf, vf, kh, vh, kr.transpose(1, 2).contiguous(), vr.transpose(1, 2).contiguous()


# ----------------------------------------------------------------------------------- cases

def _shape(i, inflate):
    """(rep, n_str) of case i: exact host lengths need 64 query rows per cell (one wave per
    tile) to split at a handful of key blocks; inflated host bounds split any cell."""
    if inflate:
        return [(1, 3), (4, 3), (8, 2), (4, 5)][(i // 2) % 4]
    return [(4, 16), (1, 16), (4, 16), (1, 64)][(i // 2) % 4]


def _dcap(i):
    return [(64, 0.0), (128, 0.0), (256, 50.0), (128, 50.0), (256, 0.0), (64, 50.0)][i % 6]


def prefix_limit_cases():
    """a. the planted key at pl - 1 (K/V head 0: visible) and at pl, the first padding row
    (K/V head 1: invisible), pl on the lane-group (4), half-block (16) and block (32) edges;
    a second, longer prefix beside it, the tested one first or (mapped) second."""
    out = []
    for i, pl in enumerate([1, 3, 4, 5, 15, 16, 17, 20, 31, 32, 33, 63, 64, 65]):
        D, cap = _dcap(i)
        inflate = i % 2 == 1
        rep, n_str = _shape(i, inflate)
        swap = i % 3 == 1
        plens, gmap, p = ([97, pl], [1, 0], 1) if swap else ([pl, 97], None, 0)
        c = Case(f"a-pl{pl}-D{D}-cap{int(cap)}-rep{rep}", "a", D, rep, n_str, 1, plens, gmap, 3, cap, 0,
                 [2000, 2000] if inflate else None)
        gi = 0                                     # the group that reads prefix p
        b = n_str - 1
        tk = c.tok(gi, b, 0)
        plant(c, ("prefix", p), 0, pl - 1, (tk, rep - 1), v_seed=1)
        c.checks.append(("limit-1", tk, rep - 1))
        if pl % 32:
            plant(c, ("prefix", p), 1, pl, (tk, 0), v_seed=2)
            c.checks.append(("limit+1", tk, rep))
        out.append(c)
    # an empty prefix beside a full one: no prefix block at all, a key planted in its padding
    for D, cap, rep, n_str, inflate in ((64, 0.0, 4, 16, False), (256, 50.0, 4, 3, True)):
        c = Case(f"a-pl0-D{D}-cap{int(cap)}-rep{rep}", "a", D, rep, n_str, 1, [0, 97], None, 3, cap, 0,
                 [2000, 2000] if inflate else None)
        tk = c.tok(0, n_str - 1, 0)
        plant(c, ("prefix", 0), 1, 0, (tk, 0), v_seed=2)
        c.checks.append(("limit+1", tk, rep))
        out.append(c)
    return out


def history_limit_cases():
    """b. hb + t across the block edges, planted keys in the history.
    T = 1: the token's own key (slot hb, K/V head 0: visible) and the same slot of a neighbour
    stream in the same 16-row tile (head 1: invisible).
    T = 3, "next": slot hb + 1 (head 0), token 1's own key: visible to token 1, not to token
    0; slot hb + 2 (head 1): visible to token 2, not to token 1.
    T = 3, "nbr": token 0's own key (head 0: visible); a neighbour stream's slot hb + 1
    (head 1): invisible to token 1.
    T = 1, "future": a history one block longer than ceil32(hb + T), so that slot hb + 1
    exists at every hb: a key planted there (head 0) is invisible; the own key (head 1)."""
    out = []
    i = 0
    for T, kind in ((1, "own"), (3, "next"), (3, "nbr"), (1, "future")):
        for hb in (0, 1, 30, 31, 32, 33, 62, 63):
            if kind == "future" and hb not in (30, 31, 63):
                continue
            D, cap = _dcap(i)
            inflate = i % 2 == 0
            if T == 1:
                rep, n_str = _shape(i, inflate)
            else:                                   # rep * T < 16: a tile spans streams
                rep, n_str = ((4, 3), (1, 5), (4, 2))[i % 3] if inflate else ((4, 6), (1, 22), (4, 11))[i % 3]
            c = Case(f"b-{kind}-hb{hb}-T{T}-D{D}-cap{int(cap)}-rep{rep}", "b", D, rep, n_str, T, [40, 33],
                     None, hb, cap, 0, [1500, 1500] if inflate else None,
                     ldh=ceil32(hb + T) + 32 if kind == "future" else None)
            gi, b = 1, 1
            s = gi * n_str + b
            nb = gi * n_str + (0 if i % 2 else 2 % n_str)     # a neighbour stream
            t0, t1, t2 = (c.tok(gi, b, t) for t in (0, 1, 2))
            if kind == "own":
                plant(c, ("hist", s), 0, hb, (t0, 0), v_seed=3)
                c.checks.append(("limit-1", t0, 0))
                plant(c, ("hist", nb), 1, hb, (t0, rep - 1), v_seed=4)
                c.checks.append(("neighbour", t0, 2 * rep - 1))
            elif kind == "next":
                plant(c, ("hist", s), 0, hb + 1, (t0, 0), aligned=[(t1, 0)], v_seed=3)
                c.checks += [("limit+1", t0, 0), ("future", t0, 0), ("limit-1", t1, 0)]
                plant(c, ("hist", s), 1, hb + 2, (t1, rep - 1), aligned=[(t2, rep - 1)], v_seed=4)
                c.checks += [("limit+1", t1, 2 * rep - 1), ("limit-1", t2, 2 * rep - 1)]
            elif kind == "nbr":
                plant(c, ("hist", s), 0, hb, (t0, 0), v_seed=3)
                c.checks.append(("limit-1", t0, 0))
                plant(c, ("hist", nb), 1, hb + 1, (t1, rep - 1), v_seed=4)
                c.checks.append(("neighbour", t1, 2 * rep - 1))
            else:
                plant(c, ("hist", s), 0, hb + 1, (t0, 0), v_seed=3)
                c.checks += [("limit+1", t0, 0), ("future", t0, 0)]
                plant(c, ("hist", s), 1, hb, (t0, rep - 1), v_seed=4)
                c.checks.append(("limit-1", t0, 2 * rep - 1))
            out.append(c)
            i += 1
    # scoring chunks: one stream's tokens fill whole tiles and walk over the block edges, so
    # the tiles of a cell attend different numbers of history blocks.  Slot e (a block's
    # first key, head 0) and slot e - 1 (its neighbour block's last, head 1) are the own keys
    # of tokens e - hb and e - hb - 1: visible to them, invisible to the token before
    for hb, T, rep, n_str, inflate, e, D, cap in ((30, 40, 1, 2, False, 64, 128, 0.0),
                                                   (0, 33, 4, 1, True, 32, 64, 0.0),
                                                   (5, 30, 4, 1, False, 32, 256, 50.0)):
        c = Case(f"b-chunk-hb{hb}-T{T}-D{D}-cap{int(cap)}-rep{rep}", "b", D, rep, n_str, T, [40, 33], None,
                 hb, cap, 0, [700, 700] if inflate else None)
        s = 1 * n_str + n_str - 1
        for g, slot in ((0, e), (1, e - 1)):
            ta, tb = c.tok(1, n_str - 1, slot - hb - 1), c.tok(1, n_str - 1, slot - hb)
            plant(c, ("hist", s), g, slot, (ta, 0), aligned=[(tb, 0)], v_seed=3 + g)
            c.checks += [("limit+1", ta, g * rep), ("limit-1", tb, g * rep)]
        out.append(c)
    return out


def window_cases():
    """c. the first visible position kmin = P + hb + t - window + 1: a planted key at kmin
    (K/V head 0: visible) and at kmin - 1 (head 1: invisible), kmin inside the prefix, on a
    32-key block edge of it, at the prefix / history seam (kmin = P, P - 1) and inside the
    history; the last two shapes hide every prefix block of some splits and some waves'
    stripes (empty partials meet finite ones in the combine and the merge)."""
    out = []
    P, hb = 75, 37
    specs = [("in-prefix", P, hb, 21, False, None), ("block-edge", P, hb, 32, True, None),
             ("block-edge64", P, hb, 64, False, None), ("seam", P, hb, P, True, None),
             ("seam-1", P, hb, P - 1, False, None), ("in-history", P, hb, P + 9, True, None),
             ("history-block-edge", P, hb, P + 32, False, None),
             ("hidden-splits", 200, 5, 197, False, (4, 16)),      # 64 rows: kw = 1, exact splits
             ("hidden-stripes", 420, 5, 410, False, (4, 3))]      # 12 rows: kw = 4
    for i, (name, P, hb, kmin, inflate, shape) in enumerate(specs):
        D, cap = _dcap(i + 1)
        rep, n_str = shape or _shape(i, inflate)
        c = Case(f"c-{name}-D{D}-cap{int(cap)}-rep{rep}", "c", D, rep, n_str, 1, [P, 50], None, hb, cap,
                 P + hb - kmin + 1, [1800, 1800] if inflate else None)
        gi, b = 0, n_str // 2
        tk = c.tok(gi, b, 0)
        for g, pos, mut in ((0, kmin, "window+1"), (1, kmin - 1, "window-1")):
            where, slot = (("prefix", 0), pos) if pos < P else (("hist", gi * n_str + b), pos - P)
            plant(c, where, g, slot, (tk, 0), v_seed=5 + g)
            c.checks.append((mut, tk, g * rep))
        out.append(c)
    return out


def window_identity_cases():
    """c. shapes for the two exact identities (window = 1; window >= every position)."""
    out = []
    for i, (T, hb) in enumerate([(1, 0), (3, 30), (1, 63)]):
        D, cap = _dcap(i)
        inflate = i % 2 == 1
        rep, n_str = ((4, 2) if inflate else (4, 6)) if T == 3 else _shape(i, inflate)
        out.append(Case(f"c-identity-T{T}-hb{hb}-D{D}-cap{int(cap)}", "c", D, rep, n_str, T, [70, 33],
                        None, hb, cap, 0, [1500, 1500] if inflate else None, sigma=1.0))
    return out


def staircase_cases():
    """d. stairs of 6, 7.5, 8.5, 12 and 30 log2 units per key block (both sides of the lazy
    rescale threshold), ascending and descending, through the prefix and on into the
    history; D = 64 and 128 uncapped, D = 256 capped; and two split-plan variants whose one
    dominant block (180 log2 units) falls in split 0 / in the last split."""
    out = []
    i = 0
    for step in (6.0, 7.5, 8.5, 12.0, 30.0):
        for desc in (False, True):
            # (the cap flattens stairs of 30: D = 256 takes the steps up to 12)
            D, cap = [(128, 0.0), (256, 50.0), (64, 0.0)][i % 3]
            inflate = i % 2 == 1
            rep, n_str = ((4, 3), (8, 2), (1, 7))[i % 3] if inflate else ((4, 16), (8, 8), (4, 16))[i % 3]
            hb = 40
            # inflated bounds: 2 splits x 4 waves over 10 + 2 blocks, so that a wave still meets
            # more than one stair (a wave with one block never rescales)
            c = Case(f"d-step{step}-{'desc' if desc else 'asc'}-D{D}-cap{int(cap)}-rep{rep}", "d", D, rep,
                     n_str, 1, [300, 70] if inflate else [100, 70], None, hb, cap, 0,
                     [600, 600] if inflate else None)
            nbp = -(-c.plens[0] // 32)
            lv = [step * j for j in range(nbp + 2)]   # the prefix blocks, then 2 history blocks
            if desc:
                lv = lv[::-1]
            staircase(c, lv[:nbp], lv[nbp:])
            _stair_checks(c, desc)
            out.append(c)
            i += 1
    for last in (False, True):
        for D, cap, rep, n_str, inflate in ((64, 0.0, 4, 16, False), (128, 0.0, 4, 3, True)):
            c = Case(f"d-dominant-{'last' if last else 'first'}-split-D{D}-rep{rep}", "d", D, rep, n_str, 1,
                     [100, 100], None, 8, cap, 0, [600, 600] if inflate else None)
            n_used = plan_cells(c)[0][(0, 0)]
            assert 2 <= n_used <= 4            # prefix block i belongs to split i % n_used
            lv = [0.0] * 4
            lv[n_used - 1 if last else 0] = 180.0
            staircase(c, lv, [0.0])
            tk = c.tok(0, 0, 0)
            c.checks.append(("combine1", tk, 0, ("plan",)))
            out.append(c)
    return out


def _stair_checks(c, desc):
    """the beta = +1 rows climb an ascending staircase, the beta = -1 rows a descending one"""
    want = 2 if desc else 0
    M = c.n_str * c.T * c.rep
    r = next(r for r in range(16, M) if r % 3 == want) if M > 16 else want
    jh, bt = r % c.rep, r // c.rep
    tk = c.tok(0, bt // c.T, bt % c.T)
    for mut in EMU_MUTANTS:
        orders = ("lds", "plan", "plan1")
        if mut == "combine1":       # only where partials are combined
            orders = ("plan",) + (("lds", "plan1") if M <= 32 else ())
        c.checks.append((mut, tk, jh, orders))
    if desc:                        # a beta = +1 row: its max is set by the first block it meets
        r = next(r for r in range(M) if r % 3 == 0 and r >= min(16, M - 3))
        jh, bt = r % c.rep, r // c.rep
        c.checks.append(("combine1", c.tok(0, bt // c.T, bt % c.T), jh, ("plan",)))


def inert_cases():
    """e. one shape per D (all four routes run on each): planted keys in visible slots, so
    the answers are not averages, T = 3 and a history that ends inside a block."""
    out = []
    for i, (D, cap) in enumerate([(64, 0.0), (128, 0.0), (256, 50.0)]):
        inflate = i == 1
        rep, n_str = (4, 2) if inflate else (4, 6)
        c = Case(f"e-inert-D{D}-cap{int(cap)}", "e", D, rep, n_str, 3, [45, 70], None, 35, cap, 0,
                 [900, 900] if inflate else None)
        tk = c.tok(1, 1, 2)
        plant(c, ("prefix", 1), 0, 69, (tk, 0), v_seed=8)
        plant(c, ("hist", n_str + 1), 1, 37, (tk, 0), v_seed=9)
        out.append(c)
    return out


def offset_cases():
    """f. background scores around -200 and +200 nats, uncapped: every key of every K/V head
    carries -+200 / (scale |q|) along the one direction all query rows share."""
    out = []
    i = 0
    for nats in (-200.0, 200.0):
        for D in (64, 128, 256):
            inflate = i % 2 == 0
            rep, n_str = _shape(i, inflate)
            c = Case(f"f-offset{int(nats)}-D{D}-rep{rep}", "f", D, rep, n_str, 1, [70, 33], None, 34, 0.0, 0,
                     [1000, 1000] if inflate else None)
            g = c.gen
            qhat = torch.randn(D, generator=g).double()
            qhat /= qhat.norm()
            qn = 4.0
            c.q[:] = (qn * qhat + 0.3 * torch.randn(c.q.shape, generator=g).double()).to(BF)
            kap = nats / (c.scale * qn)
            c.kflat[:] = (c.kflat.double() * 2 + kap * qhat).to(BF)
            c.kh[:] = (c.kh.double() * 2 + kap * qhat).to(BF)
            out.append(c)
            i += 1
    return out


_CASES = {}


def cases(family):
    """The cases of one family, built once per process and shared (read-only) by the tests."""
    if family not in _CASES:
        _CASES[family] = {"a": prefix_limit_cases, "b": history_limit_cases, "c": window_cases,
                          "ci": window_identity_cases, "d": staircase_cases, "e": inert_cases,
                          "f": offset_cases}[family]()
    return _CASES[family]
