"""Cases for the wide attention tile (prefix_attn_wide_kernel, csrc/attn.hip: 32 query rows per
wave over 64-key blocks), built from tests/attention_ref.py's pieces and shared by
tests/test_attention_wide_gpu.py (runs them) and tests/test_attention_wide_cases_host.py
(proves on the CPU that each would catch the mask mutants it is aimed at).

Every shape is one the launch rule sends to the wide tile -- D = 128, no soft-cap, no window,
32 % rep == 0, T >= 32, no plan -- except the T = 31 half of ``rule_pair``.  Hkv = 2: one
planted key per K/V head (a second plant in a head would re-orthogonalise the first one's rows).

Families:
  prefix     prefix lengths on both sides of the 32- and 64-key edges (and 0, 1, 200): a key
             at pl - 1 (head 0, visible) and at pl, the first padding row (head 1, invisible);
             two groups, the tested prefix stored last and read through a group map
  missing    plens [200, 70], T = 70, hb = 0: the last prefix is padded to 96 keys and ld_hist
             is 96, so the second 32-key tile of the last 64-key block exists for neither
  history    T = 70 / hb = 0 and T = 40 / hb = 30: slot e in {32, 64} is the own key of token
             e - hb (visible to it, not to token e - hb - 1, in head 0); slot e - 1 of the
             NEIGHBOUR stream is invisible to token e - hb (head 1).  Both tokens lie in one
             32-row tile (asserted: T = 70 streams start 24 rows into a tile)
  span       n_str = 3 and T rep not a multiple of 32: a tile carries the end of one stream
             and the start of the next (rep 4 / T 33, rep 8 / T 34, rep 2 / T 35)
  stairs     R.staircase with steps of 6, 8.5, 12 and 30 log2 units per 64 keys, up and down,
             through the prefix and on into the history
  offset     background scores around -200 / +200 nats
  rule_pair  T = 31 (the narrow tile) and T = 32 (the wide one) over the same first 31 tokens"""
import attention_ref as R

D = 128
PREFIX_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 200)
STAIR_STEPS = (6.0, 8.5, 12.0, 30.0)


def _case(name, family, rep, n_str, T, plens, gmap, hb, **kw):
    return R.Case(name, family, D, rep, n_str, T, plens, gmap, hb, 0.0, 0, None, **kw)


def prefix_cases():
    out = []
    for pl in PREFIX_LENS:
        rep, n_str, T = 4, 2, 32
        c = _case(f"w-prefix-pl{pl}", "prefix", rep, n_str, T, [97, pl], [1, 0], 3)
        tk = c.tok(0, n_str - 1, 17)            # group 0 reads prefix 1, the tested one
        if pl > 0:
            plant(c, ("prefix", 1), 0, pl - 1, (tk, rep - 1), 1)
            c.checks.append(("limit-1", tk, rep - 1))
        if pl % 32 or pl == 0:                  # a padding row exists
            plant(c, ("prefix", 1), 1, pl, (tk, 0), 2)
            c.checks.append(("limit+1", tk, rep))
        out.append(c)
    return out


def plant(c, where, g, slot, target, seed, aligned=()):
    return R.plant(c, where, g, slot, target, aligned=aligned, v_seed=seed)


def missing_tile_case():
    rep, n_str, T = 4, 2, 70
    c = _case("w-missing-second-tile", "missing", rep, n_str, T, [200, 70], None, 0)
    assert c.Lp == 224 + 96 and c.ldh == 96
    s = 1 * n_str + n_str - 1                   # the last stream: its rows end the buffers
    tk = c.tok(1, n_str - 1, T - 1)
    plant(c, ("prefix", 1), 0, 69, (tk, 0), 8)
    plant(c, ("hist", s), 1, 66, (tk, 0), 9)
    c.checks += [("limit-1", tk, 0)]
    return c


def history_cases():
    out = []
    for T, hb in ((70, 0), (40, 30)):
        for e in (32, 64):
            rep, n_str = 4, 3
            c = _case(f"w-history-T{T}-hb{hb}-slot{e}", "history", rep, n_str, T, [40, 33], None, hb)
            gi, b = 1, 1
            s, nb = gi * n_str + b, gi * n_str + 2
            ta, tb = c.tok(gi, b, e - hb - 1), c.tok(gi, b, e - hb)
            # both tokens in one 32-row tile (the stream does not start on a tile edge)
            ra, rb = ((b * T + e - hb - 1) * rep) // 32, ((b * T + e - hb) * rep) // 32
            assert ra == rb, (T, hb, e)
            plant(c, ("hist", s), 0, e, (ta, 0), 3, aligned=[(tb, 0)])
            c.checks += [("limit+1", ta, 0), ("future", ta, 0), ("limit-1", tb, 0)]
            plant(c, ("hist", nb), 1, e - 1, (tb, rep - 1), 4)
            c.checks.append(("neighbour", tb, 2 * rep - 1))
            out.append(c)
    return out


def span_cases():
    out = []
    for rep, T in ((4, 33), (8, 34), (2, 35)):
        n_str, hb = 3, 3
        c = _case(f"w-span-rep{rep}-T{T}", "span", rep, n_str, T, [40, 33], None, hb)
        assert (T * rep) % 32                   # stream 1 starts inside a tile
        gi = 0
        t0 = c.tok(gi, 1, 0)                    # stream 1's first token: shares its tile with stream 0
        plant(c, ("hist", gi * n_str + 1), 0, hb, (t0, 0), 5)
        c.checks.append(("limit-1", t0, 0))
        plant(c, ("hist", gi * n_str + 0), 1, hb, (t0, rep - 1), 6)
        c.checks.append(("neighbour", t0, 2 * rep - 1))
        out.append(c)
    return out


def stair_cases():
    out = []
    for step in STAIR_STEPS:
        for desc in (False, True):
            rep, n_str, T, hb = 4, 2, 32, 40
            c = _case(f"w-stairs-{step}-{'desc' if desc else 'asc'}", "stairs", rep, n_str, T, [200, 70],
                      None, hb)
            nbp = -(-200 // 32)                 # 7 prefix blocks of 32 keys, then 3 of history
            nbh = -(-(hb + T) // 32)
            # one stair per 64 keys: the prefix's 64-key blocks 0 .. 3, then the history's
            lv_p = [step * (j // 2) for j in range(nbp)]
            lv_h = [step * (-(-nbp // 2) + j // 2) for j in range(nbh)]
            if desc:
                top = lv_h[-1]
                lv_p, lv_h = [top - x for x in lv_p], [top - x for x in lv_h]
            R.staircase(c, lv_p, lv_h)
            out.append(c)
    return out


def offset_cases():
    import torch
    out = []
    for nats in (-200.0, 200.0):
        rep, n_str, T = 4, 2, 32
        c = _case(f"w-offset{int(nats)}", "offset", rep, n_str, T, [70, 33], None, 34)
        g = c.gen
        qhat = torch.randn(D, generator=g).double()
        qhat /= qhat.norm()
        qn = 4.0
        c.q[:] = (qn * qhat + 0.3 * torch.randn(c.q.shape, generator=g).double()).to(R.BF)
        kap = nats / (c.scale * qn)
        c.kflat[:] = (c.kflat.double() * 2 + kap * qhat).to(R.BF)
        c.kh[:] = (c.kh.double() * 2 + kap * qhat).to(R.BF)
        out.append(c)
    return out


def rule_pair():
    """(c31, c32): the same prefixes, and per stream the same first 31 tokens' q / K / V."""
    rep, n_str, hb = 4, 3, 0
    c32 = _case("w-rule-T32", "rule", rep, n_str, 32, [70, 33], None, hb)
    tk = c32.tok(1, 1, 20)
    plant(c32, ("hist", 1 * n_str + 1), 0, 20, (tk, 0), 7)
    c32.checks.append(("limit-1", tk, 0))
    c31 = _case("w-rule-T31", "rule", rep, n_str, 31, [70, 33], None, hb)
    assert c31.ldh == c32.ldh == 32
    c31.kflat, c31.vflat = c32.kflat.clone(), c32.vflat.clone()
    c31.kh, c31.vh = c32.kh.clone(), c32.vh.clone()
    c31.q = c32.q.reshape(c32.S, 32, c32.H, D)[:, :31].reshape(c31.S * 31, c31.H, D).clone()
    c31.checks.append(("limit-1", c31.tok(1, 1, 20), 0))
    return c31, c32


_BUILT = {}


def cases(family):
    """The cases of one family, built once per process and shared (read-only) by the tests."""
    if family not in _BUILT:
        _BUILT[family] = {"prefix": prefix_cases, "missing": lambda: [missing_tile_case()],
                          "history": history_cases, "span": span_cases, "stairs": stair_cases,
                          "offset": offset_cases, "rule": lambda: list(rule_pair())}[family]()
    return _BUILT[family]


FAMILIES = ("prefix", "missing", "history", "span", "stairs", "offset", "rule")
