"""CPU evidence for tests/test_rope_place_gpu.py: the reference of tests/rope_ref.py is the
documented rotation, its planted cases are exact, its rounding windows are almost always one
value, an fp32 restatement of the kernel's arithmetic with sin / cos 2 ulps off stays inside
them, and the checker rejects every wrong kernel of rope_ref.MUTANTS on a named case.

Figures measured by this file (run with -s to print them): worst |fp32 value - ref| / delta
of the restated kernel with sin / cos +-2 ulps: 0.72 over every case (the worst where cos = 1 is pushed
above 1), 0.61 on the position sweep 0 .. 131135 at D = 128; open-window share at most 0.26 % in
any random case, 0.16 % on the sweep."""
import importlib
import math
import types

import numpy as np
import pytest

import rope_ref as R

RANDOM = R.random_cases() + tuple(c for c in R.fold_cases())
ULPS = ((2, 2), (2, -2), (-2, 2), (-2, -2))


def _case(name):
    hits = [c for c in RANDOM + R.zero_cases() if c.name == name]
    assert len(hits) == 1, name
    return hits[0]


def test_case_names_are_unique_and_every_branch_is_reached():
    cases = RANDOM + R.zero_cases() + tuple(c for f in R.quarter_families() for c in f)
    assert len({c.name for c in cases}) == len(cases)
    rc = R.random_cases()
    assert {c.path() for c in rc} >= {(8, 1, False), (8, 2, False), (4, 5, False), (8, 1, True),
                                      (8, 2, True), (4, 1, True)}
    assert {c.D for c in rc if c.path()[0] == 4 and not c.col0 and not c.ldpad} == {8, 24, 40}
    assert {(c.hb, c.T, c.ldh) for c in rc if c.name.startswith("slot")} == set(R.SLOTS_TOKEN)
    assert {(c.hb, c.T, c.ldh) for c in rc if c.name.startswith("tile")} == set(R.SLOTS_TILE)
    pos = np.concatenate([c.positions() for c in rc])
    assert pos.min() == 0 and pos.max() > 1 << 17 and ((pos > 1000) & (pos < 1100)).any()
    assert {p for c in rc for p in c.plen} == {0, 17, 1000, 131071}
    gm = [c for c in rc if c.gp is not None]
    assert gm and all(c.n_groups != len(c.plen) and len(set(c.gp)) < len(c.gp)
                      and list(c.gp) != sorted(c.gp) for c in gm)
    fc = R.fold_cases()
    assert {c.splits for c in fc} == set(R.FOLD_SPLITS) == {1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17}
    assert {(c.splits, c.T, c.v_rows) for c in fc if not c.plant} == \
        {(s, T, r) for s in R.FOLD_SPLITS for T in (1, 3) for r in (False, True)}
    for fam in R.quarter_families():
        half = fam[0].half
        assert len(fam) <= math.ceil(math.log2(half)) + 1
        codes = np.stack([c.turned() for c in fam[:-1]]).astype(int)
        assert len({tuple(col) for col in codes.T}) == half      # every index told from every other
        assert fam[-1].turned().all()


def test_tables_are_the_models(pkg):
    import torch
    M = importlib.import_module(pkg.__name__ + ".model")
    for name, (_, _, D0) in R.ROPE_CFG.items():
        assert M.PRESETS[name].head_dim == D0
        for D in {D0, 8, 24, 40, 64}:
            want = M.rope_inv_freq(M.preset(name, head_dim=D), torch.device("cpu")).numpy()
            assert np.array_equal(R.table_inv_freq(name, D), want), (name, D)


def test_rne_bf16_is_exact():
    import torch
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)
    # ties and near-ties of every exponent, subnormals, the overflow threshold
    ties = ((rng.integers(0, 1 << 16, size=4096).astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000))
    bits = np.concatenate([bits, ties, ties + np.uint32(1), ties - np.uint32(1),
                           np.array([0x7F7F8000, 0x7F7F7FFF, 0x00008000, 0x00018000, 0x80000000, 0],
                                    dtype=np.uint32)])
    f = bits.view(np.float32)
    f = f[np.isfinite(f)]
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.rne_bf16(f.astype(np.float64)), want)
    # a float64 that rounding through fp32 first would get wrong: just above a bf16 tie
    x = np.float64(1.0) + 2.0 ** -8 + 2.0 ** -40
    assert R.rne_bf16(x) == 0x3F81 and R.rne_bf16(np.float64(np.float32(x))) == 0x3F80


def test_reference_is_the_direct_formula_and_the_models_convention(pkg):
    import torch
    M = importlib.import_module(pkg.__name__ + ".model")
    c = R.Case("small", 8, 2, 1, 3, 2, 32, plen=(7, 100), gp=(1, 0, 1), n_str=2, seed=77)
    e, (x, _) = R.expected(c), c.inputs()
    inv, xv = c.inv_freq(), R.bf16_value(x)
    assert c.S == 6 and list(c.positions()) == [103, 104] * 2 + [10, 11] * 2 + [103, 104] * 2
    for s in range(c.S):
        for t in range(c.T):
            pos = c.plen[c.gp[s // c.n_str]] + c.hb + t
            for h in range(c.H + c.Hkv):
                for j in range(c.half):
                    a = float(np.float32(pos) * inv[j])
                    x1, x2 = xv[s * c.T + t, h, j], xv[s * c.T + t, h, j + c.half]
                    y1 = x1 * math.cos(a) - x2 * math.sin(a)
                    y2 = x2 * math.cos(a) + x1 * math.sin(a)
                    got = e.q_ref[s * c.T + t, h] if h < c.H else e.k_ref[s, h - c.H, t]
                    assert abs(got[j] - y1) <= 1e-12 and abs(got[j + c.half] - y2) <= 1e-12
    # V: slot hb + t of the blocked layout, everything else the sentinel
    v = x[:, c.H + c.Hkv:].reshape(c.S, c.T, c.D)
    for s in range(c.S):
        for t in range(c.T):
            assert np.array_equal(e.v_full[s, 0, 0, :, c.hb + t], v[s, t])
    assert (e.v_full != R.SENT16).sum() <= c.S * c.T * c.D
    # Model._rope (the eager path's rotation: fp32 tables) follows the same convention
    ns = types.SimpleNamespace(inv_freq=torch.from_numpy(inv))
    xt = torch.from_numpy(xv[:, :c.H]).reshape(c.S, c.T, c.H, c.D).permute(0, 2, 1, 3)
    pos = torch.from_numpy(c.positions()).reshape(c.S, c.T)
    tables = M.Model._rope_tables(ns, pos, torch.float64)
    y = M.Model._rope(ns, xt, pos, tables).permute(0, 2, 1, 3).reshape(c.n_tok, c.H, c.D).numpy()
    assert (np.abs(y - e.q_ref) <= 16 * e.q_delta).all()       # fp32 sin / cos of the tables


def test_planted_cases_are_exact_in_the_reference():
    for c in R.zero_cases() + tuple(c for f in R.quarter_families() for c in f) + \
            tuple(R.zero_table(c) for c in R.fold_cases()[::7]):
        x, _ = c.inputs()
        ref, _ = R.rotate_f64(x[:, :c.H + c.Hkv], c.inv_freq(), c.positions())
        pq, pk = R.planted_expected(c)
        got = R.rne_bf16(ref)
        assert np.array_equal(got[:, :c.H], pq), c
        assert np.array_equal(got[:, c.H:].reshape(c.S, c.T, c.Hkv, c.D).transpose(0, 2, 1, 3), pk), c
        if c.table.startswith("quarter"):
            # exact for the kernel too: the contamination |x cos| stays below 2^-20
            a = np.float64(R.F32_HALF_PI)
            assert 15 * abs(math.cos(a)) < 2.0 ** -20 and np.float32(math.sin(a)) == 1
            assert not R.check(c, *R.emulate(c, ulps=(-2, 2))[:3])
            assert not R.check(c, *R.emulate(c, ulps=(2, -2))[:3])


def test_open_window_share_is_at_most_one_percent():
    worst = 0.0
    for c in RANDOM:
        share = R.expected(c).open_share()
        print(f"open-window share {c}: {100 * share:.3f} %")
        worst = max(worst, share)
        assert share <= 0.01, c
    print(f"worst open-window share: {100 * worst:.3f} %")


def _err_over_delta(c, y):
    e = R.expected(c)
    H = c.H
    k = y[:, H:].reshape(c.S, c.T, c.Hkv, c.D).transpose(0, 2, 1, 3)
    return max(float((np.abs(y[:, :H] - e.q_ref) / e.q_delta).max()),
               float((np.abs(k - e.k_ref) / e.k_delta).max()))


def test_fp32_restatement_with_two_ulp_sincos_stays_inside_every_window():
    worst = 0.0
    for c in RANDOM:
        for u in ULPS + ((0, 0),):
            q, kh, vh, y = R.emulate(c, ulps=u)
            assert not R.check(c, q, kh, vh), (c, u)
            worst = max(worst, _err_over_delta(c, y))
    print(f"worst |fp32 - ref| / delta over every case: {worst:.3f}")
    assert worst < 1.0


def test_position_sweep_at_head_dim_128():
    """D = 128, operands N(0, 2^2), positions 0 .. 131135 (64 a launch, every power of two and
    its neighbours among them)."""
    rng = np.random.default_rng(9)
    edges = sorted({p for k in range(18) for p in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | {0, 131135})
    worst, share = 0.0, 0.0
    for i in range(6):
        pl = tuple(edges[:56]) if i == 0 else tuple(int(v) for v in rng.integers(0, 131136, size=64))
        c = R.Case(f"sweep{i}", 128, 4, 2, 0, 1, 32, table="llama-3.1-8b", plen=pl, n_str=1, seed=900 + i)
        share = max(share, R.expected(c).open_share())
        for u in ULPS:
            q, kh, vh, y = R.emulate(c, ulps=u)
            assert not R.check(c, q, kh, vh), (c, u)
            worst = max(worst, _err_over_delta(c, y))
    print(f"position sweep: worst |fp32 - ref| / delta {worst:.3f}, open-window share {100 * share:.3f} %")
    assert worst < 1.0 and share <= 0.01


# mutant -> the cases that must each reject it
CAUGHT_BY = {
    "pos_off_by_one": ("p8-D128H32k8-hb5T3ld64", "slot-D64H8k2-hb0T1ld64", "tile-D256H16k8-hb24T64ld96"),
    "interleaved_pairs": ("p8-D64H8k2-hb5T3ld64", "p4dim-D8H6k2-hb5T3ld64", "tile-D24H4k2-hb0T32ld32"),
    "sine_sign": ("p8-D256H16k8-hb5T3ld64", "p4off-D128H64k8-hb5T3ld64"),
    "freq_index_shift": ("p8-D128H32k8-hb5T3ld64", "p8-D256H16k8-hb5T3ld64", "p4dim-D40H6k3-hb5T3ld64"),
    "bf16_truncate": ("p8-D64H8k2-hb5T3ld64", "tile-D128H32k8-hb5T40ld64", "fold3-D64H8k2-hb30T3ld64"),
    "group_prefix_ignored": ("gmap-D64H8k2-hb5T3ld64-g3", "gmap-D64H8k2-hb5T3ld64-rows-g5",
                             "gmap-tile-D128H32k8-hb8T33ld64-g3", "gmap-tile-D128H32k8-hb8T33ld64-g5"),
    "v_slot_off_by_one": ("slot-D64H8k2-hb31T2ld64", "slot-D64H8k2-hb31T2ld64-rows",
                          "slot-D40H6k3-hb63T1ld64"),
    "v_tile_ignored": ("slot-D64H8k2-hb32T1ld64", "slot-D40H6k3-hb31T2ld64", "slot-D64H8k2-hb37T2ld96"),
    "surplus_split_summed": ("fold3-D64H8k2-hb30T3ld64", "fold5-D128H32k8-hb30T1ld64",
                             "fold9-D256H16k8-hb30T1ld64", "fold17-D64H8k2-hb30T3ld64-rows",
                             "fold5-big-D64H8k2-hb30T3ld64"),
    "splits_reversed": ("fold5-cancel-D64H8k2-hb30T3ld64", "fold12-cancel-D128H32k8-hb30T1ld64-rows"),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_checker_rejects_the_wrong_kernel(mutant):
    assert set(CAUGHT_BY) == set(R.MUTANTS)
    for name in CAUGHT_BY[mutant]:
        c = _case(name)
        assert not R.check(c, *R.emulate(c)[:3]), name
        errs = R.check(c, *R.emulate(c, mut=[mutant])[:3])
        assert errs, f"{mutant} passes {name}"
        if c.splits and mutant in ("surplus_split_summed", "splits_reversed"):
            z = R.zero_table(c)                   # bit-exact against the fold on the zero table
            assert R.check(z, *R.emulate(z, mut=[mutant])[:3]), f"{mutant} passes {z}"


def test_quarter_turn_family_decodes_the_frequency_index_used():
    for fam in R.quarter_families():
        half = fam[0].half
        good = [R.emulate(c)[0] for c in fam]
        assert all(not R.check(c, *R.emulate(c)[:3]) for c in fam)
        assert (R.decode_freq_index(fam, good) == np.arange(half)).all()
        bad = [R.emulate(c, mut=["freq_index_shift"]) for c in fam]
        assert any(R.check(c, *b[:3]) for c, b in zip(fam, bad)), fam[0]
        used = R.decode_freq_index(fam, [b[0] for b in bad])
        assert (used == np.roll(np.arange(half), -1)).all()
        # one wrong index anywhere is caught: pair j served by index j ^ 1
        for c in fam[:1]:
            q, kh, vh, _ = R.emulate(c)
            j = half - 1
            swapped = R.emulate(R.replace(c, table="quarter:all" if not c.turned()[j] else "zero"))[0]
            q = q.copy()
            q[..., j], q[..., j + half] = swapped[..., j], swapped[..., j + half]
            assert R.check(c, q, kh, vh)


def test_slow_half_index_shift_is_outside_the_windows():
    """The old 2e-2 tolerance passed a frequency index off by one in the slow half of the
    table; the windows do not."""
    c = _case("p8-D128H32k8-hb5T3ld64")
    x, _ = c.inputs()
    inv = c.inv_freq().copy()
    inv[c.half // 2:] = np.roll(inv, -1)[c.half // 2:]
    inv[-1] = inv[-2]
    ref, _ = R.rotate_f64(x[:, :c.H], inv, c.positions())
    e = R.expected(c)
    g = R.bf16_value(R.rne_bf16(ref))
    bad = ~((R.bf16_value(e.q_lo) <= g) & (g <= R.bf16_value(e.q_hi)))
    assert bad[..., c.half // 2:c.half - 1].any()
