"""CPU evidence for tests/test_topk_proposer_gpu.py: the geometry of tests/topk_ref.py is the
library's (cs_vocab_topk_workspace_size, and a Python decode_layout against
cs_beam_decode_workspace_size, which pins decode_kp and the proposer chunk count), the planted
rows put every position class of every chunk geometry at rank 0, at rank K - 1 and at the first
loser, the selection reference is the oracle's stable sort, a numpy restatement of the two
proposers reproduces the expected ids of every case, and the checker rejects each wrong
proposer of topk_ref.MUTANTS on a named case."""
import dataclasses
from importlib import import_module

import numpy as np
import pytest

import topk_ref as T

CASES = {c.name: c for c in T.all_cases()}
N_CU = 256          # an MI355X; the GPU file asserts the grid orders from the device's own count


def _small(c, rows=6):
    """The case with at most `rows` rows (same geometry and classes, fewer probes a launch)."""
    return dataclasses.replace(c, rows=min(c.rows, rows)) if c.path == "topk" else c


def test_case_names_are_unique_and_shapes_reach_their_paths():
    assert len(CASES) == len(T.all_cases())
    for dt in T.DTYPES:
        f32 = dt == T.F32
        for c in T.decode_cases(dt):
            lay = T.decode_layout(c.A, c.rows, c.V, c.K, dt)
            assert lay["kp"] == c.kp and lay["nchunk"] == c.nchunk
            if "-kp4-" in c.name:
                assert c.kp == 4 and (c.rows, c.A) == (2, 2) and lay["cached"]
            if "-big-" in c.name:
                assert c.kp == (8 if f32 else 16) and (c.rows, c.A) == (64, 1)
                assert c.rows * -(-c.V // (c.kp * 1024)) == 128 and c.nchunk == 2 and lay["cached"]
            assert T.decode_rows_first(lay["row_blocks"], N_CU) == ("rows512" not in c.name)
        un = CASES[f"{dt}-dec-uncached"]
        assert un.kp == 4 and un.nchunk * un.K == 4608 and not T.decode_layout(2, 2, un.V, 256, dt)["cached"]
        assert T.decode_layout(8, 64, CASES[f"{dt}-dec-rows512"].V, 10, dt)["row_blocks"] == 512
        # aligned rows take the vector path on full chunks, a misaligned base the scalar path
        names = {c.geo_name for c in T.decode_cases(dt)}
        want = {"f32-kp4-vec", "f32-kp4-scalar", "f32-kp8-vec", "f32-kp8-scalar"} if f32 else \
            {"raw-kp4", "raw-kp16"}
        assert names == want, names
        for c in T.decode_cases(dt):
            assert c.ref_vec == (c.layout == "aligned"), c.name
        tk = T.topk_cases(dt)
        assert {c.K for c in tk} == {1, 10, 50, 256} and {c.rows for c in tk} == {1, 3, 300}
        for K in T.TOPK_K:
            vs = {c.V for c in tk if c.K == K}
            assert vs >= {K, 4095, 4096, 4097, 8192, 8193, 8192 + K, 8192 + K + 1, 8192 + 257,
                          8192 + 255, 8192 + 256} and (K == 1 or 8192 + K - 1 in vs)
        assert {c.layout for c in tk} == set(T.LAYOUTS)
        for c in tk + T.decode_cases(dt):
            e = T.ELT[dt]
            assert c.ld >= c.V and (c.layout == "dense") == (c.ld == c.V)
            assert c.layout not in ("aligned", "off1") or (c.ld * e % 16 == 0 and c.ld > c.V)
            assert c.layout != "odd" or c.ld * e % 16 != 0
            assert c.V * e * max(c.rows, c.rows * c.A) <= 20e6


def test_geometry_is_the_librarys(pkg):
    Lb = import_module(pkg.__name__ + "._lib").load()
    for rows, V, k in {(c.rows, c.V, c.K) for c in T.all_cases() if c.path == "topk"} | \
            {(2, 131073, 256), (1, 256000, 256), (5, 1, 1), (7, 128256, 10)}:
        assert Lb.cs_vocab_topk_workspace_size(rows, V, k) == T.topk_workspace_bytes(rows, V, k)
    shapes = {(c.A, c.rows, c.V, c.K) for c in T.all_cases() if c.path == "decode"}
    shapes |= {(A, B, V, K) for A in (1, 3, 16, 64) for B in (1, 2, 7, 8, 16, 63, 64, 128)
               for V in (1, 777, 4096, 4097, 8192, 8193, 16384, 16385, 57344, 57345, 114688, 114689,
                         128256, 256000) for K in (1, 10, 64, 65, 256) if K <= V}
    for A, B, V, K in sorted(shapes):
        assert Lb.cs_beam_decode_workspace_size(A, B, V, K) == T.decode_workspace_bytes(A, B, V, K), \
            (A, B, V, K)


def test_maps_are_bijections_and_the_stated_formulas():
    for g in (T.TOPK_GEO, T.decode_geo(T.F32, 4, True), T.decode_geo(T.F32, 8, True),
              T.decode_geo(T.F32, 4, False), T.decode_geo(T.F32, 8, False),
              T.decode_geo(T.BF16, 4, False), T.decode_geo(T.F16, 16, True)):
        tab = g.table()
        assert sorted(tab.reshape(-1)) == list(range(g.CH)), g.name
    t, j = 37, 6
    assert T.TOPK_GEO.elem(t, j) == t + 256 * j
    assert T.decode_geo(T.F32, 8, True).elem(t, j) == (j // 4 * 1024 + t) * 4 + j % 4
    assert T.decode_geo(T.F32, 8, False).elem(t, j) == t + 1024 * j
    assert T.decode_geo(T.BF16, 4, False).elem(t, 3) == t * 4 + 3
    assert T.decode_geo(T.F16, 16, True).elem(t, 13) == (13 // 8 * 1024 + t) * 8 + 13 % 8


def _required(c):
    g = c.geo(0)
    kinds = set(T.CLASS_KINDS) | {"vocab_last"}
    if c.nchunk > 1:
        kinds |= T.ROW_KINDS
    if g.raw:
        kinds |= T.RAW_KINDS
    if g.group > 1 and g.per > g.group:
        kinds |= T.GROUP_KINDS
    return kinds


def test_every_class_is_rank0_last_rank_and_first_loser_per_dtype_and_path():
    """A case whose launches sweep its class list (300 rows, 64 beams, or the swept 2-beam
    cases) plants every class of its list in each of the three roles, and per dtype and chunk
    geometry every class kind that geometry has is planted in each role."""
    table = {}
    tails = {}
    for c in T.all_cases():
        cl = c.classes()
        avail = {nm for nm, _ in cl}
        assert {T.class_kind(nm) for nm in avail} <= _required(c) | T.ROW_KINDS, c.name
        if c.nchunk > 1 and c.chunk_n(0) == c.CH:
            assert {T.class_kind(nm) for nm in avail} >= _required(c), (c.name, sorted(avail))
        swept = c.rows >= 64 or (c.path == "decode" and "r257-K10" in c.name)
        tails.setdefault((c.dtype, c.geo_name), set()).add((c.K, c.chunk_n(c.nchunk - 1)))
        if not swept or c.K < 2 or (c.path == "topk" and c.dtype != T.F32):
            continue
        have = {"rank 0": set(), f"rank {c.K - 1}": set(), "first loser": set()}
        if c.V == c.K:                  # the whole row wins
            del have["first loser"]
        for s in range(T.n_shifts(c)):
            for bg in T.BACKGROUNDS[:1 if c.rows > 64 else 2]:
                for role in T._content(T._key_case(c), bg, s)[1]:
                    for r, names in role.values():
                        if r in have:
                            have[r] |= set(names)
        for r, got in have.items():
            assert got == avail, (c.name, r, sorted(avail - got))
            dts = T.DTYPES if c.path == "topk" else (c.dtype,)
            for dt in dts:
                label = "loser" if r == "first loser" else "rank 0" if r == "rank 0" else "rank K-1"
                table.setdefault((dt, c.geo_name, label), set()).update(T.class_kind(n) for n in got)
    paths = {(c.dtype, c.geo_name): c for c in T.all_cases() if c.nchunk > 1 and c.chunk_n(0) == c.CH}
    assert len(paths) == 3 + 4 + 2 + 2
    for (dt, gn), c in paths.items():
        for r in ("rank 0", "rank K-1", "loser"):
            got = table.get((dt, gn, r), set())
            assert got >= _required(c), (dt, gn, r, sorted(_required(c) - got))
        # the tail chunk's last element at n = 1, K - 1, K, K + 1, 255, 256, 257 and 13 (K = 10)
        ns = {n for K, n in tails[(dt, gn)] if K == 10}
        assert ns >= {1, 9, 10, 11, 255, 256, 257, 13}, (dt, gn, sorted(ns))


def test_a_removed_class_fails_the_coverage_assertion(monkeypatch):
    """What the coverage test relies on: a class dropped from chunk_classes is missed."""
    real = T.chunk_classes
    monkeypatch.setattr(T, "chunk_classes", lambda g, n: [x for x in real(g, n) if x[0] != "wave_hi"])
    c = CASES["bf16-dec-big-r257-K10-aligned"]
    assert "wave_hi" not in {T.class_kind(nm) for nm, _ in c.classes()}
    assert not {T.class_kind(nm) for nm, _ in c.classes()} >= _required(c)


def test_selection_reference_is_the_oracles_stable_sort(orc):
    for name in ("f32-topk-VK-K10-r3", "bf16-topk-V4097-K50-r3", "f16-topk-V8192+K+1-K256-r3",
                 "f32-dec-kp4-r257-K10-aligned", "bf16-dec-big-r13-K10-off1"):
        c = CASES[name]
        for kind in T.KINDS:
            for cap in T.CAPS:
                Ln = T.make_launch(c, kind, 1, cap)
                with np.errstate(invalid="ignore"):
                    xc = T.softcap64(Ln.x.astype(np.float64), cap)
                ids, _ = orc.vocab_topk(np.ascontiguousarray(xc), c.K)
                assert np.array_equal(ids, Ln.exp_ids), (name, kind, cap)
    # by hand: value descending, id ascending, -0.0 ties +0.0, -inf before NaN, NaN by id
    x = np.array([[np.nan, 1.0, -np.inf, 0.0, 3.0, -0.0, 3.0, np.nan, np.inf]])
    assert T.expected_topk(x, 9).tolist() == [[8, 4, 6, 1, 3, 5, 2, 0, 7]]
    assert T.expected_topk(x, 2).tolist() == [[8, 4]]


def test_builder_rejects_values_the_cap_could_reorder():
    T.assert_unambiguous(np.array([1.0, 1.25, 4096.0, 8192.0, np.inf, np.nan]), 30.0)
    with pytest.raises(AssertionError):
        T.assert_unambiguous(np.array([400.0, 400.25]), 30.0)       # 2e-10 apart after the cap
    with pytest.raises(AssertionError):
        T.assert_unambiguous(np.array([1.0, 1.0 + 2.0 ** -20]), 75.0)


def _restated_agrees(c, kinds, shifts=(0,)):
    for i, kind in enumerate(kinds):
        for s in shifts:
            cap = T.CAPS[(i + s + c.K) % 3]
            Ln = T.make_launch(c, kind, s, cap)
            rows = np.unique(np.linspace(0, c.rows - 1, 6).astype(int))
            bad, worst = T.check(Ln, *T.Restated().launch(Ln, rows), rows)
            assert not bad, "\n".join(bad[:10])
            assert worst < 0.5


@pytest.mark.parametrize("dt", T.DTYPES)
def test_restatement_reproduces_every_case(dt):
    """The correct restatement against the expected ids (and values, inside the cap window) of
    every case: every family on the full sweeps and on one case per shape, the backgrounds and
    the special rows elsewhere, the cap rotating."""
    for c in T.decode_cases(dt):
        full = "-K10-aligned" in c.name or "r257" in c.name or "uncached" in c.name
        _restated_agrees(c, T.KINDS if full else ("flat", "stairs", "special"))
    for c in T.topk_cases(dt):          # the geometry is the same for every dtype; ld is not
        if dt == T.F32 or c.rows == 3:
            _restated_agrees(_small(c), T.KINDS if dt == T.F32 else ("flat", "stairs", "special"))


# (mutant, case, family, shift, cap): the named case that rejects each wrong proposer
REJECTS = [
    ("tail_drops_last", "bf16-topk-V8192+257-K10-r3", "flat", 0, 0.0),
    ("tail_drops_last", "f32-dec-big-r257-K10-off1", "flat", 0, 30.0),
    ("tail_reads_past", "f16-topk-V8192+1-K10-r3", "stairs", 0, 75.0),
    ("tail_reads_past", "bf16-dec-kp4-r13-K10-aligned", "flat", 0, 0.0),
    ("raw_halves_swapped", "bf16-dec-kp4-r257-K10-aligned", "flat", 0, 0.0),
    ("raw_halves_swapped", "f16-dec-big-r257-K10-aligned", "flat", 0, 30.0),
    ("vec_ids_on_scalar", "f32-dec-kp4-r257-K10-off1", "flat", 0, 0.0),
    ("vec_ids_on_scalar", "f32-dec-big-r257-K10-off1", "stairs", 0, 0.0),
    ("scalar_ids_on_vec", "f32-dec-kp4-r0-K10-aligned", "flat", 0, 0.0),
    ("scalar_ids_on_vec", "f32-dec-big-r257-K10-aligned", "flat", 0, 75.0),
    ("wrong_v0", "f32-topk-V8192+257-K10-r3", "flat", 0, 0.0),
    ("wrong_v0", "bf16-dec-big-r257-K10-aligned", "flat", 0, 0.0),
    ("chunk_keeps_k_minus_1", "f32-topk-V8192+257-K10-r3", "onechunk", 0, 0.0),
    ("chunk_keeps_k_minus_1", "f16-dec-kp4-r257-K10-aligned", "onechunk", 0, 30.0),
    ("merge_first_4096", "bf16-dec-uncached", "flat", 0, 0.0),
    ("merge_first_4096", "f32-dec-uncached", "perchunk", 0, 30.0),
    ("ties_desc_id", "f32-topk-V8192+257-K10-r3", "edge_ties", 0, 0.0),
    ("ties_desc_id", "bf16-dec-kp4-r257-K10-aligned", "edge_ties", 0, 75.0),
    ("nan_first", "f16-topk-VK-K10-r3", "special", 0, 0.0),
    ("nan_first", "bf16-dec-kp4-r257-K10-odd", "special", 0, 30.0),
    ("negzero_below", "f32-topk-V4097-K10-r3", "special", 0, 0.0),
    ("negzero_below", "bf16-dec-kp4-r257-K10-aligned", "special", 0, 0.0),
    ("padding_real", "f32-topk-V8192+1-K10-r3", "flat", 0, 0.0),
    ("padding_real", "f16-dec-big-r13-K10-aligned", "stairs", 0, 30.0),
    ("stride_ignored", "bf16-topk-V4097-K10-r3", "flat", 0, 0.0),
    ("stride_ignored", "f32-dec-kp4-r257-K10-odd", "flat", 0, 0.0),
]


@pytest.mark.parametrize("mutant,name,kind,shift,cap", REJECTS,
                         ids=[f"{m}-{n}-{k}" for m, n, k, _, _ in REJECTS])
def test_checker_rejects_the_wrong_proposer(mutant, name, kind, shift, cap):
    c = CASES[name]
    Ln = T.make_launch(c, kind, shift, cap)
    rows = np.arange(min(c.rows, 8))
    bad, _ = T.check(Ln, *T.Restated().launch(Ln, rows), rows)
    assert not bad, "\n".join(bad[:10])
    bad, _ = T.check(Ln, *T.Restated(mutant).launch(Ln, rows), rows)
    assert bad, f"{mutant} passes {name}/{kind}"
    # a failure names the case, the row, the rank and the class of the first wrong id
    assert name in bad[0] and " row " in bad[0] and " rank " in bad[0] and "class " in bad[0]


def test_every_mutant_has_a_named_case_in_both_proposers():
    assert len(T.MUTANTS) == 13
    for path in ("topk", "dec"):
        got = {m for m, n, *_ in REJECTS if f"-{path}-" in n}
        only_decode = {"raw_halves_swapped", "vec_ids_on_scalar", "scalar_ids_on_vec", "merge_first_4096"}
        assert got == set(T.MUTANTS) - (only_decode if path == "topk" else set()), (path, got)
