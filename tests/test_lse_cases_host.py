"""CPU evidence for tests/test_lse_stream_gpu.py: the geometry of tests/lse_ref.py is the
library's (plan_split against cs_workspace_size), the planted cases reach every position class
of block_lse_partial per dtype and path, the closed-form references are the float64
log-sum-exp, an fp32 restatement of the kernel's order of operations with every exp2,
reciprocal and logf pushed +-1 ulp stays inside every derived window, and the checker rejects
each wrong kernel of lse_ref.MUTANTS on a named case.

Figures measured by this file (run with -s to print them): the restated kernel uses at most
0.74 of a counting row's window (a logf one ulp off the correctly rounded one, of the two ulps
allowed), 0.27 of any other window without cap, 0.18 at cap 30 and 0.17 at cap 75."""
from importlib import import_module

import numpy as np
import pytest

import lse_ref as R

CASES = {c.name: c for c in R.all_cases()}
PUSHES = (1, -1, "mix")


def test_case_names_are_unique_and_shapes_are_the_planned_ones():
    assert len(CASES) == len(R.all_cases())
    for dt in R.DTYPES:
        e = R.EPV[dt]
        un = [c for c in R.unsplit_cases() if c.dtype == dt]
        assert all(c.plan == (1, c.V) for c in un)
        at0 = {R.geometry(dt, 0, c.V, c.plan)[0].nvec for c in un}
        assert at0 >= set(R.UNSPLIT_NVEC)
        assert max(c.V for c in un) == 4097 * e
        assert {c.V for c in un} >= {1, 2, 3, 7}
        assert any(c.rows == 300 and c.view_of > 300 for c in un)
        assert any(not c.pad for c in un) and {0, 1, 3, 1025} <= {c.k for c in un}
        # ld = 1 (mod EPV): the rows of one launch cycle through every head length
        for c in un:
            if c.pad:
                assert c.ld % e == 1 and c.ld > c.V
                assert {c.off(r) for r in range(e)} == set(range(e))
    assert max(c.V for c in R.all_cases()) <= 41000          # the counting rows' step / window
    for (dt, V), (ns, ln, last) in R.SPLIT_PLANS.items():
        for dts in ((dt, R.F16) if dt == R.BF16 else (dt,)):
            for rows in (1, 3, 64):
                assert R.plan_split(rows, V, dts) == (ns, ln)
                assert V - (ns - 1) * ln == last
                assert f"{dts}-s-V{V}-r{rows}" in CASES
    assert {c.k for c in R.split_cases()} >= {0, 1, 3, 65}


def test_plan_split_is_the_librarys(pkg):
    """cs_workspace_size is 8 bytes per (row, split) of the larger of the bf16 and f32 plans."""
    L = import_module(pkg.__name__ + "._lib").load()
    shapes = {(c.rows, c.V) for c in R.all_cases()}
    shapes |= {(r, v) for r in (1, 2, 5, 16, 63, 100, 255, 256) for v in
               (1, 4095, 4096, 8191, 8192, 16383, 16384, 50000, 128256, 256000)}
    for rows, V in sorted(shapes):
        assert L.cs_workspace_size(rows, V, 3) == R.workspace_bytes(rows, V), (rows, V)


def test_every_position_class_is_planted_per_dtype_and_path():
    """Every class that exists for a case's geometry is in its class list, the launches of a
    case with 64 rows or more plant every class of every alignment, and each class kind is
    planted in at least one case per dtype and path."""
    kinds_all = {"elem0", "elem_last", "head_last", "after_head", "tail_prev", "tail_first",
                 "tail_last", "random"}
    kinds_all |= {f"{m}_{e}" for m in ("v63", "v64", "vB-1", "vB", "v2B-1", "v2B", "sweep_last",
                                       "rem_first", "vec_last") for e in ("first", "last")}
    split_only = {"edge_prev", "edge", "quad2_first", "last_split"}
    table = {}
    lines = []
    for c in R.all_cases():
        have = set()
        for s in range(R.n_shifts(c) if c.rows >= 64 else 2):
            have |= set(R.probe_cols(c, s)[1])
        avail = {nm for r in range(min(c.rows, c.epv)) for nm, _ in c.classes(r)}
        if c.rows >= 64:
            assert have == avail, (c.name, sorted(avail - have))
        # what exists for the geometry is listed: a head when some row is misaligned, ...
        geo = [sp for r in range(min(c.rows, c.epv))
               for sp in R.geometry(c.dtype, c.off(r), c.V, c.plan)]
        kinds = {R.class_kind(n) for n in avail}
        assert ("head_last" in kinds) == any(sp.head > 0 for sp in geo)
        assert ("tail_first" in kinds) == any(sp.tail0 < sp.n for sp in geo)
        assert ("rem_first_first" in kinds) == any(
            sp.nvec and not sp.in_sweep(np.arange(sp.nvec)).all() for sp in geo
            if sp.index in (0, 1, R.SPLIT_QUAD, len(geo) // min(c.rows, c.epv) - 1))
        assert ("v2B_first" in kinds) == any(
            sp.nvec > 2 * sp.block for sp in geo
            if sp.index in (0, 1, R.SPLIT_QUAD, len(geo) // min(c.rows, c.epv) - 1))
        lacks = (kinds_all | (split_only if c.path == "split" else set())) - kinds
        if lacks:
            lines.append(f"{c.name:24s} plan {c.plan}  lacks: {' '.join(sorted(lacks))}")
        table.setdefault((c.dtype, c.path), set()).update(R.class_kind(n) for n in have)
    print("classes a case's geometry does not have (the other cases have every class):\n"
          + "\n".join(lines))
    for (dt, path), kinds in sorted(table.items()):
        want = kinds_all | (split_only if path == "split" else set())
        assert kinds >= want, (dt, path, sorted(want - kinds))
    # the quad items: a second item with one valid and three invalid sub-blocks (5 splits), and
    # three items, the last with one valid sub-block (9 splits)
    assert CASES["bf16-s-V40961-r64"].plan[0] == 5 and CASES["f32-s-V40961-r64"].plan[0] == 9


def test_closed_forms_are_the_float64_log_sum_exp():
    """The planted rows' references (a background value and one plant) against the plain
    float64 reference summed element by element, and the text's own figures."""
    for name in ("bf16-u-nvec1", "f32-u-nvec1025", "f16-s-V16385-r3", "bf16-u-V3"):
        c = CASES[name]
        for kind in R.KINDS_NOCAP + tuple(s[0] for s in R.SAT) + ("allinf",):
            L = R.make_launch(c, kind, 1)
            lse, tok = R.reference(L.values(), L.targets, L.cap, c.V)
            for a, b in ((lse, L.ref_lse), (tok, L.ref_tok)):
                assert np.array_equal(np.isnan(a), np.isnan(b)), (name, kind)
                inf = np.isinf(a)
                assert np.array_equal(a[inf], b[inf]), (name, kind)
                ok = np.isfinite(a)
                assert np.allclose(a[ok], b[ok], rtol=0, atol=1e-11), (name, kind)
    L = R.make_launch(CASES["bf16-s-V40969-r3"], "count")
    assert np.allclose(L.ref_lse, np.log(40969)) and L.win_lse.max() < np.log(40969 / 40968) / 8
    L = R.make_launch(CASES["bf16-s-V40969-r3"], "sat30+")
    assert np.allclose(L.ref_lse, np.log(np.exp(30.0) + 40968), rtol=0, atol=1e-12)
    L = R.make_launch(CASES["bf16-s-V40969-r3"], "sat75-")
    assert np.allclose(L.ref_lse, np.log(np.exp(-75.0) + 40968), rtol=0, atol=1e-12)
    L = R.make_launch(CASES["bf16-s-V40969-r3"], "latemax")
    assert (L.win_lse < 2e-5).all()                          # a missing rescale is off by log 2
    L = R.make_launch(CASES["f32-u-nvec4097"], "random")
    assert (L.win_lse < 3e-5).all() and (L.win_tok < 3e-5).all()      # the old tests: 1e-3
    L = R.make_launch(CASES["bf16-u-nvec4097"], "random", cap=75.0)
    assert (L.win_lse < 2e-4).all()


def test_reference_agrees_with_the_fp64_oracle(orc):
    """lse_ref.reference against oracle/cs_oracle.c on dense and planted rows in the three cap
    modes; they differ only on a row without a finite element (NaN there, -inf here)."""
    for name in ("f32-u-V7", "bf16-u-nvec1", "f16-u-nvec1025"):
        c = CASES[name]
        for kind, cap in [("random", cap) for cap in R.CAPS] + [("masked", 0.0), ("nan_randn", 30.0),
                                                                ("latemax", None), ("sat75+", None),
                                                                ("onehot3.5", None)]:
            L = R.make_launch(c, kind, 2, cap=cap)
            x = np.ascontiguousarray(L.values())
            tok, lse = orc.logsoftmax_gather(x, L.targets, softcap=L.cap)
            some = ~np.isneginf(L.ref_lse)      # a mask may leave a short row without an element
            assert np.isnan(lse[~some]).all() and some.sum() >= c.rows // 2
            want_lse = np.where(L.nan_row, np.nan, L.ref_lse)          # the checker's rule
            want_tok = np.where(L.nan_row[:, None], np.nan, L.ref_tok)
            for a, b in ((lse[some], want_lse[some]), (tok[some], want_tok[some])):
                assert np.array_equal(np.isnan(a), np.isnan(b)), (name, kind, cap)
                assert np.array_equal(np.isinf(a), np.isinf(b)), (name, kind, cap)
                ok = np.isfinite(a)
                assert np.allclose(a[ok], b[ok], rtol=0, atol=1e-10), (name, kind, cap)
    L = R.make_launch(CASES["f32-u-V7"], "allinf")
    tok, lse = orc.logsoftmax_gather(np.ascontiguousarray(L.values()), L.targets)
    assert np.isnan(lse).all() and np.isneginf(L.ref_lse).all()


RESTATED = [  # (case, rows restated, kinds)
    ("bf16-u-nvec0", 16, "all"), ("bf16-u-nvec1", 16, "all"), ("bf16-u-nvec1023", 8, "all"),
    ("bf16-u-nvec1025", 16, "all"), ("bf16-u-nvec2049", 8, "planted"),
    ("bf16-u-nvec4097", 8, "planted"), ("bf16-u-V1", 8, "planted"), ("bf16-u-V7", 16, "all"),
    ("f16-u-nvec1025", 8, "all"), ("f16-u-V3", 8, "planted"),
    ("f32-u-nvec1", 8, "all"), ("f32-u-nvec1025", 8, "all"), ("f32-u-nvec3073", 4, "planted"),
    ("f32-u-V2", 4, "planted"), ("bf16-u-aligned", 4, "planted"),
    ("bf16-s-V16384-r3", 3, "all"), ("bf16-s-V16385-r3", 3, "planted"),
    ("bf16-s-V40961-r3", 3, "all"), ("bf16-s-V40969-r1", 1, "planted"),
    ("bf16-s-V40967-r64", 8, "planted"), ("f16-s-V40961-r3", 3, "all"),
    ("f32-s-V8192-r3", 3, "all"), ("f32-s-V20485-r3", 3, "planted"), ("f32-s-V40961-r3", 3, "all"),
    ("f32-s-V20481-r64", 4, "planted"),
]
PLANTED = [(k, None) for k in R.KINDS_NOCAP] + [(s[0], None) for s in R.SAT] + \
          [("nan_inf", cap) for cap in R.CAPS]
DENSE = [(k, cap) for k in ("random", "masked", "nan_randn") for cap in R.CAPS]
_worst = {}


@pytest.mark.parametrize("name,nrows,which", RESTATED, ids=[r[0] for r in RESTATED])
def test_restated_kernel_stays_inside_the_windows(name, nrows, which):
    """The fp32 restatement with exp2 / rcp / logf one ulp up, one ulp down and mixed."""
    c = CASES[name]
    rows = np.unique(np.linspace(0, c.rows - 1, nrows).astype(int))
    for kind, cap in PLANTED + (DENSE if which == "all" else []):
        L = R.make_launch(c, kind, shift=len(kind), cap=cap)
        for push in PUSHES:
            lse, tok = R.Restated(push=push).launch(L, rows)
            bad, frac = R.check(L, lse, tok, rows)
            assert not bad, "\n".join(bad)
            key = "count" if kind == "count" else f"cap {L.cap:g}"
            _worst[key] = max(_worst.get(key, 0.0), frac)


# (mutant, case, kind, shift): the named case that rejects each wrong kernel
REJECTS = [
    ("drop_head", "bf16-u-nvec1025", "count", 0),
    ("drop_tail", "f32-u-nvec1025", "count", 0),
    ("drop_rem", "bf16-u-nvec1025", "count", 0),
    ("double_first", "f16-u-nvec1025", "count", 0),
    ("no_rescale", "bf16-u-nvec2049", "latemax", 0),
    ("nan_drop", "bf16-u-nvec1025", "nan_inf", 0),
    ("nan_drop", "f32-s-V20485-r3", "nan_inf", 0),
    ("read_past", "f32-u-nvec1023", "count", 0),
    ("read_past", "bf16-s-V40961-r3", "onehot0", 0),
    ("lose_last_split", "bf16-s-V40961-r3", "count", 0),
    ("merge_ignores_m", "f32-s-V20485-r3", "latemax", 0),
    ("gather_first_lanes", "bf16-s-k65", "count", 0),
    ("gather_first_lanes", "bf16-u-k1025", "count", 0),
]


@pytest.mark.parametrize("mutant,name,kind,shift", REJECTS,
                         ids=[f"{m}-{n}-{k}" for m, n, k, _ in REJECTS])
def test_checker_rejects_the_wrong_kernel(mutant, name, kind, shift):
    c = CASES[name]
    rows = np.arange(min(c.rows, 2 * c.epv))
    L = R.make_launch(c, kind, shift)
    bad, _ = R.check(L, *R.Restated().launch(L, rows), rows)
    assert not bad, "\n".join(bad)
    bad, _ = R.check(L, *R.Restated(mutant=mutant).launch(L, rows), rows)
    assert bad, f"{mutant} passes {name}/{kind}"


def test_every_mutant_has_a_named_case():
    assert {m for m, *_ in REJECTS} == set(R.MUTANTS) and len(R.MUTANTS) == 10


def _scalar(c, r, p):
    """Whether position p of row r is read by the scalar head or tail of its split."""
    sp = next(sp for sp in R.geometry(c.dtype, c.off(r), c.V, c.plan) if 0 <= p - sp.v0 < sp.n)
    return p - sp.v0 < sp.head or p - sp.v0 >= sp.tail0


def test_parent_kernel_loses_the_nan_only_on_an_empty_state():
    """The parent's lse_accum dropped a NaN that met an empty (m, s): at every scalar head or
    tail position (always the lane's first element) without cap and with the general cap, and
    in a vector of -inf and NaN without cap; the bf16 table and the fixed-offset sum were never
    affected.  Everything else about a row with a NaN was right."""
    seen = set()
    for name in ("bf16-u-nvec1025", "f32-u-nvec1025", "f16-s-V16385-r64"):
        c = CASES[name]
        rows = np.arange(1, c.rows, 2)
        for kind in ("nan_inf", "nan_randn"):
            for cap in R.CAPS:
                L = R.make_launch(c, kind, 0, cap=cap)
                lse, tok = R.Restated(mutant="nan_drop").launch(L, rows)
                for r, v in zip(rows, lse):
                    scalar = _scalar(c, r, L.nan_col[r])
                    lost = cap != 30.0 and (scalar or (kind == "nan_inf" and cap == 0.0))
                    assert np.isnan(v) != lost, (name, kind, cap, r, L.cls[r], v)
                    seen.add((lost, scalar))
                bad, _ = R.check(L, lse, tok, rows)
                assert bool(bad) == (cap != 30.0), (name, kind, cap)
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


def test_report_the_share_of_each_window_used():
    assert set(_worst) == {"count", "cap 0", "cap 30", "cap 75"}
    assert all(0.0 < v < 1.0 for v in _worst.values())
    print("worst share of a window used by the restated kernel: "
          + ", ".join(f"{k}: {v:.2f}" for k, v in sorted(_worst.items())))
