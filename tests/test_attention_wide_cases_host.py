"""The power of the wide-tile attention cases (tests/attention_wide_cases.py), on the CPU: these
tests check the CASES that tests/test_attention_wide_gpu.py runs, not the kernel.

Every planted-key case names the mask mutants it is aimed at (limit +- 1, the neighbour
streams' history or a future slot made visible).  Each, applied to the fp64 reference, must
move the targeted output row by >= 16 x the bound the GPU test holds the kernel to (so by
more than the bound, with room for the kernel's own error on both sides): a kernel with that
fault cannot pass.  No case is skipped or filtered."""
import numpy as np
import pytest

import attention_ref as R
import attention_wide_cases as W

ALL = [c for f in W.FAMILIES for c in W.cases(f)]
MASK_MUTANTS = ("limit+1", "limit-1", "neighbour", "future")


@pytest.mark.parametrize("c", ALL, ids=repr)
def test_case_is_a_wide_tile_shape_with_a_finite_reference(c):
    assert (c.D, c.cap, c.window, c.Hkv) == (128, 0.0, 0, 2)
    assert 32 % c.rep == 0 and (c.T >= 32 or c.name == "w-rule-T31")
    ref, A = R.reference(c)
    assert np.isfinite(ref).all() and np.isfinite(A).all()


@pytest.mark.parametrize("c", [c for c in ALL if c.checks], ids=repr)
def test_case_catches_its_mask_mutants(c):
    ref, A = R.reference(c)
    for mut, tok, head in c.checks:
        assert mut in MASK_MUTANTS
        bound = R.bound_of(A[tok, head])
        out = R.reference(c, mut)[0]
        ratio = float((np.abs(out[tok, head] - ref[tok, head]) / bound).max())
        assert ratio >= 16.0, f"{c}: mutant {mut} moves row ({tok}, {head}) by {ratio:.1f} x the bound only"


def test_every_planted_family_has_checks_and_every_mask_mutant_a_case():
    for fam in ("prefix", "missing", "history", "span", "rule"):
        assert all(c.checks for c in W.cases(fam)), fam
    assert {chk[0] for c in ALL for chk in c.checks} == set(MASK_MUTANTS)


def test_the_edges_the_wide_tile_adds_are_in_the_cases():
    """prefix lengths on both sides of 32 and 64, a padded prefix and an ld_hist of 96 (no
    second 32-key tile in the last 64-key block), tiles that span streams"""
    assert {c.plens[1] for c in W.cases("prefix")} == set(W.PREFIX_LENS)
    m = W.cases("missing")[0]
    assert m.Lp - m.off[-1] == 96 and m.ldh == 96 and m.ldh % 64 and (m.Lp - m.off[-1]) % 64
    for c in W.cases("span"):
        assert c.n_str == 3 and (c.T * c.rep) % 32
    assert sorted(c.rep for c in W.cases("span")) == [2, 4, 8]
    c31, c32 = W.cases("rule")
    assert (c31.T, c32.T) == (31, 32)
    q32 = c32.q.reshape(c32.S, 32, c32.H, c32.D)[:, :31].reshape(-1, c32.H, c32.D)
    assert bool((q32 == c31.q).all()) and bool((c31.kh == c32.kh).all())
