"""CPU tests of the induced-policy rollout path: the restatement (tests/rollout_ref.py, the
expected values of the GPU tests) is pinned to numpy's own stream and ``rng.choice`` loop and to
the reference's recorded rollouts (tests/golden/rollout_golden.npz), and cs_policy_rollout
rejects bad arguments with a status and a message before any launch."""
import ctypes
import os

import numpy as np
import pytest

import lottery_ref
import rollout_ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_golden.npz"))


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 + 5])
def test_uniforms_are_numpys_stream(seed):
    n = 1000
    assert np.array_equal(rollout_ref.uniforms(seed, 0, n), np.random.default_rng(seed).random(n))
    for first_draw in (2 ** 40 * 4, 3):
        want = np.random.Generator(np.random.PCG64(seed).advance(first_draw)).random(n)
        assert np.array_equal(rollout_ref.uniforms(seed, first_draw, n), want), first_draw


def test_advance_is_repeated_stepping():
    state, inc = rollout_ref.seed_state(12345)
    s = state
    for k in range(70):
        assert rollout_ref.advance(state, inc, k) == s, k
        s = rollout_ref.step(s, inc)


def test_walk_is_the_choice_loop_and_the_reference(golden):
    """walk's counts equal the rng.choice loop's, and the recorded p_hat of every 5,000-sample
    case (the 200,000-sample one is the GPU tests')."""
    names = [str(n) for n in golden["cases"]]
    assert len(names) == 12
    seen = 0
    for name in names:
        n = int(golden[f"n_{name}"])
        if n != 5000:
            continue
        B, L, seed = int(golden[f"B_{name}"]), int(golden[f"L_{name}"]), int(golden[f"seed_{name}"])
        m = B ** L
        tables = lottery_ref.policy(golden[f"p_{name}"], B, L)
        leaves = rollout_ref.walk(tables, B, L, seed, 0, n)
        counts = np.bincount(leaves, minlength=m)
        assert np.array_equal(counts, rollout_ref.host_loop(tables, B, L, seed, n)), name
        assert np.array_equal(counts / counts.sum(), golden[f"p_hat_{name}"]), name
        assert not counts[golden[f"p_{name}"] == 0.0].any(), name
        seen += 1
    assert seen == 11


def test_walk_splits_and_zero_probability_actions():
    # a split walk is the whole walk; action 0 of zero probability is never taken, u = 0 included
    p = np.random.default_rng(3).random(81)
    p[:27] = 0.0
    p /= p.sum()
    tables = lottery_ref.policy(p, 3, 4)
    whole = rollout_ref.walk(tables, 3, 4, 7, 0, 300)
    parts = [rollout_ref.walk(tables, 3, 4, 7, a, b - a) for a, b in ((0, 1), (1, 129), (129, 300))]
    assert np.array_equal(np.concatenate(parts), whole)
    assert whole.min() >= 27
    cdf = rollout_ref.cdf_tables(tables)
    assert cdf[0][0, 0] == 0.0 and cdf[0][0, -1] == 1.0
    assert np.searchsorted(cdf[0][0], 0.0, side="right") == 1


def _lib(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + "._lib").load()


def test_policy_rollout_rejects_bad_arguments(pkg):
    L = _lib(pkg)
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(260)

    def call(P=2, B=3, L_=4, first=0, n=100, policy=d, rng=d, work=d, counts=d, leaf=None,
             status=d):
        return L.cs_policy_rollout(policy, P, B, L_, rng, first, n, work, counts, leaf, status, None)

    for bad in (dict(B=0), dict(L_=0), dict(B=1, L_=65), dict(B=2, L_=15), dict(B=129, L_=2),
                dict(B=16385, L_=1), dict(P=-1), dict(first=-1), dict(n=-1),
                dict(first=2 ** 60, n=1),                    # (2^60 + 1) * 4 >= 2^62
                dict(first=2 ** 62, n=2 ** 62),
                dict(B=1, L_=1, first=2 ** 62 - 1, n=1),
                dict(P=2, n=2 ** 30, leaf=d),                # 2^31 leaves
                dict(policy=None), dict(rng=None), dict(work=None), dict(counts=None),
                dict(status=None),
                dict(policy=odd), dict(rng=odd), dict(work=odd), dict(counts=odd),
                dict(leaf=ctypes.c_void_p(258)), dict(status=ctypes.c_void_p(258))):
        assert call(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_policy_rollout: "), bad
    # an empty batch and an empty run of samples are no-ops; the limits themselves are accepted
    assert call(P=0) == 0
    assert call(n=0) == 0
    assert call(P=0, B=128, L_=2, first=2 ** 50) == 0
    assert call(P=0, B=1, L_=64) == 0
    assert call(P=0, B=1, L_=1, first=2 ** 62 - 2, n=1) == 0
    assert call(P=0, n=2 ** 31 - 1, leaf=d) == 0


def test_core_module_names_the_rollout_entry_points(pkg):
    from importlib import import_module
    core = import_module(pkg.__name__ + ".core")
    ops = import_module(pkg.__name__ + ".ops")
    for name in ("induced_policy_rollout", "induced_policy_rollout_batch",
                 "policy_equivalence_sweep"):
        assert callable(getattr(core, name, None)), name
    assert callable(ops.policy_rollout)
    st = ops.pcg64_state(7)
    assert st.dtype == np.uint64 and st.shape == (4,)
    state, inc = rollout_ref.seed_state(7)
    assert [int(x) for x in st] == [state >> 64, state & rollout_ref.MASK64,
                                    inc >> 64, inc & rollout_ref.MASK64]
