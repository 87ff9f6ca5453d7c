"""GPU tests of the induced-policy rollout (cs_policy_rollout) through ops.py and the core.py
drop-ins.

Expected values: the host restatement tests/rollout_ref.py (numpy's PCG64 stream in Python
integers and Generator.choice's cdf rule), which tests/test_rollout_host.py pins to numpy and to
the reference's recorded rollouts, and those recordings themselves
(tests/golden/rollout_golden.npz).  The restatement walks the policy tables the GPU made, so
both sides start from the same doubles and every comparison is exact: leaves element for
element, counts integer for integer, p_hat and tv bit for bit.  No tolerance anywhere.

The kernel gives a thread 16 consecutive samples and a workgroup 4096 (csrc/lottery.hip,
kRollPerThread / kRollPerGroup); the partition test sits on those boundaries."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import rollout_ref

pytestmark = pytest.mark.gpu

PER_THREAD, PER_GROUP = 16, 4096


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_golden.npz"))


@pytest.fixture(scope="module")
def core(pkg):
    return import_module(pkg.__name__ + ".core")


def _lottery(B, L, seed):
    """A random lottery with the subtree under first action 0 zeroed, and a deeper one."""
    m = B ** L
    p = np.random.default_rng(seed).random(m)
    if B > 1:
        p[: m // B] = 0.0
        if L > 1:
            p[-(m // B // B):] = 0.0
    return p / p.sum()


def _policy(ops, dev, p, B, L):
    """The GPU's policy of lottery p: (flat device tensor, the levels as host arrays)."""
    flat = ops.lottery_policy(torch.as_tensor(np.ascontiguousarray(p), device=dev), B, L, flat=True)
    host, levels, at = flat.cpu().numpy(), [], 0
    for t in range(L):
        n = B ** (t + 1)
        levels.append(host[..., at:at + n].reshape(*host.shape[:-1], B ** t, B))
        at += n
    return flat, levels


@pytest.fixture(scope="module")
def tree34(ops, dev):
    """One 3 x 4 lottery, its policy, and its first 3 * 4096 + 5 expected leaves (seed 7)."""
    p = _lottery(3, 4, 34)
    flat, levels = _policy(ops, dev, p, 3, 4)
    whole = rollout_ref.walk(levels, 3, 4, 7, 0, 3 * PER_GROUP + 5)
    whole.setflags(write=False)
    return {"p": p, "flat": flat, "levels": levels, "leaves": whole}


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 4), (2, 6), (5, 2), (1, 3), (1, 64), (128, 1), (128, 2),
                                 (2, 14)])
def test_draw_by_draw(ops, dev, B, L):
    m, n, seed = B ** L, 4097, 100 * B + L
    p = _lottery(B, L, seed)
    flat, levels = _policy(ops, dev, p, B, L)
    res = ops.policy_rollout(flat, B, L, ops.pcg64_state(seed), n, with_leaves=True)
    assert int(res["status"]) == 0
    leaves = res["leaves"].cpu().numpy()
    counts = res["counts"].cpu().numpy()
    want = rollout_ref.walk(levels, B, L, seed, 0, n)
    assert leaves.shape == (n,) and counts.shape == (m,) and counts.dtype == np.int64
    assert np.array_equal(leaves, want)
    assert np.array_equal(counts, np.bincount(want, minlength=m))
    assert not counts[p == 0.0].any()
    if B > 1:
        assert (p == 0.0).any() and len(np.unique(want)) > 1
    # the list of levels is the same policy as the flat tensor
    lv = ops.lottery_policy(torch.as_tensor(p, device=dev), B, L)
    again = ops.policy_rollout(lv, B, L, ops.pcg64_state(seed), n)
    assert torch.equal(again["counts"], res["counts"])


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, PER_THREAD - 1, PER_THREAD, PER_THREAD + 1, PER_GROUP - 1,
                               PER_GROUP, PER_GROUP + 1, 3 * PER_GROUP + 5])
def test_partition_boundaries(ops, tree34, n):
    res = ops.policy_rollout(tree34["flat"], 3, 4, ops.pcg64_state(7), n, with_leaves=True)
    want = tree34["leaves"][:n]
    assert np.array_equal(res["leaves"].cpu().numpy(), want)
    assert np.array_equal(res["counts"].cpu().numpy(), np.bincount(want, minlength=81))


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [1, 2 ** 32 + 1, 2 ** 40])
def test_jump_ahead(ops, tree34, first):
    """Samples far into the stream: the only place a wrong high word of the 128-bit jump shows."""
    res = ops.policy_rollout(tree34["flat"], 3, 4, ops.pcg64_state(7), 256, first_sample=first,
                             with_leaves=True)
    want = rollout_ref.walk(tree34["levels"], 3, 4, 7, first, 256)
    if first == 1:
        assert np.array_equal(want, tree34["leaves"][1:257])
    assert np.array_equal(res["leaves"].cpu().numpy(), want)
    assert np.array_equal(res["counts"].cpu().numpy(), np.bincount(want, minlength=81))


# 4 ---------------------------------------------------------------------------------------
def test_split_equals_whole(ops, tree34):
    N, N1 = 10_000, 3_333
    st = ops.pcg64_state(7)
    whole = ops.policy_rollout(tree34["flat"], 3, 4, st, N)["counts"]
    part = ops.policy_rollout(tree34["flat"], 3, 4, st, N1)
    assert int(part["counts"].sum()) == N1
    both = ops.policy_rollout(tree34["flat"], 3, 4, st, N - N1, first_sample=N1,
                              counts=part["counts"])
    assert both["counts"] is part["counts"]
    assert torch.equal(both["counts"], whole) and int(whole.sum()) == N
    assert np.array_equal(whole.cpu().numpy(), np.bincount(tree34["leaves"][:N], minlength=81))


# 5 ---------------------------------------------------------------------------------------
def test_batch_equals_alone(ops, dev):
    B, L, n, seeds = 3, 4, PER_GROUP + 100, [0, 7, 12345, 2 ** 64 + 5, 99]
    ps = np.stack([_lottery(B, L, 500 + k) for k in range(5)])
    flat, _ = _policy(ops, dev, ps, B, L)
    states = np.stack([ops.pcg64_state(s) for s in seeds])
    res = ops.policy_rollout(flat, B, L, states, n, with_leaves=True)
    assert res["counts"].shape == (5, 81) and res["leaves"].shape == (5, n)
    assert bool((res["status"] == 0).all())
    # the same words as a device tensor of int64 bit patterns
    dev_states = torch.as_tensor(states.view(np.int64), device=dev)
    assert torch.equal(ops.policy_rollout(flat, B, L, dev_states, n)["counts"], res["counts"])
    for k in range(5):
        alone = ops.policy_rollout(flat[k], B, L, states[k], n, with_leaves=True)
        assert torch.equal(alone["counts"], res["counts"][k]), k
        assert torch.equal(alone["leaves"], res["leaves"][k]), k
    assert not torch.equal(res["leaves"][0], res["leaves"][1])


# 6 ---------------------------------------------------------------------------------------
def test_bad_policies_get_a_status_and_leave_their_neighbours_alone(ops, core, dev):
    B, L, n = 3, 4, 1000
    ps = np.stack([_lottery(B, L, 600 + k) for k in range(7)])
    flat, _ = _policy(ops, dev, ps, B, L)
    good = flat.clone()
    row = 3 + 9 + 4 * 3                 # level 2 (after 3 + 9 entries), prefix 4
    flat[1, row] = float("nan")
    flat[3, row:row + 3] = torch.tensor([-0.1, 0.6, 0.5], dtype=torch.float64, device=dev)
    flat[5, :3] = torch.tensor([0.25 + 1e-6, 0.25, 0.5], dtype=torch.float64, device=dev)
    flat[6, :3] = torch.tensor([0.25 + 1e-9, 0.25, 0.5], dtype=torch.float64, device=dev)  # within sqrt(eps)
    states = np.stack([ops.pcg64_state(s) for s in range(7)])
    counts = torch.full((7, 81), 5, dtype=torch.int64, device=dev)
    res = ops.policy_rollout(flat, B, L, states, n, counts=counts, with_leaves=True)   # CS_OK
    assert res["status"].tolist() == [0, -1, 0, -1, 0, -1, 0]
    for k in (1, 3, 5):
        assert bool((res["counts"][k] == 5).all()), k
        assert bool((res["leaves"][k] == -1).all()), k
    for k in (0, 2, 4):
        alone = ops.policy_rollout(good[k], B, L, states[k], n, with_leaves=True)
        assert torch.equal(res["counts"][k], alone["counts"] + 5), k
        assert torch.equal(res["leaves"][k], alone["leaves"]), k
    assert int(res["counts"][6].sum()) == n + 5 * 81
    # a lottery with a negative entry induces no policy: the drop-in raises
    bad = ps[:2].copy()
    bad[1, 40] = -1e-3
    with pytest.raises(ops.CSError):
        core.induced_policy_rollout_batch(bad, B, L, num_samples=100)
    # the process is healthy afterwards
    torch.cuda.synchronize()
    assert int(res["counts"][0].sum()) == n + 5 * 81


# 7 ---------------------------------------------------------------------------------------
def test_reference_rollouts(core, golden):
    """Every recorded rollout of the reference, one call each and then batched by shape."""
    names = [str(n) for n in golden["cases"]]
    assert len(names) == 12 and int(golden["n_ref"]) == 200_000
    groups = {}
    for name in names:
        B, L, n = int(golden[f"B_{name}"]), int(golden[f"L_{name}"]), int(golden[f"n_{name}"])
        p_hat, tv = core.induced_policy_rollout(golden[f"p_{name}"], core.enumerate_leaves(B, L),
                                                B, L, num_samples=n,
                                                seed=int(golden[f"seed_{name}"]))
        assert np.array_equal(p_hat, golden[f"p_hat_{name}"]), name
        assert tv == float(golden[f"tv_{name}"]), name
        groups.setdefault((B, L, n), []).append(name)
    assert max(len(g) for g in groups.values()) >= 4
    for (B, L, n), group in groups.items():
        p_hat, tv = core.induced_policy_rollout_batch(
            np.stack([golden[f"p_{g}"] for g in group]), B, L, num_samples=n,
            seeds=[int(golden[f"seed_{g}"]) for g in group])
        for k, name in enumerate(group):
            assert np.array_equal(p_hat[k], golden[f"p_hat_{name}"]), name
            assert tv[k] == float(golden[f"tv_{name}"]), name


# 8 ---------------------------------------------------------------------------------------
def test_policy_equivalence_sweep(core, ops):
    """The sweep's tv is the single call's for each lottery.  The 0.05 is a sanity bound, not a
    tolerance: at 81 leaves and 20,000 samples the restatement on the host gives 0.0051, 0.0062
    and 0.0066 for the reference's lotteries of seed 42 at these three rhos (draws of seed 7;
    the lotteries sit on few leaves, a uniform one would give about 0.025)."""
    B, L, d, n_agents, n = 3, 4, 8, 6, 20_000
    rhos = np.linspace(0.6, 5.0, 20)[[0, 9, 19]]
    res = core.policy_equivalence_sweep(B, L, d, n_agents, [42], rhos, num_samples=n)
    assert res["tv"].shape == (1, 3) and np.array_equal(res["rho"], rhos)
    v, w = core.generate_params(B, L, d, n_agents, seed=42)
    ps = ops.nash_lottery(core.compute_utilities_fp64(v, w, rhos), max_iters=1500, tol=1e-11)["p"]
    leaves = core.enumerate_leaves(B, L)
    for k in range(3):
        _, tv = core.induced_policy_rollout(ps[k].cpu().numpy(), leaves, B, L, num_samples=n)
        print(f"rho {rhos[k]:.2f}: tv {res['tv'][0, k]:.6f}")
        assert res["tv"][0, k] == tv
        assert res["tv"][0, k] < 0.05
