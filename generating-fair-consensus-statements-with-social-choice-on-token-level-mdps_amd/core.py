"""Drop-in for the utility / welfare / lottery entry points of the reference's ``core.py``.

Same names, arguments and return types (NumPy in, NumPy out), but the per-step
log-softmax + gather and the per-leaf folding run on the GPU through the C-ABI
kernels (``ops.logsoftmax_gather`` -> ``ops.segment_reduce``), the point-mass
welfare / selection through ``ops.welfare`` / ``ops.topk``, the Nash-welfare
lottery and its induced policy through ``ops.nash_lottery`` / ``ops.lottery_policy``, the
maximin lottery and the coalition-improvement metric through ``ops.maximin_lottery``, and the
rollout of the induced policy through ``ops.policy_rollout``.

Reference (core.py):
  generate_params         49-56    (host RNG: parameters are inputs, not the hot path)
  enumerate_leaves        59-61
  log_softmax_rows        64-68    -> cs_logsoftmax_gather (k = vocab: full rows)
  compute_utilities       71-100   -> one batched launch over every (agent, leaf, step) row
  F_val                   108-113  (general lottery: host; point mass: point_mass_welfare)
  FW_nash_welfare         116-168  -> cs_nash_lottery (FW_nash_welfare_batch: a sweep per launch)
  build_prefix_index      287-294
  induced_policy_rollout  297-332  -> cs_lottery_policy tables (induced_policy), then
                                      cs_policy_rollout: the reference's own PCG64 draws, made on
                                      the GPU (induced_policy_rollout_batch: many lotteries per
                                      launch)
  main's sanity check     437-444  -> policy_equivalence_sweep: for every (seed, rho), not one
  utilitarian argmax      374-376  -> point_mass_select(U, "utilitarian")
  egalitarian_lottery     171-206  -> cs_maximin_lottery (all agents, base 1): one optimal vertex
  max_coalition_improvement 214-279 -> cs_maximin_lottery, every coalition's LP in one launch
                                      (max_coalition_improvement_batch: many problems per launch;
                                      maximin_certificate: the weak-duality bounds, host)
  main's sweep            340-435  -> coalition_sweep (the numbers, no plot): one cs_nash_lottery
                                      and one cs_maximin_lottery launch

The two LPs are one matrix game, solved by a dual simplex instead of HiGHS: the optimal values
agree with the reference's to its solver tolerance, the egalitarian lottery is an optimal vertex
but not necessarily the same one.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import torch

from . import ops


def _device() -> torch.device:
    return ops.default_device("core: the GPU path needs a HIP device (no CPU fallback)")


def generate_params(B, L, d, n_agents, seed=123):
    """Random unit token vectors v[t, a] and agent vectors w[i] (core.py:49-56 contract)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(L, B, d))
    v /= np.linalg.norm(v, axis=2, keepdims=True) + 1e-12
    w = rng.normal(size=(n_agents, d))
    w /= np.linalg.norm(w, axis=1, keepdims=True) + 1e-12
    return v, w


def enumerate_leaves(B, L):
    """All length-L action tuples in lexicographic order (core.py:59-61 contract)."""
    return list(itertools.product(range(B), repeat=L))


def log_softmax_rows(M):
    """Row-wise log-softmax of a 2-D array on the GPU (core.py:64-68 contract)."""
    M = np.asarray(M)
    dev = _device()
    X = torch.as_tensor(np.ascontiguousarray(M, dtype=np.float32), device=dev)
    n, B = X.shape
    tgt = torch.arange(B, dtype=torch.int32, device=dev).repeat(n, 1)
    out, _ = ops.logsoftmax_gather(X, tgt)
    return out.double().cpu().numpy()


def compute_utilities(v, w, rho):
    """Agent-by-leaf utilities U[i, j] (core.py:71-100 contract), returns (U, leaves).

    Every (agent i, leaf j, step t) logits row rho * w_i . (z_t(j) + v[t, b]) is
    built in one batched GEMM, the whole [n * B^L * L, B] block goes through one
    cs_logsoftmax_gather launch (target = a_t), and cs_segment_reduce folds the L
    steps of each (agent, leaf) — the sum of core.py:90.
    """
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    L, B, d = v.shape
    n = w.shape[0]
    leaves = enumerate_leaves(B, L)
    m = len(leaves)
    dev = _device()
    A = torch.as_tensor(np.array(leaves, dtype=np.int64), device=dev)          # [m, L]
    vt = torch.as_tensor(v, device=dev)                                         # [L, B, d]
    wt = torch.as_tensor(w, device=dev)                                         # [n, d]
    chosen = vt[torch.arange(L, device=dev)[None, :], A]                        # [m, L, d]
    z = torch.cumsum(chosen, dim=1) - chosen                                    # state before step t
    X = z[:, :, None, :] + vt[None, :, :, :]                                    # [m, L, B, d]
    logits = float(rho) * torch.einsum("id,mtbd->imtb", wt, X)                  # [n, m, L, B]
    logits = logits.reshape(n * m * L, B).to(torch.float32).contiguous()
    tgt = A[None, :, :].expand(n, m, L).reshape(-1, 1).to(torch.int32).contiguous()
    tok, _ = ops.logsoftmax_gather(logits, tgt)
    offs = torch.arange(0, n * m * L + 1, L, dtype=torch.int32, device=dev)
    seg = ops.segment_reduce(tok, offs)
    # fp32 segment sums carry fp64-accumulated values; finish the stabilisation in fp64
    logu = seg["sum_lp"].double().reshape(n, m)
    U = torch.exp(logu - logu.max(dim=1, keepdim=True).values) + 1e-300        # core.py:94-99
    return U.cpu().numpy(), leaves


def F_val(U, p):
    """Nash welfare of a lottery: sum_i log(U_i . p) (core.py:108-113 contract, host)."""
    a = np.asarray(U) @ np.asarray(p)
    if np.any(a <= 0):
        return -np.inf
    return float(np.sum(np.log(a)))


def FW_nash_welfare_batch(Us, max_iters=1000, tol=1e-10):
    """FW_nash_welfare of a list or stack of equal-shape problems [P, n, m] in ONE launch
    (one workgroup per problem); returns the lotteries [P, m]."""
    Us = np.ascontiguousarray(np.stack([np.asarray(U, dtype=np.float64) for U in Us]))
    if Us.ndim != 3:
        raise ops.CSError("FW_nash_welfare_batch takes equal-shape [n, m] problems")
    res = ops.nash_lottery(torch.as_tensor(Us, device=_device()), max_iters=max_iters, tol=tol)
    return res["p"].cpu().numpy()


def FW_nash_welfare(U, max_iters=1000, tol=1e-10):
    """The lottery maximising F(p) = sum_i log(U_i . p) over the simplex: Frank-Wolfe with a
    golden-section line search, on the GPU (core.py:116-168 contract), returns p [m]."""
    U = np.asarray(U, dtype=np.float64)
    if U.ndim != 2:
        raise ops.CSError("FW_nash_welfare takes U [n, m]")
    return FW_nash_welfare_batch(U[None], max_iters=max_iters, tol=tol)[0]


def nash_lottery_certificate(U, p):
    """(F, gap) of a lottery p: F = F_val(U, p) and the Frank-Wolfe gap max_j g_j - n with
    g_j = sum_i U[i, j] / (U p)_i.  F* - F(p) <= gap by concavity, so a small gap certifies p
    (host, as F_val)."""
    U = np.asarray(U, dtype=np.float64)
    a = U @ np.asarray(p, dtype=np.float64)
    if np.any(a <= 0):
        return -np.inf, np.inf
    return float(np.sum(np.log(a))), float((U / a[:, None]).sum(0).max() - U.shape[0])


MAX_COALITION_AGENTS = 16     # 2^16 - 1 = 65,535 coalitions (one workgroup each) per problem


@functools.lru_cache(maxsize=None)
def coalition_masks(n):
    """All 2^n - 1 nonempty coalitions of n agents as bit masks (bit i = agent i), in the
    reference's order: itertools.combinations by size (core.py:230-232)."""
    if not 1 <= n <= MAX_COALITION_AGENTS:
        raise ops.CSError(f"all coalitions are enumerated for at most {MAX_COALITION_AGENTS} agents "
                          f"(got {n}); pass coalitions= for a chosen few")
    out = [sum(1 << i for i in S) for r in range(1, n + 1)
           for S in itertools.combinations(range(n), r)]
    masks = np.array(out, dtype=np.uint64)
    masks.setflags(write=False)
    return masks


def _as_masks(coalitions, n):
    if coalitions is None:
        return coalition_masks(n)
    masks = []
    for S in coalitions:
        S = [int(i) for i in S]
        if not S or min(S) < 0 or max(S) >= n or len(set(S)) != len(S):
            raise ops.CSError(f"a coalition is a nonempty set of distinct agents below {n}, got {S}")
        masks.append(sum(1 << i for i in S))
    if not masks:
        raise ops.CSError("coalitions= needs at least one coalition")
    return np.array(masks, dtype=np.uint64)


def _checked(pivots, what):
    """Coalitions the kernel solved; one that ran out of pivots is an error, not a skip."""
    if bool((pivots == -2).any()):
        raise ops.CSError(f"{what}: a problem exhausted max_pivots (cs_maximin_lottery status -2)")
    return pivots >= 0


def egalitarian_lottery(U):
    """The maximin lottery argmax_p min_i U_i . p on the GPU (core.py:171-206 contract), returns
    p [m].  The LP's optimal value is unique, its p is not: this is one optimal vertex (that of a
    dual simplex with lowest-index ties), not necessarily the one HiGHS returns.  A malformed
    problem (a negative or non-finite utility, an all-zero agent) gets the uniform lottery, the
    reference's fallback for a failed solve."""
    U = np.asarray(U, dtype=np.float64)
    if U.ndim != 2:
        raise ops.CSError("egalitarian_lottery takes U [n, m]")
    res = ops.maximin_lottery(torch.as_tensor(np.ascontiguousarray(U), device=_device()),
                              with_lam=False)
    if not bool(_checked(res["pivots"], "egalitarian_lottery")):
        return np.ones(U.shape[1]) / U.shape[1]
    return res["q"].cpu().numpy()


def max_coalition_improvement_batch(Us, ps, coalitions=None):
    """max_coalition_improvement of equal-shape problems [P, n, m] with lotteries [P, m] in ONE
    launch (one workgroup per problem and coalition); returns the factors [P]."""
    Us = np.ascontiguousarray(np.stack([np.asarray(U, dtype=np.float64) for U in Us]))
    ps = np.stack([np.asarray(p, dtype=np.float64) for p in ps])
    if Us.ndim != 3 or ps.shape != (Us.shape[0], Us.shape[2]):
        raise ops.CSError("max_coalition_improvement_batch takes equal-shape [n, m] problems and "
                          "one lottery [m] each")
    masks = _as_masks(coalitions, Us.shape[1])
    dev = _device()
    base = np.stack([U @ p for U, p in zip(Us, ps)])          # core.py:226, problem by problem
    res = ops.maximin_lottery(torch.as_tensor(Us, device=dev), torch.as_tensor(base, device=dev),
                              masks, with_q=False, with_lam=False)
    ok = _checked(res["pivots"], "max_coalition_improvement")
    alpha = torch.where(ok, res["alpha"], torch.ones_like(res["alpha"]))
    return alpha.max(dim=1).values.clamp_min(1.0).cpu().numpy()


def max_coalition_improvement(U, p, coalitions=None):
    """The core-violation metric of a lottery p (core.py:214-279 contract): the largest alpha
    such that some coalition S can, with the share |S| / n of the probability, give every member
    at least alpha times its utility under p; > 1 means p is blockable.  All 2^n - 1 coalitions
    (n <= 16), or the given ``coalitions`` (iterables of agent indices), as one launch, one LP
    each.  The maximum starts from 1.0; a coalition with a member of zero (or non-finite) base
    utility is skipped, as the reference skips its unbounded LP.  Returns a float."""
    U = np.asarray(U, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if U.ndim != 2 or p.shape != (U.shape[1],):
        raise ops.CSError("max_coalition_improvement takes U [n, m] and p [m]")
    return float(max_coalition_improvement_batch(U[None], p[None], coalitions)[0])


def maximin_certificate(U, q, lam, S=None, base=None):
    """(lower, upper) of a lottery q and weights lam on the agents for coalition S (None: all)
    and ``base`` (None: ones): lower = min_{i in S} (U_i . q) / base_i, upper = max_j sum_i lam_i
    U[i, j] / base_i.  lower <= value <= upper by weak duality (lam >= 0 summing to 1 on S), so
    equal bounds certify both (host, as nash_lottery_certificate)."""
    U = np.asarray(U, dtype=np.float64)
    S = list(range(U.shape[0])) if S is None else [int(i) for i in S]
    b = np.ones(U.shape[0]) if base is None else np.asarray(base, dtype=np.float64)
    M = U[S] / b[S, None]
    return float((M @ np.asarray(q, dtype=np.float64)).min()), \
        float((np.asarray(lam, dtype=np.float64)[S] @ M).max())


def compute_utilities_fp64(v, w, rhos):
    """compute_utilities for every rho of ``rhos`` with fp64 log-softmax steps (torch on the
    device), returns U [len(rhos), n, m].  The coalition metric divides by utilities, so its
    sweep needs them to more digits than the fp32 rows of cs_logsoftmax_gather carry."""
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    L, B, d = v.shape
    dev = _device()
    A = torch.as_tensor(np.array(enumerate_leaves(B, L), dtype=np.int64), device=dev)   # [m, L]
    vt = torch.as_tensor(v, device=dev)
    wt = torch.as_tensor(w, device=dev)
    rt = torch.as_tensor(np.asarray(rhos, dtype=np.float64).reshape(-1), device=dev)
    chosen = vt[torch.arange(L, device=dev)[None, :], A]                         # [m, L, d]
    z = torch.cumsum(chosen, dim=1) - chosen
    X = z[:, :, None, :] + vt[None, :, :, :]                                     # [m, L, B, d]
    logits = rt[:, None, None, None, None] * torch.einsum("id,mtbd->imtb", wt, X)[None]
    ls = torch.log_softmax(logits, dim=-1)                                       # [R, n, m, L, B]
    idx = A[None, None, :, :, None].expand(ls.shape[0], ls.shape[1], -1, -1, 1)
    logu = ls.gather(-1, idx).squeeze(-1).sum(dim=-1)                            # [R, n, m]
    return torch.exp(logu - logu.max(dim=2, keepdim=True).values) + 1e-300       # core.py:94-99


def sweep_lotteries(Us, max_iters=1500, tol=1e-11):
    """The three lotteries the reference's sweep evaluates on every problem of Us [P, n, m]
    (device): the Nash-welfare lottery (one cs_nash_lottery launch), the utilitarian point mass
    and the uniform lottery (core.py:369-376).  Returns the problems three times over,
    U3 [3 * P, n, m] in that order of lotteries, and base [3 * P, n] = U p."""
    P, _, m = Us.shape
    p_nw = ops.nash_lottery(Us, max_iters=max_iters, tol=tol)["p"]
    p_util = torch.zeros_like(p_nw)
    p_util[torch.arange(P, device=Us.device), Us.sum(dim=1).argmax(dim=1)] = 1.0
    ps = torch.cat([p_nw, p_util, torch.full_like(p_nw, 1.0 / m)])
    U3 = Us.repeat(3, 1, 1)
    return U3, torch.einsum("pij,pj->pi", U3, ps)


def coalition_sweep(B, L, d, n_agents, seeds, rho_grid, max_iters=1500, tol=1e-11):
    """The numbers of the reference's experiment (core.py:340-435, no plotting): for every seed
    and rho, the max coalition improvement of the Nash-welfare lottery, of the utilitarian point
    mass and of the uniform lottery.  One cs_nash_lottery launch and one cs_maximin_lottery
    launch for the whole sweep.  Returns {"seeds", "rho", "nash", "utilitarian", "uniform"},
    the last three [len(seeds), len(rho_grid)]."""
    seeds = [int(s) for s in seeds]
    rho_grid = np.asarray(rho_grid, dtype=np.float64).reshape(-1)
    masks = coalition_masks(int(n_agents))
    Us = []
    for seed in seeds:
        v, w = generate_params(B, L, d, n_agents, seed=seed)
        Us.append(compute_utilities_fp64(v, w, rho_grid))
    U3, base = sweep_lotteries(torch.cat(Us).contiguous(), max_iters, tol)       # [3 * S * R, ..]
    res = ops.maximin_lottery(U3, base, masks, with_q=False, with_lam=False)
    ok = _checked(res["pivots"], "coalition_sweep")
    alpha = torch.where(ok, res["alpha"], torch.ones_like(res["alpha"]))
    top = alpha.max(dim=1).values.clamp_min(1.0).reshape(3, len(seeds), rho_grid.size).cpu().numpy()
    return {"seeds": np.array(seeds), "rho": rho_grid, "nash": top[0], "utilitarian": top[1],
            "uniform": top[2]}


def induced_policy(p, B, L):
    """The token policy a lottery over the B^L leaves (lexicographic order) induces, on the GPU:
    a list over the levels t = 0..L-1 of tables [B^t, B] with pi[t][s, b] = mass(s + b) / mass(s),
    s the prefix's index in base B; a prefix of mass <= 0 has the uniform 1/B (core.py:303-325)."""
    pt = torch.as_tensor(np.ascontiguousarray(p, dtype=np.float64), device=_device())
    if pt.dim() != 1:
        raise ops.CSError("induced_policy takes one lottery p [B^L]")
    return [t.cpu().numpy() for t in ops.lottery_policy(pt, B, L)]


def build_prefix_index(leaves):
    """prefix tuple -> indices of the leaves that start with it (core.py:287-294 contract)."""
    index = {}
    for j, leaf in enumerate(leaves):
        leaf = tuple(leaf)
        for t in range(len(leaf) + 1):
            index.setdefault(leaf[:t], []).append(j)
    return index


def _rollout_tv(pt, B, L, num_samples, states, what):
    """(p_hat [P, m], tv [P]) of the lotteries pt [P, m] (device): one cs_lottery_policy and one
    cs_policy_rollout launch, then the frequencies and distances one lottery at a time on 1-D
    arrays, the reference's own expressions (core.py:330-331; a sum over an axis of a 2-D array
    adds in another order)."""
    res = ops.policy_rollout(ops.lottery_policy(pt, B, L, flat=True), B, L, states, num_samples)
    if bool((res["status"] != 0).any()):
        raise ops.CSError(f"{what}: a lottery's induced policy is not a policy (negative or "
                          "non-finite mass; cs_policy_rollout status -1)")
    counts = res["counts"].cpu().numpy()
    ps = pt.cpu().numpy()
    p_hat = np.empty(ps.shape, dtype=np.float64)
    tv = np.empty(ps.shape[0], dtype=np.float64)
    for k in range(ps.shape[0]):
        p_hat[k] = counts[k] / counts[k].sum()
        tv[k] = 0.5 * np.sum(np.abs(p_hat[k] - ps[k]))
    return p_hat, tv


def induced_policy_rollout_batch(ps, B, L, num_samples=200_000, seeds=7):
    """induced_policy_rollout of the lotteries ps [P, m] in one cs_lottery_policy and one
    cs_policy_rollout launch; ``seeds`` is one seed for all or one per lottery.  Every lottery
    gets the draws of its own ``default_rng(seed)``, so each row is what the single call returns.
    Returns (p_hat [P, m], tv [P])."""
    ps = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in ps]))
    if ps.ndim != 2:
        raise ops.CSError("induced_policy_rollout_batch takes lotteries [P, m]")
    if np.ndim(seeds) == 0:
        seeds = [seeds] * ps.shape[0]
    if len(seeds) != ps.shape[0]:
        raise ops.CSError("induced_policy_rollout_batch takes one seed, or one per lottery")
    states = np.stack([ops.pcg64_state(int(s)) for s in seeds])
    return _rollout_tv(torch.as_tensor(ps, device=_device()), B, L, num_samples, states,
                       "induced_policy_rollout")


def induced_policy_rollout(p_star, leaves, B, L, num_samples=200_000, seed=7):
    """Sample leaves step by step from the policy p_star induces and compare their frequencies
    with p_star (core.py:297-332 contract): returns (p_hat, TV = 0.5 * |p_hat - p_star|_1).

    The step probabilities come from induced_policy's tables; the draws are the reference's
    sequence of ``default_rng(seed).choice(B, p=probs)`` calls, made by cs_policy_rollout."""
    p_star = np.asarray(p_star, dtype=np.float64)
    leaves = [tuple(int(a) for a in leaf) for leaf in leaves]
    if leaves != enumerate_leaves(B, L):
        raise ops.CSError("induced_policy_rollout needs the leaves of enumerate_leaves(B, L)")
    p_hat, tv = induced_policy_rollout_batch(p_star[None], B, L, num_samples, seed)
    return p_hat[0], tv[0]


def policy_equivalence_sweep(B, L, d, n_agents, seeds, rho_grid, num_samples=200_000, seed=7,
                             max_iters=1500, tol=1e-11):
    """The reference's policy-lottery sanity check (core.py:437-444) for every (seed, rho) of the
    sweep instead of one: the Nash-welfare lottery of each problem (one cs_nash_lottery launch),
    the policies they induce (one cs_lottery_policy launch) and a rollout of ``num_samples``
    leaves each with the draws of ``default_rng(seed)`` (one cs_policy_rollout launch).
    Returns {"seeds", "rho", "tv" [len(seeds), len(rho_grid)]}."""
    seeds = [int(s) for s in seeds]
    rho_grid = np.asarray(rho_grid, dtype=np.float64).reshape(-1)
    Us = []
    for s in seeds:
        v, w = generate_params(B, L, d, n_agents, seed=s)
        Us.append(compute_utilities_fp64(v, w, rho_grid))
    Us = torch.cat(Us).contiguous()                                              # [S * R, n, m]
    p_nw = ops.nash_lottery(Us, max_iters=max_iters, tol=tol)["p"]
    states = np.tile(ops.pcg64_state(seed), (Us.shape[0], 1))
    _, tv = _rollout_tv(p_nw, B, L, num_samples, states, "policy_equivalence_sweep")
    return {"seeds": np.array(seeds), "rho": rho_grid, "tv": tv.reshape(len(seeds), rho_grid.size)}


_KIND = {"nash": "sumlog", "utilitarian": "sum", "egalitarian": "min"}


def point_mass_welfare(U, kind="nash", eps=0.0):
    """Welfare of every point-mass lottery e_j, i.e. per column of U [n, m], on the GPU.

    nash        -> sum_i log(U[i, j])   (= F_val(U, e_j), core.py:108-113)
    utilitarian -> sum_i U[i, j]        (core.py:374)
    egalitarian -> min_i U[i, j]
    """
    dev = _device()
    Ut = torch.as_tensor(np.ascontiguousarray(U, dtype=np.float32), device=dev)
    tiny = float(np.finfo(np.float32).tiny) if eps == 0.0 else float(eps)
    return ops.welfare(Ut, _KIND.get(kind, kind), eps=tiny).double().cpu().numpy()


def point_mass_select(U, kind="utilitarian"):
    """argmax_j of the point-mass welfare, first index on ties (np.argmax, core.py:374)."""
    dev = _device()
    Ut = torch.as_tensor(np.ascontiguousarray(U, dtype=np.float32), device=dev)
    W = ops.welfare(Ut, _KIND.get(kind, kind), eps=float(np.finfo(np.float32).tiny))
    idx, _ = ops.topk(W, 1)
    return int(idx.item())
