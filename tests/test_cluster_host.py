"""CPU tests of the clustering step: the NumPy restatement (tests/kmeans_ref.py, the expected
values of the GPU tests) is pinned to what scikit-learn and the reference's
data/cluster_habermas_issues.py returned (tests/golden/cluster_golden.npz, written by
tests/golden/make_cluster_golden.py), the file writers equal the reference's text byte for byte,
and the cs_kmeans_* / cs_standardize / cs_nearest_rows entry points refuse bad arguments with a
status and a message before any launch.

Labels, iteration counts and seed rows are compared exactly.  Centres agree within
8 n 2^-53 max|Z| and the inertia within 4 n d 2^-53 relative: bounds on what the order of an fp64
sum over n points (n d terms) can move, not fits (measured values: profiles/cluster_parity.jsonl).
"""
import ctypes
import os
from importlib import import_module

import numpy as np
import pytest

import kmeans_ref as kr


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cluster_golden.npz"))


@pytest.fixture(scope="module")
def fits(golden):
    """The restatement's fit of every golden case, computed once."""
    out = []
    for i in range(int(golden["cases"])):
        g = lambda k: golden[f"c{i}_{k}"]                     # noqa: E731
        init = golden[f"c{i}_init"] if f"c{i}_init" in golden else None
        z = golden[f"z_{str(g('input'))}"]
        out.append((z, kr.fit(z, int(g("k")), int(g("seed")), int(g("n_init")), int(g("max_iter")),
                              float(g("tol")), init=init)))
    return out


def test_scaler_equals_standard_scaler(golden):
    for name in "abc":
        z, mean, scale = kr.standardize(golden[f"x_{name}"])
        assert np.array_equal(z, golden[f"z_{name}"]), name
        assert np.array_equal(mean, golden[f"mean_{name}"]), name
        assert np.array_equal(scale, golden[f"scale_{name}"]), name
    assert golden["scale_c"][11] == 1.0 and (golden["z_c"][:, 11] == 0).all()   # constant feature
    assert [golden[f"x_{n}"].shape for n in "abc"] == [(40, 3), (300, 32), (97, 33)]


def test_restatement_equals_every_golden_entry(golden, fits):
    assert int(golden["cases"]) == 33
    worst_c = worst_i = 0.0
    for i, (z, f) in enumerate(fits):
        g = lambda k: golden[f"c{i}_{k}"]                     # noqa: E731
        assert float(g("narrowest")) >= 1e-9 and f["narrowest"] >= 1e-9, i
        assert np.array_equal(f["labels"], g("labels")), i
        assert int(f["n_iter"][f["best"]]) == int(g("n_iter")), i
        if f"c{i}_indices" in golden:
            assert np.array_equal(f["indices"], g("indices")), i
        err_c = float(np.abs(f["centers"] - g("centers")).max())
        err_i = abs(f["inertia"][f["best"]] - float(g("inertia"))) / float(g("inertia"))
        print(f"case {i}: centres {err_c:.2e} (bound {kr.center_bound(z):.2e}), "
              f"inertia {err_i:.2e} (bound {kr.inertia_bound(z):.2e})")
        assert err_c <= kr.center_bound(z), i
        assert err_i <= kr.inertia_bound(z), i
        worst_c, worst_i = max(worst_c, err_c), max(worst_i, err_i)
    print(f"worst: centres {worst_c:.2e}, inertia {worst_i:.2e}")


def test_golden_covers_both_loose_exits_and_relocation(golden, fits):
    cases = {i: {k: golden[f"c{i}_{k}"] for k in ("input", "k", "max_iter", "tol")}
             for i in range(int(golden["cases"]))}
    loose_tol = [i for i, c in cases.items() if float(c["tol"]) == 0.5]
    short = [i for i, c in cases.items() if int(c["max_iter"]) == 2]
    assert len(loose_tol) == 1 and len(short) == 1
    # the tolerance ends restarts whose labels still moved; so does max_iter
    assert (fits[loose_tol[0]][1]["done"] == 2).any()
    f = fits[short[0]][1]
    assert ((f["done"] == 2) & (f["n_iter"] == 2)).any()
    planted = [i for i in cases if f"c{i}_init" in golden]
    assert len(planted) == 4
    empties = []
    for i in planted:
        z = golden[f"z_{str(cases[i]['input'])}"]
        mean = z.mean(axis=0)
        first = kr.lloyd_step(z - mean, golden[f"c{i}_init"] - mean)[0]
        empties.append(int(cases[i]["k"]) - len(set(first.tolist())))
    assert sorted(empties) == [1, 1, 2, 2]


def test_predraw_is_what_kmeans_consumed(golden, fits, pkg):
    """The rows of the k-means++ seeds come out of the draws alone; the package's predraw is the
    restatement's, and a RandomState passed in is advanced exactly as an int seed's is."""
    cl = import_module(pkg.__name__ + ".clustering")
    for i, (z, f) in enumerate(fits):
        if f"c{i}_indices" not in golden:
            continue
        k, seed = int(golden[f"c{i}_k"]), int(golden[f"c{i}_seed"])
        first, u = kr.predraw(seed, len(z), k, 10)
        assert np.array_equal(first, golden[f"c{i}_indices"][:, 0]), i
        f2, u2 = cl.predraw(np.random.RandomState(seed), len(z), k, 10)
        assert np.array_equal(first, f2) and np.array_equal(u, u2), i
        assert u.shape == (10, k - 1, 2 + int(np.log(k))) and (u >= 0).all() and (u < 1).all()


def test_reference_pipeline_is_a_golden_case(golden, fits):
    """cluster_embeddings(x, 5, 43) of the reference is KMeans(5, random_state=43, n_init=10) on
    the scaled input; its centroid issues compare those centres with the RAW embeddings."""
    for name in "abc":
        i = [j for j in range(int(golden["cases"])) if str(golden[f"c{j}_input"]) == name
             and int(golden[f"c{j}_k"]) == 5 and int(golden[f"c{j}_seed"]) == 43
             and float(golden[f"c{j}_tol"]) == 1e-4 and int(golden[f"c{j}_max_iter"]) == 300][0]
        assert np.array_equal(golden[f"ref_{name}_labels"], fits[i][1]["labels"])
        assert np.abs(golden[f"ref_{name}_centers"] - fits[i][1]["centers"]).max() <= \
            kr.center_bound(fits[i][0])
        idx, _ = kr.nearest_rows(golden[f"ref_{name}_centers"], golden[f"x_{name}"])
        assert np.array_equal(idx, golden[f"ref_{name}_centroids"]), name


def issue_info(n):
    return [{"issue": f"issue {j}: {'yes, no' if j % 7 == 0 else 'plain'}",
             "num_opinions": j % 5 + 1} for j in range(n)]


def test_file_formats_equal_the_references(golden, pkg, tmp_path):
    cl = import_module(pkg.__name__ + ".clustering")
    for name in "abc":
        labels = golden[f"ref_{name}_labels"]
        info = issue_info(len(labels))
        cents = [info[int(j)] for j in golden[f"ref_{name}_centroids"]]
        path = tmp_path / f"{name}.csv"
        cl.save_cluster_results(info, labels, cents, str(path))
        assert path.read_bytes() == str(golden[f"ref_{name}_csv"]).encode(), name

    def opinions(issue):
        return ["first view", "No opinion was provided.", None, "first view", 'a "quoted", view'], \
            "we agree"

    cents = issue_info(3)[:2]
    cl.save_centroid_issues_to_file(cents, str(tmp_path / "c.csv"), str(tmp_path / "c.txt"),
                                    opinions_for_issue=opinions)
    assert (tmp_path / "c.csv").read_text() == 'cluster,issue\n0,"issue 0: yes, no"\n1,issue 1: plain\n'
    block = ("CLUSTER {n}\n" + "=" * 50 + "\n\nISSUE:\n{issue}\n\nOPINIONS (2):\n1. first view\n\n"
             '2. a "quoted", view\n\nCONSENSUS STATEMENT:\nwe agree\n\n\n\n')
    assert (tmp_path / "c.txt").read_text() == \
        block.format(n=1, issue=cents[0]["issue"]) + block.format(n=2, issue=cents[1]["issue"])
    data = [{"issue": "x", "embedding": [1.0, 2.0]}, {"issue": "y", "embedding": None},
            {"issue": "z", "embedding": [0.5, 0.25]}]
    E, info = cl.extract_embeddings(data, max_opinions=1, opinions_for_issue=lambda s:
                                    ["one"] if s == "x" else ["one", "two"])
    assert E.tolist() == [[1.0, 2.0]] and info == [{"issue": "x", "num_opinions": 1}]
    cl.save_progress(data, str(tmp_path / "e.json"), str(tmp_path / "e.csv"))
    assert (tmp_path / "e.csv").read_text() == "issue,has_embedding\nx,True\ny,False\nz,True\n"
    assert cl.load_issue_embeddings(str(tmp_path / "e.json")) == data
    assert cl.load_issue_embeddings(str(tmp_path / "missing.json")) == []


def test_same_clustering_and_relocation_rules():
    assert kr.same_clustering([0, 0, 1, 2], [2, 2, 0, 1], 3)
    assert not kr.same_clustering([0, 0, 1, 2], [2, 1, 0, 1], 3)
    # relocation: the farthest point first, the lower index among equal distances
    Z = np.array([[0.0], [1.0], [5.0], [5.0], [-3.0]])
    labels = np.array([0, 0, 0, 0, 0], dtype=np.int32)
    sums, counts = np.array([[8.0], [0.0], [0.0]]), np.array([5, 0, 0])
    kr.relocate(Z, labels, (Z[:, 0] - 1.6) ** 2, sums, counts)
    assert counts.tolist() == [3, 1, 1] and sums[:, 0].tolist() == [6.0, -3.0, 5.0]
    with pytest.raises(ValueError, match="n_samples=2 should be >= n_clusters=3"):
        kr.fit(np.zeros((2, 2)), 3)


def _lib(pkg):
    return import_module(pkg.__name__ + "._lib").load()


def test_entry_points_refuse_bad_arguments(pkg):
    L = _lib(pkg)
    lib = import_module(pkg.__name__ + "._lib")
    d, odd, big = ctypes.c_void_p(256), ctypes.c_void_p(258), 1 << 40
    n, dim, k, R, T = 100, 8, 5, 3, 3
    first = np.array([0, 5, 99], dtype=np.int32)
    u = np.full((R, k - 1, T), 0.5)

    def seed(Z=d, ld=dim, n=n, dim=dim, k=k, R=R, T=T, fh=first, uh=u, fd=d, ud=d, cen=d, idx=d,
             ws=d, wsb=big):
        return L.cs_kmeans_seed(Z, ld, n, dim, k, R, T, fh.ctypes.data if fh is not None else None,
                                uh.ctypes.data if uh is not None else None, fd, ud, cen, idx, ws,
                                wsb, None)

    bad_u, neg_u, nan_u, bad_first = u.copy(), u.copy(), u.copy(), first.copy()
    bad_u[2, 3, 1], neg_u[0, 0, 0], nan_u[1, 1, 1], bad_first[1] = 1.0, -1e-9, np.nan, n
    for bad in (dict(Z=None), dict(cen=None), dict(idx=None), dict(fd=None), dict(ud=None),
                dict(fh=None), dict(uh=None), dict(Z=odd), dict(ld=dim - 1), dict(k=n + 1),
                dict(k=lib.KMEANS_MAX_K + 1, n=1000), dict(dim=lib.KMEANS_MAX_D + 1, ld=1 << 20),
                dict(n=lib.KMEANS_MAX_N + 1), dict(R=lib.KMEANS_MAX_R + 1), dict(R=0), dict(n=0),
                dict(T=0), dict(T=9), dict(uh=bad_u), dict(uh=neg_u), dict(uh=nan_u),
                dict(fh=bad_first)):
        assert seed(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_kmeans_seed: "), bad
    assert seed(ws=None) == -2 and seed(wsb=16) == -2
    ws = L.cs_kmeans_workspace_size(n, dim, k, R)
    assert ws > 0 and L.cs_kmeans_workspace_size(n, dim, 65, R) == 0
    assert seed(wsb=ws - 1) == -2

    def iterate(Z=d, ld=dim, n=n, k=k, R=R, cen=d, state=d, steps=1, max_iter=300, ws=d):
        return L.cs_kmeans_iterate(Z, ld, n, dim, k, R, cen, state, steps, max_iter, ws, big, None)

    for bad in (dict(Z=None), dict(cen=None), dict(state=None), dict(ld=dim - 1), dict(k=n + 1),
                dict(k=65), dict(R=1025), dict(steps=-1), dict(max_iter=0), dict(state=odd)):
        assert iterate(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_kmeans_iterate: "), bad
    assert iterate(ws=None) == -2
    assert L.cs_kmeans_init(d, dim, n, dim, k, R, -1.0, d, d, big, None) == -1
    assert L.cs_kmeans_init(d, dim, n, dim, k, R, 1e-4, None, d, big, None) == -1
    assert L.cs_kmeans_init(d, dim - 1, n, dim, k, R, 1e-4, d, d, big, None) == -1

    def finish(Z=d, ld=dim, k=k, R=R, n_init=R, cen=d, mean=None, state=d, best=d, labels=d,
               out_c=d, inertia=d, n_iter=d):
        return L.cs_kmeans_finish(Z, ld, n, dim, k, R, n_init, cen, mean, state, best, labels, out_c,
                                  inertia, n_iter, d, big, None)

    for bad in (dict(Z=None), dict(cen=None), dict(state=None), dict(best=None), dict(labels=None),
                dict(out_c=None), dict(inertia=None), dict(n_iter=None), dict(ld=dim - 1),
                dict(n_init=2), dict(n_init=0), dict(k=n + 1), dict(mean=odd)):
        assert finish(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_kmeans_finish: "), bad

    def std(X=d, ldx=dim, n=n, dim=dim, Z=d, ldz=dim, mean=d, scale=d, ws=d):
        return L.cs_standardize(X, ldx, n, dim, Z, ldz, mean, scale, ws, big, None)

    for bad in (dict(X=None), dict(Z=None), dict(mean=None), dict(scale=None), dict(ldx=dim - 1),
                dict(ldz=dim - 1), dict(n=0), dict(n=lib.KMEANS_MAX_N + 1), dict(dim=4097, ldx=8192,
                                                                              ldz=8192), dict(X=odd)):
        assert std(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_standardize: "), bad
    assert std(ws=None) == -2

    def near(Q=d, ldq=dim, q=4, X=d, ldx=dim, n=n, idx=d, dist=d, ws=d):
        return L.cs_nearest_rows(Q, ldq, q, X, ldx, n, dim, idx, dist, ws, big, None)

    for bad in (dict(Q=None), dict(X=None), dict(idx=None), dict(dist=None), dict(ldq=dim - 1),
                dict(ldx=dim - 1), dict(q=0), dict(n=0), dict(n=lib.KMEANS_MAX_N + 1), dict(idx=odd)):
        assert near(**bad) == -1, bad
        assert L.cs_last_error().decode().startswith("cs_nearest_rows: "), bad
    assert near(ws=None) == -2
    # the sizes are stated once: the header, _lib.py, the kernels' constants, the restatement
    header = open(os.path.join(os.path.dirname(__file__), "..", "include",
                               "consensus_scoring.h")).read()
    for name, v in (("K", kr.MAX_K), ("D", kr.MAX_D), ("N", kr.MAX_N), ("R", kr.MAX_R)):
        assert f"#define CS_KMEANS_MAX_{name} {v}\n" in header
        assert getattr(lib, "KMEANS_MAX_" + name) == v
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "cluster.hip")).read()
    assert (lib.KMEANS_TILE, lib.KMEANS_CHUNK, lib.KMEANS_SEG) == (kr.TILE, kr.CHUNK, kr.SEG)
    assert f"kKmTile = {kr.TILE};" in src and f"kKmChunk = {kr.CHUNK};" in src
    assert f"kKmSeg = {kr.SEG};" in src


def test_ops_and_drop_ins_check_their_arguments(pkg, ops):
    import torch
    cl = import_module(pkg.__name__ + ".clustering")
    with pytest.raises(ops.CSError, match="no CPU path"):
        ops.standardize(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ops.CSError, match="no CPU path"):
        ops.nearest_rows(torch.zeros(2, 3), torch.zeros(4, 3))
    with pytest.raises(ops.CSError):
        ops.standardize(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ops.CSError):
        ops.kmeans(torch.zeros(4, 3, dtype=torch.int32), 2, [0], np.zeros((1, 1, 2)))
    assert [ops.kmeans_trials(k) for k in (1, 2, 3, 5, 8, 20, 21, 64)] == [2, 2, 3, 3, 4, 4, 5, 6]
    with pytest.raises(ValueError, match="n_samples=3 should be >= n_clusters=5"):
        cl.cluster_embeddings(np.zeros((3, 4)), 5, 43)
    with pytest.raises(ValueError):
        cl.cluster_embeddings(np.zeros(7), 2)
    with pytest.raises(ValueError):
        cl.find_cluster_centroids(np.zeros((3, 4)), [{}] * 3, [0, 0, 0], np.zeros((1, 4)),
                                  space="whitened")
