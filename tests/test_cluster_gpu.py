"""GPU tests of the clustering step (csrc/cluster.hip through ops.standardize / kmeans_seed /
kmeans / nearest_rows and the clustering module's drop-ins) against the NumPy restatement
(tests/kmeans_ref.py), which tests/test_cluster_host.py pins to scikit-learn and the reference.

Labels, iteration counts, exits, seed rows and the chosen restart are compared exactly; centres
within 8 n 2^-53 max|Z| and inertias within 4 n d 2^-53 relative (summation-order bounds, not
fits).  The shapes sit on the kernels' edges: the point tile (64), the feature chunk (32), the
sum segment (128), both sides of the register / LDS path of the cluster sums (k = 8, 9), k from
1 to the limit of 64, n == k, duplicated rows, a constant feature."""
import json
import os
from importlib import import_module

import numpy as np
import pytest

import kmeans_ref as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cluster_golden.npz"))


@pytest.fixture(scope="module")
def cl(pkg):
    return import_module(pkg.__name__ + ".clustering")


def data(n, d, seed, blobs=4):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(blobs, d)) * 2.0
    return centres[rng.integers(0, blobs, n)] + rng.normal(size=(n, d))


def to_dev(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def gpu_fit(ops, dev, z, k, seed=None, n_init=10, init=None, **kw):
    if init is not None:
        got = ops.kmeans(to_dev(z, dev), k, init=to_dev(init, dev), **kw)
    else:
        first, u = kr.predraw(seed, len(z), k, n_init)
        got = ops.kmeans(to_dev(z, dev), k, first, u, **kw)
    return {key: (v.cpu().numpy() if hasattr(v, "cpu") else v) for key, v in got.items()}


def check_fit(got, want, z, what="", zero_inertia=False):
    assert np.array_equal(got["indices"], want["indices"]), what
    assert np.array_equal(got["n_iter"], want["n_iter"]), what
    assert np.array_equal(got["done"], want["done"]), what
    assert int(got["best"][0]) == want["best"], what
    assert np.array_equal(got["labels"][0], want["labels"]), what
    err_c = float(np.abs(got["centers"][0] - want["centers"]).max())
    if zero_inertia:
        # every point sits on its centre up to the rounding of sum * (1 / count): both inertias
        # are sums of n d squares of a few ulps of max|z|, and a relative comparison says nothing
        tiny = z.size * (8 * 2.0 ** -53 * float(np.abs(z).max())) ** 2
        assert got["inertia"].max() <= tiny and want["inertia"].max() <= tiny, what
        err_i = 0.0
    else:
        err_i = float((np.abs(got["inertia"] - want["inertia"]) / want["inertia"]).max())
    print(f"{what}: centres {err_c:.2e} (bound {kr.center_bound(z):.2e}), inertia {err_i:.2e} "
          f"(bound {kr.inertia_bound(z):.2e}), narrowest margin {want['narrowest']:.1e}")
    assert err_c <= kr.center_bound(z), what
    assert err_i <= kr.inertia_bound(z), what
    return err_c, err_i


def test_standardize_edges(ops, dev):
    """n below / at / above the row partial of a column sum, d = 1, 33; a constant feature and a
    feature whose mean dwarfs its spread."""
    for n, d in ((1, 1), (63, 1), (256, 33), (257, 33), (1000, 64)):
        x = data(n, d, 100 + n)
        if d > 2:
            x[:, 1] = -7.5                         # constant: scale 1, z 0
            x[:, 2] = 1e6 + x[:, 2]                # large mean
        want_z, want_m, want_s = kr.standardize(x)
        z, m, s = (t.cpu().numpy() for t in ops.standardize(to_dev(x, dev)))
        ax = float(np.abs(x).max())
        b_mean = 2 * n * 2.0 ** -53 * ax           # a sum of n terms of size <= ax, over n
        assert np.abs(m - want_m).max() <= b_mean, (n, d)
        if d > 2:
            assert s[1] == 1.0 and (z[:, 1] == 0).all()
        if n == 1:
            assert (s == 1.0).all() and (z == 0).all()
            continue
        # scale: sums of n squared deviations, each deviation carrying the rounding of a value of
        # size ax against a spread of size scale; z = (x - mean) / scale inherits both errors
        b_rel = 4 * n * 2.0 ** -53 * max(1.0, ax / float(want_s.min()))
        assert (np.abs(s - want_s) / want_s).max() <= b_rel, (n, d)
        b_z = b_mean / float(want_s.min()) + float(np.abs(want_z).max()) * b_rel
        print(f"n {n} d {d}: mean {np.abs(m - want_m).max():.1e} ({b_mean:.1e}) scale "
              f"{(np.abs(s - want_s) / want_s).max():.1e} ({b_rel:.1e}) z "
              f"{np.abs(z - want_z).max():.1e} ({b_z:.1e})")
        assert np.abs(z - want_z).max() <= b_z, (n, d)
    z32, _, _ = ops.standardize(to_dev(x.astype(np.float32), dev))
    assert z32.dtype.is_floating_point and z32.element_size() == 8   # widened, computed in fp64


@pytest.mark.parametrize("n,d,k,n_init", [
    (63, 1, 2, 3), (64, 33, 5, 3), (65, 33, 8, 3), (257, 5, 1, 2), (300, 33, 64, 2),
    (64, 3, 64, 2), (130, 7, 9, 2), (1000, 64, 8, 10)])
def test_seed_and_fit_equal_the_restatement(ops, dev, n, d, k, n_init):
    z = kr.standardize(data(n, d, 7 * n + d + k))[0]
    want = kr.fit(z, k, 43, n_init)
    if n > k:                               # n == k: every point its own centre, nothing to decide
        assert want["narrowest"] >= 1e-9, "an ambiguous case: choose other data, not a wider bound"
    # the seeding alone, on the centred data
    zc = z - z.mean(axis=0)
    first, u = kr.predraw(43, n, k, n_init)
    centers, indices = ops.kmeans_seed(to_dev(zc, dev), k, first, u)
    assert np.array_equal(indices.cpu().numpy(), want["indices"])
    assert np.array_equal(centers.cpu().numpy(), zc[want["indices"]])
    got = gpu_fit(ops, dev, z, k, 43, n_init)
    check_fit(got, want, z, f"n {n} d {d} k {k}", zero_inertia=n == k)
    if n_init == 10:
        assert len(set(want["n_iter"].tolist())) > 1      # restarts that finish at different times


def test_duplicated_rows_and_more_clusters_than_points(ops, dev):
    rng = np.random.default_rng(5)
    base = rng.normal(size=(20, 6))
    z = base[rng.integers(0, 20, 90)]
    for k in (5, 24):                       # 24 > 20 distinct rows: clusters stay empty
        want = kr.fit(z, k, 42, 4)
        got = gpu_fit(ops, dev, z, k, 42, 4)
        check_fit(got, want, z, f"duplicates k {k}", zero_inertia=k == 24)
    assert len(set(want["labels"].tolist())) < 24


def test_loose_exits_and_planted_empty_clusters_equal_golden(ops, dev, golden):
    rows = []
    for i in range(27, int(golden["cases"])):
        g = lambda key: golden[f"c{i}_{key}"]                 # noqa: E731
        z = golden[f"z_{str(g('input'))}"]
        init = golden[f"c{i}_init"] if f"c{i}_init" in golden else None
        kw = dict(max_iter=int(g("max_iter")), tol=float(g("tol")))
        want = kr.fit(z, int(g("k")), int(g("seed")), int(g("n_init")), init=init, **kw)
        got = gpu_fit(ops, dev, z, int(g("k")), int(g("seed")), int(g("n_init")), init=init, **kw)
        err_c, err_i = check_fit(got, want, z, f"golden case {i}")
        assert np.array_equal(got["labels"][0], g("labels")), i
        assert int(got["n_iter"][got["best"][0]]) == int(g("n_iter")), i
        assert np.abs(got["centers"][0] - g("centers")).max() <= kr.center_bound(z), i
        rows.append({"case": i, "centers_abs": err_c, "inertia_rel": err_i})
        if init is None:
            assert (got["done"] == 2).any()
    print(json.dumps(rows))


def test_runs_are_bitwise_equal_whatever_the_polling(ops, dev):
    z = kr.standardize(data(300, 33, 11))[0]
    a = gpu_fit(ops, dev, z, 5, 7, 10, poll_every=1)
    b = gpu_fit(ops, dev, z, 5, 7, 10, poll_every=7)
    c = gpu_fit(ops, dev, z, 5, 7, 10, poll_every=7)
    for key in ("labels", "centers", "inertia", "n_iter", "done", "best", "indices"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(b[key], c[key]), key
    assert a["iterations"] == int(a["n_iter"].max()) and b["iterations"] % 7 == 0


def test_nearest_rows(ops, dev):
    rng = np.random.default_rng(3)
    x = rng.normal(size=(130, 33))
    x[77] = x[12]                                   # a tie: the lower index wins
    x[129] = x[64]                                  # ... across tiles too
    q = np.concatenate([x[[77, 129, 5]], rng.normal(size=(67, 33))])
    idx, dist = ops.nearest_rows(to_dev(q, dev), to_dev(x, dev))
    want_i, want_d = kr.nearest_rows(q, x)
    assert idx.cpu().numpy()[:3].tolist() == [12, 64, 5]
    assert np.array_equal(idx.cpu().numpy(), want_i)
    assert np.abs(dist.cpu().numpy() - want_d).max() <= 33 * 2.0 ** -52 * float(want_d.max())
    i1, d1 = ops.nearest_rows(to_dev(q[:1, :1], dev), to_dev(x[:63, :1], dev))
    w1, _ = kr.nearest_rows(q[:1, :1], x[:63, :1])
    assert i1.cpu().numpy().tolist() == w1.tolist()


def info_of(n):
    return [{"issue": f"issue {j}: {'yes, no' if j % 7 == 0 else 'plain'}",
             "num_opinions": j % 5 + 1} for j in range(n)]


def test_pipeline_equals_the_reference(cl, dev, golden, tmp_path):
    """cluster_embeddings + find_cluster_centroids + save_cluster_results on the golden inputs:
    the reference's labels, centroid issues and CSV; the three seeds as one batch of R = 30."""
    for name in "abc":
        x = golden[f"x_{name}"]
        labels, centers, info = cl.cluster_embeddings(x, 5, 43, return_info=True)
        assert labels.dtype == np.int32 and centers.dtype == np.float64
        assert np.array_equal(labels, golden[f"ref_{name}_labels"]), name
        z = golden[f"z_{name}"]
        assert np.abs(centers - golden[f"ref_{name}_centers"]).max() <= kr.center_bound(z), name
        assert info["inertia"].shape == (10,) and info["indices"].shape == (10, 5)
        issues = info_of(len(x))
        cents = cl.find_cluster_centroids(x, issues, labels, centers)
        assert [issues.index(c) for c in cents] == golden[f"ref_{name}_centroids"].tolist(), name
        path = tmp_path / f"{name}.csv"
        cl.save_cluster_results(issues, labels, cents, str(path))
        assert path.read_bytes() == str(golden[f"ref_{name}_csv"]).encode(), name
        # the opt-in form compares like with like
        same = cl.find_cluster_centroids(x, issues, labels, centers, space="standardized")
        want, _ = kr.nearest_rows(centers, z)
        assert [issues.index(c) for c in same] == want.tolist(), name
    x = golden["x_b"]
    seeds = [42, 43, 7]
    batch = cl.cluster_embeddings_batch(x, 5, seeds, return_info=True)
    for s, (labels, centers, info) in zip(seeds, batch):
        one = cl.cluster_embeddings(x, 5, np.random.RandomState(s), return_info=True)
        assert np.array_equal(labels, one[0]) and np.array_equal(centers, one[1]), s
        for key in ("inertia", "n_iter", "indices", "done"):
            assert np.array_equal(info[key], one[2][key]), (s, key)
        assert info["best"] == one[2]["best"]
    i43 = [i for i in range(27) if str(golden[f"c{i}_input"]) == "b" and int(golden[f"c{i}_k"]) == 5]
    for i in i43:
        s = seeds.index(int(golden[f"c{i}_seed"]))
        assert np.array_equal(batch[s][0], golden[f"c{i}_labels"]), i


def test_embed_then_cluster_end_to_end(cl, dev, tmp_path):
    """embed_issues -> main on a random-weight encoder: shapes, files and resumability (random
    weights: no parity claim)."""
    model = "random:bge-base-en-v1.5"
    issues = [f"should the city {verb} the {thing}" for verb in ("fund", "close", "tax", "move")
              for thing in ("library", "harbour bridge", "night buses")]
    js, cs = str(tmp_path / cl.EMBEDDINGS_JSON), str(tmp_path / cl.ISSUES_CSV)
    first = cl.embed_issues(issues[:7], model=model, json_output=js, csv_output=cs)
    assert len(first) == 7 and all(len(r["embedding"]) == 768 for r in first)
    both = cl.embed_issues(issues, model=model, json_output=js, csv_output=cs)
    assert [r["issue"] for r in both] == issues and both[:7] == first        # resumed, not redone
    assert json.load(open(js)) == both
    assert open(cs).read().splitlines()[0] == "issue,has_embedding" and \
        len(open(cs).read().splitlines()) == 13
    before = os.path.getmtime(js)
    assert cl.embed_issues(issues, model=model, json_output=js, csv_output=cs) == both
    assert os.path.getmtime(js) == before                                    # nothing left to do

    def opinions(issue):
        n = 7 if "bridge" in issue and "tax" in issue else 2
        return [f"view {j}" for j in range(n)], "a consensus"

    cents = cl.main(3, 43, 5, opinions_for_issue=opinions, json_file=js, out_dir=str(tmp_path))
    assert len(cents) == 3 and all(c["num_opinions"] == 2 for c in cents)
    rows = open(tmp_path / cl.CLUSTERS_CSV).read().splitlines()
    assert rows[0] == "issue,num_opinions,cluster,is_centroid" and len(rows) == 12   # one left out
    assert sum(r.endswith(",True") for r in rows[1:]) == len({c["issue"] for c in cents})
    assert open(tmp_path / cl.CENTROIDS_CSV).read().splitlines()[0] == "cluster,issue"
    txt = open(tmp_path / cl.CENTROIDS_TXT).read()
    assert txt.count("CLUSTER ") == 3 and txt.count("CONSENSUS STATEMENT:\na consensus") == 3


def test_limits_raise(ops, dev):
    import torch
    z = torch.zeros(10, 4, dtype=torch.float64, device=dev)
    with pytest.raises(ops.CSError):
        ops.kmeans(z, 11, [0], np.zeros((1, 10, ops.kmeans_trials(11))))          # k > n
    with pytest.raises(ops.CSError):
        ops.kmeans(torch.zeros(70, 2, dtype=torch.float64, device=dev), 65, [0],
                   np.zeros((1, 64, ops.kmeans_trials(65))))                       # k > 64
    with pytest.raises(ops.CSError):
        ops.standardize(torch.zeros(2, 4097, dtype=torch.float64, device=dev))     # d > 4096
    with pytest.raises(ops.CSError):
        ops.kmeans_seed(z, 2, [0], np.ones((1, 1, 2)))                             # u outside [0, 1)
    with pytest.raises(ops.CSError):
        ops.kmeans(z, 2, np.zeros(1025, dtype=np.int32), np.zeros((1025, 1, 2)))   # R > 1024
