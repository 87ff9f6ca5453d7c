"""bench.py's multi-GPU launch contract, on CPU: `--gpus N` outside torchrun relaunches
itself as N ranks (torch.distributed.run, 127.0.0.1) and every rank checks the world
size; a world size that disagrees with --gpus fails loudly instead of reporting a
1-GPU number as N (Missing 2)."""
import json
import os
import subprocess
import sys

from conftest import REPO


def _env():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_bench_launches_n_ranks_itself():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2",
                        "--backend", "gloo", "--selftest-launch"],
                       capture_output=True, text=True, timeout=300, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2
    ranks = line["ranks"]
    assert [x["rank"] for x in ranks] == [0, 1]
    assert [x["local_rank"] for x in ranks] == [0, 1]
    # agents shard round-robin: C2 keeps 8 per GPU (weak), C3 / C5 split the config's total
    assert sorted(a for x in ranks for a in x["c2_agents"]) == list(range(16))
    assert [len(x["c3_agents"]) for x in ranks] == [8, 8]
    assert [len(x["c5_agents"]) for x in ranks] == [32, 32]


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    """--dump-outputs: every array lands as <name>.npy in float32 / float64; an array over
    its share of the size cap is cut to the same seeded sample on every run."""
    import numpy as np
    import torch

    import bench
    arrays = {"best_candidate": bench._as_np(torch.tensor([7])),
              "welfare": bench._as_np(torch.arange(6, dtype=torch.bfloat16)),
              "token_logprobs": bench._as_np(torch.arange(1000, dtype=torch.float32))}
    assert arrays["best_candidate"].dtype == np.float64
    assert arrays["welfare"].dtype == np.float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, cap_bytes=3 * 400)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert got["best_candidate"].tolist() == [7.0]
    assert got["welfare"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    lp = got["token_logprobs"]
    assert lp.dtype == np.float32 and lp.size == 100 and lp.nbytes <= 400
    assert np.all(np.diff(lp) > 0) and set(lp.tolist()) <= set(range(1000))
    assert np.array_equal(lp, np.load(tmp_path / "b" / "token_logprobs.npy"))


def test_plain_run_options_exist():
    """--full and --dump-outputs are part of the command line; --steps 0 is refused."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120, env=_env(), cwd=REPO)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120, env=_env(), cwd=REPO)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


def test_bench_rejects_world_size_mismatch():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2",
                        "--selftest-launch"], capture_output=True, text=True, timeout=120,
                       env=env, cwd=REPO)
    assert r.returncode != 0
    assert "world size 1 != --gpus 2" in r.stderr
