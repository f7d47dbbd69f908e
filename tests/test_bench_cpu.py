"""bench.py launcher contract on the CPU (gloo ranks): `--gpus N` without torchrun spawns N
ranks itself, reports the process group's size, and a rank-count mismatch exits non-zero."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["OMP_NUM_THREADS"] = "2"
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    r = _run(["bench.py", "--gpus", "2", "--device", "cpu", "--model", "mnist_mlp", "--batch", "8",
              "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json(r.stdout)
    assert out["n_gpus"] == 2 and out["world_size"] == 2
    assert out["scaling"] == "weak" and out["config"]["global_batch"] == 16
    assert len(out["per_rank_ms_per_step"]) == 2
    assert out["dp"]["comm_bytes_per_step_per_rank"] > 0
    assert "AlexNet" not in out["metric"]
    assert not isinstance(out["strong"], dict)  # a plain run times the headline figure only


def test_bench_strong_scaling_splits_global_batch():
    r = _run(["bench.py", "--gpus", "2", "--device", "cpu", "--model", "mnist_mlp", "--batch", "10",
              "--steps", "2", "--warmup", "1", "--scaling", "strong", "--dp-mode", "shard"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json(r.stdout)
    assert out["scaling"] == "strong"
    assert out["config"]["global_batch"] == 10 and out["config"]["per_gpu_batch"] == 5
    assert out["dp"]["mode"] == "shard"


def test_bench_rank_mismatch_fails():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    r = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
              "--master-port", port, "bench.py", "--gpus", "2", "--device", "cpu", "--model", "mnist_mlp",
              "--batch", "8", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "process group holds 1" in r.stderr


def test_bench_8_ranks_weak():
    r = _run(["bench.py", "--gpus", "8", "--device", "cpu", "--model", "mnist_mlp", "--batch", "8",
              "--steps", "2", "--warmup", "1", "--full"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json(r.stdout)
    assert out["n_gpus"] == 8 and out["world_size"] == 8 and len(out["per_rank_ms_per_step"]) == 8
    assert out["config"]["global_batch"] == 64 and out["dp"]["mode"] == "allreduce"
    # the same run times the conf's own (strong-scaling) configuration: 8 images over 8 ranks
    st = out["strong"]
    assert st["scaling"] == "strong" and st["global_batch"] == 8 and st["per_gpu_batch"] == 1
    assert st["value"] > 0 and len(st["per_rank_ms_per_step"]) == 8


def test_bench_8_ranks_strong_alexnet_fullc_gather():
    """AlexNet at the strong-scaling split (256 over 8 ranks = 32 rows each): fullc_gather's
    default (auto) all-gathers the fc layers' [in | out-grad] rows instead of reducing their
    58.6 M gradient values, so a rank hands <= 40 MB per step to collectives (fp32 here; the GPU
    gathers bf16) against 244 MB of fp32 gradients without it."""
    r = _run(["bench.py", "--gpus", "8", "--device", "cpu", "--model", "alexnet", "--batch", "256",
              "--scaling", "strong", "--steps", "1", "--warmup", "0"], timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json(r.stdout)
    assert out["config"]["per_gpu_batch"] == 32 and out["dp"]["fullc_gather"]
    assert out["dp"]["comm_bytes_per_step_per_rank"] <= 40e6, out["dp"]


def _dump_run(out_dir, steps, model="mnist_mlp", batch=8, warmup=1):
    import numpy as np
    r = _run(["bench.py", "--gpus", "1", "--device", "cpu", "--model", model, "--batch", str(batch),
              "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)])
    assert r.returncode == 0, r.stderr[-3000:]
    return _json(r.stdout), {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the scores, the updated parameters and their change as float32 .npy
    files within 64 MB; --steps sets the number of timed steps; two runs with the same arguments
    write the same values (the CPU step is deterministic: bitwise), and so does a run with
    another number of timed steps, since the dumped step restarts from the seeded initial state."""
    import numpy as np
    out, a = _dump_run(tmp_path / "a", 3)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert abs(out["value"] - 8 / (out["ms_per_step"] / 1000.0)) <= 0.01 * out["value"]
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["scores.npy"].shape == (8, 10)
    assert np.allclose(a["scores.npy"].sum(1), 1.0, atol=1e-5)
    params = [f for f in a if f.startswith("param_")]
    assert len(params) == 4 and sorted("step_" + f[6:] for f in params) == [f for f in a if f.startswith("step_")]
    for f in params:  # the change is what the updates added, and they did add something
        assert a["step_" + f[6:]].shape == a[f].shape
    assert all(np.abs(a[f]).max() > 0 for f in a if f.startswith("step_") and f.endswith("_wmat.npy"))
    for d, steps in (("b", 3), ("c", 6)):
        out, b = _dump_run(tmp_path / d, steps)
        assert out["steps"] == steps and a.keys() == b.keys()
        for f in a:
            np.testing.assert_array_equal(a[f], b[f])


def test_bench_dump_budget_samples_large_parameters(tmp_path):
    """AlexNet's 61 M parameters do not fit: tensors over the common cap are written as a fixed
    sample and the files stay within 64 MB."""
    _, arrs = _dump_run(tmp_path, 1, model="alexnet", batch=2, warmup=0)
    assert arrs["scores.npy"].shape == (2, 1000)
    total = sum(x.nbytes for x in arrs.values())
    assert 32 << 20 < total <= 64 << 20
    fc = [x for f, x in arrs.items() if f.startswith("param_") and f.endswith("_wmat.npy")]
    assert len({x.size for x in fc}) > 1 and max(x.size for x in fc) < 37748736


def test_bench_dump_two_ranks_sharded(tmp_path):
    """The dump under sharded data parallelism (its save is a collective): every rank writes its own
    rows' scores and rank 0 the gathered parameters, every slice of them stepped."""
    import numpy as np
    r = _run(["bench.py", "--gpus", "2", "--device", "cpu", "--model", "mnist_mlp", "--batch", "8",
              "--scaling", "strong", "--dp-mode", "shard", "--steps", "2", "--warmup", "1",
              "--dump-outputs", str(tmp_path / "dp")])
    assert r.returncode == 0, r.stderr[-3000:]
    dp = {f: np.load(tmp_path / "dp" / f) for f in sorted(os.listdir(tmp_path / "dp"))}
    assert dp["scores.npy"].shape == (4, 10) and dp["scores_rank1.npy"].shape == (4, 10)
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in dp.values())
    assert sum(x.nbytes for x in dp.values()) <= 64 << 20
    steps = [f for f in dp if f.startswith("step_")]
    assert len(steps) == 4 and all(np.abs(dp[f]).max() > 0 for f in steps)
    # every slice of the parameters was stepped and gathered: no element of a weight matrix kept its initial value
    assert all((dp[f] != 0).mean() > 0.99 for f in steps if f.endswith("_wmat.npy"))
