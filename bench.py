"""Flagship benchmark: AlexNet (reference example/ImageNet/ImageNet.conf) training
throughput in images/sec on N MI355X GPUs of one node.

  python bench.py --gpus N --steps K --warmup W [--scaling weak|strong] [--model alexnet]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints one JSON line; --dump-outputs DIR
then also writes what a step of the timed path computes (see _dump_outputs).  Every further
measurement of the same run sits behind --full.

One process per GPU, RCCL over xGMI.  Under torchrun (WORLD_SIZE set) every rank runs
the step; with --gpus N > 1 and no WORLD_SIZE this script launches
`python -m torch.distributed.run --nproc-per-node N` on itself as a CHILD process before
anything touches the GPU, and exits with its code.  A run whose process group does not
hold exactly N ranks exits non-zero.

Scaling modes (the reference's batch_size is the GLOBAL batch, split ceil(B/ndev) per
device: src/nnet/nnet_impl-inl.hpp:147-155, example/ImageNet/ImageNet.conf:108):
  weak   (default) every GPU trains a fixed per-GPU batch of --batch (256) images, the
         global batch is 256*N: the per-GPU work of the conf's 1-GPU run, N times over;
  strong the global batch is --batch (256) and each rank takes ceil(256/N) rows, exactly
         the reference's multi-device semantics for the conf as written.
With --full, the default weak scaling and N > 1 the same run also times the strong
configuration (ImageNet.conf's global batch of 256 over the N ranks) and reports it as the
nested "strong" record of the one JSON line (--strong-record 0 skips it).

Data is synthetic 3x227x227 batches resident on the device with random-init weights (no
dataset / checkpoint on the box).  By default they are uint8 HWC images -- what the
imgbin/img pipeline hands over after JPEG decode and crop -- normalised (mean
subtraction) and converted to NHWC bf16 by the fused augment kernel inside the step;
--input f32 feeds float NCHW batches instead.  A step is the full training step: input
normalisation/layout conversion, forward, loss gradient, backward, gradient reduction
(N > 1: bucketed fp32 all-reduce overlapped with backward, per-bucket optimizer on a side
stream; --dp-mode shard: reduce-scatter, sliced optimizer, bf16 weight all-gather; see
cxxnet_amd/parallel/dp.py) and the fused SGD-momentum update.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODEL_NAMES = {"alexnet": "AlexNet ImageNet", "inception_v1": "GoogLeNet/Inception-v1 ImageNet",
               "vgg16": "VGG-16 ImageNet", "mnist_mlp": "MNIST-MLP", "mnist_conv": "MNIST-conv",
               "bowl": "Kaggle-bowl convnet"}


def _args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256,
                    help="weak: per-GPU batch; strong: global batch split over the ranks")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--full", action="store_true",
                    help="also run every further measurement of this benchmark (today: the nested \"strong\" "
                         "record at N > 1); a plain run times the headline figure only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what a step of the timed path computes from the seeded "
                         "initial state (the loss layer's fp32 scores, the updated parameters and their change) "
                         "as DIR/<name>.npy, float32, <= 64 MB in all")
    ap.add_argument("--strong-record", type=int, default=1,
                    help="with --full, --scaling weak and N > 1, also time the conf's own configuration (global "
                         "batch --batch split over the ranks, strong scaling) and add it as a nested "
                         "\"strong\" record to the one JSON line")
    ap.add_argument("--model", default="alexnet")
    ap.add_argument("--input", default="u8", choices=["u8", "f32"],
                    help="u8: decoded-image batches (uint8 HWC) normalised on the GPU by the fused augment kernel, "
                         "as the imgbin pipeline delivers them; f32: float NCHW batches")
    ap.add_argument("--graph", type=int, default=-1,
                    help="replay forward/backward as HIP graphs (the optimizer and collectives stay eager). "
                         "-1 (default) = the trainer's auto rule: on under data parallelism at per-GPU batch <= 64 "
                         "(strong scaling); the 1-GPU AlexNet / GoogLeNet steps are GPU-bound, graph replay measured "
                         "-0.4%%/+0.5%% (profiles/early-r16_graph_ab.jsonl)")
    ap.add_argument("--dp-mode", default="auto", choices=["auto", "shard", "allreduce"],
                    help="gradient reduction: auto = fp32 all-reduce (shard: reduce-scatter, sliced update, "
                         "bf16 all-gather)")
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--device", default="gpu", choices=["gpu", "cpu"],
                    help="cpu: gloo ranks on the host (test hook for the launcher and the DP path)")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VAL",
                    help="extra conf overrides, e.g. --set dp_comm_dtype=bf16")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.warmup < 0:
        ap.error("--warmup must not be negative")
    return a


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(a) -> int:
    """Re-launch this script as N ranks (child process; nothing here has touched the GPU)."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def _baseline(model):
    """Same-model torch-eager img/s per GPU from BASELINE.json "measured" (None if absent)."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            b = json.load(f)
        m = b.get("measured", {}).get(f"torch_eager_{model}_img_s_per_gpu")
        return float(m) if m else None
    except Exception:
        return None



def _measure(a, world, rank, dev, global_batch, local_batch, dump=False):
    """Build the trainer at (global_batch, local_batch), run a.warmup untimed steps, then time
    a.steps steps bracketed by a barrier + device synchronisation; returns the MAX over ranks.
    dump: also hand back the batch and a copy of the initial parameters for _dump_outputs."""
    import torch
    import torch.distributed as dist
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    from cxxnet_amd.io.data import DataBatch
    lo = min(rank * local_batch, global_batch)
    my_rows = min(local_batch, global_batch - lo)  # the reference's ceil split: the last rank may hold fewer

    over = [("batch_size", str(global_batch)), ("eval_train", "0"), ("dev", a.device), ("silent", "1"),
            ("cuda_graph", str(a.graph)), ("dp_mode", a.dp_mode), ("dp_bucket_mb", str(a.bucket_mb))]
    for kv in a.set:
        k, v = kv.split("=", 1)
        over.append((k.strip(), v.strip()))
    pairs = load_conf(a.model, over)
    pairs = [(k, v) for k, v in pairs if not k.startswith("metric")]
    tr = NetTrainer()
    for k, v in pairs:
        tr.set_param(k, v)
    tr.init_model()
    assert tr._local_batch() == local_batch, (tr._local_batch(), local_batch)
    # --dump-outputs restarts from the seeded initial parameters (_dump_outputs)
    w0 = tr.net.arena.w.clone() if dump else None
    c, h, w = tr.net_cfg.input_shape
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    if a.input == "u8":
        from cxxnet_amd.io.data import U8Images
        pix = torch.randint(0, 256, (my_rows, h, w, c), generator=g, dtype=torch.uint8).to(dev)
        prm = torch.zeros((my_rows, 4), dtype=torch.int32, device=dev)
        cm = torch.tensor([[1.0, 0.0]] * my_rows, device=dev)
        mean = torch.tensor([123.68, 116.78, 103.94][:c], device=dev)  # mean_value subtraction (ImageNet RGB)
        data = U8Images(pix, prm, cm, mean, 1, 1.0)
        desc = (f"synthetic uint8 {c}x{h}x{w} images on device, mean subtraction fused on GPU; "
                f"random-init weights")
    else:
        data = torch.randn(my_rows, c, h, w, generator=g).to(dev)
        desc = f"synthetic fp32 {c}x{h}x{w} batches on device; random-init weights"
    ncls = 10 if a.model.startswith("mnist") else 1000
    label = torch.randint(0, ncls, (my_rows, 1), generator=g).float().to(dev)
    batch = DataBatch(data, label)

    def barrier():
        if world > 1:
            dist.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize()

    for _ in range(a.warmup):
        tr.update(batch, local=True)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.update(batch, local=True)
    tr.reducer.sync()
    barrier()
    el = time.perf_counter() - t0
    per_rank = [el]
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(x.item()) for x in allt]
        el = max(per_rank)
    return el, per_rank, tr, c, h, w, desc, batch, w0


def _dp_info(tr):
    red = tr.reducer
    return {"mode": ("shard" if red.shard else "allreduce") if red.active else "none",
            "buckets": len(red.buckets) if red.active else 0,
            "comm_bytes_per_step_per_rank": tr.comm_bytes_per_step(),
            "fullc_gather": any(getattr(c.layer, "_gathering", None) is not None and c.layer._gathering()
                                for c in tr.net.connections),
            "overlapped_update": red.handles_update}


DUMP_BUDGET = 6 << 20   # values per kind (param_*, step_*) written by --dump-outputs: 2 x 24 MB of float32
SCORE_BUDGET = 2 << 20  # score values over all ranks: 8 MB (AlexNet b256 on 8 GPUs fits whole)
DUMP_STEPS = 3          # steps from the initial state to the dumped one: the third has momentum behind it
assert (2 * DUMP_BUDGET + SCORE_BUDGET) * 4 <= 64 << 20


def _dump_outputs(tr, batch, w0, out_dir, rank, world):
    """What a step of the timed path hands back, as float32 <name>.npy files under out_dir.

    The state after the timed steps cannot be compared between two runs: the step sums fp32
    gradients with atomics, so runs differ in the last bit, and bf16 training amplifies that
    from step to step (profiles/bench_dump_repeatability.md).  So the dumped step is made
    independent of how many steps ran before it: NetTrainer.reset_to puts the parameters back to
    their seeded initial values (w0) and the optimizer state and counters to zero, and the timed
    path -- the same trainer, batch, plans and tuned tiles -- runs DUMP_STEPS more steps.  The
    last of them is written:
      scores.npy (scores_rank<r>.npy on ranks > 0)  the loss layer's fp32 scores of this rank's rows
                                                    (the first rows that fit SCORE_BUDGET / world);
      param_<layer index>_<layer name>_<tag>.npy    from rank 0, every parameter after the update
                                                    (the layout get_weight returns);
      step_<layer index>_<layer name>_<tag>.npy     the same elements minus their initial values:
                                                    what the DUMP_STEPS updates added, which a
                                                    comparison of the parameters alone would not
                                                    resolve (it is ~1e-3 of their range).
    (Shapes missing from the shipped GEMM tile table are timed on first use, so two runs may run
    different kernels: only dumps of shapes the table holds repeat to the last bits.)
    Each kind shares DUMP_BUDGET values: a tensor over the common cap is written as a fixed sample
    (indices drawn with a seed that depends only on the tensor's place in the net), so two builds
    write the same elements."""
    import numpy as np
    import torch
    net = tr.net
    tr.reset_to(w0)
    for _ in range(DUMP_STEPS):
        tr.update(batch, local=True)
    tr.prepare_save()  # (collective under sharded data parallelism: every rank calls it)
    tr.reducer.sync()
    os.makedirs(out_dir, exist_ok=True)
    scores = tr._node_output(len(net.nodes) - 1)[: tr._rows]
    scores = scores.reshape(scores.shape[0], -1)
    scores = scores[: SCORE_BUDGET // world // max(scores.shape[1], 1)].float().cpu().numpy()
    np.save(os.path.join(out_dir, "scores.npy" if rank == 0 else f"scores_rank{rank}.npy"), scores)
    if rank != 0:
        return
    specs = list(net.arena.specs)
    sizes = sorted(s.numel for _, s in specs)
    cap, left = (sizes[-1] if sizes else 0), DUMP_BUDGET
    for i, n in enumerate(sizes):  # the largest cap with sum(min(numel, cap)) <= DUMP_BUDGET
        if n * (len(sizes) - i) > left:
            cap = left // (len(sizes) - i)
            break
        left -= n
    for li, s in specs:
        layer = net.connections[li].layer
        w = s.w.detach().float()
        d = w - w0[s.offset:s.offset + s.numel].view(s.shape)
        name = f"{li:03d}_{tr.net_cfg.layers[li].name or 'layer'}_{s.tag}.npy"
        for kind, t in (("param", w), ("step", d)):
            t = t.cpu()
            if hasattr(layer, "to_logical") and s.tag == "wmat":
                t = layer.to_logical(t)  # (may drop channel padding: fewer values than s.numel)
            t = t.reshape(-1)
            if t.numel() > cap:
                g = torch.Generator(device="cpu").manual_seed(7919 * li + (s.tag != "wmat"))
                t = t[torch.randint(0, t.numel(), (cap,), generator=g)]
            np.save(os.path.join(out_dir, f"{kind}_{name}"), t.numpy())


def main():
    a = _args()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _spawn(a)

    import torch
    if a.device == "cpu":
        os.environ.setdefault("CXXNET_DIST_BACKEND", "gloo")
    from cxxnet_amd.parallel import init_distributed
    import torch.distributed as dist

    rank, world = init_distributed()
    if world != a.gpus:
        print(f"bench.py: --gpus {a.gpus} but the process group holds {world} rank(s)", file=sys.stderr)
        return 2
    if a.device == "gpu":
        dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    else:
        dev = torch.device("cpu")
        a.input = "f32"

    if a.scaling == "weak":
        local_batch = a.batch
        global_batch = a.batch * world
    else:
        global_batch = a.batch
        local_batch = (a.batch + world - 1) // world

    el, per_rank, tr, c, h, w, desc, batch, w0 = _measure(a, world, rank, dev, global_batch, local_batch,
                                                          dump=bool(a.dump_outputs))
    ms = el / a.steps * 1000.0
    value = global_batch * a.steps / el
    base = _baseline(a.model)
    dp = _dp_info(tr)
    if a.dump_outputs:
        _dump_outputs(tr, batch, w0, a.dump_outputs, rank, world)
        del batch, w0
    strong = None
    if a.full and a.scaling == "weak" and world > 1 and a.strong_record:
        # the conf's own configuration: its global batch split over the ranks
        del tr
        if dev.type == "cuda":
            torch.cuda.empty_cache()
        sg, sl = a.batch, (a.batch + world - 1) // world
        sel, sper, str_, *_ = _measure(a, world, rank, dev, sg, sl)
        strong = {"value": round(sg * a.steps / sel, 1), "unit": "images/sec", "scaling": "strong",
                  "global_batch": sg, "per_gpu_batch": sl, "ms_per_step": round(sel / a.steps * 1000.0, 3),
                  "per_rank_ms_per_step": [round(x / a.steps * 1000.0, 3) for x in sper], "dp": _dp_info(str_)}
    elif a.scaling == "weak" and world == 1:
        strong = "identical to the weak record at one GPU (global batch = per-GPU batch)"
    elif a.scaling == "weak" and a.strong_record:
        strong = "not measured (a run with --full times it)"
    if rank == 0:
        name = MODEL_NAMES.get(a.model, a.model)
        out = {
            "metric": f"images/sec (whole node) {name} training at 1/2/4/8 MI355X",
            "value": round(value, 1), "unit": "images/sec", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
            "scaling": a.scaling,
            "vs_baseline": round(value / (base * world), 3) if base else None,
            "dtype": "bf16" if dev.type == "cuda" else "fp32", "data": desc,
            "config": {"model": a.model, "global_batch": global_batch, "per_gpu_batch": local_batch,
                       "seq_len": None, "parallelism": f"dp{world}", "input_shape": [c, h, w]},
            "world_size": world,
            "per_rank_ms_per_step": [round(x / a.steps * 1000.0, 3) for x in per_rank],
            "dp": dp,
            "strong": strong,
            "baseline": (f"torch eager {a.model} {base:.0f} img/s per GPU x {world} (BASELINE.json measured)"
                         if base else None),
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
