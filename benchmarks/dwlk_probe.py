"""Large-kernel depthwise kernels (csrc/kernels/dwconv_lk_kernels.hip) at the four 7 x 7 pad-3 sites
of ConvNeXt-T for batch 64 -- 56^2 x 96, 28^2 x 192, 14^2 x 384, 7^2 x 768 -- forward, data gradient
and weight gradient, against torch.nn.functional.conv2d(groups = C) with its autograd backward on
channels-last bf16 tensors of the same values, and against a plain device copy of the bytes a
direction has to move (the input map in, the output map out; weights and slabs are small): timed
with device events in windows of --iters back-to-back calls after a warm-up, the arms alternating
round by round.  There is no older library route to compare with: no other kernel serves these
layers.  One JSON line per (site, direction, arm); the spread of an arm's windows is the noise a
difference has to exceed.  --step also times whole training steps of convnext_tiny.conf.

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all, so that a call
finds none of its tensors in the 256 MB Infinity Cache (at most 64 sets).
    python benchmarks/dwlk_probe.py [--iters 20] [--rounds 5] [--step]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import gemm  # noqa: E402
from cxxnet_amd.ops.gemm import ConvGeom  # noqa: E402

BATCH, K, PAD = 64, 7, 3
SITES = [(96, 56), (192, 28), (384, 14), (768, 7)]  # (C, H = W)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def site(a, C, H):
    dev = "cuda"
    g = ConvGeom(BATCH, H, H, C, H, H, C, K, K, 1, PAD, PAD, C)
    name = "%dx%dx%dx%d k%d" % (BATCH, H, H, C, K)
    n = BATCH * H * H * C
    gen = torch.Generator(device=dev).manual_seed(C + H)
    x0 = torch.randn(BATCH, H, H, C, device=dev, generator=gen).to(torch.bfloat16)
    dy0 = torch.randn(BATCH, H, H, C, device=dev, generator=gen).to(torch.bfloat16)
    w = (torch.randn(C, K, K, 1, device=dev, generator=gen) * 0.1).to(torch.bfloat16)
    wt = w.permute(0, 3, 1, 2)  # [C][1][K][K], the same storage
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (4 * n * 2))))
    sets = [{"x": x0.clone(), "dy": dy0.clone(), "y": torch.empty_like(dy0), "dx": torch.empty_like(x0),
             "dw": torch.zeros(C, K, K, 1, device=dev)} for _ in range(nsets)]
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def nchw(t):
        return t.permute(0, 3, 1, 2)

    def t_bwd(s, mask):
        return torch.ops.aten.convolution_backward(nchw(s["dy"]), nchw(s["x"]), wt, None, [1, 1], [PAD, PAD], [1, 1],
                                                   False, [0, 0], C, mask)

    arms = {
        ("forward", "dwlk"): lambda: (lambda s: gemm.dwlk_forward(s["x"], w, None, s["y"], g))(nxt()),
        ("data_grad", "dwlk"): lambda: (lambda s: gemm.dwlk_backward_data(s["dy"], w, s["dx"], g))(nxt()),
        ("weight_grad", "dwlk"): lambda: (lambda s: gemm.dwlk_backward_weight(s["x"], s["dy"], s["dw"], g))(nxt()),
        ("forward", "torch"): lambda: F.conv2d(nchw(nxt()["x"]), wt, None, 1, PAD, 1, C),
        ("data_grad", "torch"): lambda: t_bwd(nxt(), [True, False, False]),
        ("weight_grad", "torch"): lambda: t_bwd(nxt(), [False, True, False]),
        # the bytes of a direction as one copy: a map in, a map out (the weight gradient reads two maps;
        # the copy of one map moves the same 2 n elements)
        ("any", "copy"): lambda: (lambda s: s["y"].copy_(s["x"]))(nxt()),
    }
    # the arms agree before anything is timed
    s = sets[0]
    gemm.dwlk_forward(s["x"], w, None, s["y"], g)
    ref = F.conv2d(nchw(s["x"]), wt, None, 1, PAD, 1, C).permute(0, 2, 3, 1)
    assert torch.allclose(s["y"].float(), ref.float(), rtol=2e-2, atol=2e-2), "forward arms disagree"
    gemm.dwlk_backward_data(s["dy"], w, s["dx"], g)
    ref = t_bwd(s, [True, False, False])[0].permute(0, 2, 3, 1)
    assert torch.allclose(s["dx"].float(), ref.float(), rtol=2e-2, atol=5e-2), "data-gradient arms disagree"
    s["dw"].zero_()
    gemm.dwlk_backward_weight(s["x"], s["dy"], s["dw"], g)
    ref = t_bwd(s, [False, True, False])[1].permute(0, 2, 3, 1).float()
    err = ((s["dw"] - ref).abs().max() / ref.abs().max()).item()
    assert err < 2e-2, "weight-gradient arms disagree: %g" % err  # (torch stores its gradient as bf16)
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(max(a.warmup, nsets)):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k in times:  # alternate the arms
            times[k].append(window(arms[k], a.iters))
    for (direction, arm), ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        print(json.dumps({"shape": name, "direction": direction, "arm": arm, "us_median": round(med, 2),
                          "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                          "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1), "bytes": 4 * n,
                          "gb_per_s": round(4 * n / (med * 1e-6) / 1e9, 1), "iters": a.iters, "rounds": a.rounds,
                          "buffer_sets": nsets}), flush=True)


def step_time(a):
    """ms per training step of convnext_tiny.conf at batch 64 on synthetic data: a host clock around
    --step-iters steps that end in a device synchronise, after a warm-up, --rounds times."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("convnext_tiny", []) if not k.startswith("metric")] + [
            ("batch_size", str(BATCH)), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1")]:
        tr.set_param(k, v)
    tr.init_model()
    gen = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(BATCH, 3, 224, 224, generator=gen), torch.randint(0, 1000, (BATCH, 1), generator=gen).float())
    for _ in range(a.warmup):
        tr.update(b)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.step_iters):
            tr.update(b)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / a.step_iters)
    ts.sort()
    print(json.dumps({"model": "convnext_tiny", "batch": BATCH, "ms_per_step_median": round(ts[len(ts) // 2], 3),
                      "ms_min": round(ts[0], 3), "ms_max": round(ts[-1], 3), "steps_per_window": a.step_iters,
                      "rounds": a.rounds, "includes": "host-to-device copy of the batch"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--step", action="store_true", help="also time convnext_tiny.conf training steps")
    ap.add_argument("--step-iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwlk_probe needs a GPU")
    for C, H in SITES:
        site(a, C, H)
    if a.step:
        step_time(a)


if __name__ == "__main__":
    main()
