"""Depthwise kernels (csrc/kernels/dwconv_kernels.hip) against what a user has without them,
torch.nn.functional.conv2d(groups = C) and its autograd backward on channels-last bf16, at the
nine distinct depthwise layers of MobileNet-v1 for batch 64: forward, data gradient and weight
gradient of each, timed with device events in windows of --iters back-to-back calls.  The arms
alternate inside one process, --rounds times each; the spread of an arm's windows is the noise a
difference has to exceed.  One JSON line per (shape, direction, arm) with the bytes the direction
must move, computed from the shapes, over the median time (achieved GB/s) and against the measured
HBM copy rate.

    forward          reads x, writes y                       (the K K C weights are noise)
    data gradient    reads dy, writes dx
    weight gradient  reads x and dy                          (dw, db and the partial slabs are small)

The torch arms run on the same storage (an NHWC tensor is a channels-last NCHW view); its backward
is aten.convolution_backward with one output selected, the call autograd makes.

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times
the 256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM
rate (at most 64 sets).
    python benchmarks/dwconv_probe.py [--iters 50] [--rounds 5] [--out profiles/dwconv_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import gemm  # noqa: E402
from cxxnet_amd.ops.gemm import ConvGeom  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH = 64
# (C, H = W, stride) of MobileNet-v1's depthwise layers, each 3 x 3 pad 1
LAYERS = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1),
          (512, 14, 2), (1024, 7, 1)]


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--no-torch", action="store_true", help="time the library kernels only")
    ap.add_argument("--layers", default="", help="comma-separated indices into LAYERS (default: all nine)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    layers = [LAYERS[int(i)] for i in a.layers.split(",")] if a.layers else LAYERS
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_probe needs a GPU")
    dev = "cuda"
    lines = []
    for C, H, S in layers:
        Ho, Wo = gemm.conv_out_size(H, H, 3, 3, S, 1, 1)
        g = ConvGeom(BATCH, H, H, C, Ho, Wo, C, 3, 3, S, 1, 1, C)
        name = "%dx%dx%dx%d/%d" % (BATCH, H, H, C, S)
        nin, nout = BATCH * H * H * C, BATCH * Ho * Wo * C
        gen = torch.Generator(device=dev).manual_seed(C * H + S)
        x0 = torch.randn(BATCH, H, H, C, device=dev, generator=gen).to(torch.bfloat16)
        dy0 = torch.randn(BATCH, Ho, Wo, C, device=dev, generator=gen).to(torch.bfloat16)
        w = (torch.randn(C, 3, 3, 1, device=dev, generator=gen) * 0.3).to(torch.bfloat16)
        wt = w.permute(0, 3, 1, 2)  # [C][1][3][3], the same storage
        per_set = 2 * (nin + nout) * 2  # x, dx, y, dy
        nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
        sets = [{"x": x0.clone(), "dy": dy0.clone(), "y": torch.empty_like(dy0), "dx": torch.empty_like(x0),
                 "dw": torch.zeros(C, 3, 3, 1, device=dev)} for _ in range(nsets)]
        turn = {"i": 0}

        def nxt():
            turn["i"] = (turn["i"] + 1) % nsets
            return sets[turn["i"]]

        def nchw(t):
            return t.permute(0, 3, 1, 2)

        def t_bwd(s, mask):
            return torch.ops.aten.convolution_backward(nchw(s["dy"]), nchw(s["x"]), wt, None, [S, S], [1, 1], [1, 1],
                                                       False, [0, 0], C, mask)

        arms = {
            ("forward", "new"): lambda: (lambda s: gemm.conv_forward(s["x"], w, None, s["y"], g))(nxt()),
            ("data_grad", "new"): lambda: (lambda s: gemm.conv_backward_data(s["dy"], w, s["dx"], g))(nxt()),
            ("weight_grad", "new"): lambda: (lambda s: gemm.conv_backward_weight(s["x"], s["dy"], s["dw"], g))(nxt()),
        }
        if not a.no_torch:
            arms.update({
                ("forward", "torch"): lambda: F.conv2d(nchw(nxt()["x"]), wt, None, S, 1, 1, C),
                ("data_grad", "torch"): lambda: t_bwd(nxt(), [True, False, False]),
                ("weight_grad", "torch"): lambda: t_bwd(nxt(), [False, True, False]),
            })
            # the arms agree before anything is timed (bf16 outputs of fp32 sums of nine terms)
            s = sets[0]
            gemm.conv_forward(s["x"], w, None, s["y"], g)
            ref = F.conv2d(nchw(s["x"]), wt, None, S, 1, 1, C).permute(0, 2, 3, 1)
            assert torch.allclose(s["y"].float(), ref.float(), rtol=2e-2, atol=2e-2), "forward arms disagree"
            gemm.conv_backward_data(s["dy"], w, s["dx"], g)
            ref = t_bwd(s, [True, False, False])[0].permute(0, 2, 3, 1)
            assert torch.allclose(s["dx"].float(), ref.float(), rtol=2e-2, atol=2e-2), "data-gradient arms disagree"
            s["dw"].zero_()
            gemm.conv_backward_weight(s["x"], s["dy"], s["dw"], g)
            ref = t_bwd(s, [False, True, False])[1].permute(0, 2, 3, 1).float()
            err = ((s["dw"] - ref).abs().max() / ref.abs().max()).item()
            assert err < 2e-2, "weight-gradient arms disagree: %g" % err  # (torch stores its gradient as bf16)
        need = {"forward": (nin + nout) * 2, "data_grad": (nin + nout) * 2, "weight_grad": (nin + nout) * 2}
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(max(a.warmup, nsets)):
                fn()
        torch.cuda.synchronize()
        print("# %s: warmed up, %d buffer sets" % (name, nsets), flush=True)
        for _ in range(a.rounds):
            for k, fn in arms.items():  # alternate the arms
                times[k].append(window(fn, a.iters))
        for (direction, arm), ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            nbytes = need[direction]
            rec = {"shape": name, "direction": direction, "arm": arm, "us_median": round(med, 2),
                   "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                   "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1), "bytes": int(nbytes),
                   "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                   "share_of_hbm_rate": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                   "iters": a.iters, "rounds": a.rounds, "buffer_sets": nsets}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del sets
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
