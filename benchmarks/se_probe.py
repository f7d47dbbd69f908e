"""Squeeze-and-excitation kernels (csrc/kernels/se_kernels.hip) at the four SE sites of SE-ResNet-18
for batch 64: each launch timed with device events in windows of --iters back-to-back calls.  The
arms alternate inside one process, --rounds times each; the spread of an arm's windows is the noise
a difference has to exceed.  One JSON line per (shape, arm) with the bytes the arm must move,
computed from the shapes, over the median time (achieved GB/s) and against the measured HBM copy rate.

    scale_fwd_new   ch_scale forward, one launch: reads x and the gate, writes y
    scale_fwd_torch x * s[:, None, None, :]
    scale_bwd_new   ch_scale backward: reads g and x, writes dx and ds (a merge launch where the map is
                    cut into parts)
    scale_bwd_torch g * s[:, None, None, :] and (g * x).sum((1, 2)), stored as bf16
    pool_fwd_new    global avg pooling on the new kernel (ops.pool_forward's route)
    pool_fwd_old    the same call with ops.nn.GLOBAL_POOL off: the generic pool_fwd_rows, one lane per
                    output.  At 7 x 7 the route keeps the generic kernel, so the new arm there calls the
                    launcher directly
    pool_bwd        ops.pool_backward of the global avg pooling: a pure broadcast of dy / (H W)

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times the
256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM rate
(at most 64 sets).
    python benchmarks/se_probe.py [--iters 200] [--rounds 5] [--out profiles/se_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd import native, ops  # noqa: E402
from cxxnet_amd.ops import layer_ops as L  # noqa: E402
from cxxnet_amd.ops import nn as NN  # noqa: E402
from cxxnet_amd.ops.gemm import _stream  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH = 64
SHAPES = [(BATCH, 56, 56, 64), (BATCH, 28, 28, 128), (BATCH, 14, 14, 256), (BATCH, 7, 7, 512)]


def arm_bytes(B, H, W, C):
    """bytes each arm must move (bf16 tensors; the fp32 partials and the gate are counted too)"""
    n, bc = B * H * W * C, B * C
    parts = L.se_parts(B, H * W, C)
    ws = 2 * 4 * parts * bc if parts > 1 else 0  # partials written and read once
    return {"scale_fwd_new": 4 * n + 2 * bc, "scale_fwd_torch": 4 * n + 2 * bc,
            "scale_bwd_new": 6 * n + 4 * bc + ws,
            "scale_bwd_torch": (4 * n + 2 * bc) + (4 * n + 2 * n) + (2 * n + 4 * bc) + 6 * bc,  # g s; t = g x; sum; cast
            "pool_fwd_new": 2 * n + 2 * bc + ws, "pool_fwd_old": 2 * n + 2 * bc,
            "pool_bwd": 2 * n + 2 * bc}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_probe needs a GPU")
    dev = "cuda"
    k = native.kernels()
    lines = []
    for B, H, W, C in SHAPES:
        name = "%dx%dx%dx%d" % (B, H, W, C)
        n = B * H * W * C
        gen = torch.Generator(device=dev).manual_seed(n)
        x0 = torch.randn(B, H, W, C, device=dev, generator=gen).to(torch.bfloat16)
        g0 = torch.randn(B, H, W, C, device=dev, generator=gen).to(torch.bfloat16)
        s0 = torch.rand(B, 1, C, 1, device=dev, generator=gen).to(torch.bfloat16)
        per_set = 4 * n * 2  # x, g, y, dx
        nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
        sets = [{"x": x0.clone(), "g": g0.clone(), "s": s0.clone(), "y": torch.empty_like(x0), "dx": torch.empty_like(x0),
                 "ds": torch.empty_like(s0), "p": torch.empty(B, 1, 1, C, dtype=torch.bfloat16, device=dev),
                 "st": L.ChScaleState(B, H * W, C, dev, True)} for _ in range(nsets)]
        turn = {"i": 0}
        nws = int(k.cxn_se_ws_floats(B, H * W, C))
        pool_ws = torch.zeros(max(nws, 1), dtype=torch.float32, device=dev)
        routed = ops.pool_global_native("avg", H, W, C, H, W, 0, 1, 1)

        def nxt():
            turn["i"] = (turn["i"] + 1) % nsets
            return sets[turn["i"]]

        def scale_fwd_new():
            s = nxt()
            L.ch_scale_forward(s["x"], s["s"], s["y"])

        def scale_fwd_torch():
            s = nxt()
            torch.mul(s["x"], s["s"].view(B, 1, 1, C), out=s["y"])

        def scale_bwd_new():
            s = nxt()
            L.ch_scale_backward(s["g"], s["x"], s["s"], s["dx"], s["ds"], s["st"])

        def scale_bwd_torch():
            s = nxt()
            torch.mul(s["g"], s["s"].view(B, 1, 1, C), out=s["dx"])
            s["ds"].view(B, C).copy_((s["g"] * s["x"]).sum((1, 2), dtype=torch.float32))

        def pool_new(s):
            if routed:
                ops.pool_forward(s["x"], s["p"], None, H, W, 1, 0, "avg")
            else:  # below the route's window threshold: the launcher itself
                native.check(k.cxn_global_pool_fwd(s["x"].data_ptr(), s["p"].data_ptr(), pool_ws.data_ptr(),
                                                   pool_ws.numel(), B, H * W, C, 1.0 / (H * W), _stream()), "pool")

        def pool_fwd_new():
            pool_new(nxt())

        def pool_fwd_old():
            s = nxt()
            NN.GLOBAL_POOL = False
            try:
                ops.pool_forward(s["x"], s["p"], None, H, W, 1, 0, "avg")
            finally:
                NN.GLOBAL_POOL = True

        def pool_bwd():
            s = nxt()
            ops.pool_backward(s["x"], None, s["p"], s["dx"], H, W, 1, 0, "avg")

        arms = {"scale_fwd_new": scale_fwd_new, "scale_fwd_torch": scale_fwd_torch, "scale_bwd_new": scale_bwd_new,
                "scale_bwd_torch": scale_bwd_torch, "pool_fwd_new": pool_fwd_new, "pool_fwd_old": pool_fwd_old,
                "pool_bwd": pool_bwd}
        # the arms agree before anything is timed
        s = sets[0]
        scale_fwd_new_y = torch.empty_like(x0)
        L.ch_scale_forward(s["x"], s["s"], scale_fwd_new_y)
        assert torch.equal(scale_fwd_new_y, s["x"] * s["s"].view(B, 1, 1, C)), "torch computes another y"
        L.ch_scale_backward(s["g"], s["x"], s["s"], s["dx"], s["ds"], s["st"])
        assert torch.equal(s["dx"], s["g"] * s["s"].view(B, 1, 1, C))
        want = (s["g"].double() * s["x"].double()).sum((1, 2))
        assert (s["ds"].view(B, C).double() - want).abs().max() <= 2.0 ** -7 * want.abs().max() + 1e-3
        pool_new(s)
        pnew = s["p"].clone()
        NN.GLOBAL_POOL = False
        ops.pool_forward(s["x"], s["p"], None, H, W, 1, 0, "avg")
        NN.GLOBAL_POOL = True
        pref = s["x"].double().mean((1, 2))
        for got in (pnew, s["p"]):
            assert (got.view(B, C).double() - pref).abs().max() <= 2.0 ** -7 * pref.abs().max() + 1e-4
        nbytes = arm_bytes(B, H, W, C)
        times = {kk: [] for kk in arms}
        for fn in arms.values():
            for _ in range(max(a.warmup, nsets)):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for kk, fn in arms.items():  # alternate the arms
                times[kk].append(window(fn, a.iters))
        for kk, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            rec = {"shape": name, "arm": kk, "parts": L.se_parts(B, H * W, C), "pool_routed": bool(routed),
                   "us_median": round(med, 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                   "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1), "bytes": int(nbytes[kk]),
                   "gb_per_s": round(nbytes[kk] / (med * 1e-6) / 1e9, 1),
                   "share_of_hbm_rate": round(nbytes[kk] / (med * 1e-6) / HBM_BYTES_PER_S, 3),
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
