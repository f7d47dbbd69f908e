"""Narrow-group kernels (csrc/kernels/gconv_kernels.hip) at the seven grouped 3 x 3 sites of
ResNeXt-50 32x4d for batch 64, against the route such a layer took without them (one GEMM per
group, CXXNET_GC=0) and against torch.nn.functional.conv2d(groups = 32) with its autograd backward
on channels-last bf16: forward, data gradient and weight gradient of each, timed with device events
in windows of --iters back-to-back calls after a warm-up.

CXXNET_GC is read when the package is imported, so the old route runs in a fresh child process per
site (this script with --old), started right before the site's other arms: old and new alternate
site by site inside one call.  Where the old route does not run at all (the data gradient at 4
channels per group) the line says so.  One JSON line per (site, direction, arm) with the byte
floor computed from the shapes -- forward reads x and writes y, the data gradient reads dy and
writes dx, the weight gradient reads x and dy; weights and partial slabs are small -- over the
median time (achieved GB/s) and against the measured HBM copy rate.  The spread of an arm's windows
is the noise a difference has to exceed.

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all, so that a call
finds none of its tensors in the 256 MB Infinity Cache (at most 64 sets).
    python benchmarks/gconv_probe.py [--iters 20] [--rounds 5]"""
import argparse
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import gemm  # noqa: E402
from cxxnet_amd.ops.gemm import ConvGeom  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH, GROUPS = 64, 32
# (C, H = W, stride) of ResNeXt-50's grouped convs, each 3 x 3 pad 1 in 32 groups
SITES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def site(a, idx, old):
    C, H, S = SITES[idx]
    dev = "cuda"
    Ho, Wo = gemm.conv_out_size(H, H, 3, 3, S, 1, 1)
    g = ConvGeom(BATCH, H, H, C, Ho, Wo, C, 3, 3, S, 1, 1, GROUPS)
    cg = C // GROUPS
    name = "%dx%dx%dx%d/%d cg%d" % (BATCH, H, H, C, S, cg)
    nin, nout = BATCH * H * H * C, BATCH * Ho * Wo * C
    gen = torch.Generator(device=dev).manual_seed(C * H + S)
    x0 = torch.randn(BATCH, H, H, C, device=dev, generator=gen).to(torch.bfloat16)
    dy0 = torch.randn(BATCH, Ho, Wo, C, device=dev, generator=gen).to(torch.bfloat16)
    w = (torch.randn(C, 3, 3, cg, device=dev, generator=gen) * 0.1).to(torch.bfloat16)
    wt = w.permute(0, 3, 1, 2)  # [C][cg][3][3], the same storage
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (2 * (nin + nout) * 2))))
    sets = [{"x": x0.clone(), "dy": dy0.clone(), "y": torch.empty_like(dy0), "dx": torch.empty_like(x0),
             "dw": torch.zeros(C, 3, 3, cg, device=dev)} for _ in range(nsets)]
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def nchw(t):
        return t.permute(0, 3, 1, 2)

    def t_bwd(s, mask):
        return torch.ops.aten.convolution_backward(nchw(s["dy"]), nchw(s["x"]), wt, None, [S, S], [1, 1], [1, 1],
                                                   False, [0, 0], GROUPS, mask)

    lib = "old" if old else "new"
    arms = {
        ("forward", lib): lambda: (lambda s: gemm.conv_forward(s["x"], w, None, s["y"], g))(nxt()),
        ("data_grad", lib): lambda: (lambda s: gemm.conv_backward_data(s["dy"], w, s["dx"], g))(nxt()),
        ("weight_grad", lib): lambda: (lambda s: gemm.conv_backward_weight(s["x"], s["dy"], s["dw"], g))(nxt()),
    }
    if not old and not a.no_torch:
        arms.update({
            ("forward", "torch"): lambda: F.conv2d(nchw(nxt()["x"]), wt, None, S, 1, 1, GROUPS),
            ("data_grad", "torch"): lambda: t_bwd(nxt(), [True, False, False]),
            ("weight_grad", "torch"): lambda: t_bwd(nxt(), [False, True, False]),
        })
        # the arms agree before anything is timed (bf16 outputs of fp32 sums of 9 cg terms)
        s = sets[0]
        gemm.conv_forward(s["x"], w, None, s["y"], g)
        ref = F.conv2d(nchw(s["x"]), wt, None, S, 1, 1, GROUPS).permute(0, 2, 3, 1)
        assert torch.allclose(s["y"].float(), ref.float(), rtol=2e-2, atol=2e-2), "forward arms disagree"
        gemm.conv_backward_data(s["dy"], w, s["dx"], g)
        ref = t_bwd(s, [True, False, False])[0].permute(0, 2, 3, 1)
        assert torch.allclose(s["dx"].float(), ref.float(), rtol=2e-2, atol=5e-2), "data-gradient arms disagree"
        s["dw"].zero_()
        gemm.conv_backward_weight(s["x"], s["dy"], s["dw"], g)
        ref = t_bwd(s, [False, True, False])[1].permute(0, 2, 3, 1).float()
        err = ((s["dw"] - ref).abs().max() / ref.abs().max()).item()
        assert err < 2e-2, "weight-gradient arms disagree: %g" % err  # (torch stores its gradient as bf16)
    times = {}
    for k, fn in arms.items():
        try:
            for _ in range(max(a.warmup, nsets)):
                fn()
            times[k] = []
        except (ValueError, RuntimeError) as e:  # the old route has no kernel for this direction
            print(json.dumps({"shape": name, "direction": k[0], "arm": k[1], "not_served": str(e)[:120]}), flush=True)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k in times:  # alternate the arms
            times[k].append(window(arms[k], a.iters))
    for (direction, arm), ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        nbytes = (nin + nout) * 2
        print(json.dumps({"shape": name, "direction": direction, "arm": arm, "us_median": round(med, 2),
                          "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                          "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1), "floor_bytes": int(nbytes),
                          "floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                          "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                          "share_of_hbm_rate": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                          "iters": a.iters, "rounds": a.rounds, "buffer_sets": nsets}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--no-torch", action="store_true", help="time the library kernels only")
    ap.add_argument("--no-old", action="store_true", help="skip the CXXNET_GC=0 child processes")
    ap.add_argument("--sites", default="", help="comma-separated indices into SITES (default: all seven)")
    ap.add_argument("--old", action="store_true", help="(child) time the route without the narrow-group kernels")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gconv_probe needs a GPU")
    if a.old and gemm._GC:
        raise SystemExit("--old needs CXXNET_GC=0 in the environment")
    for idx in ([int(i) for i in a.sites.split(",")] if a.sites else range(len(SITES))):
        if a.old:
            site(a, idx, True)
            continue
        if not a.no_old:
            cmd = [sys.executable, os.path.abspath(__file__), "--old", "--sites", str(idx), "--iters", str(a.iters),
                   "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--rotate-mb", str(a.rotate_mb)]
            r = subprocess.run(cmd, env=dict(os.environ, CXXNET_GC="0"), stdout=subprocess.PIPE, text=True, timeout=600)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                raise SystemExit("the CXXNET_GC=0 child failed with %d" % r.returncode)
        site(a, idx, False)


if __name__ == "__main__":
    main()
