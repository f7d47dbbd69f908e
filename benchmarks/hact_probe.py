"""relu6 / hsigmoid / hswish kernels (csrc/kernels/hact_kernels.hip) at the element counts of the
activation sites of MobileNet-v3-Large (models/confs/mobilenet_v3.conf) for batch 64: each kind's
forward and backward launch timed with device events in windows of --iters back-to-back calls, beside
the existing `add` kernels moving the same streams at the same n.  The arms alternate inside one
process, --rounds times each; the spread of an arm's windows is the noise a difference has to exceed,
and the spread of the add arms is the margin the new kernels are read against.  One JSON line per
(n, arm) with the bytes the arm must move, computed from n, over the median time (achieved GB/s) and
against the measured HBM copy rate.

    <kind>_fwd   one launch: reads x, writes y                       (two streams)
    <kind>_bwd   one launch: reads x and g, writes dx                (three streams)
    add_bwd1     add backward, one destination, no mask: reads g, writes d   (two streams, a copy)
    add_fwd2     add forward, two inputs, no relu: reads x0, x1, writes y    (three streams)

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times the
256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM rate
(at most 64 sets; at the small counts, the gates and the 1280 classifier input, 64 sets still fit the
cache, and what is timed there is the launch).
    python benchmarks/hact_probe.py [--iters 200] [--rounds 5] [--out profiles/hact_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH = 64
# MobileNet-v3-Large, table 1: expansion width, SE, hswish, stride of the 15 bottlenecks (input 112 x 112)
BLOCKS = [(16, 0, 0, 1), (64, 0, 0, 2), (72, 0, 0, 1), (72, 1, 0, 2), (120, 1, 0, 1), (120, 1, 0, 1), (240, 0, 1, 2),
          (200, 0, 1, 1), (184, 0, 1, 1), (184, 0, 1, 1), (480, 1, 1, 1), (672, 1, 1, 1), (672, 1, 1, 2), (960, 1, 1, 1),
          (960, 1, 1, 1)]
STREAMS = {"fwd": 2, "bwd": 3, "add_bwd1": 2, "add_fwd2": 3}


def site_counts(batch=BATCH):
    """{n: what sits there} of the net's hswish and hsigmoid sites"""
    sites = {}

    def put(n, what):
        sites.setdefault(n, []).append(what)
    hw = 112
    put(batch * hw * hw * 16, "stem hswish")
    for i, (e, se, hs, s) in enumerate(BLOCKS, 1):
        if hs:
            put(batch * hw * hw * e, "b%d expansion hswish" % i)
        hw //= s
        if hs:
            put(batch * hw * hw * e, "b%d depthwise hswish" % i)
        if se:
            put(batch * e, "b%d gate hsigmoid" % i)
    put(batch * hw * hw * 960, "tail hswish")
    put(batch * 1280, "classifier hswish")
    return dict(sorted(sites.items(), reverse=True))


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
        raise SystemExit("hact_probe needs a GPU")
    dev = "cuda"
    lines = []
    for n, what in site_counts().items():
        gen = torch.Generator(device=dev).manual_seed(n)
        x0 = (3.0 * torch.randn(n, device=dev, generator=gen)).to(torch.bfloat16)  # every piece of every kind is hit
        g0 = torch.randn(n, device=dev, generator=gen).to(torch.bfloat16)
        per_set = 4 * n * 2  # x, g, y, dx
        nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
        sets = [{"x": x0.clone(), "g": g0.clone(), "y": torch.empty_like(x0), "dx": torch.empty_like(x0)}
                for _ in range(nsets)]
        turn = {"i": 0}

        def nxt():
            turn["i"] = (turn["i"] + 1) % nsets
            return sets[turn["i"]]

        def fwd(kind):
            def run():
                s = nxt()
                L.hact_forward(kind, s["x"], s["y"])
            return run

        def bwd(kind):
            def run():
                s = nxt()
                L.hact_backward(kind, s["x"], s["g"], s["dx"])
            return run

        def add_bwd1():
            s = nxt()
            L.add_backward(s["g"], [s["dx"]], None)

        def add_fwd2():
            s = nxt()
            L.add_forward([s["x"], s["g"]], s["y"], False, None)

        arms = {"add_bwd1": add_bwd1, "add_fwd2": add_fwd2}
        for kind in L.HACT_KINDS:
            arms[kind + "_fwd"] = fwd(kind)
            arms[kind + "_bwd"] = bwd(kind)
        # the kernels agree with the torch formulas before anything is timed
        s = sets[0]
        for kind, f in (("relu6", torch.nn.functional.relu6), ("hsigmoid", torch.nn.functional.hardsigmoid),
                        ("hswish", torch.nn.functional.hardswish)):
            L.hact_forward(kind, s["x"], s["y"])
            xa = s["x"].float().requires_grad_()
            ya = f(xa)
            ya.backward(s["g"].float())
            assert (s["y"].float() - ya.detach()).abs().max() <= 2.0 ** -7 * ya.detach().abs().max(), kind
            L.hact_backward(kind, s["x"], s["g"], s["dx"])
            assert (s["dx"].float() - xa.grad).abs().max() <= 2.0 ** -7 * xa.grad.abs().max(), kind
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(max(a.warmup, nsets)):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in arms.items():  # alternate the arms
                times[k].append(window(fn, a.iters))
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            nbytes = 2 * n * STREAMS[k if k.startswith("add") else k[-3:]]
            rec = {"n": n, "sites": what, "arm": k, "streams": nbytes // (2 * n), "us_median": round(med, 2),
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
