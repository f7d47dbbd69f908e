"""batch_norm_ma kernels (csrc/kernels/bn_ma_kernels.hip) against the existing batch_norm kernels
(csrc/kernels/layer_kernels.hip): training forward + backward of each, and the new inference
forward, timed with device events in windows of --iters back-to-back calls.  The two versions
alternate inside one process, --rounds times each; the spread of a version's windows is the
noise a difference has to exceed.  One JSON line per (shape, arm), and the bytes each version
must move, computed from the shapes, over the median time against the measured HBM copy rate.
Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times
the 256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM
rate (at most 64 sets: the small matrix shape stays partly cached and is launch-bound anyway).
    python benchmarks/bn_probe.py [--iters 200] [--rounds 5] [--out profiles/bn_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
SHAPES = [("128x28x28x192", 128 * 28 * 28, 192), ("128x14x14x512", 128 * 14 * 14, 512),
          ("64x56x56x64", 64 * 56 * 56, 64), ("256x4096", 256, 4096)]
# full [rows][C] bf16 tensor passes each arm must make (reads + writes)
#   old: stats read x twice, bn_fwd reads x and writes y, x-hat and xsave; backward reads g and
#        xsave twice each (reduction, apply) and writes dx
#   new: stats and normalise read x, normalise writes y; backward reads g and x twice, writes dx
PASSES = {"old_train": 3 + 3 + 4 + 1, "new_train": 2 + 1 + 4 + 1, "new_infer": 1 + 1}


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
        raise SystemExit("bn_probe needs a GPU")
    lines = []
    for name, R, C in SHAPES:
        dev = "cuda"
        x0 = torch.randn(R, C, device=dev).to(torch.bfloat16)
        g0 = torch.randn(R, C, device=dev).to(torch.bfloat16)
        # one set = x, y, g and the old layer's xsave
        nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (4 * R * C * 2))))
        sets = [(x0.clone(), torch.empty_like(x0), g0.clone(), L.BNState(C, dev),
                 L.BNMAState(C, R, dev, torch.bfloat16, False)) for _ in range(nsets)]
        turn = {"i": 0}

        def nxt():
            turn["i"] = (turn["i"] + 1) % nsets
            return sets[turn["i"]]
        slope = torch.rand(C, device=dev) + 0.5
        bias = torch.randn(C, device=dev)
        gs, gb = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        rmean, rvar = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        # both arms overwrite x in place (x-hat / dx), as the layers do: the values drift but stay
        # finite bf16, and the kernels' time does not depend on them
        def old_train():
            x, y, g, old, _ = nxt()
            L.bn_forward(x, y, slope, bias, 1e-5, old, True)
            L.bn_backward(g, x, slope, gs, gb, old, True)

        def new_train():
            x, y, g, _, new = nxt()
            L.bn_ma_forward(x, y, slope, bias, 1e-5, 0.9, new, rmean, rvar, True)
            L.bn_ma_backward(g, x, x, slope, gs, gb, new, True)

        def new_infer():
            x, y, g, _, new = nxt()
            L.bn_ma_forward(x, y, slope, bias, 1e-5, 0.9, new, rmean, rvar, False)

        arms = {"old_train": old_train, "new_train": new_train, "new_infer": new_infer}
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(max(a.warmup, nsets)):  # (the old arm allocates each set's xsave on first use)
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in arms.items():  # alternate the versions
                for s in sets:
                    s[0].copy_(x0)
                times[k].append(window(fn, a.iters))
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            nbytes = PASSES[k] * R * C * 2
            rec = {"shape": name, "rows": R, "C": C, "arm": k, "us_median": round(med, 2), "us_min": round(ts[0], 2),
                   "us_max": round(ts[-1], 2), "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1),
                   "bytes": nbytes, "bytes_per_s": round(nbytes / (med * 1e-6), 0),
                   "share_of_hbm_rate": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                   "iters": a.iters, "rounds": a.rounds,
                   "buffer_sets": nsets}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
