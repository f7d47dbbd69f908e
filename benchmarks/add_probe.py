"""add kernels (csrc/kernels/add_kernels.hip) against the composition of existing kernels, at the
four block-tail shapes of ResNet-18 for batch 64 (two inputs, relu): forward and backward launch
of each, timed with device events in windows of --iters back-to-back calls.  The versions alternate
inside one process, --rounds times each; the spread of a version's windows is the noise a
difference has to exceed.  One JSON line per (shape, arm) with the bytes the arm must move,
computed from the shapes, over the median time (achieved GB/s) and against the measured HBM copy
rate.

    new forward    one launch: reads x0, x1, writes y and one mask bit per element
    old forward    ops.sum_into(t, [x0, x1]), then the relu forward t -> y.  The spare buffer t
                   keeps the sum, whose sign is the sign of y: what the relu backward needs after
                   the node's buffer has been overwritten by its gradient
    new backward   one launch: reads g and the mask, writes d0 and d1
    old backward   the relu backward (t, g) -> d0, then ops.fanout_copy(d0, [d1])

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times
the 256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM
rate (at most 64 sets).
    python benchmarks/add_probe.py [--iters 200] [--rounds 5] [--out profiles/add_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd import ops  # noqa: E402
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH, N = 64, 2
SHAPES = [("64x56x56x64", BATCH * 56 * 56 * 64), ("64x28x28x128", BATCH * 28 * 28 * 128),
          ("64x14x14x256", BATCH * 14 * 14 * 256), ("64x7x7x512", BATCH * 7 * 7 * 512)]
# bytes per element each arm must move (bf16 tensors, one mask bit per element)
BYTES = {"new_fwd": (N + 1) * 2 + 1 / 8,      # N inputs, y, the mask
         "old_fwd": (N + 1) * 2 + 4,          # N inputs, t; t again, y
         "new_bwd": 2 + 1 / 8 + 2 * N,        # g, the mask, N destinations
         "old_bwd": 6 + 2 + 2 * (N - 1)}      # t, g, d0; d0 again, the other destinations
LAUNCHES = {"new_fwd": 1, "old_fwd": 2, "new_bwd": 1, "old_bwd": 2}


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
        raise SystemExit("add_probe needs a GPU")
    dev = "cuda"
    lines = []
    for name, n in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(n)
        src = [torch.randn(n, device=dev, generator=gen).to(torch.bfloat16) for _ in range(N + 1)]
        # one set = x0, x1, y, t, g, d0, d1 and the mask
        per_set = (2 * N + 3) * n * 2 + n // 8
        nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
        sets = []
        for _ in range(nsets):
            s = {"x": [t.clone() for t in src[:N]], "g": src[N].clone(), "y": torch.empty_like(src[0]),
                 "t": torch.empty_like(src[0]), "d": [torch.empty_like(src[0]) for _ in range(N)],
                 "st": L.AddState(n, dev, True)}
            sets.append(s)
        turn = {"i": 0}

        def nxt():
            turn["i"] = (turn["i"] + 1) % nsets
            return sets[turn["i"]]

        def new_fwd():
            s = nxt()
            L.add_forward(s["x"], s["y"], True, s["st"])

        def old_fwd():
            s = nxt()
            ops.sum_into(s["t"], s["x"])
            ops.act_forward("relu", s["t"], s["y"])

        def new_bwd():
            s = nxt()
            L.add_backward(s["g"], s["d"], s["st"])

        def old_bwd():
            s = nxt()
            ops.act_backward("relu", s["t"], s["g"], s["d"][0])
            ops.fanout_copy(s["d"][0], s["d"][1:])

        arms = {"new_fwd": new_fwd, "old_fwd": old_fwd, "new_bwd": new_bwd, "old_bwd": old_bwd}
        # the two versions agree before anything is timed
        s = sets[0]
        L.add_forward(s["x"], s["y"], True, s["st"])
        want = s["y"].clone()
        L.add_backward(s["g"], s["d"], s["st"])
        dwant = s["d"][0].clone()
        assert torch.equal(s["d"][1], dwant)
        ops.sum_into(s["t"], s["x"])
        ops.act_forward("relu", s["t"], s["y"])
        assert torch.equal(s["y"], want), "the composition computes another y"
        ops.act_backward("relu", s["t"], s["g"], s["d"][0])
        ops.fanout_copy(s["d"][0], s["d"][1:])
        assert torch.equal(s["d"][0].float(), dwant.float()) and torch.equal(s["d"][1].float(), dwant.float())
        times = {k: [] for k in arms}
        for fn in arms.values():  # (forward arms first: every set's t and mask are written before a backward reads them)
            for _ in range(max(a.warmup, nsets)):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in arms.items():  # alternate the versions
                times[k].append(window(fn, a.iters))
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            nbytes = BYTES[k] * n
            rec = {"shape": name, "n": n, "inputs": N, "arm": k, "launches": LAUNCHES[k], "us_median": round(med, 2),
                   "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                   "spread_pct": round(100 * (ts[-1] - ts[0]) / med, 1), "bytes_per_element": BYTES[k],
                   "bytes": int(nbytes), "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                   "share_of_hbm_rate": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                   "iters": a.iters, "rounds": a.rounds, "buffer_sets": nsets}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
