"""group_norm kernels (csrc/kernels/gn_kernels.hip) beside the batch_norm_ma kernels
(csrc/kernels/bn_ma_kernels.hip) on the same tensors: forward and backward of each at the distinct
(HW, C) shapes of ResNet-18-GN, at batch 64 and batch 8, timed with device events in windows of
--iters back-to-back calls.  The four arms alternate inside one process, --rounds times each; the
spread of an arm's windows is the noise a difference has to exceed.  The two forwards move the same
bytes (x read twice, y written), the two backwards too (g and x read twice each, dx written over x),
so group_norm should land at batch_norm_ma's time.  One JSON line per (shape, arm) with the bytes
over the median time against the measured HBM copy rate, then one line per (shape, direction) with
the ratio gn / bn and the larger of the two arms' spreads.
Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times
the 256 MB Infinity Cache -- so that a call finds none of its tensors cached (at most 64 sets: the
small shapes stay partly cached and are launch-bound anyway).
    python benchmarks/gn_probe.py [--iters 100] [--rounds 5] [--out profiles/gn_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
GROUPS = 32
# (H W, C) of the group_norm layers of models/confs/resnet18_gn.conf: the stem, stages 2 to 5
MAPS = [(112 * 112, 64), (56 * 56, 64), (28 * 28, 128), (14 * 14, 256), (7 * 7, 512)]
BATCHES = (64, 8)
# full [B][HW][C] bf16 tensor passes (reads + writes): the same for both layers
PASSES = {"fwd": 2 + 1, "bwd": 4 + 1}


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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--only", default="", help="run the shapes whose name BxHWxC contains this text")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gn_probe needs a GPU")
    dev = "cuda"
    lines = []
    for B in BATCHES:
        for HW, C in MAPS:
            name = "%dx%dx%d" % (B, HW, C)
            if a.only not in name:
                continue
            n = B * HW * C
            x0 = torch.randn(B, HW, C, device=dev).to(torch.bfloat16)
            g0 = torch.randn(B, HW, C, device=dev).to(torch.bfloat16)
            # one set = x, y, g and each layer's state
            nsets = max(2, min(64, -(-a.rotate_mb * (1 << 20) // (3 * n * 2))))
            sets = [(x0.clone(), torch.empty_like(x0), g0.clone(), L.GNState(B, HW, C, GROUPS, dev),
                     L.BNMAState(C, B * HW, dev, torch.bfloat16, False)) for _ in range(nsets)]
            turn = {"i": 0}

            def nxt():
                turn["i"] = (turn["i"] + 1) % nsets
                return sets[turn["i"]]
            slope = torch.rand(C, device=dev) + 0.5
            bias = torch.randn(C, device=dev)
            gs, gb = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            rmean, rvar = torch.zeros(C, device=dev), torch.ones(C, device=dev)

            def gn_fwd():
                x, y, g, gn, _ = nxt()
                L.gn_forward(x, y, slope, bias, 1e-5, gn)

            # the backward arms overwrite x with dx, as the layers do: the values drift but stay
            # finite bf16 (the statistics are those of the last forward), and the time does not
            # depend on them
            def gn_bwd():
                x, y, g, gn, _ = nxt()
                L.gn_backward(g, x, x, slope, gs, gb, gn, True)

            def bn_fwd():
                x, y, g, _, bn = nxt()
                L.bn_ma_forward(x.view(-1, C), y.view(-1, C), slope, bias, 1e-5, 0.9, bn, rmean, rvar, True)

            def bn_bwd():
                x, y, g, _, bn = nxt()
                L.bn_ma_backward(g.view(-1, C), x.view(-1, C), x.view(-1, C), slope, gs, gb, bn, True)

            arms = {"gn_fwd": gn_fwd, "bn_fwd": bn_fwd, "gn_bwd": gn_bwd, "bn_bwd": bn_bwd}
            times = {k: [] for k in arms}
            for fn in arms.values():  # every set's statistics exist before a backward is timed
                for _ in range(max(a.warmup, nsets)):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, fn in arms.items():  # alternate the arms
                    for s in sets:
                        s[0].copy_(x0)
                    times[k].append(window(fn, a.iters))
            stat = {}
            for k, ts in times.items():
                ts = sorted(ts)
                med = ts[len(ts) // 2]
                nbytes = PASSES[k[3:]] * n * 2
                stat[k] = (med, 100 * (ts[-1] - ts[0]) / med)
                rec = {"shape": name, "B": B, "HW": HW, "C": C, "groups": GROUPS, "arm": k, "us_median": round(med, 2),
                       "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2), "spread_pct": round(stat[k][1], 1),
                       "bytes": nbytes, "bytes_per_s": round(nbytes / (med * 1e-6), 0),
                       "share_of_hbm_rate": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3), "iters": a.iters,
                       "rounds": a.rounds, "buffer_sets": nsets}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            for d in ("fwd", "bwd"):
                (tg, sg), (tb, sb) = stat["gn_" + d], stat["bn_" + d]
                rec = {"shape": name, "direction": d, "gn_us": round(tg, 2), "bn_us": round(tb, 2),
                       "ratio_gn_over_bn": round(tg / tb, 3), "larger_spread_pct": round(max(sg, sb), 1),
                       "within_spread": bool(tg / tb - 1.0 <= max(sg, sb) / 100.0)}
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
