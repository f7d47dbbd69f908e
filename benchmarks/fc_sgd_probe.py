"""The fc weight-gradient GEMM fused with the SGD step (ops.fc_backward_weight_sgd, table key
"fws") on AlexNet's fc6 / fc7 / fc8 at batch 256 and VGG-16's fc6 at batch 64, for each MN-major
tile and each setting of the streaming kernel (cxn_gemm_set_sgd_stream: 0 = the tile kernel,
1 = the stream where the library picks it, 2 = the stream on every shape; "2:N" = with N blocks,
N >= the number of 64 x 128 chunks gives one chunk per block): median time and the parameter
stream rate (18 bytes per parameter: fp32 w and momentum read and written, the bf16 shadow
written).  Interleaved rounds in one process.

    python benchmarks/fc_sgd_probe.py [--tiles 1,2,17,23,40,41] [--stream 0,1] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd import native, ops  # noqa: E402
from cxxnet_amd.ops import gemm as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="-1,1,2,17,23,40,41")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--groups", default="8", help="tile-order groups (ops.gemm.set_tile_group) to A/B")
    ap.add_argument("--flush", type=int, default=0,
                    help="overwrite 1 GB before every timed call (w / m then come from HBM; the fill's dirty lines "
                         "are written back during the call, so times read high)")
    ap.add_argument("--ops", default="fc6,fc7")
    ap.add_argument("--stream", default="0", help="streaming-kernel settings to A/B (the tile only matters at 0)")
    a = ap.parse_args()
    junk = torch.empty(1 << 28, device="cuda") if a.flush else None
    k = native.kernels()
    for name, nin, nout, B in (("fc6", 9216, 4096, a.batch), ("fc7", 4096, 4096, a.batch), ("fc8", 4096, 1000, a.batch),
                               ("vgg_fc6", 25088, 4096, 64)):
        if name not in a.ops.split(","):
            continue
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, nin, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(B, nout, device="cuda", generator=g).to(torch.bfloat16)
        w = torch.randn(nout, nin, device="cuda", generator=g) * 0.02
        m = torch.zeros(nout, nin, device="cuda")
        wb = w.to(torch.bfloat16)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        arms = [(int(t), int(gi), sm) for sm in a.stream.split(",")
                for t in (a.tiles.split(",") if sm == "0" else ["-1"]) for gi in a.groups.split(",")]
        times = {arm: [] for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                t, gi, sm = arm
                k.cxn_gemm_set_sgd_stream(int(sm.split(":")[0]))
                k.cxn_gemm_set_sgd_stream_blocks(int(sm.split(":")[1]) if ":" in sm else 0)
                G.set_glds(True, t)
                G.set_tile_group(gi)
                assert ops.fc_backward_weight_sgd(x, dy, w, m, wb, 1e-6, 0.0, 0.9, 0.0)
                torch.cuda.synchronize()
                tot = 0.0
                for _ in range(a.iters):
                    if junk is not None:
                        junk.fill_(1.0)
                    s.record()
                    ops.fc_backward_weight_sgd(x, dy, w, m, wb, 1e-6, 0.0, 0.9, 0.0)
                    e.record()
                    e.synchronize()
                    tot += s.elapsed_time(e) * 1e3
                times[arm].append(tot / a.iters)
        G.set_glds(True, -1)
        G.set_tile_group(8)
        k.cxn_gemm_set_sgd_stream(1)
        k.cxn_gemm_set_sgd_stream_blocks(0)
        rec = {"op": name, "batch": B, "flush": a.flush}
        for (t, gi, sm), v in times.items():
            us = statistics.median(v)
            tag = ((f"t{t}" if t >= 0 else "tdef") if sm == "0" else "s" + sm.replace(":", "b")) + f"g{gi}"
            rec[f"{tag}_us"] = round(us, 1)
            rec[f"{tag}_TBps"] = round(18 * nin * nout / us / 1e6, 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
