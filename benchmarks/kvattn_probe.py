"""kv_attention kernels (csrc/kernels/kvattn_kernels.hip) at PVTv2-b1's four sites, batch 64, d = 64:
(Tq, Tk, nhead) = (3136, 49, 1), (784, 49, 2), (196, 49, 5), (49, 49, 8) -- forward and backward,
out of place and in place, against torch.nn.functional.scaled_dot_product_attention (with its
autograd backward) on strided views of the same q / kv buffers, against a plain device copy of the
bytes a direction has to move (forward: q in, O out; backward: q and dO in, dQ out; kv is small),
and at the (49, 49) site against the `attention` kernels on an equivalent fused [B T][3 C] buffer.
Method as benchmarks/attn_probe.py: device events around windows of --iters back-to-back calls
after a warm-up, the arms alternating round by round, consecutive calls on different buffer sets
(--rotate-mb of them in all, at most 64); one JSON line per (case, direction, arm) with the
median and the spread of its windows.  --step also times training steps of pvt_v2_b1.conf.
    python benchmarks/kvattn_probe.py [--iters 20] [--rounds 5] [--step]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attn_probe import window  # noqa: E402
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

B, D = 64, 64
CASES = [(3136, 49, 1), (784, 49, 2), (196, 49, 5), (49, 49, 8)]  # (Tq, Tk, nhead)


def case(a, Tq, Tk, nhead):
    dev, C = "cuda", nhead * D
    rows, krows = B * Tq, B * Tk
    gen = torch.Generator(device=dev).manual_seed(Tq + nhead)
    q0 = torch.randn(rows, C, device=dev, generator=gen).to(torch.bfloat16)
    kv0 = torch.randn(krows, 2 * C, device=dev, generator=gen).to(torch.bfloat16)
    g0 = torch.randn(rows, C, device=dev, generator=gen).to(torch.bfloat16)
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (10 * rows * C * 2))))
    sets = [{"q": q0.clone(), "kv": kv0.clone(), "g": g0.clone(), "o": torch.empty_like(g0), "dq": torch.empty_like(q0),
             "dkv": torch.empty_like(kv0), "iq": q0.clone(), "ikv": kv0.clone(), "c_in": torch.cat([q0, g0], 1),
             "c_out": torch.empty(rows, 2 * C, device=dev, dtype=torch.bfloat16),
             "st": L.KVAttnState(B, Tq, Tk, C, nhead, dev)} for _ in range(nsets)]
    same = Tq == Tk  # the fused-buffer arm: `attention` on [B T][3 C]
    if same:
        for s in sets:
            s["x"] = torch.cat([s["q"], s["kv"]], 1)
            s["dx"] = torch.empty_like(s["x"])
            s["ast"] = L.AttnState(B, Tq, C, nhead, dev)
            L.attn_forward(s["x"], s["o"], B, nhead, s["ast"])
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def heads(s):  # q [B, nhead, Tq, d], k, v [B, nhead, Tk, d]: strided views
        kv = s["kv"].view(B, Tk, 2, nhead, D).permute(2, 0, 3, 1, 4)
        return s["q"].view(B, Tq, nhead, D).permute(0, 2, 1, 3), kv[0], kv[1]

    def sdpa_bwd(s):
        q, k, v = (t.detach().requires_grad_() for t in heads(s))
        o = F.scaled_dot_product_attention(q, k, v)
        return torch.autograd.grad(o, (q, k, v), s["g"].view(B, Tq, nhead, D).permute(0, 2, 1, 3))

    def on(fn):
        return lambda: fn(nxt())

    arms = {
        ("forward", "kvattn"): on(lambda s: L.kvattn_forward(s["q"], s["kv"], s["o"], B, nhead, s["st"])),
        ("backward", "kvattn"): on(lambda s: L.kvattn_backward(s["g"], s["q"], s["kv"], s["dq"], s["dkv"], B, nhead, s["st"], True)),
        ("backward_inplace", "kvattn"): on(lambda s: L.kvattn_backward(s["g"], s["iq"], s["ikv"], s["iq"], s["ikv"], B, nhead, s["st"], True)),
        ("forward", "sdpa"): on(lambda s: F.scaled_dot_product_attention(*heads(s))),
        ("fwd+backward", "sdpa"): on(sdpa_bwd),
        # the bytes of a direction as one contiguous copy: forward C in + C out, backward 2 C in + C out (per row)
        ("forward", "copy"): on(lambda s: s["c_out"].view(-1)[:rows * C].copy_(s["c_in"].view(-1)[:rows * C])),
        ("backward", "copy"): on(lambda s: s["c_out"].view(-1)[:rows * 3 * C // 2].copy_(s["c_in"].view(-1)[:rows * 3 * C // 2])),
    }
    if same:
        arms[("forward", "attention")] = on(lambda s: L.attn_forward(s["x"], s["o"], B, nhead, s["ast"]))
        arms[("backward", "attention")] = on(lambda s: L.attn_backward(s["g"], s["x"], s["dx"], B, nhead, s["ast"], True))
    s = sets[0]  # the arms agree before anything is timed
    L.kvattn_forward(s["q"], s["kv"], s["o"], B, nhead, s["st"])
    ref = F.scaled_dot_product_attention(*heads(s)).permute(0, 2, 1, 3).reshape(rows, C)
    err = (s["o"].float() - ref.float()).abs().max().item()
    assert err < 0.05, err
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in arms.items():
            if k[0] == "backward_inplace":  # it reads its own output as input: keep that finite
                for s in sets:
                    s["iq"].copy_(s["q"])
                    s["ikv"].copy_(s["kv"])
                torch.cuda.synchronize()
            times[k].append(window(fn, a.iters if k[0] != "backward_inplace" else min(a.iters, nsets)))
    for (direction, arm), ts in times.items():
        ts = sorted(ts)
        rec = {"case": "B%d Tq%d Tk%d nhead%d d%d" % (B, Tq, Tk, nhead, D), "direction": direction, "arm": arm,
               "us_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2), "sets": nsets}
        if arm == "copy":
            rec["bytes"] = (2 if direction == "forward" else 3) * rows * C * 2
        print(json.dumps(rec), flush=True)


def step_time(a):
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("pvt_v2_b1", []) if not k.startswith("metric")] + [
            ("batch_size", "64"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1")]:
        tr.set_param(k, v)
    tr.init_model()
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(64, 3, 224, 224, generator=g), torch.randint(0, 1000, (64, 1), generator=g).float())
    for _ in range(5):
        tr.update(b)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(10):
            tr.update(b)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 100)  # ms per step
    ts.sort()
    print(json.dumps({"case": "pvt_v2_b1 step B64", "ms_median": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2),
                      "ms_max": round(ts[-1], 2), "img_per_s": round(64e3 / ts[len(ts) // 2], 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kvattn_probe: no GPU")
    for c in CASES:
        case(a, *c)
    if a.step:
        step_time(a)
