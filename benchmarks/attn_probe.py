"""Attention kernels (csrc/kernels/attn_kernels.hip) at nhead = 6, d = 64 (CPVT-S / DeiT-S):
T = 196 at batch 64 and 256, T = 49 and T = 576 at batch 64 -- forward and backward, against
torch.nn.functional.scaled_dot_product_attention (with its autograd backward) on the same strided
q / k / v views of the [B T][3 C] buffer, and against a plain device copy of the bytes a direction
has to move (forward: qkv in, O out = 4 C per row; backward: qkv and dO in, dqkv out = 7 C per
row).  Timed with device events in windows of --iters back-to-back calls after a warm-up, the arms
alternating round by round; one JSON line per (case, direction, arm) with the median and the
spread of its windows.  Consecutive calls work on different buffer sets, --rotate-mb (1024) of
them in all, so that a call finds none of its tensors in the 256 MB Infinity Cache (at most 64
sets).  --step also times whole training steps of cpvt_small.conf at batch 64.
    python benchmarks/attn_probe.py [--iters 20] [--rounds 5] [--step]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

NHEAD, D = 6, 64
CASES = [(64, 196), (256, 196), (64, 49), (64, 576)]  # (batch, T)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def case(a, B, T):
    dev, C = "cuda", NHEAD * D
    rows = B * T
    gen = torch.Generator(device=dev).manual_seed(B + T)
    x0 = torch.randn(rows, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    g0 = torch.randn(rows, C, device=dev, generator=gen).to(torch.bfloat16)
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (18 * rows * C * 2))))
    sets = [{"x": x0.clone(), "g": g0.clone(), "o": torch.empty_like(g0), "dx": torch.empty_like(x0),
             "st": L.AttnState(B, T, C, NHEAD, dev)} for _ in range(nsets)]
    for s in sets:
        L.attn_forward(s["x"], s["o"], B, NHEAD, s["st"])  # the backward arm needs every set's lse
        s["c_in"] = torch.cat([s["x"], s["g"]], 1)[:, :7 * C // 2].contiguous()  # [rows][3.5 C]
        s["c_out"] = torch.empty_like(s["c_in"])
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def heads(x):  # q, k, v [B, nhead, T, d] strided views
        v = x.view(B, T, 3, NHEAD, D).permute(2, 0, 3, 1, 4)
        return v[0], v[1], v[2]

    def sdpa_bwd(s):
        q, k, v = (t.detach().requires_grad_() for t in heads(s["x"]))
        o = F.scaled_dot_product_attention(q, k, v)
        return torch.autograd.grad(o, (q, k, v), s["g"].view(B, T, NHEAD, D).permute(0, 2, 1, 3))

    arms = {
        ("forward", "attn"): lambda: (lambda s: L.attn_forward(s["x"], s["o"], B, NHEAD, s["st"]))(nxt()),
        ("backward", "attn"): lambda: (lambda s: L.attn_backward(s["g"], s["x"], s["dx"], B, NHEAD, s["st"], True))(nxt()),
        ("backward_inplace", "attn"): lambda: (lambda s: L.attn_backward(s["g"], s["dx"], s["dx"], B, NHEAD, s["st"], True))(nxt()),
        ("forward", "sdpa"): lambda: F.scaled_dot_product_attention(*heads(nxt()["x"])),
        ("fwd+backward", "sdpa"): lambda: sdpa_bwd(nxt()),  # (autograd reruns nothing: forward + backward)
        # the bytes of a direction as one contiguous copy: forward 3 C in + C out = 2 C copied,
        # backward 4 C in + 3 C out = 3.5 C copied (per row)
        ("forward", "copy"): lambda: (lambda s: s["c_out"].view(-1)[:rows * 2 * C].copy_(s["c_in"].view(-1)[:rows * 2 * C]))(nxt()),
        ("backward", "copy"): lambda: (lambda s: s["c_out"].copy_(s["c_in"]))(nxt()),
    }
    # the arms agree before anything is timed
    s = sets[0]
    ref = F.scaled_dot_product_attention(*heads(s["x"])).permute(0, 2, 1, 3).reshape(rows, C)
    err = (s["o"].float() - ref.float()).abs().max().item()
    assert err < 0.05, err
    for s in sets:
        s["dx"].copy_(s["x"])  # the in-place arm reads dx as qkv: keep it finite input on every call
    out = []
    times = {k: [] for k in arms}
    for k, fn in arms.items():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in arms.items():
            if k[0] == "backward_inplace":
                for s in sets:
                    s["dx"].copy_(s["x"])
                torch.cuda.synchronize()
            times[k].append(window(fn, a.iters if k[0] != "backward_inplace" else min(a.iters, nsets)))
    for (direction, arm), ts in times.items():
        ts = sorted(ts)
        rec = {"case": "B%d T%d nhead%d d%d" % (B, T, NHEAD, D), "direction": direction, "arm": arm,
               "us_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
               "sets": nsets}
        if arm == "copy":
            rec["bytes"] = (4 if direction == "forward" else 7) * rows * C * 2
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def step_time(a):
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("cpvt_small", []) if not k.startswith("metric")] + [
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
    print(json.dumps({"case": "cpvt_small step B64", "ms_median": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2),
                      "ms_max": round(ts[-1], 2), "img_per_s": round(64e3 / ts[len(ts) // 2], 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_probe: no GPU")
    for B, T in CASES:
        case(a, B, T)
    if a.step:
        step_time(a)
