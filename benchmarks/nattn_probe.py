"""Neighbourhood attention kernels (csrc/kernels/nattn_kernels.hip) at NAT-Mini's four sites, batch
64, kernel 7, d = 32: 56^2 x 2 heads, 28^2 x 4, 14^2 x 8 and 7^2 x 16 -- forward and backward,
against a torch formulation of the same function on the same tensors (an index gather of every
pixel's 49 keys and values, the biased logits by einsum, a softmax, with its autograd backward), and
against a plain device copy of the bytes a direction has to move (forward 4 C per row, backward
7 C).  Timed as benchmarks/attn_probe.py does: device events around windows of --iters back-to-back
calls after a warm-up, the arms alternating round by round, consecutive calls on different buffer
sets (--rotate-mb in all, at most 64 sets); one JSON line per (case, direction, arm).  The backward
arm writes its gradient out of place; --step also times whole training steps of nat_mini.conf at
batch 64.
    python benchmarks/nattn_probe.py [--iters 20] [--rounds 5] [--step]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.attn_probe import window  # noqa: E402
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

D, K = 32, 7
CASES = [(64, 56, 2), (64, 28, 4), (64, 14, 8), (64, 7, 16)]  # (batch, H = W, nhead)


def case(a, B, H, nhead):
    dev, C = "cuda", nhead * D
    rows = B * H * H
    gen = torch.Generator(device=dev).manual_seed(H + nhead)
    x0 = torch.randn(rows, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    g0 = torch.randn(rows, C, device=dev, generator=gen).to(torch.bfloat16)
    bias = torch.randn(nhead, (2 * K - 1) ** 2, device=dev, generator=gen)
    gbias = torch.zeros_like(bias)
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // (18 * rows * C * 2))))
    sets = [{"x": x0.clone(), "g": g0.clone(), "o": torch.empty_like(g0), "dx": torch.empty_like(x0),
             "st": L.NAttnState(B, H, H, C, nhead, K, dev)} for _ in range(nsets)]
    for s in sets:
        L.nattn_forward(s["x"], s["o"], bias, B, nhead, s["st"])  # the backward arm needs every set's lse
        s["c_in"] = torch.cat([s["x"], s["g"]], 1)[:, :7 * C // 2].contiguous()  # [rows][3.5 C]
        s["c_out"] = torch.empty_like(s["c_in"])
    nbr, rel = sets[0]["st"].index(dev)
    add = bias[:, rel].to(torch.bfloat16)  # [nhead, H W, 49], built once
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def compose(x):
        xv = x.view(B, H * H, 3, nhead, D)
        k, v = xv[:, :, 1][:, nbr], xv[:, :, 2][:, nbr]  # [B, H W, 49, nhead, D]: the unfold-style gather
        s = torch.einsum("bphd,bpjhd->bhpj", xv[:, :, 0], k) * D ** -0.5 + add
        return torch.einsum("bhpj,bpjhd->bphd", torch.softmax(s.float(), -1).to(x.dtype), v).reshape(rows, C)

    def compose_bwd(s):
        x = s["x"].detach().requires_grad_()
        return torch.autograd.grad(compose(x), x, s["g"])

    arms = {
        ("forward", "nattn"): lambda: (lambda s: L.nattn_forward(s["x"], s["o"], bias, B, nhead, s["st"]))(nxt()),
        ("backward", "nattn"): lambda: (lambda s: L.nattn_backward(s["g"], s["x"], s["dx"], bias, gbias, B, nhead,
                                                                   s["st"], True))(nxt()),
        ("forward", "torch"): lambda: compose(nxt()["x"]),
        ("fwd+backward", "torch"): lambda: compose_bwd(nxt()),  # (autograd reruns nothing: forward + backward)
        ("forward", "copy"): lambda: (lambda s: s["c_out"].view(-1)[:rows * 2 * C].copy_(s["c_in"].view(-1)[:rows * 2 * C]))(nxt()),
        ("backward", "copy"): lambda: (lambda s: s["c_out"].copy_(s["c_in"]))(nxt()),
    }
    # the arms agree before anything is timed
    err = (sets[0]["o"].float() - compose(sets[0]["x"]).float()).abs().max().item()
    assert err < 0.05, err
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, a.iters))
    for (direction, arm), ts in times.items():
        ts = sorted(ts)
        rec = {"case": "B%d %dx%d nhead%d k%d" % (B, H, H, nhead, K), "direction": direction, "arm": arm,
               "us_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
               "sets": nsets}
        if arm == "copy":
            rec["bytes"] = (4 if direction == "forward" else 7) * rows * C * 2
        print(json.dumps(rec), flush=True)


def step_time(a):
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("nat_mini", []) if not k.startswith("metric")] + [
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
    print(json.dumps({"case": "nat_mini step B64", "ms_median": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2),
                      "ms_max": round(ts[-1], 2), "img_per_s": round(64e3 / ts[len(ts) // 2], 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nattn_probe: no GPU")
    for c in CASES:
        case(a, *c)
    if a.step:
        step_time(a)
