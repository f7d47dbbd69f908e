"""silu kernels (csrc/kernels/silu_kernels.hip) and the drop_path kernel (csrc/kernels/droppath_kernels.hip)
at the sizes of their sites in EfficientNet-B0 (models/confs/efficientnet_b0.conf) for batch 64, timed
with device events in windows of --iters back-to-back calls, beside kernels already in the tree that move
the same bytes.  The arms alternate inside one process, --rounds times each; the spread of an arm's
windows is the noise a difference has to exceed.  One JSON line per (size, arm) with the bytes the arm
must move over the median time (achieved GB/s) and against the measured HBM copy rate.

  silu, at the element counts of the 49 silu sites:
    silu_fwd / silu_bwd          one launch: reads x, writes y / reads x and g, writes dx
    hswish_fwd / hswish_bwd      the hswish kernels (hact_kernels.hip) on the same buffers: the same streams
    hswish_fwd_rep / hswish_bwd_rep   the same two arms once more: what two runs of ONE kernel differ by in
                                 this process is the margin silu is read against
  drop_path, at the [64][n] of its 9 sites (the residual branches), in place:
    drop_path_0.05 / drop_path_0.2   drop_prob 0.05 / 0.2: a kept sample is read and written, a dropped one
                                 only written; bytes are counted from the samples the mask keeps
    add_bwd1                     add backward, one destination, no mask: reads g, writes d (two streams)

Consecutive calls work on different buffer sets, --rotate-mb (1024) of them in all -- four times the
256 MB Infinity Cache -- so that a call finds none of its tensors cached and the rate is an HBM rate (at
most 64 sets; at the small counts 64 sets still fit the cache, and what is timed there is the launch).
    python benchmarks/silu_probe.py [--iters 200] [--rounds 5] [--out profiles/silu_probe.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd.ops import layer_ops as L  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 spec)
BATCH = 64
# EfficientNet-B0, table 1: expansion, kernel, stride, channels, blocks of the 7 stages (input 112 x 112 x 32)
STAGES = [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3), (6, 5, 2, 192, 4),
          (6, 3, 1, 320, 1)]


def sites(batch=BATCH):
    """({n: what} of the silu sites, {n per sample: what} of the drop_path sites)"""
    silu, dpath = {}, {}

    def put(d, n, what):
        d.setdefault(n, []).append(what)
    hw, cin, i = 112, 32, 0
    put(silu, batch * hw * hw * 32, "stem")
    for exp, _, stride, cout, nblk in STAGES:
        for j in range(nblk):
            i += 1
            s = stride if j == 0 else 1
            e = cin * exp
            if exp != 1:
                put(silu, batch * hw * hw * e, "b%d expansion" % i)
            hw //= s
            put(silu, batch * hw * hw * e, "b%d depthwise" % i)
            put(silu, batch * ((-(-cin // 4) + 7) // 8 * 8), "b%d squeeze" % i)
            if s == 1 and cin == cout:
                put(dpath, hw * hw * cout, "b%d" % i)
            cin = cout
    put(silu, batch * hw * hw * 1280, "head")
    assert sum(len(v) for v in silu.values()) == 49 and sum(len(v) for v in dpath.values()) == 9
    return dict(sorted(silu.items(), reverse=True)), dict(sorted(dpath.items(), reverse=True))


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def measure(arms, nbytes, a, nsets, head):
    """time every arm of one size; returns its JSON lines"""
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(max(a.warmup, nsets)):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in arms.items():  # alternate the arms
            times[k].append(window(fn, a.iters))
    lines = []
    for k, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        rec = dict(head, arm=k, us_median=round(med, 2), us_min=round(ts[0], 2), us_max=round(ts[-1], 2),
                   spread_pct=round(100 * (ts[-1] - ts[0]) / med, 1), bytes=int(nbytes[k]),
                   gb_per_s=round(nbytes[k] / (med * 1e-6) / 1e9, 1),
                   share_of_hbm_rate=round(nbytes[k] / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                   iters=a.iters, rounds=a.rounds, buffer_sets=nsets)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    return lines


def silu_size(n, what, a, dev):
    gen = torch.Generator(device=dev).manual_seed(n)
    x0 = (3.0 * torch.randn(n, device=dev, generator=gen)).to(torch.bfloat16)
    g0 = torch.randn(n, device=dev, generator=gen).to(torch.bfloat16)
    per_set = 4 * n * 2  # x, g, y, dx
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
    sets = [{"x": x0.clone(), "g": g0.clone(), "y": torch.empty_like(x0), "dx": torch.empty_like(x0)}
            for _ in range(nsets)]
    turn = {"i": 0}

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def silu_fwd():
        s = nxt()
        L.silu_forward(s["x"], s["y"])

    def silu_bwd():
        s = nxt()
        L.silu_backward(s["x"], s["g"], s["dx"])

    def hswish_fwd():
        s = nxt()
        L.hact_forward("hswish", s["x"], s["y"])

    def hswish_bwd():
        s = nxt()
        L.hact_backward("hswish", s["x"], s["g"], s["dx"])

    # the kernels agree with torch's silu before anything is timed
    s = sets[0]
    L.silu_forward(s["x"], s["y"])
    xa = s["x"].float().requires_grad_()
    ya = torch.nn.functional.silu(xa)
    ya.backward(s["g"].float())
    assert (s["y"].float() - ya.detach()).abs().max() <= 2.0 ** -7 * ya.detach().abs().max()
    L.silu_backward(s["x"], s["g"], s["dx"])
    assert (s["dx"].float() - xa.grad).abs().max() <= 2.0 ** -7 * xa.grad.abs().max()
    arms = {"silu_fwd": silu_fwd, "hswish_fwd": hswish_fwd, "hswish_fwd_rep": hswish_fwd,
            "silu_bwd": silu_bwd, "hswish_bwd": hswish_bwd, "hswish_bwd_rep": hswish_bwd}
    nbytes = {k: 2 * n * (2 if "fwd" in k else 3) for k in arms}
    return measure(arms, nbytes, a, nsets, {"layer": "silu", "n": n, "sites": what})


def drop_path_size(n, what, a, dev):
    B = BATCH
    gen = torch.Generator(device=dev).manual_seed(n)
    x0 = torch.randn(B, n, device=dev, generator=gen).to(torch.bfloat16)
    per_set = 2 * B * n * 2  # x (in place), and g / d of the add arm
    nsets = max(1, min(64, -(-a.rotate_mb * (1 << 20) // per_set)))
    sets = [{"x": x0.clone(), "d": torch.empty_like(x0)} for _ in range(nsets)]
    turn = {"i": 0}
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    seed = 12345

    def nxt():
        turn["i"] = (turn["i"] + 1) % nsets
        return sets[turn["i"]]

    def dp(pkeep):
        def run():  # (the values grow by 1 / pkeep a call and may reach inf: the time does not depend on them)
            L.drop_path_apply(nxt()["x"], seed, pkeep, counter)
        return run

    def add_bwd1():
        s = nxt()
        L.add_backward(s["x"], [s["d"]], None)

    # the kernel is the mirror's draw before anything is timed
    keep = {p: L.drop_path_keep_ref(B, L.effective_seed(seed, counter), 1.0 - p).cpu() for p in (0.05, 0.2)}
    y = x0.clone()
    L.drop_path_apply(y, seed, 0.8, counter)
    assert torch.equal((y != 0).any(1).cpu(), keep[0.2])
    arms = {"drop_path_0.05": dp(0.95), "drop_path_0.2": dp(0.8), "add_bwd1": add_bwd1}
    nbytes = {"add_bwd1": 2 * B * n * 2}
    for p in (0.05, 0.2):  # a kept sample is read and written, a dropped one written
        k = int(keep[p].sum())
        nbytes["drop_path_%s" % p] = 2 * n * (2 * k + (B - k))
    head = {"layer": "drop_path", "B": B, "n": n, "sites": what, "kept_0.05": int(keep[0.05].sum()),
            "kept_0.2": int(keep[0.2].sum())}
    return measure(arms, nbytes, a, nsets, head)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("silu_probe needs a GPU")
    dev = "cuda"
    silu, dpath = sites()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for fn, table in ((silu_size, silu), (drop_path_size, dpath)):
        for n, what in table.items():
            lines = fn(n, what, a, dev)
            if out:  # size by size: a run cut short keeps what it measured
                out.write("\n".join(lines) + "\n")
                out.flush()
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
