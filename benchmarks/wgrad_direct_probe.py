"""Time the direct weight-gradient kernel (csrc/kernels/conv_wgrad_direct.hip) per AlexNet /
VGG op, one process, interleaved rounds.  Three modes:

    python benchmarks/wgrad_direct_probe.py [--ops conv3,conv4,conv5] [--splits 0,4,8,12,16]
        per split count (0: the kernel's own choice), the shipped form of each shape
    python benchmarks/wgrad_direct_probe.py --forms narrow,wide [--libs a=DIR,b=DIR]
        the 13 x 13 forms (64 x 32 tiles of four K parts / 64 x 64 tiles of 2 x 2 waves) against
        each other, and / or several builds of the kernel library (native directories, e.g. the
        parent commit's) against each other, all arms interleaved
    python benchmarks/wgrad_direct_probe.py --decompose
        slope and intercept: N = 64, 128, 256 with the split count held fixed, and every
        compile-time ablation of the kernel (results of an ablated launch are meaningless)

Times are the kernel plus its reduce launch (device events around --iters calls).  One JSON line
per arm: median over the rounds, and the spread (max - min) of the rounds."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxxnet_amd import native  # noqa: E402
from cxxnet_amd.ops import gemm  # noqa: E402
from cxxnet_amd.ops.gemm import ConvGeom  # noqa: E402

# name -> (N, H, C, Cout, K, pad, groups)
OPS = {
    "conv2": (256, 27, 96, 256, 5, 2, 2),
    "conv3": (256, 13, 256, 384, 3, 1, 1),
    "conv4": (256, 13, 384, 384, 3, 1, 2),
    "conv5": (256, 13, 384, 256, 3, 1, 2),
    "vgg_c5": (64, 14, 512, 512, 3, 1, 1),
}
# probe bits of the entry point's `splits` argument (cxn_conv_wgrad_direct)
FORMS = {"auto": 0, "narrow": 1 << 16, "wide": 2 << 16}
ABLATIONS = {"none": 0, "no_dy_dma": 1 << 20, "no_x_dma": 2 << 20, "no_dma": 3 << 20, "no_reads": 4 << 20,
             "no_mfma": 8 << 20, "no_epilogue": 16 << 20}
_ARGTYPES = None


def _lib(path):
    """Another build of the kernel library with the loaded one's prototype for the entry point."""
    lib = ctypes.CDLL(os.path.join(path, "libcxxnet_kernels.so"))
    ref = native.kernels().cxn_conv_wgrad_direct
    lib.cxn_conv_wgrad_direct.argtypes = ref.argtypes
    lib.cxn_conv_wgrad_direct.restype = ref.restype
    return lib


def _call(lib, x, dy, dw, db, g, code):
    """One launch pair through `lib` (None: the package's own path, ops.gemm.conv_wgrad_direct)."""
    if lib is None:
        assert gemm.conv_wgrad_direct(x, dy, dw, g, splits=code, db=db)
        return
    args = (g.N, g.H, g.W, x.shape[3], dy.shape[3], g.cg_in, g.cg_out, g.groups, g.KH, g.KW, g.pad_y, g.pad_x,
            g.stride, code)
    need = int(lib.cxn_conv_wgrad_direct(None, None, None, None, None, 0, *args, 1.0, None))
    assert need > 0, need
    ws = gemm._wgd_workspace(need, dw.device)
    rc = int(lib.cxn_conv_wgrad_direct(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None,
                                       ws.data_ptr(), ws.numel(), *args, 1.0, gemm._stream()))
    assert rc == 0, rc


def _time(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _tensors(name, n=None):
    N, H, C, Cout, K, pad, G = OPS[name]
    N = n or N
    g = ConvGeom(N, H, H, C, H, H, Cout, K, K, 1, pad, pad, G)
    x = torch.randn(N, H, H, C, device="cuda").to(torch.bfloat16)
    dy = torch.randn(N, H, H, Cout, device="cuda").to(torch.bfloat16)
    dw = torch.zeros(Cout, K, K, C // G, device="cuda")
    db = torch.zeros(Cout, device="cuda") if K == 3 else None
    return g, x, dy, dw, db, 2.0 * N * H * H * Cout * K * K * (C // G)


def _run(arms, rounds, iters, out, **tag):
    """arms: name -> callable; interleaved rounds; one JSON line per arm."""
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(_time(fn, iters))
    for k, ts in res.items():
        s = sorted(ts)
        rec = dict(tag, arm=k, us=round(s[len(s) // 2], 2), spread_us=round(s[-1] - s[0], 2), rounds=rounds)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default="conv3,conv4,conv5")
    ap.add_argument("--splits", default="0,4,6,8,12,16")
    ap.add_argument("--forms", default="")
    ap.add_argument("--libs", default="", help="name=native-dir[,name=native-dir]: other builds of the kernel library")
    ap.add_argument("--decompose", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    libs = {"": None}
    for spec in filter(None, a.libs.split(",")):
        nm, path = spec.split("=", 1)
        libs[nm] = _lib(path)
    for name in a.ops.split(","):
        if a.decompose:
            # the split count held fixed at b256's own choice of each form: per block the narrow
            # form walks N / 2 / S stages of two images, the wide one N / S' stages of one
            for form in ("narrow", "wide"):
                N0, _, C, Cout, _, _, G = OPS[name]
                cg, cog = C // G, Cout // G
                npairs = G * (cg // (64 if form == "wide" else 32)) * (cog // 64)
                S = 256 // npairs
                for n in (64, 128, 256):
                    g, x, dy, dw, db, _ = _tensors(name, n)
                    _run({form: lambda: _call(None, x, dy, dw, db, g, S | FORMS[form])}, a.rounds, a.iters, out,
                         op=name, N=n, splits=S, mode="slope")
                g, x, dy, dw, db, _ = _tensors(name)
                arms = {f"{form}/{ab}": (lambda c=S | FORMS[form] | bits: _call(None, x, dy, dw, db, g, c))
                        for ab, bits in ABLATIONS.items()}
                _run(arms, a.rounds, a.iters, out, op=name, N=N0, splits=S, mode="ablation")
            continue
        g, x, dy, dw, db, flop = _tensors(name)
        if a.forms or len(libs) > 1:
            arms = {}
            for ln, lib in libs.items():
                forms = a.forms.split(",") if (a.forms and ln == "") else ["auto"]
                for form in forms:
                    arms[(ln or "tree") + "/" + form] = (lambda lib=lib, c=FORMS[form]: _call(lib, x, dy, dw, db, g, c))
            _run(arms, a.rounds, a.iters, out, op=name, N=g.N, mode="forms")
            continue
        res = {}
        for _ in range(a.rounds):
            for sp in a.splits.split(","):
                sp = int(sp)
                res.setdefault(sp, []).append(_time(lambda: _call(None, x, dy, dw, db, g, sp), a.iters))
        for sp in a.splits.split(","):
            ts = sorted(res[int(sp)])
            t = ts[len(ts) // 2]
            print(json.dumps({"op": name, "splits": int(sp), "us": round(t, 1), "tflops": round(flop / t / 1e6, 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
