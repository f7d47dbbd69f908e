"""Which kernel, tile and epilogue every conv / fc op dispatches to, pinned without a GPU.

The kernel library is replaced by a fake that records (entry point, arguments) and returns a
code; the ops run on uninitialised CPU bf16 tensors that are never read.  The cases are every
signature of the shipped tile table at its own shape (the production dispatches), the same
geometries at N = 3 (table misses: the heuristic path), and a few calls the table does not name.
Each case runs under six configurations (CONFIGS).  tests/golden/dispatch_trace.json holds, per
case and configuration, "served calls|refused count|digest": the served calls (rc 0) as
entry:tile:epi:ksplit, the number of calls the fake refused (-1), and a digest of every scalar
argument of the served calls (operand descriptors included, pointers replaced by the role of the
tensor they fall in).  A configuration equal to the case's default one is stored as "=".

    python tests/test_dispatch_trace_cpu.py --regen     rewrites the golden file
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cxxnet_amd import native  # noqa: E402
from cxxnet_amd.ops import gemm, mode, nn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_trace.json")
CONFIGS = ("default", "deterministic", "tile7", "cd_off", "wgd_off", "direct_refuse")
DIRECT_ENTRIES = ("cxn_conv_direct", "cxn_conv_wgrad_direct", "cxn_conv_rowrun_fwd2", "cxn_conv_wgrad_rowrun",
                  "cxn_conv_rowrun_fwd", "cxn_conv_fewc_fwd")
SIZE_QUERIES = ("cxn_conv_direct", "cxn_conv_wgrad_direct", "cxn_conv_wgrad_rowrun")
# positions of (tile, epilogue, K-split) in the argument lists of the GEMM entry points
TILE_EPI_KSPLIT = {"cxn_gemm": (15, 14, 17), "cxn_gemm_glds": (13, 12, 15), "cxn_gemm_glds_split": (11, None, None),
                   "cxn_gemm_glds_add": (9, None, None), "cxn_gemm_glds_sgd": (12, None, None),
                   "cxn_conv_direct": (-2, None, None)}


GLDS_ENTRIES = ("cxn_gemm_glds", "cxn_gemm_glds_split", "cxn_gemm_glds_add", "cxn_gemm_glds_sgd")


class FakeKernels:
    """Stands in for the ctypes library: every attribute is an entry point that records its call."""

    def __init__(self, refuse=()):
        self.refuse = set(refuse)
        self.roles = {}   # role -> tensor
        self.calls = []   # (entry, recorded arguments, rc)

    def _role(self, p):
        for role, t in self.roles.items():
            if t.data_ptr() <= p < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                return role
        return "ws"

    def _arg(self, a):
        if isinstance(a, native.CxnOperand):
            return {f: (self._role(a.ptr) if f == "ptr" else getattr(a, f)) for f, _ in a._fields_}
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 32:  # no size here reaches 4 Gi
            return self._role(a)
        assert a is None or isinstance(a, (int, float)), a
        return a

    def __getattr__(self, entry):
        def call(*args):
            if entry in SIZE_QUERIES and args[0] is None:
                rc = -1 if entry in self.refuse else 4096
            else:
                rc = -1 if entry in self.refuse else 0
            if entry in GLDS_ENTRIES and args[TILE_EPI_KSPLIT[entry][0]] not in gemm.GLDS_TILES:
                rc = -1  # as the library: a tile id it does not compile
            self.calls.append((entry, [self._arg(a) for a in args], rc))
            return rc
        return call


def _reset_pools():
    """Drop the CPU entries of the grow-only workspaces, so a case's workspace sizes do not depend
    on the cases before it."""
    for m in (gemm, nn, mode):
        for v in vars(m).values():
            if isinstance(v, dict):
                for k in [k for k, t in v.items() if isinstance(t, torch.Tensor) and "cpu" in str(k)]:
                    del v[k]
                for pool in v.values():
                    if isinstance(pool, dict) and isinstance(pool.get("cpu"), torch.Tensor):
                        del pool["cpu"]


def _t(*shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype)


def _f(*shape):
    return torch.empty(shape, dtype=torch.float32)


def _geom(N, H, W, C, Cout, KH, KW, stride, pad_y=0, pad_x=0, groups=1):
    Ho, Wo = gemm.conv_out_size(H, W, KH, KW, stride, pad_y, pad_x)
    return gemm.ConvGeom(N, H, W, C, Ho, Wo, Cout, KH, KW, stride, pad_y, pad_x, groups)


def _conv_tensors(g):
    return dict(x=_t(g.N, g.H, g.W, g.C), w=_t(g.Cout, g.KH, g.KW, g.cg_in), y=_t(g.N, g.Ho, g.Wo, g.Cout))


def _run_cf(*f):
    g = _geom(*f)
    r = dict(_conv_tensors(g), bias=_f(g.Cout))
    return r, lambda: gemm.conv_forward(r["x"], r["w"], r["bias"], r["y"], g, relu=True)


def _run_cfs(N, H, W, C, Cout, split):
    g = _geom(N, H, W, C, Cout, 1, 1, 1)
    r = dict(x=_t(N, H, W, C), w=_t(Cout, 1, 1, C), bias=_f(Cout), y=_t(N, H, W, split), y2=_t(N, H, W, Cout - split))
    return r, lambda: gemm.conv_forward_split(r["x"], r["w"], r["bias"], r["y"], r["y2"], split, g, relu=True)


def _run_cd(*f):
    g = _geom(*f)
    r = dict(_conv_tensors(g), wt=_t(g.Cout, g.KH, g.KW, g.cg_in), dbias=_f(g.C))
    return r, lambda: gemm.conv_backward_data(r["y"], r["w"], r["x"], g, wt_buf=r["wt"], mask_relu=True,
                                              dbias=r["dbias"])


def _run_cda(*f):
    g = _geom(*f)
    r = dict(_conv_tensors(g), wt=_t(g.Cout, g.KH, g.KW, g.cg_in), add=_t(g.N, g.H, g.W, g.C))
    return r, lambda: gemm.conv_backward_data_add(r["y"], r["w"], r["x"], r["add"], g, r["wt"], mask_relu=True)


def _run_cw(*f):
    g = _geom(*f)
    t = _conv_tensors(g)
    r = dict(x=t["x"], y=t["y"], w=_f(*t["w"].shape), dbias=_f(g.Cout))
    return r, lambda: gemm.conv_backward_weight(r["x"], r["y"], r["w"], g, db=r["dbias"])


def _fc_tensors(nin, nout, Bn):
    return dict(x=_t(Bn, nin), w=_t(nout, nin), y=_t(Bn, nout), bias=_f(nout))


def _run_fc(nin, nout, Bn, **kw):
    r = _fc_tensors(nin, nout, Bn)
    if kw.get("out_fp32"):
        r["y"] = _f(Bn, nout)
    return r, lambda: gemm.fc_forward(r["x"], r["w"], r["bias"], r["y"], relu=True, **kw)


def _run_fd(nin, nout, Bn):
    r = _fc_tensors(nin, nout, Bn)
    return r, lambda: gemm.fc_backward_data(r["y"], r["w"], r["x"], mask_relu=True)


def _run_fw(nin, nout, Bn, overwrite=False):
    r = dict(_fc_tensors(nin, nout, Bn), w=_f(nout, nin))
    return r, lambda: gemm.fc_backward_weight(r["x"], r["y"], r["w"], overwrite=overwrite)


def _run_fws(nin, nout, Bn):
    r = dict(_fc_tensors(nin, nout, Bn), w=_f(nout, nin), m=_f(nout, nin), wb=_t(nout, nin))
    return r, lambda: gemm.fc_backward_weight_sgd(r["x"], r["y"], r["w"], r["m"], r["wb"], 0.01, 0.0005, 0.9, 0.0)


def cases():
    """{case id: (builder, fields)}: the shipped table's signatures, each also at N = 3, and the
    calls the table does not name.  Signatures that lead to the same call share one case."""
    with open(gemm.TUNE_DB) as f:
        table = json.load(f)
    out = {}

    def add(name, fn, fields, **kw):
        out[name + "|" + "|".join(str(v) for v in fields) + "".join(f"|{k}" for k in kw)] = (fn, tuple(fields), kw)
    for key in sorted(table):
        op, *fields = key.split("|")
        fields = [int(v) for v in fields]
        for n3 in (False, True):
            if op in ("cf", "cr", "cd", "cw", "cws", "cwr", "cfs"):
                f = [3] + fields[1:] if n3 else fields
                if op == "cfs":
                    add("cfs", _run_cfs, f)
                    f[5] += 8  # a split the table does not hold
                    add("cfs", _run_cfs, f)
                elif op == "cd":
                    add("cd", _run_cd, f)
                    add("cda", _run_cda, f)
                else:
                    add("cf" if op in ("cf", "cr") else "cw", _run_cf if op in ("cf", "cr") else _run_cw, f)
            elif op == "fc":  # (A mode, nout, batch, nin, ldc)
                f = [fields[3], fields[1], 3 if n3 else fields[2]]
                add("fc", _run_fc, f)
                add("fd", _run_fd, f)
                add("fc", _run_fc, f, drop=(1234, None, 0.5))
                add("fc", _run_fc, f, out_fp32=True)
            else:  # fw, fws: (nin, nout, batch)
                f = fields[:2] + [3 if n3 else fields[2]]
                add("fw", _run_fw, f)
                add("fw", _run_fw, f, overwrite=True)
                add("fws", _run_fws, f)
    return out


def _configure(mp, config):
    """The patches of one configuration; returns the fake library."""
    fake = FakeKernels(DIRECT_ENTRIES if config == "direct_refuse" else ())
    mp.setattr(native, "kernels", lambda: fake)
    mp.setattr(gemm, "_native_t", lambda t: True)
    mp.setattr(gemm, "_stream", lambda: 0)
    mp.setitem(gemm._DET, "on", gemm._DET["on"])
    for k, v in list(gemm._glds_cfg.items()):
        mp.setitem(gemm._glds_cfg, k, set(v) if isinstance(v, set) else v)
    gemm.set_glds(True, 7 if config == "tile7" else -1, tune=False)
    if config == "deterministic":
        gemm.set_deterministic(True)
    if config == "cd_off":
        mp.setattr(gemm, "_CD", "0")
    if config == "wgd_off":
        mp.setattr(gemm, "_WGD", "0")
    return fake


def _entry(name, args):
    tile, epi, ksplit = TILE_EPI_KSPLIT.get(name, (None, None, None))
    s = name[4:]
    if tile is not None:
        s += ":" + ":".join(str(args[i]) for i in (tile, epi, ksplit) if i is not None)
    return s


def trace(fake, fn, fields, kw):
    _reset_pools()
    roles, call = fn(*fields, **kw)
    fake.roles, fake.calls = roles, []
    ret = call()
    served = [(e, a) for e, a, rc in fake.calls if rc != -1]
    refused = sum(1 for _, _, rc in fake.calls if rc == -1)
    digest = hashlib.sha1(json.dumps([served, ret], sort_keys=True).encode()).hexdigest()[:10]
    return ",".join(_entry(e, a) for e, a in served) + f"|{refused}|{digest}"


def run_config(config):
    with pytest.MonkeyPatch.context() as mp:
        fake = _configure(mp, config)
        return {name: trace(fake, *c) for name, c in cases().items()}


def regen():
    per = {c: run_config(c) for c in CONFIGS}
    out = {}
    for name in per["default"]:
        row = [per[c][name] for c in CONFIGS]
        out[name] = [row[0]] + ["=" if r == row[0] else r for r in row[1:]]
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({"configs": list(CONFIGS), "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("config", CONFIGS)
def test_dispatch_trace(config):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["configs"] == list(CONFIGS)
    col = CONFIGS.index(config)
    got = run_config(config)
    assert sorted(got) == sorted(golden["cases"])
    bad = []
    for name, t in got.items():
        row = golden["cases"][name]
        want = row[0] if row[col] == "=" else row[col]
        if t != want:
            bad.append((name, t, want))
    assert not bad, (len(bad), bad[:5])


def test_no_entry_point_called_twice_with_the_same_arguments():
    """Within one op call a refused kernel is not asked again with identical arguments."""
    with pytest.MonkeyPatch.context() as mp:
        fake = _configure(mp, "direct_refuse")
        twice = []
        for name, (fn, fields, kw) in cases().items():
            trace(fake, fn, fields, kw)
            seen = [json.dumps([e, a], sort_keys=True) for e, a, _ in fake.calls]
            if len(seen) != len(set(seen)):
                twice.append(name)
    assert not twice, (len(twice), twice[:5])


if __name__ == "__main__":
    if sys.argv[1:] == ["--regen"]:
        regen()
        print("wrote", GOLDEN)
    else:
        sys.exit(__doc__)
