#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every csrc/kernels/*.hip between a git revision and the
working tree (CPU only; the whole tree compiles in a few minutes).

    python tools/kernel_asm_diff.py <rev>

Both trees are compiled with the flags of cxxnet_amd.build.build_kernels plus
--cuda-device-only -S.  Lines containing __hip_cuid_ or .file are dropped; everything else must
match: instruction streams, kernel descriptors (register / LDS counts), metadata, kernel names.
Prints "identical" per file or the symbols whose bodies differ; exits 1 on any difference.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cxxnet_amd.build import kernel_compile_cmd  # noqa: E402

KDIR = os.path.join("cxxnet_amd", "csrc", "kernels")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def compile_tree(kdir, out, jobs=8):
    """kdir/*.hip -> out/<name>.s (device side only); returns the sorted file names."""
    os.makedirs(out, exist_ok=True)
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(kdir, "*.hip")))

    def one(name):
        cmd = kernel_compile_cmd(kdir) + ["--cuda-device-only", "-S", os.path.join(kdir, name),
                                          "-o", os.path.join(out, name + ".s")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("compile failed:\n" + " ".join(cmd) + "\n" + r.stdout)

    with ThreadPoolExecutor(max_workers=min(8, jobs)) as ex:
        list(ex.map(one, names))
    return names


def chunks(path):
    """The assembly split at its global labels, kernel descriptors and metadata: {symbol: lines}."""
    out, cur = {}, "<preamble>"
    for line in open(path):
        if "__hip_cuid_" in line or ".file" in line:
            continue
        m = LABEL.match(line)
        if m:
            cur = m.group(1)
        elif line.lstrip().startswith(".amdhsa_kernel "):
            cur = line.split()[1] + " (kernel descriptor)"
        elif line.lstrip().startswith(".amdgpu_metadata"):
            cur = "<metadata>"
        out.setdefault(cur, []).append(line)
    return out


def differing(a, b):
    """Symbols present in one file only or whose bodies differ."""
    ca, cb = chunks(a), chunks(b)
    return sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, KDIR], stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=ar.stdout, check=True)
        old = compile_tree(os.path.join(tmp, KDIR), os.path.join(tmp, "old"))
        new = compile_tree(os.path.join(ROOT, KDIR), os.path.join(tmp, "new"))
        bad = 0
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                print(f"{name}: only in {'the working tree' if name in new else rev}")
                bad += 1
                continue
            d = differing(os.path.join(tmp, "old", name + ".s"), os.path.join(tmp, "new", name + ".s"))
            print(f"{name}: " + ("identical" if not d else f"{len(d)} symbol(s) differ"))
            for k in d:
                print("    " + k)
            bad += bool(d)
    print(f"{len(new) - bad} of {len(new)} files identical to {rev}" if not bad else f"{bad} file(s) differ from {rev}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
