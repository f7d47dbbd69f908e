#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every csrc/kernels/*.hip between a git revision and the
working tree (CPU only; the whole tree compiles in a few minutes).

    python tools/kernel_asm_diff.py <rev> [--files | --tree]

Both trees are compiled with the flags of cxxnet_amd.build.build_kernels plus
--cuda-device-only -S, and every assembly file is cut into chunks (chunks()): per symbol its body,
kernel descriptor (register / LDS counts), resource lines and metadata record, and the rest of
the file.  Comments, the __hip_cuid_ and .file lines and the per-file numbering of local labels
are no part of a chunk (normalise()); everything else must match.

  --files  file against file, the default while both trees hold the same files: prints
           "identical" per file or the chunks that differ.
  --tree   symbol against symbol over the whole tree, the default when the file lists differ (code
           moved between files): prints the symbols found on one side only, defined in more than
           one file, or differing in a chunk, and the kernel descriptors each file contributes.
Exits 1 on any difference.
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
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):$")
LOCAL = re.compile(r"(\.LBB|\bBB|\.LJTI|\.Lfunc_end)\d+")  # numbered by the function's index in its file
RESOURCE = re.compile(r"^\.set (\S+)\.(?:num|numbered|private|uses|has)_\w+,")
REST = "<rest of file>"


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


def normalise(line):
    """One assembly line without what moves with a symbol's place in its file: the comment (its
    column shifts with the label's length), the spacing and the function index in local labels.
    "" for a line that holds nothing else and for the __hip_cuid_ / .file lines."""
    if "__hip_cuid_" in line or ".file" in line:
        return ""
    return LOCAL.sub(r"\1#", " ".join(line.split(";", 1)[0].split()))


def chunks(text):
    """{chunk name: normalised lines} of one assembly file.  Per symbol S: "S" (from its label to
    its .Lfunc_end or .size), "S (kernel descriptor)", "S (resources)" (the .set S.num_vgpr, ...
    lines) and "S (metadata)" (its record under amdhsa.kernels); REST holds every other line."""
    out, cur = {}, REST
    desc = None    # name of the open .amdhsa_kernel block (it stands inside its function's lines)
    record = None  # lines of the open record under amdhsa.kernels: (None outside that list)
    in_meta = False
    for raw in text.splitlines():
        line = normalise(raw)
        if not line:
            continue
        if record is not None and raw.startswith(" "):
            if raw.startswith("  - "):
                record = []
            record.append(line)
            if line.startswith(".name: "):
                out[line.split()[1] + " (metadata)"] = record
            continue
        record = [] if line == "amdhsa.kernels:" else None
        in_meta = in_meta or line == ".amdgpu_metadata"
        if line.startswith(".amdhsa_kernel "):
            desc = line.split()[1] + " (kernel descriptor)"
        elif LABEL.match(line) and not in_meta:
            cur = LABEL.match(line).group(1)
        elif line.startswith(".Lfunc_end") or line.startswith(".size "):
            cur = REST
        key = desc or cur
        if line == ".end_amdhsa_kernel":
            desc = None
        elif RESOURCE.match(line):
            key = RESOURCE.match(line).group(1) + " (resources)"
        out.setdefault(key, []).append(line)
    return out


def differing(ca, cb):
    """Names of the chunks present on one side only or whose lines differ."""
    return sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))


def by_symbol(per_file):
    """{file: chunks} -> {chunk name: {file: lines}} without the files' REST."""
    out = {}
    for name, cs in per_file.items():
        for k, lines in cs.items():
            if k != REST:
                out.setdefault(k, {})[name] = lines
    return out


def tree_report(old, new, rev):
    """Lines of the tree-wide report and the number of findings, from {file: chunks} per side."""
    so, sn = by_symbol(old), by_symbol(new)
    lines, bad = [], 0
    for side, syms, other in ((rev, so, sn), ("the working tree", sn, so)):
        for k in sorted(set(syms) - set(other)):
            lines.append(f"only in {side}: {k} ({', '.join(sorted(syms[k]))})")
            bad += 1
        for k in sorted(k for k in syms if len(syms[k]) > 1):
            lines.append(f"defined in {len(syms[k])} files of {side}: {k} ({', '.join(sorted(syms[k]))})")
            bad += 1
    common = sorted(set(so) & set(sn))
    for k in common:
        if set(map(tuple, so[k].values())) != set(map(tuple, sn[k].values())):
            lines.append(f"differs: {k} ({', '.join(sorted(so[k]))} -> {', '.join(sorted(sn[k]))})")
            bad += 1

    def ndesc(cs):
        return sum(k.endswith(" (kernel descriptor)") for k in cs)

    for name in sorted(set(old) | set(new)):
        if name in old and name in new:
            d = differing(old[name], new[name])
            lines.append(f"{name}: {ndesc(new[name])} kernel descriptors, " +
                         ("identical" if not d else f"{len(d)} chunk(s) differ"))
            bad += bool(d)
        else:
            cs, side = (old[name], rev) if name in old else (new[name], "the working tree")
            lines.append(f"{name}: {ndesc(cs)} kernel descriptors, only in {side}")
    moved_old = sum(ndesc(old[n]) for n in old if n not in new)
    moved_new = sum(ndesc(new[n]) for n in new if n not in old)
    lines.append(f"files only in {rev}: {moved_old} kernel descriptors; files only in the working tree: {moved_new}")
    lines.append(f"{len(common)} chunks of {sum(map(ndesc, new.values()))} kernels compared by symbol, {bad} finding(s)")
    return lines, bad


def main():
    args = [a for a in sys.argv[1:] if a not in ("--files", "--tree")]
    if len(args) != 1:
        sys.exit(__doc__)
    rev = args[0]
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, KDIR], stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=ar.stdout, check=True)
        sides = []
        for kdir, out in ((os.path.join(tmp, KDIR), "old"), (os.path.join(ROOT, KDIR), "new")):
            names = compile_tree(kdir, os.path.join(tmp, out))
            sides.append({n: chunks(open(os.path.join(tmp, out, n + ".s")).read()) for n in names})
    old, new = sides
    if "--tree" in sys.argv or ("--files" not in sys.argv and set(old) != set(new)):
        lines, bad = tree_report(old, new, rev)
        print("\n".join(lines))
        sys.exit(1 if bad else 0)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in {'the working tree' if name in new else rev}")
            bad += 1
            continue
        d = differing(old[name], new[name])
        print(f"{name}: " + ("identical" if not d else f"{len(d)} chunk(s) differ"))
        for k in d:
            print("    " + k)
        bad += bool(d)
    print(f"{len(new) - bad} of {len(new)} files identical to {rev}" if not bad else f"{bad} file(s) differ from {rev}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
