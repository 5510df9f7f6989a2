#!/usr/bin/env python
"""One sha256 per csrc/*.hip and flag set of the gfx950 device assembly.

Two trees whose digests agree compile to the same device code.  The text hashed
is hipcc's -S output (the line tests/test_kernel_resources.py uses) without the
lines that name the __hip_cuid_<hash> symbol, whose name is a hash of the source
text.  It hashes and does not look at instructions.

--per-kernel prints one sha256 per kernel symbol and flag set instead, over all
the files given, sorted by symbol: the kernel's text from its label to its
function end (the .amdhsa_kernel block lies in between), with the function's
index taken out of the compiler-local labels (.LBB<i>_<j>, .Lfunc_begin<i>,
.Lfunc_end<i>, .LJTI<i>_<j>, .LCPI<i>_<j>), .Ltmp<n> numbered from the
kernel's first and the padding in front of trailing comments (it follows the
label's width) reduced to one space.  So a kernel's digest does not depend on which file it sits in
or where, and two trees that split their sources differently can be compared.

usage: python tools/isa_digest.py [--root TREE] [--keep DIR] [--per-kernel] [-j N] [file.hip ...]
  --root TREE   a checkout of this repository (default: the one this file is in)
  --keep DIR    also write the filtered text there, to diff when digests differ
  --per-kernel  one line per kernel symbol and flag set: digest, flags, symbol
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess

FLAG_SETS = {"default": [], "checks": ["-DIRLMX_DEVICE_CHECKS=1"]}


def assembly(csrc, name, flags):
    # compiled from inside csrc/ by bare file name, so no path of the tree reaches the output
    return subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                          "-S", "-o", "-", *FLAG_SETS[flags], name], cwd=csrc, capture_output=True, text=True, check=True).stdout


def digest(csrc, name, flags, keep):
    asm = assembly(csrc, name, flags)
    text = "".join(l for l in asm.splitlines(keepends=True) if "__hip_cuid_" not in l)
    if keep:
        os.makedirs(keep, exist_ok=True)
        with open(os.path.join(keep, f"{name}.{flags}.s"), "w") as f:
            f.write(text)
    return hashlib.sha256(text.encode()).hexdigest()


LOCAL_LABEL = re.compile(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.LCPI)\d+")
TMP_LABEL = re.compile(r"\.Ltmp\d+")
COMMENT_PAD = re.compile(r"[ \t]+;")


def kernel_digests(csrc, name, flags, keep):
    """{kernel symbol: sha256 of its normalised text} of one source."""
    lines = assembly(csrc, name, flags).splitlines(keepends=True)
    kernels = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    out, sym, body = {}, None, []
    for l in lines:
        if sym is None:
            label = l.split(":", 1)[0]
            if l.startswith(label + ":") and label in kernels:
                sym, body = label, [l]
            continue
        body.append(l)
        if l.startswith(".Lfunc_end"):
            tmps = {}
            # (the index's width also moves the column that pads the label's trailing comment)
            text = COMMENT_PAD.sub(" ;", LOCAL_LABEL.sub(r"\1", "".join(body)))
            text = TMP_LABEL.sub(lambda m: tmps.setdefault(m.group(0), f".Ltmp{len(tmps)}"), text)
            if keep:
                os.makedirs(keep, exist_ok=True)
                with open(os.path.join(keep, f"{sym}.{flags}.s"), "w") as f:
                    f.write(text)
            out[sym] = hashlib.sha256(text.encode()).hexdigest()
            sym = None
    assert sym is None and set(out) == kernels, (name, flags, sorted(kernels - set(out)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--keep")
    ap.add_argument("--per-kernel", action="store_true")
    ap.add_argument("-j", "--jobs", type=int, default=4)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    csrc = os.path.join(a.root, "irl-maxent_amd", "csrc")
    names = [os.path.basename(f) for f in a.files] or sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip")))
    jobs = [(n, fl) for n in names for fl in FLAG_SETS]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        if a.per_kernel:
            rows = []
            for (n, fl), ds in zip(jobs, pool.map(lambda j: kernel_digests(csrc, j[0], j[1], a.keep), jobs)):
                rows += [(sym, fl, d) for sym, d in ds.items()]
            assert len({r[:2] for r in rows}) == len(rows), "a kernel symbol defined in two sources"
            for sym, fl, d in sorted(rows):
                print(f"{d}  {fl}  {sym}")
            return
        for (n, fl), d in zip(jobs, pool.map(lambda j: digest(csrc, j[0], j[1], a.keep), jobs)):
            print(f"{d}  {n}  {fl}")


if __name__ == "__main__":
    main()
