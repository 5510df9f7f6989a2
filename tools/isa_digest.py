#!/usr/bin/env python
"""One sha256 per csrc/*.hip and flag set of the gfx950 device assembly.

Two trees whose digests agree compile to the same device code.  The text hashed
is hipcc's -S output (the line tests/test_kernel_resources.py uses) without the
lines that name the __hip_cuid_<hash> symbol, whose name is a hash of the source
text.  It hashes and does not look at instructions.

usage: python tools/isa_digest.py [--root TREE] [--keep DIR] [-j N] [file.hip ...]
  --root TREE  a checkout of this repository (default: the one this file is in)
  --keep DIR   also write the filtered text there, to diff when digests differ
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import subprocess

FLAG_SETS = {"default": [], "checks": ["-DIRLMX_DEVICE_CHECKS=1"]}


def digest(csrc, name, flags, keep):
    # compiled from inside csrc/ by bare file name, so no path of the tree reaches the output
    asm = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                          "-S", "-o", "-", *FLAG_SETS[flags], name], cwd=csrc, capture_output=True, text=True, check=True).stdout
    text = "".join(l for l in asm.splitlines(keepends=True) if "__hip_cuid_" not in l)
    if keep:
        os.makedirs(keep, exist_ok=True)
        with open(os.path.join(keep, f"{name}.{flags}.s"), "w") as f:
            f.write(text)
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--keep")
    ap.add_argument("-j", "--jobs", type=int, default=4)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    csrc = os.path.join(a.root, "irl-maxent_amd", "csrc")
    names = [os.path.basename(f) for f in a.files] or sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip")))
    jobs = [(n, fl) for n in names for fl in FLAG_SETS]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for (n, fl), d in zip(jobs, pool.map(lambda j: digest(csrc, j[0], j[1], a.keep), jobs)):
            print(f"{d}  {n}  {fl}")


if __name__ == "__main__":
    main()
