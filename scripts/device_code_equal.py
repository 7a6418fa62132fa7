#!/usr/bin/env python3
"""Is the device code of this tree byte-identical to revision REV's?  (compiles only: no GPU needed)

    python scripts/device_code_equal.py REV [--json OUT]

Every csrc/*.hip of REV (taken from git into a temporary directory) and of the working tree is compiled device-only with the
flags of alfi_amd/build.py, the gfx950 code object is unbundled, and the SHA-256 of its .text, .rodata and .note sections
are compared file by file (a file REV does not have is listed as new and compared with nothing).  Host-only changes and shifted line numbers leave those sections alone; only the __hip_cuid_*
symbol name (.dynsym / .dynstr) differs between two builds.  Exit status 0: equal for every file.
"""
import argparse
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("alfi_amd", "csrc")
SECTIONS = (".text", ".rodata", ".note")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-I", "include", "-I", CSRC]   # build.py
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for p in (shutil.which(name), os.path.join(rocm, "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name),
              os.path.join(rocm, "llvm", "bin", name)):
        if p and os.path.exists(p):
            return p
    raise RuntimeError(name + " not found in the ROCm install")


def section_hashes(tree, name, out):
    """tree: a directory with alfi_amd/csrc and include (paths relative to it, so that __FILE__ is the same in both)."""
    base = os.path.join(out, name[:-4])
    subprocess.check_call([tool("hipcc")] + FLAGS + ["--cuda-device-only", "-c", os.path.join(CSRC, name), "-o", base + ".bundle"],
                          cwd=tree)
    subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + base + ".bundle", "--output=" + base + ".co"])
    with open(base + ".co", "rb") as f:
        elf = f.read()
    # ELF64 little-endian section table; a file without kernels has no .text / .rodata: hashed as empty
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sh = [struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, off, size
    names = elf[sh[shstrndx][4]:sh[shstrndx][4] + sh[shstrndx][5]]
    body = {names[h[0]:names.index(b"\0", h[0])].decode(): elf[h[4]:h[4] + h[5]] for h in sh if h[1] != 8}   # 8: NOBITS
    res = {s: hashlib.sha256(body.get(s, b"")).hexdigest() for s in SECTIONS}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("--json", help="write the per-file section hashes of both revisions here")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    rev = subprocess.check_output(["git", "rev-parse", a.rev], cwd=ROOT, text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "archive", rev, CSRC, "include"], cwd=ROOT, check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        jobs = []
        for side, tree in (("rev", old), ("tree", ROOT)):
            os.makedirs(os.path.join(tmp, side))
            jobs += [(side, tree, f) for f in sorted(os.listdir(os.path.join(tree, CSRC))) if f.endswith(".hip")]
        with ThreadPoolExecutor(a.j) as ex:
            hashes = list(ex.map(lambda j: section_hashes(j[1], j[2], os.path.join(tmp, j[0])), jobs))
    res = {"rev": {}, "tree": {}}
    for (side, _, f), h in zip(jobs, hashes):
        res[side][f] = h
    files = sorted(set(res["rev"]) | set(res["tree"]))
    new = [f for f in files if f not in res["rev"]]               # files REV does not have: nothing to compare them with
    differ = [f for f in files if f not in new and res["rev"].get(f) != res["tree"].get(f)]
    print("%-22s %-8s %-64s %-64s" % ("file", "section", "sha256 at " + rev[:7], "sha256 of this tree"))
    for f in files:
        for sec in SECTIONS:
            r, t = res["rev"].get(f, {}).get(sec, "-"), res["tree"].get(f, {}).get(sec, "-")
            print("%-22s %-8s %-64s %-64s %s" % (f, sec, r, t, "new" if f in new else "equal" if r == t else "DIFFERS"))
    print("device code (%s of gfx950) against %s: %s" % (", ".join(SECTIONS), rev[:7],
                                                        "DIFFERS in " + ", ".join(differ) if differ else "identical in all %d files of that revision" % (len(files) - len(new))))
    if new:
        print("new in this tree: " + ", ".join(new))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rev": rev, "flags": FLAGS + ["--cuda-device-only"], "sections": SECTIONS, "equal": not differ, "new": new,
                       "hashes_rev": res["rev"], "hashes_tree": res["tree"]}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
