#!/usr/bin/env python3
"""Per-kernel ISA record of dca_engine.hip (or any kernel file of deepcubea_amd/csrc).

Compiles the file for gfx950 with the Makefile's flags plus `--cuda-device-only -S` and prints, per kernel, how many
flat / global / scalar-load / LDS memory instructions and `s_waitcnt` it holds, and the register, scratch and occupancy
figures the compiler reports.  A report, not a test: its output for a commit is kept under profiles/.

    python tools/isa_report.py [--src deepcubea_amd/csrc/dca_engine.hip] [--asm-out FILE] [--keep kernel-name-regex]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]
COLS = ["flat_ld", "flat_st", "flat_at", "glob_ld", "glob_st", "glob_at", "s_load", "ds", "waitcnt", "sgpr", "vgpr", "agpr",
        "scratch", "occ", "lds"]


def classify(op):
    for space, tag in (("flat_", "flat"), ("global_", "glob")):
        if op.startswith(space):
            rest = op[len(space):]
            if rest.startswith("load"):
                return tag + "_ld"
            if rest.startswith("store"):
                return tag + "_st"
            if rest.startswith("atomic"):
                return tag + "_at"
            return None
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "s_load"
    if op.startswith("ds_"):
        return "ds"
    if op == "s_waitcnt":
        return "waitcnt"
    return None


def parse(asm_text):
    kernels = {}  # mangled name -> counts
    order = []
    cur = None
    last = None
    # kernels and the device functions that stayed calls (their instructions run inside the kernel that calls them)
    names = set(re.findall(r"^\s*\.type\s+(\w+),@function", asm_text, re.M))
    foot = {"; TotalNumSgprs:": "sgpr", "; NumVgprs:": "vgpr", "; NumAgprs:": "agpr", "; ScratchSize:": "scratch",
            "; Occupancy:": "occ", "; LDSByteSize:": "lds"}
    for line in asm_text.splitlines():
        s = line.strip()
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in names:
            cur = last = m.group(1)
            kernels[cur] = dict.fromkeys(COLS, 0)
            order.append(cur)
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None:
            if not s or s[0] in ".;" or s.endswith(":"):
                continue
            k = classify(s.split()[0])
            if k:
                kernels[cur][k] += 1
        elif last is not None:
            for key, col in foot.items():
                if s.startswith(key):
                    kernels[last][col] = int(s[len(key):].split()[0])
    return order, kernels


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*\)$", "", name)
    return name.replace("dca::", "").replace("(anonymous namespace)::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "deepcubea_amd", "csrc", "dca_engine.hip"))
    ap.add_argument("--asm-out", default=None, help="keep the assembly here")
    ap.add_argument("--keep", default=None, help="only kernels whose demangled name matches this regex")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        out = a.asm_out or os.path.join(td, "k.s")
        cmd = [a.hipcc] + FLAGS + ["-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S", a.src, "-o", out]
        subprocess.run(cmd, check=True)
        with open(out) as f:
            order, kernels = parse(f.read())
    dm = demangle(order)
    rows = [(short(dm[n]), kernels[n]) for n in order]
    if a.keep:
        rows = [r for r in rows if re.search(a.keep, r[0])]
    rows.sort(key=lambda r: r[0])
    w = max(len(r[0]) for r in rows)
    print("# %s  (hipcc %s --cuda-device-only -S)" % (os.path.basename(a.src), " ".join(FLAGS)))
    print("%-*s %s" % (w, "kernel", " ".join("%7s" % c for c in COLS)))
    for name, k in rows:
        print("%-*s %s" % (w, name, " ".join("%7d" % k[c] for c in COLS)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
