#!/usr/bin/env python3
"""Per-kernel ISA record of dca_engine.hip (or any kernel file of deepcubea_amd/csrc).

Compiles the file for gfx950 with the Makefile's flags plus `--cuda-device-only -S` and prints, per kernel, how many
flat / global / scalar-load / LDS memory instructions and `s_waitcnt` it holds, and the register, scratch and occupancy
figures the compiler reports.  A report, not a test: its output for a commit is kept under profiles/.

    python tools/isa_report.py [--src deepcubea_amd/csrc/dca_engine.hip] [--asm-out FILE] [--keep kernel-name-regex]

`--chain KERNEL` (the short demangled name, e.g. 'k_expand<0, 0, 0>') prints instead the kernel's dependent memory levels in
program order up to its first `s_barrier`: every vector / scalar load as it is issued, every `s_waitcnt` that ends a group of
them (a wait with no load issued since the previous wait adds no level and is marked so), and the branches and exec-mask
regions in between, which tell whether a wait sits inside a region that only some lanes or waves walk.
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


def kernel_body(asm_text, mangled):
    """the instructions of one function, in program order, with the labels in between"""
    out, on = [], False
    for line in asm_text.splitlines():
        if re.match(r"^%s:" % re.escape(mangled), line):
            on = True
            continue
        if on:
            s = line.strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s[0] == ";" or (s[0] == "." and not s.endswith(":")):
                continue
            out.append(s.split(";")[0].strip())
    return out


def writes_exec(s):
    """a scalar instruction whose destination is the exec mask (the end of an exec-masked region)"""
    parts = s.split(None, 1)
    return parts[0].startswith("s_") and len(parts) > 1 and parts[1].split(",")[0].strip() == "exec"


def chain(body):
    """[(kind, text)] up to the first s_barrier: kind = load / wait / flow / lds / barrier"""
    rows = []
    for s in body:
        op = s.split()[0]
        if op == "s_barrier":
            rows.append(("barrier", s))
            break
        if classify(op) in ("flat_ld", "glob_ld", "s_load") or op.startswith(("buffer_load", "scratch_load")):
            rows.append(("load", s))
        elif op == "s_waitcnt":
            rows.append(("wait", s))
        elif op.startswith("s_cbranch") or op == "s_branch" or "saveexec" in op or s.endswith(":") or writes_exec(s):
            rows.append(("flow", s))
        elif op.startswith(("ds_write", "ds_read")):
            rows.append(("lds", s))
    return rows


def print_chain(name, rows):
    print("# %s: loads and waits in program order up to the first s_barrier" % name)
    level = pending = 0
    lds_op, lds_n = None, 0  # LDS accesses are shown as runs: they tell where the loaded data is first used

    def flush_lds():
        nonlocal lds_op, lds_n
        if lds_n:
            print("          %s x %d" % (lds_op, lds_n))
        lds_op, lds_n = None, 0

    for kind, s in rows:
        if kind == "lds":
            op = s.split()[0]
            if op != lds_op:
                flush_lds()
            lds_op, lds_n = op, lds_n + 1
            continue
        flush_lds()
        if kind == "load":
            pending += 1
            print("    issue   %s" % s)
        elif kind == "wait":
            if pending:
                level += 1
                print("  WAIT %-2d   %s      <- ends a group of %d load(s)" % (level, s, pending))
            else:
                print("  wait      %s      (no load since the previous wait: no new level)" % s)
            pending = 0
        elif kind == "flow":
            print("      |     %s" % s)
        else:
            print("  BARRIER   %s      (%d wait level(s) in front of it, %d load(s) still uncounted)" % (s, level, pending))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "deepcubea_amd", "csrc", "dca_engine.hip"))
    ap.add_argument("--asm-out", default=None, help="keep the assembly here")
    ap.add_argument("--keep", default=None, help="only kernels whose demangled name matches this regex")
    ap.add_argument("--chain", default=None, metavar="KERNEL", help="dependent memory levels of this kernel up to its first s_barrier")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        out = a.asm_out or os.path.join(td, "k.s")
        cmd = [a.hipcc] + FLAGS + ["-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S", a.src, "-o", out]
        subprocess.run(cmd, check=True)
        with open(out) as f:
            text = f.read()
        order, kernels = parse(text)
    dm = demangle(order)
    if a.chain:
        hit = [n for n in order if short(dm[n]) == a.chain]
        if len(hit) != 1:
            sys.exit("--chain: %d kernels are called %r; there are: %s" % (len(hit), a.chain, ", ".join(sorted(short(dm[n]) for n in order))))
        print("# %s  (hipcc %s --cuda-device-only -S)" % (os.path.basename(a.src), " ".join(FLAGS)))
        print_chain(a.chain, chain(kernel_body(text, hit[0])))
        k = kernels[hit[0]]
        print("# %s" % " ".join("%s=%d" % (c, k[c]) for c in ("sgpr", "vgpr", "agpr", "scratch", "occ", "lds")))
        return 0
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
