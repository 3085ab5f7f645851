#!/usr/bin/env python3
"""Machine code of kernel files in two trees, kernel by kernel (a report, not a test; its output is kept under profiles/).

    python tools/isa_compare.py --parent DIR [--anchor REGEX] [--rename REGEX=REPL ...] FILE.hip [FILE.hip ...]

Compiles every FILE of deepcubea_amd/csrc in this tree and in the tree at DIR as tools/isa_report.py does (the Makefile's flags
plus `--cuda-device-only -S`) and prints, per __global__ kernel, parent | branch: SGPRs, VGPRs, scratch, LDS, occupancy, the
instruction counts, and a verdict on the instruction text (labels included, comments and directives dropped): identical, or
identical from the first instruction that matches --anchor (default: the first vector memory load) to the end with the
differences in front of it quoted, or different.  Kernels are matched by their short demangled names; --rename rewrites a
branch name first (a template that changed its name is matched by its arguments).  Exit status 1 unless every kernel has equal
resources and is identical at least from the anchor on."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

from isa_report import FLAGS, ROOT, demangle, kernel_body, parse, short

RES = ["sgpr", "vgpr", "scratch", "lds", "occ"]


def kernels_of(tree, name, hipcc, td, tag):
    out = os.path.join(td, "%s_%s.s" % (tag, name))
    subprocess.run([hipcc] + FLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S",
                                      os.path.join(tree, "deepcubea_amd", "csrc", name), "-o", out], check=True)
    text = open(out).read()
    order, counts = parse(text)
    globals_ = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\w+)", text, re.M))
    dm = demangle(order)
    # (block labels carry the function's number in its file: .LBB3_7 -> .LBB_7)
    return {short(dm[n]): (counts[n], [re.sub(r"\.LBB\d+_", ".LBB_", s) for s in kernel_body(text, n)]) for n in order if n in globals_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--parent", required=True, help="root of the tree to compare against")
    ap.add_argument("--anchor", default=r"^(global|flat|buffer)_load")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        for name in a.files:
            name = os.path.basename(name)
            old = kernels_of(a.parent, name, a.hipcc, td, "parent")
            new = {}
            for k, v in kernels_of(ROOT, name, a.hipcc, td, "branch").items():
                was = k
                for rx, repl in renames:
                    was = re.sub(rx, repl, was)
                new[was] = (k, v)
            w = max(len(k) for k in old)
            print("## %s: %d kernels in the parent, %d in the branch" % (name, len(old), len(new)))
            print("%-*s %s | %s   instr parent/branch  body" % (w, "kernel (parent's name)", " ".join("%7s" % c for c in RES), " ".join("%7s" % c for c in RES)))
            quotes = []
            for k, (rc, body) in old.items():
                if k not in new:
                    print("%-*s MISSING in the branch" % (w, k))
                    bad += 1
                    continue
                now, (rn, nbody) = new.pop(k)
                same_res = all(rc[c] == rn[c] for c in RES)
                fa = next((i for i, s in enumerate(body) if re.search(a.anchor, s)), None)
                fb = next((i for i, s in enumerate(nbody) if re.search(a.anchor, s)), None)
                if body == nbody:
                    verdict = "identical"
                elif fa is not None and fb is not None and body[fa:] == nbody[fb:]:
                    verdict = "identical from the anchor (parent line %d, branch line %d) to the end; differs in front of it" % (fa + 1, fb + 1)
                    quotes.append((k, list(difflib.unified_diff(body[:fa], nbody[:fb], "parent", "branch", n=0, lineterm=""))))
                else:
                    verdict = "DIFFERENT"
                    d = list(difflib.unified_diff(body, nbody, "parent", "branch", n=0, lineterm=""))
                    quotes.append((k, d[:80] + (["... (%d more lines)" % (len(d) - 80)] if len(d) > 80 else [])))
                if verdict == "DIFFERENT" or not same_res:
                    bad += 1
                print("%-*s %s | %s   %6d/%-6d  %s%s%s" % (w, k, " ".join("%7d" % rc[c] for c in RES), " ".join("%7d" % rn[c] for c in RES),
                                                          len(body), len(nbody), verdict, "" if same_res else "; RESOURCES DIFFER",
                                                          "" if now == k else "   [branch: %s]" % now))
            for k in new:
                print("%-*s NEW in the branch (%s)" % (w, k, new[k][0]))
                bad += 1
            for k, d in quotes:
                print("\n   --- %s: differences (unified diff, no context; %d lines)" % (k, len(d)))
                for ln in d:
                    print("   " + ln)
            print()
    print("ALL WITHIN THE RULE" if bad == 0 else "%d KERNEL(S) OUTSIDE THE RULE" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
