"""IDA* on the pattern databases on the MI355X, measured once -> profiles/idastar_probe.txt.

    python tools/idastar_probe.py [--out profiles/idastar_probe.txt] [--legs resources,puzzle15,puzzle24,cube3] [--seconds 150]

One GPU visit.  Every leg runs in a fresh child process under its own `timeout`, one after another, and the visit ends at the
first leg that does not exit 0 (nothing is started on a device after a leg has failed on it).  Legs:
  resources  the kernels' registers, LDS, scratch bytes and occupancy, from a compile of csrc/dca_idastar.hip with
             -Rpass-analysis=kernel-resource-usage (no device needed).  A kernel with scratch fails the leg.
  puzzle15   all 500 shipped test states with 5-5-5 and with 6-6-3: solved, length == the shipped optimal length, nodes, seconds.
  puzzle24   the shipped test states in ascending optimal length with 6-6-6-6, until --seconds of search have passed.
  cube3      the shipped test states in ascending optimal length with korf and with korf7, --seconds of search each.
  puzzle15_reflect, puzzle24_reflect
             the same states and settings with and without the reflected look-up (`+reflect`), on the same built tables in one
             process: a plain run, then a reflected one, then both restricted to the states both ran and solved.  Written to
             profiles/idastar_reflect_probe.txt with `--legs resources,puzzle15_reflect,puzzle24_reflect --out ...`.
  cube3_sym_korf, cube3_sym_korf7
             the shipped cube3 states in ascending optimal length with the plain set and with `+sym:N` for N in 2, 4, 8, 24, on
             the same built tables in one process, --seconds of search per configuration; then every configuration restricted
             to the states all of them ran and solved, as ratios to the plain run.  Written to profiles/idastar_sym_probe.txt
             with `--legs resources,cube3_sym_korf,cube3_sym_korf7 --seconds 60 --out ...`.
  cube3_dual_korf, cube3_dual_korf7
             the same method for the dual look-ups: plain, `+dual`, `+sym:4`, `+sym:4+dual`, `+sym:8`, `+sym:8+dual` and `+sym+dual`,
             plain first; per configuration also whether a state of 21 moves or more was reached.  Written to
             profiles/idastar_dual_probe.txt with `--legs resources,cube3_dual_korf,cube3_dual_korf7 --seconds 60 --out ...`.
  puzzle15_batch, puzzle24_batch
             batches of roots (`--batch`, dca_idastar_npuzzle_batch) against the single search, on the same built tables in one
             process: all 500 shipped puzzle15 states with 5-5-5 and with 6-6-3, plain and `+reflect`, in groups of 1, 16, 64 and
             500, and the 44 easiest shipped puzzle24 states with 6-6-6-6 in groups of 1, 16 and 44; the single path first and
             once more at the end.  Total seconds, nodes and nodes per second per pass, and every state's thresholds and completed
             counts checked against the single path's.  Written to profiles/idastar_batch_probe.txt with
             `--legs resources,puzzle15_batch,puzzle24_batch --out ...`.
A state's node budget is what the rate measured so far gets through in --state_seconds; a state that runs out of it is listed.
The rate of a family is nodes over seconds summed over its searches of at least 0.05 s (shorter ones time the launches, not the
kernel).  No threshold is set on any time or rate: the numbers are recorded, not met."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEG_TIMEOUT_S = {"resources": 120, "puzzle15": 500, "puzzle24": 500, "cube3": 700, "puzzle15_reflect": 500, "puzzle24_reflect": 700,
                 "cube3_sym_korf": 800, "cube3_sym_korf7": 800, "cube3_dual_korf": 1000, "cube3_dual_korf7": 1000,
                 "puzzle15_batch": 560, "puzzle24_batch": 560}
SYM_IMAGES = (2, 4, 8, 24)
DUAL_CONFIGS = ((0, False), (0, True), (4, False), (4, True), (8, False), (8, True), (48, True))  # (N of +sym:N, +dual), plain first
FIRST_BUDGET = 1 << 31  # nodes, until a rate is known


def resources_leg():
    src = os.path.join(ROOT, "deepcubea_amd", "csrc", "dca_idastar.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True, universal_newlines=True).stdout
    rows, cur = [], {}
    for key, value in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", text):
        if key == "Function Name":
            cur = {"name": value}
            rows.append(cur)
        elif cur:
            cur[key.strip()] = value
    assert rows, "no resource remarks in the compiler's output"
    print("kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):")
    for r in rows:
        name = subprocess.run(["c++filt", r["name"]], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip().split("(")[0]
        print("  %-38s VGPRs %3s  SGPRs %3s  LDS %6s B/block  scratch %s B/lane  occupancy %s waves/SIMD"
              % (name, r.get("VGPRs"), r.get("TotalSGPRs"), r.get("LDS Size"), r.get("ScratchSize"), r.get("Occupancy")))
        assert r.get("ScratchSize") == "0", "a kernel with scratch is not finished"


class Rate:
    def __init__(self):
        self.nodes, self.seconds = 0, 0.0

    def add(self, nodes, seconds):
        if seconds >= 0.05:
            self.nodes += nodes
            self.seconds += seconds

    @property
    def value(self):
        return self.nodes / self.seconds if self.seconds > 0 else None


def run_states(search, label, roots, lens, ids, seconds, state_seconds, verbose):
    """Searches the roots in order until `seconds` of search have passed -> prints a summary, returns the rate and, per state
    run, {id: (solved, nodes, seconds)}."""
    import torch
    rate = Rate()
    spent, ran, optimal, missed, nodes_all, times, records = 0.0, 0, 0, [], [], [], {}
    for root, want, i in zip(roots, lens, ids):
        if spent >= seconds:
            break
        budget = int(rate.value * state_seconds) if rate.value else FIRST_BUDGET
        torch.cuda.synchronize()
        t0 = time.time()
        res = search.solve(root, budget)
        dt = time.time() - t0
        spent += dt
        ran += 1
        rate.add(res["nodes_generated"], dt)
        nodes_all.append(res["nodes_generated"])
        times.append(dt)
        records[int(i)] = (res["solved"], res["nodes_generated"], dt)
        if res["solved"]:
            assert len(res["moves"]) == want, "state %d: length %d, shipped optimal %d" % (i, len(res["moves"]), want)
            optimal += 1
        else:
            missed.append((i, want, res["status"], res["nodes_generated"], res["thresholds"][-1:]))
        if verbose:
            print("    state %4d  optimal %3d  %-16s nodes %14d  %8.3f s  thresholds %s"
                  % (i, want, res["status"], res["nodes_generated"], dt, res["thresholds"]), flush=True)
    print("  %-18s ran %d of %d states (optimal length %d .. %d) in %.1f s of search: solved at the shipped optimal length %d / %d"
          % (label, ran, len(roots), min(lens[:ran]), max(lens[:ran]), spent, optimal, ran))
    print("  %-18s nodes per state: median %.3g, mean %.3g, max %.3g; seconds per state: median %.4f, mean %.4f, max %.3f"
          % ("", np.median(nodes_all), np.mean(nodes_all), np.max(nodes_all), np.median(times), np.mean(times), np.max(times)))
    print("  %-18s rate over the searches of >= 0.05 s: %s nodes/s" % ("", "%.3g" % rate.value if rate.value else "none that long"))
    for i, want, status, nodes, last in missed:
        print("  %-18s OUT OF BUDGET: state %d (optimal %d): %s after %d nodes, last threshold %s" % ("", i, want, status, nodes, last))
    sys.stdout.flush()
    return rate.value, records


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))


def puzzle_leg(env_name, specs, seconds, state_seconds, verbose, in_order):
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    z = golden()
    states, lens = z["%s_test_states" % env_name], z["%s_test_opt_len" % env_name].astype(int)
    ids = np.argsort(lens, kind="stable") if in_order else np.arange(len(lens))
    for spec in specs:
        t0 = time.time()
        pdb = PatternDatabase(env_name, spec).build()
        print("%s pdb:%s: %d bytes built in %.2f s" % (env_name, spec, pdb.bytes, time.time() - t0), flush=True)
        run_states(IDAStar(env_name, pdb), "%s %s" % (env_name, spec), states[ids], lens[ids], ids, seconds, state_seconds, verbose)
        del pdb


def reflect_leg(env_name, specs, seconds, state_seconds, verbose, in_order):
    """Per spec: the tables built once, a plain run and a reflected run over the same states in the same order, and the two
    compared on the states both solved."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    z = golden()
    states, lens = z["%s_test_states" % env_name], z["%s_test_opt_len" % env_name].astype(int)
    ids = np.argsort(lens, kind="stable") if in_order else np.arange(len(lens))
    for spec in specs:
        t0 = time.time()
        pdb = PatternDatabase(env_name, spec).build()
        print("%s pdb:%s: %d bytes built in %.2f s" % (env_name, spec, pdb.bytes, time.time() - t0), flush=True)
        runs = {}
        for reflect in (False, True):
            pdb.reflect = reflect  # the same tables: the suffix changes the look-up, not the bytes
            runs[reflect] = run_states(IDAStar(env_name, pdb), "%s %s" % (env_name, pdb.spec if reflect else spec), states[ids], lens[ids], ids,
                                       seconds, state_seconds, verbose)[1]
        both = [i for i in runs[False] if i in runs[True] and runs[False][i][0] and runs[True][i][0]]
        nodes = [sum(runs[r][i][1] for i in both) for r in (False, True)]
        secs = [sum(runs[r][i][2] for i in both) for r in (False, True)]
        fewer = sum(1 for i in both if runs[True][i][1] < runs[False][i][1])
        faster = sum(1 for i in both if runs[True][i][2] < runs[False][i][2])
        print("  %s %s, the %d states both runs solved: nodes plain %.4g, reflected %.4g (x %.3f); seconds plain %.2f, reflected %.2f (x %.3f)"
              % (env_name, spec, len(both), nodes[0], nodes[1], nodes[1] / nodes[0], secs[0], secs[1], secs[1] / secs[0]))
        print("  %-18s reflected has fewer nodes on %d and less time on %d of them; nodes/s plain %.3g, reflected %.3g"
              % ("", fewer, faster, nodes[0] / secs[0], nodes[1] / secs[1]), flush=True)
        del pdb


BATCH_SIZES = (1, 16, 64, 500)
BATCH_BUDGET = 1 << 36  # nodes per state, the same for every batch size: no shipped state of these legs comes near it


def batch_leg(env_name, specs, reflects, count, in_order):
    """Per spec and look-up: the tables built once, then the first `count` states searched in groups of each of BATCH_SIZES
    through the CLI's own group function (search_methods/idastar.solve_group: 1 is the single search, state by state), the
    single path first and once more at the end (the spread of the same work in the same process).  A leg's time is a host clock
    around the whole pass, which ends in a device synchronise; every state must come out solved at the shipped optimal length
    with the single path's thresholds and completed counts.  Seconds and rates are recorded, not met."""
    import torch
    from deepcubea_amd.search_methods.idastar import IDAStar, solve_group
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    z = golden()
    states, lens = z["%s_test_states" % env_name], z["%s_test_opt_len" % env_name].astype(int)
    ids = (np.argsort(lens, kind="stable") if in_order else np.arange(len(lens)))[:count]
    roots = [np.ascontiguousarray(states[i], dtype=np.uint8) for i in ids]
    for spec in specs:
        t0 = time.time()
        pdb = PatternDatabase(env_name, spec).build()
        print("%s pdb:%s: %d bytes built in %.2f s" % (env_name, spec, pdb.bytes, time.time() - t0), flush=True)
        for reflect in reflects:
            pdb.reflect = reflect  # the same tables: the suffix changes the look-up, not the bytes
            search = IDAStar(env_name, pdb)
            solve_group(search, roots[:1], BATCH_BUDGET)  # both kernels' code objects loaded in front of the first timed pass
            solve_group(search, roots[:2], BATCH_BUDGET)
            base = None
            for size in tuple(s for s in BATCH_SIZES if s < len(roots)) + (len(roots), 1):
                torch.cuda.synchronize()
                t0 = time.time()
                found = []
                for first in range(0, len(roots), size):
                    found += solve_group(search, roots[first:first + size], BATCH_BUDGET)
                torch.cuda.synchronize()
                dt = time.time() - t0
                for i, want, res in zip(ids, lens[ids], found):
                    assert res["solved"] and len(res["moves"]) == want, "state %d: %s, shipped optimal %d" % (i, res["status"], want)
                if base is None:
                    base = (found, dt)
                for i, res, one in zip(ids, found, base[0]):
                    assert res["thresholds"] == one["thresholds"] and res["nodes_per_threshold"][:-1] == one["nodes_per_threshold"][:-1], \
                        "state %d: batch %d differs from the single search" % (i, size)
                nodes = sum(res["nodes_generated"] for res in found)
                print("  %-22s batch %4d: %d states solved at the shipped optimal length, results equal the single path's | %8.2f s  "
                      "nodes %.4g  %.3g nodes/s  (x %.3f of the first single pass)"
                      % ("%s %s%s" % (env_name, spec, "+reflect" if reflect else ""), size, len(found), dt, nodes, nodes / dt, dt / base[1]),
                      flush=True)
        del pdb


def cube3_leg(seconds, state_seconds, verbose):
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    z = golden()
    states, lens = z["cube3_test_states"], z["cube3_test_opt_len"].astype(int)
    ids = np.argsort(lens, kind="stable")
    for spec in ("korf", "korf7"):
        t0 = time.time()
        pdb = Cube3PatternDatabase(spec).build()
        print("cube3 pdb:%s: %d bytes built in %.2f s" % (spec, pdb.bytes, time.time() - t0), flush=True)
        run_states(IDAStar("cube3", pdb), "cube3 %s" % spec, states[ids], lens[ids], ids, seconds, state_seconds, verbose)
        del pdb


def cube3_sym_leg(spec, seconds, state_seconds, verbose):
    """The tables built once; the plain search and the searches on the first N images of every pattern over the same states in
    the same order, compared on the states every configuration solved."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase, sym_lookups, sym_suffix
    z = golden()
    states, lens = z["cube3_test_states"], z["cube3_test_opt_len"].astype(int)
    ids = np.argsort(lens, kind="stable")
    t0 = time.time()
    pdb = Cube3PatternDatabase(spec).build()
    print("cube3 pdb:%s: %d bytes built in %.2f s" % (spec, pdb.bytes, time.time() - t0), flush=True)
    runs = {}
    for n in (0,) + SYM_IMAGES:
        pdb.sym = n  # the same tables: the suffix changes the look-ups, not the bytes
        label = "cube3 %s%s" % (spec, sym_suffix(n))
        print("  %-18s %d look-ups a node at the most" % (label, sym_lookups(pdb.patterns, n) if n else len(pdb.patterns)))
        runs[n] = run_states(IDAStar("cube3", pdb), label, states[ids], lens[ids], ids, seconds, state_seconds, verbose)[1]
    both = [i for i in runs[0] if all(i in r and r[i][0] for r in runs.values())]
    base_nodes, base_secs = sum(runs[0][i][1] for i in both), sum(runs[0][i][2] for i in both)
    print("  cube3 %s, the %d states every configuration ran and solved (optimal length %s):"
          % (spec, len(both), "%d .. %d" % (min(lens[both]), max(lens[both])) if both else "-"))
    for n, r in runs.items():
        nodes, secs = sum(r[i][1] for i in both), sum(r[i][2] for i in both)
        print("  %-18s states run %3d solved %3d | nodes %.4g (x %.4f of plain)  seconds %.3f (x %.4f of plain)  %.3g nodes/s"
              % (spec + sym_suffix(n), len(r), sum(1 for v in r.values() if v[0]), nodes, nodes / base_nodes, secs, secs / base_secs,
                 nodes / secs), flush=True)


def cube3_dual_leg(spec, seconds, state_seconds, verbose):
    """cube3_sym_leg's method over DUAL_CONFIGS: the tables built once, every configuration over the same states in the same
    order, compared on the states every configuration solved, as ratios to the plain run."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase, sym_lookups, sym_suffix
    z = golden()
    states, lens = z["cube3_test_states"], z["cube3_test_opt_len"].astype(int)
    ids = np.argsort(lens, kind="stable")
    t0 = time.time()
    pdb = Cube3PatternDatabase(spec).build()
    print("cube3 pdb:%s: %d bytes built in %.2f s" % (spec, pdb.bytes, time.time() - t0), flush=True)
    whole = sum(1 for kind, g in pdb.patterns if len(g) == (8 if kind == 0 else 12))  # skipped in the second pass
    runs = {}
    for n, dual in DUAL_CONFIGS:
        pdb.sym, pdb.dual = n, dual  # the same tables: the suffixes change the look-ups, not the bytes
        label = "cube3 %s%s" % (spec, sym_suffix(n, dual))
        first = sym_lookups(pdb.patterns, n) if n else len(pdb.patterns)
        print("  %-24s %d%s look-ups a node at the most" % (label, first, " + %d" % (first - whole) if dual else ""))
        runs[(n, dual)] = run_states(IDAStar("cube3", pdb), label, states[ids], lens[ids], ids, seconds, state_seconds, verbose)[1]
    both = [i for i in runs[(0, False)] if all(i in r and r[i][0] for r in runs.values())]
    base_nodes, base_secs = (sum(runs[(0, False)][i][k] for i in both) for k in (1, 2))
    print("  cube3 %s, the %d states every configuration ran and solved (optimal length %s):"
          % (spec, len(both), "%d .. %d" % (min(lens[both]), max(lens[both])) if both else "-"))
    for (n, dual), r in runs.items():
        nodes, secs = sum(r[i][1] for i in both), sum(r[i][2] for i in both)
        deepest = max([int(lens[i]) for i in r], default=0)
        print("  %-18s states run %3d solved %3d | nodes %.4g (x %.4f of plain)  seconds %.3f (x %.4f of plain)  %.3g nodes/s | deepest "
              "state run %d moves: %s" % (spec + sym_suffix(n, dual), len(r), sum(1 for v in r.values() if v[0]), nodes, nodes / base_nodes, secs,
                                          secs / base_secs, nodes / secs, deepest, "21 or more reached" if deepest >= 21 else "none of 21 or more"),
              flush=True)
    for n in sorted({n for n, dual in DUAL_CONFIGS if dual and (n, False) in runs}):
        a, b = runs[(n, False)], runs[(n, True)]
        pair = [i for i in a if i in b and a[i][0] and b[i][0]]
        nodes, secs = [sum(r[i][1] for i in pair) for r in (a, b)], [sum(r[i][2] for i in pair) for r in (a, b)]
        print("  %-18s against %s on the %d states both solved: nodes x %.4f, seconds x %.4f"
              % (spec + sym_suffix(n, True), spec + sym_suffix(n) if n else "plain", len(pair), nodes[1] / nodes[0], secs[1] / secs[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idastar_probe.txt"))
    ap.add_argument("--legs", default="resources,puzzle15,puzzle24,cube3")
    ap.add_argument("--seconds", type=float, default=150.0, help="seconds of search per pattern set")
    ap.add_argument("--state_seconds", type=float, default=40.0, help="a state's node budget, in seconds at the measured rate")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        if args.leg == "resources":
            resources_leg()
        elif args.leg == "puzzle15":
            puzzle_leg("puzzle15", ("5-5-5", "6-6-3"), 1e9, args.state_seconds, args.verbose, False)
        elif args.leg == "puzzle24":
            puzzle_leg("puzzle24", ("6-6-6-6",), args.seconds, args.state_seconds, args.verbose, True)
        elif args.leg == "puzzle15_reflect":
            reflect_leg("puzzle15", ("5-5-5", "6-6-3"), 1e9, args.state_seconds, args.verbose, False)
        elif args.leg == "puzzle24_reflect":
            reflect_leg("puzzle24", ("6-6-6-6",), args.seconds, args.state_seconds, args.verbose, True)
        elif args.leg == "puzzle15_batch":
            batch_leg("puzzle15", ("5-5-5", "6-6-3"), (False, True), 500, False)
        elif args.leg == "puzzle24_batch":
            batch_leg("puzzle24", ("6-6-6-6",), (False,), 44, True)
        elif args.leg == "cube3":
            cube3_leg(args.seconds, args.state_seconds, args.verbose)
        elif args.leg in ("cube3_sym_korf", "cube3_sym_korf7"):
            cube3_sym_leg(args.leg.rsplit("_", 1)[1], args.seconds, args.state_seconds, args.verbose)
        elif args.leg in ("cube3_dual_korf", "cube3_dual_korf7"):
            cube3_dual_leg(args.leg.rsplit("_", 1)[1], args.seconds, args.state_seconds, args.verbose)
        else:
            raise ValueError("unknown leg %r" % args.leg)
        return
    lines = ["IDA* on the pattern databases (tools/idastar_probe.py), one MI355X; --seconds %g --state_seconds %g" % (args.seconds, args.state_seconds),
             "For comparison, the batched A* engine on the same tables (DESIGN 4.6): puzzle15 5-5-5 solves 460 of 500 and 6-6-3 492 of 500",
             "inside its 2^24-id pool; no puzzle24 search with 6-6-6-6; cube3 korf roots up to 13 moves from the goal.", ""]
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--seconds", str(args.seconds),
               "--state_seconds", str(args.state_seconds)] + (["--verbose"] if args.verbose else [])
        print("---- leg %s" % leg, flush=True)
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        out = []
        for ln in p.stdout:  # passed on as it comes: a leg of several minutes is not silent
            print(ln, end="", flush=True)
            out.append(ln.rstrip("\n"))
        p.wait()
        lines += ["---- leg %s (exit %d)" % (leg, p.returncode)] + out + [""]
        if p.returncode != 0:
            lines.append("leg %s failed: the visit ends here" % leg)
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if lines[-1] == "" else 1)


if __name__ == "__main__":
    main()
