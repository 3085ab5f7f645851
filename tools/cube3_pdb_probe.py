"""Cube3 pattern databases on the MI355X, measured once -> profiles/cube3_pdb_probe.txt.

    python tools/cube3_pdb_probe.py [--out profiles/cube3_pdb_probe.txt] [--legs build,eval,search]

One GPU visit.  Every leg runs in a fresh child process under its own `timeout`, one after another, and the visit ends at the
first leg that does not exit 0 (nothing is started on a device after a leg has failed on it).  Legs:
  build   build time and sweeps of every table of the presets korf and korf7; the depth histogram of the corner table, which
          must equal the one a breadth-first search of all 88 179 840 corner states gives on the host.
  eval    dca_cube3_pdb_eval on korf at 131 072 and 245 760 rows of 40-move scrambles (network-input rows), median of 20
          launches, next to the puzzle15 5-5-5 eval timed in the same process.
  search  korf at --weight 1 --semantics cpp, batch 1000, `--max_nodes auto`, on roots taken from the shipped optimal paths at
          remaining distance 8 .. 13: length found against the known distance, nodes generated, seconds; the same under
          builtin:zero while it still fits.
  eval_sym  dca_cube3_pdb_eval_sym on korf with the first N images of every pattern, N in 1, 2, 4, 8, 24 and all, next to the plain
          eval on the same rows in the same process: the cost per row against the plain eval.  `--legs eval_sym --append --out
          profiles/idastar_sym_probe.txt` adds it to the symmetric searches' record.
  eval_dual  dca_cube3_pdb_eval_dual on korf with `+dual` alone and with `+sym:N+dual` for N in 4, 8 and all, next to the plain
          eval and the symmetric eval at the same N on the same rows in the same process: the cost per row against both.
          `--legs eval_dual --append --out profiles/idastar_dual_probe.txt` adds it to the dual searches' record.
No threshold is set on any time: the numbers are recorded, not met."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepcubea_amd import _lib  # noqa: E402
from deepcubea_amd.search_methods.engine import BwasEngine  # noqa: E402
from deepcubea_amd.utils.cube3_pdb import PRESETS, Cube3PatternDatabase, spec_of  # noqa: E402

LEG_TIMEOUT_S = {"build": 420, "eval": 150, "search": 420, "eval_sym": 150, "eval_dual": 150}
CORNER_HISTOGRAM = [1, 12, 114, 924, 6539, 39528, 199926, 806136, 2761740, 8656152, 22334112, 32420448, 18780864, 2166720, 6624]


def timed_build(pattern):
    torch.cuda.synchronize()
    t0 = time.time()
    table, sweeps = _lib.cube3_pdb_build(*pattern)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("build  %-28s %11d bytes  %8.3f s  sweeps %d" % (spec_of((pattern,)), table.numel(), dt, sweeps), flush=True)
    return table, sweeps, dt


def build_leg():
    seconds = {}
    for pattern in dict.fromkeys(PRESETS["korf"] + PRESETS["korf7"]):  # the corner table once
        table, sweeps, dt = timed_build(pattern)
        seconds[pattern] = dt
        if pattern == PRESETS["corners"][0]:
            hist = torch.bincount(table.to(torch.int64), minlength=256).cpu().numpy()
            reached = hist[:0xFE]
            depth = [int(x) for x in reached[:int(np.nonzero(reached)[0].max()) + 1]]
            print("       corner depth histogram %s: sum %d, unreached (0xFE) %d, sweeps %d" % (depth, sum(depth), int(hist[0xFE]), sweeps))
            assert depth == CORNER_HISTOGRAM and sum(depth) == 88179840 and int(hist[0xFE]) == 264539520 - 88179840, "corner table"
            print("       equals the host breadth-first histogram (deepest level 14)", flush=True)
        del table
        torch.cuda.empty_cache()
    for name in ("korf", "korf7"):
        pdb = Cube3PatternDatabase(name)
        print("preset %-6s %11d bytes  %8.3f s in all" % (name, pdb.bytes, sum(seconds[p] for p in pdb.patterns)), flush=True)


def scramble_rows(rows, seed=0):
    perm = _lib.lib().dca_cube3_perm_table()
    p = np.array([perm[i] for i in range(12 * 54)], np.int64).reshape(12, 54)
    rng = np.random.default_rng(seed)
    s = np.tile(np.arange(54, dtype=np.uint8), (rows, 1))
    idx = np.arange(rows)[:, None]
    for _ in range(40):
        s = s[idx, p[rng.integers(0, 12, rows)]]
    return s


def median_us(fn, reps=20):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), min(times)


def eval_leg():
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    korf = Cube3PatternDatabase("korf").build()
    p15 = PatternDatabase("puzzle15", "5-5-5").build()
    rng = np.random.default_rng(0)
    for rows in (131072, 245760):
        X = torch.from_numpy(scramble_rows(rows) // 9).cuda()
        out = torch.empty(rows, dtype=torch.float32, device="cuda")
        med, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out))
        print("eval   cube3    korf   %7d rows (40-move scrambles, colour rows)  median %.1f us  min %.1f us  %.3g rows/s (median of 20)"
              % (rows, med, low, rows / (med * 1e-6)), flush=True)
        P = torch.from_numpy(rng.permuted(np.tile(np.arange(16, dtype=np.uint8), (rows, 1)), axis=1)).cuda()
        med, low = median_us(lambda: _lib.pdb_eval(4, P, p15.partition, p15.tables, out=out))
        print("eval   puzzle15 5-5-5  %7d rows (uniform random permutations)     median %.1f us  min %.1f us  %.3g rows/s (median of 20)"
              % (rows, med, low, rows / (med * 1e-6)), flush=True)


def eval_sym_leg():
    from deepcubea_amd.utils.cube3_pdb import sym_lookups
    korf = Cube3PatternDatabase("korf").build()
    for rows in (131072, 245760):
        X = torch.from_numpy(scramble_rows(rows) // 9).cuda()
        out = torch.empty(rows, dtype=torch.float32, device="cuda")
        plain, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out))
        print("eval   cube3 korf         %7d rows   3 look-ups  median %7.1f us  min %7.1f us  %6.3f ns/row" % (rows, plain, low, plain * 1e3 / rows),
              flush=True)
        for n in (1, 2, 4, 8, 24, 48):
            med, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out, sym=n))
            print("eval   cube3 korf+sym:%-3d %7d rows  %2d look-ups  median %7.1f us  min %7.1f us  %6.3f ns/row  x %.2f of the plain eval"
                  % (n, rows, sym_lookups(korf.patterns, n), med, low, med * 1e3 / rows, med / plain), flush=True)


def eval_dual_leg():
    from deepcubea_amd.utils.cube3_pdb import sym_lookups
    korf = Cube3PatternDatabase("korf").build()
    for rows in (131072, 245760):
        X = torch.from_numpy(scramble_rows(rows) // 9).cuda()
        out = torch.empty(rows, dtype=torch.float32, device="cuda")
        plain, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out))
        print("eval   cube3 korf              %7d rows   3 look-ups          median %7.1f us  min %7.1f us  %6.3f ns/row"
              % (rows, plain, low, plain * 1e3 / rows), flush=True)
        for n in (1, 4, 8, 48):
            lookups = sym_lookups(korf.patterns, n)
            whole = sum(1 for kind, g in korf.patterns if len(g) == _lib.CUBE3_PDB_SLOTS[kind][0])  # one image each, skipped in the second pass
            base, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out, sym=n))
            print("eval   cube3 korf+sym:%-3d      %7d rows  %2d look-ups          median %7.1f us  min %7.1f us  %6.3f ns/row  x %.2f of the plain eval"
                  % (n, rows, lookups, base, low, base * 1e3 / rows, base / plain), flush=True)
            med, low = median_us(lambda: _lib.cube3_pdb_eval(X, _lib.ROWS_NNET, korf.patterns, korf.tables, out=out, sym=n, dual=True))
            print("eval   cube3 korf+sym:%-3d+dual %7d rows  %2d + %2d look-ups     median %7.1f us  min %7.1f us  %6.3f ns/row  x %.2f of the plain eval,"
                  " x %.2f of +sym:%d" % (n, rows, lookups, lookups - whole, med, low, med * 1e3 / rows, med / plain, med / base, n), flush=True)


def path_roots(distances, instances):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    perm = _lib.lib().dca_cube3_perm_table()
    p = np.array([perm[i] for i in range(12 * 54)], np.int64).reshape(12, 54)
    roots = []
    for i in range(instances):
        s, L = g["cube3_test_states"][i].astype(np.uint8), int(g["cube3_test_opt_len"][i])
        along = [s]
        for a in g["cube3_test_opt_moves"][i][:L]:
            along.append(along[-1][p[int(a)]])
        roots += [(i, d, along[L - d]) for d in distances]
    return sorted(roots, key=lambda r: (r[1], r[0]))


def search_leg(budget_s=150.0):
    korf = Cube3PatternDatabase("korf").build()
    fn = korf.heuristic_fn_dev()
    cap = BwasEngine.auto_max_nodes("cube3", 1000, 1)
    print("search cube3, weight 1, cpp semantics, batch 1000, max_nodes auto = %d ids" % cap, flush=True)
    roots = path_roots(range(8, 14), 2)
    for label in ("pdb:korf", "builtin:zero"):  # one engine at a time: each takes the pool `auto` sizes from the free memory
        eng = BwasEngine("cube3", 1.0, 1000, max_nodes=cap, semantics=_lib.SEM_CPP, packed=label == "pdb:korf")
        t_start = time.time()
        for i, d, root in roots:
            if time.time() - t_start > budget_s:
                print("search %s stopped: its time budget is used up" % label, flush=True)
                break
            t0 = time.time()
            if label == "pdb:korf":
                res = eng.solve(root, fn, max_iters=1 << 20)
            else:
                res = eng.solve_builtin(root, _lib.HEUR_ZERO, chunk=32, use_graph=True)
            dt = time.time() - t0
            print("search instance %d distance %2d  %-12s  length %2d  nodes generated %12d  %9.4f s%s"
                  % (i, d, label, len(res["moves"]) if res["solved"] else -1, res["nodes_generated"], dt,
                     "" if res["solved"] else "  NOT SOLVED inside the pool: deeper roots are left out"), flush=True)
            if not res["solved"]:
                break
        eng.close()
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube3_pdb_probe.txt"))
    ap.add_argument("--legs", default="build,eval,search")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--leg", default=None, help="run one leg in this process (what the driver starts under `timeout`)")
    args = ap.parse_args()
    if args.leg:
        _lib.require_gpu()
        print("probe leg %s on %s" % (args.leg, torch.cuda.get_device_name(0)), flush=True)
        {"build": build_leg, "eval": eval_leg, "search": search_leg, "eval_sym": eval_sym_leg, "eval_dual": eval_dual_leg}[args.leg]()
        return 0
    lines = ["$ python tools/cube3_pdb_probe.py --legs %s" % args.legs]
    rc = 0
    for leg in args.legs.split(","):
        limit = LEG_TIMEOUT_S[leg]
        child = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for ln in child.stdout:  # passed on as it comes
            print(ln, end="", flush=True)
            if ln.startswith(("probe", "build", "preset", "eval", "search", "     ")):
                lines.append(ln.rstrip("\n"))
        if child.wait() != 0:
            lines.append("leg %s ended with exit status %d (limit %d s): the visit stops here" % (leg, child.returncode, limit))
            print(lines[-1], flush=True)
            rc = child.returncode
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
