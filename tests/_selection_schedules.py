"""Directed cost schedules for the engine's selection kernels (helper of test_engine_selection_{cpu,hip}.py; no tests here).

The split stepping (pop_expand -> caller's heuristic -> commit) lets a test choose every child's cost, and the oracle's
`astar(..., heur_fn=...)` calls `heur_fn` once for the root and then once per iteration on all npop*A children in
rank*A + move order — the order of the engine's `last_children()`.  A heuristic that is a pure function of (call index,
hash of the state row) is therefore legal on both sides.  The oracle's run is RECORDED (per call: row count, row hashes,
h values); the GPU test compares the engine's children hashes with the record element for element — the exact pop order
of every parent, ties included — and hands the recorded h values back, so no float is ever recomputed.

All schedules produce float32 values that are exact in float32 by construction (small integer multiples of a power of
two, or powers of two), so the float64 cost w*g + h of the two sides is the same bit pattern."""
from __future__ import annotations

import heapq
from collections import Counter

import numpy as np

_FNV_OFFSET = np.uint64(0xCBF29CE484222325)
_FNV_PRIME = np.uint64(0x100000001B3)


def row_hash(states: np.ndarray) -> np.ndarray:
    """uint64 [n]: FNV-1a over the bytes of each row, then a shift-xor-multiply finaliser (the low bits of plain FNV-1a
    are weak, and the schedules take `hash % q`)."""
    s = np.ascontiguousarray(states, np.uint8)
    assert s.ndim == 2
    h = np.full(s.shape[0], _FNV_OFFSET, np.uint64)
    for j in range(s.shape[1]):
        h ^= s[:, j].astype(np.uint64)
        h *= _FNV_PRIME  # (array arithmetic wraps modulo 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return h


def ulp32(c: float) -> float:
    return float(np.spacing(np.float32(c)))


def _levels(hashes: np.ndarray, c: float, q: int, step: float) -> np.ndarray:
    v = (np.float64(c) + (hashes % np.uint64(q)).astype(np.float64) * step).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.float64(c) + (hashes % np.uint64(q)).astype(np.float64) * step)  # exact
    return v


class Schedule:
    """sched(call_index, hashes u64 [n]) -> h f32 [n]; `weight` is the weight of path cost the schedule is meant for."""
    name = ""
    weight = 0.0

    def __call__(self, call: int, hashes: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def __repr__(self):
        return self.name


C0 = 100.0  # the ulp-spaced schedules sit just above it: ulp32(100) = 2^-17, and 100 + 4095 ulps stays inside the binade


class OneLevel(Schedule):
    """All of OPEN is one tie group for ever: the order is by id alone."""
    name = "one_level"

    def __call__(self, call, hashes):
        return np.full(hashes.shape[0], C0, np.float32)


class UlpLevels(Schedule):
    """q adjacent float32 values: distinct and tied keys mixed inside one or a few bins.  As float64 keys they differ
    from bit 29 upwards only."""

    def __init__(self, q: int):
        self.q = q
        self.name = "ulp_levels(%d)" % q

    def __call__(self, call, hashes):
        return _levels(hashes, C0, self.q, ulp32(C0))


OUTLIER = np.float32(3e38)


class Outlier(Schedule):
    """ulp_levels(q) with about one child in a thousand at 3e38 — and one child of the root for certain: the key range is
    blown up from the first iteration on, the shift is large and the ordinary entries collapse into a single bin."""

    def __init__(self, q: int = 64):
        self.q = q
        self.name = "outlier" if q == 64 else "outlier(%d)" % q

    def __call__(self, call, hashes):
        v = _levels(hashes, C0, self.q, ulp32(C0))
        out = (hashes >> np.uint64(20)) % np.uint64(1000) == np.uint64(0)
        if call == 1:
            out = out | (hashes == hashes.min())
        v[out] = OUTLIER
        return v


class Regime(Schedule):
    """Calls 0..t1 near 100 (64 ulp-spaced levels), calls t1+1..t2 near 1 (64 ulp-spaced levels), later calls 5000 + 4096
    integer levels: children far BELOW the binning's kmin between two rebases (bin 0 clamp), then far above it (last-bin
    clamp, or beyond T into BACK).  `regime` changes after calls 10 and 22; `regime_fast` after calls 3 and 6, for the runs
    of 10 iterations."""

    def __init__(self, t1: int = 10, t2: int = 22):
        self.t1, self.t2 = t1, t2
        self.name = "regime" if (t1, t2) == (10, 22) else "regime_fast"

    def phase(self, call: int) -> int:
        return 0 if call <= self.t1 else 1 if call <= self.t2 else 2

    def __call__(self, call, hashes):
        ph = self.phase(call)
        if ph == 0:
            return _levels(hashes, 100.0, 64, ulp32(100.0))
        if ph == 1:
            return _levels(hashes, 1.0, 64, ulp32(1.0))
        return _levels(hashes, 5000.0, 4096, 1.0)


class DepthMicro(Schedule):
    """Costs dominated by w*g (w = 1) with a three-level micro-structure under it."""
    name = "depth_micro"
    weight = 1.0

    def __call__(self, call, hashes):
        return _levels(hashes, 0.0, 3, 2.0 ** -20)


class Wide(Schedule):
    """Keys spread over 120 binades (w = 0.5): log-spaced bins, dense low bins."""
    name = "wide"
    weight = 0.5

    def __call__(self, call, hashes):
        return np.ldexp(np.float32(1.0), (hashes % np.uint64(120)).astype(np.int32) - 60).astype(np.float32)


SCHEDULES = {s.name: s for s in [OneLevel(), UlpLevels(2), UlpLevels(64), UlpLevels(4096), Outlier(), Outlier(2),
                                 Outlier(4096), Regime(), Regime(3, 6), DepthMicro(), Wide()]}
MAIN_GRID = ["one_level", "ulp_levels(2)", "ulp_levels(64)", "ulp_levels(4096)", "outlier", "regime", "depth_micro", "wide"]

# (env, batch, schedule, iterations, variant): every case of test_engine_selection_hip.py; test_engine_selection_cpu.py checks
# the oracle side of each.  variant: "" = the engine as shipped, "tiers(k,m)" = set_tiers(k, m), "grid_off" = created while
# the grid-wide refinement is switched off.
CASES = (
    # creep: one threshold bin growing by 0-2 entries per iteration through 512/513 and 1024/1025.  Under ulp_levels(2) the
    # two keys get a bin each and the cheaper one is drained first (its group never exceeds ~100 entries), so the case that
    # creeps a bin of two DISTINCT keys through the boundaries is outlier(2): the outlier collapses both keys into bin 0.
    [("puzzle15", 1, n, 1400, "") for n in ("one_level", "ulp_levels(2)", "outlier(2)")]
    + [("cube3", 700, n, 34, "") for n in MAIN_GRID]
    + [("cube3", b, n, 60, "") for b in (1, 64) for n in ("ulp_levels(64)", "outlier", "regime")]
    # large batch: 4096 evenly spaced levels get a bin each (thread-per-entry ranking only) and `regime` never leaves its first
    # phase in 10 iterations; what sends a batch beyond 8192 entries through the sub-bins of ONE bin with distinct keys is
    # outlier(4096) (every ordinary entry in bin 0) and regime_fast (the stale binning's bin 0, then its last bin)
    + [("cube3", 9000, n, 10, "") for n in ("ulp_levels(4096)", "regime", "regime_fast", "outlier(4096)")]
    + [(e, b, n, 40, "") for e, b in (("puzzle15", 33), ("lightsout7", 17)) for n in ("regime", "outlier")]
    + [("cube3", 700, n, 34, v) for v in ("tiers(1,1)", "tiers(40,100)") for n in ("regime", "outlier", "wide")]
    # grid path off: ulp_levels(64) alone has no bin beyond 8192 entries (64 bins of ~3 000); with the outlier it has
    + [("cube3", 700, n, 34, "grid_off") for n in ("ulp_levels(64)", "regime", "outlier")])


def case_id(case) -> str:
    env, B, name, iters, variant = case
    return "-".join([env, "B%d" % B, name, "%dit" % iters] + ([variant] if variant else []))


_RUNS = {}


def oracle_run(co, env: str, B: int, name: str, iters: int):
    """run_oracle of one (env, batch, schedule, iterations) from deep_root(env, 0), computed once per process and shared by
    the cases that differ in the engine's variant only.  Nobody may modify what it returns."""
    key = (env, B, name, iters)
    if key not in _RUNS:
        s = SCHEDULES[name]
        _RUNS[key] = run_oracle(co, env, deep_root(co, env, 0), B, s.weight, s, iters)
    return _RUNS[key]


WALK = {"cube3": 40, "puzzle15": 200, "lightsout7": 200}


def deep_root(co, env: str, seed: int = 0) -> np.ndarray:
    """A fixed-seed random walk from the goal: 40 moves for cube3, 200 for the puzzles and lightsout7."""
    A = co.num_moves(env)
    D = {"cube3": 54, "puzzle15": 16, "lightsout7": 49}[env]
    if env == "cube3":
        s = np.arange(D, dtype=np.uint8)[None]
    elif env == "puzzle15":
        s = np.concatenate([np.arange(1, D, dtype=np.uint8), np.zeros(1, np.uint8)])[None]
    else:
        s = np.zeros((1, D), np.uint8)
    assert co.is_solved(env, s)[0]
    rng = np.random.default_rng(1000 + seed)
    for a in rng.integers(0, A, WALK[env]):
        s = co.next_state(env, s, int(a))
    assert not co.is_solved(env, s)[0]
    return np.ascontiguousarray(s[0])


def run_oracle(co, env: str, root: np.ndarray, B: int, w: float, sched: Schedule, iters: int):
    """-> (oracle result with a per-iteration trace, record): record[k] = (n, row hashes u64 [n], h f32 [n]) of the k-th
    heuristic call (call 0 = the root)."""
    rec = []

    def heur(states):
        hs = row_hash(states)
        hv = np.asarray(sched(len(rec), hs), np.float32)
        assert hv.shape == hs.shape
        rec.append((int(states.shape[0]), hs, hv))
        return hv

    res = co.astar(env, root, w, B, co.SEM_PY, heur_fn=heur, max_iters=iters, trace_cap=iters)
    return res, rec


def open_census(rec, B: int, A: int, w: float, trace=None):
    """Replays the search from the record alone (states stand in by their 64-bit row hash) and returns, per iteration,
    a Counter {float64 cost: entries} of OPEN as the iteration's pop finds it.  This is what the reach assertion "a giant
    bin holds more than one distinct key" is computed from.  With `trace` (the oracle's), the replay checks itself: OPEN
    and CLOSED sizes after every iteration must equal the oracle's.  (No child may be solved: the cases never reach a goal.)"""
    n0, hs0, hv0 = rec[0]
    c0 = w * 0.0 + max(float(hv0[0]), 0.0)
    g = [0.0]
    cost = [c0]
    heap = [(c0, 0, 0)]
    cnt = 1
    closed = {}
    live = Counter({c0: 1})
    out = []
    for it in range(len(rec) - 1):
        out.append(Counter(live))
        npop = min(B, len(heap))
        popped = [heapq.heappop(heap)[2] for _ in range(npop)]
        for nid in popped:
            live[cost[nid]] -= 1
            if live[cost[nid]] == 0:
                del live[cost[nid]]
        n, hs, hv = rec[it + 1]
        assert n == npop * A, (it, n, npop)
        for j in range(n):
            gp = g[popped[j // A]] + 1.0
            c = w * gp + max(float(hv[j]), 0.0)
            key = int(hs[j])
            old = closed.get(key)
            if old is None or old > gp:
                closed[key] = gp
                nid = len(g)
                g.append(gp)
                cost.append(c)
                heapq.heappush(heap, (c, cnt, nid))
                cnt += 1
                live[c] += 1
        if trace is not None:
            assert (len(heap), len(closed)) == (int(trace[it][0]), int(trace[it][1])), (it, len(heap), len(closed), trace[it])
    return out
