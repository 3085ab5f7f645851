"""IDA* on the pattern databases, host side (no device needed): dca_idastar_host (include/dca_debug.h) runs the kernel's own move,
index-update, pruning and work-item code sequentially from tables built on the host.  Checked here: the cube3 pruning rules
against an enumeration written below, exact lengths against puzzle8's breadth-first table, thresholds and node counts against a
plain recursive IDA*, every refusal, the ABI triple and the CLI's refusals."""
import ctypes as C
import os
import re
import sys
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_cube3_pdb_cpu as c3
from tests import test_pdb_cpu as pz
from tests import test_puzzle8_cpu as p8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_idastar_npuzzle", "dca_idastar_cube3", "dca_idastar_host", "dca_idastar_set_prefix")
P8_PARTITION = ((1, 2, 3, 4), (5, 6, 7, 8))
RETAINED = [12, 114, 1068, 10011, 93840, 879624]  # cube3 move sequences of length 1..6 that the pruning rules keep
LEVELS = [12, 114, 1068, 10011, 93840, 878880]    # cube3 states at breadth-first distance 1..6
C3_SMALL = (c3.CORNERS, (4, 5, 6, 7))
BIG = 1 << 40


# ------------------------------------------------------------------------------------------------ helpers (shared with the GPU tests)
def p8_tables():
    return [pz.host_table(3, g) for g in P8_PARTITION]


def p8_states_at(distance, count, seed=0):
    states, dist, _ = p8.bfs_table()
    rows = np.flatnonzero(dist == distance)
    pick = np.random.default_rng(seed + distance).permutation(len(rows))[:count]
    return states[rows[np.sort(pick)]]


def replay_puzzle(dim, root, moves):
    """The root after `moves`, by the numpy restatement of the environment; a no-op move is an error."""
    from deepcubea_amd import _lib
    swap = _lib.npuzzle_swap_table(dim) if dim != 3 else np.array(p8.SWAP)
    cur = np.asarray(root, np.uint8)[None]
    for a in moves:
        nxt = p8.move_np(cur, int(a), swap)
        assert not np.array_equal(nxt, cur), "a no-op move in a solution"
        cur = nxt
    return cur[0]


def puzzle_goal(dim):
    return np.array(list(range(1, dim * dim)) + [0], np.uint8)


def replay_cube3(root, moves):
    cur = np.asarray(root, np.uint8)
    for a in moves:
        cur = cur[c3.perm_table()[int(a)]]
    return cur


def cube3_allowed(a, m, mp):
    """The header's pruning rules, restated: may move a follow m (and mp before it)?  None = no such move."""
    if m is None:
        return True
    if a == m ^ 1 or (a == m and a & 1) or (a == m and m == mp):
        return False
    return not ((a >> 1) == ((m >> 1) ^ 1) and (a >> 1) < (m >> 1))


def cube3_suffix_root(instance, k, golden=None):
    """The state k moves from the goal on shipped instance `instance`'s optimal path (a suffix of an optimal path is optimal)."""
    z = golden if golden is not None else np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    L = int(z["cube3_test_opt_len"][instance])
    assert 0 <= k <= L
    return replay_cube3(z["cube3_test_states"][instance], z["cube3_test_opt_moves"][instance][:L - k])


def reference_idastar_puzzle(dim, root, partition, tables, stop_at):
    """A plain recursive IDA*: table look-ups through the header's index rule, children counted when generated.  Runs the
    thresholds below `stop_at` (the known distance) -> (thresholds, node counts)."""
    N = dim * dim
    nb = [[int(x) for x in row] for row in (p8.SWAP if dim == 3 else None)]

    def h(state):
        total = 0
        for tiles, table in zip(partition, tables):
            idx = 0
            for t in reversed(tiles):
                idx = idx * N + state.index(t)
            total += int(table[idx * N + state.index(0)])
        return total

    def visit(state, g, last, T, acc):
        z = state.index(0)
        for a in range(4):
            q = nb[z][a]
            if q == z or (last is not None and a == last ^ 1):
                continue
            child = list(state)
            child[z], child[q] = child[q], 0
            child = tuple(child)
            acc[0] += 1
            f = g + 1 + h(child)
            if f <= T:
                visit(child, g + 1, a, T, acc)
            else:
                acc[1] = min(acc[1], f)

    root = tuple(int(x) for x in root)
    T, thresholds, counts = h(root), [], []
    while T < stop_at:
        acc = [0, 1 << 30]
        visit(root, 0, None, T, acc)
        thresholds.append(T)
        counts.append(acc[0])
        T = acc[1]
    return thresholds, counts


def reference_idastar_cube3(root, pattern, table, stop_at):
    """The same for cube3 with ONE pattern: h depends on the pattern's cubie locations alone, so the recursion carries only
    those (moved by the location-move table the tests derive); the index is the header's rank rule in plain integers."""
    kind, cubies = pattern
    n, o = c3.SLOTS[kind]
    mv = [[int(x) for x in row] for row in c3.location_moves(kind)]
    k = len(cubies)

    def h(locs):
        rank = orient = 0
        for j in range(k):
            s, r = divmod(locs[j], o)
            rank = rank * (n - j) + s - sum(1 for i in range(j) if locs[i] // o < s)
            orient = orient * o + r
        return int(table[rank * o ** k + orient])

    def visit(locs, g, m, mp, T, acc):
        for a in range(12):
            if not cube3_allowed(a, m, mp):
                continue
            child = tuple(mv[a][x] for x in locs)
            acc[0] += 1
            f = g + 1 + h(child)
            if f <= T:
                visit(child, g + 1, a, m, T, acc)
            else:
                acc[1] = min(acc[1], f)

    locs = tuple(int(x) for x in c3.locations_of_states(kind, cubies, np.asarray(root)[None])[0])
    T, thresholds, counts = h(locs), [], []
    while T < stop_at:
        acc = [0, 1 << 30]
        visit(locs, 0, None, None, T, acc)
        thresholds.append(T)
        counts.append(acc[0])
        T = acc[1]
    return thresholds, counts


@lru_cache(maxsize=None)
def p8_count_cases():
    """Three puzzle8 roots (distances 18, 22, 24) with their reference thresholds and counts, computed once."""
    cases = []
    for distance in (18, 22, 24):
        root = p8_states_at(distance, 1, seed=7)[0]
        thresholds, counts = reference_idastar_puzzle(3, root, P8_PARTITION, p8_tables(), distance)
        assert sum(counts) < 200000
        cases.append((root, distance, thresholds, counts))
    return cases


@lru_cache(maxsize=None)
def c3_count_case():
    root = cube3_suffix_root(0, 7)
    table = c3.host_table(*C3_SMALL)
    thresholds, counts = reference_idastar_cube3(root, C3_SMALL, table, 7)
    return root, table, thresholds, counts


def host_puzzle(dim, root, partition, tables, max_nodes=BIG):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_NPUZZLE, dim, root, partition, tables, max_nodes)


def host_cube3(root, patterns, tables, max_nodes=BIG):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_CUBE3, 0, root, patterns, tables, max_nodes)


@pytest.fixture
def prefix():
    """Sets the work items' prefix depth for one test and puts the default back."""
    from deepcubea_amd import _lib
    yield _lib.idastar_set_prefix
    _lib.idastar_set_prefix(-1)


# ------------------------------------------------------------------------------------------------ cube3 pruning rules
def test_cube3_pruning_counts_and_cover_by_enumeration():
    """The rules as restated above keep 12, 114, 1068, 10011, 93840 sequences of length 1..5, and at every depth these reach
    every state of that breadth-first level."""
    p = c3.perm_table()
    seqs = [(None, None)]
    states = np.arange(54, dtype=np.uint8)[None]
    seen = {states[0].tobytes()}
    for depth in range(1, 6):
        src, last = [], []
        for i, (m, mp) in enumerate(seqs):
            for a in range(12):
                if cube3_allowed(a, m, mp):
                    src.append(i)
                    last.append((a, m))
        src = np.array(src)
        moves = np.array([a for a, _ in last])
        states = states[src][np.arange(len(src))[:, None], p[moves]]
        seqs = last
        assert len(seqs) == RETAINED[depth - 1]
        rows = {s.tobytes() for s in states}
        new = rows - seen
        assert len(new) == LEVELS[depth - 1]  # the whole level: every state first seen at this depth, none missed
        seen |= rows


def test_library_pruning_generates_the_retained_sequences(prefix):
    """With all-zero tables h is 0: threshold T generates every retained sequence of length 1 .. T + 1.  Through depth 5, for
    the automatic prefix depth and two forced ones (the counts do not depend on how the work is cut)."""
    from deepcubea_amd import _lib
    root = cube3_suffix_root(0, 9)
    patterns = ((c3.CORNERS, (0,)),)
    tables = [np.zeros(24, np.uint8)]
    want = [sum(RETAINED[:t + 1]) for t in range(5)]
    for depth in (-1, 0, 2, 6):
        prefix(depth)
        res = host_cube3(root, patterns, tables, max_nodes=sum(want))
        assert res["status"] == "budget exhausted" and not res["solved"] and res["moves"] == []
        assert res["thresholds"] == [0, 1, 2, 3, 4] and res["nodes_per_threshold"] == want, (depth, res)
        assert res["nodes_generated"] == sum(want)
    assert _lib.IDASTAR_MAX_PREFIX == {_lib.ENV_NPUZZLE: 15, _lib.ENV_CUBE3: 6}


# ------------------------------------------------------------------------------------------------ exact lengths
@pytest.mark.parametrize("distance", [0, 1, 2, 3, 10, 20, 30, 31])
def test_puzzle8_length_is_the_breadth_first_distance(distance):
    for root in p8_states_at(distance, 3 if distance not in (0, 31) else 2):
        res = host_puzzle(3, root, P8_PARTITION, p8_tables())
        assert res["solved"] and res["status"] == "solved" and len(res["moves"]) == distance == res["path_cost"], (root, res)
        assert np.array_equal(replay_puzzle(3, root, res["moves"]), puzzle_goal(3))
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"]) and len(res["thresholds"]) == len(res["nodes_per_threshold"])
        assert res["thresholds"] == sorted(set(res["thresholds"])) and (not res["thresholds"] or res["thresholds"][-1] == distance)


@pytest.mark.parametrize("depth", [0, 1, 3, 11])
def test_puzzle8_lengths_do_not_depend_on_the_prefix_depth(prefix, depth):
    """Roots nearer than the prefix is long, and far ones, under forced prefix depths."""
    prefix(depth)
    for distance in (0, 1, 2, 5, 11, 12, 25):
        root = p8_states_at(distance, 1, seed=3)[0]
        res = host_puzzle(3, root, P8_PARTITION, p8_tables())
        assert res["solved"] and len(res["moves"]) == distance
        assert np.array_equal(replay_puzzle(3, root, res["moves"]), puzzle_goal(3))


def test_cube3_lengths_on_a_shipped_path_with_the_goal_test_apart_from_h(prefix):
    """c4..c7 alone is 0 on many unsolved states: the goal is every cubie at home.  Suffix roots of a shipped optimal path."""
    table = c3.host_table(*C3_SMALL)
    for depth in (-1, 6):
        prefix(depth)
        for k in range(0, 7):
            root = cube3_suffix_root(1, k)
            res = host_cube3(root, (C3_SMALL,), [table])
            assert res["solved"] and len(res["moves"]) == k, (k, res)
            assert np.array_equal(replay_cube3(root, res["moves"]), np.arange(54))


# ------------------------------------------------------------------------------------------------ node counts
@pytest.mark.parametrize("case", range(3))
def test_puzzle8_thresholds_and_counts_equal_a_recursive_search(prefix, case):
    root, distance, thresholds, counts = p8_count_cases()[case]
    for depth in (-1, 4):
        prefix(depth)
        res = host_puzzle(3, root, P8_PARTITION, p8_tables())
        n = len(thresholds)
        assert res["solved"] and len(res["moves"]) == distance
        assert res["thresholds"] == thresholds + [distance] and res["nodes_per_threshold"][:n] == counts, (res, thresholds, counts)


def test_cube3_thresholds_and_counts_equal_a_recursive_search(prefix):
    root, table, thresholds, counts = c3_count_case()
    for depth in (-1, 3):
        prefix(depth)
        res = host_cube3(root, (C3_SMALL,), [table])
        n = len(thresholds)
        assert res["solved"] and len(res["moves"]) == 7 and np.array_equal(replay_cube3(root, res["moves"]), np.arange(54))
        assert res["thresholds"] == thresholds + [7] and res["nodes_per_threshold"][:n] == counts, (res, thresholds, counts)


def test_budget_and_unsolvable_statuses():
    root = p8_states_at(30, 1)[0]
    res = host_puzzle(3, root, P8_PARTITION, p8_tables(), max_nodes=50)
    assert res["status"] == "budget exhausted" and not res["solved"] and res["path_cost"] == float("inf")
    assert 50 <= res["nodes_generated"] <= 50 + 512  # one lane in flight: one poll interval
    dead = [t.copy() for t in p8_tables()]
    for t in dead:
        t[t < 0xFE] = 0xFE
    res = host_puzzle(3, root, P8_PARTITION, dead)
    assert res["status"] == "unsolvable" and res["thresholds"] == [] and res["nodes_generated"] == 0


# ------------------------------------------------------------------------------------------------ refusals, ABI, CLI
def _raw_host(env, dim, root, np_, kinds, ids, ks, tables, max_nodes, null=()):
    from deepcubea_amd import _lib
    L = _lib.lib()
    out = {"status": C.c_int(7), "length": C.c_int(0), "moves": (C.c_uint8 * 256)(), "count": C.c_int(0),
           "thresholds": (C.c_int * 256)(), "per": (C.c_int64 * 256)(), "total": C.c_int64(0)}
    keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in tables]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[t.ctypes.data for t in keep])
    arg = {"root": np.ascontiguousarray(root, dtype=np.uint8), "kinds": np.ascontiguousarray(kinds, dtype=np.int32),
           "ids": np.ascontiguousarray(ids, dtype=np.uint8), "ks": np.ascontiguousarray(ks, dtype=np.int32)}

    def p(name):
        if name in null:
            return None
        if name in arg:
            return arg[name].ctypes.data_as(C.c_void_p)
        return ptrs if name == "tables" else C.byref(out[name]) if name in ("status", "length", "count", "total") else out[name]
    rc = L.dca_idastar_host(env, dim, p("root"), np_, p("kinds"), p("ids"), p("ks"), p("tables"), max_nodes, p("status"), p("length"),
                            p("moves"), 256, p("count"), p("thresholds"), p("per"), 256, p("total"))
    return rc, L.dca_last_error().decode(), out


def test_refusals_need_no_device():
    from deepcubea_amd import _lib
    tables = p8_tables()
    ids, ks = [1, 2, 3, 4, 5, 6, 7, 8], [4, 4]
    good = p8_states_at(10, 1)[0]
    ok = lambda **kw: _raw_host(**{**dict(env=_lib.ENV_NPUZZLE, dim=3, root=good, np_=2, kinds=[0, 0], ids=ids, ks=ks, tables=tables,
                                          max_nodes=1000000), **kw})
    rc, _, out = ok()
    assert rc == 0 and out["status"].value == 0 and out["length"].value == 10
    for dim in (6, 7):  # no instantiation: out of anybody's reach
        rc, msg, _ = ok(dim=dim, root=np.arange(dim * dim))
        assert rc == -1 and "dim" in msg and "3..5" in msg and "dca_idastar_host" in msg, msg
    for dim in (2, 8, 0, -1):
        rc, msg, _ = ok(dim=dim)
        assert rc == -1 and "dim" in msg, msg
    swapped = good.copy()
    a, b = [i for i in range(9) if swapped[i] != 0][:2]
    swapped[a], swapped[b] = swapped[b], swapped[a]
    rc, msg, _ = ok(root=swapped)
    assert rc == -1 and "parity" in msg, msg
    twice = good.copy()
    twice[a] = twice[b]
    rc, msg, _ = ok(root=twice)
    assert rc == -1 and "appears twice" in msg, msg
    big = good.copy()
    big[a] = 9
    rc, msg, _ = ok(root=big)
    assert rc == -1 and "is not a tile" in msg, msg
    for name in ("root", "ids", "ks", "tables", "status", "length", "count", "total", "moves", "thresholds", "per"):
        rc, msg, _ = ok(null=(name,))
        assert rc == -1 and "NULL" in msg, (name, msg)
    for n in (0, -1, -(1 << 40)):
        rc, msg, _ = ok(max_nodes=n)
        assert rc == -1 and "max_nodes" in msg, msg
    for n in (0, 9, -3):
        rc, msg, _ = ok(np_=n)
        assert rc == -1 and "num_patterns" in msg, msg
    rc, msg, _ = ok(ids=[1, 2, 3, 4, 4, 6, 7, 8])
    assert rc == -1 and "appears twice" in msg, msg
    rc, msg, _ = ok(env=_lib.ENV_LIGHTSOUT)
    assert rc == -1 and "env" in msg, msg
    # cube3: NULLs, a root that is no permutation of the ids, a bad cubie, a bad kind
    table = c3.host_table(*C3_SMALL)
    cube = lambda **kw: _raw_host(**{**dict(env=_lib.ENV_CUBE3, dim=0, root=cube3_suffix_root(0, 2), np_=1, kinds=[0], ids=[4, 5, 6, 7],
                                            ks=[4], tables=[table], max_nodes=100000), **kw})
    rc, _, out = cube()
    assert rc == 0 and out["status"].value == 0 and out["length"].value == 2
    for name in ("root", "kinds", "ids", "ks", "tables", "status", "total"):
        rc, msg, _ = cube(null=(name,))
        assert rc == -1 and "NULL" in msg, (name, msg)
    bad = np.arange(54)
    bad[3] = 4
    rc, msg, _ = cube(root=bad)
    assert rc == -1 and "once each" in msg, msg
    assert cube(ids=[4, 5, 6, 8])[0] == -1 and cube(kinds=[2])[0] == -1 and cube(max_nodes=0)[0] == -1 and cube(np_=25)[0] == -1
    # the prefix hook
    assert _lib.lib().dca_idastar_set_prefix(16) == -1 and _lib.lib().dca_idastar_set_prefix(-2) == -1
    assert _lib.lib().dca_idastar_set_prefix(-1) == 0
    # the Python wrappers refuse a short table and a root of the wrong width themselves
    with pytest.raises(ValueError):
        host_puzzle(3, good, P8_PARTITION, [tables[0], tables[1][:-1]])
    with pytest.raises(ValueError):
        host_puzzle(3, good[:8], P8_PARTITION, tables)
    with pytest.raises(_lib.DcaError, match="parity"):
        host_puzzle(3, swapped, P8_PARTITION, tables)


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    dbg = open(os.path.join(ROOT, "include", "dca_debug.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        where = hdr if name in ("dca_idastar_npuzzle", "dca_idastar_cube3") else dbg
        assert re.search(r"\bint %s\(" % name, where) and name in _lib.ABI_SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint %s\((.*?)\);" % name, where, re.S).group(1)
        params = [a.split() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        letters = "".join("p" if "*" in " ".join(a) else {"int": "i", "int64_t": "l"}[a[0]] for a in params)
        assert _lib._SIGNATURES[name] == "i " + letters, (name, letters)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    consts = dict(re.findall(r"#define (DCA_IDASTAR_[A-Z_]+) (.+)", hdr))
    assert (int(consts["DCA_IDASTAR_SOLVED"]), int(consts["DCA_IDASTAR_BUDGET"]), int(consts["DCA_IDASTAR_UNSOLVABLE"])) == \
        (_lib.IDASTAR_SOLVED, _lib.IDASTAR_BUDGET, _lib.IDASTAR_UNSOLVABLE) == (0, 1, 2)
    assert int(consts["DCA_IDASTAR_POLL_NODES"]) == _lib.IDASTAR_POLL_NODES <= 4096
    assert eval(consts["DCA_IDASTAR_MAX_LANES"]) == _lib.IDASTAR_MAX_LANES and int(consts["DCA_IDASTAR_MAX_MOVES"]) == 254
    assert _lib.IDASTAR_OVERSHOOT == _lib.IDASTAR_MAX_LANES * _lib.IDASTAR_POLL_NODES
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for phrase in ("a == m ^ 1", "a == m == m_prev", "face(a) == face(m) ^ 1 with face(a) < face(m)", "every cubie at home",
                   "DCA_IDASTAR_MAX_LANES * DCA_IDASTAR_POLL_NODES", "the wrong parity"):
        assert phrase in flat, phrase


def test_cli_refusals_touch_no_device(monkeypatch, tmp_path):
    import torch
    from deepcubea_amd.search_methods import idastar

    def touched(*a, **k):
        raise AssertionError("torch.cuda touched before the refusal")
    for name in ("is_available", "device_count", "current_device", "init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    p = idastar.build_parser()
    args = p.parse_args(["--states", "s.pkl", "--env", "puzzle15", "--model_dir", "pdb:5-5-5", "--results_dir", "r"])
    assert args.max_nodes is None and args.start_idx == 0 and not args.verbose
    assert idastar.default_max_nodes("puzzle15") == idastar.DEFAULT_MAX_NODES["puzzle"] == int(60 * idastar.MEASURED_NODES_PER_SECOND["puzzle"])
    assert idastar.default_max_nodes("cube3") == idastar.DEFAULT_MAX_NODES["cube3"] == int(60 * idastar.MEASURED_NODES_PER_SECOND["cube3"])
    for model in ("synthetic:0", "builtin:manhattan", "exact:gf2", "saved_models/puzzle15", "pdb:7-7-7", "pdb:"):
        with pytest.raises(ValueError):
            idastar.pattern_database(SimpleNamespace(env="puzzle15", model_dir=model))
    for env in ("puzzle35", "puzzle48", "lightsout7", "cube4", "nosuch"):
        with pytest.raises(ValueError):
            idastar.pattern_database(SimpleNamespace(env=env, model_dir="pdb:auto"))
    with pytest.raises(ValueError):
        idastar.pattern_database(SimpleNamespace(env="cube3", model_dir="pdb:5-5-5"))
    assert idastar.pattern_database(SimpleNamespace(env="puzzle24", model_dir="pdb:6-6-6-6")).spec.count("/") == 3
    assert idastar.pattern_database(SimpleNamespace(env="cube3", model_dir="pdb:korf")).spec.startswith("c0,")
    with pytest.raises(ValueError):  # main() refuses before it reads the states file or makes the results directory
        idastar.main(["--states", str(tmp_path / "none.pkl"), "--env", "puzzle35", "--model_dir", "pdb:1,2,3", "--results_dir",
                      str(tmp_path / "out")])
    with pytest.raises(ValueError):
        idastar.main(["--states", str(tmp_path / "none.pkl"), "--env", "puzzle15", "--model_dir", "builtin:manhattan", "--results_dir",
                      str(tmp_path / "out")])
    with pytest.raises(ValueError):
        idastar.main(["--states", str(tmp_path / "none.pkl"), "--env", "puzzle15", "--model_dir", "pdb:5-5-5", "--max_nodes", "0",
                      "--results_dir", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists() and "deepcubea_amd.search_methods.idastar" in sys.modules
    with pytest.raises(ValueError):  # a class for an environment the kernel is not built for
        idastar.IDAStar("puzzle35", SimpleNamespace())
