"""Reflected look-ups for the sliding-puzzle pattern databases, host side (no device needed): the mirror maps, the reflected
eval through dca_pdb_eval_host (the kernels' own row value in a plain loop) on the whole puzzle8 space and on rows of any bytes,
the reflected IDA* through dca_idastar_host_reflected (the kernel's move, index-update and work-item code) against breadth-first
distances and a recursive search written here, every new refusal, the `+reflect` spec suffix and the ABI additions.

This file also holds what the GPU tests (tests/test_pdb_reflect_hip.py) compare against: the definition of include/dca.h
restated in numpy, and a recursive IDA* that takes any h."""
import ctypes as C
import os
import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_idastar_cpu as ida
from tests import test_pdb_cpu as pz
from tests import test_puzzle8_cpu as p8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"dca_pdb_eval_reflected": "dca.h", "dca_idastar_npuzzle_reflected": "dca.h",
               "dca_idastar_host_reflected": "dca_debug.h", "dca_pdb_eval_host": "dca_debug.h"}
P8_PARTITION = ida.P8_PARTITION
P8_SELF_MIRRORED = ((1, 5, 2, 4), (3, 7, 6, 8))  # phi maps each pattern's tiles onto themselves
P15_THREES = ((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
P24_THREES = ((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
COUNT_DISTANCES = (20, 26, 30)
PLAIN_TOTALS = [49, 81, 141, 483, 569, 251]      # nodes below the final threshold on p8_states_at(d, 2), d = 20, 26, 30
REFLECTED_TOTALS = [26, 54, 44, 174, 305, 170]
BIG = ida.BIG


# ------------------------------------------------------------------------------------------------ the definition, restated
def refl(dim, p):
    return (p % dim) * dim + p // dim


def phi(dim, t):
    return 0 if t == 0 else refl(dim, t - 1) + 1


def mirror_rows(dim, rows):
    """The mirror image of states in the main diagonal: position refl(p) holds phi(row[p])."""
    rows = np.asarray(rows)
    N = dim * dim
    out = np.empty_like(rows)
    tile_map = np.array([phi(dim, t) for t in range(N)], rows.dtype)
    out[:, [refl(dim, p) for p in range(N)]] = tile_map[rows]
    return out


def reflected_sum(dim, rows, partition, tables):
    """sum_p table_p[reflected index_p] by the header's digit rule, for ANY row bytes."""
    N = dim * dim
    refl_of = np.array([refl(dim, p) for p in range(N)], np.int64)
    blank = refl_of[pz.host_positions(dim, rows, 0)]
    total = np.zeros(len(rows), np.int64)
    for tiles, table in zip(partition, tables):
        idx = np.zeros(len(rows), np.int64)
        for t in reversed(tiles):
            idx = idx * N + refl_of[pz.host_positions(dim, rows, phi(dim, t))]
        idx = idx * N + blank
        assert idx.max(initial=0) < len(table)
        total += np.asarray(table)[idx]
    return total


def host_eval_reflected(dim, rows, partition, tables):
    """dca_pdb_eval_reflected on the host: max(plain sum, reflected sum) -> float32."""
    plain = pz.host_eval(dim, rows, partition, tables).astype(np.int64)
    return np.maximum(plain, reflected_sum(dim, rows, partition, tables)).astype(np.float32)


def swap_table(dim):
    """blank position, move -> the blank's new position (U D L R; a move off the board is a no-op), as include/dca.h numbers them."""
    out = []
    for z in range(dim * dim):
        i, j = divmod(z, dim)
        out.append([z + dim if i < dim - 1 else z, z - dim if i > 0 else z, z + 1 if j < dim - 1 else z, z - 1 if j > 0 else z])
    return out


def state_h(dim, partition, tables, reflect):
    """h of one state (a tuple of tiles) by the header's index rule: the plain sum, or the larger of it and the reflected sum.
    A table is anything that gives its byte at an integer index: an array, or an object that reads a table kept elsewhere."""
    N = dim * dim

    def h(state):
        pos = [0] * N
        for p, t in enumerate(state):
            pos[t] = p
        plain = mirrored = 0
        for tiles, table in zip(partition, tables):
            idx = ridx = 0
            for t in reversed(tiles):
                idx = idx * N + pos[t]
                ridx = ridx * N + refl(dim, pos[phi(dim, t)])
            plain += int(table[idx * N + pos[0]])
            mirrored += int(table[ridx * N + refl(dim, pos[0])])
        return max(plain, mirrored) if reflect else plain
    return h


def reference_idastar(dim, root, h, stop_at):
    """A plain recursive IDA* under the header's counting rules (a child counts when generated; no no-op, no undo) with any h:
    the thresholds below `stop_at` (the known distance) -> (thresholds, node counts)."""
    nb = swap_table(dim)

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


def host_puzzle(dim, root, partition, tables, reflect=True, max_nodes=BIG):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_NPUZZLE, dim, root, partition, tables, max_nodes, reflect=reflect)


@lru_cache(maxsize=None)
def p8_count_roots():
    return [root for d in COUNT_DISTANCES for root in ida.p8_states_at(d, 2)]


@lru_cache(maxsize=None)
def p8_count_cases():
    """The six count roots with their distance and the recursive search's thresholds and counts, plain and reflected; once."""
    tables = ida.p8_tables()
    cases = []
    for i, root in enumerate(p8_count_roots()):
        d = COUNT_DISTANCES[i // 2]
        plain = reference_idastar(3, root, state_h(3, P8_PARTITION, tables, False), d)
        mirrored = reference_idastar(3, root, state_h(3, P8_PARTITION, tables, True), d)
        cases.append((root, d, plain, mirrored))
    return cases


def suffix_root(golden, env, dim, instance, k):
    """The state k moves from the goal on a shipped optimal path (a suffix of an optimal path is optimal)."""
    n = int(golden["%s_test_opt_len" % env][instance])
    assert n >= k
    return ida.replay_puzzle(dim, golden["%s_test_states" % env][instance], golden["%s_test_opt_moves" % env][instance][:n - k])


@lru_cache(maxsize=None)
def small_case(env):
    """puzzle15 / puzzle24 with four 3-tile groups and host tables: a root 24 / 16 moves from the goal on shipped path 0, and the
    recursive search's thresholds and counts with h = the reflected value."""
    dim, partition, k = {"puzzle15": (4, P15_THREES, 24), "puzzle24": (5, P24_THREES, 16)}[env]
    golden = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    tables = [pz.host_table(dim, g) for g in partition]
    root = suffix_root(golden, env, dim, 0, k)
    thresholds, counts = reference_idastar(dim, root, state_h(dim, partition, tables, True), k)
    return dim, partition, tables, root, k, thresholds, counts


def random_rows_case(dim, seed):
    """Rows of random bytes 0..255 and random (not distance) tables of two 2-tile patterns: the any-bytes rule's test data."""
    N = dim * dim
    rng = np.random.default_rng(seed)
    partition = ((2, N - 1), (N - 2, 1))
    tables = [rng.integers(0, 256, N ** 3, dtype=np.uint8) for _ in partition]
    rows = rng.integers(0, 256, (4099, N), dtype=np.uint8)
    rows[:64] = rng.integers(0, N, (64, N), dtype=np.uint8)  # some rows whose bytes are all tiles, with repeats
    return partition, tables, rows


# ------------------------------------------------------------------------------------------------ maps
def test_maps_are_involutions_and_the_goal_is_its_own_mirror_image():
    for dim in range(3, 8):
        N = dim * dim
        assert sorted(refl(dim, p) for p in range(N)) == list(range(N)) == [refl(dim, refl(dim, p)) for p in range(N)]
        assert sorted(phi(dim, t) for t in range(N)) == list(range(N)) == [phi(dim, phi(dim, t)) for t in range(N)]
        assert phi(dim, 0) == 0 and refl(dim, N - 1) == N - 1
        goal = ida.puzzle_goal(dim)[None]
        assert np.array_equal(mirror_rows(dim, goal), goal)
        rows = np.stack([np.random.default_rng(dim).permutation(N).astype(np.uint8) for _ in range(5)])
        assert np.array_equal(mirror_rows(dim, mirror_rows(dim, rows)), rows)


def test_mirroring_keeps_the_breadth_first_distance():
    states, dist, _ = p8.bfs_table()
    pick = np.random.default_rng(1).permutation(len(states))[:20000]
    assert np.array_equal(p8.distance(mirror_rows(3, states[pick])), dist[pick].astype(np.int64))
    # a blank move of a state is a blank move of its mirror image: U <-> L, D <-> R
    swap = np.array(p8.SWAP)
    for a, b in ((0, 2), (1, 3), (2, 0), (3, 1)):
        assert np.array_equal(mirror_rows(3, p8.move_np(states[pick], a, swap)), p8.move_np(mirror_rows(3, states[pick]), b, swap))


# ------------------------------------------------------------------------------------------------ eval on the whole space
def test_reflected_eval_on_the_whole_puzzle8_space():
    from deepcubea_amd import _lib
    states, dist, _ = p8.bfs_table()
    tables = ida.p8_tables()
    plain = _lib.pdb_eval_host(3, states, P8_PARTITION, tables, reflect=False)
    got = _lib.pdb_eval_host(3, states, P8_PARTITION, tables, reflect=True)
    assert plain.dtype == got.dtype == np.float32
    assert np.array_equal(plain, pz.host_eval(3, states, P8_PARTITION, tables))
    assert np.array_equal(got, host_eval_reflected(3, states, P8_PARTITION, tables))
    mirrored = reflected_sum(3, states, P8_PARTITION, tables)
    assert np.array_equal(mirrored, pz.host_eval(3, mirror_rows(3, states), P8_PARTITION, tables).astype(np.int64))  # the same thing
    assert (plain <= dist).all() and (got <= dist).all()
    assert (int((mirrored > plain).sum()), int((mirrored < plain).sum()), int((mirrored == plain).sum())) == (49304, 49304, 82832)
    assert int(plain.sum()) == 3471816 and int(got.sum()) == 3589500
    assert int((got == dist).sum()) > int((plain == dist).sum())


def test_a_self_mirrored_partition_gains_nothing():
    from deepcubea_amd import _lib
    states = p8.all_states()
    tables = [pz.host_table(3, g) for g in P8_SELF_MIRRORED]
    for g in P8_SELF_MIRRORED:
        assert sorted(phi(3, t) for t in g) == sorted(g) and tuple(phi(3, t) for t in g) != g  # as a set; the digits trade places
    assert np.array_equal(_lib.pdb_eval_host(3, states, P8_SELF_MIRRORED, tables, reflect=True),
                          _lib.pdb_eval_host(3, states, P8_SELF_MIRRORED, tables, reflect=False))


# ------------------------------------------------------------------------------------------------ any bytes
@pytest.mark.parametrize("dim", [3, 4, 5, 6, 7])
def test_any_bytes_rule_with_random_tables(dim):
    from deepcubea_amd import _lib
    N = dim * dim
    partition, tables, rows = random_rows_case(dim, 40 + dim)
    want = {False: pz.host_eval(dim, rows, partition, tables), True: host_eval_reflected(dim, rows, partition, tables)}
    assert not np.array_equal(want[False], want[True])
    for ld in (N, N + 3):
        wide = np.full((len(rows), ld), 0xA5, np.uint8)
        wide[:, :N] = rows
        for reflect in (False, True):
            for n in (0, 1, len(rows)):
                got = _lib.pdb_eval_host(dim, wide[:n], partition, tables, reflect=reflect)
                assert got.shape == (n,) and np.array_equal(got, want[reflect][:n]), (dim, ld, reflect, n)


# ------------------------------------------------------------------------------------------------ host IDA*: lengths
@pytest.mark.parametrize("distance", [0, 1, 2, 3, 10, 20, 30, 31])
def test_puzzle8_reflected_length_is_the_breadth_first_distance(distance):
    for root in ida.p8_states_at(distance, 3 if distance not in (0, 31) else 2):
        res = host_puzzle(3, root, P8_PARTITION, ida.p8_tables())
        assert res["solved"] and res["status"] == "solved" and len(res["moves"]) == distance == res["path_cost"], (root, res)
        assert np.array_equal(ida.replay_puzzle(3, root, res["moves"]), ida.puzzle_goal(3))
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"])
        assert res["thresholds"] == sorted(set(res["thresholds"])) and (not res["thresholds"] or res["thresholds"][-1] == distance)


@pytest.mark.parametrize("depth", [0, 1, 3, 11])
def test_puzzle8_reflected_lengths_do_not_depend_on_the_prefix_depth(depth):
    from deepcubea_amd import _lib
    _lib.idastar_set_prefix(depth)
    try:
        for distance in (0, 1, 2, 5, 11, 12, 25):
            root = ida.p8_states_at(distance, 1, seed=3)[0]
            res = host_puzzle(3, root, P8_PARTITION, ida.p8_tables())
            assert res["solved"] and len(res["moves"]) == distance
            assert np.array_equal(ida.replay_puzzle(3, root, res["moves"]), ida.puzzle_goal(3))
    finally:
        _lib.idastar_set_prefix(-1)


# ------------------------------------------------------------------------------------------------ host IDA*: counts
def test_puzzle8_reflected_counts_equal_a_recursive_search_and_never_exceed_the_plain_ones():
    plain_totals, reflected_totals = [], []
    for root, d, (pt, pc), (rt, rc) in p8_count_cases():
        assert ida.reference_idastar_puzzle(3, root, P8_PARTITION, ida.p8_tables(), d) == (pt, pc)  # the two references agree
        for reflect, thresholds, counts in ((False, pt, pc), (True, rt, rc)):
            res = host_puzzle(3, root, P8_PARTITION, ida.p8_tables(), reflect=reflect)
            assert res["solved"] and len(res["moves"]) == d
            assert res["thresholds"] == thresholds + [d] and res["nodes_per_threshold"][:len(counts)] == counts, (reflect, res, counts)
        plain_at = dict(zip(pt, pc))
        for T, count in zip(rt, rc):
            assert T not in plain_at or count <= plain_at[T], (root, T, count, plain_at)
        plain_totals.append(sum(pc))
        reflected_totals.append(sum(rc))
    assert plain_totals == PLAIN_TOTALS and reflected_totals == REFLECTED_TOTALS


@pytest.mark.parametrize("env", ["puzzle15", "puzzle24"])
def test_four_patterns_on_the_wider_boards(env):
    """Eight live indices; puzzle15 packs the board 4 bits a position in 64 bits, puzzle24 5 bits in 128."""
    from deepcubea_amd import _lib
    dim, partition, tables, root, k, thresholds, counts = small_case(env)
    assert sum(counts) < 300000
    for depth in (-1, 6):
        _lib.idastar_set_prefix(depth)
        try:
            res = host_puzzle(dim, root, partition, tables)
        finally:
            _lib.idastar_set_prefix(-1)
        assert res["solved"] and len(res["moves"]) == k
        assert np.array_equal(ida.replay_puzzle(dim, root, res["moves"]), ida.puzzle_goal(dim))
        assert res["thresholds"] == thresholds + [k] and res["nodes_per_threshold"][:len(counts)] == counts, (res, thresholds, counts)


def test_a_dead_reflected_root_byte_is_unsolvable():
    """The root is dead if ANY of the 2 np root bytes is 0xFE or above: here only the mirror image's index holds one."""
    from deepcubea_amd import _lib
    root = ida.p8_states_at(12, 1)[0]
    tables = [t.copy() for t in ida.p8_tables()]
    N, pos = 9, {int(t): p for p, t in enumerate(root)}
    idx = ridx = 0
    for t in reversed(P8_PARTITION[0]):
        idx = idx * N + pos[t]
        ridx = ridx * N + refl(3, pos[phi(3, t)])
    idx, ridx = idx * N + pos[0], ridx * N + refl(3, pos[0])
    assert idx != ridx
    tables[0][ridx] = 0xFE
    assert host_puzzle(3, root, P8_PARTITION, tables, reflect=False)["solved"]
    res = host_puzzle(3, root, P8_PARTITION, tables, reflect=True)
    assert res["status"] == "unsolvable" and res["thresholds"] == [] and res["nodes_generated"] == 0
    assert _lib.pdb_eval_host(3, root[None], P8_PARTITION, tables, reflect=True)[0] >= 0xFE


# ------------------------------------------------------------------------------------------------ refusals, spec, ABI
def _raw_reflected(dim, root, np_, ids, ks, tables, max_nodes=1000000, null=()):
    from deepcubea_amd import _lib
    L = _lib.lib()
    out = {"status": C.c_int(7), "length": C.c_int(0), "moves": (C.c_uint8 * 256)(), "count": C.c_int(0),
           "thresholds": (C.c_int * 256)(), "per": (C.c_int64 * 256)(), "total": C.c_int64(0)}
    keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in tables]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[t.ctypes.data for t in keep])
    arg = {"root": np.ascontiguousarray(root, dtype=np.uint8), "ids": np.ascontiguousarray(ids, dtype=np.uint8),
           "ks": np.ascontiguousarray(ks, dtype=np.int32)}

    def p(name):
        if name in null:
            return None
        if name in arg:
            return arg[name].ctypes.data_as(C.c_void_p)
        return ptrs if name == "tables" else C.byref(out[name]) if name in ("status", "length", "count", "total") else out[name]
    rc = L.dca_idastar_host_reflected(dim, p("root"), np_, p("ids"), p("ks"), p("tables"), max_nodes, p("status"), p("length"), p("moves"),
                                      256, p("count"), p("thresholds"), p("per"), 256, p("total"))
    return rc, L.dca_last_error().decode(), out


def test_refusals_need_no_device():
    from deepcubea_amd import _lib
    L = _lib.lib()
    tables = ida.p8_tables()
    good = ida.p8_states_at(10, 1)[0]
    ok = lambda **kw: _raw_reflected(**{**dict(dim=3, root=good, np_=2, ids=[1, 2, 3, 4, 5, 6, 7, 8], ks=[4, 4], tables=tables), **kw})
    rc, _, out = ok()
    assert rc == 0 and out["status"].value == 0 and out["length"].value == 10
    # five patterns: the plain search takes them, the reflected one says why it does not
    ones, one_tables = [[t] for t in range(1, 6)], [pz.host_table(3, (t,)) for t in range(1, 6)]
    rc, msg, _ = ok(np_=5, ids=[1, 2, 3, 4, 5], ks=[1] * 5, tables=one_tables)
    assert rc == -1 and "dca_idastar_host_reflected" in msg and "num_patterns = 5" in msg and "1..4" in msg and "reflected" in msg, msg
    assert _lib.idastar_host(_lib.ENV_NPUZZLE, 3, good, ones, one_tables, BIG)["solved"]
    with pytest.raises(_lib.DcaError, match="num_patterns = 5"):
        host_puzzle(3, good, ones, one_tables)
    assert host_puzzle(3, good, ones[:4], one_tables[:4])["solved"]  # four are fine
    for n in (0, -1, 9):
        rc, msg, _ = ok(np_=n)
        assert rc == -1 and "num_patterns" in msg, msg
    for name in ("root", "ids", "ks", "tables", "status", "length", "count", "total", "moves", "thresholds", "per"):
        rc, msg, _ = ok(null=(name,))
        assert rc == -1 and "NULL" in msg, (name, msg)
    swapped = good.copy()
    a, b = [i for i in range(9) if swapped[i] != 0][:2]
    swapped[a], swapped[b] = swapped[b], swapped[a]
    rc, msg, _ = ok(root=swapped)
    assert rc == -1 and "parity" in msg, msg
    for dim in (2, 6, 7, 8):
        rc, msg, _ = ok(dim=dim, root=np.arange(max(dim, 3) ** 2))
        assert rc == -1 and "dim" in msg, msg
    assert ok(max_nodes=0)[0] == -1 and ok(ids=[1, 2, 3, 4, 4, 6, 7, 8])[0] == -1
    # cube3 has no reflected search
    with pytest.raises(ValueError, match="sliding puzzles"):
        _lib.idastar_host(_lib.ENV_CUBE3, 0, np.arange(54), ((0, (0,)),), [np.zeros(24, np.uint8)], 1000, reflect=True)
    # dca_pdb_eval_host: the refusals of dca_pdb_eval
    rows = np.ascontiguousarray(p8.all_states()[:8])
    out = np.zeros(8, np.float32)
    ids, ks = np.arange(1, 9, dtype=np.uint8), np.array([4, 4], np.int32)
    ptrs = (C.c_void_p * 2)(*[t.ctypes.data for t in tables])
    v = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def evaluate(dim=3, states=rows, n=8, ld=9, np_=2, ids=ids, ks=ks, tables=ptrs, reflect=1, out=out):
        return L.dca_pdb_eval_host(dim, v(states), n, ld, np_, v(ids), v(ks), tables, reflect, v(out))
    assert evaluate() == 0 and np.array_equal(out, host_eval_reflected(3, rows, P8_PARTITION, tables))
    twice = np.array([1, 2, 3, 4, 4, 6, 7, 8], np.uint8)
    for call, word in ((lambda: evaluate(dim=2), "dim"), (lambda: evaluate(dim=8), "dim"), (lambda: evaluate(ld=8), "ld"),
                       (lambda: evaluate(n=-1), "n >= 0"), (lambda: evaluate(np_=0), "num_patterns"), (lambda: evaluate(np_=25), "num_patterns"),
                       (lambda: evaluate(ids=None), "tiles"), (lambda: evaluate(ks=None), "ks"), (lambda: evaluate(tables=None), "tables"),
                       (lambda: evaluate(states=None), "states"), (lambda: evaluate(out=None), "out"),
                       (lambda: evaluate(ids=twice), "tile 4 appears twice"),
                       (lambda: evaluate(tables=(C.c_void_p * 2)(tables[0].ctypes.data, None)), "table 1 is NULL")):
        assert call() == -1, word
        msg = L.dca_last_error().decode()
        assert msg.startswith("bad argument: dca_pdb_eval_host") and word in msg, (word, msg)
    assert evaluate(n=0, states=None, out=None) == 0
    with pytest.raises(ValueError):  # the wrapper refuses a short table and a device-less wrong dtype itself
        _lib.pdb_eval_host(3, rows, P8_PARTITION, [tables[0], tables[1][:-1]])
    with pytest.raises(ValueError):
        _lib.pdb_eval_host(3, rows.astype(np.int32), P8_PARTITION, tables)


def test_spec_suffix():
    from deepcubea_amd.utils import pattern_db as pd
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    assert pd.split_reflect("5-5-5") == ("5-5-5", False) and pd.split_reflect("5-5-5+reflect") == ("5-5-5", True)
    assert pd.split_reflect(" auto +Reflect ") == ("auto", True)
    for env, spec, partition in (("puzzle15", "5-5-5+reflect", pd.PRESETS["puzzle15"]["5-5-5"]), ("puzzle24", "auto+reflect", pd.PRESETS["puzzle24"]["6-6-6-6"]),
                                 ("puzzle8", "1,2,3/4,5,6+reflect", ((1, 2, 3), (4, 5, 6)))):
        pdb = pd.PatternDatabase(env, spec)
        assert pdb.reflect and pdb.partition == partition and pdb.spec.endswith("+reflect")
        assert pd.PatternDatabase(env, pdb.spec).partition == partition and pd.PatternDatabase(env, pdb.spec).reflect
        plain = pd.PatternDatabase(env, spec[:-len("+reflect")])
        assert not plain.reflect and plain.spec + "+reflect" == pdb.spec and plain.bytes == pdb.bytes
    assert pd.PatternDatabase("puzzle8", P8_PARTITION, reflect=True).spec == "1,2,3,4/5,6,7,8+reflect"
    assert pd.PatternDatabase("puzzle8", "4-4", reflect=True).reflect and not pd.PatternDatabase("puzzle8", P8_PARTITION).reflect
    for spec in ("4-4+reflect+reflect", "4-4+mirror", "4-4+", "+reflect", "reflect", "4-4 reflect", "1,2+reflect/3,4"):
        with pytest.raises(ValueError):
            pd.PatternDatabase("puzzle8", spec)
    for spec in ("korf+reflect", "corners+reflect", "c0,c1+reflect"):
        with pytest.raises(ValueError, match="sliding puzzles"):
            Cube3PatternDatabase(spec)
    # parse_pdb_spec itself is what it was: every preset parses as before, and it takes no suffix
    for env, presets in pd.PRESETS.items():
        for name, partition in presets.items():
            assert pd.parse_pdb_spec(env, name) == partition
            with pytest.raises(ValueError):
                pd.parse_pdb_spec(env, name + "+reflect")
        assert pd.parse_pdb_spec(env, "auto") == presets[pd.AUTO[env]]


def test_save_load_round_trip_of_the_suffix(tmp_path):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    partition = ((1, 2, 3), (8, 5))
    tables = [pz.host_table(3, g) for g in partition]
    path, old = str(tmp_path / "p8r.npz"), str(tmp_path / "p8.npz")
    PatternDatabase("puzzle8", partition, reflect=True).save(path, tables=tables)
    with np.load(path) as z:
        assert sorted(z.files) == ["env_name", "partition", "table_0", "table_1"] and str(z["partition"]) == "1,2,3/8,5+reflect"
    back, got = PatternDatabase.load_host(path)
    assert back.reflect and back.partition == partition and back.spec == "1,2,3/8,5+reflect"
    assert all(np.array_equal(g, t) for g, t in zip(got, tables))
    with open(old, "wb") as f:  # a file as written before the suffix existed
        np.savez(f, env_name=np.array("puzzle8"), partition=np.array("1,2,3/8,5"), table_0=tables[0], table_1=tables[1])
    back, got = PatternDatabase.load_host(old)
    assert not back.reflect and back.partition == partition and back.spec == "1,2,3/8,5"
    assert all(np.array_equal(g, t) for g, t in zip(got, tables))


def test_cli_refusals_touch_no_device(monkeypatch):
    import torch
    from deepcubea_amd.search_methods import astar, idastar

    def touched(*a, **k):
        raise AssertionError("torch.cuda touched before the refusal")
    for name in ("is_available", "device_count", "current_device", "init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    for env, model in (("cube3", "pdb:korf+reflect"), ("puzzle15", "pdb:5-5-5+mirror"), ("puzzle15", "pdb:5-5-5+reflect+reflect"),
                       ("puzzle8", "pdb:5-5-5+reflect")):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env=env), None)
        with pytest.raises(ValueError):
            idastar.pattern_database(SimpleNamespace(model_dir=model, env=env))
    assert astar._pattern_database(SimpleNamespace(model_dir="pdb:6-6-3+reflect", env="puzzle15")).reflect
    assert astar.auto_instances(SimpleNamespace(instances_per_gpu="auto", model_dir="pdb:5-5-5+reflect", batch_size=100, env="puzzle15",
                                                max_nodes="auto"), SimpleNamespace(get_num_moves=lambda: 4), 500, None) == 1
    for env, spec in (("puzzle15", "5-5-5"), ("puzzle15", "6-6-3"), ("puzzle24", "6-6-6-6"), ("puzzle8", "auto")):
        pdb = idastar.pattern_database(SimpleNamespace(model_dir="pdb:%s+reflect" % spec, env=env))
        assert pdb.reflect and len(pdb.partition) <= 4
    five = "1/2/3/4/5"
    assert len(idastar.pattern_database(SimpleNamespace(model_dir="pdb:" + five, env="puzzle8")).partition) == 5
    with pytest.raises(ValueError, match="at most 4 patterns"):
        idastar.pattern_database(SimpleNamespace(model_dir="pdb:%s+reflect" % five, env="puzzle8"))
    assert astar._pattern_database(SimpleNamespace(model_dir="pdb:%s+reflect" % five, env="puzzle8")).reflect  # the eval has no such limit
    help_text = " ".join({a.dest: a for a in astar.build_parser()._actions}["model_dir"].help.split())
    assert "SPEC+reflect" in help_text and "pdb:SPEC" in help_text and "--weight 1 --semantics cpp the solutions are optimal" in help_text
    assert "SPEC+reflect" in " ".join({a.dest: a for a in idastar.build_parser()._actions}["model_dir"].help.split())
    assert idastar.DEFAULT_MAX_NODES == {"puzzle": int(60 * 1.14e8), "cube3": int(60 * 8.52e9)}


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    L = _lib.lib()
    text = {name: open(os.path.join(ROOT, "include", name)).read() for name in ("dca.h", "dca_debug.h")}
    for name, header in NEW_SYMBOLS.items():
        other = "dca_debug.h" if header == "dca.h" else "dca.h"
        assert re.search(r"\bint %s\(" % name, text[header]) and not re.search(r"\bint %s\(" % name, text[other]), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint %s\((.*?)\);" % name, text[header], re.S).group(1)
        params = [a.split() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        letters = "".join("p" if "*" in " ".join(a) else {"int": "i", "int64_t": "l"}[a[0]] for a in params)
        assert _lib._SIGNATURES[name] == "i " + letters, (name, letters)
    assert _lib._SIGNATURES["dca_pdb_eval_reflected"] == _lib._SIGNATURES["dca_pdb_eval"]
    assert _lib._SIGNATURES["dca_idastar_npuzzle_reflected"] == _lib._SIGNATURES["dca_idastar_npuzzle"]
    assert "#define DCA_ABI_VERSION 6" in text["dca.h"] and L.dca_abi_version() == 6
    assert _lib.IDASTAR_MAX_REFLECT_PATTERNS == 4 == _lib.IDASTAR_MAX_PUZZLE_PATTERNS // 2
    flat = re.sub(r"\s*\n \*\s*", " ", text["dca.h"])
    for phrase in ("refl(p) = (p mod dim) * dim + p div dim", "phi(0) = 0, phi(t) = refl(t - 1) + 1", "REFLECTED INDEX",
                   "max(sum_p table_p[index_p], sum_p table_p[reflected index_p])", "w(phi(t)) * (refl(b) - refl(nb))",
                   "num_patterns must be in 1..4"):
        assert phrase in flat, phrase
