"""CPU-side tests of the dual look-ups for the cube3 pattern databases (`pdb:<spec>+dual`, include/dca.h "Dual look-ups"): the
inversion rule in location words against argsort, the dual value against the symmetric value at the row and at its inverse, the
facts plain <= sym <= dual <= d on the breadth-first levels, the all-corner pattern, the any-bytes rule, the host IDA* against
a recursive search written here, the spec suffix through the class, the .npz and both CLIs, the ABI.  No GPU needed.
tests/test_cube3_dual_hip.py imports the helpers."""
import ctypes as C
import os
import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_cube3_pdb_cpu as c3
from tests import test_cube3_sym_cpu as sym
from tests import test_idastar_cpu as ida
from tests.test_cube3_sym_cpu import no_device, prefix  # noqa: F401  (fixtures)

ROOT = sym.ROOT
ALL = sym.ALL
NEW_PRODUCT = ("dca_cube3_pdb_eval_dual", "dca_idastar_cube3_dual")
NEW_DEBUG = ("dca_idastar_host_dual", "dca_cube3_pdb_eval_dual_host", "dca_cube3_inverse_locs")
SMALL4 = tuple(c3.SMALL.values())
IDA_SET = sym.IDA_SET
IDA_CASES = tuple(sym.IDA_CASES)
WHOLE = (c3.CORNERS, tuple(range(8)))  # the pattern that names every cubie of its kind


# ------------------------------------------------------------------------------------------------ the rule, in Python
@lru_cache(maxsize=None)
def corner_classes():
    """Per corner slot 0 or 1: a quarter turn carries a slot's ascending positions x -> x + c onto a slot of its own class and
    x -> c - x onto one of the other (read off the location-move table, slot 0 in class 0)."""
    mv = c3.location_moves(c3.CORNERS)
    cls = {0: 0}
    while len(cls) < 8:
        for a in range(12):
            for s in list(cls):
                t0, t1 = int(mv[a][3 * s]), int(mv[a][3 * s + 1])
                assert t0 // 3 == t1 // 3
                flips = 0 if (t1 - t0) % 3 == 1 else 1
                assert cls.setdefault(t0 // 3, cls[s] ^ flips) == cls[s] ^ flips
    assert sorted(cls.values()) == [0] * 4 + [1] * 4
    return [cls[s] for s in range(8)]


def invert(kind, locs):
    """The header's inversion rule in its replacing form on the n locations of one kind (any locations < 24)."""
    n, o = c3.SLOTS[kind]
    out = [0] * 16
    for j, l in enumerate(locs):
        s, r = divmod(int(l), o)
        if kind == c3.CORNERS and r and corner_classes()[s] == corner_classes()[j]:
            r = 3 - r
        out[s] = j * o + r
    return tuple(out[:n])


def words(kind, locs):
    return sum(int(l) << (5 * q) for q, l in enumerate(locs))


def words_of_rows(rows):
    """uint64 [m, 2]: the location words of rows that are cube states, from the Python rule of test_cube3_pdb_cpu."""
    out = np.zeros((len(rows), 2), np.uint64)
    for kind in (c3.CORNERS, c3.EDGES):
        locs = c3.locations_of_states(kind, tuple(range(c3.SLOTS[kind][0])), rows)
        out[:, kind] = [words(kind, row) for row in locs]
    return out


def inverse_rows(rows):
    return np.argsort(rows, axis=1).astype(np.uint8)


@lru_cache(maxsize=None)
def rule_rows():
    """>= 200 scrambles of 1..30 moves and every 40th shipped path state, computed once."""
    rows = np.concatenate([c3.scrambles(10, m, 100 + m) for m in range(1, 31)] + [c3.path_states()[0][::40]])
    rows.setflags(write=False)
    return rows


def host_eval(rows, row_kind, patterns, n, dual, tables=None):
    from deepcubea_amd import _lib
    return _lib.cube3_pdb_eval_host(rows, row_kind, patterns, sym.tables_of(patterns) if tables is None else tables, sym=n, dual=dual)


# ------------------------------------------------------------------------------------------------ 1. the inversion rule
def test_the_inversion_rule_gives_the_words_of_argsort():
    from deepcubea_amd import _lib
    rows = rule_rows()
    assert len(rows) >= 200 + 500
    want = words_of_rows(inverse_rows(rows))
    got = _lib.cube3_inverse_locs(rows, _lib.ROWS_STATE)
    assert got.dtype == np.uint64 and (got == want).all()
    assert (_lib.cube3_inverse_locs(rows // 9, _lib.ROWS_NNET) == want).all()
    assert (got != words_of_rows(rows)).any(axis=1).sum() > 600  # (the inverse is another state nearly everywhere)
    # the Python restatement is the same rule; twice is the identity; the goal is its own inverse
    for kind in (c3.CORNERS, c3.EDGES):
        n = c3.SLOTS[kind][0]
        locs = c3.locations_of_states(kind, tuple(range(n)), rows)
        for row, w in zip(locs[::9], got[::9, kind]):
            assert words(kind, invert(kind, row)) == int(w)
            assert invert(kind, invert(kind, row)) == tuple(int(x) for x in row)
    twice = _lib.cube3_inverse_locs(inverse_rows(rows), _lib.ROWS_STATE)
    assert (twice == words_of_rows(rows)).all()
    goal = np.arange(54, dtype=np.uint8)[None]
    assert (_lib.cube3_inverse_locs(goal, _lib.ROWS_STATE) == words_of_rows(goal)).all()
    assert (_lib.cube3_inverse_locs(goal // 9, _lib.ROWS_NNET) == words_of_rows(goal)).all()
    # (r' = (o - r) mod o for every cubie would be wrong: the corner classes matter on these rows)
    corner = c3.locations_of_states(c3.CORNERS, tuple(range(8)), rows)
    cls = np.array(corner_classes())
    assert ((cls[corner // 3] != cls[None, :]) & (corner % 3 != 0)).any()


# ------------------------------------------------------------------------------------------------ 2. the definition
@pytest.mark.parametrize("n", [1, 2, ALL])
def test_dual_value_is_the_larger_of_the_symmetric_values_at_the_row_and_its_inverse(n):
    from deepcubea_amd import _lib
    rows = rule_rows()
    inv = inverse_rows(rows)
    want = np.maximum(host_eval(rows, _lib.ROWS_STATE, SMALL4, n, False), host_eval(inv, _lib.ROWS_STATE, SMALL4, n, False))
    assert (host_eval(rows, _lib.ROWS_STATE, SMALL4, n, True) == want).all()
    want_nnet = np.maximum(host_eval(rows // 9, _lib.ROWS_NNET, SMALL4, n, False), host_eval(inv // 9, _lib.ROWS_NNET, SMALL4, n, False))
    assert (want_nnet == want).all() and (host_eval(rows // 9, _lib.ROWS_NNET, SMALL4, n, True) == want).all()
    wide = np.full((len(rows), 61), 0xA5, np.uint8)  # a row stride above 54
    wide[:, :54] = rows
    assert (host_eval(wide, _lib.ROWS_STATE, SMALL4, n, True) == want).all()
    assert (want > host_eval(rows, _lib.ROWS_STATE, SMALL4, n, False)).any()


# ------------------------------------------------------------------------------------------------ 3. admissible, monotone
@lru_cache(maxsize=None)
def breadth_first_levels():
    """(states, exact distance): every state of the levels 0..4 from the goal and every 16th of level 5."""
    p = c3.perm_table()
    seen = {bytes(range(54))}
    level = np.arange(54, dtype=np.uint8)[None]
    states, dist = [level], [np.zeros(1, np.int64)]
    for d in range(1, 6):
        nxt = np.unique(np.concatenate([level[:, p[a]] for a in range(12)]), axis=0)
        keep = np.array([row.tobytes() not in seen for row in nxt])
        level = nxt[keep]
        seen.update(row.tobytes() for row in level)
        assert len(level) == ida.LEVELS[d - 1]
        take = level if d < 5 else level[::16]
        states.append(take)
        dist.append(np.full(len(take), d, np.int64))
    return np.concatenate(states), np.concatenate(dist)


def test_plain_sym_dual_and_the_distance_on_the_breadth_first_levels():
    from deepcubea_amd import _lib
    states, dist = breadth_first_levels()
    assert len(states) == 1 + 12 + 114 + 1068 + 10011 + (93840 + 15) // 16
    plain = host_eval(states, _lib.ROWS_STATE, SMALL4, 1, False)
    for n in (1, 8, ALL):
        s, d = host_eval(states, _lib.ROWS_STATE, SMALL4, n, False), host_eval(states, _lib.ROWS_STATE, SMALL4, n, True)
        assert (plain <= s).all() and (s <= d).all() and (d <= dist).all(), n
        assert int((d > s).sum()) > 0, n  # otherwise this shows nothing
    assert d[0] == 0 and (d[1:13] == 1).all()


# ------------------------------------------------------------------------------------------------ 4. the all-corner pattern
@lru_cache(maxsize=None)
def shallow_corner_table():
    """The 8-corner table with the entries of depth <= 6 filled in (breadth first over location rows), 0xFE elsewhere."""
    mv = c3.location_moves(c3.CORNERS)
    table = np.full(c3.table_size(c3.CORNERS, 8), c3.UNREACHED, np.uint8)
    locs = np.arange(0, 24, 3)[None]
    table[c3.rank_locations(c3.CORNERS, locs)] = 0
    for depth in range(1, 7):
        nxt = np.unique(np.concatenate([mv[a][locs] for a in range(12)]), axis=0)
        idx = c3.rank_locations(c3.CORNERS, nxt)
        fresh = table[idx] == c3.UNREACHED
        locs = nxt[fresh]
        table[idx[fresh]] = depth
    table.setflags(write=False)
    return table


def test_a_pattern_of_all_the_cubies_of_its_kind_has_equal_dual_and_regular_bytes():
    from deepcubea_amd import _lib
    table = shallow_corner_table()
    rows = rule_rows()
    rows = np.concatenate([rows, inverse_rows(rows)])
    at = table[c3.host_index(*WHOLE, rows, c3.ROWS_STATE)]
    at_inverse = table[c3.host_index(*WHOLE, inverse_rows(rows), c3.ROWS_STATE)]
    assert (at == at_inverse).all()  # (0xFE on both sides where the corners are deeper than the table goes)
    reached = at != c3.UNREACHED
    assert reached.sum() >= 100 and set(at[reached]) >= set(range(1, 7))
    # so the second pass skips it: whatever the table holds, the dual value of the pattern alone is its regular value ...
    junk = np.resize(np.random.default_rng(5).integers(0, 250, 1 << 22).astype(np.uint8), table.size)
    for n in (1, ALL):
        regular = host_eval(rows, _lib.ROWS_STATE, (WHOLE,), n, False, [junk])
        assert (host_eval(rows, _lib.ROWS_STATE, (WHOLE,), n, True, [junk]) == regular).all()
        assert (regular == junk[c3.host_index(*WHOLE, rows, c3.ROWS_STATE)]).all()
    # ... and in a set it adds nothing at the inverse, first in the list or not
    small = c3.SMALL["e0,e1,e2,e3"]
    for patterns, tables in (((WHOLE, small), [junk, c3.host_table(*small)]), ((small, WHOLE), [c3.host_table(*small), junk])):
        want = np.maximum(host_eval(rows, _lib.ROWS_STATE, patterns, ALL, False, tables), host_eval(rows, _lib.ROWS_STATE, (small,), ALL, True))
        assert (host_eval(rows, _lib.ROWS_STATE, patterns, ALL, True, tables) == want).all()


# ------------------------------------------------------------------------------------------------ 5. any bytes
@lru_cache(maxsize=None)
def any_rows():
    rng = np.random.default_rng(61)
    rows = rng.integers(0, 256, (1500, 54)).astype(np.uint8)
    for i, b in enumerate((0, 0xFF, 5, 6, 53, 54, 0x80)):
        rows[i] = b  # 54 equal bytes
    rows[7:500] %= 54  # valid bytes that are no cube states: duplicate and missing cubies
    rows[500:1000] %= 6
    rows[1000:1100] = 6 + rows[1000:1100] % 250  # every byte >= 6
    rows[1100:1200] = 54 + rows[1100:1200] % 202  # every byte >= 54
    rows.setflags(write=False)
    return rows


ANY_SETS = (((c3.CORNERS, (7, 3, 0)), (c3.EDGES, (11,)), (c3.CORNERS, (4, 5, 6, 7)), (c3.EDGES, (8, 9, 10, 11))),
            ((c3.EDGES, (3, 9, 0, 5, 1)),), ((c3.CORNERS, (2, 6, 1, 5)), WHOLE, (c3.EDGES, (6, 2, 7, 1, 0, 10))))


def any_tables(patterns, seed=62):
    rng = np.random.default_rng(seed)
    return [np.resize(rng.integers(0, 256, min(c3.table_size(kind, len(g)), 1 << 22)).astype(np.uint8), c3.table_size(kind, len(g)))
            for kind, g in patterns]


def locations_by_the_rule(rows, row_kind):
    """(locations, inverted locations) of ANY rows, kind -> [m, n]: a cubie's location is the index of its one-cubie pattern."""
    from deepcubea_amd import _lib
    loc = {kind: np.stack([_lib.cube3_pdb_index(kind, (c,), rows, row_kind) for c in range(c3.SLOTS[kind][0])], 1)
           for kind in (c3.CORNERS, c3.EDGES)}
    assert all(v.min() >= 0 and v.max() < 24 for v in loc.values())
    back = {kind: np.array([invert(kind, row) for row in loc[kind]]) for kind in loc}
    assert all(v.min() >= 0 and v.max() < 24 for v in back.values())
    return loc, back


@lru_cache(maxsize=None)
def any_locations(row_kind):
    return locations_by_the_rule(any_rows(), row_kind)  # computed once per row kind


def dual_value_by_the_rule(rows, row_kind, patterns, tables, n):
    """The header's dual value in plain Python for ANY rows: a cubie's location is the index of its one-cubie pattern; the list at
    those locations, then — but for the patterns of all the cubies of their kind — at the locations inverted by the replacing rule."""
    loc, back = any_locations(row_kind) if rows is any_rows() else locations_by_the_rule(rows, row_kind)
    want = np.zeros(len(rows), np.int64)
    for (kind, cubies), table in zip(patterns, tables):
        for s, source in sym.images(kind, cubies, n):
            for at in (loc, back):
                if at is back and len(cubies) == c3.SLOTS[kind][0]:
                    continue
                mapped = np.stack([sym.location_map(s, kind, c)[at[kind][:, c]] for c in source], 1)
                idx = sym.clamped_rank(kind, mapped)
                assert idx.min() >= 0 and idx.max() < table.size
                want = np.maximum(want, table[idx])
    return want


def test_any_bytes_stay_in_bounds_and_equal_the_replacing_rule():
    from deepcubea_amd import _lib
    rows = any_rows()
    for patterns in ANY_SETS:
        tables = any_tables(patterns)
        for row_kind in (_lib.ROWS_STATE, _lib.ROWS_NNET):
            for n in (1, 3, ALL):
                want = dual_value_by_the_rule(rows, row_kind, patterns, tables, n)
                assert (host_eval(rows, row_kind, patterns, n, True, tables) == want).all(), (patterns, row_kind, n)
    # the words themselves: every field < 24, and equal to the Python rule on the row's locations
    got = _lib.cube3_inverse_locs(rows, _lib.ROWS_STATE)
    for kind in (c3.CORNERS, c3.EDGES):
        n = c3.SLOTS[kind][0]
        fields = np.stack([(got[:, kind] >> np.uint64(5 * q)) & np.uint64(31) for q in range(12)], 1)
        assert fields[:, :n].max() < 24 and (fields[:, n:] == 0).all() and (got[:, kind] >> np.uint64(60) == 0).all()
        loc = np.stack([_lib.cube3_pdb_index(kind, (c,), rows[:300], _lib.ROWS_STATE) for c in range(n)], 1)
        assert [words(kind, invert(kind, row)) for row in loc] == [int(w) for w in got[:300, kind]]


# ------------------------------------------------------------------------------------------------ 6. IDA*
def h_dual(n, patterns=None):
    """h as a callable on (corner locations, edge locations): the dual value over IDA_SET (no pattern of it is skipped)."""
    h = sym.h_of(n)
    return lambda state: max(h(state), h((invert(c3.CORNERS, state[0]), invert(c3.EDGES, state[1]))))


def host_search(root, n, dual=True, max_nodes=ida.BIG, tables=None):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_CUBE3, 0, root, IDA_SET, sym.tables_of(IDA_SET) if tables is None else tables, max_nodes, sym=n, dual=dual)


@lru_cache(maxsize=None)
def dual_reference(case, n):
    """(root, (thresholds, counts) of the recursive search under the full dual value over the first n images)."""
    root = ida.cube3_suffix_root(*case)
    return root, sym.exact_search(root, h_dual(n), case[1])


@pytest.mark.parametrize("depth", [-1, 0, 2, 3])
@pytest.mark.parametrize("case", IDA_CASES, ids=lambda c: "root%d-%d" % c)
def test_host_idastar_on_the_dual_look_ups_keeps_the_contract(case, depth, prefix):
    root, exact = dual_reference(case, ALL)
    prefix(depth)
    res = host_search(root, ALL)
    k = case[1]
    assert res["solved"] and len(res["moves"]) == k and res["nodes_generated"] == sum(res["nodes_per_threshold"])
    assert (ida.replay_cube3(root, res["moves"]) == np.arange(54)).all()
    thresholds, counts = res["thresholds"], res["nodes_per_threshold"]
    h = h_dual(ALL)
    assert all(a < b for a, b in zip(thresholds, thresholds[1:]))
    assert thresholds[0] == h(sym.root_locations(root)) and thresholds[-1] == k
    assert set(exact[0]) <= set(thresholds)
    for T, count in zip(thresholds[:-1], counts[:-1]):
        assert count == sym.tree(root, h, T)[0], T
        assert count <= sym.tree(root, sym.h_of(ALL), T)[0], T  # never more than the same spec's tree without +dual
    without = host_search(root, ALL, dual=False)
    assert without["solved"] and len(without["moves"]) == k
    for T, count in zip(thresholds[:-1], counts[:-1]):
        if T in without["thresholds"][:-1]:
            assert count <= without["nodes_per_threshold"][without["thresholds"].index(T)]


@pytest.mark.parametrize("case", IDA_CASES, ids=lambda c: "root%d-%d" % c)
def test_host_idastar_with_one_image_is_the_search_on_plain_and_dual(case, prefix):
    root, exact = dual_reference(case, 1)
    h = h_dual(1)
    for depth in (-1, 3):
        prefix(depth)
        res = host_search(root, 1)
        assert res["solved"] and len(res["moves"]) == case[1] and res["thresholds"][0] == h(sym.root_locations(root))
        assert set(exact[0]) <= set(res["thresholds"])
        for T, count in zip(res["thresholds"][:-1], res["nodes_per_threshold"][:-1]):
            assert count == sym.tree(root, h, T)[0], T
    from deepcubea_amd import _lib  # (the wrapper's sym = 0 with dual is max_images = 1)
    zero = _lib.idastar_host(_lib.ENV_CUBE3, 0, root, IDA_SET, sym.tables_of(IDA_SET), ida.BIG, dual=True)
    assert zero["thresholds"] == res["thresholds"] and zero["nodes_per_threshold"][:-1] == res["nodes_per_threshold"][:-1]


def root_reads(root, n):
    """The table reads of h(root): [(pattern number, index, is it a read of the second pass)] over IDA_SET's first n images."""
    state = sym.root_locations(root)
    back = (invert(c3.CORNERS, state[0]), invert(c3.EDGES, state[1]))
    reads = []
    for p, (kind, cubies) in enumerate(IDA_SET):
        for s, source in sym.images(kind, cubies, n):
            for at in (state, back):
                mapped = np.array([[sym.location_map(s, kind, c)[at[kind][c]] for c in source]])
                reads.append((p, int(c3.rank_locations(kind, mapped)[0]), at is back))
    return reads


def test_budget_goal_and_a_root_that_only_a_dual_byte_kills(prefix):
    from deepcubea_amd import _lib
    case = (2, 7)
    root, _ = dual_reference(case, ALL)
    full = host_search(root, ALL)
    first = full["nodes_per_threshold"][0]
    assert first >= 8 and len(full["thresholds"]) >= 2
    budget = first - 2  # the budget ends inside the first threshold: never "solved" on a lie
    out = host_search(root, ALL, max_nodes=budget)
    assert not out["solved"] and out["status"] == "budget exhausted" and out["moves"] == []
    assert budget < out["nodes_generated"] <= budget + budget // 2 and out["thresholds"] == full["thresholds"][:1]  # one lane, interval budget / 2
    goal = host_search(np.arange(54, dtype=np.uint8), ALL)
    assert goal["solved"] and goal["moves"] == [] and goal["thresholds"] == []
    # a byte that only the second pass reads at the root
    reads = root_reads(root, ALL)
    regular = {(p, idx) for p, idx, second in reads if not second}
    only_dual = [(p, idx) for p, idx, second in reads if second and (p, idx) not in regular]
    assert only_dual
    p, idx = only_dual[0]
    dead = [t.copy() for t in sym.tables_of(IDA_SET)]
    dead[p][idx] = 0xFE
    res = host_search(root, ALL, tables=dead)
    assert res["status"] == "unsolvable" and res["thresholds"] == [] and not res["solved"]
    alive = host_search(root, ALL, dual=False, tables=dead)
    assert alive["solved"] and len(alive["moves"]) == 7
    # 54 distinct sticker ids that are no cube state: the dual search names the root; the symmetric one takes it as before
    bad = np.arange(54, dtype=np.uint8)
    bad[[0, 10, 8, 12]] = bad[[10, 0, 12, 8]]  # two corner cubies are nowhere: the colour rule puts both at location 0
    with pytest.raises(_lib.DcaError, match="bad argument: dca_idastar_host_dual: root: .*no cube state"):
        host_search(bad, ALL, max_nodes=100)
    assert host_search(bad, ALL, dual=False, max_nodes=100)["status"] == "budget exhausted"
    with pytest.raises(ValueError, match="cube3 only"):
        _lib.idastar_host(_lib.ENV_NPUZZLE, 3, np.arange(9, dtype=np.uint8), ((1, 2),), [np.zeros(729, np.uint8)], 10, dual=True)


def test_library_refusals_are_those_of_the_symmetric_entry_points():
    from deepcubea_amd import _lib
    L = _lib.lib()
    small = (c3.SMALL["c0,c1,c2"],)
    tables = sym.tables_of(small)
    kinds, ids, ks = np.array([0], np.int32), np.array([0, 1, 2], np.uint8), np.array([3], np.int32)
    ptrs = (C.c_void_p * 1)(tables[0].ctypes.data)
    rows, out = np.arange(54, dtype=np.uint8)[None].copy(), np.full(1, -3.0, np.float32)

    def raw(max_images, n=1, ld=54, row_kind=0, states=rows.ctypes.data, k=kinds.ctypes.data):
        rc = L.dca_cube3_pdb_eval_dual_host(states, n, ld, row_kind, 1, k, ids.ctypes.data, ks.ctypes.data, ptrs, max_images, out.ctypes.data)
        return rc, L.dca_last_error()
    for bad in (0, -1, 49):
        rc, msg = raw(bad)
        assert rc == -1 and msg.startswith(b"bad argument: dca_cube3_pdb_eval_dual_host") and b"max_images" in msg and out[0] == -3.0
    assert raw(48, ld=53)[0] == -1 and raw(48, row_kind=2)[0] == -1 and raw(48, n=-1)[0] == -1
    assert raw(48, states=None)[0] == -1 and raw(48, k=None)[0] == -1 and out[0] == -3.0
    assert raw(48, n=0, states=None)[0] == 0 and raw(48)[0] == 0 and out[0] == 0.0
    three = (c3.SMALL["c0,c1,c2"], (c3.CORNERS, (5, 6, 7)), (c3.CORNERS, (1, 2, 4)))  # 72 look-ups: the cap counts list entries
    with pytest.raises(_lib.DcaError, match=r"72 look-ups.*\+sym:N"):
        host_eval(rows, 0, three, 48, True, [tables[0]] * 3)
    assert host_eval(rows, 0, three, 21, True, [tables[0]] * 3).shape == (1,)  # 63 list entries fit (sizes alone matter here)
    with pytest.raises(_lib.DcaError, match="max_images"):
        host_search(ida.cube3_suffix_root(0, 7), 49)
    words = np.zeros(2, np.uint64)
    assert L.dca_cube3_inverse_locs(None, 0, words.ctypes.data) == -1 and L.dca_cube3_inverse_locs(rows.ctypes.data, 0, None) == -1
    assert L.dca_cube3_inverse_locs(rows.ctypes.data, 2, words.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------ 7. spec, .npz, CLI
def test_spec_suffix_and_its_refusals(no_device):
    from deepcubea_amd.utils import cube3_pdb as cp
    from deepcubea_amd.utils import pattern_db as pd
    assert cp.split_suffixes("korf") == ("korf", 0, False) and cp.split_suffixes(" korf7 + DUAL ") == ("korf7", 0, True)
    assert cp.split_suffixes("c0,c1/e1+sym:5+dual") == ("c0,c1/e1", 5, True) and cp.split_suffixes("korf+dual+sym") == ("korf", 48, True)
    assert cp.split_suffixes("korf+sym: 48") == ("korf", 48, False)
    assert cp.split_sym("korf+sym:5") == ("korf", 5) and cp.split_sym("korf") == ("korf", 0)  # its shape and its values stay
    base = cp.Cube3PatternDatabase("korf")
    for spec, n, suffix in (("korf+dual", 0, "+dual"), ("korf+sym+dual", 48, "+sym+dual"), ("korf+dual+sym", 48, "+sym+dual"),
                            ("korf+sym:4+dual", 4, "+sym:4+dual"), ("korf+dual+sym:4", 4, "+sym:4+dual"), ("korf+sym:1+dual", 1, "+sym:1+dual"),
                            ("korf7 +Dual", 0, "+dual")):
        pdb = cp.Cube3PatternDatabase(spec)
        plain = cp.Cube3PatternDatabase(spec.split("+")[0])
        assert pdb.dual and pdb.sym == n and pdb.spec == plain.spec + suffix
        assert pdb.bytes == plain.bytes and pdb.patterns == plain.patterns  # no table bytes
        again = cp.Cube3PatternDatabase(pdb.spec)
        assert again.dual and again.sym == n and again.patterns == pdb.patterns and again.spec == pdb.spec
    assert not base.dual and "+" not in base.spec and not cp.Cube3PatternDatabase("korf+sym:8").dual
    assert cp.Cube3PatternDatabase(base.patterns, sym=8, dual=True).spec == base.spec + "+sym:8+dual"
    assert cp.Cube3PatternDatabase(base.patterns, dual=True).spec == base.spec + "+dual"
    refused = ("korf+dual+dual", "korf+dual:2", "korf+dual:", "korf+duall", "korf+dual+sym+dual", "+dual", "korf+dual+", "bogus+dual",
               "korf+dual+reflect", "korf+reflect+dual", "korf+sym+dual+sym", "korf+sym:0+dual", "korf+dual+sym:49",
               # every spec the symmetric test refuses today
               "korf+sym+sym", "korf+sym:0", "korf+sym:49", "korf+sym:-1", "korf+sym:", "korf+sym:x", "korf+symm", "korf+sym:1:2",
               "korf+", "+sym", "korf+sym+reflect", "korf+reflect+sym", "bogus+sym")
    for spec in refused:
        with pytest.raises(ValueError):
            cp.Cube3PatternDatabase(spec)
    with pytest.raises(ValueError, match="a suffix such as \\+reflect is defined for the sliding puzzles only"):  # today's message
        cp.Cube3PatternDatabase("korf+reflect")
    with pytest.raises(ValueError, match="once"):
        cp.Cube3PatternDatabase("korf+dual+dual")
    over = "c0,c1,c2/c5,c6,c7/c1,c2,c4"
    with pytest.raises(ValueError, match=r"72 look-ups.*cap of 64.*\+sym:N"):  # the cap counts list entries, dual or not
        cp.Cube3PatternDatabase(over + "+sym+dual")
    assert cp.Cube3PatternDatabase(over + "+sym:21+dual").sym == 21
    for env in ("puzzle15", "puzzle8"):
        with pytest.raises(ValueError):
            pd.PatternDatabase(env, "auto+dual")


def test_npz_round_trips_the_suffix_and_old_files_load_without_it(tmp_path, no_device):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    patterns = (c3.SMALL["c0,c1,c2"], (c3.EDGES, (11, 0)))
    tables = sym.tables_of(patterns)
    for n, dual, suffix in ((48, True, "+sym+dual"), (5, True, "+sym:5+dual"), (0, True, "+dual"), (5, False, "+sym:5"), (0, False, "")):
        path = str(tmp_path / ("c3_%d_%d.npz" % (n, dual)))
        Cube3PatternDatabase(patterns, sym=n, dual=dual).save(path, tables=tables)
        back, got = Cube3PatternDatabase.load_host(path)
        assert back.sym == n and back.dual == dual and back.patterns == patterns and back.spec == "c0,c1,c2/e11,e0" + suffix
        assert all(np.array_equal(g, t) for g, t in zip(got, tables))
    for name, spec in (("old", "c0,c1,c2/e11,e0"), ("sym", "c0,c1,c2/e11,e0+sym:5")):  # files as they were written before the suffix existed
        path = str(tmp_path / (name + ".npz"))
        np.savez(path, table_0=tables[0], table_1=tables[1], env_name=np.array("cube3"), partition=np.array(spec))
        assert not Cube3PatternDatabase.load_host(path)[0].dual


def test_cli_refusals_and_help_touch_no_device(no_device):
    from deepcubea_amd.search_methods import astar, idastar
    for module in (astar, idastar):
        help_text = " ".join({a.dest: a for a in module.build_parser()._actions}["model_dir"].help.split())
        assert "SPEC+dual" in help_text and "SPEC+sym:N+dual" in help_text and "admissible but not consistent" in help_text
        assert "SPEC+sym" in help_text and "SPEC+sym:N" in help_text and "SPEC+reflect" in help_text
    help_text = " ".join({a.dest: a for a in astar.build_parser()._actions}["model_dir"].help.split())
    assert "Without +dual admissible and consistent: with --weight 1 --semantics cpp the solutions are optimal" in help_text
    for model in ("pdb:korf+dual+dual", "pdb:korf+dual:2", "pdb:korf+reflect+dual", "pdb:c0,c1,c2/c5,c6,c7/c1,c2,c4+sym+dual", "pdb:korf+sym:49+dual"):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env="cube3"), None)
        with pytest.raises(ValueError):
            idastar.pattern_database(SimpleNamespace(model_dir=model, env="cube3"))
    for env in ("puzzle8", "puzzle15", "puzzle24"):
        for spec in ("auto+dual", "auto+reflect+dual", "auto+dual+reflect"):
            with pytest.raises(ValueError, match="cube3 only; the blank makes the inverse of a sliding-puzzle state no state of the same problem"):
                idastar.pattern_database(SimpleNamespace(model_dir="pdb:" + spec, env=env))
            with pytest.raises(ValueError):
                astar._load_heuristic(SimpleNamespace(model_dir="pdb:" + spec, env=env), None)
        assert idastar.pattern_database(SimpleNamespace(model_dir="pdb:auto+reflect", env=env)).reflect
    for model, n in (("pdb:korf+dual", 0), ("pdb:korf+sym:8+dual", 8), ("pdb:korf+dual+sym:8", 8)):
        pdb = idastar.pattern_database(SimpleNamespace(model_dir=model, env="cube3"))
        assert pdb.dual and pdb.sym == n and pdb.spec.endswith("+dual")
        assert astar._pattern_database(SimpleNamespace(model_dir=model, env="cube3")).spec == pdb.spec
    assert idastar.DEFAULT_MAX_NODES == {"puzzle": int(60 * 1.14e8), "cube3": int(60 * 8.52e9)}


# ------------------------------------------------------------------------------------------------ 8. ABI
def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    L = _lib.lib()
    product = open(os.path.join(ROOT, "include", "dca.h")).read()
    debug = open(os.path.join(ROOT, "include", "dca_debug.h")).read()
    for names, hdr, other in ((NEW_PRODUCT, product, debug), (NEW_DEBUG, debug, product)):
        declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
        elsewhere = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", other))
        for name in names:
            assert name in declared and name not in elsewhere, name
            assert name in _lib._SIGNATURES and name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    assert "#define DCA_ABI_VERSION 6" in product and L.dca_abi_version() == 6
    assert "#define DCA_CUBE3_SYM_MAX_LOOKUPS 64\n" in product
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    assert list(L.dca_cube3_pdb_eval_dual.argtypes) == list(L.dca_cube3_pdb_eval_sym.argtypes) == [p, i64, i64, i, i, p, p, p, p, i, p, p]
    assert list(L.dca_cube3_pdb_eval_dual_host.argtypes) == [p, i64, i64, i, i, p, p, p, p, i, p]
    assert list(L.dca_idastar_cube3_dual.argtypes) == list(L.dca_idastar_cube3_sym.argtypes) == [p, i, p, p, p, p, i, i64, p, p, p, i, p, p, p, i, p, p]
    assert list(L.dca_idastar_host_dual.argtypes) == [p, i, p, p, p, p, i, i64, p, p, p, i, p, p, p, i, p]
    assert list(L.dca_cube3_inverse_locs.argtypes) == [p, i, p]
    flat = re.sub(r"\s*\n \*\s*", " ", product)  # the header states the rules and the contract
    for phrase in ("S^-1[S[p]] = p (numpy: argsort(S))", "max(v(S), v(S^-1))",
                   "for cubie j = 0 ... n-1 in ascending order at location (s_j, r_j), REPLACE field s_j by the location (j, r'_j)",
                   "r' = (3 - r) mod 3 where slot s_j and slot j are of one class, r' = r where they are not",
                   "a field is replaced (mask, then or), never or-ed onto stale bits: the last writer wins",
                   "The IDA* lane uses the or-only form",
                   "a pattern that names all n cubies of its kind (the 8-corner table)", "Its dual look-ups are skipped",
                   "admissible but not consistent", "the thresholds increase strictly",
                   "every threshold of the exact search (h = the full dual value everywhere) occurs among them",
                   "a property of the tree", "ANY regular or dual byte at the root is 0xFE or 0xFF"):
        assert phrase in flat, phrase
