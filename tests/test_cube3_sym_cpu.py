"""CPU-side tests of the symmetric look-ups for the cube3 pattern databases (`pdb:<spec>+sym`, include/dca.h "Symmetric
look-ups"): the 48 symmetries against a derivation written here from the move table, the images of a pattern, the host twin of the
eval kernel against table bytes at rows conjugated in numpy, the facts on the 21 637 states of the shipped optimal paths, the host
IDA* against a recursive search written here, the any-bytes rule, every refusal that needs no device, the spec suffix through the
class, the .npz and both CLIs.  No GPU needed.  tests/test_cube3_sym_hip.py imports the helpers."""
import ctypes as C
import os
import re
from functools import lru_cache
from itertools import permutations
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_cube3_pdb_cpu as c3
from tests import test_idastar_cpu as ida

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PRODUCT = ("dca_cube3_pdb_eval_sym", "dca_idastar_cube3_sym")
NEW_DEBUG = ("dca_idastar_host_sym", "dca_cube3_pdb_eval_sym_host", "dca_cube3_sym_tables", "dca_cube3_sym_images")
ALL = 48
CAP = 64
# distinct images of a pattern: its distinct source cubie sets
DISTINCT = {(c3.EDGES, tuple(range(0, 6))): 24, (c3.EDGES, tuple(range(6, 12))): 24, (c3.EDGES, tuple(range(0, 7))): 24,
            (c3.EDGES, tuple(range(5, 12))): 24, c3.SMALL["c0,c1,c2"]: 24, c3.SMALL["e0,e1,e2,e3"]: 6, c3.SMALL["c4,c5,c6,c7"]: 6,
            c3.SMALL["e8,e9,e10,e11"]: 3, (c3.CORNERS, tuple(range(8))): 1}
IDA_SET = (c3.SMALL["c0,c1,c2"], c3.SMALL["e8,e9,e10,e11"])  # 24 + 3 = 27 look-ups
# root (instance, k) -> thresholds below the solution and their node counts: the plain search, the search on all images
IDA_CASES = {(2, 7): (([4, 5, 6], [28, 119, 834]), ([6], [31])), (0, 8): (([6, 7], [51, 392]), ([6, 7], [12, 126])),
             (0, 7): (([5, 6], [12, 117]), ([6], [12])), (1, 8): (([7], [215]), ([7], [30]))}


# ------------------------------------------------------------------------------------------------ the derivation, in Python
@lru_cache(maxsize=None)
def cubie_sets():
    """kind -> per cubie the frozenset of its colours (position // 9)."""
    return {kind: [frozenset(p // 9 for p in lst) for lst in c3.cubie_lists(kind)] for kind in (c3.CORNERS, c3.EDGES)}


@lru_cache(maxsize=None)
def symmetries():
    """-> (face maps [48][6], sticker permutations [48, 54], move maps [48, 12], cubie maps: kind -> [48][n]) in the header's
    order: face maps that keep opposite pairs, ascending lexicographically."""
    P = c3.perm_table()
    sets = cubie_sets()
    every = [s for kind in sets for s in sets[kind]]
    opposite = {f: [g for g in range(6) if g != f and not any({f, g} <= s for s in every)] for f in range(6)}
    assert all(len(v) == 1 for v in opposite.values())
    assert [opposite[f][0] for f in range(6)] == [1, 0, 3, 2, 5, 4]
    faces = [phi for phi in permutations(range(6)) if all(phi[opposite[f][0]] == opposite[phi[f]][0] for f in range(6))]
    owner = {}
    for kind in sets:
        for c, lst in enumerate(c3.cubie_lists(kind)):
            for p in lst:
                owner[p] = (kind, c)
    sticker, move, cubie = [], [], {c3.CORNERS: [], c3.EDGES: []}
    for phi in faces:
        for kind in sets:
            cubie[kind].append([sets[kind].index(frozenset(phi[f] for f in s)) for s in sets[kind]])
        sigma = np.zeros(54, np.int64)
        for p in range(54):
            if p not in owner:  # a centre
                (sigma[p],) = [q for q in range(54) if q not in owner and q // 9 == phi[p // 9]]
            else:
                kind, c = owner[p]
                (sigma[p],) = [q for q in c3.cubie_lists(kind)[cubie[kind][-1][c]] if q // 9 == phi[p // 9]]
        assert sorted(sigma) == list(range(54))
        pi = []
        for a in range(12):
            (b,) = [b for b in range(12) if (P[b][sigma] == sigma[P[a]]).all()]
            pi.append(b)
        sticker.append(sigma)
        move.append(pi)
    return faces, np.array(sticker), np.array(move), cubie


@lru_cache(maxsize=None)
def location_map(s, kind, c):
    """R_{sigma,c}: R[home(c)] = home(sigma(c)), R[move_a(l)] = move_pi(a)(R[l]), filled breadth first."""
    _, _, move, cubie = symmetries()
    o = c3.SLOTS[kind][1]
    mv = c3.location_moves(kind)
    R = {c * o: cubie[kind][s][c] * o}
    queue = [c * o]
    while queue:
        l = queue.pop(0)
        for a in range(12):
            l2, v = int(mv[a][l]), int(mv[move[s][a]][R[l]])
            if l2 not in R:
                R[l2] = v
                queue.append(l2)
            assert R[l2] == v
    assert sorted(R) == list(range(24))
    return np.array([R[l] for l in range(24)])


def images(kind, cubies, n=ALL):
    """The first n images of a pattern -> [(symmetry, source cubies)]: distinct source cubie SETS in the symmetries' order."""
    cubie = symmetries()[3][kind]
    seen, out = [], []
    for s in range(ALL):
        src = tuple(cubie[s].index(q) for q in cubies)
        if set(src) not in seen and len(out) < n:
            seen.append(set(src))
            out.append((s, src))
    return out


def conjugate(rows, s):
    """S'[sigma(p)] = sigma(S[p]) on rows of sticker ids."""
    sigma = symmetries()[1][s]
    out = np.empty_like(rows)
    out[:, sigma] = sigma[rows].astype(rows.dtype)
    return out


def tables_of(patterns):
    return [c3.host_table(*p) for p in patterns]


def conjugated_max(rows, patterns, n):
    """Max over the first n images of every pattern of the plain table byte at the conjugated row (rows: sticker ids)."""
    best = np.zeros(len(rows), np.int64)
    for (kind, cubies), table in zip(patterns, tables_of(patterns)):
        for s, _ in images(kind, cubies, n):
            best = np.maximum(best, table[c3.host_index(kind, cubies, conjugate(rows, s), c3.ROWS_STATE)])
    return best


@lru_cache(maxsize=None)
def path_values():
    """On path_states() with the four SMALL patterns: (plain value, value over all images), computed once."""
    states = c3.path_states()[0]
    patterns = tuple(c3.SMALL.values())
    plain, full = conjugated_max(states, patterns, 1), conjugated_max(states, patterns, ALL)
    for a in (plain, full):
        a.setflags(write=False)
    return plain, full


def host_eval(rows, row_kind, patterns, n, tables=None):
    from deepcubea_amd import _lib
    return _lib.cube3_pdb_eval_host(rows, row_kind, patterns, tables_of(patterns) if tables is None else tables, sym=n)


# ------------------------------------------------------------------------------------------------ the symmetries
def test_the_library_symmetries_equal_the_derivation():
    from deepcubea_amd import _lib
    faces, sticker, move, _ = symmetries()
    got_sticker, got_move = _lib.cube3_sym_tables()
    assert got_sticker.shape == (48, 54) and got_move.shape == (48, 12)
    assert (got_sticker == sticker).all() and (got_move == move).all()
    assert len(faces) == 48 and faces == sorted(faces) and faces[0] == tuple(range(6))
    assert (sticker[0] == np.arange(54)).all() and (move[0] == np.arange(12)).all()
    P = c3.perm_table()
    for s in range(48):  # each symmetry conjugates every move onto the move its map names
        for a in range(12):
            assert (P[move[s][a]][sticker[s]] == sticker[s][P[a]]).all()
        assert sorted(move[s]) == list(range(12))
    assert len({tuple(m) for m in move}) == 48
    keeps = [bool(((m & 1) == (np.arange(12) & 1)).all()) for m in move]
    flips = [bool(((m & 1) != (np.arange(12) & 1)).all()) for m in move]
    assert sum(keeps) == 24 and sum(flips) == 24
    group = {tuple(x) for x in sticker}
    assert len(group) == 48 and all(tuple(sticker[s][sticker[t]]) in group for s in range(48) for t in range(48))


def test_conjugation_commutes_with_the_moves():
    _, sticker, move, _ = symmetries()
    P = c3.perm_table()
    rows = c3.scrambles(200, 25, 11)
    rng = np.random.default_rng(12)
    for s in range(48):
        assert (conjugate(np.arange(54, dtype=np.uint8)[None], s)[0] == np.arange(54)).all()  # the goal is fixed
        a = int(rng.integers(0, 12))
        assert (conjugate(rows[:, P[a]], s) == conjugate(rows, s)[:, P[move[s][a]]]).all()


@pytest.mark.parametrize("pattern", list(DISTINCT), ids=lambda p: "%s%s" % ("ce"[p[0]], "-".join(map(str, p[1]))))
def test_images_of_a_pattern(pattern):
    from deepcubea_amd import _lib
    kind, cubies = pattern
    want = images(kind, cubies)
    syms, src, maps = _lib.cube3_sym_images(kind, cubies)
    assert len(want) == DISTINCT[pattern] == len(syms)
    assert syms.tolist() == [s for s, _ in want] and src.tolist() == [list(c) for _, c in want]
    assert syms[0] == 0 and src[0].tolist() == list(cubies) and (maps[0] == np.arange(24)).all()  # the pattern itself first
    assert len({frozenset(row) for row in src.tolist()}) == len(src)
    for i, (s, source) in enumerate(want):
        for j, c in enumerate(source):
            assert (maps[i, j] == location_map(s, kind, c)).all(), (s, c)
    for n in (1, 2, 5, 47):  # +sym:N is a prefix of +sym
        ps, pc, pm = _lib.cube3_sym_images(kind, cubies, n)
        m = min(n, len(syms))
        assert ps.tolist() == syms[:m].tolist() and (pc == src[:m]).all() and (pm == maps[:m]).all()


# ------------------------------------------------------------------------------------------------ the eval's host twin
@pytest.mark.parametrize("n", [1, 2, ALL])
def test_host_eval_is_the_max_of_the_table_bytes_at_the_conjugated_rows(n):
    from deepcubea_amd import _lib
    patterns = tuple(c3.SMALL.values())
    states = c3.path_states()[0]
    rows = np.concatenate([c3.scrambles(1500, 40, 21), states[::7], states[-40:]])
    want = conjugated_max(rows, patterns, n).astype(np.float32)
    assert (host_eval(rows, _lib.ROWS_STATE, patterns, n) == want).all()
    assert (host_eval(rows // 9, _lib.ROWS_NNET, patterns, n) == want).all()
    wide = np.full((len(rows), 61), 0xA5, np.uint8)  # a row stride above 54
    wide[:, :54] = rows
    assert (host_eval(wide, _lib.ROWS_STATE, patterns, n) == want).all()
    if n == 1:  # +sym:1 is the plain heuristic, bit for bit
        assert (want == c3.host_eval(rows, c3.ROWS_STATE, patterns, tables_of(patterns))).all()


def test_the_facts_on_the_shipped_path_states():
    from deepcubea_amd import _lib
    states, dist, last = c3.path_states()
    patterns = tuple(c3.SMALL.values())
    plain, full = path_values()
    assert (host_eval(states, _lib.ROWS_STATE, patterns, ALL) == full).all()
    assert (host_eval(states, _lib.ROWS_STATE, patterns, 1) == plain).all()
    assert (full <= dist).all() and (full[dist == 0] == 0).all()                 # admissible
    assert np.abs(full[1:] - full[:-1])[~last[:-1]].max() <= 1                    # changes by at most 1 along every path
    assert int((plain == dist).sum()) == 6258 and int((full == dist).sum()) == 7792
    assert int((full > plain).sum()) == 8740 and (full >= plain).all()


def test_the_value_never_decreases_with_n():
    from deepcubea_amd import _lib
    patterns = tuple(c3.SMALL.values())
    rows = np.concatenate([c3.scrambles(600, 40, 31), c3.path_states()[0][::40]])
    junk = np.random.default_rng(32).integers(0, 256, (300, 54)).astype(np.uint8)
    for r in (rows, junk):
        prev = host_eval(r, _lib.ROWS_STATE, patterns, 1)
        for n in list(range(2, 26)) + [ALL]:
            cur = host_eval(r, _lib.ROWS_STATE, patterns, n)
            assert (cur >= prev).all(), n
            prev = cur
    assert (host_eval(rows, _lib.ROWS_STATE, patterns, 24) == host_eval(rows, _lib.ROWS_STATE, patterns, ALL)).all()  # no pattern has more


# ------------------------------------------------------------------------------------------------ any bytes
def clamped_rank(kind, locs):
    """The header's index rule with the any-bytes clamp: digit j counts the DISTINCT earlier slots below s_j, d_j <= n - j - 1."""
    n, o = c3.SLOTS[kind]
    locs = np.asarray(locs, np.int64)
    k = locs.shape[1]
    s, r = locs // o, locs % o
    rank, orient, seen = np.zeros(len(locs), np.int64), np.zeros(len(locs), np.int64), np.zeros(len(locs), np.int64)
    for j in range(k):
        below = seen & ((1 << s[:, j]) - 1)
        d = np.minimum(s[:, j] - np.array([bin(int(x)).count("1") for x in below]), n - 1 - j)
        seen |= 1 << s[:, j]
        rank = rank * (n - j) + d
        orient = orient * o + r[:, j]
    return rank * o ** k + orient


def test_any_bytes_stay_in_bounds_and_equal_the_host_rule():
    from deepcubea_amd import _lib
    rng = np.random.default_rng(41)
    rows = rng.integers(0, 256, (3000, 54)).astype(np.uint8)
    rows[0], rows[1], rows[2] = 0, 0xFF, 5
    rows[3:1000] %= 54  # valid bytes that are no cube states: duplicate and missing cubies
    rows[1000:2000] %= 6
    sets = (((c3.CORNERS, (7, 3, 0)), (c3.EDGES, (11,)), (c3.CORNERS, (4, 5, 6, 7)), (c3.EDGES, (8, 9, 10, 11))),  # 24 + 12 + 6 + 3
            ((c3.EDGES, (3, 9, 0, 5, 1)),), ((c3.CORNERS, tuple(range(8))), (c3.EDGES, (6, 2, 7, 1, 0, 10, 4))))
    for patterns, row_kind in ((p, r) for p in sets for r in (_lib.ROWS_STATE, _lib.ROWS_NNET)):
        tables = [rng.integers(0, 256, min(c3.table_size(kind, len(g)), 1 << 22)).astype(np.uint8) for kind, g in patterns]  # random tables
        tables = [np.resize(t, c3.table_size(kind, len(g))) for t, (kind, g) in zip(tables, patterns)]
        # a cubie's location by the any-bytes rule: the index of the one-cubie pattern is s * o + r
        loc = {kind: np.stack([_lib.cube3_pdb_index(kind, (c,), rows, row_kind) for c in range(c3.SLOTS[kind][0])], 1)
               for kind in (c3.CORNERS, c3.EDGES)}
        assert all(v.min() >= 0 and v.max() < 24 for v in loc.values())
        for n in (1, 3, ALL):
            want = np.zeros(len(rows), np.int64)
            for (kind, cubies), table in zip(patterns, tables):
                for s, source in images(kind, cubies, n):
                    mapped = np.stack([location_map(s, kind, c)[loc[kind][:, c]] for c in source], 1)
                    idx = clamped_rank(kind, mapped)
                    assert idx.min() >= 0 and idx.max() < table.size
                    want = np.maximum(want, table[idx])
            assert (host_eval(rows, row_kind, patterns, n, tables) == want).all(), (patterns, row_kind, n)


# ------------------------------------------------------------------------------------------------ IDA*
@lru_cache(maxsize=None)
def ida_lookups(n):
    """IDA_SET's look-ups over the first n images as plain Python: [(kind, source cubies, their location maps, table)]."""
    out = []
    for (kind, cubies), table in zip(IDA_SET, tables_of(IDA_SET)):
        for s, source in images(kind, cubies, n):
            out.append((kind, source, [location_map(s, kind, c).tolist() for c in source], table))
    return out


def h_of(n):
    """h as a callable on (corner locations, edge locations): the header's rank rule in plain integers over the look-ups."""
    lookups = ida_lookups(n)

    def h(state):
        best = 0
        for kind, source, maps, table in lookups:
            nn, o = c3.SLOTS[kind]
            rank = orient = 0
            slots = []
            for j, c in enumerate(source):
                s, r = divmod(maps[j][state[kind][c]], o)
                rank = rank * (nn - j) + s - sum(1 for x in slots if x < s)
                orient = orient * o + r
                slots.append(s)
            best = max(best, int(table[rank * o ** len(source) + orient]))
        return best
    return h


def root_locations(root):
    return tuple(tuple(int(x) for x in c3.locations_of_states(kind, tuple(range(c3.SLOTS[kind][0])), np.asarray(root)[None])[0])
                 for kind in (c3.CORNERS, c3.EDGES))


def tree(root, h, T):
    """The recursive search at one threshold -> (children generated, the smallest f above T or None)."""
    mv = [[[int(x) for x in row] for row in c3.location_moves(kind)] for kind in (c3.CORNERS, c3.EDGES)]
    acc = [0, None]

    def visit(state, g, m, mp):
        for a in range(12):
            if not ida.cube3_allowed(a, m, mp):
                continue
            child = tuple(tuple(mv[kind][a][x] for x in state[kind]) for kind in (0, 1))
            acc[0] += 1
            f = g + 1 + h(child)
            if f <= T:
                visit(child, g + 1, a, m)
            elif acc[1] is None or f < acc[1]:
                acc[1] = f
    visit(root_locations(root), 0, None, None)
    return acc[0], acc[1]


def exact_search(root, h, stop_at):
    """The thresholds below stop_at and their node counts of the recursive search with h."""
    T, thresholds, counts = h(root_locations(root)), [], []
    while T < stop_at:
        count, T_next = tree(root, h, T)
        thresholds.append(T)
        counts.append(count)
        T = T_next
    return thresholds, counts


def host_search(root, n, max_nodes=ida.BIG, patterns=IDA_SET):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_CUBE3, 0, root, patterns, tables_of(patterns), max_nodes, sym=n)


@pytest.fixture
def prefix():
    """Sets the work items' prefix depth for one test and puts the default back."""
    from deepcubea_amd import _lib
    yield _lib.idastar_set_prefix
    _lib.idastar_set_prefix(-1)


@lru_cache(maxsize=None)
def ida_reference(case):
    root = ida.cube3_suffix_root(*case)
    return root, exact_search(root, h_of(1), case[1]), exact_search(root, h_of(ALL), case[1])


@pytest.mark.parametrize("case", list(IDA_CASES), ids=lambda c: "root%d-%d" % c)
def test_the_recursive_search_gives_the_recorded_counts(case):
    _, plain, full = ida_reference(case)
    assert plain == IDA_CASES[case][0] and full == IDA_CASES[case][1]


@pytest.mark.parametrize("depth", [-1, 0, 2, 3])
@pytest.mark.parametrize("case", list(IDA_CASES), ids=lambda c: "root%d-%d" % c)
def test_host_idastar_on_all_images_keeps_the_contract(case, depth, prefix):
    root, plain, full = ida_reference(case)
    prefix(depth)
    res = host_search(root, ALL)
    k = case[1]
    assert res["solved"] and len(res["moves"]) == k and res["nodes_generated"] == sum(res["nodes_per_threshold"])
    assert (ida.replay_cube3(root, res["moves"]) == np.arange(54)).all()
    thresholds, counts = res["thresholds"], res["nodes_per_threshold"]
    assert thresholds[:-1] == IDA_CASES[case][1][0] and counts[:-1] == IDA_CASES[case][1][1]
    # the contract, against the recursive search with h as a callable
    h = h_of(ALL)
    assert all(a < b for a, b in zip(thresholds, thresholds[1:]))
    assert thresholds[0] == h(root_locations(root)) and thresholds[-1] == k
    assert set(full[0]) <= set(thresholds)
    for T, count in zip(thresholds[:-1], counts[:-1]):
        assert count == tree(root, h, T)[0], T
        assert count <= tree(root, h_of(1), T)[0], T  # never more than the plain search's tree at that threshold


@pytest.mark.parametrize("case", list(IDA_CASES), ids=lambda c: "root%d-%d" % c)
def test_host_idastar_with_one_image_is_the_plain_search(case, prefix):
    root, plain, _ = ida_reference(case)
    for depth in (-1, 3):
        prefix(depth)
        one, ref = host_search(root, 1), ida.host_cube3(root, IDA_SET, tables_of(IDA_SET))
        assert one["thresholds"] == ref["thresholds"] and one["nodes_per_threshold"][:-1] == ref["nodes_per_threshold"][:-1]
        assert one["thresholds"][:-1] == plain[0] and one["nodes_per_threshold"][:-1] == plain[1]
        assert one["solved"] and len(one["moves"]) == case[1]


def test_host_idastar_between_one_and_all_images_and_the_budget(prefix):
    root, _, full = ida_reference((2, 7))
    h = h_of(3)
    res = host_search(root, 3)
    assert res["solved"] and len(res["moves"]) == 7 and res["thresholds"][0] == h(root_locations(root))
    for T, count in zip(res["thresholds"][:-1], res["nodes_per_threshold"][:-1]):
        assert count == tree(root, h, T)[0]
    out = host_search(root, ALL, max_nodes=20)  # the budget ends inside threshold 6 (31 nodes): never "solved" on a lie
    assert not out["solved"] and out["status"] == "budget exhausted" and out["moves"] == []
    assert 20 < out["nodes_generated"] <= 20 + 20 // 2 and out["thresholds"] == [6]  # the header's bound: one lane, interval 20 / 2
    goal = host_search(np.arange(54, dtype=np.uint8), ALL)
    assert goal["solved"] and goal["moves"] == [] and goal["thresholds"] == []
    dead = [t.copy() for t in tables_of(IDA_SET)]  # the root is dead if ANY look-up's byte is 0xFE: here one of an image alone
    from deepcubea_amd import _lib
    lk = ida_lookups(ALL)[5]
    state = root_locations(root)
    kind, o = lk[0], c3.SLOTS[lk[0]][1]
    idx = int(c3.rank_locations(kind, np.array([[lk[2][j][state[kind][c]] for j, c in enumerate(lk[1])]]))[0])
    plain_idx = int(c3.host_index(kind, IDA_SET[0][1], root[None], c3.ROWS_STATE)[0])
    assert kind == c3.CORNERS and idx != plain_idx
    dead[0][idx] = 0xFE
    res = _lib.idastar_host(_lib.ENV_CUBE3, 0, root, IDA_SET, dead, ida.BIG, sym=ALL)
    assert res["status"] == "unsolvable" and res["thresholds"] == []
    assert _lib.idastar_host(_lib.ENV_CUBE3, 0, root, IDA_SET, dead, ida.BIG, sym=1)["solved"]


# ------------------------------------------------------------------------------------------------ refusals, spec, CLI, ABI
def raw_eval(patterns, max_images, tables=None, n=1):
    from deepcubea_amd import _lib
    L = _lib.lib()
    kinds = np.array([k for k, _ in patterns], np.int32)
    ids = np.array([c for _, g in patterns for c in g], np.uint8)
    ks = np.array([len(g) for _, g in patterns], np.int32)
    tables = tables_of(patterns) if tables is None else tables
    ptrs = (C.c_void_p * len(patterns))(*[t.ctypes.data for t in tables])
    rows, out = np.arange(54, dtype=np.uint8)[None].copy(), np.full(1, -3.0, np.float32)
    rc = L.dca_cube3_pdb_eval_sym_host(rows.ctypes.data, n, 54, 0, len(patterns), kinds.ctypes.data, ids.ctypes.data, ks.ctypes.data, ptrs,
                                       max_images, out.ctypes.data)
    return rc, L.dca_last_error(), float(out[0])


def test_library_refusals_without_a_device():
    from deepcubea_amd import _lib
    L = _lib.lib()
    small = (c3.SMALL["c0,c1,c2"],)
    for bad in (0, -1, 49, 1 << 20):
        rc, msg, out = raw_eval(small, bad)
        assert rc == -1 and msg.startswith(b"bad argument: dca_cube3_pdb_eval_sym_host") and b"max_images" in msg and out == -3.0
        if bad:  # (the wrapper's sym=0 is the plain search)
            with pytest.raises(_lib.DcaError, match="max_images"):
                host_search(ida.cube3_suffix_root(0, 7), bad)
        with pytest.raises(_lib.DcaError, match="max_images"):
            _lib.cube3_sym_images(c3.CORNERS, (0, 1, 2), bad)
    assert raw_eval(small, 48)[0] == 0 and raw_eval(small, 1)[2] == 0.0
    # three patterns of 24 images each: 72 look-ups, over the cap; + sym:21 fits (63)
    three = (c3.SMALL["c0,c1,c2"], (c3.CORNERS, (5, 6, 7)), (c3.CORNERS, (1, 2, 4)))
    assert [len(images(*p)) for p in three] == [24, 24, 24]
    tables = [c3.host_table(*three[0])] * 3  # (sizes alone matter here)
    rc, msg, out = raw_eval(three, 48, tables)
    assert rc == -1 and b"72 look-ups" in msg and b"DCA_CUBE3_SYM_MAX_LOOKUPS = 64" in msg and b"+sym:N" in msg and out == -3.0
    assert raw_eval(three, 21, tables)[0] == 0 and raw_eval(three, 22, tables)[0] == -1
    with pytest.raises(_lib.DcaError, match=r"\+sym:N"):
        _lib.idastar_host(_lib.ENV_CUBE3, 0, np.arange(54, dtype=np.uint8), three, tables, 100, sym=48)
    # what the plain entry points refuse in a pattern set
    for patterns, word in ((((2, (0,)),), b"kind"), (((0, (0, 0)),), b"appears twice"), (((1, (12,)),), b"cubie 12")):
        rc, msg, _ = raw_eval(patterns, 48, [np.zeros(16, np.uint8)])
        assert rc == -1 and word in msg, msg
    assert L.dca_cube3_sym_tables(None, None) == -1 and b"sticker_perms" in L.dca_last_error()
    with pytest.raises(ValueError, match="cube3 only"):
        _lib.idastar_host(_lib.ENV_NPUZZLE, 3, np.arange(9, dtype=np.uint8), ((1, 2),), [np.zeros(729, np.uint8)], 10, sym=2)


@pytest.fixture
def no_device(monkeypatch):
    """Any touch of the device raises."""
    import torch
    from deepcubea_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "require_gpu", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_stream", boom)


def test_spec_suffix_and_its_refusals(no_device):
    from deepcubea_amd.utils import cube3_pdb as cp
    from deepcubea_amd.utils import pattern_db as pd
    assert cp.split_sym("korf") == ("korf", 0) and cp.split_sym(" korf7 + SYM ") == ("korf7", 48)
    assert cp.split_sym("c0,c1/e1+sym:5") == ("c0,c1/e1", 5) and cp.split_sym("korf+sym: 48") == ("korf", 48)
    korf = cp.Cube3PatternDatabase("korf")
    for spec, sym, suffix in (("korf+sym", 48, "+sym"), ("korf+sym:48", 48, "+sym"), ("korf+sym:24", 24, "+sym:24"), ("korf+sym:1", 1, "+sym:1"),
                              ("korf7+sym:2", 2, "+sym:2")):
        pdb = cp.Cube3PatternDatabase(spec)
        assert pdb.sym == sym and pdb.spec == cp.Cube3PatternDatabase(spec.split("+")[0]).spec + suffix
        assert pdb.bytes == cp.Cube3PatternDatabase(spec.split("+")[0]).bytes  # no table bytes
        assert cp.Cube3PatternDatabase(pdb.spec).sym == sym and cp.Cube3PatternDatabase(pdb.spec).patterns == pdb.patterns
    assert korf.sym == 0 and "+" not in korf.spec
    assert cp.Cube3PatternDatabase(korf.patterns, sym=8).spec == korf.spec + "+sym:8"
    assert cp.sym_lookups(cp.PRESETS["korf"], 48) == 49 == cp.sym_lookups(cp.PRESETS["korf7"], 48)
    assert cp.sym_lookups(cp.PRESETS["korf"], 8) == 17 and cp.sym_lookups(cp.PRESETS["korf"], 1) == 3
    with pytest.raises(ValueError, match="parser"):  # the parser itself is unchanged and takes no suffix
        try:
            cp.parse_cube3_pdb_spec("korf+sym")
        except ValueError as err:
            assert "suffix" in str(err)
            raise ValueError("parser")
    for spec in ("korf+sym+sym", "korf+sym:0", "korf+sym:49", "korf+sym:-1", "korf+sym:", "korf+sym:x", "korf+symm", "korf+sym:1:2",
                 "korf+", "+sym", "korf+sym+reflect", "korf+reflect+sym", "bogus+sym"):
        with pytest.raises(ValueError):
            cp.Cube3PatternDatabase(spec)
    with pytest.raises(ValueError, match="a suffix such as \\+reflect is defined for the sliding puzzles only"):  # today's message
        cp.Cube3PatternDatabase("korf+reflect")
    for sym in (-1, 49):
        with pytest.raises(ValueError):
            cp.Cube3PatternDatabase("korf", sym=sym)
    over = "c0,c1,c2/c5,c6,c7/c1,c2,c4"
    with pytest.raises(ValueError, match=r"72 look-ups.*cap of 64.*\+sym:N"):
        cp.Cube3PatternDatabase(over + "+sym")
    assert cp.Cube3PatternDatabase(over + "+sym:21").sym == 21
    for env in ("puzzle15", "puzzle8"):  # +sym on a puzzle
        with pytest.raises(ValueError):
            pd.PatternDatabase(env, "auto+sym")


def test_npz_round_trips_the_suffix_and_old_files_load_as_plain(tmp_path, no_device):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    patterns = (c3.SMALL["c0,c1,c2"], (c3.EDGES, (11, 0)))
    tables = tables_of(patterns)
    for sym, suffix in ((48, "+sym"), (5, "+sym:5"), (0, "")):
        path = str(tmp_path / ("c3_%d.npz" % sym))
        Cube3PatternDatabase(patterns, sym=sym).save(path, tables=tables)
        back, got = Cube3PatternDatabase.load_host(path)
        assert back.sym == sym and back.patterns == patterns and back.spec == "c0,c1,c2/e11,e0" + suffix
        assert all(np.array_equal(g, t) for g, t in zip(got, tables))
    old = str(tmp_path / "old.npz")  # a file as it was written before the suffix existed
    np.savez(old, table_0=tables[0], table_1=tables[1], env_name=np.array("cube3"), partition=np.array("c0,c1,c2/e11,e0"))
    assert Cube3PatternDatabase.load_host(old)[0].sym == 0


def test_cli_refusals_and_help_touch_no_device(no_device):
    from deepcubea_amd.search_methods import astar, idastar
    for module in (astar, idastar):
        help_text = " ".join({a.dest: a for a in module.build_parser()._actions}["model_dir"].help.split())
        assert "SPEC+sym" in help_text and "SPEC+sym:N" in help_text and "SPEC+reflect" in help_text
    for model in ("pdb:korf+sym:0", "pdb:korf+sym+sym", "pdb:korf+reflect", "pdb:c0,c1,c2/c5,c6,c7/c1,c2,c4+sym", "pdb:korf+sym:49"):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env="cube3"), None)
        with pytest.raises(ValueError):
            idastar.pattern_database(SimpleNamespace(model_dir=model, env="cube3"))
    for env in ("puzzle8", "puzzle15", "puzzle24"):
        with pytest.raises(ValueError, match="cube3 only"):  # refused with the reason
            idastar.pattern_database(SimpleNamespace(model_dir="pdb:auto+sym", env=env))
        with pytest.raises(ValueError, match="cube3 only"):
            idastar.pattern_database(SimpleNamespace(model_dir="pdb:auto+sym:4", env=env))
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir="pdb:auto+sym", env=env), None)
        assert idastar.pattern_database(SimpleNamespace(model_dir="pdb:auto+reflect", env=env)).reflect
    pdb = idastar.pattern_database(SimpleNamespace(model_dir="pdb:korf+sym:8", env="cube3"))
    assert pdb.sym == 8 and pdb.spec.endswith("+sym:8")
    assert idastar.DEFAULT_MAX_NODES == {"puzzle": int(60 * 1.14e8), "cube3": int(60 * 8.52e9)}


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    L = _lib.lib()
    product = open(os.path.join(ROOT, "include", "dca.h")).read()
    debug = open(os.path.join(ROOT, "include", "dca_debug.h")).read()
    for names, hdr in ((NEW_PRODUCT, product), (NEW_DEBUG, debug)):
        declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
        for name in names:
            assert name in declared and name in _lib._SIGNATURES and name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    assert "#define DCA_ABI_VERSION 6" in product and L.dca_abi_version() == 6
    assert "#define DCA_CUBE3_SYMS 48\n" in product and "#define DCA_CUBE3_SYM_MAX_LOOKUPS 64\n" in product
    assert (_lib.CUBE3_SYMS, _lib.CUBE3_SYM_MAX_LOOKUPS) == (ALL, CAP)
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    assert list(L.dca_cube3_pdb_eval_sym.argtypes) == [p, i64, i64, i, i, p, p, p, p, i, p, p]
    assert list(L.dca_cube3_pdb_eval_sym_host.argtypes) == [p, i64, i64, i, i, p, p, p, p, i, p]
    assert list(L.dca_idastar_cube3_sym.argtypes) == [p, i, p, p, p, p, i, i64, p, p, p, i, p, p, p, i, p, p]
    assert list(L.dca_idastar_host_sym.argtypes) == [p, i, p, p, p, p, i, i64, p, p, p, i, p, p, p, i, p]
    assert list(L.dca_cube3_sym_tables.argtypes) == [p, p] and list(L.dca_cube3_sym_images.argtypes) == [i, p, i, i, p, p, p, p]
    flat = re.sub(r"\s*\n \*\s*", " ", product)  # the header states the order and the contract
    for phrase in ("ascending lexicographic order of (phi(0), phi(1), ..., phi(5)); symmetry 0 is the identity",
                   "perm[pi(a)][sigma(i)] = sigma(perm[a][i])", "S'[sigma(p)] = sigma(S[p])", "R[move_a(l)] = move_pi(a)(R[l])",
                   "the pattern itself (the identity) first", "the thresholds increase strictly",
                   "every threshold of the exact search", "a property of the tree"):
        assert phrase in flat, phrase
