"""CPU-side tests of the cube3 pattern databases (dca_cube3_pdb_*, deepcubea_amd/utils/cube3_pdb.py, `--env cube3 --model_dir
pdb:<spec>`): the cubie numbering, the table size as a pure function, the index rule on the 21 637 states of the shipped optimal
paths, the any-bytes rule, the spec parser, the CLI's refusals and the .npz round trip.  No GPU needed.

This file also holds the HOST REFERENCE the GPU tests compare against (tests/test_cube3_pdb_hip.py imports it), written from
include/dca.h's rules: the cubies derived from dca_cube3_perm_table, the index rule in numpy, and a breadth-first table builder
over abstract states."""
import ctypes as C
import os
import re
from functools import lru_cache
from math import perm
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_cube3_pdb_bytes", "dca_cube3_pdb_cubies", "dca_cube3_pdb_index", "dca_cube3_pdb_build", "dca_cube3_pdb_eval")
CORNERS, EDGES = 0, 1
ROWS_STATE, ROWS_NNET = 0, 1
UNREACHED = 0xFE
SLOTS = {CORNERS: (8, 3), EDGES: (12, 2)}
CORNER_LISTS = [[0, 26, 47], [2, 20, 44], [6, 29, 53], [8, 35, 38], [9, 18, 42], [11, 24, 45], [15, 33, 36], [17, 27, 51]]
EDGE_LISTS = [[1, 23], [3, 50], [5, 41], [7, 32], [10, 21], [12, 39], [14, 48], [16, 30], [19, 43], [25, 46], [28, 52], [34, 37]]
# the patterns the tests use: name -> (kind, cubies)
SMALL = {"c0,c1,c2": (CORNERS, (0, 1, 2)), "c4,c5,c6,c7": (CORNERS, (4, 5, 6, 7)), "e0,e1,e2,e3": (EDGES, (0, 1, 2, 3)),
         "e8,e9,e10,e11": (EDGES, (8, 9, 10, 11))}
HISTOGRAMS = {"c0,c1,c2": [1, 10, 78, 484, 2082, 4272, 2076, 69],
              "e0,e1,e2,e3": [1, 10, 73, 500, 3078, 15528, 57180, 91654, 21849, 207],
              "c4,c5,c6,c7": [1, 10, 93, 704, 4114, 18514, 50344, 48812, 13296, 192],
              "e8,e9,e10,e11": [1, 8, 76, 592, 3666, 18428, 63128, 87164, 16961, 56]}


# ------------------------------------------------------------------------------------------------ the host reference
@lru_cache(maxsize=None)
def perm_table():
    from deepcubea_amd import _lib
    p = _lib.lib().dca_cube3_perm_table()
    t = np.array([p[i] for i in range(12 * 54)], np.int64).reshape(12, 54)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def cubie_lists(kind):
    """Two positions belong to one cubie exactly when the same set of moves displaces them; positions ascending, cubies by
    their smallest position."""
    moved = (perm_table() != np.arange(54)).T  # [54, 12]
    classes = {}
    for i in range(54):
        classes.setdefault(tuple(moved[i]), []).append(i)
    size = SLOTS[kind][1]
    return sorted(sorted(c) for c in classes.values() if len(c) == size)


@lru_cache(maxsize=None)
def position_location(kind):
    """sticker position -> slot * o + r (-1 for positions of the other kind and the centres)."""
    o = SLOTS[kind][1]
    loc = np.full(54, -1, np.int64)
    for s, lst in enumerate(cubie_lists(kind)):
        for r, p in enumerate(lst):
            loc[p] = s * o + r
    return loc


@lru_cache(maxsize=None)
def location_moves(kind):
    """[12, n * o]: where a location goes under each move (next[i] = cur[perm[a][i]]: the facelet at perm[a][i] goes to i)."""
    loc = position_location(kind)
    mv = np.full((12, 24), -1, np.int64)
    for a in range(12):
        for i in range(54):
            if loc[i] >= 0:
                mv[a, loc[perm_table()[a, i]]] = loc[i]
    assert (np.sort(mv, 1) == np.arange(24)).all()
    return mv


def locations_of_states(kind, cubies, states):
    """[m, k] locations from sticker-id rows: where the cubie's reference facelet (home = its smallest position) is."""
    states = np.asarray(states)
    where = np.argsort(states, 1)  # where[i, sticker] = its position (rows are permutations of 0..53)
    ref = [cubie_lists(kind)[c][0] for c in cubies]
    return position_location(kind)[where[:, ref]]


def locations_of_colours(kind, cubies, colours):
    """[m, k] locations from colour rows: a cubie is recognised by its colour set, oriented by where its reference colour sits."""
    colours = np.asarray(colours).astype(np.int64)
    n, o = SLOTS[kind]
    lists = np.array(cubie_lists(kind))                       # [n, o] positions
    on_slot = colours[:, lists]                               # [m, n, o]
    sets = (1 << on_slot).sum(2)                              # [m, n] colour set per slot
    out = np.zeros((len(colours), len(cubies)), np.int64)
    for j, c in enumerate(cubies):
        home = lists[c] // 9
        slot = np.argmax(sets == (1 << home).sum(), 1)
        assert (sets[np.arange(len(colours)), slot] == (1 << home).sum()).all()
        r = np.argmax(on_slot[np.arange(len(colours)), slot] == home[0], 1)
        out[:, j] = slot * o + r
    return out


def rank_locations(kind, locs):
    """include/dca.h index rule on [m, k] locations -> int64 [m]."""
    n, o = SLOTS[kind]
    locs = np.asarray(locs, np.int64)
    k = locs.shape[1]
    s, r = locs // o, locs % o
    rank = np.zeros(len(locs), np.int64)
    orient = np.zeros(len(locs), np.int64)
    for j in range(k):
        d = s[:, j] - (s[:, :j] < s[:, j:j + 1]).sum(1)
        rank = rank * (n - j) + d
        orient = orient * o + r[:, j]
    return rank * o ** k + orient


def unrank_locations(kind, idx, k):
    n, o = SLOTS[kind]
    idx = np.asarray(idx, np.int64)
    r = np.zeros((len(idx), k), np.int64)
    d = np.zeros((len(idx), k), np.int64)
    rest = idx.copy()
    for j in range(k - 1, -1, -1):
        r[:, j] = rest % o
        rest //= o
    for j in range(k - 1, -1, -1):
        d[:, j] = rest % (n - j)
        rest //= n - j
    assert (rest == 0).all()
    free = np.ones((len(idx), n), bool)  # slot j = the d_j-th slot still free
    s = np.zeros_like(d)
    rows = np.arange(len(idx))
    for j in range(k):
        order = np.cumsum(free, 1) - 1
        s[:, j] = np.argmax(free & (order == d[:, j:j + 1]), 1)
        free[rows, s[:, j]] = False
    return s * o + r


def table_size(kind, k):
    n, o = SLOTS[kind]
    return perm(n, k) * o ** k


@lru_cache(maxsize=None)
def _host_table(kind, cubies):
    k, o = len(cubies), SLOTS[kind][1]
    mv = location_moves(kind)
    table = np.full(table_size(kind, k), UNREACHED, np.uint8)
    front = rank_locations(kind, np.array([[c * o for c in cubies]]))
    table[front] = 0
    depth = 0
    while len(front):
        depth += 1
        locs = unrank_locations(kind, front, k)
        nxt = np.unique(np.concatenate([rank_locations(kind, mv[a][locs]) for a in range(12)]))
        front = nxt[table[nxt] == UNREACHED]
        table[front] = depth
    table.setflags(write=False)
    return table


def host_table(kind, cubies):
    """One pattern's table by the header's rules, computed once per pattern and never written to."""
    return _host_table(int(kind), tuple(int(c) for c in cubies))


def host_index(kind, cubies, rows, row_kind):
    f = locations_of_states if row_kind == ROWS_STATE else locations_of_colours
    return rank_locations(kind, f(kind, tuple(cubies), rows))


def host_eval(rows, row_kind, patterns, tables):
    """dca_cube3_pdb_eval on the host for rows that ARE cube states: the max of the tables' bytes at the header's index."""
    best = np.zeros(len(rows), np.int64)
    for (kind, cubies), table in zip(patterns, tables):
        if len(rows):
            best = np.maximum(best, np.asarray(table)[host_index(kind, cubies, rows, row_kind)])
    return best.astype(np.float32)


@lru_cache(maxsize=None)
def path_states():
    """The states along the 1000 shipped optimal solutions: (states [21637, 54] sticker ids, remaining distance [21637],
    is_last [21637]: the row is its path's goal end, so row i + 1 is NOT its successor).  Every suffix of an optimal solution is
    optimal: the remaining distance is exact."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    roots, moves, lens = z["cube3_test_states"], z["cube3_test_opt_moves"], z["cube3_test_opt_len"]
    p = perm_table()
    states, dist, last = [], [], []
    for root, mv, L in zip(roots, moves, lens):
        cur = root.astype(np.uint8)
        for t in range(int(L) + 1):
            states.append(cur)
            dist.append(int(L) - t)
            last.append(t == int(L))
            if t < L:
                cur = cur[p[int(mv[t])]]
        assert (cur == np.arange(54)).all()
    states, dist, last = np.array(states, np.uint8), np.array(dist, np.int64), np.array(last, bool)
    assert states.shape == (21637, 54) and dist.max() == 22
    for a in (states, dist, last):
        a.setflags(write=False)
    return states, dist, last


def scrambles(count, moves, seed):
    rng = np.random.default_rng(seed)
    p = perm_table()
    states = np.tile(np.arange(54, dtype=np.uint8), (count, 1))
    rows = np.arange(count)[:, None]
    for _ in range(moves):
        states = states[rows, p[rng.integers(0, 12, count)]]
    return states


# ------------------------------------------------------------------------------------------------ cubies, sizes
def test_cubies_equal_the_derivation_and_the_documented_lists():
    from deepcubea_amd import _lib
    assert cubie_lists(CORNERS) == CORNER_LISTS and cubie_lists(EDGES) == EDGE_LISTS
    assert _lib.cube3_pdb_cubies(_lib.CUBE3_CORNERS).tolist() == CORNER_LISTS
    assert _lib.cube3_pdb_cubies(_lib.CUBE3_EDGES).tolist() == EDGE_LISTS
    L = _lib.lib()
    buf = np.full(24, 0x5A, np.uint8)
    assert L.dca_cube3_pdb_cubies(2, buf.ctypes.data_as(C.c_void_p)) == -1 and (buf == 0x5A).all()
    assert L.dca_last_error().startswith(b"bad argument: dca_cube3_pdb_cubies") and b"kind" in L.dca_last_error()
    assert L.dca_cube3_pdb_cubies(0, None) == -1 and b"positions" in L.dca_last_error()
    with pytest.raises(ValueError):
        _lib.cube3_pdb_cubies(2)


def test_table_bytes_is_a_pure_function_with_limits():
    from deepcubea_amd import _lib
    L2 = C.CDLL(_lib.LIB_PATH)  # a second handle: no shared Python state
    L2.dca_cube3_pdb_bytes.restype, L2.dca_cube3_pdb_bytes.argtypes = C.c_int64, [C.c_int, C.c_int]
    L2.dca_last_error.restype = C.c_char_p
    for kind, (n, o) in SLOTS.items():
        for k in range(1, 9):
            want = perm(n, k) * o ** k
            assert want <= 1 << 34 and _lib.cube3_pdb_bytes(kind, k) == want == L2.dca_cube3_pdb_bytes(kind, k), (kind, k)
    assert _lib.cube3_pdb_bytes(CORNERS, 8) == 264539520 == 40320 * 6561
    assert _lib.cube3_pdb_bytes(EDGES, 6) == 42577920 and _lib.cube3_pdb_bytes(EDGES, 7) == 510935040
    assert _lib.cube3_pdb_bytes(EDGES, 8) == 5109350400
    for kind, k, word in ((2, 1, b"kind"), (-1, 1, b"kind"), (0, 0, b"k = 0"), (1, 0, b"k = 0"), (0, 9, b"k = 9"), (1, 9, b"k = 9"),
                          (1, -1, b"k = -1"), (1, 12, b"k = 12")):
        assert L2.dca_cube3_pdb_bytes(kind, k) == -1, (kind, k)
        msg = L2.dca_last_error()
        assert msg.startswith(b"bad argument: dca_cube3_pdb_bytes") and word in msg, msg
        with pytest.raises(_lib.DcaError):
            _lib.cube3_pdb_bytes(kind, k)


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    assert L.dca_cube3_pdb_bytes.restype is i64 and list(L.dca_cube3_pdb_bytes.argtypes) == [i, i]
    assert list(L.dca_cube3_pdb_cubies.argtypes) == [i, p]
    assert list(L.dca_cube3_pdb_index.argtypes) == [i, p, i, p, i, p]
    assert list(L.dca_cube3_pdb_build.argtypes) == [i, p, i, p, p, p]
    assert list(L.dca_cube3_pdb_eval.argtypes) == [p, i64, i64, i, i, p, p, p, p, p, p]
    for name, value in (("DCA_CUBE3_CORNERS", _lib.CUBE3_CORNERS), ("DCA_CUBE3_EDGES", _lib.CUBE3_EDGES),
                        ("DCA_ROWS_STATE", _lib.ROWS_STATE), ("DCA_ROWS_NNET", _lib.ROWS_NNET)):
        assert "#define %s %d\n" % (name, value) in hdr
    assert (_lib.CUBE3_CORNERS, _lib.CUBE3_EDGES, _lib.ROWS_STATE, _lib.ROWS_NNET) == (CORNERS, EDGES, ROWS_STATE, ROWS_NNET)
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)  # the header states the rules
    for phrase in ("index rule", "value rule", "colour rule", "any-bytes rule", "combined by MAX", "d_j = s_j - #{i < j : s_i < s_j} in radix n - j",
                   "cubie 0 most significant", "an entry no move sequence reaches holds 0xFE", "deepest level + 1",
                   "Up to 24 patterns", "SYNCHRONISES the stream", "d_j <= n - j - 1"):
        assert phrase in flat, phrase


# ------------------------------------------------------------------------------------------------ the index rule
def test_reference_rank_and_unrank_are_inverse():
    for kind, k in ((CORNERS, 3), (EDGES, 2), (CORNERS, 5)):
        idx = np.arange(table_size(kind, k)) if table_size(kind, k) < 200000 else np.random.default_rng(0).integers(0, table_size(kind, k), 50000)
        locs = unrank_locations(kind, idx, k)
        n, o = SLOTS[kind]
        assert all(len(set(row)) == k for row in (locs[:2000] // o).tolist())
        assert (rank_locations(kind, locs) == idx).all()


@pytest.mark.parametrize("name", list(SMALL) + ["c0,c1,c2,c3,c4,c5,c6,c7", "e11,e0"])
def test_index_equals_the_python_rule_on_the_shipped_path_states(name):
    from deepcubea_amd import _lib
    from deepcubea_amd.utils.cube3_pdb import parse_cube3_pdb_spec
    (kind, cubies), = parse_cube3_pdb_spec(name)
    states, dist, _ = path_states()
    want = host_index(kind, cubies, states, ROWS_STATE)
    assert (want == host_index(kind, cubies, states // 9, ROWS_NNET)).all()  # the two readings of the reference agree
    assert want.min() >= 0 and want.max() < table_size(kind, len(cubies))
    assert (_lib.cube3_pdb_index(kind, cubies, states, _lib.ROWS_STATE) == want).all()
    assert (_lib.cube3_pdb_index(kind, cubies, states // 9, _lib.ROWS_NNET) == want).all()
    goal = rank_locations(kind, np.array([[c * SLOTS[kind][1] for c in cubies]]))[0]
    assert (want[dist == 0] == goal).all()


def test_index_reaches_every_entry_of_a_small_pattern_on_random_scrambles():
    from deepcubea_amd import _lib
    kind, cubies = SMALL["c0,c1,c2"]
    states = scrambles(200000, 40, 1)
    got = _lib.cube3_pdb_index(kind, cubies, states, _lib.ROWS_STATE)
    assert (got == host_index(kind, cubies, states, ROWS_STATE)).all()
    assert len(np.unique(got)) == 9072 == table_size(kind, 3)
    some = states[:5000]
    assert (_lib.cube3_pdb_index(kind, cubies, some // 9, _lib.ROWS_NNET) == got[:5000]).all()


def test_any_bytes_give_an_index_inside_the_table():
    from deepcubea_amd import _lib
    rows = np.random.default_rng(7).integers(0, 256, (10000, 54)).astype(np.uint8)
    rows[0], rows[1], rows[2] = 0, 0xFF, 5
    rows[3:2000] %= 54   # rows of valid bytes that are no cube states: duplicate and missing cubies
    rows[2000:4000] %= 6
    for kind, cubies in ((CORNERS, tuple(range(8))), (CORNERS, (7, 3, 0)), (EDGES, tuple(range(4, 12))), (EDGES, (11,)),
                         (EDGES, (3, 9, 0, 5, 1))):
        for row_kind in (_lib.ROWS_STATE, _lib.ROWS_NNET):
            idx = _lib.cube3_pdb_index(kind, cubies, rows, row_kind)
            assert idx.min() >= 0 and idx.max() < table_size(kind, len(cubies)), (kind, cubies, row_kind)


def test_index_refusals():
    from deepcubea_amd import _lib
    L = _lib.lib()
    row = np.arange(54, dtype=np.uint8)
    out = C.c_int64(-7)

    def call(kind=0, cubies=(0, 1), k=None, row_=row, row_kind=0, index=out):
        c = np.array(cubies, np.uint8)
        return L.dca_cube3_pdb_index(kind, c.ctypes.data_as(C.c_void_p), len(cubies) if k is None else k,
                                     None if row_ is None else row_.ctypes.data_as(C.c_void_p), row_kind,
                                     None if index is None else C.byref(index))

    for fn, word in ((lambda: call(kind=2), b"kind"), (lambda: call(k=0), b"k = 0"), (lambda: call(cubies=(0,) * 9), b"k = 9"),
                     (lambda: call(cubies=(0, 8)), b"cubie 8"), (lambda: call(kind=1, cubies=(12,)), b"cubie 12"),
                     (lambda: call(cubies=(3, 1, 3)), b"cubie 3 appears twice"), (lambda: call(row_=None), b"row"),
                     (lambda: call(row_kind=2), b"row_kind"), (lambda: call(index=None), b"index")):
        assert fn() == -1, word
        msg = L.dca_last_error()
        assert msg.startswith(b"bad argument: dca_cube3_pdb_index") and word in msg, (word, msg)
    assert out.value == -7
    assert call() == 0 and out.value == 0  # the goal row: index of (c0 home, c1 home) is not 0 in general, but c0,c1 are slots 0,1
    assert call(kind=1, cubies=(11,)) == 0 and out.value == 22


# ------------------------------------------------------------------------------------------------ the reference tables
@pytest.mark.parametrize("name", list(SMALL))
def test_host_reference_tables_have_the_known_histograms(name):
    kind, cubies = SMALL[name]
    t = host_table(kind, cubies)
    assert t.size == sum(HISTOGRAMS[name]) == table_size(kind, len(cubies))
    assert int((t == UNREACHED).sum()) == 0
    assert np.bincount(t).tolist() == HISTOGRAMS[name]


def test_max_of_the_reference_tables_is_admissible_and_consistent_on_the_paths():
    states, dist, last = path_states()
    patterns = list(SMALL.values())
    h = host_eval(states, ROWS_STATE, patterns, [host_table(*p) for p in patterns]).astype(np.int64)
    assert (h <= dist).all() and (h[dist == 0] == 0).all() and int((h == dist).sum()) == 6258
    step = np.abs(h[1:] - h[:-1])[~last[:-1]]
    assert len(step) == 20637 and step.max() <= 1


# ------------------------------------------------------------------------------------------------ spec parser, CLI, .npz
def test_presets_and_their_byte_counts():
    from deepcubea_amd.utils import cube3_pdb as cp
    assert sorted(cp.PRESETS) == ["corners", "korf", "korf7"]
    c8 = tuple(range(8))
    assert cp.parse_cube3_pdb_spec("corners") == ((CORNERS, c8),)
    assert cp.parse_cube3_pdb_spec("korf") == ((CORNERS, c8), (EDGES, (0, 1, 2, 3, 4, 5)), (EDGES, (6, 7, 8, 9, 10, 11)))
    assert cp.parse_cube3_pdb_spec("Korf7") == ((CORNERS, c8), (EDGES, (0, 1, 2, 3, 4, 5, 6)), (EDGES, (5, 6, 7, 8, 9, 10, 11)))
    assert cp.Cube3PatternDatabase("corners").bytes == 264539520
    assert cp.Cube3PatternDatabase("korf").bytes == 349695360 == 264539520 + 2 * 42577920
    assert cp.Cube3PatternDatabase("korf7").bytes == 264539520 + 2 * 510935040
    assert cp.Cube3PatternDatabase("korf").spec == "c0,c1,c2,c3,c4,c5,c6,c7/e0,e1,e2,e3,e4,e5/e6,e7,e8,e9,e10,e11"
    assert cp.parse_cube3_pdb_spec(cp.Cube3PatternDatabase("korf7").spec) == cp.PRESETS["korf7"]


def test_spec_parser_groups_and_refusals():
    from deepcubea_amd.utils import cube3_pdb as cp
    from deepcubea_amd.utils import pattern_db as pd
    assert cp.parse_cube3_pdb_spec("c0,c1,c2/e0,e1,e2,e3") == ((CORNERS, (0, 1, 2)), (EDGES, (0, 1, 2, 3)))
    assert cp.parse_cube3_pdb_spec(" e11 , e0 / c7 ") == ((EDGES, (11, 0)), (CORNERS, (7,)))   # order kept
    assert cp.parse_cube3_pdb_spec("c0,c1/c1,c2") == ((CORNERS, (0, 1)), (CORNERS, (1, 2)))    # patterns may share cubies
    assert cp.parse_cube3_pdb_spec("e0,e1,e2,e3,e4,e5,e6,e7")[0][1] == tuple(range(8))         # 5.1 GB: under the cap
    assert len(cp.parse_cube3_pdb_spec("/".join("e%d" % (i % 12) for i in range(24)))) == 24
    refused = ["auto", "", "c0,e1", "e1,c0", "c0,c0", "e3,e4,e3", "c8", "e12", "c-1", "1,2,3", "0", "c", "c0,,c1", "c0/", "/c0",
               "c0;c1", "x0", "korf8", "4-4", "e0,e1,e2,e3,e4,e5,e6,e7,e8",           # nine edges: k > 8 (and over the cap)
               "/".join("e%d" % (i % 12) for i in range(25))]                          # 25 groups
    for spec in refused:
        with pytest.raises(ValueError):
            cp.parse_cube3_pdb_spec(spec)
        with pytest.raises(ValueError):
            cp.Cube3PatternDatabase(spec)
    with pytest.raises(ValueError, match="corners, korf, korf7"):
        cp.parse_cube3_pdb_spec("auto")
    for bad in ((), ((0, ()),), ((2, (0,)),), ((0, (8,)),), ((1, (0, 0)),), ((1, tuple(range(9))),), ((0, (0,)),) * 25):
        with pytest.raises(ValueError):
            cp.Cube3PatternDatabase(bad)
    # the puzzle module still refuses cube3
    for spec in ("auto", "korf", "c0,c1", "1,2,3"):
        with pytest.raises(ValueError):
            pd.parse_pdb_spec("cube3", spec)
        with pytest.raises(ValueError):
            pd.PatternDatabase("cube3", spec)


def test_cli_parses_the_spec_before_any_device_work():
    """`_load_heuristic` dispatches on the environment and parses first: the ValueError comes on a box without a GPU too."""
    from deepcubea_amd.search_methods import astar
    for env, model in (("cube3", "pdb:auto"), ("cube3", "pdb:c0,e1"), ("cube3", "pdb:5-5-5"), ("cube3", "pdb:1,2,3"),
                       ("cube3", "pdb:e0,e1,e2,e3,e4,e5,e6,e7,e8"), ("lightsout7", "pdb:korf"), ("cube4", "pdb:corners"),
                       ("puzzle15", "pdb:korf"), ("puzzle15", "pdb:c0,c1")):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env=env), None)
    with pytest.raises(ValueError, match="korf"):
        astar._load_heuristic(SimpleNamespace(model_dir="pdb:auto", env="cube3"), None)
    env = SimpleNamespace(get_num_moves=lambda: 12)
    args = SimpleNamespace(instances_per_gpu="auto", model_dir="pdb:korf", batch_size=1000, env="cube3", max_nodes="auto")
    assert astar._is_pdb(args) and astar.auto_instances(args, env, 500, None) == 1
    help_text = " ".join({a.dest: a for a in astar.build_parser()._actions}["model_dir"].help.split())
    assert "korf" in help_text and "c0,c1,c2,c3/e0,e1,e2,e3,e4,e5" in help_text and "pdb:SPEC" in help_text


def test_save_load_round_trip_of_host_made_tables(tmp_path):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    patterns = (SMALL["c0,c1,c2"], (EDGES, (11, 0)))
    tables = [host_table(*p) for p in patterns]
    path = str(tmp_path / "c3.npz")
    Cube3PatternDatabase(patterns).save(path, tables=tables)
    back, got = Cube3PatternDatabase.load_host(path)
    assert back.patterns == patterns and back.spec == "c0,c1,c2/e11,e0" and back.bytes == 9072 + 12 * 11 * 4
    assert len(got) == 2 and all(g.dtype == np.uint8 and np.array_equal(g, t) for g, t in zip(got, tables))
    with pytest.raises(ValueError):  # a table of the wrong size is refused on the way out
        Cube3PatternDatabase(patterns).save(path, tables=[tables[0], tables[0]])
    with pytest.raises(ValueError):
        Cube3PatternDatabase(patterns).save(path, tables=tables[:1])
    with pytest.raises(ValueError):  # a cube3 file is not a puzzle file, and the other way round
        PatternDatabase.load_host(path)
    puzzle = str(tmp_path / "p8.npz")
    PatternDatabase("puzzle8", ((1,),)).save(puzzle, tables=[np.zeros(81, np.uint8)])
    with pytest.raises(ValueError):
        Cube3PatternDatabase.load_host(puzzle)
