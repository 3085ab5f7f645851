"""CPU-side tests of the pattern databases (dca_pdb_*, deepcubea_amd/utils/pattern_db.py, `--model_dir pdb:<spec>`): the ABI
additions and their ctypes signatures, the table size as a pure function, every refusal before any device work, the presets,
the spec parser, auto_instances and the .npz round trip.  No GPU needed.

This file also holds the HOST REFERENCE the GPU tests compare against (tests/test_pdb_hip.py imports it): a 0-1 breadth-first
search with a deque over abstract states, written from include/dca.h's index / cost / 0xFF rules, and the any-bytes rule of
dca_pdb_eval restated in numpy."""
import ctypes as C
import os
import re
from collections import deque
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_pdb_bytes", "dca_pdb_build", "dca_pdb_eval")
NO_STATE, UNREACHABLE = 0xFF, 0xFE


# ------------------------------------------------------------------------------------------------ the host reference
def neighbours(dim):
    """blank position -> the positions a blank move reaches (n_puzzle.py:174-214: U D L R, ineligible moves are no-ops)."""
    out = []
    for z in range(dim * dim):
        i, j = divmod(z, dim)
        out.append([q for ok, q in ((i < dim - 1, z + dim), (i > 0, z - dim), (j < dim - 1, z + 1), (j > 0, z - 1)) if ok])
    return out


@lru_cache(maxsize=None)
def _host_table(dim, tiles):
    N, k = dim * dim, len(tiles)
    nb = neighbours(dim)
    weight = [N ** j for j in range(k + 1)]  # digit 0 = the blank, digit j + 1 = tiles[j]
    table = np.full(N ** (k + 1), NO_STATE, np.uint8)
    # every index whose digits are pairwise distinct is a state: not reached yet
    digits = np.stack(np.unravel_index(np.arange(N ** (k + 1)), (N,) * (k + 1))[::-1], 1)  # column j = digit j
    srt = np.sort(digits, 1)
    table[(srt[:, 1:] != srt[:, :-1]).all(1)] = UNREACHABLE
    goal = (N - 1,) + tuple(t - 1 for t in tiles)
    dist = {goal: 0}
    queue = deque([(0, goal)])
    while queue:
        d, s = queue.popleft()
        if d > dist[s]:
            continue
        blank = s[0]
        for q in nb[blank]:
            if q in s[1:]:  # the blank swaps with a pattern tile: cost 1
                j = s.index(q, 1)
                t = (q,) + s[1:j] + (blank,) + s[j + 1:]
                if d + 1 < dist.get(t, 1 << 30):
                    dist[t] = d + 1
                    queue.append((d + 1, t))
            else:           # with an invisible tile: cost 0
                t = (q,) + s[1:]
                if d < dist.get(t, 1 << 30):
                    dist[t] = d
                    queue.appendleft((d, t))
    idx = np.fromiter((sum(p * w for p, w in zip(s, weight)) for s in dist), np.int64, len(dist))
    val = np.fromiter(dist.values(), np.int64, len(dist))
    assert val.max() < UNREACHABLE and (table[idx] == UNREACHABLE).all()
    table[idx] = val
    table.setflags(write=False)
    return table


def host_table(dim, tiles):
    """One pattern's table by the header's rules, computed once per pattern and never written to."""
    return _host_table(int(dim), tuple(int(t) for t in tiles))


def host_positions(dim, rows, t):
    """The any-bytes rule: the LAST position p < N with row[p] == t, 0 if there is none."""
    N = dim * dim
    hit = np.asarray(rows)[:, :N] == t
    return np.where(hit.any(1), N - 1 - np.argmax(hit[:, ::-1], 1), 0).astype(np.int64)


def host_eval(dim, rows, partition, tables):
    """dca_pdb_eval on the host: the sum of the tables' bytes at the header's index, for ANY row bytes."""
    N = dim * dim
    blank = host_positions(dim, rows, 0)
    total = np.zeros(len(rows), np.int64)
    for tiles, table in zip(partition, tables):
        idx = np.zeros(len(rows), np.int64)
        for t in reversed(tiles):
            idx = idx * N + host_positions(dim, rows, t)
        idx = idx * N + blank
        assert idx.max(initial=0) < len(table)
        total += np.asarray(table)[idx]
    return total.astype(np.float32)


def manhattan_np(dim, rows):
    rows = np.asarray(rows).astype(np.int64)
    N = dim * dim
    pos = np.arange(N)
    goal = rows - 1
    d = np.abs(pos // dim - goal // dim) + np.abs(pos % dim - goal % dim)
    return np.where(rows == 0, 0, d).sum(1)


def test_host_reference_on_known_facts():
    """The reference itself: counts of valid entries, the goal, and one-tile patterns = that tile's Manhattan distance."""
    t = host_table(3, (1, 2, 3, 4))
    assert t.size == 59049 and int((t != NO_STATE).sum()) == 15120 and int((t == UNREACHABLE).sum()) == 0
    goal = 8 + 9 * (0 + 9 * (1 + 9 * (2 + 9 * 3)))
    assert t[goal] == 0 and int((t == 0).sum()) >= 1
    for tile in (1, 5, 8):
        one = host_table(3, (tile,))
        for blank in range(9):
            for p in range(9):
                want = NO_STATE if p == blank else abs(p // 3 - (tile - 1) // 3) + abs(p % 3 - (tile - 1) % 3)
                assert one[blank + 9 * p] == want


# ------------------------------------------------------------------------------------------------ ABI
def _params(hdr, name):
    decl = re.search(r"\b(?:int|int64_t) %s\((.*?)\);" % name, hdr, re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)  # the header states the rules
    for phrase in ("index rule", "cost rule", "0xFF rule", "any-bytes rule", "partition", "the blank is the lowest digit",
                   "swaps with a pattern tile costs 1, with an invisible tile 0", "two digits equal is not a state and holds 0xFF",
                   "the LAST position p < N with row[p] == t, 0 if there is none", "no tile twice across the whole set",
                   "at most 24 patterns", "SYNCHRONISES the stream"):
        assert phrase in flat, phrase
    assert (_lib.PDB_NO_STATE, _lib.PDB_UNREACHABLE, _lib.PDB_MAX_PATTERNS) == (NO_STATE, UNREACHABLE, 24)


def test_ctypes_signatures_match_the_header():
    from deepcubea_amd import _lib
    L = _lib.lib()
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    assert L.dca_pdb_bytes.restype is i64 and list(L.dca_pdb_bytes.argtypes) == [i, i]
    assert _params(hdr, "dca_pdb_bytes") == ["dim", "k"]
    assert L.dca_pdb_build.restype is i and list(L.dca_pdb_build.argtypes) == [i, p, i, p, p, p]
    assert _params(hdr, "dca_pdb_build") == ["dim", "tiles", "k", "table", "sweeps", "stream"]
    assert L.dca_pdb_eval.restype is i and list(L.dca_pdb_eval.argtypes) == [i, p, i64, i64, i, p, p, p, p, p]
    assert _params(hdr, "dca_pdb_eval") == ["dim", "states", "n", "ld", "num_patterns", "tiles", "ks", "tables", "out", "stream"]


def test_table_bytes_is_a_pure_function_with_limits():
    from deepcubea_amd import _lib
    L2 = C.CDLL(_lib.LIB_PATH)  # a second handle: no shared Python state
    L2.dca_pdb_bytes.restype, L2.dca_pdb_bytes.argtypes = C.c_int64, [C.c_int, C.c_int]
    for dim in range(3, 8):
        N = dim * dim
        for k in range(1, N):
            want = N ** (k + 1)
            if want <= 1 << 34:
                assert _lib.pdb_bytes(dim, k) == want == L2.dca_pdb_bytes(dim, k), (dim, k)
            else:
                assert L2.dca_pdb_bytes(dim, k) == -1, (dim, k)
                with pytest.raises(_lib.DcaError):
                    _lib.pdb_bytes(dim, k)
    assert _lib.pdb_bytes(4, 7) == 1 << 32 and _lib.pdb_bytes(3, 8) == 9 ** 9 and _lib.pdb_bytes(5, 6) == 25 ** 7
    for dim, k in ((2, 1), (8, 1), (0, 1), (-3, 1), (3, 0), (3, 9), (3, -1), (4, 8), (4, 16), (5, 7), (6, 6), (7, 6)):
        assert L2.dca_pdb_bytes(dim, k) == -1, (dim, k)
        with pytest.raises(_lib.DcaError):
            _lib.pdb_bytes(dim, k)
    L2.dca_last_error.restype = C.c_char_p
    assert L2.dca_pdb_bytes(8, 1) == -1 and b"dim" in L2.dca_last_error() and b"3..7" in L2.dca_last_error()
    assert L2.dca_pdb_bytes(3, 0) == -1 and b"k = 0" in L2.dca_last_error()


def test_refusals_need_no_device():
    """Every argument check comes before the first device call: DCA_E_BADARG and a message that names the argument."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(64)  # never dereferenced: every call below is refused

    def tiles_of(groups):
        return np.array([t for g in groups for t in g], np.uint8), np.array([len(g) for g in groups], np.int32)

    def build(dim=4, tiles=(1, 2, 3), k=None, table=one):
        t = np.array(tiles, np.uint8)
        return L.dca_pdb_build(dim, t.ctypes.data_as(C.c_void_p), len(tiles) if k is None else k, table, None, None)

    def evaluate(dim=4, groups=((1, 2, 3), (4, 5)), n=8, ld=16, states=one, out=one, tables=None, np_=None):
        t, ks = tiles_of(groups)
        ptrs = (C.c_void_p * max(len(groups), 1))(*([64] * len(groups) if tables is None else tables))
        return L.dca_pdb_eval(dim, states, n, ld, len(groups) if np_ is None else np_, t.ctypes.data_as(C.c_void_p),
                              ks.ctypes.data_as(C.c_void_p), ptrs, out, None)

    cases = [
        (lambda: build(k=0), b"k = 0"), (lambda: build(tiles=(0, 1)), b"tile 0"), (lambda: build(tiles=(1, 16)), b"tile 16"),
        (lambda: build(tiles=(1, 2, 1)), b"tile 1 appears twice"), (lambda: build(table=None), b"table"),
        (lambda: build(dim=2, tiles=(1,)), b"dim"), (lambda: build(dim=8, tiles=(1,)), b"dim"),
        (lambda: build(tiles=tuple(range(1, 9))), b"2^34"),
        (lambda: evaluate(groups=((1, 2), ())), b"k = 0"), (lambda: evaluate(groups=((0, 2),)), b"tile 0"),
        (lambda: evaluate(groups=((1, 16),)), b"tile 16"), (lambda: evaluate(groups=((1, 2, 3), (4, 2))), b"tile 2 appears twice"),
        (lambda: evaluate(groups=tuple((t,) for t in range(1, 26)), dim=7, ld=49), b"num_patterns"),
        (lambda: evaluate(groups=(), np_=0), b"num_patterns"),
        (lambda: evaluate(tables=[64, 0]), b"table 1 is NULL"), (lambda: evaluate(ld=15), b"ld"), (lambda: evaluate(dim=5, ld=24), b"ld"),
        (lambda: evaluate(dim=2), b"dim"), (lambda: evaluate(dim=8), b"dim"), (lambda: evaluate(n=-1), b"n >= 0"),
        (lambda: evaluate(n=1 << 31), b"n >= 0"), (lambda: evaluate(states=None), b"states"), (lambda: evaluate(out=None), b"out"),
    ]
    for fn, word in cases:
        assert fn() == -1, word
        msg = L.dca_last_error()
        assert msg.startswith(b"bad argument: dca_pdb_") and word in msg, (word, msg)
    assert evaluate(n=0, states=None, out=None) == 0  # nothing to do, nothing launched


def test_presets_cover_every_tile_once():
    from deepcubea_amd.utils import pattern_db as pd
    assert sorted(pd.PRESETS) == ["puzzle15", "puzzle24", "puzzle8"]
    assert {e: sorted(p) for e, p in pd.PRESETS.items()} == {"puzzle8": ["4-4"], "puzzle15": ["5-5-5", "6-6-3"], "puzzle24": ["6-6-6-6"]}
    for env, presets in pd.PRESETS.items():
        N = pd.puzzle_dim(env) ** 2
        for name, partition in presets.items():
            assert sorted(t for g in partition for t in g) == list(range(1, N)), (env, name)
            assert [len(g) for g in partition] == [int(x) for x in name.split("-")], (env, name)
            assert pd.parse_pdb_spec(env, name) == partition
    assert pd.parse_pdb_spec("puzzle8", "4-4") == ((1, 2, 3, 4), (5, 6, 7, 8))
    assert pd.parse_pdb_spec("puzzle15", "5-5-5") == ((1, 2, 3, 5, 6), (4, 7, 8, 11, 12), (9, 10, 13, 14, 15))
    assert pd.parse_pdb_spec("puzzle15", "6-6-3") == ((1, 5, 6, 9, 10, 13), (7, 8, 11, 12, 14, 15), (2, 3, 4))
    assert pd.parse_pdb_spec("puzzle24", "6-6-6-6") == ((1, 2, 3, 6, 7, 8), (4, 5, 9, 10, 14, 15), (11, 12, 16, 17, 21, 22),
                                                        (13, 18, 19, 20, 23, 24))
    for env, name in (("puzzle8", "4-4"), ("puzzle15", "5-5-5"), ("puzzle24", "6-6-6-6")):
        assert pd.parse_pdb_spec(env, "auto") == pd.PRESETS[env][name]
    assert pd.PatternDatabase("puzzle15", "5-5-5").bytes == 3 * 16 ** 6 and pd.PatternDatabase("puzzle15", "6-6-3").bytes == 2 * 16 ** 7 + 16 ** 4
    assert pd.PatternDatabase("puzzle24", "auto").bytes == 4 * 25 ** 7


def test_spec_parser_groups_and_refusals():
    from deepcubea_amd.utils import pattern_db as pd
    assert pd.parse_pdb_spec("puzzle8", "1,2,3,4/5,6,7,8") == ((1, 2, 3, 4), (5, 6, 7, 8))
    assert pd.parse_pdb_spec("puzzle15", "3, 2 ,1 / 15") == ((3, 2, 1), (15,))       # order kept, tiles may be left out
    assert pd.parse_pdb_spec("puzzle48", "1,2/47,48") == ((1, 2), (47, 48))
    assert pd.parse_pdb_spec("puzzle35", "35") == ((35,),)
    assert pd.parse_pdb_spec("puzzle24", "/".join("%d,%d,%d" % (a, a + 1, a + 2) for a in range(1, 25, 3)))[7] == (22, 23, 24)
    refused = [("cube3", "auto"), ("cube3", "1,2,3"), ("lightsout7", "1,2"), ("cube4", "4-4"), ("puzzle3", "1"), ("puzzle63", "1"),
               ("puzzle8", "1,2,1"), ("puzzle8", "1,2/3,2"), ("puzzle8", "0,1"), ("puzzle8", "9"), ("puzzle15", "16"),
               ("puzzle8", "5-5-5"), ("puzzle15", "4-4"), ("puzzle35", "auto"), ("puzzle48", "auto"), ("puzzle48", "6-6-6-6"),
               ("puzzle8", ""), ("puzzle8", "1,,2"), ("puzzle8", "1/"), ("puzzle8", "manhattan"), ("puzzle8", "1;2"),
               ("puzzle15", "1,2,3,4,5,6,7,8"),            # 16^9 bytes
               ("puzzle24", "1,2,3,4,5,6,7"),              # 25^8
               ("puzzle48", "1,2,3,4,5,6"),                # 49^7
               ("puzzle48", "/".join(str(t) for t in range(1, 26)))]  # 25 patterns
    for env, spec in refused:
        with pytest.raises(ValueError):
            pd.parse_pdb_spec(env, spec)
        with pytest.raises(ValueError):
            pd.PatternDatabase(env, spec)
    assert pd.parse_pdb_spec("puzzle15", "1,2,3,4,5,6,7") and pd.parse_pdb_spec("puzzle48", "1,2,3,4,5")  # at the cap
    for bad in (((1, 2), (2, 3)), ((0,),), ((9,),), ((),), ()):
        with pytest.raises(ValueError):
            pd.PatternDatabase("puzzle8", bad)


def test_auto_instances_is_one_for_a_pdb_model():
    from deepcubea_amd.search_methods import astar
    env = SimpleNamespace(get_num_moves=lambda: 4)
    for model in ("pdb:auto", "pdb:5-5-5", "pdb:1,2,3/4,5"):
        args = SimpleNamespace(instances_per_gpu="auto", model_dir=model, batch_size=100, env="puzzle15", max_nodes="auto")
        assert astar.auto_instances(args, env, 500, None) == 1
        args.instances_per_gpu = "3"
        assert astar.auto_instances(args, env, 500, None) == 3  # an explicit number is honoured, as for every model
    assert astar._is_pdb(SimpleNamespace(model_dir="pdb:4-4")) and not astar._is_pdb(SimpleNamespace(model_dir="synthetic:1"))
    action = {a.dest: a for a in astar.build_parser()._actions}["model_dir"]
    help_text = " ".join(action.help.split())
    assert "pdb:SPEC" in help_text and "--weight 1 --semantics cpp the solutions are optimal" in help_text


def test_cli_refuses_a_bad_spec_before_any_device_work():
    """`_load_heuristic` parses the spec first: the ValueError comes on a box without a GPU too."""
    from deepcubea_amd.search_methods import astar
    for env, model in (("cube3", "pdb:auto"), ("puzzle15", "pdb:1,2,3/3,4"), ("puzzle15", "pdb:nonsense")):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env=env), None)


def test_save_load_round_trip_of_a_host_made_table(tmp_path):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    partition = ((1, 2, 3), (8, 5))
    tables = [host_table(3, g) for g in partition]
    path = str(tmp_path / "p8.npz")
    PatternDatabase("puzzle8", partition).save(path, tables=tables)
    back, got = PatternDatabase.load_host(path)
    assert back.env_name == "puzzle8" and back.partition == partition and back.dim == 3 and back.bytes == 9 ** 4 + 9 ** 3
    assert len(got) == 2 and all(g.dtype == np.uint8 and np.array_equal(g, t) for g, t in zip(got, tables))
    with pytest.raises(ValueError):  # a table of the wrong size is refused on the way out
        PatternDatabase("puzzle8", partition).save(path, tables=[tables[0], tables[0]])
    with pytest.raises(ValueError):
        PatternDatabase("puzzle8", partition).save(path, tables=tables[:1])


def test_build_refuses_ids_outside_a_byte_before_any_device_call():
    """Both builds convert their ids through one helper: a value outside 0..255 is a ValueError, not a wrapped tile or cubie, and it
    comes before the table is allocated or the library is called (no device here)."""
    from deepcubea_amd import _lib
    for ids in ((1, 256), (-1,)):
        with pytest.raises(ValueError):
            _lib.pdb_build(4, ids)
        with pytest.raises(ValueError):
            _lib.cube3_pdb_build(0, ids)


def test_npz_files_written_by_hand_load_in_both_families(tmp_path):
    """The file format, pinned without save(): the keys env_name, partition and table_%d, written here with np.savez."""
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    rng = np.random.default_rng(5)
    p8, c3 = rng.integers(0, 256, 81).astype(np.uint8), rng.integers(0, 256, 528).astype(np.uint8)
    puzzle, cube = str(tmp_path / "p8.npz"), str(tmp_path / "c3.npz")
    with open(puzzle, "wb") as f:
        np.savez(f, env_name=np.array("puzzle8"), partition=np.array("1"), table_0=p8)
    with open(cube, "wb") as f:
        np.savez(f, env_name=np.array("cube3"), partition=np.array("e11,e0"), table_0=c3)
    pdb, tables = PatternDatabase.load_host(puzzle)
    assert (pdb.env_name, pdb.dim, pdb.partition, pdb.spec, pdb.bytes) == ("puzzle8", 3, ((1,),), "1", 81)
    assert len(tables) == 1 and tables[0].dtype == np.uint8 and np.array_equal(tables[0], p8)
    pdb, tables = Cube3PatternDatabase.load_host(cube)
    assert (pdb.env_name, pdb.patterns, pdb.spec, pdb.bytes) == ("cube3", ((1, (11, 0)),), "e11,e0", 528)
    assert len(tables) == 1 and tables[0].dtype == np.uint8 and np.array_equal(tables[0], c3)
    for cls, other in ((PatternDatabase, cube), (Cube3PatternDatabase, puzzle)):  # the other family's file is refused
        with pytest.raises(ValueError):
            cls.load_host(other)


def test_spec_is_the_string_save_writes_and_parses_back():
    from deepcubea_amd.utils import pattern_db as pd
    pdb = pd.PatternDatabase("puzzle15", "5-5-5")
    assert pdb.spec == "1,2,3,5,6/4,7,8,11,12/9,10,13,14,15"
    assert pd.parse_pdb_spec("puzzle15", pdb.spec) == pdb.partition == pd.PRESETS["puzzle15"]["5-5-5"]
