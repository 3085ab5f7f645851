"""CPU-side tests of the update step's heuristic cache (dca_hcache_*, `--update_cache`, DCA_UPDATE_CACHE): the ABI additions and
their ctypes signatures, the table size as a pure function, the refusals that come before any device call, the environment
variable in fresh processes, the driver's flag and the prefixes of the reference's flags.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_hcache_bytes", "dca_hcache_clear", "dca_hcache_lookup", "dca_hcache_finish")


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
    # the header states the rule: tag, probing, fill limit, byte equality, the four statuses, exactness
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "hash & (slots - 1)" in flat and "at most 32 probes" in flat and "linear probing" in flat
    assert "64-bit compare-and-swap" in flat and "slots / 2" in flat
    assert "equality is the bytes, not the hash" in flat and "compared byte for byte" in flat
    assert "batch-invariant" in flat and "No thread ever waits for another thread's write" in flat
    for i, status in enumerate(("HIT", "EVAL_STORE", "DUP", "EVAL_ONLY")):
        assert "#define DCA_HCACHE_%s %d" % (status, i) in hdr
    assert (_lib.HCACHE_HIT, _lib.HCACHE_EVAL_STORE, _lib.HCACHE_DUP, _lib.HCACHE_EVAL_ONLY) == (0, 1, 2, 3)


def test_ctypes_signatures_match_the_header():
    from deepcubea_amd import _lib
    L = _lib.lib()
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    assert L.dca_hcache_bytes.restype is i64 and list(L.dca_hcache_bytes.argtypes) == [i, i64]
    assert _params(hdr, "dca_hcache_bytes") == ["row_bytes", "slots"]
    assert L.dca_hcache_clear.restype is i and list(L.dca_hcache_clear.argtypes) == [p, i, i64, p]
    assert _params(hdr, "dca_hcache_clear") == ["table", "row_bytes", "slots", "stream"]
    assert L.dca_hcache_lookup.restype is i and list(L.dca_hcache_lookup.argtypes) == [p, i, i64, p, i64, i64, p, p, p, p]
    assert _params(hdr, "dca_hcache_lookup") == ["table", "row_bytes", "slots", "rows", "n", "ld", "h", "slot", "status", "stream"]
    assert L.dca_hcache_finish.restype is i and list(L.dca_hcache_finish.argtypes) == [p, i, i64, i64, p, p, p, p]
    assert _params(hdr, "dca_hcache_finish") == ["table", "row_bytes", "slots", "n", "slot", "status", "h", "stream"]


def test_table_bytes_is_a_pure_function():
    from deepcubea_amd import _lib
    L2 = C.CDLL(_lib.LIB_PATH)  # a second handle: no shared Python state
    L2.dca_hcache_bytes.restype, L2.dca_hcache_bytes.argtypes = C.c_int64, [C.c_int, C.c_int64]
    for rb in (1, 8, 9, 16, 25, 36, 49, 54, 64):
        for slots in (2, 64, 1 << 10, 1 << 20, 1 << 30):
            b = _lib.hcache_bytes(rb, slots)
            assert b == _lib.hcache_bytes(rb, slots) == L2.dca_hcache_bytes(rb, slots)
            assert b == 64 + slots * (24 + 8 * ((rb + 7) // 8))  # the formula the header states
            assert b % 16 == 0 and b >= slots * (rb + 12)  # room for the tag, the value and the row itself
    for rb, slots in ((0, 64), (65, 64), (-1, 64), (16, 0), (16, 1), (16, 3), (16, 96), (16, -64), (16, 1 << 31)):
        with pytest.raises(_lib.DcaError):
            _lib.hcache_bytes(rb, slots)


def test_refusals_need_no_device():
    """Every argument check comes before the first device call: DCA_E_BADARG and a message on a box without a GPU, too."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(64)  # never dereferenced: every call below is refused

    def lookup(table=one, rb=16, slots=64, rows=one, n=8, ld=16, h=one, slot=one, status=one):
        return L.dca_hcache_lookup(table, rb, slots, rows, n, ld, h, slot, status, None)

    def finish(table=one, rb=16, slots=64, n=8, slot=one, status=one, h=one):
        return L.dca_hcache_finish(table, rb, slots, n, slot, status, h, None)

    for kw in (dict(slots=96), dict(slots=0), dict(slots=63), dict(slots=-64), dict(rb=0), dict(rb=65), dict(n=-1), dict(ld=15),
               dict(rb=54, ld=53), dict(table=None), dict(table=C.c_void_p(72)), dict(rows=None), dict(h=None), dict(slot=None),
               dict(status=None), dict(h=C.c_void_p(66)), dict(n=1 << 31)):
        assert lookup(**kw) == -1, kw
        assert len(L.dca_last_error()) > 0, kw
    for kw in (dict(slots=96), dict(rb=0), dict(rb=65), dict(n=-1), dict(table=None), dict(slot=None), dict(status=None), dict(h=None)):
        assert finish(**kw) == -1, kw
    for kw in (dict(slots=96), dict(rb=0), dict(rb=65), dict(table=None)):
        assert L.dca_hcache_clear(kw.get("table", one), kw.get("rb", 16), kw.get("slots", 64), None) == -1, kw
    # the owner refuses bad arguments itself, before it allocates anything
    for rb, slots in ((0, 64), (65, 64), (16, 96), (16, 0), (16, 1)):
        with pytest.raises(ValueError):
            _lib.HeuristicCache(rb, slots)


def test_update_cache_values():
    from deepcubea_amd.updaters.updater import auto_cache_slots, parse_update_cache
    assert parse_update_cache("off") is None and parse_update_cache(None) is None
    assert parse_update_cache("auto") == "auto" and parse_update_cache("4096") == 4096 and parse_update_cache(1 << 20) == 1 << 20
    for bad in ("on", "", "AUTO", "4095", "0", "1", "-64", "1e6", "2.0", 96, str(1 << 31), True):
        with pytest.raises(ValueError):
            parse_update_cache(bad)
    # auto: a power of two that keeps every row of the shard under the fill limit, capped by a quarter of the free memory
    for rows in (1, 1000, 1_200_000, 600_000_000):
        s = auto_cache_slots(rows, 54, 256 << 30)
        assert s & (s - 1) == 0 and s >= 1024 and (s // 2 >= rows or s == 1 << 30 or 64 + 2 * s * 80 > (256 << 30) // 4)
    assert auto_cache_slots(1_200_000, 54, 256 << 30) == 1 << 22
    assert 64 + auto_cache_slots(600_000_000, 54, 8 << 30) * 80 <= (8 << 30) // 4


def _child(value, cache_arg="None"):
    env = {k: v for k, v in os.environ.items() if k != "DCA_UPDATE_CACHE"}
    if value is not None:
        env["DCA_UPDATE_CACHE"] = value
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from deepcubea_amd.updaters.updater import Updater\n"
            "class E: pass\n"
            "print(repr(Updater(E(), 10, 30, None, 1, cache=%s).cache_spec))\n" % (ROOT, cache_arg))
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_environment_variable_in_fresh_processes():
    """`Updater(..., cache=None)` reads DCA_UPDATE_CACHE; an explicit argument wins.  The children run side by side."""
    cases = ((None, "None", "None"), ("off", "None", "None"), ("auto", "None", "'auto'"), ("65536", "None", "65536"),
             ("auto", "'off'", "None"), (None, "4096", "4096"), ("on", "None", None), ("1000", "None", None), ("", "None", None))
    children = [_child(value, arg) for value, arg, _ in cases]
    for (value, arg, want), child in zip(cases, children):
        out, err = child.communicate(timeout=300)
        if want is None:
            assert child.returncode != 0 and "ValueError" in err and "DCA_UPDATE_CACHE" in err, (value, err)
        else:
            assert child.returncode == 0 and out.strip() == want, (value, arg, out, err)


def test_cli_flag_and_reference_prefixes():
    from deepcubea_amd.ctg_approx import avi
    parser = avi.build_parser()
    action = {a.dest: a for a in parser._actions}["update_cache"]
    assert action.default == "off" and not action.required and action.option_strings == ["--update_cache"]
    assert "batch-invariant" in action.help and "fp8" in action.help and "all-zeros" in action.help
    base = ["--env", "cube3", "--nnet_name", "x", "--back_max", "30"]
    assert parser.parse_args(base).update_cache == "off"
    for value in ("off", "auto", "1048576"):
        assert parser.parse_args(base + ["--update_cache", value]).update_cache == value
    # no prefix that selects a reference flag today became ambiguous
    args = parser.parse_args(base + ["--update_m", "ASTAR", "--update_nn", "123", "--update_nu", "7", "--update_c", "auto"])
    assert (args.update_method, args.update_nnet_batch_size, args.update_num, args.update_cache) == ("ASTAR", 123, 7, "auto")
    args = parser.parse_args(base + ["--max_u", "3", "--states", "50", "--eps", "0.5"])
    assert (args.max_update_steps, args.states_per_update, args.eps_max) == (3, 50, 0.5)
    # do_update hands the flag on, and builds no cache for the all-zeros heuristic
    import inspect
    assert inspect.signature(avi.do_update).parameters["update_cache"].default == "off"
    zeros = avi.target_heuristic(os.path.join(ROOT, "no_such_dir"), None, None, 100)
    assert getattr(zeros, "all_zeros", False) is True
