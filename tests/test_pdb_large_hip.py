"""GPU: the sliding-puzzle pattern databases at table indices past 2^31 and 2^32 (dca_pdb_build, dca_pdb_eval,
dca_pdb_eval_reflected, dca_idastar_npuzzle, dca_idastar_npuzzle_reflected and their wrappers in deepcubea_amd/_lib.py).

Three tables, the smallest that cross each boundary, each built once and dropped before the next (at most one is resident):
25^7 = 6 103 515 625 entries (indices past 2^32; what `pdb:auto` builds four of on puzzle24), 16^8 = 2^32 exactly (the entry
count itself needs 33 bits) and 36^6 = 2 176 782 336 (indices past 2^31; no other test builds a dim 6 table).  A variable
narrowed to 32 bits anywhere in the build, the eval or the search would still read inside its table and give plausible bytes,
so every check here is exact and independent of the code under test: the depth-bounded breadth-first search, the Bellman
equation and the mirror map of tests/test_pdb_large_cpu.py, the numpy index rule, and a recursive IDA* that reads the big
table's bytes one by one from the device.  Integer work throughout.  Whole-table reductions run in chunks of at most 2^30 bytes.

Where the inputs differ from uniform draws, and why.  The Bellman samples want >= 30 % states and >= 25 % of the indices at or
above the boundary, the eval rows >= 20 % above it: 2^22 uniform indices give 12 % states in 16^8 and 1.4 % above 2^31 in 36^6,
and uniform permutations put 1.3 % of the rows above 2^31 in 36^6, so sample_indices and eval_rows of
tests/test_pdb_large_cpu.py add draws of the lacking kind (the uniform ones stay).  The recursive search 28 moves from the goal
never leaves the part above 2^32 (78 nodes); the other three roots read both sides, and that is asserted for them.

On an MI355X (--durations=0), 37 s in all: the builds 7.0 s (25^7, 189 sweeps), 2.1 s (36^6, about 140 sweeps) and 1.4 s
(16^8, 111 sweeps), each once; the whole-partition eval on dim 6 16 s, nearly all of it the ten triples' tables by the host
reference (1.68 M entries each, a Python breadth-first search), on dim 5 under 2 s with its six; built twice 2.2 s; the Bellman
equation 0.8 - 1.6 s, the shallow region 0.2 - 0.7 s, the mirror identity 0.4 - 0.7 s a table; every search under 0.3 s; the
rest under 0.2 s."""
import time

import numpy as np
import pytest
import torch

from tests import test_idastar_cpu as ida
from tests import test_pdb_cpu as pz
from tests import test_pdb_large_cpu as big
from tests import test_pdb_reflect_cpu as rf

pytestmark = pytest.mark.gpu

CHUNK = 1 << 30
NODE_CAP = 200000  # what one root's recursive reference may generate
IDA_ROOTS = (28, 36, 44, 52)  # moves from the goal on shipped puzzle24 path 0 (optimal length 100)
IDA_REFLECTED_ROOTS = (28, 36)
IDA_CROSSING_ROOTS = (36, 44, 52)  # the recursive reference reads the big table on both sides of 2^32 (28: above it only)
REFLECTED_PARTITION_REST = ((1, 2, 3), (4, 5, 6), (7, 8, 9))


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    yield _lib
    _lib.idastar_set_prefix(-1)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


class Built:
    """One big table on the device and what several tests want of it, each computed once."""

    def __init__(self, L, dim):
        self.dim, (self.tiles, self.boundary, self.depth) = dim, big.BIG[dim]
        self.total = big.ENTRIES[dim]
        t0 = time.time()
        self.table, self.sweeps = L.pdb_build(dim, self.tiles)
        torch.cuda.synchronize()
        print("built %d^%d = %d bytes in %.1f s, %d sweeps" % (dim * dim, len(self.tiles) + 1, self.total, time.time() - t0, self.sweeps))
        self.cache = {}

    def read(self, idx):
        """the table's bytes at int64 indices, by a device gather"""
        idx = np.asarray(idx, np.int64)
        assert idx.min(initial=0) >= 0 and idx.max(initial=0) < self.total
        return self.table[dev(idx)].cpu().numpy()

    def count(self, value):
        """entries of the whole table equal to `value`, a Python integer"""
        total = 0
        for lo in range(0, self.total, CHUNK):
            total += int(torch.count_nonzero(self.table[lo:lo + CHUNK] == value))
        return total

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def shallow(self):
        return big.shallow(self.dim, self.tiles, self.depth)

    def samples(self):
        """every index the Bellman and mirror checks visit -> (all of them, how many of the first are the random samples)"""
        def make():
            random, windows = big.sample_indices(self.dim, self.tiles, self.boundary, 1000 + self.dim)
            return np.concatenate([random, windows, self.shallow()[0]]), len(random)
        return self.once("samples", make)

    def partition(self):
        return (self.tiles,) + big.rest_in_triples(self.dim, self.tiles)

    def small_tables(self):
        """the triples' tables from the host reference: on the host and on the device"""
        def make():
            host = [pz.host_table(self.dim, g) for g in self.partition()[1:]]
            return host, [dev(t) for t in host]
        return self.once("small", make)

    def drop(self):
        self.cache.clear()
        self.table = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def built(request, L):
    """The big table of request.param's board, built once for the tests that name it and gone before the next is built."""
    b = Built(L, request.param)
    assert b.table.numel() == b.total == L.pdb_bytes(b.dim, len(b.tiles)) and b.table.dtype == torch.uint8
    yield b
    b.drop()


# Tests are grouped by the POSITION of the fixture's parameter in these lists, so the lists are laid out to build each table
# once: position 0 runs the 36^6 tests and then the searches on 25^7, position 1 the other 25^7 tests, position 2 16^8.
every_table = pytest.mark.parametrize("built", [6, 5, 4], indirect=True)
eval_tables = pytest.mark.parametrize("built", [6, 5], indirect=True)
dim6_table = pytest.mark.parametrize("built", [6], indirect=True)
search_table = pytest.mark.parametrize("built", [5], indirect=True)


def first_differences(b, idx, got, want, limit=5):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))[:limit]
    digits = big.digits_of(b.dim, len(b.tiles), np.asarray(idx)[bad])
    return [("index %d" % idx[i], "digits %s" % dg.tolist(), "got %d" % got[i], "want %d" % want[i]) for i, dg in zip(bad, digits)]


# ------------------------------------------------------------------------------------------------ 1. the shallow region
@every_table
def test_shallow_region_equals_the_bounded_search_and_nothing_else_is_that_low(built):
    idx, want = built.shallow()
    per_distance, above, _ = big.SHALLOW[built.dim]
    assert np.bincount(want, minlength=built.depth + 1).tolist() == per_distance[:built.depth + 1]
    assert int((idx >= built.boundary).sum()) * 4 > len(idx) and (built.depth < 8 or int((idx >= built.boundary).sum()) == above)
    got = built.read(idx)
    assert np.array_equal(got, want), first_differences(built, idx, got, want)
    # an underestimate written ANYWHERE in the table would add to one of these counts
    for v in range(built.depth + 1):
        assert built.count(v) == per_distance[v], (built.dim, v)


# ------------------------------------------------------------------------------------------------ 2. census
@every_table
def test_census_of_the_whole_table(built):
    N, k = built.dim ** 2, len(built.tiles)
    states = 1
    for j in range(k + 1):
        states *= N - j  # N! / (N - k - 1)! in Python integers
    assert built.count(pz.NO_STATE) == N ** (k + 1) - states == big.no_state_count(built.dim, k)
    assert built.count(pz.UNREACHABLE) == 0
    assert int(built.table[big.goal_index(built.dim, built.tiles)]) == 0
    assert 1 < built.sweeps < 1000


# ------------------------------------------------------------------------------------------------ 3. the Bellman equation
@every_table
def test_bellman_equation_on_samples_windows_and_the_shallow_region(built):
    idx, random = built.samples()
    # conditions on the input, not on the kernel
    states = big.is_state(big.digits_of(built.dim, len(built.tiles), idx[:random]))
    print("dim %d: %d random samples, %.1f %% states, %.1f %% at or above the boundary" % (
        built.dim, random, 100 * states.mean(), 100 * (idx[:random] >= built.boundary).mean()))
    assert random >= big.SAMPLES and states.mean() >= 0.30 and (idx[:random] >= built.boundary).mean() >= 0.25
    bad = big.bellman_violations(built.dim, built.tiles, idx, built.read)
    assert bad == [], ["index %d, digits %s, got %d, want %d" % b for b in bad[:5]]


# ------------------------------------------------------------------------------------------------ 4. the mirror identity
@every_table
def test_mirrored_entry_holds_the_same_byte(built):
    """The pattern is self-mirrored and the goal is its own image, so the mirror map is a symmetry of the abstract space that
    fixes the goal: distances are equal, exactly.  The mirrored entry of an entry above the boundary is mostly below it."""
    idx, _ = built.samples()
    digits = big.digits_of(built.dim, len(built.tiles), idx)
    state = big.is_state(digits)
    idx, digits = idx[state], digits[state]
    mirrored = big.mirror_entries(built.dim, built.tiles, digits)
    assert ((idx >= built.boundary) != (mirrored >= built.boundary)).mean() > 0.05  # pairs that straddle the boundary
    got, want = built.read(mirrored), built.read(idx)
    assert np.array_equal(got, want), first_differences(built, mirrored, got, want)
    assert int(want.max()) < pz.UNREACHABLE


# ------------------------------------------------------------------------------------------------ 5. built twice
@dim6_table
def test_built_twice_the_same_bytes(L, built):
    again, sweeps = L.pdb_build(built.dim, built.tiles)
    assert sweeps > 1 and again.numel() == built.total
    for lo in range(0, built.total, CHUNK):
        assert torch.equal(again[lo:lo + CHUNK], built.table[lo:lo + CHUNK]), lo
    del again
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ eval
def numpy_eval(b, rows, partition, small_host, reflect):
    """the sum of the tables' bytes at the numpy index rule's entries: the big table's by a device gather"""
    entry = big.row_entries(b.dim, rows, b.tiles, reflect)
    total = b.read(entry).astype(np.int64)
    for tiles, table in zip(partition[1:], small_host):
        total += table[big.row_entries(b.dim, rows, tiles, reflect)]
    return total, entry


def layouts(N):
    """(row stride, byte offset of the base): contiguous; a stride and base that are multiples of 4 (word loads); neither (byte loads)"""
    return ((N, 0), ((N + 3) // 4 * 4 + 4, 0), (N + 2, 1))


def eval_all_layouts(L, b, rows, partition, tables, reflect, want):
    N, n = b.dim ** 2, len(rows)
    for ld, off in layouts(N):
        buf = torch.full((n * ld + off + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[off:off + n * ld].view(n, ld)[:, :N]
        view.copy_(dev(rows))
        assert view.data_ptr() % 4 == off and (off == 0 or ld % 4 != 0)
        out = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda")
        L.pdb_eval(b.dim, view, partition, tables, out=out, reflect=reflect)
        got = out[:n].cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)), (
            b.dim, ld, off, reflect, [(int(i), rows[i].tolist(), float(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:3]])
        assert bool((out[n:] == -1.0).all())  # no stray write


@eval_tables
def test_eval_of_the_whole_partition_against_the_numpy_index_rule(L, built):
    """The big pattern and the rest of the board in triples (7 patterns on dim 5, 11 on dim 6: three trips of the four-gather
    loop), plain and reflected, on 4099 permutations and on 256 rows of any bytes, under word loads and byte loads."""
    partition = built.partition()
    small_host, small_dev = built.small_tables()
    tables = [built.table] + small_dev
    for rows in (big.eval_rows(built.dim, built.tiles, built.boundary, built.dim), big.any_byte_rows(built.dim, built.dim)):
        plain, entry = numpy_eval(built, rows, partition, small_host, False)
        mirrored, mirrored_entry = numpy_eval(built, rows, partition, small_host, True)
        if len(rows) == 4099:  # conditions on the input
            assert (entry >= built.boundary).mean() >= 0.20 and (mirrored_entry >= built.boundary).mean() >= 0.20
            assert (mirrored > plain).any() and (mirrored < plain).any()
        eval_all_layouts(L, built, rows, partition, tables, False, plain)
        eval_all_layouts(L, built, rows, partition, tables, True, np.maximum(plain, mirrored))


@eval_tables
def test_reflected_eval_of_the_self_mirrored_pattern_alone_gains_nothing(L, built):
    rows = big.eval_rows(built.dim, built.tiles, built.boundary, 50 + built.dim)
    entry, mirrored_entry = big.row_entries(built.dim, rows, built.tiles), big.row_entries(built.dim, rows, built.tiles, True)
    assert (entry != mirrored_entry).mean() > 0.9 and (mirrored_entry >= built.boundary).mean() >= 0.20
    want = built.read(entry)
    plain = L.pdb_eval(built.dim, dev(rows), (built.tiles,), [built.table]).cpu().numpy()
    mirrored = L.pdb_eval(built.dim, dev(rows), (built.tiles,), [built.table], reflect=True).cpu().numpy()
    assert np.array_equal(plain, want.astype(np.float32)), first_differences(built, entry, plain, want)
    assert np.array_equal(mirrored, plain), first_differences(built, mirrored_entry, mirrored, plain)


# ------------------------------------------------------------------------------------------------ IDA*
class DeviceBytes:
    """The big table as the recursive reference reads it: single bytes from the device, each index once.  It counts the reads
    on either side of the boundary and refuses to go on past the node cap (a reflected h reads twice a node)."""

    def __init__(self, b):
        self.table, self.boundary, self.memo, self.below, self.above, self.budget = b.table, b.boundary, {}, 0, 0, 0

    def __getitem__(self, idx):
        idx = int(idx)
        self.budget -= 1
        assert self.budget >= 0, "the reference search passed its node cap"
        if idx >= self.boundary:
            self.above += 1
        else:
            self.below += 1
        v = self.memo.get(idx)
        if v is None:
            v = self.memo[idx] = int(self.table[idx])
        return v


def reference_search(b, golden, k, partition, small_host, reflect):
    """(root, thresholds, counts, reads below the boundary, reads above it) by tests/test_pdb_reflect_cpu.reference_idastar, once a root"""
    def make():
        reader = b.once("reader", lambda: DeviceBytes(b))
        root = rf.suffix_root(golden, "puzzle24", b.dim, 0, k)
        below, above = reader.below, reader.above
        reader.budget = (2 if reflect else 1) * (NODE_CAP + 1)
        thresholds, counts = rf.reference_idastar(b.dim, root, rf.state_h(b.dim, partition, [reader] + small_host, reflect), k)
        assert sum(counts) < NODE_CAP
        return root, thresholds, counts, reader.below - below, reader.above - above
    return b.once(("reference", k, reflect), make)


def search_equals_the_reference(L, b, golden, k, partition, small_host, small_dev, reflect):
    tables = [b.table] + small_dev
    root, thresholds, counts, below, above = reference_search(b, golden, k, partition, small_host, reflect)
    entry = int(big.row_entries(b.dim, root[None], b.tiles)[0])
    print("puzzle24 %d from the goal%s: root entry %d, reference thresholds %s, nodes %d, reads below / above 2^32: %d / %d" % (
        k, ", reflected" if reflect else "", entry, thresholds, sum(counts), below, above))
    assert (above if entry >= b.boundary else below) > 0 and (k not in IDA_CROSSING_ROOTS or (below > 0 and above > 0))
    h_root = float(L.pdb_eval(b.dim, dev(root[None]), partition, tables, reflect=reflect)[0])
    assert thresholds[0] == h_root
    for depth in (-1, 10):
        L.idastar_set_prefix(depth)
        try:
            res = L.idastar_npuzzle(b.dim, root, partition, tables, ida.BIG, reflect=reflect)
        finally:
            L.idastar_set_prefix(-1)
        assert res["solved"] and res["status"] == "solved" and len(res["moves"]) == k == res["path_cost"], (k, depth, res)
        assert np.array_equal(ida.replay_puzzle(b.dim, root, res["moves"]), ida.puzzle_goal(b.dim))
        assert res["thresholds"][0] == h_root and res["thresholds"] == thresholds + [k], (k, depth, res, thresholds)
        assert res["nodes_per_threshold"][:len(counts)] == counts, (k, depth, res, counts)
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"])
    return entry


@search_table
@pytest.mark.parametrize("k", IDA_ROOTS)
def test_idastar_on_the_whole_partition_equals_a_recursive_search(L, golden, built, k):
    """Seven patterns (the limit is eight running indices): the 25^7 table and six triples.  They cover the board, so they
    dominate the Manhattan distance, with which the recursive search generates 660, 6 942, 13 490 and 58 140 nodes for the four
    roots.  The roots 28 and 36 moves out index the big table above 2^32, the other two below it."""
    assert int(golden["puzzle24_test_opt_len"][0]) == 100 and len(built.partition()) == 7 <= L.IDASTAR_MAX_PUZZLE_PATTERNS
    small_host, small_dev = built.small_tables()
    entry = search_equals_the_reference(L, built, golden, k, built.partition(), small_host, small_dev, False)
    assert (entry >= built.boundary) == (k in (28, 36)) and (k != 36 or entry == 4624109033)


@search_table
@pytest.mark.parametrize("k", IDA_REFLECTED_ROOTS)
def test_reflected_idastar_with_four_patterns_equals_a_recursive_search(L, golden, built, k):
    """Four patterns, the reflected search's limit (eight running indices: the 25^7 table is read at the state and at its
    mirror image): the big pattern and the triples (1,2,3), (4,5,6), (7,8,9)."""
    partition = (built.tiles,) + REFLECTED_PARTITION_REST
    assert len(partition) == 4 == L.IDASTAR_MAX_REFLECT_PATTERNS and built.partition()[1:4] == REFLECTED_PARTITION_REST
    small_host, small_dev = built.small_tables()
    search_equals_the_reference(L, built, golden, k, partition, small_host[:3], small_dev[:3], True)
