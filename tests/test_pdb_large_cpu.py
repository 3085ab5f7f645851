"""Host side of the large pattern-database tests (tests/test_pdb_large_hip.py imports it; no GPU needed here): what the GPU
tests compare the three big tables against, and tests of that reference itself.

The tables are the smallest that cross each boundary of the index arithmetic: 25^7 entries (indices past 2^32), 16^8 = 2^32
exactly (the entry count itself needs 33 bits) and 36^6 (indices past 2^31, on a dim the device never built before).  None of
them fits a host reference that fills the whole table, so the reference here is a DEPTH-BOUNDED 0-1 breadth-first search written
from include/dca.h's index, cost and 0xFF rules like tests/test_pdb_cpu._host_table: it allocates no table and returns
{abstract state: distance} for every state at distance <= d.  Every pattern sits next to the blank's home corner, so these
shallow states already have the highest digits large: most of them lie above the boundary.

The rest restates the header in numpy int64 for entries picked by index: the digits, the 0xFF rule, the blank-move neighbours
with their costs (the Bellman equation every built entry satisfies) and the mirror map of include/dca.h's reflected look-up,
which maps the table of a self-mirrored pattern onto itself."""
import math
from collections import deque
from functools import lru_cache

import numpy as np
import pytest

from tests import test_pdb_cpu as pz
from tests import test_pdb_reflect_cpu as rf

NO_STATE, UNREACHABLE = pz.NO_STATE, pz.UNREACHABLE
# dim -> (tiles, boundary the indices cross, depth of the reference); every tile set is its own image under phi
BIG = {5: ((13, 14, 18, 19, 20, 24), 1 << 32, 7), 4: ((7, 8, 10, 11, 12, 14, 15), 1 << 31, 8), 6: ((24, 29, 30, 34, 35), 1 << 31, 8)}
ENTRIES = {5: 25 ** 7, 4: 16 ** 8, 6: 36 ** 6}
# states per distance 0..8, how many of the states at distance <= 8 have an index at or above the boundary, the largest index
SHALLOW = {5: ([1, 38, 230, 1610, 7344, 30718, 110917, 371192, 1093540], 1559698, 6092917820),
           4: ([1, 2, 20, 128, 412, 1544, 4786, 14396, 39541], 60374, 4273850281),
           6: ([1, 2, 124, 498, 2186, 7394, 22290, 62562, 172261], 109686, 2175000116)}
SAMPLES, WINDOW = 1 << 22, 1 << 16


# ------------------------------------------------------------------------------------------------ the bounded reference
def bounded_bfs(dim, tiles, d):
    """{(blank, pos of tiles[0], ...): distance} for every abstract state at distance <= d from the goal.  A 0-1 breadth-first
    search: a move that swaps the blank with an invisible tile costs 0 and is followed at any depth, a move that swaps it with a
    pattern tile costs 1 and is taken only while the result stays <= d.  Every shortest path to a state at distance <= d runs
    through such states only, so the distances are exact."""
    nb = pz.neighbours(dim)
    N = dim * dim
    goal = (N - 1,) + tuple(t - 1 for t in tiles)
    dist = {goal: 0}
    queue = deque([(0, goal)])
    while queue:
        g, s = queue.popleft()
        if g > dist[s]:
            continue
        blank = s[0]
        for q in nb[blank]:
            if q in s[1:]:
                if g < d:
                    j = s.index(q, 1)
                    t = (q,) + s[1:j] + (blank,) + s[j + 1:]
                    if g + 1 < dist.get(t, 1 << 30):
                        dist[t] = g + 1
                        queue.append((g + 1, t))
            else:
                t = (q,) + s[1:]
                if g < dist.get(t, 1 << 30):
                    dist[t] = g
                    queue.appendleft((g, t))
    return dist


def weights(dim, k):
    """digit 0 = the blank, digit j + 1 = tiles[j] (the index rule), as int64"""
    return np.array([(dim * dim) ** j for j in range(k + 1)], np.int64)


@lru_cache(maxsize=None)
def shallow(dim, tiles, d):
    """bounded_bfs as arrays, computed once and never written to -> (indices int64, ascending; their distances uint8)."""
    dist = bounded_bfs(dim, tiles, d)
    idx = np.array(list(dist.keys()), np.int64) @ weights(dim, len(tiles))
    val = np.fromiter(dist.values(), np.int64, len(dist))
    order = np.argsort(idx)
    idx, val = idx[order], val[order].astype(np.uint8)
    assert len(np.unique(idx)) == len(idx) and 0 <= idx[0] and int(idx[-1]) < (dim * dim) ** (len(tiles) + 1)
    idx.setflags(write=False)
    val.setflags(write=False)
    return idx, val


# ------------------------------------------------------------------------------------------------ the header, by index
def digits_of(dim, k, idx):
    """[n, k + 1] int64: column 0 the blank's position, column j + 1 the position of tiles[j]."""
    N, r = dim * dim, np.asarray(idx, np.int64)
    cols = []
    for _ in range(k + 1):
        cols.append(r % N)
        r = r // N
    assert not r.any()
    return np.stack(cols, 1)


def is_state(digits):
    """the 0xFF rule: an entry is a state when its digits are pairwise distinct"""
    seen, twice = np.zeros(len(digits), np.int64), np.zeros(len(digits), np.int64)
    for j in range(digits.shape[1]):
        bit = np.int64(1) << digits[:, j]
        twice |= seen & bit
        seen |= bit
    return twice == 0


def goal_index(dim, tiles):
    N = dim * dim
    return int(sum(p * N ** j for j, p in enumerate((N - 1,) + tuple(t - 1 for t in tiles))))


def no_state_count(dim, k):
    """entries that are no state, in Python integers: N^(k+1) - N! / (N - k - 1)!"""
    N = dim * dim
    return N ** (k + 1) - math.factorial(N) // math.factorial(N - k - 1)


def neighbour_entries(dim, k, digits):
    """For states given by their digits, the entries one blank move away, U D L R as tests/test_pdb_cpu.neighbours lists them
    -> (index [n, 4] int64, cost [n, 4], move exists [n, 4]).  The neighbour's digits are written out and encoded again (the
    blank's digit becomes the target position; a pattern tile standing there takes the blank's old position and the move costs
    1), so no index difference is formed as the kernels form it.  A move off the board has index 0 and exists = False."""
    w = weights(dim, k)
    cols = np.ascontiguousarray(digits.T)  # a digit per row: the loops below run over contiguous vectors
    blank = cols[0]
    i, j = blank // dim, blank % dim
    ok = np.stack([i < dim - 1, i > 0, j < dim - 1, j > 0], 1)
    idx = np.zeros((len(digits), 4), np.int64)
    cost = np.zeros((len(digits), 4), np.int64)
    for a, step in enumerate((dim, -dim, 1, -1)):
        q = np.where(ok[:, a], blank + step, blank)
        entry, swaps = q * w[0], np.zeros(len(digits), bool)
        for t in range(1, k + 1):
            hit = cols[t] == q
            entry += np.where(hit, blank, cols[t]) * w[t]
            swaps |= hit
        idx[:, a] = np.where(ok[:, a], entry, 0)
        cost[:, a] = swaps & ok[:, a]
    return idx, cost, ok


def bellman_violations(dim, tiles, idx, read, chunk=1 << 20):
    """The entries among `idx` whose byte (read(indices) -> uint8 array) is not what the build's fixed point demands:
    0xFF where two digits are equal, 0 at the goal, otherwise below 0xFE and equal to the minimum over the blank's moves of the
    neighbour's byte plus the move's cost -> a list of (index, digits, got, want), empty when all is well."""
    k, goal, bad = len(tiles), goal_index(dim, tiles), []
    idx = np.asarray(idx, np.int64)
    for lo in range(0, len(idx), chunk):
        e = idx[lo:lo + chunk]
        got = np.asarray(read(e)).astype(np.int64)
        dg = digits_of(dim, k, e)
        state = is_state(dg)
        want = np.full(len(e), NO_STATE, np.int64)
        s = np.flatnonzero(state)
        ne, cost, ok = neighbour_entries(dim, k, dg[s])
        v = np.asarray(read(ne.reshape(-1))).astype(np.int64).reshape(-1, 4)
        through = np.where(ok & (v < UNREACHABLE), v + cost, 1 << 20).min(1)
        want[s] = np.where(e[s] == goal, 0, through)
        wrong = (got != want) | (state & (got >= UNREACHABLE))
        bad += [(int(e[i]), dg[i].tolist(), int(got[i]), int(want[i])) for i in np.flatnonzero(wrong)[:8]]
    return bad


def mirror_entries(dim, tiles, digits):
    """The entry of the mirrored state, for states given by their digits: its blank digit is refl(b), its digit for tile t_j is
    refl(p_j') with t_j' = phi(t_j) — the mirror image holds phi(t) at refl(pos(t)), and the pattern holds phi(t) with t."""
    refl = np.array([rf.refl(dim, p) for p in range(dim * dim)], np.int64)
    partner = [tiles.index(rf.phi(dim, t)) for t in tiles]  # ValueError: the pattern is not self-mirrored
    cols = [refl[digits[:, 0]]] + [refl[digits[:, 1 + jp]] for jp in partner]
    return np.stack(cols, 1) @ weights(dim, len(tiles))


def sample_indices(dim, tiles, boundary, seed):
    """The entries the Bellman and mirror checks visit besides the shallow region, seeded: 2^22 uniform indices in [0, total)
    and windows of 2^16 consecutive entries at 0, across 2^31, across 2^32 where the table reaches it, and at the table's end.
    The checks want at least 30 % states and at least 25 % indices at or above the boundary among the random samples.  Where the
    uniform ones cannot give that (16^8 has 12 % states, 36^6 has 1.4 % of its entries above 2^31) half as many again are drawn
    from the lacking kind: states by drawing the digits without repetition, indices uniform in [boundary, total).
    -> (random samples, windows)"""
    N, k = dim * dim, len(tiles)
    total = N ** (k + 1)
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, total, SAMPLES, dtype=np.int64)]
    if (total - no_state_count(dim, k)) * 100 < 30 * total:
        drawn = rng.permuted(np.tile(np.arange(N, dtype=np.uint8), (SAMPLES // 2, 1)), axis=1)[:, :k + 1]
        parts.append(drawn.astype(np.int64) @ weights(dim, k))
    if (total - boundary) * 100 < 25 * total:
        parts.append(rng.integers(boundary, total, SAMPLES // 2, dtype=np.int64))
    starts = [0, (1 << 31) - WINDOW // 2] + ([(1 << 32) - WINDOW // 2] if total > (1 << 32) + WINDOW else []) + [total - WINDOW]
    windows = np.concatenate([np.arange(s, s + WINDOW, dtype=np.int64) for s in starts])
    assert windows.min() == 0 and windows.max() == total - 1
    return np.concatenate(parts), windows


# ------------------------------------------------------------------------------------------------ eval and search inputs
def rest_in_triples(dim, tiles):
    """the tiles outside the pattern, ascending, three a group: with the pattern itself a partition of the whole board"""
    rest = [t for t in range(1, dim * dim) if t not in tiles]
    assert len(rest) % 3 == 0
    return tuple(tuple(rest[i:i + 3]) for i in range(0, len(rest), 3))


def row_entries(dim, rows, tiles, reflect=False):
    """The entry dca_pdb_eval reads for each row (ANY bytes) in the pattern's table, int64; reflect: the entry of the row's
    mirror image, whose digit for tile t is refl(pos(phi(t))).  tests/test_pdb_cpu.host_eval and
    tests/test_pdb_reflect_cpu.reflected_sum sum table bytes at exactly these entries (tested below)."""
    N = dim * dim
    refl = np.array([rf.refl(dim, p) for p in range(N)], np.int64) if reflect else np.arange(N, dtype=np.int64)
    idx = np.zeros(len(rows), np.int64)
    for t in reversed(tiles):
        idx = idx * N + refl[pz.host_positions(dim, rows, rf.phi(dim, t) if reflect else t)]
    return idx * N + refl[pz.host_positions(dim, rows, 0)]


def eval_rows(dim, tiles, boundary, seed, n=4099, forced=1100):
    """n seeded rows, each a permutation of the board: `forced` of them drawn among the permutations whose entry in the pattern's
    table is at or above the boundary, `forced` more the mirror images of such rows (their MIRRORED entry is above it), the rest
    uniform, all shuffled.  (Uniform permutations alone put 28 % of the rows above 2^32 in the 25^7 table but 1.3 % above 2^31
    in the 36^6 one.)"""
    N = dim * dim
    rng = np.random.default_rng(seed)
    draw = lambda m: rng.permuted(np.tile(np.arange(N, dtype=np.uint8), (m, 1)), axis=1)
    high = np.zeros((0, N), np.uint8)
    while len(high) < 2 * forced:
        cand = draw(1 << 17)
        high = np.concatenate([high, cand[row_entries(dim, cand, tiles) >= boundary]])
    rows = np.concatenate([draw(n - 2 * forced), high[:forced], rf.mirror_rows(dim, high[forced:2 * forced])])
    return rows[rng.permutation(n)]


def any_byte_rows(dim, seed, n=256):
    """rows that are no states: all zero, all 0xFF, arbitrary bytes, bytes < N with repeats, bytes >= N only"""
    N = dim * dim
    rng = np.random.default_rng(seed)
    return np.concatenate([np.zeros((2, N), np.uint8), np.full((2, N), 0xFF, np.uint8), rng.integers(0, 256, (n - 128, N), dtype=np.uint8),
                           rng.integers(0, N, (120, N), dtype=np.uint8), rng.integers(N, 256, (4, N), dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------ tests of the reference
@pytest.mark.parametrize("dim,tiles", [(3, (1, 2, 3, 4)), (4, (1, 2, 5)), (6, (8, 35))])
def test_bounded_search_equals_the_full_table_up_to_its_depth_and_reaches_nothing_else(dim, tiles):
    table = pz.host_table(dim, tiles)
    deepest = int(table[table < UNREACHABLE].max())
    for d in (0, 1, 4, 8, deepest):
        idx, val = shallow(dim, tiles, d)
        assert np.array_equal(idx, np.flatnonzero(table <= d)) and np.array_equal(val, table[idx]), (dim, tiles, d)


@pytest.mark.parametrize("dim", [5, 4, 6])
def test_bounded_search_reproduces_the_recorded_histograms(dim):
    tiles, boundary, d = BIG[dim]
    per_distance, above, largest = SHALLOW[dim]
    idx, val = shallow(dim, tiles, 8)
    assert np.bincount(val, minlength=9).tolist() == per_distance and len(idx) == sum(per_distance)
    assert int((idx >= boundary).sum()) == above and int(idx[-1]) == largest
    assert idx[val == 0].tolist() == [goal_index(dim, tiles)] and is_state(digits_of(dim, len(tiles), idx)).all()
    assert ENTRIES[dim] == (dim * dim) ** (len(tiles) + 1) and boundary < ENTRIES[dim]
    if d < 8:  # what the GPU tests use on dim 5: depth 7, 522 050 states, the depth-8 search's states at distance <= 7
        shallower, values = shallow(dim, tiles, d)
        assert (d, len(shallower)) == (7, 522050) and int((shallower >= boundary).sum()) * 10 > 9 * len(shallower)
        assert np.array_equal(shallower, idx[val <= d]) and np.array_equal(values, val[val <= d])


def test_every_big_pattern_is_self_mirrored_and_next_to_the_blanks_corner():
    for dim, (tiles, _, _) in BIG.items():
        assert sorted(rf.phi(dim, t) for t in tiles) == sorted(tiles) and dim * dim - 1 in tiles
        assert ENTRIES[dim] == (dim * dim) ** (len(tiles) + 1) <= 1 << 34


def test_mirror_map_leaves_a_self_mirrored_table_unchanged():
    tiles = rf.P8_SELF_MIRRORED[0]
    assert tiles == (1, 5, 2, 4)
    table = pz.host_table(3, tiles)
    idx = np.flatnonzero(table != NO_STATE)
    dg = digits_of(3, 4, idx)
    assert is_state(dg).all() and len(idx) == 9 ** 5 - no_state_count(3, 4) == 15120
    m = mirror_entries(3, tiles, dg)
    assert np.array_equal(np.sort(m), idx) and not np.array_equal(m, idx)  # a permutation of the states, not the identity
    assert np.array_equal(table[m], table[idx])
    assert np.array_equal(mirror_entries(3, tiles, digits_of(3, 4, m)), idx)  # an involution
    # the same map as mirroring whole rows: a row's entry, mirrored, is the mirrored row's entry
    rows = np.stack([np.random.default_rng(s).permutation(9).astype(np.uint8) for s in range(50)])
    entry = lambda r: np.stack([pz.host_positions(3, r, t) for t in (0,) + tiles], 1) @ weights(3, 4)
    assert np.array_equal(mirror_entries(3, tiles, digits_of(3, 4, entry(rows))), entry(rf.mirror_rows(3, rows)))
    with pytest.raises(ValueError):
        mirror_entries(3, (1, 2, 3, 4), dg)


@pytest.mark.parametrize("dim,tiles", [(3, (1, 5, 2, 4)), (4, (1, 2, 5)), (6, (8, 35)), (7, (20, 48))])
def test_the_bellman_check_accepts_the_host_table_and_names_a_wrong_byte(dim, tiles):
    table = pz.host_table(dim, tiles)
    everything = np.arange(table.size, dtype=np.int64)
    assert bellman_violations(dim, tiles, everything, lambda i: table[i]) == []
    assert int((table == NO_STATE).sum()) == no_state_count(dim, len(tiles)) and table[goal_index(dim, tiles)] == 0
    rng = np.random.default_rng(dim)
    states = np.flatnonzero((table != NO_STATE) & (table > 1))
    for e in states[rng.integers(0, len(states), 4)]:
        for wrong in (int(table[e]) - 1, int(table[e]) + 1, UNREACHABLE, NO_STATE):  # an underestimate, an overestimate, ...
            broken = table.copy()
            broken[e] = wrong
            bad = bellman_violations(dim, tiles, everything, lambda i: broken[i])
            assert (int(e), digits_of(dim, len(tiles), [e])[0].tolist(), wrong, int(table[e])) in bad, (dim, tiles, e, wrong)
    broken = table.copy()
    broken[0] = 3  # an entry that is no state
    assert bellman_violations(dim, tiles, everything[:100], lambda i: broken[i])[0] == (0, [0] * (len(tiles) + 1), 3, NO_STATE)


def test_sample_sets_meet_their_conditions_by_construction():
    for dim, (tiles, boundary, _) in BIG.items():
        random, windows = sample_indices(dim, tiles, boundary, dim)
        total = ENTRIES[dim]
        assert random.min() >= 0 and random.max() < total and len(random) >= SAMPLES
        assert np.array_equal(random[:SAMPLES], np.random.default_rng(dim).integers(0, total, SAMPLES, dtype=np.int64))
        assert len(random) == {5: 2, 4: 3, 6: 3}[dim] * SAMPLES // 2 and len(windows) == {5: 4, 4: 3, 6: 3}[dim] * WINDOW
        assert is_state(digits_of(dim, len(tiles), random)).mean() >= 0.30 and (random >= boundary).mean() >= 0.25
        assert (windows == boundary).any() and (windows == boundary - 1).any()


@pytest.mark.parametrize("dim", [5, 6])
def test_eval_rows_meet_their_conditions_by_construction(dim):
    tiles, boundary, _ = BIG[dim]
    rows = eval_rows(dim, tiles, boundary, dim)
    assert rows.shape == (4099, dim * dim) and (np.sort(rows, 1) == np.arange(dim * dim)).all()
    plain, mirrored = row_entries(dim, rows, tiles), row_entries(dim, rows, tiles, reflect=True)
    assert (plain >= boundary).mean() >= 0.20 and (mirrored >= boundary).mean() >= 0.20
    assert max(plain.max(), mirrored.max()) < ENTRIES[dim] and (plain < boundary).mean() >= 0.20
    assert np.array_equal(mirrored, row_entries(dim, rf.mirror_rows(dim, rows), tiles))
    partition = (tiles,) + rest_in_triples(dim, tiles)
    assert sorted(t for g in partition for t in g) == list(range(1, dim * dim)) and len(partition) == {5: 7, 6: 11}[dim]
    junk = any_byte_rows(dim, dim)
    assert junk.shape == (256, dim * dim) and (junk >= dim * dim).any() and 0 <= row_entries(dim, junk, tiles).min()
    assert max(row_entries(dim, junk, tiles).max(), row_entries(dim, junk, tiles, reflect=True).max()) < ENTRIES[dim]


@pytest.mark.parametrize("dim", [3, 4, 6])
def test_row_entries_are_where_the_existing_host_evals_read(dim):
    partition, tables, rows = rf.random_rows_case(dim, 70 + dim)
    plain = sum(tables[i][row_entries(dim, rows, g)].astype(np.int64) for i, g in enumerate(partition))
    mirrored = sum(tables[i][row_entries(dim, rows, g, reflect=True)].astype(np.int64) for i, g in enumerate(partition))
    assert np.array_equal(plain.astype(np.float32), pz.host_eval(dim, rows, partition, tables))
    assert np.array_equal(mirrored, rf.reflected_sum(dim, rows, partition, tables))
