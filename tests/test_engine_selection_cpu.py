"""CPU: the conditions test_engine_selection_hip.py rests on, checked against the oracle alone (no GPU).

Every (env, batch, schedule, iterations) tuple of `_selection_schedules.CASES` — the list the GPU file is parametrised
with — is run here: the heuristic is called once per iteration plus once for the root and sees npop*A rows, no case reaches
a goal inside its iteration cap, every schedule produces what its name promises, the creeping cases cross the 512/513 and
1024/1025 marks, and the cases the GPU file asks "a giant bin with more than one distinct key" of can answer it."""
import numpy as np
import pytest

from tests import _selection_schedules as ss

RUNS = sorted(set(c[:4] for c in ss.CASES))


def run_id(run):
    return ss.case_id(run + ("",))


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    c_oracle.lib()
    return c_oracle


def test_row_hash_is_the_documented_mix():
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 256, (2000, 54), dtype=np.uint8)
    rows[1] = rows[0]
    rows[2] = rows[0]
    rows[2, 53] ^= 1
    h = ss.row_hash(rows)
    assert h.dtype == np.uint64 and h.shape == (2000,)
    M = (1 << 64) - 1
    for i in (0, 2, 1999):
        x = 0xCBF29CE484222325
        for b in rows[i].tolist():
            x = ((x ^ b) * 0x100000001B3) & M
        x ^= x >> 29
        x = (x * 0xBF58476D1CE4E5B9) & M
        x ^= x >> 32
        assert int(h[i]) == x
    assert h[0] == h[1] and h[0] != h[2] and len(np.unique(h)) == 1999
    # `hash % q` is close to uniform for the q the schedules use
    big = ss.row_hash(rng.integers(0, 256, (1 << 16, 16), dtype=np.uint8))
    for q in (2, 3, 64, 120):
        cnt = np.bincount((big % np.uint64(q)).astype(np.int64), minlength=q)
        assert cnt.min() > 0.8 * len(big) / q and cnt.max() < 1.2 * len(big) / q, (q, cnt.min(), cnt.max())


def test_deep_roots_are_fixed_and_unsolved(co):
    for env in ss.WALK:
        a, b = ss.deep_root(co, env, 0), ss.deep_root(co, env, 0)
        assert np.array_equal(a, b) and not co.is_solved(env, a[None])[0]
        assert not np.array_equal(a, ss.deep_root(co, env, 1))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_call_count_rows_and_no_goal(co, run):
    env, B, name, iters = run
    res, rec = ss.oracle_run(co, env, B, name, iters)
    A = co.num_moves(env)
    assert not res["solved"] and res["iterations"] == iters and res["moves"] is None
    assert len(rec) == iters + 1 and rec[0][0] == 1
    open_before = np.concatenate([[1], res["trace"][:-1, 0]])
    for i in range(iters):
        assert rec[i + 1][0] == min(B, int(open_before[i])) * A, i
        assert rec[i + 1][1].shape == rec[i + 1][2].shape == (rec[i + 1][0],) and rec[i + 1][2].dtype == np.float32
    assert int(res["trace"][-1, 2]) == sum(r[0] for r in rec[1:]) == res["nodes_generated"]


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_schedule_gives_what_its_name_promises(co, run):
    env, B, name, iters = run
    res, rec = ss.oracle_run(co, env, B, name, iters)
    sched = ss.SCHEDULES[name]
    allv = np.concatenate([r[2] for r in rec])
    big = [k for k, r in enumerate(rec) if r[0] >= 8000]  # calls with enough rows to show every level
    u100, u1 = ss.ulp32(100.0), ss.ulp32(1.0)
    assert u100 == 2.0 ** -17 and u1 == 2.0 ** -23
    lv = np.round((allv.astype(np.float64) - 100.0) / u100)
    if name == "one_level":
        assert all(len(np.unique(r[2])) == 1 for r in rec) and np.all(allv == np.float32(100.0))
    elif name.startswith("ulp_levels"):
        q = sched.q
        assert np.array_equal(100.0 + lv * u100, allv.astype(np.float64)) and lv.min() >= 0 and lv.max() < q
        assert all(len(np.unique(r[2])) <= q for r in rec)
        if len(allv) >= 50 * q:
            assert len(np.unique(allv)) == q
        if q == 4096 and big:
            assert max(len(np.unique(rec[k][2])) for k in big) > 3000
        # as float64 keys the levels differ from bit 29 upwards only
        assert not np.any(allv.astype(np.float64).view(np.uint64) & np.uint64((1 << 29) - 1))
    elif name.startswith("outlier"):
        out = allv == ss.OUTLIER
        assert sum(int((r[2] == ss.OUTLIER).sum()) for r in rec[:4]) >= 1  # the key range is blown up before call 4
        if len(allv) >= 100000:
            assert 0.0005 < out.mean() < 0.002, out.mean()
        o = lv[~out]
        assert np.array_equal(100.0 + o * u100, allv[~out].astype(np.float64)) and o.min() >= 0 and o.max() < sched.q
        if len(allv) >= 50 * sched.q:
            assert len(np.unique(allv[~out])) == sched.q
    elif name.startswith("regime"):
        phases = [sched.phase(k) for k in range(len(rec))]
        if iters > sched.t2:
            assert set(phases) == {0, 1, 2}
        for k, r in enumerate(rec):
            v = r[2].astype(np.float64)
            if phases[k] == 0:
                assert v.min() >= 100.0 and v.max() <= 100.0 + 63 * u100
            elif phases[k] == 1:
                assert v.min() >= 1.0 and v.max() <= 1.0 + 63 * u1
            else:
                assert v.min() >= 5000.0 and v.max() <= 5000.0 + 4095 and np.array_equal(v, np.round(v))
            if k in big:
                assert len(np.unique(v)) == 64 if phases[k] < 2 else len(np.unique(v)) > 3000, (k, len(np.unique(v)))
    elif name == "depth_micro":
        assert sched.weight == 1.0 and set(np.unique(allv).tolist()) == {0.0, 2.0 ** -20, 2.0 ** -19}
        assert all(len(np.unique(rec[k][2])) == 3 for k in big) and big
    elif name == "wide":
        m, e = np.frexp(allv.astype(np.float64))
        assert sched.weight == 0.5 and np.all(m == 0.5) and e.min() == -59 and e.max() == 60 and len(np.unique(allv)) == 120
    else:
        raise AssertionError("no structural check for schedule %s" % name)


@pytest.mark.parametrize("name", ["one_level", "ulp_levels(2)", "outlier(2)"])
def test_creeping_cases_cross_the_size_boundaries(co, name):
    """|OPEN| grows by 0-2 entries per iteration through 512/513 and 1024/1025.  The bin the pop orders is all of OPEN under
    one_level and all but the outliers under outlier(2) (the outlier's key range leaves one bin for the two ordinary keys)."""
    assert ("puzzle15", 1, name, 1400, "") in ss.CASES
    res, rec = ss.oracle_run(co, "puzzle15", 1, name, 1400)
    o = res["trace"][:, 0]
    assert np.all(np.abs(np.diff(o)) <= 2)
    for lo, hi in ((505, 512), (513, 520), (1017, 1024), (1025, 1032)):
        assert np.any((o >= lo) & (o <= hi)), (lo, hi)
    if name != "ulp_levels(2)":
        cen = ss.open_census(rec, 1, 4, 0.0, res["trace"])
        ordinary = np.array([sum(v for c, v in x.items() if c < 1e38) for x in cen])
        for lo, hi in ((505, 512), (513, 520), (1017, 1024), (1025, 1032)):
            assert np.any((ordinary >= lo) & (ordinary <= hi)), (lo, hi)
        if name == "outlier(2)":
            assert all(len([c for c in x if c < 1e38]) == 2 for x in cen[200:])  # both ordinary keys are always present


@pytest.mark.parametrize("name", ["outlier", "regime", "depth_micro"])
def test_no_single_cost_can_fill_a_giant_bin(co, name):
    """The GPU file's `distinct` reach assertion (a bin of more than 8192 entries that holds more entries than any one cost
    has in OPEN) needs OPEN to outgrow 8192 entries; under outlier and regime no cost ever has 8192 entries, so there EVERY
    bin beyond that size mixes distinct keys.  The replay the census comes from checks itself against the oracle's trace."""
    from tests.test_engine_selection_hip import reach_of
    case = ("cube3", 700, name, 34, "")
    assert case in ss.CASES and "distinct" in reach_of(case)
    res, rec = ss.oracle_run(co, "cube3", 700, name, 34)
    cen = ss.open_census(rec, 700, 12, ss.SCHEDULES[name].weight, res["trace"])
    assert len(cen) == 34 and [sum(c.values()) for c in cen[1:]] == res["trace"][:-1, 0].tolist()
    assert sum(cen[3].values()) < 8192 < sum(cen[5].values())  # OPEN passes 8192 entries early in the run
    assert all(len(c) > 1 for c in cen[2:])
    if name != "depth_micro":
        assert max(max(c.values()) for c in cen) < 8192
