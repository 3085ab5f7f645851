"""GPU: the engine's pop ORDER under adversarial cost distributions (k_sel_scan / k_sel_collect / collect_giant / k_rank /
the hand-back of the threshold bin's overshoot / FRONT-BACK refill and spill).

The other engine tests compare per-iteration counts and the final move list, under costs that real heuristics happen to
produce.  Here the test chooses every child's cost (tests/_selection_schedules.py) and compares, in EVERY iteration, the hashes
of `last_children()` — the batch's children in rank*A + move order — with the oracle's record element for element: which
nodes were popped, in which order, ties included.  The recorded h values are handed back, so no float is recomputed.

Reach assertions (conditions on the inputs, not correctness checks) make a case fail when it misses the path it aims at:
`giant` = a threshold bin beyond k_rank's LDS capacity (8192 entries) was seen; `distinct` = such a bin held more entries
than any single cost has in OPEN (replayed from the record), i.e. more than one distinct key; `creep` = the largest bin took
sizes on both sides of 512 and of 1024; `mid` = bins between 512 and 8192 entries, none above; `tiny` = no bin above 512
entries; `grid_off` = a bin beyond 8192 entries on an engine whose grid-wide refinement is off (`giant_bins_seen` counts the
bins beyond 8192 entries on either path, so it cannot tell the two apart; `info()` does).

Sizing: `max_nodes` is the oracle's node count plus the ids the engine skips (every iteration's children start at a multiple
of 16) plus the usual slack; a pool that runs out stops the search, and the next pop would hand back stale children.

Durations on an MI355X (pytest --durations=0), whole file 10 s: cube3 B=9000 outlier(4096) 1.16 s, regime_fast 1.10 s,
ulp_levels(4096) 0.56 s, regime 0.41 s; puzzle15 B=1 one_level 0.57 s, outlier(2) 0.30 s, ulp_levels(2) 0.27 s; cube3 B=700
with the OPEN replay (outlier, regime, depth_micro, wide, tiny tiers) 0.27-0.34 s each, the other B=700 cases 0.02-0.09 s;
cube3 B=1 / B=64, puzzle15 B=33, lightsout7 B=17 0.01-0.07 s."""
import numpy as np
import pytest

from tests import _selection_schedules as ss

pytestmark = pytest.mark.gpu


def reach_of(case):
    """The path a case must reach.  Evenly spaced levels get a bin each under the adaptive binning — 64 levels of ~3 000
    entries are mid-sized bins, 4096 levels tiny ones, two levels two single-key bins — so what puts DISTINCT keys into one
    bin beyond 8192 entries is the outlier, a stale binning (regime), or a micro-structure below the bin width."""
    env, B, name, iters, variant = case
    collapsing = name.startswith("outlier") or name in ("regime", "regime_fast")
    if variant == "grid_off":
        return ("grid_off",) if collapsing else ("mid",)
    if (env, B) == ("puzzle15", 1):
        return () if name == "ulp_levels(2)" else ("creep",)  # (ulp_levels(2): see the note at _selection_schedules.CASES)
    if (env, B) == ("cube3", 700):  # the main grid and the tiny tiers
        return {"one_level": ("giant",), "ulp_levels(2)": ("giant",), "ulp_levels(64)": ("mid",), "ulp_levels(4096)": ("tiny",),
                "outlier": ("giant", "distinct"), "regime": ("giant", "distinct"), "depth_micro": ("giant", "distinct"),
                "wide": ("giant", "distinct")}[name]
    if (env, B) == ("cube3", 64) and name == "outlier":  # a giant bin refined down to a batch of 64
        return ("giant", "distinct")
    if (env, B) == ("cube3", 9000) and name in ("regime_fast", "outlier(4096)"):  # a batch beyond the LDS capacity out of one bin
        return ("giant", "distinct")
    if env == "lightsout7":
        return ("giant",)
    return ()


def first_mismatch(got, want, A):
    j = int(np.flatnonzero(got != want)[0])
    return "first differing child row %d = pop rank %d, move %d (of %d rows)" % (j, j // A, j % A, len(want))


def follow(case):
    """The one driver: the engine follows the oracle's record iteration by iteration; -> the debug() record."""
    import torch
    from deepcubea_amd import _lib
    from deepcubea_amd.search_methods.engine import BwasEngine
    from oracle import c_oracle as co
    env, B, name, iters, variant = case
    res, rec = ss.oracle_run(co, env, B, name, iters)
    assert not res["solved"] and res["iterations"] == iters and len(rec) == iters + 1
    A = co.num_moves(env)
    w = ss.SCHEDULES[name].weight
    if variant == "grid_off":
        _lib.check(_lib.lib().dca_debug_tune(5, 1), "dca_debug_tune")
    try:
        # (every iteration's children start at a node id that is a multiple of 16: up to 15 ids per iteration are skipped)
        eng = BwasEngine(env, w, B, max_nodes=int(res["nodes_generated"]) + 16 * iters + 4 * B * A + 64)
    finally:
        if variant == "grid_off":
            _lib.check(_lib.lib().dca_debug_tune(5, 0), "dca_debug_tune")
    info = eng.info()
    assert info["grid_refinement"] == (0 if variant == "grid_off" else 1), info
    if variant.startswith("tiers"):
        eng.set_tiers(*[int(v) for v in variant[6:-1].split(",")])
    eng.reset(ss.deep_root(co, env, 0))
    eng.root_commit(torch.from_numpy(rec[0][2].copy()).cuda())
    dbg = []
    h = torch.zeros(eng.m_capacity, dtype=torch.float32, device="cuda")
    for it in range(iters):
        n, want_hash, hv = rec[it + 1]
        eng.pop_expand()
        ch = eng.last_children()
        assert ch.shape[0] == n, "iteration %d: %d children, the oracle has %d; %s" % (it, ch.shape[0], n, dbg[-1:])
        got_hash = ss.row_hash(ch.cpu().numpy())
        if not np.array_equal(got_hash, want_hash):
            st = eng.status()  # (a search that has stopped — node pool exhausted, a goal — pops nothing: stale children)
            raise AssertionError("%s, iteration %d: %s; engine done=%d failed=%d; debug of this pop %s, of the iterations before %s"
                                 % (ss.case_id(case), it, first_mismatch(got_hash, want_hash, A), st["done"], st["failed"],
                                    eng.debug(), dbg[-2:]))
        h[:n] = torch.from_numpy(hv).cuda()
        eng.commit(h)
        st = eng.status()
        assert not st["failed"] and not st["done"], (it, st)
        assert (st["open_size"], st["closed_size"], st["nodes_generated"]) == tuple(int(v) for v in res["trace"][it]), it
        d = eng.debug()
        dbg.append({k: d[k] for k in ("max_bin", "giant_bins_seen", "max_sub", "front_n", "back_n", "n_ord")})
    info = eng.info()
    eng.close()
    return res, rec, dbg, info


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_pop_order_follows_the_oracle(case):
    from oracle import c_oracle as co
    env, B, name, iters, variant = case
    res, rec, dbg, info = follow(case)
    mb = np.array([int(d["max_bin"]) for d in dbg])
    seen = int(dbg[-1]["giant_bins_seen"])
    print("%s: max_bin max %d, giant_bins_seen %d, max_sub max %d, back_n max %d, n_ord max %d, info %s"
          % (ss.case_id(case), mb.max(), seen, max(int(d["max_sub"]) for d in dbg), max(int(d["back_n"]) for d in dbg),
             max(int(d["n_ord"]) for d in dbg), info))
    reach = reach_of(case)
    if "giant" in reach:
        assert seen > 0 and mb.max() > 8192, (seen, mb.max())
        assert info["coop_off"] == 0, info  # (the grid-wide path was never given up)
    if "distinct" in reach:
        # debug() after iteration `it` describes that iteration's pop; census[it] is OPEN as that pop found it
        cen = ss.open_census(rec, B, co.num_moves(env), ss.SCHEDULES[name].weight, res["trace"])
        assert any(mb[it] > 8192 and mb[it] > max(cen[it].values()) for it in range(iters)), \
            [(int(mb[it]), max(cen[it].values())) for it in range(iters)]
    if "mid" in reach:
        assert 512 < mb.max() <= 8192 and seen == 0, (mb.max(), seen)
    if "tiny" in reach:
        assert mb.max() <= 512 and seen == 0, (mb.max(), seen)
    if B > 8192:  # the batch itself is beyond k_rank's LDS capacity
        assert max(int(d["n_ord"]) for d in dbg) > 8192
    if "creep" in reach:
        # (max_bin is only recorded for bins of more than 256 entries)
        assert ((mb > 256) & (mb <= 512)).any() and ((mb > 512) & (mb <= 1024)).any() and (mb > 1024).any(), mb.max()
    if "grid_off" in reach:
        assert mb.max() > 8192 and info["grid_refinement"] == 0, (mb.max(), info)
    if variant.startswith("tiers"):
        assert max(int(d["back_n"]) for d in dbg) > 0  # entries really lived in BACK
