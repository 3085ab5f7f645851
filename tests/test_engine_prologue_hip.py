"""GPU: the engine's kernels at the shapes where a launch's opening reads matter — batches smaller than a 16-parent tile
and ragged last tiles, OPEN shorter than the batch, several instances with their own control blocks, launches after the
search has finished, weights changed between two replays of one cached graph, and solved children on their way through
OPEN.  Every case follows the oracle step by step (PY: |OPEN| / |CLOSED| / generated per iteration exactly; CPP: nodes
generated per iteration exactly — equal float32 costs may pop in another order there)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HID = 1  # KNUTH3: cost ties are rare


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    return c_oracle


SCRAMBLES = {
    "cube3": [3, 8, 1, 10, 6, 4, 11, 2, 9, 0],
    "puzzle15": [1, 3, 1, 1, 3, 0, 2, 0, 3, 1, 1, 2],
    "lightsout7": [3, 17, 40, 22, 9, 31, 45, 12],
}


def start_state(co, env, moves):
    if env == "cube3":
        s = np.arange(54, dtype=np.uint8)[None]
    elif env == "lightsout7":
        s = np.zeros((1, 49), np.uint8)
    else:
        s = np.concatenate((np.arange(1, 16), [0])).astype(np.uint8)[None]
    for a in moves:
        s = co.next_state(env, s, a)
    return s[0]


def begin(L, eng, root, hid=HID, instance=0):
    eng.reset(root, instance)
    if eng.semantics == L.SEM_PY:
        eng.root_commit(L.heuristic_builtin(hid, torch.from_numpy(root[None].copy()).cuda()), instance)


def row(st):
    return (st["open_size"], st["closed_size"], st["nodes_generated"])


def same(a, b):
    """two status / counter dicts, NaN equal to NaN (best_cost of a search without a goal yet)"""
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def check_row(st, ref, it, py, what):
    """status after iteration `it` (0-based) against the oracle's trace; a finished search stays where it ended"""
    k = min(it, ref["iterations"] - 1)
    want = tuple(int(v) for v in ref["trace"][k])
    if py:
        assert row(st) == want, (what, it, row(st), want)
    else:
        assert st["nodes_generated"] == want[2], (what, it, row(st), want)
    assert st["iterations"] == k + 1, (what, it, st["iterations"])


ITERS = 12


@pytest.mark.parametrize("sem", ["py", "cpp"])
@pytest.mark.parametrize("B", [1, 3, 17, 33])
@pytest.mark.parametrize("env", ["cube3", "puzzle15", "lightsout7"])
def test_small_and_ragged_batches_follow_the_oracle(L, co, env, B, sem):
    """A batch below one 16-parent tile (1, 3), one tile plus one parent (17) and two tiles plus one (33): 12 iterations,
    one eager launch sequence at a time, then the same search replayed as two graph chunks."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    py = sem == "py"
    root = start_state(co, env, SCRAMBLES[env])
    ref = co.astar(env, root, 0.8, B, co.SEM_PY if py else co.SEM_CPP, heur_builtin_id=HID, max_iters=ITERS, trace_cap=ITERS)
    assert 1 <= ref["iterations"] <= ITERS
    eng = BwasEngine(env, 0.8, B, max_nodes=1 << 16, semantics=L.SEM_PY if py else L.SEM_CPP)
    begin(L, eng, root)
    for it in range(ITERS):
        eng.run_builtin(HID, 1)
        st = eng.status()
        assert not st["failed"]
        check_row(st, ref, it, py, "eager")
    begin(L, eng, root)
    done = 0
    for n in (5, 7):
        eng.run_builtin(HID, n, use_graph=True)
        done += n
        check_row(eng.status(), ref, done - 1, py, "graph")
    eng.close()


def test_each_instance_reads_its_own_control_block(L, co):
    """K = 3: a deep root, a shallow one and a root one move from the goal, batch 17 — the instances fill their batches
    differently and finish at different iterations, in one launch sequence."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    B = 17
    roots = [start_state(co, "cube3", m) for m in ([3, 8, 1, 10, 6], [0, 5], [7])]
    refs = [co.astar("cube3", r, 0.8, B, co.SEM_PY, heur_builtin_id=HID, trace_cap=100000) for r in roots]
    assert all(r["solved"] for r in refs) and len({r["iterations"] for r in refs}) == 3
    for graph in (False, True):
        eng = BwasEngine("cube3", 0.8, B, max_nodes=1 << 20, num_instances=3)
        for i, r in enumerate(roots):
            begin(L, eng, r, instance=i)
        for it in range(max(r["iterations"] for r in refs)):
            eng.run_builtin(HID, 1, use_graph=graph)
            for i, ref in enumerate(refs):
                st = eng.status(i)
                check_row(st, ref, it, True, "instance %d" % i)
                assert bool(st["done"]) == (it >= ref["iterations"] - 1)
        for i, ref in enumerate(refs):
            res = eng._result(i)
            assert res["moves"] == ref["moves"] and res["nodes_generated"] == ref["nodes_generated"]
        eng.close()


@pytest.mark.parametrize("sem", ["py", "cpp"])
def test_launches_after_the_end_change_nothing(L, co, sem):
    """Stepped with several times the iterations the search needs: what a launch reads ahead of its `done` test must have
    no effect — status, the engine's counters, the pool size and the solution stay as they were when it finished."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    py = sem == "py"
    root = start_state(co, "cube3", [3, 8, 1, 10, 6])
    ref = co.astar("cube3", root, 0.8, 33, co.SEM_PY if py else co.SEM_CPP, heur_builtin_id=HID, trace_cap=100000)
    assert ref["solved"]
    eng = BwasEngine("cube3", 0.8, 33, max_nodes=1 << 18, semantics=L.SEM_PY if py else L.SEM_CPP)
    begin(L, eng, root)
    for _ in range(ref["iterations"]):
        eng.run_builtin(HID, 1)
    st0, dbg0, sol0 = eng.status(), eng.debug(), eng.solution()
    assert st0["done"] and not st0["failed"] and st0["iterations"] == ref["iterations"]
    assert st0["nodes_generated"] == ref["nodes_generated"] and sol0[0] == ref["moves"]
    for graph in (False, True):
        eng.run_builtin(HID, 5 * ref["iterations"] + 7, use_graph=graph)
        assert same(eng.status(), st0) and eng.solution() == sol0, (graph, eng.status(), st0)
        assert same(eng.debug(), dbg0), (graph, eng.debug(), dbg0)
    eng.close()


@pytest.mark.parametrize("env,scr,B,sem", [("puzzle15", SCRAMBLES["puzzle15"], 33, "py"),
                                           ("puzzle15", SCRAMBLES["puzzle15"], 33, "cpp"),
                                           ("cube3", [4, 9], 64, "cpp"), ("cube3", [4, 9, 1], 200, "cpp")])
def test_open_shorter_than_the_batch(L, co, env, scr, B, sem):
    """A 15-puzzle's OPEN grows by two or three children per parent, so the pop asks for fewer than B entries for several
    iterations; CPP semantics with a root two or three moves from the goal stop the pop at the first solved node, in the
    middle of a batch that OPEN could not fill either."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    py = sem == "py"
    root = start_state(co, env, scr)
    ref = co.astar(env, root, 0.8, B, co.SEM_PY if py else co.SEM_CPP, heur_builtin_id=HID, trace_cap=100000)
    assert ref["solved"]
    if env == "puzzle15":  # (the test is about iterations whose batch OPEN cannot fill)
        assert sum(1 for k in range(1, len(ref["trace"])) if ref["trace"][k - 1][0] < B) >= 3
    eng = BwasEngine(env, 0.8, B, max_nodes=1 << 18, semantics=L.SEM_PY if py else L.SEM_CPP)
    begin(L, eng, root)
    for it in range(ref["iterations"]):
        eng.run_builtin(HID, 1)
        check_row(eng.status(), ref, it, py, "eager")
    res = eng._result()
    assert res["solved"] and res["moves"] == ref["moves"] and res["nodes_generated"] == ref["nodes_generated"]
    if py:
        assert res["nodes_expanded"] == ref["nodes_expanded"]
    r2 = eng.solve_builtin(root, HID, chunk=3, use_graph=True)
    assert r2["moves"] == ref["moves"] and r2["nodes_generated"] == ref["nodes_generated"]
    eng.close()


def test_device_weights_between_two_replays_of_one_graph(L, co):
    """The instance descriptors are read from device memory by every launch: dca_engine_set_weights_dev between two
    replays of the SAME cached graph (same chunk length after a reset: same pattern of rebase iterations) must make the
    second replay search with the new weight."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    root = start_state(co, "cube3", SCRAMBLES["cube3"])
    n = 16
    refs = {w: co.astar("cube3", root, w, 33, co.SEM_PY, heur_builtin_id=HID, max_iters=n, trace_cap=n) for w in (1.0, 0.2)}
    assert tuple(refs[1.0]["trace"][-1]) != tuple(refs[0.2]["trace"][-1])  # (the test can tell the weights apart)
    eng = BwasEngine("cube3", 1.0, 33, max_nodes=1 << 18)
    begin(L, eng, root)
    eng.run_builtin(HID, n, use_graph=True)
    check_row(eng.status(), refs[1.0], n - 1, True, "w=1.0")
    begin(L, eng, root)  # (the root's cost is w * 0 + h: the same under either weight)
    eng.set_weights_dev(torch.tensor([0.2], dtype=torch.float64, device="cuda"))
    eng.run_builtin(HID, n, use_graph=True)
    check_row(eng.status(), refs[0.2], n - 1, True, "w=0.2")
    eng.close()


@pytest.mark.parametrize("sem", ["py", "cpp"])
@pytest.mark.parametrize("env,scr,B", [("cube3", [2, 9, 4], 17), ("cube3", [2, 9, 4], 200), ("puzzle15", [1, 3, 1, 1], 3)])
def test_solved_children_travel_through_open(L, co, env, scr, B, sem):
    """Heuristic 0, weight 1: uniform-cost search, goals after a handful of iterations.  A solved child is kept, pushed with
    the solved flag in bit 31 of its OPEN id and popped as a goal one iteration later.  (CPP: every cost ties with many
    others, so only what does not depend on the order among equal costs is compared.)"""
    from deepcubea_amd.search_methods.engine import BwasEngine
    py = sem == "py"
    root = start_state(co, env, scr)
    ref = co.astar(env, root, 1.0, B, co.SEM_PY if py else co.SEM_CPP, heur_builtin_id=L.HEUR_ZERO, trace_cap=100000)
    assert ref["solved"] and 2 <= len(ref["moves"]) <= len(scr)
    eng = BwasEngine(env, 1.0, B, max_nodes=1 << 18, semantics=L.SEM_PY if py else L.SEM_CPP)
    for graph in (False, True):
        begin(L, eng, root, hid=L.HEUR_ZERO)
        for it in range(4 * ref["iterations"]):
            eng.run_builtin(L.HEUR_ZERO, 1, use_graph=graph)
            st = eng.status()
            if py:
                check_row(st, ref, it, True, "graph" if graph else "eager")
            if st["done"]:
                break
        res = eng._result()
        assert res["solved"] and len(res["moves"]) == len(ref["moves"]) and res["path_cost"] == ref["path_cost"]
        if py:
            assert res["moves"] == ref["moves"] and res["nodes_generated"] == ref["nodes_generated"]
            assert res["iterations"] == ref["iterations"]
        s = root[None].copy()
        for a in res["moves"]:
            s = co.next_state(env, s, a)
        assert co.is_solved(env, s)[0]
    eng.close()
