"""GPU: the expansion's parent gather and per-child arithmetic (k_expand) at every row length the engine instantiates
(9, 16, 25, 36, 49, 49 and 54 bytes) and every raggedness of its 16-parent tiles.  The gather fetches a row as dwords — the
tail word of a row whose length is no multiple of 4 as the dword that ENDS at the row's last byte — beside the parent's path
cost and move; is_solved compares 8-byte words with the last one masked to the row; the built-in heuristics' byte sum is a
32-bit sum.  Nothing of that may show: every case follows the C++ oracle step by step through the C ABI (PY semantics:
|OPEN|, |CLOSED| and nodes generated per iteration exactly; cpp semantics: nodes generated exactly — equal float32 costs may
pop in another order there).  puzzle8, which the oracle does not know, follows the sequential model of
tests/test_engine_known_dup_hip.py."""
import numpy as np
import pytest
import torch

from test_engine_known_dup_hip import expand_host, heur_host, model_bwas, puzzle_dim, walk

pytestmark = pytest.mark.gpu

PY, CPP = 0, 1
MOD97, KNUTH3, HASHU01, MANHATTAN = 0, 1, 2, 4
ENVS = ["puzzle8", "puzzle15", "puzzle24", "puzzle35", "puzzle48", "lightsout7", "cube3"]  # D = 9 16 25 36 49 49 54
PUZZLE_WALK = [1, 3, 1, 1, 3, 0, 2, 0, 3, 1]  # (the 3 x 3 board runs into its edge twice on the way: those moves change nothing)
WALKS = {"cube3": [3, 8, 1, 10, 6, 4, 11, 2], "lightsout7": [3, 17, 40, 22, 9, 31, 45, 12]}
NEAR = {"cube3": [4], "lightsout7": [24]}  # one move from the goal; the puzzles: the blank one step up
ITERS = 9


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    return c_oracle


def root_of(L, co, env, near=False):
    if near:
        return walk(L, co, env, NEAR.get(env, [1]))
    return walk(L, co, env, WALKS.get(env, PUZZLE_WALK))


_REF = {}


def reference(L, co, env, root, w, B, sem, hid, iters):
    """-> (trace [k, 3], solved, moves), computed once per case: the oracle's run; the model's for puzzle8"""
    case = (env, root.tobytes(), w, B, sem, hid, iters)
    if case not in _REF:
        if env == "puzzle8":
            _REF[case] = model_bwas(L, co, env, root, w, B, sem, hid, iters)
        else:
            kw = dict(heur_fn=lambda X: heur_host(co, env, MANHATTAN, X)) if hid == MANHATTAN else dict(heur_builtin_id=hid)
            r = co.astar(env, root, w, B, co.SEM_PY if sem == PY else co.SEM_CPP, max_iters=iters, trace_cap=iters, **kw)
            _REF[case] = (np.array(r["trace"][:r["iterations"]], np.int64).reshape(-1, 3), bool(r["solved"]), list(r["moves"] or []))
    return _REF[case]


def begin(L, eng, root, hid, instance=0):
    eng.reset(root, instance)
    if eng.semantics == L.SEM_PY:
        eng.root_commit(L.heuristic_builtin(hid, torch.from_numpy(root[None].copy()).cuda()), instance)


def check_row(st, trace, it, sem, what):
    k = min(it, len(trace) - 1)  # a finished search stays where it ended
    got, want = (st["open_size"], st["closed_size"], st["nodes_generated"]), tuple(int(v) for v in trace[k])
    if sem == PY:
        assert got == want, (what, it, got, want)
    else:
        assert got[2] == want[2], (what, it, got, want)


def hids_of(env):
    return [MOD97, KNUTH3, HASHU01] + ([MANHATTAN] if puzzle_dim(env) else [])


# ------------------------------------------------------------------------------------------------ 1. traces
@pytest.mark.parametrize("env", ENVS)
def test_trace_at_every_row_length_and_tile_raggedness(L, co, env):
    """Batches of 1 (one lane group of the tile at work), 15, 16 (one parent short of a tile, a full tile), 17 and 33 (one and two
    tiles plus one parent), both semantics, the heuristics that read the byte sum (MOD97, KNUTH3), the hash (HASHU01) and, on
    the puzzles, MANHATTAN: nine iterations from a short scramble."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    root = root_of(L, co, env)
    for sem in (PY, CPP):
        for B in (1, 15, 16, 17, 33):
            eng = BwasEngine(env, 0.8, B, max_nodes=1 << 15, semantics=L.SEM_PY if sem == PY else L.SEM_CPP)
            for hid in hids_of(env):
                trace, _, _ = reference(L, co, env, root, 0.8, B, sem, hid, ITERS)
                assert 1 <= len(trace) <= ITERS
                begin(L, eng, root, hid)
                for it in range(ITERS):
                    eng.run_builtin(hid, 1)
                    st = eng.status()
                    assert not st["failed"]
                    check_row(st, trace, it, sem, (env, sem, B, hid))
            eng.close()


# ------------------------------------------------------------------------------------------------ 2. rows
@pytest.mark.parametrize("env", ENVS)
def test_child_rows_equal_the_cpu_expansion_of_the_popped_parents(L, co, env):
    """B = 17, stepped with the two-call interface (the launch then writes the network-input rows as well) until a pop takes all
    17 parents — two tiles, the second with one parent: after every pop the node pool's child rows are, row for row, the CPU's
    children of the parents just popped, and the network-input rows are those rows (cube3: sticker // 9)."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    B = 17
    root = root_of(L, co, env)
    eng = BwasEngine(env, 0.8, B, max_nodes=1 << 15)
    begin(L, eng, root, KNUTH3)
    full = False
    for _ in range(12):
        nn, _ = eng.pop_expand()
        st, fl = eng.last_popped()
        par = st.cpu().numpy()[fl.cpu().numpy() != 0]
        ch = eng.last_children()
        want = expand_host(L, co, env, par)
        got = ch.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (env, len(par))
        assert np.array_equal(nn[:len(want)].cpu().numpy(), want // 9 if env == "cube3" else want)
        h = torch.zeros(eng.m_capacity, dtype=torch.float32, device="cuda")
        h[:len(want)] = L.heuristic_builtin(KNUTH3, ch.contiguous())
        eng.commit(h)
        full = full or len(par) == B
        if full or eng.status()["done"]:
            break
    assert full, env
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. solved children
@pytest.mark.parametrize("sem", [PY, CPP])
@pytest.mark.parametrize("env", ENVS)
def test_a_solved_child_ends_the_search_as_the_oracles(L, co, env, sem):
    """A root one move from the goal: the first expansion makes a solved child (is_solved on 8-byte words, the last one masked for
    D = 9, 25, 49 and 54), which is pushed with its flag, popped and ends the search — at the iteration, with the counters and with
    the moves of the reference."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    root = root_of(L, co, env, near=True)
    for B in (1, 17):
        trace, solved, moves = reference(L, co, env, root, 0.8, B, sem, KNUTH3, 64)
        assert solved and len(moves) == 1
        eng = BwasEngine(env, 0.8, B, max_nodes=1 << 15, semantics=L.SEM_PY if sem == PY else L.SEM_CPP)
        begin(L, eng, root, KNUTH3)
        for it in range(len(trace)):
            assert not eng.status()["done"], (env, sem, B, it)
            eng.run_builtin(KNUTH3, 1)
            check_row(eng.status(), trace, it, sem, (env, sem, B))
        res = eng._result()
        assert res["solved"] and res["moves"] == moves and res["iterations"] == len(trace), (env, sem, B, res)
        assert res["nodes_generated"] == int(trace[-1][2])
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. two instances
@pytest.mark.parametrize("env,walks", [("cube3", ([3, 8, 1, 10, 6, 4, 11, 2], [7, 0, 11, 5])),
                                       ("puzzle24", (PUZZLE_WALK, [3, 3, 1, 1, 2, 0]))])
def test_two_instances_on_different_roots(L, co, env, walks):
    """grid.y = 2, B = 17: each instance gathers from its own pool through its own descriptor."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    B = 17
    roots = [walk(L, co, env, s) for s in walks]
    for sem in (PY, CPP):
        refs = [reference(L, co, env, r, 0.8, B, sem, KNUTH3, ITERS)[0] for r in roots]
        eng = BwasEngine(env, 0.8, B, max_nodes=1 << 15, semantics=L.SEM_PY if sem == PY else L.SEM_CPP, num_instances=2)
        for i, r in enumerate(roots):
            begin(L, eng, r, KNUTH3, i)
        for it in range(ITERS):
            eng.run_builtin(KNUTH3, 1)
            for i, trace in enumerate(refs):
                check_row(eng.status(i), trace, it, sem, (env, sem, i))
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. the pool's end
def test_trace_up_to_the_iteration_that_fills_the_pool(L, co):
    """puzzle24, B = 17, a pool of 640 nodes: the search follows the oracle until an expansion no longer fits, reports failure
    there — not before the pool is really short of a batch — and leaves the counters of the last complete iteration."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    env, B, cap, n = "puzzle24", 17, 640, 40
    root = root_of(L, co, env)
    trace, solved, _ = reference(L, co, env, root, 0.8, B, PY, KNUTH3, n)
    assert not solved and int(trace[-1][2]) > 2 * cap
    eng = BwasEngine(env, 0.8, B, max_nodes=cap)
    begin(L, eng, root, KNUTH3)
    last = None
    for it in range(n):
        eng.run_builtin(KNUTH3, 1)
        st = eng.status()
        if st["failed"]:
            break
        check_row(st, trace, it, PY, "before the pool's end")
        last = st
    assert st["failed"] and st["done"] and last is not None
    # ids are handed out in 16-aligned batches: the root, then per iteration at most 15 ids of padding and the children
    assert last["nodes_generated"] + 16 * (it + 1) + B * 4 + 1 > cap, (it, last)
    assert (st["open_size"], st["closed_size"], st["nodes_generated"]) == (last["open_size"], last["closed_size"], last["nodes_generated"])
    eng.close()
