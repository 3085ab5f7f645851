"""GPU: cube3's child rows in k_expand.  The kernel builds them in registers, one constant byte-permute body per move
(cube3_child_words, dca_tile.h), with three moves in each of a workgroup's four waves: lane t holds parent t & 15 and move
3 * (t >> 6) + ((t >> 4) & 3).  The lane-to-child map is a bijection on the tile's children and nothing of it may show: after
every pop the node pool's child rows are, row for row and for all 12 moves of every parent, the CPU's children of the popped
parents in pop order, the network-input rows are those rows // 9, the one-hot rows their one-hot, and every search follows the
C++ oracle's trace (PY semantics: |OPEN|, |CLOSED| and nodes generated per iteration exactly; cpp semantics: nodes generated
exactly — equal float32 costs may pop in another order there).  Batches of 1 (one lane group), 15 (a ragged
tile), 16 (a full tile), 17 and 33 (one and two tiles plus one parent); built-in heuristic throughout."""
import numpy as np
import pytest
import torch

from test_engine_known_dup_hip import expand_host, walk

pytestmark = pytest.mark.gpu

PY, CPP = 0, 1
KNUTH3 = 1
ENV = "cube3"
WALK = [3, 8, 1, 10, 6, 4, 11, 2]  # (the 8-move walk of tests/test_engine_gather_hip.py)
NEAR = [4]  # one move from the goal: is_solved fires on a child of the first expansion
BATCHES = (1, 15, 16, 17, 33)
ITERS = 6
NEAR_ITERS = 64  # (bound on the search from the near root: the oracle's ends well before)


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    return c_oracle


_REF = {}


def reference(co, root, B, sem, iters=ITERS):
    """-> (trace [k, 3], solved, moves): the oracle's search from `root`, computed once per case"""
    case = (root.tobytes(), B, sem, iters)
    if case not in _REF:
        r = co.astar(ENV, root, 0.8, B, co.SEM_PY if sem == PY else co.SEM_CPP, max_iters=iters, trace_cap=iters,
                     heur_builtin_id=KNUTH3)
        _REF[case] = (np.array(r["trace"][:r["iterations"]], np.int64).reshape(-1, 3), bool(r["solved"]), list(r["moves"] or []))
    return _REF[case]


def engine(L, B, sem, **kw):
    from deepcubea_amd.search_methods.engine import BwasEngine
    return BwasEngine(ENV, 0.8, B, max_nodes=1 << 15, semantics=L.SEM_PY if sem == PY else L.SEM_CPP, **kw)


def begin(L, eng, root, instance=0):
    eng.reset(root, instance)
    if eng.semantics == L.SEM_PY:
        eng.root_commit(L.heuristic_builtin(KNUTH3, torch.from_numpy(root[None].copy()).cuda()), instance)


def check_row(st, trace, it, sem, what):
    k = min(it, len(trace) - 1)  # a finished search stays where it ended
    got, want = (st["open_size"], st["closed_size"], st["nodes_generated"]), tuple(int(v) for v in trace[k])
    if sem == PY:
        assert got == want, (what, it, got, want)
    else:
        assert got[2] == want[2], (what, it, got, want)


def onehot_of(rows):
    """[n, 54 * 6] float32: index = position * 6 + colour (pytorch_models.py:49-52)"""
    return np.eye(6, dtype=np.float32)[rows // 9].reshape(len(rows), -1)


def step_and_check_rows(L, co, eng, sem, traces, it, what, onehot=False):
    """One iteration in two calls: pop and expand, compare every instance's rows with the CPU's children of its popped parents,
    commit the built-in heuristic of those rows, compare the counters with the oracle's.  -> parents popped, per instance"""
    K, B, M = eng.num_instances, eng.batch_size, eng.batch_size * 12
    nn, oh = eng.pop_expand()
    st, fl = eng.last_popped()
    st, fl = st.cpu().numpy(), fl.cpu().numpy()
    h = torch.zeros(eng.m_capacity, dtype=torch.float32, device="cuda")
    npar = []
    for i in range(K):
        par = st[i * B:(i + 1) * B][fl[i * B:(i + 1) * B] != 0]
        want = expand_host(L, co, ENV, par) if len(par) else np.zeros((0, 54), np.uint8)
        n = len(want)
        assert n == 12 * len(par)
        if i == 0:  # (the node pool's rows of the last batch: instance 0's)
            got = eng.last_children().cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (what, it, len(par))
        assert np.array_equal(nn[i * M:i * M + n].cpu().numpy(), want // 9), (what, it, i, len(par))
        if onehot:
            assert oh is not None and oh.dtype == torch.float32
            assert np.array_equal(oh[i * M:i * M + n].cpu().numpy(), onehot_of(want)), (what, it, i, len(par))
        if n:
            h[i * M:i * M + n] = L.heuristic_builtin(KNUTH3, torch.from_numpy(want).cuda())
        npar.append(len(par))
    eng.commit(h)
    for i in range(K):
        s = eng.status(i)
        assert not s["failed"]
        check_row(s, traces[i], it, sem, (what, i))
    return npar


def run_rows(L, co, eng, sem, roots, what, onehot=False, iters=ITERS):
    traces = [reference(co, r, eng.batch_size, sem, iters)[0] for r in roots]
    for i, r in enumerate(roots):
        begin(L, eng, r, i)
    most = 0
    for it in range(iters):
        if all(eng.status(i)["done"] for i in range(len(roots))):
            break
        most = max(most, max(step_and_check_rows(L, co, eng, sem, traces, it, what, onehot)))
    return most


def run_fused(L, co, eng, sem, root, what, iters=ITERS):
    """the same search with the fused stepping (one launch sequence per iteration, no network-input rows)"""
    trace = reference(co, root, eng.batch_size, sem, iters)[0]
    begin(L, eng, root)
    for it in range(min(iters, len(trace))):
        eng.run_builtin(KNUTH3, 1)
        st = eng.status()
        assert not st["failed"]
        check_row(st, trace, it, sem, what)


# ------------------------------------------------------------------------------------------------ 1. every tile shape
@pytest.mark.parametrize("sem", [PY, CPP])
@pytest.mark.parametrize("B", BATCHES)
def test_rows_and_trace_at_every_tile_raggedness(L, co, B, sem):
    """The 8-move walk for six iterations, and the root one move from the goal to the end of its search (the first expansion makes
    a solved child, which is pushed with its flag, popped and ends the search where and as the oracle's ends): stepped in two
    calls, the rows compared after every pop, and fused."""
    eng = engine(L, B, sem)
    far, near = walk(L, co, ENV, WALK), walk(L, co, ENV, NEAR)
    most = run_rows(L, co, eng, sem, [far], ("walk", B, sem))
    assert most == B, (B, most)  # some pop of the six took a whole batch: every tile shape of the list was built
    run_fused(L, co, eng, sem, far, ("walk, fused", B, sem))
    trace, solved, moves = reference(co, near, B, sem, NEAR_ITERS)
    assert solved and len(moves) == 1
    for fused in (False, True):
        if fused:
            run_fused(L, co, eng, sem, near, ("near, fused", B, sem), NEAR_ITERS)
        else:
            run_rows(L, co, eng, sem, [near], ("near", B, sem), iters=NEAR_ITERS)
        res = eng._result()
        assert res["solved"] and res["moves"] == moves and res["iterations"] == len(trace), (B, sem, fused, res)
        assert res["nodes_generated"] == int(trace[-1][2])
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. every move
@pytest.mark.parametrize("sem", [PY, CPP])
def test_a_root_reached_by_each_move(L, co, sem):
    """Twelve roots, the last move of each another one of the 12: every move body makes children of every root, and every move
    is some parent's undo child (a known duplicate: never probed, its row written all the same)."""
    eng = engine(L, 17, sem)
    for a in range(12):
        root = walk(L, co, ENV, WALK[:3] + [a])
        run_rows(L, co, eng, sem, [root], ("move", a, sem))
        run_fused(L, co, eng, sem, root, ("move, fused", a, sem))
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. two instances
@pytest.mark.parametrize("sem", [PY, CPP])
def test_two_instances_on_different_roots(L, co, sem):
    """grid.y = 2, B = 17: each instance builds the children of its own parents into its own buffers."""
    eng = engine(L, 17, sem, num_instances=2)
    roots = [walk(L, co, ENV, WALK), walk(L, co, ENV, [7, 0, 11, 5])]
    most = run_rows(L, co, eng, sem, roots, ("two instances", sem))
    assert most == 17
    refs = [reference(co, r, 17, sem)[0] for r in roots]
    for i, r in enumerate(roots):
        begin(L, eng, r, i)
    for it in range(ITERS):
        eng.run_builtin(KNUTH3, 1)
        for i, trace in enumerate(refs):
            check_row(eng.status(i), trace, it, sem, ("two instances, fused", sem, i))
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. one-hot rows
@pytest.mark.parametrize("B", [17, 33])
def test_onehot_rows_are_the_onehot_of_the_expected_children(L, co, B):
    """onehot_dtype = float32 (the launch's OH = 4 instantiation): the one-hot rows against the one-hot of the CPU's child rows."""
    eng = engine(L, B, PY, onehot_dtype=torch.float32)
    most = run_rows(L, co, eng, PY, [walk(L, co, ENV, WALK)], ("onehot", B), onehot=True)
    assert most == B
    eng.close()
