"""GPU: children that the expansion knows to be duplicates from their parent's node fields alone (the undo child, a sliding
puzzle's ineligible move — known_duplicate, dca_common.h) skip the CLOSED probe.  The search must not notice: every case here
compares per-iteration (|OPEN|, |CLOSED|, generated) traces EXACTLY.

References.  `model_bwas` below is a sequential restatement of both BWAS semantics (oracle/dca_oracle.cpp's astar_py / astar_cpp
line for line) that probes CLOSED for every child and orders equal costs by push count — the reference's rule in PY semantics
(astar.py:64-67) and the engine's documented one in cpp semantics ((cost, id)).  It is needed because the C++ oracle
has no 3 x 3 tables (puzzle8) and because its cpp semantics order equal float32 costs as libstdc++'s heap happens to, which is
why tests/test_engine_hip.py compares cpp runs on a heuristic without ties; the zero and Manhattan heuristics asked for here are
nothing but ties.  Wherever the oracle IS a valid exact reference — PY semantics on every environment it knows, cpp semantics on
the tie-free hash heuristic — every case ALSO compares the model against it (`reference`), entry for entry in both semantics
(stricter than test_cpp_semantics_vs_oracle's 1e-2 on |OPEN| / |CLOSED|, which no tie is there to need), so the model cannot
drift from it."""
import heapq

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PY, CPP = 0, 1
HASHU01, ZERO, MANHATTAN = 2, 3, 4


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    return c_oracle


# ------------------------------------------------------------------------------------------------ host restatement
def puzzle_dim(env):
    return {"puzzle8": 3, "puzzle15": 4, "puzzle24": 5, "puzzle35": 6, "puzzle48": 7}.get(env, 0)


def goal_of(env):
    if env == "cube3":
        return np.arange(54, dtype=np.uint8)
    if env == "lightsout7":
        return np.zeros(49, np.uint8)
    n = puzzle_dim(env)
    return np.concatenate((np.arange(1, n * n), [0])).astype(np.uint8)


def expand_host(L, co, env, X):
    """children [n * A, D] of X [n, D]: the C++ oracle's moves; puzzle8 (which it does not know) from the library's swap table."""
    if env != "puzzle8":
        return co.expand(env, X)[0].reshape(-1, X.shape[1])
    swap = L.npuzzle_swap_table(3)
    out = np.empty((X.shape[0], 4, 9), np.uint8)
    for i, s in enumerate(X):
        z = int(np.flatnonzero(s == 0)[0])
        for a in range(4):
            t = int(swap[z, a])
            c = s.copy()
            c[z] = s[t]  # next[z] = cur[s]; next[s] = 0 (n_puzzle.py:226-227; t == z: the move is not eligible, nothing moves)
            c[t] = 0
            out[i, a] = c
    return out.reshape(-1, 9)


def heur_host(co, env, hid, X):
    if hid == MANHATTAN:
        n = puzzle_dim(env)
        pos = np.arange(n * n)
        t = X.astype(np.int64)
        g = t - 1
        d = np.abs(pos // n - g // n) + np.abs(pos % n - g % n)
        return np.where(t == 0, 0, d).sum(1).astype(np.float32)
    return co.heur_builtin(hid, X)  # hash / zero: generic in the row width


def model_bwas(L, co, env, root, w, B, sem, hid, iters):
    """-> (trace [k, 3], solved, moves or None).  Every child goes through CLOSED; equal costs pop in push order.  On the way it
    holds the rule itself to the search: a child the library calls a known duplicate is never kept (host-side, no kernel)."""
    goal = goal_of(env).tobytes()
    e, d, _, A, _ = L.env_ids(env)

    def known(state, g, mv, a):
        blank = state.index(0) if e == L.ENV_NPUZZLE else 0
        return L.engine_known_duplicate(e, d, int(g), 0xFF if mv < 0 else mv, a, blank)

    trace, cnt = [], 0
    heap = []
    if sem == PY:
        key = root.tobytes()
        h0 = max(float(heur_host(co, env, hid, root[None])[0]), 0.0)
        nodes = [(key, 0.0, -1, -1)]  # state, g, parent, move
        heapq.heappush(heap, (w * 0.0 + h0 * (0.0 if key == goal else 1.0), cnt, 0))
        cnt += 1
        closed, gen, goals = {}, 0, []
        while not goals and len(trace) < iters and heap:
            popped = [heapq.heappop(heap)[2] for _ in range(min(B, len(heap)))]
            goals = [i for i in popped if nodes[i][0] == goal]
            ch = expand_host(L, co, env, np.stack([np.frombuffer(nodes[i][0], np.uint8) for i in popped]))
            hv = heur_host(co, env, hid, ch)
            gen += len(ch)
            for j in range(len(ch)):
                k = ch[j].tobytes()
                gp = nodes[popped[j // A]][1] + 1.0
                cost = w * gp + max(float(hv[j]), 0.0) * (0.0 if k == goal else 1.0)  # astar.py:196, float64, two roundings
                old = closed.get(k)
                par = nodes[popped[j // A]]
                assert not (known(par[0], par[1], par[3], j % A) and (old is None or old > gp)), (env, sem, len(trace), j)
                if old is None or old > gp:
                    closed[k] = gp
                    nodes.append((k, gp, popped[j // A], j % A))
                    heapq.heappush(heap, (cost, cnt, len(nodes) - 1))
                    cnt += 1
            trace.append((len(heap), len(closed), gen))
        moves = None
        if goals:
            best = min(goals, key=lambda i: nodes[i][1])  # first on ties (astar.py:327-333)
            moves = []
            while nodes[best][2] >= 0:
                moves.append(nodes[best][3])
                best = nodes[best][2]
            moves.reverse()
        return np.array(trace, np.int64).reshape(-1, 3), bool(goals), moves
    # cpp semantics: float32 costs, the root in CLOSED (a node of its own), pops break at the first solved node, deferred
    # termination, a shallower duplicate rewrites the CLOSED node in place (cpp:160-166, 185-208, 247-265, 298)
    wf = np.float32(w)
    key = root.tobytes()
    heapq.heappush(heap, (0.0, cnt, [key, 0, None, -1]))  # node: state, depth, parent node, move
    cnt += 1
    closed = {key: [key, 0, None, -1]}
    gen, solved_node, is_solved = 1, None, False
    while not is_solved and len(trace) < iters and heap:
        popped, prev = [], solved_node is not None
        for _ in range(min(len(heap), B)):
            c, _, n = heapq.heappop(heap)
            popped.append((c, n))
            if n[0] == goal:
                if B == 1:
                    solved_node, is_solved = (c, n), True
                elif solved_node is None or solved_node[0] > c:
                    solved_node = (c, n)
                break
        if prev and popped[0][0] >= solved_node[0]:
            is_solved = True
        ch = expand_host(L, co, env, np.stack([np.frombuffer(n[0], np.uint8) for _, n in popped]))
        hv = heur_host(co, env, hid, ch)
        gen += len(ch)
        # the children are made before the CLOSED check (cpp:217-230): a popped node that the check rewrites while it runs has
        # handed its children the depth (and the rule below the move) it had when it was popped
        snap = [(n[1], n[3]) for _, n in popped]
        for j in range(len(ch)):
            k = ch[j].tobytes()
            par = popped[j // A][1]
            pdepth, pmove = snap[j // A]
            n = [k, pdepth + 1, par, j % A]
            f = closed.get(k)
            assert not (known(par[0], pdepth, pmove, j % A) and (f is None or f[1] > n[1])), (env, sem, len(trace), j)
            if f is None:
                closed[k] = n
            elif f[1] > n[1]:
                f[1], f[2], f[3] = n[1], n[2], n[3]
            else:
                continue
            v = np.float32(max(np.float32(hv[j]), np.float32(0.0)))
            cost = np.float32(v * np.float32(0.0 if k == goal else 1.0)) + np.float32(wf * np.float32(n[1]))
            heapq.heappush(heap, (float(np.float32(cost)), cnt, n))
            cnt += 1
        trace.append((len(heap), len(closed), gen))
    moves = None
    if is_solved and solved_node is not None:
        moves, n = [], solved_node[1]
        while n[1] > 0:
            moves.append(n[3])
            n = n[2]
        moves.reverse()
    return np.array(trace, np.int64).reshape(-1, 3), is_solved and solved_node is not None, moves


_REF = {}


def reference(L, co, env, root, w, B, sem, hid, iters):
    """The model's run (computed once per case), cross-checked against the C++ oracle wherever that is an exact reference."""
    case = (env, root.tobytes(), w, B, sem, hid, iters)
    if case not in _REF:
        trace, solved, moves = model_bwas(L, co, env, root, w, B, sem, hid, iters)
        if env != "puzzle8" and hid != MANHATTAN and (sem == PY or hid == HASHU01):
            orc = co.astar(env, root, w, B, sem, heur_builtin_id=hid, max_iters=iters, trace_cap=iters)
            assert np.array_equal(trace, orc["trace"]), ("model vs oracle", case[0], case[2:])
            assert bool(orc["solved"]) == solved and (not solved or len(orc["moves"]) == len(moves))
        _REF[case] = (trace, solved, moves)
    return _REF[case]


def engine_trace(L, eng, root, hid, iters, instance=None):
    eng.reset(root)
    if eng.semantics == L.SEM_PY:
        eng.root_commit(L.heuristic_builtin(hid, torch.from_numpy(root[None].copy()).cuda()))
    trace = []
    for _ in range(iters):
        eng.run_builtin(hid, 1)
        st = eng.status()
        trace.append((st["open_size"], st["closed_size"], st["nodes_generated"]))
        if st["done"]:
            break
    return np.array(trace, np.int64).reshape(-1, 3), eng._result()


def check_case(L, co, env, root, w, B, sem, hid, iters, max_nodes=1 << 15):
    from deepcubea_amd.search_methods.engine import BwasEngine
    want, solved, moves = reference(L, co, env, root, w, B, sem, hid, iters)
    eng = BwasEngine(env, w, B, max_nodes=max_nodes, semantics=L.SEM_PY if sem == PY else L.SEM_CPP)
    got, res = engine_trace(L, eng, root, hid, iters)
    eng.close()
    what = (env, root.tolist(), w, B, sem, hid)
    assert not res["failed"], what
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())  # exact in both semantics: the model's tie rule is the engine's
    assert res["solved"] == solved, what
    if solved:
        assert res["moves"] == moves, what
    return got


def walk(L, co, env, moves):
    s = goal_of(env)[None].copy()
    for a in moves:
        s = expand_host(L, co, env, s)[a][None].copy()
    return s[0]


# ------------------------------------------------------------------------------------------------ 1. depth boundary, cube3
@pytest.mark.parametrize("sem", [PY, CPP])
@pytest.mark.parametrize("scr", [[4], [4, 9], [4, 9, 2]])
def test_depth_boundary_cube3(L, co, scr, sem):
    """Roots 1, 2 and 3 moves from the goal; with B = 1 the pops pass through g_P = 0, 1, 2 in turn.  The depth-1 node's undo child
    is the root's state: kept in PY semantics (the root is not in CLOSED), dropped in cpp — the rule's threshold g_P >= 2."""
    root = walk(L, co, "cube3", scr)
    for B in (1, 2, 13):
        for w in (0.0, 0.8):
            for hid in (HASHU01, ZERO):
                got = check_case(L, co, "cube3", root, w, B, sem, hid, 12)
                if B == 1 and w == 0.0 and hid == ZERO and sem == PY and len(got) >= 2:
                    # uniform costs, FIFO: pop 1 is the root's first child, whose undo child (the root's state, g = 2) is NEW in PY
                    assert got[1, 1] - got[0, 1] == 12 and got[1, 0] - got[0, 0] == 11


# ------------------------------------------------------------------------------------------------ 2. illegal moves near the root
PUZZLE_ROOTS = {
    # the blank in a corner, on an edge and in the centre (walks from the goal, whose blank sits in the last corner)
    "puzzle8": {"corner": [1, 1, 3, 3, 0, 2, 0, 2, 1, 3, 3, 1], "edge": [1, 1, 3, 3, 0, 2, 0, 2, 1, 3, 3, 1, 2],
                "centre": [1, 1, 3, 3, 0, 2, 0, 2, 1, 3, 3, 1, 2, 0]},
    "puzzle15": {"corner": [3, 3, 1, 1, 2, 0, 3, 3, 1, 1], "edge": [3, 3, 1, 1, 2, 0, 3, 3, 1, 1, 2],
                 "centre": [3, 3, 1, 1, 2, 0, 3, 3, 1, 1, 2, 0]},
}


@pytest.mark.parametrize("sem", [PY, CPP])
@pytest.mark.parametrize("where", ["corner", "edge", "centre"])
@pytest.mark.parametrize("env", ["puzzle8", "puzzle15"])
def test_illegal_moves_at_and_near_the_root(L, co, env, where, sem):
    """PY keeps the root-equal child of the root at g = 1 (threshold g_P >= 1 of the no-op rule); cpp has the root in CLOSED."""
    n = puzzle_dim(env)
    root = walk(L, co, env, PUZZLE_ROOTS[env][where])
    z =int(np.flatnonzero(root == 0)[0])
    r, c = divmod(z, n)
    edges = (r in (0, n - 1)) + (c in (0, n - 1))
    assert edges == {"corner": 2, "edge": 1, "centre": 0}[where]
    for B in (1, 3):
        for hid in (MANHATTAN, HASHU01):
            got = check_case(L, co, env, root, 0.8, B, sem, hid, 15)
            if sem == PY:  # iteration 0 pops the root alone: its no-op children are new states there, all equal to each other
                assert got[0].tolist() == [4 - edges + (1 if edges else 0), 4 - edges + (1 if edges else 0), 4]


# ------------------------------------------------------------------------------------------------ 3. re-discovery at a smaller g
@pytest.mark.parametrize("sem", [PY, CPP])
@pytest.mark.parametrize("w", [0.0, 0.2])
def test_rediscovery_at_a_smaller_path_cost_puzzle8(L, co, w, sem):
    """A small state space at B = 50: shallower duplicates (PY: a new node; cpp: the representative rewritten in place, whose
    (g, parent, move) triple the rule then reads) occur within 40 iterations."""
    root = walk(L, co, "puzzle8", [1, 1, 3, 3, 0, 2, 0, 2, 1, 3, 0, 3, 1, 2, 2, 0, 3, 1])
    got = check_case(L, co, "puzzle8", root, w, 50, sem, HASHU01, 40, max_nodes=1 << 16)
    assert len(got) >= 10 and got[-1, 1] < got[-1, 2] // 2  # most children were duplicates
    # the same walk on puzzle15, where the C++ oracle holds the model to the reference's rewrites (`reference` compares them)
    check_case(L, co, "puzzle15", walk(L, co, "puzzle15", [1, 1, 3, 3, 0, 2, 0, 2, 1, 3, 0, 3, 1, 2, 2, 0, 3, 1]), w, 50, sem, HASHU01, 40,
               max_nodes=1 << 16)


# ------------------------------------------------------------------------------------------------ 4. LightsOut
@pytest.mark.parametrize("sem", [PY, CPP])
def test_lightsout_every_press_is_its_own_inverse(L, co, sem):
    root = walk(L, co, "lightsout7", [3, 17, 40, 22, 9])
    check_case(L, co, "lightsout7", root, 0.8, 2, sem, HASHU01, 6)
    check_case(L, co, "lightsout7", root, 0.2, 2, sem, ZERO, 4)


# ------------------------------------------------------------------------------------------------ 5. K = 2 instances
@pytest.mark.parametrize("env,scrs", [("cube3", ([4, 9], [7, 0, 11])), ("puzzle15", ([1, 3, 1], [3, 3, 1, 1, 2]))])
def test_two_instances_on_different_roots(L, co, env, scrs):
    from deepcubea_amd.search_methods.engine import BwasEngine
    w, B, hid, iters = 0.8, 3, HASHU01, 10
    roots = [walk(L, co, env, s) for s in scrs]
    for sem in (PY, CPP):
        refs = [reference(L, co, env, r, w, B, sem, hid, iters) for r in roots]
        eng = BwasEngine(env, w, B, max_nodes=1 << 15, semantics=L.SEM_PY if sem == PY else L.SEM_CPP, num_instances=2)
        for i, r in enumerate(roots):
            eng.reset(r, i)
            if sem == PY:
                eng.root_commit(L.heuristic_builtin(hid, torch.from_numpy(r[None].copy()).cuda()), i)
        for it in range(iters):
            eng.run_builtin(hid, 1)
            for i, (trace, _, _) in enumerate(refs):
                st = eng.status(i)
                k = min(it, len(trace) - 1)  # a finished instance freezes
                assert (st["open_size"], st["closed_size"], st["nodes_generated"]) == tuple(trace[k]), (env, sem, it, i)
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. dedup-first stepping
def test_packed_stepping_with_a_closure_evaluates_exactly_the_kept_children(L, co):
    """Dedup-first stepping hands the heuristic closure the children that survive the CLOSED check — a skipped child is never one
    of them, and nothing else changes: rows_evaluated is the oracle's count of pushes."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    env, w, B, hid = "puzzle15", 0.8, 50, 1
    root = walk(L, co, env, [1, 3, 1, 1, 3, 0, 2, 0, 3, 1])
    orc = co.astar(env, root, w, B, co.SEM_PY, heur_builtin_id=hid, trace_cap=100000)
    assert orc["solved"]
    pushes = int(orc["trace"][-1, 0]) - 1 + int(orc["trace"][-1, 2]) // 4  # |OPEN| = 1 + pushes - pops, pops = generated / A
    eng = BwasEngine(env, w, B, max_nodes=1 << 18, packed=True)

    def hfn(x, is_onehot=False):  # packed network-input rows of a puzzle are the raw tiles
        return L.heuristic_builtin(hid, x.contiguous())

    res = eng.solve(root, hfn)
    assert res["solved"] and res["moves"] == orc["moves"] and res["nodes_generated"] == orc["nodes_generated"]
    assert res["iterations"] == orc["iterations"]
    assert eng.rows_evaluated == pushes, (eng.rows_evaluated, pushes)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. the predicate itself
@pytest.mark.parametrize("env", ["cube3", "lightsout7", "puzzle8", "puzzle15", "puzzle24", "puzzle35", "puzzle48"])
def test_predicate_against_the_librarys_own_moves(L, env):
    """Every environment and dimension the engine instantiates, random states S, every (m, a): P = next_state(S, m),
    C = next_state(P, a).  Predicate true => C is S (undo) or C is P (no-op); no-op alone (g = 1) => C is P; and the rule is
    exactly the stated one: undo iff a inverts m from g >= 2, no-op iff the move is ineligible from g >= 1; never for the root."""
    e, d, D, A, _ = L.env_ids(env)
    n = 24
    S, _, _ = L.generate_states(e, d, n, 0, 40, 11)
    Sh = S.cpu().numpy()
    kd = L.engine_known_duplicate
    for m in range(A):
        P = L.next_state(e, d, S, m)
        Ph = P.cpu().numpy()
        m_moved = (Ph != Sh).any(1)
        zP = [int(np.flatnonzero(p == 0)[0]) if e == L.ENV_NPUZZLE else 0 for p in Ph]
        for a in range(A):
            Ch = L.next_state(e, d, P, a).cpu().numpy()
            back, stay = (Ch == Sh).all(1), (Ch == Ph).all(1)
            inv = a == (m if e == L.ENV_LIGHTSOUT else m ^ 1)
            for i in (range(n) if e == L.ENV_NPUZZLE else range(1)):
                if e != L.ENV_NPUZZLE:
                    assert not stay.any() and (back.all() if inv else not back.any())  # the rule does not look at the state
                assert kd(e, d, 0, 0xFF, a, zP[i]) is False and kd(e, d, 0, m, a, zP[i]) is False  # the root, whatever its fields
                assert kd(e, d, 1, m, a, zP[i]) == bool(stay[i])  # g = 1: the no-op rule alone (the undo child may be NEW in PY)
                assert kd(e, d, 7, 0xFF, a, zP[i]) == bool(stay[i])  # 0xFF inverts nothing
                if m_moved[i] or e != L.ENV_NPUZZLE:  # (a node with g >= 2 was never made by an ineligible move)
                    for g in (2, 3, 1 << 20):
                        k = kd(e, d, g, m, a, zP[i])
                        assert k == bool(inv or stay[i])
                        assert not k or back[i] or stay[i]
    with pytest.raises(L.DcaError):
        kd(e, d, 1, 0, A, 0)
    with pytest.raises(L.DcaError):
        kd(e, d, -1, 0, 0, 0)
    with pytest.raises(L.DcaError):
        kd(L.ENV_NPUZZLE, 8, 1, 0, 0, 0)
