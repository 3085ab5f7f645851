"""GPU: puzzle8 (the 8-puzzle) through every layer, held to GROUND TRUTH on all 181 440 reachable states where a layer allows it.

The yardsticks (tests/test_puzzle8_cpu.py pins them on the CPU): fixtures recorded from the reference
(tests/golden/puzzle8.npz), the numpy restatement of the move, and the breadth-first distance table rebuilt from the recorded
swap table.  The C++ oracle has no 3 x 3 tables, so nothing here asks it about moves; its hash and its float64 network
evaluation are generic and are used.  Byte / integer work is compared exactly; the floating-point bounds are stated where used."""
import ctypes as C
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from tests import test_puzzle8_cpu as p8

pytestmark = pytest.mark.gpu
GOAL = np.array([1, 2, 3, 4, 5, 6, 7, 8, 0], np.uint8)


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def fx():
    return p8.fixture()


@pytest.fixture(scope="module")
def table():
    """(all states [181440, 9] in breadth-first order, their distances) — computed once, never written to."""
    states, d, _ = p8.bfs_table()
    assert np.bincount(d, minlength=32).tolist() == p8.DEPTH_COUNTS
    return states, d.astype(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def replay(root, moves, swap):
    s = np.asarray(root, np.uint8)[None].copy()
    for a in moves:
        s = p8.move_np(s, int(a), swap)
    return s[0]


def lookup_heuristic():
    """A heuristic closure written in torch: permutation rank -> exact distance (0 for rows that are no reachable state)."""
    tab = torch.from_numpy(np.maximum(p8.bfs_table()[2], 0).astype(np.float32)).cuda()
    fact = [40320, 5040, 720, 120, 24, 6, 2, 1]

    def h(x, is_onehot=False):
        assert not is_onehot
        s = x.long()
        r = torch.zeros(s.shape[0], dtype=torch.long, device=s.device)
        for i in range(8):
            r += (s[:, i + 1:] < s[:, i:i + 1]).sum(1) * fact[i]
        return tab[r.clamp_(0, 362879)]
    return h


# ------------------------------------------------------------------------------------------------ 1. environment kernels
def test_env_kernels_vs_fixture_and_numpy_restatement(L, fx, table):
    from oracle import c_oracle as co
    from oracle import np_oracle as no
    e, d, D, A, depth = L.env_ids("puzzle8")
    assert (e, d, D, A, depth) == (L.ENV_NPUZZLE, 3, 9, 4, 9)
    assert np.array_equal(L.npuzzle_swap_table(3), fx["swap_zero_idxs"])
    swap, S = fx["swap_zero_idxs"], fx["states"]
    dS = dev(S)
    for a in range(4):
        got = L.next_state(e, d, dS, a)
        assert np.array_equal(got.cpu().numpy(), fx["next_state_all_actions"][a]), a
        back = L.next_state(e, d, got, a, prev=True).cpu().numpy()  # prev_state(a) = next_state(a ^ 1) (moves_rev)
        assert np.array_equal(back, p8.move_np(fx["next_state_all_actions"][a], a ^ 1, swap))
        moved = (fx["next_state_all_actions"][a] != S).any(1)
        assert moved.any() and np.array_equal(back[moved], S[moved])  # move o inverse = identity wherever the move is legal
    assert np.array_equal(L.expand_fused(e, d, dev(S[:8].copy()))["children"].cpu().numpy(), fx["expand_children_8"])
    allst, _ = table
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 64, 65, 1000, 4099):  # ragged sizes around the 64-parent tile; one row is shorter than a 16-byte chunk
        X = allst[rng.choice(len(allst), n, replace=False)].copy()
        if n > 2:
            X[0] = GOAL
            X[1] = p8.move_np(GOAL[None], 1, swap)[0]  # one move from the goal: a solved child exists
        ch = p8.expand_np(X, swap) if n else np.zeros((0, 4, 9), np.uint8)
        flat = ch.reshape(-1, 9)
        for off in ((0,) if n == 0 else (0, 3)):  # aligned, and every base pointer off the 16-byte grid
            buf = torch.zeros(n * 9 + 64, dtype=torch.uint8, device="cuda")
            view = buf[off:off + n * 9].view(n, 9)
            view.copy_(dev(X))
            obuf = torch.zeros(n * 36 + 64, dtype=torch.uint8, device="cuda")
            och = obuf[off:off + n * 36].view(n, 4, 9)
            ohb = torch.zeros(n * 4 * 81 + 16, dtype=torch.float32, device="cuda")
            oh = ohb[(1 if off else 0):(1 if off else 0) + n * 4 * 81].view(n * 4, 81)
            out = L.expand_fused(e, d, view, nnet_in=True, out={"children": och, "onehot": oh})
            torch.cuda.synchronize()
            assert np.array_equal(out["children"].cpu().numpy(), ch), (n, off)
            assert np.array_equal(out["solved"].cpu().numpy().astype(bool), (flat == GOAL).all(1))
            assert np.array_equal(u64(out["hash"]), co.hash64(flat)) and np.array_equal(co.hash64(flat), no.hash64(flat))
            assert np.array_equal(out["nnet_in"].cpu().numpy(), flat)
            assert np.array_equal(oh.cpu().numpy().view(np.uint32), no.onehot(flat, 9).astype(np.float32).view(np.uint32))
            assert int(obuf[:off].sum()) == 0 and int(obuf[off + n * 36:].sum()) == 0  # no stray writes
            assert float(ohb[:1 if off else 0].abs().sum()) == 0 and float(ohb[(1 if off else 0) + n * 324:].abs().sum()) == 0
            assert n <= 2 or int(out["solved"].sum()) >= 3  # the goal's two no-op moves and the one move back to it
        if n == 0:
            continue
        dX = dev(X)
        bf = L.expand_fused(e, d, dX, children=False, onehot_dtype=torch.bfloat16, solved=False, hashes=False)["onehot"]
        want = torch.from_numpy(no.onehot(flat, 9)).to(torch.bfloat16)
        assert torch.equal(bf.cpu().view(torch.int16), want.view(torch.int16))
        assert np.array_equal(L.is_solved(e, d, dX).cpu().numpy().astype(bool), (X == GOAL).all(1))
        assert np.array_equal(L.nnet_input(e, d, dX).cpu().numpy(), X)
        assert np.array_equal(u64(L.hash64(dX)), co.hash64(X))
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            assert np.array_equal(L.onehot(dX, 9, dt).float().cpu().numpy(), no.onehot(X, 9))


def test_environment_api_mirror(L, fx):
    from deepcubea_amd.environments.n_puzzle import NPuzzleState
    from deepcubea_amd.utils import env_utils
    env = env_utils.get_environment("puzzle8")
    states = [NPuzzleState(s.copy()) for s in fx["states"][:8]]
    for a in range(4):
        ns, tc = env.next_state(states, a)
        assert tc == [1.0] * 8 and all(np.array_equal(x.tiles, fx["next_state_all_actions"][a][i]) for i, x in enumerate(ns))
        ps = env.prev_state(ns, a)
        want = p8.move_np(fx["next_state_all_actions"][a][:8], a ^ 1, fx["swap_zero_idxs"])
        assert all(np.array_equal(p.tiles, w) for p, w in zip(ps, want))
    exp, tcs = env.expand(states)
    assert len(exp) == 8 and len(exp[0]) == 4 and all(np.all(t == 1.0) and t.shape == (4,) for t in tcs)
    assert np.array_equal(np.stack([np.stack([c.tiles for c in row]) for row in exp]), fx["expand_children_8"])
    probe = [NPuzzleState(s.copy()) for s in fx["is_solved_probe_states"]]
    assert np.array_equal(env.is_solved(probe), fx["is_solved_probe"])
    assert np.array_equal(env.state_to_nnet_input(states)[0], fx["states"][:8])
    st, nb = env.generate_states(200, (0, 30), seed=4)
    arr = np.stack([s.tiles for s in st])
    assert len(st) == 200 and min(nb) >= 0 and max(nb) <= 30 and (np.sort(arr, 1) == np.arange(9)).all()
    dd = p8.distance(arr)
    assert (dd >= 0).all() and (dd <= np.array(nb)).all() and all(np.array_equal(a, GOAL) for a, k in zip(arr, nb) if k == 0)


# ------------------------------------------------------------------------------------------------ 2. all 181 440 states
def test_all_states_solved_flag_manhattan_and_bellman_backup_return_the_table(L, fx, table):
    e, d, D, A, depth = L.env_ids("puzzle8")
    X, dist = table
    dX = dev(X)
    sv = L.is_solved(e, d, dX)
    assert int(sv.sum()) == 1 and int(sv[0]) == 1  # exactly one: the goal, first in breadth-first order
    mh = L.heuristic_builtin(L.HEUR_MANHATTAN, dX).cpu().numpy()
    assert np.array_equal(mh, p8.manhattan_np(X).astype(np.float32))
    assert (mh <= dist).all() and ((mh == 0) == (dist == 0)).all()  # admissible everywhere; 0 only at the goal
    out = L.expand_fused(e, d, dX, hashes=False)
    ch = out["children"].cpu().numpy()
    assert np.array_equal(ch, p8.expand_np(X, fx["swap_zero_idxs"]))
    dch = p8.distance(ch.reshape(-1, 9)).reshape(-1, 4)
    assert (dch >= 0).all()
    assert np.array_equal(out["solved"].cpu().numpy().reshape(-1, 4).astype(bool), dch == 0)
    ctg, am = L.bellman_backup(dev(dch.astype(np.float32)).view(-1), sv, 4)
    assert np.array_equal(ctg.cpu().numpy(), dist.astype(np.float32)) and float(ctg[0]) == 0.0  # the table itself
    am = am.cpu().numpy()
    step = dch[np.arange(len(X)), am]
    assert np.array_equal(step[1:], dist[1:] - 1)  # the argmin child is one step closer for every non-goal state
    assert np.array_equal(am, np.argmin(dch, 1))   # first index on ties (gbfs.py:108)


# ------------------------------------------------------------------------------------------------ 3. scrambler
def test_scrambler_reproducible_disjoint_replayable_and_inside_the_table(L, fx):
    e, d, D, A, depth = L.env_ids("puzzle8")
    n, hi = 20000, 40
    parts = []
    for index0 in (0, n):
        st, nb, mv = L.generate_states(e, d, n, 0, hi, 77, index0=index0, want_moves=True)
        st2, nb2, _ = L.generate_states(e, d, n, 0, hi, 77, index0=index0)
        assert torch.equal(st, st2) and torch.equal(nb, nb2)  # reproducible
        parts.append((st.cpu().numpy(), nb.cpu().numpy(), mv.cpu().numpy()))
    both, nbb, _ = L.generate_states(e, d, 2 * n, 0, hi, 77, index0=0)
    assert np.array_equal(both.cpu().numpy(), np.concatenate([parts[0][0], parts[1][0]]))  # a state is a function of its index
    assert np.array_equal(nbb.cpu().numpy(), np.concatenate([parts[0][1], parts[1][1]]))
    assert not np.array_equal(parts[0][0], parts[1][0])
    for st, nb, mv in parts:
        assert nb.min() == 0 and nb.max() == hi and ((mv >= 0).sum(1) == nb).all() and (mv[mv >= 0] < 4).all()
        cur = np.tile(GOAL, (n, 1))  # the recorded walk, replayed from the goal (a reverse move a = next_state(a ^ 1))
        for t in range(hi):
            for a in range(4):
                sel = mv[:, t] == a
                if sel.any():
                    cur[sel] = p8.move_np(cur[sel], a ^ 1, fx["swap_zero_idxs"])
        assert np.array_equal(cur, st)
        dd = p8.distance(st)
        assert (dd >= 0).all() and (dd <= nb).all()  # every state is in the table, no farther than its walk is long


# ------------------------------------------------------------------------------------------------ 4. engine, python semantics
def test_engine_python_semantics_reproduces_reference_astar_traces(L, fx):
    from deepcubea_amd.search_methods.engine import BwasEngine
    from tests.test_engine_hip import run_traced
    for key in [str(k) for k in fx["astar_py_cases"]]:
        w, B, hid = fx[key + "_cfg"]
        pc, nn = fx[key + "_result"]
        eng = BwasEngine("puzzle8", float(w), int(B), max_nodes=max(1 << 16, int(nn) + 4 * int(B) * 4 + 64))
        res = run_traced(L, eng, fx[key + "_root"], int(hid))
        assert res["solved"] and res["moves"] == fx[key + "_moves"].tolist(), key
        assert res["path_cost"] == pc and res["nodes_generated"] == int(nn), key
        assert res["iterations"] == len(fx[key + "_trace"]) and np.array_equal(res["trace"], fx[key + "_trace"]), key
        r2 = eng.solve_builtin(fx[key + "_root"], int(hid), chunk=9, use_graph=True)
        assert r2["moves"] == fx[key + "_moves"].tolist() and r2["nodes_generated"] == int(nn), key
        assert r2["iterations"] == len(fx[key + "_trace"]), key
        eng.close()


def test_four_instances_equal_four_single_runs(L, fx):
    from deepcubea_amd.search_methods.engine import BwasEngine
    keys = [str(k) for k in fx["astar_py_cases"]][:4]
    roots = [fx[k + "_root"] for k in keys]
    w, B, hid = 0.6, 7, 1
    one = BwasEngine("puzzle8", w, B, max_nodes=1 << 19)
    singles = [one.solve_builtin(r, hid, chunk=9, use_graph=True) for r in roots]
    one.close()
    many = BwasEngine("puzzle8", w, B, max_nodes=1 << 19, num_instances=4)
    multi = many.solve_many_builtin(roots, hid, chunk=9, use_graph=True)
    many.close()
    for root, a, b in zip(roots, singles, multi):
        assert a["solved"] and b["solved"] and a["moves"] == b["moves"]
        assert a["nodes_generated"] == b["nodes_generated"] and a["iterations"] == b["iterations"]
        assert np.array_equal(replay(root, b["moves"], fx["swap_zero_idxs"]), GOAL)


# ------------------------------------------------------------------------------------------------ 5. engine, optimality
def _depth_cases(table, depths):
    X, dist = table
    rng = np.random.default_rng(31)
    cases = []
    for k in depths:
        idx = np.flatnonzero(dist == k)
        for i in (idx if len(idx) <= 2 else rng.choice(idx, 2, replace=False)):
            cases.append((X[i].copy(), k))
    return cases


def test_engine_finds_optimal_solutions_at_every_depth(L, fx, table):
    """SEM_CPP, weight 1, Manhattan distance (admissible, consistent): the solution length is the exact distance.  Two states
    of every depth 0..31 at B = 1000 (both depth-31 states), the same states of depths 0..12 at B = 1; one engine each."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    cases = _depth_cases(table, range(32))
    assert sum(1 for _, k in cases if k == 31) == 2 and len(cases) == 63  # (depth 0 has one state)
    for B, sel in ((1000, cases), (1, [c for c in cases if c[1] <= 12])):
        eng = BwasEngine("puzzle8", 1.0, B, max_nodes=1 << 21, semantics=L.SEM_CPP)
        for root, k in sel:
            res = eng.solve_builtin(root, L.HEUR_MANHATTAN, max_iters=1 << 20, chunk=64, use_graph=True)
            assert res["solved"], (B, k, res)
            assert len(res["moves"]) == k and res["path_cost"] == float(k), (B, k, root.tolist(), len(res["moves"]))
            assert np.array_equal(replay(root, res["moves"], fx["swap_zero_idxs"]), GOAL)
        eng.close()
    with pytest.raises(L.DcaError):
        BwasEngine("puzzle8", 1.0, 1000, max_nodes=100)  # max_nodes < one batch of children
    e2 = BwasEngine("puzzle8", 1.0, 4, max_nodes=1 << 12)
    with pytest.raises(L.DcaError):  # a root byte >= 9 is refused (root[i] < D with D = 9)
        e2.reset(np.array([1, 2, 3, 4, 5, 6, 7, 9, 0], np.uint8))
    e2.reset(np.array([1, 2, 3, 4, 5, 6, 7, 0, 8], np.uint8))
    e2.close()


# ------------------------------------------------------------------------------------------------ 6. layer 1
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_l1_embed_bit_for_bit_every_output_form(L, m):
    from tests.test_embed_hip import _case, _host_sum
    assert L.l1_embed_supported(9, 9)
    n_pad = 192
    w, b, x = _case(9, 9, m, n_pad, 9000 + m)
    wt, bc, xc = w.t().contiguous().cuda(), b.cuda(), x.cuda()
    for relu in (True, False):
        want = _host_sum(w, b, x, 9, relu)
        got = L.l1_embed(xc, 9, wt, bc, relu).cpu().numpy()
        assert got.shape == (m, n_pad) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (m, relu)
    want = torch.from_numpy(_host_sum(w, b, x, 9, True))
    got16 = L.l1_embed(xc, 9, wt, bc, True, torch.bfloat16).cpu()
    assert torch.equal(got16.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    big = 150.0
    want8 = torch.from_numpy(_host_sum(w * big, b * big, x, 9, True)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    got8 = L.l1_embed(xc, 9, (w * big).t().contiguous().cuda(), (b * big).cuda(), True, torch.float8_e4m3fn).cpu()
    assert float(want8.float().max()) == 448.0  # (the saturating branch is exercised)
    assert torch.equal(got8.view(torch.uint8), want8.view(torch.uint8))
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    pl = L.l1_embed(xc, 9, wt, bc, True, split="planes", overflow=ovf).cpu()
    hi = want.to(torch.float16)
    assert pl.shape == (2, m, n_pad) and int(ovf.item()) == 0
    assert torch.equal(pl[0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(pl[1].view(torch.int16), (want - hi.float()).to(torch.float16).view(torch.int16))
    b2 = b.clone()
    b2[77] = 70000.0  # beyond fp16: the planes' overflow flag
    L.l1_embed(xc, 9, wt, b2.cuda(), True, split="planes", overflow=ovf)
    assert int(ovf.item()) == 1


def test_l1_embed_same_row_same_bits_anywhere_and_refusals(L):
    from tests.test_embed_hip import _case, _host_sum
    w, b, x = _case(9, 9, 1000, 128, 5)
    wt, bc, xc = w.t().contiguous().cuda(), b.cuda(), x.cuda()
    whole = L.l1_embed(xc, 9, wt, bc, True)
    assert torch.equal(L.l1_embed(xc[100:333].contiguous(), 9, wt, bc, True), whole[100:333])
    assert xc[3:].data_ptr() % 16 != 0 and torch.equal(L.l1_embed(xc[3:], 9, wt, bc, True), whole[3:])  # rows off the 16-byte grid
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(L.l1_embed(xc[perm].contiguous(), 9, wt, bc, True), whole[perm])
    wide = _case(9, 9, 700, 5120, 6)  # the network's real width: 80 column tiles
    got = L.l1_embed(wide[2].cuda(), 9, wide[0].t().contiguous().cuda(), wide[1].cuda(), True).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), _host_sum(wide[0], wide[1], wide[2], 9, True).view(np.uint32))
    assert not L.l1_embed_supported(9, 6) and not L.l1_embed_supported(9, 10) and not L.l1_embed_supported(4, 4)
    with pytest.raises(L.DcaError):  # a state matrix of another width
        L.l1_embed(torch.zeros(8, 10, dtype=torch.uint8).cuda(), 9, torch.zeros(90, 64).cuda(), b[:64].cuda(), True)
    with pytest.raises(L.DcaError):  # n_pad not a multiple of the column tile
        L.l1_embed(xc[:8].contiguous(), 9, torch.zeros(81, 32).cuda(), b[:32].cuda(), True)
    assert L.l1_embed(xc[:0], 9, wt, bc, True).shape == (0, 128)


def _wgrad_host(s, dy, S):
    """include/dca.h's order at (9, 9), with the byte guard: a position whose byte is >= 9 selects no row; db counts every row."""
    m, n = s.shape[0], dy.shape[1]
    base = np.arange(9) * 9
    tot_w, tot_b = np.zeros((81, n), np.float32), np.zeros(n, np.float32)
    for a in range(0, m, S):
        pw, pb = np.zeros((81, n), np.float32), np.zeros(n, np.float32)
        for r in range(a, min(a + S, m)):
            ok = s[r] < 9
            pw[(base + s[r])[ok]] += dy[r]
            pb += dy[r]
        tot_w += pw
        tot_b += pb
    return np.ascontiguousarray(tot_w.T), tot_b


@pytest.mark.parametrize("m_label", ["1", "S-1", "S", "S+1", "2*S+3"])
def test_l1_embed_wgrad_bit_for_bit_against_the_host_loop(L, m_label):
    from tests.test_l1_train_hip import SENTINEL, _case, _check_bits, _host_model, _launch, _same
    S = L.l1_embed_wgrad_slice_rows(9, 9)
    assert 0 < S <= 2048
    m = int(eval(m_label, {"S": S}))
    for n in (64, 128):
        s, dy = _case(m, n, 9, 9, seed=m * 1000 + n)
        _check_bits(s, dy, 9, strided=True)   # ld_dy = n + 4, ldw = K + 3, db present; the rows' slack keeps its sentinel
        _check_bits(s, dy, 9, strided=False)
        rc, dw, db = _launch(s, dy, 9, want_db=False)  # db absent
        want_w, _ = _host_model(s, dy, 9, S)
        assert rc == 0 and db is None and _same(dw, torch.from_numpy(want_w).cuda())
    assert SENTINEL != 0


def test_l1_embed_wgrad_bad_bytes_unaligned_states_and_refusals(L):
    from tests.test_l1_train_hip import SENTINEL, _case, _launch, _p, _same
    lib = L.lib()
    S = L.l1_embed_wgrad_slice_rows(9, 9)
    s, dy = _case(S + 70, 64, 9, 9, seed=12)
    bad = np.random.default_rng(1).random(s.shape) < 0.2
    s[bad] = np.random.default_rng(2).integers(9, 256, size=int(bad.sum()), dtype=np.uint8)  # bytes >= 9 contribute nothing
    rc, dw, db = _launch(s, dy, 9)
    want_w, want_b = _wgrad_host(s, dy, S)
    assert rc == 0 and _same(dw, torch.from_numpy(want_w).cuda()) and _same(db, torch.from_numpy(want_b).cuda())
    # a state matrix off the 16-byte grid (read byte by byte), and m == 0 (zeros)
    s2, dy2 = _case(200, 36, 9, 9, seed=11)
    buf = torch.zeros(200 * 9 + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(s2).cuda().flatten()
    s_dev = buf[1:].view(200, 9)
    dw2 = torch.full((36, 81), SENTINEL, dtype=torch.float32, device="cuda")
    db2 = torch.full((36,), SENTINEL, dtype=torch.float32, device="cuda")
    dy_dev = torch.from_numpy(dy2).cuda()
    assert s_dev.data_ptr() % 2 == 1
    assert lib.dca_l1_embed_wgrad(_p(s_dev), C.c_int64(200), 9, 9, _p(dy_dev), C.c_int64(36), C.c_int64(36), _p(dw2), C.c_int64(81),
                                  _p(db2), _p(None), C.c_int64(0), L.stream_ptr()) == 0
    w2, b2 = _wgrad_host(s2, dy2, S)
    assert _same(dw2, torch.from_numpy(w2).cuda()) and _same(db2, torch.from_numpy(b2).cuda())
    rc, dw0, db0 = _launch(s2[:0], dy2[:0], 9, ldw=84)
    assert rc == 0 and bool((dw0[:, :81].view(torch.int32) == 0).all()) and bool((dw0[:, 81:] == SENTINEL).all())
    # every refusal of the other geometries' test, at (9, 9)
    K, m, n = 81, S + 1, 8
    st = torch.zeros((m, 9), dtype=torch.uint8, device="cuda")
    dyb = torch.ones((m, n + 8), dtype=torch.float32, device="cuda")
    dwb = torch.full((n, K + 4), SENTINEL, dtype=torch.float32, device="cuda")
    dbb = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    need = int(lib.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(m), 9, 9, C.c_int64(n)))
    assert need == 2 * (n * K + n) * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    good = dict(s=_p(st), m=m, d=9, depth=9, dy=_p(dyb), ld_dy=n + 8, n=n, dw=_p(dwb), ldw=K + 4, db=_p(dbb), ws=_p(ws), wsb=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dca_l1_embed_wgrad(a["s"], C.c_int64(a["m"]), a["d"], a["depth"], a["dy"], C.c_int64(a["ld_dy"]), C.c_int64(a["n"]),
                                      a["dw"], C.c_int64(a["ldw"]), a["db"], a["ws"], C.c_int64(a["wsb"]), L.stream_ptr())

    refused = {"unsupported geometry": dict(d=9, depth=6), "n % 4 != 0": dict(n=6), "m < 0": dict(m=-1), "null states": dict(s=_p(None)),
               "null dy": dict(dy=_p(None)), "null dW": dict(dw=_p(None)), "misaligned dy": dict(dy=C.c_void_p(dyb.data_ptr() + 4)),
               "ld_dy % 4 != 0": dict(ld_dy=n + 2), "ldw < K": dict(ldw=K - 1), "ld_dy < n": dict(ld_dy=n - 4),
               "workspace too small": dict(wsb=need - 1), "workspace missing": dict(ws=_p(None))}
    for what, kw in refused.items():
        assert call(**kw) == -1, what
        assert len(lib.dca_last_error()) > 0, what
    torch.cuda.synchronize()
    assert bool((dwb == SENTINEL).all()) and bool((dbb == SENTINEL).all()), "a refused call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dwb[:, :K] != SENTINEL).all()) and bool((dwb[:, K:] == SENTINEL).all())


@pytest.mark.parametrize("m", [1, 257, 1500])
def test_l1_mfma_kernels_against_float64_on_the_exact_operands(L, m):
    """The matrix-pipe layer-1 kernels at (9, 9) (K = 81: k_pad 96 for the bf16 planes, 128 for e4m3), by the criteria of
    tests/test_mlp_hip.py and tests/test_gemm8_hip.py for their geometries, at ragged row counts."""
    from tests.test_gemm8_hip import _q, test_layer1_fp8_pipe_kernel_against_float64
    from tests.test_mlp_hip import test_l1_onehot_gemm_matches_float64
    from deepcubea_amd.utils.pytorch_models import l1_weight_tiles
    assert L.l1_supported(9, 9) and L.l1_kpad(9, 9) == 96 and L.l1_supported8(9, 9) and L.l1_kpad8(9, 9) == 128
    for planes, dt, tol in ((3, torch.float32, 2e-6), (2, torch.float16, 2e-3), (1, torch.bfloat16, 1.5e-2), (3, torch.bfloat16, 1e-2),
                            (1, torch.float32, 1e-2)):
        test_l1_onehot_gemm_matches_float64(9, 9, planes, dt, tol, m)
    test_layer1_fp8_pipe_kernel_against_float64(9, 9, 128, max(m, 64) + 1)
    # e4m3 and block-scaled e4m3 outputs of the bf16-plane kernel: the fp32 accumulator, rounded (per tensor / per 64 columns)
    g = torch.Generator().manual_seed(11 + m)
    n_pad = 192
    w1 = (torch.randn(n_pad, 81, generator=g) * 60.0).to(torch.bfloat16).float()
    b1 = torch.randn(n_pad, generator=g) * 100.0
    tiles = l1_weight_tiles(w1, 1, 96).cuda()
    x = torch.randint(0, 9, (m, 9), dtype=torch.uint8, generator=g).cuda()
    y32 = L.l1_onehot_gemm(x, 9, tiles, 1, b1.cuda(), True, torch.float32)
    y8 = L.l1_onehot_gemm(x, 9, tiles, 1, b1.cuda(), True, L.E4M3)
    assert float(y32.max()) > 448.0 or m == 1
    assert torch.equal(y8.cpu().view(torch.uint8), _q(y32.cpu()).view(torch.uint8))
    y8x, ysc = L.l1_onehot_gemm_mx(x, 9, tiles, b1.cuda(), True)
    y64 = y32.double().cpu()
    e = ysc.cpu().to(torch.float64) - 127.0
    am = y64.abs().view(m, n_pad // 64, 64).amax(dim=2)
    assert torch.equal(e, torch.ceil(torch.log2((am / 448.0).clamp_min(2.0 ** -126))).clamp(-126, 126))
    f = torch.pow(torch.tensor(2.0, dtype=torch.float64), e).repeat_interleave(64, dim=1)
    assert torch.equal(y8x.cpu().view(torch.uint8), _q((y64 / f).float()).view(torch.uint8))


# ------------------------------------------------------------------------------------------------ 7. network
def _recorded_net(fx):
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    net = ResnetModel(9, 9, 128, 64, 1, 1, True)
    net.load_state_dict({str(k): torch.tensor(fx["net_" + str(k)]) for k in fx["net_keys"]})
    return net


@torch.no_grad()
def test_recorded_network_within_1e5_of_the_reference_and_batch_independent(L, fx):
    """|h| <= 1 on this fixture: the project's bound there is 1e-5 ABSOLUTE against the reference's recorded fp32 outputs."""
    from deepcubea_amd.utils.pytorch_models import FastResnet, Fp64Resnet, L1_EMBED_MIN_DEPTH
    net = _recorded_net(fx).eval()
    x = dev(fx["net_x"])
    y32, y64 = fx["net_y32"], fx["net_y64"]
    assert np.abs(y32).max() <= 1.0
    assert np.abs(net.cuda()(x)[:, 0].cpu().numpy() - y32).max() < 1e-5  # the module itself
    fast = FastResnet(net).cuda()
    assert fast.uses_l1_kernel and (fast.l1_embed_w is None) == (9 < L1_EMBED_MIN_DEPTH[torch.float32]) and fast.l1_tiles is not None
    yf = fast(x)[:, 0]
    assert fast.split_fallbacks == 0 and np.abs(yf.cpu().numpy() - y32).max() < 1e-5
    emb = FastResnet(net, l1="embed").cuda()
    ye = emb(x)[:, 0]
    assert emb.l1_embed_w is not None and np.abs(ye.cpu().numpy() - y32).max() < 1e-5
    f64 = Fp64Resnet(net).cuda()
    y6 = f64(x)[:, 0]
    assert np.abs(y6.double().cpu().numpy() - y32).max() < 1e-5
    assert np.abs(f64.forward64(x)[:, 0].cpu().numpy() - y64).max() < 1e-9  # float64 against float64
    for model, whole in ((fast, yf), (emb, ye), (f64, y6)):  # a row's value has the same bits in any batch
        assert torch.equal(model(x[10:37].contiguous())[:, 0], whole[10:37])
        assert torch.equal(model(x[63:].contiguous())[:, 0], whole[63:])


def test_one_training_step_embed_and_gemm_against_float64(L, fx):
    """One forward + backward of the recorded network in "embed" and in "gemm" mode: loss and every gradient as close to
    float64 as torch's own fp32 step is — the rule of tests/test_l1_train_hip.py's whole-step comparison (factor 4; floors
    2^-22 of the loss and 2e-7 of a tensor's largest element; analytically-zero gradients within 4x torch32's)."""
    from tests.test_l1_train_hip import NOISE, _plain_trunk, _rel
    e, d = L.env_ids("puzzle8")[:2]
    states, nb, _ = L.generate_states(e, d, 515, 0, 30, 5, 0)
    x = L.nnet_input(e, d, states)
    y = nb.float().contiguous()

    def step(mode):
        net = _recorded_net(fx).cuda().train()
        onehot = torch.nn.functional.one_hot(x.long(), 9).view(x.shape[0], -1)
        if mode == "float64":
            net = net.double()
            out = net.trunk(onehot.double())[:, 0]
            loss = torch.nn.functional.mse_loss(out, y.double())
        elif mode == "torch32":
            loss = torch.nn.functional.mse_loss(_plain_trunk(net, onehot.float())[:, 0], y)
        else:
            net.set_l1_train(mode)
            loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
        loss.backward()
        return float(loss.detach().double()), {k: p.grad.double().cpu() for k, p in net.named_parameters()}

    l64, g64 = step("float64")
    l32, g32 = step("torch32")
    failures = []
    for mode in ("embed", "gemm"):
        lo, go = step(mode)
        bound = max(4.0 * abs(l32 - l64), 2.0 ** -22 * abs(l64))
        print("PUZZLE8 STEP %s: loss err %.3g (bound %.3g)" % (mode, abs(lo - l64), bound))
        if not abs(lo - l64) <= bound:
            failures.append((mode, "loss", abs(lo - l64), bound))
        for k in g64:
            if NOISE.fullmatch(k):
                if not float(go[k].abs().max()) <= 4.0 * float(g32[k].abs().max()):
                    failures.append((mode, "zero-gradient " + k, float(go[k].abs().max()), float(g32[k].abs().max())))
                continue
            e_o, e_t = _rel(go[k], g64[k]), _rel(g32[k], g64[k])
            if not e_o <= max(4.0 * e_t, 2e-7):
                failures.append((mode, "grad " + k, e_o, e_t))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 8. network in the loop
@torch.no_grad()
def test_full_size_network_in_the_loop_both_orders_and_three_instances(L, fx, table):
    from deepcubea_amd.search_methods.engine import BwasEngine
    from deepcubea_amd.utils import env_utils, nnet_utils
    from deepcubea_amd.utils.pytorch_models import FastResnet
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    net = env_utils.get_environment("puzzle8").get_nnet_model()
    load_synthetic_weights(net, 2033)
    fast = FastResnet(net.cuda().eval()).cuda()
    assert fast.uses_l1_kernel
    hfn = nnet_utils.get_heuristic_fn_dev(fast, clip_zero=False, batch_size=1 << 17)
    X, dist = table
    roots = [X[np.flatnonzero(dist == k)[7]].copy() for k in (8, 10, 12)]
    B, w = 200, 0.8

    def traced(eng, root):
        eng.reset(root)
        eng.root_commit(hfn(eng.root_nnet_in()).to(torch.float32))
        tr = []
        for _ in range(2000):
            eng.step(hfn)
            st = eng.status()
            tr.append((st["open_size"], st["closed_size"], st["nodes_generated"]))
            if st["done"]:
                break
        return eng._result(), tr

    dedup = BwasEngine("puzzle8", w, B, max_nodes=1 << 20, packed=True)       # the CLI's default: dedup-first stepping
    every = BwasEngine("puzzle8", w, B, max_nodes=1 << 20)                    # --eval_all_children: the reference's order
    singles = []
    for root in roots:
        ra, ta = traced(dedup, root)
        rb, tb = traced(every, root)
        assert ra["solved"] and rb["solved"] and ta == tb and ra["moves"] == rb["moves"]
        assert np.array_equal(replay(root, ra["moves"], fx["swap_zero_idxs"]), GOAL)
        assert len(ra["moves"]) >= int(p8.distance(root[None])[0])
        singles.append(ra)
    assert dedup.rows_evaluated < every.rows_evaluated
    dedup.close()
    every.close()
    three = BwasEngine("puzzle8", w, B, max_nodes=1 << 20, packed=True, num_instances=3)
    multi = three.solve_many(roots, hfn)
    three.close()
    for a, b in zip(singles, multi):
        assert b["solved"] and a["moves"] == b["moves"] and a["nodes_generated"] == b["nodes_generated"]
        assert a["iterations"] == b["iterations"]
    # the reduced-precision modes have their layer-1 kernels at (9, 9) too (non-parity: finite values, loosely near fp32)
    from deepcubea_amd.utils.pytorch_models import Fp8Resnet
    xs = dev(X[:4096])
    ref = fast(xs)[:, 0]
    scale = max(1.0, float(ref.abs().max()))
    b16 = FastResnet(net, torch.bfloat16).cuda()
    assert b16.l1_tiles is not None and float((b16(xs)[:, 0] - ref).abs().max()) < 0.05 * scale
    for scaling in ("tensor", "block"):
        m8 = Fp8Resnet(net, scaling=scaling).cuda()
        assert m8.l1_fp8 == (scaling == "tensor")
        y8 = m8(xs)[:, 0]
        assert bool(torch.isfinite(y8).all()) and float((y8 - ref).abs().max()) < 0.5 * scale


# ------------------------------------------------------------------------------------------------ 9. update step
@torch.no_grad()
def test_update_step_targets_are_the_exact_distances(L, fx):
    from deepcubea_amd.updaters.updater import Updater, gbfs_test_dev
    from deepcubea_amd.utils import env_utils
    env = env_utils.get_environment("puzzle8")
    h = lookup_heuristic()
    allst = dev(p8.all_states()[::37])
    assert np.array_equal(h(allst).cpu().numpy(), p8.distance(allst.cpu().numpy()).astype(np.float32))  # the closure itself
    for method, n, steps, bs in (("GBFS", 3000, 1, 1024), ("ASTAR", 300, 4, 128)):
        upd = Updater(env, n, 30, h, steps, method, update_batch_size=bs, seed=3, cache="off")
        sn, ctg, sv = upd.update_dev()
        assert sn.shape[1] == 9 and ctg.shape == (sn.shape[0], 1) and sv.shape == (n,) and sn.shape[0] >= n
        assert np.array_equal(ctg[:, 0].cpu().numpy(), p8.distance(sn.cpu().numpy()).astype(np.float32)), method
    # the greedy walk on the exact distances solves every state in exactly d steps (32 > the eccentricity 31)
    rows = gbfs_test_dev(600, 30, env, h, max_solve_steps=32, seed=2)
    back_steps = list(np.linspace(0, 30, 30, dtype=int))
    index0, want = 0, {}
    for bs_ in back_steps:
        st, _, _ = L.generate_states(env._env_id, env._dim, 20, int(bs_), int(bs_), 2, index0)
        want.setdefault(int(bs_), []).append(p8.distance(st.cpu().numpy()))
        index0 += 20
    assert len(rows) == len(want)
    for back, per_solved, avg_steps, ctg_mean in rows:
        dd = np.concatenate(want[back])
        assert per_solved == 100.0 and abs(avg_steps - float(dd.mean())) < 1e-9 and abs(ctg_mean - float(dd.mean())) < 1e-5, back
    # the heuristic cache: the targets keep their bits and the counters add up
    off = Updater(env, 3000, 30, h, 2, "GBFS", update_batch_size=1024, seed=3, cache="off").update_dev()
    on_u = Updater(env, 3000, 30, h, 2, "GBFS", update_batch_size=1024, seed=3, cache="auto")
    on = on_u.update_dev()
    assert all(torch.equal(a, b) for a, b in zip(off, on))
    c = on_u.cache_counters()
    assert c["rows"] > 0 and c["rows"] == c["hits"] + c["dups"] + c["evaluated"] and c["hits"] + c["dups"] > 0


# ------------------------------------------------------------------------------------------------ 10. CLIs
def _states_pickle(path, arrays):
    from deepcubea_amd.environments.n_puzzle import NPuzzleState
    from deepcubea_amd.utils import data_utils
    data_utils.dump_pickle({"states": [NPuzzleState(a.copy()) for a in arrays]}, path)
    assert b"environments.n_puzzle" in open(path, "rb").read()


def test_astar_cli_manhattan_is_optimal_and_network_mode_is_valid(tmp_path, L, fx, table):
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils
    X, dist = table
    rng = np.random.default_rng(12)
    depths = [0, 3, 6, 9, 12, 15, 18, 20, 22, 24, 27, 31]
    roots = [X[rng.choice(np.flatnonzero(dist == k))].copy() for k in depths]
    spath = str(tmp_path / "states.pkl")
    _states_pickle(spath, roots)
    rdir = str(tmp_path / "opt")
    try:
        astar.main(["--states", spath, "--model_dir", "builtin:manhattan", "--env", "puzzle8", "--weight", "1", "--semantics", "cpp",
                    "--batch_size", "1000", "--results_dir", rdir, "--max_nodes", str(1 << 21)])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert [len(s) for s in res["solutions"]] == depths  # every length equals d
    for root, soln in zip(roots, res["solutions"]):
        assert np.array_equal(replay(root, soln, fx["swap_zero_idxs"]), GOAL)
    rdir = str(tmp_path / "net")
    try:
        astar.main(["--states", spath, "--model_dir", "synthetic:11", "--env", "puzzle8", "--weight", "0.8", "--batch_size", "100",
                    "--results_dir", rdir, "--nnet_batch_size", "1024", "--max_nodes", str(1 << 20)])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert sorted(res.keys()) == ["num_nodes_generated", "paths", "solutions", "states", "times"]  # astar.py:382-397
    log = open(os.path.join(rdir, "output.txt")).read()
    assert len(re.findall(r"State: (\d+), SolnCost: ([\d.]+), # Moves: (\d+), # Nodes Gen: ([\d,]+), Time: ([\d.]+)", log)) == 12
    for root, soln, path, k in zip(roots, res["solutions"], res["paths"], depths):
        assert np.array_equal(replay(root, soln, fx["swap_zero_idxs"]), GOAL) and len(path) == len(soln) + 1 and len(soln) >= k


def test_avi_loop_end_to_end_with_l1_train_embed(tmp_path):
    from deepcubea_amd.ctg_approx import avi
    save = str(tmp_path / "saved_models")
    argv = ["--env", "puzzle8", "--states_per_update", "3000", "--batch_size", "1000", "--nnet_name", "t", "--max_itrs", "6",
            "--loss_thresh", "1e9", "--back_max", "20", "--num_test", "60", "--save_dir", save, "--update_nnet_batch_size",
            "2000", "--max_update_steps", "2", "--l1_train", "embed"]
    try:
        avi.main(argv)
    finally:
        sys.stdout = sys.__stdout__
    cur, targ = os.path.join(save, "t", "current"), os.path.join(save, "t", "target")
    assert pickle.load(open(os.path.join(cur, "train_itr.pkl"), "rb")) == 6
    assert pickle.load(open(os.path.join(cur, "update_num.pkl"), "rb")) == 2
    for d_ in (cur, targ):
        sd = torch.load(os.path.join(d_, "model_state_dict.pt"), map_location="cpu")
        assert sd["fc1.weight"].shape == (5000, 81) and all(torch.isfinite(v.float()).all() for v in sd.values())
    log = open(os.path.join(save, "t", "output.txt")).read()
    assert log.count("Updating cost-to-go with value iteration") == 2 and log.count("Updating target network") == 2
    assert "Using GBFS with 2 step(s) to add extra states to training set" in log
    assert len(re.findall(r"Itr: \d+, lr: [\d.E+-]+, loss: [\d.E+-]+, targ_ctg: [\d.-]+, nnet_ctg: [\d.-]+, Time: [\d.]+", log)) >= 1
    assert len(re.findall(r"Back Steps: \d+, %Solved: [\d.]+, avgSolveSteps: [\d.]+, CTG Mean\(Std/Min/Max\): ", log)) >= 5
    m = re.findall(r"Cost-to-go \(mean/min/max\): ([\d.]+)/([\d.]+)/([\d.]+)", log)
    assert len(m) == 2 and float(m[0][1]) == 0.0 and float(m[0][2]) == 1.0  # all-zeros target: 1 everywhere but at the goal


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_dims_2_and_8_are_refused_at_every_entry_point(L):
    from deepcubea_amd.utils import env_utils
    lib = L.lib()
    i64 = C.c_int64
    one = torch.zeros(64 * 4 * 4, dtype=torch.uint8, device="cuda")
    p, s = C.c_void_p(one.data_ptr()), L.stream_ptr()
    host = np.zeros(256, np.uint8).ctypes.data_as(C.c_void_p)
    for dim in (2, 8):
        eng = C.c_void_p(0)
        calls = {
            "dca_npuzzle_swap_table": lambda: lib.dca_npuzzle_swap_table(dim, host),
            "dca_npuzzle_next_state": lambda: lib.dca_npuzzle_next_state(p, i64(1), dim, 0, p, s),
            "dca_npuzzle_prev_state": lambda: lib.dca_npuzzle_prev_state(p, i64(1), dim, 0, p, s),
            "dca_npuzzle_expand_fused": lambda: lib.dca_npuzzle_expand_fused(p, i64(1), dim, p, None, 0, None, None, s),
            "dca_is_solved": lambda: lib.dca_is_solved(L.ENV_NPUZZLE, dim, p, i64(1), p, s),
            "dca_nnet_input": lambda: lib.dca_nnet_input(L.ENV_NPUZZLE, dim, p, i64(1), p, s),
            "dca_generate_states": lambda: lib.dca_generate_states(L.ENV_NPUZZLE, dim, i64(1), 0, 1, C.c_uint64(1), i64(0), p, None, None, 1, s),
            "dca_engine_create": lambda: lib.dca_engine_create(C.byref(eng), L.ENV_NPUZZLE, dim, C.c_double(1.0), 4, i64(1 << 12),
                                                               L.SEM_PY, -1),
            "dca_engine_create_multi": lambda: lib.dca_engine_create_multi(C.byref(eng), L.ENV_NPUZZLE, dim, C.c_double(1.0), 4,
                                                                           i64(1 << 12), L.SEM_PY, -1, 2),
        }
        for name, fn in calls.items():
            assert fn() == -1, (name, dim)
            assert b"3..7" in lib.dca_last_error(), (name, dim, lib.dca_last_error())
        assert not eng.value
    torch.cuda.synchronize()
    assert int(one.sum()) == 0  # nothing was launched
    for bad in ("puzzle3", "puzzle63"):
        with pytest.raises(ValueError):
            env_utils.get_environment(bad)
        with pytest.raises(ValueError):
            L.env_ids(bad)
