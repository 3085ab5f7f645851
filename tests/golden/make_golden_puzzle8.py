#!/usr/bin/env python3
"""puzzle8 fixtures recorded by IMPORTING the reference (build container only; /root/reference never travels):

    python tests/golden/make_golden_puzzle8.py   ->  tests/golden/puzzle8.npz

Data only — inputs and what the reference's own functions returned for them:
  environments/n_puzzle.py     NPuzzle(3): swap_zero_idxs, goal, next_state, prev_state, expand, is_solved,
                               state_to_nnet_input, get_num_moves, the network's dimensions
  search_methods/astar.py      AStar (python BWAS) traces on scrambles of 8-20 moves with the deterministic heuristics shared
                               with include/dca.h (DCA_HEUR_MOD97 / DCA_HEUR_KNUTH3): B = 1, 7, 100, 1000, and a goal root
  utils/pytorch_models.py      ResnetModel(9, 9, 128, 64, 1, 1, True) in eval mode: its weights and running statistics, 64
                               inputs, its fp32 outputs, and oracle/np_oracle.py's float64 evaluation of the same weights
"""
import os
import sys

import numpy as np

np.float = float  # noqa: the reference targets numpy 1.22
np.int = int  # noqa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402
from environments.n_puzzle import NPuzzle, NPuzzleState  # noqa: E402
from search_methods.astar import AStar, get_path  # noqa: E402
from utils.pytorch_models import ResnetModel  # noqa: E402
from make_golden import heur_knuth3, heur_mod97  # noqa: E402
from make_golden_nets import det_weights  # noqa: E402
from oracle import np_oracle as no  # noqa: E402


def main():
    torch.set_num_threads(1)
    g = {}
    env = NPuzzle(3)
    g["swap_zero_idxs"] = env.swap_zero_idxs.astype(np.uint8)
    g["goal"] = env.goal_tiles.astype(np.uint8)
    g["num_moves"] = np.array(env.get_num_moves())
    net = env.get_nnet_model()
    g["nnet_dims"] = np.array([net.state_dim, net.one_hot_depth, net.fc1.out_features, net.fc2.out_features, net.num_resnet_blocks])

    def mk(a):
        return NPuzzleState(np.asarray(a).astype(env.dtype))

    # 64 states scrambled from the goal (walks of 0..40 moves; ineligible moves are no-ops in the reference)
    rng = np.random.default_rng(8)
    S = np.zeros((64, 9), np.uint8)
    for i in range(64):
        st = mk(env.goal_tiles.copy())
        for a in rng.integers(0, 4, size=int(rng.integers(0, 41))):
            st = env.next_state([st], int(a))[0][0]
        S[i] = st.tiles
    g["states"] = S
    states = [mk(s.copy()) for s in S]
    nxt = np.zeros((4, 64, 9), np.uint8)
    rev = {0: 1, 1: 0, 2: 3, 3: 2}
    for a in range(4):
        ns, tc = env.next_state(states, a)
        assert all(t == 1.0 for t in tc)
        nxt[a] = np.stack([x.tiles for x in ns])
        moved = [i for i in range(64) if not np.array_equal(nxt[a][i], S[i])]
        back, _ = env.next_state([ns[i] for i in moved], rev[a])
        assert all(np.array_equal(b.tiles, S[i]) for b, i in zip(back, moved))  # move o inverse = identity where the move is legal
        ps = env.prev_state([ns[i] for i in moved], a)
        assert all(np.array_equal(p.tiles, S[i]) for p, i in zip(ps, moved))
    g["next_state_all_actions"] = nxt
    exp, tcs = env.expand(states[:8])
    g["expand_children_8"] = np.stack([np.stack([c.tiles for c in row]) for row in exp]).astype(np.uint8)
    assert all(np.all(t == 1.0) for t in tcs)
    probe = [mk(env.goal_tiles.copy())] + [env.next_state([mk(env.goal_tiles.copy())], a)[0][0] for a in (1, 3)] + states[:5]
    g["is_solved_probe_states"] = np.stack([s.tiles for s in probe]).astype(np.uint8)
    g["is_solved_probe"] = env.is_solved(probe)
    g["nnet_input_64"] = env.state_to_nnet_input(states)[0]

    def run_ref_astar(root_arr, heur, w, B):
        def hfn(sts, is_nnet_format=False):
            arr = np.stack([s.tiles for s in sts]).astype(np.uint8)
            return np.maximum(heur(arr).astype(np.float64), 0.0)
        astar = AStar([mk(root_arr.copy())], env, hfn, [w])
        trace = []
        while not min(astar.has_found_goal()):
            astar.step(hfn, B)
            inst = astar.instances[0]
            trace.append((len(inst.open_set), len(inst.closed_dict), inst.num_nodes_generated))
            assert len(trace) < 100000
        goal_node = astar.get_goal_node_smallest_path_cost(0)
        _, moves, pc = get_path(goal_node)
        return np.array(trace, np.int64), np.array(moves, np.int32), float(pc), astar.get_num_nodes_generated(0)

    cases = []
    for ci, (scr, w, B, hname) in enumerate([
            ([1, 3, 1, 3, 0, 2, 0, 3], 0.8, 1, "knuth3"),
            ([1, 1, 3, 3, 0, 2, 0, 3, 1, 2, 1, 3], 0.6, 7, "mod97"),
            ([3, 1, 3, 0, 2, 1, 3, 0, 0, 2, 1, 1, 3, 0, 2, 0], 0.8, 100, "knuth3"),
            ([1, 3, 3, 1, 2, 0, 2, 1, 3, 0, 3, 0, 2, 2, 1, 3, 1, 2, 0, 0], 0.5, 1000, "mod97"),
            ([3, 3, 1, 1, 2, 0, 2, 0, 3, 1], 1.0, 1000, "knuth3"),
            ([], 0.8, 10, "mod97")]):
        st = mk(env.goal_tiles.copy())
        for a in scr:
            st = env.next_state([st], a)[0][0]
        root = st.tiles.astype(np.uint8)
        tr, mv, pc, nn = run_ref_astar(root, heur_mod97 if hname == "mod97" else heur_knuth3, w, B)
        print("puzzle8 trace", scr, w, B, hname, "->", mv.tolist(), pc, nn, len(tr))
        key = "astar_py_puzzle8_%d" % ci
        g[key + "_root"] = root
        g[key + "_cfg"] = np.array([w, B, 0 if hname == "mod97" else 1], np.float64)
        g[key + "_trace"] = tr
        g[key + "_moves"] = mv
        g[key + "_result"] = np.array([pc, nn], np.float64)
        cases.append(key)
    g["astar_py_cases"] = np.array(cases)

    # a small network of the puzzle8 geometry; fc_out rescaled so that |h| <= 1 (the regime of the 1e-5 absolute bound)
    small = ResnetModel(9, 9, 128, 64, 1, 1, True)
    det_weights(small, 2038)
    small.eval()
    x = np.stack([rng.permutation(9) for _ in range(64)]).astype(np.uint8)
    with torch.no_grad():
        y0 = small(torch.tensor(x)).numpy()[:, 0]
        s = 0.9 / max(float(np.abs(y0).max()), 1e-6)
        small.fc_out.weight.mul_(s)
        small.fc_out.bias.mul_(s)
        y32 = small(torch.tensor(x)).numpy()[:, 0]
    sd = {k: v.numpy() for k, v in small.state_dict().items()}
    y64 = no.resnet_forward(sd, x, 9, 1, np.float64)
    print("small net: max|y32|", np.abs(y32).max(), " fp32 vs float64: max abs", np.abs(y32 - y64).max())
    assert np.abs(y32).max() <= 1.0
    for k, v in sd.items():
        g["net_" + k] = v
    g["net_keys"] = np.array(list(sd.keys()))
    g["net_x"] = x
    g["net_y32"] = y32.astype(np.float32)
    g["net_y64"] = y64.astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "puzzle8.npz"), **g)
    print("wrote", os.path.join(HERE, "puzzle8.npz"), os.path.getsize(os.path.join(HERE, "puzzle8.npz")), "bytes")


if __name__ == "__main__":
    main()
