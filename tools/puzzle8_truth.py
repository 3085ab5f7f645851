#!/usr/bin/env python3
"""update -> train -> search on puzzle8, judged against GROUND TRUTH: does the chain converge to optimal solutions?

The 8-puzzle is the one environment of the family whose whole state space (181 440 states, eccentricity 31) fits in a table.
This runs `ctg_approx/avi.py --env puzzle8` for a stated wall-time budget on one MI355X, then evaluates the network that came
out on ALL states against their exact breadth-first distances, and runs BWAS (`BwasEngine`, the network in the loop) on a fixed
sample of states with the search settings of the reference's puzzle15 line (train.sh: weight 0.8, batch 20 000) and at weight 1.

    python tools/puzzle8_truth.py [train_seconds=600] [out=profiles/puzzle8_e2e.txt] [states_per_update=500000] [sample=2000] [total_seconds=0]

total_seconds > 0 is a wall-time budget for the whole run: the searches of a weight stop at their share of what is left and the row
says how many states of the (fixed, ordered) sample it covers.

Reports: mean and max |h - d| per depth, the share of states with round(h) == d, the share of the sample solved optimally per
weight.  No number is fixed in advance: the file records what was measured and for how long.  Seeds are fixed."""
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcubea_amd import _lib  # noqa: E402
from deepcubea_amd.ctg_approx import avi  # noqa: E402
from deepcubea_amd.search_methods.engine import BwasEngine  # noqa: E402
from deepcubea_amd.utils import env_utils, nnet_utils  # noqa: E402
from deepcubea_amd.utils.pytorch_models import FastResnet  # noqa: E402

FACT = np.array([40320, 5040, 720, 120, 24, 6, 2, 1, 1], np.int64)


def rank(states):
    s = np.asarray(states, np.int64)
    r = np.zeros(len(s), np.int64)
    for i in range(9):
        r += (s[:, i + 1:] < s[:, i:i + 1]).sum(1) * FACT[i]
    return r


def move(states, a, swap):
    rows = np.arange(len(states))
    z = np.argmax(states == 0, axis=1)
    t = swap[z, a]
    out = states.copy()
    out[rows, z] = states[rows, t]
    out[rows, t] = 0
    return out


def bfs(swap):
    """-> (states in breadth-first order, their distances) over the library's own swap table."""
    dist = np.full(362880, -1, np.int8)
    front = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 0]], np.uint8)
    dist[rank(front)] = 0
    layers, d = [front], 0
    while len(front):
        ch = np.concatenate([move(front, a, swap) for a in range(4)])
        r = rank(ch)
        new = dist[r] < 0
        r, first = np.unique(r[new], return_index=True)
        front = ch[new][first]
        d += 1
        dist[r] = d
        if len(front):
            layers.append(front)
    states = np.concatenate(layers)
    return states, dist[rank(states)].astype(np.int64)


def main():
    train_s = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "puzzle8_e2e.txt")
    spu = int(sys.argv[3]) if len(sys.argv) > 3 else 500_000
    n_sample = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    total_s = float(sys.argv[5]) if len(sys.argv) > 5 else 0.0
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    _lib.require_gpu()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    t0 = time.time()
    states, dist = bfs(_lib.npuzzle_swap_table(3))
    assert len(states) == 181440 and dist.max() == 31
    say("puzzle8 end to end against the breadth-first table (181 440 states, eccentricity 31; table built in %.2f s)" % (time.time() - t0))
    save = tempfile.mkdtemp()
    argv = ["--env", "puzzle8", "--states_per_update", str(spu), "--batch_size", "10000", "--nnet_name", "puzzle8", "--max_itrs",
            "100000000", "--loss_thresh", "0.1", "--back_max", "40", "--num_test", "1000", "--save_dir", save, "--max_seconds",
            str(train_s), "--update_nnet_batch_size", "100000", "--seed", "0", "--l1_train", "embed"]
    say("avi.py " + " ".join("<tmp>" if a == save else a for a in argv))
    t1 = time.time()
    try:
        avi.main(argv)
    finally:
        sys.stdout = sys.__stdout__
    train_wall = time.time() - t1
    cur = os.path.join(save, "puzzle8", "current")
    import pickle
    itr = pickle.load(open(os.path.join(cur, "train_itr.pkl"), "rb"))
    upd = pickle.load(open(os.path.join(cur, "update_num.pkl"), "rb"))
    say("trained for %.0f s wall (budget %.0f s): %d iterations of batch 10 000, %d target updates" % (train_wall, train_s, itr, upd))
    env = env_utils.get_environment("puzzle8")
    net = nnet_utils.load_nnet(os.path.join(cur, "model_state_dict.pt"), env.get_nnet_model(), device=torch.device("cuda"))
    fast = FastResnet(net.cuda().eval()).cuda()
    hfn = nnet_utils.get_heuristic_fn_dev(fast, clip_zero=False, batch_size=1 << 17)
    h = hfn(torch.from_numpy(states).cuda()).double().cpu().numpy()
    err = np.abs(h - dist)
    say("depth  states  mean|h-d|  max|h-d|  mean h")
    for k in range(32):
        sel = dist == k
        say("%5d  %6d  %9.4f  %8.4f  %6.3f" % (k, int(sel.sum()), err[sel].mean(), err[sel].max(), h[sel].mean()))
    say("all states: mean |h-d| %.4f, max %.4f, round(h) == d on %.2f %%" % (err.mean(), err.max(), 100.0 * float((np.rint(h) == dist).mean())))
    sample = np.random.default_rng(8).choice(len(states), n_sample, replace=False)
    for wi, w in enumerate((0.8, 1.0)):
        eng = BwasEngine("puzzle8", w, 20000, max_nodes=1 << 22, packed=True)
        t2 = time.time()
        stop_at = t2 + (t0 + total_s - t2) / (2 - wi) if total_s > 0 else float("inf")
        solved = optimal = extra = done = 0
        for i in sample:
            if time.time() > stop_at:
                break
            done += 1
            res = eng.solve(states[i], hfn, max_iters=2000)
            if res["solved"]:
                solved += 1
                optimal += int(len(res["moves"]) == dist[i])
                extra += len(res["moves"]) - int(dist[i])
        eng.close()
        say("BWAS weight %.1f batch 20000, first %d of the %d sampled states: %d solved, %d optimal (%.2f %%), mean excess length %.4f, %.1f s"
            % (w, done, n_sample, solved, optimal, 100.0 * optimal / max(done, 1), extra / max(solved, 1), time.time() - t2))
    say("total wall %.0f s" % (time.time() - t0))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
