#!/usr/bin/env python3
"""How far is a lightsout7 network from the true cost-to-go?  The exact distance of ANY lightsout7 state is popcount(A^-1 s) over
GF(2) (include/dca.h "exact LightsOut heuristic"), so the question puzzle8 answers from a breadth-first table
(tools/puzzle8_truth.py) is answered here for the environment the reference trains with ASTAR updates.

    python tools/lightsout7_truth.py MODEL [n=200000] [out=profiles/lightsout7_truth.txt] [note]

MODEL is a model directory (model_state_dict.pt inside, e.g. <save_dir>/lightsout7/current of a `ctg_approx/avi.py --env
lightsout7` run) or synthetic:SEED.  The states are scrambles over the reference's back-step range (train.sh:65: 0..50) drawn
by the library's generator; the network and dca_lightsout_exact_eval see the same device rows.  `note` is copied into the
output: the place to say which run made the model, for how long and with which seeds.

Reports: mean and max |h - h*| per exact distance, the share with round(h) == h*, and the distribution of h* against the number
of back steps.  No training here and no number fixed in advance: the file records what was measured, from which model and seed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACK_MAX = 50  # train.sh:65
SCRAMBLE_SEED = 7


def error_by_distance(h, h_star):
    """h: network values, h_star: exact distances (same length) -> (rows, summary).  rows: one (distance, states, mean |h - h*|,
    max |h - h*|, mean h) per distance that occurs, ascending; summary: (mean |h - h*|, max |h - h*|, share with
    round(h) == h*) over all states."""
    h, h_star = np.asarray(h, np.float64).reshape(-1), np.asarray(h_star, np.int64).reshape(-1)
    if h.shape != h_star.shape or h.size == 0:
        raise ValueError("error_by_distance: two non-empty arrays of one length, not %s and %s" % (h.shape, h_star.shape))
    err = np.abs(h - h_star)
    rows = []
    for d in np.unique(h_star):
        sel = h_star == d
        rows.append((int(d), int(sel.sum()), float(err[sel].mean()), float(err[sel].max()), float(h[sel].mean())))
    return rows, (float(err.mean()), float(err.max()), float((np.rint(h) == h_star).mean()))


def distance_by_back_steps(h_star, num_back):
    """exact distances and the back steps of the scrambles that made them -> one (back steps, states, min h*, mean h*, max h*,
    share with h* == back steps) per number of back steps that occurs, ascending.  (h* <= back steps, same parity.)"""
    h_star, num_back = np.asarray(h_star, np.int64).reshape(-1), np.asarray(num_back, np.int64).reshape(-1)
    if h_star.shape != num_back.shape:
        raise ValueError("distance_by_back_steps: two arrays of one length, not %s and %s" % (h_star.shape, num_back.shape))
    rows = []
    for k in np.unique(num_back):
        v = h_star[num_back == k]
        rows.append((int(k), int(v.size), int(v.min()), float(v.mean()), int(v.max()), float((v == k).mean())))
    return rows


def _network(model: str):
    import torch
    from deepcubea_amd.utils import env_utils, nnet_utils
    from deepcubea_amd.utils.pytorch_models import FastResnet
    env = env_utils.get_environment("lightsout7")
    net = env.get_nnet_model()
    if model.startswith("synthetic:"):
        from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
        load_synthetic_weights(net, int(model.split(":", 1)[1]))
        what = "synthetic weights, seed %d (untrained: the figures show the tool, not a heuristic)" % int(model.split(":", 1)[1])
    else:
        net = nnet_utils.load_nnet(os.path.join(model, "model_state_dict.pt"), net, device=torch.device("cuda"))
        what = "model directory %s" % model
        for name in ("train_itr.pkl", "update_num.pkl"):
            path = os.path.join(model, name)
            if os.path.exists(path):
                import pickle
                what += ", %s %s" % (name[:-4], pickle.load(open(path, "rb")))
    fast = FastResnet(net.cuda().eval()).cuda()
    return nnet_utils.get_heuristic_fn_dev(fast, clip_zero=False, batch_size=1 << 17), what


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    model = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lightsout7_truth.txt")
    note = sys.argv[4] if len(sys.argv) > 4 else ""
    import torch
    from deepcubea_amd import _lib
    _lib.require_gpu()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    t0 = time.time()
    hfn, what = _network(model)
    env, dim = _lib.env_ids("lightsout7")[:2]
    states, num_back, _ = _lib.generate_states(env, dim, n, 0, BACK_MAX, SCRAMBLE_SEED)
    h_star = _lib.lightsout_exact_eval(states)
    h = hfn(states)
    torch.cuda.synchronize()
    say("lightsout7: a network against the exact distance popcount(A^-1 s) (tools/lightsout7_truth.py)")
    say("network: %s; fp32 inference path (FastResnet)" % what)
    if note:
        say("model made by: %s" % note)
    say("states: %d scrambles of 0..%d back steps, dca_generate_states seed %d; wall %.1f s" % (n, BACK_MAX, SCRAMBLE_SEED, time.time() - t0))
    rows, (mean, worst, share) = error_by_distance(h.double().cpu().numpy(), h_star.cpu().numpy())
    say("   h*  states  mean|h-h*|  max|h-h*|   mean h")
    for d, count, m, w, mh in rows:
        say("%5d  %6d  %10.4f  %9.4f  %7.3f" % (d, count, m, w, mh))
    say("all states: mean |h-h*| %.4f, max %.4f, round(h) == h* on %.2f %%" % (mean, worst, 100.0 * share))
    say(" back  states  min h*  mean h*  max h*  h* == back")
    for k, count, lo, m, hi, eq in distance_by_back_steps(h_star.cpu().numpy(), num_back.cpu().numpy()):
        say("%5d  %6d  %6d  %7.3f  %6d  %8.2f %%" % (k, count, lo, m, hi, 100.0 * eq))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
