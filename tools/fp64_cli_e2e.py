"""The fp64 heuristic mode end to end through the CLI (`python -m deepcubea_amd.search_methods.astar`), against the fp32 parity
mode on the same states: seeded cube3 scrambles, `--model_dir synthetic:SEED`, one batch size.  Prints per mode the wall time,
nodes generated / expanded per second (expanded = generated / 12 on cube3) and the network's share of the search time (the
heuristic closure timed with a device synchronise on each side of every call).
Usage: python tools/fp64_cli_e2e.py [n_states] [min_moves] [max_moves] [batch] [weight] [seed] [mode ...]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from deepcubea_amd.environments.cube3 import Cube3State
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils, nnet_utils
    from oracle import c_oracle as co
    a = sys.argv[1:]
    n, lo, hi = int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 6, int(a[2]) if len(a) > 2 else 8
    batch, weight, seed = int(a[3]) if len(a) > 3 else 10000, float(a[4]) if len(a) > 4 else 0.6, int(a[5]) if len(a) > 5 else 2028
    modes = a[6:] or ["fp32", "fp64"]
    rng = np.random.default_rng(12345)
    states = []
    for _ in range(n):
        s = np.arange(54, dtype=np.uint8)[None]
        for mv in rng.integers(0, 12, int(rng.integers(lo, hi + 1))):
            s = co.next_state("cube3", s, int(mv))
        states.append(Cube3State(s[0].astype(np.int64)))
    tmp = tempfile.mkdtemp()
    spath = os.path.join(tmp, "states.pkl")
    data_utils.dump_pickle({"states": states}, spath)
    orig = nnet_utils.get_heuristic_fn_dev
    net_s = [0.0]

    def timed_closure(*args, **kw):
        fn = orig(*args, **kw)

        def wrapped(x, *a2, **k2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = fn(x, *a2, **k2)
            torch.cuda.synchronize()
            net_s[0] += time.perf_counter() - t0
            return y
        wrapped.valid_rows = None
        return wrapped

    nnet_utils.get_heuristic_fn_dev = timed_closure
    print("%d cube3 scrambles of %d-%d moves, batch %d, weight %g, synthetic:%d" % (n, lo, hi, batch, weight, seed))
    for mode in modes:
        rdir = os.path.join(tmp, mode)
        net_s[0] = 0.0
        t0 = time.perf_counter()
        astar.main(["--states", spath, "--model_dir", "synthetic:%d" % seed, "--env", "cube3", "--weight", str(weight),
                    "--batch_size", str(batch), "--results_dir", rdir, "--language", "hip", "--nnet_batch_size", "10000",
                    "--nnet_dtype", mode, "--instances_per_gpu", "1", "--debug"])
        wall = time.perf_counter() - t0
        res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
        gen, search = float(sum(res["num_nodes_generated"])), float(sum(res["times"]))
        print("%s: wall %.2f s, search time %.2f s, nodes generated %d -> %.3e generated/s, %.3e expanded/s; network %.2f s = "
              "%.1f %% of the search time; solution lengths %s"
              % (mode, wall, search, gen, gen / search, gen / 12 / search, net_s[0], 100.0 * net_s[0] / search,
                 [len(s) for s in res["solutions"]]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
