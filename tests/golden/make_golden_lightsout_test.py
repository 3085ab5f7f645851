#!/usr/bin/env python3
"""The reference's shipped lightsout7 test set and its recorded run (build container only; /root/reference never travels):

    python tests/golden/make_golden_lightsout_test.py   ->  tests/golden/lightsout_test.npz

Data only — what two of the reference's pickles hold:
  data/lightsout7/test/data_0.pkl    the 500 test states                      -> states    uint8 [500, 49]
  results/lightsout7/results.pkl     the solutions its search recorded for    -> soln_len  int16 [500]
                                     them (train.sh:68: weight 0.2,              solutions int8 [sum soln_len], the presses of
                                     batch 1000)                                 state i at solution_offsets[i] : [i + 1]
                                                                                 solution_offsets int32 [501]
"""
import os
import pickle
import sys

import numpy as np

np.float = float  # noqa: the reference targets numpy 1.22
np.int = int  # noqa

sys.path.insert(0, "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    with open("/root/reference/data/lightsout7/test/data_0.pkl", "rb") as f:
        data = pickle.load(f)
    with open("/root/reference/results/lightsout7/results.pkl", "rb") as f:
        results = pickle.load(f)
    states = np.stack([np.asarray(s.tiles) for s in data["states"]]).astype(np.uint8)
    recorded = np.stack([np.asarray(s.tiles) for s in results["states"]]).astype(np.uint8)
    assert states.shape == (500, 49) and np.array_equal(states, recorded) and set(np.unique(states)) <= {0, 1}
    solutions = [[int(a) for a in soln] for soln in results["solutions"]]
    assert len(solutions) == 500 and all(0 <= a < 49 for soln in solutions for a in soln)
    lens = np.array([len(s) for s in solutions], np.int16)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    flat = np.array([a for soln in solutions for a in soln], np.int8)
    path = os.path.join(OUT, "lightsout_test.npz")
    np.savez_compressed(path, states=states, soln_len=lens, solutions=flat, solution_offsets=offsets)
    print("wrote", path, os.path.getsize(path), "bytes; lengths min %d max %d mean %.2f" % (lens.min(), lens.max(), lens.mean()))


if __name__ == "__main__":
    main()
