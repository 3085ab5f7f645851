"""Record tests/golden/ref_envs.json: SHA-256 digests of what the reference's own compiled environments (oracle/_ref, built by
`make -C oracle ref` where the reference's sources lie) return on the seeded inputs of the CPU tests that compare the
oracle with them (test_oracle_golden.py, test_lightsout_cpu.py, test_cube4_cpu.py).  The tests check the oracle against
these records, so they need no reference build.  Run from the repository root after `make -C oracle all ref`:

    python tests/golden/make_golden_ref_envs.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import c_oracle as co  # noqa: E402
from tests.conftest import synth_states  # noqa: E402


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()


def cube4_states(n, seed):  # test_cube4_cpu._states
    rng = np.random.default_rng(seed)
    return rng.permuted(np.tile(np.arange(96, dtype=np.uint8), (n, 1)), axis=1)


def main():
    assert co.ref_lib() is not None, "oracle/_ref not built"
    rec = {}
    # test_oracle_golden.test_reference_cpp_envs_agree
    ch, sv = co.ref_expand("cube3", synth_states(256, 54, 11))
    rec["cube3_synth256_seed11_expand"] = [sha(ch), sha(sv)]
    for name, n in [("puzzle15", 4), ("puzzle24", 5), ("puzzle35", 6), ("puzzle48", 7)]:
        ch, sv = co.ref_expand(name, synth_states(128, n * n, 12))
        rec[name + "_synth128_seed12_expand"] = [sha(ch), sha(sv)]
        goal = np.concatenate((np.arange(1, n * n), [0])).astype(np.uint8)[None]
        rec[name + "_goal_expand_solved"] = co.ref_expand(name, goal)[1].astype(int).tolist()
    # test_lightsout_cpu.test_oracle_moves_equal_the_reference_cpp_env
    rng = np.random.default_rng(5)
    S = rng.integers(0, 2, size=(3000, 49)).astype(np.uint8)
    S[0] = 0
    S[1] = co.next_state("lightsout7", S[:1], 24)[0]
    ch, sv = co.ref_expand("lightsout7", S)
    rec["lightsout7_rand3000_seed5_expand"] = [sha(ch), sha(sv)]
    for a in (0, 6, 24, 42, 48, 13):
        rec["lightsout7_rand3000_seed5_next_state_%d" % a] = sha(co.ref_next_state("lightsout7", S, a))
    # test_cube4_cpu.test_cube4_oracle_vs_reference_class
    s = cube4_states(300, 1)
    rec["cube4_rand300_seed1_next_state_all_actions"] = sha(np.stack([co.ref_next_state("cube4", s, a) for a in range(24)]))
    ch, sv = co.ref_expand("cube4", s[:64])
    rec["cube4_rand64_seed1_expand"] = [sha(ch), sha(sv)]
    goal = np.arange(96, dtype=np.uint8)
    same_colours = goal.copy()
    rng = np.random.default_rng(2)
    for f in range(6):
        same_colours[f * 16:(f + 1) * 16] = f * 16 + rng.permutation(16)
    swapped_faces = np.concatenate([goal[16:32], goal[0:16], goal[32:]])
    one_off = goal.copy()
    one_off[[5, 21]] = one_off[[21, 5]]
    cases = np.stack([goal, same_colours, swapped_faces, one_off, s[0], co.next_state("cube4", goal[None], 7)[0]])
    got = np.empty(len(cases), np.uint8)
    co.ref_lib().ref_is_solved(3, 0, co._p8(cases), co.C.c_int64(len(cases)), co._p8(got))
    rec["cube4_is_solved_cases"] = [int(v != 0) for v in got]
    with open(os.path.join(ROOT, "tests", "golden", "ref_envs.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
