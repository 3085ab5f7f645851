"""CPU: the oracle's LightsOut (oracle/dca_oracle.cpp) pinned to (a) fixtures recorded by importing the reference's
environments/lights_out.py and search_methods/astar.py (tests/golden/make_golden_lightsout.py) and (b) the reference's own
cpp/environments.cpp compiled in place (oracle/_ref; its answers recorded in tests/golden/ref_envs.json), plus the host logic of the Environment mirror."""
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lo():
    return np.load(os.path.join(ROOT, "tests", "golden", "lightsout.npz"))


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    return c_oracle


def test_oracle_moves_equal_the_reference_python_env(lo, co):
    S = lo["states"]
    for a in range(49):
        assert np.array_equal(co.next_state("lightsout7", S, a), lo["next_state_all_actions"][a]), a
    ch, sv, _ = co.expand("lightsout7", S[:8])
    assert np.array_equal(ch, lo["expand_children_8"]) and not sv.any()
    assert np.array_equal(co.is_solved("lightsout7", lo["is_solved_probe_states"]), lo["is_solved_probe"])
    assert np.array_equal(co.nnet_input("lightsout7", S), lo["nnet_input_64"])
    assert np.array_equal(lo["goal"], np.zeros((3, 49), np.uint8)) and int(lo["num_moves"]) == 49
    assert lo["nnet_dims"].tolist() == [49, 6, 5000, 1000, 4]


def test_oracle_moves_equal_the_reference_cpp_env(co):
    """Digests of the reference's compiled environment on these states: tests/golden/ref_envs.json (make_golden_ref_envs.py)."""
    with open(os.path.join(ROOT, "tests", "golden", "ref_envs.json")) as f:
        ref = json.load(f)
    rng = np.random.default_rng(5)
    S = rng.integers(0, 2, size=(3000, 49)).astype(np.uint8)
    S[0] = 0
    S[1] = co.next_state("lightsout7", S[:1], 24)[0]  # one press from the goal: a solved child exists
    ch, sv, _ = co.expand("lightsout7", S)
    assert [_sha(ch), _sha(sv)] == ref["lightsout7_rand3000_seed5_expand"] and sv.sum() >= 1
    for a in (0, 6, 24, 42, 48, 13):
        assert _sha(co.next_state("lightsout7", S, a)) == ref["lightsout7_rand3000_seed5_next_state_%d" % a], a


def test_oracle_python_semantics_reproduces_reference_astar_traces(lo, co):
    for key in [str(k) for k in lo["astar_py_cases"]]:
        w, B, hid = lo[key + "_cfg"]
        res = co.astar("lightsout7", lo[key + "_root"], float(w), int(B), co.SEM_PY, heur_builtin_id=int(hid), trace_cap=4096)
        pc, nn = lo[key + "_result"]
        assert res["solved"] and res["moves"] == lo[key + "_moves"].tolist(), key
        assert res["path_cost"] == pc and res["nodes_generated"] == int(nn), key
        assert np.array_equal(res["trace"], lo[key + "_trace"]), key


def test_environment_mirror_host_side(lo):
    from deepcubea_amd.environments.lights_out import LightsOut, LOState
    from deepcubea_amd.utils import data_utils, env_utils
    env = env_utils.get_environment("lightsout7")
    assert isinstance(env, LightsOut) and env.get_num_moves() == 49 and env.state_dim == 49
    assert np.array_equal(env.move_matrix, lo["move_matrix"])
    net = env.get_nnet_model()
    assert (net.state_dim, net.one_hot_depth) == (49, 6)
    goal = env.generate_goal_states(2)
    assert isinstance(goal[0], LOState) and not goal[0].tiles.any()
    assert goal[0] == goal[1] and hash(goal[0]) == hash(goal[1])
    with pytest.raises(ValueError):
        env_utils.get_environment("lightsout5")
    # results written here carry the reference's class path (environments.lights_out.LOState) and load back
    import tempfile
    p = os.path.join(tempfile.mkdtemp(), "r.pkl")
    data_utils.dump_pickle({"states": goal}, p)
    assert b"environments.lights_out" in open(p, "rb").read() and b"deepcubea_amd" not in open(p, "rb").read()
    back = data_utils.load_pickle(p)["states"]
    assert isinstance(back[0], LOState) and back[0] == goal[0]
