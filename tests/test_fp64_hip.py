"""The float64 heuristic mode (`--nnet_dtype fp64`) on the MI355X: dca_gemm64 (v_mfma_f64_16x16x4_f64) and dca_l1_embed64 exact
against host float64, `Fp64Resnet` within the north star's 1e-5 ABSOLUTE of the reference's fp32 forward at trained magnitudes,
batch / padding invariance, agreement with the library's float64 evaluation at scale, and the mode in the search loop."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from test_fp64_cpu import trained_magnitude_net

pytestmark = pytest.mark.gpu


def _host_gemm(a, w):
    return torch.from_numpy(a.cpu().numpy() @ w.cpu().numpy().T)


@pytest.mark.parametrize("k", [1024, 5120])
@torch.no_grad()
def test_gemm64_exact_on_integer_data(k):
    """Small integers: every product and partial sum is exact in float64, so the result must equal the host's bit for bit —
    which also pins the f64 C/D lane map (a wrong row map puts 3 of 4 results in the wrong row).  W is asymmetric."""
    from deepcubea_amd import _lib
    g = torch.Generator().manual_seed(k)
    n = 1024
    w = torch.randint(-4, 5, (n, k), generator=g).double()
    w[:, 0] += torch.arange(n, dtype=torch.float64)  # asymmetric, and every output unit distinct
    bias = torch.randint(-50, 51, (n,), generator=g).double()
    wd, bd = w.cuda(), bias.cuda()
    for m in (1, 17, 1000, 4099):
        a = torch.randint(-4, 5, (m, k), generator=g).double()
        a[:, 0] += torch.arange(m, dtype=torch.float64) % 7
        skip = torch.randint(-1000, 1001, (m, n), generator=g).double()
        ad = a.cuda()
        prod = _host_gemm(a, w)
        assert torch.equal(_lib.gemm64(ad, wd, None, None, False).cpu(), prod), (m, k)
        assert torch.equal(_lib.gemm64(ad, wd, bd, None, True).cpu(), (prod + bias).relu()), (m, k)
        assert torch.equal(_lib.gemm64(ad, wd, bd, skip.cuda(), False).cpu(), prod + bias + skip), (m, k)
        out = skip.cuda()  # the residual form: skip aliasing out
        _lib.gemm64(ad, wd, None, out, True, out=out)
        assert torch.equal(out.cpu(), (prod + skip).relu()), (m, k)


@torch.no_grad()
def test_gemm64_random_data_within_1e13():
    from deepcubea_amd import _lib
    g = torch.Generator().manual_seed(11)
    m, k, n = 4099, 5120, 1024
    a = torch.randn((m, k), generator=g, dtype=torch.float64)
    w = torch.randn((n, k), generator=g, dtype=torch.float64)
    got = _lib.gemm64(a.cuda(), w.cuda(), None, None, False).cpu()
    want = _host_gemm(a, w)
    scale = _host_gemm(a.abs(), w.abs())  # sum of |products|: the natural bound of a reordered sum's error
    assert float(((got - want).abs() / scale).max()) <= 1e-13


GEOMETRIES = [(54, 6), (16, 16), (25, 25), (36, 36), (49, 49), (49, 6)]  # cube3, puzzle15/24/35/48, lightsout7 (state_dim, depth)


@pytest.mark.parametrize("d,depth", GEOMETRIES)
@torch.no_grad()
def test_l1_embed64_bitwise_vs_host(d, depth):
    """Layer 1 in float64 for every geometry of the product: bias first, positions ascending — the host sums in the same order."""
    from deepcubea_amd import _lib
    g = torch.Generator().manual_seed(d * 100 + depth)
    n_pad, m = 5120, 3001
    wt = torch.randn((d * depth, n_pad), generator=g, dtype=torch.float64)
    b = torch.randn((n_pad,), generator=g, dtype=torch.float64)
    x = torch.randint(0, depth, (m, d), generator=g, dtype=torch.uint8)
    for relu in (False, True):
        got = _lib.l1_embed64(x.cuda(), depth, wt.cuda(), b.cuda(), relu).cpu()
        want = b.expand(m, -1).clone()
        for p in range(d):
            want += wt[p * depth + x[:, p].long()]
        if relu:
            want = want.relu()
        assert torch.equal(got, want), (d, depth, relu)


@pytest.mark.parametrize("key", ["cube3_big_seed2028", "cube3_big_seed2029", "cube3_big_seed2030", "puzzle48_big_seed2031"])
@torch.no_grad()
def test_fp64_mode_meets_the_north_star_at_trained_magnitudes(nets, key):
    """The fp32 parity mode is 1.34e-5 / 1.14e-5 from the reference's fp32 values on seeds 2029 / 2030 (test_parity_configs_hip);
    the reference's own fp32 forward is <= 7.2e-6 from float64, so float64-accurate values rounded once land inside 1e-5."""
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet
    net = trained_magnitude_net(nets, key)
    f = Fp64Resnet(net).cuda()
    x = torch.tensor(nets[key + "_x"]).cuda()
    y32, y64 = nets[key + "_y32"].astype(np.float64), nets[key + "_y64"]
    h64 = f.forward64(x)[:, 0].cpu().numpy()
    h32 = f(x)[:, 0].cpu().numpy()
    assert np.array_equal(h32, h64.astype(np.float32))  # one rounding, at the end
    rel64 = float(np.max(np.abs(h64 - y64) / np.maximum(1.0, np.abs(y64))))
    abs32 = float(np.max(np.abs(h32.astype(np.float64) - y32)))
    print("%s: fp64 mode vs float64 %.3e * |h|, fp32 output vs reference fp32 %.3e abs" % (key, rel64, abs32))
    assert rel64 <= 1e-9
    if key.startswith("cube3"):
        assert 20.0 < y64.min() and y64.max() < 30.0
        assert abs32 <= 1e-5
    else:  # puzzle48, |h| 100-280: no fp32 value meets 1e-5 absolute there; the float64 bar holds
        assert 99.0 < y64.min() and y64.max() < 300.0
    # the host path of the same re-layout agrees to float64 rounding
    hh = Fp64Resnet(net).forward64(x.cpu())[:, 0].numpy()
    assert np.max(np.abs(hh - h64) / np.maximum(1.0, np.abs(h64))) <= 1e-13


@torch.no_grad()
def test_fp64_values_do_not_depend_on_batch_or_padding(nets):
    from deepcubea_amd.utils import nnet_utils
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet
    key = "cube3_big_seed2029"
    f = Fp64Resnet(trained_magnitude_net(nets, key)).cuda()
    hfn = nnet_utils.get_heuristic_fn_dev(f, batch_size=1 << 17)
    x = torch.tensor(nets[key + "_x"]).cuda()
    n = x.shape[0]
    base = hfn(x)
    g = torch.Generator().manual_seed(5)
    pad = torch.randint(0, 6, (1024 - n, 54), generator=g, dtype=torch.uint8).cuda()
    assert torch.equal(hfn(torch.cat([x, pad]))[:n], base)  # padded to 1024 rows with random rows behind
    big = torch.randint(0, 6, (8192, 54), generator=g, dtype=torch.uint8).cuda()
    big[3001:3001 + n] = x  # at another position of a larger batch
    assert torch.equal(hfn(big)[3001:3001 + n], base)


@pytest.mark.parametrize("env", ["cube3", "puzzle48"])
@torch.no_grad()
def test_fp64_at_scale_against_library_float64(env):
    """131 072 random rows against the library's float64 evaluation of the module on the GPU.  (The module itself, BatchNorm
    applied in float64: `fold_batchnorm` rounds the folded weights to fp32, ~7e-8 relative away from the float64 fold.)"""
    import copy
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet, ResnetModel
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    D, depth = (54, 6) if env == "cube3" else (49, 49)
    net = ResnetModel(D, depth, 5000, 1000, 4, 1, True)
    load_synthetic_weights(net, 2028)
    net.eval()
    f = Fp64Resnet(net).cuda()
    ref = copy.deepcopy(net).double().cuda().eval()
    g = torch.Generator().manual_seed(7)
    m = 131072
    if env == "cube3":
        x = torch.randint(0, 6, (m, D), generator=g, dtype=torch.uint8)
    else:
        x = torch.argsort(torch.rand((m, D), generator=g), dim=1).to(torch.uint8)
    x = x.cuda()
    y = f.forward64(x)[:, 0]
    for s in range(0, m, 16384):  # (the module's one-hot input in float64: chunks)
        xb = x[s:s + 16384]
        oh = torch.nn.functional.one_hot(xb.long(), depth).view(xb.shape[0], -1).double()
        want = ref.forward_onehot(oh)[:, 0]
        assert float(((y[s:s + 16384] - want).abs() / want.abs().clamp_min(1.0)).max()) <= 1e-9


def _scrambles(env_name, scr):
    from oracle import c_oracle as co
    D = 54 if env_name == "cube3" else 16
    start = np.arange(D, dtype=np.uint8) if env_name == "cube3" else np.concatenate([np.arange(1, 16), [0]]).astype(np.uint8)
    roots = []
    for mv in scr:
        s = start[None].copy()
        for a in mv:
            s = co.next_state(env_name, s, a)
        roots.append(s[0])
    return roots


@pytest.mark.parametrize("env_name,scr", [("cube3", [[0, 5, 7, 2], [3, 8, 1]]), ("puzzle15", [[0, 2, 1, 3, 0, 2], [1, 1, 3, 3]])])
def test_fp64_closure_in_the_loop_matches_oracle(env_name, scr):
    """Dedup-first engine stepping with the fp64 closure vs the C++ oracle evaluating every child through the same closure
    (batches padded to 1024 rows, as __graft_entry__._engine_smoke does): moves, nodes generated, iterations identical."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    from deepcubea_amd.utils import nnet_utils
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet, ResnetModel
    from oracle import c_oracle as co
    torch.manual_seed(0)
    D, depth = (54, 6) if env_name == "cube3" else (16, 16)
    f = Fp64Resnet(ResnetModel(D, depth, 64, 32, 1, 1, True).eval()).cuda()
    hfn = nnet_utils.get_heuristic_fn_dev(f, batch_size=1024)
    nn_div = 9 if env_name == "cube3" else 1  # network input: cube3 colour index = sticker // 9; puzzles: the tiles
    for root in _scrambles(env_name, scr):
        eng = BwasEngine(env_name, 0.8, 50, max_nodes=1 << 18, packed=True)
        res = eng.solve(root, hfn)
        eng.close()

        def heur(states):
            x = torch.zeros((1024, D), dtype=torch.uint8, device="cuda")
            x[:len(states)] = torch.from_numpy(np.ascontiguousarray(states // nn_div)).cuda()
            return hfn(x)[:len(states)].cpu().numpy()

        ref = co.astar(env_name, root, 0.8, 50, co.SEM_PY, heur_fn=heur)
        assert res["solved"] and res["moves"] == ref["moves"], (res, ref)
        assert res["nodes_generated"] == ref["nodes_generated"] and res["iterations"] == ref["iterations"]


def test_cli_fp64_produces_valid_solutions(tmp_path):
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils
    from oracle import c_oracle as co
    from test_astar_cli_hip import _ref_pickle
    roots = _scrambles("cube3", [[0, 5, 7], [1, 3, 8, 10], [4, 9, 2, 6]])
    spath = str(tmp_path / "states.pkl")
    _ref_pickle(spath, roots)
    rdir = str(tmp_path / "res")
    try:
        astar.main(["--states", spath, "--model", "synthetic:11", "--env", "cube3", "--weight", "0.8", "--batch_size", "200",
                    "--results_dir", rdir, "--language", "hip", "--nnet_batch_size", "4096", "--max_nodes", str(1 << 21),
                    "--nnet_dtype", "fp64"])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert len(res["solutions"]) == len(roots)
    from deepcubea_amd.utils import env_utils, search_utils
    env = env_utils.get_environment("cube3")
    for state, soln in zip(res["states"], res["solutions"]):
        assert search_utils.is_valid_soln(state, soln, env)


def test_cli_fp64_rejects_eval_all_children(tmp_path):
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import env_utils
    args = astar.build_parser().parse_args(["--states", "s.pkl", "--model_dir", "synthetic:11", "--env", "cube3",
                                            "--results_dir", str(tmp_path), "--nnet_dtype", "fp64", "--eval_all_children"])
    with pytest.raises(ValueError, match="fp64"):
        astar._load_heuristic(args, env_utils.get_environment("cube3"))
