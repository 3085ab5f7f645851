"""The float64 heuristic mode (`--nnet_dtype fp64`) on the host: the re-layout of `Fp64Resnet` against the reference's float64
evaluation of its weights (tests/golden/nets.npz, make_golden_nets.py), the ABI surface of its kernels, the CLI flag.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_gemm64", "dca_l1_embed64", "dca_head_gemv64")


def _rescaled(net, nets, key):
    """fc_out rescaled exactly as make_golden_nets.py did for the reference's module (float32 arithmetic on both sides)."""
    with torch.no_grad():
        s, t = float(nets[key + "_out_scale"]), float(nets[key + "_out_shift"])
        net.fc_out.weight.copy_((net.fc_out.weight * np.float32(s)).float())
        net.fc_out.bias.copy_((net.fc_out.bias * np.float32(s) + np.float32(t)).float())
    return net.eval()


def trained_magnitude_net(nets, key):
    """The fixture's network: synthetic weights of its seed, fc_out rescaled to trained magnitudes (as test_parity_configs_hip)."""
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    env, seed = key.split("_big_seed")
    D, depth = (54, 6) if env == "cube3" else (49, 49)
    net = ResnetModel(D, depth, 5000, 1000, 4, 1, True)
    load_synthetic_weights(net, int(seed))
    return _rescaled(net, nets, key)


@pytest.mark.parametrize("key", ["cube3_big_seed2028", "cube3_big_seed2029", "cube3_big_seed2030", "puzzle48_big_seed2031"])
def test_fp64_host_path_matches_float64_reference(nets, key):
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet
    torch.set_num_threads(4)
    f = Fp64Resnet(trained_magnitude_net(nets, key))
    x = torch.tensor(nets[key + "_x"])
    y64 = nets[key + "_y64"]
    y = f.forward64(x)[:, 0].numpy()
    assert y.dtype == np.float64
    assert np.max(np.abs(y - y64) / np.maximum(1.0, np.abs(y64))) <= 1e-9
    # forward: the same values rounded once to fp32
    assert np.array_equal(f(x)[:, 0].numpy(), y.astype(np.float32))
    if key.startswith("cube3"):  # the north star's bar at |h| 21-29: 1e-5 ABSOLUTE of the reference's fp32 forward
        assert np.max(np.abs(f(x)[:, 0].numpy().astype(np.float64) - nets[key + "_y32"])) <= 1e-5


def test_fp64_relayout_pads_and_carries_block_bias():
    """The padded float64 layout is the same function as the module, for a small network without BatchNorm too."""
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet, ResnetModel
    torch.manual_seed(3)
    for bn in (True, False):
        m = ResnetModel(16, 16, 64, 32, 2, 1, bn).eval()
        if bn:
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.running_mean.uniform_(-0.5, 0.5)
                    mod.running_var.uniform_(0.5, 2.0)
                    mod.weight.data.uniform_(0.5, 1.5)
                    mod.bias.data.uniform_(-0.2, 0.2)
        f = Fp64Resnet(m)
        assert f.res_pad == 64 and f.weights[0].dtype == torch.float64 and f.uses_l1_kernel
        x = torch.stack([torch.randperm(16) for _ in range(40)]).to(torch.uint8)
        with torch.no_grad():
            oh = torch.nn.functional.one_hot(x.long(), 16).view(40, -1).double()
            ref = m.double().forward_onehot(oh)[:, 0].numpy()
        m.float()
        assert np.max(np.abs(f.forward64(x)[:, 0].numpy() - ref)) <= 1e-12 * max(1.0, float(np.abs(ref).max()))


def test_fp64_symbols_declared_and_exported():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert re.search(r"#define DCA_DT_F64 6\b", hdr) and _lib.DT_F64 == 6
    assert _lib.lib().dca_abi_version() == 6


def test_cli_accepts_fp64():
    from deepcubea_amd.search_methods import astar
    p = astar.build_parser()
    args = p.parse_args(["--states", "s.pkl", "--model_dir", "synthetic:1", "--env", "cube3", "--results_dir", "r",
                         "--nnet_dtype", "fp64"])
    assert args.nnet_dtype == "fp64"
    assert "fp64" in p.format_help()
