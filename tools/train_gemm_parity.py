"""How far the NON-parity GEMM mode of the training step (`--train_gemm f16`: forward and input gradient on the high fp16 planes
alone) sits from the same step in float64, next to the default f16x3 step as the yardstick.  No tolerance for a whole step can
be derived through ten BatchNorms, so this tool MEASURES the two metrics tests/test_train_gemm_hip.py asserts against, on
ResnetModel(16, 16, 256, 128, 2 blocks) and 512 puzzle15 states:

  * one forward + backward, network seeds 11, 12, 13: |loss - loss64| / |loss64|, and per parameter max |g - g64| / max |g64|
    (its worst over the parameters whose gradient is not analytically zero; the Linear biases in front of a BatchNorm are reported
    as the largest |g| over the default step's);
  * 60 Adam steps of batch 256 from identical weights and batches, batch seeds 1-5: final loss of the f16 run over the f16x3 run's.

The functions here are the ones the tests call: the table and the assertions cannot drift apart.
Usage: python tools/train_gemm_parity.py > profiles/train_gemm_parity.txt
"""
import os
import random
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOISE = re.compile(r"(fc1|fc2|blocks\.\d\.[02])\.bias")  # a Linear bias in front of a BatchNorm: analytically zero gradient
NET_SEEDS = (11, 12, 13)
RUN_SEEDS = (1, 2, 3, 4, 5)


def small_net(seed=11):
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    torch.manual_seed(seed)
    return ResnetModel(16, 16, 256, 128, 2, 1, True)  # puzzle15's input, h1 256, residual width 128, 2 blocks


def small_data():
    """(uint8 network input [512, 16], targets [512]) of 512 puzzle15 states: the construction of tests/test_wgrad_hip.py."""
    from deepcubea_amd import _lib
    env_id, dim = _lib.env_ids("puzzle15")[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, 512, 0, 30, 5, 0)
    return _lib.nnet_input(env_id, dim, states), nb.float().contiguous()


def step(x, y, sd, train_gemm, wgrad="library"):
    """One forward + backward from the state dict `sd` -> (loss, {param: grad float64 on the host}, net); train_gemm "float64": the
    same step in double precision on the library's kernels."""
    net = small_net()
    net.load_state_dict(sd)
    net = net.cuda().train()
    if train_gemm == "float64":
        net = net.double()
        onehot = torch.nn.functional.one_hot(x.long(), 16).view(x.shape[0], -1).double()
        loss = torch.nn.functional.mse_loss(net.trunk(onehot)[:, 0], y.double())
    else:
        net.set_train_gemm(train_gemm).set_wgrad(wgrad)
        loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
    loss.backward()
    return float(loss.detach().double()), {k: p.grad.double().cpu() for k, p in net.named_parameters()}, net


def rel(a, ref):
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def step_metrics(x, y, seed, train_gemm, wgrad, ref=None, base=None):
    """{"loss": relative loss difference to float64, "grad": worst rel() over the parameters with a real gradient, "which": that
    parameter, "noise": largest zero-gradient |g| over the default step's, "per": {param: rel()}} of one step at network `seed`.
    ref / base: the float64 step and the default (f16x3, library) step of the same seed, where the caller has them."""
    sd = small_net(seed).state_dict()
    l64, g64, _ = ref if ref is not None else step(x, y, sd, "float64")
    _, g_base, _ = base if base is not None else step(x, y, sd, "f16x3", "library")
    loss, grads, _ = step(x, y, sd, train_gemm, wgrad)
    per = {k: rel(grads[k], g64[k]) for k in g64 if not NOISE.fullmatch(k)}
    which = max(per, key=per.get)
    noise = max(float(grads[k].abs().max()) / max(float(g_base[k].abs().max()), 1e-300) for k in g64 if NOISE.fullmatch(k))
    finite = all(bool(torch.isfinite(g).all()) for g in grads.values())
    return {"loss": abs(loss - l64) / abs(l64), "grad": per[which], "which": which, "noise": noise, "per": per, "finite": finite}


def short_run(x, y, sd, train_gemm, seed, steps=60, wgrad="library"):
    """Final loss of `steps` Adam iterations of batch 256 from `sd`, batches drawn with `seed`."""
    from deepcubea_amd.utils import nnet_utils
    net = small_net()
    net.load_state_dict(sd)
    net = net.cuda().set_train_gemm(train_gemm).set_wgrad(wgrad)
    np.random.seed(seed)
    random.seed(seed)
    return nnet_utils.train_nnet(net, x, y.view(-1, 1), torch.device("cuda"), 256, steps, 0, 1e-3, 0.9999993, display=False)


def short_run_ratio(x, y, sd, seed, steps=60):
    base, ours = short_run(x, y, sd, "f16x3", seed, steps), short_run(x, y, sd, "f16", seed, steps)
    return ours / base, ours, base


def main():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, y = small_data()
    print("train_gemm_parity: ResnetModel(16, 16, 256, 128, 2 blocks), 512 puzzle15 states, %s" % torch.cuda.get_device_name())
    print("one step against float64: loss = |loss - loss64| / |loss64|; grad = worst max|g - g64| / max|g64| over the parameters;")
    print("noise = largest zero-gradient |g| over the default step's")
    worst = {}
    for seed in NET_SEEDS:
        sd = small_net(seed).state_dict()
        ref, base = step(x, y, sd, "float64"), step(x, y, sd, "f16x3", "library")
        for gemm, wgrad in (("f16x3", "library"), ("f16", "library"), ("f16", "f16x3"), ("f16", "f16")):
            mt = step_metrics(x, y, seed, gemm, wgrad, ref, base)
            print("  seed %d  train_gemm %-6s wgrad %-8s loss %.3e  grad %.3e (%s)  noise %.3g  finite %s"
                  % (seed, gemm, wgrad, mt["loss"], mt["grad"], mt["which"], mt["noise"], mt["finite"]))
            w = worst.setdefault((gemm, wgrad), {"loss": 0.0, "grad": 0.0, "noise": 0.0})
            for key in w:
                w[key] = max(w[key], mt[key])
    for (gemm, wgrad), w in worst.items():
        print("  worst of %d seeds  train_gemm %-6s wgrad %-8s loss %.3e  grad %.3e  noise %.3g" % (len(NET_SEEDS), gemm, wgrad, w["loss"],
                                                                                               w["grad"], w["noise"]))
    print("60 Adam steps of batch 256 from the seed-11 weights: final loss, f16 over f16x3")
    sd = small_net(11).state_dict()
    ratios = []
    for seed in RUN_SEEDS:
        ratio, ours, base = short_run_ratio(x, y, sd, seed)
        ratios.append(ratio)
        print("  batch seed %d  f16 %.6f  f16x3 %.6f  ratio %.4f" % (seed, ours, base, ratio))
    print("  worst ratio of %d seeds %.4f" % (len(RUN_SEEDS), max(ratios)))


if __name__ == "__main__":
    main()
