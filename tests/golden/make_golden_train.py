#!/usr/bin/env python3
"""Golden fixture for the training step, made by IMPORTING the reference (build container only):

    python tests/golden/make_golden_train.py      -> tests/golden/train_nnet.npz, tests/golden/train_nnet_b256.npz

Calls the reference's own `utils/nnet_utils.py:train_nnet` (Adam, MSE, lr*lr_d^itr, make_batches + shuffle) on
the tiny ResnetModel whose weights are in tiny_resnet.npz, CPU, fixed numpy / random seeds, and records the
inputs, the returned last loss and the final state dict (weights, BN running stats).  Data only.

train_nnet.npz holds the two small cases (batch 16 and 8: every Linear below the 256-row threshold of the device's
hand-written GEMM path).  train_nnet_b256.npz holds one case that reaches it: 64-wide layers, 1024 examples cut into four
batches of 256 and reshuffled once within the six iterations, the reference's default learning-rate decay.  A file whose
arrays come out identical to the ones already on disk is left alone (the zip container carries a time stamp).
"""
import os
import random
import sys

import numpy as np

np.float = float  # noqa: the reference targets numpy 1.22
np.int = int  # noqa

sys.path.insert(0, "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
from utils import nnet_utils  # noqa: E402
from utils.pytorch_models import ResnetModel  # noqa: E402

torch.set_num_threads(1)
tiny = np.load(os.path.join(OUT, "tiny_resnet.npz"))


def write_if_changed(name, arrays):
    path = os.path.join(OUT, name)
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(arrays) and all(
                old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v, equal_nan=True) for k, v in arrays.items()):
            print("%s: unchanged (%d arrays)" % (name, len(arrays)))
            return
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d arrays" % (name, len(arrays)))


files = {"train_nnet.npz": {}, "train_nnet_b256.npz": {}}
for fname, tag, bn, dims, n, bs, itrs, itr0, lr, lr_d in (("train_nnet.npz", "bn", True, (64, 32), 50, 16, 5, 3, 0.01, 0.9),
                                                          ("train_nnet.npz", "nobn", False, (64, 32), 40, 8, 7, 0, 0.005, 0.99),
                                                          ("train_nnet_b256.npz", "b256", True, (64, 64), 1024, 256, 6, 2, 1e-3, 0.9999993)):
    out = files[fname]
    torch.manual_seed(5)
    net = ResnetModel(54, 6, dims[0], dims[1], 2, 1, bn)
    if tag == "bn":
        net.load_state_dict({k[2:]: torch.tensor(tiny[k]) for k in tiny.files if k.startswith("w:")})
    rng = np.random.default_rng(11)
    x = rng.integers(0, 6, size=(n, 54)).astype(np.uint8)
    y = (rng.random((n, 1)) * 10).astype(np.float64)
    for k, v in net.state_dict().items():
        out["%s:init:%s" % (tag, k)] = v.numpy().copy()
    np.random.seed(7)
    random.seed(7)
    last = nnet_utils.train_nnet(net, [x], y, torch.device("cpu"), bs, itrs, itr0, lr, lr_d, display=False)
    out["%s:x" % tag], out["%s:y" % tag] = x, y
    out["%s:args" % tag] = np.array([bs, itrs, itr0, lr, lr_d], np.float64)
    out["%s:last_loss" % tag] = np.array(last, np.float64)
    for k, v in net.state_dict().items():
        out["%s:final:%s" % (tag, k)] = v.numpy().copy()
    print(tag, "last loss", last)
for fname, arrays in files.items():
    write_if_changed(fname, arrays)
