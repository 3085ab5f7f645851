"""CPU-side tests of the training step's "embed" layer 1 (`--l1_train`): the ABI additions, `ResnetModel.set_l1_train`'s
refusals and what the switch leaves alone (state dict, the host path), and the driver's flag.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_l1_embed_wgrad_slice_rows", "dca_l1_embed_wgrad_workspace_bytes", "dca_l1_embed_wgrad")
GEOMETRIES = [(54, 6), (16, 16), (25, 25), (36, 36), (49, 49), (49, 6)]


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    # the header states the order rule and the byte guard
    assert "ascending slice order" in hdr and ">= depth contributes NOTHING" in hdr


def test_slice_rows_and_workspace_bytes_are_host_functions_of_the_geometry():
    from deepcubea_amd import _lib
    L = _lib.lib()
    for d, depth in GEOMETRIES:
        S = _lib.l1_embed_wgrad_slice_rows(d, depth)
        assert S >= 0
        for n in (4, 5000):
            ws = lambda m: int(L.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(m), d, depth, C.c_int64(n)))
            if S == 0:
                assert ws(10 ** 6) == 0
                continue
            assert ws(0) == 0 and ws(S) == 0  # one slice goes straight to dW
            assert ws(S + 1) == 2 * (n * d * depth + n) * 4 and ws(3 * S) == 3 * (n * d * depth + n) * 4
    assert int(L.dca_l1_embed_wgrad_slice_rows(5, 5)) == -1 and len(L.dca_last_error()) > 0
    with pytest.raises(_lib.DcaError):
        _lib.l1_embed_wgrad_slice_rows(96, 6)
    assert int(L.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(-1), 16, 16, C.c_int64(8))) == -1


def test_refusals_need_no_device():
    """Every argument check comes before the first device call: DCA_E_BADARG and a message on a box without a GPU, too."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)  # never dereferenced: every call below is refused
    i64 = C.c_int64

    def call(s=one, m=8, d=16, depth=16, dy=one, ld_dy=8, n=8, dw=one, ldw=256, ws=None, wsb=0):
        return L.dca_l1_embed_wgrad(s, i64(m), d, depth, dy, i64(ld_dy), i64(n), dw, i64(ldw), None, ws, i64(wsb), None)

    for kw in (dict(d=5, depth=5), dict(n=6), dict(m=-1), dict(s=None), dict(dy=None), dict(dw=None), dict(dy=C.c_void_p(20)),
               dict(ld_dy=10), dict(ldw=255), dict(ld_dy=4), dict(m=5000), dict(m=5000, ws=one, wsb=15)):
        assert call(**kw) == -1, kw
        assert len(L.dca_last_error()) > 0, kw


def _net(state_dim=16, depth=16, bn=True):
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    torch.manual_seed(0)
    return ResnetModel(state_dim, depth, 24, 16, 1, 1, bn)


def test_set_l1_train_refusals_and_default():
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    net = _net()
    assert net.l1_train == "gemm"
    assert net.set_l1_train("embed") is net and net.l1_train == "embed"
    assert net.set_l1_train("gemm").l1_train == "gemm"
    with pytest.raises(ValueError):
        net.set_l1_train("scatter")
    assert net.l1_train == "gemm"
    with pytest.raises(ValueError):  # no one-hot input
        ResnetModel(16, 0, 24, 16, 1, 1, True).set_l1_train("embed")
    with pytest.raises(ValueError):  # a geometry dca_l1_embed_supported does not name
        _net(10, 3).set_l1_train("embed")
    ResnetModel(16, 0, 24, 16, 1, 1, True).set_l1_train("gemm")  # the default is always accepted


def test_mode_is_no_parameter_or_buffer_and_the_host_path_ignores_it():
    a, b = _net(), _net().set_l1_train("embed")
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [k for k, _ in a.named_buffers()] == [k for k, _ in b.named_buffers()]
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    b.load_state_dict(a.state_dict())
    assert b.l1_train == "embed"
    x = torch.randint(0, 16, (12, 16), dtype=torch.uint8)
    for mode in (True, False):  # training and eval mode on the host: today's code either way
        a.train(mode), b.train(mode)
        ya, yb = a(x), b(x)
        assert torch.equal(ya, yb)
    nobn = _net(bn=False).set_l1_train("embed")  # accepted; without BatchNorm the forward never takes the path
    assert nobn.train()(x).shape == (12, 1)


def test_driver_flag():
    from deepcubea_amd.ctg_approx import avi
    parser = avi.build_parser()
    action = {a.dest: a for a in parser._actions}["l1_train"]
    assert tuple(action.choices) == ("gemm", "embed") and action.default == "gemm"
    base = ["--env", "puzzle15", "--back_max", "10", "--nnet_name", "t"]
    assert parser.parse_args(base).l1_train == "gemm"
    assert parser.parse_args(base + ["--l1_train", "embed"]).l1_train == "embed"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--l1_train", "onehot"])
    assert "embed" in action.help and "gemm" in action.help
