"""CPU-side tests of the training step's weight-gradient modes (`--wgrad`, dca_wgrad_f16): the ABI additions and their ctypes
signatures, the slice rule as a host function of the sizes, `ResnetModel.set_wgrad`'s refusals and what the switch leaves alone,
the driver's flag, DCA_TRAIN_WGRAD, and the argument checks that come before any device call.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_wgrad_f16", "dca_wgrad_splits", "dca_wgrad_workspace_bytes")
MODES = ("library", "f16x3", "f16")
SIZES = [(1, 4, 4), (256, 4, 4), (257, 4, 4), (513, 64, 64), (4096, 4, 4), (300, 132, 68), (777, 256, 512), (1000, 324, 200),
         (10000, 5000, 324), (10000, 1000, 5000), (10000, 1000, 1000), (10000, 1000, 2404)]


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    # the header states the plane convention, the slice rule and the arithmetic
    assert "ascending\n * slice order" in hdr or "ascending slice order" in hdr
    assert "dyh.xh + dyh.xl + dyl.xh" in hdr and "pad64" in hdr and "dca_wgrad_splits(m, n, k)" in hdr


def test_ctypes_signatures():
    from deepcubea_amd import _lib
    L = _lib.lib()
    i64, i, p = C.c_int64, C.c_int, C.c_void_p
    assert L.dca_wgrad_splits.restype is C.c_int and list(L.dca_wgrad_splits.argtypes) == [i64, i, i]
    assert L.dca_wgrad_workspace_bytes.restype is i64 and list(L.dca_wgrad_workspace_bytes.argtypes) == [i64, i, i]
    assert L.dca_wgrad_f16.restype is C.c_int
    assert list(L.dca_wgrad_f16.argtypes) == [p, p, i64, p, p, i64, i64, i, i, p, p, i, p, i64, p, i64, p]
    # the header's parameter list, in order
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    decl = re.search(r"int dca_wgrad_f16\((.*?)\);", hdr, re.S).group(1)
    names = [re.sub(r"/\*.*?\*/", "", a).split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert names == ["dy_h", "dy_l", "ld_dy", "x_h", "x_l", "ld_x", "m", "n", "k", "amax_dy_bits", "amax_x_bits", "products", "dw",
                     "ld_dw", "workspace", "workspace_bytes", "stream"]


def test_splits_and_workspace_are_functions_of_the_sizes():
    from deepcubea_amd import _lib
    seen = set()
    for m, n, k in SIZES:
        S = _lib.wgrad_splits(m, n, k)
        assert S >= 1 and S == _lib.wgrad_splits(m, n, k)  # (no state between calls)
        assert _lib.wgrad_workspace_bytes(m, n, k) == (0 if S == 1 else S * n * k * 4)
        # slices of one length, a multiple of the K-tile (32 rows), none empty: S - 1 full slices leave rows for the last
        rows = -(-m // S)
        rows = -(-rows // 32) * 32
        assert (S - 1) * rows < m <= S * rows
        seen.add(min(S, 3))
    assert seen == {1, 2, 3}
    # a second library handle (no shared Python state) answers the same
    L2 = C.CDLL(_lib.LIB_PATH)
    L2.dca_wgrad_splits.argtypes = [C.c_int64, C.c_int, C.c_int]
    for m, n, k in SIZES:
        assert L2.dca_wgrad_splits(m, n, k) == _lib.wgrad_splits(m, n, k)
    for bad in ((0, 4, 4), (8, 6, 4), (8, 4, 0), (8, -4, 4)):
        with pytest.raises(_lib.DcaError):
            _lib.wgrad_splits(*bad)
        with pytest.raises(_lib.DcaError):
            _lib.wgrad_workspace_bytes(*bad)


def test_refusals_need_no_device():
    """Every argument check comes before the first device call: DCA_E_BADARG and a message on a box without a GPU, too."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(64)  # never dereferenced: every call below is refused

    def call(dyh=one, dyl=one, ld_dy=64, xh=one, xl=one, ld_x=64, m=8, n=8, k=8, products=3, dw=one, ld_dw=8, ws=None, wsb=0):
        return L.dca_wgrad_f16(dyh, dyl, ld_dy, xh, xl, ld_x, m, n, k, None, None, products, dw, ld_dw, ws, wsb, None)

    for kw in (dict(products=2), dict(products=0), dict(n=6), dict(k=0), dict(n=-4), dict(m=0), dict(ld_dy=56), dict(ld_x=8),
               dict(n=68, ld_dy=64), dict(ld_dy=68), dict(ld_x=132), dict(ld_dw=4), dict(dyh=None), dict(xh=None), dict(dw=None),
               dict(dyl=None), dict(xl=None), dict(dyh=C.c_void_p(72)), dict(xl=C.c_void_p(8)), dict(dw=C.c_void_p(66)),
               dict(m=600), dict(m=600, ws=one, wsb=_lib.wgrad_workspace_bytes(600, 8, 8) - 1), dict(m=600, ws=C.c_void_p(66), wsb=1 << 20)):
        assert call(**kw) == -1, kw
        assert len(L.dca_last_error()) > 0, kw


def _net():
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    torch.manual_seed(0)
    return ResnetModel(16, 16, 64, 32, 1, 1, True)


def test_set_wgrad_modes_refusals_and_default():
    from deepcubea_amd import _lib
    net = _net()
    assert net.WGRAD_MODES == MODES == _lib.WGRAD_MODES
    assert net.wgrad == os.environ.get("DCA_TRAIN_WGRAD", "library")  # (the initial mode; "library" unless the variable says otherwise)
    for mode in MODES:
        assert net.set_wgrad(mode) is net and net.wgrad == mode
    net.set_wgrad("f16x3")
    for bad in ("f32", "", None, "F16"):
        with pytest.raises(ValueError):
            net.set_wgrad(bad)
        assert net.wgrad == "f16x3"  # a refused mode leaves the old one
    lin = torch.nn.Linear(64, 64)
    with pytest.raises(ValueError):
        _lib.linear_train(torch.zeros(4, 64), lin, wgrad="bf16")


def test_state_dict_and_host_path_do_not_know_the_mode():
    nets = [_net().set_wgrad(mode) for mode in MODES]
    x = torch.randint(0, 16, (12, 16), dtype=torch.uint8)
    ref_sd = nets[0].state_dict()
    for net in nets[1:]:
        sd = net.state_dict()
        assert list(sd) == list(ref_sd) and all(torch.equal(sd[key], ref_sd[key]) for key in sd)
    ys = [net.train()(x) for net in nets]  # the host goes through nn.Linear in every mode
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_cli_flag():
    from deepcubea_amd.ctg_approx import avi
    parser = avi.build_parser()
    action = {a.dest: a for a in parser._actions}["wgrad"]
    assert tuple(action.choices) == MODES and action.default == "library" and not action.required
    assert "parity" in action.help
    base = ["--env", "puzzle15", "--nnet_name", "x", "--back_max", "30"]
    assert parser.parse_args(base).wgrad == "library"
    for mode in MODES:
        assert parser.parse_args(base + ["--wgrad", mode]).wgrad == mode
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--wgrad", "fp32"])


def _child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "DCA_TRAIN_WGRAD"}
    if env_value is not None:
        env["DCA_TRAIN_WGRAD"] = env_value
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from deepcubea_amd import _lib\n"
            "from deepcubea_amd.utils.pytorch_models import ResnetModel\n"
            "print(_lib.TRAIN_WGRAD, ResnetModel(16, 16, 64, 32, 1, 1, True).wgrad)\n" % ROOT)
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_environment_variable_sets_the_initial_mode_in_a_fresh_process():
    """DCA_TRAIN_WGRAD is read once, at import: each value gets a fresh child (the four run side by side)."""
    values = (None, "f16x3", "f16", "fp32")
    children = [_child(v) for v in values]
    for value, child in zip(values, children):
        out, err = child.communicate(timeout=300)
        if value == "fp32":
            assert child.returncode != 0 and "ValueError" in err and "DCA_TRAIN_WGRAD" in err
        else:
            assert child.returncode == 0 and out.split() == [value or "library"] * 2, err
