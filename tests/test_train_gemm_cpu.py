"""CPU-side tests of the training step's one-product GEMM mode (`--train_gemm f16`, dca_f16_gemm): the ABI additions and their
ctypes signatures, `ResnetModel.set_train_gemm`'s refusals, the driver's flag, DCA_TRAIN_GEMM, the argument checks that come
before any device call, and that the host path never reaches the kernels.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dca_f16_gemm", "dca_cast_planes_scaled", "dca_cast_rows_scaled")
MODES = ("f16x3", "f16")


def _header_names(hdr, fn):
    decl = re.search(r"int %s\((.*?)\);" % fn, hdr, re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    declared = set(re.findall(r"\b(dca_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    doc = hdr[:hdr.index("int dca_f16_gemm(")].rsplit("/*", 1)[1]  # the comment in front of the declaration names the mode for what it is
    assert "NON-parity" in doc and "--train_gemm f16" in doc and "k % 64 == 0" in doc


def test_ctypes_signatures_follow_the_header():
    from deepcubea_amd import _lib
    L = _lib.lib()
    i64, i, p, d = C.c_int64, C.c_int, C.c_void_p, C.c_double
    assert L.dca_f16_gemm.restype is C.c_int and list(L.dca_f16_gemm.argtypes) == [p, i64, i, i64, p, i, i64, p, d, p, p, i64, p]
    assert L.dca_cast_planes_scaled.restype is C.c_int and list(L.dca_cast_planes_scaled.argtypes) == [p, i64, i64, i64, p, p, i64, i64, p]
    assert L.dca_cast_rows_scaled.restype is C.c_int and list(L.dca_cast_rows_scaled.argtypes) == [p, i64, i64, i64, p, i64, i64, p, p, p]
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    assert _header_names(hdr, "dca_f16_gemm") == ["a_h", "m", "k", "lda", "w_h", "n", "ldw", "col_scale", "alpha", "bias", "x_out", "ldo",
                                                  "stream"]
    # the twins' parameter lists without the low plane
    for cast, twin in (("dca_cast_planes_scaled", "dca_split_planes_scaled"), ("dca_cast_rows_scaled", "dca_split_rows_scaled")):
        assert _header_names(hdr, cast) == [a for a in _header_names(hdr, twin) if a != "out_l"]


def test_refusals_need_no_device():
    """Every argument check comes before the first device call: DCA_E_BADARG and a message on a box without a GPU, too."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(64)  # never dereferenced: every call below is refused

    def gemm(a=one, m=8, k=64, lda=64, w=one, n=8, ldw=64, out=one, ldo=8):
        return L.dca_f16_gemm(a, m, k, lda, w, n, ldw, None, 1.0, None, out, ldo, None)

    for kw in (dict(k=96), dict(k=32), dict(k=0), dict(lda=56), dict(lda=68), dict(ldw=56), dict(ldw=68), dict(ldo=4), dict(ldo=10),
               dict(n=0), dict(m=-1), dict(a=None), dict(w=None), dict(out=None), dict(a=C.c_void_p(72)), dict(w=C.c_void_p(66)),
               dict(out=C.c_void_p(68))):
        assert gemm(**kw) == -1, kw
        assert L.dca_last_error().startswith(b"bad argument: "), kw

    def planes(x=one, m=8, n=8, ld=8, out=one, ldo=64, n_pad=64):
        return L.dca_cast_planes_scaled(x, m, n, ld, None, out, ldo, n_pad, None)

    def rows(w=one, n=8, k=8, ld=8, out=one, ldo=64, k_pad=64, cs=one):
        return L.dca_cast_rows_scaled(w, n, k, ld, out, ldo, k_pad, cs, None, None)

    for kw in (dict(x=None), dict(out=None), dict(m=-1), dict(n=0), dict(n=6), dict(ld=4), dict(ld=10), dict(n_pad=4), dict(n_pad=62),
               dict(ldo=60), dict(ldo=66), dict(x=C.c_void_p(72)), dict(out=C.c_void_p(68))):
        assert planes(**kw) == -1, kw
        assert L.dca_last_error().startswith(b"bad argument: "), kw
    for kw in (dict(w=None), dict(out=None), dict(cs=None), dict(n=-1), dict(n=1 << 31), dict(k=0), dict(k=6), dict(ld=4), dict(ld=10),
               dict(k_pad=4), dict(k_pad=62), dict(ldo=60), dict(ldo=66), dict(w=C.c_void_p(72)), dict(out=C.c_void_p(68))):
        assert rows(**kw) == -1, kw
        assert L.dca_last_error().startswith(b"bad argument: "), kw


def test_dense_launchers_refuse_before_the_first_device_call():
    """The dense-layer launchers — dca_f16x3_gemm, dca_f16_gemm, dca_gemm16, dca_gemm8, dca_gemm8_mx — count their tiles in front of
    the first HIP call: arguments that pass every clause but ask for more than 2^31 - 1 workgroups are refused with DCA_E_BADARG and
    "<entry point>: too many tiles", not with whatever the runtime says without a device; and a broken clause is still refused in
    the entry point's own name.  Only where no device is visible: there a regression fails cleanly, on a GPU box it would launch
    on the fake addresses below."""
    if torch.cuda.is_available():
        pytest.skip("what happens before the first device call is told apart only without a device")
    from deepcubea_amd import _lib
    L = _lib.lib()
    a, w = C.c_void_p(1 << 12), C.c_void_p(1 << 13)  # never dereferenced; aligned for every entry point
    far = C.c_void_p(1 << 60)                        # an output far above the operand's extent (m * lda elements from `a`)
    huge = 1 << 40                                   # 2^32 row tiles of 256: one tile column already exceeds the grid

    def f16x3(m=huge, k=64, n=256):
        return L.dca_f16x3_gemm(a, a, m, k, 64, w, w, n, 64, None, 1.0, None, None, 0, None, None, far, 256, None, None)

    def f16(m=huge, k=64, n=256):
        return L.dca_f16_gemm(a, m, k, 64, w, n, 64, None, 1.0, None, far, 256, None)

    def g16(m=huge, k=64, n=256):
        return L.dca_gemm16(a, m, k, 64, w, n, 64, _lib.DT_BF16, None, None, 0, far, 256, None)

    def g8(m=huge, k=128, n=256):
        return L.dca_gemm8(a, m, k, 128, w, n, 128, w, None, None, 0, far, 256, None, 0, 1.0, None)

    def g8mx(m=huge, k=256, n=256):
        return L.dca_gemm8_mx(a, w, m, k, 256, 4, w, n, 256, w, None, None, 0, far, 256, None, 0, None, 0, None)

    calls = {"dca_f16x3_gemm": f16x3, "dca_f16_gemm": f16, "dca_gemm16": g16, "dca_gemm8": g8, "dca_gemm8_mx": g8mx}
    for name, call in calls.items():
        assert call() == -1, name
        assert L.dca_last_error() == b"%s: too many tiles" % name.encode(), (name, L.dca_last_error())
        assert call(m=0) == 0, name  # nothing to do comes before the count, as before
    for name, call in calls.items():  # one broken clause each: k below / off the entry point's K granularity
        assert call(m=8, k=32 if name != "dca_gemm8_mx" else 128) == -1, name
        assert L.dca_last_error().startswith(b"bad argument: %s: " % name.encode()), (name, L.dca_last_error())


def _net():
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    torch.manual_seed(0)
    return ResnetModel(16, 16, 64, 32, 1, 1, True)


def test_set_train_gemm_modes_refusals_and_default():
    from deepcubea_amd import _lib
    net = _net()
    assert net.TRAIN_GEMM_MODES == MODES == _lib.TRAIN_GEMM_MODES
    assert net.train_gemm == ("f16" if os.environ.get("DCA_TRAIN_GEMM") == "f16" else "f16x3")
    for mode in MODES:
        assert net.set_train_gemm(mode) is net and net.train_gemm == mode
    net.set_train_gemm("f16")
    for bad in ("bf16", "library", "", None, "F16"):
        with pytest.raises(ValueError):
            net.set_train_gemm(bad)
        assert net.train_gemm == "f16"  # a refused mode leaves the old one
    lin = torch.nn.Linear(64, 64)
    with pytest.raises(ValueError):
        _lib.linear_train(torch.zeros(4, 64), lin, "library", gemm="bf16")
    assert "parity" in net.set_train_gemm.__doc__ and "parity" in _lib.linear_train.__doc__


def test_state_dict_and_host_path_do_not_know_the_mode():
    """A host forward / backward never reaches the kernels: bit-equal in both modes, and so is the state dict."""
    nets = [_net().set_train_gemm(mode) for mode in MODES]
    x = torch.randint(0, 16, (12, 16), dtype=torch.uint8)
    sds = [net.state_dict() for net in nets]
    assert list(sds[0]) == list(sds[1]) and all(torch.equal(sds[0][key], sds[1][key]) for key in sds[0])
    outs = []
    for net in nets:
        y = net.train()(x)
        y.square().mean().backward()
        outs.append((y.detach(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_default_mode_keeps_the_three_argument_call(monkeypatch):
    """In the default mode the trunk calls linear_train(t, layer, wgrad) — three positional arguments, what the spies of the existing
    tests take; `gemm` is passed, by keyword, in "f16" mode alone."""
    from deepcubea_amd import _lib
    calls = []

    def spy(*args, **kw):
        calls.append((len(args), dict(kw)))
        return torch.nn.functional.linear(args[0], args[1].weight, args[1].bias)

    monkeypatch.setattr(_lib, "linear_train", spy)
    monkeypatch.setattr(_lib, "bn_train", lambda x, bn, relu, skip=None: torch.relu(x if skip is None else x + skip))
    net = _net().train()
    x = torch.rand(8, 256)
    net.set_train_gemm("f16x3")._trunk_train_dev(x)
    assert calls == [(3, {})] * 4
    del calls[:]
    net.set_train_gemm("f16")._trunk_train_dev(x)
    assert calls == [(3, {"gemm": "f16"})] * 4


def test_cli_flag():
    from deepcubea_amd.ctg_approx import avi
    parser = avi.build_parser()
    action = {a.dest: a for a in parser._actions}["train_gemm"]
    assert tuple(action.choices) == MODES and action.default == "f16x3" and not action.required
    assert "NOT a parity mode" in action.help
    base = ["--env", "puzzle15", "--nnet_name", "x", "--back_max", "30"]
    assert parser.parse_args(base).train_gemm == "f16x3"
    assert parser.parse_args(base + ["--train_gemm", "f16"]).train_gemm == "f16"
    assert parser.parse_args(base + ["--train_gemm", "f16x3", "--wgrad", "f16", "--l1_train", "embed"]).train_gemm == "f16x3"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--train_gemm", "bf16"])


def _child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "DCA_TRAIN_GEMM"}
    if env_value is not None:
        env["DCA_TRAIN_GEMM"] = env_value
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from deepcubea_amd import _lib\n"
            "from deepcubea_amd.utils.pytorch_models import ResnetModel\n"
            "print(_lib.TRAIN_GEMM, ResnetModel(16, 16, 64, 32, 1, 1, True).train_gemm, _lib.TRAIN_F16X3)\n" % ROOT)
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_environment_variable_sets_the_initial_mode_in_a_fresh_process():
    """DCA_TRAIN_GEMM is read once, at import: each value gets a fresh child (they run side by side).  Exactly "f16" selects the
    new mode; "library" keeps its meaning; every other value behaves as without the variable."""
    want = {None: "f16x3 f16x3 True", "f16": "f16 f16 True", "f16x3": "f16x3 f16x3 True", "library": "f16x3 f16x3 False",
            "F16": "f16x3 f16x3 True"}
    children = {value: _child(value) for value in want}
    for value, child in children.items():
        out, err = child.communicate(timeout=300)
        assert child.returncode == 0 and out.strip() == want[value], (value, out, err)
