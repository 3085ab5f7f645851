"""The fp64 heuristic mode's forward at the closure's minimum call (131 072 rows), per environment:

  * Fp64Resnet.forward (layer 1 dca_l1_embed64 + dense layers dca_gemm64 + dca_head_gemv) and its parts;
  * the library's float64 path on the same rows: fold_batchnorm(net).double() (and the module itself in float64) through torch,
    one-hot rows built by the library's encoder first (timed apart);
  * the fp32 parity mode (FastResnet) for the ratio;
  * the dense layers' FLOP rate: 2 x rows x (h1_pad x res_pad + 2 x blocks x res_pad^2) over their time.
Medians of device-event timings after warm-up.  Usage: python tools/fp64_forward_probe.py [rows] [reps] [env ...]
"""
import copy
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    from deepcubea_amd import _lib
    from deepcubea_amd.utils.pytorch_models import FastResnet, Fp64Resnet, ResnetModel, fold_batchnorm
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    _lib.require_gpu()
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    envs = sys.argv[3:] or ["cube3", "puzzle48"]
    geo = {"cube3": (54, 6), "puzzle15": (16, 16), "puzzle24": (25, 25), "puzzle35": (36, 36), "puzzle48": (49, 49),
           "lightsout7": (49, 6)}
    print("rows %d, reps %d (median ms)" % (rows, reps))
    for env in envs:
        D, depth = geo[env]
        net = ResnetModel(D, depth, 5000, 1000, 4, 1, True)
        load_synthetic_weights(net, 2028)
        net.eval()
        g = torch.Generator().manual_seed(1)
        if depth == D:
            x = torch.argsort(torch.rand((rows, D), generator=g), dim=1).to(torch.uint8).cuda()
        else:
            x = torch.randint(0, depth, (rows, D), generator=g, dtype=torch.uint8).cuda()
        f = Fp64Resnet(net).cuda()
        W, B = f.weights, f.biases
        t_fwd = timed(lambda: f(x), reps)
        h1 = _lib.l1_embed64(x, depth, f.l1_w_t, f.l1_bias, True)
        t_l1 = timed(lambda: _lib.l1_embed64(x, depth, f.l1_w_t, f.l1_bias, True), reps)

        def dense():
            y = _lib.gemm64(h1, W[0], B[0], None, True)
            for k in range(1, len(W), 2):
                h = _lib.gemm64(y, W[k], B[k], None, True)
                y = _lib.gemm64(h, W[k + 1], None, y, True, out=y)
            return y

        t_dense = timed(dense, reps)
        xr = dense()
        t_head = timed(lambda: _lib.head_gemv(xr, f.w_out, f.b_out), reps)
        t_first = timed(lambda: _lib.gemm64(h1, W[0], B[0], None, True), reps)
        hb = _lib.gemm64(xr, W[1], B[1], None, True)
        t_sq = timed(lambda: _lib.gemm64(xr, W[1], B[1], None, True), reps)
        t_res = timed(lambda: _lib.gemm64(hb, W[2], None, xr.clone(), True), reps)
        del hb
        h1p, rp = W[0].shape[1], W[0].shape[0]
        nblk = (len(W) - 1) // 2
        flop = 2.0 * rows * (h1p * rp + 2 * nblk * rp * rp)
        # the library's float64 path
        enc = lambda: torch.nn.functional.one_hot(x.long(), depth).view(rows, -1).double()  # noqa: E731
        t_enc = timed(enc, reps)
        oh = enc()
        lib64 = fold_batchnorm(net).double().cuda().eval()
        t_lib = timed(lambda: lib64.forward_onehot(oh), reps)
        mod64 = copy.deepcopy(net).double().cuda().eval()
        t_mod = timed(lambda: mod64.forward_onehot(oh), reps)
        del oh, lib64, mod64
        fast = FastResnet(net).cuda()
        t_fp32 = timed(lambda: fast(x), reps)
        y64 = f.forward64(x)[:, 0]
        print("%s: Fp64Resnet.forward %.2f ms = %.1f rows/us | layer 1 (dca_l1_embed64) %.2f ms (%.1f %%) | dense layers %.2f ms = "
              "%.1f TFLOP/s (%.3f TFLOP) | head %.3f ms" % (env, t_fwd, rows / t_fwd / 1e3, t_l1, 100.0 * t_l1 / t_fwd, t_dense,
                                                         flop / t_dense / 1e9, flop / 1e12, t_head))
        print("%s: per layer: %dx%d %.2f ms = %.1f TFLOP/s, %dx%d bias+relu %.2f ms = %.1f TFLOP/s, residual %.2f ms (incl. a skip copy)"
              % (env, h1p, rp, t_first, 2.0 * rows * h1p * rp / t_first / 1e9, rp, rp, t_sq, 2.0 * rows * rp * rp / t_sq / 1e9, t_res))
        print("%s: library float64: fold_batchnorm(net).double() %.2f ms (+ one-hot rows %.2f ms), module .double() %.2f ms | "
              "fp32 parity mode (FastResnet) %.2f ms -> fp64 / fp32 = %.1fx | fp64 / library = %.2fx | max|h| %.2f"
              % (env, t_lib, t_enc, t_mod, t_fp32, t_fwd / t_fp32, t_fwd / (t_lib + t_enc), float(y64.abs().max())))
        sys.stdout.flush()
        del f, fast, h1, xr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("wall %.1f s" % (time.time() - t0))
