"""The training step's forward / input-gradient GEMMs, "f16x3" (dca_f16x3_gemm: three products on two fp16 planes, fp32-accurate)
against "f16" (dca_f16_gemm: the high planes alone, NON-parity) — `ResnetModel.set_train_gemm`, `avi.py --train_gemm` — the modes
taking turns in ONE process at the production network (5000 / 1000 / 4 blocks) and batch:

  * per shape (k -> n): forward 324 -> 5000, 5000 -> 1000, 1000 -> 1000 and the input-gradient shapes 1000 -> 5000, 1000 -> 1000:
    the GEMM alone on operands that exist, the operand preparation alone (absmax + activation split / cast + row split / cast),
    and both together — what the step pays per layer;
  * the whole `train_nnet` step (forward, loss, backward, Adam) for (f16x3, f16) x wgrad (library, f16), the four alternating round
    by round: cube3, and puzzle48 with `--l1_train embed`.  Median, minimum, quartiles and full range of `reps` steps: f16 is ahead
    when its median beats f16x3's (same wgrad) by more than twice the quartile range of f16x3's own steps.
Device-event timings after warm-up.
Usage: python tools/train_gemm_probe.py [batch] [reps] > profiles/train_gemm_probe.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from wgrad_probe import _med, _stats, timed_alternating  # noqa: E402

MODES = ("f16x3", "f16")


def per_shape(batch, reps):
    from deepcubea_amd import _lib
    print("forward / input-gradient GEMM alone, per shape (k -> n), batch %d: median ms" % batch)
    for what, k, n in (("forward", 324, 5000), ("forward", 5000, 1000), ("forward", 1000, 1000), ("input gradient", 1000, 5000),
                       ("input gradient", 1000, 1000)):
        a = torch.relu(torch.randn(batch, k, device="cuda"))
        w = torch.randn(n, k, device="cuda") / k ** 0.5
        bias = torch.randn(n, device="cuda") if what == "forward" else None
        kp = (k + 63) // 64 * 64
        amax = _lib.absmax_bits(a)
        ap = _lib.split_planes_scaled(a, amax, n_pad=kp)
        wp, cs = _lib.split_rows_scaled(w, amax, k_pad=kp)
        ah = _lib.cast_planes_scaled(a, amax, n_pad=kp)
        wh, cs1 = _lib.cast_rows_scaled(w, amax, k_pad=kp)

        def prep3():
            am = _lib.absmax_bits(a, out=amax)
            _lib.split_planes_scaled(a, am, n_pad=kp, out=ap)
            _lib.split_rows_scaled(w, am, k_pad=kp, out=wp, col_scale=cs)

        def prep1():
            am = _lib.absmax_bits(a, out=amax)
            _lib.cast_planes_scaled(a, am, n_pad=kp, out=ah)
            _lib.cast_rows_scaled(w, am, k_pad=kp, out=wh, col_scale=cs1)

        def gemm3():
            _lib.f16x3_gemm(ap, wp[0], wp[1], cs, 1.0, bias, None, False, False, True)

        def gemm1():
            _lib.f16_gemm(ah[0], wh[0], cs1, 1.0, bias)

        ts = timed_alternating({"prep f16x3": prep3, "prep f16": prep1, "gemm f16x3": gemm3, "gemm f16": gemm1,
                                "both f16x3": lambda: (prep3(), gemm3()), "both f16": lambda: (prep1(), gemm1())}, reps)
        print("  %-14s %4d -> %4d" % (what, k, n))
        for name, v in ts.items():
            rate = "   %.0f TFLOP/s of 2 m n k" % (2.0 * batch * n * k / _med(v) / 1e9) if name.startswith("gemm") else ""
            print("    %-11s %s%s" % (name, _stats(v), rate))
        del a, w, ap, wp, ah, wh
        torch.cuda.empty_cache()


def whole_step(env_name, l1_train, batch, reps):
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    env = env_utils.get_environment(env_name)
    env_id, dim = _lib.env_ids(env_name)[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, batch, 0, 200, 5, 0)
    x = _lib.nnet_input(env_id, dim, states)
    y = nb.float().contiguous()
    net = env.get_nnet_model()
    load_synthetic_weights(net, 2024)
    net = net.cuda().train().set_l1_train(l1_train)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)

    def step(gemm, wgrad):
        def run():
            net.set_train_gemm(gemm).set_wgrad(wgrad)
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
            loss.backward()
            opt.step()
        return run

    ts = timed_alternating({(gemm, wgrad): step(gemm, wgrad) for wgrad in ("library", "f16") for gemm in MODES}, reps)
    print("%s, l1_train %s: whole training step, batch %d, ms" % (env_name, l1_train, batch))
    for wgrad in ("library", "f16"):
        base, ours = ts[("f16x3", wgrad)], ts[("f16", wgrad)]
        iqr, full = base[(3 * len(base)) // 4] - base[len(base) // 4], base[-1] - base[0]
        for gemm in MODES:
            v = ts[(gemm, wgrad)]
            print("  train_gemm %-6s wgrad %-8s %s   %.3g samples/s" % (gemm, wgrad, _stats(v), batch / _med(v) * 1e3))
        gain = _med(base) - _med(ours)
        print("  wgrad %-8s f16x3's own spread: quartile range %.3f, full range %.3f; f16 ahead of f16x3 by %.3f ms = %.1f x the "
              "quartile range (%.2fx faster): %s" % (wgrad, iqr, full, gain, gain / max(iqr, 1e-9), _med(base) / _med(ours),
                                                     "AHEAD" if gain > 2.0 * iqr else "NOT ahead"))
    del net, opt
    torch.cuda.empty_cache()


def main():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    print("train_gemm_probe: batch %d, network 5000/1000/4, %d steps per figure after warm-up, %s"
          % (batch, reps, torch.cuda.get_device_name()))
    whole_step("cube3", "gemm", batch, reps)
    whole_step("puzzle48", "embed", batch, reps)
    per_shape(batch, reps)


if __name__ == "__main__":
    main()
