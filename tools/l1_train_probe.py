"""The training step's layer 1, "gemm" against "embed" (`ResnetModel.set_l1_train`, `avi.py --l1_train`), both modes back to back
in ONE process, per environment at the production network (5000 / 1000 / 4 blocks) and batch:

  * layer 1 alone, forward + backward: "gemm" = one-hot encoder + fc1 through `_lib.linear_train` (dca_f16x3_gemm where
    in_features % 4 == 0, F.linear otherwise; weight gradient dy^T . x on the library's fp32 GEMM) — the parent's code;
    "embed" = `_lib.l1_embed_train` (dca_l1_embed forward, dca_l1_embed_wgrad backward, the padded W^T copy included);
  * the parts of "embed": the W^T copy, the forward kernel, the scatter (+ fold) kernel;
  * the whole `train_nnet` step (forward, loss, backward, Adam) in either mode, modes alternating round by round.
Device-event timings after warm-up, median (and minimum) of `reps` steps.
Usage: python tools/l1_train_probe.py [batch] [reps] [env ...]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = sorted(_time_once(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts[0]


def timed_alternating(fns, reps, warm=5):
    """{name: (median, min)} with the variants alternating round by round (one process, one clock state)."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_time_once(fn))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


def main():
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    _lib.require_gpu()
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    envs = sys.argv[3:] or ["puzzle15", "puzzle24", "puzzle35", "puzzle48", "cube3"]
    print("l1_train_probe: batch %d, network 5000/1000/4, median (min) ms of %d steps after warm-up, %s"
          % (batch, reps, torch.cuda.get_device_name()))
    for env_name in envs:
        env = env_utils.get_environment(env_name)
        env_id, dim = _lib.env_ids(env_name)[:2]
        states, nb, _ = _lib.generate_states(env_id, dim, batch, 0, 200, 5, 0)
        x = _lib.nnet_input(env_id, dim, states)
        y = nb.float().contiguous()
        net = env.get_nnet_model()
        load_synthetic_weights(net, 2024)
        net = net.cuda().train()
        depth, fc1 = net.one_hot_depth, net.fc1
        n, k = fc1.weight.shape
        dy = torch.randn(batch, n, device="cuda") * 1e-3

        def l1_gemm():
            fc1.zero_grad(set_to_none=True)
            _lib.linear_train(net.encode(x), fc1).backward(dy)

        def l1_embed():
            fc1.zero_grad(set_to_none=True)
            _lib.l1_embed_train(x, fc1, depth).backward(dy)

        n_pad = (n + 63) // 64 * 64
        w_t = torch.empty((k, n_pad), device="cuda")
        b_pad = torch.zeros(n_pad, device="cuda")

        def wt_copy():
            w_t[:, :n].copy_(fc1.weight.detach().t())
            w_t[:, n:].zero_()

        wt_copy()
        parts = {
            "one-hot encoder (gemm mode only)": lambda: net.encode(x),
            "W^T copy [%d, %d]" % (k, n_pad): wt_copy,
            "dca_l1_embed forward": lambda: _lib.l1_embed(x, depth, w_t, b_pad, relu=False),
            "dca_l1_embed_wgrad": lambda: _lib.l1_embed_wgrad(x, dy, depth),
        }
        l1 = timed_alternating({"gemm": l1_gemm, "embed": l1_embed}, reps)

        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def step(mode):
            def run():
                net.set_l1_train(mode)
                opt.zero_grad()
                loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
                loss.backward()
                opt.step()
            return run

        whole = timed_alternating({"gemm": step("gemm"), "embed": step("embed")}, reps)
        print("%s (state_dim %d, depth %d, fc1 %d x %d; slice rows %d)"
              % (env_name, net.state_dim, depth, n, k, _lib.l1_embed_wgrad_slice_rows(net.state_dim, depth)))
        for mode in ("gemm", "embed"):
            print("  layer 1 forward + backward, %-5s  %8.3f (%.3f)" % (mode, *l1[mode]))
        for name, fn in parts.items():
            print("    %-36s %8.3f (%.3f)" % (name, *timed(fn, reps)))
        for mode in ("gemm", "embed"):
            print("  whole training step, %-5s        %8.3f (%.3f)   %.3g samples/s"
                  % (mode, *whole[mode], batch / whole[mode][0] * 1e3))
        print("  embed / gemm: layer 1 %.2fx, whole step %.2fx faster" % (l1["gemm"][0] / l1["embed"][0], whole["gemm"][0] / whole["embed"][0]))
        del net, opt, x, y, dy, w_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
