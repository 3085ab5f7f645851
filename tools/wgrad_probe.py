"""The training step's weight gradients, "library" against "f16x3" and "f16" (`ResnetModel.set_wgrad`, `avi.py --wgrad`), the three
modes taking turns in ONE process at the production network (5000 / 1000 / 4 blocks) and batch:

  * per shape of dW (5000 x 324 cube3's fc1, 1000 x 5000 fc2, 1000 x 1000 the blocks' Linears): the library's fp32 GEMM
    dy.t().mm(x) against dca_wgrad_f16 with three products and with one, on planes that exist already — what the step pays, the
    transposes of round 4 gone; the split count S = wgrad_splits(m, n, k), and the device time of the partial-tile kernel and of
    the workspace sum (k_wgrad_fold) separately, from the profiler's kernel records;
  * the whole `train_nnet` step (forward, loss, backward, Adam) per mode, modes alternating round by round: cube3, and puzzle48
    with `--l1_train embed`.  Median, minimum, quartiles and full range of `reps` steps: a mode is ahead when its median beats
    library's by more than twice the spread of library's own steps.
Device-event timings after warm-up.
Usage: python tools/wgrad_probe.py [batch] [reps] > profiles/wgrad_probe.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("library", "f16x3", "f16")


def _time_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_alternating(fns, reps, warm=5):
    """{name: sorted times} with the variants alternating round by round (one process, one clock state)."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_time_once(fn))
    return {k: sorted(v) for k, v in ts.items()}


def _med(v):
    return v[len(v) // 2]


def _stats(v):
    return "%8.3f (min %.3f, quartiles %.3f-%.3f, range %.3f-%.3f)" % (_med(v), v[0], v[len(v) // 4], v[(3 * len(v)) // 4], v[0], v[-1])


def _kernel_times(fn, reps):
    """{kernel name: median device us} of the kernels `fn` launches, from the profiler's records; {} where it has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and "wgrad" in ev.name:
                per.setdefault(ev.name.split("(")[0], []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {k: _med(sorted(v)) for k, v in per.items()}
    except Exception as exc:  # the probe's other figures do not depend on the profiler
        print("    (no kernel records: %s)" % exc)
        return {}


def per_shape(batch, reps):
    from deepcubea_amd import _lib
    print("weight gradient alone, per shape (n x k), batch %d: median ms" % batch)
    for n, k in ((5000, 324), (1000, 5000), (1000, 1000)):
        dy = torch.randn(batch, n, device="cuda") * 1e-3
        x = torch.relu(torch.randn(batch, k, device="cuda"))
        a_dy, a_x = _lib.absmax_bits(dy), _lib.absmax_bits(x)
        dyp = _lib.split_planes_scaled(dy, a_dy, n_pad=(n + 63) // 64 * 64)
        xp = _lib.split_planes_scaled(x, a_x, n_pad=(k + 63) // 64 * 64)
        out = torch.empty((n, k), device="cuda")
        fns = {"library": lambda: torch.mm(dy.t(), x, out=out),
               "f16x3": lambda: _lib.wgrad_f16(dyp, xp, n, k, a_dy, a_x, 3, out=out),
               "f16": lambda: _lib.wgrad_f16(dyp, xp, n, k, a_dy, a_x, 1, out=out)}
        ts = timed_alternating(fns, reps)
        S = _lib.wgrad_splits(batch, n, k)
        print("  %4d x %4d  S = %d, workspace %.1f MB" % (n, k, S, _lib.wgrad_workspace_bytes(batch, n, k) / 1e6))
        for name in MODES:
            print("    %-8s %s   %.0f TFLOP/s of 2 m n k" % (name, _stats(ts[name]), 2.0 * batch * n * k / _med(ts[name]) / 1e9))
        for name in ("f16x3", "f16"):
            kt = _kernel_times(fns[name], 10)
            for kern, us in sorted(kt.items()):
                print("    %-8s kernel %-48s %8.1f us" % (name, kern[:48], us))
        del dy, x, dyp, xp, out
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

    def step(mode):
        def run():
            net.set_wgrad(mode)
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
            loss.backward()
            opt.step()
        return run

    ts = timed_alternating({mode: step(mode) for mode in MODES}, reps)
    lib = ts["library"]
    iqr, full = lib[(3 * len(lib)) // 4] - lib[len(lib) // 4], lib[-1] - lib[0]
    print("%s, l1_train %s: whole training step, batch %d, ms" % (env_name, l1_train, batch))
    for mode in MODES:
        print("  %-8s %s   %.3g samples/s" % (mode, _stats(ts[mode]), batch / _med(ts[mode]) * 1e3))
    print("  library's own spread: quartile range %.3f, full range %.3f" % (iqr, full))
    for mode in ("f16x3", "f16"):
        gain = _med(lib) - _med(ts[mode])
        print("  %-8s ahead of library by %.3f ms = %.1f x the quartile range, %.1f x the full range (%.2fx faster)"
              % (mode, gain, gain / max(iqr, 1e-9), gain / max(full, 1e-9), _med(lib) / _med(ts[mode])))
    del net, opt
    torch.cuda.empty_cache()


def main():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    print("wgrad_probe: batch %d, network 5000/1000/4, %d steps per figure after warm-up, %s" % (batch, reps, torch.cuda.get_device_name()))
    whole_step("cube3", "gemm", batch, reps)
    whole_step("puzzle48", "embed", batch, reps)
    per_shape(batch, reps)


if __name__ == "__main__":
    main()
