"""The AVI update step with the heuristic cache off and on (`Updater(..., cache=...)`, DCA_UPDATE_CACHE / `--update_cache`),
alternating in ONE process: per environment (cube3, puzzle15), network mode (the fp32 parity mode, bf16) and size (200 000 and
2 000 000 states in 100 000-state batches, the batch `avi.py` and `bench.py` use) it prints the network rows evaluated / rows,
ms per update for both (median and the spread of the repeats) and whether the training triple was bit-equal.

    python tools/update_cache_probe.py [repeats=5] [envs=cube3,puzzle15] [sizes=200000,2000000] > profiles/update_cache_probe.txt

The claim it checks: cache on is ahead of cache off by more than twice the spread of the off runs.  bf16 is NOT a
batch-invariant mode: its line reports whether the outputs happened to be bit-equal, nothing rests on it."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepcubea_amd.updaters.updater import Updater  # noqa: E402
from deepcubea_amd.utils import env_utils, nnet_utils  # noqa: E402
from deepcubea_amd.utils.pytorch_models import FastResnet  # noqa: E402
from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights  # noqa: E402

BACK_MAX = {"cube3": 30, "puzzle15": 500}  # the values of the reference's train.sh


def one_update(env, n, hfn, oh, cache, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    upd = Updater(env, n, BACK_MAX[env.env_name], hfn, 1, update_batch_size=100_000, seed=seed, onehot_dtype=oh, cache=cache)
    out = upd.update_dev()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out, upd


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    envs = (sys.argv[2] if len(sys.argv) > 2 else "cube3,puzzle15").split(",")
    sizes = [int(s) for s in (sys.argv[3] if len(sys.argv) > 3 else "200000,2000000").split(",")]
    print("update step, heuristic cache off vs auto, alternating in one process; %d repeats each; %s" % (
        repeats, torch.cuda.get_device_name(0)))
    print("%-9s %-5s %9s | %12s %9s | %25s | %25s | %7s %7s | %s" % (
        "env", "mode", "states", "eval/rows", "slots", "off ms med (min..max)", "on ms med (min..max)", "gain", "2xsprd", "bit-equal"))
    for env_name in envs:
        env = env_utils.get_environment(env_name)
        model = env.get_nnet_model()
        load_synthetic_weights(model, 2024)
        for mode, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            fast = FastResnet(model, dt).cuda()
            hfn = nnet_utils.get_heuristic_fn_dev(fast, clip_zero=False, batch_size=131072)
            oh = None if fast.uses_l1_kernel else fast.onehot_dtype
            for n in sizes:
                one_update(env, min(n, 200_000), hfn, oh, "off", 1)  # warm-up: allocator, kernels
                one_update(env, min(n, 200_000), hfn, oh, "auto", 1)
                off_ms, on_ms, equal, frac, slots = [], [], True, None, None
                for r in range(repeats):
                    t_off, want, _ = one_update(env, n, hfn, oh, "off", 100 + r)
                    t_on, got, upd = one_update(env, n, hfn, oh, "auto", 100 + r)
                    off_ms.append(t_off)
                    on_ms.append(t_on)
                    equal = equal and all(torch.equal(a, b) for a, b in zip(want, got)) and torch.equal(
                        want[1].view(torch.int32), got[1].view(torch.int32))
                    c = upd.cache_counters()
                    frac = (c["evaluated"] / max(c["rows"], 1), c["uncached"]) if c else (1.0, 0)
                    slots = upd.cached_fn.cache.slots if upd.cached_fn is not None else 0
                    del want, got, upd
                m_off, m_on = statistics.median(off_ms), statistics.median(on_ms)
                spread = max(off_ms) - min(off_ms)
                print("%-9s %-5s %9d | %6.4f (%d unc) %9d | %8.1f (%7.1f..%7.1f) | %8.1f (%7.1f..%7.1f) | %+6.1f%% %6.1f%% | %s" % (
                    env_name, mode, n, frac[0], frac[1], slots, m_off, min(off_ms), max(off_ms), m_on, min(on_ms), max(on_ms),
                    100.0 * (m_off - m_on) / m_off, 100.0 * 2 * spread / m_off, "yes" if equal else "NO"), flush=True)
            del fast, hfn
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
