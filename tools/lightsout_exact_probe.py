"""The exact LightsOut heuristic on the MI355X, measured once -> profiles/lightsout_exact_probe.txt.

    python tools/lightsout_exact_probe.py [rows=1048576] [out=profiles/lightsout_exact_probe.txt] [window_s=0.3]

dca_lightsout_exact_eval and dca_lightsout_exact_solve at `rows` random 0/1 rows, for ld = 49 (rows back to back: byte loads) and
ld = 64 (word loads), and again at 8 * `rows` (rows that do not fit the 256 MiB Infinity Cache, and a kernel long enough that
the host's enqueue rate cannot bound the figure).  Per leg: 5 warm-up calls, 50 timed calls to size the window, then device
events around as many back-to-back calls as fill about `window_s` seconds; the host clock around the same loop (before the
synchronise) is the enqueue time per call — where it is close to the device time the leg measures the host, not the kernel.
Bytes read = rows * 49 (the bytes a row needs), bytes written = rows * 4 (eval)
or rows * 8 (solve); the rate is set against the 8 TB/s HBM peak DESIGN quotes.  A record, not a gate: nothing is asserted."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepcubea_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12


def leg(name, fn, view, out, window_s):
    for _ in range(5):
        fn(view, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        fn(view, out=out)
    b.record()
    b.synchronize()
    reps = max(10, int(window_s / max(a.elapsed_time(b) * 1e-3 / 50, 1e-7)))
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn(view, out=out)
    b.record()
    host = (time.perf_counter() - t0) / reps
    b.synchronize()
    return reps, a.elapsed_time(b) * 1e-3 / reps, host


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lightsout_exact_probe.txt")
    window_s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3
    _lib.require_gpu()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("lightsout_exact_probe: %s, random 0/1 cells (numpy default_rng(0)), device events around back-to-back calls filling about "
        "%.2f s after 5 warm-up and 50 sizing calls" % (torch.cuda.get_device_name(0), window_s))
    say("bytes read = rows * 49, bytes written = rows * 4 (eval) or rows * 8 (solve); peak = the 8 TB/s HBM figure of DESIGN")
    for rows in (rows, 8 * rows):
        measure(rows, window_s, say)
    say("%d rows (51-67 MB a leg) fit the 256 MiB Infinity Cache and every call reads the same rows: there the read rate is what the "
        "kernel sustains from wherever the rows sit, NOT an HBM rate; %d rows (411-537 MB) do not fit.  No counter run was made"
        % (rows // 8, rows))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def measure(rows, window_s, say):
    X = torch.from_numpy(np.random.default_rng(0).integers(0, 2, (rows, 49), dtype=np.uint8)).cuda()
    for ld in (49, 64):
        buf = torch.zeros((rows, ld), dtype=torch.uint8, device="cuda")
        view = buf[:, :49]
        view.copy_(X)
        for name, fn, dtype, width in (("eval", _lib.lightsout_exact_eval, torch.float32, 4),
                                       ("solve", _lib.lightsout_exact_solve, torch.int64, 8)):
            out = torch.empty(rows, dtype=dtype, device="cuda")
            reps, t, host = leg(name, fn, view, out, window_s)
            say("%8d rows  %-5s ld %2d (%s loads)  %5d calls  %8.2f us / call (host enqueue %6.2f us)  %.3g rows/s  read %.3g B/s = %.3f of "
                "peak  (read + write %.3g B/s; row footprint ld * rows = %.1f MB)"
                % (rows, name, ld, "word" if ld % 4 == 0 else "byte", reps, t * 1e6, host * 1e6, rows / t, rows * 49 / t,
                   rows * 49 / t / HBM_PEAK, rows * (49 + width) / t, rows * ld / 1e6))


if __name__ == "__main__":
    main()
