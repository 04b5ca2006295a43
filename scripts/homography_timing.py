"""Times mavba_homography_ransac on the GPU: batches of 1, 64 and 512 image pairs x 100 trials x 1 000 matches, after a
warm-up. Per batch: the median of the launch's device-event time (kernel_seconds of the call), the median wall time of
the whole call (pack, upload, launch, download; it ends in a device synchronise) and, for the first pairs of the batch,
the one-thread host build of the same header (tests/host/h4_math_host.cpp) on the same machine, whose results the
kernel's are compared with.

    python scripts/homography_timing.py [--out profiles/homography_timing.txt] [--reps 30]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mavmap_amd  # noqa: E402
from tests import test_homography_host as T  # noqa: E402

HOST_PAIRS = 8  # the host build runs this many pairs of a batch (one thread: its time per pair does not depend on the batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_timing.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if mavmap_amd.device_count() < 1:
        raise SystemExit("homography_timing: no HIP device - nothing is measured without one")
    keys = ("points2D1", "points2D2", "max_trials", "max_reproj_error", "probability", "stop_num_inliers", "seed")
    lines = ["mavba_homography_ransac, medians over %d calls after %d warm-up calls (1 000 matches per pair, half of the pairs planar, half with"
             % (args.reps, args.warmup),
             "parallax, 30 % outliers, 100 trials, stop at 70 % of the matches, all per-trial outputs downloaded)",
             "%-8s %14s %16s %24s %26s" % ("pairs", "kernel [us]", "whole call [us]", "kernel per pair [us]", "host build per pair [us]")]
    for count in (1, 64, 512):
        items = []
        for q in range(count):
            it = T.make_item(1000, seed=300 + q, kind=("planar", "parallax")[q % 2], max_trials=100)
            it["stop_num_inliers"] = mavmap_amd.view_change_stop(1000, 0.7)
            items.append({k: v for k, v in it.items() if k in keys})
        for _ in range(args.warmup):
            res = mavmap_amd.homography_ransac(items)
        kern, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = mavmap_amd.homography_ransac(items)
            wall.append(time.perf_counter() - t0)
            kern.append(res[0].kernel_seconds)
        sub = items[:HOST_PAIRS]
        cpu = []
        for _ in range(5):
            t0 = time.perf_counter()
            hres = T.host_run(sub)
            cpu.append((time.perf_counter() - t0) / len(sub))
        same = sum(int(r.best_trial == h["best_trial"] and r.trials_used == h["trials_used"] and np.array_equal(r.inlier_mask, h["inlier_mask"])
                       and r.trial_models.tobytes() == h["trial_models"].tobytes()) for r, h in zip(res, hres))
        lines.append("%-8d %14.1f %16.1f %24.2f %26.1f" % (count, 1e6 * np.median(kern), 1e6 * np.median(wall), 1e6 * np.median(kern) / count,
                                                         1e6 * np.median(cpu)))
        lines.append("         best trial, trials used, inlier mask and all 100 models identical to the host build's in %d of the first %d pairs; kept by the gate: %d of %d"
                     % (same, len(sub), len(mavmap_amd.view_change_pairs(items, res, 0.7)), count))
    lines.append("whole call: Python wrapper included; host build: one thread, all 100 trials, the ctypes call of tests/host/h4_math_host.cpp per pair")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
