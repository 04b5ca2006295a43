"""Times mavba_relative_pose_ransac on the GPU: a batch of 8 image pairs x 1000 trials x 1 024 matches and a batch of
one, after a warm-up, against the host build of the same header (tests/host/e5_math_host.cpp, one thread) on the same
machine. Per batch: the median of the launch's device-event time (kernel_seconds of the call), the median wall time
of the whole call (lift, pack, upload, launch, download; it ends in a device synchronise) and the host build's median
for all 1000 trials, and for the trials a sequential run would have used before its dynamic limit ended it.

    python scripts/relative_pose_timing.py [--out profiles/relative_pose_timing.txt] [--reps 50]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mavmap_amd  # noqa: E402
from mavmap_amd import _abi as A  # noqa: E402
from tests import test_relative_pose_host as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative_pose_timing.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if mavmap_amd.device_count() < 1:
        raise SystemExit("relative_pose_timing: no HIP device - nothing is measured without one")
    keys = ("camera_params1", "camera_params2", "points2D1", "points2D2", "max_trials", "max_reproj_error", "probability", "stop_num_inliers", "seed")
    lines = ["mavba_relative_pose_ransac, medians over %d calls after %d warm-up calls (OPENCV cameras, 1 024 matches, 30 %% outliers, 1000 trials)"
             % (args.reps, args.warmup),
             "%-8s %14s %16s %23s %26s %12s" % ("pairs", "kernel [us]", "whole call [us]", "host, 1000 trials [us]", "host, trials used only [us]", "trials used")]
    for count in (8, 1):
        items = [{k: v for k, v in T.make_item(1024, A.MODEL_OPENCV, A.MODEL_OPENCV, seed=200 + q, max_trials=1000).items() if k in keys} for q in range(count)]
        for _ in range(args.warmup):
            res = mavmap_amd.relative_pose_ransac(items)
        kern, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = mavmap_amd.relative_pose_ransac(items)
            wall.append(time.perf_counter() - t0)
            kern.append(res[0].kernel_seconds)
        short = [dict(it, max_trials=r.trials_used) for it, r in zip(items, res)]
        cpu, cpu_short = [], []
        for _ in range(max(3, args.reps // 10)):
            t0 = time.perf_counter()
            hres = T.host_run(items)
            cpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            T.host_run(short)
            cpu_short.append(time.perf_counter() - t0)
        same = sum(int((r.best_trial, r.best_model) == (h["best_trial"], h["best_model"]) and np.array_equal(r.inlier_mask, h["inlier_mask"])
                       and r.trial_models.tobytes() == h["trial_models"].tobytes() and np.array_equal(r.R, h["R"])) for r, h in zip(res, hres))
        models = sum(int(r.trial_num_models.sum()) for r in res)
        lines.append("%-8d %14.1f %16.1f %23.1f %26.1f %12s" % (count, 1e6 * np.median(kern), 1e6 * np.median(wall), 1e6 * np.median(cpu),
                                                               1e6 * np.median(cpu_short), "/".join(str(r.trials_used) for r in res)))
        lines.append("         %d models scored; best model, inlier mask, R and all models identical to the host build's in %d of %d pairs" % (models, same, count))
    lines.append("whole call: Python wrapper included; host build: one thread, the ctypes call of tests/host/e5_math_host.cpp per pair")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
