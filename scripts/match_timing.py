"""Times mavba_match_descriptors on the GPU: batches of 1, 16 and 128 image pairs of 2 000 x 2 000 keypoints at dim 128,
and one batch at dim 64, after a warm-up. Per batch: the median of the two launches' device-event time (kernel_seconds
of the call), the median wall time of the whole call (pack, upload, launches, download, scatter, the host's medians),
the algorithmic rate 2 * 2 * n1 * n2 * dim / kernel time beside the 157 TFLOP/s f32 matrix peak of the MI355X, and the
one-thread host build of the same header (tests/host/match_math_host.cpp) on a 500 x 500 slice of a pair, scaled by the
number of keypoint pairs and labelled as scaled.

    python scripts/match_timing.py [--out profiles/match_timing.txt] [--reps 30]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mavmap_amd  # noqa: E402
from tests import test_match_host as T  # noqa: E402

N = 2000
HOST_N = 500
DISTINCT = 8  # a batch repeats this many generated pairs (the kernel's time does not depend on the data)
PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_timing.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if mavmap_amd.device_count() < 1:
        raise SystemExit("match_timing: no HIP device - nothing is measured without one")
    lines = ["mavba_match_descriptors, medians over %d calls after %d warm-up calls (%d x %d keypoints per pair, max_ratio 0.9, no spatial mask,"
             % (args.reps, args.warmup, N, N),
             "every output downloaded; a batch repeats %d generated pairs)" % DISTINCT,
             "%-6s %-5s %13s %16s %21s %16s %32s" % ("pairs", "dim", "kernel [us]", "whole call [us]", "kernel per pair [us]", "rate [TFLOP/s]",
                                                      "host build per pair [us], scaled")]
    for count, dim in ((1, 128), (16, 128), (128, 128), (16, 64)):
        pool = [T.make_item(N, N, dim, 500 + q) for q in range(min(count, DISTINCT))]
        items = [pool[q % len(pool)] for q in range(count)]
        for _ in range(args.warmup):
            res = mavmap_amd.match_descriptors(items)
        kern, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = mavmap_amd.match_descriptors(items)
            wall.append(time.perf_counter() - t0)
            kern.append(res[0].kernel_seconds)
        sub = dict(pool[0], descriptors1=pool[0]["descriptors1"][:HOST_N].copy(), descriptors2=pool[0]["descriptors2"][:HOST_N].copy(),
                   keypoints1=pool[0]["keypoints1"][:HOST_N].copy(), keypoints2=pool[0]["keypoints2"][:HOST_N].copy())
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            hres = T.host_run([sub])
            cpu.append(time.perf_counter() - t0)
        gres = mavmap_amd.match_descriptors([sub])[0]
        same = gres.num_matches == hres[0]["num_matches"] and np.array_equal(gres.matches, hres[0]["matches"][:gres.num_matches])
        k = float(np.median(kern))
        lines.append("%-6d %-5d %13.1f %16.1f %21.2f %16.2f %32.0f" % (count, dim, 1e6 * k, 1e6 * np.median(wall), 1e6 * k / count,
                                                                     4.0 * N * N * dim * count / k / 1e12, 1e6 * np.median(cpu) * (N / HOST_N) ** 2))
        lines.append("       matches per pair: %d of %d keypoints; the %d x %d slice's matches identical to the host build's: %s"
                     % (res[0].num_matches, N, HOST_N, HOST_N, "yes" if same else "NO"))
    lines.append("rate: both directions, 2 * 2 * n1 * n2 * dim flop per pair, against a matrix peak of %.1f TFLOP/s (f32 inputs)" % PEAK_TFLOPS)
    lines.append("whole call: Python wrapper included; host build: one thread, exhaustive, a %d x %d slice timed and multiplied by %d"
                 % (HOST_N, HOST_N, (N // HOST_N) ** 2))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
