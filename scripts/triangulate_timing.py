"""Times mavba_triangulate_pairs on the GPU: a batch of 8 image pairs x 4 096 correspondences and a batch of one,
after a warm-up, against the host build of the same header (tests/host/tri_math_host.cpp, one thread) on the same
machine. Per batch: the median of the launch's device-event time (kernel_seconds of the call), the median wall time
of the whole call (pack, upload, launch, download; it ends in a device synchronise) and the host build's median.

    python scripts/triangulate_timing.py [--out profiles/triangulate_timing.txt] [--reps 50]
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
from mavmap_amd import synth  # noqa: E402
from tests import test_triangulate_host as T  # noqa: E402


def make_item(n, seed):
    """A nadir pair (OPENCV / OPENCV, altitude 50, 0.5 px noise): 80 % new points of which a tenth are gross
    mismatches, 20 % continued tracks."""
    rng = np.random.default_rng(seed)
    baseline = rng.uniform(3.0, 20.0)
    rvec1, tvec1, R1 = T._pose(rng, np.array([0.0, 0.0, synth.ALTITUDE]))
    rvec2, tvec2, R2 = T._pose(rng, np.array([baseline, 0.0, synth.ALTITUDE]))
    X = np.stack([rng.uniform(-15, 15, n) + baseline / 2, rng.uniform(-15, 15, n), rng.normal(0, 2.0, n)], axis=1)
    uv1 = synth.project(A.MODEL_OPENCV, synth.OPENCV_PARAMS, X @ R1.T + tvec1) + rng.normal(0, 0.5, (n, 2))
    uv2 = synth.project(A.MODEL_OPENCV, synth.OPENCV_PARAMS, X @ R2.T + tvec2) + rng.normal(0, 0.5, (n, 2))
    bad = rng.random(n) < 0.08
    uv2[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    has = (rng.random(n) < 0.2).astype(np.uint8)
    cp = T._camera_params(A.MODEL_OPENCV, synth.OPENCV_PARAMS)
    return dict(rvec1=rvec1, tvec1=tvec1, rvec2=rvec2, tvec2=tvec2, camera_params1=cp, camera_params2=cp, points2D1=uv1, points2D2=uv2,
                points3D=X + rng.normal(0, 0.02, X.shape), has_point3D=has, reject=A.TRI_REJECT_EXTEND, tri_max_reproj_error=4.0,
                tri_min_angle=2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_timing.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if mavmap_amd.device_count() < 1:
        raise SystemExit("triangulate_timing: no HIP device - nothing is measured without one")
    host = T.load_host()
    lines = ["mavba_triangulate_pairs, medians over %d calls after %d warm-up calls (OPENCV / OPENCV pairs, 4 096 correspondences each)" % (args.reps, args.warmup),
             "%-8s %16s %16s %18s %10s" % ("pairs", "kernel [us]", "whole call [us]", "host build [us]", "accepted")]
    for count in (8, 1):
        items = [make_item(4096, 100 + q) for q in range(count)]
        for _ in range(args.warmup):
            res = mavmap_amd.triangulate_pairs(items)
        kern, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = mavmap_amd.triangulate_pairs(items)
            wall.append(time.perf_counter() - t0)
            kern.append(res[0].kernel_seconds)
        cpu = []
        for _ in range(max(3, args.reps // 5)):
            t0 = time.perf_counter()
            hres = [T.host_pair(host, it) for it in items]
            cpu.append(time.perf_counter() - t0)
        # the two builds keep the same correspondences (a different verdict needs a quantity within rounding of a threshold)
        same = sum(int(np.array_equal(r.accepted, h["accepted"])) for r, h in zip(res, hres))
        lines.append("%-8d %16.1f %16.1f %18.1f %10d" % (count, 1e6 * np.median(kern), 1e6 * np.median(wall), 1e6 * np.median(cpu),
                                                         sum(r.num_accepted for r in res)))
        lines.append("         accepted lists identical to the host build's in %d of %d pairs" % (same, count))
    lines.append("whole call: Python wrapper included; host build: one thread, the ctypes call of tests/host/tri_math_host.cpp per pair")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
