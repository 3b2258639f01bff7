#!/usr/bin/env python3
"""Context.register_batch_global on N copies of the dense bunny pair (every 6th point of the bunny from 0, turned 149 degrees about
(1, 2, 3) and shifted, against every 6th from 3: 5 992 x 5 991 points, fp32), without and with keypoints=rule (ISS: 7 mm, 5.25 mm,
0.975, 0.975, 5): wall time of the call, and the start and end poses against the truth.  The call runs twice in the process on
the same batch -- the first is the warm-up -- so under `rocprofv3 --kernel-trace --stats -d DIR --` every kernel's launches have
one shape (tools/prof_summary.py DIR).

    python tools/keypoint_time.py [N = 1] [keypoints = 0 | 1] [hypotheses = 2000]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (torch's HIP runtime first, as in tests/conftest.py)
except Exception:
    pass
from __graft_entry__ import load_package  # noqa: E402


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def angle_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    use = bool(int(sys.argv[2])) if len(sys.argv) > 2 else False
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    pkg = load_package()
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::6], np.ascontiguousarray(B[3::6])
    R, t = rodrigues((1.0, 2.0, 3.0), 149.0), np.array([0.05, -0.03, 0.08])
    moving = np.ascontiguousarray((src.astype(np.float64) @ R.T + t).astype(np.float32))
    Rt, tt = R.T, -R.T @ t
    pairs = [(moving, model)] * N
    K, MD, GATE = 24, 0.0075, 0.01
    more = dict(keypoints=(0.007, 0.00525, 0.975, 0.975, 5)) if use else {}
    with pkg.Context(0) as ctx:
        ctx.register_batch_global(pairs, 0.0, K, H, MD, seed=1, gate=GATE, **more)   # (warm-up: code objects, allocations)
        t0 = time.perf_counter()
        out = ctx.register_batch_global(pairs, 0.0, K, H, MD, seed=1, gate=GATE, **more)
        wall = time.perf_counter() - t0
    g = out[0].extra["global"]
    err = lambda T: (angle_deg(T[:3, :3] @ Rt.T), float(np.linalg.norm(T[:3, 3] - tt)) * 1e3)
    same = all(np.array_equal(r.T, out[0].T) and np.array_equal(r.extra["global"]["T"], g["T"]) for r in out)
    print(f"{N} pair(s) of {moving.shape[0]} x {model.shape[0]} points, {H} hypotheses, keypoints {'on' if use else 'off'}"
          f"{' ' + str(g['keypoints']) if use else ''}: register_batch_global {wall * 1e3:.1f} ms (host wall, the numpy normals included)")
    print(f"correspondences {g['correspondences']} inliers {g['inliers']}; start pose {err(g['T'])[0]:.3f} deg {err(g['T'])[1]:.2f} mm; "
          f"end pose {err(out[0].T)[0]:.3f} deg {err(out[0].T)[1]:.2f} mm; every pair of the batch the same bytes: {same}")


if __name__ == "__main__":
    main()
