#!/usr/bin/env python3
"""Context.register_batch_global over N bunny-sized pairs in unknown relative pose (tools/global_time.py's pairs: every 24th point of
the bunny against the points between them, each pair turned by an angle of its own) with device_normals off and on, alternated in
one process: the median and the span of the call's host wall over RUNS runs of each after a warm-up of each, the stage walls of
both routes, and the pose errors of both.  Run it under `rocprofv3 --kernel-trace --stats -d DIR --` for the per-launch times
(tools/prof_summary.py DIR).

    python tools/normals_time.py [N = 64] [runs = 10] [hypotheses = 2000]
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


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    pkg = load_package()
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::24], np.ascontiguousarray(B[12::24])
    rng = np.random.default_rng(1)
    pairs, truth = [], []
    for b in range(N):
        R, t = rodrigues(rng.standard_normal(3), rng.uniform(60.0, 180.0)), rng.uniform(-0.1, 0.1, 3)
        pairs.append((np.ascontiguousarray((src.astype(np.float64) @ R.T + t).astype(np.float32)), model))
        truth.append(R.T)
    K, MD, GATE = 24, 0.0075, 0.01
    call = lambda on: ctx.register_batch_global(pairs, 0.0, K, H, MD, seed=1, gate=GATE, device_normals=on)
    with pkg.Context(0) as ctx:
        for on in (False, True):   # (warm-up: code objects, allocations)
            call(on)
        wall, out = {False: [], True: []}, {}
        for _ in range(RUNS):
            for on in (False, True):
                dt, out[on] = timed(lambda: call(on))
                wall[on].append(dt)
        stage = {False: {}, True: {}}
        with ctx.batch(pairs) as bt:   # the stages of the start pose, one by one: the host route ...
            s = stage[False]
            s["covariances + download"], (cm, cq) = timed(lambda: bt.estimate_covariances(K, None, regularisation="none", want=True))
            s["get_clouds"], clouds = timed(bt.get_clouds)
            s["normals (numpy)"], (nm, nq) = timed(lambda: ([pkg.oriented_normals(D, c, D.astype(np.float64).mean(0)) for (D, _), c in zip(clouds, cm)],
                                                            [pkg.oriented_normals(M, c, M.astype(np.float64).mean(0)) for (_, M), c in zip(clouds, cq)]))
            s["descriptors + upload"], _ = timed(lambda: bt.compute_features(K, (nm, nq)))
            s["matching"], _ = timed(bt.match_features)
            s["ransac"], _ = timed(lambda: bt.ransac(H, MD, seed=1))
        with ctx.batch(pairs) as bt:   # ... and the device route: the first two calls only enqueue, the descriptor call's wait covers all three
            s = stage[True]
            s["covariances (enqueue)"], _ = timed(lambda: bt.estimate_covariances(K, None, regularisation="none"))
            s["normals (enqueue)"], _ = timed(lambda: bt.estimate_point_normals("centroid"))
            s["descriptors (with the wait for all three)"], _ = timed(lambda: bt.compute_features_stored(K))
            s["matching"], _ = timed(bt.match_features)
            s["ransac"], _ = timed(lambda: bt.ransac(H, MD, seed=1))
    print(f"{N} pairs of {src.shape[0]} x {model.shape[0]} points, {H} hypotheses, {RUNS} runs of each route, alternated, after one warm-up of each")
    for on in (False, True):
        w = np.array(wall[on]) * 1e3
        start = np.array([angle_deg(r.extra["global"]["T"][:3, :3] @ Rt.T) for r, Rt in zip(out[on], truth)])
        final = np.array([angle_deg(r.T[:3, :3] @ Rt.T) for r, Rt in zip(out[on], truth)])
        print(f"device_normals={on}: register_batch_global median {np.median(w):.1f} ms, span {w.min():.1f} .. {w.max():.1f} ms")
        print("  stages (ms, host wall): " + ", ".join(f"{k} {v * 1e3:.2f}" for k, v in stage[on].items()))
        print(f"  start pose error (deg): median {np.median(start):.2f} max {start.max():.2f}; after the loop: median {np.median(final):.2f} max {final.max():.2f}; "
              f"within 10 deg at the start: {int((start < 10).sum())} of {N}; within 2 deg at the end: {int((final < 2).sum())} of {N}")


if __name__ == "__main__":
    main()
