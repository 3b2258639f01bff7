#!/usr/bin/env python3
"""Context.register_batch_global over N bunny-sized pairs in unknown relative pose (every 24th point of the bunny against the
points between them, each pair turned by an angle of its own): wall time of the whole call and of its stages, and the pose errors.
Run it under `rocprofv3 --kernel-trace --stats -d DIR --` for the per-launch times (tools/prof_summary.py DIR).

    python tools/global_time.py [N = 64] [hypotheses = 2000]
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
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
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
    with pkg.Context(0) as ctx:
        ctx.register_batch_global(pairs[:2], 0.0, K, 100, MD, gate=GATE)   # (warm-up: code objects, allocations)
        t0 = time.perf_counter()
        out = ctx.register_batch_global(pairs, 0.0, K, H, MD, seed=1, gate=GATE)
        wall = time.perf_counter() - t0
        with ctx.batch(pairs) as bt:   # the stages of the start pose, one by one
            stage = {}
            t = time.perf_counter(); cm, cq = bt.estimate_covariances(K, None, regularisation="none", want=True); stage["covariances"] = time.perf_counter() - t
            clouds = bt.get_clouds()
            t = time.perf_counter()
            nm = [pkg.oriented_normals(D, c, D.astype(np.float64).mean(0)) for (D, _), c in zip(clouds, cm)]
            nq = [pkg.oriented_normals(M, c, M.astype(np.float64).mean(0)) for (_, M), c in zip(clouds, cq)]
            stage["normals (numpy)"] = time.perf_counter() - t
            t = time.perf_counter(); bt.compute_features(K, (nm, nq)); stage["descriptors"] = time.perf_counter() - t
            t = time.perf_counter(); bt.match_features(); stage["matching"] = time.perf_counter() - t
            t = time.perf_counter(); bt.ransac(H, MD, seed=1); stage["ransac"] = time.perf_counter() - t
    start = [angle_deg(r.extra["global"]["T"][:3, :3] @ Rt.T) for r, Rt in zip(out, truth)]
    final = [angle_deg(r.T[:3, :3] @ Rt.T) for r, Rt in zip(out, truth)]
    print(f"{N} pairs of {src.shape[0]} x {model.shape[0]} points, {H} hypotheses: register_batch_global {wall * 1e3:.1f} ms")
    print("stages (ms, host wall, with their waits): " + ", ".join(f"{k} {v * 1e3:.2f}" for k, v in stage.items()))
    print(f"start pose error (deg): median {np.median(start):.2f} max {np.max(start):.2f}; after the loop: median {np.median(final):.2f} max {np.max(final):.2f}; "
          f"within 10 deg at the start: {int((np.array(start) < 10).sum())} of {N}; within 2 deg at the end: {int((np.array(final) < 2).sum())} of {N}")


if __name__ == "__main__":
    main()
