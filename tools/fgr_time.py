#!/usr/bin/env python3
"""Fast Global Registration beside RANSAC over N copies of the bunny pair (every 24th point of the bunny, turned 149 degrees, against
the points between them: 1 498 points each, 391 mutual correspondences): host wall time of Batch.fgr at I iterations and of
Batch.ransac at H hypotheses on the same batch, alternated in one process, and the time of one FGR iteration with the host's share of
it -- enqueue, wait and solve as the library's own clock reads report them (Batch.diag_fgr_times).  Every figure is the median of
reps runs after a warm-up, with min and max.  Run it under `rocprofv3 --kernel-trace --stats -d DIR --` for the per-launch times
(tools/prof_summary.py DIR).

    python tools/fgr_time.py [N = 64] [I = 64] [H = 2000] [reps = 20]
"""
import json
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
    I = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    pkg = load_package()
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::24], np.ascontiguousarray(B[12::24])
    R, t = rodrigues((1.0, 2.0, 3.0), 149.0), np.array([0.05, -0.03, 0.08])
    moving = np.ascontiguousarray((src.astype(np.float64) @ R.T + t).astype(np.float32))
    K, MD = 24, 0.0075
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    with pkg.Context(0) as ctx, ctx.batch([(moving, model)] * N) as bt:
        cm, cq = bt.estimate_covariances(K, None, regularisation="none", want=True)
        nm = [pkg.oriented_normals(moving, cm[0], moving.astype(np.float64).mean(0))] * N
        nq = [pkg.oriented_normals(model, cq[0], model.astype(np.float64).mean(0))] * N
        bt.compute_features(K, (nm, nq))
        _, _, kept = bt.match_features()
        bt.fgr(MD, iterations=I)         # (warm-up: code objects, allocations)
        bt.ransac(H, MD, seed=1)
        tf, tr, it_s, enq, wait, solve = [], [], [], [], [], []
        for _ in range(reps):            # alternated, so that both see the same box
            s, f = timed(lambda: bt.fgr(MD, iterations=I))
            tf.append(s)
            tm = bt.diag_fgr_times()
            it_s.append((tm["enqueue_s"] + tm["wait_s"] + tm["solve_s"]) / tm["iterations"])
            enq.append(tm["enqueue_s"] / tm["iterations"])
            wait.append(tm["wait_s"] / tm["iterations"])
            solve.append(tm["solve_s"] / tm["iterations"])
            s, r = timed(lambda: bt.ransac(H, MD, seed=1))
            tr.append(s)
    Rt = R.T
    row = dict(pairs=N, points=int(src.shape[0]), model_points=int(model.shape[0]), correspondences=int(kept[0].sum()), iterations=I, hypotheses=H,
               reps=reps, fgr_s=stat(tf), ransac_s=stat(tr), fgr_iteration_s=stat(it_s), iteration_enqueue_s=stat(enq), iteration_wait_s=stat(wait),
               iteration_solve_s=stat(solve), host_wait_and_solve_share=float((np.median(wait) + np.median(solve)) / np.median(it_s)),
               fgr_rot_deg=angle_deg(f[0]["T"][:3, :3] @ Rt.T), ransac_rot_deg=angle_deg(r[0]["T"][:3, :3] @ Rt.T),
               fgr_status_ok=int(sum(x["status"] == 0 for x in f)), ransac_status_ok=int(sum(x["status"] == 0 for x in r)))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
