#!/usr/bin/env python3
"""The symmetric metric over N bunny-sized pairs (every 24th point of the bunny against the points between them, each pair moved by
a small motion of its own; point normals made on the device from the covariances of k neighbours): host wall time of the first and
the second step of a symmetric loop and of the steps of a gated point-to-plane loop of the same batch, alternated, and of a whole
symmetric registration.  A build without the symmetric metric (ICP_LIB_PATH) reports its plane steps alone.  Run it under
`rocprofv3 --kernel-trace --stats -d DIR --` for the per-launch times (tools/prof_summary.py DIR).

    python tools/sym_time.py [N = 64] [k = 10] [reps = 9]
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


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    pkg = load_package()
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::24], np.ascontiguousarray(B[12::24])
    rng = np.random.default_rng(1)
    pairs = []
    for b in range(N):
        R, t = rot("z", rng.uniform(-0.02, 0.02)) @ rot("x", rng.uniform(-0.01, 0.01)), rng.uniform(-0.002, 0.002, 3)
        pairs.append((np.ascontiguousarray((src.astype(np.float64) @ R.T + t).astype(np.float32)), model))
    GATE = 0.01
    med = lambda v: float(np.median(v)) if v else None

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    with pkg.Context(0) as ctx, ctx.batch(pairs) as bt:
        have = hasattr(ctx._lib, "icp_solve_symmetric")
        SYM = 4
        bt.estimate_normals()
        bt.set_max_distance(GATE)
        bt.estimate_covariances(K)
        bt.estimate_point_normals("centroid")
        bt.get_moving()

        def steps(metric):   # (first step, second step) of a fresh loop
            bt.begin(max_iter=30, tol=1e-7, metric=metric)
            return timed(lambda: bt.run(1)), timed(lambda: bt.run(1))

        steps(pkg.ICP_POINT_TO_PLANE)   # (warm-up: code objects, allocations)
        if have:
            steps(SYM)
        pl, sy = [], []
        for _ in range(reps):   # alternated, so that both see the same box
            pl.append(steps(pkg.ICP_POINT_TO_PLANE))
            if have:
                sy.append(steps(SYM))

        def whole(metric):   # a whole registration, for the record
            bt.begin(max_iter=30, tol=1e-7, metric=metric)
            t0 = time.perf_counter()
            while bt.run(1 << 20)[1]:
                pass
            loop_s = time.perf_counter() - t0
            st = [bt.state(b) for b in range(N)]
            return dict(loop_s=loop_s, ok=int(sum(s["status"] == 0 for s in st)), passes=int(sum(s["passes"] for s in st)))

        plane_loop = whole(pkg.ICP_POINT_TO_PLANE)
        sym_loop = whole(SYM) if have else None
    sec = lambda v, i: med([x[i] for x in v])
    row = dict(pairs=N, points=int(src.shape[0]), model_points=int(model.shape[0]), k=K, reps=reps, build=os.environ.get("ICP_LIB_PATH") or "this build",
               plane_first_step_s=sec(pl, 0), plane_step_s=sec(pl, 1), plane_step_s_min=float(min(y for _, y in pl)), plane_step_s_max=float(max(y for _, y in pl)),
               symmetric_first_step_s=sec(sy, 0) if sy else None, symmetric_step_s=sec(sy, 1) if sy else None,
               symmetric_step_s_min=float(min(y for _, y in sy)) if sy else None, symmetric_step_s_max=float(max(y for _, y in sy)) if sy else None,
               plane_loop=plane_loop, symmetric_loop=sym_loop)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
