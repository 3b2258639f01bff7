#!/usr/bin/env python3
"""Time one plane segmentation of a batch on the device (Batch.segment_plane) beside the host path that makes the same bytes and
beside a step of the same batch.

usage: segment_time.py [--hypotheses H] [--reps R] [--only CASE,...] [--out FILE] [--profile-case CASE]

Cases: those of `batch_time.py --outliers` -- 64 fp32 grids of 1 024 points, 64 fp64 configs[0] pairs, 16 Bunny_res pairs, one pair
of 65 536 points.  The rule is ("remove", 1 % of the moving cloud's extent, H hypotheses, no axis) on both sides, seed 0 for
every pair.  Per case one JSON row, host clock, median of --reps (3):
  segment_s        one Batch.segment_plane call
  segment_h1_s     the same call with a single hypothesis: what is left of the call without the draws, the three-point solves and
                   the scoring work -- the uploads, the refit, the decision, the compaction, the new batch and the five waits
  host_path_s      get_clouds, the numpy rule (tests/batch_segment_ref.py), icp_batch_create on the result; a cloud object the case
                   repeats is segmented once, so the figure is a lower bound
  first_step_s, step_s   the first and the second step of a fresh point-to-point loop of the same batch
  same_bytes       the device's new clouds equal the host path's
--profile-case runs that case's device call twice and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases(pkg, orc):
    import batch_voxel_ref as vr
    ds = pkg.datasets
    D64, M64 = orc.synth_icp_cpu(32)
    G = ds.synthetic_grid(32, np.float32)
    Gm = ds.make_model_gpu(G, *ds.P2P_GPU)
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    rng = np.random.default_rng(5)
    bunny = [(B, ds.make_model_gpu(B, tuple(np.asarray(ds.BUNNY[0]) + rng.uniform(-0.05, 0.05, 3)), ds.BUNNY[1])) for _ in range(16)]
    N = vr.normal(vr.MAX_POINTS, 12, np.float32)
    return [("grid1024_fp32_x64", [(G, Gm)] * 64, 40, 1e-6), ("configs0_fp64_x64", [(D64, M64)] * 64, 200, 1e-5),
            ("bunny_res_fp32_x16", bunny, 100, 1e-6), ("normal65536_fp32_x1", [(N, N)], 2, 1e-6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--profile-case", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: it bundles the HIP runtime)
    from __graft_entry__ import load_package
    import batch_segment_ref as sr
    import oracle_lib
    pkg = load_package()
    orc = oracle_lib.Oracle()
    only = [c for c in a.only.split(",") if c]
    med = lambda v: float(np.median(v))
    rows = []

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    with pkg.Context(0) as ctx:
        for name, pairs, it, tol in cases(pkg, orc):
            if (only and name not in only) or (a.profile_case and name != a.profile_case):
                continue
            D0 = pairs[0][0]
            extent = float((D0.max(axis=0).astype(np.float64) - D0.min(axis=0).astype(np.float64)).max())
            dist = 0.01 * extent
            seeds = np.zeros(len(pairs), dtype=np.uint64)
            with ctx.batch(pairs) as bt:
                def device(H=a.hypotheses):
                    return bt.segment_plane(("remove", dist, H), ("remove", dist, H), seed=seeds)[0]

                def host():
                    seen = {}

                    def one(src, X, seed, side):
                        key = (id(src), int(seed), side)
                        if key not in seen:
                            seen[key] = sr.segment(X, sr.rule(sr.REMOVE, dist, a.hypotheses), int(seed), side)["cloud"]
                        return seen[key]
                    return ctx.batch([(one(D, g[0], s, 0), one(M, g[1], s, 1)) for (D, M), g, s in zip(pairs, bt.get_clouds(), seeds)])

                if a.profile_case:
                    for _ in range(2):
                        device().close()
                    print(json.dumps(dict(case=name, pairs=len(pairs), hypotheses=a.hypotheses)), flush=True)
                    continue

                def steps():   # (first step, second step) of a fresh loop
                    bt.begin(max_iter=it, tol=tol, metric=pkg.ICP_POINT_TO_POINT)
                    return timed(lambda: bt.run(1))[0], timed(lambda: bt.run(1))[0]

                steps()
                st = [steps() for _ in range(a.reps)]
                with device() as X:   # (warm-up, and the check: the same bytes)
                    after = (int(X._moff[-1]), int(X._qoff[-1]))
                    with host() as Y:
                        same = all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(X.get_clouds(), Y.get_clouds()))
                td, t1, th = [], [], []
                for _ in range(a.reps):   # alternated, so that all see the same box
                    s, nb = timed(device)
                    nb.close()
                    td.append(s)
                    s, nb = timed(lambda: device(1))
                    nb.close()
                    t1.append(s)
                    s, nb = timed(host)
                    nb.close()
                    th.append(s)
            row = dict(case=name, pairs=len(pairs), points=int(D0.shape[0]), hypotheses=a.hypotheses, distance=dist,
                       points_before=[int(bt._moff[-1]), int(bt._qoff[-1])], points_after=list(after),
                       segment_s=med(td), segment_s_min=float(min(td)), segment_s_max=float(max(td)), segment_h1_s=med(t1),
                       host_path_s=med(th), host_path_s_min=float(min(th)), host_path_s_max=float(max(th)),
                       host_segmented_clouds=len({(id(X), int(s), k) for pr, s in zip(pairs, seeds) for k, X in enumerate(pr)}),
                       first_step_s=med([x for x, _ in st]), step_s=med([y for _, y in st]), reps=a.reps, same_bytes=same)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
