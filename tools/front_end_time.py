#!/usr/bin/env python3
"""The point-to-plane front end alone (kNN(4) + PCA normals), host wall of the whole call with its download and wait:
Context.estimate_normals on the hall model (16 384 points) in float32 (knn4_f32_v2 + knn4_merge_kernel + normals_kernel<float>) and
in float64 (knn4_kernel<double, 1024> + normals_kernel<double>), and Batch.estimate_normals on 64 grids of 1 024 points in both
precisions (knn4_batch + normals_batch_kernel).  Median and span over RUNS calls of each after two warm-up calls, one JSON line.
ICP_LIB_PATH selects another build: alternate two builds in ONE session and compare the medians against the spans.

    python tools/front_end_time.py [runs = 30] [--label TEXT]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (torch's HIP runtime first, as in tests/conftest.py)
except Exception:
    pass
from __graft_entry__ import load_package  # noqa: E402


def stats(fn, runs):
    for _ in range(2):
        fn()
    w = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        w.append((time.perf_counter() - t) * 1e3)
    w = np.array(w)
    return dict(median_ms=round(float(np.median(w)), 4), min_ms=round(float(w.min()), 4), max_ms=round(float(w.max()), 4))


def main():
    args = [a for a in sys.argv[1:]]
    label = args.pop(args.index("--label") + 1) if "--label" in args else (os.environ.get("ICP_LIB_PATH") or "this build")
    args = [a for a in args if a != "--label"]
    runs = int(args[0]) if args else 30
    import oracle_lib
    pkg = load_package()
    hall = oracle_lib.Oracle().hall_clouds(os.path.join(ROOT, "tests", "golden"))[1]
    row = dict(label=label, runs=runs)
    with pkg.Context(0) as ctx:
        for name, dtype in (("f32", np.float32), ("f64", np.float64)):
            ctx.set_model(hall.astype(dtype))
            row[f"hall_{name}"] = stats(ctx.estimate_normals, runs)
            G = pkg.datasets.synthetic_grid(32, np.float32)
            M = pkg.datasets.make_model_gpu(G, *pkg.datasets.P2P_GPU).astype(dtype)
            with ctx.batch([(G.astype(dtype), M)] * 64) as bt:
                row[f"batch64x1024_{name}"] = stats(bt.estimate_normals, runs)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
