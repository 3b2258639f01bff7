#!/usr/bin/env python3
"""Which kernels, grids and blocks the launch plan (csrc/icp_plan.cpp) produces, form by form: a fresh context per form, three
passes of a point-to-point and of a point-to-plane registration, at the smallest size that selects the form.  Run it under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/launch_shapes.py` for two builds (ICP_LIB_PATH selects the
other one) and compare `python3 tools/launch_shapes.py --reduce DIR` of the two: sorted `kernel name, grid, workgroup, count` lines.
usage: launch_shapes.py [--reduce DIR]"""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("ICP_NN_SPARSE", "ICP_NN_CULL", "ICP_NN_ROW", "ICP_NN_WAVES", "ICP_NN_WAVES128", "ICP_NN_COLD8", "ICP_NN_HIER", "ICP_NN_ORDER", "ICP_NN_SHARE",
            "ICP_NN_SHARE_RESIDENT", "ICP_NN_SPECULATE", "ICP_F64_SPARSE", "ICP_SORT")

# (name, switches, n, m, float64, exclusive, registrations) -- sizes for 256 CUs
FORMS = [
    # rows of 64: up to 2 x CUs rows
    ("row64", {}, 1024, 1024, False, False, 1),
    ("row64_exclusive", {}, 1024, 1024, False, True, 1),
    ("row64_waves16", {"ICP_NN_WAVES": "16"}, 1024, 1024, False, False, 1),
    ("row64_forced", {"ICP_NN_ROW": "64"}, 33000, 33000, False, False, 1),
    ("cull0", {"ICP_NN_CULL": "0"}, 1024, 1024, False, False, 1),
    # rows of 128, flat: more rows than CUs -> 8 waves and shared rows; beyond 2 CUs - CUs / 4 rows -> 16 waves
    ("row128_shared", {}, 33000, 33000, False, False, 2),
    ("row128_share0", {"ICP_NN_SHARE": "0"}, 33000, 33000, False, False, 1),
    ("row128_waves16", {"ICP_NN_WAVES128": "16"}, 33000, 33000, False, False, 1),
    ("row128_16", {}, 57345, 57345, False, False, 1),
    ("row128_forced", {"ICP_NN_ROW": "128"}, 1024, 1024, False, False, 1),
    ("row128_forced_split", {"ICP_NN_ROW": "128"}, 1024, 4096, False, False, 1),
    ("row128_forced_waves8", {"ICP_NN_ROW": "128", "ICP_NN_WAVES128": "8"}, 1024, 1024, False, False, 1),
    # rows of 128, hierarchical: by the cloud from 2^16 model points, by the model from 2^17; 4 waves and ordered rows from 2 CUs rows
    ("hier_by_cloud", {}, 66000, 66000, False, False, 1),
    ("hier0", {"ICP_NN_HIER": "0"}, 66000, 66000, False, False, 1),
    ("hier_waves8", {"ICP_NN_WAVES128": "8"}, 66000, 66000, False, False, 1),
    ("hier_ordered_4_waves", {}, 131072, 131072, False, False, 2),
    ("hier_order0", {"ICP_NN_ORDER": "0"}, 131072, 131072, False, False, 1),
    ("hier1", {"ICP_NN_HIER": "1"}, 1024, 1024, False, False, 1),
    ("row128_waves4_hier1", {"ICP_NN_ROW": "128", "ICP_NN_WAVES128": "4", "ICP_NN_HIER": "1"}, 2048, 1024, False, False, 1),
    # (a model of 1024 points: one segment -- only unsplit rows take fewer than 16 waves or an order)
    # the ordered 4-wave form: a first (cold, 8 waves) and a second registration (its counters hold history: 4 waves)
    ("order2_waves4", {"ICP_NN_ORDER": "2", "ICP_NN_WAVES128": "4", "ICP_NN_HIER": "1", "ICP_NN_ROW": "128"}, 2048, 1024, False, False, 2),
    ("order2_waves8", {"ICP_NN_ORDER": "2", "ICP_NN_WAVES128": "8", "ICP_NN_HIER": "1", "ICP_NN_ROW": "128"}, 2048, 1024, False, False, 2),
    # every pair, packed: 2 points per lane with and without the early-out, 4 points per lane from n_pad / 256 >= 8 CUs
    ("dense_packed", {"ICP_NN_SPARSE": "0"}, 1024, 1024, False, False, 1),
    ("dense_packed_cull0", {"ICP_NN_SPARSE": "0", "ICP_NN_CULL": "0"}, 1024, 1024, False, False, 1),
    ("dense_packed_4_per_lane", {"ICP_NN_SPARSE": "0"}, 523265, 1024, False, False, 1),
    # fp64: rows of 64 with rows <= CUs (16 waves) and > CUs (8 waves); thread per point beyond 2 CUs rows or by the switch
    ("f64_rows_fit", {}, 1024, 1024, True, False, 1),
    ("f64_rows_exceed", {}, 16385, 1024, True, False, 1),
    ("f64_dense_by_size", {}, 33000, 1024, True, False, 1),
    ("f64_dense", {"ICP_F64_SPARSE": "0"}, 1024, 1024, True, False, 1),
]


def clouds(pkg, n, m, dtype):
    import numpy as np

    def grid(count):
        return np.ascontiguousarray(pkg.datasets.synthetic_grid(int(np.ceil(np.sqrt(count))), dtype)[:count])
    make_model = pkg.datasets.make_model_cpu if np.dtype(dtype) == np.float64 else pkg.datasets.make_model_standard
    return grid(n), np.ascontiguousarray(make_model(grid(m)))


def run():
    import numpy as np
    from __graft_entry__ import load_package
    pkg = load_package()
    for name, env, n, m, f64, exclusive, registrations in FORMS:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)   # (the switches are read by icp_create)
        D, M = clouds(pkg, n, m, np.float64 if f64 else np.float32)
        with pkg.Context(0) as ctx:
            if exclusive:
                ctx.set_exclusive(True)
            for r in range(registrations):
                a = ctx.point_to_point(D, M, max_iter=3, tol=1e-6, fixed_iterations=True)
                info = ctx.nn_launch_info()
                b = ctx.point_to_plane(D, M, max_iter=3, tol=1e-6, fixed_iterations=True)
                print(f"{name} #{r}: {n} x {m} {'f64' if f64 else 'f32'} {env} -> {info}; errors {a.err[-1]:.9g} {b.err[-1]:.9g}", flush=True)


def kernel_name(full):
    """the kernel with its template arguments: no return type, namespace or parameter list; a library's long names cut at 100 characters"""
    name = full[:full.rindex("(")] if full.endswith(")") else full
    if name.startswith("void "):
        name = name[5:]
    return name.replace("icp::", "")[:100]


def reduce(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit(f"expected one kernel trace under {d}, found {files}")
    count = collections.Counter()
    for r in csv.DictReader(open(files[0])):
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        block = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        count[(kernel_name(r["Kernel_Name"]), grid, block)] += 1
    for (kernel, grid, block), c in sorted(count.items()):
        print(f"{kernel}, {grid}, {block}, {c}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    elif len(sys.argv) == 1:
        run()
    else:
        sys.exit(__doc__)
