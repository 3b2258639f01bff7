#!/usr/bin/env python3
"""Pair-iterations per second of the batched loops (Context.point_to_point_batch / point_to_plane_batch, one launch per step
for all pairs) against a loop of Context.point_to_point / point_to_plane over the same pairs (GPU box).

  python3 tools/batch_time.py [--metric point|plane] [--reps 5] [--out FILE] [--only CASE,CASE] [--max-distance V] [--trim R]
                              [--reciprocal] [--robust KIND:SCALE] [--label TEXT] [--init | --premoved] [--evaluate] [--voxel V]
                              [--outliers KIND:N:VALUE] [--generalized K]

Cases, --metric point: 64 and 256 configs[0] pairs (synth_icp_cpu(32), fp64, tol 1e-5); 64 fp32 1 024-point grids
(make_model_gpu, tol 1e-6); 16 Bunny_res pairs (rotated copies, fp32, tol 1e-6).  --metric plane: the fp32 case sets and the
64 grids in fp64 (max_iter 50, tol 1e-6), each once with the caller's normals (the oracle's, computed outside the timed region)
and once with normals estimated on the device (the batch: one neighbour launch + one normals launch for all pairs; the
sequential loop: icp_estimate_normals per pair).  Both sides are timed end to end (upload included) with a host clock
around calls that end in a device synchronisation; a pair-iteration is one matching pass of one pair (Result.passes).  The
sequential side also reports its loops alone (Result.seconds_total, the registration without the upload and the normals).
Median of --reps after one warm-up of every case.  Every pair must run the same passes on both sides: the rows carry the number of
pairs that did not (pairs_stopping_apart), and the tool exits non-zero if there is one.

--max-distance V (a distance, or inf) runs the batched side with that maximum correspondence distance on every pair
(Context.point_to_point_batch(max_distance=V) / point_to_plane_batch_gated: the gated kernels, through the Batch object); the
sequential side has no gate, so the passes agree only for inf and only then are they compared.  The cost of the gate is
--max-distance inf against a run without the option.  Every row carries the fastest and the slowest of its --reps runs beside the
median (batched_s_min / batched_s_max), and --label TEXT as "label" (which build, which round).  ICP_LIB_PATH selects another
build of the library for an A/B run on one box.

--trim R (a share in (0, 1]) runs the batched side with that share of every moving cloud kept (Context.point_to_*_batch(trim=R):
the deferred route, four launches per step; R = 1.0 goes through the Batch object and runs the fused pass).  The sequential side
does not trim, so the passes are compared only for R = 1.0.  The cost of trimming is --trim R against --max-distance inf of the
same build (both through the Batch object).

--reciprocal runs the batched side with every pair reciprocal (Context.register_batch(reciprocal=True): the deferred route with the
reverse search, four launches per step, five with --trim), combinable with --max-distance and --trim.  The sequential side has no
such rule, so the passes are not compared.  The cost of reciprocity is --reciprocal against --trim R of the same build (the
deferred route without the reverse search), and --reciprocal --trim R against both.  With --evaluate the timed steps (first_step_s,
step_s) and the registration run with the gate, the trim and the flags given; the evaluation itself never looks at them.

--robust KIND:SCALE (huber, cauchy or tukey, and the kernel's k in the clouds' unit) runs the batched side with that robust kernel on
every pair (Context.register_batch_robust: the deferred route with batch_robust_moments, three launches per step, up to five with
--reciprocal and --trim), combinable with the options above.  The sequential side has no kernels, so the passes are not compared.
The cost of a robust step is --robust against a run without it of the same build (--evaluate: step_s), and against --trim R (the
deferred route without the weights).

--init times the batched side from a far pose -- every moving cloud carried off by G (40 degrees about z, shifted by (3, -2, 1))
outside the timed region -- with the inverse pose as every pair's initial transform (Context.point_to_*_batch(init=...)).
--premoved is its baseline: the same far clouds moved back on the host with the same arithmetic (ref_moments.apply_rt, outside
the timed region) and no initial transform, through the same Batch route (create, begin, run, per-pair state), so the two differ
by the start-cloud launch of icp_batch_begin and its synchronisation alone and run the same bits.  Under either option the
sequential side registers the pre-moved clouds, and every pair must run the same passes on both sides.

--evaluate times one evaluation of every case's batch (Batch.evaluate: three launches and one download, without and with the
matches) beside one step of the same batch (Batch.run(1): the first step after begin, which matches only, and the second, which
applies and matches) and the whole batched registration (batched_s, as in the rows without the option); nothing sequential is
run.  A build without icp_batch_evaluate (ICP_LIB_PATH) reports the steps and the registration alone (evaluate_s null).

--voxel V times one voxel-grid downsampling of every case's batch on the device (Batch.downsample: four launches, two host waits)
beside a host path that does the same job -- Batch.get_clouds, the numpy rule (tests/batch_voxel_ref.downsample) and a new Batch
from the result -- and beside the first and the second step of the same batch; nothing sequential is run.  The cases' clouds differ
in scale by orders of magnitude, so V is a share of the largest extent of the case's first moving cloud (0.05: about 20 cells along
it); the row carries the edge itself (voxel_edge) and the points before and after.  Two more rows time one pair of 65 536
normal points at its extremes: every point alone (the widest scan) and every point in one cell (one lane adds them all).  The two paths must make the same bytes (same_bytes in
the row): the tool exits non-zero if they do not.  With --profile-case the case's batch is downsampled twice and nothing else is run.

--outliers KIND:N:VALUE times one outlier removal of every case's batch on the device (Batch.remove_outliers with that rule on both
sides: three launches, two host waits) beside a host path that does the same job -- Batch.get_clouds, the numpy brute force of the
rule (tests/batch_outlier_ref.remove; a cloud the case repeats is filtered once, host_filtered_clouds in the row, so the host time is
a lower bound) and a new Batch from the result -- and beside the first and the second step of the same batch;
nothing sequential is run.  statistical:K:RATIO, or radius:MIN:R with R a share of the largest extent of the case's first moving
cloud (the cases differ in scale by orders of magnitude; the row carries the radius itself).  One more row times one pair of
65 536 normal points on the device alone (host_path_s null: the numpy brute force of 2 x 65 536^2 distances takes minutes).  The
two paths must make the same bytes (same_bytes), or the tool exits non-zero.  With --profile-case the case's batch is filtered
twice and nothing else is run.

--generalized K times, for every case's batch, one covariance call (Batch.estimate_covariances with K neighbours on both sides: one
launch, no host wait, closed by a get_moving download so that the clock sees the device finish) and the first and second step of a
generalized loop (Batch.begin with ICP_GENERALIZED: the deferred route, three launches per step), beside the steps of the same batch
under the case's own metric (step_s: what the rows of --evaluate report, and what a build without the generalized metric,
ICP_LIB_PATH, reports alone) and under point-to-plane with device normals (plane_step_s).  Nothing sequential is run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def plane_cases(pkg, orc):
    """(name, pairs, normals or None, max_iter, tol)"""
    ds = pkg.datasets
    G = ds.synthetic_grid(32, np.float32)
    Gm = ds.make_model_gpu(G, *ds.P2P_GPU)
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    rng = np.random.default_rng(5)
    bunny = [(B, ds.make_model_gpu(B, tuple(np.asarray(ds.BUNNY[0]) + rng.uniform(-0.05, 0.05, 3)), ds.BUNNY[1])) for _ in range(16)]
    nrm = lambda M: orc.normals(M, orc.knn4(M))[0]
    Gn = nrm(Gm)
    sets = [("grid1024_fp32_x64", [(G, Gm)] * 64, [Gn] * 64),
            ("grid1024_fp64_x64", [(G.astype(np.float64), Gm.astype(np.float64))] * 64, [Gn.astype(np.float64)] * 64),
            ("bunny_res_fp32_x16", bunny, [nrm(M) for _, M in bunny])]
    out = []
    for name, pairs, normals in sets:
        out.append((name + "_plane_given", pairs, normals, 50, 1e-6))
        out.append((name + "_plane_estimated", pairs, None, 50, 1e-6))
    return out


def cases(pkg, orc):
    ds = pkg.datasets
    D64, M64 = orc.synth_icp_cpu(32)
    G = ds.synthetic_grid(32, np.float32)
    Gm = ds.make_model_gpu(G, *ds.P2P_GPU)
    B = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    rng = np.random.default_rng(5)
    bunny = [(B, ds.make_model_gpu(B, tuple(np.asarray(ds.BUNNY[0]) + rng.uniform(-0.05, 0.05, 3)), ds.BUNNY[1])) for _ in range(16)]
    return [
        ("configs0_fp64_x64", [(D64, M64)] * 64, 200, 1e-5),
        ("configs0_fp64_x256", [(D64, M64)] * 256, 200, 1e-5),
        ("grid1024_fp32_x64", [(G, Gm)] * 64, 40, 1e-6),
        ("bunny_res_fp32_x16", bunny, 100, 1e-6),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric", choices=("point", "plane"), default="point")
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma-separated case names: run only these")
    ap.add_argument("--max-distance", type=float, default=None, help="gate the batched side at this distance (inf: the gated kernels, nothing rejected)")
    ap.add_argument("--trim", type=float, default=None, help="keep this share of every moving cloud on the batched side (the deferred route)")
    ap.add_argument("--reciprocal", action="store_true", help="every pair keeps only mutual nearest neighbours on the batched side (the deferred route with the reverse search)")
    ap.add_argument("--robust", default="", metavar="KIND:SCALE", help="every pair weighs its matches with this robust kernel on the batched side, e.g. cauchy:0.05")
    ap.add_argument("--label", default="", help="copied into every row")
    ap.add_argument("--init", action="store_true", help="the batched side starts from a far pose with the inverse pose as initial transform")
    ap.add_argument("--premoved", action="store_true", help="the baseline of --init: the far clouds moved back on the host, no initial transform, same route")
    ap.add_argument("--evaluate", action="store_true", help="time one evaluation of every case's batch beside one step of the same batch")
    ap.add_argument("--voxel", type=float, default=None, metavar="V", help="time one device downsampling of every case's batch at V x the cloud's extent beside the host path")
    ap.add_argument("--outliers", default="", metavar="KIND:N:VALUE", help="time one device outlier removal of every case's batch beside the host path, e.g. statistical:16:1.0 or radius:4:0.05")
    ap.add_argument("--generalized", type=int, default=None, metavar="K", help="time the covariance call (K neighbours) and the steps of a generalized loop of every case's batch beside its own steps")
    ap.add_argument("--profile-case", default="", help="run only this case's batched registration, once after a warm-up (for a kernel trace)")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: it bundles the HIP runtime)
    from __graft_entry__ import load_package
    import oracle_lib
    import ref_moments
    pkg = load_package()
    orc = oracle_lib.Oracle()
    rows = []
    if a.init and a.premoved:
        sys.exit("--init or --premoved, not both")
    ang = np.deg2rad(40.0)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], (3.0, -2.0, 1.0)
    G_inv = np.eye(4)
    G_inv[:3, :3], G_inv[:3, 3] = G[:3, :3].T, -G[:3, :3].T @ G[:3, 3]

    def carried(pairs, back):
        """every moving cloud carried to the far pose (and back again, as icp_batch_begin would move it); one cloud object once"""
        seen = {}
        for D, _ in pairs:
            if id(D) not in seen:
                far = ref_moments.apply_rt(D, G[:3, :3], G[:3, 3])
                seen[id(D)] = ref_moments.apply_rt(far, G_inv[:3, :3], G_inv[:3, 3]) if back else far
        return [(seen[id(D)], M) for D, M in pairs]

    with pkg.Context(0) as ctx:
        plane = a.metric == "plane"
        todo = plane_cases(pkg, orc) if plane else [(name, pairs, None, it, tol) for name, pairs, it, tol in cases(pkg, orc)]
        edge_of = {}
        if a.voxel is not None and not plane:   # the two extremes of one cloud at ICP_BATCH_MAX_POINTS: the widest scan, the longest sum
            import batch_voxel_ref as vr
            B = vr.normal(vr.MAX_POINTS, 12, np.float32)
            todo += [("normal65536_fp32_x1_alone", [(B, B)], None, 2, 1e-6), ("normal65536_fp32_x1_one_cell", [(B, B)], None, 2, 1e-6)]
            edge_of = {"normal65536_fp32_x1_alone": vr.identity_voxel(B), "normal65536_fp32_x1_one_cell": 1e6}
        outlier = None
        if a.outliers:
            kind, _, rest = a.outliers.partition(":")
            cnt, _, val = rest.partition(":")
            if kind not in ("statistical", "radius") or not cnt or not val:
                sys.exit("--outliers statistical:K:RATIO or radius:MIN:SHARE")
            outlier = (kind, int(cnt), float(val))
            if not plane:
                import batch_voxel_ref as vr
                B = vr.normal(vr.MAX_POINTS, 12, np.float32)
                todo += [("normal65536_fp32_x1", [(B, B)], None, 2, 1e-6)]
        only = [c for c in a.only.split(",") if c]
        unknown = [c for c in only if c not in [t[0] for t in todo]]
        if unknown:
            sys.exit(f"unknown case(s) {unknown}: {[t[0] for t in todo]}")
        gate = a.max_distance
        trim = a.trim
        recip = True if a.reciprocal else None
        robust = None
        if a.robust:
            kind, _, scale = a.robust.partition(":")
            if kind not in ("huber", "cauchy", "tukey") or not scale:
                sys.exit("--robust KIND:SCALE with KIND huber, cauchy or tukey")
            robust = (kind, float(scale))
        for name, pairs, normals, it, tol in todo:
            if only and name not in only:
                continue
            seq_pairs = carried(pairs, True) if a.init or a.premoved else pairs
            bat_pairs = carried(pairs, False) if a.init else seq_pairs
            metric = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT

            def run_batched():
                if robust:
                    return ctx.register_batch_robust(bat_pairs, robust[0], robust[1], metric=metric, normals=normals, max_iter=it, tol=tol,
                                                     max_distance=gate, init=G_inv if a.init else None, trim=trim, reciprocal=recip)
                if a.init or a.premoved or recip:   # through the Batch object (--init / --premoved differ by the initial transforms alone)
                    return ctx._run_batch_gated(metric, bat_pairs, normals, it, tol, False, gate, G_inv if a.init else None, trim, recip)
                if plane and (gate is not None or trim is not None):
                    return ctx.point_to_plane_batch_gated(pairs, gate, normals=normals, max_iter=it, tol=tol, trim=trim)
                if plane:
                    return ctx.point_to_plane_batch(pairs, normals=normals, max_iter=it, tol=tol)
                return ctx.point_to_point_batch(pairs, max_iter=it, tol=tol, max_distance=gate, trim=trim)

            def run_sequential():
                if plane:
                    return [ctx.point_to_plane(D, M, normals=None if normals is None else normals[k], max_iter=it, tol=tol)
                            for k, (D, M) in enumerate(seq_pairs)]
                return [ctx.point_to_point(D, M, max_iter=it, tol=tol) for D, M in seq_pairs]

            if outlier is not None:
                import batch_outlier_ref as ro
                if a.profile_case and name != a.profile_case:
                    continue
                D0 = pairs[0][0]
                extent = float((D0.max(axis=0).astype(np.float64) - D0.min(axis=0).astype(np.float64)).max())
                rule = ("statistical", outlier[1], outlier[2]) if outlier[0] == "statistical" else ("radius", outlier[2] * extent, outlier[1])
                med = lambda v: float(np.median(v))
                with_host = pairs[0][0].shape[0] < 65536

                def timed(fn):
                    t0 = time.perf_counter()
                    out = fn()
                    return time.perf_counter() - t0, out

                with ctx.batch(pairs) as bt:
                    def device():
                        return bt.remove_outliers(rule, rule)[0]

                    def host():
                        seen = {}   # (a cloud object the case repeats is filtered once: the row says so, and the host time is a lower bound)

                        def one(src, X):
                            if id(src) not in seen:
                                seen[id(src)] = ro.remove(X, rule)[0]
                            return seen[id(src)]
                        return ctx.batch([(one(D, g[0]), one(M, g[1])) for (D, M), g in zip(pairs, bt.get_clouds())])

                    if a.profile_case:
                        for _ in range(2):
                            device().close()
                        print(json.dumps(dict(case=name, pairs=len(pairs), rule=list(rule))), flush=True)
                        continue

                    def steps():   # (first step, second step) of a fresh loop
                        bt.begin(max_iter=it, tol=tol, metric=pkg.ICP_POINT_TO_POINT)
                        return timed(lambda: bt.run(1))[0], timed(lambda: bt.run(1))[0]

                    steps()
                    st = [steps() for _ in range(a.reps)]
                    same = None
                    with device() as X:   # (warm-up, and the check: the same bytes)
                        after = (int(X._moff[-1]), int(X._qoff[-1]))
                        if with_host:
                            with host() as Y:
                                same = all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(X.get_clouds(), Y.get_clouds()))
                    td, th = [], []
                    for _ in range(a.reps):   # alternated, so that both see the same box
                        s, nb = timed(device)
                        nb.close()
                        td.append(s)
                        if with_host:
                            s, nb = timed(host)
                            nb.close()
                            th.append(s)
                row = dict(case=name, pairs=len(pairs), points=int(pairs[0][0].shape[0]), outliers=a.outliers, rule=list(rule),
                           points_before=[int(bt._moff[-1]), int(bt._qoff[-1])], points_after=list(after),
                           remove_outliers_s=med(td), remove_outliers_s_min=float(min(td)), remove_outliers_s_max=float(max(td)),
                           host_path_s=med(th) if th else None, host_path_s_min=float(min(th)) if th else None, host_path_s_max=float(max(th)) if th else None,
                           host_filtered_clouds=len({id(X) for pr in pairs for X in pr}),
                           first_step_s=med([x for x, _ in st]), step_s=med([y for _, y in st]), reps=a.reps,
                           pairs_stopping_apart=0, same_bytes=same, label=a.label)
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue

            if a.voxel is not None:
                import batch_voxel_ref as vr
                if a.profile_case and name != a.profile_case:
                    continue
                D0 = pairs[0][0]
                edge = edge_of.get(name, float(a.voxel) * float((D0.max(axis=0).astype(np.float64) - D0.min(axis=0).astype(np.float64)).max()))
                med = lambda v: float(np.median(v))

                def timed(fn):
                    t0 = time.perf_counter()
                    out = fn()
                    return time.perf_counter() - t0, out

                with ctx.batch(pairs) as bt:
                    def device():
                        return bt.downsample(edge)

                    def host():
                        thin = [(vr.downsample(D, edge)[0], vr.downsample(M, edge)[0]) for D, M in bt.get_clouds()]
                        return ctx.batch(thin)

                    if a.profile_case:
                        for _ in range(2):
                            device().close()
                        print(json.dumps(dict(case=name, pairs=len(pairs), voxel_edge=edge)), flush=True)
                        continue

                    def steps():   # (first step, second step) of a fresh loop
                        bt.begin(max_iter=it, tol=tol, metric=pkg.ICP_POINT_TO_POINT)
                        return timed(lambda: bt.run(1))[0], timed(lambda: bt.run(1))[0]

                    steps()
                    st = [steps() for _ in range(a.reps)]
                    with device() as X, host() as Y:   # (warm-up, and the check: the same bytes)
                        same = all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(X.get_clouds(), Y.get_clouds()))
                        after = (int(X._moff[-1]), int(X._qoff[-1]))
                    td, th = [], []
                    for _ in range(a.reps):   # alternated, so that both see the same box
                        s, nb = timed(device)
                        nb.close()
                        td.append(s)
                        s, nb = timed(host)
                        nb.close()
                        th.append(s)
                row = dict(case=name, pairs=len(pairs), points=int(pairs[0][0].shape[0]), voxel=a.voxel, voxel_edge=edge,
                           points_before=[int(bt._moff[-1]), int(bt._qoff[-1])], points_after=list(after),
                           downsample_s=med(td), downsample_s_min=float(min(td)), downsample_s_max=float(max(td)),
                           host_path_s=med(th), host_path_s_min=float(min(th)), host_path_s_max=float(max(th)),
                           first_step_s=med([x for x, _ in st]), step_s=med([y for _, y in st]), reps=a.reps,
                           pairs_stopping_apart=0, same_bytes=bool(same), label=a.label)
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue

            if a.profile_case:
                if name == a.profile_case:
                    for _ in range(2):
                        res = run_batched()
                    print(json.dumps(dict(case=name, pairs=len(pairs), pair_iterations=sum(r.passes for r in res),
                                          steps=max(r.passes for r in res) + 1)), flush=True)
                continue

            if a.generalized is not None:
                med = lambda v: float(np.median(v))
                have = hasattr(ctx._lib, "icp_batch_estimate_covariances")
                with ctx.batch(pairs) as bt:
                    def timed(fn):
                        t0 = time.perf_counter()
                        fn()
                        return time.perf_counter() - t0

                    def steps(m):   # (first step, second step) of a fresh loop
                        bt.begin(max_iter=it, tol=tol, metric=m)
                        return timed(lambda: bt.run(1)), timed(lambda: bt.run(1))

                    def cov():
                        bt.estimate_covariances(a.generalized)
                        bt.get_moving()

                    if plane:
                        bt.set_model_normals(normals) if normals is not None else bt.estimate_normals()
                    own, pl, gen, tc = [], [], [], []
                    steps(metric)
                    if not plane:
                        bt.estimate_normals()
                    steps(pkg.ICP_POINT_TO_PLANE)
                    if have:
                        cov()
                        steps(pkg.ICP_GENERALIZED)
                    for _ in range(a.reps):   # alternated, so that all see the same box
                        own.append(steps(metric))
                        pl.append(steps(pkg.ICP_POINT_TO_PLANE))
                        if have:
                            tc.append(timed(cov))
                            gen.append(steps(pkg.ICP_GENERALIZED))
                sec = lambda v, i: med([x[i] for x in v]) if v else None
                row = dict(case=name, pairs=len(pairs), points=int(pairs[0][0].shape[0]), k=a.generalized,
                           first_step_s=sec(own, 0), step_s=sec(own, 1), step_s_min=float(min(y for _, y in own)), step_s_max=float(max(y for _, y in own)),
                           plane_first_step_s=sec(pl, 0), plane_step_s=sec(pl, 1),
                           covariances_s=med(tc) if tc else None, covariances_s_min=float(min(tc)) if tc else None, covariances_s_max=float(max(tc)) if tc else None,
                           generalized_first_step_s=sec(gen, 0), generalized_step_s=sec(gen, 1),
                           generalized_step_s_min=float(min(y for _, y in gen)) if gen else None, generalized_step_s_max=float(max(y for _, y in gen)) if gen else None,
                           reps=a.reps, pairs_stopping_apart=0, label=a.label)
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue

            if a.evaluate:
                med = lambda v: float(np.median(v))
                have = hasattr(ctx._lib, "icp_batch_evaluate")
                with ctx.batch(pairs) as bt:
                    if plane:
                        bt.set_model_normals(normals) if normals is not None else bt.estimate_normals()
                    if gate is not None:
                        bt.set_max_distance(gate)
                    if trim is not None:
                        bt.set_trim(trim)
                    if recip:
                        bt.set_reciprocal(True)
                    if robust:
                        bt.set_robust(*robust)

                    def timed(fn):
                        t0 = time.perf_counter()
                        fn()
                        return time.perf_counter() - t0

                    def steps():   # (first step, second step) of a fresh loop
                        bt.begin(max_iter=it, tol=tol, metric=metric)
                        return timed(lambda: bt.run(1)), timed(lambda: bt.run(1))

                    steps()
                    st = [steps() for _ in range(a.reps)]
                    ev, evm = [], []
                    if have:   # where the second step left the clouds
                        bt.evaluate(metric=metric, want_matches=True)   # (allocates the evaluation's buffers)
                        ev = [timed(lambda: bt.evaluate(metric=metric)) for _ in range(a.reps)]
                        evm = [timed(lambda: bt.evaluate(metric=metric, want_matches=True)) for _ in range(a.reps)]
                run_batched()
                tb = [timed(run_batched) for _ in range(a.reps)]
                row = dict(case=name, pairs=len(pairs), points=int(pairs[0][0].shape[0]), batched_s=med(tb), batched_s_min=float(min(tb)),
                           batched_s_max=float(max(tb)), first_step_s=med([x for x, _ in st]), step_s=med([y for _, y in st]),
                           step_s_min=float(min(y for _, y in st)), step_s_max=float(max(y for _, y in st)),
                           evaluate_s=med(ev) if have else None, evaluate_s_min=float(min(ev)) if have else None,
                           evaluate_s_max=float(max(ev)) if have else None, evaluate_matches_s=med(evm) if have else None,
                           reps=a.reps, pairs_stopping_apart=0, max_distance=None if gate is None else str(gate), trim=trim,
                           reciprocal=bool(recip), robust=a.robust or None, label=a.label)
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue

            def batched():
                t0 = time.perf_counter()
                res = run_batched()
                return time.perf_counter() - t0, [r.passes for r in res], None

            def sequential():
                t0 = time.perf_counter()
                res = run_sequential()
                return time.perf_counter() - t0, [r.passes for r in res], sum(r.seconds_total for r in res)

            batched()
            sequential()
            tb, ts, tl = [], [], []
            for _ in range(a.reps):   # alternated, so that both see the same box
                s, pb, _ = batched()
                tb.append(s)
                s, ps, loops = sequential()
                ts.append(s)
                tl.append(loops)
            # the same registrations: every pair must run the same passes on both sides (checked when all rows are out)
            apart = sum(1 for x, y in zip(pb, ps) if x != y) if (gate is None or np.isinf(gate)) and (trim is None or trim == 1.0) and not recip and not robust else 0
            pb, ps = sum(pb), sum(ps)
            mb, ms, ml = float(np.median(tb)), float(np.median(ts)), float(np.median(tl))
            row = dict(case=name, pairs=len(pairs), points=int(pairs[0][0].shape[0]), pair_iterations=pb, sequential_pair_iterations=ps, pairs_stopping_apart=apart,
                       batched_s=mb, sequential_s=ms, sequential_loops_s=ml,
                       batched_pair_it_per_s=pb / mb, sequential_pair_it_per_s=ps / ms,
                       batched_us_per_pair_it=1e6 * mb / pb, sequential_us_per_pair_it=1e6 * ms / ps,
                       sequential_loops_us_per_pair_it=1e6 * ml / ps, speedup=ms / mb, speedup_vs_loops=ml / mb,
                       batched_s_min=float(min(tb)), batched_s_max=float(max(tb)), reps=a.reps,
                       max_distance=None if gate is None else str(gate), trim=trim, reciprocal=bool(recip), robust=a.robust or None, start="init" if a.init else "premoved" if a.premoved else "uploaded",
                       label=a.label)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    differ = [r["case"] for r in rows if r.get("same_bytes", True) is False]
    if differ:
        sys.exit(f"the device's new clouds are not the host path's bytes in: {differ}")
    bad = [r["case"] for r in rows if r["pairs_stopping_apart"]]
    if bad:
        sys.exit(f"batched and sequential registrations ran different passes in: {bad}")


if __name__ == "__main__":
    main()
