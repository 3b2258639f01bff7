"""GPU: every pass's ICP_NMOM moment vector against exact sums, on every route that produces it.

A pass gives the host one thing -- the moment vector -- and the host derives the stop rule and the next (R, t) from it.  The other
suites see that vector only through what is derived (T at 1e-5, the error series at 1e-5).  Here the vector itself, read with
icp_diag_loop_moments / icp_diag_batch_moments, is held to the exact sums over (P_k, Q, idx_k) of the same pass (ref_moments.py:
Python integers, rounded once), slot by slot, at the bound derived there:

    tol_s = 2 (n + 16) 2^-53 A_s      (+ 2^-36 A_s for the four tagged slots of compact rows)

P_k is the cloud pass k was matched on and idx_k its correspondences, both as the device holds them; slot ERR is
sum |P_k - Q[idx_{k-1}]|^2 (exactly 0 for k = 0); CNT is exactly n; SPP / SQQ are exactly 0 where the compact rows leave them
out.  Every test asserts the ICP_ROUTE_* bits of the vectors it reads: a test that fell back to another route proves nothing.
With the vector readable the transform front end is pinned too: P_{k+1} must be BIT-EQUAL to ((r0 x + r1 y) + r2 z) + t, every
operation rounded in the storage precision, with (R, t) = the host solve of that very vector -- in every kernel that moves points
(transform_error_kernel, the front ends of nn_match_row64, nn_match_sparse, the dense kernel and the fp64 kernels, nn_match_batch;
a launch argument, a mailbox message or the batch's control block must all round R, t alike).

Each test prints, per route, the largest |device - exact| / tol_s it saw.
"""
import numpy as np
import pytest

import clouds as cl
import ref_moments as rm
from switches import fresh_context

pytestmark = pytest.mark.gpu

PASSES = 4        # matching passes of a fixed_iterations loop; pass PASSES is the error-only one
RATIO = {}        # route label -> largest |device - exact| / tol seen
_REF = {}         # exact sums are shared by the forms that must reproduce one trajectory


def bits(pkg):
    return pkg.capi


def expect_route(route, must=0, never=0, what=""):
    assert route & must == must and route & never == 0, f"{what}: route bits {route:#05x}, expected all of {must:#05x} and none of {never:#05x}"


def expect_pass_route(pkg, rec, final, must, never, what, form_bits=0):
    """a matching pass: the route the test claims; the loop's last, error-only pass has no moment rows -- its error rows go to the
    host (or through finalize_kernel) whatever the matching passes' route is.  form_bits: ROUTE_ARMED / ROUTE_RESIDENT / 0, exactly"""
    B = pkg.capi
    forms = B.ROUTE_ARMED | B.ROUTE_RESIDENT
    if final:
        # (its error share travels in a compact row only as a message to the resident kernel of a compact route)
        compact = B.ROUTE_COMPACT if (must & B.ROUTE_COMPACT and form_bits & B.ROUTE_RESIDENT) else 0
        expect_route(rec["route"], B.ROUTE_ERROR_ONLY | form_bits | compact,
                     ((B.ROUTE_FUSED_TAIL | B.ROUTE_MOMENTS_KERNEL | forms) & ~form_bits) | (B.ROUTE_COMPACT & ~compact), what)
    else:
        expect_route(rec["route"], must | form_bits, ((never | forms) & ~form_bits) | B.ROUTE_ERROR_ONLY, what)


def _numeric_end(pkg, e):
    return e.code in (pkg.capi.ICP_ERR_SINGULAR, pkg.capi.ICP_ERR_INVALID)


def _record(c, k, failed=False):
    mom, route = c.diag_loop_moments()
    return dict(k=k, P=c.get_moving(), idx=c.get_indices(), mom=mom, route=route, failed=failed)


def _begin(c, pkg, D, M, metric, normals, passes):
    c.set_model(M)
    if metric == pkg.ICP_POINT_TO_PLANE:
        c.set_model_normals(normals)
    c.set_moving(D)
    c.loop_begin(metric, max_iter=passes, tol=0.0, fixed_iterations=True)
    with pytest.raises(pkg.IcpError) as e:   # nothing to read before the first completed pass of a loop
        c.diag_loop_moments()
    assert e.value.code == pkg.capi.ICP_ERR_STATE


def stepwise(c, pkg, D, M, metric, normals=None, passes=PASSES, after_enqueue=None):
    """the trajectory, one icp_loop_enqueue + icp_loop_complete per pass: [dict(k, P, idx, mom, route)].  A minimisation that
    refuses a pass's sums (fewer points than unknowns) ends the loop; that pass's vector is still the one the host received."""
    _begin(c, pkg, D, M, metric, normals, passes)
    out = []
    for k in range(passes + 1):
        c.loop_enqueue()
        seen = after_enqueue() if after_enqueue else None
        try:
            done = c.loop_complete()
        except pkg.IcpError as e:
            assert _numeric_end(pkg, e), e
            out.append(_record(c, k, failed=True))
            break
        out.append(_record(c, k))
        out[-1]["seen"] = seen
        assert done == (k == passes)
    return out


def in_runs(c, pkg, D, M, metric, normals, schedule, passes=PASSES):
    """the same loop driven by icp_loop_run in runs of `schedule` steps: {k: record of the pass the run ended on, "second": it was
    the second pass of its run}"""
    _begin(c, pkg, D, M, metric, normals, passes)
    out, k = {}, -1
    for steps in schedule:
        took, done = c.loop_run(steps)
        assert took == steps
        k += steps
        out[k] = _record(c, k)
        out[k]["second"] = steps >= 2
        assert done == (k == passes)
    return out


def reference(metric_plane, P, Q, Nrm, idx, idx_prev):
    key = (metric_plane, P.tobytes(), idx.tobytes(), None if idx_prev is None else idx_prev.tobytes(), Q.shape[0], P.dtype.str)
    if key not in _REF:
        if len(_REF) > 4096:
            _REF.clear()
        P_new = P if idx_prev is not None else None
        _REF[key] = rm.plane(P, Q, Nrm, idx, P_new, idx_prev) if metric_plane else rm.p2p(P, Q, idx, P_new, idx_prev)
    return _REF[key]


def check_pass(pkg, label, rec, prev, Q, plane=False, Nrm=None, final=False, compact=False):
    """one pass's vector against the exact sums of (P_k, Q, idx_k) and of (P_k, Q, idx_{k-1}).  compact: the TEST's word that this
    pass's rows travel in the compact format (the wider bound on its four tagged slots) -- never the library's own report"""
    P, idx, mom = rec["P"], rec["idx"], rec["mom"]
    if "route" in rec:
        assert bool(rec["route"] & pkg.capi.ROUTE_COMPACT) == compact, f"{label} pass {rec['k']}: route {rec['route']:#05x}, compact rows expected: {compact}"
    n = P.shape[0]
    idx_prev = prev["idx"] if prev is not None else None
    what = f"{label} n={n} m={Q.shape[0]} pass {rec['k']}"
    worst = RATIO.get(label, 0.0)
    if final:   # only the error means anything
        want = rm.sq_error(P, Q, idx_prev)
        tol = rm.tolerance(np.full(rm.NMOM, want), n, compact)[rm.ERR]
        assert abs(mom[rm.ERR] - want) <= tol, f"{what}: ERR {mom[rm.ERR]!r} exact {want!r} tol {tol:.3e}"
        RATIO[label] = max(worst, abs(mom[rm.ERR] - want) / tol if tol > 0 else 0.0)
        return
    want, maj = reference(plane, P, Q, Nrm, idx, idx_prev)
    tol = rm.tolerance(maj, n, compact)
    assert mom[rm.CNT] == float(n), f"{what}: CNT {mom[rm.CNT]!r}"
    if prev is None:
        assert mom[rm.ERR] == 0.0, f"{what}: ERR {mom[rm.ERR]!r} without a transform"
    slots = rm.PLANE_SLOTS if plane else (rm.P2P_COMPACT_SLOTS if compact else rm.P2P_SLOTS)
    for s in (rm.ERR,) + tuple(slots):
        dev = abs(mom[s] - want[s])
        assert dev <= tol[s], f"{what}: slot {s} device {mom[s]!r} exact {want[s]!r} |diff| {dev:.3e} tol {tol[s]:.3e}"
        if tol[s] > 0:
            worst = max(worst, dev / tol[s])
    if compact:   # the header's word: the fast path, whose rows the host adds itself, leaves them 0
        assert mom[rm.SPP] == 0.0 and mom[rm.SQQ] == 0.0, what
    RATIO[label] = worst


def check_transform(pkg, label, rec, nxt, plane=False):
    """P_{k+1} bit-equal to apply_rt(P_k; R_k, t_k) with (R_k, t_k) the host solve of pass k's vector"""
    if plane:
        R, t, _ = pkg.solve_point_to_plane(rec["mom"])
    else:
        R, t = pkg.solve_point_to_point(rec["mom"])
    want = rm.apply_rt(rec["P"], R, t)
    got = nxt["P"]
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.flatnonzero((got.view(np.uint32 if got.dtype == np.float32 else np.uint64) != want.view(np.uint32 if got.dtype == np.float32 else np.uint64)).any(axis=1))
    assert bad.size == 0, f"{label} n={got.shape[0]} pass {rec['k']} -> {nxt['k']}: {bad.size} moved points differ in their bits, first {bad[:4]}: {got[bad[:2]]!r} vs {want[bad[:2]]!r}"


def check_trajectory(pkg, label, traj, Q, must, never, plane=False, Nrm=None, passes=PASSES):
    """a step-wise trajectory (icp_loop_enqueue / icp_loop_complete: neither armed nor resident)"""
    assert len(traj) >= 1
    for k, rec in enumerate(traj):
        final = k == passes
        expect_pass_route(pkg, rec, final, must, never, f"{label} n={rec['P'].shape[0]} pass {k}")
        check_pass(pkg, label, rec, traj[k - 1] if k else None, Q, plane, Nrm, final, compact=bool(must & pkg.capi.ROUTE_COMPACT) and not final)
        if k + 1 < len(traj):
            check_transform(pkg, label, rec, traj[k + 1], plane)
    assert traj[-1]["failed"] or len(traj) == passes + 1


def report(*labels):
    for lb in labels:
        if lb in RATIO:
            print(f"[moments] {lb}: largest |device - exact| / tol = {RATIO[lb]:.4f}")


def normals_of(orc, M):
    return orc.normals(M, orc.knn4(M))[0]


# ---- 1. compact rows: rows of 64 / of 128, the AVX and the scalar adder, every loop form ---------------------------------------
COMPACT = {
    "row64": ({}, cl.ROW64_N),
    "row64_scalar_adder": ({"ICP_MAILBOX": "plain"}, cl.ROW64_N),
    "row128": ({"ICP_NN_ROW": "128"}, cl.ROW128_N),
    "row128_w8": ({"ICP_NN_ROW": "128", "ICP_NN_WAVES128": "8"}, cl.ROW128_N),
    "row128_w4_hier": ({"ICP_NN_ROW": "128", "ICP_NN_WAVES128": "4", "ICP_NN_HIER": "1"}, cl.ROW128_N),
}
# (a plan with shared rows -- 8-wave blocks -- runs armed launches unless told otherwise: ICP_RESIDENT=2)
FORMS = {"resident": {}, "armed": {"ICP_RESIDENT": "0"}, "stepwise": {"ICP_RESIDENT": "0", "ICP_ARMED": "0"}}
SCHEDULES = ((2, 2, 1), (1, 2, 2))   # every pass 0 .. PASSES ends a run once; passes 1, 2, 3 are once the second pass of a run


def run_forms_against(c, pkg, label, form, base, D, M, metric, Nrm, plane, must, never):
    """the loop in runs of icp_loop_run: the same clouds and matches as the step-wise trajectory, bit for bit, every observed
    vector within its bound of the exact sums, and produced by the form the test claims"""
    B = bits(pkg)
    if base[-1]["failed"]:
        return
    for schedule in SCHEDULES:
        got = in_runs(c, pkg, D, M, metric, Nrm, schedule)
        for k, rec in got.items():
            what = f"{label}/{form} n={D.shape[0]} m={M.shape[0]} runs {schedule} pass {k}"
            assert rec["P"].tobytes() == base[k]["P"].tobytes() and rec["idx"].tobytes() == base[k]["idx"].tobytes(), f"{what}: not the step-wise trajectory"
            final = k == PASSES
            form_bits = B.ROUTE_RESIDENT if form == "resident" else B.ROUTE_ARMED if (form == "armed" and rec["second"] and not final) else 0
            expect_pass_route(pkg, rec, final, must, never, what, form_bits)
            compact = bool(must & B.ROUTE_COMPACT) and (not final or form == "resident")
            check_pass(pkg, f"{label}/{form}", rec, base[k - 1] if k else None, M, plane, Nrm, final, compact)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", list(COMPACT))
def test_compact_rows(pkg, monkeypatch, variant, form):
    B = bits(pkg)
    env, sizes = COMPACT[variant]
    env = dict(env, **FORMS[form])
    if variant == "row128_w8" and form == "resident":
        env["ICP_RESIDENT"] = "2"
    avx = 0 if "ICP_MAILBOX" in env else B.ROUTE_AVX
    must = B.ROUTE_HOST_ROWS | B.ROUTE_COMPACT | B.ROUTE_FUSED_TAIL | avx
    never = B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | B.ROUTE_MOMENTS_KERNEL | (B.ROUTE_AVX if not avx else 0)
    label = f"compact/{variant}"
    with fresh_context(pkg, monkeypatch, env) as c:
        for m in cl.MODEL_M:
            for n in sizes:
                D, M = cl.case_pair(n, m)
                base = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_POINT)
                check_trajectory(pkg, label, base, M, must, never)
                run_forms_against(c, pkg, label, form, base, D, M, pkg.ICP_POINT_TO_POINT, None, False, must, never)
    report(label, f"{label}/{form}")


# ---- 2. sorted views: the Morton / Hilbert views permute slots ------------------------------------------------------------------
@pytest.mark.parametrize("sort", ["1", "0"])
@pytest.mark.parametrize("row", ["64", "128"])
def test_compact_rows_sorted_views(pkg, monkeypatch, capfd, row, sort):
    """ICP_SORT=1 puts every cloud of more points than one group (a row of the moving cloud -- judged from 129 points up --, an
    8-point chunk of the model) on its curve-ordered view, ICP_SORT=0 forbids the views.  That the views really are (not) in use is
    read from the set-up's own account of its order decisions (ICP_TRACE=1, stderr): a silent fall-back to the cloud's own order
    would make this the default test.  Permuted here: the moving clouds of 130 and 1000 / 129, 191 and 1200 points, both models."""
    import re
    B = bits(pkg)
    must = B.ROUTE_HOST_ROWS | B.ROUTE_COMPACT | B.ROUTE_FUSED_TAIL | B.ROUTE_AVX
    never = B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | B.ROUTE_MOMENTS_KERNEL
    label = f"compact/row{row}_sort{sort}"
    decision = re.compile(r"(\d+) points, groups of (\d+):.*-> (sorted view|Morton view|own order)")
    permuted = 0
    with fresh_context(pkg, monkeypatch, {"ICP_NN_ROW": row, "ICP_SORT": sort, "ICP_TRACE": "1"}) as c:
        for m in cl.MODEL_M:
            for n in (cl.ROW64_N if row == "64" else cl.ROW128_N):
                D, M = cl.case_pair(n, m)
                capfd.readouterr()
                base = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_POINT)
                said = decision.findall(capfd.readouterr().err)
                assert any(int(cnt) == m for cnt, _, _ in said), said
                for cnt, grp, how in said:
                    assert (how != "own order") == (sort == "1" and int(cnt) > int(grp)), (n, m, said)
                if n > 128:   # (smaller moving clouds are not judged: one row, nothing to order)
                    assert any(int(cnt) == n and int(grp) == int(row) for cnt, grp, _ in said), (n, m, said)
                    permuted += sort == "1"
                check_trajectory(pkg, label, base, M, must, never)
                run_forms_against(c, pkg, label, "resident", base, D, M, pkg.ICP_POINT_TO_POINT, None, False, must, never)
    assert permuted == (0 if sort == "0" else 2 * (2 if row == "64" else 3))
    report(label, f"{label}/resident")


# ---- 3. full rows to the host: point-to-plane (28 sums) and every fp64 form -------------------------------------------------------
@pytest.mark.parametrize("row", ["64", "128"])
def test_full_rows_point_to_plane(pkg, orc, monkeypatch, row):
    B = bits(pkg)
    must = B.ROUTE_HOST_ROWS | B.ROUTE_FUSED_TAIL | B.ROUTE_AVX
    never = B.ROUTE_COMPACT | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | B.ROUTE_MOMENTS_KERNEL
    label = f"full/plane_row{row}"
    with fresh_context(pkg, monkeypatch, {"ICP_NN_ROW": row}) as c:
        for m in cl.MODEL_M:
            for n in (cl.ROW64_N if row == "64" else cl.ROW128_N):
                D, M = cl.case_pair(n, m)
                Nrm = normals_of(orc, M)
                base = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_PLANE, Nrm)
                check_trajectory(pkg, label, base, M, must, never, plane=True, Nrm=Nrm)
                run_forms_against(c, pkg, label, "resident", base, D, M, pkg.ICP_POINT_TO_PLANE, Nrm, True, must, never)
    report(label, f"{label}/resident")


@pytest.mark.parametrize("sparse", ["1", "0"])
def test_full_rows_fp64(pkg, monkeypatch, sparse):
    """ICP_F64_SPARSE=1: rows of 64 with a fused tail (nn_match_row64_f64); =0: the dense kernel + moments_kernel<double> and the
    stand-alone transform_error_kernel<double>"""
    B = bits(pkg)
    kernel = B.ROUTE_FUSED_TAIL if sparse == "1" else B.ROUTE_MOMENTS_KERNEL
    must = B.ROUTE_HOST_ROWS | B.ROUTE_AVX | kernel
    never = B.ROUTE_COMPACT | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | ((B.ROUTE_FUSED_TAIL | B.ROUTE_MOMENTS_KERNEL) & ~kernel)
    label = f"full/fp64_sparse{sparse}"
    with fresh_context(pkg, monkeypatch, {"ICP_F64_SPARSE": sparse}) as c:
        for m in cl.MODEL_M:
            for n in cl.ROW64_N:
                D, M = cl.case_pair(n, m, np.float64)
                base = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_POINT)
                check_trajectory(pkg, label, base, M, must, never)
                if base[-1]["failed"]:
                    continue
                for schedule in SCHEDULES:   # icp_loop_run, whichever form it takes for this plan: the same trajectory
                    for k, rec in in_runs(c, pkg, D, M, pkg.ICP_POINT_TO_POINT, None, schedule).items():
                        assert rec["P"].tobytes() == base[k]["P"].tobytes() and rec["idx"].tobytes() == base[k]["idx"].tobytes()
                        expect_pass_route(pkg, rec, k == PASSES, must, never, f"{label} runs {schedule} pass {k}", rec["route"] & (B.ROUTE_ARMED | B.ROUTE_RESIDENT))
                        check_pass(pkg, f"{label}/loop_run", rec, base[k - 1] if k else None, M, final=(k == PASSES))
    report(label, f"{label}/loop_run")


@pytest.mark.parametrize("sparse", ["1", "0"])
def test_full_rows_fp64_point_to_plane(pkg, orc, monkeypatch, sparse):
    """the 28 sums of the single-pair fp64 routes: ICP_F64_SPARSE=1, the TAIL == 2 branch of nn_match_row64_f64; =0, the dense kernel
    + moments_kernel<double, POINT_TO_PLANE>.  Normals: the fp32 model's oracle normals cast to double, as the batch test takes them.
    A cloud of one or two points has six unknowns: its loop may end ICP_ERR_SINGULAR after the first vector (stepwise() keeps that
    vector)."""
    B = bits(pkg)
    kernel = B.ROUTE_FUSED_TAIL if sparse == "1" else B.ROUTE_MOMENTS_KERNEL
    must = B.ROUTE_HOST_ROWS | B.ROUTE_AVX | kernel
    never = B.ROUTE_COMPACT | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | ((B.ROUTE_FUSED_TAIL | B.ROUTE_MOMENTS_KERNEL) & ~kernel)
    label = f"full/fp64_plane_sparse{sparse}"
    with fresh_context(pkg, monkeypatch, {"ICP_F64_SPARSE": sparse}) as c:
        for m in cl.MODEL_M:
            for n in cl.ROW64_N:
                D, M = cl.case_pair(n, m, np.float64)
                Nrm = normals_of(orc, cl.case_pair(n, m)[1]).astype(np.float64)
                base = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_PLANE, Nrm)
                assert base[0]["P"].dtype == np.float64
                check_trajectory(pkg, label, base, M, must, never, plane=True, Nrm=Nrm)   # (P_{k+1} = apply_rt of the solve of pass k's vector, bit for bit)
                assert n < 63 or not base[-1]["failed"], (n, m)   # (one or two points: six unknowns; the batch test draws the same line)
                if base[-1]["failed"]:
                    continue
                for schedule in SCHEDULES:   # icp_loop_run, whichever form it takes for this plan: the same trajectory
                    for k, rec in in_runs(c, pkg, D, M, pkg.ICP_POINT_TO_PLANE, Nrm, schedule).items():
                        assert rec["P"].tobytes() == base[k]["P"].tobytes() and rec["idx"].tobytes() == base[k]["idx"].tobytes()
                        expect_pass_route(pkg, rec, k == PASSES, must, never, f"{label} runs {schedule} pass {k}", rec["route"] & (B.ROUTE_ARMED | B.ROUTE_RESIDENT))
                        check_pass(pkg, f"{label}/loop_run", rec, base[k - 1] if k else None, M, plane=True, Nrm=Nrm, final=(k == PASSES))
    report(label, f"{label}/loop_run")


# ---- 4. rows left on the device and added by finalize_kernel (an external moments buffer) ------------------------------------------
def with_external_buffer(c, pkg, fn):
    """fn(read) with the loop's vector in a torch tensor; read() = the tensor's content once everything enqueued has run"""
    import torch
    ext = torch.zeros(pkg.ICP_NMOM, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    def read():
        torch.cuda.synchronize()   # (the whole device: the context's stream is its own)
        return ext.cpu().numpy().copy()

    c.loop_set_moments_dev(ext.data_ptr())
    try:
        return fn(read)
    finally:
        c.loop_set_moments_dev(0)


def check_seen_on_device(label, traj):
    """what the tensor held after icp_loop_enqueue is what icp_loop_complete copied back: slots 0 .. 30, bit for bit"""
    for rec in traj:
        if rec.get("seen") is not None:
            assert rec["seen"][:rm.NMOM - 1].tobytes() == rec["mom"][:rm.NMOM - 1].tobytes(), f"{label} n={rec['P'].shape[0]} pass {rec['k']}"


@pytest.mark.parametrize("metric", ["point_to_point", "point_to_plane"])
def test_device_rows_finalize_kernel(pkg, orc, monkeypatch, metric):
    B = bits(pkg)
    plane = metric == "point_to_plane"
    must = B.ROUTE_FIN_KERNEL | B.ROUTE_FUSED_TAIL
    never = B.ROUTE_HOST_ROWS | B.ROUTE_COMPACT | B.ROUTE_AVX | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_TWO_STAGE | B.ROUTE_MOMENTS_KERNEL
    label = f"device_rows/finalize_kernel_{metric}"
    with fresh_context(pkg, monkeypatch, {}) as c:
        for m in cl.MODEL_M:
            for n in cl.ROW64_N:
                D, M = cl.case_pair(n, m)
                Nrm = normals_of(orc, M) if plane else None
                met = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
                traj = with_external_buffer(c, pkg, lambda read: stepwise(c, pkg, D, M, met, Nrm, after_enqueue=read))
                check_seen_on_device(label, traj)
                # (the final pass adds the transform's error rows with the same kernel)
                for rec in traj:
                    expect_route(rec["route"], B.ROUTE_FIN_KERNEL, 0, label)
                check_trajectory(pkg, label, traj, M, must, never, plane=plane, Nrm=Nrm)
    report(label)


# ---- 5. rows added up inside the matching launch (fin_close): ragged last groups ----------------------------------------------------
@pytest.mark.parametrize("where", ["pinned", "device_vector"])
@pytest.mark.parametrize("metric", ["point_to_point", "point_to_plane"])
def test_in_launch_finalize(pkg, orc, monkeypatch, metric, where):
    """ICP_NN_ROW=128 ICP_HOST_ROWS_MAX=4: the launch adds its rows up in ~sqrt(rows) groups.  The rows include those of the padding
    (clouds.FIN_N), which are all zeros and come last.  1000 points = 8 rows, all real, in groups of 3, 3, 2 and 3000 = 24 rows, all
    real, in 5, 5, 5, 5, 4: the short last group carries the cloud's last points, so a lost last row, last group or half of it
    shows.  640 and 1200 points (8 and 16 rows, 5 and 10 of them real) end in the middle of a group, with padding behind."""
    B = bits(pkg)
    plane = metric == "point_to_plane"
    pinned = where == "pinned"
    must = B.ROUTE_FIN_LAUNCH | B.ROUTE_FUSED_TAIL | (B.ROUTE_FIN_PINNED if pinned else 0)
    never = B.ROUTE_HOST_ROWS | B.ROUTE_COMPACT | B.ROUTE_AVX | B.ROUTE_FIN_KERNEL | B.ROUTE_MOMENTS_KERNEL | (0 if pinned else B.ROUTE_FIN_PINNED)
    label = f"in_launch_finalize/{where}_{metric}"
    met = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    with fresh_context(pkg, monkeypatch, {"ICP_NN_ROW": "128", "ICP_HOST_ROWS_MAX": "4"}) as c:
        for m in cl.MODEL_M:
            for n in cl.FIN_N:
                D, M = cl.case_pair(n, m)
                Nrm = normals_of(orc, M) if plane else None
                if pinned:
                    traj = stepwise(c, pkg, D, M, met, Nrm)
                else:
                    traj = with_external_buffer(c, pkg, lambda read: stepwise(c, pkg, D, M, met, Nrm, after_enqueue=read))
                    check_seen_on_device(label, traj)
                info = c.nn_launch_info()
                assert info["blocks"] == 8 * ((n + 1023) // 1024) and info["splits"] == 1, info   # the rows the groups are cut from
                # (the error-only pass has no matching launch to add anything up in: its rows go the plain way)
                check_trajectory(pkg, label, traj, M, must, never, plane=plane, Nrm=Nrm)
                if pinned and not traj[-1]["failed"]:   # such a pass can be armed ahead like any other (and is never resident)
                    for schedule in SCHEDULES:
                        for k, rec in in_runs(c, pkg, D, M, met, Nrm, schedule).items():
                            assert rec["P"].tobytes() == traj[k]["P"].tobytes() and rec["idx"].tobytes() == traj[k]["idx"].tobytes()
                            armed = B.ROUTE_ARMED if (rec["second"] and k != PASSES) else 0
                            expect_pass_route(pkg, rec, k == PASSES, must, never, f"{label} runs {schedule} pass {k}", armed)
                            check_pass(pkg, f"{label}/loop_run", rec, traj[k - 1] if k else None, M, plane, Nrm, k == PASSES)
    report(label, f"{label}/loop_run")


# ---- 6. the two-kernel form (moments_kernel) and the dense kernel -----------------------------------------------------------------
TWO_KERNEL = {
    "sparse_two_kernel": {"ICP_FUSED_TAIL": "0"},
    "dense_fused_tail": {"ICP_NN_SPARSE": "0"},
    "dense_two_kernel": {"ICP_NN_SPARSE": "0", "ICP_FUSED_TAIL": "0"},
}


@pytest.mark.parametrize("metric", ["point_to_point", "point_to_plane"])
@pytest.mark.parametrize("form", list(TWO_KERNEL))
def test_two_kernel_form_and_dense_kernel(pkg, orc, monkeypatch, form, metric):
    """(the switches are read by icp_create, so a fresh context of this process takes them: no child process is needed)"""
    B = bits(pkg)
    plane = metric == "point_to_plane"
    kernel = B.ROUTE_FUSED_TAIL if form == "dense_fused_tail" else B.ROUTE_MOMENTS_KERNEL
    must = B.ROUTE_HOST_ROWS | B.ROUTE_AVX | kernel
    never = B.ROUTE_COMPACT | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | ((B.ROUTE_FUSED_TAIL | B.ROUTE_MOMENTS_KERNEL) & ~kernel)
    label = f"two_kernel/{form}_{metric}"
    met = pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT
    with fresh_context(pkg, monkeypatch, TWO_KERNEL[form]) as c:
        for m in cl.MODEL_M:
            for n in cl.ROW64_N:
                D, M = cl.case_pair(n, m)
                Nrm = normals_of(orc, M) if plane else None
                traj = stepwise(c, pkg, D, M, met, Nrm)
                check_trajectory(pkg, label, traj, M, must, never, plane=plane, Nrm=Nrm)
    report(label)


def test_moments_kernel_past_its_block_cap(pkg, monkeypatch):
    """64 * 1024 + 65 points: moments_kernel's 1024 blocks take a second, ragged trip of their grid-stride loop (blocks 0 and 1)"""
    B = bits(pkg)
    must = B.ROUTE_HOST_ROWS | B.ROUTE_AVX | B.ROUTE_MOMENTS_KERNEL
    never = B.ROUTE_COMPACT | B.ROUTE_FIN_LAUNCH | B.ROUTE_FIN_KERNEL | B.ROUTE_FUSED_TAIL
    label = "two_kernel/past_block_cap"
    D, M = cl.case_pair(cl.CAP_N, 17)
    with fresh_context(pkg, monkeypatch, {"ICP_FUSED_TAIL": "0"}) as c:
        traj = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_POINT, passes=2)
    assert (D.shape[0] + 63) // 64 > 1024
    check_trajectory(pkg, label, traj, M, must, never, passes=2)
    report(label)


# ---- 7. the two-stage finalize (more than 2048 rows on the device, not added up inside the launch) -----------------------------------
def test_two_stage_finalize(pkg, monkeypatch):
    """launch_finalize takes finalize_ranges_kernel + finalize_kernel for more than 2048 rows.  Rows of 128 points add themselves
    up inside the launch from host_rows_max + 1 rows on, and moments_kernel never leaves more than 1024 rows: what reaches the two
    stages is the fused tail of rows of 64 points (nn_match_row64 has no in-launch finalize) on a cloud of more than
    64 * 2048 points -- ICP_NN_ROW=64 keeps such a cloud on rows of 64.  More than 1024 rows are never added by the host, so no
    external buffer or communicator is needed.  64 * 2064 - 5 points fill all 2064 rows of the padded cloud: 229 ranges of 9 rows,
    a short last range of 3 (rows 2061-2063, the last one 59 points) and 26 empty ranges -- the ragged end carries real points."""
    B = bits(pkg)
    must = B.ROUTE_FIN_KERNEL | B.ROUTE_FIN_TWO_STAGE | B.ROUTE_FUSED_TAIL
    never = B.ROUTE_HOST_ROWS | B.ROUTE_COMPACT | B.ROUTE_AVX | B.ROUTE_FIN_LAUNCH | B.ROUTE_MOMENTS_KERNEL
    label = "device_rows/two_stage_finalize"
    D, M = cl.case_pair(cl.TWO_STAGE_N, 17)
    with fresh_context(pkg, monkeypatch, {"ICP_NN_ROW": "64"}) as c:
        traj = stepwise(c, pkg, D, M, pkg.ICP_POINT_TO_POINT, passes=2)
        assert c.nn_launch_info()["blocks"] == 2064 == (D.shape[0] + 63) // 64
    check_trajectory(pkg, label, traj, M, must, never, passes=2)
    report(label)


# ---- 8. the batch kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_moments(ctx, pkg, dtype):
    label = f"batch/{np.dtype(dtype).name}"
    pairs = [cl.case_pair(n, m, dtype) for m in cl.MODEL_M for n in cl.BATCH_N]
    checked = [0] * len(pairs)
    with ctx.batch(pairs) as bt:
        bt.begin(max_iter=PASSES, tol=0.0, fixed_iterations=True)
        with pytest.raises(pkg.IcpError) as e:
            bt.diag_moments(0)
        assert e.value.code == pkg.capi.ICP_ERR_STATE
        prev = [None] * len(pairs)
        for k in range(PASSES + 1):
            running = ~bt.done()
            took, _ = bt.run(1)
            assert took == (1 if running.any() else 0)
            moving, idx = bt.get_moving(), bt.get_indices()
            for b in np.flatnonzero(running):
                rec = dict(k=k, P=moving[b], idx=idx[b], mom=bt.diag_moments(b))
                check_pass(pkg, label, rec, prev[b], pairs[b][1], final=(k == PASSES))
                if prev[b] is not None:
                    check_transform(pkg, label, prev[b], rec)
                prev[b] = rec
                checked[b] += 1
        assert bt.done().all()
        for b in range(len(pairs)):
            st = bt.state(b)
            assert checked[b] == PASSES + 1 or st["status"] != pkg.capi.ICP_OK, (b, checked[b], st["status"])
            assert checked[b] >= 1
    report(label)
