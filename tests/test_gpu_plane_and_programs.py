"""GPU: point-to-plane front end and loop against the oracle, and the three reference-named executables."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-point-cloud-registration-with-gpus_amd", "bin")


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _clouds(pkg, golden, which):
    if which == "grid":
        D = pkg.datasets.synthetic_grid(40, np.float32)
        return D, pkg.datasets.make_model_gpu(D, *pkg.datasets.P2P_GPU)
    if which == "random":
        rng = np.random.default_rng(17)
        D = rng.standard_normal((1500, 3)).astype(np.float32)
        return D, pkg.datasets.make_model_gpu(D, (0.05, -0.04, 0.03), (0.02, -0.01, 0.03))
    B = np.fromfile(os.path.join(golden, "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    return B, pkg.datasets.make_model_gpu(B, *pkg.datasets.BUNNY)


# ---------------------------------------------------------------------------------------------------
# kNN(4) + normals  (src/CUDA/GPU_point_to_plane_real.cu:54-188,413-423 / CPU_ICP_point_to-plane.cpp:184-275)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grid", "random", "bunny"])
def test_knn4_neighbours_bit_exact(ctx, pkg, orc, golden, which):
    _, M = _clouds(pkg, golden, which)
    ctx.set_model(M)
    _, nbr = ctx.estimate_normals(want_neighbours=True)
    assert np.array_equal(nbr, orc.knn4(M))


def test_knn4_with_coincident_points(ctx, pkg, orc, golden):
    _, Q = orc.hall_clouds(golden)          # 4361 model points coincide: rank order among equal distances
    ctx.set_model(Q)
    _, nbr = ctx.estimate_normals(want_neighbours=True)
    assert np.array_equal(nbr, orc.knn4(Q))


# fraction of model points whose normal is DEFINED (the two smallest eigenvalues of the neighbourhood covariance are
# separated by more than 1e-3 of the largest): measured from the oracle's covariances -- grid 40x40 0.9625, Bunny_res
# 1.0, hall 0.7175 (another 0.266 of the hall points are the 4361 no-return points at the origin, whose four nearest
# neighbours coincide with them: zero covariance, every direction is an eigenvector).  The gate sits just below.
NORMAL_DEFINED_MIN = {"grid": 0.95, "bunny": 0.99, "hall": 0.70}


@pytest.mark.parametrize("which", ["grid", "bunny", "hall"])
def test_normals_match_oracle_up_to_sign(ctx, pkg, orc, golden, which):
    M = orc.hall_clouds(golden)[1] if which == "hall" else _clouds(pkg, golden, which)[1]
    ctx.set_model(M)
    nrm, nbr = ctx.estimate_normals(want_neighbours=True)
    assert np.array_equal(nbr, orc.knn4(M))
    want, A = orc.normals(M, nbr)
    Af = A.reshape(-1, 3, 3).astype(np.float64)
    Af = np.triu(Af) + np.transpose(np.triu(Af, 1), (0, 2, 1))
    w = np.linalg.eigvalsh(Af)
    scale = np.maximum(np.abs(w).max(1), 1e-30)
    # (1) EVERY point: the vector is a unit eigenvector of the eigenvalue of smallest magnitude -- checked through its
    # Rayleigh quotient, which does not care which vector of a degenerate eigenspace was picked, and its residual
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1.0).max() < 1e-5
    w_min = w[np.arange(len(w)), np.abs(w).argmin(1)]
    ray = np.einsum("ni,nij,nj->n", n64, Af, n64)
    assert (np.abs(ray - w_min) <= 1e-5 * scale + 1e-12).all()
    resid = np.linalg.norm(np.einsum("nij,nj->ni", Af, n64) - ray[:, None] * n64, axis=1)
    assert (resid <= 1e-4 * scale + 1e-12).all()
    # (2) where the direction is defined it is the oracle's, up to sign; the share of such points is asserted
    ok = (w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30)
    assert ok.mean() >= NORMAL_DEFINED_MIN[which], ok.mean()
    dots = np.abs((nrm * want).sum(1))
    assert np.abs(dots[ok] - 1.0).max() < 1e-4
    # (3) zero covariance (coincident neighbourhood): both sides fall back to the same axis
    zero = np.abs(Af).max((1, 2)) == 0
    if zero.any():
        assert np.abs(np.abs((nrm[zero] * want[zero]).sum(1)) - 1.0).max() < 1e-6


# ---------------------------------------------------------------------------------------------------
# point-to-plane minimisation and loop  (src/ICP_point_to_plane.cu:517-631)
# ---------------------------------------------------------------------------------------------------
TOL_T = 1e-5      # relative, composed 4x4 transform (BASELINE.json north_star)
TOL_E = 1e-5      # absolute, RMS error series


def assert_same_plane_run(res, want, tol, length=1.0):
    """the gate of the point-to-point loops (tests/test_gpu_parity.py, assert_same_run): error series and composed
    transform within 1e-5, the same iteration count -- one apart only if the deciding |dE| (or E) sits within 5e-7 of
    the stop threshold, where the last bits of a sum may decide.  length: the unit of clouds scaled by it (the error is a
    length, its two absolute gates are in that unit; tests/test_gpu_knn_normals.py)"""
    n = min(len(res.err), len(want["err"]))
    assert np.abs(np.asarray(res.err)[:n] - want["err"][:n]).max() < TOL_E * length
    if res.iterations != want["iterations"]:
        assert abs(res.iterations - want["iterations"]) == 1, (res.iterations, want["iterations"])
        k = min(res.iterations, want["iterations"]) + 1
        dE = abs(want["err"][k] - want["err"][k - 1])
        assert abs(dE - tol) < 5e-7 * length or abs(want["err"][k] - tol) < 5e-7 * length, f"stop rule disagreed away from the threshold: dE={dE}"
    else:
        assert rel(res.T, want["T"]) < TOL_T


@pytest.mark.parametrize("which", ["grid", "bunny"])
def test_point_to_plane_single_pass(ctx, pkg, orc, golden, which):
    D, M = _clouds(pkg, golden, which)
    normals, _ = orc.normals(M, orc.knn4(M))
    res = ctx.point_to_plane(D, M, normals=normals, max_iter=1, tol=1e-6)
    idx = orc.nn(D, M)
    assert res.passes == 1 and np.array_equal(res.idx, idx)
    # the same statements in the same precision (fp64 sums of fp64 terms, fp64 solve): the same 6x6 system, the same motion
    rc, R, t, Cm, b = orc.p2plane_minimize_f32x(D, M, idx, normals)
    assert rc == 0
    assert rel(res.T[:3, :3], R) < 1e-6 and np.abs(res.T[:3, 3] - t).max() < 1e-6 * max(1.0, np.abs(t).max())
    # float terms summed in double (the oracle's other variant): float noise of the terms only
    rc, R, t, Cm, b = orc.p2plane_minimize(D, M, idx, normals, accumulate_f64=True)
    assert rc == 0
    assert rel(res.T[:3, :3], R) < 1e-5 and np.abs(res.T[:3, 3] - t).max() < 1e-5 * max(1.0, np.abs(t).max())
    # the letter-faithful twin accumulates C and b in float: agreement inside its noise band
    rc, Rf, tf, _, _ = orc.p2plane_minimize(D, M, idx, normals, accumulate_f64=False)
    assert rc == 0 and rel(res.T[:3, :3], Rf) < 2e-3


@pytest.mark.parametrize("which", ["grid", "bunny"])
def test_point_to_plane_loop(ctx, pkg, orc, golden, which):
    D, M = _clouds(pkg, golden, which)
    normals, _ = orc.normals(M, orc.knn4(M))
    res = ctx.point_to_plane(D, M, normals=normals, max_iter=50, tol=1e-6)
    # tight: fp32 matching + fp64 minimisation, the arithmetic the product uses (oracle/icp_oracle.c, orc_icp_p2plane_f32x)
    want = orc.icp_p2plane_f32x(D, M, normals, 50, 1e-6)
    assert_same_plane_run(res, want, 1e-6)
    assert np.array_equal(res.idx, want["idx"]) or res.iterations != want["iterations"]
    # the letter-faithful fp32 twin (float accumulators, float error norm; CPU_ICP_point_to-plane.cpp) and its variant
    # with double accumulators: the three oracle loops agree among themselves to 1e-7 in T and 3e-6 in E on these
    # clouds (measured), so the same 1e-5 gate holds against each of them
    for acc64 in (True, False):
        twin = orc.icp_p2plane(D, M, normals, 50, 1e-6, accumulate_f64=acc64)
        assert_same_plane_run(res, twin, 1e-6)
    assert res.err[-1] < 0.5 * res.err[1]                     # and it actually converges
    # normals estimated on the device give the same registration (sign of a normal does not matter)
    res2 = ctx.point_to_plane(D, M, normals=None, max_iter=50, tol=1e-6)
    assert rel(res2.T, res.T) < 5e-3


def test_point_to_plane_degenerate_is_reported(ctx, pkg):
    # all normals parallel and the cloud planar: the 6x6 system is singular -> ICP_ERR_SINGULAR, not garbage
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([g, np.zeros((64, 1))], 1).astype(np.float32)
    N = np.tile(np.array([[0, 0, 1]], dtype=np.float32), (64, 1))
    with pytest.raises(pkg.IcpError) as e:
        ctx.point_to_plane(P, P, normals=N, max_iter=3)
    assert e.value.code == pkg.capi.ICP_ERR_SINGULAR


# ---------------------------------------------------------------------------------------------------
# the executables keep the reference's stdout format and numbers
# ---------------------------------------------------------------------------------------------------
def _errors(stdout):
    body = stdout.split("Error:\n", 1)[1]
    vals = []
    for line in body.splitlines():
        m = re.match(r"^(\d+): (-?\d+\.\d{4})$", line)
        if not m:
            break
        assert int(m.group(1)) == len(vals) + 1
        vals.append(float(m.group(2)))
    return np.array(vals)


def _transform(stdout):
    rows = stdout.split("Transform (row-major 4x4, moving -> model):\n", 1)[1].splitlines()[:4]
    return np.array([[float(x) for x in r.split()] for r in rows])


def test_icp_standard_program(pkg, orc):
    r = subprocess.run([os.path.join(BIN, "icp_standard"), "--transform"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.match(r"^Grid Size: \d+, Block Size: \d+\n", r.stdout)           # src/ICP_standard.cu:358
    assert re.search(r"\nElapsed time: \d+\.\d+ ms\n", r.stdout)               # :475
    err = _errors(r.stdout)
    assert len(err) == 40                                                      # fixed 40 passes, :19,369
    D, M = orc.synth_icp_standard(32)
    want = orc.icp_p2p_f32x(D, M, 40, 0.0, fixed=True)
    assert np.abs(err - want["err"][1:41]).max() < 1.5e-4                      # 4 printed decimals
    assert rel(_transform(r.stdout), want["T"]) < 1e-5


def test_icp_point_to_point_program_bunny_and_hall(pkg, orc, golden, tmp_path):
    B = np.fromfile(os.path.join(golden, "bunny_res_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    txt = tmp_path / "Bunny_res.csv"
    with open(txt, "w", newline="") as f:
        for p in B:
            f.write("%.9g %.9g %.9g\r\n" % tuple(p))
    r = subprocess.run([os.path.join(BIN, "ICP_point_to_point"), "--bunny", str(txt), "--transform"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "ICP converged successfully!" in r.stdout
    M = pkg.datasets.make_model_gpu(B, *pkg.datasets.BUNNY)
    want = orc.icp_p2p_f32x(B, M, 100, 1e-6)
    err = _errors(r.stdout)
    assert abs(len(err) - (want["iterations"] + 1)) <= 1 and err[0] == 0.0
    k = min(len(err), want["iterations"] + 1)
    assert np.abs(err[:k] - want["err"][:k]).max() < 1.5e-4
    assert rel(_transform(r.stdout), want["T"]) < 1e-5

    # hall: rebuild a raw 64-packet OS1 dump around the fixture ranges and feed it through the program
    ranges = np.fromfile(os.path.join(golden, "hall_ranges_u32.bin"), dtype=np.uint32)
    enc = json.load(open(os.path.join(golden, "hall_meta.json")))["encoder_count0"]
    pk = np.zeros(64 * 12608, dtype=np.uint8)
    pk[12], pk[13] = enc & 0xFF, (enc >> 8) & 0xFF
    o = 0
    for p in range(64):
        for blk in range(16):
            base = p * 12608 + blk * 788 + 16
            for ch in range(2, 64, 4):
                w = base + 12 * ch
                v = int(ranges[o]); o += 1
                pk[w], pk[w + 1], pk[w + 2] = v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0x0F
    raw = tmp_path / "Donut_1024x16.bin"
    pk.tofile(raw)
    r = subprocess.run([os.path.join(BIN, "ICP_point_to_point"), "--hall", str(raw), os.path.join(golden, "beam_intrinsics.csv"),
                        "--transform"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the report of src/CUDA/GPU_point_to_point_real.cu:386-403, line by line: `iteration + 1` and four phase lines
    m = re.search(r"\nThe ICP algorithm was computed in (\d+\.\d{4}) ms with (\d+) iterations\n\n", r.stdout)
    assert m, r.stdout[-800:]
    phases = {}
    for name in ("matching", "minimization", "transformation", "error estimation"):
        ph = re.search(r"The %s step represents the (\d+\.\d{4})%% of the total time with (\d+\.\d{4}) ms\n\n" % name, r.stdout)
        assert ph, f"missing the {name} line:\n" + r.stdout[-800:]
        phases[name] = (float(ph.group(1)), float(ph.group(2)))
    order = [r.stdout.index("The %s step" % n) for n in ("matching", "minimization", "transformation", "error estimation")]
    assert order == sorted(order)                       # in the reference's order
    assert phases["matching"][1] > 0.0 and phases["minimization"][1] > 0.0
    # transformation and error estimation ride in the front of the matching kernel: their own lines read zero
    assert phases["transformation"] == (0.0, 0.0) and phases["error estimation"] == (0.0, 0.0)
    T = _transform(r.stdout)
    ang, t_mm = pkg.datasets.HALL_MM
    assert np.abs(T[:3, 3] - np.array(t_mm) / 1000.0).max() < 5e-3 and abs(T[1, 0] - np.sin(ang[2])) < 5e-3
    err = _errors(r.stdout)
    # like the reference, the program prints E[0..iterations]: the value that tripped the stop rule is not shown
    assert err[0] == 0.0 and len(err) >= 3 and err[-1] < 0.5 * err[1]
    assert int(m.group(2)) == len(err)                  # "with %d iterations" prints iteration + 1 = the entries of the error list (:383,387)
    # the same dump in the reference's own file form, at full size: one decimal byte value per line, 806 912 lines
    # (Donut_1024x16.csv, :432-488) -- read by the text path of icp_read_os1_ranges, same registration to the last digit
    csv = tmp_path / "Donut_1024x16.csv"
    with open(csv, "w") as f:
        f.write("\n".join(map(str, pk.tolist())) + "\n")
    assert sum(1 for _ in open(csv)) == 806912
    r2 = subprocess.run([os.path.join(BIN, "ICP_point_to_point"), "--hall", str(csv), os.path.join(golden, "beam_intrinsics.csv"),
                         "--transform"], capture_output=True, text=True, timeout=180)
    assert r2.returncode == 0, r2.stderr
    assert np.array_equal(_errors(r2.stdout), err) and np.array_equal(_transform(r2.stdout), T)


def test_icp_point_to_plane_program(pkg):
    r = subprocess.run([os.path.join(BIN, "ICP_point_to_plane"), "--width", "48", "--transform"], capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("For normals:\nGrid Size: ")                    # src/ICP_point_to_plane.cu:381
    assert re.search(r"Normals were calculated in \d+\.\d+ ms", r.stdout)      # :427
    assert "For ICP loop:\nGrid Size: " in r.stdout                            # :513
    cur = [float(x) for x in re.findall(r"Current error \(\d+\): (\d+\.\d{4})", r.stdout)]   # :623
    assert len(cur) >= 3 and cur[-1] < 0.2 * cur[0]
    assert "ICP converged successfully!" in r.stdout
    T = _transform(r.stdout)
    assert np.abs(T[:3, 3] - np.array([0.8, -0.3, 0.2])).max() < 0.05          # the motion baked into the model


# ---------------------------------------------------------------------------------------------------
# hall packets decoded on the device, the sweep program, the per-iteration trace dump
# ---------------------------------------------------------------------------------------------------
def _hall_packets(golden):
    ranges = np.fromfile(os.path.join(golden, "hall_ranges_u32.bin"), dtype=np.uint32)
    enc = json.load(open(os.path.join(golden, "hall_meta.json")))["encoder_count0"]
    pk = np.zeros(64 * 12608, dtype=np.uint8)
    pk[12], pk[13] = enc & 0xFF, (enc >> 8) & 0xFF
    idx = np.arange(ranges.size)
    w = (idx // 256) * 12608 + ((idx // 16) % 16) * 788 + 16 + 12 * (2 + 4 * (idx % 16))
    pk[w], pk[w + 1], pk[w + 2] = ranges & 0xFF, (ranges >> 8) & 0xFF, (ranges >> 16) & 0x0F
    return pk, ranges, enc


def test_os1_packets_decoded_on_device(ctx, pkg, orc, golden):
    pk, ranges, enc = _hall_packets(golden)
    alt, az = pkg.datasets.read_os1_intrinsics(os.path.join(golden, "beam_intrinsics.csv"))
    xyz, rng = ctx.os1_packets_to_cartesian(pk, alt, az)
    assert np.array_equal(rng, ranges)                                   # 20-bit ranges, bit-exact
    assert np.array_equal(xyz, ctx.os1_to_cartesian(ranges, enc, alt, az))   # same arithmetic as the two-step path
    want = orc.os1_conversion(ranges.astype(np.float32), enc, alt, az)   # the reference's Conversion, restated
    assert np.abs(xyz - want).max() < 2e-5 * np.abs(want).max()
    # the first two packets of the real dump, as text -> bytes
    vals = np.array([int(x) for x in open(os.path.join(golden, "os1_two_packets.csv")).read().split()], dtype=np.uint8)
    xyz2, rng2 = ctx.os1_packets_to_cartesian(vals, alt, az)
    assert np.array_equal(rng2, ranges[:512]) and np.array_equal(xyz2, xyz[:512])


def test_time_complexity_program(tmp_path):
    for flags, name, header in (([], "p2p.csv", "NUM_POINTS,TIME"), (["--plane"], "plane.csv", "NUM_POINTS,TIME"),
                                (["--matching"], "match.csv", "#POINTS,TIME")):
        out = tmp_path / name
        r = subprocess.run([os.path.join(BIN, "ICP_time_complexity"), "--max-width", "12", "--out", str(out)] + flags,
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        lines = open(out).read().split()
        assert lines[0] == header
        rows = [ln.split(",") for ln in lines[1:]]
        assert [int(a) for a, _ in rows][-1] == 144 and all(float(b) > 0 for _, b in rows)
        assert len(rows) >= 9


def test_trace_dump_layout(tmp_path):
    out = tmp_path / "Test_icp"
    r = subprocess.run([os.path.join(BIN, "ICP_point_to_point"), "--width", "8", "--trace", str(out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = open(out).read().splitlines()
    head = lines[0].split("|")
    assert head[:6] == ["x_data", "y_data", "z_data", "x_model", "y_model", "z_model"] and head[6] == "TDx_1"   # src/ICP_CPU.c:416-417
    n_it = (len(head) - 6) // 3
    assert n_it >= 2 and len(lines[1].split("|")) == 6 + 3 * n_it + 1
    assert lines[1 + 64] == "" and lines[2 + 64].startswith("Error|")


def test_point_to_plane_hall(ctx, pkg, orc, golden):
    """BASELINE configs[3]: hall LiDAR scan, point-to-plane (6x6 solve), fp32 -- device kNN/normals included"""
    P, Q = orc.hall_clouds(golden)
    ctx.set_model(Q)
    nrm, nbr = ctx.estimate_normals(want_neighbours=True)
    assert np.array_equal(nbr, orc.knn4(Q))
    res = ctx.point_to_plane(P, Q, normals=nrm, max_iter=100, tol=1e-6)
    want = orc.icp_p2plane_f32x(P, Q, nrm, 100, 1e-6)                     # same normals on both sides
    assert_same_plane_run(res, want, 1e-6)
    assert np.array_equal(res.idx, want["idx"]) or res.iterations != want["iterations"]
    for acc64 in (True, False):                                          # the fp32 twin and its double-accumulating variant
        assert_same_plane_run(res, orc.icp_p2plane(P, Q, nrm, 100, 1e-6, accumulate_f64=acc64), 1e-6)
    ang, t_mm = pkg.datasets.HALL_MM
    assert np.abs(res.T[:3, 3] - np.array(t_mm) / 1000.0).max() < 5e-3 and abs(res.T[1, 0] - np.sin(ang[2])) < 5e-3
    # the oracle's own normals (host eigen-solve) instead of the device's: the registration is the same
    onrm, _ = orc.normals(Q, nbr)
    res_o = ctx.point_to_plane(P, Q, normals=onrm, max_iter=100, tol=1e-6)
    assert_same_plane_run(res_o, orc.icp_p2plane_f32x(P, Q, onrm, 100, 1e-6), 1e-6)
