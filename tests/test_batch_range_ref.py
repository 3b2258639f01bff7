"""CPU: the numpy rules of the batched neighbourhood calls across the floating-point range (tests/batch_range_ref.py).

    1  anchor: the range rule of icp_eigh3 changes nothing within 2^+-400 -- both numpy Jacobis with and without it give equal bytes
       on the matrices of test_batch_normals_ref (the 1e150 sets included: 2^498 is past the rule's 2^400, but their squares are
       still finite, so the rule's exact power of two must change no bit; of the 1e-300 sets the zero matrices alone) and on 1 000
       random positive semi-definite matrices just inside 2^+-400; icp_eigh3 is the numpy Jacobi byte for byte at every magnitude of MAGS
    2  the Jacobi against LAPACK at every magnitude of MAGS, within 1e-9 rad under the gap mask; the eigenvalues are the m = 0
       eigenvalues times 2^m exactly (what IEEE makes of the product, where it leaves the range); rank-1, rank-2 and zero matrices
       at 2^+-1000
       ... and icp::eigh3 itself in a program of its own under the address and undefined-behaviour sanitizers (tests/eigh3_check.cpp;
       nothing is loaded into this process)
    3  every rule on a cloud times 2^e is the scale-1 answer exactly scaled: raw and Frobenius covariances, normals in the three
       orientations, ISS saliency and keypoint maps, statistical and radius outlier scores and maps, voxel points and maps, FPFH
"""
import os
import subprocess

import numpy as np
import pytest

import batch_gicp_ref as gr
import batch_keypoint_ref as kr
import batch_normals_ref as nr
import batch_range_ref as rr
from test_batch_normals_ref import matrices, sym6

u64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
CLOUDS = ((311, 200), (312, 65))   # (seed, points) of the blobs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-point-cloud-registration-with-gpus_amd", "csrc")


def in_range(C6):
    """(n,) bool: the matrices of C6 (6, n) the range rule leaves as they are"""
    amax = np.abs(C6).max(axis=0)
    return ((amax >= 2.0 ** -400) & (amax <= 2.0 ** 400)) | (amax == 0) | ~np.isfinite(C6).all(axis=0)


def same_with_and_without(C6, what):
    for a, b in zip(nr.jacobi(C6), nr.jacobi(C6, _scale=False)):
        assert np.array_equal(u64(a), u64(b)), what
    assert np.array_equal(u64(kr.jacobi_eigenvalues(C6)), u64(kr.jacobi_eigenvalues(C6, _scale=False))), what


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_range_rule_changes_nothing_in_range():
    for name, A in matrices().items():
        C6 = sym6(A)
        if name.endswith("_tiny"):                                # 1e-300: the squares are 0 without the rule; the zero matrices stay
            C6 = C6[:, in_range(C6)]
        elif name.endswith("_huge"):                              # 1e150 = 2^498: the squares are still finite, so the statements
            assert not in_range(C6).any() or name == "zero_huge"  # without the rule are right -- and the rule's are their bytes
        else:
            assert in_range(C6).all(), name
        same_with_and_without(C6, name)
    rng = np.random.default_rng(5)
    R = rng.standard_normal((1000, 3, 3))
    C6 = rr.unit6(sym6(R @ R.transpose(0, 2, 1)).T).T             # the largest magnitude in [0.5, 1)
    for m in (399, -399):                                         # ... in [2^398, 2^399) and [2^-400, 2^-399)
        S = np.ldexp(C6[:, (m < 0) * 500:(m < 0) * 500 + 500], m)
        assert in_range(S).all() and (np.abs(S).max(axis=0) > 2.0 ** (m - 2)).all()
        same_with_and_without(S, m)


def test_icp_eigh3_is_the_numpy_jacobi_at_every_magnitude(pkg):
    r1, _, r2 = rr.deficient()
    C6 = np.concatenate([rr.gapped(7, 40), rr.unit6(r1), rr.unit6(r2), np.zeros((1, 6))])
    for m in rr.MAGS:
        S = np.ldexp(C6, m)
        w, n, Z = nr.jacobi(S.T)
        assert np.array_equal(u64(kr.jacobi_eigenvalues(S.T)), u64(w)), m
        for k, A in enumerate(gr.full(S)):
            want_w, want_Z = pkg.eigh3(A)
            want_Z = np.asarray(want_Z, dtype=np.float64).reshape(3, 3)
            assert np.array_equal(u64(w[:, k]), u64(want_w)), (m, k, w[:, k], want_w)
            assert np.array_equal(u64(Z[:, :, k]), u64(want_Z)), (m, k)
            assert np.array_equal(u64(n[:, k]), u64(want_Z[:, 0])), (m, k)


# 2 ------------------------------------------------------------------------------------------------------------------------
def blob_covariances():
    X, _, one = rr.witness(*CLOUDS[0], np.float64)
    return rr.unit6(one["raw"])


def test_jacobi_agrees_with_lapack_at_every_magnitude():
    for name, C6 in (("gapped", rr.gapped(11, 500)), ("blob", blob_covariances())):
        w1, n1, _ = nr.jacobi(C6.T)
        for m in rr.MAGS:
            S = np.ldexp(C6, m)
            assert np.ldexp(S, -m).tobytes() == C6.tobytes()      # the matrices are exact
            w, n, _ = nr.jacobi(S.T)
            worst = rr.check_lapack(n.T, S, f"{name} 2^{m}")
            print(f"{name} 2^{m}: largest angle under the gap mask {worst:.3e} rad")
            assert n.tobytes() == n1.tobytes(), (name, m)         # the rotations do not depend on the power of two
            with np.errstate(under="ignore", over="ignore"):
                assert w.tobytes() == np.ldexp(w1, m).tobytes(), (name, m)   # what IEEE makes of w * 2^m ...
                normal = np.abs(np.ldexp(w1, m)) >= np.finfo(np.float64).tiny
                assert np.ldexp(w, -m)[normal].tobytes() == w1[normal].tobytes(), (name, m)   # ... which is exact wherever it stays normal
            assert normal.all(), (name, m)                        # ... which is everywhere on these matrices
            assert np.array_equal(u64(kr.jacobi_eigenvalues(S.T)), u64(w)), (name, m)


def test_rank_deficient_and_zero_matrices_at_the_ends_of_the_range():
    r1, _, r2 = rr.deficient()
    zero = np.zeros((3, 6))
    base = [nr.jacobi(C.T)[1] for C in (r1, r2, zero)]
    for m in (-1000, 0, 1000):
        got = [nr.jacobi(np.ldexp(C, m).T)[1] for C in (r1, r2, zero)]
        rr.check_deficient(got[0].T, got[1].T, got[2].T, f"2^{m}")
        assert all(g.tobytes() == b.tobytes() for g, b in zip(got, base)), m
        N = nr.normals(np.zeros((4, 3)), np.ldexp(r2, m), nr.NONE)   # ... and through the rule's non-finite test
        assert N.tobytes() == np.ascontiguousarray(got[1].T).tobytes()


def test_host_eigh3_under_sanitizers(tmp_path):
    # the flags the library's host objects are built with, as the Makefile spells them (tests/test_batch_clouds.py)
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "--eval", "print-hostflags: ; @echo $(HOSTFLAGS)", "print-hostflags"],
                           capture_output=True, text=True, check=True).stdout.split()
    assert "-O3" in flags and "-D__HIP_PLATFORM_AMD__" in flags, flags
    exe = str(tmp_path / "eigh3_check")
    cc = subprocess.run(["g++"] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g", "-o", exe,
                                           os.path.join(ROOT, "tests", "eigh3_check.cpp"), os.path.join(CSRC, "icp_host_math.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "eigh3_check passed" in r.stdout and "FAIL" not in r.stdout


# 3 ------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("seed,n", CLOUDS)
def test_every_rule_is_equivariant_under_a_power_of_two(dtype, seed, n):
    X, N, one = rr.witness(seed, n, dtype)
    assert 0 < (one["saliency"] > 0).sum() < n and (one["keypoint_map"] >= 0).any()       # the rules decide something at scale 1
    assert 0 < (one["stat_map"] >= 0).sum() < n and 0 < (one["radius_map"] >= 0).sum() < n
    assert 1 < one["voxel_points"].shape[0] < n
    rr.check_lapack(one["normals"][nr.NONE], one["raw"], "scale 1")   # the blob keeps the gap condition
    for e in rr.exponents(dtype):
        rr.check_equivariant(rr.rules_at(X, N, e), one, e, f"{np.dtype(dtype).name} n {n}")
