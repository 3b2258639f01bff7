"""CPU: the numpy restatement of the symmetric metric (tests/batch_sym_ref.py) alone.

    1  solve's motion is a rotation: R R^T - I below 1e-14 for |a| from 0 to 10, a = 0 the identity exactly, and the angle of R is
       2 atan(|a|) about a
    2  exactness on a second-order patch: two points of a common circle of radius r with the circle's own normals have a symmetric
       residual below 1e-15 r, while the plane residual (p - q) . nq is the squared chord over 2r
    3  the scene (batch_sym_ref.scene: 40 degrees about z, fp64, analytic normals), both loops in numpy: after pass 2 the symmetric
       rotation error is below 0.1 degrees and the plane loop's above 1 degree (measured: 0.010 and 7.6, tenfold and sevenfold
       margins); at the end the symmetric error is below the plane loop's, which keeps the bias of the two clouds' sampling
    4  the sign rule: flipping the sign of any subset of moving normals changes no term, bit for bit"""
import numpy as np

import batch_sym_ref as sr
import ref_moments as rm
from batch_ref import bits_equal


def test_motion_is_a_rotation():
    rng = np.random.default_rng(3)
    R, t = sr.motion(np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1]))
    assert bits_equal(R, np.eye(3)) and bits_equal(t, np.array([0.3, -0.2, 0.1]))
    worst = 0.0
    for length in (0.0, 1e-12, 1e-6, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0):
        for _ in range(8):
            u = rng.standard_normal(3)
            a = length * u / np.linalg.norm(u)
            tt = rng.standard_normal(3)
            R, t = sr.motion(np.concatenate([a, tt]))
            worst = max(worst, float(np.abs(R @ R.T - np.eye(3)).max()))
            assert abs(np.linalg.det(R) - 1.0) < 1e-13
            assert np.abs(R @ a - a).max() <= 1e-14 * max(1.0, length)          # a is the axis
            # R is the rotation by 2 atan(|a|) about a, t = Ra (cos(theta) tt)
            want = sr.rodrigues(a, np.degrees(2.0 * np.arctan(length))) if length > 0 else np.eye(3)
            assert np.abs(R - want).max() < 1e-14, (length, np.abs(R - want).max())
            half = sr.rodrigues(a, np.degrees(np.arctan(length))) if length > 0 else np.eye(3)
            assert np.abs(t - half @ (np.cos(np.arctan(length)) * tt)).max() < 1e-14 * max(1.0, np.abs(tt).max())
    print(f"[sym ref] largest |R R^T - I| = {worst:.3e}")
    assert worst < 1e-14


def test_residual_vanishes_on_a_common_circle():
    worst = 0.0
    for r in (0.5, 1.0, 7.0, 1000.0):
        for a0 in (0.1, 1.3, 2.9, 4.4):
            for da in (0.01, 0.1, 0.3):
                for plane in ((0, 1), (1, 2), (2, 0)):
                    def on(a):
                        v = np.zeros(3)
                        v[plane[0]], v[plane[1]] = np.cos(a), np.sin(a)
                        return v
                    p, q = (r * on(a0))[None, :], (r * on(a0 + da))[None, :]
                    npn, nq = on(a0)[None, :], on(a0 + da)[None, :]
                    _, h, _ = sr.residual(p, q, npn, nq, np.array([0]), np.eye(3))
                    chord2 = float(((p - q) ** 2).sum())
                    plane_res = float(((p - q) * nq).sum())
                    worst = max(worst, abs(float(h[0])) / r)
                    assert abs(h[0]) < 1e-15 * r, (r, a0, da, h[0])
                    assert 0.5 * chord2 / (2 * r) < abs(plane_res) < 2.0 * chord2 / (2 * r), (r, a0, da, plane_res, chord2)
    print(f"[sym ref] largest |h| / r on a circle = {worst:.3e}")


def test_scene_symmetric_beats_plane(orc):
    sc = sr.scene(np.float64)
    assert sc["A"].shape == (625, 3) and sc["M"].shape == (1600, 3)
    sym = sr.reference_loop(orc, sc["A"], sc["M"], sc["Np"], sc["Nq"], sr.ITER_SCENE, 0.0, truth=sc["R"])
    pl = sr.reference_loop(orc, sc["A"], sc["M"], sc["Np"], sc["Nq"], sr.ITER_SCENE, 0.0, metric="plane", truth=sc["R"])
    print("[sym scene] rotation error in degrees after passes 1, 2, 3 and at the end: "
          f"symmetric {sym['ang'][0]:.4g} {sym['ang'][1]:.4g} {sym['ang'][2]:.4g} {sym['ang'][-1]:.3g}, "
          f"plane {pl['ang'][0]:.4g} {pl['ang'][1]:.4g} {pl['ang'][2]:.4g} {pl['ang'][-1]:.3g}")
    assert not sym["singular"] and not pl["singular"]
    assert sym["ang"][1] < 0.1 and pl["ang"][1] > 1.0
    assert sym["ang"][-1] < pl["ang"][-1]
    assert np.abs(sym["T"][:3, 3] - sr.SHIFT).max() < 1e-3


def test_sign_of_a_moving_normal_changes_no_term():
    rng = np.random.default_rng(11)
    n, m = 300, 400
    P, Q = rng.standard_normal((n, 3)), rng.standard_normal((m, 3))
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    Np, Nq = unit(rng.standard_normal((n, 3))), unit(rng.standard_normal((m, 3)))
    idx = rng.integers(0, m, n)
    for Rc in (np.eye(3), sr.rodrigues((1.0, -2.0, 0.5), 33.0)):
        base = sr.terms(P, Q, Np, Nq, idx, Rc)
        assert np.abs(base[:, rm.MB:rm.MB + 6]).max() > 0
        for seed in range(4):
            sign = np.where(np.random.default_rng(seed).uniform(size=n) < (0.5 if seed else 1.0), -1.0, 1.0)
            assert bits_equal(sr.terms(P, Q, Np * sign[:, None], Nq, idx, Rc), base), seed
