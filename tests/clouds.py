"""The clouds of tests/test_gpu_moments.py and tests/test_ref_moments.py (and the ragged pairs of tests/test_gpu_batch.py): one
construction, and the sizes that sit around the granules of each route that produces a moment vector."""
import numpy as np


def ragged_pair(rng_seed, n, m):
    """a model of m standard-normal points and n rotated, shifted, noisy picks of it (fp32): coordinates of order 1, no exact
    zeros (the construction of test_gpu_parity.test_resident_loop_small_and_ragged_clouds)"""
    rng = np.random.default_rng(rng_seed)
    M = rng.standard_normal((m, 3)).astype(np.float32)
    pick = rng.integers(0, m, size=n)
    ang = np.array([0.05, -0.03, 0.04])
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    D = ((M[pick].astype(np.float64) - np.array([0.02, -0.01, 0.03])) @ R).astype(np.float32) + (1e-3 * rng.standard_normal((n, 3))).astype(np.float32)
    return D, M


# the clouds of tests/test_gpu_moments.py: moving-cloud sizes around the granules of the rows (64 points, one per lane; 128 points,
# two per lane), the models, and the sizes that reach a route of their own; test_ref_moments.py shows on the CPU that the
# tolerance sees a one-point defect in every one of them
ROW64_N = (1, 2, 63, 64, 65, 130, 1000)
ROW128_N = (1, 64, 65, 127, 128, 129, 191, 1200)
# in-launch finalize under ICP_HOST_ROWS_MAX=4.  The moving cloud is padded to a multiple of 1024 points (NN_POINT_ALIGN), the
# padding's rows are rows like any other (all zeros, at the end), and the ~sqrt(rows) groups are cut from the padded count:
#   1000 points:  8 rows, all real, groups of 3, 3, 2 -- the short last group holds the last points (row 7: 104 of them)
#   3000 points: 24 rows, all real, groups of 5, 5, 5, 5, 4 -- likewise (row 23: 56 points)
#    640 / 1200 points: 8 / 16 rows of which 5 / 10 are real -- the last real point in the middle of a group, the last group padding
FIN_N = (640, 1000, 1200, 3000)
MODEL_M = (17, 1000)
BATCH_N = (1, 63, 64, 65, 130, 1025)
CAP_N = 64 * 1024 + 65                 # moments_kernel past MOM_MAX_BLOCKS = 1024 blocks: a second, ragged trip of its grid-stride loop
# more than 2048 rows of 64 points: finalize_ranges_kernel + finalize_kernel.  2064 rows in ranges of 9: 229 full ranges, a short
# last one of rows 2061-2063 -- all real (the last row holds 59 points) -- and 26 empty ranges behind it
TWO_STAGE_N = 64 * 2064 - 5


def case_pair(n, m, dtype=np.float32):
    """the pair of one (n, m) case, seed n * 1000 + m; in float64 with mantissas that fp32 cannot hold"""
    D, M = ragged_pair(n * 1000 + m, n, m)
    if np.dtype(dtype) == np.float32:
        return D, M
    rng = np.random.default_rng(n * 1000 + m + 1)
    return D.astype(np.float64) + 1e-9 * rng.standard_normal(D.shape), M.astype(np.float64) + 1e-9 * rng.standard_normal(M.shape)


# ---- clouds of tests/test_gpu_plane_f64.py (conditions on them: tests/test_oracle.py) -------------------------------------------
FUSED_SHIFT = (0.3, -0.7, 1.1)
FAR_OFF, FAR_H = (1000.0, -700.0, 400.0), 1e-3       # a survey-coordinate patch: float32 holds 6e-5 there, the points lie 2.5e-5 apart
NEAR_OFF, NEAR_H = (0.0, 0.0, 0.0), 1.0


def fused_tie_lattice(dtype, tiles=1):
    """integer points (i, j, k), i, j < 12, k < 3, kept where (i + 2 j + 3 k) % 5 == 0 (86 of them), times 0.1, plus FUSED_SHIFT,
    in a fixed random order; tiles = 3: nine copies of those 86 points, 1.2 apart in x and y and centred on the first (774 points).
    The nearest shells mix offsets like (a, 2a, 0) and (2a, -a, 0) with a not representable: dx*dx + dy*dy, every operation
    rounded, ties between them bit for bit where the differences happen to round alike, and an expression that fuses a product into
    a sum orders them differently (ref_numpy.order_fused; the shares are asserted in test_oracle.py)."""
    g = np.array([(i, j, k) for i in range(12) for j in range(12) for k in range(3) if (i + 2 * j + 3 * k) % 5 == 0], dtype=np.float64)
    assert g.shape == (86, 3)
    pts = g * 0.1 + np.array(FUSED_SHIFT)
    half = tiles // 2
    pts = np.concatenate([pts + np.array([1.2 * tx, 1.2 * ty, 0.0]) for tx in range(-half, tiles - half) for ty in range(-half, tiles - half)])
    return pts[np.random.default_rng(86).permutation(pts.shape[0])].astype(dtype)


FUSED_CENTRE_SHIFTS = tuple((sx, sy, sz) for sx in (-0.25, 0.25) for sy in (-0.25, 0.25) for sz in (-0.05, 0.15))


def fused_tie_centres(Q):
    """moving points for the matching on Q = fused_tie_lattice(np.float64, 3): cell centres -- the lattice points shifted by the
    half-cell offsets FUSED_CENTRE_SHIFTS -- kept where the separately rounded distance itself ties bit for bit at the minimum
    between model points whose |dx|, |dy|, |dz| differ (359 of 8 x 774).  The plain shift (0.05, 0.05, 0.05) does not serve: the model
    points are 1.4 cells apart at least, a centre's nearest ones are mirror images with the same |dx|, |dy|, |dz|, and a fused form
    keeps such a tie; every single shift of half cells within +-2.5 cells left one of the two fused forms under 5 % of its rows."""
    assert Q.dtype == np.float64
    out = []
    for s in FUSED_CENTRE_SHIFTS:
        P = Q + np.array(s)
        df = np.abs(Q[None, :, :] - P[:, None, :])
        dd = df * df
        sep = (dd[:, :, 0] + dd[:, :, 1]) + dd[:, :, 2]
        tie = (sep == sep.min(axis=1, keepdims=True))[:, :, None]
        out.append(P[(np.where(tie, df, np.inf).min(axis=1) != np.where(tie, df, -np.inf).max(axis=1)).any(axis=1)])
    return np.concatenate(out)


def far_surface(off, h, W=40):
    """a W x W saddle patch of edge h at offset off, float64: grid steps jittered by 5 % of the spacing in every coordinate,
    z = x^2 - y^2 over [-1, 1]^2, the whole scaled to h / 2 and moved to off"""
    rng = np.random.default_rng(4040)
    u = np.linspace(-1.0, 1.0, W)
    x, y = (a.reshape(-1) for a in np.meshgrid(u, u, indexing="ij"))
    local = np.stack([x, y, x * x - y * y], axis=1) + 0.05 * (u[1] - u[0]) * rng.standard_normal((W * W, 3))
    return np.asarray(off, dtype=np.float64) + 0.5 * h * local


def widen_pairs(pairs):
    """fp32 pairs in float64 with mantissas that fp32 cannot hold, as case_pair widens its own (seed = the pair's place)"""
    out = []
    for k, (D, M) in enumerate(pairs):
        rng = np.random.default_rng(7000 + k)
        out.append((D.astype(np.float64) + 1e-9 * rng.standard_normal(D.shape), M.astype(np.float64) + 1e-9 * rng.standard_normal(M.shape)))
    return out
