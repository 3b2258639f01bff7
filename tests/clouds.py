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
