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


# ---- clouds of the matching fuzzes (tests/test_gpu_parity.py in float32, tests/test_gpu_f64_matching.py in float64; conditions on
# ---- them: tests/test_f64_clouds.py) ----------------------------------------------------------------------------------------------
FUZZ_KINDS = ("uniform", "clustered", "lattice", "line")
FUZZ_SCALES = (1e-3, 1.0, 1e3)


def fuzz_cloud(rng, n, kind, scale, dtype=np.float32, signed_zeros=False):
    """n points of one kind -- uniform / clustered with exact duplicates / integer lattice / line -- times scale.  float32 rounds
    the float64 construction once; float64 keeps it as it is, mantissas full.  signed_zeros: about half of the exact zeros
    (lattice coordinates, a line's y and z) become -0.0 -- the same point to every comparison, other bits to a sort by bit
    pattern; their draws come after all the others, so a cloud without them has the bytes it always had."""
    if kind == "uniform":
        X = rng.uniform(-1, 1, (n, 3))
    elif kind == "clustered":          # a few tight clusters with exact duplicates sprinkled in
        c = rng.uniform(-1, 1, (6, 3))
        X = c[rng.integers(0, 6, n)] + 0.01 * rng.standard_normal((n, 3))
        d = rng.integers(0, n, max(1, n // 10))
        X[d] = X[rng.integers(0, n, d.size)]
    elif kind == "lattice":            # integer lattice: exact ties everywhere
        X = rng.integers(-3, 4, (n, 3)).astype(np.float64)
    else:                              # "line": degenerate extent in two axes
        X = np.zeros((n, 3))
        X[:, 0] = rng.uniform(-1, 1, n)
    X = scale * X
    if signed_zeros:
        X[(X == 0.0) & (rng.random(X.shape) < 0.5)] = -0.0
    return X.astype(np.float32) if np.dtype(dtype) == np.float32 else X


F64_FUZZ_SEEDS = {"1": 6401, "0": 6400}     # ICP_F64_SPARSE -> the seed of its cases


def f64_matching_cases(seed, cases):
    """the cases of the float64 matching fuzz, in order: (n, m, kind of the cloud, kind of the model, scale, P, Q) -- n in [1, 700),
    m in [1, 900), the kinds independent, one scale per case, signed zeros in every second case"""
    rng = np.random.default_rng(seed)
    for case in range(cases):
        n, m = int(rng.integers(1, 700)), int(rng.integers(1, 900))
        kp, km = (str(k) for k in rng.choice(FUZZ_KINDS, 2))
        scale = float(rng.choice(FUZZ_SCALES))
        sz = case % 2 == 1
        yield n, m, kp, km, scale, fuzz_cloud(rng, n, kp, scale, np.float64, sz), fuzz_cloud(rng, m, km, scale, np.float64, sz)


# ---- models of more than one round of nn_match_row64_f64 (a round is 4096 chunks of 8 = 32 768 model points) -------------------
ROUND_POINTS = 32768
SPARSE_M_PAD_BELOW = 1 << 17       # larger models (padded to a multiple of NN_CHUNK = 16 points) go to the dense kernel
EIGHT_WAVE_N = 16448               # 257 rows of 64; padded to 17 408 points it is 272 blocks, more than the 256 CUs of an MI355X
TIE_DIMS = (35, 35, 33)


def straddling_tie_pair(n=700, replace=False, scale=1.0, dtype=np.float64):
    """model: the 35 x 35 x 33 integer lattice (40 425 distinct points) in a fixed random order; cloud: n cell centres (+0.5) drawn
    by the same generator.  Every centre has 8 tied minima at d = 0.75, scattered over the model's indices: for four centres in
    five on both sides of point 32 768, where the first round ends.  scale 1e-170 / 1e160: every squared distance underflows to 0 /
    overflows to +inf, and the first minimum of an ascending scan is point 0 for every centre.  float32: the scaled float64
    coordinates rounded once (F32_TIE_SCALES says what each scale does to the squared distances)."""
    rng = np.random.default_rng(6464)
    a, b, c = TIE_DIMS
    g = np.stack(np.meshgrid(np.arange(float(a)), np.arange(float(b)), np.arange(float(c)), indexing="ij"), -1).reshape(-1, 3)
    M = g[rng.permutation(g.shape[0])]
    cells = np.stack(np.meshgrid(np.arange(a - 1.0), np.arange(b - 1.0), np.arange(c - 1.0), indexing="ij"), -1).reshape(-1, 3) + 0.5
    P = cells[rng.choice(cells.shape[0], n, replace=replace)]
    return np.ascontiguousarray((P * scale).astype(dtype, copy=False)), np.ascontiguousarray((M * scale).astype(dtype, copy=False))


UNDERFLOW_SCALE, OVERFLOW_SCALE = 1e-170, 1e160


def far_pair(n=700, m=40000, dtype=np.float64):
    """model: m uniform float64 points in [-1, 1]^3; cloud: n picks of it shifted by (5, 5, 5) -- the bound a cold start gets from
    any model point is wider than the model, so nearly every chunk of both rounds is a hit (float32: both rounded once)"""
    rng = np.random.default_rng(4000)
    M = rng.uniform(-1, 1, (m, 3))
    return (M[rng.integers(0, m, n)] + 5.0).astype(dtype, copy=False), M.astype(dtype, copy=False)


def twin_model(m=40000, dtype=np.float64):
    """a model with exact twins, and a cloud that hits them: (P, M, want).  M is m uniform float64 points whose x or y is exactly 0
    for every fifth point (a -0.0 must not look nearer or farther than them either); groups of three model indices a < b < c hold one point -- b and c in a's chunk of 8, in other chunks of
    a's round, and (c, or b and c) in the other round --, the copies of a point with a zero coordinate with the zero's sign
    flipped.  Every group is hit through its HIGHER members' coordinates (signed zeros included); want is the lowest member.
    float32: the same model rounded once -- copies stay copies, zeros keep their signs, and tests/test_f32_clouds.py shows that no
    two other points fell together."""
    rng = np.random.default_rng(2222)
    M = rng.uniform(-1, 1, (m, 3))
    M[::5, 0] = 0.0
    M[2::10, 1] = 0.0
    used = set()
    groups = []

    def free(lo, hi, chunk=None):
        while True:
            j = int(rng.integers(lo, hi)) if chunk is None else chunk * 8 + int(rng.integers(0, 8))
            if j not in used and lo <= j < hi:
                used.add(j)
                return j

    for rep in range(60):
        form = rep % 4
        a = free(0, ROUND_POINTS - 8) if form != 3 else free(ROUND_POINTS, m - 8)
        if form == 0:      # the same chunk
            b, c = free(0, m, a // 8), free(0, m, a // 8)
        elif form == 1:    # other chunks of the first round
            b, c = free(0, ROUND_POINTS), free(0, ROUND_POINTS)
        elif form == 2:    # the other round
            b, c = free(0, ROUND_POINTS), free(ROUND_POINTS, m)
        else:              # all in the second round
            b, c = free(ROUND_POINTS, m), free(ROUND_POINTS, m)
        groups.append(sorted((a, b, c)))
    P, want = [], []
    for k, (a, b, c) in enumerate(groups):
        src = M[(a, b, c)[k % 3]].copy()   # the group's point is the one any of the three held ...
        if k % 2 == 0:
            src[k % 3] = 0.0               # ... every second one with an exact zero
        for j in (a, b, c):
            M[j] = src
        for j, flip in ((b, k % 2 == 0), (c, True)):
            if flip:
                M[j] = np.where(src == 0.0, -0.0, src)
        for j in (b, c):
            P.append(M[j].copy())
            want.append(a)
    return np.array(P).astype(dtype, copy=False), M.astype(dtype, copy=False), np.array(want, dtype=np.int32)


# ---- float32 across its range (tests/test_gpu_f32_matching.py; conditions: tests/test_f32_clouds.py) ----------------------------
# what a scale does to float32 squared distances, shown on the tie pair in tests/test_f32_clouds.py:
#   1e-25        every squared distance is 0: the oracle answers point 0
#   3e-22, 1e-20 every minimum is a non-zero subnormal (6.7e-44, 7.5e-41): a rounding is absolute there, all 8 ties survive
#   1e19         nearly every squared distance is +inf, every minimum finite; the rounding of the coordinates thins the ties out
#   1e20         every squared distance is +inf: the oracle answers point 0
F32_ZERO_SCALE, F32_SUBNORMAL_SCALES, F32_PART_INF_SCALE, F32_INF_SCALE = 1e-25, (3e-22, 1e-20), 1e19, 1e20
F32_TIE_SCALES = (1.0, 1e-20, 3e-22, 1e-25, 1e19, 1e20)
F32_FUZZ_SCALES = (1e-25, 3e-22, 1e-20, 1e-3, 1.0, 1e3, 1e15, 1e19, 1e20)
F32_FUZZ_CASES = 36
F32_FUZZ_SEEDS = {"0": 3202, "1": 3201}     # ICP_SORT -> the seed of its cases (chosen in tests/test_f32_clouds.py)
SUPER_BOX_POINTS = 32768                    # a level-3 box of the hierarchy: 64 x 64 chunks of 8 (and the m_pad border of the sample probe)


def f32_matching_cases(seed, cases):
    """the cases of the float32 matching fuzz, f64_matching_cases' in float32 over F32_FUZZ_SCALES: (n, m, kind of the cloud, kind of
    the model, scale, P, Q), signed zeros in every second case"""
    rng = np.random.default_rng(seed)
    for case in range(cases):
        n, m = int(rng.integers(1, 700)), int(rng.integers(1, 900))
        kp, km = (str(k) for k in rng.choice(FUZZ_KINDS, 2))
        scale = float(rng.choice(F32_FUZZ_SCALES))
        sz = case % 2 == 1
        yield n, m, kp, km, scale, fuzz_cloud(rng, n, kp, scale, np.float32, sz), fuzz_cloud(rng, m, km, scale, np.float32, sz)


MIXED_OUTLIERS = (0, 63, 127, 128, 704)     # lanes 0 and 63 of a row of 64, both sides of the first row-of-128 border, the last point


def mixed_overflow_pair(m=1000):
    """float32.  model: m uniform points in [-1, 1]^3; cloud: 705 points -- noisy picks of the model, except the five at
    MIXED_OUTLIERS, whose coordinates are about 2e19: every squared distance from them overflows to +inf (they match point 0),
    while their neighbours in the same rows have finite minima"""
    rng = np.random.default_rng(1919)
    M = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    P = (M[rng.integers(0, m, 705)] + (1e-2 * rng.standard_normal((705, 3))).astype(np.float32)).astype(np.float32)
    for k, i in enumerate(MIXED_OUTLIERS):
        P[i] = np.array([2e19, -2.5e19, 3e19], dtype=np.float32)[[k % 3, (k + 1) % 3, (k + 2) % 3]] * np.float32(1 + 0.125 * k)
    return P, M
