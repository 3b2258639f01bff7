"""The rule of the point-to-plane front end (include/icp_mi355x.h, icp_estimate_normals) in numpy, and the clouds that take the
neighbour search and the normals to the ends of the float range (tests/test_gpu_knn_normals.py; what the clouds are is shown on the
CPU in tests/test_knn_ref.py).  Nothing here touches a device.

Neighbours: d(i, j) = (dx*dx + dy*dy) + dz*dz, every operation rounded in the cloud's dtype; the candidates of query i are all j,
i included, with d < +inf, in (d, j)-ascending order; rank 0 is dropped, ranks 1-4 are the neighbours, a rank that does not exist
holds index 0.  No sentinel: orc_knn4_f32 (the reference's letter, which overwrites a taken distance with 10000) is this rule
exactly where every query's fifth-smallest distance is below 10000.
Normals: pca_normal's covariance in the cloud's dtype; a covariance with a non-finite entry gives exactly (+0, +0, +0)."""
import functools

import numpy as np

import clouds as cl
import ref_numpy
from batch_ref import knn_models

SENTINEL = 10000.0                      # orc_knn4_f32 overwrites a taken distance with it
SEED = 7

# ---- what a scale does to the squared distances of a fuzz_cloud in each dtype (shown in tests/test_knn_ref.py) -------------------
ZERO_SCALE = {np.float32: 1e-25, np.float64: 1e-170}                 # every d underflows to 0
SUBNORMAL_SCALES = {np.float32: (3e-22, 1e-20), np.float64: (1e-157,)}   # every d is below the smallest normal, some are not 0
SENTINEL_SCALES = {np.float32: (60.0, 1000.0), np.float64: (1e3,)}   # fifth distances of 10000 and more
LARGE_SCALES = {np.float32: (1e15,), np.float64: (1e150,)}           # d near the top of the range, all finite
PART_INF_SCALE = {np.float32: 3e19, np.float64: 3e154}               # some d overflow: every count of empty slots occurs
INF_SCALE = {np.float32: 1e20, np.float64: 1e160}                    # apart(): every d off the diagonal is +inf
SCALES = {np.float32: (1e-25, 3e-22, 1e-20, 60.0, 1000.0, 1e15, 3e19, 1e20), np.float64: (1e-170, 1e-157, 1e3, 1e150, 3e154, 1e160)}
SCALE_M = (300, 1025)
# model sizes of sized(): on 256 CUs one block / two query blocks / two, three and nine model segments / two LDS tiles per wave
SIZED_M = (5, 6, 17, 129, 513, 1025, 4097, 12001)
# icp_diag_knn4_geometry on 256 CUs: m -> (n_pad, blocks_x, splits, seg_len, tiles).  tests/test_gpu_knn_normals.py holds the
# context's own answer against this table (where it has 256 CUs) and takes the borders from that answer; the CPU tests use the table
GEOMETRY_256 = {5: (128, 1, 1, 32, 1), 6: (128, 1, 1, 32, 1), 17: (128, 1, 1, 32, 1), 129: (256, 2, 1, 160, 1), 513: (640, 5, 2, 288, 1),
                1025: (1152, 9, 3, 352, 1), 4097: (4224, 33, 9, 480, 1), 12001: (12032, 94, 11, 1120, 2)}
TWIN_M = (1025, 12001)


def _dt(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def sq_dist_rows(P, Q):
    """[len(P), len(Q)] of (dx*dx + dy*dy) + dz*dz, every operation rounded in the clouds' dtype"""
    assert P.dtype == Q.dtype
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dx, dy, dz = (P[:, None, a] - Q[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == Q.dtype
    return d


def _first_five(d, plain):
    """the first five columns of np.argsort(d, axis=1, kind="stable").  Not plain: the same sort over every row's candidates alone --
    the columns whose distance is at most the row's fifth smallest (np.partition), in ascending column order, padded behind with
    +inf; whatever the sort puts in front of the fifth place is among them, so the first five are the full sort's (shown on the
    clouds of up to 1025 points and on rows of the 12 001-point cloud in tests/test_knn_ref.py).  A full sort of 12 001 rows takes 16 s, this one 2 s."""
    if plain:
        return np.argsort(d, axis=1, kind="stable")[:, :5]
    cand = d <= np.partition(d, 4, axis=1)[:, 4:5]
    count = cand.sum(axis=1)
    r, c = np.nonzero(cand)                                   # row-major: ascending columns within a row
    place = np.arange(r.size) - np.repeat(np.cumsum(count) - count, count)
    dd = np.full((d.shape[0], int(count.max())), np.inf, dtype=d.dtype)
    jj = np.zeros(dd.shape, dtype=np.int64)
    dd[r, place], jj[r, place] = d[r, c], c
    return np.take_along_axis(jj, np.argsort(dd, axis=1, kind="stable")[:, :5], axis=1)


def knn4_rule(Q, rows=512, plain=False):
    """(neighbours (m, 4) int32, the five smallest distances (m, 5) in Q's dtype, rank 0 included)"""
    Q = np.ascontiguousarray(Q)
    m = Q.shape[0]
    assert m >= 5 and rows <= 512
    nbr, d5 = np.empty((m, 5), dtype=np.int32), np.empty((m, 5), dtype=Q.dtype)
    for s in range(0, m, rows):
        d = sq_dist_rows(Q[s:s + rows], Q)
        first = _first_five(d, plain)
        dd = np.take_along_axis(d, first, axis=1)
        nbr[s:s + rows] = np.where(np.isfinite(dd), first, 0)     # (+inf sorts last; a finite input gives no NaN: inf + inf = inf)
        d5[s:s + rows] = dd
    return np.ascontiguousarray(nbr[:, 1:]), d5


@functools.lru_cache(maxsize=None)
def _rule_cached(dtype_name, shape, raw):
    return knn4_rule(np.frombuffer(raw, dtype=dtype_name).reshape(shape))


def rule(Q):
    """knn4_rule, computed once per cloud"""
    Q = np.ascontiguousarray(Q)
    return _rule_cached(Q.dtype.name, Q.shape, Q.tobytes())


def empty_slots(d5):
    """per query: how many of the ranks 1-4 do not exist"""
    return (~np.isfinite(d5[:, 1:])).sum(axis=1)


def covariance_rule(Q, nbr):
    """pca_normal's covariance in Q's dtype (ref_numpy.covariance4: sequential sums, bar * 0.25, the six products in its order):
    ((m, 3, 3) symmetric in Q's dtype, finite (m,) -- every entry finite)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        A9 = ref_numpy.covariance4(Q, nbr)
    A = A9.reshape(-1, 3, 3)
    A = np.triu(A) + np.transpose(np.triu(A, 1), (0, 2, 1))
    assert A.dtype == Q.dtype
    return A, np.isfinite(A).all(axis=(1, 2))


def scaled_eigenvalues(A, finite):
    """(amax (m,), w (m, 3) ascending eigenvalues of A / max|A| formed in float64 -- the conversion to double is exact --, rows with a
    non-finite or an all-zero covariance zero)"""
    Af = np.where(finite[:, None, None], A, 0).astype(np.float64)
    amax = np.abs(Af).max(axis=(1, 2))
    An = Af / np.where(amax > 0, amax, 1.0)[:, None, None]
    return amax, An, np.linalg.eigvalsh(An)


def defined(w):
    """where the direction is defined: the two smallest eigenvalues are separated by more than 1e-3 of the largest"""
    return (w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2]


def check_normals(nrm, A, finite, Q, nbr, orc):
    """the three checks of test_gpu_plane_and_programs.test_normals_match_oracle_up_to_sign without their absolute floors: per point
    the covariance is divided by its largest magnitude first.  Returns the defined mask (rows with a finite covariance only).
      ~finite          the normal is exactly (+0, +0, +0): bytes, so -0.0 fails
      max|A| == 0      the oracle's axis up to sign within 1e-6
      otherwise        unit norm within 1e-5; Rayleigh quotient within 1e-5 (of the largest eigenvalue magnitude) of the eigenvalue
                       of smallest magnitude; residual within 1e-4.  One widening, on rows whose smallest eigenvalue magnitude is
                       SUBNORMAL in the cloud's dtype only: pca_normal compares the magnitudes rounded to that dtype and takes
                       the first of the smallest, and a subnormal has so few bits that the rounding ties eigenvalues which
                       differ in double; there each eigenvalue whose rounded magnitude lies within one spacing of the smallest
                       (what the two eigen-solvers may differ by) is the rule's.  Every other row is held to the eigenvalue of
                       smallest magnitude alone.
      defined          |dot| with orc.normals on the same neighbours within 1e-4 of 1"""
    assert nrm.dtype == Q.dtype and not np.isnan(nrm).any()
    dt = Q.dtype.type
    assert nrm[~finite].tobytes() == np.zeros((int((~finite).sum()), 3), dtype=Q.dtype).tobytes()
    amax, An, w = scaled_eigenvalues(A, finite)
    live = finite & (amax > 0)
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64[finite], axis=1) - 1.0).max(initial=0.0) < 1e-5
    scale = np.abs(w).max(axis=1)
    first = np.abs(w).argmin(axis=1)[:, None] == np.arange(3)[None, :]
    with np.errstate(over="ignore", under="ignore"):
        mag = np.abs((w * amax[:, None]).astype(dt))                       # the magnitudes as the cloud's dtype holds them
        least = mag.min(axis=1, keepdims=True)
        tied = first | ((least < np.finfo(dt).tiny) & (mag <= least + np.spacing(least)))
    ray = np.einsum("ni,nij,nj->n", n64, An, n64)
    miss = np.where(tied, np.abs(ray[:, None] - w), np.inf).min(axis=1)
    bad = live & ~(miss <= 1e-5 * scale)
    assert not bad.any(), (int(bad.sum()), float((miss / np.maximum(scale, 1e-300))[live].max()))
    resid = np.linalg.norm(np.einsum("nij,nj->ni", An, n64) - ray[:, None] * n64, axis=1)
    bad = live & ~(resid <= 1e-4 * scale)
    assert not bad.any(), (int(bad.sum()), float((resid / np.maximum(scale, 1e-300))[live].max()))
    want = orc.normals(Q, np.where(finite[:, None], nbr, 0))[0]            # (the oracle sees finite covariances only)
    dots = np.abs((n64 * want.astype(np.float64)).sum(axis=1))
    ok = live & defined(w)
    assert np.abs(dots[ok] - 1.0).max(initial=0.0) < 1e-4
    zero = finite & (amax == 0)
    assert np.abs(dots[zero] - 1.0).max(initial=0.0) < 1e-6
    return ok


# ---- the clouds ------------------------------------------------------------------------------------------------------------------
def sized(m, dtype=np.float32):
    """m standard-normal points (batch_ref.knn_models' construction), one of SIZED_M"""
    return knn_models(dtype, sizes=(m,))[0]


def borders(geom, m):
    """every model index in (0, m) at which knn4_f32_v2 merges two lists: the segment starts s * seg_len and the wave-quarter starts
    s * seg_len + w * seg_len / 4 inside them (geom: icp_diag_knn4_geometry's n_pad, blocks_x, splits, seg_len, tiles), ascending"""
    splits, seg = geom[2], geom[3]
    assert seg % 4 == 0
    return sorted(b for b in {s * seg + w * (seg // 4) for s in range(splits) for w in range(4)} if 0 < b < m)


def border_twins(m, geom, dtype=np.float32):
    """(Q, triples): m uniform points in which, for every border b (borders(geom, m)), the points b - 1 and b are exact copies of
    one point X_b of their own, and a third copy sits at the head of a segment: for a wave-quarter border in segment s at
    s * seg_len + 1 + w, for a segment start b = s * seg_len at (s - 1) * seg_len + 1.  Equal distances then straddle every merge,
    wave over wave and segment over segment, through up to three lists, and a query at X_b must list the copies in index order.
    triples[k] = (third, b - 1, b)."""
    seg = geom[3]
    assert seg // 4 >= 8
    Q = cl.fuzz_cloud(np.random.default_rng(SEED + m), m, "uniform", 1.0, dtype)
    triples = []
    for b in borders(geom, m):
        s, w = divmod(b, seg)
        third = s * seg + 1 + w // (seg // 4) if w else (s - 1) * seg + 1
        Q[b] = Q[b - 1]
        Q[third] = Q[b - 1]
        triples.append((third, b - 1, b))
    flat = [j for t in triples for j in t]
    assert len(set(flat)) == len(flat)
    return np.ascontiguousarray(Q), triples


def coincident(m, dtype=np.float32):
    """every point the same point: every query's neighbours are (1, 2, 3, 4) -- except those of the queries 1-4, whose rank 0 is point 0"""
    return np.tile(np.array([[0.25, -1.5, 3.0]], dtype=dtype), (m, 1))


def scale_cloud(kind, m, scale, dtype):
    """fuzz_cloud of SEED, signed zeros throughout"""
    return np.ascontiguousarray(cl.fuzz_cloud(np.random.default_rng(SEED), m, kind, scale, dtype, signed_zeros=True))


def apart(m, dtype=np.float32):
    """points 8 x INF_SCALE apart in every coordinate: every d(i, j != i) is +inf, every neighbour is 0"""
    k = np.arange(m, dtype=np.float64)
    return np.ascontiguousarray((8.0 * INF_SCALE[_dt(dtype)] * np.stack([k, -k, k], axis=1)).astype(dtype))


_BRINK = {
    np.float32: ((9.2233456e18, 9.2233742e18), (-9.2233830e18, -9.2233841e18)),
    np.float64: ((6.703903964971291e+153, 6.703903964971303e+153), (-6.703903964971306e+153, -6.7039039649712926e+153)),
}


def brink(dtype=np.float32):
    """five points: the origin, (u, v), (v, u), (-s, -t), (-t, -s) with u ~ v ~ s ~ t ~ sqrt(max / 4).  The origin's neighbours are
    the other four, at finite distances of about max / 2; its covariance has xx = yy = the largest finite number and xy = +inf --
    the separately rounded sum of the four products dx * dy overflows where the sums of the squares just do not.  Not finite: the
    normal is (+0, +0, +0).  A test of the diagonal alone lets it through (it did: the Jacobi then ran on the inf and stored NaNs)."""
    dt = _dt(dtype)
    (u, v), (s, t) = _BRINK[dt]
    return np.array([[0, 0, 0], [u, v, 0], [v, u, 0], [s, t, 0], [t, s, 0]], dtype=dt)


def scale_clouds(dtype):
    """[(name, cloud)]: every kind x every scale of the dtype x SCALE_M, then apart(300)"""
    dt = _dt(dtype)
    out = [(f"{kind}-{scale:g}-{m}", scale_cloud(kind, m, scale, dt)) for scale in SCALES[dt] for kind in cl.FUZZ_KINDS for m in SCALE_M]
    return out + [("apart-300", apart(300, dt))]


def normals_clouds(dtype):
    """[(name, cloud)] of the normals check: the scale clouds, the uniform cloud at scale 1, coincident(300), sized(1025) and brink()"""
    dt = _dt(dtype)
    return scale_clouds(dt) + [("uniform-1-300", scale_cloud("uniform", 300, 1.0, dt)), ("coincident-300", coincident(300, dt)),
                               ("sized-1025", sized(1025, dt)), ("brink-5", brink(dt))]


# the share of points with a defined direction (defined(), from the rule's neighbours and covariance alone), measured in
# tests/test_knn_ref.py, which asserts these floors: the direction check of check_normals is not vacuous on these clouds
NORMAL_DEFINED_MIN = {
    np.float32: {"uniform-1-300": 0.95, "uniform-1000-300": 0.95, "uniform-1000-1025": 0.95, "uniform-1e+15-300": 0.95, "uniform-1e-20-300": 0.95,
                 "sized-1025": 0.95},
    np.float64: {"uniform-1-300": 0.95, "uniform-1000-300": 0.95, "uniform-1000-1025": 0.95, "uniform-1e+150-300": 0.95, "uniform-1e-157-300": 0.95,
                 "sized-1025": 0.95},
}
