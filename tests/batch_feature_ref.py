"""What the tests of batched global registration share (tests/test_batch_feature_ref.py, test_batch_feature_abi.py,
test_gpu_batch_feature.py): the rules of icp_batch_compute_features, icp_batch_match_features, icp_batch_score_transforms and
icp_batch_ransac in numpy, bit for bit as include/icp_mi355x.h states them.  Nothing here touches a device.

    neighbourhood  d2(i, j) = (dx*dx + dy*dy) + dz*dz on arrays of the cloud's own dtype F (batch_outlier_ref.d2_rows); tau_i the
                   k-th smallest over j != i by index (np.partition); every j != i with d2(i, j) <= tau_i
    pair terms     one numpy operation per rounding on float64 arrays over all (i, j) of all neighbourhoods at once, in the
                   header's order; only + - * / sqrt fabs floor
    SPFH           integer counts (np.add.at): no order
    FPFH           np.nonzero lists a row's neighbours in ascending j; the r-th neighbour of every row is added in step r, so each
                   row's sum runs in ascending j; the normalising sum is a Python-ordered loop over 11 bins
    matching       D accumulated bin by bin from 0.0; np.argmin returns the first (lowest) index of the minimum
    scoring        the front end's ((r0 x + r1 y) + r2 z) + t and the matching's distance on arrays of dtype F
    draws          Python integers masked to 64 bits
"""
import numpy as np

import batch_outlier_ref as orf

BINS = 33
MIN_K, MAX_K = 3, 32
MASK = (1 << 64) - 1


# ---- descriptors -----------------------------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def diamond(x, y):
    """t in [-2, 2], monotone in atan2(y, x)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.abs(x) + np.abs(y)
        q = y / s
        return np.where(s == 0, 0.0, np.where(x >= 0, q, np.where(y >= 0, 2.0 - q, -2.0 - q)))


def bin_of(val, lo, width):
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((11.0 * (val - lo)) / width)
        return np.where(f >= 10.0, 10, np.where(f >= 0.0, f, 0.0)).astype(np.int64)   # (a NaN lands in bin 0)


def neighbourhood(X, k):
    """(d (n, n) of dtype F, tau (n,) of dtype F, nb (n, n) bool: j != i and d2(i, j) <= tau_i)"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    assert MIN_K <= k <= MAX_K and n >= k + 1
    d = orf.d2_rows(X, 0, n)
    off = d.copy()
    off[np.arange(n), np.arange(n)] = np.inf
    tau = np.partition(off, k - 1, axis=1)[:, k - 1]
    nb = d <= tau[:, None]
    nb[np.arange(n), np.arange(n)] = False
    return d, tau, nb


def pair_terms(X, N, ii, jj):
    """(ok, t, f2, f3) of the pairs (ii[e], jj[e]): ok False where the pair is skipped"""
    X64, N = np.asarray(X, dtype=np.float64), np.asarray(N, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dx, dy, dz = (X64[jj, a] - X64[ii, a] for a in range(3))
        r2 = (dx * dx + dy * dy) + dz * dz
        ok = (r2 != 0) & np.isfinite(r2)
        r = np.sqrt(r2)
        nix, niy, niz = (N[ii, a] for a in range(3))
        njx, njy, njz = (N[jj, a] for a in range(3))
        a1 = _dot(nix, niy, niz, dx, dy, dz) / r
        a2 = _dot(njx, njy, njz, dx, dy, dz) / r
        sw = np.abs(a1) < np.abs(a2)
        n1x, n1y, n1z = np.where(sw, njx, nix), np.where(sw, njy, niy), np.where(sw, njz, niz)
        n2x, n2y, n2z = np.where(sw, nix, njx), np.where(sw, niy, njy), np.where(sw, niz, njz)
        dx, dy, dz = np.where(sw, -dx, dx), np.where(sw, -dy, dy), np.where(sw, -dz, dz)
        f3 = np.where(sw, -a2, a1)
        vx, vy, vz = dy * n1z - dz * n1y, dz * n1x - dx * n1z, dx * n1y - dy * n1x
        vv = _dot(vx, vy, vz, vx, vy, vz)
        ok &= (vv != 0) & np.isfinite(vv)
        sv = np.sqrt(vv)
        vx, vy, vz = vx / sv, vy / sv, vz / sv
        wx, wy, wz = n1y * vz - n1z * vy, n1z * vx - n1x * vz, n1x * vy - n1y * vx
        f2 = _dot(vx, vy, vz, n2x, n2y, n2z)
        x = _dot(n1x, n1y, n1z, n2x, n2y, n2z)
        y = _dot(wx, wy, wz, n2x, n2y, n2z)
        t = diamond(x, y)
    return ok, t, f2, f3


def spfh(X, N, k, hood=None):
    """(S (n, 33) float64, c (n,) the pair terms not skipped)"""
    n = X.shape[0]
    d, tau, nb = neighbourhood(X, k) if hood is None else hood
    ii, jj = np.nonzero(nb)
    ok, t, f2, f3 = pair_terms(X, N, ii, jj)
    cnt = np.zeros((n, BINS), dtype=np.int64)
    i = ii[ok]
    np.add.at(cnt, (i, bin_of(t[ok], -2.0, 4.0)), 1)
    np.add.at(cnt, (i, 11 + bin_of(f2[ok], -1.0, 2.0)), 1)
    np.add.at(cnt, (i, 22 + bin_of(f3[ok], -1.0, 2.0)), 1)
    c = np.bincount(i, minlength=n)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(c[:, None] > 0, (100.0 * cnt.astype(np.float64)) / c.astype(np.float64)[:, None], 0.0)
    return S, c


def fpfh(X, N, k):
    """(n, 33) float64: the descriptors of the cloud X (dtype F) with the normals N (float64) from k neighbours"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    hood = neighbourhood(X, k)
    d, tau, nb = hood
    S, _ = spfh(X, N, k, hood)
    use = nb & (d != 0)
    A = np.zeros((n, BINS))
    ii, jj = np.nonzero(use)                                   # row-major: ascending j within a row
    start = np.searchsorted(ii, np.arange(n))
    count = np.bincount(ii, minlength=n)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for r in range(int(count.max()) if count.size else 0):
            rows = np.flatnonzero(count > r)
            j = jj[start[rows] + r]
            wgt = 1.0 / d[rows, j].astype(np.float64)
            A[rows] = A[rows] + S[j] * wgt[:, None]
        F = np.zeros((n, BINS))
        for h in range(3):
            s = np.zeros(n)
            for b in range(11):
                s = s + A[:, 11 * h + b]
            ok = (s > 0) & np.isfinite(s)
            F[:, 11 * h:11 * h + 11] = np.where(ok[:, None], (A[:, 11 * h:11 * h + 11] * 100.0) / s[:, None], 0.0)
    return F


# ---- matching --------------------------------------------------------------------------------------------------------------------
def match(F, G, mutual=True):
    """(fwd (n,) int32, rev (m,) int32, kept (n,) uint8)"""
    F, G = np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64)
    D = np.zeros((F.shape[0], G.shape[0]))
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(BINS):
            e = F[:, b, None] - G[None, :, b]
            D = D + e * e
    D = np.where(np.isnan(D), np.inf, D)
    fwd = np.argmin(D, axis=1).astype(np.int32)
    rev = np.argmin(D, axis=0).astype(np.int32)
    kept = np.ones(F.shape[0], dtype=np.uint8) if not mutual else (rev[fwd] == np.arange(F.shape[0])).astype(np.uint8)
    return fwd, rev, kept


def correspondences(fwd, kept):
    i = np.flatnonzero(kept).astype(np.int32)
    return i, fwd[i]


# ---- scoring ---------------------------------------------------------------------------------------------------------------------
def hits(P, Q, ci, cj, T, max_distance):
    """(C,) bool: which entries of the list count for the pose T (rounded once to the clouds' dtype F here)"""
    F = P.dtype.type
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3].astype(P.dtype), T[:3, 3].astype(P.dtype)
    x, y, z = (np.ascontiguousarray(P[ci, a]) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        o = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)]
        G = Q[cj]
        dx, dy, dz = G[:, 0] - o[0], G[:, 1] - o[1], G[:, 2] - o[2]
        d = (dx * dx + dy * dy) + dz * dz
        thr = F(float(max_distance) * float(max_distance))
        fin = np.isfinite(o[0]) & np.isfinite(o[1]) & np.isfinite(o[2])
        return fin & (d <= thr)


def score(P, Q, ci, cj, T, max_distance):
    return int(hits(P, Q, ci, cj, T, max_distance).sum())


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------------
def mix(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, h, r, C):
    return mix((mix((mix(seed) + h) & MASK) + r) & MASK) % C


def triple(seed, h, C):
    """the list positions of slots 0, 1, 2 (-1: left empty)"""
    slot = []
    for r in range(16):
        if len(slot) == 3:
            break
        v = draw(seed, h, r, C)
        if v not in slot:
            slot.append(v)
    return slot + [-1] * (3 - len(slot))


def kabsch(p, q):
    """the rotation and translation that carry the points p (k, 3) onto q in the least-squares sense, det = +1, as a 4 x 4"""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    pb, qb = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((q - qb).T @ (p - pb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, qb - R @ pb
    return T


def edges_ok(p, q, e):
    if e <= 0:
        return True
    for a, b in ((0, 1), (1, 2), (0, 2)):
        d = p[a] - p[b]
        la = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        d = q[a] - q[b]
        lb = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if not (la >= e * lb and lb >= e * la):
            return False
    return True


def hypotheses(P, Q, ci, cj, seed, H, e):
    """(triples (H, 3) int32, valid (H,) uint8): the draws and the edge check of every hypothesis"""
    C = len(ci)
    tr = np.full((H, 3), -1, dtype=np.int32)
    valid = np.zeros(H, dtype=np.uint8)
    if C < 3:
        return tr, valid
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    for h in range(H):
        s = triple(seed, h, C)
        tr[h] = s
        if s[2] < 0:
            continue
        valid[h] = 1 if edges_ok(P64[ci[s]], Q64[cj[s]], e) else 0
    return tr, valid


def ransac(P, Q, ci, cj, seed, H, max_distance, e):
    """the whole driver: dict(T, inliers, status (0 / "empty"), winner, triples, valid, counts)"""
    tr, valid = hypotheses(P, Q, ci, cj, seed, H, e)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    counts = np.full(H, -1, dtype=np.int32)
    Ts = np.tile(np.eye(4), (H, 1, 1))
    for h in np.flatnonzero(valid):
        Ts[h] = kabsch(P64[ci[tr[h]]], Q64[cj[tr[h]]])
        counts[h] = score(P, Q, ci, cj, Ts[h], max_distance)
    if not valid.any():
        return dict(T=np.eye(4), inliers=0, status="empty", winner=-1, triples=tr, valid=valid, counts=counts)
    best = int(np.argmax(np.where(valid > 0, counts, -1)))     # the first of the largest: the lowest h among equals
    T, inl = Ts[best], int(counts[best])
    hit = hits(P, Q, ci, cj, T, max_distance)
    if hit.sum() >= 3:
        T2 = kabsch(P64[ci[hit]], Q64[cj[hit]])
        c2 = score(P, Q, ci, cj, T2, max_distance)
        if c2 >= inl:
            T, inl = T2, c2
    return dict(T=T, inliers=inl, status=0, winner=best, triples=tr, valid=valid, counts=counts)


# ---- clouds and normals ----------------------------------------------------------------------------------------------------------
def oriented_normals(points, cov6, viewpoint):
    """engine.oriented_normals, restated: the eigenvector of the smallest eigenvalue of every covariance, flipped to face viewpoint"""
    C6 = np.asarray(cov6, dtype=np.float64)
    ix = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    _, Z = np.linalg.eigh(C6[:, ix])
    N = Z[:, :, 0]
    to = np.asarray(viewpoint, dtype=np.float64)[None, :] - np.asarray(points, dtype=np.float64)
    flip = (N * to).sum(1) < 0
    N = np.where(flip[:, None], -N, N)
    return np.ascontiguousarray(N)


def blob(seed, n, dtype):
    """n points on a bumpy sphere, with their outward unit normals (float64)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 1.0 + 0.15 * np.sin(3.0 * v[:, 0]) * np.cos(2.0 * v[:, 1]) + 0.1 * v[:, 2]
    X = np.ascontiguousarray((v * r[:, None]).astype(dtype))
    Nn = v + 0.2 * rng.standard_normal((n, 3))
    Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    return X, np.ascontiguousarray(Nn)


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def angle_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


BUNNY_STEP, BUNNY_T = 24, np.array([0.05, -0.03, 0.08])


def bunny_pair(golden):
    """the issue's pair: every 24th point of the bunny from 0, turned 149 degrees about (1, 2, 3) and shifted, against every 24th
    from 12 -- 1 498 points each, disjoint samples.  (moving, model, T_true): T_true carries the moving cloud onto the model"""
    import os
    B = np.fromfile(os.path.join(golden, "bunny_xyz_f32.bin"), dtype=np.float32).reshape(-1, 3)
    src, model = B[0::BUNNY_STEP], np.ascontiguousarray(B[12::BUNNY_STEP])
    R = rodrigues((1.0, 2.0, 3.0), 149.0)
    moving = np.ascontiguousarray((src.astype(np.float64) @ R.T + BUNNY_T).astype(np.float32))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ BUNNY_T
    return moving, model, T
