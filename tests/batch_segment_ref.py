"""What the plane segmentation tests share (tests/test_batch_segment_ref.py, test_batch_segment_abi.py, test_gpu_batch_segment.py):
the rule of icp_batch_segment_plane in numpy, bit for bit as include/icp_mi355x.h states it.  Nothing here touches a device.

    draws       batch_feature_ref's generator (Python integers masked to 64 bits) on the seed (seed_p + side) mod 2^64
    plane       u, v, the cross product, l, the three divisions, the sign rule, d -- one float64 operation per statement
    axis        ahat by three divisions, fabs of the grouped dot product against min_cos
    score       ((nx*x + ny*y) + nz*z) + d on float64 arrays, fabs(s) <= distance (a NaN compares false)
    winner      np.argmax returns the first (lowest) index of the maximum
    refit       granules of 64 consecutive points; np.cumsum adds sequentially (np.sum adds pairwise: not used), from a leading 0.0
    Jacobi      batch_normals_ref.jacobi: icp_eigh3's statements with the range rule, column 0 of the ordered vectors
"""
import numpy as np

import batch_feature_ref as fr
import batch_normals_ref as nr

NONE, DETECT, REMOVE, KEEP = 0, 1, 2, 3   # ICP_PLANE_NONE, ICP_PLANE_DETECT, ICP_PLANE_REMOVE, ICP_PLANE_KEEP
OK, ERR_EMPTY = 0, -4
GRANULE = 64
GROUP, CHUNK = 32, 4096   # hypotheses per block and per launch of batch_plane_score: the sizes at which the device code changes path


def rule(kind, distance, hypotheses=1000, axis=(0.0, 0.0, 0.0), min_cos=0.0):
    return dict(kind=kind, distance=float(distance), hypotheses=int(hypotheses), axis=tuple(float(x) for x in axis), min_cos=float(min_cos))


def as_tuple(r):
    """the rule as Batch.segment_plane takes it (None: copy)"""
    if r is None or r["kind"] == NONE:
        return None
    return ({DETECT: "detect", REMOVE: "remove", KEEP: "keep"}[r["kind"]], r["distance"], r["hypotheses"], r["axis"], r["min_cos"])


def _seq(v):
    """the sum of v from 0.0 in ascending index"""
    return np.cumsum(np.concatenate([[0.0], np.asarray(v, dtype=np.float64)]))[-1]


def sign_rule(n):
    """all three components negated iff the component of largest magnitude is negative; the lowest index decides among equals"""
    k = 0
    for a in (1, 2):
        if np.fabs(n[a]) > np.fabs(n[k]):
            k = a
    return -n if n[k] < 0.0 else n


def plane_from_points(a, b, c):
    """((4,) float64, ok): the rule's plane of three points; four zeros where the hypothesis is invalid"""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        w = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        l = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        if not (l > 0.0 and np.isfinite(l)):
            return np.zeros(4), False
        n = sign_rule(w / l)
        d = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2])
    return np.array([n[0], n[1], n[2], d]), True


def plane_from_moments(c, cov6):
    """((4,) float64, ok): the refit's last step"""
    c = np.asarray(c, dtype=np.float64)
    _, n, _ = nr.jacobi(np.asarray(cov6, dtype=np.float64).reshape(6, 1))
    n = n[:, 0]
    if not np.isfinite(n).all() or (n == 0.0).all():
        return np.zeros(4), False
    n = sign_rule(n)
    with np.errstate(all="ignore"):
        d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
    return np.array([n[0], n[1], n[2], d]), True


def axis_ok(plane, axis, min_cos):
    ax = np.asarray(axis, dtype=np.float64)
    if (ax == 0.0).all():
        return True
    with np.errstate(all="ignore"):
        la = np.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
        h = ax / la
        return bool(np.fabs((plane[0] * h[0] + plane[1] * h[1]) + plane[2] * h[2]) >= min_cos)


def on_plane(X64, plane, distance):
    """(n,) bool: fabs(((nx*x + ny*y) + nz*z) + d) <= distance"""
    with np.errstate(all="ignore"):
        s = ((plane[0] * X64[:, 0] + plane[1] * X64[:, 1]) + plane[2] * X64[:, 2]) + plane[3]
        return np.fabs(s) <= distance


def hypotheses(X, seed, side, r):
    """(triples (H, 3) int32, valid (H,) uint8, planes (H, 4)) of one cloud"""
    X64 = np.asarray(X).astype(np.float64)
    n, H = X64.shape[0], r["hypotheses"]
    s = (int(seed) + int(side)) & fr.MASK
    tr, va, pl = np.full((H, 3), -1, dtype=np.int32), np.zeros(H, dtype=np.uint8), np.zeros((H, 4))
    for h in range(H):
        t = fr.triple(s, h, n)
        tr[h] = t
        if t[2] < 0:
            continue
        p, ok = plane_from_points(X64[t[0]], X64[t[1]], X64[t[2]])
        if ok and axis_ok(p, r["axis"], r["min_cos"]):
            va[h], pl[h] = 1, p
    return tr, va, pl


def counts(X64, valid, planes, distance):
    """(H,) int32: the inliers of every valid hypothesis, -1 for an invalid one"""
    out = np.full(valid.shape[0], -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for h0 in range(0, valid.shape[0], 256):
            P = planes[h0:h0 + 256]
            s = ((P[:, 0:1] * X64[None, :, 0] + P[:, 1:2] * X64[None, :, 1]) + P[:, 2:3] * X64[None, :, 2]) + P[:, 3:4]
            c = (np.fabs(s) <= distance).sum(axis=1).astype(np.int32)
            out[h0:h0 + 256] = np.where(valid[h0:h0 + 256] != 0, c, -1)
    return out


def moments(X64, mask):
    """(c (3,), cov6 (6,), k): the refit's sums over the points where mask, in the granule order"""
    n = X64.shape[0]
    k = int(mask.sum())
    kk = np.float64(k)
    with np.errstate(all="ignore"):
        def total(vals):
            return _seq([_seq(vals[g:g + GRANULE][mask[g:g + GRANULE]]) for g in range(0, n, GRANULE)])
        c = np.array([total(X64[:, a]) for a in range(3)]) / kk
        e = X64 - c[None, :]
        cov = np.array([total(e[:, a] * e[:, b]) / kk for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    return c, cov, k


def segment(X, r, seed=0, side=0):
    """everything icp_batch_segment_plane and icp_diag_batch_segment report for one cloud X (n, 3) under rule r (None: copy): a dict
    of triples, valid, planes, counts (the hypotheses), status, plane (4,), inliers, mask (n,) uint8, map (n,) int32, cloud (the new
    cloud, X's dtype), winner (the winning h, -1: none), refit (the refit was returned)"""
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    out = dict(status=OK, plane=np.zeros(4), inliers=0, mask=np.zeros(n, dtype=np.uint8), map=np.arange(n, dtype=np.int32), cloud=X.copy(),
               winner=-1, refit=False, triples=None, valid=None, planes=None, counts=None)
    if r is None or r["kind"] == NONE:
        return out
    X64 = X.astype(np.float64)
    tr, va, pl = hypotheses(X, seed, side, r)
    cn = counts(X64, va, pl, r["distance"])
    out.update(triples=tr, valid=va, planes=pl, counts=cn)
    if not va.any():
        out["status"] = ERR_EMPTY
        if r["kind"] == KEEP:
            out.update(map=np.full(n, -1, dtype=np.int32), cloud=X[:0].copy())
        return out
    best = int(np.argmax(cn))                                   # (invalid: -1, below every count; the first of the largest)
    plane, cw = pl[best].copy(), int(cn[best])
    out["winner"] = best
    if cw >= 3:
        c, cov, _ = moments(X64, on_plane(X64, plane, r["distance"]))
        fit, ok = plane_from_moments(c, cov)
        if ok and axis_ok(fit, r["axis"], r["min_cos"]):
            cr = int(on_plane(X64, fit, r["distance"]).sum())
            if cr >= cw:
                plane, cw = fit, cr
                out["refit"] = True
    inl = on_plane(X64, plane, r["distance"])
    keep = np.ones(n, dtype=bool) if r["kind"] == DETECT else ~inl if r["kind"] == REMOVE else inl
    out.update(plane=plane, inliers=cw, mask=inl.astype(np.uint8), map=np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32),
               cloud=np.ascontiguousarray(X[keep]))
    return out


def segment_pairs(pairs, moving, model, seeds):
    """the reference of a whole batch: (moving, model), per pair the dict of segment; moving, model: per pair a rule or None"""
    return ([segment(p[0], r, s, 0) for p, r, s in zip(pairs, moving, seeds)], [segment(p[1], r, s, 1) for p, r, s in zip(pairs, model, seeds)])


# ---- clouds the tests share -------------------------------------------------------------------------------------------------------
def planted(n, share, dtype, seed=0, normal=(0.0, 0.0, 1.0), offset=0.25, noise=0.002):
    """n points in the unit cube of which the first round(share * n) lie within `noise` of the plane normal . x = offset, shuffled"""
    rng = np.random.default_rng(seed)
    nv = np.asarray(normal, dtype=np.float64)
    nv = nv / np.linalg.norm(nv)
    X = rng.uniform(-1.0, 1.0, (n, 3))
    k = int(round(share * n))
    X[:k] += ((offset + rng.uniform(-noise, noise, k)) - X[:k] @ nv)[:, None] * nv[None, :]
    return np.ascontiguousarray(X[rng.permutation(n)].astype(dtype))


HALL_RULE = rule(REMOVE, 0.02, 1000)   # the hall tests' rule: 1 000 hypotheses, 2 cm, no axis
HALL_SEED = 2024
_hall = {}


def hall():
    """the hall pair (fp32, metres) converted on the CPU by the oracle from the golden ranges, the zero returns dropped from both
    clouds: (P (n, 3), Q (n, 3)); made once"""
    if "pair" not in _hall:
        import os

        import oracle_lib
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        ranges = np.fromfile(os.path.join(golden, "hall_ranges_u32.bin"), dtype=np.uint32)
        P, Q = oracle_lib.Oracle().hall_clouds(golden)
        keep = ranges != 0
        _hall["pair"] = (np.ascontiguousarray(P[keep]), np.ascontiguousarray(Q[keep]))
    return _hall["pair"]


def hall_reference():
    """segment of both hall clouds under HALL_RULE and HALL_SEED; made once, shared, never changed"""
    if "ref" not in _hall:
        P, Q = hall()
        _hall["ref"] = (segment(P, HALL_RULE, HALL_SEED, 0), segment(Q, HALL_RULE, HALL_SEED, 1))
    return _hall["ref"]
