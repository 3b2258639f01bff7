"""numpy restatement of batched Fast Global Registration (icp_batch_fgr; the rules: include/icp_mi355x.h).  Everything is float64
from coordinates widened once; every numpy operation below is one rounding of the header's statement, in its order.

    used_list    every correspondence, or the list positions that occur in a valid triple of RANSAC's generator (each once, ascending)
    scale        pbar, qbar (sequential sums in list order), D2, the start value of mu
    schedule     mu of every iteration
    terms        what one used correspondence adds to every slot of an iteration's vector, and its weight l
    exact_sums   math.fsum of the terms and of their absolute values: the device adds the same terms in another order
    solve        icp_solve_point_to_plane, restated operation by operation (None: not positive definite)
    fgr          the driver: dict(T, weights, used, objective, status, mu_hist, mom_hist, T_hist)

The tolerance of a sum is ref_moments.tolerance(maj, U) = 2 (U + 16) 2^-53 A_s: derived there, nothing is tuned here."""
import math

import numpy as np

import batch_feature_ref as fr
import ref_moments as rm

OK, EMPTY, SINGULAR = 0, -4, -5        # ICP_OK, ICP_ERR_EMPTY, ICP_ERR_SINGULAR
W = 29                                 # ICP_MOM_W
FGR_SLOTS = (rm.ERR, rm.CNT) + rm.PLANE_SLOTS + (W,)


# ---- the used list, the scale, the schedule --------------------------------------------------------------------------------------
def used_list(P, Q, ci, cj, seed, tuples, similarity):
    """(U,) int32: positions in the correspondence list, ascending"""
    C = len(ci)
    if tuples == 0:
        return np.arange(C, dtype=np.int32)
    tr, valid = fr.hypotheses(P, Q, ci, cj, seed, tuples, similarity)
    return np.unique(tr[valid > 0]).astype(np.int32)      # each position once, however often it was drawn


def drawn(seed, tuples, C):
    """every list position a hypothesis with three distinct picks drew (the used list with the similarity 0)"""
    if C < 3:
        return np.zeros(0, dtype=np.int32)
    s = [fr.triple(seed, h, C) for h in range(tuples)]
    return np.unique([v for t in s if t[2] >= 0 for v in t]).astype(np.int32)


def scale(Pu, Qu):
    """(D2, pbar, qbar) of the used points (U, 3) float64 of both sides"""
    U = Pu.shape[0]
    with np.errstate(all="ignore"):
        pbar = np.array([np.cumsum(Pu[:, a])[-1] for a in range(3)]) / float(U)     # (cumsum adds in order)
        qbar = np.array([np.cumsum(Qu[:, a])[-1] for a in range(3)]) / float(U)
        d2 = []
        for X, c in ((Pu, pbar), (Qu, qbar)):
            dx, dy, dz = X[:, 0] - c[0], X[:, 1] - c[1], X[:, 2] - c[2]
            d2.append((dx * dx + dy * dy) + dz * dz)
        d2 = np.concatenate(d2)
    D2 = float("nan") if np.isnan(d2).any() else float(d2.max())
    return D2, pbar, qbar


def schedule(D2, delta, iterations, division_factor, decrease_every):
    mu, out = float(D2), []
    d2 = float(delta) * float(delta)
    for it in range(iterations):
        if it % decrease_every == 0 and mu > d2:
            mu = max(mu / float(division_factor), d2)
        out.append(mu)
    return np.array(out)


# ---- one iteration ---------------------------------------------------------------------------------------------------------------
def terms(Pu, Qu, T, mu):
    """(t (U, 32), l (U,), ok (U,) bool): the terms of every used correspondence at the pose T, its weight, and whether it counts
    (p and r2 finite; the terms and the weight of the others are not to be used: the device adds nothing and reports 0.0)"""
    Pu, Qu, T = np.asarray(Pu, dtype=np.float64), np.asarray(Qu, dtype=np.float64), np.asarray(T, dtype=np.float64)
    U = Pu.shape[0]
    mu = np.float64(mu)
    x, y, z = Pu[:, 0], Pu[:, 1], Pu[:, 2]
    with np.errstate(all="ignore"):
        p = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
        e = [p[a] - Qu[:, a] for a in range(3)]
        r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        s = mu / (mu + r2)
        l = s * s
        ok = np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2]) & np.isfinite(r2)
        zero, one = np.zeros(U), np.ones(U)
        cn = [(zero, p[2], -p[1], one, zero, zero), (-p[2], zero, p[0], zero, one, zero), (p[1], -p[0], zero, zero, zero, one)]
        w = [[l * cn[a][r] for r in range(6)] for a in range(3)]
        t = np.zeros((U, rm.NMOM))
        t[:, rm.CNT] = 1.0
        o = rm.MC
        for r in range(6):
            for c in range(r, 6):
                t[:, o] = (w[0][r] * cn[0][c] + w[1][r] * cn[1][c]) + w[2][r] * cn[2][c]
                o += 1
        for r in range(6):
            t[:, rm.MB + r] = -((w[0][r] * e[0] + w[1][r] * e[1]) + w[2][r] * e[2])
        t[:, W] = l
        d = 1.0 - s
        t[:, rm.ERR] = l * r2 + mu * (d * d)
    return t, l, ok


def exact_sums(t, ok):
    """(moments[32], majorants[32]) over the rows that count"""
    mom, maj = np.zeros(rm.NMOM), np.zeros(rm.NMOM)
    rows = t[np.asarray(ok, dtype=bool)]
    for s in FGR_SLOTS:
        mom[s] = math.fsum(rows[:, s].tolist())
        maj[s] = math.fsum(np.abs(rows[:, s]).tolist())
    return mom, maj


def tolerance(maj, U):
    return rm.tolerance(maj, U)


def solve(mom):
    """icp_solve_point_to_plane on the vector's slots C and B, operation by operation: (R (3, 3), t (3,)), or None where the
    Cholesky factorisation meets a pivot that is not > 0"""
    Uc = [[0.0] * 6 for _ in range(6)]
    o = rm.MC
    for a in range(6):
        for c in range(a, 6):
            Uc[a][c] = float(mom[o])
            o += 1
    for k in range(6):
        d = Uc[k][k]
        for r in range(k):
            d -= Uc[r][k] * Uc[r][k]
        if not d > 0.0:
            return None
        d = math.sqrt(d)
        Uc[k][k] = d
        for c in range(k + 1, 6):
            s = Uc[k][c]
            for r in range(k):
                s -= Uc[r][k] * Uc[r][c]
            Uc[k][c] = s / d
    yv, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = float(mom[rm.MB + i])
        for r in range(i):
            s -= Uc[r][i] * yv[r]
        yv[i] = s / Uc[i][i]
    for i in range(5, -1, -1):
        s = yv[i]
        for c in range(i + 1, 6):
            s -= Uc[i][c] * x[c]
        x[i] = s / Uc[i][i]
    cx, cy, cz, sx, sy, sz = math.cos(x[0]), math.cos(x[1]), math.cos(x[2]), math.sin(x[0]), math.sin(x[1]), math.sin(x[2])
    R = np.array([[cy * cz, cz * sx * sy - cx * sz, cx * cz * sy + sx * sz],
                  [cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx],
                  [-sy, cy * sx, cx * cy]])
    return R, np.array(x[3:6])


def compose(R, t, T):
    """S T for S = [R t; 0 1]: every entry (s0 a + s1 b) + s2 c, the translation + t"""
    out = np.eye(4)
    for a in range(3):
        for c in range(4):
            v = (R[a, 0] * T[0, c] + R[a, 1] * T[1, c]) + R[a, 2] * T[2, c]
            out[a, c] = v + t[a] if c == 3 else v
    return out


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def fgr(P, Q, ci, cj, delta, iterations=64, division_factor=1.4, decrease_every=4, tuples=0, tuple_similarity=0.95, seed=0):
    """icp_batch_fgr for one pair.  The sums of an iteration are exact_sums' (the device's differ within the tolerance)"""
    n = P.shape[0]
    used = used_list(P, Q, ci, cj, seed, tuples, tuple_similarity)
    out = dict(T=np.eye(4), weights=np.zeros(n), used=used, objective=0.0, status=EMPTY, mu_hist=np.zeros(iterations),
               mom_hist=np.zeros((iterations, rm.NMOM)), T_hist=np.zeros((iterations, 4, 4)))
    if used.size < 3:
        return out
    Pu, Qu = P[ci[used]].astype(np.float64), Q[cj[used]].astype(np.float64)
    D2, _, _ = scale(Pu, Qu)
    if not (np.isfinite(D2) and D2 > 0):
        return out
    mus = schedule(D2, delta, iterations, division_factor, decrease_every)
    T, status = np.eye(4), OK
    for it in range(iterations):
        t, _, ok = terms(Pu, Qu, T, mus[it])
        mom, _ = exact_sums(t, ok)
        out["mu_hist"][it], out["mom_hist"][it], out["T_hist"][it] = mus[it], mom, T
        out["objective"] = float(mom[rm.ERR])
        s = solve(mom)
        if s is not None:
            Tn = compose(s[0], s[1], T)
        if s is None or not np.isfinite(Tn).all():
            status = SINGULAR
            break
        T = Tn
    _, l, ok = terms(Pu, Qu, T, mus[min(it, iterations - 1)])
    out["T"], out["status"] = T, status
    out["weights"][ci[used]] = np.where(ok, l, 0.0)
    return out


# ---- planted pairs ---------------------------------------------------------------------------------------------------------------
def planted_pair(seed, n, dtype, wrong=3):
    """test_gpu_batch_feature.ransac_pair: a cloud, its rigidly moved copy, and descriptors whose forward matches are right except
    for every `wrong`-th point.  (P, Q, F, G, T)"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, 3)).astype(dtype)
    R, t = fr.rodrigues(rng.standard_normal(3), 140.0), rng.uniform(-1, 1, 3)
    Q = (P.astype(np.float64) @ R.T + t).astype(dtype)
    target = np.arange(n)
    target[::wrong] = rng.integers(0, n, target[::wrong].size)
    G = np.round(rng.uniform(0, 100, (n, 33)), 2)
    F = np.ascontiguousarray(G[target])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return P, Q, F, G, T


def collinear_pair(dtype):
    """three points on the x axis and their copy pushed 0.5 along it, matched one to one: at the identity row and column rx of C
    are exactly zero -- the first pivot of the factorisation is 0 whatever the order of the sums"""
    P = np.array([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0]], dtype=dtype)
    Q = np.ascontiguousarray(P + np.array([0.5, 0.0, 0.0], dtype=dtype))
    G = np.zeros((3, 33))
    G[np.arange(3), np.arange(3)] = 50.0
    return P, Q, G.copy(), G
