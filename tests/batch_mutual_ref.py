"""What the tests of a batch's reciprocal matches share (tests/test_batch_mutual_ref.py, tests/test_gpu_batch_reciprocal.py): the
mutual rule as numpy states it, its combination with the gate and the trim, a numpy loop whose keep rule sees the clouds, and the
integer clouds with tied minima in both directions.  Everything else comes from batch_ref.py, which this module only imports.

The rule (include/icp_mi355x.h, icp_batch_set_reciprocal): idx[i] = the lowest j that minimises dist2(p_i, q_j), rev[j] = the
lowest i that minimises the same dist2 over the moving cloud, the match of i is mutual iff rev[idx[i]] == i.  dist2 squares its
differences, so nn(M, P) compares, for the pair (j, i), the very number nn(P, M) compares for (i, j)."""
import numpy as np

import ref_numpy
from batch_ref import hom, rank, sq_dist, tau_ref, threshold


def mutual_mask(orc, P, M):
    """idx, rev, mask: the forward matches, the reverse matches, and where the two agree"""
    idx = orc.nn(P, M)
    rev = orc.nn(M, P)
    return idx, rev, rev[idx] == np.arange(P.shape[0])


def mutual_mask_numpy(P, M):
    """the same through ref_numpy.nn alone (a second opinion on orc.nn in both directions)"""
    idx = ref_numpy.nn(P, M)
    rev = ref_numpy.nn(M, P)
    return idx, rev, rev[idx] == np.arange(P.shape[0])


def combined_mask(P, M, idx, rev, md=None, rho=None, mutual=True):
    """kept = mutual && d <= tau && d <= thr, three independent tests: tau is the K-th smallest of ALL n winning distances (None: no
    trim), thr = (F)(md * md) (None: no gate).  Returns (mask, d, tau) -- tau is +inf in P's dtype without a trim"""
    d = sq_dist(P, M, idx)
    mask = (rev[idx] == np.arange(P.shape[0])) if mutual else np.ones(P.shape[0], dtype=bool)
    tau = P.dtype.type(np.inf)
    if rho is not None and float(rho) != 1.0:
        tau = tau_ref(d, rank(rho, P.shape[0]))
        mask = mask & (d <= tau)
    if md is not None:
        mask = mask & (d <= threshold(md, P.dtype))
    return mask, d, tau


def keep_mutual(orc, md=None, rho=None):
    """mutual_loop's rule: reciprocal matches, with a gate at md and / or a trim to the share rho"""
    def keep(P, M, idx):
        return combined_mask(P, M, idx, orc.nn(M, P), md, rho)[0]
    return keep


def mutual_loop(orc, A, M, keep, max_iter, tol):
    """batch_ref.reference_loop with a keep rule that sees (P, M, idx): orc.nn + keep + ref_numpy.minimize on the kept points; the
    error over the kept points, divided by their count.  A pass that keeps nothing ends the loop.  kept: the count of every pass;
    masks: its mask (mask: the last)"""
    P = A.copy()
    E, T, i, kept, masks = [0.0], np.eye(4), 0, [], []
    while True:
        idx = orc.nn(P, M)
        mask = keep(P, M, idx)
        kept.append(int(mask.sum()))
        masks.append(mask)
        if not mask.any():
            break
        R, t = ref_numpy.minimize(P[mask], M, idx[mask])
        P = (P.astype(np.float64) @ R.T + t).astype(A.dtype)
        T = hom(R, t) @ T
        diff = M[idx][mask].astype(np.float64) - P[mask].astype(np.float64)
        E.append(float(np.sqrt((diff ** 2).sum() / mask.sum())))
        if E[-1] < tol or abs(E[-1] - E[-2]) < tol:
            break
        i += 1
        if i > max_iter - 1:
            break
    return dict(iterations=i, err=np.array(E), T=T, kept=kept, masks=masks, mask=masks[-1])


def tie_clouds(dtype):
    """the integer clouds of test_gpu_batch_trim.test_trim_keeps_every_point_tied_with_the_kth: 200 points with coordinates 0 .. 7
    against the 5 x 5 x 5 grid of even coordinates -- every distance is a small integer, minima are tied in both directions"""
    A = np.random.default_rng(5).integers(0, 8, (200, 3)).astype(dtype)
    g = np.arange(5) * 2
    M = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(dtype)
    return A, M


def all_sq_dist(P, M):
    """(n, m): every (dx*dx + dy*dy) + dz*dz, rounded in P's dtype"""
    return ref_numpy._sq_dist_rows(np.ascontiguousarray(P), np.ascontiguousarray(M, dtype=P.dtype))


def nn_highest(P, M):
    """the HIGHEST j that minimises dist2(p_i, q_j): what a search that broke ties the other way would answer"""
    D = all_sq_dist(P, M)
    return (D.shape[1] - 1 - np.argmin(D[:, ::-1], axis=1)).astype(np.int32)
