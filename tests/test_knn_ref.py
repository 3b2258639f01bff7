"""CPU: what makes the clouds of tests/test_gpu_knn_normals.py tests of the point-to-plane front end -- conditions on the inputs and
on the references, shown with numpy and the oracle alone (no device).  knn_ref.knn4_rule is the oracle on every neighbour model the
suite had, and on every float64 cloud of the range (orc_knn4_f64 no longer lets an overflowed distance in); in float32 it is
orc_knn4_f32 below the sentinel and differs from it past it; every scale does to the distances what knn_ref says; the partly-inf
clouds hold every count of empty slots; the border twins tie across every border; the covariances are non-finite, subnormal and zero
where the normals test needs them to be; and the direction check has something to check.
(The existing grid, random and Bunny models come from the package's dataset functions: like other CPU tests here, this module needs
libicp_mi355x.so built, not a device.)"""
import numpy as np
import pytest

import clouds as cl
import knn_ref as kr
from batch_ref import knn_models

DTYPES = [np.float32, np.float64]
TINY = {np.float32: float(np.finfo(np.float32).tiny), np.float64: float(np.finfo(np.float64).tiny)}


def _names(dtype, scales, kinds=cl.FUZZ_KINDS, sizes=kr.SCALE_M):
    return [f"{kind}-{scale:g}-{m}" for scale in scales for kind in kinds for m in sizes]


# ---- the rule is the oracle wherever the oracle is the rule ------------------------------------------------------------------------
def _existing_models(pkg, orc, golden):
    from test_gpu_plane_and_programs import _clouds
    from test_oracle import far_surface_references
    out = [(f"knn_models[{k}] {M.dtype}", M) for dt in DTYPES for k, M in enumerate(knn_models(dt))]
    assert len(out) == 32
    out += [(which, _clouds(pkg, golden, which)[1]) for which in ("grid", "random", "bunny")]
    out.append(("hall", orc.hall_clouds(golden)[1]))
    out += [(f"fused_tie_lattice x{t}", cl.fused_tie_lattice(np.float64, t)) for t in (1, 3)]
    out.append(("far_surface", far_surface_references(orc, cl.FAR_OFF, cl.FAR_H)[0]))
    return out


def test_rule_is_the_oracle_on_every_existing_model(pkg, orc, golden):
    for name, M in _existing_models(pkg, orc, golden):
        nbr, d5 = kr.rule(M)
        assert np.array_equal(nbr, orc.knn4(M)), name
        assert np.isfinite(d5).all() and float(d5[:, 4].max()) < kr.SENTINEL, name     # (largest fifth distance: 14.8)


def test_rule_is_the_fixed_fp64_oracle_over_the_range(orc):
    """orc_knn4_f64 with "+inf enters nothing" on every float64 cloud of this suite; before, it listed the lowest indices where
    fewer than five distances are finite (lattice at 3e154, every kind at 1e160)"""
    seen_empty = 0
    for name, Q in kr.normals_clouds(np.float64):
        nbr, d5 = kr.rule(Q)
        assert np.array_equal(nbr, orc.knn4(Q)), name
        seen_empty += int(kr.empty_slots(d5).sum())
    assert seen_empty > 1000


def test_rule_is_the_fp32_letter_below_the_sentinel_only(orc):
    differ = {}
    for name, Q in kr.normals_clouds(np.float32):
        nbr, d5 = kr.rule(Q)
        below = bool((d5[:, 4] < kr.SENTINEL).all())
        same = np.array_equal(nbr, orc.knn4(Q))
        assert same or not below, name
        differ[name] = not same
    # the sentinel's reach, on record: the lattice at 60 and the uniform cloud at 1000 already differ
    assert differ["lattice-60-300"] and differ["uniform-1000-300"] and differ["uniform-1000-1025"]
    assert not differ["uniform-1-300"] and not differ["uniform-60-300"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_candidate_sort_is_the_plain_sort(dtype):
    """knn4_rule's sort over the candidates alone gives what np.argsort(kind="stable") of the whole row gives"""
    for name, Q in kr.normals_clouds(dtype) + [("twins-1025", kr.border_twins(1025, kr.GEOMETRY_256[1025], dtype)[0])]:
        fast, plain = kr.rule(Q), kr.knn4_rule(Q, plain=True)
        assert np.array_equal(fast[0], plain[0]) and fast[1].tobytes() == plain[1].tobytes(), name
    if dtype == np.float32:     # and on the largest clouds: rows around the middle of sized(12001) and of its border twins, whole rows
        for Q in (kr.sized(12001), kr.border_twins(12001, kr.GEOMETRY_256[12001])[0]):
            d = kr.sq_dist_rows(Q[5900:6156], Q)
            assert np.array_equal(kr._first_five(d, False), kr._first_five(d, True))


# ---- every scale does what its name says -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scales_do_what_their_names_say(dtype):
    assert kr.SCALES[np.float32] == (1e-25, 3e-22, 1e-20, 60.0, 1000.0, 1e15, 3e19, 1e20)
    assert kr.SCALES[np.float64] == (1e-170, 1e-157, 1e3, 1e150, 3e154, 1e160)
    assert set(kr.SCALES[dtype]) == ({kr.ZERO_SCALE[dtype], kr.PART_INF_SCALE[dtype], kr.INF_SCALE[dtype]} | set(kr.SUBNORMAL_SCALES[dtype]) |
                                     set(kr.SENTINEL_SCALES[dtype]) | set(kr.LARGE_SCALES[dtype]))
    clouds = dict(kr.scale_clouds(dtype))
    assert all(Q.dtype == dtype and np.isfinite(Q).all() for Q in clouds.values())
    table = lambda Q: kr.sq_dist_rows(Q, Q)
    for name in _names(dtype, [kr.ZERO_SCALE[dtype]]):
        assert (table(clouds[name]) == 0).all(), name
    for name in _names(dtype, kr.SUBNORMAL_SCALES[dtype]):
        d = table(clouds[name])
        assert (d < TINY[dtype]).all() and (d > 0).any(), name
    # fifth distance >= 10000 for at least half the queries: at 1000 on the lattice (whose smallest non-zero distance is scale^2) and
    # on the uniform cloud.  60 is where the sentinel begins to reach: the lattice's distances are multiples of 3600, and the few
    # queries at its rim with a fifth distance of 10800 (measured: 4 of 300) are enough for orc_knn4_f32 to leave the rule
    for scale in kr.SENTINEL_SCALES[dtype]:
        past = lambda name: kr.rule(clouds[name])[1][:, 4] >= kr.SENTINEL
        if scale >= 1000:
            for name in _names(dtype, [scale], ("lattice", "uniform")):
                assert past(name).mean() >= 0.5, name
        else:
            assert 4 <= past(f"lattice-{scale:g}-300").sum() < 150
    for name in _names(dtype, kr.LARGE_SCALES[dtype]):
        d = table(clouds[name])
        assert np.isfinite(d).all() and float(d.max()) > 1e26 * (1.0 if dtype == np.float32 else 1e270), name
    d = table(clouds["apart-300"])
    assert np.isinf(d[~np.eye(300, dtype=bool)]).all() and (np.diag(d) == 0).all()
    nbr, d5 = kr.rule(clouds["apart-300"])
    assert (nbr == 0).all() and (kr.empty_slots(d5) == 4).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_partly_inf_clouds_hold_every_count_of_empty_slots(dtype):
    """measured for the lattice of 300 points: 5 / 4 / 54 / 124 / 113 queries with 0 / 1 / 2 / 3 / 4 ranks that do not exist"""
    for m in kr.SCALE_M:
        Q = kr.scale_cloud("lattice", m, kr.PART_INF_SCALE[dtype], dtype)
        nbr, d5 = kr.rule(Q)
        count = np.bincount(kr.empty_slots(d5), minlength=5)
        assert (count >= 4).all(), (m, count)
        if m == 300:
            assert count.tolist() == [5, 4, 54, 124, 113]
        assert nbr.min() == 0 and nbr.max() < m
        # an empty slot is the last of its row: the existing ranks come first
        assert (np.diff(np.isfinite(d5).astype(int), axis=1) <= 0).all()


def test_signed_zeros_are_there():
    for dtype in DTYPES:
        Q = kr.scale_cloud("lattice", 300, 1.0 if dtype == np.float64 else 60.0, dtype)
        zero = Q == 0
        assert (np.signbit(Q) & zero).sum() > 50 and (~np.signbit(Q) & zero).sum() > 50


# ---- sizes and borders -----------------------------------------------------------------------------------------------------------------
def test_sizes_reach_every_launch_shape_on_256_cus():
    g = kr.GEOMETRY_256
    assert tuple(g) == kr.SIZED_M
    assert [g[m][1] for m in kr.SIZED_M[:4]] == [1, 1, 1, 2]                    # one query block, then two
    assert [g[m][2] for m in kr.SIZED_M] == [1, 1, 1, 1, 2, 3, 9, 11]           # model segments
    assert [g[m][4] for m in kr.SIZED_M] == [1, 1, 1, 1, 1, 1, 1, 2]            # LDS tiles per wave
    for m in kr.SIZED_M:
        assert kr.sized(m).shape == (m, 3) and kr.sized(m).dtype == np.float32


@pytest.mark.parametrize("m", kr.TWIN_M)
def test_border_twins_tie_across_every_border(m):
    geom = kr.GEOMETRY_256[m]
    brd = kr.borders(geom, m)
    assert len(brd) == 4 * geom[2] - 1 - sum(1 for s in range(geom[2]) for w in range(4) if s * geom[3] + w * (geom[3] // 4) >= m)
    Q, triples = kr.border_twins(m, geom)
    assert [t[2] for t in triples] == brd
    nbr, d5 = kr.rule(Q)
    for third, lo, hi in triples:
        assert Q[third].tobytes() == Q[lo].tobytes() == Q[hi].tobytes()
        # from each of the three copies the other two and itself are at distance 0, in index order: rank 0 is the third copy (the
        # lowest index, not the query itself), the first two neighbours are b - 1 and b -- the tie straddles the border
        for q in (third, lo, hi):
            assert tuple(nbr[q, :2]) == (lo, hi) and (d5[q, :3] == 0).all() and d5[q, 3] > 0, (third, lo, hi, q)
    # and nobody else coincides: every other tie would be an accident of the draw
    assert np.unique(Q, axis=0).shape[0] == m - 2 * len(triples)


def test_coincident_cloud():
    Q = kr.coincident(300)
    nbr, d5 = kr.rule(Q)
    assert (d5 == 0).all()
    assert np.array_equal(nbr[5:], np.tile(np.array([1, 2, 3, 4], dtype=np.int32), (295, 1)))
    assert np.array_equal(nbr[0], [1, 2, 3, 4]) and np.array_equal(nbr[1], [1, 2, 3, 4]) and np.array_equal(nbr[4], [1, 2, 3, 4])


# ---- covariances -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_covariances_are_what_the_normals_test_needs(dtype):
    clouds = dict(kr.normals_clouds(dtype))
    cov = lambda name: kr.covariance_rule(clouds[name], kr.rule(clouds[name])[0])
    for m in kr.SCALE_M:
        A, finite = cov(f"lattice-{kr.PART_INF_SCALE[dtype]:g}-{m}")
        assert (~finite).sum() >= 10 and finite.sum() >= 10, m
    for name in _names(dtype, kr.SUBNORMAL_SCALES[dtype]):
        A, finite = cov(name)
        assert finite.all() and float(np.abs(A).max()) < TINY[dtype], name
        # not all zero -- except the float32 clusters at 3e-22: they are 0.01 wide, every product of two of their differences is
        # below half the smallest subnormal, and their covariances are all zero (asserted: they are zero-covariance clouds here)
        if dtype == np.float32 and name.startswith("clustered-3e-22"):
            assert (A == 0).all(), name
        else:
            assert (np.abs(A).max(axis=(1, 2)) > 0).any(), name
    A, finite = cov("coincident-300")
    assert finite.all() and (A == 0).all()
    A, finite = cov("apart-300")            # every neighbour is point 0: a zero covariance, not an overflowed one
    assert finite.all() and (A == 0).all()
    # brink(): the origin's four neighbours are finite distances away, the diagonal of its covariance is finite (the largest finite
    # number), the xy entry is +inf: a test of the diagonal alone would let it through
    Q = clouds["brink-5"]
    nbr, d5 = kr.rule(Q)
    A, finite = cov("brink-5")
    assert np.array_equal(nbr[0], [1, 2, 3, 4]) and np.isfinite(d5[0]).all()
    assert not finite[0] and np.isfinite(np.diag(A[0])).all() and A[0, 0, 0] == A[0, 1, 1] == np.finfo(dtype).max and np.isposinf(A[0, 0, 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_direction_check_is_not_vacuous(dtype):
    """the share of points whose direction is defined, from the rule's neighbours and covariance alone, on every cloud that
    knn_ref.NORMAL_DEFINED_MIN lists (measured: 1.000 on every one of them)"""
    clouds = dict(kr.normals_clouds(dtype))
    floors = kr.NORMAL_DEFINED_MIN[dtype]
    assert {"uniform-1-300", "uniform-1000-300", "uniform-1000-1025"} <= set(floors) and min(floors.values()) >= 0.5
    for name, floor in floors.items():
        Q = clouds[name]
        A, finite = kr.covariance_rule(Q, kr.rule(Q)[0])
        amax, An, w = kr.scaled_eigenvalues(A, finite)
        share = float((finite & (amax > 0) & kr.defined(w)).mean())
        print(f"[defined] {np.dtype(dtype).name} {name}: {share:.4f}")
        assert share >= floor, (name, share)


def test_oracle_normals_hold_at_the_ends_of_the_fp64_range(orc):
    """orc_normals_f64 hands orc_eigh3 a covariance beyond 2^+-400 times an exact power of two: its normals at 1e-157 and 1e150 are
    the normals of the same cloud at scale 1 wherever the direction is defined (the scaling by a power of ten is not exact, so the
    neighbours are compared first)"""
    Q1 = kr.scale_cloud("uniform", 300, 1.0, np.float64)
    nbr1 = kr.rule(Q1)[0]
    want = orc.normals(Q1, nbr1)[0]
    A, finite = kr.covariance_rule(Q1, nbr1)
    ok = kr.defined(kr.scaled_eigenvalues(A, finite)[2])
    for scale in (1e-157, 1e150):
        Q = kr.scale_cloud("uniform", 300, scale, np.float64)
        nbr = kr.rule(Q)[0]
        same = (nbr == nbr1).all(axis=1) & ok
        assert same.mean() > 0.9
        got = orc.normals(Q, nbr)[0]
        assert np.abs(np.abs((got * want).sum(axis=1))[same] - 1.0).max() < 1e-4, scale
