"""CPU: the numpy reference of icp_batch_downsample (tests/batch_voxel_ref.py) pinned on every cloud tests/test_gpu_batch_voxel.py
uses -- the counts of output points, the largest cell population, the identity case, the single-cell case and the boundary cases.
Every condition the GPU file relies on is asserted here, on the reference alone: the device is then compared with it for byte
equality and nothing else."""
import numpy as np
import pytest

import batch_voxel_ref as vr
from batch_ref import bits_equal

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@DTYPES
def test_reference_is_the_plain_loop(dtype):
    """np.unique + np.bincount say what the loop over the points says, byte for byte"""
    for X, v in [(vr.normal(5000, 1, dtype), 0.25), (vr.coincident(dtype), 0.5), (vr.signed_zeros(dtype), vr.GRANULE_V),
                 (vr.half_lattice(dtype), 1.0), (vr.tenth_lattice(dtype)[0], 0.1), (vr.far(dtype), 0.5), (vr.negative(dtype), 0.5)]:
        Y, m, pop = vr.downsample(X, v)
        Yl, ml = vr.downsample_loop(X, v)
        assert bits_equal(Y, Yl) and np.array_equal(m, ml)
        assert pop.sum() == X.shape[0] and np.array_equal(np.bincount(m), pop)
        first = np.array([np.flatnonzero(m == r)[0] for r in range(Y.shape[0])])
        assert np.all(np.diff(first) > 0)   # first occurrence: the output keeps the order of the input


@DTYPES
def test_granule_clouds(dtype):
    pairs = vr.granule_pairs(dtype)
    assert [D.shape[0] for D, _ in pairs] == [1, 2, 63, 64, 65, 511, 512, 513, 1025, 255, 257]
    assert [M.shape[0] for _, M in pairs] == [65, 511, 512, 513, 1025, 255, 257, 1, 2, 63, 64]
    outs = [(vr.downsample(D, vr.GRANULE_V), vr.downsample(M, vr.GRANULE_V)) for D, M in pairs]
    assert [a[0].shape[0] for a, _ in outs] == [1, 2, 57, 55, 59, 307, 318, 301, 449, 187, 192]
    assert [b[0].shape[0] for _, b in outs] == [60, 316, 314, 311, 447, 207, 192, 1, 2, 58, 58]
    assert max(int(a[2].max()) for a, _ in outs) == 12   # cells of 1 to about 10 points
    assert all((a[2] == 1).any() for a, _ in outs)        # ... and copied points in every cloud
    big = outs[8][0]   # 1025 points: cells whose members lie in different key tiles (a leader adds across a tile boundary)
    spans = [np.flatnonzero(big[1] == r) for r in np.flatnonzero(big[2] >= 2)]
    assert any(s[0] // vr.TILE != s[-1] // vr.TILE for s in spans)


@DTYPES
def test_extreme_clouds(dtype):
    Z = vr.coincident(dtype)
    assert Z.shape == (300, 3) and (Z[100:140] == 0).all()
    Y, m, pop = vr.downsample(Z, 0.5)
    assert Y.shape[0] == 199 and pop.max() == 42 and len(set(m[100:140].tolist())) == 1
    # every point alone: the input byte for byte, the identity map -- inside the 21 bits
    for X in (vr.normal(300, 11, dtype), vr.signed_zeros(dtype), vr.normal(vr.MAX_POINTS, 12, dtype)):
        v = vr.identity_voxel(X)
        assert 1999998 <= vr.top_cell(X, v) <= 2000001 <= vr.MAX_CELL
        Y, m, pop = vr.downsample(X, v)
        assert bits_equal(Y, X) and np.array_equal(m, np.arange(X.shape[0])) and pop.max() == 1
    # every point in one cell: the longest sequential sum
    for X in (vr.normal(300, 11, dtype), vr.normal(vr.MAX_POINTS, 12, dtype)):
        Y, m, pop = vr.downsample(X, 1e6)
        assert Y.shape == (1, 3) and not m.any() and pop[0] == X.shape[0]
        s = [0.0, 0.0, 0.0]
        for row in X.astype(np.float64).tolist():   # the sequential sum, in Python floats
            s = [a + b for a, b in zip(s, row)]
        assert bits_equal(Y[0], np.array([a / float(X.shape[0]) for a in s]).astype(dtype))
    # -0.0 coordinates: kept where the point is alone, at the identity grid and at a coarse one
    S = vr.signed_zeros(dtype)
    assert np.signbit(S[5, 1]) and np.signbit(S[17]).all() and np.signbit(S[33, 1])
    Y, m, pop = vr.downsample(S, vr.GRANULE_V)
    assert Y.shape[0] == 161 and pop[m[33]] == 1 and bits_equal(Y[m[33]], S[33]) and np.signbit(Y[m[33], 1])
    assert pop[m[17]] >= 2   # (the origin's cell is shared: its output is computed)
    # a too-fine grid is outside the range (the library refuses it)
    X = vr.normal(300, 11, dtype)
    assert vr.top_cell(X, vr.identity_voxel(X) / 2.0) > vr.MAX_CELL


@DTYPES
def test_boundary_clouds(dtype):
    H = vr.half_lattice(dtype)
    Y, m, pop = vr.downsample(H, 1.0)
    assert H.shape[0] == 405 and Y.shape[0] == 75 and sorted(set(pop.tolist())) == [1, 2, 4, 8]
    assert np.array_equal(vr.cells(H, 1.0), np.floor(H.astype(np.float64)).astype(np.int64))   # every quotient exact
    X, K = vr.tenth_lattice(dtype)
    c = vr.cells(X, 0.1)
    off = (c != K).any(axis=1)
    assert off.any() and (c[off] >= K[off] - 1).all()   # quotients that round below the integer: the cell is k - 1, not k
    if dtype == np.float64:
        assert (c[K[:, 0] == 43, 0] == 42).all()
        # a reciprocal would put these points elsewhere: x * (1 / v) is not x / v (in fp32 the two agree on this lattice)
        assert (np.floor(X * (1.0 / 0.1)).astype(np.int64) != c).any()
    assert vr.downsample(X, 0.1)[0].shape[0] == (408 if dtype == np.float32 else 564)
    for X, cells in ((vr.far(dtype), 260), (vr.negative(dtype), 254)):
        Y, m, pop = vr.downsample(X, 0.5)
        assert Y.shape[0] == cells and pop.max() >= 4
    assert vr.far(dtype).min() > 9990 and vr.negative(dtype)[:, 0].max() < 0


@DTYPES
def test_copy_and_independence(dtype):
    X = vr.signed_zeros(dtype)
    Y, m, _ = vr.downsample(X, 0.0)
    assert bits_equal(Y, X) and np.array_equal(m, np.arange(200))
    pairs = vr.granule_pairs(dtype)[2:7]
    vm, vq = [0.3, 0.5, 0.0, 0.7, 0.4], [0.6, 0.0, 0.2, 0.5, 0.9]
    out, mm, qm = vr.downsample_pairs(pairs, vm, vq)
    rev, _, _ = vr.downsample_pairs(pairs[::-1], vm[::-1], vq[::-1])
    for b in range(5):
        assert bits_equal(out[b][0], rev[4 - b][0]) and bits_equal(out[b][1], rev[4 - b][1])
    assert len({o[0].shape[0] for o in out}) == 5   # (different v: different clouds)
