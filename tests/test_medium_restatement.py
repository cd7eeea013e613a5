"""The numpy restatement of the medium's density lookup (medium_restatement.py) against the
oracle's own (orc_kat_density) point by point, the coverage of its read-path classes, the 8^3 brick
cut, the draw helpers and the argument checks of the medium self-tests that need no device."""
import ctypes as C

import numpy as np
import pytest

import medium_restatement as mr
import pyoracle
from xraytracer_amd import abi


@pytest.fixture(scope="module")
def points():
    """per grid name: (points, family) of the unit-multiplier medium (the points do not depend on it)"""
    return {name: mr.all_points(mr.medium(name)) for name in mr.GRIDS}


def check_equal(med, pts, fam, nan_equal=False):
    got, ref = mr.density(med, pts), pyoracle.density(med, pts)
    bad = mr.mismatch_by_class(got, ref, fam, nan_equal)
    assert not bad, bad


@pytest.mark.parametrize("name", mr.PLAIN)
def test_restatement_equals_the_oracle(name, points):
    pts, fam = points[name]
    assert len(pts) <= 30000
    for mult in mr.MULTIPLIERS:
        check_equal(mr.medium(name, mult), pts, fam)


@pytest.mark.parametrize("name", mr.SPARSE)
def test_restatement_equals_the_oracle_on_sparse_grids(name, points):
    pts, fam = points[name]
    for mult in mr.MULTIPLIERS:
        check_equal(mr.medium(name, mult, sparse=True), pts, fam)


def test_restatement_equals_the_oracle_on_the_overflow_grid(points):
    """neighbours of +-3e38: b - a is infinite, and at w == 0 the lerp is inf * 0 = NaN, whose sign
    and payload the hardware chooses: a NaN on both sides counts as equal here, and only here"""
    pts, fam = points["overflow"]
    med = mr.medium("overflow")
    ref = pyoracle.density(med, pts)
    assert np.isnan(ref).sum() >= 64 and np.isinf(ref).sum() >= 64 and np.isfinite(ref).sum() >= 64
    check_equal(med, pts, fam, nan_equal=True)


def test_planted_values_are_in_the_grids():
    for name in mr.PLAIN:
        w = mr.grid_values(name).view(np.uint32)
        for v in mr.PLANTED:
            assert np.any(w == np.float32(v).view(np.uint32)), (name, v)
    g = mr.grid_values("overflow")
    with np.errstate(over="ignore"):
        assert np.all(np.abs(g) == np.float32(3e38))
        for axis in range(3):   # neighbours of either sign along every axis: b - a overflows
            d = np.diff(g, axis=axis)
            assert np.any(d == np.inf) and np.any(d == -np.inf) and np.any(d == 0)


@pytest.mark.parametrize("name", [n for n in mr.GRIDS if min(mr.GRIDS[n][0]) >= 2])
def test_dense_read_paths_are_covered(name, points):
    pts, _ = points[name]
    cls = mr.read_path(mr.medium(name), pts)
    for c in mr.DENSE_CLASSES:
        assert np.count_nonzero(cls == c) >= 64, (name, c)


def test_a_grid_without_a_cell_has_no_interior(points):
    pts, _ = points["flat"]
    cls = mr.read_path(mr.medium("flat"), pts)
    assert not np.any(cls == "interior")
    assert np.count_nonzero(cls == "shell") >= 64 and np.count_nonzero(cls == "outside") >= 64


@pytest.mark.parametrize("name", mr.SPARSE)
def test_brick_read_paths_are_covered(name, points):
    pts, _ = points[name]
    med = mr.medium(name, sparse=True)
    table, _ = med.bricks()
    assert np.any(table < 0) and np.any(table >= 0)
    cls = mr.read_path(med, pts, table)
    for c in ("leaf_interior", "leaf_face", "inactive", "mixed", "shell", "outside"):
        assert np.count_nonzero(cls == c) >= 64, (name, c)
    # the unzeroed grid has every leaf active: the two active classes alone
    dense = mr.medium(name)
    cls = mr.read_path(dense, pts, mr.cut_bricks(dense.density)[0])
    assert np.count_nonzero(cls == "leaf_interior") >= 64 and np.count_nonzero(cls == "leaf_face") >= 64
    assert not np.any(np.isin(cls, ("inactive", "mixed", "inactive_face")))


def test_the_edge_cells_the_lookup_can_get_wrong_are_hit(points):
    """u == 0 and one float below a voxel plane, the half-outside shell on either side, the far-corner
    cell and the last cell of a leaf: each by name, on the grid whose index arithmetic is exact"""
    med = mr.medium("exact")
    pts, fam = points["exact"]
    ijk, uvw = mr.cells(med, pts)
    nz, ny, nx = med.density.shape
    assert np.count_nonzero(np.all(uvw[fam == "lattice"] == 0.0, axis=1)) == np.count_nonzero(fam == "lattice")
    below = uvw[fam == "below"]
    assert np.all((below > 0.999) & (below <= 1.0))
    assert np.any(below == 1.0)   # one denormal below world 0: cell -1 with a weight that rounds to 1
    assert np.any(ijk[:, 0] == -1) and np.any(ijk[:, 0] == nx - 1) and np.any(ijk[:, 2] == nz - 1)
    assert np.count_nonzero(np.all(ijk == (nx - 2, ny - 2, nz - 2), axis=1)) >= 512
    assert np.any((ijk[:, 0] & 7) == 7) and np.any((ijk[:, 1] & 7) == 7)


@pytest.mark.parametrize("name", mr.GRIDS)
def test_brick_cut_reads_back_every_voxel(name):
    for sparse in (False, True) if name in mr.SPARSE else (False,):
        med = mr.medium(name, sparse=sparse)
        g = med.density
        for table, bricks in (med.bricks(), mr.cut_bricks(g), mr.cut_bricks(g, pad=1e30)):
            assert table.shape == tuple((n + 7) // 8 for n in g.shape)
            assert int(table.max()) + 1 == len(bricks)
            back = mr.read_bricks(table, bricks, g.shape)
            # a dropped leaf reads as +0 where the grid holds a zero of either sign
            assert np.array_equal(back, g)
            kept = np.repeat(np.repeat(np.repeat(table >= 0, 8, 0), 8, 1), 8, 2)[:g.shape[0], :g.shape[1], :g.shape[2]]
            assert np.array_equal(back.view(np.uint32)[kept], g.view(np.uint32)[kept])
        t0, b0 = mr.cut_bricks(g)
        t1, b1 = med.bricks()
        assert np.array_equal(t0, t1) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))


def test_padded_cut_holds_the_padding_outside_the_grid_only():
    med = mr.medium("odd", sparse=True)
    table, bricks = mr.cut_bricks(med.density, pad=1e30)
    assert np.count_nonzero(bricks == np.float32(1e30)) > 0
    assert not np.any(mr.read_bricks(table, bricks, med.density.shape) == np.float32(1e30))


# ------------------------------------------------------------------ draws ----
def test_untemper_inverts_the_tempering():
    rng = np.random.default_rng(1)
    z = np.concatenate([rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 1 << 31, mr.LARGEST], np.uint32)])
    y = np.array([mr.untemper(v) for v in z], np.uint32)
    assert np.array_equal(mr.temper(y), z)


def test_ring_words_give_the_chosen_draws_in_the_oracle():
    outs = [0, 1, mr.output_of(0.75), mr.LARGEST, mr.output_of(np.nextafter(np.float32(0.5), np.float32(1)))]
    m = pyoracle.OrcMT()
    for q, w in enumerate(mr.ring_words(outs)):
        m.x[q] = w
    m.p = 0
    lib = pyoracle.lib()
    got = [np.float32(lib.orc_draw(C.byref(m))) for _ in outs]
    assert got == [mr.draw_value(o) for o in outs]
    assert got[0] == 0.0 and got[1] == np.float32(2.0 ** -32) and got[3] == np.nextafter(np.float32(1), np.float32(0))


def test_wavelength_items_cover_the_branches():
    thr, alb, words, note = mr.wavelength_items()
    assert 150 <= len(note) <= 300
    u = np.array([mr.draw_value(int(mr.temper(w[0]))) for w in words])
    c = np.array([mr.cdf_of(t, a) for t, a in zip(thr, alb)])
    assert np.count_nonzero(u == 0.0) >= 10 and np.count_nonzero(u == np.float32(2.0 ** -32)) >= 10
    with np.errstate(invalid="ignore"):
        assert np.count_nonzero(u > c[:, 2]) >= 4          # beyond the last cdf entry: the clamp
        for q in range(3):
            assert np.count_nonzero(u == c[:, q]) >= 4     # on a cdf entry
    assert np.count_nonzero(np.isnan(c[:, 0])) >= 3        # zero sum
    assert np.count_nonzero(np.isinf(c[:, 0]) & np.isnan(c[:, 2])) >= 3


def test_hg_items_cover_the_switch_and_the_axes():
    items = mr.hg_items()
    assert set(items) == set(mr.HG_G) and 150 <= sum(len(w) for w, _ in items.values()) <= 300
    assert sum(abs(g) < 1e-3 for g in items) == 3 and sum(abs(g) >= 1e-3 for g in items) == 6
    wo, words = items[0.3]
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = np.zeros(3, np.float32)
            e[axis] = sign
            assert np.any(np.all(wo == e, axis=1))
    outs = {int(mr.temper(w)) for w in words[:, 1]}
    assert {0, mr.LARGEST} <= outs


# ------------------------------------------------------------------ argument checks ----
def test_medium_self_tests_reject_null_arguments_without_a_gpu():
    lib = abi.lib()
    one = np.zeros(8, np.float32)
    w = np.zeros(8, np.uint32)
    lay = C.c_int32(-7)
    inv = abi.XRT_ERR_INVALID
    assert lib.xrt_test_density(None, abi.fptr(one), 1, abi.fptr(one), C.byref(lay)) == inv
    assert lib.xrt_test_density(None, None, 0, None, None) == inv
    assert lay.value == -7
    assert lib.xrt_test_corner_grid_limit(None, 0) == inv
    assert lib.xrt_test_hg(None, 0.3, abi.fptr(one), abi.u32ptr(w), 1, abi.fptr(one)) == inv
    assert lib.xrt_test_wavelength(None, abi.fptr(one), abi.fptr(one), abi.u32ptr(w), 1, abi.u32ptr(w), abi.fptr(one)) == inv
