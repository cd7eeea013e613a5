"""The medium's density lookup and its two samplers on the device, point by point and draw by draw:
xrt_test_density (the kernels' own medium_density) against the oracle on the dense grid in every
grid layout — the per-cell corner table, the four row loads a grid above the corner limit falls back
to (forced here with xrt_test_corner_grid_limit), and leaf bricks — then whole renders with the row
loads inside the render kernels themselves, and xrt_test_hg / xrt_test_wavelength against
orc_kat_hg / orc_kat_wavelength with every draw chosen.  Inputs: medium_restatement.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import medium_restatement as mr
import pyoracle
from gpu_checks import assert_frame, assert_same_bits
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu

CORNERS, ROWS, BRICKS = abi.XRT_DENSITY_CORNERS, abi.XRT_DENSITY_ROWS, abi.XRT_DENSITY_BRICKS
DEFAULT_LIMIT = 2 << 30


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: its corner limit changes"""
    c = C.c_void_p()
    rc = abi.lib().xrt_create(0, C.byref(c))
    assert rc == 0, abi.lib().xrt_last_error(None).decode()
    yield c
    abi.lib().xrt_destroy(c)


def check(ctx, rc, what):
    assert rc == 0, (what, rc, abi.lib().xrt_last_error(ctx).decode())


def set_dense(ctx, med, limit=DEFAULT_LIMIT):
    check(ctx, abi.lib().xrt_test_corner_grid_limit(ctx, limit), "xrt_test_corner_grid_limit")
    md = med.desc()
    try:
        check(ctx, abi.lib().xrt_set_medium(ctx, C.byref(md)), "xrt_set_medium")
    finally:
        abi.lib().xrt_test_corner_grid_limit(ctx, DEFAULT_LIMIT)


def set_bricks(ctx, med, table, bricks):
    md = med.desc()
    nbz, nby, nbx = table.shape
    table = np.ascontiguousarray(table, np.int32)
    flat = np.ascontiguousarray(bricks, np.float32).reshape(-1)
    bg = abi.XrtBrickGrid(nbx, nby, nbz, table.ctypes.data_as(C.POINTER(C.c_int32)), len(bricks),
                          abi.fptr(flat) if len(bricks) else None)
    check(ctx, abi.lib().xrt_set_medium_bricks(ctx, C.byref(md), C.byref(bg)), "xrt_set_medium_bricks")


def device_density(ctx, pts):
    """(xrt_test_density at the points, the layout it reports)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    buf = pts if len(pts) else np.zeros((1, 3), np.float32)
    out = np.full(max(1, len(pts)), np.nan, np.float32)
    lay = C.c_int32(-1)
    check(ctx, abi.lib().xrt_test_density(ctx, abi.fptr(buf), len(pts), abi.fptr(out), C.byref(lay)), "xrt_test_density")
    return out[:len(pts)], lay.value


@functools.lru_cache(maxsize=None)
def reference(name, multiplier=1.0, sparse=False):
    """(points, family, the oracle's density on the dense grid), computed once and never written"""
    med = mr.medium(name, multiplier, sparse)
    pts, fam = mr.all_points(med)
    ref = pyoracle.density(med, pts)
    for a in (pts, ref):
        a.setflags(write=False)
    return pts, fam, ref


def assert_density(ctx, name, multiplier, sparse, layout, table=None):
    """the context's current medium gives the oracle's bits at every point of the grid's families;
    a failure names the read-path classes (and point families) that differ"""
    med = mr.medium(name, multiplier, sparse)
    pts, fam, ref = reference(name, multiplier, sparse)
    got, lay = device_density(ctx, pts)
    assert lay == layout, (abi.DENSITY_LAYOUTS[lay], abi.DENSITY_LAYOUTS[layout])
    overflow = name == "overflow"
    cls = np.char.add(np.char.add(mr.read_path(med, pts, table), "/"), fam)
    bad = mr.mismatch_by_class(got, ref, cls, nan_equal=overflow)
    assert not bad, (name, multiplier, abi.DENSITY_LAYOUTS[lay], bad)
    if not overflow:
        assert_same_bits(got, np.asarray(ref), name)


def dense_cases():
    return [(n, False) for n in mr.GRIDS] + [(n, True) for n in mr.SPARSE]


def multipliers(name):
    return (1.0,) if name == "overflow" else mr.MULTIPLIERS


def table_layout(name):
    """a grid without a cell has no corner table: it reads rows (and never takes the interior path)"""
    return CORNERS if min(mr.GRIDS[name][0]) >= 2 else ROWS


# ------------------------------------------------------------------ density ----
@pytest.mark.parametrize("name,zeroed", dense_cases())
def test_density_with_the_corner_table(ctx, name, zeroed):
    for mult in multipliers(name):
        set_dense(ctx, mr.medium(name, mult, zeroed))
        assert_density(ctx, name, mult, zeroed, table_layout(name))


@pytest.mark.parametrize("name,zeroed", dense_cases())
def test_density_with_the_row_loads(ctx, name, zeroed):
    """the corner limit at 0: the layout of every dense grid above 2 GiB of corner values"""
    for mult in multipliers(name):
        set_dense(ctx, mr.medium(name, mult, zeroed), limit=0)
        assert_density(ctx, name, mult, zeroed, ROWS)


@pytest.mark.parametrize("name", ["odd", "cell", "overflow"])
def test_layout_flips_at_the_corner_limit(ctx, name):
    nz, ny, nx = mr.GRIDS[name][0]
    need = (nz - 1) * (ny - 1) * (nx - 1) * 32
    med = mr.medium(name)
    set_dense(ctx, med, limit=need)
    assert_density(ctx, name, 1.0, False, CORNERS)
    set_dense(ctx, med, limit=need - 1)
    assert_density(ctx, name, 1.0, False, ROWS)
    set_dense(ctx, med)   # the limit is back at its default
    assert_density(ctx, name, 1.0, False, CORNERS)


@pytest.mark.parametrize("name", mr.SPARSE)
def test_density_in_bricks(ctx, name):
    """the zeroed grids cut by scenes.Medium.bricks (inactive leaves dropped) and the full grids
    (every leaf active), against the oracle on the dense grid"""
    for mult in mr.MULTIPLIERS:
        for zeroed in (True, False):
            med = mr.medium(name, mult, zeroed)
            table, bricks = med.bricks()
            assert np.any(table < 0) == zeroed
            set_bricks(ctx, med, table, bricks)
            assert_density(ctx, name, mult, zeroed, BRICKS, table)


@pytest.mark.parametrize("name,zeroed", dense_cases())
def test_density_in_bricks_never_reads_the_padding(ctx, name, zeroed):
    """a cut handed to xrt_set_medium_bricks directly, the voxels of its partial leaves that lie
    outside the grid set to 1e30: one read of them would show in the result"""
    med = mr.medium(name, 1.0, zeroed)
    table, bricks = mr.cut_bricks(med.density, pad=1e30)
    if any(n % 8 for n in med.density.shape):
        assert np.any(bricks == np.float32(1e30))
    set_bricks(ctx, med, table, bricks)
    assert_density(ctx, name, 1.0, zeroed, BRICKS, table)


def test_every_layout_is_reported(ctx):
    med = mr.medium("odd", sparse=True)
    seen = []
    set_dense(ctx, med)
    seen.append(device_density(ctx, np.zeros((0, 3)))[1])   # n == 0 is valid: the layout alone
    set_dense(ctx, med, limit=0)
    seen.append(device_density(ctx, np.zeros((0, 3)))[1])
    set_bricks(ctx, med, *med.bricks())
    seen.append(device_density(ctx, np.zeros((0, 3)))[1])
    assert seen == [CORNERS, ROWS, BRICKS]


def test_density_needs_a_heterogeneous_medium():
    lib = abi.lib()
    c = C.c_void_p()
    assert lib.xrt_create(0, C.byref(c)) == 0
    try:
        p, out, lay = np.zeros(3, np.float32), np.zeros(1, np.float32), C.c_int32(-1)
        args = (abi.fptr(p), 1, abi.fptr(out), C.byref(lay))
        assert lib.xrt_test_density(c, *args) == abi.XRT_ERR_STATE              # no medium
        assert lib.xrt_test_density(c, None, 1, abi.fptr(out), C.byref(lay)) == abi.XRT_ERR_INVALID
        assert lib.xrt_test_density(c, abi.fptr(p), 1, None, C.byref(lay)) == abi.XRT_ERR_INVALID
        assert lib.xrt_test_density(c, abi.fptr(p), 1, abi.fptr(out), None) == abi.XRT_ERR_INVALID
        hm = scenes.HomogeneousMedium("mis", 0.2, (0.1, 0.1, 0.1), (0.5, 0.5, 0.5), (0, 0, 0), (1, 1, 1)).desc()
        assert lib.xrt_set_medium(c, C.byref(hm)) == 0
        assert lib.xrt_test_density(c, *args) == abi.XRT_ERR_STATE              # a homogeneous one
        assert lay.value == -1
        w = np.zeros(8, np.uint32)
        assert lib.xrt_test_hg(c, 0.3, None, abi.u32ptr(w), 1, abi.fptr(p)) == abi.XRT_ERR_INVALID
        assert lib.xrt_test_hg(c, 0.3, abi.fptr(p), None, 1, abi.fptr(p)) == abi.XRT_ERR_INVALID
        assert lib.xrt_test_wavelength(c, abi.fptr(p), abi.fptr(p), abi.u32ptr(w), 1, None, abi.fptr(p)) == abi.XRT_ERR_INVALID
    finally:
        lib.xrt_destroy(c)


# ------------------------------------------------------------------ renders through the row loads ----
W, H, SPP, SIDE = 48, 36, 4, 32


@functools.lru_cache(maxsize=None)
def smoke_reference(integ):
    return pyoracle.render(scenes.smoke(W, H, n=SIDE), W, H, SPP, integrator=integ)


def render_with_rows(integ, schedule, devices=None):
    s = scenes.smoke(W, H, n=SIDE)
    r = HipRenderer(SPP, devices=devices)
    try:
        check(r.ctx, abi.lib().xrt_test_corner_grid_limit(r.ctx, 0), "xrt_test_corner_grid_limit")
        img = r.render(s, W, H, integrator=integ, schedule=schedule)
        assert device_density(r.ctx, np.zeros((0, 3)))[1] == ROWS
        ref, st = smoke_reference(integ)
        assert_frame(img, ref)
        assert r.stats.draws == st["draws"] and r.stats.segments == st["segments"]
        assert st["segments"] > W * H * SPP   # paths did scatter in the medium
    finally:
        r.close()


@pytest.mark.parametrize("schedule", ["auto", "wavefront"])
@pytest.mark.parametrize("integ", ["vpt", "vpt_nee"])
def test_render_with_the_row_loads(integ, schedule):
    render_with_rows(integ, schedule)


def test_render_with_the_row_loads_on_two_devices():
    """the limit reaches every device of a multi-device context: both shards read rows"""
    render_with_rows("vpt_nee", "auto", devices=[0, 0])


# ------------------------------------------------------------------ samplers ----
def oracle_mt(words):
    m = pyoracle.OrcMT()
    for q, w in enumerate(words):
        m.x[q] = int(w)
    m.p = 0
    return m


def test_samplers_equal_the_oracle(gpu):
    lib, orc = abi.lib(), pyoracle.lib()
    # sampleWavelength: channel and pmf, the NaN of a zero or cancelling sum as a class in pmf only
    thr, alb, words, note = mr.wavelength_items()
    n = len(note)
    ch, pmf = np.full(n, 99, np.uint32), np.zeros((n, 3), np.float32)
    check(gpu, lib.xrt_test_wavelength(gpu, abi.fptr(thr), abi.fptr(alb), abi.u32ptr(words.reshape(-1)), n, abi.u32ptr(ch),
                                       abi.fptr(pmf.reshape(-1))), "xrt_test_wavelength")
    rch, rpmf = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)
    for q in range(n):
        m = oracle_mt(words[q])
        rch[q] = orc.orc_kat_wavelength(C.byref(m), pyoracle.fp(thr[q]), pyoracle.fp(alb[q]), pyoracle.fp(rpmf[q]))
        assert m.p == 1
    bad = np.flatnonzero(ch != rch)
    assert len(bad) == 0, [(note[q], thr[q].tolist(), alb[q].tolist(), int(ch[q]), int(rch[q])) for q in bad[:8]]
    assert set(rch.tolist()) == {0, 1, 2}
    both_nan = np.isnan(pmf) & np.isnan(rpmf)
    assert both_nan.sum() >= 6
    bad = np.argwhere((pmf.view(np.uint32) != rpmf.view(np.uint32)) & ~both_nan)
    assert len(bad) == 0, [(note[q], thr[q].tolist(), pmf[q].tolist(), rpmf[q].tolist()) for q, _ in bad[:8]]
    # HenyeyGreenstein::sampleDirection: wi bit for bit
    for g, (wo, hw) in mr.hg_items().items():
        n = len(wo)
        wi = np.zeros((n, 3), np.float32)
        check(gpu, lib.xrt_test_hg(gpu, C.c_float(g), abi.fptr(wo.reshape(-1)), abi.u32ptr(hw.reshape(-1)), n,
                                   abi.fptr(wi.reshape(-1))), "xrt_test_hg")
        ref = np.zeros((n, 3), np.float32)
        for q in range(n):
            m = oracle_mt(hw[q])
            orc.orc_kat_hg(C.byref(m), C.c_float(g), pyoracle.fp(wo[q]), pyoracle.fp(ref[q]))
            assert m.p == 2
        assert np.all(np.isfinite(ref)), g
        assert_same_bits(wi, ref, f"hg_sample g = {g}")
