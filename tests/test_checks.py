"""tests/gpu_checks.py's comparison helpers on arrays of a few pixels: what the GPU tests rely on
them to refuse, they refuse.  No GPU."""
import types

import numpy as np
import pytest

from gpu_checks import assert_frame, assert_same_bits, counters_equal, read_ppm, words

BOTH = pytest.mark.parametrize("check", [assert_frame, assert_same_bits])


def frame():
    return np.linspace(0.25, 2.0, 2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)


@BOTH
def test_equal_arrays_pass(check):
    check(frame(), frame())
    check(frame()[::2], frame()[::2])   # a strided view, as the row subsets of the GPU tests are


@BOTH
def test_one_ulp_in_one_channel_fails_and_names_the_pixel(check):
    ref, img = frame(), frame()
    img[1, 2, 1] = np.nextafter(img[1, 2, 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"\(1, 2") as e:
        check(img, ref)
    assert "(0, " not in str(e.value)   # and no other pixel


@BOTH
def test_signed_zero_fails(check):
    ref, img = frame(), frame()
    ref[0, 1, 2], img[0, 1, 2] = 0.0, -0.0
    assert np.array_equal(img, ref)   # equal as values
    with pytest.raises(AssertionError, match=r"\(0, 1"):
        check(img, ref)


def test_nan_with_equal_bits():
    ref = frame()
    ref[1, 0, 0] = np.nan
    img = ref.copy()
    assert_same_bits(img, ref)
    with pytest.raises(AssertionError):
        assert_frame(img, ref)


@pytest.mark.parametrize("side", ["img", "ref", "both"])
def test_inf_fails_assert_frame(side):
    ref, img = frame(), frame()
    if side != "ref":
        img[0, 0, 0] = np.inf
    if side != "img":
        ref[0, 0, 0] = np.inf
    with pytest.raises(AssertionError):
        assert_frame(img, ref)


@BOTH
def test_shape_mismatch_fails(check):
    with pytest.raises(AssertionError):
        check(frame(), frame()[:1])
    with pytest.raises(AssertionError):
        check(frame().reshape(3, 2, 3), frame())   # as many elements, another shape


def test_dtype_mismatch_fails_assert_same_bits():
    plane = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert_same_bits(plane, plane.copy())
    with pytest.raises(AssertionError):
        assert_same_bits(plane.astype(np.float32), plane)
    with pytest.raises(AssertionError):
        assert_same_bits(plane.astype(np.int64), plane)


def test_assert_same_bits_names_the_plane():
    a = np.zeros((2, 2), np.int32)
    b = a.copy()
    b[1, 0] = -1
    with pytest.raises(AssertionError, match=r"object.*\(1, 0\), 0, -1"):
        assert_same_bits(a, b, "object")


def test_words():
    obj = np.array([[-1, 0], [7, -2]], np.int32)
    assert words(obj).dtype == np.uint32
    assert words(obj).tolist() == [[0xFFFFFFFF, 0], [7, 0xFFFFFFFE]]
    assert words(obj.astype(np.int64)).tolist() == words(obj).tolist()
    f = np.array([1.0, -0.0, np.inf], np.float32)
    assert words(f).tolist() == [0x3F800000, 0x80000000, 0x7F800000]
    with pytest.raises(TypeError):
        words(f.astype(np.float64))


def stats(**kw):
    base = dict(segments=10, shadow_rays=4, draws=50, rejected=0, stalled=0)
    return dict(base, **kw)


def test_counters_equal():
    st = stats()
    counters_equal(types.SimpleNamespace(**st), st)
    for field in st:
        g = types.SimpleNamespace(**stats(**{field: st[field] + 1}))
        with pytest.raises(AssertionError, match=field):
            counters_equal(g, st)


def test_counters_equal_leaves_other_fields_alone():
    st = stats()
    g = types.SimpleNamespace(**stats(rejected=3, stalled=1))
    counters_equal(g, st, ("segments", "shadow_rays", "draws"))
    with pytest.raises(AssertionError, match="rejected"):
        counters_equal(g, st, ("segments", "shadow_rays", "draws", "rejected"))


def test_read_ppm(tmp_path):
    p = tmp_path / "a.ppm"
    p.write_text("P3\n2 1\n255\n1 2 3\n250 251 252\n")
    got = read_ppm(p, 2, 1)
    assert got.dtype == np.int64 and got.shape == (1, 2, 3)
    assert got.tolist() == [[[1, 2, 3], [250, 251, 252]]]
    assert read_ppm(str(p), 2, 1).tolist() == got.tolist()
    with pytest.raises(AssertionError):
        read_ppm(p, 1, 2)   # the header's size is not the caller's
    p.write_text("P6\n2 1\n255\n1 2 3\n250 251 252\n")
    with pytest.raises(AssertionError):
        read_ppm(p, 2, 1)
