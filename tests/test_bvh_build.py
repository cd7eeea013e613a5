"""The host's hierarchy build (xraytracer_amd/csrc/bvh.h, host/bvh.cpp: build_bvh, its breadth-first
renumbering, build_bvh_fit, thread_bvh, collapse_bvh4) checked by a stand-alone program,
tests/cpp/bvh_kat.cpp, which lists what it checks, over layouts of its own and over the boxes of
every scene of tests/irregular_meshes.py.  CPU only: g++ compiles the build and the program together,
once plainly and once with AddressSanitizer and UBSan (float-cast-overflow included: the build turns
floats into bin numbers), and each build runs once.  The plain run's
records are then held to what each scene was built for (irregular_meshes.EDGES): the depths of the
first build, which scenes it leaves beyond the walks' stacks, and the node counts around
kBvhTopNodes."""
import pytest

import irregular_meshes as im

LIMITS = im.limits()


def test_limits_are_the_documented_ones():
    """the figures irregular_meshes' docstring, EDGES and include/xrt.h name"""
    assert LIMITS == dict(KAT_MAX_DEPTH=48, KAT_STACK=24, KAT_STACK4=48)
    assert im.constant("tuning.h", "XRT_BVH_LEAF") == im.LEAF_TRI and im.constant("bvh.h", "kBvhTopNodes") == 64


@pytest.fixture(scope="module")
def box_files(tmp_path_factory):
    return im.box_files(tmp_path_factory.mktemp("boxes"))


def test_bvh_program_sanitized(tmp_path, box_files):
    im.run_program(tmp_path, box_files, ("-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-g"))


def test_bvh_program_and_edges(tmp_path, box_files):
    rec = im.run_program(tmp_path, box_files)
    assert set(im.CASES) <= set(rec) and "spheres_irregular" in rec and "identical" in rec and "flt_max" in rec
    for name in im.CASES:
        r = {k: (v if k in ("first", "fnv") else int(v)) for k, v in rec[name].items()}
        two = name.endswith("-two")
        assert r["two_level"] == two
        first_fits = r["first_depth"] < LIMITS["KAT_STACK"] and (not two or 3 * r["first_depth4"] + 1 <= LIMITS["KAT_STACK4"])
        # the program has checked that the tree returned fits; a first build that fits is the one returned
        assert (r["first"] == r["fnv"]) == first_fits, (name, r)
        e = im.EDGES.get(name, dict(fits=True))
        assert first_fits == e["fits"], (name, r)
        if "depth" in e:
            assert r["first_depth"] == e["depth"], (name, r)
        if "depth4" in e:
            assert r["first_depth4"] == e["depth4"], (name, r)
        if "nodes" in e:
            assert r["nodes"] == e["nodes"], (name, r)
    # the instances at the walks' limits: the full binary stack, and 46 of the 4-wide walk's 48 entries
    assert int(rec["spiral_38d-one"]["depth"]) + 1 == LIMITS["KAT_STACK"]
    assert 43 <= 3 * int(rec["spiral_22x-two"]["depth4"]) + 1 <= LIMITS["KAT_STACK4"]
    # concentric boxes: the centroid extent is 0 at the root, so the count halves at every level
    assert int(rec["concentric-two"]["depth"]) == 9                    # 1200 -> ... -> 3 triangles
