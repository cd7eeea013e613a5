"""The cases of xrt_render_var under XRT_FLAG_VAR_FUSED (the moments builds of k_step, k_step_tri and
k_step_merged) — a helper, not a test file.

The contract is tests/render_var_restatement.py's: the flag changes the schedule, not one bit of the
frame or the plane.  A case names a scene, its size, its sample count, the keywords that are
semantics (what the restatement and the oracle take) and the keywords that are launch geometry (what
only the device takes), and the schedule the render must report.  Cases that share a scene, a size,
a sample count and the semantics share one restatement and one oracle frame (`reference`,
`oracle_frame`: computed once, read-only).  tests/test_gpu_render_var_fused.py renders them;
tests/test_render_var_fused_cases.py shows without a GPU that they reach what they are chosen for."""
import functools

from xraytracer_amd import abi, scenes

import pyoracle
import render_var_restatement as rv

MERGED, BVH, TRI, STEP = abi.XRT_SCHED_STEP_MERGED, abi.XRT_SCHED_STEP_BVH, abi.XRT_SCHED_STEP_TRI, abi.XRT_SCHED_STEP


def two_quad_lights(w, h):
    """the Cornell box with a second quad light under its ceiling: two shadow rays per segment, so
    GIIntegrator's NEE term is not folded at sampling time (step_merged.h, kFold)"""
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", (343.0, 548.0, 227.0), (343.0, 548.0, 332.0), (213.0, 548.0, 227.0), (25.0, 25.0, 25.0))
    s.add_quad_light("QuadLight2", (150.0, 540.0, 100.0), (150.0, 540.0, 160.0), (90.0, 540.0, 100.0), (12.0, 6.0, 3.0))
    s.flatten()
    s.camera = scenes.pinhole(scenes.CORNELL_C2W, 60.0, w, h)
    return s


# scene name -> builder; one SceneBundle per name (`scene`)
SCENES = {
    "cornell_64": lambda: scenes.cornell(64, 48),
    "cornell_8": lambda: scenes.cornell(8, 6),
    "cornell_256": lambda: scenes.cornell(256, 128),
    "two_lights": lambda: two_quad_lights(64, 48),
    "rejecting": lambda: rv.rejecting_cornell(64, 48),
    "spheremesh": lambda: scenes.cornell_spheremesh(32, 24, n_theta=24, n_phi=24),
    "spheres": lambda: scenes.spheres(32, 24, nx=40, nz=2),
    "homogeneous_512": lambda: rv.homogeneous(512, 256),
}

# name -> (scene name, width, height, spp, semantics, launch geometry, schedule)
CASES = {}


def _case(name, scene_name, w, h, spp, sem, geo, sched):
    assert name not in CASES, name
    CASES[name] = (scene_name, w, h, spp, sem, geo, sched)


# 1. the merged kernel over a one-level scene: every layout launch_merged_spw can pick (64 / 32 / 16 / 4
#    slots per wave, with the group traces and with pair passes), both integrators
for _integ in ("gi", "direct"):
    for _spw in (64, 32, 16, 4):
        for _group in (True, False):
            _case(f"merged_{_integ}_{_spw}_{'group' if _group else 'pairs'}", "cornell_64", 64, 48, 5,
                  dict(integrator=_integ), dict(slots_per_wave=_spw, group=_group), MERGED)
#    ... and samples, deferred finishes and the drain across launch boundaries, in a group layout and in whole waves
for _v in (1, 2, 3):
    _case(f"merged_gi_16_group_visits_{_v}", "cornell_64", 64, 48, 5, dict(integrator="gi"),
          dict(slots_per_wave=16, group=True, visits_per_launch=_v), MERGED)
_case("merged_direct_64_visits_1", "cornell_64", 64, 48, 5, dict(integrator="direct"),
      dict(slots_per_wave=64, visits_per_launch=1), MERGED)
# 2. two lights: no folded NEE
for _integ in ("gi", "direct"):
    _case(f"two_lights_{_integ}", "two_lights", 64, 48, 3, dict(integrator=_integ), {}, MERGED)
# 3. rejected samples
for _integ in ("gi", "direct"):
    _case(f"rejects_{_integ}", "rejecting", 64, 48, 6, dict(integrator=_integ), {}, MERGED)
# 4. rings twisted inside the launch: the refill reuses the wave's trace scratch after the last finish
_case("twists", "cornell_8", 8, 6, 200, dict(integrator="gi"), {}, MERGED)
# 5. partition groups (16 partitions: the smallest grouped frame), one launch per round, the interleaved slot map
for _n, _kw in (("groups", {}), ("no_overlap", dict(overlap=False)), ("interleave", dict(interleave=True))):
    _case(f"{_n}_256", "cornell_256", 256, 128, 4, dict(integrator="gi"), dict(slots_per_wave=64, visits_per_launch=2, **_kw), MERGED)
# 6. the two-level form (16 slots per wave over 768 slots: the XRT_BVH_LOW_WAVES build)
for _spw in (64, 32, 16):
    _case(f"two_level_{_spw}", "spheremesh", 32, 24, 3, dict(integrator="gi"), dict(slots_per_wave=_spw), BVH)
# 7. k_step_tri
for _integ in ("gi", "direct"):
    _case(f"step_tri_{_integ}", "cornell_64", 64, 48, 5, dict(integrator=_integ), dict(schedule="step_tri"), TRI)
# 8. k_step: the cases of tests/render_var_restatement.py that reach it (sphere, mixed and medium scenes,
#    Indirect and Normal, whose only fused kernel it is), the 512-thread Direct build, the 4-wave volumetric one
KSTEP_FROM_RV = ("spheres", "example", "mixed_lit", "indirect", "normal", "vpt_smoke", "vpt_nee_smoke", "vpt_homogeneous",
                 "vpt_nee_homogeneous")
_case("kstep_direct_512", "spheres", 32, 24, 3, dict(integrator="direct"), {}, STEP)
_case("kstep_vpt_4_waves", "homogeneous_512", 512, 256, 2, dict(integrator="vpt"), {}, STEP)


@functools.lru_cache(maxsize=None)
def scene(scene_name):
    return SCENES[scene_name]()


def _sem_key(sem):
    return tuple(sorted(sem.items()))


@functools.lru_cache(maxsize=None)
def _reference(scene_name, w, h, spp, sem):
    img, var, rec = rv.render(scene(scene_name), w, h, spp, **dict(sem))
    img.setflags(write=False), var.setflags(write=False)
    return img, var, rec


@functools.lru_cache(maxsize=None)
def _oracle(scene_name, w, h, spp, sem):
    img, cnt = pyoracle.render(scene(scene_name), w, h, spp, **dict(sem))
    img.setflags(write=False)
    return img, cnt


def reference(name):
    """(frame, variance, record) of the restatement for CASES[name]"""
    scene_name, w, h, spp, sem, _, _ = CASES[name]
    return _reference(scene_name, w, h, spp, _sem_key(sem))


def oracle_frame(name):
    """(frame, counters) of the oracle for CASES[name]"""
    scene_name, w, h, spp, sem, _, _ = CASES[name]
    return _oracle(scene_name, w, h, spp, _sem_key(sem))
