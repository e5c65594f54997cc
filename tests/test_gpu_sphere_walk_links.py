"""The linked form of the sphere walk (csrc/rt_sphere_walk.h: links as LDS addresses, the sentinel
after the last node, pre-masked leaf words) inside the path kernel's sphere-only instances that
stage the scene: every case bit-exact against the CPU oracle -- accumulation bits, RGBA8 and ray
count -- and, for C2 at 64x36, against the committed golden fixture as well.
tests/test_sphere_walk_links_cpu.py checks the staging rewrite and the block step by step; here
they run with the block group tests, the threshold logic and the drain around them.

Scenes: C1 and C2 at 64x36 and at 37x21 (partial tiles), the cluster scene, 12 spheres (under the
builder's 16: all brute-force, no nodes, the image's node area is the sentinel alone), and 16
spheres of which 1, 4 and 5 have a finite extent (the others, centred at infinity, are kept out of
the tree by the builder and hit by no ray): no tree (the builder wants two), a tree whose root is
a leaf, and the smallest tree with an internal root.
Launches of each scene: a frame-parallel batch on the frame-parallel and on the generic instance,
a batch with "frame_parallel" 0, a non-accumulating frame, and "lds_mode" 0 (the scene in global
memory: the index walk, which the linked form must leave as it was). Then one context that has
launched goes from ordered to plain boxes and from eight layouts to one.
Each scene's oracle frames are computed once and shared.
"""
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.camera import Camera
from rust_gpu_raytracing_amd.scene import RenderScene, _sphere, build_config
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.sphere_cluster_scene import cluster_scene
from tests.test_gpu_parity import assert_same, oracle_frames

pytestmark = pytest.mark.gpu

FRAMES = 3
FRAME_PAR = N.RT_PASS_PATH | N.RT_PASS_RESOLVE | N.RT_PASS_PATH_FRAME_PAR
GENERIC_BATCH = N.RT_PASS_PATH | N.RT_PASS_RESOLVE
GENERIC = N.RT_PASS_PATH

SCENES = ["c1_64x36", "c1_37x21", "c2_64x36", "c2_37x21", "clusters_64x36", "twelve_brute_force", "bvh_1", "bvh_4",
          "bvh_5"]
# name: (tuning, accumulate, frames, the launch's pass mask, the scene is staged in LDS)
LAUNCHES = {
    "frame_par_instance": ({}, True, FRAMES, FRAME_PAR, True),
    "generic_instance": ({"frame_par_instance": 0}, True, FRAMES, GENERIC_BATCH, True),
    "frame_parallel_0": ({"frame_parallel": 0}, True, FRAMES, GENERIC, True),
    "non_accumulating": ({}, False, 1, GENERIC, True),
    "lds_mode_0": ({"lds_mode": 0}, True, FRAMES, FRAME_PAR, False),
}


def small_scene(name):
    """The cluster scene's camera, materials and sky over a handful of spheres."""
    base = cluster_scene(64, 36)
    rng = np.random.default_rng(5)

    def near():
        return _sphere(np.array([rng.uniform(-7, 7), rng.uniform(-2.0, 1.0), rng.uniform(-5, 5)], np.float32),
                       float(rng.uniform(0.8, 1.8)), int(rng.integers(0, 3)))

    if name == "twelve_brute_force":
        sph = [near() for _ in range(12)]
    else:
        finite = int(name.split("_")[1])
        away = _sphere(np.array([np.inf, 0.0, 0.0], np.float32), 1.0, 0)
        sph = [near() for _ in range(finite)] + [away] * (16 - finite)
    pos = np.array([2.0, -9.0, 30.0], np.float32)
    cam = Camera(64, 36, position=pos, direction=(-pos / np.linalg.norm(pos)).astype(np.float32), vertical_fov=50.0)
    return RenderScene(np.stack(sph).astype(B.SPHERE), base.materials, [], base.textures, base.environment_map, cam,
                       name=name)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name.startswith(("c1_", "c2_")):
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        scene, bounces = build_config("c1_four_spheres" if name.startswith("c1") else "c2_rtiow", width=w, height=h)
    elif name == "clusters_64x36":
        scene, bounces = cluster_scene(64, 36), 8
    else:
        scene, bounces = small_scene(name), 8
    return scene, bounces, scene.camera.recalculate_ray_directions()


@functools.lru_cache(maxsize=None)
def reference(name, accumulate, frames):
    """The oracle's (accumulation, RGBA8, rays) after `frames` frames; never modified."""
    from oracle import oracle as O

    O.build()
    scene, bounces, rays = scene_of(name)
    return oracle_frames(O, scene, bounces, frames, rays, accumulate=1 if accumulate else 0)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("name", SCENES)
def test_scenes_match_oracle(gpu, name, launch):
    tuning, accumulate, frames, mask, staged = LAUNCHES[launch]
    scene, bounces, rays = scene_of(name)
    with Renderer(scene, accumulate=accumulate, camera_rays=rays, frame_batch=frames, tuning=tuning or None) as r:
        for _ in range(frames):
            r.compute_frame(bounces)
        r.synchronize()
        assert r.last_launch_pass_mask() == mask, (hex(r.last_launch_pass_mask()), hex(mask))
        assert (r.launch_config()["scene_in_lds"] >= 1) == staged
        got = r.read_accumulation(), r.read_output(), r.ray_count()
    assert_same(*got, *reference(name, accumulate, frames))


def test_golden_fixture(gpu):
    name = "c2_64x36_b8"
    g, case = load(name), CASES[name]
    with Renderer(scene_from_inputs(g), camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=case["frames"]) as r:
        for _ in range(case["frames"]):
            r.compute_frame(case["bounces"])
        r.synchronize()
        assert r.last_launch_pass_mask() == FRAME_PAR and r.launch_config()["scene_in_lds"] >= 1
        assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), g["accum"], g["out"], int(g["rays"]))


# BVH nodes per layout of the scenes whose tree shape a case is about (sphere_bvh.cpp: no tree below
# two BVH spheres, one leaf up to four, then an internal root with two children)
NODES = {"c1_64x36": 0, "c1_37x21": 0, "twelve_brute_force": 0, "bvh_1": 0, "bvh_4": 1, "bvh_5": 3}


@pytest.mark.parametrize("name", SCENES)
def test_tuning_changes_after_a_launch(gpu, name):
    """A context that has launched with eight ordered layouts, then plain boxes, then one layout: the
    image is laid out and restaged for each (the sentinel moves with the node count). The LDS size tells the tree's shape: eight layouts against one differ by 7 x 32 bytes
    per node, so the scenes meant to have no tree, a leaf root and an internal root do."""
    scene, bounces, rays = scene_of(name)
    with Renderer(scene, camera_rays=rays, frame_batch=FRAMES) as r:
        lds = []
        for key in (None, "sphere_box_order", "sphere_octants"):
            if key:
                r.set_tuning(key, 0)
                r.reset_accumulation()
                r.reset_ray_count()
            for _ in range(FRAMES):
                r.compute_frame(bounces)
            r.synchronize()
            assert r.last_launch_pass_mask() == FRAME_PAR and r.launch_config()["scene_in_lds"] >= 1
            lds.append(r.launch_config()["lds_bytes"])
            assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), *reference(name, True, FRAMES))
        assert lds[0] == lds[1]
        drop = lds[1] - lds[2]  # eight layouts, then one
        assert drop % (7 * 32) == 0
        if name in NODES:
            assert drop == 7 * 32 * NODES[name]
        else:
            assert drop > 7 * 32 * 3
