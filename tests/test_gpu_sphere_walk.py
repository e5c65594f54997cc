"""The path kernel's sphere walk in branch-free blocks of node steps (csrc/rt_sphere_walk.h) on the
GPU: every case bit-exact against the CPU oracle -- accumulation bits, RGBA8 and ray count --
after a 3-frame batch. tests/test_sphere_walk_cpu.py checks the block itself step by step; here it
runs inside rt_pathtrace_kernel<*, *, false> with the block group tests, the threshold logic and
the drain around it.

Scenes: C2 at 64x36 and at 37x21 (partial tiles), C1, the cluster scene, and three small ones at
the edges of the builder: two spheres (one small, the huge ground: sphere_bvh.cpp builds no tree
for fewer than two BVH spheres, so both are swept and the walk is over at once -- a one-node tree
itself is walked in the CPU harness), 15 small spheres plus the ground (the smallest tree the
builder makes), and 12 spheres (under the builder's 16: all brute-force, no nodes). C2 again with
one and eight BVH layouts crossed with plain and (near, far) ordered boxes, with trav_threshold
0 / 12 / 63 and with the frames of a batch back to back on a lane or in parallel. Each scene's
oracle frames are computed once and shared.
"""
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.camera import Camera
from rust_gpu_raytracing_amd.scene import RenderScene, _sphere, build_config
from tests.sphere_cluster_scene import cluster_scene
from tests.test_gpu_parity import assert_same, gpu_render, oracle_frames

pytestmark = pytest.mark.gpu

FRAMES = 3


def small_scene(kind):
    """The cluster scene's camera, materials and sky over a handful of spheres."""
    base = cluster_scene(64, 36)
    rng = np.random.default_rng(3)
    ground = _sphere(np.array([0.0, 1001.0, 0.0], np.float32), 1000.0, 0)
    if kind == "one_plus_ground":
        sph = [_sphere(np.array([0.0, 0.0, 0.0], np.float32), 2.0, 2), ground]
    else:
        n = 15 if kind == "fifteen_plus_ground" else 12
        sph = [_sphere(np.array([rng.uniform(-12, 12), rng.uniform(-1.5, 0.5), rng.uniform(-8, 8)], np.float32),
                       float(rng.uniform(0.5, 1.5)), i % 3) for i in range(n)]
        if kind == "fifteen_plus_ground":
            sph.insert(7, ground)
    pos = np.array([2.0, -9.0, 30.0], np.float32)
    cam = Camera(64, 36, position=pos, direction=(-pos / np.linalg.norm(pos)).astype(np.float32), vertical_fov=50.0)
    return RenderScene(np.stack(sph).astype(B.SPHERE), base.materials, [], base.textures, base.environment_map, cam,
                       name=kind)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, bounces, camera rays, oracle (accumulation, RGBA8, rays) after FRAMES frames); never modified."""
    from oracle import oracle as O

    O.build()
    if name == "c2_64x36":
        scene, bounces = build_config("c2_rtiow", width=64, height=36)
    elif name == "c2_37x21":
        scene, bounces = build_config("c2_rtiow", width=37, height=21)
    elif name == "c1_40x24":
        scene, bounces = build_config("c1_four_spheres", width=40, height=24)
    elif name == "clusters_64x36":
        scene, bounces = cluster_scene(64, 36), 8
    else:
        scene, bounces = small_scene(name), 8
    if name.startswith("c2"):
        assert bounces == 8
    rays = scene.camera.recalculate_ray_directions()
    return scene, bounces, rays, oracle_frames(O, scene, bounces, FRAMES, rays)


def check(name, tuning=None):
    scene, bounces, rays, (acc_o, out_o, n_o) = reference(name)
    kw = {"tuning": tuning} if tuning else {}
    acc, out, n = gpu_render(scene, bounces, FRAMES, rays=rays, frame_batch=FRAMES, **kw)
    assert_same(acc, out, n, acc_o, out_o, n_o)


@pytest.mark.parametrize("name", ["c2_64x36", "c2_37x21", "c1_40x24", "clusters_64x36", "one_plus_ground",
                                  "fifteen_plus_ground", "twelve_brute_force"])
def test_scenes_match_oracle(gpu, name):
    check(name)


@pytest.mark.parametrize("box_order", [0, 1])
@pytest.mark.parametrize("octants", [0, 1])
def test_layouts_match_oracle(gpu, octants, box_order):
    """One / eight BVH layouts, plain / (near, far) ordered boxes: both instantiations of the block."""
    check("c2_64x36", {"sphere_octants": octants, "sphere_box_order": box_order})


@pytest.mark.parametrize("threshold", [0, 12, 63])
def test_trav_threshold_match_oracle(gpu, threshold):
    """0: by scene; 63: back to shading after every block, so lanes enter most blocks mid-walk."""
    check("c2_64x36", {"trav_threshold": threshold})


@pytest.mark.parametrize("parallel", [0, 1])
def test_frame_parallel_match_oracle(gpu, parallel):
    check("c2_64x36", {"frame_parallel": parallel})
    check("c2_37x21", {"frame_parallel": parallel})
