"""The two instances of the path kernel (csrc/pathtrace.hip, kFramePar) on the GPU: the
frame-parallel instance, which a frame-parallel batch with bounces >= 1 runs, and the generic
instance, which every other launch runs and which the tuning key "frame_par_instance" 0 forces.

Every case is bit-exact against the CPU oracle -- accumulation bits, RGBA8 and ray count -- and
asserts through the raw pass mask (Renderer.last_launch_pass_mask, RT_PASS_PATH_FRAME_PAR) that the
instance it means to run did run. Sizes are the smallest with partial tiles, more than one tile per
wave and, for the cost-ordered schedule, the smallest at which the schedule switches on. Each
scene's oracle frames are computed once and shared.
"""
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.sphere_cluster_scene import cluster_scene
from tests.test_gpu_parity import assert_same, oracle_frames, owned_mask

pytestmark = pytest.mark.gpu

VARIANT = N.RT_PASS_PATH | N.RT_PASS_RESOLVE | N.RT_PASS_PATH_FRAME_PAR  # a frame-parallel batch, its own instance
GENERIC_BATCH = N.RT_PASS_PATH | N.RT_PASS_RESOLVE                       # a frame-parallel batch, generic instance
GENERIC = N.RT_PASS_PATH                                                 # a launch that is no frame-parallel batch


def path_bits(r):
    """The last launch's mask without the primary pre-pass bit (triangle scenes in global memory run it)."""
    return r.last_launch_pass_mask() & ~N.RT_PASS_PRIMARY


def render(scene, bounces, frames, rays, expect, *, spp=1, tuning=None, **kw):
    """`frames` frames as one batch; the launch's pass mask must be `expect`."""
    with Renderer(scene, compute_per_frame=spp, camera_rays=rays, frame_batch=frames, tuning=tuning, **kw) as r:
        for _ in range(frames):
            r.compute_frame(bounces)
        r.synchronize()
        assert path_bits(r) == expect, (hex(path_bits(r)), hex(expect))
        return r.read_accumulation(), r.read_output(), r.ray_count()


@functools.lru_cache(maxsize=None)
def reference(config, w, h, frames, spp=1, bounces=None):
    """(scene, bounces, camera rays, the oracle's (accumulation, RGBA8, rays) after `frames` frames); never modified."""
    from oracle import oracle as O

    O.build()
    scene, b = build_config(config, width=w, height=h)
    b = b if bounces is None else bounces
    rays = scene.camera.recalculate_ray_directions()
    return scene, b, rays, oracle_frames(O, scene, b, frames, rays, compute_per_frame=spp)


@pytest.mark.parametrize("config,w,h", [("c2_rtiow", 64, 36), ("c1_four_spheres", 37, 21)])
def test_both_instances_match_oracle(gpu, config, w, h):
    """A batch of 3 frames on each instance (37x21: partial tiles, the refill's x < width, y < height guard)."""
    scene, bounces, rays, ref = reference(config, w, h, 3)
    new = render(scene, bounces, 3, rays, VARIANT)
    old = render(scene, bounces, 3, rays, GENERIC_BATCH, tuning={"frame_par_instance": 0})
    assert_same(*new, *ref)
    assert_same(*old, *ref)
    assert_same(*new, *old)


def test_samples_restart_in_the_variant(gpu):
    """compute_per_frame 2: finish_sample starts the pixel's second sample inside the variant."""
    scene, bounces, rays, ref = reference("c1_four_spheres", 40, 24, 2, spp=2)
    assert_same(*render(scene, bounces, 2, rays, VARIANT, spp=2), *ref)


@pytest.mark.parametrize("bounces,expect", [(0, GENERIC_BATCH), (1, VARIANT)])
def test_bounce_limit_selects_the_instance(gpu, bounces, expect):
    """bounces 0: every sample ends in setup without a trace, which only the generic instance handles."""
    scene, b, rays, ref = reference("c2_rtiow", 37, 21, 3, bounces=bounces)
    assert b == bounces
    assert_same(*render(scene, bounces, 3, rays, expect), *ref)


def test_one_context_alternates_instances(gpu, oracle_lib):
    """One context: an accumulating batch (variant), a non-accumulating frame (generic), a reset,
    a batch with "frame_parallel" 0 (generic, a pixel's frames back to back on its lane), a batch
    again (variant), and a batch cut short by a readback (variant): the oracle's sequence throughout."""
    scene, bounces = build_config("c2_rtiow", width=64, height=36)
    rays = scene.camera.recalculate_ray_directions()
    o = oracle_lib.Oracle(scene, camera_rays=rays)
    acc_o = np.zeros((36, 64, 4), np.float32)
    out_o = np.zeros((36, 64), np.uint32)
    n_o = 0

    def oracle_step(k, accumulate=1):
        return o.render_frame(scene.params(accumulate=accumulate, accumulation_index=k), bounces, acc_o, out_o)

    with Renderer(scene, camera_rays=rays, frame_batch=3) as r:
        def batch(frames, expect, readback=False):
            for _ in range(frames):
                r.compute_frame(bounces)
            if not readback:
                r.synchronize()
            got = r.read_accumulation(), r.read_output(), r.ray_count()  # (the readback launches the queue)
            assert path_bits(r) == expect, (hex(path_bits(r)), hex(expect))
            return got

        got = batch(3, VARIANT)
        n_o += sum(oracle_step(k) for k in (1, 2, 3))
        assert_same(*got, acc_o, out_o, n_o)

        r.accumulate = False  # a non-accumulating frame: no batch, the generic instance
        r.reset_accumulation()
        acc_o[:] = 0
        got = batch(1, GENERIC)
        n_o += oracle_step(1, accumulate=0)
        assert_same(*got, acc_o, out_o, n_o)

        r.accumulate = True
        r.reset_accumulation()
        acc_o[:] = 0
        r.set_tuning("frame_parallel", 0)
        got = batch(3, GENERIC)
        n_o += sum(oracle_step(k) for k in (1, 2, 3))
        assert_same(*got, acc_o, out_o, n_o)

        r.set_tuning("frame_parallel", 1)
        got = batch(3, VARIANT)
        n_o += sum(oracle_step(k) for k in (4, 5, 6))
        assert_same(*got, acc_o, out_o, n_o)

        got = batch(2, VARIANT, readback=True)  # two queued frames, launched by the readback
        n_o += sum(oracle_step(k) for k in (7, 8))
        assert_same(*got, acc_o, out_o, n_o)


@pytest.mark.parametrize("device_rays", [False, True], ids=["ray_buffer", "device_rays"])
def test_rank_of_a_world_split(gpu, oracle_lib, device_rays):
    """World size 3, rank 1, a batch of 4: the rank's tiles equal the oracle's and nothing else is
    written; then the same with the camera rays generated on the device (rt_update_camera_matrices)."""
    w, h, rank, world, frames = 64, 36, 1, 3, 4
    scene, bounces = build_config("c2_rtiow", width=w, height=h)
    rays = scene.camera.recalculate_ray_directions()
    o = oracle_lib.Oracle(scene, camera_rays=rays)
    acc_o = np.zeros((h, w, 4), np.float32)
    out_o = np.zeros((h, w), np.uint32)
    n_o = sum(o.render_frame(scene.params(accumulation_index=k), bounces, acc_o, out_o, rank=rank, world_size=world)
              for k in range(1, frames + 1))
    kw = dict(device_rays=True) if device_rays else {}
    acc, out, n = render(scene, bounces, frames, None if device_rays else rays, VARIANT, rank=rank, world_size=world,
                         **kw)
    mask = owned_mask(w, h, rank, world)
    assert mask.any() and not acc[~mask].any() and not out[~mask].any()
    assert_same(acc, out, n, acc_o, out_o, n_o)


def schedule_run(scene, bounces, rays, launches, tuning):
    """`launches` batches of 2 frames with cost-ordered claims in batches; the claim order before the last."""
    with Renderer(scene, camera_rays=rays, frame_batch=2,
                  tuning=dict(tuning, tile_schedule=1, batch_schedule=1, batch_overlap=0)) as r:
        order = None
        for i in range(launches):
            if i == launches - 1:
                order, _ = r.tile_schedule_state()
            r.compute_frame(bounces)
            r.compute_frame(bounces)
            r.synchronize()
            assert path_bits(r) == VARIANT
        return order, (r.read_accumulation(), r.read_output(), r.ray_count())


def test_cluster_scene_with_cost_ordered_schedule(gpu, oracle_lib):
    """The cluster scene at its test size (64x40, 6 bounces), batches of 2 with the cost-ordered
    schedule asked for. At this size every wave gets about one unit, so the library leaves the
    schedule off (index order): the variant with the schedule's arguments null."""
    scene = cluster_scene(64, 40)
    rays = scene.camera.recalculate_ray_directions()
    order, got = schedule_run(scene, 6, rays, 2, {})
    assert np.array_equal(order, np.arange(order.size))
    assert_same(*got, *oracle_frames(oracle_lib, scene, 6, 4, rays))


def test_cluster_scene_claims_in_sorted_order(gpu, oracle_lib):
    """The same scene at 512x256 with one wave per SIMD-quarter of a CU ("waves_per_cu" 1: one
    256-thread workgroup per CU, 1024 waves on 256 CUs): 4096 units per batch, the smallest size
    at which the schedule switches on (four units per wave).
    The first batch records costs, the second sorts them, the third claims in the sorted order
    (checked: a permutation that is not the identity) and records in the variant."""
    scene = cluster_scene(512, 256)
    rays = scene.camera.recalculate_ray_directions()
    order, got = schedule_run(scene, 6, rays, 3, {"waves_per_cu": 1})
    assert np.array_equal(np.sort(order), np.arange(order.size))
    assert not np.array_equal(order, np.arange(order.size))
    assert_same(*got, *oracle_frames(oracle_lib, scene, 6, 6, rays))


def test_triangles_in_lds(gpu):
    """C3 at the golden's size (triangle accelerator in LDS), its 2 frames as one batch, on each instance."""
    g, case = load("c3_64x36_b8"), CASES["c3_64x36_b8"]
    assert case["frames"] == 2 and case["spp"] == 1
    scene = scene_from_inputs(g)
    rays = g["camera_rays"].astype(B.RAY)
    ref = g["accum"], g["out"], int(g["rays"])
    assert_same(*render(scene, case["bounces"], 2, rays, VARIANT), *ref)
    assert_same(*render(scene, case["bounces"], 2, rays, GENERIC_BATCH, tuning={"frame_par_instance": 0}), *ref)


def test_triangles_in_global_memory(gpu, oracle_lib):
    """The heightfield of the global-walk parity cases (60x30 cells at 96x64, "lds_mode" 1: the
    triangle accelerator stays in global memory, the primary pre-pass runs), a batch of 2."""
    scene, bounces = build_config("c5_heightfield", width=96, height=64, nx=60, nz=30)
    rays = scene.camera.recalculate_ray_directions()
    ref = oracle_frames(oracle_lib, scene, bounces, 2, rays)
    for tuning, expect in (({"lds_mode": 1}, VARIANT), ({"lds_mode": 1, "frame_par_instance": 0}, GENERIC_BATCH)):
        with Renderer(scene, camera_rays=rays, frame_batch=2, tuning=tuning) as r:
            r.compute_frame(bounces)
            r.compute_frame(bounces)
            r.synchronize()
            assert r.launch_config()["scene_in_lds"] <= 1
            assert path_bits(r) == expect
            assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), *ref)
