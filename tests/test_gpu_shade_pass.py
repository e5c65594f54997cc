"""The path kernel's shading pass on the GPU (csrc/pathtrace.hip, DESIGN.md §5 "Shading pass"): the
environment line -- the decoded texels of a rows- or columns-uniform environment map staged in LDS
by the instances that stage the scene -- and the tile costs of a frame-parallel batch, recorded
from the batch's first frame only.

Every case is bit-exact against the CPU oracle: accumulation bits, RGBA8 and ray count
(``assert_same``). Frames are 64x36 or smaller, but the one case that needs 4096 queue units for
the cost-ordered schedule to switch on in a batch. Whether the line was staged is read from the
launch's LDS size (Renderer.launch_config): the line lies after the scene image, 16 bytes per texel.
Oracle references are computed once per input and shared, never modified.
"""
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import RenderScene, _sphere, build_config
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.test_gpu_parity import assert_same, owned_mask

pytestmark = pytest.mark.gpu

ENV_LINE_MAX = 512  # kEnvLineMax, csrc/rt_kernel_args.h
FRAME_PAR = N.RT_PASS_PATH | N.RT_PASS_RESOLVE | N.RT_PASS_PATH_FRAME_PAR
GENERIC_BATCH = N.RT_PASS_PATH | N.RT_PASS_RESOLVE
GENERIC = N.RT_PASS_PATH
BATCH = 4


# ---------------------------------------------------------------------------- inputs
def env_map(kind):
    """(map, texels of its environment line: 0 when rt_upload_env_map finds no uniform axis or the
    line is longer than ENV_LINE_MAX). Rows-uniform maps are 3 wide, columns-uniform ones 3 high."""
    rng = np.random.default_rng(29)
    axis, _, n = kind.partition("_")
    if axis == "rows":
        n = int(n)
        env = np.broadcast_to(rng.integers(0, 256, (n, 1, 4), dtype=np.uint8), (n, 3, 4))
        line = 1 if n == 1 else n  # one row: its columns are uniform too
    elif axis == "cols":
        n = int(n)
        env = np.broadcast_to(rng.integers(0, 256, (1, n, 4), dtype=np.uint8), (3, n, 4))
        line = 1 if n == 1 else n
    elif kind == "both":
        env, line = np.broadcast_to(np.array([40, 90, 200, 255], np.uint8), (5, 9, 4)), 1
    elif kind == "one_texel_off":
        env = np.array(np.broadcast_to(rng.integers(0, 256, (16, 1, 4), dtype=np.uint8), (16, 3, 4)))
        env[8, 1, 0] ^= 0x40
        line = 0
    else:
        assert kind == "random"
        env, line = rng.integers(0, 256, (16, 8, 4), dtype=np.uint8), 0
    return np.ascontiguousarray(env), (line if line <= ENV_LINE_MAX else 0)


SIZES = (1, 2, 512, ENV_LINE_MAX, ENV_LINE_MAX + 1)
MAPS = ["rows_%d" % n for n in dict.fromkeys(SIZES)] + ["cols_%d" % n for n in dict.fromkeys(SIZES)] + [
    "both", "one_texel_off", "random"]


@functools.lru_cache(maxsize=None)
def base_scene(name):
    """(scene, bounces, camera rays). "c2": the C2 fixture's scene, 64x36, 8 bounces. "four": four small
    spheres in front of the C1 camera at 40x24, most rays miss; the first pixels of its ray table hold
    a zero direction, directions with one infinite component and one with a NaN (sample_env's v, or
    u, is then NaN or out of range: texel_coord's clamps decide the texel)."""
    if name == "c2":
        scene, bounces = build_config("c2_rtiow", width=64, height=36)
        return scene, bounces, scene.camera.recalculate_ray_directions()
    base, bounces = build_config("c1_four_spheres", width=40, height=24)
    rays = base.camera.recalculate_ray_directions().copy()
    cam = np.asarray(base.camera.position, np.float32)
    mid = rays["direction"].reshape(24, 40, 3)[12, 20]
    right = rays["direction"].reshape(24, 40, 3)[12, 30] - mid
    up = rays["direction"].reshape(24, 40, 3)[4, 20] - mid
    sph = [_sphere((cam + 6.0 * (mid + a * right + b * up)).astype(np.float32), 0.45, i % base.materials.shape[0])
           for i, (a, b) in enumerate([(-1.2, 0.4), (-0.3, -0.7), (0.5, 0.6), (1.3, -0.2)])]
    scene = RenderScene(np.stack(sph).astype(B.SPHERE), base.materials, [], base.textures, base.environment_map,
                        base.camera, name="four_small")
    inf = np.float32(np.inf)
    special = [(0, 0, 0), (inf, 0, 0), (0, inf, 0), (0, -inf, 0), (0, 0, inf), (0.3, np.nan, -1.0)]
    rays["direction"][:len(special)] = np.array(special, np.float32)
    return scene, bounces, rays


def with_env(scene, env):
    return dataclasses.replace(scene, environment_map=env)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """(scene with the map, bounces, rays, oracle after BATCH accumulated frames, oracle's one
    non-accumulating frame)."""
    from oracle import oracle as O

    O.build()
    scene, bounces, rays = base_scene(name)
    scene = with_env(scene, env_map(kind)[0])
    o = O.Oracle(scene, camera_rays=rays)
    acc = np.zeros((o.height, o.width, 4), np.float32)
    out = np.zeros((o.height, o.width), np.uint32)
    n = sum(o.render_frame(scene.params(accumulation_index=k), bounces, acc, out) for k in range(1, BATCH + 1))
    acc1 = np.zeros_like(acc)
    out1 = np.zeros_like(out)
    n1 = o.render_frame(scene.params(accumulate=0, accumulation_index=1), bounces, acc1, out1)
    return scene, bounces, rays, (acc, out, n), (acc1, out1, n1)


# launch kind -> (Renderer arguments, frames, expected pass mask, scene staged in LDS)
LAUNCHES = {
    "frame_par_instance": (dict(frame_batch=BATCH), BATCH, FRAME_PAR, True),
    "generic_instance": (dict(frame_batch=BATCH, tuning={"frame_par_instance": 0}), BATCH, GENERIC_BATCH, True),
    "no_accumulation": (dict(accumulate=False), 1, GENERIC, True),
    "frame_parallel_0": (dict(frame_batch=BATCH, tuning={"frame_parallel": 0}), BATCH, GENERIC, True),
    "lds_mode_0": (dict(frame_batch=BATCH, tuning={"lds_mode": 0}), BATCH, FRAME_PAR, False),
}


def launch(scene, bounces, rays, kind):
    """One launch of `kind`: (accumulation, RGBA8, rays), the launch's LDS bytes."""
    kw, frames, expect, staged = LAUNCHES[kind]
    with Renderer(scene, camera_rays=rays, **kw) as r:
        for _ in range(frames):
            r.compute_frame(bounces)
        r.synchronize()
        assert r.last_launch_pass_mask() & ~N.RT_PASS_PRIMARY == expect
        cfg = r.launch_config()
        assert (cfg["scene_in_lds"] >= 1) == staged
        return (r.read_accumulation(), r.read_output(), r.ray_count()), cfg["lds_bytes"]


@functools.lru_cache(maxsize=None)
def lds_without_line(name, kind):
    """The launch's LDS bytes with a map that has no line (the scene image does not depend on the map)."""
    scene, bounces, rays, _, _ = reference(name, "random")
    return launch(scene, bounces, rays, kind)[1]


# ---------------------------------------------------------------------------- environment line
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("name", ["c2", "four"])
def test_env_line_matches_oracle(gpu, name, kind):
    """Every map through the frame-parallel instance (a batch of 4), the generic instance (the same
    batch with "frame_par_instance" 0, and a non-accumulating frame), "frame_parallel" 0 and mode 0
    ("lds_mode" 0: the global path). The line is staged exactly where it applies: its texels x 16
    bytes of LDS after the image in modes 1 and 2, none in mode 0, for lines over the cap and for
    maps without a uniform axis."""
    scene, bounces, rays, ref_acc, ref_one = reference(name, kind)
    line = env_map(kind)[1]
    for launch_kind, (_, _, _, staged) in LAUNCHES.items():
        got, lds = launch(scene, bounces, rays, launch_kind)
        assert_same(*got, *(ref_one if launch_kind == "no_accumulation" else ref_acc))
        want = 16 * line if staged else 0
        assert lds - lds_without_line(name, launch_kind) == want, (launch_kind, lds, want)


def test_env_upload_between_launches(gpu, oracle_lib):
    """Two batches with a rows-uniform map, another rows-uniform map of the same size, a batch, a
    map without a uniform axis, a batch: each upload takes effect at the next launch (the line is
    staged per launch from the map in device memory; the last launch has no line)."""
    scene, bounces, rays = base_scene("four")
    rng = np.random.default_rng(31)
    maps = [np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, (16, 1, 4), dtype=np.uint8), (16, 3, 4)))
            for _ in range(2)] + [rng.integers(0, 256, (16, 3, 4), dtype=np.uint8)]
    steps = [(maps[0], 2, 16), (maps[1], 1, 16), (maps[2], 1, 0)]  # (map, batches, line texels)
    acc_o = np.zeros((24, 40, 4), np.float32)
    out_o = np.zeros((24, 40), np.uint32)
    n_o, k = 0, 1
    with Renderer(with_env(scene, maps[0]), camera_rays=rays, frame_batch=2) as r:
        lds = []
        for env, batches, line in steps:
            r.scene = with_env(scene, env)
            r._upload_textures()
            o = oracle_lib.Oracle(r.scene, camera_rays=rays)
            for _ in range(batches):
                r.compute_frame(bounces)
                r.compute_frame(bounces)
                r.synchronize()
                assert r.last_launch_pass_mask() == FRAME_PAR
                n_o += sum(o.render_frame(r.scene.params(accumulation_index=j), bounces, acc_o, out_o)
                           for j in (k, k + 1))
                k += 2
                assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), acc_o, out_o, n_o)
                lds.append(r.launch_config()["lds_bytes"])
        assert [b - lds[-1] for b in lds] == [256, 256, 256, 0]


# ---------------------------------------------------------------------------- tile costs
SCHEDULE = dict(tile_schedule=1, batch_schedule=1, batch_overlap=0)
LAUNCHES_PER_RUN = 3  # record, sort, claim in the sorted order


def schedule_run(scene, bounces, rays, batch, tuning, **kw):
    """LAUNCHES_PER_RUN launches of `batch` frames; the claim order of the last one, and the result."""
    with Renderer(scene, camera_rays=rays, frame_batch=batch, tuning=tuning, **kw) as r:
        order = None
        for i in range(LAUNCHES_PER_RUN):
            if i == LAUNCHES_PER_RUN - 1:
                order, _ = r.tile_schedule_state()
            for _ in range(batch):
                r.compute_frame(bounces)
            r.synchronize()
        return order, (r.read_accumulation(), r.read_output(), r.ray_count())


@functools.lru_cache(maxsize=None)
def schedule_reference(name, frames, rank=0, world=1):
    from oracle import oracle as O

    O.build()
    if name == "c3":
        g, case = load("c3_64x36_b8"), CASES["c3_64x36_b8"]
        scene, bounces, rays = scene_from_inputs(g), case["bounces"], g["camera_rays"].astype(B.RAY)
    elif name == "c1_128x104":
        scene, bounces = build_config("c1_four_spheres", width=128, height=104)
        rays = scene.camera.recalculate_ray_directions()
    else:
        scene, bounces, rays = base_scene("c2")
    o = O.Oracle(scene, camera_rays=rays)
    acc = np.zeros((o.height, o.width, 4), np.float32)
    out = np.zeros((o.height, o.width), np.uint32)
    n = sum(o.render_frame(scene.params(accumulation_index=k), bounces, acc, out, rank=rank, world_size=world)
            for k in range(1, frames + 1))
    return scene, bounces, rays, (acc, out, n)


@pytest.mark.parametrize("batch", [1, 2, 5, 20])
@pytest.mark.parametrize("name", ["c2", "c3"])
def test_tile_costs_of_a_batch(gpu, name, batch):
    """C2 64x36 and C3's fixture with the cost-ordered schedule asked for in batches too, three
    launches of 1, 2, 5 and 20 frames: bit-identical to "tile_schedule" 0 and to the oracle, the
    oracle's ray count. (At this size a wave gets about one unit, so the library leaves the order
    alone: the cases check the recording's gate; the sorted order is claimed in
    test_first_frame_costs_sort_a_batch and tests/test_gpu_frame_par_instance.py.)"""
    scene, bounces, rays, ref = schedule_reference(name, LAUNCHES_PER_RUN * batch)
    _, on = schedule_run(scene, bounces, rays, batch, SCHEDULE)
    _, off = schedule_run(scene, bounces, rays, batch, dict(SCHEDULE, tile_schedule=0))
    assert_same(*on, *ref)
    assert_same(*off, *ref)


def test_tile_costs_of_a_rank(gpu):
    """C2 64x36 split over 4 ranks, batches of 5: every rank's tiles equal the oracle's."""
    for rank in range(4):
        scene, bounces, rays, ref = schedule_reference("c2", LAUNCHES_PER_RUN * 5, rank, 4)
        _, (acc, out, n) = schedule_run(scene, bounces, rays, 5, SCHEDULE, rank=rank, world_size=4)
        mask = owned_mask(64, 36, rank, 4)
        assert mask.any() and not acc[~mask].any() and not out[~mask].any()
        assert_same(acc, out, n, *ref)


def test_first_frame_costs_sort_a_batch(gpu):
    """C1 at 128x104 (208 tiles) in batches of 20 with one 256-thread workgroup per CU
    ("waves_per_cu" 1): 4160 units per batch, four per wave on 256 CUs, the smallest batch of 20 at which
    the schedule switches on. The first batch records its first frame's rays per tile, the second
    sorts them, the third claims in that order: a permutation that is not the identity, and the
    image of "tile_schedule" 0 and of the oracle."""
    scene, bounces, rays, ref = schedule_reference("c1_128x104", LAUNCHES_PER_RUN * 20)
    order, on = schedule_run(scene, bounces, rays, 20, dict(SCHEDULE, waves_per_cu=1))
    _, off = schedule_run(scene, bounces, rays, 20, dict(SCHEDULE, waves_per_cu=1, tile_schedule=0))
    assert np.array_equal(np.sort(order), np.arange(order.size))
    assert not np.array_equal(order, np.arange(order.size))
    assert_same(*on, *ref)
    assert_same(*off, *ref)
