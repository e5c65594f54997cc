"""Tuning and mode changes made during a context's life (rt_set_tuning, rt_set_triangle_pruning,
rt_set_brute_force, rt_set_tile_schedule after the first launch).

include/rt_abi.h promises that every setting renders the same bits as the default and that a
setting takes effect from the next launch. The host runtime carries state from launch to launch
-- the double-buffered tile-queue counters, the per-stream schedule state, the occupancy cache,
the dirty flags of the derived accelerator data, capacity-sized buffers, the two batch streams --
so every case here changes a setting on a context that has already launched and compares the
frames after the change, and after the change back, with the CPU oracle, whose result depends on
no tuning: accumulation f32 bits, RGBA8 and ray count equal, no tolerance.

Scenes are the smallest at which each path is live: S (spheres only, 36 tiles: the queue stripes
1..31 own tiles), L (triangle accelerator in LDS), G (accelerator in global memory: quantized
nodes, octant layouts, certificates, cooperative leaves, the primary pre-pass), M (both walks).
Each scene's oracle frames are computed once, frame by frame as the tests ask for them, and shared.
"""
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd.scene import build_config
from tests.sphere_cluster_scene import cluster_scene
from tests.test_gpu_occlusion import INF, check, expected, next_up
from tests.test_gpu_parity import assert_same, oracle_frames
from tests.test_gpu_query import camera_rays, check_hits, oracle_records

pytestmark = pytest.mark.gpu

SCENES = {
    "S": ("c2_rtiow", dict(width=64, height=36)),
    "S2": ("c2_rtiow", dict(width=13, height=7)),  # 2 tiles: fewer units than stripes
    "L": ("c3_chess", dict(width=64, height=40, env_size=(512, 256))),
    "G": ("c5_heightfield", dict(width=64, height=48, nx=200, nz=100)),
    "M": ("c4_mixed", dict(width=96, height=64, env_size=(256, 128))),
}
N_QUERY_RAYS = 300


# ---------------------------------------------------------------------------- references
class Reference:
    """A scene with the oracle's running result: (accumulation, RGBA8, rays) after k = 1, 2, ...
    frames, rendered on demand and kept, and the oracle's records of a few hundred camera rays."""

    def __init__(self, name):
        from oracle import oracle as O

        O.build()
        config, kw = SCENES[name]
        self.O = O
        self.scene, self.bounces = build_config(config, **kw)
        self.rays = self.scene.camera.recalculate_ray_directions()
        self._oracle = O.Oracle(self.scene, camera_rays=self.rays)
        self._acc = np.zeros((self._oracle.height, self._oracle.width, 4), np.float32)
        self._out = np.zeros((self._oracle.height, self._oracle.width), np.uint32)
        self._n = 0
        self._after = []
        self._query = None

    def after(self, frames):
        while len(self._after) < frames:
            k = len(self._after) + 1
            self._n += self._oracle.render_frame(self.scene.params(accumulation_index=k), self.bounces, self._acc,
                                                 self._out)
            self._after.append((self._acc.copy(), self._out.copy(), self._n))
        return self._after[frames - 1]

    def query(self):
        if self._query is None:
            rays = camera_rays(self.scene, N_QUERY_RAYS)
            self._query = rays, oracle_records(self.O, self.scene, rays)
        return self._query


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(name)


def check_frame(label, got, want):
    """(accumulation, RGBA8, rays) against the oracle's, naming the step and the wrong pixels."""
    bad = int((got[0].view(np.uint32) != want[0].view(np.uint32)).any(axis=-1).sum())
    bad_out = int((got[1] != want[1]).sum())
    assert bad == 0 and bad_out == 0 and got[2] == want[2], \
        f"{label}: {bad} accumulation pixels and {bad_out} RGBA8 pixels differ; rays {got[2]}, the oracle's {want[2]}"
    assert_same(*got, *want)


def readback(r):
    return r.read_accumulation(), r.read_output(), r.ray_count()


@dataclasses.dataclass
class Launch:
    """What the library reports about the last launch."""
    cfg: dict
    mask: int
    passes: list
    frames: int


class Run:
    """One context and the number of frames it has rendered; every step is compared with the oracle."""

    def __init__(self, r, ref, frames):
        self.r, self.ref, self.frames, self.k = r, ref, frames, 0

    def step(self, label, frames=None):
        """One launch pattern's worth of frames (one compute_frame with frame_batch 1, or one
        compute_frames batch), compared with the oracle's running result."""
        frames = self.frames if frames is None else frames
        if frames == 1:
            self.r.compute_frame(self.ref.bounces)
        else:
            self.r.compute_frames(self.ref.bounces, frames)
        self.k += frames
        check_frame(f"{label}, frame {self.k}", readback(self.r), self.ref.after(self.k))
        return Launch(self.r.launch_config(), self.r.last_launch_pass_mask(), self.r.last_launch_passes(), frames)


# ---------------------------------------------------------------------------- 1. the transition walk
def effect_threads(v, now, base):
    assert now.cfg["threads"] == (v or base.cfg["threads"])


def effect_scene_in_lds(v, now, base):
    assert now.cfg["scene_in_lds"] == (base.cfg["scene_in_lds"] if v else 0)


def effect_lds_mode(v, now, base):
    assert now.cfg["scene_in_lds"] == min(v, base.cfg["scene_in_lds"])


def effect_primary(v, now, base):
    mode = now.cfg["scene_in_lds"]  # by default the pre-pass runs where the accelerator stays in global memory
    assert bool(now.mask & N.RT_PASS_PRIMARY) == (mode >= 1 and (v == 1 or (v == -1 and mode == 1)))


def effect_brute(v, now, base):
    assert now.passes == {0: base.passes, 1: ["brute"], 2: ["brute", "brute_stream"]}[v]


def effect_frame_parallel(v, now, base):
    batch = now.frames > 1 and v == 1  # a frame-parallel batch: its resolve pass, its own instance
    assert bool(now.mask & N.RT_PASS_RESOLVE) == batch and bool(now.mask & N.RT_PASS_PATH_FRAME_PAR) == batch


def effect_frame_par_instance(v, now, base):
    assert bool(now.mask & N.RT_PASS_RESOLVE) == (now.frames > 1)
    assert bool(now.mask & N.RT_PASS_PATH_FRAME_PAR) == (now.frames > 1 and v == 1)


def tuning(name):
    return lambda r, v: r.set_tuning(name, v)


@dataclasses.dataclass
class Key:
    name: str
    values: tuple            # the non-default values, each followed by the default ...
    default: int
    effect: object = None    # what launch_config / last_launch_passes must report under a value
    sequence: tuple = None   # ... or the values to step through as given
    call: object = None      # how the value is set (default: rt_set_tuning)

    def steps(self):
        if self.sequence is not None:
            return self.sequence
        return tuple(x for v in self.values for x in (v, self.default))

    def set(self, r, v):
        (self.call or tuning(self.name))(r, v)


SPHERE_KEYS = [
    Key("sphere_bvh", (0,), 1),
    Key("sphere_leaf", (1, 64), 0),
    Key("sphere_octants", (0,), 1),
    Key("sphere_box_order", (0,), 1),
    Key("trav_threshold", (1, 63), 0),
    Key("drain_threshold", (0, 63), 32),
    Key("drain_min_steps", (0,), 64),
    Key("block_threads", (256, 512, 1024), 0, effect_threads),
    Key("waves_per_cu", (1, 32), 0),
    Key("scene_in_lds", (0,), 1, effect_scene_in_lds),
    Key("lds_mode", (0, 1), 2, effect_lds_mode),
    Key("frame_parallel", (0,), 1, effect_frame_parallel),
    Key("frame_par_instance", (0,), 1, effect_frame_par_instance),
    Key("unit_tile_major", (0,), 1),
    Key("batch_overlap", (0,), 1),
    Key("batch_schedule", (1,), 0),
    Key("tile_schedule", (0,), 1),
]
TRIANGLE_KEYS = [
    Key("tri_bvh", (0,), 1),
    Key("tri_octants", (0,), 1),
    Key("tri_qnodes", (0,), 1),
    Key("coop_leaves", (0,), 1),
    Key("stage_subs", (0,), 1),
    Key("leaf_batch", (1, 8), 0),
    Key("lds_mode", (0, 1), 2, effect_lds_mode),
    Key("primary_pass", (0, 1), -1, effect_primary),
    Key("primary_threads", (64, 1024), 256),
    Key("primary_waves", (0,), 8),
    Key("primary_tile_major", (0,), 1),
    Key("rt_set_triangle_pruning", (0,), 1, call=lambda r, v: r.set_triangle_pruning(v)),  # (mode 2 is not exact)
    Key("rt_set_brute_force", (), 0, effect_brute, sequence=(1, 2, 0), call=lambda r, v: r.set_brute_force(v)),
]
# where both walks matter: the sphere and the triangle structures rebuilt and re-placed in one scene
MIXED_KEYS = [
    Key("sphere_bvh", (0,), 1),
    Key("sphere_leaf", (1,), 0),
    Key("tri_bvh", (0,), 1),
    Key("tri_octants", (0,), 1),
    Key("scene_in_lds", (0,), 1, effect_scene_in_lds),
    Key("lds_mode", (0, 1), 2, effect_lds_mode),
]
WALKS = {"S": SPHERE_KEYS, "L": TRIANGLE_KEYS, "G": TRIANGLE_KEYS, "M": MIXED_KEYS}


@pytest.mark.parametrize("frames", [1, 3], ids=["frame_batch_1", "batches_of_3"])
@pytest.mark.parametrize("name", sorted(WALKS))
def test_transition_walk(gpu, oracle_lib, name, frames):
    """One context; for each key in turn: a non-default value, a launch, the default again, a
    launch, every launch compared with the oracle's running result -- so a leftover of key i
    shows at key i's second launch or at key i + 1. A launch is one frame (frame_batch 1), or a
    batch of 3 (compute_frames: the frame-parallel path with its resolve, alternating streams).
    Where launch_config() or last_launch_passes() reports the setting, the launch after the call
    ran under it."""
    ref = reference(name)
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=1) as r:
        run = Run(r, ref, frames)
        base = run.step("defaults")
        if name == "L":
            assert base.cfg["scene_in_lds"] == 2  # the triangle accelerator in LDS
        if name == "G":
            assert base.cfg["scene_in_lds"] == 1 and base.mask & N.RT_PASS_PRIMARY  # ... in global memory
        for key in WALKS[name]:
            for v in key.steps():
                key.set(r, v)
                now = run.step(f"{name}: {key.name} = {v}")
                if key.effect:
                    key.effect(v, now, base)
                if v == key.default:  # back at the defaults' launch, whatever the key does
                    assert (now.cfg["threads"], now.cfg["scene_in_lds"], now.mask) == \
                           (base.cfg["threads"], base.cfg["scene_in_lds"], base.mask), (key.name, now, base)


# ---------------------------------------------------------------------------- 2. queue stripes
STRIPE_SEQUENCES = {"32_1_32": (32, 1, 32), "32_64_3_64_1_32_7": (32, 64, 3, 64, 1, 32, 7)}


@pytest.mark.parametrize("pattern", ["frames", "batches_of_3", "split_12"])
@pytest.mark.parametrize("seq", sorted(STRIPE_SEQUENCES))
def test_queue_stripes_sequence(gpu, oracle_lib, seq, pattern):
    """A launch zeroes the counter half the stream's next launch claims from. After launches at
    32, 1 and 32 stripes the third finds, unless all 64 counters of a half are zeroed whatever
    the stripe count, stripes 1..31 of its half at the first launch's final counts: drained, so
    their tiles are never rendered. Single-frame launches, batches of 3, and 12-frame calls that a
    1 MiB batch budget splits into two batches on the two streams, each with its own parity."""
    ref = reference("S")
    frames = {"frames": 1, "batches_of_3": 3, "split_12": 12}[pattern]
    extra = {"batch_memory_mb": 1} if pattern == "split_12" else {}
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=1, tuning=extra) as r:
        run = Run(r, ref, frames)
        for stripes in STRIPE_SEQUENCES[seq]:
            r.set_tuning("queue_stripes", stripes)
            now = run.step(f"queue_stripes = {stripes} of {seq}, {pattern}")
            assert bool(now.mask & N.RT_PASS_RESOLVE) == (frames > 1)


def test_queue_stripes_more_stripes_than_units(gpu, oracle_lib):
    """13x7, 2 tiles: 1, 2, 33 and 64 stripes, most of which own no unit."""
    ref = reference("S2")
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=1) as r:
        assert r.owned_pixel_count() // 64 == 2
        run = Run(r, ref, 1)
        for stripes in (1, 2, 33, 64, 1):
            r.set_tuning("queue_stripes", stripes)
            run.step(f"queue_stripes = {stripes}, 2 tiles")
        for stripes in (64, 2):
            r.set_tuning("queue_stripes", stripes)
            run.step(f"queue_stripes = {stripes}, 2 tiles, a batch of 3", frames=3)


# ---------------------------------------------------------------------------- 3. changes that meet other state
def check_queries(r, ref, label):
    """trace_rays and occluded on the camera rays against the oracle's records: t_max at the
    closest distance (0), one ulp above it (1) and +inf."""
    rays, want = ref.query()
    check_hits(ref.O, ref.scene, rays, r.trace_rays(rays), want)
    t = want["rec"]["t"]
    for t_max in (t, next_up(t), np.full_like(t, INF)):
        check(r.occluded(np.concatenate([rays, t_max[:, None]], axis=1).astype(np.float32)), expected(t, t_max))


@pytest.mark.parametrize("name,key,value,default", [
    ("S", "sphere_leaf", 1, 0), ("S", "sphere_bvh", 0, 1),
    ("L", "tri_octants", 0, 1), ("L", "tri_bvh", 0, 1), ("L", "tri_qnodes", 0, 1),
    ("G", "tri_octants", 0, 1), ("G", "tri_bvh", 0, 1), ("G", "tri_qnodes", 0, 1),
])
def test_queries_after_a_change(gpu, oracle_lib, name, key, value, default):
    """A change that marks an accelerator stale, then queries before any frame is rendered: the
    query path does the rebuild and the derivations itself. Then a frame, the change back, queries
    and a frame again."""
    ref = reference(name)
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=1) as r:
        run = Run(r, ref, 1)
        run.step("defaults")
        for v in (value, default):
            r.set_tuning(key, v)
            check_queries(r, ref, f"{name}: {key} = {v}")
            run.step(f"{name}: {key} = {v}, after the queries")
            check_queries(r, ref, f"{name}: {key} = {v}, after the frame")


@pytest.mark.parametrize("lds_mode", [2, 1], ids=["accelerator_in_lds", "accelerator_in_global_memory"])
@pytest.mark.parametrize("edit_first", [False, True], ids=["dirty_then_edit", "edit_then_dirty"])
def test_device_edit_while_the_accelerator_is_dirty(gpu, oracle_lib, edit_first, lds_mode):
    """set_tuning("tri_octants", 0) marks the triangle accelerator for a host rebuild; a device
    edit (update_scene(device=True), two pieces moved) then meets a tree it must not refit, and
    the rebuild must start from the device's geometry. And the reverse order. The frame equals the
    oracle's on the edited scene; the device's geometry equals the host rebuild."""
    from rust_gpu_raytracing_amd import builder

    config, kw = SCENES["L"]
    scene, bounces = build_config(config, **kw)  # (edited below: not the shared one)
    rays = scene.camera.recalculate_ray_directions()
    with Renderer(scene, camera_rays=rays, frame_batch=1, tuning={"lds_mode": lds_mode}) as r:
        r.compute_frame(bounces)  # the accelerator is built and in use
        assert r.launch_config()["scene_in_lds"] == lds_mode
        for o, shift in ((scene.objects[3], (0.75, 0.0, -0.5)), (scene.objects[17], (-0.5, 0.25, 1.0))):
            o.transformation = (np.asarray(o.transformation) + np.array(shift)).astype(np.float32)
        scene.objects[17].rotation = np.array([0.0, 35.0, 0.0], np.float32)
        if edit_first:
            r.update_scene(device=True)
            r.set_tuning("tri_octants", 0)
        else:
            r.set_tuning("tri_octants", 0)
            r.update_scene(device=True)
        r.reset_ray_count()
        r.compute_frame(bounces)
        got = readback(r)
        geo = r.read_geometry()
        r.set_tuning("tri_octants", 1)  # and the rebuild back, from the edited geometry again
        r.compute_frame(bounces)
        got2 = readback(r)
    for o in scene.objects:
        builder.update_object(o)
    objs, subs, tris = scene.flatten()
    assert geo[0].tobytes() == objs.tobytes()
    assert geo[1].tobytes() == subs.tobytes()
    assert geo[2].tobytes() == tris.tobytes()
    o = oracle_lib.Oracle(scene, camera_rays=rays)
    acc = np.zeros((o.height, o.width, 4), np.float32)
    out = np.zeros((o.height, o.width), np.uint32)
    n = o.render_frame(scene.params(accumulation_index=1), bounces, acc, out)
    check_frame("the frame after the edit", got, (acc, out, n))
    n += o.render_frame(scene.params(accumulation_index=2), bounces, acc, out)
    check_frame("the frame after tri_octants = 1", got2, (acc, out, n))


@pytest.mark.parametrize("name,key,value", [("S", "queue_stripes", 1), ("L", "tri_bvh", 0), ("L", "block_threads", 256),
                                            ("G", "tri_bvh", 0)])
def test_change_with_frames_queued(gpu, oracle_lib, name, key, value):
    """The default frame queue: two frames queued, the change (which launches them, under the
    setting they were queued with), one more frame and a readback: the oracle's three frames."""
    ref = reference(name)
    with Renderer(ref.scene, camera_rays=ref.rays) as r:
        assert r.frame_batch()[0] > 3
        r.compute_frame(ref.bounces)
        r.compute_frame(ref.bounces)
        assert r.frame_batch()[1] == 2
        r.set_tuning(key, value)
        assert r.frame_batch()[1] == 0
        check_frame(f"{name}: the two frames queued before {key} = {value}", readback(r), ref.after(2))
        r.compute_frame(ref.bounces)
        assert r.frame_batch()[1] == 1
        check_frame(f"{name}: {key} = {value} with frames queued", readback(r), ref.after(3))
        if key == "block_threads":
            assert r.launch_config()["threads"] == value


def test_growth_across_a_change(gpu, oracle_lib):
    """G starts without cooperative leaves and with box culling only, so neither the leaf triangle
    blocks nor the leaf certificates exist when it first renders; both are switched on and must be
    allocated and derived then."""
    ref = reference("G")
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=1, tuning={"coop_leaves": 0}) as r:
        r.set_triangle_pruning(0)
        run = Run(r, ref, 1)
        run.step("coop_leaves = 0, pruning 0")
        assert r.check_leaf_certificates() == (0, 0, 0)  # none built
        r.set_tuning("coop_leaves", 1)
        r.set_triangle_pruning(1)
        run.step("coop_leaves = 1, pruning 1")
        mismatches, valid, total = r.check_leaf_certificates()
        assert mismatches == 0 and total > 0 and valid > 0, (mismatches, valid, total)
        run.step("coop_leaves = 1, pruning 1, a batch of 3", frames=3)
        mismatches, valid, total = r.check_leaf_certificates()
        assert mismatches == 0 and total > 0, (mismatches, valid, total)


def test_batch_buffers_grow_between_overlapped_batches(gpu, oracle_lib):
    """G with frame_batch 2: the first batch sizes the frame lights and the primary records for
    batches of 2. Batches of 2, 2, 8 and 2 frames: the batch of 8 needs more of both, so both
    pairs are reallocated while the batch before it ran on the other stream, and the batch after
    it runs in the larger buffers. Every batch equals the oracle's running result."""
    ref = reference("G")
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=2) as r:
        run = Run(r, ref, 2)
        for i, frames in enumerate((2, 2, 8, 2)):
            now = run.step(f"G: batch {i} of {frames} frames", frames=frames)
            if frames == 8:  # a frame-parallel batch with the pre-pass: the two buffers that grew
                assert now.mask & N.RT_PASS_PRIMARY and now.mask & N.RT_PASS_RESOLVE, now
        assert run.k == 14


def test_launch_timing_across_overlapped_batches(gpu, oracle_lib):
    """S in batches of 3: one untimed batch (the primary stream), then timing on and four more,
    the first of them on the auxiliary stream behind the primary stream's zeroing of the clock
    slots. One path launch and one resolve per frame-parallel batch: exactly 4 timed spans of
    each, with positive totals (no bound on the times), and the 15 frames equal the oracle's."""
    ref = reference("S")
    with Renderer(ref.scene, camera_rays=ref.rays, frame_batch=3) as r:
        run = Run(r, ref, 3)
        run.step("S: the untimed batch")
        r.set_timing(True)
        for i in range(4):
            now = run.step(f"S: timed batch {i}")
            assert now.mask & N.RT_PASS_RESOLVE, now
        r.synchronize()
        ms, n = r.dispatch_time_total()
        assert n == 4 and ms > 0.0, (ms, n)
        ms, n = r.resolve_time_total()
        assert n == 4 and ms > 0.0, (ms, n)
        assert run.k == 15


# ---------------------------------------------------------------------------- 4. the schedule key
def test_tile_schedule_key_discards_the_recorded_schedule(gpu, oracle_lib):
    """The size and pattern of test_cluster_scene_claims_in_sorted_order (512x256, "waves_per_cu" 1,
    batches of 2: the smallest size at which the schedule switches on). Once a claim order that is
    not the identity exists, the key "tile_schedule" set to 0 and to 1 again must leave what
    rt_set_tile_schedule documents: the identity order and zero costs. The batches after it equal
    the oracle's, and sort a new order."""
    scene = cluster_scene(512, 256)
    rays = scene.camera.recalculate_ray_directions()
    bounces = 6
    identity = np.arange(512 * 256 // 64)
    with Renderer(scene, camera_rays=rays, frame_batch=2,
                  tuning=dict(waves_per_cu=1, tile_schedule=1, batch_schedule=1, batch_overlap=0)) as r:
        def batch():
            r.compute_frame(bounces)
            r.compute_frame(bounces)
            r.synchronize()

        batch()  # records costs
        batch()  # sorts them
        order, costs = r.tile_schedule_state()
        assert np.array_equal(np.sort(order), identity) and not np.array_equal(order, identity)
        assert costs.any()
        r.set_tuning("tile_schedule", 0)
        r.set_tuning("tile_schedule", 1)
        order, costs = r.tile_schedule_state()
        assert np.array_equal(order, identity) and not costs.any()
        batch()
        order, costs = r.tile_schedule_state()
        assert np.array_equal(order, identity) and costs.any()  # the first launch since: index order, costs recorded
        batch()
        order, _ = r.tile_schedule_state()
        assert np.array_equal(np.sort(order), identity) and not np.array_equal(order, identity)
        batch()
        got = readback(r)
    check_frame("five batches of 2 around the schedule reset", got, oracle_frames(oracle_lib, scene, bounces, 10, rays))
