"""Motion records for the temporal denoiser on the GPU (rt_read_feature_ids,
rt_denoise_temporal_motion).

Every comparison is bit for bit: the ID plane against ``trace_rays`` on the pixel rays; the filtered
f32 result, the packed result, rt_read_temporal's colour and its history plane against the NumPy
restatement of the motion contract (tests/temporal_motion_ref.py), fed the device's own accumulation
readback, oracle-built features of the host-rebuilt scene and ids from ``trace_rays``.
"""
import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError, builder, motion
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd.camera import Camera
from rust_gpu_raytracing_amd.scene import build_config
from tests import denoise_ref as R
from tests import temporal_motion_ref as TM
from tests import temporal_ref as T
from tests.golden.fixtures import CASES

pytestmark = pytest.mark.gpu

CHESS = dict(width=64, height=36, env_size=(512, 256))
# The sequence looks at the board's centre from closer than the scene's own camera, from where a piece
# covers two to four pixels of a 64x36 frame: from here the largest covers about fifty.
CHESS_EYE, CHESS_TARGET = (0.0, -3.085, 11.25), (0.0, -0.7, 0.0)
# The edit of step 2: the chosen piece is translated, rotated and scaled.
MAIN_EDIT = dict(translate=(0.35, 0.0, -0.25), rotation=(0.0, 25.0, 0.0), scale=1.1)
# The edit of step 3: another piece and a sphere move, and the camera does.
SECOND_EDIT = dict(translate=(-0.3, 0.0, 0.4), rotation=(0.0, -15.0, 0.0), scale=0.95)
SPHERE_MOVE = (0.3, 0.1, -0.2)
CAMERA_MOVE = dict(right=0.6, up=0.4, forward=0.0, yaw=6.0, pitch=-4.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def apply_edit(obj, edit):
    obj.transformation = (np.asarray(obj.transformation, np.float32) + np.asarray(edit["translate"], np.float32)) \
        .astype(np.float32)
    obj.rotation = np.asarray(edit["rotation"], np.float32)
    obj.scale = np.float32(edit["scale"])


def moved_camera(cam0, right, up, forward, yaw, pitch):
    fwd = cam0.direction.astype(np.float64) / np.linalg.norm(cam0.direction)
    rgt = np.cross(fwd, [0.0, 1.0, 0.0])
    rgt /= np.linalg.norm(rgt)
    upv = np.cross(rgt, fwd)
    a, b = np.radians(yaw), np.radians(pitch)
    d = (fwd * np.cos(a) + rgt * np.sin(a)) * np.cos(b) + upv * np.sin(b)
    return Camera(cam0.viewport_width, cam0.viewport_height,
                  position=(cam0.position + right * rgt + up * upv + forward * fwd).astype(np.float32),
                  direction=d.astype(np.float32))


def chess_scene():
    scene, bounces = build_config("c3_chess", **CHESS)
    eye, d = np.asarray(CHESS_EYE, np.float32), np.asarray(CHESS_TARGET, np.float64) - np.asarray(CHESS_EYE, np.float64)
    scene.camera = Camera(CHESS["width"], CHESS["height"], position=eye,
                          direction=(d / np.linalg.norm(d)).astype(np.float32))
    return scene, bounces


def pixel_rays(scene, rays):
    h, w = scene.camera.viewport_height, scene.camera.viewport_width
    q = np.zeros((h * w, 6), np.float32)
    q[:, :3] = np.asarray(scene.camera.position, np.float32)
    q[:, 3:] = rays["direction"].reshape(h * w, 3)
    return q


def traced_ids(r, scene, rays):
    """(kind, index) of ``trace_rays`` on the pixel rays, (0, 0) on a miss: what the ID plane holds."""
    hits = r.trace_rays(pixel_rays(scene, rays))
    ids = np.stack([hits["kind"], np.where(hits["kind"] != 0, hits["index"], 0)], axis=-1).astype(np.uint32)
    return ids.reshape(r.height, r.width, 2)


def largest_piece(ids, exclude=()):
    """The chess piece (objects 1..32: 0 and 33 are the room and the board) with the most pixels."""
    idx = ids[..., 1][ids[..., 0] == 2]
    counts = np.bincount(idx, minlength=34)[:33]
    counts[0] = 0
    for e in exclude:
        counts[e] = 0
    assert counts.max() > 0
    return int(counts.argmax())


# ---------------------------------------------------------------------------- 1. the ID plane
def id_scene(name):
    if name == "c3_chess":
        scene, _ = build_config("c3_chess", **CHESS)
    elif name == "c1_37x21":
        scene, _ = build_config("c1_four_spheres", width=37, height=21)
    else:  # the scene of the golden case of that name
        case = CASES[name]
        scene, _ = build_config(case["config"], width=case["width"], height=case["height"])
    return scene


@pytest.mark.parametrize("device_rays", [False, True])
@pytest.mark.parametrize("name", ["c3_chess", "c2_64x36_b8", "c1_37x21"])
def test_id_plane_is_kind_and_index_of_trace_rays(gpu, name, device_rays):
    scene = id_scene(name)
    rays = scene.camera.recalculate_ray_directions()
    with Renderer(scene, camera_rays=rays, device_rays=device_rays) as r:
        feats = {k: v.copy() for k, v in r.features().items()}
        ids = r.feature_ids()
        want = traced_ids(r, scene, rays)
        assert ids.dtype == np.uint32 and ids.shape == (r.height, r.width, 2)
        assert np.array_equal(ids, want)
        assert (ids[..., 0] == 0).any() or name == "c3_chess"
        assert ((ids[..., 0] != 0) == (feats["hit"] != 0)).all()
        assert (ids[ids[..., 0] == 0] == 0).all()
        assert r.feature_ids_device()
        again = r.features()  # planes A and B are what they were
        assert all(np.array_equal(bits(feats[k]), bits(again[k])) for k in feats)
        # after an update_scene: the spheres move, and on the chess scene a piece does
        scene.spheres["position"][:, 0] += np.float32(0.4)
        if name == "c3_chess":
            apply_edit(scene.objects[largest_piece(ids)], MAIN_EDIT)
        r.update_scene()
        ids2 = r.feature_ids()
        assert np.array_equal(ids2, traced_ids(r, scene, rays))
        assert not np.array_equal(ids2, ids)


# ---------------------------------------------------------------------------- 2. the sequence
_FEATURES = {}


class Pair:
    """A renderer on the chess scene and the restatement, driven together. The restatement's features
    come from the CPU oracle on the host-rebuilt scene, its ids from trace_rays."""

    def __init__(self, scene=None, bounces=None, **kw):
        from oracle import oracle as O

        O.build()
        self.O = O
        if scene is None:
            scene, bounces = chess_scene()
        self.scene, self.bounces = scene, bounces
        self.rays = scene.camera.recalculate_ray_directions()
        self.r = Renderer(scene, accumulate=True, compute_per_frame=1, camera_rays=self.rays, **kw)
        self.ref = TM.TemporalMotionRef()
        self.generation = 0
        self.totals = dict.fromkeys(T.COUNTERS + T.EDGE_COUNTERS + TM.MOTION_COUNTERS, 0)
        self._feats = None
        self.snap = motion.snapshot(scene)  # the states at the previous temporal call

    def frames(self, n):
        for _ in range(n):
            self.r.compute_frame(self.bounces)

    def update_scene(self, device):
        self.r.update_scene(device=device)
        if device:  # the host records follow: the oracle and the next snapshot see the edited scene
            for o in self.scene.objects:
                builder.update_object(o)
        self.generation += 1
        self._feats = None

    def update_camera(self, cam):
        self.r.update_camera(cam)
        self.rays = cam.recalculate_ray_directions()
        self.generation += 1
        self._feats = None

    def reset(self):
        self.r.reset_accumulation()
        self.generation += 1

    def inputs(self):
        """(oracle features, traced ids) of the scene as it is; the features are computed once per
        scene state and shared between the tests, never modified."""
        if self._feats is None:
            s = self.scene
            key = b"".join(np.ascontiguousarray(a).tobytes() for a in (
                motion.snapshot(s)["objects"], s.spheres, s.materials, s.flatten()[0], s.camera.position,
                self.rays["direction"]))
            if key not in _FEATURES:
                _FEATURES[key] = R.oracle_features(self.O, s, camera_rays=self.rays)
            self._feats = (_FEATURES[key], traced_ids(self.r, s, self.rays))
        return self._feats

    def records(self):
        """The helper's records of everything that moved since the previous temporal call."""
        now = motion.snapshot(self.scene)
        return (motion.object_motion(self.snap["objects"], now["objects"]),
                motion.sphere_motion(self.snap["spheres"], now["spheres"]))

    def check(self, objects=None, spheres=None, plain=False, **params):
        """One temporal call against the restatement: all four results, bit for bit."""
        r, cam = self.r, self.scene.camera
        feats, ids = self.inputs()
        acc = r.read_accumulation()
        dirs = self.rays["direction"].reshape(r.height, r.width, 3)
        if plain:
            f, u = r.denoise_temporal(cam.world_to_pixel(), **params)
            want = self.ref.call(acc, feats, cam.position, dirs, r.accumulation_index, 1, self.generation,
                                 cam.world_to_pixel(), **params)
        else:
            f, u = r.denoise_temporal_motion(cam.world_to_pixel(), objects=objects, spheres=spheres, **params)
            want = self.ref.call_motion(acc, feats, ids, cam.position, dirs, r.accumulation_index, 1, self.generation,
                                        cam.world_to_pixel(), objects=objects, spheres=spheres, **params)
        out, n = r.read_temporal()
        for key, v in want["counters"].items():
            self.totals[key] += v
        for what, got, exp in (("history", n, want["n_out"]), ("blend", out, want["out"]), ("filtered", f, want["f"])):
            bad = np.argwhere(bits(got) != bits(exp))
            assert bad.size == 0, (what, self.generation, params, bad[:5], got[tuple(bad[0])], exp[tuple(bad[0])])
        assert np.array_equal(u, want["u"]), (self.generation, params)
        return want


def run_sequence(p):
    """The five steps; returns the per-step counters."""
    s, steps = p.scene, []
    # 1. no history
    p.frames(1)
    steps.append(p.check()["counters"])
    assert steps[-1]["no_previous"] == p.r.width * p.r.height
    # 2. the piece with the most pixels moves, rebuilt on the host
    ids = p.inputs()[1]
    main = largest_piece(ids)
    apply_edit(s.objects[main], MAIN_EDIT)
    p.update_scene(device=False)
    p.frames(1)
    objs, sph = p.records()
    assert objs["flags"][main] == motion.MOVED and objs["flags"].sum() == motion.MOVED and not sph["flags"].any()
    steps.append(p.check(objects=objs, spheres=sph)["counters"])
    p.snap = motion.snapshot(s)
    second = largest_piece(p.inputs()[1], exclude=(main,))
    # 3. the camera, another piece (rebuilt on the device) and a sphere move; two calls in one generation
    p.update_camera(moved_camera(s.camera, **CAMERA_MOVE))
    apply_edit(s.objects[second], SECOND_EDIT)
    s.spheres["position"][0] += np.asarray(SPHERE_MOVE, np.float32)
    p.update_scene(device=True)
    objs, sph = p.records()
    assert objs["flags"][second] == motion.MOVED and sph["flags"][0] == motion.MOVED
    p.frames(1)
    steps.append(p.check(objects=objs, spheres=sph, iterations=0, max_history=3, sigma_position=0.1,
                         normal_min=0.5)["counters"])
    p.frames(2)
    steps.append(p.check(objects=objs, spheres=sph, iterations=2, max_history=5, sigma_position=0.05,
                         normal_min=0.7)["counters"])
    p.snap = motion.snapshot(s)
    # 4. a material edit, marked DROP
    s.objects[main].object_info["material_index"] = (int(s.objects[main].object_info["material_index"]) + 3) % 18
    p.update_scene(device=False)
    p.frames(1)
    objs, sph = p.records()
    assert not objs["flags"].any()
    objs["flags"][main] = motion.DROP
    steps.append(p.check(objects=objs, spheres=sph, max_history=2)["counters"])
    assert steps[-1]["dropped"] == int((p.inputs()[1][..., 1][p.inputs()[1][..., 0] == 2] == main).sum()) > 0
    # 5. a plain call writes a slot without ids; the next motion call skips the id test
    p.reset()
    p.frames(1)
    steps.append(p.check(plain=True)["counters"])
    p.reset()
    p.frames(1)
    steps.append(p.check(sigma_position=0.1)["counters"])
    assert steps[-1]["ids_absent"] == p.r.width * p.r.height and steps[-2].get("ids_absent") is None
    assert all(c["ids_absent"] == 0 for c in steps[1:5])
    return steps


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("device_rays", [False, True])
def test_sequence_matches_the_restatement(gpu, device_rays, lds):
    """No history; a piece translated, rotated and scaled on the host; camera, a second piece (on the
    device) and a sphere moved with two calls in one generation and non-default parameters; a
    material edit marked DROP; a plain call, then a motion call without ids to test. Every counter
    of the restatement is non-zero over the sequence."""
    p = Pair(device_rays=device_rays, tuning={"denoise_lds": lds})
    with p.r:
        run_sequence(p)
    assert all(p.totals[key] > 0 for key in T.COUNTERS + T.EDGE_COUNTERS + TM.MOTION_COUNTERS), p.totals


# ---------------------------------------------------------------------------- 3. spheres and edges
def test_spheres_edges_and_a_short_table(gpu):
    """c1_four_spheres 37x21 (no multiple of the tile): one sphere moves, the camera yaws so that taps
    fall off both edges, and the sphere table is shorter than the sphere count -- an index beyond
    it is static."""
    scene, bounces = build_config("c1_four_spheres", width=37, height=21)
    p = Pair(scene, bounces)
    with p.r:
        p.frames(1)
        p.check()
        before = motion.snapshot(scene)
        scene.spheres["position"][1] += np.asarray((0.25, 0.1, 0.0), np.float32)
        p.update_scene(device=False)
        p.update_camera(moved_camera(scene.camera, right=0.3, up=0.2, forward=0.0, yaw=9.0, pitch=-5.0))
        p.frames(2)
        sph = motion.sphere_motion(before["spheres"], scene.spheres)
        assert sph["flags"][1] == motion.MOVED and sph.shape[0] == scene.spheres.shape[0] > 2
        short = sph[:2].copy()
        ids = p.inputs()[1]
        assert ((ids[..., 0] == 1) & (ids[..., 1] >= 2)).any() and ((ids[..., 0] == 1) & (ids[..., 1] == 1)).any()
        c = p.check(spheres=short, sigma_position=0.1)["counters"]
        assert c["moved_found"] > 0 and c["static_found"] > 0
        # beyond the table is static: the same call with the whole (static beyond 1) table gives the same bits
        got = [bits(x).copy() for x in p.r.read_temporal()]
        p.r.denoise_temporal_motion(scene.camera.world_to_pixel(), spheres=sph, sigma_position=0.1)
        assert all(np.array_equal(a, bits(b)) for a, b in zip(got, p.r.read_temporal()))
    assert all(p.totals[key] > 0 for key in T.EDGE_COUNTERS), p.totals


# ---------------------------------------------------------------------------- 4. what it is for
def test_motion_keeps_history_on_the_moved_piece(gpu):
    """The edit of step 2 on two fresh renderers: on the moved piece's pixels the motion call keeps
    history (n_out > N) on strictly more pixels than plain rt_denoise_temporal, and on at least one."""
    kept = {}
    for with_motion in (True, False):
        scene, bounces = chess_scene()
        rays = scene.camera.recalculate_ray_directions()
        with Renderer(scene, accumulate=True, compute_per_frame=1, camera_rays=rays) as r:
            m = scene.camera.world_to_pixel()
            r.compute_frame(bounces)
            if with_motion:
                r.denoise_temporal_motion(m)
            else:
                r.denoise_temporal(m)
            before = motion.snapshot(scene)
            main = largest_piece(r.feature_ids())
            apply_edit(scene.objects[main], MAIN_EDIT)
            r.update_scene(device=False)
            r.compute_frame(bounces)
            if with_motion:
                r.denoise_temporal_motion(m, objects=motion.object_motion(before["objects"],
                                                                         motion.snapshot(scene)["objects"]))
            else:
                r.denoise_temporal(m)
            ids = r.feature_ids()
            on_piece = (ids[..., 0] == 2) & (ids[..., 1] == main)
            n = r.read_temporal()[1]
            assert on_piece.any()
            kept[with_motion] = int((n[on_piece] > 1).sum())
    print("pixels of the moved piece that kept history: motion", kept[True], "plain", kept[False])
    assert kept[True] > kept[False] and kept[True] >= 1


# ---------------------------------------------------------------------------- 5. errors
def test_invalid_calls_leave_the_history_intact(gpu):
    def invalid(fn, *a, **kw):
        with pytest.raises(RtError) as e:
            fn(*a, **kw)
        assert e.value.code == N.RT_E_INVALID

    scene, bounces = build_config("c1_four_spheres", width=37, height=21)
    lib = N.load_library()
    with Renderer(scene, accumulate=True, compute_per_frame=1) as r:
        m = scene.camera.world_to_pixel()
        call = r.denoise_temporal_motion
        invalid(call, m)                                        # no frame since the reset
        r.compute_frame(bounces)
        call(m)
        held = [bits(x).copy() for x in r.read_temporal()]
        r.reset_accumulation()
        invalid(call, m)                                        # k - 1 == 0 again
        r.compute_frame(bounces)
        t = N.rt_temporal_params()
        lib.rt_temporal_default_params(t)
        t.world_to_pixel[:] = [float(v) for v in m.reshape(16)]
        rec = motion.static(2)
        assert lib.rt_denoise_temporal_motion(r._ctx, t, None, None, 2, None, 0) == N.RT_E_INVALID   # NULL, count > 0
        assert lib.rt_denoise_temporal_motion(r._ctx, t, None, None, 0, None, 1) == N.RT_E_INVALID
        assert lib.rt_denoise_temporal_motion(r._ctx, None, None, None, 0, None, 0) == N.RT_E_INVALID  # no matrix
        for flags in (4, 8, 1 << 31, motion.MOVED | 4):
            bad = rec.copy()
            bad["flags"][1] = flags
            invalid(call, m, objects=bad)
            invalid(call, m, spheres=bad)
        for value in (float("inf"), float("-inf"), float("nan")):
            for slot in (0, 7, 11):
                bad = rec.copy()
                bad["flags"][1] = motion.MOVED
                bad["m"][1, slot] = value
                invalid(call, m, spheres=bad)
            bad = rec.copy()
            bad["flags"][0] = motion.MOVED | motion.DROP
            bad["normal_scale"][0] = value
            invalid(call, m, objects=bad)
        ok = rec.copy()                                          # not finite, but not MOVED: ignored
        ok["m"][0, 3] = np.nan
        ok["flags"][1] = motion.DROP
        for value in (float("inf"), float("nan")):               # the old errors through the new entry point
            mm = m.copy().reshape(16)
            mm[5] = value
            invalid(call, mm)
        for kw in (dict(max_history=0), dict(max_history=65537), dict(sigma_position=0.0),
                   dict(sigma_position=float("nan")), dict(normal_min=1.5), dict(normal_min=float("nan")),
                   dict(iterations=9), dict(sigma_color=0.0), dict(sigma_albedo=float("nan")), dict(sigma_depth=0.0)):
            invalid(call, m, **kw)
        assert [bits(x).tolist() for x in r.read_temporal()] == [h.tolist() for h in held]
        call(m, spheres=ok)                                      # the context is usable; history was intact
        assert (r.read_temporal()[1] > 1).any()
    with Renderer(scene, rank=1, world_size=2) as rk:             # a rank context
        rk.compute_frame(bounces)
        invalid(rk.denoise_temporal_motion, m)
        rk.read_output()
    with Renderer(scene, accumulate=False) as na:                 # Params.accumulate == 0
        na.compute_frame(bounces)
        invalid(na.denoise_temporal_motion, m)


# ---------------------------------------------------------------------------- 6. no side effects
@pytest.mark.parametrize("batch", [None, 1, 4])
def test_motion_calls_do_not_disturb_a_render(gpu, batch):
    """The same frames, edits and camera moves with and without interleaved motion calls:
    accumulation, output, k, the ray count and a plain rt_denoise are the same bits. With
    frame_batch = 4 a frame is queued when the call is made: it is an observation point."""
    def drive(temporal):
        scene, bounces = build_config("c2_rtiow", width=64, height=36)
        with Renderer(scene, accumulate=True, compute_per_frame=1, frame_batch=batch) as r:
            m = scene.camera.world_to_pixel()
            r.compute_frame(bounces)
            if temporal:
                if batch == 4:
                    assert r.frame_batch() == (4, 1)
                before = motion.snapshot(scene)
                r.denoise_temporal_motion(m)
                state = r.ray_count(), r.accumulation_index, r.frame_batch(), r.tile_schedule_state()[0].tobytes()
                r.denoise_temporal_motion(m, iterations=0)
                assert state == (r.ray_count(), r.accumulation_index, r.frame_batch(),
                                 r.tile_schedule_state()[0].tobytes())
                assert r.frame_batch()[1] == 0
            r.compute_frame(bounces)
            mid = r.read_accumulation()
            scene.spheres["position"][1] += np.asarray((0.2, 0.0, 0.1), np.float32)
            r.update_scene()
            r.compute_frame(bounces)
            r.compute_frame(bounces)
            if temporal:
                r.denoise_temporal_motion(m, spheres=motion.sphere_motion(before["spheres"], scene.spheres),
                                          iterations=1)
                assert (r.read_temporal()[1] > 2).any()
            r.compute_frame(bounces)
            if temporal:
                r.denoise_temporal_motion(m, spheres=motion.sphere_motion(before["spheres"], scene.spheres))
            plain_f, plain_u = r.denoise()
            return mid, r.read_accumulation(), r.read_output(), r.accumulation_index, r.ray_count(), plain_f, plain_u

    a, b = drive(True), drive(False)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
        else:
            assert x == y
    assert a[1].any()
