"""Temporal reprojection on the GPU (rt_denoise_temporal, rt_temporal_reset, rt_read_temporal).

Every comparison is bit for bit: the filtered f32 result, the packed result, rt_read_temporal's
colour and its history plane against the NumPy restatement of the contract (tests/temporal_ref.py),
fed the device's own accumulation readback and oracle-built features. The camera sequences and
their features are computed once per scene and shared, never modified.
"""
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd.camera import Camera
from rust_gpu_raytracing_amd.scene import build_config
from tests import denoise_ref as R
from tests import temporal_ref as T
from tests.golden.fixtures import CASES, load, scene_from_inputs

pytestmark = pytest.mark.gpu

SCENES = ("c2_64x36_b8", "c3_64x36_b8", "c1_37x21", "c1_150x70")
# Five camera positions: (right, up, forward) offsets from the scene's camera in its own frame and a
# yaw in degrees: translate; rotate so that part of the frame leaves the screen; move back past the
# start so that disocclusions appear; a last small move. Frames rendered at each, and the parameters
# of the temporal call(s) there: two calls (after the first and after the last frame) at position 3.
MOVES = ((0.0, 0.0, 0.0, 0.0), (0.7, 0.15, 0.0, 0.0), (0.7, 0.15, 0.0, 14.0), (-0.8, -0.1, -0.5, 0.0),
         (-0.6, 0.0, 0.4, -3.0))
FRAMES = (1, 3, 1, 3, 1)
CALLS = (({},), (dict(iterations=1),), (dict(iterations=0, max_history=2),),
         (dict(sigma_position=0.1, normal_min=0.5), {}),
         (dict(iterations=2, max_history=3, sigma_position=0.05, sigma_color=0.7),))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def base_scene(name):
    """(a fresh scene, bounces, spp) of a test scene; the scene's camera is the sequence's start."""
    if name == "c1_150x70":
        scene, bounces = build_config("c1_four_spheres", width=150, height=70)
        return scene, bounces, 1
    g = load({"c1_37x21": "c1_37x21_noacc"}.get(name, name))
    case = CASES[{"c1_37x21": "c1_37x21_noacc"}.get(name, name)]
    scene = scene_from_inputs(g)
    pos = np.asarray(g["camera_origin"], np.float32)
    if name.startswith("c2"):  # the RTIOW camera looks at the origin
        scene.camera = Camera(scene.camera.viewport_width, scene.camera.viewport_height, position=pos,
                              direction=(-pos / np.linalg.norm(pos)).astype(np.float32))
    return scene, case["bounces"], case["spp"]


def cameras(cam0):
    fwd = cam0.direction.astype(np.float64) / np.linalg.norm(cam0.direction)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    out = []
    for r, u, f, yaw in MOVES:
        a = np.radians(yaw)
        d = fwd * np.cos(a) + right * np.sin(a)
        out.append(Camera(cam0.viewport_width, cam0.viewport_height,
                          position=(cam0.position + r * right + u * up + f * fwd).astype(np.float32),
                          direction=d.astype(np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def sequence(name):
    """Per camera position: (camera, ray buffer, oracle features)."""
    from oracle import oracle as O

    O.build()
    scene, _, _ = base_scene(name)
    seq = []
    for cam in cameras(scene.camera):
        scene.camera = cam
        rays = cam.recalculate_ray_directions()
        seq.append((cam, rays, R.oracle_features(O, scene, camera_rays=rays)))
    return seq


class Pair:
    """A renderer and the restatement, driven together."""

    def __init__(self, name, **kw):
        self.seq = sequence(name)
        self.scene, self.bounces, self.spp = base_scene(name)
        self.scene.camera = self.seq[0][0]
        self.r = Renderer(self.scene, accumulate=True, compute_per_frame=self.spp, camera_rays=self.seq[0][1], **kw)
        self.ref = T.TemporalRef()
        self.generation = 0
        self.at = 0
        self.totals = dict.fromkeys(T.COUNTERS + T.EDGE_COUNTERS, 0)

    def move(self, i):
        self.r.update_camera(self.seq[i][0])  # resets the accumulation: a new generation
        self.generation += 1
        self.at = i

    def frames(self, n):
        for _ in range(n):
            self.r.compute_frame(self.bounces)

    def check(self, **params):
        """denoise_temporal(**params) against the restatement: all four results, bit for bit."""
        r, (cam, rays, feats) = self.r, self.seq[self.at]
        acc = r.read_accumulation()
        f, u = r.denoise_temporal(cam.world_to_pixel(), **params)
        out, n = r.read_temporal()
        want = self.ref.call(acc, feats, cam.position, rays["direction"].reshape(r.height, r.width, 3),
                             r.accumulation_index, self.spp, self.generation, cam.world_to_pixel(), **params)
        for key, v in want["counters"].items():
            self.totals[key] += v
        for what, got, exp in (("history", n, want["n_out"]), ("blend", out, want["out"]), ("filtered", f, want["f"])):
            bad = np.argwhere(bits(got) != bits(exp))
            assert bad.size == 0, (what, self.at, params, bad[:5], got[tuple(bad[0])], exp[tuple(bad[0])])
        assert np.array_equal(u, want["u"]), (self.at, params)
        return want

    def run(self):
        for i in range(len(MOVES)):
            if i:
                self.move(i)
            first, *rest = CALLS[i]
            if rest:
                self.frames(1)
                self.check(**first)
                self.frames(FRAMES[i] - 1)
                self.check(**rest[0])
            else:
                self.frames(FRAMES[i])
                self.check(**first)


# ---------------------------------------------------------------------------- 1. sequences
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("device_rays", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_sequence_matches_the_restatement(gpu, name, device_rays, lds):
    """Five camera positions with a reset at each, 1 or 3 frames, two calls within one generation at
    one of them; iterations 0, 1, 2 and the default; non-default max_history, sigma_position and
    normal_min; ray-buffer cameras and rt_update_camera_matrices; the step-1 and step-2 passes
    LDS-tiled and direct. Every branch of the restatement is taken, and on the frames that are no
    multiple of the 32x8 tile taps fall off both edges."""
    p = Pair(name, device_rays=device_rays, tuning={"denoise_lds": lds})
    with p.r:
        p.run()
    assert all(p.totals[key] > 0 for key in T.COUNTERS), p.totals
    if name.startswith("c1"):
        assert all(p.totals[key] > 0 for key in T.EDGE_COUNTERS), p.totals


# ---------------------------------------------------------------------------- 2. reset
def test_temporal_reset_forgets_the_history(gpu):
    def invalid(fn, *a, **kw):
        with pytest.raises(RtError) as e:
            fn(*a, **kw)
        assert e.value.code == N.RT_E_INVALID

    p = Pair("c2_64x36_b8")
    with p.r:
        invalid(p.r.read_temporal)            # before any rt_denoise_temporal
        p.r.temporal_reset()                  # RT_OK when there is no history
        p.frames(1)
        first = p.check()
        p.move(1)
        p.frames(1)
        p.check()
        assert p.totals["no_previous"] == p.r.width * p.r.height
        p.r.temporal_reset()
        p.ref.reset()
        invalid(p.r.read_temporal)
        again = p.check()                      # equals a first call at this camera: no history
        assert again["counters"]["no_previous"] == p.r.width * p.r.height
        assert (again["n_out"] == 1).all() and first["counters"]["no_previous"] > 0
        p.r.read_temporal()


# ---------------------------------------------------------------------------- 3. no side effects
@pytest.mark.parametrize("batch", [None, 1])
def test_temporal_does_not_disturb_a_render(gpu, batch):
    """The same frames and camera moves with and without interleaved temporal calls: accumulation,
    output, k, the ray count and a plain rt_denoise are the same bits."""
    def drive(temporal):
        p = Pair("c2_64x36_b8", frame_batch=batch)
        with p.r:
            r = p.r
            p.frames(1)
            if temporal:
                before = r.ray_count(), r.accumulation_index, r.frame_batch(), r.tile_schedule_state()[0].tobytes()
                p.check()
                assert before == (r.ray_count(), r.accumulation_index, r.frame_batch(),
                                  r.tile_schedule_state()[0].tobytes())
            p.frames(1)
            mid = r.read_accumulation()
            p.move(1)
            p.frames(2)
            if temporal:
                p.check(iterations=1)
            p.frames(1)
            if temporal:
                p.check()
            plain_f, plain_u = r.denoise()
            return mid, r.read_accumulation(), r.read_output(), r.accumulation_index, r.ray_count(), plain_f, plain_u

    a, b = drive(True), drive(False)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
        else:
            assert x == y
    assert a[1].any()


def test_temporal_launches_the_queued_frame(gpu):
    """frame_batch = 4 with one frame queued: rt_denoise_temporal is an observation point."""
    p = Pair("c2_64x36_b8", frame_batch=4)
    with p.r:
        p.r.compute_frame(p.bounces)
        assert p.r.frame_batch() == (4, 1)
        cam = p.seq[0][0]
        f, u = p.r.denoise_temporal(cam.world_to_pixel())
        assert p.r.frame_batch() == (4, 0) and p.r.accumulation_index == 2
        acc = p.r.read_accumulation()
        out, n = p.r.read_temporal()
        want = p.ref.call(acc, p.seq[0][2], cam.position, p.seq[0][1]["direction"].reshape(p.r.height, p.r.width, 3),
                          2, p.spp, 0, cam.world_to_pixel())
    assert acc.any()
    assert np.array_equal(bits(f), bits(want["f"])) and np.array_equal(u, want["u"])
    assert np.array_equal(bits(out), bits(want["out"])) and np.array_equal(bits(n), bits(want["n_out"]))


# ---------------------------------------------------------------------------- 4. errors
def test_invalid_calls_leave_the_context_usable_and_the_history_intact(gpu):
    p = Pair("c2_64x36_b8")
    with p.r:
        r, m = p.r, p.seq[0][0].world_to_pixel()

        def invalid(fn, *a, **kw):
            with pytest.raises(RtError) as e:
                fn(*a, **kw)
            assert e.value.code == N.RT_E_INVALID

        invalid(r.denoise_temporal, m)                               # no frame since the reset
        invalid(r.read_temporal)
        p.frames(1)
        p.check()
        held = [bits(x).copy() for x in r.read_temporal()]
        p.move(1)
        invalid(r.denoise_temporal, p.seq[1][0].world_to_pixel())     # k - 1 == 0 again
        p.frames(1)
        m = p.seq[1][0].world_to_pixel()
        lib = N.load_library()
        assert lib.rt_denoise_temporal(r._ctx, None, None) == N.RT_E_INVALID  # the matrix has no default
        for bad in (float("inf"), float("-inf"), float("nan")):
            for slot in (0, 7, 15):
                mm = m.copy().reshape(16)
                mm[slot] = bad
                invalid(r.denoise_temporal, mm)
        for bad in (0, 65537):
            invalid(r.denoise_temporal, m, max_history=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            invalid(r.denoise_temporal, m, sigma_position=bad)
        for bad in (-1.5, 1.5, float("inf"), float("nan")):
            invalid(r.denoise_temporal, m, normal_min=bad)
        invalid(r.denoise_temporal, m, iterations=9)                  # rt_denoise's own errors
        for key in ("sigma_color", "sigma_albedo", "sigma_depth"):
            for bad in (0.0, float("nan")):
                invalid(r.denoise_temporal, m, **{key: bad})
        assert [bits(x).tolist() for x in r.read_temporal()] == [h.tolist() for h in held]
        p.check(max_history=65536, normal_min=-1.0)                  # the limits are valid; history was intact
        p.check(max_history=1, normal_min=1.0)
    scene, bounces, _ = base_scene("c2_64x36_b8")
    with Renderer(scene, rank=1, world_size=2) as rk:                 # a rank context
        rk.compute_frame(bounces)
        invalid(rk.denoise_temporal, m)
        rk.read_output()
    scene, bounces, _ = base_scene("c1_37x21")                        # Params.accumulate == 0
    with Renderer(scene, accumulate=False) as na:
        na.compute_frame(bounces)
        invalid(na.denoise_temporal, scene.camera.world_to_pixel())


# ---------------------------------------------------------------------------- 5. device copy
def test_copy_denoised_to_device_serves_the_temporal_result(gpu):
    import torch

    p = Pair("c2_64x36_b8")
    with p.r:
        r = p.r
        p.frames(1)
        p.check()
        p.move(1)
        p.frames(2)
        want = p.check()
        bpr = 512  # padded rows: 256 B of image, 256 B of padding
        disp = torch.full((r.height * bpr,), 0xAB, dtype=torch.uint8, device=gpu)
        r.copy_denoised_to_device(disp.data_ptr(), bpr)
        r.synchronize()  # the copy is ordered on the renderer's stream, not torch's
        img = disp.cpu().numpy().reshape(r.height, bpr)
        f, u = r.read_denoised()
    assert np.array_equal(img[:, : 4 * r.width].copy().view(np.uint32), want["u"])
    assert np.array_equal(u, want["u"]) and np.array_equal(bits(f), bits(want["f"]))
    assert (img[:, 4 * r.width:] == 0xAB).all()
