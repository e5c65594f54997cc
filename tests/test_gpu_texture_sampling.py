"""Texture and env-map sampling on the GPU at non-square, odd, one-wide and clamped sizes.

Inputs are those of tests/texel_probe_scene.py: coded arrays (every texel its own 32-bit value),
the two census scenes with their closed-form texel per ray, and the probe scenes whose
sensitivity to a wrong fetch the CPU suite asserts (tests/test_texture_sampling_cpu.py). Everything
is bit-exact, against the closed form and against the CPU oracle on the same inputs: accumulation
bits, RGBA8 and ray count (``assert_same``), radiance bits and segments (``check``). Frames are
48x32 or smaller, ray sets under 2,000 rays; oracle references are computed once per input and
shared, never modified.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd.scene import build_config
from tests import denoise_ref as R
from tests import gather_ref as G
from tests import texel_probe_scene as T
from tests.test_gpu_denoise import assert_features_equal
from tests.test_gpu_parity import assert_same, gpu_render, oracle_frames
from tests.test_gpu_query import logged_rays, oracle_records
from tests.test_gpu_radiance import check, oracle_radiance
from tests.test_texture_sampling_cpu import CENSUS_CASES, CENSUS_IDS, bits, census, probe, probe_id

pytestmark = pytest.mark.gpu

FRAME_PAR = N.RT_PASS_PATH | N.RT_PASS_RESOLVE | N.RT_PASS_PATH_FRAME_PAR
GENERIC_BATCH = N.RT_PASS_PATH | N.RT_PASS_RESOLVE


def path_bits(r):
    return r.last_launch_pass_mask() & ~N.RT_PASS_PRIMARY


# ---------------------------------------------------------------------------- census, ray queries
@functools.lru_cache(maxsize=None)
def census_oracle(kind, shape, layer):
    from oracle import oracle as O

    O.build()
    c, _ = census(kind, shape, layer)
    n = c.rays.shape[0]
    return oracle_radiance(O, c.scene, c.rays, np.arange(n, dtype=np.uint32), 1, 1, 1)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape,layer", CENSUS_CASES, ids=CENSUS_IDS)
@pytest.mark.parametrize("kind", ["floor", "sphere"])
def test_census_radiance(gpu, oracle_lib, kind, shape, layer, mode):
    """Renderer.radiance with bounces 1: every ray returns its closed-form texel, and the oracle's
    bits; one segment per ray."""
    c, want = census(kind, shape, layer)
    assert c.rays.shape[0] < 2000
    with Renderer(c.scene, tuning={"query_lds_mode": mode}) as r:
        got, segments = r.radiance(c.rays, bounces=1, first_sample=1, samples=1, return_segments=True)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], c.coords[bad[:5]], got[bad[:3]], want[bad[:3]])
    check(got, segments, *census_oracle(kind, shape, layer))
    assert segments == c.rays.shape[0]


FRAME_MODES = {
    "lds_mode_0": dict(tuning={"lds_mode": 0}),
    "lds_mode_2": dict(tuning={"lds_mode": 2}),
    "primary_pass": dict(tuning={"primary_pass": 1}),
    "brute_force_1": dict(brute=1),
    "brute_force_2": dict(brute=2),
}


@pytest.mark.parametrize("shape", T.CENSUS_SHAPES, ids=probe_id)
@pytest.mark.parametrize("mode", sorted(FRAME_MODES))
def test_floor_census_frame(gpu, mode, shape):
    """The floor census as camera rays, bounces 1, one frame: without accumulation (the packed
    image of the clamped layer L) and as the first accumulated frame (the accumulation's bits, layer
    0), each equal to the closed form."""
    opts = FRAME_MODES[mode]
    for accumulate, layer in ((False, shape[0]), (True, 0)):
        c, want = census("floor", shape, layer)
        scene, rays = T.floor_frame(c)
        want = want[np.arange(rays.shape[0]) % want.shape[0]]
        with Renderer(scene, accumulate=accumulate, camera_rays=rays, tuning=opts.get("tuning")) as r:
            if "brute" in opts:
                r.set_brute_force(opts["brute"])
            r.compute_frame(1)
            acc, out, n = r.read_accumulation().reshape(-1, 4), r.read_output().reshape(-1), r.ray_count()
            passes = r.last_launch_passes()
        assert n == rays.shape[0]
        assert np.array_equal(out, R.pack_rgba8(want)), np.nonzero(out != R.pack_rgba8(want))[0][:5]
        if accumulate:
            bad = np.nonzero((bits(acc) != bits(want)).any(axis=1))[0]
            assert bad.size == 0, (bad[:5], acc[bad[:3]], want[bad[:3]])
        if "brute" in opts:
            assert "brute" in passes
        if mode == "primary_pass":
            assert "primary" in passes


# ---------------------------------------------------------------------------- full paths
def run_frames(scene, rays, frames=T.PROBE_FRAMES, *, expect=None, brute=None, spp=1, **kw):
    with Renderer(scene, camera_rays=rays, compute_per_frame=spp, **kw) as r:
        if brute is not None:
            r.set_brute_force(brute)
        for _ in range(frames):
            r.compute_frame(T.PROBE_BOUNCES)
        r.synchronize()
        if expect is not None:
            assert path_bits(r) == expect, (hex(path_bits(r)), hex(expect))
        got = r.read_accumulation(), r.read_output(), r.ray_count()
        if kw.get("tuning", {}).get("primary_pass") == 1:
            assert r.last_launch_pass_mask() & N.RT_PASS_PRIMARY
        return got


LAUNCHES = {
    "default": dict(),
    "lds_mode_0": dict(tuning={"lds_mode": 0}),
    "lds_mode_1": dict(tuning={"lds_mode": 1}),
    "lds_mode_2": dict(tuning={"lds_mode": 2}),
    "frame_par_instance": dict(frame_batch=2, expect=FRAME_PAR),
    "generic_instance_batch": dict(frame_batch=2, tuning={"frame_par_instance": 0}, expect=GENERIC_BATCH),
    "frame_batch_1": dict(frame_batch=1),
    "primary_pass": dict(tuning={"primary_pass": 1}),
    "brute_force_1": dict(brute=1),
    "brute_force_2": dict(brute=2),
    "compute_per_frame_2": dict(spp=2),
}

S, TR = (T.SPHERE_SEED, False), (T.TRI_SEED, True)
# (launch, (seed, with_tris), texture shape index, env shape index): every launch kind meets both
# texture orientations (but compute_per_frame 2, run once); every env shape meets the default launch
# and the frame-parallel instance
PATH_CASES = [("default", TR if j % 2 else S, j % 2, j) for j in range(5)]
PATH_CASES += [("frame_par_instance", S if j % 2 else TR, (j + 1) % 2, j) for j in range(5)]
PATH_CASES += [
    ("lds_mode_0", TR, 0, 1), ("lds_mode_0", TR, 1, 0),
    ("lds_mode_1", S, 0, 2), ("lds_mode_1", TR, 1, 2),
    ("lds_mode_2", TR, 0, 3), ("lds_mode_2", S, 1, 3),
    ("generic_instance_batch", S, 0, 4), ("generic_instance_batch", TR, 1, 4),
    ("frame_batch_1", S, 0, 0), ("frame_batch_1", S, 1, 1),
    ("primary_pass", TR, 0, 0), ("primary_pass", TR, 1, 1),
    ("brute_force_1", TR, 0, 1), ("brute_force_1", TR, 1, 2),
    ("brute_force_2", TR, 0, 3), ("brute_force_2", TR, 1, 4),
    ("compute_per_frame_2", TR, 0, 0),
]


def probe_input(kind, tex_i, env_j):
    key = (*kind, T.TEX_SHAPES[tex_i], T.ENV_SHAPES[env_j])
    assert key in T.PROBE_INPUTS, key  # the CPU suite's sensitivity guard covers it
    return key


@pytest.mark.parametrize("launch,kind,tex_i,env_j", PATH_CASES,
                         ids=["%s-%s-tex%s-env%s" % (c[0], "tris" if c[1][1] else "spheres",
                                                      probe_id(T.TEX_SHAPES[c[2]]), probe_id(T.ENV_SHAPES[c[3]]))
                              for c in PATH_CASES])
def test_full_paths(gpu, launch, kind, tex_i, env_j):
    """6 bounces, 2 accumulated frames of a probe scene under one launch kind: the oracle's bits."""
    opts = dict(LAUNCHES[launch])
    scene, rays, ref = probe(*probe_input(kind, tex_i, env_j), spp=opts.get("spp", 1))
    assert_same(*run_frames(scene, rays, **opts), *ref)


def test_launch_table_is_complete():
    for launch in LAUNCHES:
        mine = [c for c in PATH_CASES if c[0] == launch]
        assert {c[2] for c in mine} == ({0} if launch == "compute_per_frame_2" else {0, 1}), launch
    for launch in ("default", "frame_par_instance"):
        assert {c[3] for c in PATH_CASES if c[0] == launch} == set(range(len(T.ENV_SHAPES)))


# ---------------------------------------------------------------------------- env shortcut
@pytest.mark.parametrize("eh,ew", [(9, 5), (5, 9)])
@pytest.mark.parametrize("kind", ["cols_uniform", "rows_uniform", "both_uniform", "one_texel_off"])
def test_env_map_uniform_rows_columns_odd_sizes(gpu, oracle_lib, kind, eh, ew):
    """test_gpu_env_map_uniform_rows_columns' kinds on 9x5 and 5x9 maps (rt_upload_env_map's
    detection and sample_env's skipped coordinate); the 1xN and Nx1 maps of test_full_paths make
    the detection loops run zero times on one axis."""
    scene, bounces = build_config("c2_rtiow", width=48, height=32)
    rng = np.random.default_rng(11)
    if kind == "cols_uniform":
        env = np.broadcast_to(rng.integers(0, 256, (1, ew, 4), dtype=np.uint8), (eh, ew, 4))
    elif kind in ("rows_uniform", "one_texel_off"):
        env = np.broadcast_to(rng.integers(0, 256, (eh, 1, 4), dtype=np.uint8), (eh, ew, 4))
    else:
        env = np.broadcast_to(np.array([40, 90, 200, 255], np.uint8), (eh, ew, 4))
    env = np.ascontiguousarray(env)
    if kind == "one_texel_off":
        env[eh // 2, ew // 3, 0] ^= 0x40
    scene.environment_map = env
    acc_o, out_o, rays_o = oracle_lib.render_frames(scene, bounces, 2)
    assert_same(*gpu_render(scene, bounces, 2), acc_o, out_o, rays_o)


# ---------------------------------------------------------------------------- params != upload
MISMATCH = TR + ((3, 3, 7), (5, 9))  # W = 7, H = 3; env 9 x 5
PARAM_SIZES = {
    "texture_2w_2h": dict(texture_width=14, texture_height=6),
    "texture_w-2_1": dict(texture_width=5, texture_height=1),
    "texture_0_negative": dict(texture_width=0, texture_height=0x80000003),
    "env_2w_2h": dict(env_map_width=18, env_map_height=10),
    "env_w-2_1": dict(env_map_width=7, env_map_height=1),
    "env_0_negative": dict(env_map_width=0, env_map_height=0x80000003),
}


@functools.lru_cache(maxsize=None)
def mismatch_reference(sizes):
    from oracle import oracle as O

    O.build()
    scene, rays, _ = probe(*MISMATCH)
    o = O.Oracle(scene, camera_rays=rays)
    acc = np.zeros((o.height, o.width, 4), np.float32)
    out = np.zeros((o.height, o.width), np.uint32)
    n = 0
    for k in range(1, T.PROBE_FRAMES + 1):
        n += o.render_frame(mismatch_params(scene, sizes, k), T.PROBE_BOUNCES, acc, out)
    return acc, out, n


def mismatch_params(scene, sizes, k):
    p = scene.params(accumulation_index=k)
    for name, value in PARAM_SIZES[sizes].items():
        p[name] = value
    return p


@pytest.mark.parametrize("call", ["rt_update_params", "rt_reset_accumulation"])
@pytest.mark.parametrize("sizes", sorted(PARAM_SIZES))
def test_params_disagree_with_upload(gpu, sizes, call):
    """rt_params' texture / env sizes (the factors of u and v) differ from the uploaded sizes (the
    clamps): the oracle's bits with the same rt_params. Every index is clamped by the uploaded
    sizes (texel_coord, fetch_texture's layer clamp), so these are values, not memory safety."""
    scene, rays, plain = probe(*MISMATCH)
    ref = mismatch_reference(sizes)
    assert not np.array_equal(bits(ref[0]), bits(plain[0]))
    with Renderer(scene, camera_rays=rays) as r:
        p = N.params_struct(mismatch_params(scene, sizes, 1))
        r._call(call, ctypes.byref(p))
        for _ in range(T.PROBE_FRAMES):
            r.compute_frame(T.PROBE_BOUNCES)
        assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), *ref)


# ---------------------------------------------------------------------------- one context
@pytest.mark.parametrize("batch", [1, None])
def test_one_context_changing_shapes(gpu, batch):
    """rt_upload_textures on a live context: 1x1 layers (the staged texel of shade<true>, uv
    skipped), 7 wide, 7 high with the same texel count (the buffer is kept, only the sizes change)
    and 1x1 again, each step's 2 frames against the oracle."""
    base = (T.TRI_SEED, True)
    scene0, rays, _ = probe(*base, (3, 3, 7), (5, 9))
    with Renderer(scene0, camera_rays=rays, frame_batch=batch) as r:
        for shape in [(4, 1, 1), (3, 3, 7), (3, 7, 3), (4, 1, 1)]:
            scene = dataclasses.replace(scene0, textures=T.coded_textures(*shape))
            _, _, ref = shape_reference(shape)
            r.scene = scene
            r._upload_textures()
            r.reset_accumulation()
            r.reset_ray_count()
            for _ in range(T.PROBE_FRAMES):
                r.compute_frame(T.PROBE_BOUNCES)
            assert_same(r.read_accumulation(), r.read_output(), r.ray_count(), *ref)


@functools.lru_cache(maxsize=None)
def shape_reference(shape):
    from oracle import oracle as O

    O.build()
    scene0, rays, _ = probe(T.TRI_SEED, True, (3, 3, 7), (5, 9))
    scene = dataclasses.replace(scene0, textures=T.coded_textures(*shape))
    return scene, rays, oracle_frames(O, scene, T.PROBE_BOUNCES, T.PROBE_FRAMES, rays)


# ---------------------------------------------------------------------------- queries
N_QUERY = 500


@functools.lru_cache(maxsize=None)
def radiance_reference():
    from oracle import oracle as O

    O.build()
    scene, cam, _ = probe(*MISMATCH)
    rays = logged_rays(O, scene, T.PROBE_BOUNCES, N_QUERY)
    streams = np.random.default_rng(5).permutation(N_QUERY).astype(np.uint32)
    want, segs = oracle_radiance(O, scene, rays, streams, T.PROBE_BOUNCES, 2, 2)
    assert 4 * int((segs >= 4).sum()) >= N_QUERY and 10 * int(bits(want).any(axis=1).sum()) >= 9 * N_QUERY
    return scene, cam, rays, streams, want, segs


@pytest.mark.parametrize("mode", [0, 2])
def test_radiance_on_the_probe_scene(gpu, mode):
    scene, cam, rays, streams, want, segs = radiance_reference()
    with Renderer(scene, camera_rays=cam, tuning={"query_lds_mode": mode}) as r:
        got, n = r.radiance(rays, streams, bounces=T.PROBE_BOUNCES, first_sample=2, samples=2, return_segments=True)
    check(got, n, want, segs)


@functools.lru_cache(maxsize=None)
def gather_reference():
    from oracle import oracle as O

    O.build()
    scene, cam, _ = probe(*MISMATCH)
    count, samples = N_QUERY // 4, 4
    points = G.first_hit_points(O, scene, cam, scene.camera.position, count)
    streams = (1 + np.random.default_rng(6).permutation(count)).astype(np.uint32)
    lights, segs = G.oracle_lights(O, scene, points, streams, T.PROBE_BOUNCES, 1, samples)
    return scene, cam, points, streams, samples, G.tree(lights), segs


@pytest.mark.parametrize("mode", [0, 2])
def test_gather_on_the_probe_scene(gpu, mode):
    scene, cam, points, streams, samples, want, segs = gather_reference()
    assert 10 * int(bits(want).any(axis=1).sum()) >= 9 * points.shape[0]
    with Renderer(scene, camera_rays=cam, tuning={"query_lds_mode": mode}) as r:
        got, n = r.gather(points, streams, bounces=T.PROBE_BOUNCES, first_sample=1, samples=samples,
                          return_segments=True)
    check(got, n, want, segs)


def test_features_on_the_probe_scene(gpu, oracle_lib):
    """Albedo, normal and depth planes at 48x28: hits on the flat quads (NaN and infinite uv), the
    clamped layers and the coded env map, through rt_feature_resolve_kernel's fetch."""
    scene, rays = T.probe_scene(T.TRI_SEED, 48, 28, (3, 7, 3), (9, 5), with_tris=True)
    want = R.oracle_features(oracle_lib, scene, camera_rays=rays)
    hit = want["hit"] == 1
    for part in (hit, ~hit):  # many texels of the textures and of the env map
        assert np.unique(want["albedo"][part], axis=0).shape[0] > 10
    with Renderer(scene, camera_rays=rays) as r:
        assert_features_equal(r.features(), want)


def flat_quad_rays(scene, n=12):
    """Rays onto the two flat quads: an n x n grid of oblique unit rays from 37.3 away to each
    (the hit lies an ulp or so off the plane: +-inf), and an n x n grid of axis-parallel rays
    from 2 away to each (the hit lies exactly in the plane: 0 / 0)."""
    cam = np.asarray(scene.camera.position, np.float64)
    g = (np.arange(n) + 0.37) / n * 3.6 - 1.8
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g))
    zero = np.zeros_like(a)
    on_z = cam + np.stack([a, b, zero - 3], axis=1)  # points of the quad in the plane z = cam.z - 3
    on_x = cam + np.stack([zero + 3, a, b], axis=1)
    rays = []
    for target, normal in ((on_z, (0, 0, 1)), (on_x, (-1, 0, 0))):
        d = target - cam
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays.append(np.concatenate([target - 37.3 * d, d], axis=1))
        start = target.astype(np.float32).astype(np.float64) + 2 * np.array(normal, np.float64)
        rays.append(np.concatenate([start, np.broadcast_to(-np.array(normal, np.float64), target.shape)], axis=1))
    return np.ascontiguousarray(np.concatenate(rays), np.float32)


def test_trace_rays_on_flat_objects(gpu, oracle_lib):
    """rt_trace_rays returns the uv of hits on objects whose bounds are flat in z or x: the oracle's
    bits, NaN payloads and the signs of the infinities included."""
    scene, cam, _ = probe(*MISMATCH)
    rays = flat_quad_rays(scene)
    ref = oracle_records(oracle_lib, scene, rays)["rec"]
    for f in ("u", "v"):
        assert np.isnan(ref[f]).any() and np.isposinf(ref[f]).any() and np.isneginf(ref[f]).any(), f
    with Renderer(scene, camera_rays=cam) as r:
        hits = r.trace_rays(rays)
    n = rays.shape[0]
    got, want = hits.view(np.uint8).reshape(n, 64)[:, :44], ref.view(np.uint8).reshape(n, 64)[:, :44]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], hits[bad[:3]], ref[bad[:3]])
