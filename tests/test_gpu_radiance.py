"""Radiance queries (rt_radiance, rt_radiance_device) against the CPU oracle, bit for bit.

The reference of a ray (o, stream, d) is the oracle's own per_pixel: an ``Oracle`` whose ray
buffer holds d at index ``stream`` and whose camera origin is o renders pixel ``stream`` from a
zeroed accumulation with accumulate = 1, compute_per_frame = samples and accumulation_index =
first_sample; the accumulation row it returns is the expected radiance and its ray count the
ray's segments. All comparisons are on the u32 bit patterns of the four floats.

Rays: the secondary rays the oracle logs while rendering the scene (``logged_rays`` of
tests/test_gpu_query.py: real bounce origins on surfaces, every third direction rescaled) plus a
few camera rays. Streams are a fixed permutation of 0..n-1 that is not the identity (a kernel
that seeded with the ray's position would fail) and, being a permutation, holds 0 (seed 0 is
pixel 0's stream in the reference). Against vacuous inputs each test asserts, on the oracle's
output, that at least 25% of its rays take two or more segments per sample and at least 90%
return non-zero light (the oracle gives 34-41% and >= 99.7% on these scenes). Runs whose loop
limit is 1 admit one segment per sample, and on scenes without emitters no light: the two
conditions are asserted on the runs with the case's bounces, over the same rays.
References are computed once per (scene, count, run) and shared.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.test_gpu_query import logged_rays

pytestmark = pytest.mark.gpu

GOLDEN = {"c1": "c1_64x48_b4", "c2": "c2_64x36_b8", "c3": "c3_64x36_b8"}
N_CAMERA = 48  # camera rays per set; the rest are logged secondary rays


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- rays and references
@functools.lru_cache(maxsize=None)
def golden_scene(key):
    name = GOLDEN[key]
    g = load(name)
    return g, CASES[name], scene_from_inputs(g)


def oracle_radiance(O, scene, rays, streams, bounces, first_sample, samples):
    """(radiance (n, 4), segments (n,)) of the oracle: per ray, pixel ``stream`` of an oracle whose
    ray buffer holds the ray's direction there and whose camera origin is the ray's origin."""
    n = rays.shape[0]
    buf = np.zeros(int(streams.max()) + 1 if n else 1, B.RAY)
    buf["direction"][streams] = rays[:, 3:]
    o = O.Oracle(scene, camera_rays=buf)
    origin = o._arrays["origin"]  # the array the oracle's scene record points to
    p = scene.params(accumulate=1, compute_per_frame=samples, accumulation_index=first_sample)
    want = np.zeros((n, 4), np.float32)
    segs = np.zeros(n, np.int64)
    camera_origin = origin.copy()  # (the array may be the scene's own camera position)
    try:
        for j in range(n):
            origin[:] = rays[j, :3]
            acc, _, cnt = o.render_pixels(p, bounces, [int(streams[j])], threads=1)
            want[j] = acc[0]
            segs[j] = cnt
    finally:
        origin[:] = camera_origin
    return want, segs


def assert_not_vacuous(want, segs, samples):
    n = want.shape[0]
    assert 4 * int((segs >= 2 * samples).sum()) >= n, (int((segs >= 2 * samples).sum()), n)
    assert 10 * int(bits(want).any(axis=1).sum()) >= 9 * n, (int(bits(want).any(axis=1).sum()), n)


@functools.lru_cache(maxsize=None)
def ray_set(key, n):
    """``n`` rays of the golden scene ``key`` and their streams (never modified). The first ray
    is one that bounces under stream 0 with the case's settings, so that the one-ray batch of the
    wave-edge test is not a path that escapes at once."""
    from oracle import oracle as O

    O.build()
    g, case, scene = golden_scene(key)
    d = g["camera_rays"].astype(B.RAY)["direction"]
    cam = np.zeros((N_CAMERA, 6), np.float32)
    cam[:, :3] = np.asarray(g["camera_origin"], np.float32)
    cam[:, 3:] = d[np.linspace(0, d.shape[0] - 1, N_CAMERA).astype(np.int64)]
    rays = np.concatenate([cam, logged_rays(O, scene, case["bounces"], n - N_CAMERA, stride=1 if key == "c1" else 3)])
    rays = rays[np.random.default_rng(21).permutation(n)]
    zero = np.zeros(1, np.uint32)
    for j in range(n):
        w, s = oracle_radiance(O, scene, rays[j:j + 1], zero, case["bounces"], 1, 1)
        if s[0] >= 2 and bits(w).any():
            rays[[0, j]] = rays[[j, 0]]
            break
    else:
        raise AssertionError("no ray of the set bounces under stream 0")
    rays.setflags(write=False)
    return rays


def streams_for(count):
    s = np.random.default_rng(100 + count).permutation(count).astype(np.uint32)
    assert (s == 0).any() and (count == 1 or (s != np.arange(count)).any())
    return s


@functools.lru_cache(maxsize=None)
def reference(key, count, bounces, first_sample, samples, total=None):
    """(rays, streams, expected radiance, expected segments per ray) for the first ``count`` rays
    of the scene's set of ``total`` rays, computed once and shared (never modified)."""
    from oracle import oracle as O

    O.build()
    _, _, scene = golden_scene(key)
    rays = ray_set(key, total or count)[:count]
    streams = streams_for(count)
    want, segs = oracle_radiance(O, scene, rays, streams, bounces, first_sample, samples)
    for a in (streams, want, segs):
        a.setflags(write=False)
    return rays, streams, want, segs


def renderer(key, **kw):
    g, case, scene = golden_scene(key)
    return Renderer(scene, accumulate=True, compute_per_frame=case["spp"], camera_rays=g["camera_rays"].astype(B.RAY),
                    **kw)


def check(got, segments, want, segs):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])
    assert segments == int(segs.sum()), (segments, int(segs.sum()))


# ---------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("count", [1, 63, 64, 65, 777])
def test_c1_wave_edges(gpu, oracle_lib, count):
    """Sphere-only instance; counts at the wave edges, the refill and the tail: prefixes of one
    set of 777 rays, each count with its own permutation of streams."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    rays, streams, want, segs = reference("c1", count, bounces, 1, 1, total=777)
    assert_not_vacuous(want, segs, 1)
    with renderer("c1") as r:
        got, n = r.radiance(rays, streams, bounces=bounces, first_sample=1, samples=1, return_segments=True)
    check(got, n, want, segs)


def runs_of(key):
    bounces = CASES[GOLDEN[key]]["bounces"]
    return [(bounces, 1, 1), (bounces, 7, 4), (1, 3, 2)]


@pytest.mark.parametrize("mode", [0, 1])
def test_c2_sphere_bvh(gpu, oracle_lib, mode):
    """Sphere BVH plus the brute-force set, 1x1 textures (the staged texel of shade<true>), in
    both placements: the oracle's bits, so the same bits in both."""
    with renderer("c2", tuning={"query_lds_mode": mode}) as r:
        for bounces, first, samples in runs_of("c2"):
            rays, streams, want, segs = reference("c2", 384, bounces, first, samples)
            if bounces > 1:
                assert_not_vacuous(want, segs, samples)
            got, n = r.radiance(rays, streams, bounces=bounces, first_sample=first, samples=samples,
                                return_segments=True)
            check(got, n, want, segs)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles_textures_environment(gpu, oracle_lib, mode):
    """Triangles, non-1x1 textures and the environment map, in the three placements (the
    LDS-resident triangle walk and the global-memory walks): the oracle's bits in each."""
    _, _, scene = golden_scene("c3")
    assert scene.texture_size != (1, 1)
    with renderer("c3", tuning={"query_lds_mode": mode}) as r:
        for bounces, first, samples in runs_of("c3"):
            rays, streams, want, segs = reference("c3", 384, bounces, first, samples)
            if bounces > 1:
                assert_not_vacuous(want, segs, samples)
            got, n = r.radiance(rays, streams, bounces=bounces, first_sample=first, samples=samples,
                                return_segments=True)
            check(got, n, want, segs)


# ---------------------------------------------------------------------------- against the frame path
@pytest.mark.parametrize("name", ["c1_64x48_b4", "c1_40x24_b10_spp5"])
def test_identity_with_the_frame_path(gpu, name):
    """One frame from a zeroed accumulation equals the radiance query of the frame's own rays
    (camera origin, camera_rays[i], stream = i, first_sample = 1, samples = compute_per_frame),
    pixel for pixel, pixel 0 included; the segments equal the frame's ray count."""
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    cam = g["camera_rays"].astype(B.RAY)
    n = cam.shape[0]
    rays = np.zeros(n, B.RADIANCE_RAY)
    rays["origin"] = np.asarray(g["camera_origin"], np.float32)
    rays["direction"] = cam["direction"]
    rays["stream"] = np.arange(n, dtype=np.uint32)
    with Renderer(scene, accumulate=True, compute_per_frame=case["spp"], camera_rays=cam) as r:
        r.reset_accumulation()
        r.compute_frame(case["bounces"])
        acc, frame_rays = r.read_accumulation().reshape(n, 4), r.ray_count()
        got, segments = r.radiance(rays, bounces=case["bounces"], first_sample=1, samples=case["spp"],
                                   return_segments=True)
        # the default streams of an (n, 6) array are the positions: the same query
        plain = np.concatenate([rays["origin"], rays["direction"]], axis=1)
        again = r.radiance(plain, bounces=case["bounces"], first_sample=1, samples=case["spp"])
    assert bits(acc).any()
    bad = np.nonzero((bits(got) != bits(acc)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], acc[bad[:3]])
    assert np.array_equal(bits(got[0]), bits(acc[0]))
    assert segments == frame_rays
    assert again.tobytes() == got.tobytes()


# ---------------------------------------------------------------------------- semantics
def test_zero_bounces_and_errors(gpu):
    rays, streams, _, _ = reference("c1", 65, CASES[GOLDEN["c1"]]["bounces"], 1, 1, total=777)
    with renderer("c1") as r:
        got, n = r.radiance(rays, streams, bounces=0, samples=3, return_segments=True)
        assert got.shape == (65, 4) and not bits(got).any() and n == 0
        with pytest.raises(RtError) as e:
            r.radiance(rays, streams, samples=0)
        assert e.value.code == N.RT_E_INVALID
        lib, ctx = r._lib, r._ctx
        q = np.zeros(4, B.RADIANCE_RAY)
        q["direction"] = (0.0, 0.0, -1.0)
        out = np.zeros((4, 4), np.float32)
        seg = ctypes.c_uint64(5)
        assert lib.rt_radiance(ctx, None, N.ptr(out), 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_radiance(ctx, N.ptr(q), None, 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_radiance(ctx, N.ptr(q), N.ptr(out), 4, 4, 1, 0, None) == N.RT_E_INVALID
        assert lib.rt_radiance(ctx, None, None, 0, 4, 1, 1, ctypes.byref(seg)) == N.RT_OK
        assert seg.value == 0
        assert lib.rt_radiance(ctx, N.ptr(q), N.ptr(out), 4, 4, 1, 1, None) == N.RT_OK  # segments may be NULL
        assert lib.rt_radiance_device(ctx, None, None, 0, 4, 1, 1, None) == N.RT_OK
        assert lib.rt_radiance_device(ctx, None, None, 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_radiance_device(ctx, None, None, 4, 4, 1, 0, None) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_radiance_device(ctx, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(out.ctypes.data), 4, 4, 1, 1,
                                      None) == N.RT_E_INVALID
        assert r.radiance(np.zeros((0, 6), np.float32)).shape == (0, 4)


def test_chunking_and_device_entry_point(gpu):
    """777 rays staged in chunks of 100, in one chunk, and through the device entry point give
    the same bits and the same segment total; the row after the last result is not written."""
    import torch

    bounces = CASES[GOLDEN["c1"]]["bounces"]
    rays, streams, want, segs = reference("c1", 777, bounces, 1, 1, total=777)
    q = np.zeros(777, B.RADIANCE_RAY)
    q["origin"], q["direction"], q["stream"] = rays[:, :3], rays[:, 3:], streams
    with renderer("c1", tuning={"query_chunk": 100}) as r:
        chunked, n_chunked = r.radiance(q, bounces=bounces, return_segments=True)
        r.set_tuning("query_chunk", 65536)
        base, n_base = r.radiance(q, bounces=bounces, return_segments=True)
        t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(gpu)
        dev, n_dev = r.radiance(t, bounces=bounces, return_segments=True)
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (777, 4)
        dev_host = dev.cpu().numpy()
        # the caller's buffer with one row to spare, and a counter that is added to
        room = torch.full((778, 4), -7.25, dtype=torch.float32, device=gpu)
        counter = torch.full((1,), 1000, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize(gpu)
        r._call("rt_radiance_device", ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(room.data_ptr()), 777, bounces,
                1, 1, ctypes.c_void_p(counter.data_ptr()))
        r.synchronize()
        room_host, counted = room.cpu().numpy(), int(counter.item())
    check(base, n_base, want, segs)
    assert chunked.tobytes() == base.tobytes() and n_chunked == n_base
    assert dev_host.tobytes() == base.tobytes() and n_dev == n_base
    assert room_host[:777].tobytes() == base.tobytes()
    assert np.array_equal(bits(room_host[777]), bits(np.full(4, -7.25, np.float32)))
    assert counted == 1000 + n_base


@pytest.mark.parametrize("batch", [None, 1])
def test_radiance_does_not_disturb_a_render(gpu, batch):
    """The golden case c2_64x36_b8 with a 100-ray radiance query between the compute_frame calls,
    with the default frame queue and with one launch per frame: accumulation, output, k and ray
    count equal the golden's, and a queued frame stays queued."""
    g, case, scene = golden_scene("c2")
    rays = ray_set("c2", 384)[:100]
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                got = r.radiance(rays, bounces=case["bounces"], samples=2)
                assert (r.frame_batch(), r.accumulation_index) == before
                if batch is None:
                    assert before[0][1] == i + 1  # the frames so far are still queued
        k = r.accumulation_index
        acc, out, n = r.read_accumulation(), r.read_output(), r.ray_count()
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
        k_plain = r.accumulation_index
    assert got.shape == (100, 4) and bits(got).any()
    assert k == k_plain
    assert n == int(g["rays"])
    assert np.array_equal(out, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_sees_the_scene_as_of_the_call(gpu, oracle_lib):
    """After rt_update_materials (one material's emission_power) and rt_upload_textures (one
    layer's colour) the radiance equals the oracle's on the edited scene and differs from the
    earlier result."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    rays, streams, want, segs = reference("c1", 384, bounces, 1, 1, total=777)
    _, _, scene = golden_scene("c1")
    materials = np.ascontiguousarray(scene.materials.copy())
    textures = np.ascontiguousarray(np.array(scene.textures, np.uint8))
    lit = int(np.argmin(materials["emission_power"]))  # a material that does not emit yet
    materials["emission_power"][lit] = np.float32(2.5)
    layer = int(materials["texture_index"][(lit + 1) % materials.shape[0]])
    textures[layer, ..., :3] = (200, 40, 90)
    edited = dataclasses.replace(scene, materials=materials, textures=textures)
    edited.flatten = scene.flatten
    with renderer("c1") as r:
        before, n_before = r.radiance(rays, streams, bounces=bounces, return_segments=True)
        check(before, n_before, want, segs)
        r.scene = edited
        r._call("rt_update_materials", N.ptr(materials), materials.shape[0])
        r._upload_textures()
        after, n_after = r.radiance(rays, streams, bounces=bounces, return_segments=True)
    want2, segs2 = oracle_radiance(oracle_lib, edited, rays, streams, bounces, 1, 1)
    check(after, n_after, want2, segs2)
    assert after.tobytes() != before.tobytes()


def test_rank_context(gpu):
    """A rank context (world_size 2, rank 1) returns the bits of a full context."""
    bounces = CASES[GOLDEN["c3"]]["bounces"]
    rays, streams, want, segs = reference("c3", 384, bounces, 7, 4)
    with renderer("c3", rank=1, world_size=2) as r:
        got, n = r.radiance(rays, streams, bounces=bounces, first_sample=7, samples=4, return_segments=True)
    check(got, n, want, segs)
