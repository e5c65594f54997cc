"""Lens queries (rt_lens, rt_lens_device, rt_lens_rays, rt_lens_rays_device) on the GPU, bit for bit.

The pinhole descriptor of a scene's own camera is compared with the oracle's frames (consequence 1
of the contract in include/rt_abi.h); the rays of all three kinds with the NumPy restatement
(tests/lens_ref.py); the thin lens, the orthographic view and the panorama with the oracle's
per_pixel on the restatement's records, summed in sample order (tests/test_lens_cpu.py builds the
cameras and the references and checks on the CPU that they are not vacuous). All comparisons are on
the u32 bit patterns. References are computed once and shared.
"""
import ctypes
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.camera import lens_camera
from tests import lens_ref as L
from tests.test_lens_cpu import (FIRST_SAMPLE, RANGE, SAMPLES, assert_not_vacuous, bits, golden_scene, lens_cases,
                                 lens_reference, tilted)

pytestmark = pytest.mark.gpu

KINDS = ("thin", "orthographic", "equirect")


def renderer(key, **kw):
    g, case, scene = golden_scene(key)
    return Renderer(scene, accumulate=True, compute_per_frame=case["spp"], camera_rays=g["camera_rays"].astype(B.RAY),
                    **kw)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape, got.dtype)
    flat_got, flat_want = bits(got).reshape(-1, got.shape[-1]), bits(want).reshape(-1, got.shape[-1])
    bad = np.nonzero((flat_got != flat_want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], got.reshape(flat_got.shape)[bad[:3]], want.reshape(flat_got.shape)[bad[:3]])


# ---------------------------------------------------------------------------- the pinhole
@functools.lru_cache(maxsize=None)
def frame_reference(key, first_sample, samples):
    """(accumulation (h, w, 4), ray count) of the oracle for the scene's own camera from a zeroed
    buffer: accumulate = 1, compute_per_frame = samples, accumulation_index = first_sample."""
    from oracle import oracle as O

    O.build()
    _, case, scene = golden_scene(key)
    o = O.Oracle(scene)
    p = scene.params(accumulate=1, compute_per_frame=samples, accumulation_index=first_sample)
    acc, _, rays = o.render_pixels(p, case["bounces"], np.arange(o.width * o.height, dtype=np.uint32))
    acc = acc.reshape(o.height, o.width, 4)
    acc.setflags(write=False)
    return acc, rays


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_pinhole_reproduces_the_frame(gpu, oracle_lib, key, mode):
    """Consequence 1 on all 2304 pixels, in every scene placement, through the host form (in chunks
    of 1000 pixels too) and the device form; the segments are the oracle's ray count."""
    _, case, scene = golden_scene(key)
    want, rays = frame_reference(key, 3, 2)
    assert bits(want).any(axis=2).sum() * 10 >= 9 * 2304 and rays > 2 * 2304
    cam = lens_camera(scene.camera)
    with renderer(key, tuning={"query_lds_mode": mode}) as r:
        got, n = r.lens(cam, bounces=case["bounces"], first_sample=3, samples=2, return_segments=True)
        dev, n_dev = r.lens(cam, bounces=case["bounces"], first_sample=3, samples=2, device=True, return_segments=True)
        dev = dev.cpu().numpy()
        r.set_tuning("query_chunk", 1000)
        chunked, n_chunked = r.lens(cam, bounces=case["bounces"], first_sample=3, samples=2, return_segments=True)
    same(got, want)
    assert n == rays
    assert dev.tobytes() == got.tobytes() and n_dev == n
    assert chunked.tobytes() == got.tobytes() and n_chunked == n


def test_pinhole_equals_the_frames_of_the_context(gpu):
    """The same against the library's own frames, with the matrices in effect
    (rt_update_camera_matrices): two frames from accumulation_index 1 into a zeroed buffer."""
    _, case, scene = golden_scene("c3")
    with Renderer(scene, accumulate=True, compute_per_frame=1, device_rays=True) as r:
        r.reset_accumulation()
        r.compute_frame(case["bounces"])
        r.compute_frame(case["bounces"])
        acc, frames_rays = r.read_accumulation(), r.ray_count()
        got, n = r.lens(lens_camera(scene.camera), bounces=case["bounces"], first_sample=1, samples=2,
                        return_segments=True)
    assert bits(acc).any()
    same(got, acc)
    assert n == frames_rays


# ---------------------------------------------------------------------------- the rays
def ray_camera(kind, size):
    camera = tilted(*size)
    kw = {"thin": dict(kind="perspective", aperture=0.3, focus=20.0), "pinhole": dict(kind="perspective"),
          "orthographic": dict(kind="orthographic", ortho_half_height=4.0), "equirect": dict(kind="equirect")}[kind]
    return lens_camera(camera, stream_base=7, **kw)


@functools.lru_cache(maxsize=None)
def ray_reference(kind, size, u):
    out = L.rays(ray_camera(kind, size), 0, size[0] * size[1], u)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind", KINDS + ("pinhole",))
def test_lens_rays_against_the_restatement(gpu, oracle_lib, kind):
    """Images of 1x1, 64x1 and 37x21 pixels, stream_base 7; the ranges of 1, 63, 64 and 65 pixels
    from pixel 5 that the image holds, and the whole image; sample indices 1 and 2^32 - 1; host and
    device form. Every record equals the restatement's, the padding word is +0.0f, and the record
    after the range is not written."""
    import torch

    with renderer("c2") as r:
        for size in ((1, 1), (64, 1), (37, 21)):
            pixels = size[0] * size[1]
            cam = ray_camera(kind, size)
            ranges = [(5, n) for n in (1, 63, 64, 65) if 5 + n <= pixels] + [(0, pixels)]
            for u in (1, 0xFFFFFFFF):
                want = ray_reference(kind, size, u)
                for first, n in ranges:
                    got = r.lens_rays(cam, u, region=(first, n))
                    assert got.dtype == B.RADIANCE_RAY and got.shape == (n,)
                    assert got.tobytes() == want[first:first + n].tobytes(), (kind, size, u, first, n)
                dev = r.lens_rays(cam, u, device=True)
                assert tuple(dev.shape) == (size[1], size[0], 8) and dev.dtype == torch.float32
                assert dev.cpu().numpy().tobytes() == want.tobytes(), (kind, size, u)
        # one record to spare after the range
        cam = ray_camera(kind, (37, 21))
        room = torch.full((66, 8), -7.25, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize(gpu)
        r._call("rt_lens_rays_device", ctypes.c_void_p(cam.ctypes.data), 5, 65, 1, ctypes.c_void_p(room.data_ptr()))
        r.synchronize()
        room = room.cpu().numpy()
    assert room[:65].tobytes() == ray_reference(kind, (37, 21), 1)[5:70].tobytes()
    assert (room[65] == -7.25).all()
    if kind == "thin":  # the lens point follows the sample index; the other kinds do not
        assert ray_reference(kind, (37, 21), 1).tobytes() != ray_reference(kind, (37, 21), 0xFFFFFFFF).tobytes()
    else:
        assert ray_reference(kind, (37, 21), 1).tobytes() == ray_reference(kind, (37, 21), 0xFFFFFFFF).tobytes()


# ---------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_lens_against_the_oracle(gpu, oracle_lib, key, kind):
    """A 24-pixel range of a 16x9 image, samples = 3 from first_sample = 5: the sequential sum of
    the oracle's per_pixel over the restatement's records, and the oracle's segments; host form,
    device form, and the staged scene placements."""
    _, case, _ = golden_scene(key)
    cam, first, want, segs, lights, path_segs = lens_reference(key, kind)
    assert_not_vacuous(lights, path_segs)
    with renderer(key) as r:
        for mode in (-1, 1, 2):
            r.set_tuning("query_lds_mode", mode)
            got, n = r.lens(cam, bounces=case["bounces"], first_sample=FIRST_SAMPLE, samples=SAMPLES,
                            region=(first, RANGE), return_segments=True)
            same(got, want)
            assert n == int(segs.sum()), (mode, n, int(segs.sum()))
        dev, n_dev = r.lens(cam, bounces=case["bounces"], first_sample=FIRST_SAMPLE, samples=SAMPLES,
                            region=(first, RANGE), device=True, return_segments=True)
        assert dev.is_cuda and tuple(dev.shape) == (RANGE, 4)
        dev = dev.cpu().numpy()
    assert dev.tobytes() == got.tobytes() and n_dev == n


@pytest.mark.parametrize("kind", KINDS)
def test_radiance_of_the_lens_rays_is_the_lens_query(gpu, kind):
    """Consequence 2: rt_radiance on rt_lens_rays(u) with first_sample = u, samples = 1 equals
    rt_lens with the same u, over the whole 16x9 image, on the host and on the device."""
    _, case, _ = golden_scene("c3")
    cam, _ = lens_cases("c3")[kind]
    with renderer("c3") as r:
        for u in (1, 6):
            rays = r.lens_rays(cam, u)
            assert rays.shape == (9, 16)
            via_rays, n_rays = r.radiance(rays.reshape(-1), bounces=case["bounces"], first_sample=u, samples=1,
                                          return_segments=True)
            direct, n = r.lens(cam, bounces=case["bounces"], first_sample=u, samples=1, return_segments=True)
            assert bits(direct).any()
            same(direct.reshape(-1, 4), via_rays)
            assert n == n_rays
        dev_rays = r.lens_rays(cam, 6, device=True)
        dev = r.radiance(dev_rays.reshape(-1, 8), bounces=case["bounces"], first_sample=6, samples=1)
        assert dev.cpu().numpy().tobytes() == direct.tobytes()


def test_host_forms_in_chunks_equal_the_device_forms(gpu):
    """The staging of the host forms at the smallest shape at which its chunks can go wrong: a 7x5
    image, the range first_pixel = 3, count = 29 with "query_chunk" = 8 -- four chunks, the last of
    five pixels. rt_lens and rt_lens_rays equal their device forms on the range bit for bit, and
    the segments equal the device form's counter."""
    _, case, scene = golden_scene("c3")
    cam = lens_camera(scene.camera, "perspective", aperture=0.3, focus=20.0, width=7, height=5, stream_base=1)
    with renderer("c3", tuning={"query_chunk": 8}) as r:
        dev, n_dev = r.lens(cam, bounces=case["bounces"], first_sample=2, samples=3, region=(3, 29), device=True,
                            return_segments=True)
        got, n = r.lens(cam, bounces=case["bounces"], first_sample=2, samples=3, region=(3, 29), return_segments=True)
        dev_rays = r.lens_rays(cam, 2, region=(3, 29), device=True).cpu().numpy()
        rays = r.lens_rays(cam, 2, region=(3, 29))
    dev = dev.cpu().numpy()
    assert got.shape == (29, 4) and bits(got).any() and n >= 3 * 29  # (a segment per path at least)
    assert got.tobytes() == dev.tobytes() and n == n_dev
    assert rays.shape == (29,) and dev_rays.shape == (29, 8) and rays.tobytes() == dev_rays.tobytes()
    assert np.array_equal(rays["stream"], 1 + 3 + np.arange(29, dtype=np.uint32))


# ---------------------------------------------------------------------------- side effects
@pytest.mark.parametrize("batch", [None, 1])
def test_lens_does_not_disturb_a_render(gpu, batch):
    """The golden case c2_64x36_b8 with lens queries and lens rays between the compute_frame calls:
    queued frames stay queued, and the accumulation, the output, the accumulation index and the ray
    count equal the golden's."""
    import torch

    g, case, scene = golden_scene("c2")
    cam, first = lens_cases("c2")["thin"]
    room = torch.zeros((RANGE, 4), dtype=torch.float32, device=gpu)
    torch.cuda.synchronize(gpu)
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            before = r.frame_batch(), r.accumulation_index, None if batch is None else r.ray_count()
            got = r.lens(cam, bounces=case["bounces"], samples=2, region=(first, RANGE))
            r.lens_rays(cam, 3)
            # (the entry point itself: Renderer.lens(device=True) asks for the context's stream, which
            # launches the queued frames)
            r._call("rt_lens_device", ctypes.c_void_p(cam.ctypes.data), first, RANGE, ctypes.c_void_p(room.data_ptr()),
                    case["bounces"], 1, 2, None)
            assert (r.frame_batch(), r.accumulation_index, None if batch is None else r.ray_count()) == before
            if batch is None:
                assert before[0][1] == i + 1  # the frames so far are still queued
        k = r.accumulation_index
        acc, out, n = r.read_accumulation(), r.read_output(), r.ray_count()
        r.synchronize()
        assert room.cpu().numpy().tobytes() == got.tobytes()
    assert got.shape == (RANGE, 4) and bits(got).any()
    assert k == case["frames"] + 1
    assert n == int(g["rays"])
    assert np.array_equal(out, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_rank_context(gpu, oracle_lib):
    """A rank context (world_size 2, rank 1) returns the bits of a full context."""
    _, case, _ = golden_scene("c3")
    cam, first, want, segs, _, _ = lens_reference("c3", "thin")
    with renderer("c3", rank=1, world_size=2) as r:
        got, n = r.lens(cam, bounces=case["bounces"], first_sample=FIRST_SAMPLE, samples=SAMPLES, region=(first, RANGE),
                        return_segments=True)
    same(got, want)
    assert n == int(segs.sum())


# ---------------------------------------------------------------------------- semantics
def test_zero_bounces_empty_ranges_and_errors(gpu):
    import torch

    _, case, scene = golden_scene("c2")
    good, _ = lens_cases("c2")["thin"]
    ortho, _ = lens_cases("c2")["orthographic"]

    def changed(base=good, **fields):
        cam = np.array(base, copy=True)
        for name, value in fields.items():
            cam[name] = value
        return cam

    with renderer("c2") as r:
        lib, ctx = r._lib, r._ctx
        out = np.full((RANGE, 4), 3.5, np.float32)
        rays = np.zeros(RANGE, B.RADIANCE_RAY)
        seg = ctypes.c_uint64(5)
        d_out = torch.full((RANGE, 4), 3.5, dtype=torch.float32, device=gpu)
        d_rays = torch.zeros((RANGE, 8), dtype=torch.float32, device=gpu)
        d_seg = torch.zeros(2, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize(gpu)
        P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        D = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

        def every_form(cam, first=0, count=RANGE):
            """The four entry points' answers to the descriptor and the range."""
            return [lib.rt_lens(ctx, P(cam), first, count, N.ptr(out), 4, 1, 1, None),
                    lib.rt_lens_device(ctx, P(cam), first, count, D(d_out), 4, 1, 1, None),
                    lib.rt_lens_rays(ctx, P(cam), first, count, 1, N.ptr(rays)),
                    lib.rt_lens_rays_device(ctx, P(cam), first, count, 1, D(d_rays))]

        assert every_form(good) == [N.RT_OK] * 4
        # bounces == 0: zeros, no segments, RT_OK
        got, n = r.lens(good, bounces=0, samples=3, region=(0, RANGE), return_segments=True)
        assert got.shape == (RANGE, 4) and not bits(got).any() and n == 0
        dev = r.lens(good, bounces=0, samples=3, region=(0, RANGE), device=True)
        assert not bits(dev.cpu().numpy()).any()
        # samples == 0, whatever count is
        for count in (0, RANGE):
            assert lib.rt_lens(ctx, P(good), 0, count, N.ptr(out), 4, 1, 0, None) == N.RT_E_INVALID
            assert lib.rt_lens_device(ctx, P(good), 0, count, D(d_out), 4, 1, 0, None) == N.RT_E_INVALID
        assert b"samples" in lib.rt_last_error(ctx)
        # count == 0 launches nothing, whatever the pointers are
        out[:] = 3.5
        assert lib.rt_lens(ctx, None, 0, 0, None, 4, 1, 1, ctypes.byref(seg)) == N.RT_OK and seg.value == 0
        assert lib.rt_lens_device(ctx, None, 0, 0, None, 4, 1, 1, None) == N.RT_OK
        assert lib.rt_lens_rays(ctx, None, 0, 0, 1, None) == N.RT_OK
        assert lib.rt_lens_rays_device(ctx, None, 0, 0, 1, None) == N.RT_OK
        assert r.lens(good, region=(0, 0)).shape == (0, 4) and r.lens_rays(good, region=(144, 0)).shape == (0,)
        # consequence 6, descriptor and range
        invalid = [changed(kind=3), changed(kind=0xFFFFFFFF), changed(width=0), changed(height=0),
                   changed(width=65536, height=65537),
                   changed(aperture=-0.1), changed(aperture=np.inf), changed(aperture=np.nan),
                   changed(focus=0.0), changed(focus=-1.0), changed(focus=np.nan),
                   changed(ortho, ortho_half_height=0.0), changed(ortho, ortho_half_height=-2.0),
                   changed(ortho, ortho_half_height=np.nan)]
        for cam in invalid:
            assert every_form(cam) == [N.RT_E_INVALID] * 4, cam
        for first, count in ((144, 1), (121, RANGE), (0, 145), (2 ** 40, 1), (1, 2 ** 64 - 1)):
            assert every_form(good, first, count) == [N.RT_E_INVALID] * 4, (first, count)
        assert b"range" in lib.rt_last_error(ctx)
        # what one kind ignores does not make another's descriptor invalid
        assert every_form(changed(ortho, focus=0.0, aperture=0.5)) == [N.RT_OK] * 4
        assert every_form(changed(focus=0.0, aperture=0.0, ortho_half_height=-1.0)) == [N.RT_OK] * 4
        assert every_form(changed(width=65536, height=65536, aperture=0.0), 2 ** 32 - RANGE, RANGE) == [N.RT_OK] * 4
        # NULL pointers with count > 0
        assert lib.rt_lens(ctx, None, 0, RANGE, N.ptr(out), 4, 1, 1, None) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_lens(ctx, P(good), 0, RANGE, None, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_lens_device(ctx, None, 0, RANGE, D(d_out), 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE, None, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_lens_rays(ctx, None, 0, RANGE, 1, N.ptr(rays)) == N.RT_E_INVALID
        assert lib.rt_lens_rays(ctx, P(good), 0, RANGE, 1, None) == N.RT_E_INVALID
        assert lib.rt_lens_rays_device(ctx, None, 0, RANGE, 1, D(d_rays)) == N.RT_E_INVALID
        assert lib.rt_lens_rays_device(ctx, P(good), 0, RANGE, 1, None) == N.RT_E_INVALID
        # host memory is not device memory of the context's device; alignment 16, 16 and 8
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE, P(out), 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE, D(d_out), 4, 1, 1, ctypes.c_void_p(ctypes.addressof(seg))) == N.RT_E_INVALID
        assert lib.rt_lens_rays_device(ctx, P(good), 0, RANGE, 1, P(rays)) == N.RT_E_INVALID
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE - 1, D(d_out, 8), 4, 1, 1, None) == N.RT_E_INVALID
        assert b"aligned" in lib.rt_last_error(ctx)
        assert lib.rt_lens_rays_device(ctx, P(good), 0, RANGE - 1, 1, D(d_rays, 8)) == N.RT_E_INVALID
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE, D(d_out), 4, 1, 1, D(d_seg, 4)) == N.RT_E_INVALID
        # the segments of the device form are added to
        d_seg[0] = 1000
        torch.cuda.synchronize(gpu)
        assert lib.rt_lens_device(ctx, P(good), 0, RANGE, D(d_out), case["bounces"], 1, 1, D(d_seg)) == N.RT_OK
        r.synchronize()
        _, n = r.lens(good, bounces=case["bounces"], region=(0, RANGE), return_segments=True)
        assert int(d_seg[0].item()) == 1000 + n and n >= RANGE
        with pytest.raises(RtError) as e:
            r.lens(good, samples=0)
        assert e.value.code == N.RT_E_INVALID
