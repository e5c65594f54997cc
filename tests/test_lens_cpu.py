"""Lens queries without a GPU: the ABI surface (rt_lens_camera, the four entry points), the three
copies of the contract, the NumPy restatement (tests/lens_ref.py) against the host camera, the
geometry of the thin lens and of the panorama, and the cameras the GPU tests use.

No kernel launches here; tests/test_gpu_lens.py compares the kernels with the restatement.
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.camera import Camera, lens_camera
from tests import lens_ref as L
from tests.golden.fixtures import CASES, load, scene_from_inputs

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
KERNELS = ROOT / "rust_gpu_raytracing_amd" / "csrc" / "radiance.hip"
FUNCTIONS = ("rt_lens", "rt_lens_device", "rt_lens_rays", "rt_lens_rays_device")
FIELDS = ("inverse_projection", "inverse_view", "origin", "aspect", "kind", "width", "height", "stream_base",
          "aperture", "focus", "ortho_half_height", "_pad")
GOLDEN = {"c2": "c2_64x36_b8", "c3": "c3_64x36_b8"}
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- ABI
def test_functions_declared_exported_and_bound(native_lib):
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", HEADER.read_text(), re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in FUNCTIONS:
        assert name in declared
        assert name in exported
        assert name in N.SIGNATURES
        assert hasattr(native_lib, name)
    assert native_lib.rt_abi_version() == 12
    assert "12, additive: lens queries" in HEADER.read_text()


def test_header_compiles_as_c_and_layout_matches(tmp_path):
    """The header compiles as C11; sizeof(rt_lens_camera) == 176 and every field's offset in a C
    program equals the ctypes structure's and the numpy dtype's."""
    src = tmp_path / "off.c"
    offsets = ", ".join(f"offsetof(rt_lens_camera, {f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt} %u %u %u\\n", sizeof(rt_lens_camera), {offsets}, '
                   'RT_LENS_PERSPECTIVE, RT_LENS_ORTHOGRAPHIC, RT_LENS_EQUIRECT); return 0;}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[0] == 176 == ctypes.sizeof(N.rt_lens_camera) == B.LENS_CAMERA.itemsize
    assert got[1:-3] == [getattr(N.rt_lens_camera, f).offset for f in FIELDS]
    assert got[1:-3] == [B.LENS_CAMERA.fields[f][1] for f in FIELDS]
    assert tuple(f for f, _ in N.rt_lens_camera._fields_) == B.LENS_CAMERA.names == FIELDS
    assert got[-3:] == [0, 1, 2] == [B.LENS_PERSPECTIVE, B.LENS_ORTHOGRAPHIC, B.LENS_EQUIRECT]
    assert got[-3:] == [N.RT_LENS_PERSPECTIVE, N.RT_LENS_ORTHOGRAPHIC, N.RT_LENS_EQUIRECT]


def test_null_context_fails_cleanly(native_lib):
    cam = lens_camera(Camera(4, 2))
    out = np.full((8, 4), 3.5, np.float32)
    rays = np.zeros(8, B.RADIANCE_RAY)
    seg = ctypes.c_uint64(9)
    p = ctypes.c_void_p(cam.ctypes.data)
    assert native_lib.rt_lens(None, p, 0, 8, N.ptr(out), 4, 1, 1, ctypes.byref(seg)) == N.RT_E_INVALID
    assert native_lib.rt_lens_device(None, p, 0, 8, None, 4, 1, 1, None) == N.RT_E_INVALID
    assert native_lib.rt_lens_rays(None, p, 0, 8, 1, N.ptr(rays)) == N.RT_E_INVALID
    assert native_lib.rt_lens_rays_device(None, p, 0, 8, 1, None) == N.RT_E_INVALID
    assert (out == 3.5).all() and seg.value == 9


def _contract(path, lead):
    """The lens contract of ``path`` with the comment leader ``lead`` stripped."""
    lines = path.read_text().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith(lead + " THE LENS CONTRACT."))
    last = next(i for i, l in enumerate(lines) if l.startswith(lead + " End of the lens contract."))
    assert all(l.startswith(lead) for l in lines[first:last + 1])
    return [l[len(lead):].rstrip() for l in lines[first:last + 1]]


def test_contract_text_is_in_header_kernel_source_and_restatement():
    """The contract in include/rt_abi.h equals the header comment of radiance.hip and the docstring
    of tests/lens_ref.py line for line, and the lines the restatement is written from are there."""
    in_header, in_kernels = _contract(HEADER, " *"), _contract(KERNELS, "//")
    in_ref = _contract(Path(L.__file__), "")
    assert in_header == in_kernels == in_ref
    assert len(in_header) == 30
    text = "\n".join(in_header)
    for line in ["stream = stream_base + i (u32, wrapping) and sample index u:",
                 "xc = f32(x)/f32(width), yc = f32(y)/f32(height).",
                 "nx = xc*2.0f - 1.0f, ny = yc*2.0f - 1.0f, ax = nx*aspect.",
                 "((c0*x + c1*y) + c2*z) + c3*w per component",
                 "ws = normalize(t.xyz / t.w) with normalize(v) = v * (1.0f / sqrt((x*x + y*y) + z*z)).",
                 "If aperture == 0: o = origin, d = (V^-1 * (ws, 0)).xyz: the very bits of camera_ray.",
                 "lseed = (stream * u * 326624u) ^ 0x85EBCA6Bu (u32, wrapping).",
                 "r1 = random(&lseed), r2 = random(&lseed), in that order",
                 "rad = aperture * sqrt(r1), th = 6.2831850051879883f * r2.",
                 "lx = rad * cos(th), ly = rad * cos(th - 1.5707963705062866f).",
                 "k = focus / (0.0f - ws.z), f = ws * k.",
                 "dv = normalize((f.x - lx, f.y - ly, f.z)), d = (V^-1 * (dv, 0)).xyz.",
                 "o = origin + (V^-1 * (lx, ly, 0, 0)).xyz.",
                 "o = origin + (V^-1 * (ax*ortho_half_height, ny*ortho_half_height, 0, 0)).xyz.",
                 "d = (V^-1 * (0, 0, -1, 0)).xyz.",
                 "uc = (f32(x) + 0.5f)/f32(width), vc = (f32(y) + 0.5f)/f32(height).",
                 "az = (uc - 0.5f) * (2.0f*WGSL_PI), el = (vc - 0.5f) * WGSL_PI, ce = cos(el), with",
                 "d = (ce*cos(az), cos(el - 1.5707963705062866f), ce*cos(az - 1.5707963705062866f)). o = origin.",
                 "R = R + L_s per channel. radiance[i] = R."]:
        assert line in text, line


# ---------------------------------------------------------------------------- the restatement
def tilted(width, height, position=(1.5, -2.0, 7.0)):
    """A camera that looks neither along an axis nor level: every entry of V^-1's rotation matters."""
    d = np.array([0.3, 0.5, -0.8])
    return Camera(width, height, position=np.array(position, f32), direction=(d / np.linalg.norm(d)).astype(f32))


@pytest.mark.parametrize("size", [(37, 21), (64, 36)])
def test_pinhole_equals_the_host_camera(oracle_lib, size):
    """PERSPECTIVE with aperture 0 is Camera.recalculate_ray_directions bit for bit, for the default
    camera and a tilted one; the origin is the camera's and the streams count from stream_base."""
    for camera in (Camera(*size), tilted(*size)):
        want = camera.recalculate_ray_directions()["direction"]
        cam = lens_camera(camera, stream_base=5)
        got = L.rays(cam, 0, size[0] * size[1], 9)
        assert np.array_equal(bits(got["direction"]), bits(want))
        assert np.array_equal(bits(got["origin"]), bits(np.broadcast_to(camera.position, want.shape)))
        assert np.array_equal(got["stream"], 5 + np.arange(size[0] * size[1], dtype=np.uint32))
        assert not bits(got["_pad1"]).any()


def _thin(camera, **kw):
    return lens_camera(camera, "perspective", aperture=0.3, focus=20.0, stream_base=1, **kw)


def test_lens_rays_pass_through_the_focus_point(oracle_lib):
    """Every lens ray of a pixel passes through origin + V^-1 * (f, 0), to 1e-4 of the focus distance
    (f32 rounding is some 1e-7 of it; an axis or sign mistake is of the order of the aperture, 0.3),
    and leaves the lens within the aperture, off its centre."""
    camera = tilted(37, 21)
    cam = _thin(camera)
    for pixel in (0, 36, 388, 500, 776):
        p = L.focus_point(cam, pixel)
        for u in range(1, 9):
            o, _, d = L.ray(cam, pixel, u)
            o, d = o.astype(np.float64), d.astype(np.float64)
            dist = np.linalg.norm(np.cross(p - o, d)) / np.linalg.norm(d)
            assert dist <= 1e-4 * 20.0, (pixel, u, dist)
            assert (p - o) @ d > 0  # ahead of the lens, not behind it
            off = o - camera.position.astype(np.float64)
            assert 1e-3 < np.linalg.norm(off) <= 0.3 * (1 + 1e-6)
            assert abs(off @ camera.direction.astype(np.float64)) <= 1e-6  # in the lens plane


def test_lens_rays_differ_from_the_pinhole(oracle_lib):
    """On at least 90% of (pixel, sample) pairs the thin-lens ray differs from the pinhole's in origin
    and direction; stream 0 repeats its lens point (consequence 4) and other streams do not."""
    camera = tilted(37, 21)
    cam, pin = _thin(camera), lens_camera(camera, stream_base=1)
    differ = total = 0
    for pixel in range(0, 777, 7):
        _, _, d0 = L.ray(pin, pixel, 1)
        for u in (1, 2, 3):
            o, _, d = L.ray(cam, pixel, u)
            differ += int(bits(d).tobytes() != bits(d0).tobytes() and bits(o).tobytes() != bits(camera.position).tobytes())
            total += 1
    assert 10 * differ >= 9 * total, (differ, total)
    zero = _thin(camera)
    zero["stream_base"] = 0
    assert L.lens_point(zero, 0, 1) == L.lens_point(zero, 0, 2)
    assert L.lens_point(cam, 1, 1) != L.lens_point(cam, 1, 2)


def test_orthographic_rays_are_parallel_and_span_the_view_volume(oracle_lib):
    camera = tilted(16, 9)
    cam = lens_camera(camera, "orthographic", ortho_half_height=4.0, stream_base=1)
    rec = L.rays(cam, 0, 144, 1)
    assert (bits(rec["direction"]) == bits(rec["direction"][0])).all()
    assert np.abs(rec["direction"][0].astype(np.float64) - camera.direction).max() < 1e-6
    off = rec["origin"].astype(np.float64) - camera.position
    assert np.abs(off @ camera.direction.astype(np.float64)).max() < 1e-5
    # pixel (0, 0) is the corner (-aspect * h, -h) of the view volume: |offset|^2 = h^2 (aspect^2 + 1)
    assert abs(np.linalg.norm(off[0]) - 4.0 * np.hypot(16 / 9, 1.0)) < 1e-4


@pytest.mark.parametrize("size", [(16, 8), (37, 21)])
def test_equirect_round_trip(oracle_lib, size):
    """environment_map_coords (oracle/pathtrace_oracle.c:458-459, :291-292) of every pixel's direction
    lands in texel (x, y) of a map of the image's size: the panorama uploads as an environment map."""
    w, h = size
    lib = oracle_lib.lib()
    cam = lens_camera(Camera(w, h), "equirect", stream_base=1)
    rec = L.rays(cam, 0, w * h, 1)
    assert np.abs(np.linalg.norm(rec["direction"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(bits(rec["origin"]), bits(np.broadcast_to(cam["origin"], (w * h, 3))))
    for i, d in enumerate(rec["direction"]):
        u = f32(f32(0.5) + f32(f32(lib.oracle_atan2f(float(d[2]), float(d[0]))) / f32(f32(2.0) * L.WGSL_PI)))
        v = f32(f32(0.5) + f32(f32(lib.oracle_asinf(float(d[1]))) / L.WGSL_PI))
        x, y = int(f32(u * f32(w))), int(f32(v * f32(h)))
        assert (x, y) == (i % w, i // w), (i, x, y, u, v)


def test_lens_camera_builder():
    camera = tilted(64, 36)
    cam = lens_camera(camera, "orthographic", ortho_half_height=2.5, width=16, height=9, stream_base=7)
    assert cam.dtype == B.LENS_CAMERA and cam.shape == ()
    assert (int(cam["kind"]), int(cam["width"]), int(cam["height"]), int(cam["stream_base"])) == (1, 16, 9, 7)
    assert cam["aspect"] == f32(16) / f32(9) and cam["ortho_half_height"] == f32(2.5)
    assert np.array_equal(cam["inverse_view"].reshape(4, 4), camera.inverse_view)
    assert np.array_equal(cam["inverse_projection"].reshape(4, 4), camera.inverse_projection)
    assert np.array_equal(cam["origin"], camera.position)
    assert int(lens_camera(camera, B.LENS_EQUIRECT)["kind"]) == 2
    frame = lens_camera(camera)  # the camera's own frame: consequence 1's descriptor
    assert (int(frame["width"]), int(frame["height"]), int(frame["stream_base"]), float(frame["aperture"])) == (64, 36, 0, 0.0)
    with pytest.raises(KeyError):
        lens_camera(camera, "fisheye")


# ---------------------------------------------------------------------------- the GPU tests' cameras
@functools.lru_cache(maxsize=None)
def golden_scene(key):
    g = load(GOLDEN[key])
    return g, CASES[GOLDEN[key]], scene_from_inputs(g)


def lens_cases(key):
    """kind -> (descriptor, first pixel) of the 24-pixel ranges tests/test_gpu_lens.py runs against
    the oracle on the golden scene ``key``: a 16x9 image at the scene's camera position, tilted
    towards the ground; the ranges start where the thin lens and the panorama see both sky and
    surfaces (the orthographic view of c3 sees surfaces only)."""
    _, _, scene = golden_scene(key)
    d = np.array([0.2, 0.35, -0.9])
    camera = Camera(16, 9, position=scene.camera.position.copy(), direction=(d / np.linalg.norm(d)).astype(f32))
    return {"thin": (lens_camera(camera, "perspective", aperture=0.3, focus=20.0, stream_base=7), 24),
            "orthographic": (lens_camera(camera, "orthographic", ortho_half_height=4.0, stream_base=7), 104),
            "equirect": (lens_camera(camera, "equirect", stream_base=7), 72)}


FIRST_SAMPLE, SAMPLES, RANGE = 5, 3, 24


@functools.lru_cache(maxsize=None)
def lens_reference(key, kind):
    """(descriptor, first pixel, expected radiance (24, 4), expected segments (24,), per-path lights,
    per-path segments) from the oracle, computed once and shared (never modified)."""
    from oracle import oracle as O
    from tests.test_gpu_radiance import oracle_radiance

    O.build()
    _, case, scene = golden_scene(key)
    cam, first = lens_cases(key)[kind]
    out = L.oracle_lens(oracle_radiance, O, scene, cam, first, RANGE, case["bounces"], FIRST_SAMPLE, SAMPLES)
    for a in out:
        a.setflags(write=False)
    return (cam, first) + out


def assert_not_vacuous(lights, segs):
    """At least 25% of the paths take two or more segments and at least 90% return non-zero light."""
    n = segs.size
    two = int((segs >= 2).sum())
    lit = int(bits(lights).reshape(n, 4).any(axis=1).sum())
    print(f"{two}/{n} paths of two or more segments, {lit}/{n} with light")
    assert 4 * two >= n, (two, n)
    assert 10 * lit >= 9 * n, (lit, n)


@pytest.mark.parametrize("kind", ["thin", "orthographic", "equirect"])
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_gpu_test_cameras_are_not_vacuous(oracle_lib, key, kind):
    """The reference alone: the ranges the GPU tests compare hold enough paths that bounce and
    return light, and the sums are not the sums of one sample."""
    cam, first, want, segs, lights, path_segs = lens_reference(key, kind)
    assert_not_vacuous(lights, path_segs)
    assert want.shape == (RANGE, 4) and (segs == path_segs.sum(axis=1)).all()
    assert (bits(want) != bits(lights[:, 0])).any()
