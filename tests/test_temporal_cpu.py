"""Temporal reprojection without a GPU: the ABI surface (rt_temporal_params, the four entry points),
``Camera.world_to_pixel``, the NumPy restatement of the temporal contract (tests/temporal_ref.py)
and its quality against converged oracle renders over a moving camera.

No kernel launches here; tests/test_gpu_temporal.py compares the kernels with the restatement.
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
from rust_gpu_raytracing_amd.camera import Camera
from tests import denoise_ref as R
from tests import temporal_ref as T
from tests.golden.fixtures import CASES, load, params_for, scene_from_inputs

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
KERNELS = ROOT / "rust_gpu_raytracing_amd" / "csrc" / "denoise.hip"
FUNCTIONS = ("rt_temporal_default_params", "rt_denoise_temporal", "rt_temporal_reset", "rt_read_temporal")
PARAM_FIELDS = ("world_to_pixel", "max_history", "sigma_position", "normal_min", "_reserved")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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
    assert "12, additive: temporal denoiser" in HEADER.read_text()


def test_params_layout_against_compiled_header(tmp_path):
    """sizeof and every field offset of rt_temporal_params from a C program compiled against the
    real header equal the ctypes structure's and the numpy dtype's: 80 bytes, offsets 0, 64, 68, 72, 76."""
    args = ["sizeof(rt_temporal_params)"] + [f"offsetof(rt_temporal_params, {f})" for f in PARAM_FIELDS]
    fmt = " ".join(["%zu"] * len(args))
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [80, 0, 64, 68, 72, 76]
    assert ctypes.sizeof(N.rt_temporal_params) == B.TEMPORAL_PARAMS.itemsize == 80
    assert [getattr(N.rt_temporal_params, f).offset for f in PARAM_FIELDS] == got[1:]
    assert [B.TEMPORAL_PARAMS.fields[f][1] for f in PARAM_FIELDS] == got[1:]
    assert tuple(f for f, _ in N.rt_temporal_params._fields_) == B.TEMPORAL_PARAMS.names == PARAM_FIELDS


def test_default_params(native_lib):
    p = N.rt_temporal_params()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    assert native_lib.rt_temporal_default_params(ctypes.byref(p)) == N.RT_OK
    assert not any(p.world_to_pixel)
    assert (p.max_history, p._reserved) == (32, 0)
    for got, want in ((p.sigma_position, 0.02), (p.normal_min, 0.9)):
        assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
    assert native_lib.rt_temporal_default_params(None) == N.RT_E_INVALID
    d = T.DEFAULTS
    assert (d["max_history"], d["sigma_position"], d["normal_min"]) == (32, 0.02, 0.9)


def test_null_context_fails_cleanly(native_lib):
    buf = (ctypes.c_float * 8)()
    t = N.rt_temporal_params()
    assert native_lib.rt_denoise_temporal(None, ctypes.byref(t), None) == N.RT_E_INVALID
    assert native_lib.rt_temporal_reset(None) == N.RT_E_INVALID
    assert native_lib.rt_read_temporal(None, buf, buf) == N.RT_E_INVALID
    assert not any(buf)


def _contract(path, lead):
    """The temporal contract of ``path`` with the comment leader ``lead`` stripped."""
    lines = path.read_text().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith(lead + " THE TEMPORAL STAGE"))
    last = next(i for i, l in enumerate(lines) if l.startswith(lead + " End of the temporal contract."))
    assert all(l.startswith(lead) for l in lines[first:last + 1])
    return [l[len(lead):].rstrip() for l in lines[first:last + 1]]


def test_contract_text_is_in_kernel_source_and_header():
    """The contract in include/rt_abi.h equals the header comment of denoise.hip line for line, and
    the lines the restatement is written from are there."""
    in_header, in_kernels = _contract(HEADER, " *"), _contract(KERNELS, "//")
    assert in_header == in_kernels
    text = "\n".join(in_kernels)
    for line in ["c = accumulation(p) / D on all four channels;",
                 "Hit: X_p = o + d*t_p per component (one multiply, one add), and wv = 1.",
                 "Miss: X_p = d, and wv = 0.",
                 "For rows i = 0, 1, 3: c_i = (M[i]*X.x + M[4+i]*X.y) + M[8+i]*X.z. On a hit, c_i = c_i + M[12+i] follows.",
                 "There is no history unless c_3 > 0.",
                 "There is no history unless fx > -1 && fx < W && fy > -1 && fy < H. Every one of these tests is false for NaN.",
                 "x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0, bx = 1 - ax, by = 1 - ay.",
                 "A tap counts only if q is inside the image, w > 0, and hit_q == hit_p.",
                 "the normal: (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_min;",
                 "the position: e2 <= (sigma_position*sigma_position) * r2, with",
                 "sw = sw + w, hc = hc + w*C_q (per channel) and hn = hn + w*n_q, in tap order starting from 0.",
                 "Otherwise h = hc/sw and nh = min(hn/sw, (float)max_history).",
                 "With history: tot = nh + N, a = N/tot, out = h + (c - h)*a per channel, and n_out = tot.",
                 "k_c(p) = n_out(p) * K_i, using the centre pixel's count.",
                 "is not promised bit-equal"]:
        assert line in text, line


# ---------------------------------------------------------------------------- Camera.world_to_pixel
@pytest.mark.parametrize("size", [(37, 21), (64, 36)])
def test_world_to_pixel_inverts_the_ray_generator(size):
    """For every pixel, o + d*t for t in {0.5, 7, 300} maps to within 1e-3 px of (x, y); a point
    behind the camera gives w <= 0."""
    w, h = size
    cam = Camera(w, h, position=np.array([1.5, -2.0, 9.0], np.float32),
                 direction=np.array([0.3, -0.2, -1.0], np.float32))
    m = cam.world_to_pixel()
    assert m.dtype == np.float32 and m.shape == (4, 4)
    rows = m.astype(np.float64).T  # rows[i] . (X, 1)
    d = cam.recalculate_ray_directions()["direction"].astype(np.float64)
    o = cam.position.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for t in (0.5, 7.0, 300.0):
        X = np.concatenate([o + d * t, np.ones((w * h, 1))], axis=1)
        c = X @ rows.T
        assert (c[:, 3] > 0).all()
        err = np.maximum(np.abs(c[:, 0] / c[:, 3] - xs.reshape(-1)), np.abs(c[:, 1] / c[:, 3] - ys.reshape(-1)))
        assert err.max() < 1e-3, (t, err.max())
    behind = np.concatenate([o - d * 3.0, np.ones((w * h, 1))], axis=1) @ rows.T
    assert (behind[:, 3] <= 0).all()
    # a direction (w = 0: what a miss projects) lands on its own pixel too
    c = d @ rows[:, :3].T
    assert np.abs(c[:, 0] / c[:, 3] - xs.reshape(-1)).max() < 1e-3


# ---------------------------------------------------------------------------- the restatement
def _flat(h, w, hit, colour, n):
    """A fronto-parallel plane at z = 0 seen from (0, 0, 5) (or all misses), one colour, n samples."""
    cam = Camera(w, h, position=np.array([0.0, 0.0, 5.0], np.float32))
    d = cam.recalculate_ray_directions()["direction"].reshape(h, w, 3)
    feats = {"normal": np.zeros((h, w, 3), np.float32), "depth": np.full((h, w), R.F32_MAX, np.float32),
             "albedo": np.full((h, w, 3), 0.25, np.float32), "hit": np.full((h, w), float(hit), np.float32)}
    if hit:
        feats["normal"][...] = (0.0, 0.0, 1.0)
        feats["depth"] = (np.float32(-5.0) / d[..., 2]).astype(np.float32)
    acc = np.broadcast_to(np.asarray(colour, np.float32) * np.float32(n), (h, w, 4)).copy()
    return cam, d, feats, acc


def test_restatement_without_a_previous_slot_is_the_scaled_accumulation():
    rng = np.random.default_rng(0)
    cam, d, feats, _ = _flat(9, 13, 1, (0, 0, 0, 0), 1)
    acc = (rng.random((9, 13, 4)) * 7).astype(np.float32)
    ref = T.TemporalRef()
    r = ref.call(acc, feats, cam.position, d, 4, 5, 0, cam.world_to_pixel(), iterations=0)
    want = acc / np.float32(15)
    assert np.array_equal(bits(r["out"]), bits(want)) and np.array_equal(bits(r["f"]), bits(want))
    assert (r["n_out"] == np.float32(15)).all()
    assert r["counters"]["no_previous"] == 9 * 13
    assert np.array_equal(r["u"], R.pack_rgba8(R.clamp01(want)))
    out, n = ref.read()
    assert out is r["out"] and np.array_equal(n, r["n_out"])


@pytest.mark.parametrize("hit", [1, 0])
def test_restatement_static_camera_constant_colour(hit):
    """A static camera and one colour: the output is that colour and n_out = min(n_prev, max_history)
    + N; a second call in the same generation reads the same previous slot (no double counting);
    max_history = 1 caps nh at 1; reset makes the next call a first call."""
    colour = (0.5, 0.25, 0.75, 1.0)
    cam, d, feats, acc3 = _flat(10, 20, hit, colour, 3)
    acc2 = _flat(10, 20, hit, colour, 2)[3]
    m = cam.world_to_pixel()
    ref = T.TemporalRef()
    a = ref.call(acc3, feats, cam.position, d, 4, 1, 0, m)
    assert (a["n_out"] == 3).all()
    b = ref.call(acc2, feats, cam.position, d, 3, 1, 1, m)                    # generation 1: history 3, N 2
    inner = (slice(1, -1), slice(1, -1))                                      # a reprojection may round off an edge
    assert (b["n_out"][inner] == 5).all() and set(np.unique(b["n_out"])) <= {2.0, 5.0}
    assert np.allclose(b["out"], colour, rtol=1e-6, atol=0) and np.allclose(b["f"], colour, rtol=1e-5, atol=0)
    b2 = ref.call(acc3, feats, cam.position, d, 4, 1, 1, m)                   # same generation: still history 3
    assert (b2["n_out"][inner] == 6).all() and b2["counters"]["no_previous"] == 0
    c = ref.call(acc2, feats, cam.position, d, 3, 1, 2, m, max_history=4)     # history min(6, 4)
    assert (c["n_out"][inner] == 6).all() and c["counters"]["capped"] > 0
    if not hit:
        assert c["counters"]["miss_to_miss"] > 0
    e = ref.call(acc2, feats, cam.position, d, 3, 1, 3, m, max_history=1)     # nh capped at 1
    assert (e["n_out"][inner] == 3).all()
    ref.reset()
    g = ref.call(acc2, feats, cam.position, d, 3, 1, 4, m)
    assert (g["n_out"] == 2).all() and g["counters"]["no_previous"] == 200


def test_restatement_rejects_history_across_hit_and_miss():
    """The previous frame all misses, the current all hits: nothing is reused."""
    cam, d, miss, acc_m = _flat(8, 16, 0, (1.0, 0.0, 0.0, 1.0), 1)
    _, _, hits, acc_h = _flat(8, 16, 1, (0.0, 1.0, 0.0, 1.0), 1)
    ref = T.TemporalRef()
    ref.call(acc_m, miss, cam.position, d, 2, 1, 0, cam.world_to_pixel())
    r = ref.call(acc_h, hits, cam.position, d, 2, 1, 1, cam.world_to_pixel(), iterations=0)
    assert np.array_equal(r["out"], acc_h) and (r["n_out"] == 1).all()
    assert r["counters"]["off_screen"] == 0 and not any(r["counters"][f"taps_{n}"] for n in (1, 2, 3, 4))


# ---------------------------------------------------------------------------- quality against the oracle
# The sideways translation per frame. A pixel of these 36-row frames covers 2*tan(22.5 deg)/36 = 0.023 r at
# distance r, so 0.45 is about one pixel of parallax at r = 20 (the middle of both scenes) and more in front.
STEP = np.array([0.45, 0.0, 0.0], np.float32)
FRAMES = 8
# The bilinear taps lie up to one pixel from the reprojected point and a pixel is 0.023 r wide (more on
# an oblique surface): the default sigma_position of 0.02 suits frames of a few hundred rows and rejects
# nearly every off-centre tap here. 0.1 is about four pixel widths at this size; max_history = 6 lets the
# cap be reached within the 8 frames.
SMALL_FRAME = dict(sigma_position=0.1, max_history=6)


@functools.lru_cache(maxsize=None)
def moving_sequence(name):
    """Per camera of the sideways sequence: (camera, rays, oracle 1-spp accumulation, oracle features);
    and the 256-frame accumulation of the last camera."""
    from oracle import oracle as O

    O.build()
    g, case = load(name), CASES[name]
    w, h = int(g["width"]), int(g["height"])
    seq = []
    for i in range(FRAMES):
        scene = scene_from_inputs(g)
        cam = Camera(w, h, position=np.asarray(g["camera_origin"], np.float32) + np.float32(i) * STEP)
        scene.camera = cam
        rays = cam.recalculate_ray_directions()
        o = O.Oracle(scene, camera_rays=rays)
        acc = np.zeros((h, w, 4), np.float32)
        out = np.zeros((h, w), np.uint32)
        o.render_frame(params_for(scene, case, 1), case["bounces"], acc, out)
        seq.append((cam, rays, acc.copy(), R.oracle_features(O, scene, camera_rays=rays)))
    for k in range(2, 257):
        o.render_frame(params_for(scene, case, k), case["bounces"], acc, out)
    return seq, acc / np.float32(256)


@pytest.mark.parametrize("name", ["c2_64x36_b8", "c3_64x36_b8"])
def test_temporal_beats_the_spatial_filter_on_a_moving_camera(oracle_lib, name):
    """A camera translating sideways for 8 frames, a reset and 1 spp at each step. On the last
    camera, temporal + default filter is strictly closer (RMSE over rgb clamped to [0, 1]) to the
    oracle's 256-frame accumulation than the spatial-only filter of the same 1-spp frame, with the
    default temporal parameters and with SMALL_FRAME (every branch counter of the restatement is
    non-zero over that sequence). Measured, temporal against spatial-only: C2 0.0178 against 0.0203
    (ratio 0.878) with the defaults and 0.0178 (0.878) with SMALL_FRAME; C3 0.1110 against 0.1159
    (0.958) and 0.1063 (0.918). DESIGN.md §5.4f says why the gain is small at this size."""
    seq, converged = moving_sequence(name)
    ref = np.clip(converged[..., :3], 0, 1).astype(np.float64)
    case = CASES[name]

    def rmse(a):
        return float(np.sqrt(np.mean((np.clip(a[..., :3], 0, 1).astype(np.float64) - ref) ** 2)))

    cam, rays, acc, feats = seq[-1]
    spatial = rmse(R.filter_ref(acc, feats, k=2, compute_per_frame=case["spp"])[0])
    for tparams in ({}, SMALL_FRAME):
        tr = T.TemporalRef()
        totals = dict.fromkeys(T.COUNTERS + T.EDGE_COUNTERS, 0)
        for i, (cam, rays, acc, feats) in enumerate(seq):
            h, w = acc.shape[:2]
            r = tr.call(acc, feats, cam.position, rays["direction"].reshape(h, w, 3), 2, case["spp"], i,
                        cam.world_to_pixel(), **tparams)
            for key, v in r["counters"].items():
                totals[key] += v
        temporal = rmse(r["f"])
        print(f"{name} {tparams}: temporal {temporal:.4f} spatial {spatial:.4f} "
              f"ratio {temporal / spatial:.3f} counters {totals}")
        assert np.isfinite(r["f"]).all()
        assert temporal < spatial
    assert all(totals[key] > 0 for key in T.COUNTERS), totals
