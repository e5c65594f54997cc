"""Feature buffers and denoiser without a GPU: the ABI surface (rt_denoise_params, the seven entry
points), the NumPy restatement of the filter contract (tests/denoise_ref.py), and the default
parameters pinned against converged oracle renders.

No kernel launches here; tests/test_gpu_denoise.py compares the kernels with the restatement.
"""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from tests import denoise_ref as R
from tests.golden.fixtures import params_for

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
FUNCTIONS = ("rt_denoise_default_params", "rt_compute_features", "rt_read_features", "rt_features_device",
             "rt_denoise", "rt_read_denoised", "rt_copy_denoised_to_device")
PARAM_FIELDS = ("iterations", "sigma_color", "sigma_albedo", "sigma_depth")


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
    assert "additive: denoiser" in HEADER.read_text()


def test_params_layout_against_compiled_header(tmp_path):
    """sizeof and every field offset of rt_denoise_params from a C program compiled against the
    real header equal the ctypes structure's and the numpy dtype's: 16 bytes, offsets 0, 4, 8, 12."""
    args = ["sizeof(rt_denoise_params)"] + [f"offsetof(rt_denoise_params, {f})" for f in PARAM_FIELDS]
    fmt = " ".join(["%zu"] * len(args))
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [16, 0, 4, 8, 12]
    assert ctypes.sizeof(N.rt_denoise_params) == B.DENOISE_PARAMS.itemsize == 16
    assert [getattr(N.rt_denoise_params, f).offset for f in PARAM_FIELDS] == got[1:]
    assert [B.DENOISE_PARAMS.fields[f][1] for f in PARAM_FIELDS] == got[1:]
    assert tuple(f for f, _ in N.rt_denoise_params._fields_) == B.DENOISE_PARAMS.names == PARAM_FIELDS


def test_default_params(native_lib):
    p = N.rt_denoise_params()
    assert native_lib.rt_denoise_default_params(ctypes.byref(p)) == N.RT_OK
    assert p.iterations == 4
    for got, want in ((p.sigma_color, 1.0), (p.sigma_albedo, 0.1), (p.sigma_depth, 0.05)):
        assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
    assert native_lib.rt_denoise_default_params(None) == N.RT_E_INVALID
    d = R.DEFAULTS
    assert (d["iterations"], d["sigma_color"], d["sigma_albedo"], d["sigma_depth"]) == (4, 1.0, 0.1, 0.05)


def test_null_context_fails_cleanly(native_lib):
    buf = (ctypes.c_float * 8)()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    p = N.rt_denoise_params(1, 1.0, 1.0, 1.0)
    assert native_lib.rt_compute_features(None) == N.RT_E_INVALID
    assert native_lib.rt_read_features(None, buf, buf) == N.RT_E_INVALID
    assert native_lib.rt_features_device(None, ctypes.byref(a), ctypes.byref(b)) == N.RT_E_INVALID
    assert native_lib.rt_denoise(None, ctypes.byref(p)) == N.RT_E_INVALID
    assert native_lib.rt_denoise(None, None) == N.RT_E_INVALID
    assert native_lib.rt_read_denoised(None, buf, buf) == N.RT_E_INVALID
    assert native_lib.rt_copy_denoised_to_device(None, buf, 64) == N.RT_E_INVALID
    assert not any(buf) and a.value is None and b.value is None


def test_contract_text_is_in_kernel_source_and_header():
    """The restatement is written from the header comment of denoise.hip; the lines it restates
    are there and in include/rt_abi.h, word for word."""
    lines = ["c0(p) = accumulation(p) / D, all four channels;",
             "D = (float)((k-1) * compute_per_frame);",
             "s0 = sigma_color / sqrtf((float)N);",
             "k_a = 1.0f / (sigma_albedo*sigma_albedo);",
             "for iteration i: s_i = s0 * 0.5f^i (exact scaling) and k_c = 1.0f / (s_i*s_i).",
             "h = {1/16, 1/4, 3/8, 1/4, 1/16};",
             "dy is the outer loop and dx the inner loop, each running -2..2 ascending.",
             "d = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z);",
             "wn = d^32, by five squarings;",
             "x = |z_p - z_q| / (sigma_depth*(z_p + z_q) + 1e-30f);",
             "xa = ((da.r*da.r + da.g*da.g) + da.b*da.b) * k_a;",
             "xc = ((dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b) * k_c;",
             "Weight: w = (((h[dy]*h[dx]) * g) * (ra*ra)) * (rc*rc).",
             "The tap is skipped unless w > 0. That test is false for NaN."]
    for path in (ROOT / "rust_gpu_raytracing_amd" / "csrc" / "denoise.hip", HEADER):
        text = path.read_text()
        for line in lines:
            assert line in text, (path.name, line)


# ---------------------------------------------------------------------------- the restatement
def _flat_features(h, w, hit):
    return {"normal": np.zeros((h, w, 3), np.float32), "depth": np.full((h, w), R.F32_MAX if not hit else 2.0, np.float32),
            "albedo": np.full((h, w, 3), 0.25, np.float32), "hit": np.full((h, w), float(hit), np.float32)}


def test_restatement_iterations_zero_is_the_scaled_accumulation():
    rng = np.random.default_rng(0)
    acc = (rng.random((9, 13, 4)) * 7).astype(np.float32)
    f, u = R.filter_ref(acc, _flat_features(9, 13, 0), k=4, compute_per_frame=5, iterations=0)
    want = acc / np.float32(15)
    assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(u, R.pack_rgba8(R.clamp01(want)))
    assert R.pack_rgba8(np.array([[1.0, 0.5, 0.999, 0.0]], np.float32))[0] == 255 | (127 << 8) | (254 << 16)


def test_restatement_constant_misses_stay_constant_and_finite():
    """Every pixel a miss (depth 3.4e38: z_p + z_q overflows, but the guide of two misses is 1 and
    evaluates no depth) with one colour: every iteration returns that colour, finite."""
    acc = np.broadcast_to(np.array([0.6, 0.3, 0.9, 1.0], np.float32) * np.float32(3), (11, 17, 4)).copy()
    f, _ = R.filter_ref(acc, _flat_features(11, 17, 0), k=4, compute_per_frame=1, iterations=5)
    assert np.isfinite(f).all()
    assert np.allclose(f, acc / np.float32(3), rtol=1e-6, atol=0)


def test_restatement_does_not_blend_across_hit_and_miss():
    """Left half misses, right half hits on one plane, different colours: no tap crosses."""
    h, w = 8, 16
    feats = _flat_features(h, w, 1)
    feats["normal"][...] = (0.0, 1.0, 0.0)
    feats["hit"][:, :8] = 0.0
    feats["normal"][:, :8] = 0.0
    feats["depth"][:, :8] = R.F32_MAX
    acc = np.zeros((h, w, 4), np.float32)
    acc[:, :8], acc[:, 8:] = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)
    f, _ = R.filter_ref(acc, feats, k=2, compute_per_frame=1, iterations=3)
    assert np.array_equal(f, acc)


# ---------------------------------------------------------------------------- defaults against the oracle
@pytest.mark.parametrize("name", ["c2_64x36_b8", "c3_64x36_b8"])
def test_defaults_reduce_the_error_of_four_frames(oracle_lib, name):
    """The oracle's 4-frame accumulation filtered with the default parameters and oracle-built
    features is strictly closer (RMSE over rgb clamped to [0, 1]) to the oracle's 256-frame
    accumulation than the unfiltered 4 frames. Measured: C2 0.0459 against 0.0595 (ratio 0.771), C3
    0.0820 against 0.1002 (ratio 0.819)."""
    g, case, scene, feats = R.golden_case(name)
    o = oracle_lib.Oracle(scene, camera_rays=np.asarray(g["camera_rays"]).astype(B.RAY))
    acc = np.zeros((o.height, o.width, 4), np.float32)
    out = np.zeros((o.height, o.width), np.uint32)
    for k in range(1, 257):
        o.render_frame(params_for(scene, case, k), case["bounces"], acc, out)
        if k == 4:
            acc4 = acc.copy()
    ref = np.clip((acc / np.float32(256))[..., :3], 0, 1).astype(np.float64)
    f, _ = R.filter_ref(acc4, feats, k=5, compute_per_frame=case["spp"])

    def rmse(a):
        return float(np.sqrt(np.mean((np.clip(a[..., :3], 0, 1).astype(np.float64) - ref) ** 2)))

    filtered, unfiltered = rmse(f), rmse(acc4 / np.float32(4))
    print(f"{name}: filtered {filtered:.4f} unfiltered {unfiltered:.4f} ratio {filtered / unfiltered:.3f}")
    assert np.isfinite(f).all()
    assert filtered < unfiltered
