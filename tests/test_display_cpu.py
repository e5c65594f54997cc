"""The display transform without a GPU: the ABI surface (rt_display_params, the six entry points), the
documented defaults, NULL-context calls, and self-checks of the NumPy restatement of the display
contract (tests/display_ref.py).

No kernel launches here; tests/test_gpu_display.py compares the kernels with the restatement.
"""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from tests import display_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
FUNCTIONS = ("rt_display_default_params", "rt_display", "rt_read_display", "rt_copy_display_to_device",
             "rt_display_state", "rt_display_reset")
PARAM_FIELDS = ("source", "tone_operator", "encode", "auto_exposure", "exposure", "key", "min_exposure",
                "max_exposure", "adaptation", "white", "low_permille", "high_permille")
f32 = np.float32


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---------------------------------------------------------------------------- ABI
def test_functions_declared_exported_and_bound(native_lib):
    text = HEADER.read_text()
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", text, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in FUNCTIONS:
        assert name in declared
        assert name in exported
        assert name in N.SIGNATURES
        assert hasattr(native_lib, name)
    assert native_lib.rt_abi_version() == 12
    assert "additive: display transform" in text
    for name, value in (("RT_DISPLAY_ACCUMULATION", 0), ("RT_DISPLAY_DENOISED", 1), ("RT_DISPLAY_PLANE", 2),
                        ("RT_TONE_LINEAR", 0), ("RT_TONE_REINHARD", 1), ("RT_TONE_ACES", 2), ("RT_ENCODE_NONE", 0),
                        ("RT_ENCODE_SRGB", 1)):
        assert re.search(rf"#define {name}\s+{value}u\b", text), name
        assert getattr(N, name) == value
    assert (R.ACCUMULATION, R.DENOISED, R.PLANE, R.LINEAR, R.REINHARD, R.ACES, R.NONE, R.SRGB) == (0, 1, 2, 0, 1, 2, 0, 1)


def test_params_layout_against_compiled_header(tmp_path):
    """sizeof and every field offset of rt_display_params from a C program compiled against the real
    header equal the ctypes structure's and the numpy dtype's: 48 bytes, twelve 4-byte fields."""
    args = ["sizeof(rt_display_params)"] + [f"offsetof(rt_display_params, {f})" for f in PARAM_FIELDS]
    fmt = " ".join(["%zu"] * len(args))
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [48] + [4 * i for i in range(12)]
    assert ctypes.sizeof(N.rt_display_params) == B.DISPLAY_PARAMS.itemsize == 48
    assert [getattr(N.rt_display_params, f).offset for f in PARAM_FIELDS] == got[1:]
    assert [B.DISPLAY_PARAMS.fields[f][1] for f in PARAM_FIELDS] == got[1:]
    assert tuple(f for f, _ in N.rt_display_params._fields_) == B.DISPLAY_PARAMS.names == PARAM_FIELDS


def test_default_params(native_lib):
    p = N.rt_display_params()
    assert native_lib.rt_display_default_params(ctypes.byref(p)) == N.RT_OK
    assert (p.source, p.tone_operator, p.encode, p.auto_exposure) == (0, 1, 1, 1)
    assert (p.low_permille, p.high_permille) == (100, 50)
    for got, want in ((p.exposure, 1.0), (p.key, 0.18), (p.min_exposure, 1.0 / 64.0), (p.max_exposure, 64.0),
                      (p.adaptation, 1.0), (p.white, 4.0)):
        assert bits(got) == bits(want)
    assert native_lib.rt_display_default_params(None) == N.RT_E_INVALID
    for f in PARAM_FIELDS:  # the restatement's defaults are the library's
        assert f32(R.DEFAULTS[f]) == f32(getattr(p, f)), f


def test_null_context_fails_cleanly(native_lib):
    buf = (ctypes.c_uint32 * 256)()
    e, m = ctypes.c_float(7.0), ctypes.c_uint64(7)
    p = N.rt_display_params()
    native_lib.rt_display_default_params(ctypes.byref(p))
    assert native_lib.rt_display(None, ctypes.byref(p), None) == N.RT_E_INVALID
    assert native_lib.rt_display(None, None, None) == N.RT_E_INVALID
    assert native_lib.rt_read_display(None, buf) == N.RT_E_INVALID
    assert native_lib.rt_copy_display_to_device(None, buf, 64) == N.RT_E_INVALID
    assert native_lib.rt_display_state(None, ctypes.byref(e), buf, ctypes.byref(m)) == N.RT_E_INVALID
    assert native_lib.rt_display_reset(None) == N.RT_E_INVALID
    assert not any(buf) and e.value == 7.0 and m.value == 7


def test_contract_text_is_in_kernel_source_and_header():
    """The restatement is written from the header comment of display.hip; the lines it restates are
    there and in include/rt_abi.h, word for word."""
    lines = ["L = (0.2126f*S.r + 0.7152f*S.g) + 0.0722f*S.b.",
             "The pixel is metered iff L > 0 && L < +inf. Both tests are false for NaN.",
             "j = clamp((int)(bits(L) >> 20) - 888, 0, 255).",
             "lo = total*low_permille/1000.",
             "hi = total - total*high_permille/1000.",
             "a = (2*Sn + Nn) / (2*Nn).",
             "n = 256 - a, q = floor(n / 16), r = n - 16*q.",
             "E_t = key * ldexpf(T16[r], q).",
             "E_t = min(max(E_t, min_exposure), max_exposure).",
             "0x3f800000, 0x3f85aac3, 0x3f8b95c2, 0x3f91c3d3, 0x3f9837f0, 0x3f9ef532, 0x3fa5fed7, 0x3fad583f,",
             "0x3fb504f3, 0x3fbd08a4, 0x3fc5672a, 0x3fce248c, 0x3fd744fd, 0x3fe0ccdf, 0x3feac0c7, 0x3ff5257d.",
             "State none, target none: E = min(max(1.0f, min_exposure), max_exposure).",
             "State E_prev, target E_t: E = E_prev + (E_t - E_prev)*adaptation.",
             "x = x > 0 ? x : 0. NaN and -0 give +0.",
             "x = min(x, 65536.0f).",
             "y = (x*(1.0f + x*iw2)) / (1.0f + x).",
             "ACES: y = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f).",
             "NONE: code = (uint32_t)(y*255.0f) & 0xff, which is pack_rgba8.",
             "SRGB: code is the largest j in 0..255 with srgb_table[j] <= y.",
             "The packed word is r | g<<8 | b<<16 | a<<24."]
    for path in (ROOT / "rust_gpu_raytracing_amd" / "csrc" / "display.hip", HEADER):
        text = path.read_text()
        for line in lines:
            assert line in text, (path.name, line)


# ---------------------------------------------------------------------------- the restatement
def test_restatement_table_is_the_librarys(native_lib):
    assert np.array_equal(bits(R.srgb_table()), bits(N.srgb_table()))
    assert np.array_equal(R.T16, (2.0 ** (np.arange(16) / 16.0)).astype(f32))


def test_restatement_srgb_encode_inverts_the_decode():
    t = R.srgb_table()
    assert (np.diff(t) > 0).all() and t[0] == 0 and t[255] == 1
    assert np.array_equal(R.code_srgb(t), np.arange(256))
    below = np.nextafter(t[1:], f32(0.0))
    assert below.dtype == f32
    assert np.array_equal(R.code_srgb(below), np.arange(255))
    assert R.code_srgb(f32(0.0)) == 0  # j = 0 has no value below it: 0 is the smallest y


def test_restatement_bin_edges():
    def bin_of(v):
        j, metered = R.bins_of(f32(v))
        assert metered
        return int(j.reshape(-1)[0])

    assert bin_of(2.0 ** -16) == 0 and bin_of(1.0) == 128 and bin_of(0.18) == 107
    assert bin_of(2.0 ** 16) == 255 and bin_of(3e38) == 255 and bin_of(1e-30) == 0
    assert bin_of(np.nextafter(f32(2.0 ** -16), f32(0))) == 0 and bin_of(np.nextafter(f32(1.0), f32(0))) == 127
    assert bin_of(np.nextafter(f32(2.0 ** 16), f32(0))) == 255 and bin_of(2.0 ** 15) == 248
    assert bin_of(1e-45) == 0  # a denormal is metered
    for v in (0.0, -0.0, -1.0, np.inf, -np.inf, np.nan):
        assert not R.bins_of(f32(v))[1], v
    # the luminance is the written sum; a grey pixel keeps its value to within two roundings
    assert bits(R.luminance(np.array([1.0, 2.0, 4.0, 9.0], f32))) == bits((f32(0.2126) * f32(1) + f32(0.7152) * f32(2))
                                                                          + f32(0.0722) * f32(4))
    h = R.histogram(np.array([[1, 1, 1, 1], [0, 0, 0, 1], [np.nan, 1, 1, 1], [0.18, 0.18, 0.18, 0]], f32))
    assert h.sum() == 2 and h[107] == 1 and h[128] + h[127] == 1


def test_restatement_curves_are_monotonic():
    x = np.unique(np.concatenate([np.exp2(np.linspace(-20, 17, 20001)).astype(f32), [f32(0), f32(4), f32(65536)]]))
    for op in (R.LINEAR, R.REINHARD, R.ACES):
        y = R.tone(x, 1.0, op)
        assert (np.diff(y) >= 0).all(), op
        assert y.min() >= 0 and y.max() == 1
    assert R.tone(f32(4.0), 1.0, R.REINHARD, white=4.0) == f32(1.0)
    assert R.tone(np.nextafter(f32(4.0), f32(0)), 1.0, R.REINHARD, white=4.0) <= f32(1.0)
    assert R.tone(f32(0.5), 2.0, R.LINEAR) == f32(1.0) and R.tone(f32(0.25), 2.0, R.LINEAR) == f32(0.5)
    for bad in (np.nan, -0.0, -3.0, -np.inf):
        for op in (R.LINEAR, R.REINHARD, R.ACES):
            assert bits(R.tone(f32(bad), 1.0, op)) == 0, (bad, op)  # +0
    assert R.tone(f32(np.inf), 1.0, R.ACES) == 1 and R.tone(f32(3e38), 8.0, R.REINHARD) == 1


def test_restatement_solve_known_answers():
    d = R.DEFAULTS
    h = np.zeros(256, np.uint32)
    h[107] = 777
    s = R.solve(h, 0.18, d["min_exposure"], d["max_exposure"], 100, 50)
    assert (s["a"], s["n"], s["q"], s["r"]) == (215, 41, 2, 9) and bits(s["e_t"]) == bits(1.0633149)
    h = np.zeros(256, np.uint32)
    h[0] = h[255] = 5
    s = R.solve(h, 0.18, d["min_exposure"], d["max_exposure"], 100, 50)
    assert (s["a"], s["q"], s["r"]) == (284, -2, 4) and bits(s["e_t"]) == bits(0.05351432)
    h = np.zeros(256, np.uint32)
    h[255] = 1
    s = R.solve(h, 0.18, 1.0 / 64.0, 64.0, 499, 499)
    assert s["a"] == 511 and bits(s["e_t"]) == bits(0.015625)
    assert R.solve(np.zeros(256, np.uint32), 0.18, 1.0 / 64.0, 64.0, 100, 50) is None
    h = np.zeros(256, np.uint32)
    h[0] = 3  # the other end: a = 1, the target far above the clamp
    s = R.solve(h, 0.18, 1.0 / 64.0, 64.0, 0, 0)
    assert s["a"] == 1 and s["q"] == 15 and s["r"] == 15 and s["e_t"] == f32(64.0)


def test_restatement_adaptation_table():
    assert R.adapt(None, None, 1 / 64, 64.0, 0.25) == f32(1.0)
    assert R.adapt(None, None, 2.0, 64.0, 0.25) == f32(2.0) and R.adapt(None, None, 0.1, 0.5, 1.0) == f32(0.5)
    assert R.adapt(None, f32(3.0), 1 / 64, 64.0, 0.25) == f32(3.0)
    assert R.adapt(f32(2.0), None, 1 / 64, 64.0, 0.25) == f32(2.0)
    assert R.adapt(f32(2.0), f32(4.0), 1 / 64, 64.0, 0.25) == f32(2.5)
    e = R.adapt(f32(0.3), f32(1.7), 1 / 64, 64.0, 0.1)
    assert e.dtype == f32 and bits(e) == bits(f32(0.3) + (f32(1.7) - f32(0.3)) * f32(0.1))


def test_restatement_identity_is_the_frames_pack():
    """Manual exposure 1, LINEAR and NONE is clamp01 and the truncating pack of the frame output."""
    from tests import denoise_ref as D

    rng = np.random.default_rng(3)
    s = (rng.random((7, 11, 4)) * 3 - 0.5).astype(f32)
    img, e, state, hist, metered = R.display_ref(s, e_prev=f32(9.0), auto_exposure=0, exposure=1.0,
                                                 tone_operator=R.LINEAR, encode=R.NONE)
    assert np.array_equal(img, D.pack_rgba8(D.clamp01(s)))
    assert e == 1 and state == f32(9.0) and hist is None and metered is None
