"""Occlusion-query surface of the C ABI (rt_occluded, rt_occluded_device): declared, exported, and
rt_occlusion_ray laid out identically in the header, ctypes and numpy -- and as rt_query_ray, with
t_max in the place of its second pad.

No kernel launches here (no GPU in the CPU suite); tests/test_gpu_occlusion.py runs the queries.
"""
import ctypes
import re
import subprocess
from pathlib import Path

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
OCCLUSION_FUNCTIONS = ("rt_occluded", "rt_occluded_device")

RAY_FIELDS = ("origin", "_pad0", "direction", "t_max")
QUERY_RAY_FIELDS = ("origin", "_pad0", "direction", "_pad1")


def test_occlusion_functions_declared_and_exported(native_lib):
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", HEADER.read_text(), re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in OCCLUSION_FUNCTIONS:
        assert name in declared
        assert name in exported
        assert name in N.SIGNATURES
        assert hasattr(native_lib, name)


def test_record_size_and_names():
    assert ctypes.sizeof(N.rt_occlusion_ray) == B.OCCLUSION_RAY.itemsize == 32
    assert B.OCCLUSION_RAY.names == RAY_FIELDS
    assert tuple(f for f, _ in N.rt_occlusion_ray._fields_) == RAY_FIELDS


def test_record_layout_against_compiled_header(tmp_path):
    """sizeof and every field offset from a C program compiled against the real header equal the
    ctypes structure's and the numpy dtype's, and rt_query_ray's field by field."""
    args = ["sizeof(rt_occlusion_ray)"]
    args += [f"offsetof(rt_occlusion_ray, {f})" for f in RAY_FIELDS]
    args += [f"offsetof(rt_query_ray, {f})" for f in QUERY_RAY_FIELDS]
    fmt = " ".join(["%zu"] * len(args))
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[0] == 32
    off, query_off = got[1:1 + len(RAY_FIELDS)], got[1 + len(RAY_FIELDS):]
    assert off == [getattr(N.rt_occlusion_ray, f).offset for f in RAY_FIELDS]
    assert off == [B.OCCLUSION_RAY.fields[f][1] for f in RAY_FIELDS]
    # one buffer serves rt_trace_rays and rt_occluded: t_max sits where rt_query_ray pads
    assert off == query_off == [0, 12, 16, 28]
    assert query_off == [B.QUERY_RAY.fields[f][1] for f in QUERY_RAY_FIELDS]


def test_header_pins_record_size_and_history():
    text = HEADER.read_text()
    assert re.search(r"static_assert\(sizeof\(rt_occlusion_ray\) == 32", text)
    assert re.search(r"_Static_assert\(sizeof\(rt_occlusion_ray\) == 32", text)
    assert "additive: occlusion queries" in text
    assert "12, additive: ray queries" in text


def test_null_context_fails_cleanly(native_lib):
    rays = (N.rt_occlusion_ray * 2)()
    out = (ctypes.c_uint8 * 2)()
    assert native_lib.rt_occluded(None, rays, out, 2) == N.RT_E_INVALID
    assert native_lib.rt_occluded(None, None, None, 0) == N.RT_E_INVALID
    assert native_lib.rt_occluded_device(None, rays, out, 2) == N.RT_E_INVALID
    assert native_lib.rt_occluded_device(None, None, None, 0) == N.RT_E_INVALID
    assert bytes(out) == b"\0\0"


def test_abi_version_unchanged(native_lib):
    assert native_lib.rt_abi_version() == 12
