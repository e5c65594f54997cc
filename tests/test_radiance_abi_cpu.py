"""Radiance-query surface of the C ABI (rt_radiance, rt_radiance_device): declared, exported, and
the ray record laid out identically in the header, ctypes and numpy.

No kernel launches here (no GPU in the CPU suite); tests/test_gpu_radiance.py runs the queries.
"""
import ctypes
import re
import subprocess
from pathlib import Path

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
RADIANCE_FUNCTIONS = ("rt_radiance", "rt_radiance_device")
RAY_FIELDS = ("origin", "stream", "direction", "_pad1")


def test_radiance_functions_declared_and_exported(native_lib):
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", HEADER.read_text(), re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in RADIANCE_FUNCTIONS:
        assert name in declared
        assert name in exported
        assert name in N.SIGNATURES
        assert hasattr(native_lib, name)
    # (ctx, rays, radiance, count, bounces, first_sample, samples, segments)
    for name in RADIANCE_FUNCTIONS:
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 8
        assert args[3] is ctypes.c_uint64 and args[4:7] == [ctypes.c_uint32] * 3


def test_record_size_and_fields():
    assert ctypes.sizeof(N.rt_radiance_ray) == B.RADIANCE_RAY.itemsize == 32
    assert B.RADIANCE_RAY.names == RAY_FIELDS
    assert tuple(f for f, _ in N.rt_radiance_ray._fields_) == RAY_FIELDS
    assert B.RADIANCE_RAY.fields["stream"][0] == "<u4"
    assert N.rt_radiance_ray.stream.size == 4


def test_record_layout_against_compiled_header(tmp_path):
    """sizeof and every field offset from a C program compiled against the real header equal the
    ctypes structure's and the numpy dtype's; the record overlays rt_query_ray and rt_occlusion_ray
    field for field."""
    records = ("rt_radiance_ray", "rt_query_ray", "rt_occlusion_ray")
    fmt = " ".join(["%zu"] * (len(records) + len(RAY_FIELDS) + 4))
    args = [f"sizeof({r})" for r in records]
    args += [f"offsetof(rt_radiance_ray, {f})" for f in RAY_FIELDS]
    args += ["offsetof(rt_query_ray, _pad0)", "offsetof(rt_query_ray, direction)",
             "offsetof(rt_occlusion_ray, direction)", "offsetof(rt_occlusion_ray, t_max)"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:3] == [32, 32, 32]
    off = got[3:3 + len(RAY_FIELDS)]
    assert off == [getattr(N.rt_radiance_ray, f).offset for f in RAY_FIELDS]
    assert off == [B.RADIANCE_RAY.fields[f][1] for f in RAY_FIELDS]
    # two 16-byte loads: {origin, stream}, {direction, pad}
    assert off == [0, 12, 16, 28]
    assert off[RAY_FIELDS.index("stream")] == 12 and off[RAY_FIELDS.index("direction")] == 16
    # one buffer serves rt_trace_rays, rt_occluded and rt_radiance
    assert got[3 + len(RAY_FIELDS):] == [off[1], off[2], off[2], off[3]]


def test_header_pins_record_size_and_history():
    text = HEADER.read_text()
    assert re.search(r"static_assert\(sizeof\(rt_radiance_ray\) == 32", text)
    assert re.search(r"_Static_assert\(sizeof\(rt_radiance_ray\) == 32", text)
    assert "12, additive: radiance queries" in text


def test_null_context_fails_cleanly(native_lib):
    rays = (N.rt_radiance_ray * 2)()
    out = (ctypes.c_float * 8)()
    seg = ctypes.c_uint64(7)
    assert native_lib.rt_radiance(None, rays, out, 2, 4, 1, 1, ctypes.byref(seg)) == N.RT_E_INVALID
    assert native_lib.rt_radiance(None, None, None, 0, 4, 1, 1, None) == N.RT_E_INVALID
    assert native_lib.rt_radiance_device(None, rays, out, 2, 4, 1, 1, None) == N.RT_E_INVALID
    assert seg.value == 7 and not any(out)


def test_abi_version_unchanged(native_lib):
    assert native_lib.rt_abi_version() == 12
