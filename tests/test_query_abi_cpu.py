"""Ray-query surface of the C ABI (rt_trace_rays, rt_trace_rays_device, rt_pick): declared,
exported, and the two records laid out identically in the header, ctypes and numpy.

No kernel launches here (no GPU in the CPU suite); tests/test_gpu_query.py runs the queries.
"""
import ctypes
import re
import subprocess
from pathlib import Path

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
QUERY_FUNCTIONS = ("rt_trace_rays", "rt_trace_rays_device", "rt_pick")

RAY_FIELDS = ("origin", "_pad0", "direction", "_pad1")
HIT_FIELDS = ("t", "position", "normal", "u", "v", "material_index", "front_face", "kind", "index", "sub_object",
              "triangle", "_reserved")


def test_query_functions_declared_and_exported(native_lib):
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", HEADER.read_text(), re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in QUERY_FUNCTIONS:
        assert name in declared
        assert name in exported
        assert name in N.SIGNATURES
        assert hasattr(native_lib, name)


def test_record_sizes():
    assert ctypes.sizeof(N.rt_query_ray) == B.QUERY_RAY.itemsize == 32
    assert ctypes.sizeof(N.rt_hit) == B.HIT.itemsize == 64
    assert B.QUERY_RAY.names == RAY_FIELDS and B.HIT.names == HIT_FIELDS


def test_record_layouts_against_compiled_header(tmp_path):
    """sizeof and every field offset from a C program compiled against the real header equal the
    ctypes structures' and the numpy dtypes'."""
    fmt = " ".join(["%zu"] * (2 + len(RAY_FIELDS) + len(HIT_FIELDS)))
    args = ["sizeof(rt_query_ray)", "sizeof(rt_hit)"]
    args += [f"offsetof(rt_query_ray, {f})" for f in RAY_FIELDS]
    args += [f"offsetof(rt_hit, {f})" for f in HIT_FIELDS]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:2] == [32, 64]
    ray_off, hit_off = got[2:2 + len(RAY_FIELDS)], got[2 + len(RAY_FIELDS):]
    assert ray_off == [getattr(N.rt_query_ray, f).offset for f in RAY_FIELDS]
    assert ray_off == [B.QUERY_RAY.fields[f][1] for f in RAY_FIELDS]
    assert hit_off == [getattr(N.rt_hit, f).offset for f in HIT_FIELDS]
    assert hit_off == [B.HIT.fields[f][1] for f in HIT_FIELDS]
    # laid out for 16-byte vector loads and stores
    assert ray_off[0] == 0 and ray_off[2] == 16
    assert hit_off[HIT_FIELDS.index("normal")] == 16 and hit_off[HIT_FIELDS.index("v")] == 32
    assert hit_off[HIT_FIELDS.index("index")] == 48


def test_header_pins_record_sizes():
    text = HEADER.read_text()
    assert re.search(r"static_assert\(sizeof\(rt_query_ray\) == 32", text)
    assert re.search(r"static_assert\(sizeof\(rt_hit\) == 64", text)
    assert "12, additive: ray queries" in text


def test_null_context_queries_fail_cleanly(native_lib):
    rays = (N.rt_query_ray * 2)()
    hits = (N.rt_hit * 2)()
    assert native_lib.rt_trace_rays(None, rays, hits, 2) == N.RT_E_INVALID
    assert native_lib.rt_trace_rays(None, None, None, 0) == N.RT_E_INVALID
    assert native_lib.rt_trace_rays_device(None, rays, hits, 2) == N.RT_E_INVALID
    assert native_lib.rt_pick(None, 0, 0, hits) == N.RT_E_INVALID


def test_abi_version_unchanged(native_lib):
    assert native_lib.rt_abi_version() == 12
