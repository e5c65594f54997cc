"""Probe queries without a GPU: the ABI surface (rt_probe, the two entry points, "probe_chunk"), the
three copies of the contract, the NumPy restatement (tests/probe_ref.py) operation by operation, the
distribution of its directions, the package's sh module, and the contract's reduction against a
plain ascending sum.

No kernel launches here; tests/test_gpu_probe.py compares the kernels with the restatement.
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
from tests import gather_ref as G
from tests import host_sources
from tests import probe_ref as P
from tests.golden.fixtures import CASES, load, scene_from_inputs

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
KERNELS = ROOT / "rust_gpu_raytracing_amd" / "csrc" / "radiance.hip"
FUNCTIONS = ("rt_probe_sh", "rt_probe_sh_device")
GOLDEN = {"c1": "c1_64x48_b4", "c2": "c2_64x36_b8", "c3": "c3_64x36_b8"}
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
    assert N.SIGNATURES["rt_probe_sh"] == N.SIGNATURES["rt_gather"]
    assert N.SIGNATURES["rt_probe_sh_device"] == N.SIGNATURES["rt_gather_device"]
    assert native_lib.rt_abi_version() == 12
    assert "12, additive: probe queries" in HEADER.read_text()


def test_probe_layout_against_compiled_header(tmp_path):
    """sizeof and the field offsets of rt_probe from a C program compiled against the real header
    equal the ctypes structure's and the numpy dtype's: 16 bytes, offsets 0 and 12."""
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(rt_probe), offsetof(rt_probe, position), '
                   'offsetof(rt_probe, stream)); return 0;}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [16, 0, 12]
    assert ctypes.sizeof(N.rt_probe) == B.PROBE.itemsize == 16
    assert [N.rt_probe.position.offset, N.rt_probe.stream.offset] == got[1:]
    assert [B.PROBE.fields[f][1] for f in ("position", "stream")] == got[1:]
    assert tuple(f for f, _ in N.rt_probe._fields_) == B.PROBE.names == ("position", "stream")
    assert B.PROBE.fields["stream"][0] == np.dtype("<u4")


def test_null_context_fails_cleanly(native_lib):
    probes = np.zeros(2, B.PROBE)
    out = np.full((2, 9, 4), 3.5, np.float32)
    seg = ctypes.c_uint64(9)
    assert native_lib.rt_probe_sh(None, N.ptr(probes), N.ptr(out), 2, 4, 1, 8, ctypes.byref(seg)) == N.RT_E_INVALID
    assert native_lib.rt_probe_sh_device(None, None, None, 2, 4, 1, 8, None) == N.RT_E_INVALID
    assert (out == 3.5).all() and seg.value == 9


def test_probe_chunk_is_a_tuning_key():
    src = host_sources.TUNING.read_text()
    body = src[src.index("int rt_set_tuning("):]
    assert 'k == "probe_chunk"' in body[:body.index("\n}\n")]
    assert re.search(r"kDefaultProbeChunk = 1048576;", host_sources.CONTEXT.read_text())
    assert '"probe_chunk" 1048576' in HEADER.read_text()


def _contract(path, lead):
    """The probe contract of ``path`` with the comment leader ``lead`` stripped."""
    lines = path.read_text().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith(lead + " THE PROBE CONTRACT."))
    last = next(i for i, l in enumerate(lines) if l.startswith(lead + " End of the probe contract."))
    assert all(l.startswith(lead) for l in lines[first:last + 1])
    return [l[len(lead):].rstrip() for l in lines[first:last + 1]]


def test_contract_text_is_in_header_kernel_source_and_restatement():
    """The contract in include/rt_abi.h equals the header comment of radiance.hip and the docstring
    of tests/probe_ref.py line for line, and the lines the restatement is written from are there."""
    in_header, in_kernels = _contract(HEADER, " *"), _contract(KERNELS, "//")
    in_ref = _contract(Path(P.__file__), "")
    assert in_header == in_kernels == in_ref
    assert len(in_header) == 22
    text = "\n".join(in_header)
    for line in ["u = first_sample + s (u32, wrapping).",
                 "dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).",
                 "gx, gy, gz = normal_distribution(&dseed) three times, in that order",
                 "dir = normalize((gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and",
                 "dot(v, v) = (x*x + y*y) + z*z: a uniform direction on the sphere.",
                 "first_sample = u, samples = 1 and the call's bounces. The origin is x as given (no offset).",
                 "b0 = 0.28209479f                       b1 = 0.48860251f * dy",
                 "b2 = 0.48860251f * dz                  b3 = 0.48860251f * dx",
                 "b4 = 1.09254843f * (dx*dy)             b5 = 1.09254843f * (dy*dz)",
                 "b6 = 0.31539157f * (3.0f*(dz*dz) - 1.0f)",
                 "b7 = 1.09254843f * (dx*dz)             b8 = 0.54627422f * (dx*dx - dy*dy)",
                 "T_{s,k} = L_s * b_k: one multiply per channel, all four channels.",
                 "P_{s mod 64} = P_{s mod 64} + T_{s,k}. Then, for off = 32, 16, 8, 4, 2, 1:",
                 "P_j = P_j + P_{j+off} for every j < off. sh[i][k] = P_0."]:
        assert line in text, line


# ---------------------------------------------------------------------------- the restatement
def test_direction_and_basis_arithmetic(oracle_lib):
    """Steps 2 and 4 on one sample, written out operation by operation."""
    stream, u = 5, 77
    seed = ctypes.c_uint32(((stream * u * 326624) & 0xFFFFFFFF) ^ 0x9E3779B9)
    g = [G.normal_distribution(seed) for _ in range(3)]
    inv = f32(1.0) / np.sqrt(f32(f32(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
    d = P.direction(stream, u)
    assert [d[k] for k in range(3)] == [f32(g[k] * inv) for k in range(3)]
    # with no drawn component +-0 this is the gather direction of a zero normal
    assert d.tobytes() == G.direction(np.zeros(3, f32), stream, u).tobytes()
    assert P.direction(stream, u + 1).tobytes() != d.tobytes()
    assert P.direction(0, 1, nonzero=False).tobytes() == P.direction(0, 2, nonzero=False).tobytes()  # stream 0
    x, y, z = d
    want = [f32(0.28209479),
            f32(f32(0.48860251) * y), f32(f32(0.48860251) * z), f32(f32(0.48860251) * x),
            f32(f32(1.09254843) * f32(x * y)), f32(f32(1.09254843) * f32(y * z)),
            f32(f32(0.31539157) * f32(f32(f32(3.0) * f32(z * z)) - f32(1.0))),
            f32(f32(1.09254843) * f32(x * z)),
            f32(f32(0.54627422) * f32(f32(x * x) - f32(y * y)))]
    b = P.basis(d)
    assert b.dtype == np.float32 and b.shape == (9,)
    assert [b[k] for k in range(9)] == want
    # one multiply per channel
    light = np.array([[[0.3, 1.7, 2.9, 1.0]]], f32)
    t = P.terms(light, d.reshape(1, 1, 3))
    assert t.shape == (1, 1, 9, 4)
    for k in range(9):
        assert [t[0, 0, k, c] for c in range(4)] == [f32(light[0, 0, c] * want[k]) for c in range(4)]


def test_tree_and_sequential_on_known_values():
    """The reduction per coefficient on values whose order of addition shows: 2^24 first and
    sixty-four ones (tests/test_gather_cpu.py has the derivation of 2^24 + 62)."""
    t = np.zeros((1, 65, 9, 4), f32)
    t[0, 0] = 2.0 ** 24
    t[0, 1:] = 1.0
    # coefficient 3 holds other values, to show that the coefficients do not mix
    t[0, :, 3] = 0.5
    seq, tree = P.sequential(t), P.tree(t)
    assert seq.shape == tree.shape == (1, 9, 4)
    others = [k for k in range(9) if k != 3]
    assert (seq[0, others] == 2.0 ** 24).all()
    assert (tree[0, others] == 2.0 ** 24 + 62).all()
    assert (seq[0, 3] == 32.5).all() and (tree[0, 3] == 32.5).all()
    assert not bits(P.tree(np.zeros((2, 5, 9, 4), f32))).any()


def test_directions_are_uniform_on_the_sphere(oracle_lib):
    """Stream 7, u = 1 .. 4096: unit norms to 1e-6, and every entry of (4 pi / N) sum b b^T lies
    within 6 sqrt(2 / N) = 0.133 of the identity. (An entry's variance is at most 8/7 / N, the
    (3 z^2 - 1)^2 term's, so the bound is six standard deviations with room.)"""
    n = 4096
    d = P.directions([7], 1, n)[0]
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    b = P.basis(d).astype(np.float64)
    gram = (4.0 * np.pi / n) * (b.T @ b)
    worst = np.abs(gram - np.eye(9)).max()
    print(f"largest deviation of the Gram matrix from I: {worst:.4f}")
    assert worst <= 6.0 * np.sqrt(2.0 / n)


# ---------------------------------------------------------------------------- the sh module
def _sphere_grid():
    """An 8-node Gauss-Legendre x 16-azimuth grid: directions and weights that integrate
    polynomials of degree 15 over the sphere exactly."""
    z, wz = np.polynomial.legendre.leggauss(8)
    phi = 2.0 * np.pi * np.arange(16) / 16.0
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    dirs = np.stack([r * np.cos(pp), r * np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = (wz[:, None] * np.full(16, 2.0 * np.pi / 16.0)[None, :]).reshape(-1)
    return dirs, w


def test_sh_module_basis_is_orthonormal_and_agrees_with_the_contract():
    import rust_gpu_raytracing_amd as pkg
    from rust_gpu_raytracing_amd import sh

    assert pkg.sh is sh and "sh" in pkg.__all__
    dirs, w = _sphere_grid()
    b = sh.basis(dirs)
    assert b.dtype == np.float64 and b.shape == (128, 9)
    assert np.abs((b * w[:, None]).T @ b - np.eye(9)).max() < 1e-12
    # the contract's f32 basis is this one to f32 precision
    assert np.abs(P.basis(dirs.astype(f32)).astype(np.float64) - b).max() < 1e-6
    with pytest.raises(ValueError):
        sh.basis(np.zeros((4, 2)))


def test_sh_module_radiance_and_irradiance_of_a_linear_field():
    """L(w) = 1 + w . a projected on the grid: radiance gives L back, and irradiance equals
    pi + (2 pi / 3) (a . n), to 1e-12."""
    from rust_gpu_raytracing_amd import sh

    dirs, w = _sphere_grid()
    a = np.array([0.3, -0.5, 0.2])
    field = 1.0 + dirs @ a
    samples = 1000
    # what probe_sh would return for `samples` uniform samples, without noise:
    # sum_s L b_k = samples / (4 pi) * integral of L b_k
    coeff = (samples / (4.0 * np.pi)) * ((field * w) @ sh.basis(dirs))
    probe = np.repeat(coeff[:, None], 4, axis=1)  # (9, 4): the same field on every channel
    normals = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, -0.8], [-1.0, 0.0, 0.0]])
    for n in normals:
        assert np.abs(sh.irradiance(probe, n, samples) - (np.pi + (2.0 * np.pi / 3.0) * (a @ n))).max() < 1e-12
        assert np.abs(sh.radiance(probe, n, samples) - (1.0 + a @ n)).max() < 1e-12
    # batched: (3, 9, 4) against (3, 3)
    many = np.broadcast_to(probe, (3, 9, 4))
    assert sh.irradiance(many, normals, samples).shape == (3, 4)
    assert np.allclose(sh.irradiance(many, normals, samples)[:, 0], np.pi + (2.0 * np.pi / 3.0) * (normals @ a),
                       rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        sh.radiance(np.zeros((8, 4)), normals[0], samples)
    with pytest.raises(ValueError):
        sh.irradiance(probe, normals[0], 0)


# ---------------------------------------------------------------------------- tree against sum
@functools.lru_cache(maxsize=None)
def golden_scene(key):
    g = load(GOLDEN[key])
    return g, CASES[GOLDEN[key]], scene_from_inputs(g)


@functools.lru_cache(maxsize=None)
def positions_of(key, count=24):
    from oracle import oracle as O

    O.build()
    g, _, scene = golden_scene(key)
    pos = P.probe_positions(G.first_hit_points(O, scene, g["camera_rays"], g["camera_origin"], count))
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("key,samples", [("c1", 200), ("c2", 200), ("c3", 200), ("c1", 65), ("c2", 65),
                                         ("c3", 65)])
def test_tree_differs_from_the_sequential_sum(oracle_lib, key, samples):
    """On 24 probes a quarter of a unit off the first-hit points, streams 1..24: the contract's
    reduction and the plain ascending sums of the same terms differ in bits on at least 75% of the
    probes, and at least 90% of the results are non-zero -- a kernel that summed in sample order
    would fail the GPU tests."""
    _, case, scene = golden_scene(key)
    streams = np.arange(1, 25, dtype=np.uint32)
    lights, dirs, segs = P.oracle_probe(oracle_lib, scene, positions_of(key), streams, case["bounces"], 1, samples)
    t = P.terms(lights, dirs)
    tree, seq = P.tree(t), P.sequential(t)
    differ = int((bits(tree) != bits(seq)).reshape(24, -1).any(axis=1).sum())
    nonzero = int(bits(tree).reshape(24, -1).any(axis=1).sum())
    print(f"{key} samples {samples}: {differ}/24 differ, {nonzero}/24 non-zero, {int(segs.sum())} segments")
    assert 4 * differ >= 3 * 24, differ
    assert 10 * nonzero >= 9 * 24, nonzero
    # both orders round each of at most 200 additions to 2^-24 of a partial sum of the |terms|
    assert (np.abs(tree.astype(np.float64) - seq) <= 1e-4 * np.abs(t.astype(np.float64)).sum(axis=1)).all()
