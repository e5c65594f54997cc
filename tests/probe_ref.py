"""NumPy restatement of the probe contract (rt_probe_sh, rt_probe_sh_device).

Written from the contract in include/rt_abi.h, which the header comment of
rust_gpu_raytracing_amd/csrc/radiance.hip repeats (tests/test_probe_cpu.py checks that the
three copies are equal):

 THE PROBE CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 written order, with no contraction. For probe i with record (x, stream):
  1. Sample index. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
     gx, gy, gz = normal_distribution(&dseed) three times, in that order
     (compute_shader.wgsl:622-628, theta drawn before rho).
     dir = normalize((gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
     dot(v, v) = (x*x + y*y) + z*z: a uniform direction on the sphere.
  3. Path. L_s is the result rt_radiance defines for the record (x, stream, dir) with
     first_sample = u, samples = 1 and the call's bounces. The origin is x as given (no offset).
  4. Basis, on dir = (dx, dy, dz) of step 2 (before per_pixel's jitter):
     b0 = 0.28209479f                       b1 = 0.48860251f * dy
     b2 = 0.48860251f * dz                  b3 = 0.48860251f * dx
     b4 = 1.09254843f * (dx*dy)             b5 = 1.09254843f * (dy*dz)
     b6 = 0.31539157f * (3.0f*(dz*dz) - 1.0f)
     b7 = 1.09254843f * (dx*dz)             b8 = 0.54627422f * (dx*dx - dy*dy)
     T_{s,k} = L_s * b_k: one multiply per channel, all four channels.
  5. Reduction, for each k = 0 .. 8 on its own: P_j (j = 0 .. 63) starts at +0.0f. For s ascending,
     P_{s mod 64} = P_{s mod 64} + T_{s,k}. Then, for off = 32, 16, 8, 4, 2, 1:
     P_j = P_j + P_{j+off} for every j < off. sh[i][k] = P_0. Lanes that got no sample take part
     with +0.0f.
 End of the probe contract.

Step 2 is ``direction`` (the draws are tests/gather_ref.py's ``normal_distribution``), step 3 is
a gather point at x with normal (0, 0, 0), which tests/gather_ref.py's ``oracle_lights`` has the
oracle answer: its origin x + 0 * 0.0001f is x and its direction normalize(0 + g) is normalize(g)
wherever no drawn component is +-0, and ``directions`` asserts that on every set it builds. Step 4
is ``basis``, step 5 is ``tree`` (gather_ref's, coefficient by coefficient).
TEST INFRASTRUCTURE ONLY.
"""
import ctypes

import numpy as np

from tests import gather_ref as G

f32 = np.float32
MASK = 0xFFFFFFFF
C0, C1, C2, C20, C22 = f32(0.28209479), f32(0.48860251), f32(1.09254843), f32(0.31539157), f32(0.54627422)


def draws(stream, u):
    """Step 2's three draws (gx, gy, gz) for the stream and the sample index."""
    seed = ctypes.c_uint32(G.seed_of(stream, u) ^ 0x9E3779B9)
    return np.array([G.normal_distribution(seed) for _ in range(3)], f32)


def direction(stream, u, nonzero=True):
    """Step 2. With ``nonzero`` the draws are asserted to be neither +0 nor -0 (the condition
    under which a gather point with a zero normal is the probe)."""
    g = draws(stream, u)
    if nonzero:
        assert (g != 0).all(), (stream, u, g)
    dot = f32(f32(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    return (g * (f32(1.0) / np.sqrt(dot))).astype(f32)


def directions(streams, first_sample, samples):
    """(n, samples, 3): step 2 for every sample of every probe, each draw asserted non-zero."""
    out = np.zeros((len(streams), samples, 3), f32)
    for i, stream in enumerate(streams):
        for s in range(samples):
            out[i, s] = direction(int(stream), (first_sample + s) & MASK)
    return out


def basis(dirs):
    """Step 4 on ``dirs`` (..., 3) f32: (..., 9) f32, every operation one f32 operation."""
    d = np.asarray(dirs, f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = np.empty(d.shape[:-1] + (9,), f32)
    b[..., 0] = C0
    b[..., 1] = C1 * y
    b[..., 2] = C1 * z
    b[..., 3] = C1 * x
    b[..., 4] = C2 * (x * y)
    b[..., 5] = C2 * (y * z)
    b[..., 6] = C20 * (f32(3.0) * (z * z) - f32(1.0))
    b[..., 7] = C2 * (x * z)
    b[..., 8] = C22 * (x * x - y * y)
    return b


def terms(lights, dirs):
    """Step 4's T: ``lights`` (n, samples, 4) and ``dirs`` (n, samples, 3) give (n, samples, 9, 4)."""
    return (np.asarray(lights, f32)[:, :, None, :] * basis(dirs)[:, :, :, None]).astype(f32)


def tree(t):
    """Step 5 on T (n, samples, 9, 4): (n, 9, 4)."""
    return np.stack([G.tree(t[:, :, k]) for k in range(9)], axis=1)


def sequential(t):
    """The plain ascending sums: what the contract is NOT."""
    return np.stack([G.sequential(t[:, :, k]) for k in range(9)], axis=1)


def gather_points(positions):
    """The gather points that stand for the probes: (n, 6), normal (0, 0, 0)."""
    positions = np.asarray(positions, f32)
    return np.concatenate([positions, np.zeros_like(positions)], axis=1)


def probe_positions(points, distance=0.25):
    """Points in free space from surface points (position, normal): x + n * distance in f32."""
    points = np.asarray(points, f32)
    return (points[:, :3] + points[:, 3:] * f32(distance)).astype(f32)


def oracle_probe(O, scene, positions, streams, bounces, first_sample, samples):
    """(lights (n, samples, 4), dirs (n, samples, 3), segments (n,)): steps 1 to 3 with the oracle's
    per_pixel answering every path."""
    dirs = directions(streams, first_sample, samples)  # (asserts the draws non-zero)
    lights, segs = G.oracle_lights(O, scene, gather_points(positions), streams, bounces, first_sample, samples)
    return lights, dirs, segs
