"""NumPy restatement of the gather contract (rt_gather, rt_gather_device).

Written from the contract in include/rt_abi.h, which the header comment of
rust_gpu_raytracing_amd/csrc/radiance.hip repeats (tests/test_gather_cpu.py checks that the
three copies are equal):

 THE GATHER CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 written order, with no contraction. For point i with record (x, stream, n):
  1. Sample index and origin. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
     o = x + n * 0.0001f per component: one multiply and one add (the reference's bounce
     offset, as restated at oracle/pathtrace_oracle.c:511).
  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
     gx, gy, gz = normal_distribution(&dseed) three times, in that order
     (compute_shader.wgsl:622-628, theta drawn before rho).
     dir = normalize(n + (gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
     dot(v, v) = (x*x + y*y) + z*z. n is used as given and is not normalised.
  3. Path. L_s is the result rt_radiance defines for the record (o, stream, dir) with
     first_sample = u, samples = 1 and the call's bounces: per_pixel with its own seed
     stream * u * 326624u, its own jitter, and everything else of a frame.
  4. Reduction. P_j (j = 0 .. 63) starts at +0.0f on all four channels. For s ascending,
     P_{s mod 64} = P_{s mod 64} + L_s. Then, for off = 32, 16, 8, 4, 2, 1:
     P_j = P_j + P_{j+off} for every j < off. radiance[i] = P_0. Lanes that got no sample
     take part with +0.0f. (An xor butterfly gives the same bits on finite values, because
     f32 addition commutes.)
 End of the gather contract.

Steps 1 and 2 are ``origin`` and ``direction`` (the RNG, the logarithm and the cosine are the
oracle library's own oracle_random, oracle_logf and oracle_cosf), step 3 is a radiance query
record (``records``; ``oracle_lights`` has the oracle answer each), step 4 is ``tree``.
TEST INFRASTRUCTURE ONLY.
"""
import ctypes

import numpy as np

from rust_gpu_raytracing_amd import buffers as B

f32 = np.float32
MASK = 0xFFFFFFFF
F32_MAX = f32(3.4028235e38)
TWO_PI = f32(6.2831850051879883)  # 2.0 * 3.1415926 folded to f32 (compute_shader.wgsl:623)


def _lib():
    from oracle import oracle as O

    return O.lib()


def seed_of(stream, u):
    """per_pixel's seed for the stream and the sample index (:217 with index := stream)."""
    return (int(stream) * int(u) * 326624) & MASK


def normal_distribution(seed):
    """compute_shader.wgsl:622-628 on the ctypes u32 ``seed`` (advanced in place)."""
    L = _lib()
    theta = TWO_PI * f32(L.oracle_random(ctypes.byref(seed)))
    r = L.oracle_random(ctypes.byref(seed))
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.sqrt(f32(-2.0) * f32(L.oracle_logf(r)))
    return f32(rho * f32(L.oracle_cosf(float(theta))))


def lobe(n, seed):
    """normalize(n + (gx, gy, gz)) with the three draws taken from the ctypes u32 ``seed``."""
    n = np.asarray(n, f32)
    g = np.array([normal_distribution(seed) for _ in range(3)], f32)
    v = n + g
    dot = f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (v * (f32(1.0) / np.sqrt(dot))).astype(f32)


def direction(n, stream, u):
    """Step 2: the direction of the sample with index ``u`` of a point with normal ``n``."""
    return lobe(n, ctypes.c_uint32(seed_of(stream, u) ^ 0x9E3779B9))


def origin(x, n):
    """Step 1: x + n * 0.0001f."""
    return (np.asarray(x, f32) + np.asarray(n, f32) * f32(0.0001)).astype(f32)


def records(points, streams, first_sample, samples):
    """The radiance query records of the contract's step 3, sample-major within a point: a
    ``buffers.RADIANCE_RAY`` array of n * samples records (record i * samples + s is sample s of
    point i) and the matching (n * samples,) array of sample indices u."""
    points = np.asarray(points, f32)
    n = points.shape[0]
    rec = np.zeros(n * samples, B.RADIANCE_RAY)
    us = np.zeros(n * samples, np.uint32)
    for i in range(n):
        o = origin(points[i, :3], points[i, 3:])
        for s in range(samples):
            u = (first_sample + s) & MASK
            k = i * samples + s
            rec["origin"][k] = o
            rec["stream"][k] = streams[i]
            rec["direction"][k] = direction(points[i, 3:], streams[i], u)
            us[k] = u
    return rec, us


def tree(lights):
    """Step 4 on ``lights`` (n, samples, 4) f32: the stripes, then the tree. Returns (n, 4)."""
    lights = np.asarray(lights, f32)
    n, samples = lights.shape[:2]
    p = np.zeros((n, 64, 4), f32)
    for s in range(samples):
        p[:, s % 64] = p[:, s % 64] + lights[:, s]
    off = 32
    while off:
        p[:, :off] = p[:, :off] + p[:, off:2 * off]
        off //= 2
    return p[:, 0].copy()


def sequential(lights):
    """The plain ascending sum a radiance query would return: what the contract is NOT."""
    lights = np.asarray(lights, f32)
    acc = np.zeros((lights.shape[0], 4), f32)
    for s in range(lights.shape[1]):
        acc = acc + lights[:, s]
    return acc


def oracle_lights(O, scene, points, streams, bounces, first_sample, samples):
    """(L (n, samples, 4), segments (n,)): the oracle's per_pixel for every record of ``records``
    -- pixel ``stream`` of an oracle whose ray buffer holds the record's direction there and
    whose camera origin is the record's origin, from a zeroed accumulation with accumulate = 1,
    compute_per_frame = 1 and accumulation_index = u."""
    points = np.asarray(points, f32)
    n = points.shape[0]
    rec, us = records(points, streams, first_sample, samples)
    buf = np.zeros(int(np.max(streams)) + 1 if n else 1, B.RAY)
    o = O.Oracle(scene, camera_rays=buf)
    origin_arr, ray_arr = o._arrays["origin"], o._arrays["rays"]  # the arrays the oracle's scene record points to
    params = {}
    lights = np.zeros((n, samples, 4), f32)
    segs = np.zeros(n, np.int64)
    camera_origin = origin_arr.copy()  # (the array may be the scene's own camera position)
    try:
        for k in range(n * samples):
            u = int(us[k])
            if u not in params:
                params[u] = scene.params(accumulate=1, compute_per_frame=1, accumulation_index=u)
            origin_arr[:] = rec["origin"][k]
            ray_arr["direction"][int(rec["stream"][k])] = rec["direction"][k]
            acc, _, cnt = o.render_pixels(params[u], bounces, [int(rec["stream"][k])], threads=1)
            lights[k // samples, k % samples] = acc[0]
            segs[k // samples] += cnt
    finally:
        origin_arr[:] = camera_origin
    return lights, segs


def first_hit_points(O, scene, camera_rays, camera_origin, count):
    """``count`` surface points (position, normal) of the scene: the first hits of camera rays
    spread evenly over the image, from the oracle's own trace_ray."""
    o = O.Oracle(scene)
    p = scene.params(accumulation_index=1)
    d = np.asarray(camera_rays).astype(B.RAY)["direction"]
    org = np.asarray(camera_origin, f32)
    hits = []
    for i in range(d.shape[0]):
        h = o.trace(p, org, d[i])
        if f32(h.t) != F32_MAX:
            hits.append((h.px, h.py, h.pz, h.nx, h.ny, h.nz))
    hits = np.array(hits, f32)
    assert hits.shape[0] >= count, (hits.shape[0], count)
    return hits[np.linspace(0, hits.shape[0] - 1, count).astype(np.int64)].copy()
