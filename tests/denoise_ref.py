"""References for the feature buffers and the guided a-trous filter (rt_compute_features, rt_denoise).

Written from the contract in the header comment of rust_gpu_raytracing_amd/csrc/denoise.hip (the
same text as include/rt_abi.h), not from the kernel:

* ``filter_ref``: a NumPy float32 restatement of the filter, one ufunc per written operation (NumPy
  never fuses a multiply with an add), skipped taps selected with ``np.where`` -- never multiplied
  by zero.
* ``oracle_features``: the two feature planes built with ``Oracle.trace`` per pixel and the
  samplers restated with the oracle's own sRGB table, atan2 and asin.

Shared by tests/test_denoise_cpu.py and tests/test_gpu_denoise.py; results are cached per scene by
the callers and never modified.
"""
import ctypes
import functools

import numpy as np

f32 = np.float32
F32_MAX = f32(3.4028235e38)
WGSL_PI = f32(3.1415926536)  # compute_shader.wgsl:3
DEFAULTS = dict(iterations=4, sigma_color=1.0, sigma_albedo=0.1, sigma_depth=0.05)
H5 = (f32(1.0 / 16.0), f32(1.0 / 4.0), f32(3.0 / 8.0), f32(1.0 / 4.0), f32(1.0 / 16.0))


# ------------------------------------------------------------------------------------- the filter
def clamp01(x):
    return np.minimum(np.maximum(x, f32(0.0)), f32(1.0))


def pack_rgba8(c):
    """pack_to_u32 (compute_shader.wgsl:192-208): truncating, byte i = channel i."""
    b = (c * f32(255.0)).astype(np.uint32) & np.uint32(0xFF)
    return b[..., 0] | (b[..., 1] << np.uint32(8)) | (b[..., 2] << np.uint32(16)) | (b[..., 3] << np.uint32(24))


def _pass(c, normal, depth, albedo, hit, step, k_a, k_c, sigma_depth):
    h, w = depth.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    num = np.zeros((h, w, 4), f32)
    den = np.zeros((h, w), f32)
    hit_p = hit != 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            hh = H5[dy + 2] * H5[dx + 2]
            if dx == 0 and dy == 0:
                num = num + hh * c
                den = den + hh
                continue
            qy, qx = ys + step * dy, xs + step * dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            n_q, z_q, a_q, c_q, hit_q = normal[qy, qx], depth[qy, qx], albedo[qy, qx], c[qy, qx], hit[qy, qx] != 0
            d = np.maximum(f32(0.0), (normal[..., 0] * n_q[..., 0] + normal[..., 1] * n_q[..., 1])
                           + normal[..., 2] * n_q[..., 2])
            d2 = d * d
            d4 = d2 * d2
            d8 = d4 * d4
            d16 = d8 * d8
            wn = d16 * d16
            x = np.abs(depth - z_q) / (sigma_depth * (depth + z_q) + f32(1e-30))
            wz = f32(1.0) / (f32(1.0) + x * x)
            g = np.where(~hit_p & ~hit_q, f32(1.0), np.where(hit_p != hit_q, f32(0.0), wn * wz)).astype(f32)
            da = albedo - a_q
            xa = ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * k_a
            ra = f32(1.0) / (f32(1.0) + xa)
            dc = c[..., :3] - c_q[..., :3]
            xc = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * k_c
            rc = f32(1.0) / (f32(1.0) + xc)
            wgt = ((hh * g) * (ra * ra)) * (rc * rc)
            take = inside & (wgt > 0)  # false for NaN
            num = np.where(take[..., None], num + wgt[..., None] * c_q, num)
            den = np.where(take, den + wgt, den)
    for a in (num, den):
        assert a.dtype == f32
    return num / den[..., None]


def filter_ref(acc, feats, k, compute_per_frame, iterations=None, sigma_color=None, sigma_albedo=None,
               sigma_depth=None):
    """(rgba_f32 (H, W, 4), rgba8 (H, W) uint32) of rt_denoise for the accumulation ``acc`` at
    accumulation counter ``k`` (the value rt_accumulation_index reports) and the feature dict ``feats``."""
    it = DEFAULTS["iterations"] if iterations is None else int(iterations)
    sc = f32(DEFAULTS["sigma_color"] if sigma_color is None else sigma_color)
    sa = f32(DEFAULTS["sigma_albedo"] if sigma_albedo is None else sigma_albedo)
    sd = f32(DEFAULTS["sigma_depth"] if sigma_depth is None else sigma_depth)
    n_samples = np.uint32((int(k) - 1) * int(compute_per_frame) & 0xFFFFFFFF)
    acc = np.asarray(acc)
    assert acc.dtype == f32
    normal, depth = feats["normal"].astype(f32, copy=False), feats["depth"].astype(f32, copy=False)
    albedo, hit = feats["albedo"].astype(f32, copy=False), feats["hit"].astype(f32, copy=False)
    with np.errstate(all="ignore"):
        c = acc / f32(n_samples)
        s0 = sc / np.sqrt(f32(n_samples))
        k_a = f32(1.0) / (sa * sa)
        for i in range(it):
            s_i = s0 * f32(0.5 ** i)
            k_c = f32(1.0) / (s_i * s_i)
            c = _pass(c, normal, depth, albedo, hit, 1 << i, k_a, k_c, sd)
            assert c.dtype == f32
        return c, pack_rgba8(clamp01(c))


# ------------------------------------------------------------------------------------- the features
def _texel_coord(c, size):
    """Truncate toward zero, clamp to [0, size-1]; NaN -> 0 (compute_shader.wgsl:26-40, naga Restrict)."""
    if not (c >= 0):
        return 0
    if c >= f32(size):
        return size - 1
    return min(int(c), size - 1)


def oracle_features(O, scene, camera_rays=None):
    """The feature planes of ``scene`` from the CPU oracle: per pixel ``Oracle.trace`` of the camera
    origin and the pixel's ray-buffer direction, then sample_texture / the environment lookup."""
    L = O.lib()
    o = O.Oracle(scene, camera_rays=camera_rays)
    p = scene.params(accumulation_index=1)
    srgb = np.zeros(256, f32)
    L.oracle_srgb_table(srgb.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    w, h = o.width, o.height
    dirs = np.ascontiguousarray(o._arrays["rays"]["direction"], f32).reshape(h * w, 3)
    origin = np.ascontiguousarray(scene.camera.position, f32)
    mats = np.ascontiguousarray(scene.materials)
    tex = np.ascontiguousarray(scene.textures, np.uint8)
    env = np.ascontiguousarray(scene.environment_map, np.uint8)
    layers, th, tw = tex.shape[:3]
    eh, ew = env.shape[:2]
    ptw, pth = f32(np.int32(p["texture_width"])), f32(np.int32(p["texture_height"]))
    pew, peh = f32(np.int32(p["env_map_width"])), f32(np.int32(p["env_map_height"]))
    normal = np.zeros((h * w, 3), f32)
    depth = np.zeros(h * w, f32)
    albedo = np.zeros((h * w, 3), f32)
    hit = np.zeros(h * w, f32)
    for i in range(h * w):
        d = dirs[i]
        r = o.trace(p, origin, d)
        depth[i] = r.t
        if f32(r.t) == F32_MAX:
            u = f32(0.5) + f32(L.oracle_atan2f(d[2], d[0])) / (f32(2.0) * WGSL_PI)
            v = f32(0.5) + f32(L.oracle_asinf(d[1])) / WGSL_PI
            t = env[_texel_coord(v * peh, eh), _texel_coord(u * pew, ew)]
        else:
            normal[i] = (r.nx, r.ny, r.nz)
            hit[i] = 1.0
            mi = min(int(r.material_index), mats.shape[0] - 1)
            layer = min(int(mats["texture_index"][mi]), layers - 1)
            t = tex[layer, _texel_coord(f32(r.v) * pth, th), _texel_coord(f32(r.u) * ptw, tw)]
        albedo[i] = srgb[t[:3]]
    return {"normal": normal.reshape(h, w, 3), "depth": depth.reshape(h, w), "albedo": albedo.reshape(h, w, 3),
            "hit": hit.reshape(h, w)}


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(golden arrays, case, scene, oracle features) of a committed golden fixture, computed once."""
    from oracle import oracle as O
    from rust_gpu_raytracing_amd import buffers as B
    from tests.golden.fixtures import CASES, load, scene_from_inputs

    O.build()
    g = load(name)
    scene = scene_from_inputs(g)
    feats = oracle_features(O, scene, camera_rays=np.asarray(g["camera_rays"]).astype(B.RAY))
    return g, CASES[name], scene, feats


def planes(feats):
    """The two float4 planes (normal.xyz, t) and (albedo.rgb, hit) of a feature dict."""
    nd = np.concatenate([feats["normal"], feats["depth"][..., None]], axis=-1).astype(f32)
    ah = np.concatenate([feats["albedo"], feats["hit"][..., None]], axis=-1).astype(f32)
    return np.ascontiguousarray(nd), np.ascontiguousarray(ah)
