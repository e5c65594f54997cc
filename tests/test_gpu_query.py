"""Ray queries (rt_trace_rays, rt_trace_rays_device, rt_pick) against the CPU oracle.

Every record is compared bit for bit with ``Oracle.trace`` (t, position, normal, u, v,
material_index, front_face: bytes 0-43 of the 64; ``_reserved`` is 0), and the identity fields
(kind, index, sub_object, triangle) are checked against what the oracle can say about them:
which of its two sweeps won, the one-sphere scene, the triangle's ranges and face normal.

Rays: camera rays (coherent) and the rays the oracle logs while rendering the same scene (the
real bounce distribution, rays starting on surfaces included), a third of the logged directions
scaled by factors in [0.25, 4]. References are computed once per scene and shared.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests.golden.fixtures import CASES, load, scene_from_inputs

pytestmark = pytest.mark.gpu

F32_MAX = np.float32(3.4028235e38)
N_CAMERA, N_LOGGED = 200, 450  # rays per scene: 650 rays x 3 oracle traces


# ---------------------------------------------------------------------------- rays and references
def camera_rays(scene, n):
    d = scene.camera.recalculate_ray_directions()["direction"]
    pick = np.linspace(0, d.shape[0] - 1, n).astype(np.int64)
    out = np.zeros((n, 6), np.float32)
    out[:, :3] = np.asarray(scene.camera.position, np.float32)
    out[:, 3:] = d[pick]
    return out


def logged_rays(O, scene, bounces, n, seed=7, stride=3):
    """``n`` of the rays the oracle traces while rendering the scene (one thread, trace log on),
    every third direction scaled by a factor in [0.25, 4]."""
    o = O.Oracle(scene)
    pixels = np.arange(0, o.width * o.height, stride, dtype=np.uint32)
    cap = len(pixels) * (bounces + 1)
    log = np.zeros((cap, 6), np.float32)
    O.lib().oracle_set_trace_log(log.ctypes.data, cap)
    try:
        _, _, rays = o.render_pixels(scene.params(accumulation_index=1), bounces, pixels, threads=1)
        got = int(O.lib().oracle_trace_log_count())
    finally:
        O.lib().oracle_set_trace_log(None, 0)
    assert got == rays and got >= n, (got, rays, n)
    rng = np.random.default_rng(seed)
    out = log[np.sort(rng.choice(got, n, replace=False))].copy()
    scale = np.exp2(rng.uniform(-2.0, 2.0, n)).astype(np.float32)
    out[::3, 3:] *= scale[::3, None]
    return out


def oracle_records(O, scene, rays):
    """Per ray: the first 44 bytes of the expected record, and the distances of the oracle's two
    sweeps on their own (spheres only, triangles only)."""
    o = O.Oracle(scene)
    p = scene.params(accumulation_index=1)
    p_sph, p_tri = p.copy(), p.copy()
    p_sph["object_count"] = 0
    p_tri["sphere_count"] = 0
    n = rays.shape[0]
    rec = np.zeros(n, B.HIT)
    hs_t = np.full(n, F32_MAX, np.float32)
    ht_t = np.full(n, F32_MAX, np.float32)
    for i in range(n):
        h = o.trace(p, rays[i, :3], rays[i, 3:])
        rec["t"][i] = h.t
        rec["position"][i] = (h.px, h.py, h.pz)
        rec["normal"][i] = (h.nx, h.ny, h.nz)
        rec["u"][i], rec["v"][i] = h.u, h.v
        rec["material_index"][i] = h.material_index
        rec["front_face"][i] = h.front_face
        if scene.spheres.shape[0]:
            hs_t[i] = o.trace(p_sph, rays[i, :3], rays[i, 3:]).t
        if scene.objects:
            ht_t[i] = o.trace(p_tri, rays[i, :3], rays[i, 3:]).t
    return dict(rec=rec, hs_t=hs_t, ht_t=ht_t)


def check_hits(O, scene, rays, hits, ref, geometry=None):
    """``hits`` against the oracle reference ``ref`` of the same rays. ``geometry``: (objects,
    sub-objects, triangles) as the device holds them, when not the scene's own."""
    n = rays.shape[0]
    assert hits.shape == (n,) and hits.dtype == B.HIT
    got = hits.view(np.uint8).reshape(n, 64)
    want = ref["rec"].view(np.uint8).reshape(n, 64)
    bad = np.nonzero((got[:, :44] != want[:, :44]).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], hits[bad[:3]], ref["rec"][bad[:3]])
    assert not hits["_reserved"].any()
    # kind: the sphere sweep wins iff strictly closer (compute_shader.wgsl:347)
    hs, ht = ref["hs_t"], ref["ht_t"]
    with np.errstate(invalid="ignore"):
        sphere = hs < ht
    kind = np.where(sphere, 1, np.where(ht.view(np.uint32) != F32_MAX.view(np.uint32), 2, 0)).astype(np.uint32)
    assert np.array_equal(hits["kind"], kind), np.nonzero(hits["kind"] != kind)[0][:5]
    miss = kind == 0
    for f in ("index", "sub_object", "triangle"):
        assert not hits[f][miss].any()
    assert np.array_equal(hits["t"][miss].view(np.uint32), np.full(miss.sum(), F32_MAX).view(np.uint32))
    # sphere hits: the scene cut down to that one sphere gives the same distance
    sph = np.nonzero(kind == 1)[0]
    assert not hits["sub_object"][sph].any() and not hits["triangle"][sph].any()
    if sph.size:
        spheres = np.ascontiguousarray(scene.spheres)
        assert (hits["index"][sph] < spheres.shape[0]).all()
        assert np.array_equal(hits["material_index"][sph], spheres["material_index"][hits["index"][sph]])
        cut = O.Oracle(scene)
        p1 = scene.params(accumulation_index=1)
        p1["object_count"] = 0
        p1["sphere_count"] = 1
        for i in sph:
            cut._s.spheres = spheres.ctypes.data + B.SPHERE.itemsize * int(hits["index"][i])
            h = cut.trace(p1, rays[i, :3], rays[i, 3:])
            assert np.float32(h.t).view(np.uint32) == hits["t"][i:i + 1].view(np.uint32)[0], (i, h.t, hits[i])
    # triangle hits: ranges, face normal, material
    tri = np.nonzero(kind == 2)[0]
    if tri.size:
        objs, subs, tris = geometry if geometry is not None else scene.flatten()
        oi, si, ti = hits["index"][tri], hits["sub_object"][tri], hits["triangle"][tri]
        assert (oi < objs.shape[0]).all() and (si < subs.shape[0]).all() and (ti < tris.shape[0]).all()
        first_t, n_t = subs["first_triangle_index"][si], subs["triangle_count"][si]
        assert ((ti >= first_t) & (ti - first_t < n_t)).all()
        first_s, n_s = objs["first_sub_object_index"][oi], objs["sub_object_count"][oi]
        assert ((si >= first_s) & (si - first_s < n_s)).all()
        assert np.array_equal(hits["material_index"][tri], objs["material_index"][oi])
        fn = tris["face_normal"][ti].astype(np.float32)
        nrm = hits["normal"][tri]
        same = (nrm.view(np.uint32) == fn.view(np.uint32)).all(axis=1)
        flip = (nrm.view(np.uint32) == (-fn).view(np.uint32)).all(axis=1)
        front = hits["front_face"][tri] == 1  # front face: +face_normal, else -face_normal
        assert np.where(front, same, flip).all()


SCENES = {
    "c1": ("c1_four_spheres", dict(width=37, height=21)),
    "c2": ("c2_rtiow", dict(width=64, height=36)),
    "c3": ("c3_chess", dict(width=64, height=36, env_size=(1024, 512))),
    "c4": ("c4_mixed", dict(width=64, height=36)),
    "c5": ("c5_heightfield", dict(width=64, height=36, nx=160, nz=80)),
}


@functools.lru_cache(maxsize=None)
def reference(key):
    """(scene, rays, oracle reference) of one scene, computed once and shared (never modified)."""
    from oracle import oracle as O

    O.build()
    config, kw = SCENES[key]
    scene, bounces = build_config(config, **kw)
    if key == "c1":  # 777 rays: the counts of test_c1_wave_edges are prefixes of one set
        rays = np.concatenate([camera_rays(scene, 260), logged_rays(O, scene, bounces, 517, stride=1)])
        rays = rays[np.random.default_rng(1).permutation(rays.shape[0])]
    else:
        rays = np.concatenate([camera_rays(scene, N_CAMERA), logged_rays(O, scene, max(bounces, 8), N_LOGGED)])
    ref = oracle_records(O, scene, rays)
    t = ref["rec"]["t"]
    assert (t == F32_MAX).any() and (t != F32_MAX).any(), "the ray set must hold hits and misses"
    return scene, rays, ref


def take(ref, n):
    return {k: v[:n] for k, v in ref.items()}


# ---------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("count", [1, 63, 64, 65, 777])
def test_c1_wave_edges(gpu, oracle_lib, count):
    """Sphere-only instance; counts at the wave edges, the refill and the tail. uv is compared:
    the 1x1-texture case in which the path kernel's trace_end skips it."""
    scene, rays, ref = reference("c1")
    # 1x1 texture layers (no texel depends on uv): a trace result does not read the textures
    flat = dataclasses.replace(scene, textures=np.ascontiguousarray(scene.textures[:, :1, :1]))
    assert flat.texture_size == (1, 1)
    with Renderer(flat) as r:
        hits = r.trace_rays(rays[:count])
    check_hits(oracle_lib, scene, rays[:count], hits, take(ref, count))
    if count == 777:
        sph = hits["kind"] == 1
        assert sph.any() and (hits["u"][sph] != 0).any() and (hits["v"][sph] != 0).any()


@pytest.mark.parametrize("mode", [0, 1, -1])
def test_c2_sphere_bvh(gpu, oracle_lib, mode):
    """Sphere BVH plus the brute-force set, in the forced placements and the automatic one."""
    scene, rays, ref = reference("c2")
    assert scene.texture_size == (1, 1)  # the path kernel skips uv here; a query returns it
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        hits = r.trace_rays(rays)
    check_hits(oracle_lib, scene, rays, hits, ref)
    assert (hits["u"][hits["kind"] == 1] != 0).any()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles_in_lds(gpu, oracle_lib, mode):
    """The LDS-resident triangle walk (mode 2) and the global-memory walks, non-1x1 textures."""
    scene, rays, ref = reference("c3")
    assert scene.texture_size != (1, 1)
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        hits = r.trace_rays(rays)
    check_hits(oracle_lib, scene, rays, hits, ref)
    assert (hits["kind"] == 2).any()


def test_c4_spheres_and_triangles(gpu, oracle_lib):
    """Both kinds in one scene: a sphere wins only if strictly closer."""
    scene, rays, ref = reference("c4")
    with Renderer(scene) as r:
        hits = r.trace_rays(rays)
    check_hits(oracle_lib, scene, rays, hits, ref)
    assert (hits["kind"] == 1).any() and (hits["kind"] == 2).any()


def test_c5_global_walk_pruning_modes(gpu, oracle_lib):
    """The global-memory walk (quantized nodes, leaf certificates, cooperative batches): pruning
    modes 0 and 1 give the same bytes, the oracle's."""
    scene, rays, ref = reference("c5")
    got = []
    for prune in (1, 0):
        with Renderer(scene, tuning={"query_lds_mode": 1}) as r:
            r.set_triangle_pruning(prune)
            got.append(r.trace_rays(rays))
    assert got[0].tobytes() == got[1].tobytes()
    check_hits(oracle_lib, scene, rays, got[0], ref)
    assert (got[0]["kind"] == 2).any()


def test_grazing_rays_certified_pruning(gpu, oracle_lib):
    """500 rays within 1e-6..1e-3 rad of a tilted plane of triangles that passes 1e-4..1e-2 from
    their origins (tests/adversarial.py): the certified walk returns the sweep's triangle."""
    from tests.adversarial import grazing_rays, tilted_plane_grid

    scene, _ = build_config("c1_four_spheres", width=32, height=24)
    _, _, _, obj, frame = tilted_plane_grid(3, n=40, size=0.1)
    scene.objects = [obj]
    rays = grazing_rays(frame, 500, (1e-4, 1e-2), (1e-6, 1e-3), 13, span=1.5).astype(np.float32)
    ref = oracle_records(oracle_lib, scene, rays)
    assert (ref["ht_t"] != F32_MAX).sum() > 50
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            hits = r.trace_rays(rays)
        check_hits(oracle_lib, scene, rays, hits, ref)


def test_identical_spheres_first_wins(gpu, oracle_lib):
    """Two identical spheres at indices 0 and 1: the reference's sweep keeps the first."""
    scene, _ = build_config("c1_four_spheres", width=32, height=24)
    scene.spheres = np.ascontiguousarray(scene.spheres.copy())
    scene.spheres[1] = scene.spheres[0]
    c = scene.spheres["position"][0].astype(np.float32)
    rng = np.random.default_rng(3)
    rays = np.zeros((64, 6), np.float32)
    rays[:, :3] = c + np.float32(3.0) * scene.spheres["radius"][0] * rng.standard_normal((64, 3)).astype(np.float32)
    rays[:, 3:] = c - rays[:, :3] + np.float32(0.05) * rng.standard_normal((64, 3)).astype(np.float32)
    ref = oracle_records(oracle_lib, scene, rays)
    with Renderer(scene) as r:
        hits = r.trace_rays(rays)
    check_hits(oracle_lib, scene, rays, hits, ref)
    r0 = scene.spheres["radius"][0]
    on_it = np.abs(np.linalg.norm(hits["position"] - c, axis=1) - r0) < 1e-3 * r0
    assert on_it.sum() > 20
    assert (hits["kind"][on_it] == 1).all() and (hits["index"][on_it] == 0).all()


# ---------------------------------------------------------------------------- semantics
@pytest.mark.parametrize("batch", [None, 1])
def test_queries_do_not_disturb_a_render(gpu, batch):
    """The golden case c2_64x36_b8 with a 100-ray query between the compute_frame calls, with the
    default frame queue and with one launch per frame: accumulation, output and ray count equal
    the golden's, and a queued frame stays queued."""
    name = "c2_64x36_b8"
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    rays = reference("c2")[1][:100]
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                hits = r.trace_rays(rays)
                assert (r.frame_batch(), r.accumulation_index) == before
                if batch is None:
                    assert before[0][1] == i + 1  # the frames so far are still queued
        acc, out, n = r.read_accumulation(), r.read_output(), r.ray_count()
    assert hits.shape == (100,)
    assert n == int(g["rays"])
    assert np.array_equal(out, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_chunking_and_device_entry_point(gpu):
    """10,000 rays staged in chunks of 4,096 equal the default run; the device entry point
    (torch tensor in, torch tensor out) equals the host one."""
    import torch

    scene, rays, _ = reference("c4")
    rng = np.random.default_rng(5)
    big = rays[rng.integers(0, rays.shape[0], 10_000)].copy()
    big[:, :3] += (1e-3 * rng.standard_normal((10_000, 3))).astype(np.float32)
    with Renderer(scene) as r:
        base = r.trace_rays(big)
        r.set_tuning("query_chunk", 4096)
        chunked = r.trace_rays(big)
        q = np.zeros(big.shape[0], B.QUERY_RAY)
        q["origin"], q["direction"] = big[:, :3], big[:, 3:]
        assert r.trace_rays(q).tobytes() == base.tobytes()
        t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(gpu)
        dev = r.trace_rays(t)
        assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (10_000, 16)
        dev_host = dev.cpu().numpy()
    assert (base["kind"] != 0).any() and (base["kind"] == 0).any()
    assert chunked.tobytes() == base.tobytes()
    assert dev_host.tobytes() == base.tobytes()


@pytest.mark.parametrize("device_rays", [False, True])
def test_pick(gpu, oracle_lib, device_rays):
    """pick(x, y) at the four corners and 50 random pixels of C3 == Oracle.trace of the camera
    origin and that pixel's direction; with rt_update_camera_matrices the direction is the host
    generator's (test_gpu_device_camera_rays shows the device's to be bit-equal)."""
    scene, _, _ = reference("c3")
    w, h = scene.camera.viewport_width, scene.camera.viewport_height
    d = scene.camera.recalculate_ray_directions()["direction"]
    rng = np.random.default_rng(9)
    px = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + \
        [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 50), rng.integers(0, h, 50))]
    rays = np.zeros((len(px), 6), np.float32)
    rays[:, :3] = np.asarray(scene.camera.position, np.float32)
    rays[:, 3:] = [d[y * w + x] for x, y in px]
    ref = oracle_records(oracle_lib, scene, rays)
    with Renderer(scene, device_rays=device_rays) as r:
        hits = np.stack([r.pick(x, y) for x, y in px]).astype(B.HIT)
        with pytest.raises(RtError) as e:
            r.pick(w, 0)
        assert e.value.code == N.RT_E_INVALID
        with pytest.raises(RtError):
            r.pick(0, h)
    check_hits(oracle_lib, scene, rays, hits, ref)


def test_live_edit(gpu, oracle_lib):
    """After rt_update_objects moves one chess piece, queries equal the oracle on the edited
    scene (the pattern of test_gpu_device_scene_edit)."""
    from rust_gpu_raytracing_amd import builder

    scene, bounces = build_config("c3_chess", width=64, height=36, env_size=(1024, 512))
    rays = reference("c3")[1][:400]
    with Renderer(scene) as r:
        before = r.trace_rays(rays)
        hit_objects = before["index"][before["kind"] == 2]
        o = scene.objects[int(np.bincount(hit_objects).argmax())]  # the piece most rays hit
        o.rotation = np.array([0.0, 35.0, 0.0], np.float32)
        o.transformation = (np.asarray(o.transformation) + np.array([0.3, 0.0, -0.2])).astype(np.float32)
        r.update_objects()
        hits = r.trace_rays(rays)
        geo = r.read_geometry()
    for ob in scene.objects:
        builder.update_object(ob)
    objs, subs, tris = scene.flatten()
    assert geo[2].tobytes() == tris.tobytes()
    ref = oracle_records(oracle_lib, scene, rays)
    check_hits(oracle_lib, scene, rays, hits, ref, geometry=(objs, subs, tris))
    assert before.tobytes() != hits.tobytes()  # the edit is visible to the rays


def test_errors(gpu):
    scene, rays, _ = reference("c1")
    with Renderer(scene) as r:
        lib, ctx = r._lib, r._ctx
        q = np.zeros(4, B.QUERY_RAY)
        hits = np.zeros(4, B.HIT)
        assert lib.rt_trace_rays(ctx, None, N.ptr(hits), 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_trace_rays(ctx, N.ptr(q), None, 4) == N.RT_E_INVALID
        assert lib.rt_trace_rays(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_trace_rays_device(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_trace_rays_device(ctx, None, None, 4) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_trace_rays_device(ctx, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(hits.ctypes.data),
                                        4) == N.RT_E_INVALID
        one = np.zeros(1, B.HIT)
        assert lib.rt_pick(ctx, r.width, 0, N.ptr(one)) == N.RT_E_INVALID
        assert lib.rt_pick(ctx, 0, 0, None) == N.RT_E_INVALID
        assert r.trace_rays(np.zeros((0, 6), np.float32)).shape == (0,)
