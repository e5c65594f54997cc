"""Occlusion queries (rt_occluded, rt_occluded_device) against the CPU oracle.

A ray is occluded iff some primitive is accepted by the reference's own test at a distance
t < t_max (strict, f32). For a ray set whose oracle distances hold no NaN that is
``hit and t_closest < t_max``, so every byte is checked against ``Oracle.trace``'s distance. The
sharp pair is t_max = t (0) and t_max = nextafter(t) (1): it fails if the culling by t_max loses the
closest primitive or accepts a farther one.

The ray sets and oracle references are those of tests/test_gpu_query.py (computed once, shared).
"""
import ctypes

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.test_gpu_query import oracle_records, reference

pytestmark = pytest.mark.gpu

F32_MAX = np.float32(3.4028235e38)
INF = np.float32(np.inf)


# ---------------------------------------------------------------------------- expected bytes
def expected(t, t_max):
    """The definition on oracle distances without NaN: a hit strictly before t_max."""
    assert not np.isnan(t).any()
    with np.errstate(invalid="ignore"):
        return ((t != F32_MAX) & (t < t_max)).astype(np.uint8)


def next_up(t):
    with np.errstate(over="ignore"):  # (past F32_MAX: +inf)
        return np.nextafter(t, INF, dtype=np.float32)


def variants(rays, t):
    """One batch of (n, 7) rays holding every variant of the table for the set (rays, oracle
    distances t), and its expected bytes."""
    assert not np.isnan(t).any()
    hit = np.nonzero(t != F32_MAX)[0]
    miss = np.nonzero(t == F32_MAX)[0]
    every = np.arange(t.shape[0])
    assert hit.size and miss.size
    th = t[hit]
    assert (th > 0).all() and (th / 2 < th).all() and (th * 2 > th).all()
    one = np.ones(1, np.float32)
    table = [
        (hit, th, 0), (hit, next_up(th), 1), (hit, th / np.float32(2), 0), (hit, th * np.float32(2), 1),
        (hit, INF * one, 1), (hit, F32_MAX * one, 1),
        (miss, one, 0), (miss, INF * one, 0), (miss, F32_MAX * one, 0),
        (every, 0 * one, 0), (every, -one, 0), (every, np.float32(np.nan) * one, 0),
    ]
    parts, want = [], []
    for idx, t_max, byte in table:
        part = np.zeros((idx.size, 7), np.float32)
        part[:, :6] = rays[idx]
        part[:, 6] = t_max
        parts.append(part)
        want.append(np.full(idx.size, byte, np.uint8))
        # the table's byte is the definition's
        assert np.array_equal(expected(t[idx], part[:, 6]), want[-1])
    batch, want = np.concatenate(parts), np.concatenate(want)
    order = np.random.default_rng(17).permutation(batch.shape[0])  # the variants of a ray in different waves
    return batch[order], want[order]


def check(out, want):
    assert out.dtype == np.uint8 and out.shape == want.shape
    assert set(np.unique(out)) <= {0, 1}
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, (bad.size, bad[:8], out[bad[:8]], want[bad[:8]])


def check_variants(r, rays, t):
    batch, want = variants(rays, t)
    out = r.occluded(batch)
    check(out, want)
    return batch, out


# ---------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("count", [1, 63, 64, 65, 777])
def test_c1_wave_edges(gpu, count):
    """Sphere-only instance; counts at the wave edges, the refill and the tail, t_max alternating
    between t (0) and nextafter(t) (1). No byte outside the result is written: guard bytes around
    the host result, and a device result at byte offsets 0 and 3 of a larger tensor (unaligned,
    neighbours sharing a dword)."""
    import torch

    scene, rays, ref = reference("c1")
    t = ref["rec"]["t"][:count]
    assert not np.isnan(t).any()
    q = np.zeros(count, B.OCCLUSION_RAY)
    q["origin"], q["direction"] = rays[:count, :3], rays[:count, 3:]
    q["t_max"] = np.where(t == F32_MAX, INF, np.where(np.arange(count) % 2 == 0, t, next_up(t)))
    want = expected(t, q["t_max"])
    if count == 777:
        hit = t != F32_MAX
        assert (want[hit] == 1).sum() > 50 and (want[hit] == 0).sum() > 50
    with Renderer(scene) as r:
        lib, ctx = r._lib, r._ctx
        buf = np.full(count + 128, 0xAA, np.uint8)
        assert lib.rt_occluded(ctx, N.ptr(q), ctypes.c_void_p(buf.ctypes.data + 64), count) == N.RT_OK
        check(buf[64:64 + count].copy(), want)
        assert (buf[:64] == 0xAA).all() and (buf[64 + count:] == 0xAA).all()
        d_rays = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(gpu)
        for off in (0, 3):
            big = torch.full((count + 64,), 0xAA, dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            assert lib.rt_occluded_device(ctx, ctypes.c_void_p(d_rays.data_ptr()),
                                          ctypes.c_void_p(big.data_ptr() + off), count) == N.RT_OK
            r.synchronize()
            got = big.cpu().numpy()
            check(got[off:off + count].copy(), want)
            assert (got[:off] == 0xAA).all() and (got[off + count:] == 0xAA).all()


@pytest.mark.parametrize("mode", [0, 1, -1])
def test_c2_sphere_bvh(gpu, mode):
    """Sphere BVH plus the brute-force set, in the forced placements and the automatic one."""
    scene, rays, ref = reference("c2")
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        check_variants(r, rays, ref["rec"]["t"])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles_in_lds(gpu, mode):
    """The LDS-resident triangle walk (mode 2, box culling and the early exit only) and the
    global-memory walks (leaf certificates seeded with t_max)."""
    scene, rays, ref = reference("c3")
    assert (ref["hs_t"] < ref["ht_t"]).any() and (ref["ht_t"] < ref["hs_t"]).any()
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        check_variants(r, rays, ref["rec"]["t"])


def test_c4_spheres_and_triangles(gpu):
    """Both kinds in one scene, and both decide some rays."""
    scene, rays, ref = reference("c4")
    t = ref["rec"]["t"]
    with Renderer(scene) as r:
        batch, out = check_variants(r, rays, t)
        sure = r.occluded(rays, t_max=None)
    check(sure, expected(t, INF))
    with np.errstate(invalid="ignore"):
        sphere_first = ref["hs_t"] < ref["ht_t"]
    assert (sure[sphere_first] == 1).any() and (sure[~sphere_first] == 1).any()
    assert (out == 1).any() and (out == 0).any() and batch.shape[1] == 7


def test_c5_global_walk_pruning_modes(gpu):
    """The global-memory walk (quantized nodes, leaf certificates, cooperative batches): pruning
    modes 1 and 0 give the same bytes, the oracle's."""
    scene, rays, ref = reference("c5")
    got = []
    for prune in (1, 0):
        with Renderer(scene, tuning={"query_lds_mode": 1}) as r:
            r.set_triangle_pruning(prune)
            got.append(check_variants(r, rays, ref["rec"]["t"])[1])
    assert got[0].tobytes() == got[1].tobytes()


def test_grazing_rays_certified(gpu, oracle_lib):
    """The tilted-plane set of test_grazing_rays_certified_pruning (500 rays within 1e-6..1e-3 rad of
    a 40x40 grid of triangles): where the certificates' error bounds matter most."""
    from tests.adversarial import grazing_rays, tilted_plane_grid

    scene, _ = build_config("c1_four_spheres", width=32, height=24)
    _, _, _, obj, frame = tilted_plane_grid(3, n=40, size=0.1)
    scene.objects = [obj]
    rays = grazing_rays(frame, 500, (1e-4, 1e-2), (1e-6, 1e-3), 13, span=1.5).astype(np.float32)
    ref = oracle_records(oracle_lib, scene, rays)
    assert (ref["ht_t"] != F32_MAX).sum() > 50
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            check_variants(r, rays, ref["rec"]["t"])


def in_plane_scene(triangles=(0, 1)):
    """The two-triangle plane at y = 0.5 over the C1 spheres (test_gpu_in_plane_rays_nan_distance),
    or one of its triangles."""
    from rust_gpu_raytracing_amd.scene import SceneObject

    scene, _ = build_config("c1_four_spheres", width=48, height=32)
    y0 = np.float32(0.5)
    a = np.array([[-1, y0, -1], [1, y0, -1]], np.float32)
    b = np.array([[1, y0, -1], [1, y0, 1]], np.float32)
    c = np.array([[-1, y0, 1], [-1, y0, 1]], np.float32)
    pick = list(triangles)
    info = np.zeros((), B.OBJECT_INFO)
    info["min_bounds"] = [-1, y0, -1]
    info["max_bounds"] = [1, y0, 1]
    obj = SceneObject(info, B.scene_triangles(a[pick], b[pick], c[pick]))
    obj.create_sub_objects(0, 0)
    scene.objects = [obj]
    return scene


def test_in_plane_rays_never_occlude(gpu, oracle_lib):
    """Rays lying exactly in the plane of two triangles (origin.y == 0.5, direction.y == 0): every
    triangle candidate has a NaN distance, which never occludes, so the spheres alone decide --
    here the ground sphere, which the plane touches: the rays aimed at the point of contact graze
    it in f32 or not, as the reference's own sphere test says."""
    n = 201
    rng = np.random.default_rng(21)
    rays = np.zeros((n, 6), np.float32)
    rays[:, 0] = rng.uniform(-3, 3, n)  # over the plane (|x|, |z| <= 1) and beside it
    rays[:, 2] = rng.uniform(-3, 3, n)
    rays[:, 1] = 0.5
    aimed = np.arange(n) % 3 != 0  # at the ground sphere's point of contact; the rest at the sky
    rays[aimed, 3], rays[aimed, 5] = -rays[aimed, 0], -rays[aimed, 2]
    ang = rng.uniform(0, 2 * np.pi, n)
    rays[~aimed, 3], rays[~aimed, 5] = np.cos(ang[~aimed]), np.sin(ang[~aimed])
    rays[::4, 3:] *= np.exp2(rng.uniform(-2, 2, n)).astype(np.float32)[::4, None]
    assert (rays[:, 1] == np.float32(0.5)).all() and (rays[:, 4] == 0).all()
    over = (np.abs(rays[:, 0]) < 1) & (np.abs(rays[:, 2]) < 1)
    assert over.sum() > 10 and (~over).sum() > 10

    # no triangle can occlude: each of the two alone gives a miss or a NaN distance
    for k in (0, 1):
        alone = in_plane_scene((k,))
        o = oracle_lib.Oracle(alone)
        p = alone.params(accumulation_index=1)
        p["sphere_count"] = 0
        tt = np.array([o.trace(p, ray[:3], ray[3:]).t for ray in rays], np.float32)
        assert (np.isnan(tt) | (tt == F32_MAX)).all()
        assert np.isnan(tt).any()
    # the spheres on their own
    scene = in_plane_scene()
    o = oracle_lib.Oracle(scene)
    p = scene.params(accumulation_index=1)
    p["object_count"] = 0
    ts = np.array([o.trace(p, ray[:3], ray[3:]).t for ray in rays], np.float32)
    hit = ts != F32_MAX
    near = np.where(hit, ts, np.float32(1))
    t_max = np.where(hit, np.choose(np.arange(n) % 5, [np.full(n, INF), next_up(near), near * 2, near, near / 2]),
                     np.choose(np.arange(n) % 3, [INF, np.float32(1), F32_MAX])).astype(np.float32)
    want = expected(ts, t_max)
    assert (want == 1).sum() >= 20 and (want == 0).sum() >= 20 and (want[hit] == 0).sum() >= 5
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            check(r.occluded(rays, t_max), want)
    with Renderer(scene, tuning={"tri_bvh": 0}) as r:  # the any-hit sweep
        check(r.occluded(rays, t_max), want)


def test_matches_closest_hit_on_a_large_batch(gpu):
    """10,000 C4 rays with t_max drawn from {t, nextafter(t), +inf} of the closest-hit record:
    the byte is (kind != miss) & (t < t_max); staged in chunks of 4,096 and through the device
    entry point (torch tensor in, torch tensor out) the same bytes."""
    import torch

    scene, rays, _ = reference("c4")
    rng = np.random.default_rng(5)
    big = rays[rng.integers(0, rays.shape[0], 10_000)].copy()
    big[:, :3] += (1e-3 * rng.standard_normal((10_000, 3))).astype(np.float32)
    with Renderer(scene) as r:
        hits = r.trace_rays(big)
        t = hits["t"]
        assert not np.isnan(t).any()
        q = np.zeros(big.shape[0], B.OCCLUSION_RAY)
        q["origin"], q["direction"] = big[:, :3], big[:, 3:]
        q["t_max"] = np.choose(rng.integers(0, 3, t.shape[0]), [t, next_up(t), np.full_like(t, INF)])
        with np.errstate(invalid="ignore"):
            want = ((hits["kind"] != B.HIT_MISS) & (t < q["t_max"])).astype(np.uint8)
        base = r.occluded(q)
        assert r.occluded(np.column_stack([big, q["t_max"]])).tobytes() == base.tobytes()
        r.set_tuning("query_chunk", 4096)
        chunked = r.occluded(q)
        dev = r.occluded(torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(gpu))
        assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (10_000,)
        dev_host = dev.cpu().numpy()
    assert (hits["kind"] != 0).any() and (hits["kind"] == 0).any()
    check(base, want)
    assert (want == 1).sum() > 1000 and (want[hits["kind"] != 0] == 0).sum() > 1000
    assert chunked.tobytes() == base.tobytes()
    assert dev_host.tobytes() == base.tobytes()


def test_occluded_segments(gpu, oracle_lib):
    """300 segments in C3 from the camera to closest-hit positions pushed 1% beyond (something is
    strictly before the end point) or pulled 1% short (mostly nothing is)."""
    scene, _, _ = reference("c3")
    o = oracle_lib.Oracle(scene)
    p = scene.params(accumulation_index=1)
    eye = np.asarray(scene.camera.position, np.float32)
    pos = []
    for d in scene.camera.recalculate_ray_directions()["direction"][::3]:
        h = o.trace(p, eye, d)
        if h.t != F32_MAX and len(pos) < 300:
            pos.append((h.px, h.py, h.pz))
    pos = np.array(pos, np.float32)
    assert pos.shape == (300, 3)
    a = np.tile(eye, (300, 1))
    f = np.where(np.arange(300) % 2 == 0, np.float32(1.01), np.float32(0.99)).astype(np.float32)
    b = (a + (pos - a) * f[:, None]).astype(np.float32)
    t = np.array([o.trace(p, a[i], b[i] - a[i]).t for i in range(300)], np.float32)
    want = expected(t, np.float32(1.0))
    assert (want == 1).sum() > 50 and (want == 0).sum() > 50
    with Renderer(scene) as r:
        check(r.occluded_segments(a, b), want)


# ---------------------------------------------------------------------------- semantics
def test_does_not_disturb_a_render(gpu):
    """The golden case c2_64x36_b8 with a 100-ray occlusion query between the compute_frame calls:
    accumulation, output and ray count equal the golden's, and the queued frames stay queued."""
    name = "c2_64x36_b8"
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    rays = reference("c2")[1][:100]
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY)) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                out = r.occluded(rays)
                assert (r.frame_batch(), r.accumulation_index) == before
                assert before[0][1] == i + 1  # the frames so far are still queued
        acc, img, n = r.read_accumulation(), r.read_output(), r.ray_count()
    assert out.shape == (100,) and out.any() and not out.all()
    assert n == int(g["rays"])
    assert np.array_equal(img, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_live_edit(gpu, oracle_lib):
    """After rt_update_objects moves one chess piece, the bytes equal the oracle's on the edited
    scene."""
    from rust_gpu_raytracing_amd import builder

    scene, _ = build_config("c3_chess", width=64, height=36, env_size=(1024, 512))
    rays = reference("c3")[1][:400]
    with Renderer(scene) as r:
        before = r.trace_rays(rays)
        hit_objects = before["index"][before["kind"] == 2]
        o = scene.objects[int(np.bincount(hit_objects).argmax())]  # the piece most rays hit
        o.rotation = np.array([0.0, 35.0, 0.0], np.float32)
        o.transformation = (np.asarray(o.transformation) + np.array([0.3, 0.0, -0.2])).astype(np.float32)
        just_past = next_up(before["t"])
        stale = r.occluded(rays, t_max=just_past)  # every hit ray, before the edit
        r.update_objects()
        for ob in scene.objects:
            builder.update_object(ob)
        orc = oracle_lib.Oracle(scene)
        p = scene.params(accumulation_index=1)
        t = np.array([orc.trace(p, ray[:3], ray[3:]).t for ray in rays], np.float32)
        t_max = np.where(np.arange(400) % 2 == 0, t, next_up(t)).astype(np.float32)
        out = r.occluded(rays, t_max=t_max)
        moved = r.occluded(rays, t_max=just_past)
    check(stale, (before["kind"] != B.HIT_MISS).astype(np.uint8))
    check(out, expected(t, t_max))
    check(moved, expected(t, just_past))
    assert out.any() and (moved != stale).any()  # the edit is visible to the rays


def test_errors(gpu):
    import torch

    scene, rays, _ = reference("c1")
    with Renderer(scene) as r:
        lib, ctx = r._lib, r._ctx
        q = np.zeros(4, B.OCCLUSION_RAY)
        out = np.zeros(4, np.uint8)
        assert lib.rt_occluded(ctx, None, N.ptr(out), 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_occluded(ctx, N.ptr(q), None, 4) == N.RT_E_INVALID
        assert lib.rt_occluded(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_occluded_device(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_occluded_device(ctx, None, None, 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        # host memory is not device memory of the context's device
        assert lib.rt_occluded_device(ctx, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(out.ctypes.data),
                                      4) == N.RT_E_INVALID
        assert b"device memory" in lib.rt_last_error(ctx)
        # rays misaligned by 4 bytes
        d_rays = torch.zeros(4 * 8 + 4, dtype=torch.float32, device=gpu)
        d_out = torch.zeros(8, dtype=torch.uint8, device=gpu)
        torch.cuda.synchronize()
        assert lib.rt_occluded_device(ctx, ctypes.c_void_p(d_rays.data_ptr() + 4), ctypes.c_void_p(d_out.data_ptr()),
                                      4) == N.RT_E_INVALID
        assert b"aligned" in lib.rt_last_error(ctx)
        q["origin"], q["direction"], q["t_max"] = rays[:4, :3], rays[:4, 3:], INF
        d_rays[:32] = torch.from_numpy(q.view(np.float32)).to(gpu)
        torch.cuda.synchronize()
        assert lib.rt_occluded_device(ctx, ctypes.c_void_p(d_rays.data_ptr()), ctypes.c_void_p(d_out.data_ptr() + 1),
                                      4) == N.RT_OK  # the result may have any alignment
        r.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[1:5], r.occluded(q))
        assert r.occluded(np.zeros((0, 7), np.float32)).shape == (0,)
        assert r.occluded(np.zeros((0, 7), np.float32)).dtype == np.uint8
        for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 8), np.float32), np.zeros(7, np.float32)):
            with pytest.raises(ValueError):
                r.occluded(bad)
        with pytest.raises(ValueError):
            r.occluded(np.zeros((4, 6), np.float32), t_max=np.ones(3, np.float32))
        with pytest.raises(ValueError):
            r.occluded_segments(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32))
