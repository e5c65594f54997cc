"""Hit-list queries (rt_trace_hits, rt_trace_hits_device, rt_pick_hits) against THE HIT-LIST
CONTRACT as tests/hits_ref.py restates it.

Every comparison is bit for bit: all 64 bytes of every entry of every ray, plus the counts. The
references of the golden scenes are computed once for 16 entries and shared; shorter lists are
their prefixes (consequence 3, which test_hits_cpu.py checks on the restatement itself).
"""
import ctypes
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests import hits_ref as H
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.test_gpu_occlusion import in_plane_scene, next_up, variants
from tests.test_gpu_query import SCENES, camera_rays
from tests.test_hits_cpu import identical_spheres_scene, in_plane_rays, tie_scene

pytestmark = pytest.mark.gpu

F32_MAX, INF = H.F32_MAX, H.INF


def same(got, want, max_hits):
    """(hits, counts) of a call against the reference's 16-entry (hits, counts)."""
    hits, counts = got
    want_hits, want_counts = H.truncate(want[0], want[1], max_hits)
    assert hits.dtype == B.HIT and hits.shape == want_hits.shape, (hits.shape, want_hits.shape)
    assert counts.dtype == np.uint32 and np.array_equal(counts, want_counts), np.nonzero(counts != want_counts)[0][:8]
    bad = np.nonzero((hits.view(np.uint8).reshape(hits.shape[0], -1) !=
                      want_hits.view(np.uint8).reshape(hits.shape[0], -1)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], hits[bad[:1]], want_hits[bad[:1]])


@functools.lru_cache(maxsize=None)
def built_reference(key, n):
    """Of a scene of tests/test_gpu_query.py's table: (scene, n camera rays, the 16-entry reference,
    every ray's number of candidates). Computed once and shared (never modified)."""
    from oracle import oracle as O

    O.build()
    config, kw = SCENES[key]
    scene, _ = build_config(config, **kw)
    rays = camera_rays(scene, n)
    ref = H.HitsRef(O, scene)
    hits, counts, total = ref.records(rays)
    return scene, rays, (hits, counts), total


# ---------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("count", [1, 63, 64, 65, 777])
def test_c1_wave_edges(gpu, count):
    """Sphere-only instance; counts at the wave edges, a ragged last chunk, and lists longer than
    any ray's candidates. At 65 rays the raw entry point writes into guarded buffers: every entry
    of every ray is written and nothing else is."""
    scene, rays, _, hits, counts, _ = H.golden_reference("c1")
    with Renderer(scene) as r:
        for k in (1, 2, 16):
            same(r.trace_hits(rays[:count], max_hits=k), (hits[:count], counts[:count]), k)
        if count == 65:
            q = np.zeros(count, B.OCCLUSION_RAY)
            q["origin"], q["direction"], q["t_max"] = rays[:count, :3], rays[:count, 3:], INF
            buf = np.full(64 + count * 2 * 64 + 64, 0xAA, np.uint8)
            cnt = np.full(count + 2, 0xAAAAAAAA, np.uint32)
            assert r._lib.rt_trace_hits(r._ctx, N.ptr(q), ctypes.c_void_p(buf.ctypes.data + 64),
                                        ctypes.c_void_p(cnt.ctypes.data + 4), count, 2) == N.RT_OK
            assert (buf[:64] == 0xAA).all() and (buf[-64:] == 0xAA).all()
            assert cnt[0] == cnt[-1] == 0xAAAAAAAA
            got = buf[64:-64].copy().view(B.HIT).reshape(count, 2)
            same((got, cnt[1:-1].copy()), (hits[:count], counts[:count]), 2)
            # counts may be NULL
            again = np.zeros((count, 2), B.HIT)
            assert r._lib.rt_trace_hits(r._ctx, N.ptr(q), N.ptr(again), None, count, 2) == N.RT_OK
            assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("mode", [0, 1, -1])
def test_c2_sphere_bvh(gpu, mode):
    """Sphere BVH plus the always-tested set, all 2304 camera rays, in the forced placements and
    the automatic one. At 4 entries 42 rays truncate."""
    scene, rays, _, hits, counts, total = H.golden_reference("c2")
    assert (total > 4).sum() == 42
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        for k in (1, 4, 8):
            same(r.trace_hits(rays, max_hits=k), (hits, counts), k)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles(gpu, mode):
    """The LDS-resident triangle walk (mode 2) and the global-memory walks, all 2304 camera rays.
    At 8 entries 13 rays truncate, and the 4 natural ties are ordered."""
    scene, rays, cand, hits, counts, total = H.golden_reference("c3")
    assert (total > 8).sum() == 13 and H.equal_t_pairs(cand) == 4
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        for k in (1, 4, 8, 16):
            same(r.trace_hits(rays, max_hits=k), (hits, counts), k)


@pytest.mark.parametrize("variant", ["prune0", "prune1", "brute"])
def test_c3_pruning_modes_and_brute_force(gpu, variant):
    """The result does not depend on triangle pruning modes 0 and 1 or on the brute-force mode."""
    scene, rays, _, hits, counts, _ = H.golden_reference("c3")
    with Renderer(scene) as r:
        if variant == "brute":
            r.set_brute_force(True)
        else:
            r.set_triangle_pruning(int(variant[-1]))
        for k in (1, 4, 8, 16):
            same(r.trace_hits(rays, max_hits=k), (hits, counts), k)


def test_c5_global_walk(gpu):
    """The small C5 heightfield of test_c5_global_walk_pruning_modes: the global-memory walk with
    quantized nodes, pruning modes 1 and 0."""
    scene, rays, want, total = built_reference("c5", 600)
    assert (total > 0).sum() > 100 and (total > 1).sum() > 20
    for prune in (1, 0):
        with Renderer(scene, tuning={"query_lds_mode": 1}) as r:
            r.set_triangle_pruning(prune)
            for k in (1, 4):
                same(r.trace_hits(rays, max_hits=k), want, k)


@pytest.mark.parametrize("key", ["c2", "c3"])
def test_secondary_style_rays(gpu, oracle_lib, key):
    """300 rays that start on surfaces (closest-hit positions, half of them pushed off along the
    normal) in random directions with finite t_max: lists bounded by t_max, not by the far end of
    the scene."""
    scene, cam, _, _, _, _ = H.golden_reference(key)
    rng = np.random.default_rng(11)
    with Renderer(scene) as r:
        first = r.trace_rays(cam)
        on = np.nonzero(first["kind"] != 0)[0]
        pick = rng.choice(on, 300, replace=False)
        rays = np.zeros((300, 6), np.float32)
        rays[:, :3] = first["position"][pick]
        rays[::2, :3] += np.float32(1e-4) * first["normal"][pick][::2]
        rays[:, 3:] = rng.standard_normal((300, 3)).astype(np.float32)
        t_max = np.exp2(rng.uniform(-3, 3, 300)).astype(np.float32)
        ref = H.HitsRef(oracle_lib, scene)
        hits, counts, total = ref.records(rays, t_max)
        unbounded = np.bincount(ref.lists(rays)["ray"], minlength=300)
        assert (total > 0).sum() > 30 and (total < unbounded).sum() > 30  # t_max cuts lists short
        for k in (1, 4, 16):
            same(r.trace_hits(rays, t_max, max_hits=k), (hits, counts), k)
        assert hits["t"][hits["kind"] != 0].max() < t_max.max()


def test_grazing_rays(gpu, oracle_lib):
    """The tilted-plane set of test_grazing_rays_certified (500 rays within 1e-6..1e-3 rad of a
    40x40 grid of triangles), at 4 entries: where the certificates' error bounds matter most. The
    lists are short here, so the certificates get a bound two more ways: a full list (1 entry), and
    t_max just past and exactly at each ray's nearest hit (the tie: nothing is listed at t_max)."""
    from tests.adversarial import grazing_rays, tilted_plane_grid

    scene, _ = build_config("c1_four_spheres", width=32, height=24)
    _, _, _, obj, frame = tilted_plane_grid(3, n=40, size=0.1)
    scene.objects = [obj]
    rays = grazing_rays(frame, 500, (1e-4, 1e-2), (1e-6, 1e-3), 13, span=1.5).astype(np.float32)
    ref = H.HitsRef(oracle_lib, scene)
    hits, counts, total = ref.records(rays, max_hits=4)
    assert ((hits["kind"] == 2).any(axis=1)).sum() > 50
    t0 = hits["t"][:, 0]
    past = np.where(np.arange(500) % 2 == 0, next_up(t0), t0).astype(np.float32)
    near_hits, near_counts, _ = ref.records(rays, past, max_hits=4)
    assert (near_counts == 1).sum() > 100 and ((near_counts == 0) & (counts > 0)).sum() > 100
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            same(r.trace_hits(rays, max_hits=4), (hits, counts), 4)
            same(r.trace_hits(rays, max_hits=1), (hits, counts), 1)
            same(r.trace_hits(rays, past, max_hits=4), (near_hits, near_counts), 4)


# ---------------------------------------------------------------------------- ties and NaN
def test_identical_spheres(gpu, oracle_lib):
    scene, rays = identical_spheres_scene()
    hits, counts, _ = H.HitsRef(oracle_lib, scene).records(rays)
    both = (hits["kind"] == 1) & (hits["index"] <= 1)
    assert (both.sum(axis=1) == 2).sum() > 20
    with Renderer(scene) as r:
        for k in (1, 2, 4):
            same(r.trace_hits(rays, max_hits=k), (hits, counts), k)


@pytest.mark.parametrize("objects", [1, 2])
def test_constructed_ties(gpu, oracle_lib, objects):
    """A sphere and one or two copies of a triangle at exactly equal t: triangles first, by sweep
    position; with the accelerator and with the sweep, and at every list length that cuts the tie."""
    scene, rays = tie_scene(objects)
    hits, counts, total = H.HitsRef(oracle_lib, scene).records(rays)
    assert list(hits["kind"][0, :objects + 1]) == [2] * objects + [1]
    assert (hits["t"][0, :objects + 1] == np.float32(4)).all()
    for tuning in ({"query_lds_mode": 0}, {"query_lds_mode": 2}, {"tri_bvh": 0}):
        with Renderer(scene, tuning=tuning) as r:
            for k in (1, 2, 3, 16):
                same(r.trace_hits(rays, max_hits=k), (hits, counts), k)


def test_in_plane_nan_triangles_never_listed(gpu, oracle_lib):
    scene = in_plane_scene()
    rays = in_plane_rays()
    hits, counts, total = H.HitsRef(oracle_lib, scene).records(rays, max_hits=4)
    assert not (hits["kind"] == 2).any() and (counts > 0).sum() > 20
    for tuning in ({"query_lds_mode": 0}, {"query_lds_mode": 2}, {"tri_bvh": 0}):
        with Renderer(scene, tuning=tuning) as r:
            same(r.trace_hits(rays, max_hits=4), (hits, counts), 4)


# ---------------------------------------------------------------------------- consequences
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_consequences_against_the_other_queries(gpu, key):
    """1: with t_max = +inf entry 0 is rt_trace_rays' record. 2: counts > 0 exactly when
    rt_occluded answers 1, for the t_max variants of the occlusion tests. 3: lists nest."""
    scene, rays, _, _, _, _ = H.golden_reference(key)
    with Renderer(scene) as r:
        closest = r.trace_rays(rays)
        assert not np.isnan(closest["t"]).any()
        lists = {k: r.trace_hits(rays, max_hits=k) for k in (1, 2, 4, 8, 16)}
        assert lists[1][0][:, 0].tobytes() == closest.tobytes()
        for k in (1, 2, 4, 8):
            assert lists[k][0].tobytes() == np.ascontiguousarray(lists[16][0][:, :k]).tobytes()
            assert np.array_equal(lists[k][1], np.minimum(lists[16][1], k))
        batch, want = variants(rays[::3], closest["t"][::3])
        occluded = r.occluded(batch)
        assert np.array_equal(occluded, want)
        for k in (1, 4):
            assert np.array_equal(r.trace_hits(batch, max_hits=k)[1] > 0, occluded == 1)


def test_chunking_and_device_form(gpu):
    """The host form in several chunks, and the device form through torch tensors, give the bits
    of the default run."""
    import torch

    scene, rays, _, hits, counts, _ = H.golden_reference("c3")
    with Renderer(scene) as r:
        r.set_tuning("query_chunk", 1000)  # 250 rays per chunk at 4 entries, 62 at 16
        for k in (4, 16):
            same(r.trace_hits(rays, max_hits=k), (hits, counts), k)
        q = np.zeros(rays.shape[0], B.OCCLUSION_RAY)
        q["origin"], q["direction"], q["t_max"] = rays[:, :3], rays[:, 3:], INF
        same(r.trace_hits(q, max_hits=4), (hits, counts), 4)
        d_hits, d_counts = r.trace_hits(torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(gpu), max_hits=4)
        assert d_hits.is_cuda and d_hits.dtype == torch.int32 and tuple(d_hits.shape) == (rays.shape[0], 4, 16)
        assert d_counts.is_cuda and d_counts.dtype == torch.int32 and tuple(d_counts.shape) == (rays.shape[0],)
        got = d_hits.cpu().numpy().view(B.HIT).reshape(rays.shape[0], 4), d_counts.cpu().numpy().view(np.uint32)
        same(got, (hits, counts), 4)
        e_hits, e_counts = r.trace_hits(torch.zeros((0, 8), dtype=torch.float32, device=gpu))
        assert tuple(e_hits.shape) == (0, 4, 16) and tuple(e_counts.shape) == (0,)
        h0, c0 = r.trace_hits(np.zeros((0, 7), np.float32))
        assert h0.shape == (0, 4) and c0.shape == (0,)


@pytest.mark.parametrize("device_rays", [False, True])
def test_pick_hits(gpu, oracle_lib, device_rays):
    """pick_hits(x, y) at the four corners and 30 random pixels of C3 is the list of that pixel's
    camera ray, with ray-buffer cameras and with rt_update_camera_matrices."""
    config, kw = SCENES["c3"]
    scene, _ = build_config(config, **kw)
    w, h = scene.camera.viewport_width, scene.camera.viewport_height
    d = scene.camera.recalculate_ray_directions()["direction"]
    rng = np.random.default_rng(9)
    px = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + \
        [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 30), rng.integers(0, h, 30))]
    rays = np.zeros((len(px), 6), np.float32)
    rays[:, :3] = np.asarray(scene.camera.position, np.float32)
    rays[:, 3:] = [d[y * w + x] for x, y in px]
    hits, counts, total = H.HitsRef(oracle_lib, scene).records(rays)
    assert (total > 2).any() and (total == 0).any()
    with Renderer(scene, device_rays=device_rays) as r:
        for i, (x, y) in enumerate(px):
            for k in (1, 3, 16):
                got = r.pick_hits(x, y, max_hits=k)
                n = min(int(total[i]), k)
                assert got.shape == (n,) and got.tobytes() == np.ascontiguousarray(hits[i, :n]).tobytes()
        hit = int(np.nonzero(total)[0][0])  # entry 0 is rt_pick's record
        assert r.pick_hits(*px[hit], max_hits=1)[0].tobytes() == r.pick(*px[hit]).tobytes()
        for bad in ((w, 0), (0, h)):
            with pytest.raises(RtError) as e:
                r.pick_hits(*bad)
            assert e.value.code == N.RT_E_INVALID


# ---------------------------------------------------------------------------- semantics
def test_does_not_disturb_a_render(gpu):
    """The golden case c2_64x36_b8 with a hit-list query between the compute_frame calls:
    accumulation, output, k and ray count equal the golden's, and the queued frames stay queued."""
    name = "c2_64x36_b8"
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    _, rays, _, hits, counts, _ = H.golden_reference("c2")
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY)) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                got = r.trace_hits(rays[:200], max_hits=4)
                one = r.pick_hits(3, 5)
                assert (r.frame_batch(), r.accumulation_index) == before
                assert before[0][1] == i + 1  # the frames so far are still queued
        acc, img, n = r.read_accumulation(), r.read_output(), r.ray_count()
    same(got, (hits[:200], counts[:200]), 4)
    assert one.shape[0] <= 4
    assert n == int(g["rays"])
    assert np.array_equal(img, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_rank_context(gpu):
    """A rank context (world_size 2, rank 1) returns the bits of a full context."""
    scene, rays, _, hits, counts, _ = H.golden_reference("c3")
    with Renderer(scene, rank=1, world_size=2) as r:
        same(r.trace_hits(rays, max_hits=8), (hits, counts), 8)


def test_live_edit(gpu, oracle_lib):
    """After rt_update_objects moves one chess piece, the lists are the contract's on the edited
    scene."""
    from rust_gpu_raytracing_amd import builder

    config, kw = SCENES["c3"]
    scene, _ = build_config(config, **kw)
    rays = camera_rays(scene, 400)
    with Renderer(scene) as r:
        before = r.trace_hits(rays, max_hits=4)
        hit_objects = before[0]["index"][before[0]["kind"] == 2]
        o = scene.objects[int(np.bincount(hit_objects).argmax())]  # the piece most entries lie on
        o.rotation = np.array([0.0, 35.0, 0.0], np.float32)
        o.transformation = (np.asarray(o.transformation) + np.array([0.3, 0.0, -0.2])).astype(np.float32)
        r.update_objects()
        after = r.trace_hits(rays, max_hits=4)
    for ob in scene.objects:
        builder.update_object(ob)
    hits, counts, _ = H.HitsRef(oracle_lib, scene).records(rays, max_hits=4)
    same(after, (hits, counts), 4)
    assert before[0].tobytes() != after[0].tobytes()  # the edit is visible to the rays


def test_errors(gpu):
    import torch

    scene, rays, _, hits, counts, _ = H.golden_reference("c1")
    with Renderer(scene) as r:
        lib, ctx = r._lib, r._ctx
        q = np.zeros(4, B.OCCLUSION_RAY)
        q["origin"], q["direction"], q["t_max"] = rays[:4, :3], rays[:4, 3:], INF
        out = np.zeros((4, 4), B.HIT)
        cnt = np.zeros(4, np.uint32)
        n = ctypes.c_uint32()
        d_rays = torch.zeros(4 * 8 + 4, dtype=torch.float32, device=gpu)
        d_rays[:32] = torch.from_numpy(q.view(np.float32).reshape(-1)).to(gpu)
        d_hits = torch.zeros(4 * 4 * 16 + 4, dtype=torch.int32, device=gpu)
        d_cnt = torch.zeros(8, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        P = ctypes.c_void_p
        # max_hits out of range, whatever count is
        for bad in (0, N.RT_HITS_MAX + 1):
            for count in (0, 4):
                assert lib.rt_trace_hits(ctx, N.ptr(q), N.ptr(out), N.ptr(cnt), count, bad) == N.RT_E_INVALID
                assert b"max_hits" in lib.rt_last_error(ctx)
                assert lib.rt_trace_hits_device(ctx, P(d_rays.data_ptr()), P(d_hits.data_ptr()), P(d_cnt.data_ptr()),
                                                count, bad) == N.RT_E_INVALID
            assert lib.rt_pick_hits(ctx, 0, 0, N.ptr(out), ctypes.byref(n), bad) == N.RT_E_INVALID
        # NULL rays or hits with count > 0; count == 0 launches nothing
        assert lib.rt_trace_hits(ctx, None, N.ptr(out), N.ptr(cnt), 4, 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_trace_hits(ctx, N.ptr(q), None, N.ptr(cnt), 4, 4) == N.RT_E_INVALID
        assert lib.rt_trace_hits(ctx, None, None, None, 0, 4) == N.RT_OK
        assert lib.rt_trace_hits_device(ctx, None, None, None, 0, 4) == N.RT_OK
        assert lib.rt_trace_hits_device(ctx, None, None, None, 4, 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_pick_hits(ctx, 0, 0, None, ctypes.byref(n), 4) == N.RT_E_INVALID
        assert lib.rt_pick_hits(ctx, 0, 0, N.ptr(out), None, 4) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_trace_hits_device(ctx, P(q.ctypes.data), P(out.ctypes.data), P(cnt.ctypes.data), 4,
                                        4) == N.RT_E_INVALID
        assert b"device memory" in lib.rt_last_error(ctx)
        assert lib.rt_trace_hits_device(ctx, P(d_rays.data_ptr()), P(d_hits.data_ptr()), P(cnt.ctypes.data), 4,
                                        4) == N.RT_E_INVALID
        # misaligned: rays and hits by 4 bytes, counts by 2
        for args in ((d_rays.data_ptr() + 4, d_hits.data_ptr(), d_cnt.data_ptr()),
                     (d_rays.data_ptr(), d_hits.data_ptr() + 4, d_cnt.data_ptr()),
                     (d_rays.data_ptr(), d_hits.data_ptr(), d_cnt.data_ptr() + 2)):
            assert lib.rt_trace_hits_device(ctx, P(args[0]), P(args[1]), P(args[2]), 4, 4) == N.RT_E_INVALID
            assert b"aligned" in lib.rt_last_error(ctx)
        # pixels outside the framebuffer
        assert lib.rt_pick_hits(ctx, r.width, 0, N.ptr(out), ctypes.byref(n), 4) == N.RT_E_INVALID
        assert lib.rt_pick_hits(ctx, 0, r.height, N.ptr(out), ctypes.byref(n), 4) == N.RT_E_INVALID
        assert not out.view(np.uint8).any() and not cnt.any() and not d_hits.cpu().numpy().any()
        # the context is still usable: counts at 4-byte alignment, no counts at all
        assert lib.rt_trace_hits_device(ctx, P(d_rays.data_ptr()), P(d_hits.data_ptr()), P(d_cnt.data_ptr() + 4), 4,
                                        4) == N.RT_OK
        r.synchronize()
        got = d_hits.cpu().numpy()[:256].view(B.HIT).reshape(4, 4), d_cnt.cpu().numpy()[1:5].view(np.uint32)
        same(got, (hits[:4], counts[:4]), 4)
        assert not d_hits.cpu().numpy()[256:].any() and not d_cnt.cpu().numpy()[5:].any()  # nothing else is written
        same(r.trace_hits(q, max_hits=4), (hits[:4], counts[:4]), 4)
        for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 8), np.float32), np.zeros(7, np.float32)):
            with pytest.raises(ValueError):
                r.trace_hits(bad)
        with pytest.raises(ValueError):
            r.trace_hits(np.zeros((4, 7), np.float32), t_max=1.0)
        with pytest.raises(RtError):
            r.trace_hits(q, max_hits=17)
