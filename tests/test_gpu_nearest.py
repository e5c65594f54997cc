"""Proximity queries (rt_nearest, rt_nearest_device) against THE NEAREST-POINT CONTRACT as
tests/nearest_ref.py restates it.

Every comparison is of all 64 bytes of every record. Points are drawn around and inside each
scene's bounds, plus the hit positions of its camera rays so that many points have a distance near
0, some with a finite max_distance. A scene's points and reference are computed once and shared.
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
from tests import nearest_ref as R
from tests.golden.fixtures import CASES, load, scene_from_inputs
from tests.test_gpu_query import SCENES, camera_rays

pytestmark = pytest.mark.gpu

INF, F32_MAX = R.INF, R.F32_MAX
same = R.same_records


def next_down(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(-np.inf)).astype(np.float32)


def scene_bounds(scene):
    """The box of the scene's geometry, the huge ground spheres left out."""
    spheres, _, _, tris = R.scene_arrays(scene)
    lo, hi = [], []
    small = spheres[np.abs(spheres["radius"]) < 100] if spheres.shape[0] else spheres
    if small.shape[0]:
        lo.append((small["position"] - np.abs(small["radius"])[:, None]).min(axis=0))
        hi.append((small["position"] + np.abs(small["radius"])[:, None]).max(axis=0))
    if tris.shape[0]:
        v = np.concatenate([tris["a"], tris["a"] + tris["edge_ab"], tris["a"] + tris["edge_ac"]])
        lo.append(v.min(axis=0))
        hi.append(v.max(axis=0))
    return np.min(lo, axis=0).astype(np.float32), np.max(hi, axis=0).astype(np.float32)


def scene_points(scene, r, n, seed):
    """(positions (n, 3), max_distance (n,)): a third on surfaces (camera-ray hit positions, half
    of them pushed off a little), the rest uniform in the scene's box grown by half; every fourth
    point with a finite max_distance of the order of the box."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(scene)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    pts = (mid + rng.uniform(-1.5, 1.5, (n, 3)) * half).astype(np.float32)
    hits = r.trace_rays(camera_rays(scene, max(n, 64)))
    on = hits[hits["kind"] != 0]
    k = min(n // 3, on.shape[0])
    if k:
        pick = rng.choice(on.shape[0], k, replace=False)
        pts[:k] = on["position"][pick]
        pts[:k:2] += np.float32(1e-3) * on["normal"][pick][::2]
    maxd = np.full(n, INF, np.float32)
    maxd[3::4] = (np.exp2(rng.uniform(-6, 0, maxd[3::4].shape[0])) * np.linalg.norm(half)).astype(np.float32)
    return pts, maxd


@functools.lru_cache(maxsize=None)
def reference(key, n):
    """(scene, positions, max_distance, the restatement's records) of a scene of
    tests/test_gpu_query.py's table. Computed once and shared (never modified)."""
    config, kw = SCENES[key]
    scene, _ = build_config(config, **kw)
    with Renderer(scene) as r:
        pts, maxd = scene_points(scene, r, n, 5)
    want = R.scene_nearest(scene, pts, maxd)
    return scene, pts, maxd, want


def records(pts, maxd):
    q = np.zeros(pts.shape[0], B.NEAR_POINT)
    q["position"], q["max_distance"] = pts, maxd
    return q


# ---------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("count", [1, 63, 64, 65, 777])
def test_c1_wave_edges(gpu, count):
    """Four spheres, the always-tested set only; counts at the wave edges and a ragged last chunk.
    At 65 points the raw entry point writes into guarded buffers: every record is written and
    nothing else is."""
    scene, pts, maxd, want = reference("c1", 777)
    assert (want["kind"] == R.SPHERE).sum() > 500
    with Renderer(scene) as r:
        same(r.nearest(pts[:count], maxd[:count]), want[:count])
        if count == 65:
            q = records(pts[:count], maxd[:count])
            buf = np.full(64 + count * 64 + 64, 0xAA, np.uint8)
            assert r._lib.rt_nearest(r._ctx, N.ptr(q), ctypes.c_void_p(buf.ctypes.data + 64), count) == N.RT_OK
            assert (buf[:64] == 0xAA).all() and (buf[-64:] == 0xAA).all()
            same(buf[64:-64].copy().view(B.NEAREST), want[:count])


@pytest.mark.parametrize("mode", [0, 1, -1])
def test_c2_sphere_bvh(gpu, mode):
    """The sphere BVH plus the always-tested set, in the forced placements and the automatic one."""
    scene, pts, maxd, want = reference("c2", 1500)
    assert len(set(want["index"][want["kind"] == R.SPHERE])) > 100
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        same(r.nearest(pts, maxd), want)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles(gpu, mode):
    """The chess scene: the LDS-resident triangle walk (mode 2) and the walks from global memory."""
    scene, pts, maxd, want = reference("c3", 512)
    tri = want[want["kind"] == R.TRIANGLE]
    assert tri.shape[0] > 300 and len(set(tri["feature"])) >= 4  # (each region: tests/test_nearest_cpu.py)
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        same(r.nearest(pts, maxd), want)


def test_c4_spheres_and_triangles(gpu):
    """Triangles and 486 spheres together: a sphere beats a triangle and the reverse."""
    scene, pts, maxd, want = reference("c4", 512)
    assert (want["kind"] == R.SPHERE).sum() >= 30 and (want["kind"] == R.TRIANGLE).sum() >= 30
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            same(r.nearest(pts, maxd), want)


def test_c5_global_walk(gpu):
    """The small heightfield (25,600 triangles): the walk from global memory with quantized nodes,
    and with the 32-byte nodes."""
    scene, pts, maxd, want = reference("c5", 300)
    assert (want["kind"] == R.TRIANGLE).sum() > 200
    for tuning in ({"query_lds_mode": 1}, {"query_lds_mode": 0, "tri_qnodes": 0}):
        with Renderer(scene, tuning=tuning) as r:
            same(r.nearest(pts, maxd), want)


@pytest.mark.parametrize("key", ["c2", "c3", "c4"])
@pytest.mark.parametrize("variant", ["sweep", "plain_walk", "brute", "tri_bvh0", "prune0"])
def test_does_not_depend_on_modes(gpu, key, variant):
    """Tuning "nearest_walk" 0 (the sweep) and 2 (the walk without its descent) against 1,
    rt_set_brute_force, the accelerator off, the pruning mode: identical bytes, the contract's."""
    scene, pts, maxd, want = reference(key, {"c2": 1500}.get(key, 512))
    with Renderer(scene) as r:
        walk = r.nearest(pts, maxd)
        if variant == "sweep":
            r.set_tuning("nearest_walk", 0)
        elif variant == "plain_walk":
            r.set_tuning("nearest_walk", 2)
        elif variant == "brute":
            r.set_brute_force(True)
        elif variant == "tri_bvh0":
            r.set_tuning("tri_bvh", 0)
        else:
            r.set_triangle_pruning(0)
        other = r.nearest(pts, maxd)
    same(walk, want)
    assert other.tobytes() == walk.tobytes()


def test_wrong_sub_object_boxes(gpu):
    """Sub-object boxes that are deliberately wrong, shrunk and shifted: still the contract's
    answer (the boxes carry no meaning; the library stops culling by them). Restoring the boxes
    gives the same bytes again."""
    scene, pts, maxd, want = reference("c3", 512)
    _, subs, _ = scene.flatten()
    wrong = np.ascontiguousarray(subs.copy())
    mid = (subs["min_bounds"] + subs["max_bounds"]) / 2
    half = (subs["max_bounds"] - subs["min_bounds"]) / 2
    wrong["min_bounds"] = mid - half / 4 + np.float32(0.5)
    wrong["max_bounds"] = mid + half / 4 + np.float32(0.5)
    subs = np.ascontiguousarray(subs)
    for mode in (0, 2):
        with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
            same(r.nearest(pts, maxd), want)
            r._call("rt_update_sub_object_info", N.ptr(wrong), wrong.shape[0])
            same(r.nearest(pts, maxd), want)
            r._call("rt_update_sub_object_info", N.ptr(subs), subs.shape[0])
            same(r.nearest(pts, maxd), want)


def test_infinite_edge_triangle_in_a_wrong_box(gpu):
    """A triangle with an infinite edge, a = (50, 50, 50), ab = (inf, 0, 0), ac = (0, 1, 0), uploaded
    into a chess sub-object whose finite box stays where it was: the triangle's keys are finite
    through the regions that do not touch the edge (1.41, 1.41 and 0.54 from the three points
    here, nothing else within 40), and no box holds it, so the library must not cull by the boxes."""
    scene, pts, maxd, _ = reference("c3", 512)
    objs, subs, tris = scene.flatten()
    tris = np.ascontiguousarray(tris.copy())
    ti = int(subs["first_triangle_index"][0])
    tris["a"][ti], tris["edge_ab"][ti], tris["edge_ac"][ti] = (50, 50, 50), (np.inf, 0, 0), (0, 1, 0)
    near = np.float32([50, 50, 50]) + np.float32([[-1, -1, 0], [-1, 2, 0], [-0.5, 0.5, 0.2]])
    p = np.concatenate([near, pts[:125]]).astype(np.float32)
    d = np.concatenate([np.full(3, INF, np.float32), maxd[:125]])
    want = R.scene_nearest(scene, p, d, geometry=(objs, subs, tris))
    assert (want["triangle"][:3] == ti).all() and list(want["feature"][:3]) == [1, 4, 5]
    assert (want["distance"][:3] < 1.5).all() and np.isfinite(subs["max_bounds"][0]).all()
    for tuning in ({"query_lds_mode": 0}, {"query_lds_mode": 2}, {"nearest_walk": 0}):
        with Renderer(scene, tuning=tuning) as r:
            r._call("rt_update_triangles", N.ptr(tris), tris.shape[0])
            same(r.nearest(p, d), want)


# ---------------------------------------------------------------------------- edits
def test_sees_a_live_sphere_edit(gpu):
    """After rt_update_spheres moves and grows the spheres of c2 (one made a hollow shell), the
    results are the contract's on the edited scene."""
    scene, pts, maxd, want = reference("c2", 1500)
    spheres = np.ascontiguousarray(scene.spheres.copy())
    spheres["position"][:, 0] += np.float32(0.15)
    spheres["radius"] *= np.float32(1.1)
    spheres["radius"][7] = -spheres["radius"][7]
    edited = dataclasses.replace(scene, spheres=spheres)
    edited.flatten = scene.flatten
    want2 = R.scene_nearest(edited, pts, maxd)
    assert want2.tobytes() != want.tobytes()
    with Renderer(scene) as r:
        same(r.nearest(pts, maxd), want)
        r._call("rt_update_spheres", N.ptr(spheres), spheres.shape[0])
        same(r.nearest(pts, maxd), want2)


def test_sees_a_live_object_edit(gpu):
    """After rt_update_objects moves a chess piece, the results are the contract's on the triangles
    read back with rt_read_triangles; the walk and the sweep agree on the refitted boxes."""
    config, kw = SCENES["c3"]
    scene, _ = build_config(config, **kw)
    _, pts, maxd, want = reference("c3", 512)
    with Renderer(scene) as r:
        before = r.nearest(pts, maxd)
        on = before["index"][before["kind"] == R.TRIANGLE]
        o = scene.objects[int(np.bincount(on).argmax())]  # the piece most points are nearest to
        o.rotation = np.array([0.0, 35.0, 0.0], np.float32)
        o.transformation = (np.asarray(o.transformation) + np.array([0.3, 0.0, -0.2])).astype(np.float32)
        r.update_objects()
        after = r.nearest(pts, maxd)
        geometry = r.read_geometry()
        r.set_tuning("nearest_walk", 0)
        swept = r.nearest(pts, maxd)
    same(before, want)
    same(after, R.scene_nearest(scene, pts, maxd, geometry=geometry))
    assert swept.tobytes() == after.tobytes() and after.tobytes() != before.tobytes()


# ---------------------------------------------------------------------------- the device entry
def test_device_entry_and_chunks(gpu):
    """The device form through torch tensors and the host form in several chunks give the bytes of
    the default run."""
    import torch

    scene, pts, maxd, want = reference("c3", 512)
    q = records(pts, maxd)
    with Renderer(scene) as r:
        r.set_tuning("query_chunk", 100)
        same(r.nearest(q), want)
        same(r.nearest(np.concatenate([pts, maxd[:, None]], axis=1)), want)
        d = r.nearest(torch.from_numpy(q.view(np.float32).reshape(-1, 4)).to(gpu))
        assert d.is_cuda and d.dtype == torch.int32 and tuple(d.shape) == (pts.shape[0], 16)
        same(d.cpu().numpy().view(B.NEAREST).reshape(-1), want)
        e = r.nearest(torch.zeros((0, 4), dtype=torch.float32, device=gpu))
        assert tuple(e.shape) == (0, 16)
        assert r.nearest(np.zeros((0, 3), np.float32)).shape == (0,)


def test_does_not_disturb_a_render(gpu):
    """The golden case c2_64x36_b8 with a proximity query (host and device forms) between the
    compute_frame calls: accumulation, output, k and ray count equal the golden's, and the queued
    frames stay queued."""
    import torch

    name = "c2_64x36_b8"
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    _, pts, maxd, _ = reference("c2", 1500)
    want = R.scene_nearest(scene, pts[:200], maxd[:200])
    q = torch.from_numpy(records(pts[:200], maxd[:200]).view(np.float32).reshape(-1, 4)).to(gpu)
    got_d = torch.zeros((200, 16), dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY)) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                got = r.nearest(pts[:200], maxd[:200])
                # the raw device entry (Renderer.nearest asks for rt_stream first, which launches
                # what is queued so that the caller's work follows it)
                assert r._lib.rt_nearest_device(r._ctx, ctypes.c_void_p(q.data_ptr()),
                                                ctypes.c_void_p(got_d.data_ptr()), 200) == N.RT_OK
                assert (r.frame_batch(), r.accumulation_index) == before
                assert before[0][1] == i + 1  # the frames so far are still queued
        acc, img, n = r.read_accumulation(), r.read_output(), r.ray_count()
    same(got, want)
    same(got_d.cpu().numpy().view(B.NEAREST).reshape(-1), want)
    assert n == int(g["rays"])
    assert np.array_equal(img, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_first_call_after_an_upload_keeps_frames_queued(gpu):
    """The golden case c3_64x36_b8, a scene with objects: the first device-form call, which makes
    the host pass over the boxes (it reads the triangles back and waits for the stream), and the
    calls after it, between the compute_frame calls. The queued frames stay queued, and the
    accumulation, output and ray count equal the golden's."""
    import torch

    name = "c3_64x36_b8"
    g, case = load(name), CASES[name]
    scene = scene_from_inputs(g)
    _, pts, maxd, _ = reference("c3", 512)
    want = R.scene_nearest(scene, pts[:200], maxd[:200])
    q = torch.from_numpy(records(pts[:200], maxd[:200]).view(np.float32).reshape(-1, 4)).to(gpu)
    got_d = torch.zeros((200, 16), dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY)) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            before = r.frame_batch(), r.accumulation_index
            assert r._lib.rt_nearest_device(r._ctx, ctypes.c_void_p(q.data_ptr()),
                                            ctypes.c_void_p(got_d.data_ptr()), 200) == N.RT_OK
            got = r.nearest(pts[:200], maxd[:200])
            assert (r.frame_batch(), r.accumulation_index) == before
            assert before[0][1] == i + 1  # the frames so far are still queued
        acc, img, n = r.read_accumulation(), r.read_output(), r.ray_count()
    same(got, want)
    same(got_d.cpu().numpy().view(B.NEAREST).reshape(-1), want)
    assert n == int(g["rays"])
    assert np.array_equal(img, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


# ---------------------------------------------------------------------------- edges
@pytest.mark.parametrize("key", ["c2", "c3"])
def test_max_distance_edges(gpu, key):
    """max_distance at the key, at the next value below the key, at 0, +inf, NaN and negative; NaN
    coordinates give a miss."""
    scene, pts, _, _ = reference(key, {"c2": 1500}.get(key, 512))
    pts = pts[:240]
    free = R.scene_nearest(scene, pts, INF)
    assert (free["kind"] != R.MISS).all()
    key_d = free["distance"]
    maxd = np.full(pts.shape[0], INF, np.float32)
    maxd[0::6] = key_d[0::6]
    maxd[1::6] = next_down(key_d[1::6])
    maxd[2::6] = 0
    maxd[3::6] = np.nan
    maxd[4::6] = -1
    p = pts.copy()
    p[5::12, 1] = np.nan
    want = R.scene_nearest(scene, p, maxd)
    assert want[0::6].tobytes() == free[0::6].tobytes()  # at the key: still found
    assert (want["distance"][1::6][key_d[1::6] > 0] > key_d[1::6][key_d[1::6] > 0]).all()  # another one, or a miss
    assert (want["kind"][3::6] == R.MISS).all() and (want["kind"][4::6] == R.MISS).all()
    assert (want["kind"][5::12] == R.MISS).all()
    for tuning in ({"query_lds_mode": 0}, {"nearest_walk": 0}):
        with Renderer(scene, tuning=tuning) as r:
            same(r.nearest(p, maxd), want)


def test_empty_scene_and_errors(gpu):
    import torch

    scene, pts, maxd, want = reference("c1", 777)
    empty = dataclasses.replace(scene, spheres=np.zeros(0, B.SPHERE))
    empty.flatten = scene.flatten
    with Renderer(empty) as r:
        got = r.nearest(pts[:70])
    miss = np.zeros(70, B.NEAREST)
    miss["distance"] = F32_MAX
    same(got, miss)
    with Renderer(scene) as r:
        lib, ctx, P = r._lib, r._ctx, ctypes.c_void_p
        q = records(pts[:4], maxd[:4])
        out = np.zeros(4, B.NEAREST)
        d_q = torch.zeros(4 * 4 + 4, dtype=torch.float32, device=gpu)
        d_q[:16] = torch.from_numpy(q.view(np.float32).reshape(-1)).to(gpu)
        d_out = torch.zeros(4 * 16 + 4, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        # count == 0 launches nothing; NULL pointers with count > 0
        assert lib.rt_nearest(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_nearest_device(ctx, None, None, 0) == N.RT_OK
        assert lib.rt_nearest(ctx, None, N.ptr(out), 4) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_nearest(ctx, N.ptr(q), None, 4) == N.RT_E_INVALID
        assert lib.rt_nearest_device(ctx, None, None, 4) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_nearest_device(ctx, P(q.ctypes.data), P(out.ctypes.data), 4) == N.RT_E_INVALID
        assert b"device memory" in lib.rt_last_error(ctx)
        # misaligned by 4 bytes
        assert lib.rt_nearest_device(ctx, P(d_q.data_ptr() + 4), P(d_out.data_ptr()), 4) == N.RT_E_INVALID
        assert b"aligned" in lib.rt_last_error(ctx)
        assert lib.rt_nearest_device(ctx, P(d_q.data_ptr()), P(d_out.data_ptr() + 4), 4) == N.RT_E_INVALID
        assert not out.view(np.uint8).any() and not d_out.cpu().numpy().any()
        # the context is still usable, and nothing but the records is written
        assert lib.rt_nearest_device(ctx, P(d_q.data_ptr()), P(d_out.data_ptr()), 4) == N.RT_OK
        r.synchronize()
        same(d_out.cpu().numpy()[:64].view(B.NEAREST), want[:4])
        assert not d_out.cpu().numpy()[64:].any()
        for bad in (np.zeros((4, 5), np.float32), np.zeros(7, np.float32)):
            with pytest.raises(ValueError):
                r.nearest(bad)
        with pytest.raises(ValueError):
            r.nearest(np.zeros((4, 4), np.float32), max_distance=1.0)
    with pytest.raises(RtError):
        r.nearest(pts[:4])  # closed
