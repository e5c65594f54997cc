"""Ambient queries (rt_ambient, rt_ambient_device) against the CPU oracle, bit for bit.

The reference of a point is the NumPy restatement of the contract (tests/ambient_ref.py) fed the
oracle's own trace_ray: every sample is the ray (x + n * 0.0001f, the restatement's direction),
open iff the oracle's closest distance is a miss or not below t_max, and the stripe-and-tree
reduction of the terms (dir, 1) / +0 is the expected (bent, open). All comparisons are on the u32
bit patterns of the four floats.

Points and streams are tests/test_gpu_gather.py's ``point_set`` (first hits of camera rays, with
the dressed normals on points 0 and 2 and stream 0 on point 1). A run is one oracle evaluation of
a point set at (first_sample, samples); it is computed once and shared, and the cases that use
fewer points take a prefix of it (a point's result does not depend on its neighbours). Against
vacuous inputs every run of 63 or more samples with a finite bound uses as t_max the median of the
finite oracle distances of its sample rays and asserts, on the oracle's output alone: at least 50
samples open, at least 50 occluded, at least a quarter of the points with 0 < open < samples; and
every run of 65 or more samples that the contract's reduction of bent differs in bits from the
plain ascending sum on at least half the points. No oracle distance is NaN (asserted in
ambient_ref.oracle_distances).
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from tests import ambient_ref as A
from tests import gather_ref as G
from tests.test_gpu_gather import bits, golden_scene, point_set, renderer

pytestmark = pytest.mark.gpu

F32_MAX = np.float32(3.4028235e38)
INF = np.float32(np.inf)


# ---------------------------------------------------------------------------- runs and references
@dataclasses.dataclass(frozen=True)
class Run:
    points: np.ndarray   # (n, 6)
    streams: np.ndarray  # (n,)
    origins: np.ndarray  # (n, 3)
    dirs: np.ndarray     # (n, samples, 3)
    t: np.ndarray        # (n, samples) oracle distances
    t_max: np.float32    # the run's bound: the median of the finite distances
    want: np.ndarray     # (n, 4)

    def records(self, count=None, t_max=None):
        n = self.points.shape[0] if count is None else count
        return A.records(self.points[:n], self.streams[:n], self.t_max if t_max is None else t_max)


def evaluate(scene, points, streams, first_sample, samples):
    """One run on ``scene``, with the conditions against vacuous inputs asserted on the oracle's
    output."""
    from oracle import oracle as O

    O.build()
    n = points.shape[0]
    origins, dirs = A.rays(points, streams, first_sample, samples)
    t = A.oracle_distances(O, scene, origins, dirs)
    finite = t[t != F32_MAX]
    t_max = np.float32(np.median(finite)) if finite.size else INF
    v = A.visibility(t, t_max)
    want = A.ambient(dirs, t, t_max)
    if samples >= 63:
        assert np.isfinite(t_max)
        opened = v.sum(axis=1)
        partly = int(((opened > 0) & (opened < samples)).sum())
        assert int(v.sum()) >= 50 and int((1 - v).sum()) >= 50, (int(v.sum()), int((1 - v).sum()))
        assert 4 * partly >= n, (partly, n)
    if samples >= 65:
        plain = G.sequential(A.terms(dirs, v))
        differ = int((bits(want[:, :3]) != bits(plain[:, :3])).any(axis=1).sum())
        assert 2 * differ >= n, (differ, n)
    for a in (origins, dirs, t, want):
        a.setflags(write=False)
    return Run(points, streams, origins, dirs, t, t_max, want)


@functools.lru_cache(maxsize=None)
def run(key, total, first_sample, samples):
    """The run of the scene's whole set of ``total`` points (never modified)."""
    points, streams = point_set(key, total)
    return evaluate(golden_scene(key)[2], points, streams, first_sample, samples)


def result(bent, opened):
    """(n, 4) from what Renderer.ambient returns, host or device."""
    if hasattr(bent, "is_cuda"):
        bent, opened = bent.cpu().numpy(), opened.cpu().numpy()
    assert bent.dtype == np.float32 and opened.dtype == np.float32 and bent.shape == (opened.shape[0], 3)
    return np.concatenate([bent, opened[:, None]], axis=1)


def check(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


# ---------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("samples", [1, 63, 64, 65, 200])
def test_c1_sample_counts(gpu, oracle_lib, samples):
    """Sphere-only instance, 5 points (the first 5 of the set of 12, whose runs meet the
    conditions): fewer stripes than lanes, exactly 64, one stripe with a second sample, and
    stripes of three and four samples."""
    ref = run("c1", 12, 1, samples)
    with renderer("c1") as r:
        got = result(*r.ambient(ref.records(5), samples=samples, first_sample=1))
    check(got, ref.want[:5])


@pytest.mark.parametrize("count", [1, 4, 5, 63, 65])
def test_c1_point_counts(gpu, oracle_lib, count):
    """Point counts at the item and wave edges, 65 samples each (64 stripes per point, of which
    stripe 0 has two samples): prefixes of one run of 65 points."""
    ref = run("c1", 65, 1, 65)
    opened = A.visibility(ref.t, ref.t_max).sum(axis=1)
    assert 0 < opened[0] < 65  # (the one-point case is a point that is partly occluded)
    with renderer("c1") as r:
        got = result(*r.ambient(ref.records(count), samples=65))
    check(got, ref.want[:count])


@pytest.mark.parametrize("mode", [0, 1])
def test_c2_sphere_bvh(gpu, oracle_lib, mode):
    """Sphere BVH plus the brute-force set, in both placements: the oracle's bits in each."""
    ref = run("c2", 16, 1, 65)
    with renderer("c2", tuning={"query_lds_mode": mode}) as r:
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
    check(got, ref.want)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles(gpu, oracle_lib, mode):
    """Triangles and spheres in the three placements: the oracle's bits in each."""
    ref = run("c3", 16, 1, 65)
    with renderer("c3", tuning={"query_lds_mode": mode}) as r:
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
    check(got, ref.want)


@pytest.mark.parametrize("key,mode", [("c2", 1), ("c3", 2), ("c3", 0)])
def test_stripes_of_several_samples(gpu, oracle_lib, key, mode):
    """200 samples from first_sample 7 on the scenes whose searches traverse: every stripe runs
    three or four searches back to back, and the last of them run after the wave's items are
    exhausted, with few lanes still traversing."""
    ref = run(key, 16, 7, 200)
    with renderer(key, tuning={"query_lds_mode": mode}) as r:
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=200, first_sample=7))
    check(got, ref.want)


@functools.lru_cache(maxsize=None)
def sharp_pairs(key):
    """Point pairs that differ only in t_max, for samples = 1 at first_sample 3: among 96 points
    those whose one sample hits, once with t_max equal to the oracle distance (open = 1) and once
    with nextafter of it (open = 0)."""
    ref = run(key, 96, 3, 1)
    hit = np.nonzero(ref.t[:, 0] != F32_MAX)[0]
    assert hit.size >= 20, hit.size
    t = ref.t[hit, 0]
    up = np.nextafter(t, INF, dtype=np.float32)
    assert (up > t).all()
    rec = np.concatenate([A.records(ref.points[hit], ref.streams[hit], t), A.records(ref.points[hit], ref.streams[hit], up)])
    want = np.concatenate([A.ambient(ref.dirs[hit], ref.t[hit], t), A.ambient(ref.dirs[hit], ref.t[hit], up)])
    assert (want[:hit.size, 3] == 1).all() and (want[hit.size:, 3] == 0).all() and not bits(want[hit.size:]).any()
    assert np.array_equal(bits(want[:hit.size, :3]), bits(ref.dirs[hit, 0]))
    order = np.random.default_rng(5).permutation(rec.shape[0])  # the two of a pair in different lanes
    return rec[order], want[order]


@pytest.mark.parametrize("key,modes", [("c2", (0, 1)), ("c3", (0, 1, 2))])
def test_sharp_bound(gpu, oracle_lib, key, modes):
    """t_max == t leaves the sample open and the next float above occludes it, in every
    placement: the cull by t_max neither loses the closest primitive nor accepts it early."""
    rec, want = sharp_pairs(key)
    for mode in modes:
        with renderer(key, tuning={"query_lds_mode": mode}) as r:
            got = result(*r.ambient(rec, samples=1, first_sample=3))
        check(got, want)


def test_special_bounds_in_one_batch(gpu, oracle_lib):
    """+inf, F32_MAX, 0, -1 and NaN bounds, point by point in one batch on c3: sky visibility for
    the first two, everything open for the others."""
    ref = run("c3", 16, 1, 65)
    bounds = np.array([INF, F32_MAX, 0.0, -1.0, np.nan], np.float32)[np.arange(16) % 5]
    want = A.ambient(ref.dirs, ref.t, bounds)
    sky = A.ambient(ref.dirs, ref.t, INF)
    assert np.array_equal(bits(want[0::5]), bits(sky[0::5])) and np.array_equal(bits(want[1::5]), bits(sky[1::5]))
    assert (want[np.arange(16) % 5 >= 2, 3] == 65).all() and (sky[:, 3] < 65).sum() >= 8
    with renderer("c3") as r:
        got = result(*r.ambient(ref.points, ref.streams, bounds, samples=65))
        whole = result(*r.ambient(ref.points, ref.streams, samples=65))  # the default bound: +inf
    check(got, want)
    check(whole, sky)


def test_first_sample_wraps(gpu, oracle_lib):
    """first_sample two below 2^32: the sample index wraps to 0, 1, ... as u32."""
    first = 0xFFFFFFFE
    ref = run("c2", 16, first, 65)
    assert np.array_equal(bits(ref.dirs[3, 2]), bits(G.direction(ref.points[3, 3:], ref.streams[3], 0)))
    with renderer("c2") as r:
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65, first_sample=first))
    check(got, ref.want)


# ---------------------------------------------------------------------------- chunking, device entry
def test_chunking_and_device_entry_point(gpu, oracle_lib):
    """100 points at 70 samples in launches of 7 points, staged in chunks of 33, in one launch, and
    through the device entry point give the oracle's bits; guard floats on both sides of the
    device result are not written."""
    import torch

    ref = run("c1", 100, 1, 70)
    q = ref.records()
    with renderer("c1", tuning={"gather_chunk": 7}) as r:
        chunked = result(*r.ambient(q, samples=70))
        r.set_tuning("query_chunk", 33)
        staged = result(*r.ambient(q, samples=70))
        t = torch.from_numpy(q.view(np.float32).reshape(-1, 8).copy()).to(gpu)
        dev7 = r.ambient(t, samples=70)
        assert dev7[0].is_cuda and tuple(dev7[0].shape) == (100, 3) and tuple(dev7[1].shape) == (100,)
        dev7 = result(*dev7)
        r.set_tuning("gather_chunk", 16384)
        r.set_tuning("query_chunk", 65536)
        base = result(*r.ambient(q, samples=70))
        uploaded = result(*r.ambient(q, samples=70, device=True))
        room = torch.full((102, 4), -7.25, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize(gpu)
        r._call("rt_ambient_device", ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(room.data_ptr() + 16), 100, 1, 70)
        r.synchronize()
        room_host = room.cpu().numpy()
    for got in (chunked, staged, dev7, base, uploaded, room_host[1:101].copy()):
        check(got, ref.want)
    guard = bits(np.full(4, -7.25, np.float32))
    assert np.array_equal(bits(room_host[0]), guard) and np.array_equal(bits(room_host[101]), guard)


def test_misaligned_device_pointers_are_refused(gpu):
    import torch

    points, streams = point_set("c1", 12)
    q = A.records(points[:4], streams[:4], 1.0)
    with renderer("c1") as r:
        t = torch.zeros(4 * 8 + 8, dtype=torch.float32, device=gpu)
        t[:32] = torch.from_numpy(q.view(np.float32).copy()).to(gpu)
        out = torch.zeros(4 * 4 + 8, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize(gpu)
        lib, ctx = r._lib, r._ctx
        P = ctypes.c_void_p
        assert lib.rt_ambient_device(ctx, P(t.data_ptr() + 4), P(out.data_ptr()), 4, 1, 8) == N.RT_E_INVALID
        assert lib.rt_ambient_device(ctx, P(t.data_ptr()), P(out.data_ptr() + 8), 4, 1, 8) == N.RT_E_INVALID
        assert lib.rt_ambient_device(ctx, P(t.data_ptr()), P(out.data_ptr()), 4, 1, 8) == N.RT_OK
        r.synchronize()
        assert not bool(out[16:].any()) and bool(out[:16].any())


# ---------------------------------------------------------------------------- semantics
def test_errors(gpu):
    points, streams = point_set("c1", 12)
    q = A.records(points[:4], streams[:4], 1.0)
    with renderer("c1") as r:
        with pytest.raises(RtError) as e:
            r.ambient(q, samples=0)
        assert e.value.code == N.RT_E_INVALID
        with pytest.raises(RtError) as e:
            r.ambient(q, samples=(1 << 24) + 1)
        assert e.value.code == N.RT_E_INVALID
        lib, ctx = r._lib, r._ctx
        out = np.zeros((4, 4), np.float32)
        assert lib.rt_ambient(ctx, None, N.ptr(out), 4, 1, 1) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_ambient(ctx, N.ptr(q), None, 4, 1, 1) == N.RT_E_INVALID
        assert lib.rt_ambient(ctx, N.ptr(q), N.ptr(out), 4, 1, 0) == N.RT_E_INVALID
        assert lib.rt_ambient(ctx, None, None, 0, 1, 0) == N.RT_E_INVALID  # whatever count is
        assert lib.rt_ambient(ctx, None, None, 0, 1, (1 << 24) + 1) == N.RT_E_INVALID
        assert lib.rt_ambient(ctx, None, None, 0, 1, 1) == N.RT_OK
        assert not out.any()
        assert lib.rt_ambient(ctx, N.ptr(q), N.ptr(out), 4, 1, 1) == N.RT_OK
        assert set(out[:, 3]) <= {0.0, 1.0}
        assert lib.rt_ambient_device(ctx, None, None, 0, 1, 1) == N.RT_OK
        assert lib.rt_ambient_device(ctx, None, None, 4, 1, 1) == N.RT_E_INVALID
        assert lib.rt_ambient_device(ctx, None, None, 4, 1, 0) == N.RT_E_INVALID
        assert lib.rt_ambient_device(ctx, None, None, 0, 1, (1 << 24) + 1) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_ambient_device(ctx, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(out.ctypes.data), 4, 1,
                                     1) == N.RT_E_INVALID
        bent, opened = r.ambient(np.zeros((0, 6), np.float32))
        assert bent.shape == (0, 3) and opened.shape == (0,)
        with pytest.raises(ValueError):
            r.ambient(q, streams[:4])
        with pytest.raises(ValueError):
            r.ambient(points[:, :5])
        with pytest.raises(ValueError):
            r.ambient(points[:4], streams[:4], np.ones(3, np.float32))


@pytest.mark.parametrize("batch", [1, 16])
def test_ambient_does_not_disturb_a_render(gpu, oracle_lib, batch):
    """The golden case c2_64x36_b8 with a 16-point ambient query between the compute_frame calls,
    with one launch per frame and with a frame queue of 16: accumulation, output, k and ray count
    equal the golden's, and a queued frame stays queued."""
    g, case, scene = golden_scene("c2")
    ref = run("c2", 16, 1, 65)
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
                assert (r.frame_batch(), r.accumulation_index) == before
                if batch == 16:
                    assert before[0][1] == i + 1  # the frames so far are still queued
        k = r.accumulation_index
        acc, out, n = r.read_accumulation(), r.read_output(), r.ray_count()
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
        k_plain = r.accumulation_index
    check(got, ref.want)
    assert k == k_plain
    assert n == int(g["rays"])
    assert np.array_equal(out, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_sees_a_live_sphere_edit(gpu, oracle_lib):
    """After rt_update_spheres grows and moves the spheres of c1, the query equals the restatement
    on the edited scene (a run of its own) and, at the earlier bound, differs from the earlier
    result as the oracle's does."""
    _, _, scene = golden_scene("c1")
    ref = run("c1", 65, 1, 65)
    spheres = np.ascontiguousarray(scene.spheres.copy())
    spheres["position"][:, 0] += np.float32(0.15)
    spheres["radius"] *= np.float32(1.1)
    edited = dataclasses.replace(scene, spheres=spheres)
    edited.flatten = scene.flatten
    ref2 = evaluate(edited, ref.points, ref.streams, 1, 65)
    at_old_bound = A.ambient(ref2.dirs, ref2.t, ref.t_max)
    assert (bits(at_old_bound) != bits(ref.want)).any(axis=1).sum() >= 16
    with renderer("c1") as r:
        before = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
        r._call("rt_update_spheres", N.ptr(spheres), spheres.shape[0])
        after = result(*r.ambient(ref.points, ref.streams, ref2.t_max, samples=65))
        after_old = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
    check(before, ref.want)
    check(after, ref2.want)
    check(after_old, at_old_bound)


def test_rank_context(gpu, oracle_lib):
    """A rank context (world_size 2, rank 1) returns the bits of a full context."""
    ref = run("c3", 16, 1, 65)
    with renderer("c3", rank=1, world_size=2) as r:
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
    check(got, ref.want)


def test_equals_rt_occluded_on_its_own_records(gpu, oracle_lib):
    """One c3 run: Renderer.occluded fed the restatement's records (o, dir, t_max) gives 1 - V_s
    for every sample, and the query equals the tree over those bytes' terms."""
    ref = run("c3", 16, 1, 65)
    rec = A.occlusion_records(ref.origins, ref.dirs, ref.t_max)
    with renderer("c3") as r:
        occluded = r.occluded(rec).reshape(16, 65)
        got = result(*r.ambient(ref.points, ref.streams, ref.t_max, samples=65))
    v = A.visibility(ref.t, ref.t_max)
    assert np.array_equal(occluded, 1 - v)
    check(got, G.tree(A.terms(ref.dirs, 1 - occluded)))
    check(got, ref.want)
