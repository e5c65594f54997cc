"""Probe queries (rt_probe_sh, rt_probe_sh_device) against the CPU oracle, bit for bit.

The reference of a probe is the NumPy restatement of the contract (tests/probe_ref.py) fed the
oracle's own per_pixel: every sample is a radiance query record (origin x, the restatement's
direction, the probe's stream, first_sample = u, samples = 1) that the oracle answers as in
tests/test_gpu_gather.py, the products with the restatement's basis are reduced stripe-and-tree
per coefficient, and the oracle's ray counts are the expected segments. All comparisons are on the
u32 bit patterns of the 36 floats.

Probes: first hits of camera rays spread over the golden scenes' images (the oracle's trace_ray),
moved 0.25 along the normal into free space. The streams are a fixed permutation of 1..n, and
probe 1 has stream 0 (both seeds constant: every sample goes the same way). Probe 0 is one whose
paths bounce, so that the one-probe set is not a probe whose paths all escape at once. Against
vacuous inputs every oracle run whose loop limit exceeds 1 asserts, on the oracle's output, that
at least 10% of its probes take 1.5 or more segments per sample, and every run of 65 or more
samples that the contract's reduction differs in bits from the plain ascending sums on at least
75% of its probes and that at least 90% of its results are non-zero. References are computed once
per (scene, count, run) and shared.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer, RtError
from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from tests import gather_ref as G
from tests import probe_ref as P
from tests.golden.fixtures import CASES, load, scene_from_inputs

pytestmark = pytest.mark.gpu

GOLDEN = {"c1": "c1_64x48_b4", "c2": "c2_64x36_b8", "c3": "c3_64x36_b8"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- probes and references
@functools.lru_cache(maxsize=None)
def golden_scene(key):
    name = GOLDEN[key]
    g = load(name)
    return g, CASES[name], scene_from_inputs(g)


@functools.lru_cache(maxsize=None)
def probe_set(key, total):
    """``total`` probe positions of the golden scene ``key`` and their streams (never modified);
    prefixes of it are the smaller sets. Probe 0 is one that bounces under its stream with the
    case's settings, and probe 1 has stream 0."""
    from oracle import oracle as O

    O.build()
    g, case, scene = golden_scene(key)
    pos = P.probe_positions(G.first_hit_points(O, scene, g["camera_rays"], g["camera_origin"], total))
    pos = pos[np.random.default_rng(34).permutation(total)]
    streams = (1 + np.random.default_rng(300 + total).permutation(total)).astype(np.uint32)
    for j in range(total):
        if j == 1:
            continue  # (probe 1's stream is replaced below)
        pos[[0, j]], streams[[0, j]] = pos[[j, 0]], streams[[j, 0]]  # (the stream decides the directions)
        lights, _, segs = P.oracle_probe(O, scene, pos[:1], streams[:1], case["bounces"], 1, 5)
        if 2 * segs[0] >= 3 * 5 and bits(lights).any():
            break
        pos[[0, j]], streams[[0, j]] = pos[[j, 0]], streams[[j, 0]]
    else:
        raise AssertionError("no probe of the set bounces as probe 0")
    if total > 1:
        streams[1] = 0
    assert streams[0] != 0 and (total < 3 or (streams[2:] != 1 + np.arange(2, total)).any())
    pos.setflags(write=False)
    streams.setflags(write=False)
    return pos, streams


@functools.lru_cache(maxsize=None)
def reference(key, count, bounces, first_sample, samples, total=None):
    """(positions, streams, expected sh (count, 9, 4), expected segments per probe) for the first
    ``count`` probes of the scene's set of ``total``, computed once and shared (never modified);
    the conditions against vacuous inputs are asserted here, on the oracle's output."""
    from oracle import oracle as O

    O.build()
    _, _, scene = golden_scene(key)
    pos, streams = probe_set(key, total or count)
    pos, streams = pos[:count], streams[:count]
    lights, dirs, segs = P.oracle_probe(O, scene, pos, streams, bounces, first_sample, samples)
    t = P.terms(lights, dirs)
    want = P.tree(t)
    if bounces > 1:
        busy = int((2 * segs >= 3 * samples).sum())
        assert 10 * busy >= count, (busy, count)
    if samples >= 65:
        differ = int((bits(want) != bits(P.sequential(t))).reshape(count, -1).any(axis=1).sum())
        nonzero = int(bits(want).reshape(count, -1).any(axis=1).sum())
        assert 4 * differ >= 3 * count, (differ, count)
        assert 10 * nonzero >= 9 * count, (nonzero, count)
    for a in (want, segs):
        a.setflags(write=False)
    return pos, streams, want, segs


def renderer(key, **kw):
    g, case, scene = golden_scene(key)
    return Renderer(scene, accumulate=True, compute_per_frame=case["spp"], camera_rays=g["camera_rays"].astype(B.RAY),
                    **kw)


def check(got, segments, want, segs):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.nonzero((bits(got) != bits(want)).reshape(want.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:2]], want[bad[:2]])
    assert segments == int(segs.sum()), (segments, int(segs.sum()))


def records_of(pos, streams):
    rec = np.zeros(pos.shape[0], B.PROBE)
    rec["position"], rec["stream"] = pos, streams
    return rec


# ---------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("samples", [1, 63, 64, 65, 200])
def test_c1_sample_counts(gpu, oracle_lib, samples):
    """Sphere-only instance, 24 probes: fewer samples than the resolve's lanes, exactly one per
    lane, a second sample on one lane, and three to four samples per lane."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams, want, segs = reference("c1", 24, bounces, 1, samples)
    with renderer("c1") as r:
        got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=1, samples=samples, return_segments=True)
    check(got, n, want, segs)


@pytest.mark.parametrize("count", [1, 4, 5, 63, 65])
def test_c1_probe_counts(gpu, oracle_lib, count):
    """Probe counts at the workgroup and wave edges, 5 samples each (a resolve workgroup holds four
    probes, and a path wave's 64 items end inside a probe): prefixes of one set of 65."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams, want, segs = reference("c1", count, bounces, 1, 5, total=65)
    with renderer("c1") as r:
        got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=1, samples=5, return_segments=True)
    check(got, n, want, segs)


def runs_of(key):
    bounces = CASES[GOLDEN[key]]["bounces"]
    return [(bounces, 1, 65), (bounces, 7, 130), (1, 3, 2)]


@pytest.mark.parametrize("mode", [0, 1])
def test_c2_sphere_bvh(gpu, oracle_lib, mode):
    """Sphere BVH plus the brute-force set, 1x1 textures, in both placements: the oracle's bits,
    so the same bits in both."""
    with renderer("c2", tuning={"query_lds_mode": mode}) as r:
        for bounces, first, samples in runs_of("c2"):
            pos, streams, want, segs = reference("c2", 24, bounces, first, samples)
            got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=first, samples=samples,
                                return_segments=True)
            check(got, n, want, segs)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c3_triangles_textures_environment(gpu, oracle_lib, mode):
    """Triangles, non-1x1 textures and the environment map, in the three placements: the oracle's
    bits in each."""
    with renderer("c3", tuning={"query_lds_mode": mode}) as r:
        for bounces, first, samples in runs_of("c3"):
            pos, streams, want, segs = reference("c3", 24, bounces, first, samples)
            got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=first, samples=samples,
                                return_segments=True)
            check(got, n, want, segs)


def test_first_sample_wraps(gpu, oracle_lib):
    """first_sample = 0xFFFFFFFE with 5 samples: the sample indices wrap through 0."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams, want, segs = reference("c1", 24, bounces, 0xFFFFFFFE, 5)
    with renderer("c1") as r:
        got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=0xFFFFFFFE, samples=5, return_segments=True)
    check(got, n, want, segs)


# ---------------------------------------------------------------------------- on the GPU alone
def test_one_sample_equals_gather_with_a_zero_normal(gpu, oracle_lib):
    """200 probes at one sample: sh[i][k] equals what rt_gather returns for the point (x, normal 0)
    at the same stream and first_sample, times the restatement's b_k of the restatement's
    direction (which asserts its draws non-zero), bit for bit; the segments are equal."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams = probe_set("c1", 200)
    dirs = P.directions(streams, 9, 1)
    with renderer("c1") as r:
        lights, n_gather = r.gather(P.gather_points(pos), streams, bounces=bounces, first_sample=9, samples=1,
                                    return_segments=True)
        got, n_got = r.probe_sh(pos, streams, bounces=bounces, first_sample=9, samples=1, return_segments=True)
        # the default streams are 1 + the position in the batch; PROBE records carry their own
        plain = r.probe_sh(pos, bounces=bounces, first_sample=9, samples=1)
        same = r.probe_sh(records_of(pos, 1 + np.arange(200, dtype=np.uint32)), bounces=bounces, first_sample=9, samples=1)
    want = P.tree(P.terms(lights[:, None, :], dirs))
    assert bits(lights).any(axis=1).sum() >= 20
    bad = np.nonzero((bits(got) != bits(want)).reshape(200, -1).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:2]], want[bad[:2]])
    assert n_got == n_gather
    assert plain.tobytes() == same.tobytes() and plain.tobytes() != got.tobytes()


# ---------------------------------------------------------------------------- chunking, device entry
def test_chunking_and_device_entry_point(gpu, oracle_lib):
    """40 probes at 70 samples with one probe per launch, with fewer paths per launch than a probe
    has, staged in chunks of 7, in one launch, and through the device entry point give the same
    bits and the same segment total; the nine float4 after the last probe's row are not written
    and the counter is added to."""
    import torch

    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams = probe_set("c1", 65)
    q = records_of(pos[:40], streams[:40])
    with renderer("c1", tuning={"probe_chunk": 70}) as r:
        single, n_single = r.probe_sh(q, bounces=bounces, samples=70, return_segments=True)
        r.set_tuning("probe_chunk", 50)
        small, n_small = r.probe_sh(q, bounces=bounces, samples=70, return_segments=True)
        r.set_tuning("probe_chunk", 1048576)
        r.set_tuning("query_chunk", 7)
        staged, n_staged = r.probe_sh(q, bounces=bounces, samples=70, return_segments=True)
        r.set_tuning("query_chunk", 65536)
        base, n_base = r.probe_sh(q, bounces=bounces, samples=70, return_segments=True)
        t = torch.from_numpy(q.view(np.float32).reshape(-1, 4)).to(gpu)
        dev, n_dev = r.probe_sh(t, bounces=bounces, samples=70, return_segments=True)
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (40, 9, 4)
        dev_host = dev.cpu().numpy()
        # the caller's buffer with one probe's row to spare, and a counter that is added to
        room = torch.full((41, 9, 4), -7.25, dtype=torch.float32, device=gpu)
        counter = torch.full((1,), 1000, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize(gpu)
        r._call("rt_probe_sh_device", ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(room.data_ptr()), 40, bounces,
                1, 70, ctypes.c_void_p(counter.data_ptr()))
        r.synchronize()
        room_host, counted = room.cpu().numpy(), int(counter.item())
    assert bits(base).reshape(40, -1).any(axis=1).sum() >= 36 and n_base >= 40 * 70
    assert single.tobytes() == base.tobytes() and n_single == n_base
    assert small.tobytes() == base.tobytes() and n_small == n_base
    assert staged.tobytes() == base.tobytes() and n_staged == n_base
    assert dev_host.tobytes() == base.tobytes() and n_dev == n_base
    assert room_host[:40].tobytes() == base.tobytes()
    assert np.array_equal(bits(room_host[40]), bits(np.full((9, 4), -7.25, np.float32)))
    assert counted == 1000 + n_base


# ---------------------------------------------------------------------------- semantics
def test_zero_bounces_and_errors(gpu):
    pos, streams = probe_set("c1", 65)
    with renderer("c1") as r:
        got, n = r.probe_sh(pos, streams, bounces=0, samples=3, return_segments=True)
        assert got.shape == (65, 9, 4) and not bits(got).any() and n == 0
        for samples in (0, 16777217):
            with pytest.raises(RtError) as e:
                r.probe_sh(pos, streams, samples=samples)
            assert e.value.code == N.RT_E_INVALID
        with pytest.raises(RtError) as e:
            r.set_tuning("probe_chunk", 0)
        assert e.value.code == N.RT_E_INVALID
        lib, ctx = r._lib, r._ctx
        q = records_of(pos[:4], streams[:4])
        out = np.zeros((4, 9, 4), np.float32)
        seg = ctypes.c_uint64(5)
        assert lib.rt_probe_sh(ctx, None, N.ptr(out), 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert b"NULL" in lib.rt_last_error(ctx)
        assert lib.rt_probe_sh(ctx, N.ptr(q), None, 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh(ctx, N.ptr(q), N.ptr(out), 4, 4, 1, 0, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh(ctx, N.ptr(q), N.ptr(out), 4, 4, 1, 16777217, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh(ctx, None, None, 0, 4, 1, 0, None) == N.RT_E_INVALID  # whatever count is
        assert not bits(out).any()
        assert lib.rt_probe_sh(ctx, None, None, 0, 4, 1, 1, ctypes.byref(seg)) == N.RT_OK
        assert seg.value == 0
        assert lib.rt_probe_sh(ctx, N.ptr(q), N.ptr(out), 4, 4, 1, 1, None) == N.RT_OK  # segments may be NULL
        assert bits(out).any()
        assert lib.rt_probe_sh_device(ctx, None, None, 0, 4, 1, 1, None) == N.RT_OK
        assert lib.rt_probe_sh_device(ctx, None, None, 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh_device(ctx, None, None, 4, 4, 1, 0, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh_device(ctx, None, None, 0, 4, 1, 16777217, None) == N.RT_E_INVALID
        # host memory is not device memory of the context's device
        assert lib.rt_probe_sh_device(ctx, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(out.ctypes.data), 4, 4, 1, 1,
                                      None) == N.RT_E_INVALID
        assert r.probe_sh(np.zeros((0, 3), np.float32)).shape == (0, 9, 4)
        with pytest.raises(ValueError):
            r.probe_sh(q, streams[:4])
        with pytest.raises(ValueError):
            r.probe_sh(pos[:, :2])
        with pytest.raises(ValueError):
            r.probe_sh(pos, streams[:3])


def test_misaligned_device_pointers_are_refused(gpu):
    import torch

    pos, streams = probe_set("c1", 65)
    q = records_of(pos[:4], streams[:4])
    with renderer("c1") as r:
        t = torch.zeros(4 * 4 + 8, dtype=torch.float32, device=gpu)
        t[:16] = torch.from_numpy(q.view(np.float32).copy()).to(gpu)
        out = torch.zeros(4 * 36 + 8, dtype=torch.float32, device=gpu)
        cnt = torch.zeros(4, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize(gpu)
        lib, ctx = r._lib, r._ctx
        V = ctypes.c_void_p
        assert lib.rt_probe_sh_device(ctx, V(t.data_ptr() + 4), V(out.data_ptr()), 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh_device(ctx, V(t.data_ptr()), V(out.data_ptr() + 8), 4, 4, 1, 1, None) == N.RT_E_INVALID
        assert lib.rt_probe_sh_device(ctx, V(t.data_ptr()), V(out.data_ptr()), 4, 4, 1, 1,
                                      V(cnt.data_ptr() + 4)) == N.RT_E_INVALID
        r.synchronize()
        assert not bool(out.any())
        assert lib.rt_probe_sh_device(ctx, V(t.data_ptr()), V(out.data_ptr()), 4, 4, 1, 1, V(cnt.data_ptr())) == N.RT_OK
        r.synchronize()
        assert not bool(out[144:].any()) and bool(out[:144].any())


# ---------------------------------------------------------------------------- carried over
@pytest.mark.parametrize("batch", [1, 16])
def test_probe_does_not_disturb_a_render(gpu, batch):
    """The golden case c2_64x36_b8 with a 24-probe bake between the compute_frame calls, with one
    launch per frame and with a frame queue of 16: accumulation, output, k and ray count equal the
    golden's, and a queued frame stays queued."""
    g, case, scene = golden_scene("c2")
    pos, streams = probe_set("c2", 24)
    with Renderer(scene, accumulate=bool(case["accumulate"]), compute_per_frame=case["spp"],
                  camera_rays=g["camera_rays"].astype(B.RAY), frame_batch=batch) as r:
        for i in range(case["frames"]):
            r.compute_frame(case["bounces"])
            if i + 1 < case["frames"]:
                before = r.frame_batch(), r.accumulation_index
                got = r.probe_sh(pos, streams, bounces=case["bounces"], samples=70)
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
    assert got.shape == (24, 9, 4) and bits(got).any()
    assert k == k_plain
    assert n == int(g["rays"])
    assert np.array_equal(out, g["out"])
    assert np.array_equal(acc.view(np.uint32), g["accum"].view(np.uint32))


def test_sees_the_scene_as_of_the_call(gpu, oracle_lib):
    """After rt_update_materials (one material's emission_power) and rt_upload_textures (one
    layer's colour) the bake equals the restatement over the oracle's lights on the edited scene
    and differs from the earlier result."""
    bounces = CASES[GOLDEN["c1"]]["bounces"]
    pos, streams, want, segs = reference("c1", 24, bounces, 1, 65)
    _, _, scene = golden_scene("c1")
    materials = np.ascontiguousarray(scene.materials.copy())
    textures = np.ascontiguousarray(np.array(scene.textures, np.uint8))
    lit = int(np.argmin(materials["emission_power"]))  # a material that does not emit yet
    materials["emission_power"][lit] = np.float32(2.5)
    layer = int(materials["texture_index"][(lit + 1) % materials.shape[0]])
    textures[layer, ..., :3] = (200, 40, 90)
    edited = dataclasses.replace(scene, materials=materials, textures=textures)
    edited.flatten = scene.flatten
    with renderer("c1") as r:
        before, n_before = r.probe_sh(pos, streams, bounces=bounces, samples=65, return_segments=True)
        check(before, n_before, want, segs)
        r.scene = edited
        r._call("rt_update_materials", N.ptr(materials), materials.shape[0])
        r._upload_textures()
        after, n_after = r.probe_sh(pos, streams, bounces=bounces, samples=65, return_segments=True)
    lights2, dirs2, segs2 = P.oracle_probe(oracle_lib, edited, pos, streams, bounces, 1, 65)
    check(after, n_after, P.tree(P.terms(lights2, dirs2)), segs2)
    assert after.tobytes() != before.tobytes()


def test_rank_context(gpu, oracle_lib):
    """A rank context (world_size 2, rank 1) returns the bits of a full context."""
    bounces = CASES[GOLDEN["c3"]]["bounces"]
    pos, streams, want, segs = reference("c3", 24, bounces, 7, 130)
    with renderer("c3", rank=1, world_size=2) as r:
        got, n = r.probe_sh(pos, streams, bounces=bounces, first_sample=7, samples=130, return_segments=True)
    check(got, n, want, segs)
