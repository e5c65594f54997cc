"""The ray domain include/rt_abi.h promises (finite components, |direction| in [1e-5, 1e5],
|origin| <= 1e15) at its edges, on every walk, bit for bit against the CPU oracle.

Rays: the four sets of tests/ray_domain.py, 300 rays each per scene -- |d| at 1.01e-5, 1e-3, 1,
1e3 and 0.99e5; one or two components scaled down to denormals and signed zeros; origins 1e3, 1e5
and 1e7 from the geometry; origins inside boxes and spheres and within 1e-4 of surfaces. The
quantities in units of the ray parameter (t_max, the K-nearest insertion bound, the pruning
limit) scale by 1/|d|, so t runs from about 1e-10 to 1e12 here.

Scenes: C1 (sphere-only kernel, v_rcp_f32), C2 (sphere BVH in LDS), C3 with a small environment
map and textures (triangle accelerator and spheres in LDS), C5 at 40x20 cells (the
global-memory triangle walk). No tolerance appears anywhere. Before any GPU run the oracle's
answers are asserted not to be degenerate: per (scene, set) at least 25% hits and 5% misses, at
least 20 rays won by each kind where a scene has both, at most 1% of the rays dropped for a NaN
distance (the occlusion and hit-list references are defined for NaN-free distances only).
References are computed once per scene and shared, never modified.
"""
import copy
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests import denoise_ref as R
from tests import hits_ref as H
from tests import ray_domain as RD
from tests.test_gpu_denoise import assert_features_equal
from tests.test_gpu_hits import same
from tests.test_gpu_occlusion import check, expected, next_up
from tests.test_gpu_parity import assert_same, gpu_render, oracle_frames
from tests.test_gpu_query import check_hits, oracle_records
from tests.test_gpu_radiance import check as check_radiance
from tests.test_gpu_radiance import oracle_radiance

pytestmark = pytest.mark.gpu

F32_MAX = np.float32(3.4028235e38)
INF = np.float32(np.inf)
PER_SET = 300
WIDTH, HEIGHT = 40, 30  # a frame of 1,200 pixels: as many rays as the four sets hold

# scene -> (config, build arguments, the placement that reaches the walk under test: tuning
# "query_lds_mode" of the queries, "lds_mode" of the frames)
SCENES = {
    "c1": ("c1_four_spheres", {}, {}, {}),
    "c2": ("c2_rtiow", {}, {"query_lds_mode": 1}, {}),
    "c3": ("c3_chess", dict(env_size=(16, 8), texture_size=(8, 8)), {"query_lds_mode": 2}, {}),
    "c5": ("c5_heightfield", dict(nx=40, nz=20), {"query_lds_mode": 1}, {"lds_mode": 1}),
}
KEYS = sorted(SCENES)


def build(key):
    config, kw, _, _ = SCENES[key]
    return build_config(config, width=WIDTH, height=HEIGHT, **kw)[0]


def query_tunings(key):
    """The default (small batches read the scene from global memory) and the scene's placement."""
    return [t for i, t in enumerate(({}, SCENES[key][2])) if i == 0 or t]


def assert_not_degenerate(scene, ref, where, kinds=True):
    """The conditions on the oracle's answers; returns the rays to keep (no NaN distance) and
    the counts (hits, misses, dropped)."""
    t = ref["rec"]["t"]
    n = t.shape[0]
    nan = np.isnan(t)
    hit = ~nan & (t != F32_MAX)
    miss = t == F32_MAX
    assert 4 * hit.sum() >= n and 20 * miss.sum() >= n and 100 * nan.sum() <= n, (where, hit.sum(), miss.sum(), nan.sum())
    if kinds and scene.spheres.shape[0] and scene.objects:
        with np.errstate(invalid="ignore"):
            sphere = hit & (ref["hs_t"] < ref["ht_t"])
        assert sphere.sum() >= 20 and (hit & ~sphere).sum() >= 20, (where, sphere.sum(), (hit & ~sphere).sum())
    return ~nan, (int(hit.sum()), int(miss.sum()), int(nan.sum()))


@functools.lru_cache(maxsize=None)
def reference(key):
    """(scene, rays, oracle reference, counts per set) of one scene: the four sets, their rays
    with a NaN oracle distance dropped."""
    from oracle import oracle as O

    O.build()
    scene = build(key)
    geo = RD.scene_geometry(1, scene)
    rays, refs, counts = [], [], {}
    for i, name in enumerate(RD.SETS):
        part = RD.ray_set(name, 100 + i, PER_SET, geo)
        ref = oracle_records(O, scene, part)
        keep, counts[name] = assert_not_degenerate(scene, ref, (key, name))
        rays.append(part[keep])
        refs.append({k: v[keep] for k, v in ref.items()})
    rays = np.concatenate(rays)
    ref = {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}
    rays.setflags(write=False)
    for v in ref.values():
        v.setflags(write=False)
    print(f"ray domain {key}: (hits, misses, dropped) {counts}")
    return scene, rays, ref, counts


# ---------------------------------------------------------------------------- the queries
@pytest.mark.parametrize("key", KEYS)
def test_trace_rays(gpu, oracle_lib, key):
    """rt_trace_rays: every record equals the oracle's, in the default placement and the scene's
    own, and on C3 and C5 with triangle pruning off and in the brute-force mode."""
    scene, rays, ref, _ = reference(key)
    runs = [(t, None) for t in query_tunings(key)]
    if scene.objects:
        runs += [(SCENES[key][2], "prune0"), (SCENES[key][2], "brute")]
    for tuning, variant in runs:
        with Renderer(scene, tuning=tuning) as r:
            if variant == "prune0":
                r.set_triangle_pruning(0)
            elif variant == "brute":
                r.set_brute_force(True)
            hits = r.trace_rays(rays)
        check_hits(oracle_lib, scene, rays, hits, ref)


@pytest.mark.parametrize("key", KEYS)
def test_occluded(gpu, key):
    """rt_occluded with t_max cycling through t, next_up(t), t / 2, 2 t and +inf of the oracle's
    distance t: the walk culls by t_max from the first node, and t spans 1e-10 .. 1e12."""
    scene, rays, ref, _ = reference(key)
    t = ref["rec"]["t"]
    with np.errstate(over="ignore"):
        cycle = np.stack([t, next_up(t), t / np.float32(2), t * np.float32(2), np.full_like(t, INF)])
    batch = np.zeros((rays.shape[0], 7), np.float32)
    batch[:, :6] = rays
    batch[:, 6] = cycle[np.arange(t.shape[0]) % 5, np.arange(t.shape[0])]
    want = expected(t, batch[:, 6])
    hit = t != F32_MAX
    for k in range(5):  # each t_max decides hits of the set: 0 at t and t / 2, else 1
        assert (want[hit & (np.arange(t.shape[0]) % 5 == k)] == (0 if k in (0, 2) else 1)).all()
        assert (hit & (np.arange(t.shape[0]) % 5 == k)).sum() >= 50
    for tuning in query_tunings(key):
        with Renderer(scene, tuning=tuning) as r:
            check(r.occluded(batch), want)
            if scene.objects:
                r.set_triangle_pruning(0)
                check(r.occluded(batch), want)


@functools.lru_cache(maxsize=None)
def hits_reference(key):
    """The 16-entry hit lists of the scene's rays, t_max alternating between +inf and 4 x the
    oracle's closest distance (a bound that cuts lists short without emptying them)."""
    from oracle import oracle as O

    scene, rays, ref, _ = reference(key)
    t = ref["rec"]["t"]
    with np.errstate(over="ignore"):
        t_max = np.where(np.arange(t.shape[0]) % 2 == 0, INF, t * np.float32(4)).astype(np.float32)
    h = H.HitsRef(O, scene)
    cand = h.lists(rays, t_max)
    hits, counts, total = h.records(rays, t_max, lists=cand)
    # the closest entry is the oracle's closest hit
    assert np.array_equal(hits["t"][:, 0].view(np.uint32), t.view(np.uint32))
    return t_max, hits, counts, total


@pytest.mark.parametrize("key", KEYS)
def test_trace_hits(gpu, key):
    """rt_trace_hits with 4 and 16 entries against the restated contract, entry by entry."""
    scene, rays, _, _ = reference(key)
    t_max, hits, counts, total = hits_reference(key)
    assert (total > 1).sum() >= 100  # lists with an order to get right
    for tuning in query_tunings(key):
        with Renderer(scene, tuning=tuning) as r:
            for k in (4, 16):
                same(r.trace_hits(rays, t_max=t_max, max_hits=k), (hits, counts), k)


@pytest.mark.parametrize("key", KEYS)
def test_radiance(gpu, oracle_lib, key):
    """rt_radiance, 2 bounces, 1 sample: the first segment carries the set's direction, the rest
    are the kernel's own rays from the far or near hit points. Against the oracle's per_pixel."""
    scene, rays, _, _ = reference(key)
    streams = np.random.default_rng(5).permutation(rays.shape[0]).astype(np.uint32)
    want, segs = oracle_radiance(oracle_lib, scene, rays, streams, 2, 1, 1)
    assert 4 * (segs >= 2).sum() >= rays.shape[0]
    for tuning in query_tunings(key):
        with Renderer(scene, tuning=tuning) as r:
            got, n = r.radiance(rays, streams, bounces=2, first_sample=1, samples=1, return_segments=True)
        check_radiance(got, n, want, segs)


# ---------------------------------------------------------------------------- frames and features
@functools.lru_cache(maxsize=None)
def frame_reference(key, far):
    """(scene, ray buffer, rays, oracle records, oracle features, oracle frames) of a frame whose
    camera rays are in-domain directions from one origin: the scene's own camera position, or
    (``far``) a point 1e5 beside the scene."""
    from oracle import oracle as O

    O.build()
    scene = copy.deepcopy(build(key))
    geo = RD.scene_geometry(1, scene)
    if far:
        # level with the scene: the rays run nearly along an axis, so those with their two small
        # components scaled down still cross the scene, and some pass over a ground sphere
        u = np.array([1.0, 0.0, 0.0])
        centre = 0.5 * (np.asarray(geo.region[0]) + np.asarray(geo.region[1]))
        scene.camera.position = (centre + 1e5 * u).astype(np.float32)
    rays = RD.from_one_origin(200 + int(far), WIDTH * HEIGHT, scene.camera.position, geo.region, geo.targets,
                              wide=0.4 if far else 0.2)
    ref = oracle_records(O, scene, rays)
    keep, counts = assert_not_degenerate(scene, ref, (key, "far" if far else "near"), kinds=False)
    assert keep.all()  # (a frame cannot drop a pixel)
    buf = np.zeros(WIDTH * HEIGHT, B.RAY)
    buf["direction"] = rays[:, 3:]
    feats = R.oracle_features(O, scene, camera_rays=buf)
    frames = oracle_frames(O, scene, 4, 2, buf)
    print(f"ray domain frame {key} far={far}: (hits, misses, dropped) {counts}")
    return scene, buf, rays, ref, feats, frames


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("key", KEYS)
def test_frames(gpu, oracle_lib, key, far):
    """2 accumulated frames of 4 bounces of a 40x30 frame whose camera rays are in-domain
    directions: accumulation, output and ray count equal the oracle's, with and (scenes with
    triangles) without the primary pre-pass."""
    scene, buf, _, _, _, frames = frame_reference(key, far)
    base = SCENES[key][3]
    tunings = [dict(base, primary_pass=1), dict(base, primary_pass=0)] if scene.objects else [base]
    for tuning in tunings:
        assert_same(*gpu_render(scene, 4, 2, rays=buf, tuning=tuning), *frames)


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("key", KEYS)
def test_features(gpu, oracle_lib, key, far):
    """rt_compute_features on the same camera rays: the planes equal the oracle-built ones, and
    the ID plane holds kind and index of the records rt_trace_rays returns, themselves checked
    against the oracle."""
    scene, buf, rays, ref, feats, _ = frame_reference(key, far)
    with Renderer(scene, camera_rays=buf, tuning=SCENES[key][3]) as r:
        got = r.features()
        ids = r.feature_ids()
        hits = r.trace_rays(rays)
    assert_features_equal(got, feats)
    check_hits(oracle_lib, scene, rays, hits, ref)
    assert np.array_equal(ids[..., 0].reshape(-1), hits["kind"])
    assert np.array_equal(ids[..., 1].reshape(-1), hits["index"])
