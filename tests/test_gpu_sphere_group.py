"""The sphere group test's root passes on the GPU: leaf groups whose four slots are candidates
together (tests/sphere_cluster_scene.py; tests/test_sphere_group_cpu.py shows on the CPU that the
scene's rays do visit leaf groups with 2, 3 and 4 candidates).

Ray queries and occlusion queries on the scene's 4,000 rays against the CPU oracle, record for
record, and the path tracer's frames bit for bit (accumulation, RGBA8, ray count), with the
ground sphere (the lone brute-force sphere) and without it. The oracle references are computed
once and shared.
"""
import functools

import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from tests.sphere_cluster_scene import cluster_rays, cluster_scene
from tests.test_gpu_occlusion import check_variants
from tests.test_gpu_parity import assert_same, gpu_render, oracle_frames
from tests.test_gpu_query import F32_MAX, check_hits, oracle_records

pytestmark = pytest.mark.gpu

W, H, BOUNCES, FRAMES = 64, 40, 6, 3


@functools.lru_cache(maxsize=None)
def query_reference():
    """(scene, rays, oracle records) of the cluster scene's ray set (never modified)."""
    from oracle import oracle as O

    O.build()
    scene, rays = cluster_scene(W, H), cluster_rays()
    ref = oracle_records(O, scene, rays)
    t = ref["rec"]["t"]
    assert not np.isnan(t).any() and (t == F32_MAX).any() and (t != F32_MAX).sum() > 2000
    return scene, rays, ref


@functools.lru_cache(maxsize=None)
def frame_reference(ground):
    from oracle import oracle as O

    O.build()
    scene = cluster_scene(W, H, ground=ground)
    rays = scene.camera.recalculate_ray_directions()
    return scene, rays, oracle_frames(O, scene, BOUNCES, FRAMES, rays)


def test_trace_rays_match_oracle(gpu, oracle_lib):
    """Every one of the 4,000 rays: bytes 0-43 of the record, kind, index, and the one-sphere cut."""
    scene, rays, ref = query_reference()
    with Renderer(scene) as r:
        hits = r.trace_rays(rays)
    assert hits.shape == (rays.shape[0],)
    check_hits(oracle_lib, scene, rays, hits, ref)
    # equal distances (identical spheres) went to the lower index: the oracle's sweep keeps the first
    sph = scene.spheres
    hit = np.nonzero(hits["kind"] == 1)[0]
    twin = [i for i in hit if ((sph["position"] == sph["position"][hits["index"][i]]).all(axis=1) &
                               (sph["radius"] == sph["radius"][hits["index"][i]])).sum() > 1]
    assert len(twin) > 200
    for i in twin:
        same = np.nonzero((sph["position"] == sph["position"][hits["index"][i]]).all(axis=1) &
                          (sph["radius"] == sph["radius"][hits["index"][i]]))[0]
        assert hits["index"][i] == same.min()


@pytest.mark.parametrize("batch", [None, 1])
@pytest.mark.parametrize("ground", [True, False], ids=["ground", "no_ground"])
def test_path_tracer_matches_oracle(gpu, ground, batch):
    """64x40, 6 bounces, 3 accumulated frames, with the default frame queue and one launch per
    frame; without the ground sphere the brute-force set is empty."""
    scene, rays, (acc_o, out_o, n_o) = frame_reference(ground)
    acc, out, n = gpu_render(scene, BOUNCES, FRAMES, rays=rays, frame_batch=batch)
    assert_same(acc, out, n, acc_o, out_o, n_o)


def test_occluded_matches_oracle(gpu):
    """rt_occluded on the same rays: every t_max variant of tests/test_gpu_occlusion.py."""
    scene, rays, ref = query_reference()
    with Renderer(scene) as r:
        check_variants(r, rays, ref["rec"]["t"])
