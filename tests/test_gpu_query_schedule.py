"""The counter-dealt half of the query kernels' chunk schedule (claim_chunk, csrc/rt_query_frame.h).

A wave of the occlusion, radiance and gather kernels takes its first chunk of rays by its own index
in the launch and every later chunk from one device counter, which hands out the rays from
``claimed_from`` = first_chunk x the launch's waves on; the closest-hit kernel takes every chunk
from the counter. Each test makes one device call of N rays that must reach the counter and
compares it, bit for bit, with the same rays submitted in consecutive calls of 4,096 rays. A call
of 4,096 rays launches 64 waves whose first chunks of 64 rays cover it (claimed_from >= count), so
the any-hit, radiance and gather references never touch the counter; a ray's answer depends on
its record alone (the radiance stream and the gather stream travel in the record).

Why N = 2^20 + 77 reaches the counter: a CU holds at most 32 wave64s (8 workgroups of 256 threads,
or 2 of 1,024), so the 256 CUs of an MI355X hold at most 8,192 waves of a launch. The first chunk
is count / waves / 2 rounded down to whole waves, at least 64: with any number of waves from
4,096 to 8,192 that is 64 rays at this N, so the first chunks cover at most 8,192 x 64 = 2^19 rays,
half of N, and the counter deals the rest (with fewer than 4,096 waves the first chunks are
count / waves / 2 < N / 2 rays by construction). A device with more CUs gets N scaled by
ceil(CUs / 256), which keeps the dealt share at a half or more -- above the third that is asked
for. The gather case has 16,385 points x 64 stripes = 2^20 + 64 items (again scaled by the CUs).
"""
import numpy as np
import pytest

from rust_gpu_raytracing_amd import Renderer
from rust_gpu_raytracing_amd.scene import build_config

pytestmark = pytest.mark.gpu

N_RAYS = (1 << 20) + 77
N_POINTS = 16_385
PART = 4_096  # rays per reference call: 64 waves x their own first chunk of 64 rays


def _scale(gpu):
    import torch

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    return max(1, -(-cus // 256))


def _scene():
    return build_config("c1_four_spheres", width=37, height=21)[0]


def _rays(scene, n, seed):
    """(n, 8) float32 records: camera rays of the scene, origins and directions jittered."""
    rng = np.random.default_rng(seed)
    d = scene.camera.recalculate_ray_directions()["direction"].astype(np.float32)
    rec = np.zeros((n, 8), np.float32)
    rec[:, :3] = np.asarray(scene.camera.position, np.float32) + rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    rec[:, 4:7] = d[rng.integers(0, d.shape[0], n)] + rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    return rec


def _in_parts(call, records, per_part):
    import torch

    return torch.cat([call(records[i:i + per_part]) for i in range(0, records.shape[0], per_part)])


def _same(whole, parts):
    import torch

    assert whole.shape == parts.shape and whole.dtype == parts.dtype
    if not torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)):
        bad = torch.nonzero((whole != parts).reshape(whole.shape[0], -1).any(dim=1)).flatten()
        raise AssertionError((int(bad.numel()), bad[:8].tolist()))


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_closest_hit_whole_equals_parts(gpu, mode):
    import torch

    scene = _scene()
    rays = torch.from_numpy(_rays(scene, N_RAYS * _scale(gpu), 31)).to(gpu)
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        whole = r.trace_rays(rays)
        parts = _in_parts(r.trace_rays, rays, PART)
        r.synchronize()
    _same(whole, parts)
    kind = whole[:, 11]
    assert bool((kind == 1).any()) and bool((kind == 0).any())


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_occlusion_whole_equals_parts(gpu, mode):
    import torch

    scene = _scene()
    rec = _rays(scene, N_RAYS * _scale(gpu), 32)
    rng = np.random.default_rng(33)
    rec[:, 7] = rng.uniform(0.5, 8.0, rec.shape[0]).astype(np.float32)  # t_max: decides both ways
    rec[::5, 7] = np.inf
    rays = torch.from_numpy(rec).to(gpu)
    with Renderer(scene, tuning={"query_lds_mode": mode}) as r:
        whole = r.occluded(rays)
        parts = _in_parts(r.occluded, rays, PART)
        r.synchronize()
    _same(whole, parts)
    assert int(whole.max()) == 1 and int(whole.min()) == 0
    share = float(whole.float().mean())
    assert 0.05 < share < 0.95, share


def test_radiance_whole_equals_parts(gpu):
    import torch

    scene = _scene()
    rec = _rays(scene, N_RAYS * _scale(gpu), 34)
    rec.view(np.uint32)[:, 3] = np.arange(rec.shape[0], dtype=np.uint32)  # the stream: the ray's index
    rays = torch.from_numpy(rec).to(gpu)
    with Renderer(scene) as r:
        call = lambda x: r.radiance(x, bounces=2, first_sample=1, samples=1)  # noqa: E731
        whole, segs = r.radiance(rays, bounces=2, first_sample=1, samples=1, return_segments=True)
        parts = _in_parts(call, rays, PART)
        r.synchronize()
    _same(whole, parts)
    assert rays.shape[0] <= segs <= 2 * rays.shape[0]
    assert bool((whole[:, :3] > 0).any())


def test_gather_whole_equals_parts(gpu):
    import torch

    scene = _scene()
    n = N_POINTS * _scale(gpu)
    rng = np.random.default_rng(35)
    rec = np.zeros((n, 8), np.float32)
    # points just above the ground sphere's top (y = 0.5; the scene's up is -y), normals up
    rec[:, 0], rec[:, 2] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    rec[:, 1] = 0.499
    rec[:, 4:7] = np.array([0, -1, 0], np.float32) + rng.normal(0, 0.1, (n, 3)).astype(np.float32)
    rec.view(np.uint32)[:, 3] = 1 + np.arange(n, dtype=np.uint32)
    points = torch.from_numpy(rec).to(gpu)
    with Renderer(scene, tuning={"gather_chunk": n}) as r:  # one launch of all n x 64 items
        call = lambda x: r.gather(x, bounces=2, first_sample=1, samples=64)  # noqa: E731
        whole = r.gather(points, bounces=2, first_sample=1, samples=64)
        parts = _in_parts(call, points, PART // 64)  # 64 points x 64 stripes = 4,096 items
        r.synchronize()
    _same(whole, parts)
    assert bool((whole[:, :3] > 0).any())
