"""The cluster scene of the sphere group tests (tests/test_sphere_group_cpu.py,
tests/test_gpu_sphere_group.py): BVH leaves whose four slots are candidates together.

24 clusters on a 6x4 grid (spacing 6), each cluster's spheres sharing one centre, so a ray
through a cluster has a discriminant >= 0 for several slots of one leaf group:
  concentric radii 0.5 0.6 0.7 0.8 | four identical 0.6 | two identical pairs 0.5 0.5 0.8 0.8 |
  three spheres 0.4 0.6 0.8 (the leaf's fourth slot is the NaN padding sphere).
Identical spheres give equal distances, which the reference's sweep resolves to the lowest
index. A ground sphere of radius 1000 stays out of the BVH (the lone brute-force sphere). The
sphere order is shuffled with a fixed seed, so slot order differs from index order. Materials
cycle through diffuse, metal and glass: glass sends rays on from inside spheres, where the near
root is negative.
"""
import numpy as np

from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.camera import Camera
from rust_gpu_raytracing_amd.scene import RenderScene, _material, _sphere, sky_gradient_env_map, srgb_encode

RADII = [(0.5, 0.6, 0.7, 0.8), (0.6, 0.6, 0.6, 0.6), (0.5, 0.5, 0.8, 0.8), (0.4, 0.6, 0.8)]
# (texture_index, roughness, emission_power, specular, specular_scatter, glass, refraction_index)
MATERIALS = [(0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), (1, 1.0, 0.0, 1.0, 0.1, 0.0, 1.0), (2, 0.0, 0.0, 1.0, 0.0, 1.0, 1.5)]
N_RAYS = 4000


def cluster_centres():
    return np.array([[6.0 * (i - 2.5), 0.0, 6.0 * (j - 1.5)] for j in range(4) for i in range(6)], np.float32)


def cluster_spheres(ground=True, seed=5):
    """The scene's spheres (B.SPHERE), shuffled: 90 in clusters, plus the ground sphere."""
    out = []
    for k, c in enumerate(cluster_centres()):
        for r in RADII[k % 4]:
            out.append((c, r))
    if ground:
        out.append((np.array([0.0, 1001.0, 0.0], np.float32), 1000.0))  # up is -Y: under the clusters
    order = np.random.default_rng(seed).permutation(len(out))
    return np.stack([_sphere(out[i][0], out[i][1], n % len(MATERIALS)) for n, i in enumerate(order)]).astype(B.SPHERE)


def cluster_scene(width=64, height=40, ground=True):
    mats = np.stack([_material(*m) for m in MATERIALS]).astype(B.MATERIAL)
    tex = np.zeros((3, 1, 1, 4), np.uint8)
    tex[:, 0, 0, :3] = srgb_encode(np.array([[0.7, 0.3, 0.2], [0.8, 0.8, 0.9], [1.0, 1.0, 1.0]]))
    tex[..., 3] = 255
    pos = np.array([2.0, -9.0, 30.0], np.float32)
    cam = Camera(width, height, position=pos, direction=(-pos / np.linalg.norm(pos)).astype(np.float32),
                 vertical_fov=50.0)
    return RenderScene(cluster_spheres(ground), mats, [], tex, sky_gradient_env_map(64, 32), cam, name="clusters")


def cluster_rays(n=N_RAYS, seed=11):
    """(n, 6) f32 origin + direction: 70% from outside aimed near a cluster centre, 30% starting
    within 0.3 of one (inside the spheres); directions scaled by 0.5..2 (not unit length)."""
    rng = np.random.default_rng(seed)
    centres = cluster_centres().astype(np.float64)
    c = centres[rng.integers(0, len(centres), n)]
    inside = rng.random(n) < 0.3
    o = np.where(inside[:, None], c + rng.uniform(-1, 1, (n, 3)) * (0.3 / np.sqrt(3.0)),
                 c + rng.standard_normal((n, 3)) * 8.0 + np.array([0.0, -6.0, 0.0]))
    target = c + rng.standard_normal((n, 3)) * 0.35
    d = np.where(inside[:, None], rng.standard_normal((n, 3)), target - o)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0.5, 2.0, (n, 1))
    return np.concatenate([o, d], axis=1).astype(np.float32)
