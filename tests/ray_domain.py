"""Ray sets at the edges of the domain include/rt_abi.h promises exactness for: finite
components, |direction| in [1e-5, 1e5], |origin| <= 1e15.

Four sets, each a fixed function of its seed: ``length_edges`` (|d| just inside both ends of
the domain and between them), ``mixed_components`` (one or two components scaled down as far as
denormals and signed zeros while the third carries the length), ``far_origins`` (origins 1e3,
1e5 and 1e7 from the geometry) and ``near_and_inside`` (origins inside boxes and spheres and
within 1e-4 of surfaces). Every set asserts, on |d| computed in float64 from the f32
components, that it stays inside the domain. Shared by the CPU harness tests
(tests/test_tri_accel_cpu.py, tests/test_sphere_bvh_cpu.py) and tests/test_gpu_ray_domain.py.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

D_MIN, D_MAX, O_MAX = 1e-5, 1e5, 1e15
# |d| just inside each end of the domain and in the middle, in equal shares
LENGTHS = np.array([1.01e-5, 1e-3, 1.0, 1e3, 0.99e5])
FAR_RADII = (1e3, 1e5, 1e7)
BIG_RADIUS = 100.0  # spheres beyond this (grounds) do not shape the region


class Geometry(NamedTuple):
    """What the generators need of a scene: the bounding ``region`` (lo, hi) of everything but
    ground-sized spheres, ``targets`` (m, 3) on the surfaces with their unit ``normals``, the
    object and sub-object ``boxes`` (k, 2, 3) and the ``spheres`` (s, 4: centre, radius)."""
    region: tuple
    targets: np.ndarray
    normals: np.ndarray
    boxes: np.ndarray
    spheres: np.ndarray


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def geometry(seed, spheres=None, objs=None, subs=None, tris=None, n_targets=2048):
    """The ``Geometry`` of sphere records and flattened triangle buffers (either may be absent).
    Targets are drawn half from each kind present: uniform points of random triangles, and
    points of the sphere surfaces (of a ground-sized sphere, the part next to the region)."""
    rng = np.random.default_rng(seed)
    sph = np.zeros((0, 4))
    if spheres is not None and spheres.shape[0]:
        sph = np.concatenate([spheres["position"], spheres["radius"][:, None]], axis=1).astype(np.float64)
    pts = []
    if tris is not None and tris.shape[0]:
        a = tris["a"].astype(np.float64)
        pts += [a, a + tris["edge_ab"], a + tris["edge_ac"]]
    small = sph[sph[:, 3] <= BIG_RADIUS]
    if small.shape[0]:
        pts += [small[:, :3] - small[:, 3:], small[:, :3] + small[:, 3:]]
    pts = np.concatenate(pts)
    lo, hi = pts.min(0), pts.max(0)
    tgt, nrm = [], []
    kinds = (tris is not None and tris.shape[0] > 0) + (sph.shape[0] > 0)
    if tris is not None and tris.shape[0]:
        m = n_targets // kinds
        i = rng.integers(0, tris.shape[0], m)
        u, v = rng.uniform(0, 1, m), rng.uniform(0, 1, m)
        flip = u + v > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        tgt.append(tris["a"][i] + u[:, None] * tris["edge_ab"][i] + v[:, None] * tris["edge_ac"][i])
        fn = tris["face_normal"][i].astype(np.float64)
        nrm.append(fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30))
    if sph.shape[0]:
        m = n_targets - sum(t.shape[0] for t in tgt)
        s = sph[rng.integers(0, sph.shape[0], m)]
        n = _unit(rng, m)
        big = s[:, 3] > BIG_RADIUS  # the point of the ground below (above) a point of the region
        toward = rng.uniform(lo, hi, (m, 3)) - s[:, :3]
        toward /= np.linalg.norm(toward, axis=1, keepdims=True)
        n = np.where(big[:, None], toward, n)
        tgt.append(s[:, :3] + s[:, 3:] * n)
        nrm.append(n)
    boxes = np.zeros((0, 2, 3))
    if objs is not None and objs.shape[0]:
        boxes = np.concatenate([np.stack([objs["min_bounds"], objs["max_bounds"]], axis=1),
                                np.stack([subs["min_bounds"], subs["max_bounds"]], axis=1)]).astype(np.float64)
    order = rng.permutation(n_targets)
    return Geometry((lo, hi), np.concatenate(tgt)[order], np.concatenate(nrm)[order], boxes, sph)


def scene_geometry(seed, scene, **kw):
    objs, subs, tris = scene.flatten()
    return geometry(seed, scene.spheres, objs, subs, tris, **kw)


# ---------------------------------------------------------------------------- pieces
def length_of(d):
    """|d| in float64 from the f32 components."""
    return np.linalg.norm(np.asarray(d, np.float32).astype(np.float64), axis=1)


def rescale(d, want):
    """Each direction times one f32 factor that brings its length to ``want``."""
    d = np.asarray(d, np.float32)
    out = d.copy()
    for _ in range(2):  # (a factor beyond f32's range is applied in two steps)
        f = (want / length_of(out)).astype(np.float32)
        assert np.isfinite(f).all() and (f > 0).all()
        out = (out * f[:, None]).astype(np.float32)
    return out


def in_domain(rays):
    """The set as (n, 6) float32, asserted to lie inside the documented domain."""
    rays = np.ascontiguousarray(rays, np.float32)
    assert rays.ndim == 2 and rays.shape[1] == 6 and np.isfinite(rays).all()
    ln = length_of(rays[:, 3:])
    assert (ln >= D_MIN).all() and (ln <= D_MAX).all(), (ln.min(), ln.max())
    assert (length_of(rays[:, :3]) <= O_MAX).all()
    return rays


def edge_lengths(rng, n):
    """The five lengths in equal shares, in random order."""
    return LENGTHS[rng.permutation(n) % LENGTHS.size]


def aimed(rng, n, region, targets, wide=0.2):
    """Origins around the region (it grown by half its size on every side) and directions
    to points on the geometry; a share ``wide`` of them to points up to half the region's
    diagonal off it, so that a set holds misses too. Returns float64 (origins, aim points)."""
    lo, hi = (np.asarray(x, np.float64) for x in region)
    size = np.maximum(hi - lo, 1.0)
    o = rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (n, 3))
    t = targets[rng.integers(0, targets.shape[0], n)].astype(np.float64)
    off = np.where(rng.uniform(0, 1, n) < wide, 0.5 * np.linalg.norm(size), 1e-3)
    t = t + off[:, None] * rng.uniform(0, 1, (n, 1)) * _unit(rng, n)
    return o, t


# ---------------------------------------------------------------------------- the four sets
def length_edges(seed, n, region, targets):
    rng = np.random.default_rng(seed)
    o, t = aimed(rng, n, region, targets)
    return in_domain(np.concatenate([o.astype(np.float32), rescale(t - o, edge_lengths(rng, n))], axis=1))


def scale_components(rng, d, want):
    """Directions ``d`` with one or two components times 10^-U(0, 36) (a tenth of them: exactly +0
    or -0 instead, the component keeping its sign), the largest component left alone, and the
    whole brought to the lengths ``want``: the scaled components reach denormals."""
    n = d.shape[0]
    d = rescale(d, want).astype(np.float64)
    keep = np.abs(d).argmax(axis=1)
    other = (keep[:, None] + rng.permuted(np.tile([1, 2], (n, 1)), axis=1)) % 3  # the two other axes
    factor = 10.0 ** -rng.uniform(0, 36, (n, 2))
    factor[rng.uniform(0, 1, (n, 2)) < 0.1] = 0.0
    factor[rng.uniform(0, 1, n) < 0.5, 1] = 1.0  # half of the rays: one component only
    rows = np.arange(n)
    for k in range(2):
        d[rows, other[:, k]] *= factor[:, k]
    with np.errstate(under="ignore"):
        return rescale(d.astype(np.float32), want)


def mixed_components(seed, n, region, targets):
    """The aimed rays with ``scale_components`` applied; each origin is then moved, at its
    distance, to where the new direction still passes through the ray's aim point."""
    rng = np.random.default_rng(seed)
    o, t = aimed(rng, n, region, targets)
    d = scale_components(rng, t - o, edge_lengths(rng, n))
    u = d.astype(np.float64) / length_of(d)[:, None]
    o = t - u * np.linalg.norm(t - o, axis=1, keepdims=True)
    return in_domain(np.concatenate([o.astype(np.float32), d], axis=1))


def far_origins(seed, n, region, targets):
    """origin = target + R u, R in {1e3, 1e5, 1e7} in equal shares, u uniform on the sphere; the
    direction is target - origin of the f32 origin, rescaled to the lengths of ``length_edges``.
    A quarter of the targets are moved off the geometry by R 10^-U(0.3, 3), for misses."""
    rng = np.random.default_rng(seed)
    t = targets[rng.integers(0, targets.shape[0], n)].astype(np.float64)
    R = np.asarray(FAR_RADII)[rng.permutation(n) % len(FAR_RADII)]
    off = np.where(rng.uniform(0, 1, n) < 0.25, R * 10.0 ** -rng.uniform(0.3, 3, n), 0.0)
    t = t + off[:, None] * _unit(rng, n)
    o = (t + R[:, None] * _unit(rng, n)).astype(np.float32)
    d = (t.astype(np.float32) - o).astype(np.float32)
    return in_domain(np.concatenate([o, rescale(d, edge_lengths(rng, n))], axis=1))


def near_and_inside(seed, n, region, targets, normals=None, boxes=None, spheres=None):
    """Origins within 1e-4 of either side of a surface, inside spheres and inside object and
    sub-object boxes (equal shares of the kinds the scene has), directions to points on the
    geometry or uniformly random, lengths as in ``length_edges``."""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, targets.shape[0], n)
    near = targets[i] + rng.uniform(-1e-4, 1e-4, (n, 1)) * normals[i]
    places = [near]
    if spheres is not None and spheres.shape[0]:
        s = spheres[rng.integers(0, spheres.shape[0], n)]
        inside = s[:, :3] + 0.999 * s[:, 3:] * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * _unit(rng, n)
        # (of a ground-sized sphere: the part within a region's size of a surface point)
        size = np.linalg.norm(np.asarray(region[1], np.float64) - np.asarray(region[0], np.float64))
        below = near - size * rng.uniform(0, 1, (n, 1)) * normals[i]
        places.append(np.where((s[:, 3] > BIG_RADIUS)[:, None], below, inside))
    if boxes is not None and boxes.shape[0]:
        b = boxes[rng.integers(0, boxes.shape[0], n)]
        places.append(rng.uniform(b[:, 0], b[:, 1]))
    kind = rng.permutation(n) % len(places)
    o = np.choose(kind[:, None], places)
    free = rng.uniform(0, 1, n) < 0.5
    d = np.where(free[:, None], _unit(rng, n), targets[rng.integers(0, targets.shape[0], n)] - o)
    return in_domain(np.concatenate([o.astype(np.float32), rescale(d, edge_lengths(rng, n))], axis=1))


def from_one_origin(seed, n, origin, region, targets, wide=0.2):
    """A frame's worth of rays, which share one origin (the camera's): directions to points on
    or near the geometry, the first half scaled as in ``length_edges``, the second as in
    ``mixed_components`` (without moving the origin, so fewer of those still hit). A share ``wide``
    aims up to half the region's diagonal, or 3% of the distance if that is more, off its point:
    from 1e5 away the reference's f32 sphere test accepts rays that pass a sphere by tens of units."""
    rng = np.random.default_rng(seed)
    o = np.broadcast_to(np.asarray(origin, np.float32), (n, 3))
    size = np.maximum(np.asarray(region[1], np.float64) - np.asarray(region[0], np.float64), 1.0)
    t = targets[rng.integers(0, targets.shape[0], n)].astype(np.float64)
    far = np.maximum(0.5 * np.linalg.norm(size), 0.03 * np.linalg.norm(t - o, axis=1))
    off = np.where(rng.uniform(0, 1, n) < wide, far, 1e-3)
    t = t + off[:, None] * rng.uniform(0, 1, (n, 1)) * _unit(rng, n)
    d = (t.astype(np.float32) - o).astype(np.float32)
    want = edge_lengths(rng, n)
    d = np.concatenate([rescale(d[:n // 2], want[:n // 2]), scale_components(rng, d[n // 2:], want[n // 2:])])
    return in_domain(np.concatenate([o, d], axis=1))


SETS = ("length_edges", "mixed_components", "far_origins", "near_and_inside")


def ray_set(name, seed, n, geo):
    """Set ``name`` of ``n`` rays on a ``Geometry``."""
    if name == "near_and_inside":
        return near_and_inside(seed, n, geo.region, geo.targets, geo.normals, geo.boxes, geo.spheres)
    return globals()[name](seed, n, geo.region, geo.targets)
