"""THE HIT-LIST CONTRACT (include/rt_abi.h) restated in NumPy float32, for tests.

Written from the header, not from the kernel: per ray the ordered list of candidates, each
primitive tested on its own by the reference's test, one ufunc per written operation
(``dot = (x*x + y*y) + z*z``, the NaN-ignoring min/max of ray_in_bounds, the sweep's index clamps).
The full 64-byte records of listed entries come from ``Oracle.trace`` on a scene cut down to that
one primitive, so the oracle's hit-point, normal and uv arithmetic is not restated -- and every
listed distance is checked against the oracle's own on the way.
"""
import functools

import numpy as np

from rust_gpu_raytracing_amd import buffers as B

F32_MAX = np.float32(3.4028235e38)
INF = np.float32(np.inf)
HITS_MAX = 16

# one candidate: distance, kind (1 sphere, 2 triangle), sphere or object index, sub-object,
# triangle, sweep position (triangles) -- and the ray it belongs to
CAND = np.dtype([("ray", "<u4"), ("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("sub_object", "<u4"),
                 ("triangle", "<u4"), ("seq", "<u4")])


def _dot(ax, ay, az, bx, by, bz):
    return np.add(np.add(np.multiply(ax, bx), np.multiply(ay, by)), np.multiply(az, bz))


def _ray_in_bounds(o, inv, mn, mx):
    """ray_in_bounds (compute_shader.wgsl:407-419) for rays (n, 3) against one box."""
    tmin = np.multiply(np.subtract(mn[None, :], o), inv)
    tmax = np.multiply(np.subtract(mx[None, :], o), inv)
    t1 = np.fmin(tmin, tmax)  # (min/max that ignore a NaN operand, as the oracle's)
    t2 = np.fmax(tmin, tmax)
    near = np.fmax(np.fmax(t1[:, 0], t1[:, 1]), t1[:, 2])
    far = np.fmin(np.fmin(t2[:, 0], t2[:, 1]), t2[:, 2])
    return (near <= far) & (far >= 0)


def candidates(spheres, objs, subs, tris, rays, t_max):
    """Every candidate of every ray, as a CAND array sorted by (ray, the contract's order)."""
    rays = np.ascontiguousarray(rays, np.float32)
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    t_max = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    with np.errstate(all="ignore"):
        live = t_max > 0  # (NaN: no candidates)
        bound = np.minimum(np.where(live, t_max, np.float32(0)), F32_MAX).astype(np.float32)
        out = []
        # -- spheres, check_spheres' test (:355-404) on each alone
        if spheres.shape[0]:
            pos = spheres["position"].astype(np.float32)
            rad = spheres["radius"].astype(np.float32)
            a = _dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])[:, None]
            ocx = np.subtract(o[:, 0:1], pos[None, :, 0])
            ocy = np.subtract(o[:, 1:2], pos[None, :, 1])
            ocz = np.subtract(o[:, 2:3], pos[None, :, 2])
            b = np.multiply(np.float32(2), _dot(d[:, 0:1], d[:, 1:2], d[:, 2:3], ocx, ocy, ocz))
            c = np.subtract(_dot(ocx, ocy, ocz, ocx, ocy, ocz), np.multiply(rad, rad)[None, :])
            disc = np.subtract(np.multiply(b, b), np.multiply(np.multiply(np.float32(4), a), c))
            t = np.divide(np.subtract(np.negative(b), np.sqrt(disc)), np.multiply(np.float32(2), a))
            ok = ~(disc < 0) & (t > 0) & (t < bound[:, None]) & live[:, None]
            ri, si = np.nonzero(ok)
            part = np.zeros(ri.size, CAND)
            part["ray"], part["t"], part["kind"], part["index"] = ri, t[ri, si], 1, si
            out.append(part)
        # -- triangles, the sweep of check_triangles (:422-517), each visit on its own
        if objs.shape[0]:
            inv = np.divide(np.float32(1), d)
            seq = 0
            last_sub, last_tri = subs.shape[0] - 1, tris.shape[0] - 1
            for oi in range(objs.shape[0]):
                ob = objs[oi]
                in_obj = _ray_in_bounds(o, inv, ob["min_bounds"], ob["max_bounds"]) & live
                for i in range(int(ob["sub_object_count"])):
                    si = min(int(ob["first_sub_object_index"]) + i, last_sub)
                    sub = subs[si]
                    cnt = int(sub["triangle_count"])
                    base, seq = seq, seq + cnt
                    if cnt == 0 or not in_obj.any():
                        continue
                    rows = np.nonzero(in_obj & _ray_in_bounds(o, inv, sub["min_bounds"], sub["max_bounds"]))[0]
                    if rows.size == 0:
                        continue
                    ti = np.minimum(int(sub["first_triangle_index"]) + np.arange(cnt), last_tri)
                    tr = tris[ti]
                    ro, rd = o[rows], d[rows]
                    cn, ta, ab, ac = tr["calc_normal"], tr["a"], tr["edge_ab"], tr["edge_ac"]
                    det = np.negative(_dot(rd[:, 0:1], rd[:, 1:2], rd[:, 2:3],
                                           cn[None, :, 0], cn[None, :, 1], cn[None, :, 2]))
                    inv_det = np.divide(np.float32(1), det)
                    aox = np.subtract(ro[:, 0:1], ta[None, :, 0])
                    aoy = np.subtract(ro[:, 1:2], ta[None, :, 1])
                    aoz = np.subtract(ro[:, 2:3], ta[None, :, 2])
                    dist = np.multiply(_dot(aox, aoy, aoz, cn[None, :, 0], cn[None, :, 1], cn[None, :, 2]), inv_det)
                    # cross(ao, d)
                    cx = np.subtract(np.multiply(aoy, rd[:, 2:3]), np.multiply(aoz, rd[:, 1:2]))
                    cy = np.subtract(np.multiply(aoz, rd[:, 0:1]), np.multiply(aox, rd[:, 2:3]))
                    cz = np.subtract(np.multiply(aox, rd[:, 1:2]), np.multiply(aoy, rd[:, 0:1]))
                    v = np.multiply(np.negative(_dot(ab[None, :, 0], ab[None, :, 1], ab[None, :, 2], cx, cy, cz)),
                                    inv_det)
                    u = np.multiply(_dot(ac[None, :, 0], ac[None, :, 1], ac[None, :, 2], cx, cy, cz), inv_det)
                    w = np.subtract(np.subtract(np.float32(1), u), v)
                    ok = ~(dist < 0) & ~(v < 0) & ~(u < 0) & ~(w < 0) & ~np.isnan(dist) & (dist < bound[rows, None])
                    rr, jj = np.nonzero(ok)
                    part = np.zeros(rr.size, CAND)
                    part["ray"], part["t"], part["kind"], part["index"] = rows[rr], dist[rr, jj], 2, oi
                    part["sub_object"], part["triangle"], part["seq"] = si, ti[jj], base + jj
                    out.append(part)
    cand = np.concatenate(out) if out else np.zeros(0, CAND)
    # ascending t; at equal t triangles before spheres, triangles by seq, spheres by index
    minor = np.where(cand["kind"] == 2, cand["seq"], cand["index"])
    order = np.lexsort((minor, cand["kind"] == 1, cand["t"], cand["ray"]))
    return cand[order]


class HitsRef:
    """The contract on one scene: ``lists`` (every candidate, in order) and ``records`` (the first
    ``max_hits`` as rt_hit records plus the counts). ``geometry``: (objects, sub-objects, triangles)
    as the device holds them, when not the scene's own."""

    def __init__(self, O, scene, geometry=None):
        self.O, self.scene = O, scene
        self.objs, self.subs, self.tris = geometry if geometry is not None else scene.flatten()
        self.spheres = np.ascontiguousarray(scene.spheres)
        self._cut = O.Oracle(scene)
        self._p = scene.params(accumulation_index=1)

    def lists(self, rays, t_max=None):
        return candidates(self.spheres, self.objs, self.subs, self.tris, rays, INF if t_max is None else t_max)

    def _record(self, ray, c):
        """The rt_hit record of candidate ``c``: Oracle.trace on the scene cut down to it."""
        cut, p = self._cut, self._p.copy()
        s = cut._s
        if c["kind"] == 1:
            p["object_count"], p["sphere_count"] = 0, 1
            s.spheres = self.spheres.ctypes.data + B.SPHERE.itemsize * int(c["index"])
            keep = ()
        else:
            # the object with its own box and material, the sub-object with its own box, one triangle
            ob = self.objs[int(c["index"]):int(c["index"]) + 1].copy()
            sub = self.subs[int(c["sub_object"]):int(c["sub_object"]) + 1].copy()
            tri = np.ascontiguousarray(self.tris[int(c["triangle"]):int(c["triangle"]) + 1])
            ob["first_sub_object_index"], ob["sub_object_count"] = 0, 1
            sub["first_triangle_index"], sub["triangle_count"] = 0, 1
            p["object_count"], p["sphere_count"] = 1, 0
            s.objects, s.object_capacity = ob.ctypes.data, 1
            s.subs, s.sub_count = sub.ctypes.data, 1
            s.triangles, s.triangle_count = tri.ctypes.data, 1
            keep = (ob, sub, tri)
        h = cut.trace(p, ray[:3], ray[3:])
        del keep
        assert np.float32(h.t).view(np.uint32) == c["t"].view(np.uint32), ("the restatement's distance", c, h.t)
        rec = np.zeros((), B.HIT)
        rec["t"], rec["position"], rec["normal"] = h.t, (h.px, h.py, h.pz), (h.nx, h.ny, h.nz)
        rec["u"], rec["v"], rec["material_index"], rec["front_face"] = h.u, h.v, h.material_index, h.front_face
        rec["kind"], rec["index"] = c["kind"], c["index"]
        rec["sub_object"], rec["triangle"] = c["sub_object"], c["triangle"]
        return rec

    def records(self, rays, t_max=None, max_hits=HITS_MAX, lists=None):
        """(hits (n, max_hits) HIT, counts (n,) uint32, every ray's number of candidates)."""
        rays = np.ascontiguousarray(rays, np.float32)
        cand = self.lists(rays, t_max) if lists is None else lists
        n = rays.shape[0]
        hits = np.zeros((n, max_hits), B.HIT)
        hits["t"] = F32_MAX
        total = np.bincount(cand["ray"], minlength=n).astype(np.uint32)
        start = np.concatenate([[0], np.cumsum(total)[:-1]]).astype(np.int64)
        for i in np.nonzero(total)[0]:
            for j in range(min(int(total[i]), max_hits)):
                hits[i, j] = self._record(rays[i], cand[start[i] + j])
        return hits, np.minimum(total, max_hits).astype(np.uint32), total


def truncate(hits, counts, max_hits):
    """The list for ``max_hits`` from a longer one (consequence 3: lists nest)."""
    assert max_hits <= hits.shape[1]
    return np.ascontiguousarray(hits[:, :max_hits]), np.minimum(counts, max_hits).astype(np.uint32)


def equal_t_pairs(cand):
    """Neighbours in a ray's list at exactly equal distance."""
    return int(((cand["ray"][1:] == cand["ray"][:-1]) & (cand["t"][1:] == cand["t"][:-1])).sum())


def golden_camera_rays(g):
    d = np.asarray(g["camera_rays"]["direction"], np.float32)
    rays = np.zeros((d.shape[0], 6), np.float32)
    rays[:, :3] = np.asarray(g["camera_origin"], np.float32)
    rays[:, 3:] = d
    return rays


GOLDENS = {"c1": "c1_37x21_noacc", "c2": "c2_64x36_b8", "c3": "c3_64x36_b8"}


@functools.lru_cache(maxsize=None)
def golden_reference(key):
    """Of one golden scene: (scene, every pixel's camera ray, the candidates with t_max = +inf,
    the 16-entry records and counts, every ray's number of candidates). Computed once and shared
    (never modified)."""
    from oracle import oracle as O
    from tests.golden.fixtures import load, scene_from_inputs

    O.build()
    g = load(GOLDENS[key])
    scene = scene_from_inputs(g)
    rays = golden_camera_rays(g)
    ref = HitsRef(O, scene)
    cand = ref.lists(rays)
    hits, counts, total = ref.records(rays, lists=cand)
    return scene, rays, cand, hits, counts, total
