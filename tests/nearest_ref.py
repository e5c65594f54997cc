"""THE NEAREST-POINT CONTRACT (include/rt_abi.h) restated in NumPy float32, for tests.

Written from the header, not from the kernel: a brute force over every candidate -- every sphere,
every triangle visit of the reference's sweep with its index clamps, boxes disregarded -- one
ufunc per written operation (``dot = (x*x + y*y) + z*z``; NumPy's float32 divide and sqrt are
correctly rounded), then the contract's tie order. Points are taken in chunks so that the chess
scene (5,552 triangles) and the small heightfield (25,600) stay within seconds.
"""
import numpy as np

from rust_gpu_raytracing_amd import buffers as B

F32_MAX = np.float32(3.4028235e38)
INF = np.float32(np.inf)
ONE, ZERO = np.float32(1), np.float32(0)
MISS, SPHERE, TRIANGLE = 0, 1, 2


def _dot(a, b):
    return np.add(np.add(np.multiply(a[0], b[0]), np.multiply(a[1], b[1])), np.multiply(a[2], b[2]))


def _sub(a, b):
    return [np.subtract(a[k], b[k]) for k in range(3)]


def _add(a, b):
    return [np.add(a[k], b[k]) for k in range(3)]


def _scale(a, s):
    return [np.multiply(a[k], s) for k in range(3)]


def _weight(x):
    """W(x): x if 0 <= x <= 1, 1 if x > 1, else 0 (NaN included)."""
    return np.where(x >= 0, np.where(x > 1, ONE, x), ZERO).astype(np.float32)


def sweep_visits(objs, subs, n_tris):
    """The triangle visits of the reference's sweep in order: (triangle, object, sub-object) per
    sweep position, with the reference's index clamps."""
    tri, obj, sub = [], [], []
    last_sub, last_tri = subs.shape[0] - 1, n_tris - 1
    for oi in range(objs.shape[0]):
        ob = objs[oi]
        for i in range(int(ob["sub_object_count"])):
            si = min(int(ob["first_sub_object_index"]) + i, last_sub)
            cnt = int(subs[si]["triangle_count"])
            ti = np.minimum(int(subs[si]["first_triangle_index"]) + np.arange(cnt, dtype=np.int64), last_tri)
            tri.append(ti)
            obj.append(np.full(cnt, oi, np.int64))
            sub.append(np.full(cnt, si, np.int64))
    if not tri:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(tri), np.concatenate(obj), np.concatenate(sub)


def triangle_closest(a, ab, ac, p):
    """Step 2 for broadcastable component lists a, ab, ac (triangles) and p (points): the closest
    point q (three arrays) and the region number."""
    ap = _sub(p, a)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = _sub(ap, ab)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    vc = np.subtract(np.multiply(d1, d4), np.multiply(d3, d2))
    cp = _sub(ap, ac)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vb = np.subtract(np.multiply(d5, d2), np.multiply(d1, d6))
    va = np.subtract(np.multiply(d3, d6), np.multiply(d5, d4))
    e1, e2 = np.subtract(d4, d3), np.subtract(d5, d6)
    conds = [
        (d1 <= 0) & (d2 <= 0),
        (d3 >= 0) & (d4 <= d3),
        (vc <= 0) & (d1 >= 0) & (d3 <= 0),
        (d6 >= 0) & (d5 <= d6),
        (vb <= 0) & (d2 >= 0) & (d6 <= 0),
        (va <= 0) & (e1 >= 0) & (e2 >= 0),
    ]
    shape = np.broadcast(d1).shape
    a_b = [np.broadcast_to(a[k], shape) for k in range(3)]
    v3 = _weight(np.divide(d1, np.subtract(d1, d3)))
    w5 = _weight(np.divide(d2, np.subtract(d2, d6)))
    w6 = _weight(np.divide(e1, np.add(e1, e2)))
    denom = np.divide(ONE, np.add(np.add(va, vb), vc))
    v7 = _weight(np.multiply(vb, denom))
    w7 = _weight(np.multiply(vc, denom))
    rest = np.subtract(ONE, v7)
    w7 = np.where(w7 > rest, rest, w7)
    qs = [
        a_b,
        _add(a, ab),
        _add(a, _scale(ab, v3)),
        _add(a, ac),
        _add(a, _scale(ac, w5)),
        _add(_add(a, _scale(ab, np.subtract(ONE, w6))), _scale(ac, w6)),
        _add(_add(a, _scale(ab, v7)), _scale(ac, w7)),
    ]
    region = np.full(shape, 7, np.uint32)
    q = [np.broadcast_to(qs[6][k], shape).astype(np.float32) for k in range(3)]
    for r in range(5, -1, -1):  # the first condition that holds decides
        c = np.broadcast_to(conds[r], shape)
        region = np.where(c, np.uint32(r + 1), region)
        q = [np.where(c, qs[r][k], q[k]).astype(np.float32) for k in range(3)]
    return q, region


def point_key(q, p):
    e = _sub(q, p)
    return np.sqrt(_dot(e, e))


def _first_min(key, cand):
    """Per row the first candidate of the smallest key: (found, column)."""
    masked = np.where(cand, key, INF)
    col = np.argmin(masked, axis=1)
    rows = np.arange(key.shape[0])
    fallback = ~cand[rows, col]  # every candidate's key is +inf: the first of them
    col = np.where(fallback, np.argmax(cand, axis=1), col)
    return cand.any(axis=1), col


def nearest(spheres, objs, subs, tris, points, max_distance=INF, chunk=None):
    """The ``buffers.NEAREST`` records of ``points`` (n, 3) with ``max_distance`` a scalar or (n,)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    maxd = np.broadcast_to(np.asarray(max_distance, np.float32), (n,))
    out = np.zeros(n, B.NEAREST)
    out["distance"] = F32_MAX
    vt, vo, vs = sweep_visits(objs, subs, tris.shape[0]) if objs.shape[0] and tris.shape[0] else (np.zeros(0, np.int64),) * 3
    n_cand = vt.size + spheres.shape[0]
    if chunk is None:
        chunk = max(1, min(n, (1 << 22) // max(n_cand, 1)))
    with np.errstate(all="ignore"):
        for at in range(0, n, chunk):
            sl = slice(at, min(n, at + chunk))
            _nearest_chunk(spheres, objs, tris, vt, vo, vs, pts[sl], maxd[sl], out[sl])
    return out


def _nearest_chunk(spheres, objs, tris, vt, vo, vs, pts, maxd, out):
    m = pts.shape[0]
    p = [pts[:, k:k + 1] for k in range(3)]
    rows = np.arange(m)
    t_found = np.zeros(m, bool)
    t_key = np.full(m, INF, np.float32)
    if vt.size:
        tr = tris[vt]
        a = [tr["a"][None, :, k] for k in range(3)]
        ab = [tr["edge_ab"][None, :, k] for k in range(3)]
        ac = [tr["edge_ac"][None, :, k] for k in range(3)]
        q, region = triangle_closest(a, ab, ac, p)
        key = point_key(q, p)
        cand = ~np.isnan(key) & (key <= maxd[:, None])
        t_found, t_col = _first_min(key, cand)
        t_key = key[rows, t_col]
    s_found = np.zeros(m, bool)
    s_key = np.full(m, INF, np.float32)
    if spheres.shape[0]:
        c = [spheres["position"][None, :, k].astype(np.float32) for k in range(3)]
        r_abs = np.abs(spheres["radius"].astype(np.float32))[None, :]
        v = _sub(c, p)
        l = np.sqrt(_dot(v, v))
        key_s = np.abs(np.subtract(l, r_abs))
        cand_s = ~np.isnan(key_s) & (key_s <= maxd[:, None])
        s_found, s_col = _first_min(key_s, cand_s)
        s_key = key_s[rows, s_col]
    tri_wins = t_found & (~s_found | (t_key <= s_key))  # a triangle before a sphere at equal keys
    sph_wins = s_found & ~tri_wins
    if tri_wins.any():
        w = np.nonzero(tri_wins)[0]
        col = t_col[w]
        out["distance"][w] = t_key[w]
        for k in range(3):
            out["point"][w, k] = q[k][w, col]
        out["normal"][w] = tris["face_normal"][vt[col]]
        out["feature"][w] = region[w, col]
        out["kind"][w] = TRIANGLE
        out["index"][w] = vo[col]
        out["sub_object"][w] = vs[col]
        out["triangle"][w] = vt[col]
        out["material_index"][w] = objs["material_index"][vo[col]]
        cn = tris["calc_normal"][vt[col]]
        ap = [np.subtract(pts[w, k], tris["a"][vt[col], k]) for k in range(3)]
        out["side"][w] = _dot([cn[:, k] for k in range(3)], ap) >= 0
    if sph_wins.any():
        w = np.nonzero(sph_wins)[0]
        col = s_col[w]
        cw = [spheres["position"][col, k].astype(np.float32) for k in range(3)]
        rw = np.abs(spheres["radius"][col].astype(np.float32))
        vw = _sub(cw, [pts[w, k] for k in range(3)])
        lw = np.sqrt(_dot(vw, vw))
        s = np.divide(rw, lw)
        at_centre = lw == 0
        point = [np.subtract(cw[k], np.multiply(vw[k], s)) for k in range(3)]
        normal = [np.negative(np.divide(vw[k], lw)) for k in range(3)]
        point[0] = np.where(at_centre, np.add(cw[0], rw), point[0])
        point[1] = np.where(at_centre, cw[1], point[1])
        point[2] = np.where(at_centre, cw[2], point[2])
        normal[0] = np.where(at_centre, ONE, normal[0])
        normal[1] = np.where(at_centre, ZERO, normal[1])
        normal[2] = np.where(at_centre, ZERO, normal[2])
        out["distance"][w] = s_key[w]
        for k in range(3):
            out["point"][w, k] = point[k]
            out["normal"][w, k] = normal[k]
        out["feature"][w] = 0
        out["kind"][w] = SPHERE
        out["index"][w] = col
        out["material_index"][w] = spheres["material_index"][col]
        out["side"][w] = lw >= rw


def scene_arrays(scene):
    """(spheres, objects, sub-objects, triangles) of a Scene."""
    objs, subs, tris = scene.flatten()
    return np.ascontiguousarray(scene.spheres), objs, subs, tris


def scene_nearest(scene, points, max_distance=INF, geometry=None):
    """``nearest`` on a Scene; ``geometry``: (objects, sub-objects, triangles) as the device holds
    them, when not the scene's own."""
    spheres, objs, subs, tris = scene_arrays(scene)
    if geometry is not None:
        objs, subs, tris = geometry
    return nearest(spheres, objs, subs, tris, points, max_distance)


def same_records(got, want):
    """All 64 bytes of every record."""
    assert got.dtype == B.NEAREST and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    g = got.view(np.uint8).reshape(got.shape[0], 64)
    w = want.view(np.uint8).reshape(want.shape[0], 64)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:1]], want[bad[:1]])
