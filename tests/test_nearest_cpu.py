"""CPU checks of THE NEAREST-POINT CONTRACT (include/rt_abi.h): the NumPy restatement
(tests/nearest_ref.py) against float64 geometry and on constructed cases, the certified box bound
of the accelerated walk (tests/cpp/nearest_bound.cpp, which compiles csrc/rt_nearest_math.h, the
text the kernel compiles), and the parts of the ABI that need no device.
"""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd.scene import build_config
from tests import nearest_ref as R

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rust_gpu_raytracing_amd" / "csrc"
INF, F32_MAX = R.INF, R.F32_MAX
NO = np.zeros(0, B.SPHERE), np.zeros(0, B.OBJECT_INFO), np.zeros(0, B.SUB_OBJECT_INFO), np.zeros(0, B.TRIANGLE)


# ---------------------------------------------------------------------------- constructed scenes
def spheres_of(rows):
    s = np.zeros(len(rows), B.SPHERE)
    for i, (c, r) in enumerate(rows):
        s["position"][i], s["radius"][i], s["material_index"][i] = c, r, i + 1
    return s


def triangles_of(tris, per_object=None):
    """Triangle records of (a, b, c) vertex triples, one sub-object per triangle; ``per_object``:
    sub-objects per object (default: all in one)."""
    t = np.zeros(len(tris), B.TRIANGLE)
    for i, (a, b, c) in enumerate(tris):
        a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))
        t["a"][i], t["edge_ab"][i], t["edge_ac"][i] = a, b - a, c - a
        cn = np.cross(t["edge_ab"][i], t["edge_ac"][i]).astype(np.float32)
        t["calc_normal"][i] = cn
        with np.errstate(all="ignore"):
            t["face_normal"][i] = cn / np.sqrt((cn * cn).sum(dtype=np.float32))
    subs = np.zeros(len(tris), B.SUB_OBJECT_INFO)
    subs["first_triangle_index"], subs["triangle_count"] = np.arange(len(tris)), 1
    per = per_object or [len(tris)]
    objs = np.zeros(len(per), B.OBJECT_INFO)
    objs["first_sub_object_index"] = np.concatenate([[0], np.cumsum(per)[:-1]])
    objs["sub_object_count"], objs["material_index"] = per, 7 + np.arange(len(per))
    return objs, subs, t


UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0))  # a = origin, b on x, c on y, in the plane z = 0


def one(spheres, geom, p, maxd=INF):
    objs, subs, tris = geom if geom is not None else NO[1:]
    return R.nearest(spheres if spheres is not None else NO[0], objs, subs, tris,
                     np.asarray([p], np.float32), maxd)[0]


# ---------------------------------------------------------------------------- float64 geometry
def exact_sphere(spheres, p):
    c = spheres["position"].astype(np.float64)
    return np.abs(np.linalg.norm(c[None] - p[:, None], axis=2) - np.abs(spheres["radius"].astype(np.float64))[None])


def exact_segment(p, a, b):
    ab = b - a
    t = np.einsum("ptk,ptk->pt", p - a, ab) / np.maximum(np.einsum("ptk,ptk->pt", ab, ab), 1e-300)
    q = a + np.clip(t, 0, 1)[..., None] * ab
    return np.linalg.norm(p - q, axis=2)


def exact_triangle(tris, p):
    """Point-triangle distances in float64 by another route than the contract's: the distance to
    the plane where the projection falls inside, else the smallest of the three edge distances."""
    a = tris["a"].astype(np.float64)[None]
    b = a + tris["edge_ab"].astype(np.float64)[None]
    c = a + tris["edge_ac"].astype(np.float64)[None]
    pp = p[:, None, :]
    n = np.cross(b - a, c - a)
    nn = np.einsum("ptk,ptk->pt", n, n)
    edges = np.minimum(np.minimum(exact_segment(pp, a, b), exact_segment(pp, b, c)), exact_segment(pp, c, a))
    with np.errstate(all="ignore"):
        inside = np.ones(edges.shape, bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= np.einsum("ptk,ptk->pt", np.cross(v - u, pp - u), n) >= 0
        plane = np.abs(np.einsum("ptk,ptk->pt", pp - a, n)) / np.sqrt(nn)
    return np.where(inside & (nn > 0), np.minimum(plane, edges), edges)


def error_against_float64(scene_key, n, seed):
    """(largest absolute error, largest relative error among points further than 1e-3 from the
    surface) of the restatement's winning key against the float64 minimum, on random points around
    the scene, on its vertices and sphere poles, and on the winners' own closest points."""
    from tests.test_gpu_query import SCENES

    config, kw = SCENES[scene_key]
    scene, _ = build_config(config, **kw)
    spheres, objs, subs, tris = R.scene_arrays(scene)
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    if tris.shape[0]:
        pick = rng.integers(0, tris.shape[0], n // 4)
        pts[:n // 4] = tris["a"][pick] + tris["edge_ab"][pick] * rng.uniform(0, 1, (n // 4, 1)).astype(np.float32)
    if spheres.shape[0]:
        pick = rng.integers(0, spheres.shape[0], n // 8)
        pts[n // 4:n // 4 + n // 8] = spheres["position"][pick] + np.abs(spheres["radius"][pick])[:, None] * \
            np.float32([0, 1, 0])
    first = R.nearest(spheres, objs, subs, tris, pts)
    pts = np.concatenate([pts, first["point"]])  # points on the surface: distances near 0
    got = R.nearest(spheres, objs, subs, tris, pts)
    p64 = pts.astype(np.float64)
    exact = np.full(pts.shape[0], np.inf)
    vt, _, _ = R.sweep_visits(objs, subs, tris.shape[0]) if tris.shape[0] else (np.zeros(0, np.int64),) * 3
    for at in range(0, pts.shape[0], 256):
        sl = slice(at, at + 256)
        if vt.size:
            exact[sl] = np.minimum(exact[sl], exact_triangle(tris[vt], p64[sl]).min(axis=1))
        if spheres.shape[0]:
            exact[sl] = np.minimum(exact[sl], exact_sphere(spheres, p64[sl]).min(axis=1))
    err = np.abs(got["distance"].astype(np.float64) - exact)
    far = exact > 1e-3
    return err.max(), (err[far] / exact[far]).max()


# The figures error_against_float64 measured for these point sets (seed 3, scenes of a few units
# across), written into DESIGN.md §5.4n: (largest absolute, largest relative error). Both come
# from the face region of small chess triangles seen from afar, where va, vb and vc cancel (a
# sphere's key loses what the root loses before |r| is subtracted: c4's spheres stay below these
# figures). The assertion allows each one doubling, for rounding-mode differences.
MEASURED = {"c3": (1.114e-5, 4.910e-5), "c4": (1.114e-5, 4.910e-5)}


@pytest.mark.parametrize("key", ["c3", "c4"])
def test_winning_key_agrees_with_float64_geometry(key):
    abs_err, rel_err = error_against_float64(key, 600, 3)
    print(f"{key}: largest absolute error {abs_err:.3e}, largest relative error {rel_err:.3e}")
    assert abs_err <= 2 * MEASURED[key][0] and rel_err <= 2 * MEASURED[key][1], (abs_err, rel_err)


# ---------------------------------------------------------------------------- coverage
def test_each_region_is_reached():
    geom = triangles_of([UNIT])
    cases = {1: (-1, -1, 2), 2: (3, -1, 1), 3: (0.5, -2, 0), 4: (-1, 3, 1), 5: (-2, 0.5, 0), 6: (2, 2, 0.5),
             7: (0.25, 0.25, 3)}
    want_q = {1: (0, 0, 0), 2: (1, 0, 0), 3: (0.5, 0, 0), 4: (0, 1, 0), 5: (0, 0.5, 0), 6: (0.5, 0.5, 0),
              7: (0.25, 0.25, 0)}
    for region, p in cases.items():
        r = one(None, geom, p)
        assert r["kind"] == R.TRIANGLE and r["feature"] == region, (region, r)
        assert np.array_equal(r["point"], np.float32(want_q[region])), (region, r["point"])
        assert r["distance"] == np.float32(np.linalg.norm(np.float64(p) - np.float64(want_q[region])))
        assert r["side"] == 1 and np.array_equal(r["normal"], np.float32([0, 0, 1]))
        assert (r["index"], r["sub_object"], r["triangle"], r["material_index"]) == (0, 0, 0, 7)
    assert one(None, geom, (0.25, 0.25, -3))["side"] == 0  # behind calc_normal; the normal is not flipped
    assert np.array_equal(one(None, geom, (0.25, 0.25, -3))["normal"], np.float32([0, 0, 1]))


def test_points_on_the_triangle_have_distance_zero():
    geom = triangles_of([UNIT])
    for p, region in (((0, 0, 0), 1), ((1, 0, 0), 2), ((0, 1, 0), 4), ((0.5, 0, 0), 3), ((0, 0.25, 0), 5),
                      ((0.5, 0.5, 0), 6), ((0.25, 0.5, 0), 7)):
        r = one(None, geom, p)
        assert r["distance"] == 0 and r["feature"] == region and np.array_equal(r["point"], np.float32(p)), (p, r)


def test_sphere_cases():
    s = spheres_of([((1, 2, 3), 2.0)])
    centre = one(s, None, (1, 2, 3))
    assert centre["distance"] == 2 and np.array_equal(centre["point"], np.float32([3, 2, 3]))
    assert np.array_equal(centre["normal"], np.float32([1, 0, 0])) and centre["side"] == 0
    inside = one(s, None, (1, 2, 4))
    assert inside["distance"] == 1 and inside["side"] == 0 and np.array_equal(inside["point"], np.float32([1, 2, 5]))
    assert np.array_equal(inside["normal"], np.float32([0, 0, 1]))
    on = one(s, None, (1, 4, 3))
    assert on["distance"] == 0 and on["side"] == 1 and np.array_equal(on["point"], np.float32([1, 4, 3]))
    outside = one(s, None, (1, 2, -2))
    assert outside["distance"] == 3 and outside["side"] == 1 and np.array_equal(outside["normal"], np.float32([0, 0, -1]))
    assert (outside["kind"], outside["index"], outside["feature"], outside["material_index"]) == (R.SPHERE, 0, 0, 1)
    # a hollow shell: only |r| matters
    shell = spheres_of([((1, 2, 3), -2.0)])
    for p in ((1, 2, 3), (1, 2, 4), (1, 4, 3), (1, 2, -2)):
        a, b = one(s, None, p), one(shell, None, p)
        assert a.tobytes() == b.tobytes()


def test_ties():
    # two identical spheres: the lower index
    twins = spheres_of([((5, 5, 5), 1.0), ((0, 0, 0), 1.0), ((0, 0, 0), 1.0)])
    assert one(twins, None, (0, 3, 0))["index"] == 1
    # a triangle and a sphere at equal key: the triangle
    geom = triangles_of([UNIT])
    ball = spheres_of([((0.25, 0.25, 5), 1.0)])
    r = one(ball, geom, (0.25, 0.25, 2))
    assert r["kind"] == R.TRIANGLE and r["distance"] == 2
    assert one(ball, None, (0.25, 0.25, 2))["distance"] == 2
    assert one(ball, geom, (0.25, 0.25, 2.5))["kind"] == R.SPHERE  # and a strictly closer sphere wins
    # a shared edge of two triangles: the lower sweep position, across sub-objects and objects
    quad = [UNIT, ((1, 0, 0), (1, 1, 0), (0, 1, 0))]
    for per in ([2], [1, 1]):
        r = one(None, triangles_of(quad, per), (0.5, 0.5, 1))
        assert (r["triangle"], r["distance"], r["feature"]) == (0, 1, 6)
        flipped = one(None, triangles_of(quad[::-1], per), (0.5, 0.5, 1))
        assert flipped["triangle"] == 0 and flipped["distance"] == 1 and flipped["index"] == 0


def test_max_distance_edges_and_nan():
    geom = triangles_of([UNIT])
    s = spheres_of([((0.25, 0.25, 10), 1.0)])
    p = (0.25, 0.25, 3)
    key = one(s, geom, p)["distance"]
    assert key == 3
    assert one(s, geom, p, key)["kind"] == R.TRIANGLE
    below = one(s, geom, p, np.nextafter(key, np.float32(0)))
    assert below["kind"] == R.MISS  # the sphere's key is 6
    assert one(s, geom, p, 6)["kind"] == R.TRIANGLE
    miss = np.zeros(1, B.NEAREST)
    miss["distance"] = F32_MAX
    for maxd in (np.nan, -1.0, -0.5, -np.inf, 2.0):
        assert one(s, geom, p, maxd).tobytes() == miss[0].tobytes(), maxd
    assert one(s, geom, (0.25, 0.25, 0), 0)["kind"] == R.TRIANGLE  # max_distance 0 admits a key of 0
    assert one(s, geom, p, 0)["kind"] == R.MISS
    assert one(s, geom, p, INF)["kind"] == R.TRIANGLE
    for bad in ((np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (np.nan,) * 3):
        assert one(s, geom, bad).tobytes() == miss[0].tobytes()


def test_degenerate_triangles_never_poison_the_result():
    """A point, a zero edge, collinear vertices and a NaN vertex beside a proper triangle: the keys
    stay distances to points of the degenerate triangle's own hull (or NaN, which is no candidate),
    and the proper triangle still wins where it is closer."""
    nan = np.nan
    bad = [((5, 5, 5), (5, 5, 5), (5, 5, 5)), ((5, 0, 0), (6, 0, 0), (6, 0, 0)), ((0, 5, 0), (0, 6, 0), (0, 8, 0)),
           ((nan, 0, 0), (1, nan, 0), (0, 1, 0))]
    geom = triangles_of(bad + [UNIT])
    rng = np.random.default_rng(2)
    pts = rng.uniform(-3, 9, (400, 3)).astype(np.float32)
    got = R.nearest(NO[0], *geom, pts)
    assert not np.isnan(got["distance"]).any() and (got["kind"] == R.TRIANGLE).all() and (got["triangle"] != 3).all()
    assert len(set(got["triangle"])) == 4
    # against float64 distances to the hulls (segments and a point)
    p64 = pts.astype(np.float64)
    seg = lambda a, b: exact_segment(p64[:, None], np.float64(a)[None, None], np.float64(b)[None, None])[:, 0]
    exact = np.minimum.reduce([np.linalg.norm(p64 - 5.0, axis=1), seg((5, 0, 0), (6, 0, 0)), seg((0, 5, 0), (0, 8, 0)),
                               exact_triangle(geom[2][4:], p64)[:, 0]])
    assert np.abs(got["distance"] - exact).max() < 1e-5


# ---------------------------------------------------------------------------- the certified bound
def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", *extra, f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "nearest_bound.cpp"), str(CSRC / "sphere_bvh.cpp"), "-o", str(exe)],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("nearest") / "nearest_bound")


def test_box_bound_never_exceeds_a_key_and_walk_equals_sweep(harness):
    out = subprocess.run([str(harness), "walk", "1"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("ok walk"), out.stdout[-2000:]
    w = out.stdout.split()
    count = lambda key: int(w[w.index(key) + 1])
    # six built trees x 250 points: every node against every primitive below it, 8 walks a point
    assert count("points") == 1500 and count("walks") == 12000 and count("pairs") > 1000000
    for key in ("culled", "ties", "inside", "on_face", "far", "bound_zero", "bound_pos", "boxes"):
        assert count(key) > 100, key


def test_harness_detects_a_bound_without_shrink_and_a_non_strict_cull(harness):
    out = subprocess.run([str(harness), "mutants", "1"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok mutants detected 2"), out.stdout[-2000:]


def test_harness_clean_under_sanitizers(tmp_path):
    """The stand-alone harness (host code, its own main) with AddressSanitizer and UBSan."""
    exe = _build(tmp_path / "nearest_bound_san",
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    out = subprocess.run([str(exe), "walk", "2"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok walk"), (out.stdout[-1000:], out.stderr[-3000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]


# ---------------------------------------------------------------------------- the ABI without a device
def test_record_layouts_against_the_compiled_header(tmp_path):
    fields = ["distance", "point", "normal", "feature", "kind", "index", "sub_object", "triangle", "material_index",
              "side", "_reserved"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                   'printf("%zu %zu %zu", sizeof(rt_near_point), offsetof(rt_near_point, max_distance), sizeof(struct rt_nearest));'
                   + "".join(f'printf(" %zu", offsetof(struct rt_nearest, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:3] == [16, 12, 64] == [B.NEAR_POINT.itemsize, B.NEAR_POINT.fields["max_distance"][1], B.NEAREST.itemsize]
    assert got[3:] == [B.NEAREST.fields[f][1] for f in fields] == [getattr(N.rt_nearest, f).offset for f in fields]
    assert ctypes.sizeof(N.rt_near_point) == 16 and ctypes.sizeof(N.rt_nearest) == 64


def test_entry_points_without_a_context(native_lib):
    q = np.zeros(2, B.NEAR_POINT)
    out = np.zeros(2, B.NEAREST)
    for count in (0, 2):
        assert native_lib.rt_nearest(None, N.ptr(q), N.ptr(out), count) == N.RT_E_INVALID
        assert native_lib.rt_nearest_device(None, None, None, count) == N.RT_E_INVALID
    assert not out.view(np.uint8).any()
    assert "rt_nearest" in N.SIGNATURES and "rt_nearest_device" in N.SIGNATURES
