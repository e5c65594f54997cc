"""Native scene building, CPU only.

The C++ restatement of src/triangle_object.rs (csrc/scene_build.cpp, through the
C ABI) must produce bit for bit the records of the Python restatement in
scene.py -- SceneObject::new, create_sub_objects, and the edit path
update_triangles + update_sub_objects under arbitrary rotations, scales and
translations -- and the chess scene must build to the counts the reference
asserts (src/main.rs:39-44, :123-128). STL parsing is checked against the
binary meshes in the committed fixture and against the reference's own
3D_models/*.stl files (copies under tests/golden/stl/).
"""
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import RtError
from rust_gpu_raytracing_amd import builder as NB
from rust_gpu_raytracing_amd import scene as S

REF_MODELS = Path(__file__).resolve().parent / "golden" / "stl"  # the reference's 3D_models/*.stl, as fixtures


def chess_meshes():
    assets = S.load_chess_assets()
    return {k[4:]: v for k, v in assets.items() if k.startswith("stl_")}


def chess_creations(meshes):
    captured = []
    orig = S.load_stl_files
    try:
        S.load_stl_files = lambda c, m: captured.append(list(c)) or orig(c, m)
        objs = S.chess_objects(meshes)
    finally:
        S.load_stl_files = orig
    return captured[0], objs


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def assert_objects_equal(py, nat):
    assert len(py) == len(nat)
    for i, (p, c) in enumerate(zip(py, nat)):
        assert same(p.object_info, c.object_info), i
        assert same(p.triangles, c.triangles), i
        assert same(p.sub_object_info, c.sub_object_info), i
        assert same(p.normalized_points, c.normalized_points), i
        assert same(p.transformation, c.transformation), i
        assert same(p.rotation, c.rotation) and np.float32(p.scale) == np.float32(c.scale), i


def test_native_chess_build_matches_restatement_and_reference_counts(native_lib):
    meshes = chess_meshes()
    creations, objs_py = chess_creations(meshes)
    objs = NB.load_stl_files(creations, meshes)
    assert_objects_equal(objs_py, objs)
    # src/main.rs:39-44 (asserted at :123-128)
    assert sum(o.triangles.shape[0] for o in objs) == 5552
    assert sum(o.sub_object_info.shape[0] for o in objs) == 802
    assert len(objs) == 34


@pytest.mark.parametrize("seed", [0, 1])
def test_native_update_matches_restatement(native_lib, seed):
    meshes = chess_meshes()
    creations, objs_py = chess_creations(meshes)
    objs = NB.load_stl_files(creations, meshes)
    rng = np.random.default_rng(seed)
    for step in range(2):
        for p, c in zip(objs_py, objs):
            rot = (rng.random(3) * 720 - 360).astype(np.float32)
            sc = np.float32(0.25 + 2 * rng.random())
            tr = (rng.random(3) * 20 - 10).astype(np.float32)
            if step == 1:  # the UI's "drop to surface" and "reset rotation" (:149-158)
                p.set_model_to_surface(), c.set_model_to_surface()
                p.reset_rotation(), c.reset_rotation()
            else:
                for o in (p, c):
                    o.rotation, o.scale, o.transformation = rot.copy(), sc, tr.copy()
            p.update_triangles()
            p.update_sub_objects()
            NB.update_object(c)
        assert_objects_equal(objs_py, objs)


def test_update_with_identity_state_moves_only_by_rounding(native_lib):
    # update_triangles right after new(): rotation 0, scale 1, same total translation,
    # but (p + surface) + coords becomes p + (coords + surface): equal to f32 rounding
    meshes = chess_meshes()
    o = NB.object_new(meshes["Knight"], 2.0, [5.3, -0.7, 1.5], [90.0, 0.0, 0.0], 9)
    NB.create_sub_objects(o, 0, 0)
    before = o.triangles.copy()
    NB.update_object(o)
    np.testing.assert_allclose(o.triangles["a"], before["a"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(o.triangles["face_normal"], before["face_normal"], rtol=0, atol=1e-4)


def test_bounding_box_scan_semantics():
    # get_bounding_box (src/triangle_object.rs:292-321): strict < / > from +-f32::MAX:
    # NaN never wins, the first of equal values (+0 / -0) is kept, empty -> (MAX, MIN)
    nz = np.float32(-0.0)
    pts = np.array([[0.0, np.nan, 1.0], [nz, 2.0, 1.0], [3.0, -1.0, nz]], np.float32)
    mn, mx = S.bounding_box(pts)
    assert mn.tolist() == [0.0, -1.0, 0.0] and not np.signbit(mn[0]) and np.signbit(mn[2])
    assert mx.tolist() == [3.0, 2.0, 1.0]
    mn, mx = S.bounding_box(np.zeros((0, 3), np.float32))
    big = np.finfo(np.float32).max
    assert mn.tolist() == [big] * 3 and mx.tolist() == [-big] * 3


def test_stl_binary_roundtrip(native_lib):
    meshes = chess_meshes()
    for name, v in meshes.items():
        got = NB.read_stl(NB.write_binary_stl(v))
        assert got.shape == v.shape and same(got, v), name


def test_stl_ascii_and_errors(native_lib):
    text = b"""solid tri
facet normal 0 0 1
 outer loop
  vertex 0 0 0
  vertex 1 0 0
  vertex 0 1.5 -2e-3
 endloop
endfacet
facet normal 0 0 1
 outer loop
  vertex 1 1 1
  vertex 2 2 2
  vertex 3 3 3
 endloop
endfacet
endsolid tri
"""
    v = NB.read_stl(text)
    assert v.shape == (2, 3, 3)
    assert v[0, 2].tolist() == [0.0, 1.5, np.float32(-2e-3)]
    with pytest.raises(RtError):
        NB.read_stl(b"not an stl file at all" * 10)
    with pytest.raises(RtError):
        NB.read_stl(b"solid x\n vertex 1 2 3\n vertex 4 5 6\nendsolid\n")  # 2 vertices
    with pytest.raises(RtError):
        NB.object_new(np.zeros((1, 3, 3), np.float32), 0.0, [0, 0, 0], [0, 0, 0], 0)  # scale > 0 (:67)


def test_stl_reference_files(native_lib):
    meshes = chess_meshes()
    for name, v in meshes.items():
        got = NB.read_stl((REF_MODELS / f"{name}.stl").read_bytes())
        assert same(got, v), name
