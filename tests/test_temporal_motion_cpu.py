"""Motion records for the temporal denoiser without a GPU: the ABI surface (rt_motion, the four new
entry points), the host helper rt_motion_from_transforms against the scene builder, and the NumPy
restatement of the motion contract (tests/temporal_motion_ref.py).

No kernel launches here; tests/test_gpu_temporal_motion.py compares the kernels with the restatement.
"""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import _native as N
from rust_gpu_raytracing_amd import buffers as B
from rust_gpu_raytracing_amd import builder, motion
from rust_gpu_raytracing_amd.scene import build_config
from tests import temporal_motion_ref as TM
from tests import temporal_ref as T
from tests.test_gpu_temporal_motion import MAIN_EDIT, SECOND_EDIT, apply_edit
from tests.test_temporal_cpu import FRAMES, SMALL_FRAME, _flat, moving_sequence

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_abi.h"
KERNELS = ROOT / "rust_gpu_raytracing_amd" / "csrc" / "denoise.hip"
FUNCTIONS = ("rt_read_feature_ids", "rt_feature_ids_device", "rt_motion_from_transforms", "rt_denoise_temporal_motion")
FIELDS = ("m", "normal_scale", "flags", "_reserved")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------- ABI
def test_functions_declared_exported_and_bound(native_lib):
    declared = set(re.findall(r"^RT_API\s+[\w\s\*]+?\b(rt_\w+)\s*\(", HEADER.read_text(), re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in FUNCTIONS:
        assert name in declared and name in exported and name in N.SIGNATURES and hasattr(native_lib, name)
    assert native_lib.rt_abi_version() == 12
    assert "12, additive: motion records for the temporal denoiser" in HEADER.read_text()


def test_rt_motion_is_64_bytes_in_every_mirror(tmp_path):
    args = ["sizeof(rt_motion)"] + [f"offsetof(rt_motion, {f})" for f in FIELDS]
    fmt = " ".join(["%zu"] * len(args))
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {", ".join(args)}); return 0;}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [64, 0, 48, 52, 56]
    assert ctypes.sizeof(N.rt_motion) == motion.MOTION.itemsize == TM.MOTION.itemsize == 64
    assert [getattr(N.rt_motion, f).offset for f in FIELDS] == got[1:]
    assert [motion.MOTION.fields[f][1] for f in FIELDS] == got[1:]
    assert (N.RT_MOTION_MOVED, N.RT_MOTION_DROP) == (motion.MOVED, motion.DROP) == (TM.MOVED, TM.DROP) == (1, 2)
    assert ctypes.sizeof(N.rt_object_transform) == B.OBJECT_TRANSFORM.itemsize == 32


def test_null_context_fails_cleanly(native_lib):
    t = N.rt_temporal_params()
    buf = (ctypes.c_uint32 * 4)()
    assert native_lib.rt_denoise_temporal_motion(None, ctypes.byref(t), None, None, 0, None, 0) == N.RT_E_INVALID
    assert native_lib.rt_read_feature_ids(None, buf) == N.RT_E_INVALID
    assert native_lib.rt_feature_ids_device(None, None) == N.RT_E_INVALID
    assert not any(buf)


def _contract(path, lead):
    lines = path.read_text().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith(lead + " THE MOTION STAGE"))
    last = next(i for i, l in enumerate(lines) if l.startswith(lead + " End of the motion contract."))
    assert all(l.startswith(lead) for l in lines[first:last + 1])
    return [l[len(lead):].rstrip().rstrip("/").rstrip("*").rstrip() for l in lines[first:last + 1]]


def test_contract_text_is_in_kernel_source_and_header():
    """The motion contract in include/rt_abi.h equals the header comment of denoise.hip line for
    line, and the lines the restatement is written from are there."""
    in_header, in_kernels = _contract(HEADER, " *"), _contract(KERNELS, "//")
    assert in_header == in_kernels
    text = "\n".join(in_kernels)
    for line in ["The record R is objects[id.y] if id.x == 2 && id.y < object_count.",
                 "R is spheres[id.y] if id.x == 1 && id.y < sphere_count.",
                 "Otherwise there is no record. Misses never have one.",
                 "If R has DROP, the pixel has no history.",
                 "Y_i = ((m[4i]*X.x + m[4i+1]*X.y) + m[4i+2]*X.z) + m[4i+3];",
                 "g_i = ((m[4i]*n.x + m[4i+1]*n.y) + m[4i+2]*n.z) * normal_scale.",
                 "Otherwise Y = X_p and g = n_p, chosen by selection. The pixel does no arithmetic.",
                 "3m. Projection. Step 3 projects Y instead of X_p.",
                 "with g in the normal test and e = Y - X_q in the position test.",
                 "f = X_p - o and r2 are unchanged. The tolerance scales with the current distance.",
                 "On a hit, and only when the previous slot has an I plane, one further test applies: both words of",
                 "7m. Store. Store as step 7: X = (X_p, hit_p) and Nn = (n_p, n_out). In addition I = id_p."]:
        assert line in text, line


# ---------------------------------------------------------------------------- the helper
def _states(n=3):
    s = np.zeros(n, B.OBJECT_TRANSFORM)
    s["scale"] = 1.0
    s["rotation"] = [(0, 0, 0), (10, 20, 30), (-45, 5, 170)][:n]
    s["transformation"] = [(0, 0, 0), (1, -2, 3), (5.3, -0.7, 1.51)][:n]
    return s


def test_flag_rules():
    prev = _states()
    cur = prev.copy()
    cur["transformation"][1] += np.float32(0.25)
    cur["_padding"][2] = 7  # not byte-identical: MOVED, with A the identity up to rounding
    rec = motion.object_motion(prev, cur)
    assert rec["flags"].tolist() == [0, motion.MOVED, motion.MOVED]
    assert np.array_equal(rec[0:1], motion.static(1)) and not rec["_reserved"].any()
    assert np.allclose(rec["m"][2].reshape(3, 4), np.eye(3, 4), atol=1e-6) and rec["normal_scale"][2] == 1
    assert motion.object_motion(prev[:0], cur[:0]).shape == (0,)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for which in (prev, cur):
            broken = which.copy()
            broken["scale"][1] = bad
            args = (broken, cur) if which is prev else (prev, broken)
            with pytest.raises(N.RtError) as e:
                motion.object_motion(*args)
            assert e.value.code == N.RT_E_INVALID
    lib = N.load_library()
    assert lib.rt_motion_from_transforms(None, None, 0, None) == N.RT_OK
    assert lib.rt_motion_from_transforms(None, N.ptr(cur), 3, N.ptr(rec)) == N.RT_E_INVALID
    # spheres: L = I, t = c_prev - c_cur, flags 0 where the centres are byte-equal
    a = np.zeros(3, B.SPHERE)
    a["position"] = [(1, 2, 3), (4, 5, 6), (0, 0, 0)]
    a["radius"] = 1.0
    b = a.copy()
    b["position"][1] += np.float32(0.5)
    b["radius"][2] = 2.0  # a radius change is the caller's business
    sm = motion.sphere_motion(a, b)
    assert sm["flags"].tolist() == [0, motion.MOVED, 0]
    assert np.array_equal(sm["m"][1].reshape(3, 4), np.concatenate([np.eye(3), [[-0.5], [-0.5], [-0.5]]], axis=1))
    assert np.array_equal(sm[[0, 2]], motion.static(2))


def test_helper_record_carries_the_builders_vertices_back():
    """For the edits the GPU test makes (MAIN_EDIT, SECOND_EDIT, and one after the other) on a chess
    piece: the record of rt_motion_from_transforms, applied in f32 exactly as step 2m applies it, to
    the current pose's triangle vertices from builder.update_object, against the previous pose's
    vertices. The two f32 pose evaluations round independently, so the bound is four times the
    largest deviation measured on the CPU: measured 9.54e-7 (two ulps of a coordinate near 5; the
    pieces are about 2 across and up to 8 from the origin), bound 3.82e-6."""
    scene, _ = build_config("c3_chess", width=16, height=16, env_size=(16, 8), texture_size=(8, 8))
    f32 = np.float32
    worst = 0.0
    for index, edits in ((1, (MAIN_EDIT,)), (9, (SECOND_EDIT,)), (20, (MAIN_EDIT, SECOND_EDIT))):
        obj = scene.objects[index]
        builder.update_object(obj)
        for edit in edits:
            prev_state, prev_tris = builder.transform_of(obj), obj.triangles.copy()
            apply_edit(obj, edit)
            builder.update_object(obj)
            rec = motion.object_motion(prev_state[None], builder.transform_of(obj)[None])[0]
            assert rec["flags"] == motion.MOVED
            m = rec["m"]
            for field, edges in (("a", ()), ("a", ("edge_ab",)), ("a", ("edge_ac",))):
                X = obj.triangles[field].astype(f32)
                P = prev_tris[field].astype(f32)
                for e in edges:
                    X, P = (X + obj.triangles[e]).astype(f32), (P + prev_tris[e]).astype(f32)
                Y = np.stack([((m[4 * i] * X[:, 0] + m[4 * i + 1] * X[:, 1]) + m[4 * i + 2] * X[:, 2]) + m[4 * i + 3]
                              for i in range(3)], axis=-1)
                assert Y.dtype == f32
                worst = max(worst, float(np.abs(Y.astype(np.float64) - P).max()))
    print(f"largest vertex deviation {worst:.3e}")
    assert 0.0 < worst <= 4 * 9.54e-7


# ---------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["c2_64x36_b8", "c3_64x36_b8"])
def test_restatement_without_records_or_ids_is_the_plain_restatement(oracle_lib, name):
    """The inputs of test_temporal_cpu's moving-camera sequence: plain calls of the motion restatement
    are TemporalRef bit for bit, and so is a motion call with empty tables whose previous slot was
    written by a plain call (no ids to test) -- whatever the ID plane holds."""
    from tests.golden.fixtures import CASES

    seq, _ = moving_sequence(name)
    spp = CASES[name]["spp"]
    rng = np.random.default_rng(3)
    for tparams in ({}, SMALL_FRAME):
        plain, ref = T.TemporalRef(), TM.TemporalMotionRef()
        for i, (cam, rays, acc, feats) in enumerate(seq):
            h, w = acc.shape[:2]
            args = (cam.position, rays["direction"].reshape(h, w, 3), 2, spp, i, cam.world_to_pixel())
            want = plain.call(acc, feats, *args, **tparams)
            if i % 2 == 0:
                got = ref.call(acc, feats, *args, **tparams)
            else:
                ids = rng.integers(0, 3, (h, w, 2)).astype(np.uint32)
                got = ref.call_motion(acc, feats, ids, *args, **tparams)
                assert got["counters"]["ids_absent"] == h * w  # the slot before it was written by a plain call
            for key in ("out", "n_out", "f"):
                assert np.array_equal(bits(got[key]), bits(want[key])), (i, key)
            assert np.array_equal(got["u"], want["u"])
            assert all(got["counters"][k] == v for k, v in want["counters"].items())
    assert len(seq) == FRAMES


def _synthetic(region_x, colour_region, n):
    """The fronto-parallel plane of test_temporal_cpu._flat, 12 x 24 pixels: object 1 everywhere but for
    a 3-pixel-wide band of object 0 starting at column ``region_x``, which has its own colour."""
    cam, d, feats, acc = _flat(12, 24, 1, (0.2, 0.2, 0.2, 1.0), n)
    ids = np.zeros((12, 24, 2), np.uint32)
    ids[..., 0], ids[..., 1] = 2, 1
    ids[2:10, region_x:region_x + 3, 1] = 0
    region = ids[..., 1] == 0
    acc[region] = np.asarray(colour_region, np.float32) * np.float32(n)
    return cam, d, feats, acc, ids, region


def test_restatement_follows_a_region_that_shifts_by_whole_pixels():
    """An id region shifts by 5 pixels between two generations. With its MOVED record its pixels find
    history and n_out = N + nh; without the record they do not (the id test rejects what they
    reproject onto), and with DROP they do not."""
    colour = (0.9, 0.1, 0.4, 1.0)
    cam, d, feats, acc0, ids0, region0 = _synthetic(4, colour, 3)
    _, _, _, acc1, ids1, region1 = _synthetic(9, colour, 2)
    m = cam.world_to_pixel()
    X = cam.position + d * feats["depth"][..., None]
    step = np.float32(X[0, 1, 0] - X[0, 0, 0])  # world units per pixel on the plane
    rec = motion.static(2)
    rec["m"][0, 3] = -5 * step
    rec["flags"][0] = motion.MOVED
    results = {}
    for what, objects in (("moved", rec), ("none", None), ("short", rec[:0]), ("drop", None)):
        if what == "drop":
            objects = rec.copy()
            objects["flags"][0] |= motion.DROP
        ref = TM.TemporalMotionRef()
        a = ref.call_motion(acc0, feats, ids0, cam.position, d, 4, 1, 0, m)
        assert (a["n_out"] == 3).all()
        results[what] = ref.call_motion(acc1, feats, ids1, cam.position, d, 3, 1, 1, m, objects=objects,
                                        sigma_position=0.05, iterations=0)
    r = results["moved"]
    assert np.allclose(r["n_out"][region1], 5.0, rtol=1e-6) and (r["n_out"][region1] > 2).all()   # N + nh = 2 + 3
    assert np.allclose(r["out"][region1], colour, rtol=1e-5)
    c = r["counters"]
    assert c["moved_found"] == region1.sum() and c["moved_lost"] == 0 and c["dropped"] == 0 and c["ids_absent"] == 0
    middle = np.zeros_like(region0)
    middle[2:10, 5] = True  # uncovered, and both columns a reprojection can tap were object 0: the id test rejects
    assert (r["n_out"][middle] == 2).all() and c["rejected_id"] >= middle.sum()
    for what in ("none", "short"):
        r = results[what]
        assert (r["n_out"][region1] == 2).all() and np.array_equal(r["out"][region1], (acc1 / np.float32(2))[region1])
        assert r["counters"]["moved_found"] == 0 and r["counters"]["rejected_id"] >= region1.sum()
    assert np.array_equal(bits(results["none"]["out"]), bits(results["short"]["out"]))
    r = results["drop"]
    assert (r["n_out"][region1] == 2).all() and r["counters"]["dropped"] == region1.sum()
    assert r["counters"]["moved_found"] == r["counters"]["moved_lost"] == 0
    far = ~region0 & ~region1
    far[:, [0, -1]] = far[[0, -1], :] = False
    for r in results.values():  # everything else is static and keeps its history
        assert np.allclose(r["n_out"][far], 5.0, rtol=1e-6) and r["counters"]["static_found"] >= far.sum()
