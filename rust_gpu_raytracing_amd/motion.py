"""Motion records for ``Renderer.denoise_temporal_motion`` (rt_motion, include/rt_abi.h).

A record says where the surface point that is now at X was at the previous temporal call: A X with
A = (L | t) a row-major 3x4, and how a normal goes back with it, n' = (L n) * normal_scale.

    before = motion.snapshot(scene)          # at the previous denoise_temporal_motion
    ...edit scene.objects / scene.spheres, renderer.update_scene()...
    now = motion.snapshot(scene)
    renderer.denoise_temporal_motion(w2p, objects=motion.object_motion(before["objects"], now["objects"]),
                                     spheres=motion.sphere_motion(before["spheres"], now["spheres"]))

Mark a primitive that appeared, teleported or changed material with ``records["flags"][i] = DROP``.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from . import buffers as B

MOTION = np.dtype([("m", "<f4", 12), ("normal_scale", "<f4"), ("flags", "<u4"), ("_reserved", "<u4", 2)])
assert MOTION.itemsize == 64
MOVED, DROP = N.RT_MOTION_MOVED, N.RT_MOTION_DROP


def static(count: int) -> np.ndarray:
    """``count`` records of primitives that did not move (flags 0, A the identity)."""
    out = np.zeros(count, MOTION)
    out["m"][:, [0, 5, 10]] = 1.0
    out["normal_scale"] = 1.0
    return out


def snapshot(scene) -> dict:
    """The states ``object_motion`` and ``sphere_motion`` need later: copies of every object's edit
    state (``buffers.OBJECT_TRANSFORM``) and of the sphere records."""
    from . import builder

    objs = np.stack([builder.transform_of(o) for o in scene.objects]) if scene.objects \
        else np.zeros(0, B.OBJECT_TRANSFORM)
    return {"objects": np.ascontiguousarray(objs), "spheres": np.array(scene.spheres, B.SPHERE, copy=True)}


def object_motion(prev_states, cur_states, lib=None) -> np.ndarray:
    """rt_motion_from_transforms: one record per object from its edit state at the previous and at
    the current call (``buffers.OBJECT_TRANSFORM`` arrays of equal length). A byte-identical pair is
    static (flags 0); a scale that is not finite or <= 0 raises RtError (RT_E_INVALID)."""
    lib = lib or N.load_library()
    prev = np.ascontiguousarray(prev_states, B.OBJECT_TRANSFORM).reshape(-1)
    cur = np.ascontiguousarray(cur_states, B.OBJECT_TRANSFORM).reshape(-1)
    if prev.shape != cur.shape:
        raise ValueError("prev_states and cur_states must have the same length")
    out = np.zeros(prev.shape[0], MOTION)
    N.check(None, lib.rt_motion_from_transforms(N.ptr(prev), N.ptr(cur), prev.shape[0], N.ptr(out)), lib)
    return out


def sphere_motion(prev_spheres, cur_spheres) -> np.ndarray:
    """One record per sphere (``buffers.SPHERE`` arrays of equal length): L = I, t = c_prev - c_cur in
    f32; flags 0 where the centres are byte-equal. A radius change is the caller's business (DROP)."""
    prev = np.ascontiguousarray(prev_spheres, B.SPHERE).reshape(-1)
    cur = np.ascontiguousarray(cur_spheres, B.SPHERE).reshape(-1)
    if prev.shape != cur.shape:
        raise ValueError("prev_spheres and cur_spheres must have the same length")
    out = static(prev.shape[0])
    pc, cc = np.ascontiguousarray(prev["position"]), np.ascontiguousarray(cur["position"])
    moved = (pc.view(np.uint32) != cc.view(np.uint32)).any(axis=1)
    t = (pc - cc).astype(np.float32)
    for i in range(3):
        out["m"][:, 4 * i + 3] = np.where(moved, t[:, i], np.float32(0.0))
    out["flags"] = np.where(moved, MOVED, 0).astype(np.uint32)
    return out
