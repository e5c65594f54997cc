"""``Renderer`` — the host side of the hot path, over the C ABI.

Mirrors ``Renderer`` in src/renderer.rs:28-320 (names, argument meaning and
call order), with wgpu replaced by ``include/rt_abi.h``:

===========================================  ==========================================
reference (src/renderer.rs)                  here
===========================================  ==========================================
``Renderer::new`` :42-101                    ``Renderer(scene, ...)`` -> ``rt_create`` +
                                             ``rt_upload_textures`` + ``rt_upload_env_map``
``reset_accumulation`` :131-151              ``reset_accumulation()`` -> ``rt_reset_accumulation``
``update_scene`` :153-199                    ``update_scene()`` -> ``rt_update_*``, or
                                             ``update_scene(device=True)`` -> ``rt_update_objects``
``compute_frame`` :201-252                   ``compute_frame(bounces)`` -> ``rt_compute_frame``
``on_update`` (camera moved) :109-129        ``update_camera(camera)``
(no readback in the reference)               ``read_output`` / ``read_accumulation``
===========================================  ==========================================

Errors raise :class:`RtError` (the reference panics via ``.expect``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from . import buffers as B
from .scene import RenderScene

REFERENCE_BOUNCES = 10  # compute_shader.wgsl:150


class Renderer:
    def __init__(
        self,
        scene: RenderScene,
        *,
        accumulate: bool = True,
        compute_per_frame: int = 1,
        device: int = 0,
        rank: int = 0,
        world_size: int = 1,
        camera_rays: np.ndarray | None = None,
        device_rays: bool | None = None,
        frame_batch: int | None = None,
        tuning: dict[str, int] | None = None,
        lib=None,
    ):
        """``camera_rays``: explicit per-pixel directions (the reference's ray buffer;
        default: ``scene.camera.recalculate_ray_directions()``). ``device_rays=True``
        computes them on the device from the camera's matrices instead
        (rt_update_camera_matrices; bit-identical, no ray buffer read, but measured
        2% slower on C2 than reading the buffer, so off by default).
        ``frame_batch``: frames one launch may render (rt_set_frame_batch): with
        F > 1, ``compute_frame`` queues frames and launches F at a time (or at the
        next readback / update / sync), each frame's results written as before.
        None keeps the library's default (RT_DEFAULT_FRAME_BATCH, include/rt_abi.h).
        ``tuning``: exact variants of the schedule and acceleration structures for A/B
        runs, {key: value} passed to rt_set_tuning (include/rt_abi.h lists the keys)."""
        self._lib = N.load_library() if lib is None else lib
        self.scene = scene
        self.accumulate = accumulate
        self.compute_per_frame = compute_per_frame
        self.width = scene.camera.viewport_width
        self.height = scene.camera.viewport_height
        self.rank, self.world_size = rank, world_size
        self.device = device
        self._ctx = None
        rays = scene.camera.recalculate_ray_directions() if camera_rays is None else camera_rays
        self.camera_rays = np.ascontiguousarray(rays, dtype=B.RAY)
        objs, subs, tris = scene.flatten()
        self._keep = [self.camera_rays, scene.materials, scene.spheres, tris, objs, subs]

        info = N.rt_create_info()
        info.width, info.height, info.device = self.width, self.height, device
        info.camera.origin[:] = [float(x) for x in scene.camera.position]
        info.camera_rays = N.ptr(self.camera_rays)
        info.materials, info.material_count = N.ptr(scene.materials), scene.materials.shape[0]
        info.spheres, info.sphere_count = N.ptr(scene.spheres), scene.spheres.shape[0]
        info.triangles, info.triangle_count = N.ptr(tris), tris.shape[0]
        info.objects, info.object_count = N.ptr(objs), objs.shape[0]
        info.sub_objects, info.sub_object_count = N.ptr(subs), subs.shape[0]
        info.params = N.params_struct(self._params(accumulation_index=1))
        info.rank, info.world_size = rank, world_size
        ctx = ctypes.c_void_p()
        N.check(None, self._lib.rt_create(ctypes.byref(info), ctypes.byref(ctx)), self._lib)
        self._ctx = ctx
        self._upload_textures()
        self.device_rays = bool(device_rays)
        if self.device_rays:
            self._set_camera_matrices(scene.camera)
        if frame_batch is not None:
            self.set_frame_batch(frame_batch)
        for key, value in (tuning or {}).items():
            self.set_tuning(key, value)

    # ------------------------------------------------------------------ helpers
    def _params(self, accumulation_index: int) -> np.ndarray:
        return self.scene.params(
            accumulate=int(self.accumulate),
            compute_per_frame=self.compute_per_frame,
            accumulation_index=accumulation_index,
        )

    def _call(self, name, *args):
        if self._ctx is None:
            raise N.RtError(N.RT_E_INVALID, "renderer is closed")
        N.check(self._ctx, getattr(self._lib, name)(self._ctx, *args), self._lib)

    def _upload_textures(self):
        tex = np.ascontiguousarray(self.scene.textures, np.uint8)
        layers, th, tw, _ = tex.shape
        self._call("rt_upload_textures", N.ptr(tex), tw, th, layers)
        env = np.ascontiguousarray(self.scene.environment_map, np.uint8)
        eh, ew, _ = env.shape
        self._call("rt_upload_env_map", N.ptr(env), ew, eh)

    # ------------------------------------------------------------------ reference surface
    def reset_accumulation(self) -> None:
        """src/renderer.rs:131-151."""
        p = N.params_struct(self._params(accumulation_index=1))
        self._call("rt_reset_accumulation", ctypes.byref(p))

    def update_scene(self, device: bool = False) -> None:
        """src/renderer.rs:153-199: reset, re-upload spheres, rebuild every object's
        triangles from its edit state (update_triangles + update_sub_objects,
        src/triangle_object.rs:129-150, :199-220), re-upload textures, env map,
        triangles, objects, sub-objects and materials.

        ``device=False`` rebuilds the objects on the host (native builder,
        bit-identical to scene.py) and uploads them, as the reference does.
        ``device=True`` runs the rebuild on the GPU instead (``update_objects``):
        nothing but the 32-B edit state per object crosses PCIe, and the host
        ``scene.objects`` records are left as they were."""
        from . import builder

        self.reset_accumulation()
        s = self.scene
        self._call("rt_update_spheres", N.ptr(s.spheres), s.spheres.shape[0])
        self._upload_textures()
        if device:
            # the device rebuild rewrites bounds only; every other ObjectInfo field
            # (material_index, src/renderer.rs:188-193) comes from the host records
            self._upload_object_fields()
            self.update_objects()
        else:
            self._models = None  # the host path may change the objects: re-upload models for device edits
            for o in s.objects:
                builder.update_object(o, lib=self._lib)
            objs, subs, tris = s.flatten()
            self._keep[3:6] = [tris, objs, subs]
            self._call("rt_update_triangles", N.ptr(tris), tris.shape[0])
            self._call("rt_update_object_info", N.ptr(objs), objs.shape[0])
            self._call("rt_update_sub_object_info", N.ptr(subs), subs.shape[0])
        self._call("rt_update_materials", N.ptr(s.materials), s.materials.shape[0])

    def _upload_object_fields(self) -> None:
        """The host ObjectInfo records with the device's current bounds (a device
        edit leaves the host bounds stale): material index and sub-object range
        reach the device without invalidating the triangle accelerator."""
        objs = np.stack([np.asarray(o.object_info) for o in self.scene.objects]).astype(B.OBJECT_INFO) \
            if self.scene.objects else np.zeros(0, B.OBJECT_INFO)
        if objs.shape[0] == 0:
            return
        dev = np.zeros(objs.shape[0], B.OBJECT_INFO)
        self._call("rt_read_object_info", N.ptr(dev), dev.shape[0])
        merged = objs.copy()
        merged["min_bounds"] = dev["min_bounds"]
        merged["max_bounds"] = dev["max_bounds"]
        merged = np.ascontiguousarray(merged)
        self._call("rt_update_object_info", N.ptr(merged), merged.shape[0])

    def upload_object_models(self) -> None:
        """The objects' normalised points (rt_set_object_models), once, for device-side edits."""
        pts = [np.asarray(o.normalized_points, np.float32).reshape(-1, 9) for o in self.scene.objects]
        self._models = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 9), np.float32))
        self._models_key = tuple(id(o) for o in self.scene.objects)
        self._call("rt_set_object_models", N.ptr(self._models), self._models.shape[0])

    def update_objects(self) -> None:
        """update_triangles + update_sub_objects for every object, on the device
        (rt_update_objects): triangles, object and sub-object bounds rebuilt and
        the triangle accelerator refitted, stream-ordered before the next frame."""
        from . import builder

        if getattr(self, "_models", None) is None or \
                getattr(self, "_models_key", None) != tuple(id(o) for o in self.scene.objects):
            self.upload_object_models()
        t = np.ascontiguousarray(np.stack([builder.transform_of(o) for o in self.scene.objects])) \
            if self.scene.objects else np.zeros(0, B.OBJECT_TRANSFORM)
        self._call("rt_update_objects", N.ptr(t), t.shape[0])

    def read_geometry(self):
        """(objects, sub-objects, triangles) as the device holds them (rt_read_*)."""
        objs, subs, tris = self.scene.flatten()
        o = np.zeros(objs.shape[0], B.OBJECT_INFO)
        so = np.zeros(subs.shape[0], B.SUB_OBJECT_INFO)
        t = np.zeros(tris.shape[0], B.TRIANGLE)
        self._call("rt_read_object_info", N.ptr(o), o.shape[0])
        self._call("rt_read_sub_object_info", N.ptr(so), so.shape[0])
        self._call("rt_read_triangles", N.ptr(t), t.shape[0])
        return o, so, t

    def _set_camera_matrices(self, camera) -> None:
        self._inv = [np.ascontiguousarray(camera.inverse_projection, np.float32).reshape(16),
                     np.ascontiguousarray(camera.inverse_view, np.float32).reshape(16)]
        self._call("rt_update_camera_matrices", N.ptr(self._inv[0]), N.ptr(self._inv[1]))

    def update_camera(self, camera) -> None:
        """src/renderer.rs:109-129 after a move: reset, new origin, new ray directions."""
        self.scene.camera = camera
        self.reset_accumulation()
        rc = N.rt_ray_camera()
        rc.origin[:] = [float(x) for x in camera.position]
        self._call("rt_update_camera", ctypes.byref(rc))
        if self.device_rays:
            self._set_camera_matrices(camera)
            return
        self.camera_rays = np.ascontiguousarray(camera.recalculate_ray_directions())
        self._keep[0] = self.camera_rays
        self._call("rt_update_ray_directions", N.ptr(self.camera_rays), self.camera_rays.shape[0])

    def compute_frame(self, bounces: int = REFERENCE_BOUNCES) -> None:
        """src/renderer.rs:201-252 (asynchronous). Called once per frame: one ctypes
        call, the error path only on failure."""
        rc = self._lib.rt_compute_frame(self._ctx, bounces)
        if rc != N.RT_OK:
            if self._ctx is None:
                raise N.RtError(N.RT_E_INVALID, "renderer is closed")
            N.check(self._ctx, rc, self._lib)

    def compute_frames(self, bounces: int = REFERENCE_BOUNCES, frames: int = 1) -> None:
        """``frames`` compute_frame calls fused into one launch (same results;
        rt_compute_frames in include/rt_abi.h). Asynchronous."""
        self._call("rt_compute_frames", bounces, frames)

    def submit_frames(self, bounces: int = REFERENCE_BOUNCES, count: int = 1) -> None:
        """``count`` compute_frame calls in one C call (rt_submit_frames: the host loop a native
        caller runs, without a ctypes round trip per frame). Asynchronous."""
        self._call("rt_submit_frames", bounces, count)

    def set_frame_batch(self, max_frames: int) -> None:
        """rt_set_frame_batch: up to ``max_frames`` queued compute_frame calls per launch."""
        self._call("rt_set_frame_batch", max_frames)

    def frame_batch(self):
        """(max frames per launch, frames queued now)."""
        m, p = ctypes.c_uint32(), ctypes.c_uint32()
        N.check(self._ctx, self._lib.rt_frame_batch(self._ctx, ctypes.byref(m), ctypes.byref(p)), self._lib)
        return m.value, p.value

    def flush(self) -> None:
        """Launch the queued frames now (rt_flush); every other call does so implicitly."""
        self._call("rt_flush")

    # ------------------------------------------------------------------ readback & stats
    def synchronize(self) -> None:
        self._call("rt_synchronize")

    def read_output(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.uint32)
        self._call("rt_read_output", N.ptr(out))
        return out

    def read_accumulation(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._call("rt_read_accumulation", N.ptr(out))
        return out

    # ------------------------------------------------------------------ ray queries
    def trace_rays(self, rays):
        """The closest hit of every ray (rt_trace_rays): bit-identical to the reference's
        trace_ray, against the scene as it is now, without touching anything a render reads.

        ``rays``: an (n, 6) float32 array (origin, direction) or a ``buffers.QUERY_RAY`` array;
        returns a ``buffers.HIT`` array. A CUDA torch tensor of shape (n, 8) float32
        (rt_query_ray records) goes through rt_trace_rays_device instead -- no host round
        trip, stream-ordered on the context's stream -- and returns a CUDA (n, 16) int32
        tensor of rt_hit records."""
        if not isinstance(rays, np.ndarray) and hasattr(rays, "is_cuda"):
            return self._device_query("rt_trace_rays_device", rays, 8, "rays", (16,), "int32", call_empty=False)
        rays = np.asarray(rays)
        if rays.dtype != B.QUERY_RAY:
            r = np.ascontiguousarray(rays, np.float32)
            if r.ndim != 2 or r.shape[1] != 6:
                raise ValueError("rays must be (n, 6) float32 or a QUERY_RAY array")
            rays = np.zeros(r.shape[0], B.QUERY_RAY)
            rays["origin"] = r[:, :3]
            rays["direction"] = r[:, 3:]
        rays = np.ascontiguousarray(rays.reshape(-1))
        hits = np.zeros(rays.shape[0], B.HIT)
        self._call("rt_trace_rays", N.ptr(rays), N.ptr(hits), rays.shape[0])
        return hits

    def _device_query(self, entry, records, columns, noun, out_shape, out_dtype, scalars=(), segments=None,
                      call_empty=True):
        """The device form of a query, ``entry``: ``records``, a CUDA float32 tensor of shape
        (n, ``columns``) that the messages call ``noun``, answered into a new (n, *``out_shape``)
        tensor of the torch dtype named ``out_dtype``. ``scalars`` follow the count in the call.
        ``segments``: None for an entry without a segments argument, else whether to count them (a
        null pointer if not); counted, (out, segments) comes back. Without ``call_empty`` an empty
        batch returns before the call, else the call is made with null record pointers."""
        import torch

        if not records.is_cuda or records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != columns:
            raise ValueError(f"device {noun} must be a CUDA float32 tensor of shape (n, {columns})")
        if records.device.index != self.device:
            raise ValueError(f"device {noun} must live on the renderer's device")
        records = records.contiguous()
        n = records.shape[0]
        out = torch.empty((n, *out_shape), dtype=getattr(torch, out_dtype), device=records.device)
        if n == 0 and not call_empty:
            return out
        counter = torch.zeros(1, dtype=torch.int64, device=records.device) if segments else None
        args = [ctypes.c_void_p(records.data_ptr() if n else None), ctypes.c_void_p(out.data_ptr() if n else None), n,
                *scalars]
        if segments is not None:
            args.append(ctypes.c_void_p(counter.data_ptr()) if segments else None)
        # the query runs on the context's stream: order it after the tensor's producers,
        # and the caller's stream after it
        mine = torch.cuda.ExternalStream(self.stream_handle, device=records.device)
        cur = torch.cuda.current_stream(records.device)
        mine.wait_stream(cur)
        self._call(entry, *args)
        # (no record_stream on the context's stream: the caller's stream, which owns both tensors,
        # is ordered after the query here, and the context's stream may be destroyed -- close() --
        # before the tensors are freed)
        cur.wait_stream(mine)
        return (out, int(counter.item())) if segments else out

    @staticmethod
    def _t_max_column(t_max, n):
        """``t_max``, a scalar or an (n,) array, as what a record array's t_max field takes."""
        bound = np.asarray(t_max, np.float32)
        if bound.ndim > 1 or (bound.ndim == 1 and bound.shape[0] != n):
            raise ValueError("t_max must be a scalar or an (n,) array")
        return bound

    @staticmethod
    def _pack_records(values, name, fields, noun, first_stream, streams, t_max=None):
        """The flat record array of a query with RNG streams, of the dtype ``name`` of ``buffers``:
        ``values`` as it is if it has that dtype (``streams`` must then be None), else an
        (n, 3 * len(fields)) float32 array whose columns fill ``fields`` three at a time, with
        ``streams`` (default: ``first_stream`` + the record's position in the batch) and, for
        records that have one, ``t_max``."""
        dtype = getattr(B, name)
        values = np.asarray(values)
        if values.dtype == dtype:
            if streams is not None:
                raise ValueError(f"{name} records carry their own stream" + (" and t_max" if "t_max" in dtype.names else ""))
        else:
            r = np.ascontiguousarray(values, np.float32)
            if r.ndim != 2 or r.shape[1] != 3 * len(fields):
                article = "an" if name[0] in "AEIOU" else "a"
                raise ValueError(f"{noun} must be (n, {3 * len(fields)}) float32 or {article} {name} array")
            values = np.zeros(r.shape[0], dtype)
            for i, field in enumerate(fields):
                values[field] = r[:, 3 * i:3 * i + 3]
            s = first_stream + np.arange(r.shape[0], dtype=np.uint32) if streams is None else np.asarray(streams, np.uint32)
            if s.shape != (r.shape[0],):
                raise ValueError("streams must be an (n,) array")
            values["stream"] = s
            if "t_max" in dtype.names:
                values["t_max"] = Renderer._t_max_column(t_max, r.shape[0])
        return np.ascontiguousarray(values.reshape(-1))

    def pick(self, x: int, y: int) -> np.ndarray:
        """The closest hit of pixel (x, y)'s un-jittered camera ray (rt_pick): one ``buffers.HIT``."""
        hit = np.zeros(1, B.HIT)
        self._call("rt_pick", int(x), int(y), N.ptr(hit))
        return hit[0]

    # ------------------------------------------------------------------ occlusion queries
    @staticmethod
    def _occlusion_rays(rays, t_max):
        """The flat ``buffers.OCCLUSION_RAY`` array of the host forms ``occluded`` and
        ``trace_hits`` accept."""
        rays = np.asarray(rays)
        if rays.dtype == B.OCCLUSION_RAY:
            if t_max is not None:
                raise ValueError("OCCLUSION_RAY records carry their own t_max")
        else:
            r = np.ascontiguousarray(rays, np.float32)
            if r.ndim != 2 or r.shape[1] not in (6, 7) or (r.shape[1] == 7 and t_max is not None):
                raise ValueError("rays must be (n, 7) float32, (n, 6) float32 with t_max, or an OCCLUSION_RAY array")
            rays = np.zeros(r.shape[0], B.OCCLUSION_RAY)
            rays["origin"] = r[:, :3]
            rays["direction"] = r[:, 3:6]
            if r.shape[1] == 7:
                rays["t_max"] = r[:, 6]
            else:
                rays["t_max"] = Renderer._t_max_column(np.inf if t_max is None else t_max, r.shape[0])
        return np.ascontiguousarray(rays.reshape(-1))

    def occluded(self, rays, t_max=None):
        """Whether anything lies on each ray before its ``t_max`` (rt_occluded): 1 iff a primitive
        is hit at a distance strictly below t_max (in units of |direction|, like ``HIT["t"]``),
        against the scene as it is now, without touching anything a render reads.

        ``rays``: an (n, 7) float32 array (origin, direction, t_max); an (n, 6) array with
        ``t_max`` a scalar or an (n,) array (None: +inf, "is there any hit at all"); or a
        ``buffers.OCCLUSION_RAY`` array. Returns an (n,) uint8 array. A CUDA torch tensor of
        shape (n, 8) float32 (rt_occlusion_ray records) goes through rt_occluded_device instead
        -- no host round trip, stream-ordered on the context's stream -- and returns a CUDA (n,)
        uint8 tensor."""
        if not isinstance(rays, np.ndarray) and hasattr(rays, "is_cuda"):
            if t_max is not None:
                raise ValueError("device rays carry t_max in their last column")
            return self._device_query("rt_occluded_device", rays, 8, "rays", (), "uint8", call_empty=False)
        rays = self._occlusion_rays(rays, t_max)
        out = np.zeros(rays.shape[0], np.uint8)
        self._call("rt_occluded", N.ptr(rays), N.ptr(out), rays.shape[0])
        return out

    def occluded_segments(self, a, b):
        """Whether anything lies strictly before ``b`` on the way from ``a``, per pair of (n, 3)
        float32 points: the ray origin = a, direction = b - a (in f32), t_max = 1."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError("a and b must both be (n, 3) float32")
        rays = np.zeros(a.shape[0], B.OCCLUSION_RAY)
        rays["origin"] = a
        rays["direction"] = b - a
        rays["t_max"] = 1.0
        return self.occluded(rays)

    # ------------------------------------------------------------------ hit-list queries
    def trace_hits(self, rays, t_max=None, max_hits: int = 4):
        """The ``max_hits`` nearest hits of every ray before its ``t_max``, in order
        (rt_trace_hits; THE HIT-LIST CONTRACT in include/rt_abi.h): every primitive the
        reference's test accepts on its own, ascending by distance, each as the record
        ``trace_rays`` builds for it, against the scene as it is now, without touching anything a
        render reads.

        ``rays``: what ``occluded`` accepts. Returns ``(hits, counts)``: an (n, max_hits)
        ``buffers.HIT`` array whose entries past a ray's count are miss records, and an (n,) uint32
        array of counts (saturating at ``max_hits``). A CUDA torch tensor of shape (n, 8) float32
        (rt_occlusion_ray records) goes through rt_trace_hits_device instead -- no host round
        trip, stream-ordered on the context's stream -- and returns CUDA tensors: (n, max_hits, 16)
        int32 records and (n,) int32 counts."""
        max_hits = int(max_hits)
        if not isinstance(rays, np.ndarray) and hasattr(rays, "is_cuda"):
            import torch

            if t_max is not None:
                raise ValueError("device rays carry t_max in their last column")
            if not rays.is_cuda or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
                raise ValueError("device rays must be a CUDA float32 tensor of shape (n, 8)")
            if rays.device.index != self.device:
                raise ValueError("device rays must live on the renderer's device")
            rays = rays.contiguous()
            n = rays.shape[0]
            hits = torch.empty((n, max(max_hits, 0), 16), dtype=torch.int32, device=rays.device)
            counts = torch.empty((n,), dtype=torch.int32, device=rays.device)
            # the query runs on the context's stream: after the tensor's producers, before the
            # caller's stream goes on (_device_query)
            mine = torch.cuda.ExternalStream(self.stream_handle, device=rays.device)
            cur = torch.cuda.current_stream(rays.device)
            mine.wait_stream(cur)
            self._call("rt_trace_hits_device", ctypes.c_void_p(rays.data_ptr() if n else None),
                       ctypes.c_void_p(hits.data_ptr() if n and max_hits > 0 else None),
                       ctypes.c_void_p(counts.data_ptr() if n else None), n, max_hits)
            cur.wait_stream(mine)
            return hits, counts
        rays = self._occlusion_rays(rays, t_max)
        hits = np.zeros((rays.shape[0], max(max_hits, 0)), B.HIT)
        counts = np.zeros(rays.shape[0], np.uint32)
        self._call("rt_trace_hits", N.ptr(rays), N.ptr(hits), N.ptr(counts), rays.shape[0], max_hits)
        return hits, counts

    # ------------------------------------------------------------------ proximity queries
    def nearest(self, points, max_distance=None):
        """The closest surface point to every point (rt_nearest; THE NEAREST-POINT CONTRACT in
        include/rt_abi.h): over every sphere and every triangle of the scene as it is now, within
        ``max_distance`` of the point, without touching anything a render reads.

        ``points``: an (n, 3) float32 array with ``max_distance`` a scalar or an (n,) array (None:
        +inf, "anything"); an (n, 4) array (position, max_distance); or a ``buffers.NEAR_POINT``
        array. Returns a ``buffers.NEAREST`` array. A CUDA torch tensor of shape (n, 4) float32
        (rt_near_point records) goes through rt_nearest_device instead -- no host round trip,
        stream-ordered on the context's stream -- and returns a CUDA (n, 16) int32 tensor of
        rt_nearest records."""
        if not isinstance(points, np.ndarray) and hasattr(points, "is_cuda"):
            if max_distance is not None:
                raise ValueError("device points carry max_distance in their last column")
            return self._device_query("rt_nearest_device", points, 4, "points", (16,), "int32", call_empty=False)
        points = np.asarray(points)
        if points.dtype == B.NEAR_POINT:
            if max_distance is not None:
                raise ValueError("NEAR_POINT records carry their own max_distance")
        else:
            r = np.ascontiguousarray(points, np.float32)
            if r.ndim != 2 or r.shape[1] not in (3, 4) or (r.shape[1] == 4 and max_distance is not None):
                raise ValueError("points must be (n, 4) float32, (n, 3) float32 with max_distance, or a NEAR_POINT array")
            points = np.zeros(r.shape[0], B.NEAR_POINT)
            points["position"] = r[:, :3]
            if r.shape[1] == 4:
                points["max_distance"] = r[:, 3]
            else:
                bound = np.asarray(np.inf if max_distance is None else max_distance, np.float32)
                if bound.ndim > 1 or (bound.ndim == 1 and bound.shape[0] != r.shape[0]):
                    raise ValueError("max_distance must be a scalar or an (n,) array")
                points["max_distance"] = bound
        points = np.ascontiguousarray(points.reshape(-1))
        out = np.zeros(points.shape[0], B.NEAREST)
        self._call("rt_nearest", N.ptr(points), N.ptr(out), points.shape[0])
        return out

    def pick_hits(self, x: int, y: int, max_hits: int = 4) -> np.ndarray:
        """The hits of pixel (x, y)'s un-jittered camera ray, nearest first (rt_pick_hits): the
        valid records of that ray's list, at most ``max_hits`` of them."""
        max_hits = int(max_hits)
        hits = np.zeros(max(max_hits, 1), B.HIT)
        n = ctypes.c_uint32()
        self._call("rt_pick_hits", int(x), int(y), N.ptr(hits), ctypes.byref(n), max_hits)
        return hits[:n.value]

    # ------------------------------------------------------------------ radiance queries
    def radiance(self, rays, streams=None, bounces: int = REFERENCE_BOUNCES, first_sample: int = 1,
                 samples: int = 1, return_segments: bool = False):
        """The light arriving along each ray (rt_radiance): the sum over ``samples`` samples of the
        reference's per_pixel with the camera origin, the pixel's direction and the pixel index of
        the seed taken from the ray's record -- what one compute_frame would add to a zeroed
        accumulation for such a pixel with accumulation_index = ``first_sample``. Divide by
        ``samples`` for the mean; nothing is clamped. Against the scene as it is now, without
        touching anything a render reads.

        ``rays``: an (n, 6) float32 array (origin, direction), with ``streams`` an (n,) uint32
        array of RNG streams (default: the ray's position in the batch, as a pixel index would
        be), or a ``buffers.RADIANCE_RAY`` array. Returns an (n, 4) float32 array, and with
        ``return_segments`` the batch's counted ray segments (the rule of ``ray_count``). A CUDA
        torch tensor of shape (n, 8) float32 (rt_radiance_ray records: the stream's bits in
        column 3) goes through rt_radiance_device instead -- no host round trip, stream-ordered
        on the context's stream -- and returns a CUDA (n, 4) float32 tensor."""
        if not isinstance(rays, np.ndarray) and hasattr(rays, "is_cuda"):
            if streams is not None:
                raise ValueError("device rays carry their stream in column 3")
            return self._device_query("rt_radiance_device", rays, 8, "rays", (4,), "float32",
                                      (int(bounces), int(first_sample), int(samples)), bool(return_segments))
        rays = self._pack_records(rays, "RADIANCE_RAY", ("origin", "direction"), "rays", 0, streams)
        out = np.zeros((rays.shape[0], 4), np.float32)
        segments = ctypes.c_uint64(0)
        self._call("rt_radiance", N.ptr(rays), N.ptr(out), rays.shape[0], int(bounces), int(first_sample),
                   int(samples), ctypes.byref(segments))
        return (out, segments.value) if return_segments else out

    # ------------------------------------------------------------------ gather queries
    def gather(self, points, streams=None, bounces: int = REFERENCE_BOUNCES, first_sample: int = 1,
               samples: int = 64, return_segments: bool = False):
        """The light each surface point gathers (rt_gather): per point, the sum over ``samples``
        paths that leave the point through the renderer's diffuse lobe -- what a roughness-1,
        non-specular, non-glass surface there would gather in the reference's per_pixel. The
        directions are drawn on the device; the sum is the contract's stripe-and-tree reduction
        (include/rt_abi.h), bit-exact whatever the schedule. Divide by ``samples`` for the mean;
        nothing is clamped. Against the scene as it is now, without touching anything a render
        reads.

        ``points``: an (n, 6) float32 array (position, normal; the normal is used as given), with
        ``streams`` an (n,) uint32 array of RNG streams (default: 1 + the point's position in
        the batch: stream 0 draws the same sample every time), or a ``buffers.GATHER_POINT``
        array. Returns an (n, 4) float32 array, and with ``return_segments`` the call's counted
        ray segments. A CUDA torch tensor of shape (n, 8) float32 (rt_gather_point records: the
        stream's bits in column 3) goes through rt_gather_device instead -- no host round trip,
        stream-ordered on the context's stream -- and returns a CUDA (n, 4) float32 tensor."""
        if not isinstance(points, np.ndarray) and hasattr(points, "is_cuda"):
            if streams is not None:
                raise ValueError("device points carry their stream in column 3")
            return self._device_query("rt_gather_device", points, 8, "points", (4,), "float32",
                                      (int(bounces), int(first_sample), int(samples)), bool(return_segments))
        points = self._pack_records(points, "GATHER_POINT", ("position", "normal"), "points", 1, streams)
        out = np.zeros((points.shape[0], 4), np.float32)
        segments = ctypes.c_uint64(0)
        self._call("rt_gather", N.ptr(points), N.ptr(out), points.shape[0], int(bounces), int(first_sample),
                   int(samples), ctypes.byref(segments))
        return (out, segments.value) if return_segments else out

    # ------------------------------------------------------------------ ambient queries
    def ambient(self, points, streams=None, t_max=np.inf, samples: int = 64, first_sample: int = 1,
                device: bool = False):
        """How open the hemisphere over each surface point is (rt_ambient): per point, ``open``, the
        number of ``samples`` directions through the gather's lobe that nothing blocks before
        ``t_max``, and ``bent``, the sum of those directions. Ambient occlusion is
        ``open / samples``, the bent normal ``bent`` normalised. The directions are drawn on the
        device and each is one any-hit search of ``occluded``; the sums are the contract's
        stripe-and-tree reduction (include/rt_abi.h), bit-exact whatever the schedule. Only
        geometry matters. Against the scene as it is now, without touching anything a render reads.

        ``points``: an (n, 6) float32 array (position, normal; the normal is used as given), with
        ``streams`` an (n,) uint32 array of RNG streams (default: 1 + the point's position in the
        batch) and ``t_max`` a scalar or an (n,) array (+inf: sky visibility), or a
        ``buffers.AMBIENT_POINT`` array. Returns ``(bent, open)``: (n, 3) and (n,) float32 arrays.
        With ``device`` the records are uploaded and answered by rt_ambient_device -- stream-ordered
        on the context's stream -- and CUDA tensors come back; a CUDA torch tensor of shape (n, 8)
        float32 (rt_ambient_point records: the stream's bits in column 3, t_max in column 7)
        always goes that way."""
        if not isinstance(points, np.ndarray) and hasattr(points, "is_cuda"):
            if streams is not None:
                raise ValueError("device points carry their stream in column 3 and t_max in column 7")
            return self._ambient_device(points, first_sample, samples)
        points = self._pack_records(points, "AMBIENT_POINT", ("position", "normal"), "points", 1, streams, t_max)
        if device:
            import torch

            t = torch.from_numpy(points.view(np.float32).reshape(-1, 8).copy()).to(f"cuda:{self.device}")
            return self._ambient_device(t, first_sample, samples)
        out = np.zeros((points.shape[0], 4), np.float32)
        self._call("rt_ambient", N.ptr(points), N.ptr(out), points.shape[0], int(first_sample), int(samples))
        return out[:, :3].copy(), out[:, 3].copy()

    def _ambient_device(self, points, first_sample, samples):
        out = self._device_query("rt_ambient_device", points, 8, "points", (4,), "float32",
                                 (int(first_sample), int(samples)))
        return out[:, :3], out[:, 3]

    # ------------------------------------------------------------------ probe queries
    def probe_sh(self, positions, streams=None, bounces: int = REFERENCE_BOUNCES, first_sample: int = 1,
                 samples: int = 256, return_segments: bool = False):
        """The light arriving at each point in free space, as second-order spherical harmonics
        (rt_probe_sh): per probe and colour channel, the nine sums of L * b_k over ``samples``
        paths that leave the point in uniform directions drawn on the device. The sums are the
        contract's stripe-and-tree reduction (include/rt_abi.h), bit-exact whatever the schedule.
        Multiply by 4 pi / ``samples`` for the radiance coefficients (``sh.radiance`` and
        ``sh.irradiance`` do); nothing is clamped. Against the scene as it is now, without
        touching anything a render reads.

        ``positions``: an (n, 3) float32 array, with ``streams`` an (n,) uint32 array of RNG
        streams (default: 1 + the probe's position in the batch: stream 0 draws the same sample
        every time), or a ``buffers.PROBE`` array. Returns an (n, 9, 4) float32 array, and with
        ``return_segments`` the call's counted ray segments. A CUDA torch tensor of shape (n, 4)
        float32 (rt_probe records: the stream's bits in column 3) goes through
        rt_probe_sh_device instead -- no host round trip, stream-ordered on the context's stream
        -- and returns a CUDA (n, 9, 4) float32 tensor."""
        if not isinstance(positions, np.ndarray) and hasattr(positions, "is_cuda"):
            if streams is not None:
                raise ValueError("device probes carry their stream in column 3")
            return self._device_query("rt_probe_sh_device", positions, 4, "probes", (9, 4), "float32",
                                      (int(bounces), int(first_sample), int(samples)), bool(return_segments))
        probes = self._pack_records(positions, "PROBE", ("position",), "positions", 1, streams)
        out = np.zeros((probes.shape[0], 9, 4), np.float32)
        segments = ctypes.c_uint64(0)
        self._call("rt_probe_sh", N.ptr(probes), N.ptr(out), probes.shape[0], int(bounces), int(first_sample),
                   int(samples), ctypes.byref(segments))
        return (out, segments.value) if return_segments else out

    # ------------------------------------------------------------------ lens queries
    @staticmethod
    def _lens_range(cam, region):
        """(the descriptor as one C-contiguous LENS_CAMERA record, first pixel, count, result shape)
        for ``region``: None (the whole image) or (first_pixel, count)."""
        cam = np.ascontiguousarray(np.asarray(cam, B.LENS_CAMERA).reshape(1))
        w, h = int(cam["width"][0]), int(cam["height"][0])
        if region is None:
            return cam, 0, w * h, (h, w)
        first, count = (int(v) for v in region)
        return cam, first, count, (count,)

    def lens(self, cam, bounces: int = REFERENCE_BOUNCES, first_sample: int = 1, samples: int = 1, region=None,
             device: bool = False, return_segments: bool = False):
        """What a thin-lens, orthographic or equirectangular camera sees (rt_lens): per pixel of the
        descriptor's image, the sum over ``samples`` paths whose first ray is drawn on the device
        from ``cam`` (a ``buffers.LENS_CAMERA`` record; ``camera.lens_camera`` builds one) by the lens
        contract of include/rt_abi.h. Divide by ``samples`` for the mean; nothing is clamped. Against
        the scene as it is now, without touching the framebuffer or anything else a render reads.

        Returns an (h, w, 4) float32 array, or with ``region`` = (first_pixel, count) -- a row-major
        range of pixels, which is how callers tile -- a (count, 4) array; with ``return_segments``
        also the call's counted ray segments. With ``device`` the result stays on the GPU
        (rt_lens_device, stream-ordered on the context's stream) and comes back as a CUDA tensor."""
        cam, first, count, shape = self._lens_range(cam, region)
        scalars = (int(bounces), int(first_sample), int(samples))
        if device:
            return self._lens_device("rt_lens_device", cam, first, count, shape + (4,), scalars, bool(return_segments))
        out = np.zeros(shape + (4,), np.float32)
        segments = ctypes.c_uint64(0)
        self._call("rt_lens", ctypes.c_void_p(cam.ctypes.data), first, count, N.ptr(out), *scalars, ctypes.byref(segments))
        return (out, segments.value) if return_segments else out

    def lens_rays(self, cam, sample_index: int = 1, region=None, device: bool = False):
        """The rays ``lens`` starts the paths of sample ``sample_index`` with (rt_lens_rays): a
        ``buffers.RADIANCE_RAY`` array of shape (h, w), or (count,) with ``region``, which
        ``radiance(rays, first_sample=sample_index, samples=1)`` answers with the bits of
        ``lens(first_sample=sample_index, samples=1)``. With ``device`` a CUDA float32 tensor of
        shape (..., 8) (rt_lens_rays_device), which ``radiance`` takes as it is once flattened."""
        cam, first, count, shape = self._lens_range(cam, region)
        if device:
            return self._lens_device("rt_lens_rays_device", cam, first, count, shape + (8,), (int(sample_index),), None)
        out = np.zeros(shape, B.RADIANCE_RAY)
        self._call("rt_lens_rays", ctypes.c_void_p(cam.ctypes.data), first, count, int(sample_index), N.ptr(out))
        return out

    def _lens_device(self, entry, cam, first, count, shape, scalars, segments):
        """The device form of a lens entry point into a new CUDA float32 tensor of ``shape``.
        ``segments``: None for an entry without a segments argument, else whether to count them."""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev) if segments else None
        args = [ctypes.c_void_p(cam.ctypes.data), first, count]
        result = ctypes.c_void_p(out.data_ptr() if count else None)
        if segments is None:  # rt_lens_rays_device(cam, first, count, sample_index, rays)
            args += [*scalars, result]
        else:
            args += [result, *scalars, ctypes.c_void_p(counter.data_ptr()) if segments else None]
        mine = torch.cuda.ExternalStream(self.stream_handle, device=dev)
        cur = torch.cuda.current_stream(dev)
        mine.wait_stream(cur)  # (the ordering of _device_query)
        self._call(entry, *args)
        cur.wait_stream(mine)
        return (out, int(counter.item())) if segments else out

    # ------------------------------------------------------------------ feature buffers & denoiser
    def compute_features(self) -> None:
        """rt_compute_features: the first-hit feature planes, recomputed only after a camera or
        scene change. Asynchronous."""
        self._call("rt_compute_features")

    def features(self) -> dict:
        """The first-hit feature buffers of the un-jittered camera rays (rt_read_features):
        ``normal`` (H, W, 3) f32, ``depth`` (H, W) f32 (3.4028235e38 on a miss), ``albedo``
        (H, W, 3) f32 (the environment texel on a miss), ``hit`` (H, W) f32, 1 or 0."""
        nd = np.zeros((self.height, self.width, 4), np.float32)
        ah = np.zeros((self.height, self.width, 4), np.float32)
        self._call("rt_read_features", N.ptr(nd), N.ptr(ah))
        return {"normal": np.ascontiguousarray(nd[..., :3]), "depth": np.ascontiguousarray(nd[..., 3]),
                "albedo": np.ascontiguousarray(ah[..., :3]), "hit": np.ascontiguousarray(ah[..., 3])}

    def features_device(self):
        """(normal_depth, albedo_hit) device pointers of the two float4 planes (rt_features_device)."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self._call("rt_features_device", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def feature_ids(self) -> np.ndarray:
        """The ID plane of the feature buffers (rt_read_feature_ids): (H, W, 2) uint32, the ``kind``
        and ``index`` of the record ``trace_rays`` returns for each pixel's un-jittered camera ray;
        (0, 0) on a miss."""
        ids = np.zeros((self.height, self.width, 2), np.uint32)
        self._call("rt_read_feature_ids", N.ptr(ids))
        return ids

    def feature_ids_device(self):
        """The device pointer of the ID plane (rt_feature_ids_device)."""
        a = ctypes.c_void_p()
        self._call("rt_feature_ids_device", ctypes.byref(a))
        return a.value

    def denoise_temporal(self, world_to_pixel, max_history=None, sigma_position=None, normal_min=None,
                         **denoise_kwargs):
        """Temporal reprojection, then the guided a-trous filter (rt_denoise_temporal; the contract
        is in include/rt_abi.h). ``world_to_pixel`` is the current camera's column-major 4x4
        (``Camera.world_to_pixel()``); arguments left None take rt_temporal_default_params and
        ``denoise_kwargs`` are ``denoise``'s. Returns (rgba_f32 (H, W, 4), rgba8 (H, W) uint32)."""
        t, p = self._temporal_params(world_to_pixel, max_history, sigma_position, normal_min, denoise_kwargs,
                                     "denoise_temporal")
        self._call("rt_denoise_temporal", ctypes.byref(t), ctypes.byref(p))
        return self.read_denoised()

    def denoise_temporal_motion(self, world_to_pixel, objects=None, spheres=None, **params):
        """``denoise_temporal`` that follows moving objects and spheres (rt_denoise_temporal_motion;
        the motion contract is in include/rt_abi.h). ``objects`` and ``spheres`` are ``motion.MOTION``
        arrays indexed like ``scene.objects`` and ``scene.spheres`` (``motion.object_motion``,
        ``motion.sphere_motion``); None or a short table leaves the rest static. ``params`` are
        ``denoise_temporal``'s. Returns what ``denoise_temporal`` returns."""
        from .motion import MOTION

        t, p = self._temporal_params(world_to_pixel, params.pop("max_history", None), params.pop("sigma_position", None),
                                     params.pop("normal_min", None), params, "denoise_temporal_motion")
        tables = []
        for table in (objects, spheres):
            a = np.zeros(0, MOTION) if table is None else np.ascontiguousarray(table, MOTION).reshape(-1)
            tables += [N.ptr(a) if a.shape[0] else None, a.shape[0]]
        self._call("rt_denoise_temporal_motion", ctypes.byref(t), ctypes.byref(p), *tables)
        return self.read_denoised()

    def _temporal_params(self, world_to_pixel, max_history, sigma_position, normal_min, denoise_kwargs, who):
        t = N.rt_temporal_params()
        N.check(None, self._lib.rt_temporal_default_params(ctypes.byref(t)), self._lib)
        t.world_to_pixel[:] = [float(v) for v in np.asarray(world_to_pixel, np.float32).reshape(16)]
        for key, value in (("max_history", max_history), ("sigma_position", sigma_position),
                           ("normal_min", normal_min)):
            if value is not None:
                setattr(t, key, value)
        p = N.rt_denoise_params()
        N.check(None, self._lib.rt_denoise_default_params(ctypes.byref(p)), self._lib)
        for key, value in denoise_kwargs.items():
            if key not in ("iterations", "sigma_color", "sigma_albedo", "sigma_depth"):
                raise TypeError(f"{who}() got an unexpected keyword argument {key!r}")
            if value is not None:
                setattr(p, key, value)
        return t, p

    def temporal_reset(self) -> None:
        """Drop all reprojection history (rt_temporal_reset): after texture or lighting edits, and
        after a material edit not marked ``motion.DROP``, which reprojection cannot validate.
        Object and sphere motion need none with ``denoise_temporal_motion``."""
        self._call("rt_temporal_reset")

    def read_temporal(self):
        """(rgba_f32 (H, W, 4) pre-filter blend, history (H, W) float32 per-pixel sample count) of
        the last ``denoise_temporal`` (rt_read_temporal)."""
        f = np.zeros((self.height, self.width, 4), np.float32)
        n = np.zeros((self.height, self.width), np.float32)
        self._call("rt_read_temporal", N.ptr(f), N.ptr(n))
        return f, n

    def denoise(self, iterations=None, sigma_color=None, sigma_albedo=None, sigma_depth=None):
        """The guided a-trous filter over the accumulated frame (rt_denoise; the contract is in
        include/rt_abi.h): an observation point that changes nothing a render reads. Arguments left
        None take rt_denoise_default_params. Returns (rgba_f32 (H, W, 4), rgba8 (H, W) uint32)."""
        p = N.rt_denoise_params()
        N.check(None, self._lib.rt_denoise_default_params(ctypes.byref(p)), self._lib)
        if iterations is not None:
            p.iterations = int(iterations)
        if sigma_color is not None:
            p.sigma_color = float(sigma_color)
        if sigma_albedo is not None:
            p.sigma_albedo = float(sigma_albedo)
        if sigma_depth is not None:
            p.sigma_depth = float(sigma_depth)
        self._call("rt_denoise", ctypes.byref(p))
        return self.read_denoised()

    def read_denoised(self):
        """(rgba_f32 (H, W, 4), rgba8 (H, W) uint32) of the last ``denoise`` (rt_read_denoised)."""
        f = np.zeros((self.height, self.width, 4), np.float32)
        u = np.zeros((self.height, self.width), np.uint32)
        self._call("rt_read_denoised", N.ptr(u), N.ptr(f))
        return f, u

    def denoised_image(self) -> np.ndarray:
        """The last ``denoise`` as an (H, W, 4) RGBA8 array (R first), like ``image()``."""
        u = np.zeros((self.height, self.width), np.uint32)
        self._call("rt_read_denoised", N.ptr(u), None)
        return np.ascontiguousarray(u.view(np.uint8).reshape(self.height, self.width, 4))

    def copy_denoised_to_device(self, dst_device_ptr: int, bytes_per_row: int) -> None:
        """``copy_output_to_device`` for the packed denoised output (rt_copy_denoised_to_device)."""
        self._call("rt_copy_denoised_to_device", ctypes.c_void_p(dst_device_ptr), bytes_per_row)

    # ------------------------------------------------------------------ display transform
    _DISPLAY_SOURCES = {"accumulation": N.RT_DISPLAY_ACCUMULATION, "denoised": N.RT_DISPLAY_DENOISED}
    _DISPLAY_ENUMS = {"tone_operator": {"linear": N.RT_TONE_LINEAR, "reinhard": N.RT_TONE_REINHARD,
                                        "aces": N.RT_TONE_ACES},
                      "encode": {"none": N.RT_ENCODE_NONE, "srgb": N.RT_ENCODE_SRGB}}

    def display(self, source="accumulation", **params):
        """Radiance to display codes on the device (rt_display; the contract is in include/rt_abi.h):
        metered auto-exposure, a tone curve and the encode. ``source``: "accumulation" (an observation
        point: queued frames launch first), "denoised" (what the last ``denoise`` /
        ``denoise_temporal`` left) or a CUDA float32 torch tensor of height*width*4 values, whose
        producers on the current torch stream are ordered before the call (through ``stream_handle``,
        which launches queued frames; the C call with a plane leaves them queued). ``params`` are the fields
        of rt_display_params (``tone_operator`` and ``encode`` also by name: "linear", "reinhard",
        "aces"; "none", "srgb"); those left out take rt_display_default_params. Returns the packed
        image, (H, W) uint32."""
        p = N.rt_display_params()
        N.check(None, self._lib.rt_display_default_params(ctypes.byref(p)), self._lib)
        fields = {name for name, _ in N.rt_display_params._fields_} - {"source"}
        for key, value in params.items():
            if key not in fields:
                raise TypeError(f"display() got an unexpected keyword argument {key!r}")
            if isinstance(value, str):
                value = self._DISPLAY_ENUMS[key][value]
            setattr(p, key, value)
        if isinstance(source, str):
            if source not in self._DISPLAY_SOURCES:
                raise ValueError('source must be "accumulation", "denoised" or a CUDA tensor')
            p.source = self._DISPLAY_SOURCES[source]
            self._call("rt_display", ctypes.byref(p), None)
        else:
            self._display_plane(source, p)
        return self.read_display()

    def _display_plane(self, plane, p):
        import torch

        if (not getattr(plane, "is_cuda", False) or plane.dtype != torch.float32
                or plane.numel() != self.height * self.width * 4):
            raise ValueError("a display plane must be a CUDA float32 tensor of height*width*4 values")
        if plane.device.index != self.device:
            raise ValueError("a display plane must live on the renderer's device")
        plane = plane.contiguous()
        p.source = N.RT_DISPLAY_PLANE
        # the transform runs on the context's stream: order it after the tensor's producers, and the
        # caller's stream after it (as _device_query does)
        mine = torch.cuda.ExternalStream(self.stream_handle, device=plane.device)
        cur = torch.cuda.current_stream(plane.device)
        mine.wait_stream(cur)
        self._call("rt_display", ctypes.byref(p), ctypes.c_void_p(plane.data_ptr()))
        cur.wait_stream(mine)

    def read_display(self) -> np.ndarray:
        """The packed image of the last ``display`` (rt_read_display), (H, W) uint32."""
        u = np.zeros((self.height, self.width), np.uint32)
        self._call("rt_read_display", N.ptr(u))
        return u

    def display_image(self) -> np.ndarray:
        """The last ``display`` as an (H, W, 4) RGBA8 array (R first), like ``image()``."""
        return np.ascontiguousarray(self.read_display().view(np.uint8).reshape(self.height, self.width, 4))

    def display_state(self):
        """(exposure, histogram (256,) uint32, metered) of the last auto-exposure ``display``
        (rt_display_state); the exposure is 0.0 while there is no adapted exposure."""
        e, m = ctypes.c_float(), ctypes.c_uint64()
        hist = np.zeros(256, np.uint32)
        self._call("rt_display_state", ctypes.byref(e), N.ptr(hist), ctypes.byref(m))
        return np.float32(e.value), hist, m.value

    def display_reset(self) -> None:
        """Drop the adapted exposure (rt_display_reset): the next auto-exposure call jumps to its target."""
        self._call("rt_display_reset")

    def copy_display_to_device(self, dst_device_ptr: int, bytes_per_row: int) -> None:
        """``copy_output_to_device`` for the display plane (rt_copy_display_to_device)."""
        self._call("rt_copy_display_to_device", ctypes.c_void_p(dst_device_ptr), bytes_per_row)

    def update_texture(self, alignment: int = 256) -> np.ndarray:
        """``Renderer::update_texture`` (src/renderer.rs:254-283), headless: the
        packed output as the Rgba8Unorm display texture the reference copies it
        into, one row every ``calculate_bytes_per_row`` bytes (:285-295). Returns
        the (height, bytes_per_row) u8 staging image; ``image()`` strips the pitch."""
        bpr = int(self._lib.rt_bytes_per_row(self.width, alignment))
        if bpr == 0:
            raise ValueError(f"alignment {alignment} must be a power of two")
        out = np.zeros((self.height, bpr), np.uint8)
        self._call("rt_read_output_pitched", N.ptr(out), bpr)
        return out

    def copy_output_to_device(self, dst_device_ptr: int, bytes_per_row: int) -> None:
        """``Renderer::update_texture`` on the device (src/renderer.rs:254-283): the packed
        output copied into device memory at ``dst_device_ptr`` with a row pitch, stream-ordered
        and asynchronous (rt_copy_output_to_device) -- a display loop's observation point."""
        self._call("rt_copy_output_to_device", ctypes.c_void_p(dst_device_ptr), bytes_per_row)

    def image(self) -> np.ndarray:
        """The displayed frame as an (height, width, 4) RGBA8 array (R first)."""
        return np.ascontiguousarray(self.update_texture()[:, : 4 * self.width].reshape(self.height, self.width, 4))

    def ray_count(self) -> int:
        v = ctypes.c_uint64()
        self._call("rt_ray_count", ctypes.byref(v))
        return v.value

    def reset_ray_count(self) -> None:
        self._call("rt_reset_ray_count")

    @property
    def accumulation_index(self) -> int:
        v = ctypes.c_uint32()
        self._call("rt_accumulation_index", ctypes.byref(v))
        return v.value

    def set_timing(self, enable: bool) -> None:
        self._call("rt_set_timing", int(enable))

    def dispatch_time_total(self):
        """(total milliseconds of timed path-kernel launches, number timed): each launch's
        span on the device clock (rt_set_timing)."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._call("rt_dispatch_time_total", ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    def set_brute_force(self, enable) -> None:
        """rt_set_brute_force: the reference's own sphere and triangle sweeps (BASELINE config
        5's stress mode) instead of the acceleration structures: True / 1 with the sub-object
        records LDS-tiled, 2 streamed through the scalar cache, False / 0 off."""
        self._call("rt_set_brute_force", int(enable))

    def set_triangle_pruning(self, mode: int) -> None:
        """rt_set_triangle_pruning: distance pruning of the triangle walk.
        1 (default): per-leaf certificates (each triangle's own normal and a derived f32 error
        bound), exact by construction; 0: box culling only (exact); 2: the round-3 relative slack (faster
        on incoherent meshes, not exact)."""
        self._call("rt_set_triangle_pruning", int(mode))

    def set_tuning(self, key: str, value: int) -> None:
        """An exact variant of the schedule or of an acceleration structure (rt_set_tuning)."""
        self._call("rt_set_tuning", key.encode(), int(value))

    def streamed_bytes_l2(self) -> int:
        """Sub-object bytes the brute-force sweeps read from L2 (rt_streamed_bytes_l2)."""
        v = ctypes.c_uint64()
        self._call("rt_streamed_bytes_l2", ctypes.byref(v))
        return v.value

    def streamed_bytes(self) -> int:
        """The brute-force launches' tile-streaming bytes by SURVEY §8d's convention
        (32 B x the swept sub-objects per started 256 rays of a bounce level)."""
        v = ctypes.c_uint64()
        self._call("rt_streamed_bytes", ctypes.byref(v))
        return v.value

    def resolve_time_total(self):
        """(total milliseconds, number) of the timed batches' resolve passes
        (rt_resolve_frames_kernel), which dispatch_time_total does not include."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._call("rt_resolve_time_total", ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    def reset_timing(self) -> None:
        self._call("rt_reset_timing")

    def owned_pixel_count(self, rank: int | None = None, world_size: int | None = None) -> int:
        v = ctypes.c_uint64()
        r = self.rank if rank is None else rank
        w = self.world_size if world_size is None else world_size
        N.check(self._ctx, self._lib.rt_owned_pixel_count(self._ctx, r, w, ctypes.byref(v)), self._lib)
        return v.value

    def pack_owned_accumulation(self, dst_device_ptr: int) -> None:
        self._call("rt_pack_owned_accumulation", ctypes.c_void_p(dst_device_ptr))

    def unpack_accumulation(self, src_device_ptr: int, src_rank: int, world_size: int, divisor: int) -> None:
        self._call("rt_unpack_accumulation", ctypes.c_void_p(src_device_ptr), src_rank, world_size, divisor)

    def pack_owned_output(self, dst_device_ptr: int) -> None:
        self._call("rt_pack_owned_output", ctypes.c_void_p(dst_device_ptr))

    def unpack_output(self, src_device_ptr: int, src_rank: int, world_size: int) -> None:
        self._call("rt_unpack_output", ctypes.c_void_p(src_device_ptr), src_rank, world_size)

    def unpack_accumulation_ranks(self, src_device_ptr: int, stride_px: int, world_size: int, skip_rank: int,
                                  divisor: int) -> None:
        """Every rank's block of a gather (block r at r * stride_px pixels) but skip_rank's, one launch."""
        self._call("rt_unpack_accumulation_ranks", ctypes.c_void_p(src_device_ptr), stride_px, world_size, skip_rank,
                   divisor)

    def unpack_output_ranks(self, src_device_ptr: int, stride_px: int, world_size: int, skip_rank: int) -> None:
        self._call("rt_unpack_output_ranks", ctypes.c_void_p(src_device_ptr), stride_px, world_size, skip_rank)

    def debug_counters(self, n: int = 8) -> list:
        """Diagnostic builds only: the 8 counters, then per-wave stamps (include/rt_abi.h)."""
        v = (ctypes.c_uint64 * n)()
        N.check(self._ctx, self._lib.rt_debug_counters(self._ctx, v, n), self._lib)
        return list(v)

    def check_leaf_certificates(self) -> tuple:
        """(mismatches, valid, total): the device's leaf certificates re-derived on the host from
        the device's own leaf records, sub-objects and triangles (include/rt_abi.h)."""
        m, v, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        N.check(self._ctx, self._lib.rt_debug_check_leaf_certificates(self._ctx, m, v, t), self._lib)
        return m.value, v.value, t.value

    def set_tile_schedule(self, schedule: int) -> None:
        """0: claim tiles in index order; 1: cost-ordered (most rays of an earlier launch first)."""
        self._call("rt_set_tile_schedule", schedule)

    def tile_schedule_state(self):
        """(order, costs): the next launch's claim order over this rank's tiles and the rays recorded per tile."""
        n = self.owned_pixel_count() // 64
        order = np.zeros(n, np.uint32)
        costs = np.zeros(n, np.uint32)
        self._call("rt_tile_schedule_state", order.ctypes.data_as(ctypes.c_void_p),
                   costs.ctypes.data_as(ctypes.c_void_p))
        return order, costs

    def launch_config(self) -> dict:
        """Geometry of the last launch: workgroup threads, workgroups, LDS bytes, scene staged in LDS."""
        v = [ctypes.c_uint32() for _ in range(4)]
        N.check(self._ctx, self._lib.rt_launch_config(self._ctx, *[ctypes.byref(x) for x in v]), self._lib)
        return dict(zip(("threads", "blocks", "lds_bytes", "scene_in_lds"), (x.value for x in v)))

    def last_launch_pass_mask(self) -> int:
        """The raw RT_PASS_* mask of the last launch (include/rt_abi.h): what last_launch_passes()
        names, plus RT_PASS_PATH_FRAME_PAR when the path kernel ran as its frame-parallel instance."""
        v = ctypes.c_uint32()
        N.check(self._ctx, self._lib.rt_last_launch_passes(self._ctx, ctypes.byref(v)), self._lib)
        return v.value

    def last_launch_passes(self) -> list:
        """Kernels the last launch ran: "path", "primary" (pre-pass), "resolve", "brute",
        "brute_stream" (the brute-force sweep's scalar-cache variant)."""
        v = ctypes.c_uint32(self.last_launch_pass_mask())
        names = ((N.RT_PASS_PATH, "path"), (N.RT_PASS_PRIMARY, "primary"), (N.RT_PASS_RESOLVE, "resolve"),
                 (N.RT_PASS_BRUTE, "brute"), (N.RT_PASS_BRUTE_STREAM, "brute_stream"))
        return [n for bit, n in names if v.value & bit]

    @property
    def stream_handle(self) -> int:
        return self._lib.rt_stream(self._ctx) or 0

    def close(self) -> None:
        if self._ctx is not None:
            self._lib.rt_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
