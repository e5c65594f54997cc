"""Throughput of the ray-query kernel (rt_trace_rays_device) and its placement crossover.

usage: python tools/query_bench.py [--config c2_rtiow] [--width 1920 --height 1080]
                                   [--reps 20] [--sweep] [--occluded] [--hits] [--nearest] [--radiance] [--gather] [--probe] [--ambient]
                                   [--lens]
                                   [--out profiles/query_bench.jsonl]

Rays: the configuration's width x height camera rays (coherent: neighbouring rays are
neighbouring pixels), and the same rays in a fixed random permutation (incoherent). They live in
device memory; each timing is a host clock around `reps` stream-ordered rt_trace_rays_device
calls ending in a device synchronise, after a warm-up of every (ray set, placement) it times.

Default: Mray/s of both ray sets with the automatic placement, next to the render's own rate for
the same configuration measured the same way in this process (frames through rt_compute_frame,
rays from rt_ray_count): the yardstick a query is held against.
--sweep: time per call of the first n camera rays, n from 64 to the whole set, with the mode-0
instance (scene read from global memory) and with the staged placement the scene takes
(tuning "query_lds_mode" 0 against 2): where they cross is the kQueryStageMinRays threshold.
Every mode returns the same bits; the sweep checks that on each n.
--occluded: the occlusion kernel (rt_occluded_device) against the closest-hit call on the same
rays in the same process. Series, each on the coherent and the permuted camera
rays: (a) rt_trace_rays_device, the yardstick; (b) rt_occluded_device with t_max = +inf (the early
exit); (c) with each ray's own closest-hit t (every byte 0: a full search pruned from the first
node); (d) shadow rays from each hit point, offset 1e-4 along the normal, toward one fixed
direction, t_max = +inf. Device events around `reps` launches on the context's stream; the series
alternate over --rounds rounds; median, minimum and maximum Mray/s per series. With --sweep: the
placement crossover of the occlusion kernel, as the default sweep measures the closest-hit one's.
--hits: the hit-list kernel (rt_trace_hits_device) against the closest-hit call on the same rays in
the same process: the camera rays with t_max = +inf at max_hits 1, 4 and 16, next
to rt_trace_rays_device, the yardstick. Entry 0 of every list is checked against the closest-hit
record. Device events around `reps` launches on the context's stream; the series alternate over
--rounds rounds; median, minimum and maximum Mray/s per series, and the mean count per ray.
--nearest: the proximity kernel (rt_nearest_device) beside the closest-hit call in
the same process: one point per camera ray, off the ray's first hit by 2^-10 .. 1 along the normal
(rays that miss: a point 10 along the ray), max_distance = +inf; the accelerated walk on all of
them, the sweep instance (tuning "nearest_walk" 0) on the first --sweep-points of them and the walk
without its greedy descent ("nearest_walk" 2) on all of them, whose records are checked against
the walk's. Device events around `reps` launches (a tenth of them for
the sweep); the series alternate over --rounds rounds; median, minimum and maximum Mitems/s.
--radiance: the radiance kernel (rt_radiance_device) against the frame it reproduces, in one process
(DESIGN.md §5.4e). The frame's own rays -- camera origin, each pixel's direction, stream = pixel
index, samples = 1 -- are submitted as one batch; the yardstick is the same context rendering one
frame per launch (frame batch 1), timed on the device clock with rt_set_timing. A round renders
`reps` frames, then queries the same samples (first_sample = each frame's accumulation index), so
both sides trace the same segments (checked: the batch's segments equal rt_ray_count, and the
first query equals the first frame's accumulation bit for bit); Mray/s from the segments over
device events, and from rt_ray_count over the launch spans. The closest-hit query of the same rays
is timed next to them. Median, minimum and maximum over --rounds rounds after --settle-ms of
untimed work.
--gather: the gather query (rt_gather_device) against the same paths done by hand, in one process
(DESIGN.md §5.4g). --points points (4,096) are taken from the first hits of the camera rays,
streams 1..n, at --samples samples (1,024). The yardstick is what a caller without rt_gather does:
the contract's records generated once on the host (tools/gather_records.c, compiled here against
the CPU oracle's library) and traced by one rt_radiance_device call with samples = 1 and
first_sample = 1 (each record's stream is stream * u, which gives the contract's seed): that code
is the parent's. The records are laid out sample-major (neighbouring records are neighbouring
points) and point-major (a point's samples are consecutive), each its own series. Each round
checks that all trace equal segments and that the contract's tree over the by-hand results equals
the gather bit for bit. Next to them: rt_radiance_device on the points' first records at samples
= --samples, the shape the gather call replaces (one direction per point, its samples back to
back on one lane). Device events on the context's stream; median, minimum and maximum over --rounds.
--probe: the probe query (rt_probe_sh_device) against the same paths done by hand, in one process
(DESIGN.md §5.4i). --points probes (4,096) are the first hits of the camera rays moved 0.25 along the
normal, streams 1..n, at --samples samples (1,024). The yardstick is the parent's code, as for
--gather: the records of the same paths made on the host (tools/gather_records.c with zero normals,
folded streams) and traced by one rt_radiance_device call with samples = 1 and first_sample = 1, in
both record orders. Each round checks that all trace equal segments and that steps 4 and 5 of the
probe contract over the by-hand results (torch's f32 multiply and add, one operation each) equal
the probe call bit for bit.
--ambient: the ambient query (rt_ambient_device) against the two ways to get its answer without
it, in one process per configuration of --ambient-configs (c2_rtiow and c3_chess), after a warm-up
of each. --points points (here 65,536 by default) are taken from the first hits of
the camera rays, streams 1..n, at --samples samples (here 256), all with the bound --t-max. Series:
(a) rt_ambient_device; (b) rt_gather_device at bounces = 1 on the same points (the path tracer per
sample); (c) rt_occluded_device fed the contract's n x samples records (o, dir, t_max), made once on
the host (tools/gather_records.c) and already resident in device memory: the walk-only floor, which
leaves out the transfer of 32 B per sample that a caller would pay. Each round checks that the
open counts of (a) equal samples minus the sums of (c)'s bytes, and that the contract's tree over
(c)'s terms equals (a) bit for bit. Device events on the context's stream; median, minimum and
maximum over --rounds.
--lens: the lens query (rt_lens_device) against the radiance query of the same rays, in one process
(DESIGN.md §5.4l). The pinhole descriptor of the configuration's camera (stream_base 0: the frame's
own samples) at samples = 1, next to rt_radiance_device on the host-built records of the same rays
(camera origin, each pixel's direction, stream = pixel index), which is the parent's code; and a thin
lens (aperture 0.3, focused at 10) next to rt_lens_rays_device followed by rt_radiance_device on its
records. A round runs `reps` calls of each series with first_sample = 1 .. reps; each pair is checked
to return the same bits and the same segments. Device events on the context's stream; median, minimum
and maximum milliseconds per call over --rounds rounds after --settle-ms of untimed work.
Prints one JSON line per measurement (and appends them to --out).
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from rust_gpu_raytracing_amd import Renderer  # noqa: E402
from rust_gpu_raytracing_amd import buffers as B  # noqa: E402
from rust_gpu_raytracing_amd.scene import build_config  # noqa: E402


def camera_query_rays(scene):
    d = scene.camera.recalculate_ray_directions()["direction"]
    q = np.zeros(d.shape[0], B.QUERY_RAY)
    q["origin"] = np.asarray(scene.camera.position, np.float32)
    q["direction"] = d
    return q


def time_queries(r, rays_t, hits_t, n, reps, call="rt_trace_rays_device"):
    """Seconds per `call` over the first n rays (device tensors)."""
    args = (ctypes.c_void_p(rays_t.data_ptr()), ctypes.c_void_p(hits_t.data_ptr()), n)
    r._call(call, *args)  # warm-up of this shape and placement
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r._call(call, *args)
    r.synchronize()
    return (time.perf_counter() - t0) / reps


SHADOW_DIRECTION = (0.35, -0.85, 0.4)  # towards the sky (y points down), off every axis


def occlusion_bench(r, args, q, dev, emit):
    """The --occluded series (module docstring)."""
    import torch

    n = q.shape[0]
    perm = np.random.default_rng(2024).permutation(n)
    hits_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    occ_t = torch.empty((n,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)

    def upload(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1, 8)).to(dev)
        torch.cuda.synchronize()  # uploaded on torch's stream, read on the context's
        return t

    def launch(call, rays_t, out_t):
        r._call(call, ctypes.c_void_p(rays_t.data_ptr()), ctypes.c_void_p(out_t.data_ptr()), rays_t.shape[0])

    base = upload(q)
    launch("rt_trace_rays_device", base, hits_t)
    r.synchronize()
    h = hits_t.cpu().numpy().view(B.HIT).reshape(-1)
    hit = h["kind"] != B.HIT_MISS
    series = {}  # name -> (call, rays tensor, output tensor, expected count of ones)
    for order, idx in (("coherent", np.arange(n)), ("permuted", perm)):
        rays = q[idx]
        any_hit, own_t = rays.view(B.OCCLUSION_RAY).copy(), rays.view(B.OCCLUSION_RAY).copy()
        any_hit["t_max"] = np.inf
        own_t["t_max"] = h["t"][idx]
        from_hit = idx[hit[idx]]
        shadow = np.zeros(from_hit.shape[0], B.OCCLUSION_RAY)
        shadow["origin"] = h["position"][from_hit] + np.float32(1e-4) * h["normal"][from_hit]
        shadow["direction"] = np.asarray(SHADOW_DIRECTION, np.float32)
        shadow["t_max"] = np.inf
        series["a_closest_hit/" + order] = ("rt_trace_rays_device", upload(rays), hits_t, None)
        series["b_any_hit_inf/" + order] = ("rt_occluded_device", upload(any_hit), occ_t, int(hit.sum()))
        series["c_own_t/" + order] = ("rt_occluded_device", upload(own_t), occ_t, 0)
        if shadow.shape[0]:
            series["d_shadow/" + order] = ("rt_occluded_device", upload(shadow), occ_t, None)
    rates = {k: [] for k in series}
    fraction = {}
    for k, (call, rays_t, out_t, want) in series.items():  # warm-up and a check of what is timed
        launch(call, rays_t, out_t)
        r.synchronize()
        if call == "rt_occluded_device":
            ones = int(out_t[:rays_t.shape[0]].sum(dtype=torch.int64).item())
            fraction[k] = ones / rays_t.shape[0]
            assert want is None or ones == want, (k, ones, want)
    for _ in range(args.rounds):
        for k, (call, rays_t, out_t, _) in series.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                launch(call, rays_t, out_t)
            t1.record(stream)
            t1.synchronize()
            rates[k].append(rays_t.shape[0] * args.reps / (t0.elapsed_time(t1) * 1e-3) / 1e6)
    for k, v in rates.items():
        name, order = k.split("/")
        emit(kind="occlusion", series=name, rays_set=order, rays=int(series[k][1].shape[0]), rounds=args.rounds,
             reps=args.reps, mray_s=round(float(np.median(v)), 1), mray_s_min=round(min(v), 1),
             mray_s_max=round(max(v), 1), occluded_fraction=None if k not in fraction else round(fraction[k], 4),
             hit_fraction=round(float(hit.mean()), 4), build=r._lib.rt_build_hash().decode())


def hits_bench(r, args, q, dev, emit):
    """The --hits series (module docstring)."""
    import torch

    n = q.shape[0]
    rays = q.view(B.OCCLUSION_RAY).copy()
    rays["t_max"] = np.inf
    rays_t = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to(dev)
    closest_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    counts_t = torch.empty((n,), dtype=torch.int32, device=dev)
    lists_t = {k: torch.empty((n, k, 16), dtype=torch.int32, device=dev) for k in (1, 4, 16)}
    torch.cuda.synchronize()  # uploaded on torch's stream, read on the context's
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
    P = ctypes.c_void_p

    def launch(k):
        if k == 0:
            r._call("rt_trace_rays_device", P(rays_t.data_ptr()), P(closest_t.data_ptr()), n)
        else:
            r._call("rt_trace_hits_device", P(rays_t.data_ptr()), P(lists_t[k].data_ptr()), P(counts_t.data_ptr()), n, k)

    series = {"a_closest_hit": 0, "b_hits_1": 1, "c_hits_4": 4, "d_hits_16": 16}
    mean_count = {}
    for name, k in series.items():  # warm-up and a check of what is timed
        launch(k)
        r.synchronize()
        if k:
            mean_count[name] = float(counts_t.sum(dtype=torch.int64).item()) / n
            assert torch.equal(lists_t[k][:, 0], closest_t), name  # consequence 1 of the contract
    rates = {name: [] for name in series}
    for _ in range(args.rounds):
        for name, k in series.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                launch(k)
            t1.record(stream)
            t1.synchronize()
            rates[name].append(n * args.reps / (t0.elapsed_time(t1) * 1e-3) / 1e6)
    for name, v in rates.items():
        emit(kind="hits", series=name, max_hits=series[name] or None, rays=n, rounds=args.rounds, reps=args.reps,
             mray_s=round(float(np.median(v)), 1), mray_s_min=round(min(v), 1), mray_s_max=round(max(v), 1),
             ms=round(n / float(np.median(v)) / 1e3, 4),
             mean_count=None if name not in mean_count else round(mean_count[name], 3), build=r._lib.rt_build_hash().decode())


def nearest_bench(r, args, q, dev, emit):
    """The --nearest series (module docstring)."""
    import torch

    n = q.shape[0]
    P = ctypes.c_void_p
    rays_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    closest_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # uploaded on torch's stream, read on the context's
    r._call("rt_trace_rays_device", P(rays_t.data_ptr()), P(closest_t.data_ptr()), n)
    r.synchronize()
    h = closest_t.cpu().numpy().view(B.HIT).reshape(-1)
    hit = h["kind"] != B.HIT_MISS
    rng = np.random.default_rng(2024)
    pts = np.zeros(n, B.NEAR_POINT)
    # off the first hits by 2^-10 .. 1 along the normal; rays that miss: a point 10 along the ray
    off = np.exp2(rng.uniform(-10, 0, n)).astype(np.float32)
    pts["position"] = np.where(hit[:, None], h["position"] + off[:, None] * h["normal"],
                               q["origin"] + np.float32(10) * q["direction"])
    pts["max_distance"] = np.inf
    m = min(n, args.sweep_points)
    pts_t = torch.from_numpy(pts.view(np.float32).reshape(-1, 4)).to(dev)
    out_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    few_t = torch.empty((m, 16), dtype=torch.int32, device=dev)
    plain_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)

    def launch(name):
        if name == "a_closest_hit":
            r._call("rt_trace_rays_device", P(rays_t.data_ptr()), P(closest_t.data_ptr()), n)
        elif name == "b_nearest_walk":
            r._call("rt_nearest_device", P(pts_t.data_ptr()), P(out_t.data_ptr()), n)
        elif name == "d_nearest_plain_walk":  # the skip walk without the greedy descent before it
            r.set_tuning("nearest_walk", 2)
            r._call("rt_nearest_device", P(pts_t.data_ptr()), P(plain_t.data_ptr()), n)
            r.set_tuning("nearest_walk", 1)
        else:  # the sweep instance, on the first m points (every candidate per point)
            r.set_tuning("nearest_walk", 0)
            r._call("rt_nearest_device", P(pts_t.data_ptr()), P(few_t.data_ptr()), m)
            r.set_tuning("nearest_walk", 1)

    series = {"a_closest_hit": n, "b_nearest_walk": n, "c_nearest_sweep": m, "d_nearest_plain_walk": n}
    for name in series:  # warm-up and a check of what is timed
        launch(name)
    r.synchronize()
    assert torch.equal(out_t[:m], few_t), "the walk and the sweep disagree"
    assert torch.equal(out_t, plain_t), "the walks with and without the descent disagree"
    found = float((out_t[:, 8] != 0).float().mean().item())
    rates = {name: [] for name in series}
    for _ in range(args.rounds):
        for name, count in series.items():
            reps = args.reps if name != "c_nearest_sweep" else max(1, args.reps // 10)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(reps):
                launch(name)
            t1.record(stream)
            t1.synchronize()
            rates[name].append(count * reps / (t0.elapsed_time(t1) * 1e-3) / 1e6)
    for name, v in rates.items():
        emit(kind="nearest", series=name, items=series[name], rounds=args.rounds, reps=args.reps,
             mitems_s=round(float(np.median(v)), 4), mitems_s_min=round(min(v), 4), mitems_s_max=round(max(v), 4),
             ms=round(series[name] / float(np.median(v)) / 1e3, 4), found_fraction=round(found, 4),
             build=r._lib.rt_build_hash().decode())


def radiance_bench(r, args, scene, bounces, dev, emit):
    """The --radiance series (module docstring)."""
    import statistics

    import torch

    d = scene.camera.recalculate_ray_directions()["direction"]
    n = d.shape[0]
    q = np.zeros(n, B.RADIANCE_RAY)
    q["origin"] = np.asarray(scene.camera.position, np.float32)
    q["direction"] = d
    q["stream"] = np.arange(n, dtype=np.uint32)
    rays_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    out_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
    hits_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    seg_t = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # uploaded on torch's stream, read on the context's
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)

    def radiance(first_sample):
        r._call("rt_radiance_device", ctypes.c_void_p(rays_t.data_ptr()), ctypes.c_void_p(out_t.data_ptr()), n, bounces,
                first_sample, 1, ctypes.c_void_p(seg_t.data_ptr()))

    def closest_hit():
        r._call("rt_trace_rays_device", ctypes.c_void_p(rays_t.data_ptr()), ctypes.c_void_p(hits_t.data_ptr()), n)

    r.set_frame_batch(1)  # the yardstick: one frame per launch
    # what is timed is the same computation: the first frame's accumulation, bit for bit
    r.reset_accumulation()
    r.compute_frame(bounces)
    acc = r.read_accumulation().reshape(n, 4)
    frame_rays = r.ray_count()
    radiance(1)
    r.synchronize()
    same = bool(np.array_equal(out_t.cpu().numpy().view(np.uint32), acc.view(np.uint32)))
    assert same and int(seg_t.item()) == frame_rays, (same, int(seg_t.item()), frame_rays)
    closest_hit()
    t_settle = time.perf_counter()  # untimed work until the clocks settle
    while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
        r.compute_frame(bounces)
        radiance(1)
        r.synchronize()
    frame_ms, rad_ms, hit_ms, frame_rate, rad_rate = [], [], [], [], []
    for _ in range(args.rounds):
        # frames k0 .. k0+reps-1, then the radiance queries of the same samples: the same segments
        k0 = r.accumulation_index
        r.reset_timing()
        r.reset_ray_count()
        r.set_timing(True)
        for _ in range(args.reps):
            r.compute_frame(bounces)
        r.synchronize()
        r.set_timing(False)
        ms, _ = r.dispatch_time_total()
        rays = r.ray_count()
        seg_t.zero_()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for i in range(args.reps):
            radiance(k0 + i)
        t1.record(stream)
        t1.synchronize()
        segments = int(seg_t.item())
        assert segments == rays, (segments, rays)
        h0, h1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0.record(stream)
        for _ in range(args.reps):
            closest_hit()
        h1.record(stream)
        h1.synchronize()
        frame_ms.append(ms / args.reps)
        rad_ms.append(t0.elapsed_time(t1) / args.reps)
        hit_ms.append(h0.elapsed_time(h1) / args.reps)
        frame_rate.append(rays / ms / 1e3)
        rad_rate.append(segments / t0.elapsed_time(t1) / 1e3)
    med = statistics.median
    emit(kind="radiance", bounces=bounces, rays=n, rounds=args.rounds, reps=args.reps,
         segments_per_ray=round(rays / args.reps / n, 4), bit_identical_to_frame=same,
         frame_ms=round(med(frame_ms), 4), frame_ms_min=round(min(frame_ms), 4), frame_ms_max=round(max(frame_ms), 4),
         radiance_ms=round(med(rad_ms), 4), radiance_ms_min=round(min(rad_ms), 4), radiance_ms_max=round(max(rad_ms), 4),
         frame_mray_s=round(med(frame_rate), 1), radiance_mray_s=round(med(rad_rate), 1),
         ratio=round(med(rad_rate) / med(frame_rate), 3),
         closest_hit_ms=round(med(hit_ms), 4), closest_hit_mray_s=round(n / med(hit_ms) / 1e3, 1),
         closest_hit_ratio=round(n / med(hit_ms) / 1e3 / med(frame_rate), 3), build=r._lib.rt_build_hash().decode())


def lens_bench(r, args, scene, bounces, dev, emit):
    """The --lens series (module docstring)."""
    import statistics

    import torch

    from rust_gpu_raytracing_amd.camera import lens_camera

    d = scene.camera.recalculate_ray_directions()["direction"]
    n = d.shape[0]
    q = np.zeros(n, B.RADIANCE_RAY)
    q["origin"] = np.asarray(scene.camera.position, np.float32)
    q["direction"] = d
    q["stream"] = np.arange(n, dtype=np.uint32)
    records_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    drawn_t = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out_t = {k: torch.empty((n, 4), dtype=torch.float32, device=dev) for k in ("lens", "records")}
    seg_t = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in ("lens", "records")}
    torch.cuda.synchronize()  # uploaded on torch's stream, read on the context's
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
    cams = {"pinhole": np.ascontiguousarray(lens_camera(scene.camera).reshape(1)),
            "thin_lens": np.ascontiguousarray(lens_camera(scene.camera, aperture=0.3, focus=10.0, stream_base=1).reshape(1))}
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def lens(cam, u):
        r._call("rt_lens_device", ctypes.c_void_p(cam.ctypes.data), 0, n, P(out_t["lens"]), bounces, u, 1, P(seg_t["lens"]))

    def radiance(rays_t, u):
        r._call("rt_radiance_device", P(rays_t), P(out_t["records"]), n, bounces, u, 1, P(seg_t["records"]))

    def drawn(cam, u):  # what a caller of the parent would have had to build on the host, per sample
        r._call("rt_lens_rays_device", ctypes.c_void_p(cam.ctypes.data), 0, n, u, P(drawn_t))
        radiance(drawn_t, u)

    series = {"pinhole/lens": lambda u: lens(cams["pinhole"], u),
              "pinhole/records": lambda u: radiance(records_t, u),
              "thin_lens/lens": lambda u: lens(cams["thin_lens"], u),
              "thin_lens/rays_then_records": lambda u: drawn(cams["thin_lens"], u)}
    same = {}
    for camera in cams:  # what is timed is the same computation
        names = [k for k in series if k.startswith(camera + "/")]
        for t in seg_t.values():
            t.zero_()
        torch.cuda.synchronize()
        for k in names:
            series[k](2)
        r.synchronize()
        same[camera] = bool(torch.equal(out_t["lens"].view(torch.int32), out_t["records"].view(torch.int32)))
        assert same[camera] and int(seg_t["lens"].item()) == int(seg_t["records"].item()) > 0, (camera, same)
    t_settle = time.perf_counter()
    while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
        for f in series.values():
            f(1)
        r.synchronize()
    ms = {k: [] for k in series}
    for _ in range(args.rounds):
        for k, f in series.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for i in range(args.reps):
                f(1 + i)
            t1.record(stream)
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / args.reps)
    med = statistics.median
    for k, v in ms.items():
        camera, name = k.split("/")
        emit(kind="lens", camera=camera, series=name, bounces=bounces, pixels=n, samples=1, rounds=args.rounds,
             reps=args.reps, ms=round(med(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
             spread=round((max(v) - min(v)) / med(v), 4), ratio_to_lens=round(med(v) / med(ms[camera + "/lens"]), 4),
             bit_identical=same[camera], build=r._lib.rt_build_hash().decode())


def build_gather_records():
    """tools/gather_records.c as a shared library next to the oracle's (compiled on first use)."""
    import subprocess

    from oracle import oracle as O

    oracle_so = O.build()
    src = Path(__file__).resolve().parent / "gather_records.c"
    out = oracle_so.parent / "libgather_records.so"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, oracle_so.stat().st_mtime):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared", "-std=c11",
                        "-Wall", "-o", str(out), str(src), f"-L{oracle_so.parent}", "-l:" + oracle_so.name,
                        "-Wl,-rpath,$ORIGIN", "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.gather_records.restype = None
    lib.gather_records.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.c_void_p]
    return lib


def gather_bench(r, args, scene, bounces, dev, emit):
    """The --gather series (module docstring)."""
    import statistics

    import torch

    n, samples, first = args.points, args.samples, 1
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
    P = ctypes.c_void_p

    # the points: first hits of the camera rays, spread evenly over the image
    q = camera_query_rays(scene)
    q_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    hits_t = torch.empty((q.shape[0], 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r._call("rt_trace_rays_device", P(q_t.data_ptr()), P(hits_t.data_ptr()), q.shape[0])
    r.synchronize()
    h = hits_t.cpu().numpy().view(B.HIT).reshape(-1)
    hit = np.nonzero(h["kind"] != B.HIT_MISS)[0]
    assert hit.shape[0] >= n, (hit.shape[0], n)
    pick = hit[np.linspace(0, hit.shape[0] - 1, n).astype(np.int64)]
    points = np.zeros(n, B.GATHER_POINT)
    points["position"], points["normal"] = h["position"][pick], h["normal"][pick]
    points["stream"] = 1 + np.arange(n, dtype=np.uint32)
    del q_t, hits_t

    # the by-hand records in both orders (streams folded: one call traces them all)
    helper = build_gather_records()
    rec_t, host_ms = {}, {}
    for order, point_major in (("sample_major", 0), ("point_major", 1)):
        t0 = time.perf_counter()
        records = np.zeros((samples * n, 8), np.float32)
        helper.gather_records(points.ctypes.data, n, first, samples, point_major, records.ctypes.data)
        host_ms[order] = (time.perf_counter() - t0) * 1e3
        rec_t[order] = torch.from_numpy(records).to(dev)
    # the shape the call replaces: each point's first direction, the point's own stream
    long_rec = records.reshape(n, samples, 8)[:, 0].copy()
    long_rec.view(np.uint32)[:, 3] = points["stream"]
    long_rec_t = torch.from_numpy(long_rec).to(dev)
    points_t = torch.from_numpy(points.view(np.float32).reshape(-1, 8)).to(dev)
    hand_t = torch.empty((samples * n, 4), dtype=torch.float32, device=dev)
    gather_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
    long_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
    seg_t = torch.zeros(4, dtype=torch.int64, device=dev)  # by hand in both orders, gather, the replaced shape
    torch.cuda.synchronize()
    seg = [P(seg_t.data_ptr() + 8 * i) for i in range(4)]

    def by_hand(order, counter):
        r._call("rt_radiance_device", P(rec_t[order].data_ptr()), P(hand_t.data_ptr()), n * samples, bounces, 1, 1,
                seg[counter])

    def gather():
        r._call("rt_gather_device", P(points_t.data_ptr()), P(gather_t.data_ptr()), n, bounces, first, samples, seg[2])

    def replaced():
        r._call("rt_radiance_device", P(long_rec_t.data_ptr()), P(long_t.data_ptr()), n, bounces, first, samples, seg[3])

    def tree(lights):  # step 4 of the contract on (samples, n, 4): torch's f32 add is the IEEE one
        p = torch.zeros((64, n, 4), dtype=torch.float32, device=dev)
        for k in range(0, samples, 64):
            m = min(64, samples - k)
            p[:m] = p[:m] + lights[k:k + m]
        off = 32
        while off:
            p[:off] = p[:off] + p[off:2 * off]
            off //= 2
        return p[0]

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def hand_tree(order):  # the contract's tree over what the by-hand call just wrote
        r.synchronize()
        lights = hand_t.view(samples, n, 4) if order == "sample_major" else hand_t.view(n, samples, 4).permute(1, 0, 2)
        ok = bool(torch.equal(tree(lights).view(torch.int32), gather_t.view(torch.int32)))
        torch.cuda.synchronize()
        return ok

    for fn in (lambda: by_hand("sample_major", 0), lambda: by_hand("point_major", 1), gather, replaced):
        fn()  # warm-up of every shape and placement
    r.synchronize()
    ms = {"by_hand_sample_major": [], "by_hand_point_major": [], "gather": [], "replaced": []}
    segments, same = [], []
    for _ in range(args.rounds):
        seg_t.zero_()
        gather_t.zero_()
        torch.cuda.synchronize()
        ms["gather"].append(timed(gather))
        assert bool(gather_t.view(torch.int32).any())
        ok = []
        for counter, order in enumerate(("sample_major", "point_major")):
            hand_t.zero_()
            torch.cuda.synchronize()
            ms["by_hand_" + order].append(timed(lambda: by_hand(order, counter)))
            ok.append(hand_tree(order))
        ms["replaced"].append(timed(replaced))
        r.synchronize()
        counted = [int(v) for v in seg_t.cpu().numpy()]
        assert counted[0] == counted[1] == counted[2], counted
        assert all(ok), "the tree over the by-hand results differs from the gather"
        segments.append(counted)
        same.append(all(ok))
    med = statistics.median
    ms["by_hand"] = min(ms["by_hand_sample_major"], ms["by_hand_point_major"], key=med)  # the faster order is the yardstick
    row = {k + "_ms": round(med(v), 3) for k, v in ms.items()}
    row.update({k + "_ms_min": round(min(v), 3) for k, v in ms.items()})
    row.update({k + "_ms_max": round(max(v), 3) for k, v in ms.items()})
    emit(kind="gather", bounces=bounces, points=n, samples=samples, rounds=args.rounds, paths=n * samples,
         segments_per_path=round(segments[0][2] / (n * samples), 4), segments_equal=True, tree_bit_identical=all(same),
         gather_over_by_hand=round(med(ms["gather"]) / med(ms["by_hand"]), 4),
         gather_over_replaced=round(med(ms["gather"]) / med(ms["replaced"]), 4),
         replaced_segments_per_path=round(segments[0][3] / (n * samples), 4),
         gather_mray_s=round(segments[0][2] / med(ms["gather"]) / 1e3, 1),
         by_hand_mray_s=round(segments[0][0] / med(ms["by_hand"]) / 1e3, 1),
         records_host_ms=round(min(host_ms.values()), 1), records_mb=round(records.nbytes / 2 ** 20, 1), build=r._lib.rt_build_hash().decode(), **row)


def probe_bench(r, args, scene, bounces, dev, emit):
    """The --probe series (module docstring)."""
    import statistics

    import torch

    n, samples, first = args.points, args.samples, 1
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
    P = ctypes.c_void_p

    # the probes: first hits of the camera rays, spread evenly over the image, moved into free space
    q = camera_query_rays(scene)
    q_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    hits_t = torch.empty((q.shape[0], 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r._call("rt_trace_rays_device", P(q_t.data_ptr()), P(hits_t.data_ptr()), q.shape[0])
    r.synchronize()
    h = hits_t.cpu().numpy().view(B.HIT).reshape(-1)
    hit = np.nonzero(h["kind"] != B.HIT_MISS)[0]
    assert hit.shape[0] >= n, (hit.shape[0], n)
    pick = hit[np.linspace(0, hit.shape[0] - 1, n).astype(np.int64)]
    probes = np.zeros(n, B.PROBE)
    probes["position"] = h["position"][pick] + h["normal"][pick] * np.float32(0.25)
    probes["stream"] = 1 + np.arange(n, dtype=np.uint32)
    points = np.zeros(n, B.GATHER_POINT)  # the same paths as gather points: normal (0, 0, 0)
    points["position"], points["stream"] = probes["position"], probes["stream"]
    del q_t, hits_t

    helper = build_gather_records()
    rec_t, host_ms = {}, {}
    for order, point_major in (("sample_major", 0), ("point_major", 1)):
        t0 = time.perf_counter()
        records = np.zeros((samples * n, 8), np.float32)
        helper.gather_records(points.ctypes.data, n, first, samples, point_major, records.ctypes.data)
        host_ms[order] = (time.perf_counter() - t0) * 1e3
        # a draw of -0 (rho = -0 at r = 1: about one in 2^24 draws) is +0 in these records, 0 + g, and
        # -0 in the probe's direction; the jitter's add and step 5's +0.0f start absorb the sign, and
        # the bit comparison of every round is the check
        zero_draws = int((records[:, 4:7] == 0).sum())
        rec_t[order] = torch.from_numpy(records).to(dev)
    probes_t = torch.from_numpy(probes.view(np.float32).reshape(-1, 4)).to(dev)
    hand_t = torch.empty((samples * n, 4), dtype=torch.float32, device=dev)
    sh_t = torch.empty((n, 9, 4), dtype=torch.float32, device=dev)
    seg_t = torch.zeros(3, dtype=torch.int64, device=dev)  # by hand in both orders, the probe call
    torch.cuda.synchronize()
    seg = [P(seg_t.data_ptr() + 8 * i) for i in range(3)]

    def by_hand(order, counter):
        r._call("rt_radiance_device", P(rec_t[order].data_ptr()), P(hand_t.data_ptr()), n * samples, bounces, 1, 1,
                seg[counter])

    def probe():
        r._call("rt_probe_sh_device", P(probes_t.data_ptr()), P(sh_t.data_ptr()), n, bounces, first, samples, seg[2])

    def basis(d):  # step 4 on (..., 3): each torch operation is one f32 operation
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        c1, c2 = 0.48860251, 1.09254843
        return torch.stack([torch.full_like(x, 0.28209479), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z),
                            0.31539157 * (3.0 * (z * z) - 1.0), c2 * (x * z), 0.54627422 * (x * x - y * y)], dim=-1)

    def tree(terms):  # step 5 on (samples, n, 4)
        p = torch.zeros((64, n, 4), dtype=torch.float32, device=dev)
        for k in range(0, samples, 64):
            m = min(64, samples - k)
            p[:m] = p[:m] + terms[k:k + m]
        off = 32
        while off:
            p[:off] = p[:off] + p[off:2 * off]
            off //= 2
        return p[0]

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def hand_projection(order):  # steps 4 and 5 over what the by-hand call just wrote
        r.synchronize()
        rec = rec_t[order]
        if order == "sample_major":
            lights, dirs = hand_t.view(samples, n, 4), rec.view(samples, n, 8)[..., 4:7]
        else:
            lights, dirs = hand_t.view(n, samples, 4).permute(1, 0, 2), rec.view(n, samples, 8).permute(1, 0, 2)[..., 4:7]
        b = basis(dirs)
        ok = True
        for k in range(9):
            want = tree(lights * b[..., k:k + 1])
            ok = ok and bool(torch.equal(want.view(torch.int32), sh_t[:, k].contiguous().view(torch.int32)))
        torch.cuda.synchronize()
        return ok

    for fn in (lambda: by_hand("sample_major", 0), lambda: by_hand("point_major", 1), probe):
        fn()  # warm-up of every shape and placement
    r.synchronize()
    ms = {"by_hand_sample_major": [], "by_hand_point_major": [], "probe": []}
    segments, same = [], []
    for _ in range(args.rounds):
        seg_t.zero_()
        sh_t.zero_()
        torch.cuda.synchronize()
        ms["probe"].append(timed(probe))
        assert bool(sh_t.view(torch.int32).any())
        ok = []
        for counter, order in enumerate(("sample_major", "point_major")):
            hand_t.zero_()
            torch.cuda.synchronize()
            ms["by_hand_" + order].append(timed(lambda: by_hand(order, counter)))
            ok.append(hand_projection(order))
        r.synchronize()
        counted = [int(v) for v in seg_t.cpu().numpy()]
        assert counted[0] == counted[1] == counted[2], counted
        assert all(ok), "steps 4 and 5 over the by-hand results differ from the probe call"
        segments.append(counted)
        same.append(all(ok))
    med = statistics.median
    ms["by_hand"] = min(ms["by_hand_sample_major"], ms["by_hand_point_major"], key=med)  # the faster order is the yardstick
    row = {k + "_ms": round(med(v), 3) for k, v in ms.items()}
    row.update({k + "_ms_min": round(min(v), 3) for k, v in ms.items()})
    row.update({k + "_ms_max": round(max(v), 3) for k, v in ms.items()})
    emit(kind="probe", bounces=bounces, probes=n, samples=samples, rounds=args.rounds, paths=n * samples,
         segments_per_path=round(segments[0][2] / (n * samples), 4), segments_equal=True, sh_bit_identical=all(same),
         probe_over_by_hand=round(med(ms["probe"]) / med(ms["by_hand"]), 4),
         probe_mray_s=round(segments[0][2] / med(ms["probe"]) / 1e3, 1),
         by_hand_mray_s=round(segments[0][0] / med(ms["by_hand"]) / 1e3, 1),
         records_host_ms=round(min(host_ms.values()), 1), records_mb=round(records.nbytes / 2 ** 20, 1),
         zero_draws=zero_draws, build=r._lib.rt_build_hash().decode(), **row)


def ambient_bench(r, args, scene, config, dev, emit):
    """The --ambient series of one configuration (module docstring)."""
    import statistics

    import torch

    n, samples, first = args.points, args.samples, 1
    stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
    P = ctypes.c_void_p

    # the points: first hits of the camera rays, spread evenly over the image
    q = camera_query_rays(scene)
    q_t = torch.from_numpy(q.view(np.float32).reshape(-1, 8)).to(dev)
    hits_t = torch.empty((q.shape[0], 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r._call("rt_trace_rays_device", P(q_t.data_ptr()), P(hits_t.data_ptr()), q.shape[0])
    r.synchronize()
    h = hits_t.cpu().numpy().view(B.HIT).reshape(-1)
    hit = np.nonzero(h["kind"] != B.HIT_MISS)[0]
    assert hit.shape[0] >= n, (hit.shape[0], n)
    pick = hit[np.linspace(0, hit.shape[0] - 1, n).astype(np.int64)]
    points = np.zeros(n, B.AMBIENT_POINT)
    points["position"], points["normal"] = h["position"][pick], h["normal"][pick]
    points["stream"] = 1 + np.arange(n, dtype=np.uint32)
    points["t_max"] = args.t_max
    del q_t, hits_t

    # (c)'s records, point-major: a radiance record's pad is an occlusion record's t_max
    helper = build_gather_records()
    t0 = time.perf_counter()
    records = np.zeros((n * samples, 8), np.float32)
    helper.gather_records(points.ctypes.data, n, first, samples, 1, records.ctypes.data)
    records[:, 7] = args.t_max
    host_ms = (time.perf_counter() - t0) * 1e3
    rec_t = torch.from_numpy(records).to(dev)
    points_t = torch.from_numpy(points.view(np.float32).reshape(-1, 8)).to(dev)
    out_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
    gather_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
    bytes_t = torch.empty((n * samples,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def ambient():
        r._call("rt_ambient_device", P(points_t.data_ptr()), P(out_t.data_ptr()), n, first, samples)

    def gather():
        r._call("rt_gather_device", P(points_t.data_ptr()), P(gather_t.data_ptr()), n, 1, first, samples, None)

    def occluded():
        r._call("rt_occluded_device", P(rec_t.data_ptr()), P(bytes_t.data_ptr()), n * samples)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def same_as_occluded():  # steps 4 and 5 over (c)'s bytes: torch's f32 add is the IEEE one
        r.synchronize()
        v = (1 - bytes_t.view(n, samples)).to(torch.float32)
        ok = bool(torch.equal(v.sum(dim=1, dtype=torch.float64).to(torch.float32), out_t[:, 3]))
        p = torch.zeros((n, 64, 4), dtype=torch.float32, device=dev)
        d = rec_t.view(n, samples, 8)[..., 4:7]
        for k in range(0, samples, 64):
            m = min(64, samples - k)
            open_k = v[:, k:k + m, None]
            terms = torch.cat([torch.where(open_k != 0, d[:, k:k + m], torch.zeros_like(d[:, k:k + m])), open_k], dim=2)
            p[:, :m] = p[:, :m] + terms
        off = 32
        while off:
            p[:, :off] = p[:, :off] + p[:, off:2 * off]
            off //= 2
        ok = ok and bool(torch.equal(p[:, 0].contiguous().view(torch.int32), out_t.view(torch.int32)))
        torch.cuda.synchronize()
        return ok

    for fn in (ambient, gather, occluded):
        fn()  # warm-up of every shape and placement
    r.synchronize()
    ms = {"ambient": [], "gather_b1": [], "occluded_resident": []}
    same = []
    for _ in range(args.rounds):
        out_t.zero_()
        bytes_t.zero_()
        torch.cuda.synchronize()
        ms["ambient"].append(timed(ambient))
        ms["gather_b1"].append(timed(gather))
        ms["occluded_resident"].append(timed(occluded))
        same.append(same_as_occluded())
        assert same[-1], "the tree over rt_occluded's bytes differs from rt_ambient"
    med = statistics.median
    row = {k + "_ms": round(med(v), 3) for k, v in ms.items()}
    row.update({k + "_ms_min": round(min(v), 3) for k, v in ms.items()})
    row.update({k + "_ms_max": round(max(v), 3) for k, v in ms.items()})
    emit(kind="ambient", config=config, points=n, samples=samples, t_max=args.t_max, rounds=args.rounds,
         searches=n * samples, open_fraction=round(float(out_t[:, 3].sum(dtype=torch.float64).item()) / (n * samples), 4),
         bit_identical_to_occluded=all(same),
         ambient_over_gather=round(med(ms["ambient"]) / med(ms["gather_b1"]), 4),
         ambient_over_occluded=round(med(ms["ambient"]) / med(ms["occluded_resident"]), 4),
         ambient_msearch_s=round(n * samples / med(ms["ambient"]) / 1e3, 1),
         records_host_ms=round(host_ms, 1), records_mb=round(records.nbytes / 2 ** 20, 1),
         build=r._lib.rt_build_hash().decode(), **row)


def lines_out(args, lines):
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2_rtiow")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32, help="frames of the render yardstick")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--occluded", action="store_true", help="the occlusion kernel against the closest-hit call")
    ap.add_argument("--hits", action="store_true", help="the hit-list kernel against the closest-hit call")
    ap.add_argument("--nearest", action="store_true", help="the proximity kernel, walk and sweep, beside the closest-hit call")
    ap.add_argument("--sweep-points", type=int, default=16384, help="--nearest: points of the sweep series")
    ap.add_argument("--radiance", action="store_true", help="the radiance kernel against a frame of the same rays")
    ap.add_argument("--gather", action="store_true", help="the gather query against the same paths done by hand")
    ap.add_argument("--probe", action="store_true", help="the probe query against the same paths done by hand")
    ap.add_argument("--ambient", action="store_true",
                    help="the ambient query against the gather at one bounce and the resident occlusion records")
    ap.add_argument("--lens", action="store_true", help="the lens query against the radiance query of the same rays")
    ap.add_argument("--ambient-configs", default="c2_rtiow,c3_chess", help="--ambient: the configurations, in one process")
    ap.add_argument("--t-max", type=float, default=1.0, help="--ambient: the bound of every point, in world units")
    ap.add_argument("--points", type=int, default=None,
                    help="--gather: surface points; --probe: probes (4096); --ambient: surface points (65536)")
    ap.add_argument("--samples", type=int, default=None,
                    help="--gather, --probe: samples per point (1024); --ambient: samples per point (256)")
    ap.add_argument("--bounces", type=int, default=None,
                    help="--radiance, --gather, --probe, --lens: bounce limit (default: the configuration's)")
    ap.add_argument("--settle-ms", type=float, default=150.0, help="--radiance: untimed work before the rounds")
    ap.add_argument("--rounds", type=int, default=7, help="--occluded, --radiance: rounds the series alternate over")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="rt_set_tuning settings of the context (e.g. primary_pass=0: the yardstick frame without its pre-pass)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "query_bench needs a HIP device"
    dev = torch.device("cuda:0")
    if args.points is None:
        args.points = 65536 if args.ambient else 4096
    if args.samples is None:
        args.samples = 256 if args.ambient else 1024
    scene, bounces = build_config(args.config, width=args.width, height=args.height)
    q = camera_query_rays(scene)
    n = q.shape[0]
    perm = np.random.default_rng(2024).permutation(n)
    if args.occluded:  # (rt_occlusion_ray: t_max where rt_query_ray pads; +inf, "any hit at all")
        q["_pad1"] = np.inf
    sets = {"coherent": q, "incoherent": np.ascontiguousarray(q[perm])}
    tensors = {k: torch.from_numpy(v.view(np.float32).reshape(-1, 8)).to(dev) for k, v in sets.items()}
    hits_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the uploads ran on torch's stream, the queries run on the context's
    lines = []

    def emit(**kw):
        rec = dict(config=args.config, width=args.width, height=args.height)
        rec.update(kw)
        if tuning:
            rec["tuning"] = tuning
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    call = "rt_occluded_device" if args.occluded else "rt_trace_rays_device"
    tuning = {k: int(v) for k, v in (kv.split("=", 1) for kv in args.tune)}
    if args.ambient:
        for config in args.ambient_configs.split(","):
            scene, _ = build_config(config, width=args.width, height=args.height)
            with Renderer(scene, tuning=tuning) as r:
                ambient_bench(r, args, scene, config, dev, emit)
        lines_out(args, lines)
        return
    with Renderer(scene, tuning=tuning) as r:
        if args.lens:
            lens_bench(r, args, scene, bounces if args.bounces is None else args.bounces, dev, emit)
        elif args.probe:
            probe_bench(r, args, scene, bounces if args.bounces is None else args.bounces, dev, emit)
        elif args.gather:
            gather_bench(r, args, scene, bounces if args.bounces is None else args.bounces, dev, emit)
        elif args.radiance:
            radiance_bench(r, args, scene, bounces if args.bounces is None else args.bounces, dev, emit)
        elif args.occluded and not args.sweep:
            occlusion_bench(r, args, q, dev, emit)
        elif args.hits:
            hits_bench(r, args, q, dev, emit)
        elif args.nearest:
            nearest_bench(r, args, q, dev, emit)
        elif args.sweep:
            sizes = [s for s in (64, 256, 1024, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 1048576) if s < n] + [n]
            for m in sizes:
                row, ref = {}, None
                for name, mode in (("mode0", 0), ("staged", 2)):
                    r.set_tuning("query_lds_mode", mode)
                    reps = max(args.reps, min(400, (1 << 22) // m))
                    row[name + "_us"] = round(time_queries(r, tensors["coherent"], hits_t, m, reps, call) * 1e6, 2)
                    got = hits_t[:m].cpu().numpy().tobytes()
                    ref = got if ref is None else ref
                    assert got == ref, "placements disagree"
                emit(kind="sweep", call=call, rays=m, **row)
            r.set_tuning("query_lds_mode", -1)
        else:
            for name, t in tensors.items():
                s = time_queries(r, t, hits_t, n, args.reps)
                h = hits_t.cpu().numpy().view(B.HIT).reshape(-1)
                emit(kind="throughput", rays_set=name, rays=n, ms=round(s * 1e3, 4), mray_s=round(n / s / 1e6, 1),
                     hit_fraction=round(float((h["kind"] != 0).mean()), 4))
            # the render's rate for the same configuration, measured the same way
            for _ in range(16):
                r.compute_frame(bounces)
            r.synchronize()
            r.reset_ray_count()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                r.compute_frame(bounces)
            r.synchronize()
            s = time.perf_counter() - t0
            emit(kind="render", frames=args.frames, bounces=bounces, ms_per_frame=round(s * 1e3 / args.frames, 4),
                 mray_s=round(r.ray_count() / s / 1e6, 1))
    lines_out(args, lines)


if __name__ == "__main__":
    main()
