"""Throughput of the ray-query kernel (rt_trace_rays_device) and its placement crossover.

usage: python tools/query_bench.py [--config c2_rtiow] [--width 1920 --height 1080]
                                   [--reps 20] [--sweep] [--out profiles/query_bench.jsonl]

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


def time_queries(r, rays_t, hits_t, n, reps):
    """Seconds per rt_trace_rays_device call over the first n rays (device tensors)."""
    args = (ctypes.c_void_p(rays_t.data_ptr()), ctypes.c_void_p(hits_t.data_ptr()), n)
    r._call("rt_trace_rays_device", *args)  # warm-up of this shape and placement
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r._call("rt_trace_rays_device", *args)
    r.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2_rtiow")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32, help="frames of the render yardstick")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "query_bench needs a HIP device"
    dev = torch.device("cuda:0")
    scene, bounces = build_config(args.config, width=args.width, height=args.height)
    q = camera_query_rays(scene)
    n = q.shape[0]
    perm = np.random.default_rng(2024).permutation(n)
    sets = {"coherent": q, "incoherent": np.ascontiguousarray(q[perm])}
    tensors = {k: torch.from_numpy(v.view(np.float32).reshape(-1, 8)).to(dev) for k, v in sets.items()}
    hits_t = torch.empty((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the uploads ran on torch's stream, the queries run on the context's
    lines = []

    def emit(**kw):
        rec = dict(config=args.config, width=args.width, height=args.height, **kw)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    with Renderer(scene) as r:
        if args.sweep:
            sizes = [s for s in (64, 256, 1024, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 1048576) if s < n] + [n]
            for m in sizes:
                row, ref = {}, None
                for name, mode in (("mode0", 0), ("staged", 2)):
                    r.set_tuning("query_lds_mode", mode)
                    reps = max(args.reps, min(400, (1 << 22) // m))
                    row[name + "_us"] = round(time_queries(r, tensors["coherent"], hits_t, m, reps) * 1e6, 2)
                    got = hits_t[:m].cpu().numpy().tobytes()
                    ref = got if ref is None else ref
                    assert got == ref, "placements disagree"
                emit(kind="sweep", rays=m, **row)
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
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
