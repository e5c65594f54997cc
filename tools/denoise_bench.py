"""Time of the feature buffers and the guided a-trous denoiser (rt_compute_features, rt_denoise).

usage: python tools/denoise_bench.py [--configs c2_rtiow c3_chess] [--width 1920 --height 1080]
                                     [--reps 50] [--rounds 7] [--frames 4] [--bench-line FILE]
                                     [--out profiles/denoise/denoise_bench.json]

Per configuration, after `--frames` rendered frames and a warm-up of every series:

* ms per rt_compute_features (the scene epoch is bumped before each call with an rt_update_camera
  of the same camera, a host-only call, so every call recomputes the planes);
* ms per rt_denoise with iterations = 0..5, the step-1 and step-2 passes LDS-tiled (tuning
  "denoise_lds" 1) and with direct loads (0); the time of the pass with step 2^i is the difference
  t(i+1) - t(i) of the medians (the clamp-and-pack moves from one pass to the next, so it cancels);
* ms per whole default rt_denoise (4 iterations), both ways;
* ms per rt_denoise_temporal with iterations = 0 (the temporal stage alone, plus the 20 B per pixel of
  its result and pack) and with the default iterations, without a previous slot (rt_temporal_reset,
  a host-only call, before each call) and with one (before each timed round: a call, a reset of the
  accumulation, the same frames again and one untimed call; every timed call then reprojects the
  same previous slot). The stage is quoted against its one-touch floor of 144 B per pixel (16 B of
  accumulation, 32 B of features, 48 B of history read once, 48 B written) and the whole call
  against the default rt_denoise of the same job.

Timing: device events on the context's stream around `--reps` stream-ordered calls; the series
alternate over `--rounds` rounds (an A/B in one process, same clocks); median, minimum and maximum
over the rounds. The spread of a series over its rounds is the run-to-run noise a difference has
to exceed. Beside each pass: its one-touch traffic floor -- 48 B read and 16 B written per pixel
at the HBM peak bench.py's roofline uses -- and the fraction of it achieved. `--bench-line`: a
file holding bench.py's JSON result line, whose ms_per_step (the C2 frame) each figure is also
given as a ratio of. The record carries the library's build hash.

`--motion [--parent-lib FILE]`: instead of the above, on c3_chess only, rt_denoise_temporal against
rt_denoise_temporal_motion with one moved piece (iterations 0, the stage alone, and the default 4),
every timed call reprojecting the same previous slot; with `--parent-lib` (a build of the parent
commit, tools/build_at_commit.py) the plain call is also timed on that library in the same process,
the series alternating over the rounds, on two contexts per library. The plain call of this commit
has to sit within the spread of the parent's repeated runs (minimum to maximum over the rounds of
both parent contexts); the record says whether it does. Default
`--out` then: profiles/temporal_motion/bench.json.
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from rust_gpu_raytracing_amd import Renderer  # noqa: E402
from rust_gpu_raytracing_amd import _native as N  # noqa: E402
from rust_gpu_raytracing_amd.scene import build_config  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py: MI355X HBM3E peak
PASS_BYTES_PER_PIXEL = 48 + 16
TEMPORAL_BYTES_PER_PIXEL = 16 + 32 + 48 + 48
MOTION_BYTES_PER_PIXEL = TEMPORAL_BYTES_PER_PIXEL + 8 + 8 + 8  # the ID plane, the I taps once, the I plane written
MAX_ITERATIONS = 5  # steps 1, 2, 4, 8, 16


def motion_case(args):
    """--motion: plain rt_denoise_temporal (this build and, if given, the parent's) against
    rt_denoise_temporal_motion with one moved piece."""
    import torch

    from rust_gpu_raytracing_amd import motion

    assert torch.cuda.is_available(), "denoise_bench needs a HIP device"
    dev = torch.device("cuda:0")
    # two contexts per library: what differs between two contexts of one build (where their planes
    # landed in memory, their place in the round) is part of the spread a difference has to exceed
    libs = {"this": None}
    if args.parent_lib:
        parent = N.load_library(args.parent_lib)
        libs.update({"parent": parent, "this_b": None, "parent_b": parent})
    series, renderers = {}, []
    for which, lib in libs.items():
        for kind in (("plain", "motion") if which == "this" else ("plain",)):
            scene, bounces = build_config("c3_chess", width=args.width, height=args.height)
            r = Renderer(scene, lib=lib)
            renderers.append(r)
            stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
            t = N.rt_temporal_params()
            r._lib.rt_temporal_default_params(ctypes.byref(t))
            t.world_to_pixel[:] = [float(v) for v in scene.camera.world_to_pixel().reshape(16)]
            for _ in range(args.frames):
                r.compute_frame(bounces)
            if kind == "motion":  # a first call, then the piece with the most pixels moves
                r._call("rt_denoise_temporal_motion", ctypes.byref(t), None, None, 0, None, 0)
                before = motion.snapshot(scene)
                ids = r.feature_ids()
                counts = np.bincount(ids[..., 1][ids[..., 0] == 2], minlength=34)[:33]
                counts[0] = 0
                piece = scene.objects[int(counts.argmax())]
                piece.transformation = (np.asarray(piece.transformation, np.float32)
                                        + np.float32([0.35, 0.0, -0.25])).astype(np.float32)
                piece.rotation = np.float32([0.0, 25.0, 0.0])
                piece.scale = np.float32(1.1)
                r.update_scene(device=True)
                records = motion.object_motion(before["objects"], motion.snapshot(scene)["objects"])
            else:
                r._call("rt_denoise_temporal", ctypes.byref(t), None)
                r.reset_accumulation()
                records = None
            for _ in range(args.frames):
                r.compute_frame(bounces)
            for it in (0, 4):
                p = N.rt_denoise_params()
                r._lib.rt_denoise_default_params(ctypes.byref(p))
                p.iterations = it
                if records is None:
                    fn = (lambda r=r, t=t, p=p: r._call("rt_denoise_temporal", ctypes.byref(t), ctypes.byref(p)))
                else:
                    fn = (lambda r=r, t=t, p=p, rec=records: r._call(
                        "rt_denoise_temporal_motion", ctypes.byref(t), ctypes.byref(p), N.ptr(rec), rec.shape[0], None, 0))
                series[f"{kind}_it{it}/{which}"] = (r, stream, fn)
    for r, stream, fn in series.values():  # warm-up
        fn()
        r.synchronize()
    kept = int((renderers[1].read_temporal()[1] > args.frames).sum())  # this build's motion renderer
    ms = {k: [] for k in series}
    for _ in range(args.rounds):
        for name, (r, stream, fn) in series.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                fn()
            t1.record(stream)
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.reps)
    px = args.width * args.height
    record = dict(width=args.width, height=args.height, reps=args.reps, rounds=args.rounds, frames=args.frames,
                  config="c3_chess", device=torch.cuda.get_device_name(0), hbm_peak_gbs=HBM_PEAK_GBS,
                  build={w: (lib or renderers[0]._lib).rt_build_hash().decode() for w, lib in libs.items()},
                  pixels_with_history_after_the_move=kept,
                  traffic_floor_ms=dict(plain_stage=round(px * TEMPORAL_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3, 5),
                                        motion_stage=round(px * MOTION_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3, 5)),
                  series={k: dict(ms=round(float(np.median(v)), 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5))
                          for k, v in ms.items()})
    if args.parent_lib:
        for it in (0, 4):
            par = [record["series"][f"plain_it{it}/{w}"] for w in ("parent", "parent_b")]
            lo, hi = min(b["ms_min"] for b in par), max(b["ms_max"] for b in par)
            record[f"plain_it{it}_parent_spread_ms"] = [lo, hi]
            record[f"plain_it{it}_within_parent_spread"] = {
                w: bool(lo <= record["series"][f"plain_it{it}/{w}"]["ms"] <= hi) for w in ("this", "this_b")}
    for r in renderers:
        r.close()
    print(json.dumps(record), flush=True)
    out = Path(args.out if args.out != "profiles/denoise/denoise_bench.json" else "profiles/temporal_motion/bench.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2_rtiow", "c3_chess"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default="profiles/denoise/denoise_bench.json")
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if args.motion:
        return motion_case(args)
    assert torch.cuda.is_available(), "denoise_bench needs a HIP device"
    dev = torch.device("cuda:0")
    frame_ms = None
    if args.bench_line:
        for line in Path(args.bench_line).read_text().splitlines():
            if line.startswith("{") and "ms_per_step" in line:
                frame_ms = float(json.loads(line)["ms_per_step"])
    record = dict(width=args.width, height=args.height, reps=args.reps, rounds=args.rounds, frames=args.frames,
                  hbm_peak_gbs=HBM_PEAK_GBS, pass_bytes_per_pixel=PASS_BYTES_PER_PIXEL,
                  temporal_bytes_per_pixel=TEMPORAL_BYTES_PER_PIXEL, c2_frame_ms=frame_ms,
                  device=torch.cuda.get_device_name(0), configs={})
    for config in args.configs:
        scene, bounces = build_config(config, width=args.width, height=args.height)
        with Renderer(scene) as r:
            record["build"] = r._lib.rt_build_hash().decode()
            stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
            for _ in range(args.frames):
                r.compute_frame(bounces)
            cam = N.rt_ray_camera()
            cam.origin[:] = [float(x) for x in scene.camera.position]

            def features():
                r._call("rt_update_camera", ctypes.byref(cam))
                r._call("rt_compute_features")

            def denoise(iterations):
                p = N.rt_denoise_params()
                r._lib.rt_denoise_default_params(ctypes.byref(p))
                p.iterations = iterations
                return lambda: r._call("rt_denoise", ctypes.byref(p))

            def temporal(iterations, previous):
                t = N.rt_temporal_params()
                r._lib.rt_temporal_default_params(ctypes.byref(t))
                t.world_to_pixel[:] = [float(v) for v in scene.camera.world_to_pixel().reshape(16)]
                p = N.rt_denoise_params()
                r._lib.rt_denoise_default_params(ctypes.byref(p))
                p.iterations = iterations

                def call():
                    if not previous:
                        r._call("rt_temporal_reset")
                    r._call("rt_denoise_temporal", ctypes.byref(t), ctypes.byref(p))

                def setup():  # a previous slot from the generation before, the same accumulation again
                    r._call("rt_temporal_reset")
                    r._call("rt_denoise_temporal", ctypes.byref(t), ctypes.byref(p))
                    r.reset_accumulation()
                    for _ in range(args.frames):
                        r.compute_frame(bounces)
                    r._call("rt_denoise_temporal", ctypes.byref(t), ctypes.byref(p))
                    r.synchronize()

                return call, (setup if previous else None)

            series = {"features": (None, features, None)}
            for lds in (1, 0):
                for it in range(MAX_ITERATIONS + 1):
                    series[f"denoise_it{it}/lds{lds}"] = (lds, denoise(it), None)
            for it in (0, 4):
                for previous in (0, 1):
                    series[f"temporal_it{it}/prev{previous}"] = (None, *temporal(it, previous))
            results = {}
            for name, (lds, fn, setup) in series.items():  # warm-up of everything timed; the variants agree
                if lds is not None:
                    r.set_tuning("denoise_lds", lds)
                elif name.startswith("temporal"):
                    r.set_tuning("denoise_lds", 1)
                if setup:
                    setup()
                fn()
                r.synchronize()
                if lds is not None:
                    f, u = r.read_denoised()
                    key = name.split("/")[0]
                    if key in results:
                        assert results[key] == (f.tobytes(), u.tobytes()), "LDS-tiled and direct passes disagree"
                    results[key] = (f.tobytes(), u.tobytes())
            ms = {k: [] for k in series}
            for _ in range(args.rounds):
                for name, (lds, fn, setup) in series.items():
                    if lds is not None:
                        r.set_tuning("denoise_lds", lds)
                    elif name.startswith("temporal"):
                        r.set_tuning("denoise_lds", 1)
                    if setup:
                        setup()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(args.reps):
                        fn()
                    t1.record(stream)
                    t1.synchronize()
                    ms[name].append(t0.elapsed_time(t1) / args.reps)
            floor_ms = args.width * args.height * PASS_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3

            def stat(v):
                out = dict(ms=round(float(np.median(v)), 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5))
                if frame_ms:
                    out["of_c2_frame"] = round(out["ms"] / frame_ms, 4)
                return out

            rec = dict(bounces=bounces, features=stat(ms["features"]), traffic_floor_ms_per_pass=round(floor_ms, 5))
            for lds in (1, 0):
                med = [float(np.median(ms[f"denoise_it{it}/lds{lds}"])) for it in range(MAX_ITERATIONS + 1)]
                passes = {}
                for it in range(MAX_ITERATIONS):
                    t = med[it + 1] - med[it]
                    passes[f"step{1 << it}"] = dict(ms=round(t, 5), floor_fraction=round(floor_ms / t, 4) if t > 0 else None,
                                                    of_c2_frame=round(t / frame_ms, 4) if frame_ms else None)
                rec[f"lds{lds}"] = dict(
                    denoise_by_iterations={f"it{it}": stat(ms[f"denoise_it{it}/lds{lds}"]) for it in range(MAX_ITERATIONS + 1)},
                    passes=passes, default_denoise=stat(ms[f"denoise_it4/lds{lds}"]))
            t_floor = args.width * args.height * TEMPORAL_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3
            plain = float(np.median(ms["denoise_it4/lds1"]))
            rec["temporal"] = dict(traffic_floor_ms_stage=round(t_floor, 5))
            for previous in (0, 1):
                stage, whole = stat(ms[f"temporal_it0/prev{previous}"]), stat(ms[f"temporal_it4/prev{previous}"])
                stage["floor_multiple"] = round(stage["ms"] / t_floor, 3)
                whole["of_default_denoise"] = round(whole["ms"] / plain, 4)
                rec["temporal"][f"prev{previous}"] = dict(stage_it0=stage, default_it4=whole)
            record["configs"][config] = rec
            print(json.dumps({config: rec}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
