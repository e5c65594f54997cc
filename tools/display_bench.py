"""Time of the display transform (rt_display): metering, exposure solve, tone curve and encode.

usage: python tools/display_bench.py [--configs c2_rtiow c3_chess] [--width 1920 --height 1080]
                                     [--reps 50] [--rounds 7] [--frames 4] [--bench-line FILE]
                                     [--sources frame uniform noise] [--calls-only]
                                     [--out profiles/display/display_bench.json]

Per configuration, after `--frames` rendered frames and a warm-up of every series, ms per call of:

* the full auto-exposure call (meter, solve, tone: three launches) and the manual call (the tone pass
  only: one launch) with the default curve and encode, on the real frame (source accumulation), on
  a uniform plane (every lane of every wave in one bin) and on a log-uniform noise plane over
  2^-20..2^20 (the bins spread over most of the histogram);
* the manual call with every operator x encode on the real frame;
* rt_denoise with 0 iterations, the existing one-touch kernel of the same shape (16 B read per
  pixel, 16 B + 4 B written), for comparison.

The library has no entry point that runs the metering kernel alone: "meter_and_solve" is the
difference of the medians of the auto and the manual call on the same source, that is the metering
kernel plus the one-wave solve kernel and their two launches. For the kernels' own times run it
under `rocprofv3 --kernel-trace --stats` with `--calls-only --sources <one source>`: the trace's
statistics are per kernel name, so one source per run keeps the metering kernel's figure apart.

Timing: device events on the context's stream around `--reps` stream-ordered calls; the series
alternate over `--rounds` rounds (one process, same clocks); median, minimum and maximum over the
rounds. One-touch floors from shapes at the HBM peak bench.py's roofline uses: metering reads 16 B
per pixel, the tone pass reads 16 B and writes 4 B per pixel. `--bench-line`: a file holding
bench.py's JSON result line, whose ms_per_step (the C2 frame) each figure is also given as a ratio
of. The record carries the library's build hash.
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
METER_BYTES_PER_PIXEL = 16
TONE_BYTES_PER_PIXEL = 16 + 4
OPS = {"linear": N.RT_TONE_LINEAR, "reinhard": N.RT_TONE_REINHARD, "aces": N.RT_TONE_ACES}
ENCODES = {"none": N.RT_ENCODE_NONE, "srgb": N.RT_ENCODE_SRGB}


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
    ap.add_argument("--sources", nargs="+", default=["frame", "uniform", "noise"], choices=["frame", "uniform", "noise"],
                    help="the sources to time (one at a time under a kernel trace, whose statistics are per kernel)")
    ap.add_argument("--calls-only", action="store_true", help="skip rt_denoise and the operator x encode series")
    ap.add_argument("--out", default="profiles/display/display_bench.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "display_bench needs a HIP device"
    dev = torch.device("cuda:0")
    frame_ms = None
    if args.bench_line:
        for line in Path(args.bench_line).read_text().splitlines():
            if line.startswith("{") and "ms_per_step" in line:
                frame_ms = float(json.loads(line)["ms_per_step"])
    n = args.width * args.height
    meter_floor = n * METER_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3
    tone_floor = n * TONE_BYTES_PER_PIXEL / (HBM_PEAK_GBS * 1e9) * 1e3
    record = dict(width=args.width, height=args.height, reps=args.reps, rounds=args.rounds, frames=args.frames,
                  hbm_peak_gbs=HBM_PEAK_GBS, meter_bytes_per_pixel=METER_BYTES_PER_PIXEL,
                  tone_bytes_per_pixel=TONE_BYTES_PER_PIXEL, meter_floor_ms=round(meter_floor, 5),
                  tone_floor_ms=round(tone_floor, 5), c2_frame_ms=frame_ms, device=torch.cuda.get_device_name(0),
                  configs={})
    gen = torch.Generator(device=dev).manual_seed(20)
    planes = {"uniform": torch.tensor([0.5, 0.25, 0.75, 0.5], device=dev).repeat(n, 1).contiguous(),
              "noise": torch.exp2(torch.rand((n, 4), generator=gen, device=dev) * 40.0 - 20.0).contiguous()}
    torch.cuda.synchronize()
    for config in args.configs:
        scene, bounces = build_config(config, width=args.width, height=args.height)
        with Renderer(scene) as r:
            record["build"] = r._lib.rt_build_hash().decode()
            stream = torch.cuda.ExternalStream(r.stream_handle, device=dev)
            for _ in range(args.frames):
                r.compute_frame(bounces)

            def display(source, auto, op="reinhard", encode="srgb"):
                p = N.rt_display_params()
                r._lib.rt_display_default_params(ctypes.byref(p))
                p.auto_exposure, p.tone_operator, p.encode = auto, OPS[op], ENCODES[encode]
                plane = None
                if source != "frame":
                    p.source, plane = N.RT_DISPLAY_PLANE, ctypes.c_void_p(planes[source].data_ptr())
                return lambda: r._call("rt_display", ctypes.byref(p), plane)

            dn = N.rt_denoise_params()
            r._lib.rt_denoise_default_params(ctypes.byref(dn))
            dn.iterations = 0
            series = {} if args.calls_only else {"denoise_it0": lambda: r._call("rt_denoise", ctypes.byref(dn))}
            for source in args.sources:
                series[f"auto/{source}"] = display(source, 1)
                series[f"manual/{source}"] = display(source, 0)
            for op in ({} if args.calls_only else OPS):
                for encode in ENCODES:
                    series[f"tone/{op}/{encode}"] = display("frame", 0, op, encode)
            for fn in series.values():  # warm-up of everything timed
                fn()
                r.synchronize()
            ms = {k: [] for k in series}
            for _ in range(args.rounds):
                for name, fn in series.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(args.reps):
                        fn()
                    t1.record(stream)
                    t1.synchronize()
                    ms[name].append(t0.elapsed_time(t1) / args.reps)
            exposure, hist, metered = r.display_state()

            def stat(v, floor=None):
                out = dict(ms=round(float(np.median(v)), 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5))
                if floor:
                    out["floor_multiple"] = round(out["ms"] / floor, 2)
                if frame_ms:
                    out["of_c2_frame"] = round(out["ms"] / frame_ms, 5)
                return out

            rec = dict(bounces=bounces)
            if not args.calls_only:
                rec["denoise_it0"] = stat(ms["denoise_it0"])
            for source in args.sources:
                auto, manual = stat(ms[f"auto/{source}"], meter_floor + tone_floor), stat(ms[f"manual/{source}"], tone_floor)
                diff = auto["ms"] - manual["ms"]
                rec[source] = dict(auto=auto, manual=manual,
                                   meter_and_solve=dict(ms=round(diff, 5), floor_multiple=round(diff / meter_floor, 2)))
            if not args.calls_only:
                rec["tone"] = {f"{op}/{encode}": stat(ms[f"tone/{op}/{encode}"], tone_floor)
                               for op in OPS for encode in ENCODES}
            rec["last_state"] = dict(exposure=float(exposure), metered=int(metered), bins_used=int(np.count_nonzero(hist)))
            record["configs"][config] = rec
            print(json.dumps({config: rec}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
