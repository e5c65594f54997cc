"""bench.py's plain run: the result line's contract, --dump-outputs and what --full keeps out.

One small run of the benchmark (72x40, 3 timed steps): the line must carry the headline
fields and none of the secondary measurements, and the dumped arrays must be exactly what
a Renderer holds after the same number of frames from a fresh accumulation -- whatever
the warmup and settle frames before the timed steps were.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
W, H, STEPS = 72, 40, 3


@pytest.mark.gpu
def test_gpu_bench_plain_run_dumps_the_timed_steps_outputs(gpu, tmp_path):
    from rust_gpu_raytracing_amd import Renderer
    from rust_gpu_raytracing_amd.scene import build_config

    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
           "--settle-ms", "5", "--width", str(W), "--height", str(H), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["unit"] == "Mray/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["launches"] == 1  # the 3 steps ran as one 3-frame launch
    # the secondary measurements are --full's
    assert not any(k.startswith("ms_per_step_") for k in line) and "cpu_baseline" not in line and "weak" not in line

    scene, bounces = build_config("c2_rtiow", width=W, height=H)
    with Renderer(scene) as r:
        for _ in range(STEPS):
            r.compute_frame(bounces)
        acc, packed, rays = r.read_accumulation(), r.read_output(), r.ray_count()
    assert round(line["config"]["rays_per_step"] * STEPS) == rays
    got_acc = np.load(tmp_path / "out" / "accumulation.npy")
    got_rgba = np.load(tmp_path / "out" / "output_rgba8.npy")
    assert got_acc.dtype == np.float32 and got_rgba.dtype == np.float32
    assert got_acc.shape == got_rgba.shape == (H, W, 4)
    assert np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(got_rgba, packed.view(np.uint8).reshape(H, W, 4).astype(np.float32))


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    """Above DUMP_BYTES_MAX the dump keeps one seeded sample of pixels, the same for both arrays."""
    import bench

    class Stub:  # 1920x1080: 2 x 33 MB in full
        height, width = 1080, 1920

        def read_accumulation(self):
            return np.arange(self.height * self.width * 4, dtype=np.float32).reshape(self.height, self.width, 4)

        def read_output(self):
            return np.arange(self.height * self.width, dtype=np.uint32).reshape(self.height, self.width)

    bench.dump_outputs(tmp_path / "out", Stub())
    acc, rgba = np.load(tmp_path / "out" / "accumulation.npy"), np.load(tmp_path / "out" / "output_rgba8.npy")
    assert sum(f.stat().st_size for f in (tmp_path / "out").iterdir()) <= 64_000_000
    n = bench.DUMP_BYTES_MAX // 32
    assert acc.dtype == rgba.dtype == np.float32 and acc.shape == rgba.shape == (n, 4)
    px = (acc[:, 0] / 4).astype(np.int64)  # the stub's accumulation names its pixel (exact below 2^24)
    assert np.all(np.diff(px) > 0) and px[-1] < 1080 * 1920
    word = (rgba @ np.array([1.0, 256.0, 65536.0, 16777216.0])).astype(np.int64)
    assert np.array_equal(word, px)
    assert np.array_equal(px, np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(1080 * 1920, n, replace=False)))
