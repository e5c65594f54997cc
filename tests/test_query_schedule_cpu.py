"""CPU check of the ray queries' launch schedule (csrc/rt_query_schedule.h).

tests/cpp/query_schedule.cpp includes the header rt_queries.cpp compiles and compares query_schedule
with the three formulas the query paths carried before they shared it (closest hit, any hit,
radiance / gather), written out in the harness: counts 1, 63, 64, 65, 777, 10,000, 2^20 + 77 and
2^32 + 5, 4 / 8 / 16 waves per workgroup, 1 / 256 / 2,048 resident workgroups, the four cap sets.
Per case: equal (blocks, first chunk, dealt chunk), every chunk a multiple of 64 and at least 64,
blocks >= 1, and blocks x waves x 64 >= min(count, resident x waves x 64).
"""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rust_gpu_raytracing_amd" / "csrc"
CASES = 4 * 8 * 3 * 3


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "query_schedule.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("schedule") / "query_schedule")


def test_schedule_matches_the_three_formulas(harness):
    out = subprocess.run([str(harness)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("ok schedule"), out.stdout[-2000:]
    w = out.stdout.split()
    assert int(w[w.index("cases") + 1]) == CASES
    assert int(w[w.index("dealt") + 1]) > 0 and int(w[w.index("first_only") + 1]) > 0


def test_harness_clean_under_sanitizers(tmp_path):
    """The stand-alone harness (host code, its own main) with AddressSanitizer and UBSan."""
    exe = _build(tmp_path / "query_schedule_san",
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok schedule"), (out.stdout[-1000:], out.stderr[-3000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
