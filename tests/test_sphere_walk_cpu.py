"""CPU check of the sphere walk's block of node steps (csrc/rt_sphere_walk.h).

tests/cpp/sphere_walk_block.cpp includes the header the path kernel compiles and walks every lane
twice in lockstep -- by sphere_walk_block and by the one-node-at-a-time walk (node_visit's logic,
written out in the harness) -- requiring identical (node, pending) after every block and an
identical sequence of visited nodes: BVHs of sphere_bvh.cpp over a random and a clustered sphere
set in the 8 octant layouts with plain and ordered boxes, a one-node tree, an empty tree, NaN box
planes; lanes that enter a block waiting at a leaf or past the end, that reach a leaf or the end at
the first, a middle and the last step of a block; zero direction components, limits below / at /
above a box entry, negative far_t inside and outside -slack; blocks of 1, 3, 4, 5, 6 and 8 steps.
The harness asserts that coverage itself and prints the counts.
"""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rust_gpu_raytracing_amd" / "csrc"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", *extra, f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "sphere_walk_block.cpp"), str(CSRC / "sphere_bvh.cpp"), "-o", str(exe)],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("walk") / "sphere_walk_block")


def test_block_walk_matches_single_steps(harness):
    out = subprocess.run([str(harness), "walk", "1"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("ok walk"), out.stdout[-2000:]
    w = out.stdout.split()
    assert int(w[w.index("octants") + 1], 16) == 0xFF
    # 4 built trees x 160 rays x 6 block sizes x at least 9 lane variants each
    assert int(w[w.index("lanes") + 1]) >= 4 * 160 * 6 * 9 and int(w[w.index("nan_box_visits") + 1]) > 0
    for key, n in (("leaf_at", 3), ("end_at", 3), ("far_neg", 2), ("near_vs_limit", 3)):
        i = w.index(key)
        assert min(int(v) for v in w[i + 1:i + 1 + n]) > 0, (key, w[i + 1:i + 1 + n])
    assert int(w[w.index("enter_waiting") + 1]) > 0 and int(w[w.index("enter_done") + 1]) > 0


def test_harness_detects_broken_walks(harness):
    """A leaf that does not take its skip link, and a waiting lane that moves, must both fail."""
    out = subprocess.run([str(harness), "mutants", "1"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok mutants detected 2"), out.stdout[-2000:]


def test_harness_clean_under_sanitizers(tmp_path):
    """The stand-alone harness (host code, its own main) with AddressSanitizer and UBSan."""
    exe = _build(tmp_path / "sphere_walk_block_san",
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    out = subprocess.run([str(exe), "walk", "2"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok walk"), (out.stdout[-1000:], out.stderr[-3000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
