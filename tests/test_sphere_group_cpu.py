"""CPU check of the sphere group test's root passes (csrc/rt_sphere_roots.h).

tests/cpp/sphere_group_select.cpp includes the header the kernels compile and checks, bit for
bit in (t, original index, slot), the candidate-compacted selection against the four positional
arms and against a brute lexicographic (t, index) minimum: every candidate mask, equal distances
with the indices in every order, roots at and behind the origin, zero / NaN / infinite / tiny
discriminants, an incoming best below, at and above every candidate, and 10^6 random groups --
in both pass layouts of the header (RT_SPHERE_ROOTS_FORM 0 and 1).

The cluster scene (tests/sphere_cluster_scene.py, shared with tests/test_gpu_sphere_group.py) is
walked with the group test at the BVH leaves: the walk equals the reference's brute-force scan on
every ray, and the leaf groups the rays visit do hold 2, 3 and 4 candidates (so the GPU test on
the same scene and rays exercises every pass) -- which a builder that split the clusters over
several leaves would no longer give.
"""
import subprocess
from pathlib import Path

import pytest

from tests.sphere_cluster_scene import cluster_rays, cluster_spheres

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rust_gpu_raytracing_amd" / "csrc"


@pytest.fixture(scope="module", params=[0, 1], ids=["low_high_middle", "mask_loop"])
def harness(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("roots") / f"sphere_group_select_{request.param}"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", f"-DRT_SPHERE_ROOTS_FORM={request.param}",
                    f"-I{ROOT / 'include'}", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "sphere_group_select.cpp"),
                    str(CSRC / "sphere_bvh.cpp"), "-o", str(exe)], check=True)
    return exe


def test_selection_matches_arms_and_brute_minimum(harness):
    out = subprocess.run([str(harness), "select", "1000000", "1"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok select"), out.stdout
    w = out.stdout.split()
    groups, masks, by_count = int(w[3]), int(w[5], 16), [int(v) for v in w[7:12]]
    assert masks == 0xFFFF  # all 16 candidate masks were met
    assert groups > 1_000_000 and min(by_count) > 10_000


def test_cluster_scene_walk(harness, tmp_path):
    """24 clusters + ground, 91 spheres, 4,000 rays. (Reference run with the builder of the
    day: 240 / 747 / 573 / 2053 visited leaf groups with 1 / 2 / 3 / 4 candidates, 0 mismatches.)"""
    spheres, rays = cluster_spheres(), cluster_rays()
    assert spheres.shape == (91,) and rays.shape == (4000, 6)
    (tmp_path / "spheres.bin").write_bytes(spheres.tobytes())
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    out = subprocess.run([str(harness), "scene", str(tmp_path / "spheres.bin"), str(tmp_path / "rays.bin")],
                         capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("ok scene"), out.stdout
    w = out.stdout.split()
    assert int(w[3]) == 4000 and int(w[w.index("always") + 1]) == 1  # the ground: the lone brute-force sphere
    by_count = [int(v) for v in w[w.index("by_count") + 1:w.index("by_count") + 6]]
    assert min(by_count[2:]) >= 200, by_count
    assert int(w[-1]) == 0
