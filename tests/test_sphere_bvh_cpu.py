"""CPU proof-by-test of the sphere BVH's exact culling (tests/cpp/bvh_exactness.cpp).

The kernel's traversal logic, restated in C++ with the same f32 operation order,
must return exactly the sphere and distance of the reference's brute-force scan
(compute_shader.wgsl:355-404, first-wins ties) on adversarial rays: camera rays,
rays leaving sphere surfaces (+-n*1e-4, tangent), far-away origins, axis-parallel
and near-zero direction components, non-unit directions, duplicate spheres.
It also shows the bounds matter: with the lateral box inflation cut to 1/100 of
sphere_cull_bounds' value it finds a divergence, so the test is not vacuous
(at 1/10 it still passes: the bound carries a ~10-100x safety factor here).
"""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rust_gpu_raytracing_amd import buffers as B
from tests import ray_domain as RD

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bvh") / "bvh_exactness"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'rust_gpu_raytracing_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "bvh_exactness.cpp"),
                    str(ROOT / "rust_gpu_raytracing_amd" / "csrc" / "sphere_bvh.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bvh_matches_brute_force(harness, seed):
    out = subprocess.run([str(harness), "400000", str(seed)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout
    _, n, hits, avg_tests, n_spheres, _, ordered = out.stdout.split()
    assert float(avg_tests) < 0.1 * int(n_spheres)  # the culling actually culls
    assert ordered == "1"  # the sphere-only kernels' box-ordered layouts (slab_hit_ordered) were walked


def test_bvh_unordered_boxes(harness):
    """The octant layouts with bmin/bmax kept (scenes with objects, RT_SPHERE_BOX_ORDER=0) and slab_hit."""
    env = dict(os.environ, UNORDERED_BOXES="1")
    out = subprocess.run([str(harness), "200000", "5"], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.startswith("ok") and out.stdout.split()[-1] == "0", out.stdout


def test_bvh_with_one_ulp_reciprocals(harness):
    """Sphere-only kernels take 1/d from v_rcp_f32 (<= 1 ulp); the culling stays exact
    with every component of 1/d one ulp off in either direction."""
    env = dict(os.environ, INV_ULP="1")
    out = subprocess.run([str(harness), "400000", "4"], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout


def test_margin_is_load_bearing(harness):
    env = dict(os.environ, LAT_SCALE="0.01")
    out = subprocess.run([str(harness), "1000000", "3"], capture_output=True, text=True, env=env)
    assert out.returncode == 1 and "MISMATCH" in out.stdout


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bvh_adversarial_derived_bound(harness, seed):
    """The derived bound of rt_bvh_slab.h (gamma_n constants) on the adversarial
    sets VERDICT r04 asked for: BVH spheres with radii 1e-3..1e3, rays tangent to a sphere in exact
    arithmetic (the reference's discriminant within a few ulp of 0 on most of them) from 1..1e6
    radii away, nudged across the tangent by a few ulp, rays aimed at centres from far away, and
    |d| from 1e-12 (below the bound's range: no culling) to 1e6. Exact on every ray."""
    out = subprocess.run([str(harness), "300000", str(seed), "adv"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok adversarial"), out.stdout
    words = out.stdout.split()
    n, near_zero = int(words[2]), int(words[-1])
    assert near_zero > n // 2  # most rays do sit at a near-zero discriminant


def test_adversarial_bound_is_load_bearing(harness):
    """On the same sets, the lateral bound cut to 0.03x finds a ray the walk gets wrong: the
    adversarial rays reach within ~10-30x of the derived bound."""
    env = dict(os.environ, LAT_SCALE="0.03")
    out = subprocess.run([str(harness), "300000", "1", "adv"], capture_output=True, text=True, env=env)
    assert out.returncode == 1 and "MISMATCH" in out.stdout


@pytest.mark.parametrize("inv_ulp", [False, True])
@pytest.mark.parametrize("name", ["mixed_components", "far_origins"])
def test_ray_domain_sets(harness, tmp_path, name, inv_ulp):
    """The harness's RTIOW-like scene (dumped, then replayed) on two in-domain sets of
    tests/ray_domain.py: components scaled down to denormals and signed zeros with |d| from
    1.01e-5 to 0.99e5, and origins 1e3, 1e5 and 1e7 from the spheres; with exact reciprocals and
    with every component of 1/d one ulp off (the sphere-only kernels' v_rcp_f32). The length sweep
    itself is test_bvh_adversarial_derived_bound's."""
    sph = tmp_path / "spheres.bin"
    subprocess.run([str(harness), "0", "6", "dump", str(sph)], check=True)
    spheres = np.fromfile(sph, B.SPHERE)
    assert spheres.shape[0] > 400
    geo = RD.geometry(2, spheres)
    rays = RD.ray_set(name, 70 + RD.SETS.index(name), 20000, geo)
    rays.tofile(tmp_path / "rays.f32")
    env = dict(os.environ, INV_ULP="1") if inv_ulp else None
    out = subprocess.run([str(harness), "--replay", str(tmp_path / "rays.f32"), str(sph)], capture_output=True,
                         text=True, env=env)
    assert out.returncode == 0 and out.stdout.startswith("replay rays 20000 mismatches 0 "), out.stdout
    accepted = float(out.stdout.splitlines()[0].split("accepted")[1])
    assert accepted > 0.25  # (candidates accepted per ray: the set does hit spheres)
