"""The oracle's texture and env-map fetch against the closed form, and the sensitivity of the
GPU suite's full-path inputs (tests/test_gpu_texture_sampling.py) to a wrong fetch.

Census: both census scenes of tests/texel_probe_scene.py through the oracle with bounces = 1, one
frame. Every ray's RGBA must equal its expected texel decoded through ``oracle_srgb_table`` (alpha
f32(a) / f32(255)), bit for bit, with one segment per ray and every texel of the layer fetched. No
ray is left out.

Guard: for every input of ``PROBE_INPUTS`` the oracle's accumulation must differ from the true
image in at least 5% of the pixels under each of four mutations of the input -- a condition on the
inputs (a kernel with that error would differ from the oracle in as many pixels), not a
measurement of any kernel. References are computed once and shared, never modified.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from tests import texel_probe_scene as T
from tests.test_gpu_parity import oracle_frames
from tests.test_gpu_radiance import oracle_radiance


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def srgb_table(O):
    srgb = np.zeros(256, np.float32)
    O.lib().oracle_srgb_table(srgb.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return srgb


@functools.lru_cache(maxsize=None)
def census(kind, shape, layer):
    """The census (never modified) with the closed-form radiance per ray."""
    from oracle import oracle as O

    O.build()
    c = (T.floor_census if kind == "floor" else T.sphere_census)(shape, layer)
    want = T.decode(c.texels, srgb_table(O))
    for a in (c.rays, c.texels, c.coords, want):
        a.setflags(write=False)
    return c, want


def assert_census_complete(c):
    """Every texel of the (clamped) layer is aimed at, by the same number of rays."""
    layers, h, w = c.scene.textures.shape[:3]
    assert (c.coords[:, 0] == min(int(c.scene.materials["texture_index"][0]), layers - 1)).all()
    counts = np.zeros((h, w), np.int64)
    np.add.at(counts, (c.coords[:, 1], c.coords[:, 2]), 1)
    assert counts.min() == counts.max() >= 1


CENSUS_CASES = [(shape, layer) for shape in T.CENSUS_SHAPES for layer in T.census_layers(shape)]
CENSUS_IDS = ["%dx%dx%d-layer%d" % (*shape, layer) for shape, layer in CENSUS_CASES]


def probe_id(value):
    return "x".join(map(str, value)) if isinstance(value, tuple) else None


@pytest.mark.parametrize("shape,layer", CENSUS_CASES, ids=CENSUS_IDS)
@pytest.mark.parametrize("kind", ["floor", "sphere"])
def test_census_matches_closed_form(oracle_lib, kind, shape, layer):
    c, want = census(kind, shape, layer)
    assert_census_complete(c)
    n = c.rays.shape[0]
    got, segs = oracle_radiance(oracle_lib, c.scene, c.rays, np.arange(n, dtype=np.uint32), 1, 1, 1)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], c.coords[bad[:5]], got[bad[:3]], want[bad[:3]])
    assert (segs == 1).all()
    # the fetched texels, recovered from the results: all of the layer's (the values are distinct)
    assert np.unique(bits(got), axis=0).shape[0] == shape[1] * shape[2]


def test_floor_census_through_the_frame(oracle_lib):
    """The camera-ray form of the floor census (one origin, rays aimed at the sub-cell centres),
    which the GPU suite renders as a frame: the same closed form."""
    for shape in T.CENSUS_SHAPES:
        c, want = census("floor", shape, shape[0])
        scene, rays = T.floor_frame(c)
        acc, _, n = oracle_frames(oracle_lib, scene, 1, 1, rays)
        assert n == rays.shape[0]
        assert np.array_equal(bits(acc).reshape(-1, 4)[:want.shape[0]], bits(want))


# ------------------------------------------------------------------------------------ the guard
@functools.lru_cache(maxsize=None)
def probe(seed, with_tris, tex_shape, env_shape, spp=1):
    """(scene, camera rays, the oracle's (accumulation, RGBA8, rays)) of a probe input; never modified."""
    from oracle import oracle as O

    O.build()
    scene, rays = T.probe_scene(seed, T.PROBE_W, T.PROBE_H, tex_shape, env_shape, with_tris)
    ref = oracle_frames(O, scene, T.PROBE_BOUNCES, T.PROBE_FRAMES, rays, compute_per_frame=spp)
    for a in ref[:2]:
        a.setflags(write=False)
    return scene, rays, ref


def mutations(scene):
    """name -> the scene as a kernel with that error would see it."""
    tex, env = scene.textures, scene.environment_map
    layers, h, w = tex.shape[:3]
    eh, ew = env.shape[:2]
    mats = scene.materials.copy()
    beyond = T.out_of_range_materials(scene)
    assert {layers, layers + 2, 0xFFFFFFFF} <= set(int(t) for t in mats["texture_index"][beyond])
    mats["texture_index"][beyond] = 0
    return {
        "texture_h_w_exchanged": dataclasses.replace(scene, textures=tex.reshape(layers, w, h, 4)),
        "texture_rolled_in_x": dataclasses.replace(scene, textures=np.ascontiguousarray(np.roll(tex, 1, axis=2))),
        "layer_clamp_to_0": dataclasses.replace(scene, materials=mats),
        # (a square map reinterpreted is itself: there the mutation is the transposed map, x for y)
        "env_h_w_exchanged": dataclasses.replace(
            scene,
            environment_map=env.reshape(ew, eh, 4) if eh != ew else np.ascontiguousarray(env.transpose(1, 0, 2))),
    }


def changed_share(oracle_lib, scene, rays, ref):
    acc, _, _ = oracle_frames(oracle_lib, scene, T.PROBE_BOUNCES, T.PROBE_FRAMES, rays)
    return float((bits(acc) != bits(ref[0])).any(axis=-1).mean())


@pytest.mark.parametrize("seed,with_tris,tex_shape,env_shape", T.PROBE_INPUTS, ids=probe_id)
def test_probe_inputs_are_sensitive(oracle_lib, seed, with_tris, tex_shape, env_shape):
    scene, rays, ref = probe(seed, with_tris, tex_shape, env_shape)
    shares = {name: changed_share(oracle_lib, m, rays, ref) for name, m in mutations(scene).items()}
    print(seed, with_tris, tex_shape, env_shape, {k: round(v, 3) for k, v in shares.items()})
    for name, share in shares.items():
        assert share >= 0.05, (name, share)
    if with_tris:  # NaN / +-inf uv on the flat quads: real bounds there change the image
        flat = changed_share(oracle_lib, T.unflattened(scene), rays, ref)
        print("flat bounds widened", round(flat, 3))
        assert flat > 0
