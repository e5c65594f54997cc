// rt_occlusion_walk.h -- the any-hit search of the occlusion and ambient kernels (occlusion.hip,
// ambient.hip): the seed of a search bounded by t_max, what ends a step of
// it, and how its answer is read. The walk itself is rt_walk.h's, the traversal step
// rt_query_frame.h's.
//
//  * The bound is the search state's seed. Both running bests start at t_max instead of "none":
//    the walk's own acceptance rule (strictly closer than the best; an equal distance only with a
//    lower sweep position / sphere index, and the seed's is 0) then accepts exactly the candidates
//    with t < t_max, and every bound the closest-hit walk has proved for its best hit culls for
//    t_max from the first node.
//  * A search is over the moment a best drops below the seed.
//  * Candidates with a NaN distance (a ray lying exactly in a triangle's plane) are ignored: the
//    walk's nan_hit flag is dropped before phase_end would rerun the sweep for it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

namespace {

// A candidate was accepted: the walk replaces a best only by a strictly closer candidate (the
// seed's tie-break position is 0, which no candidate undercuts), so either best below the seed
// is a primitive accepted at t < bound. Neither is ever NaN (sphere_candidate requires t > 0,
// tri_leaf and coop_leaf_batch route NaN distances to nan_hit).
__device__ __forceinline__ bool occluder_found(const TraceState& ts, float bound) {
    return ts.sph.t < bound || ts.tri.t < bound;
}

// check_triangles (compute_shader.wgsl:422-517) as an any-hit sweep, for scenes whose triangle
// accelerator is off: the first triangle accepted at a non-NaN distance below `bound` decides (the
// sweep's order is free for an any-hit answer). Each test is tri_leaf's.
__device__ __forceinline__ bool sweep_any_triangle(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, f3 inv,
                                                   float bound) {
    const uint32_t n_obj = ka.object_count;
    for (uint32_t oi = 0; oi < n_obj; ++oi) {
        const RtObject& ob = sv.obj[oi];
        if (!ray_in_bounds(o, inv, ob.min_bounds, ob.max_bounds)) continue;
        const uint32_t first_sub = ob.first_sub_object_index;
        const uint32_t n_sub = ob.sub_object_count;
        for (uint32_t i = 0; i < n_sub; ++i) {
            const uint32_t si = min(first_sub + i, ka.sub_object_count - 1u);
            const RtSubObject sub = sv.sub[si];
            if (!ray_in_bounds(o, inv, sub.min_bounds, sub.max_bounds)) continue;
            for (uint32_t j = 0; j < sub.triangle_count; ++j) {
                const uint32_t ti = min(sub.first_triangle_index + j, ka.triangle_count - 1u);
                const TriGeom g = load_tri(ka.triangles, ti);
                const float det = -dot(d, g.cn);
                const float inv_det = 1.0f / det;
                const f3 ao = o - g.a;
                const float dist = dot(ao, g.cn) * inv_det;
                if (!(dist < bound) || dist < 0.0f) continue;  // (a NaN distance never occludes)
                const f3 dao = cross(ao, d);
                const float v = -dot(g.ab, dao) * inv_det;
                if (v < 0.0f) continue;
                const float u = dot(g.ac, dao) * inv_det;
                if (u < 0.0f) continue;
                const float w = 1.0f - u - v;
                if (w < 0.0f) continue;
                return true;
            }
        }
    }
    return false;
}

// trace_begin (rt_walk.h) for an any-hit search bounded by `bound` in (0, F32_MAX]: the bests are
// seeded with the bound, and the search is over (ts.phase == 2) as soon as the brute-force sphere
// set or the sweep finds an occluder.
template <bool kTris>
__device__ __forceinline__ void occlusion_begin(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, float bound,
                                                TraceState& ts) {
    if constexpr (kTris) {
        ts.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // ray_in_bounds (:407-419) needs the IEEE quotient
    } else {
        ts.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    }
    const float a = dot(d, d);
    ts.a4 = 4.0f * a;
    ts.a2 = 2.0f * a;
    ts.sph = SphereHit{bound, 0u, 0u};
    ts.tri = TriHit{bound, 0u, 0u, 0u, false};
    ts.nan_hit = false;
    ts.node = 0;
    ts.pending = kNoLeaf;
    ts.phase = 2;
    // brute-force sphere set, as trace_begin sweeps it
    uint32_t i = 0;
    for (; i + 4u <= ka.sphere_always; i += 4u) test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    if (ka.sphere_always - i >= 2u) {
        test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    } else if (ka.sphere_always - i == 1u) {
        float b;
        const float disc = sphere_disc(sv.sph[i], o, d, ts.a4, b);
        sphere_candidate(disc, b, ts.a2, sv.orig[i], i, ts.sph);
    }
    if (occluder_found(ts, bound)) return;
    uint32_t phase;
    if constexpr (!kTris) {
        phase = 1;
    } else if (!ka.tri_accel) {
        if (sweep_any_triangle(sv, ka, o, d, ts.inv, bound)) {
            ts.tri.t = 0.0f;  // below every bound
            return;
        }
        phase = 1;
    } else {
        phase = ka.tri_nodes != 0 ? 0u : 1u;
    }
    if (phase == 1 && ka.sphere_nodes == 0) return;
    ts.phase = phase;
    phase_setup<kTris>(sv, ka, o, a, phase, ts);
}

// What ends a step of the any-hit search: a lane's search ends when its walks do or when an
// occluder is found, whichever is first. (NaN candidates never occlude: the flag is dropped so
// that phase_end does not sweep for it.)
struct OccluderEnd {
    float bound;
    template <bool kTris>
    __device__ __forceinline__ void step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                         uint32_t& mode) const {
        ts.nan_hit = false;
        phase_end<kTris>(sv, ka, o, d, ts);
        if (ts.phase == 2 || occluder_found(ts, bound)) mode = kLaneDone;
    }
};

}  // namespace
