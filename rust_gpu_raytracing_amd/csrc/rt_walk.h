// rt_walk.h -- the resumable closest-hit search of one ray, shared by the kernels that walk the
// accelerators per lane (pathtrace.hip: the persistent path kernel and the primary pre-pass;
// query.hip: the ray-query kernel): trace_begin, then node_step / leaf_step / coop_leaf_batch with
// phase_end after each until ts.phase == 2, then trace_end (rt_path_common.h). Any (o, d) is a
// valid input; which steps a wave runs when is the kernel's choice and does not change the result
// (the lexicographic minimum over the tested primitives).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_path_common.h"

#pragma clang fp contract(off)

using namespace rtk;

namespace {

// Slab constants and depth bounds of a BVH walk. The triangle walk culls by
// box, and by distance when pruning is on (tri_limit), with no slack.
template <bool kTris>
__device__ __forceinline__ void phase_setup(const SceneView& sv, const KernelArgs& ka, f3 o, float a, uint32_t phase,
                                            TraceState& ts) {
    const float r = sqrt_up(dot(o, o));  // |o| sizes the margins only: an upper bound will do
    float m;
    if (phase == 0) {
        m = kTriMarginScale * (r + sv.tri_extent) + 1.0e-30f;
        ts.slack = 0.0f;
    } else {
        sphere_cull_bounds(r, ka.sphere_extent, ka.sphere_rmin, ka.sphere_rmax, __builtin_amdgcn_rsqf(a), m,
                           ts.slack);
    }
    ts.slab = slab_ray(o.x, o.y, o.z, ts.inv.x, ts.inv.y, ts.inv.z, m);
    ts.limit = phase == 0 ? __builtin_inff() : prune_limit(ts);
    if (kTris && phase == 0) {  // the accelerator layout ordered for this ray's direction octant (global walks)
        const uint32_t oct = (__float_as_uint(ts.inv.x) >> 31) | ((__float_as_uint(ts.inv.y) >> 31) << 1) |
                             ((__float_as_uint(ts.inv.z) >> 31) << 2);
        ts.node = oct * ka.tri_octant_stride;
    }
    if (phase == 1) {  // the sphere BVH layout ordered for this ray's direction octant (sphere_bvh.h)
        const uint32_t oct = (__float_as_uint(ts.inv.x) >> 31) | ((__float_as_uint(ts.inv.y) >> 31) << 1) |
                             ((__float_as_uint(ts.inv.z) >> 31) << 2);
        ts.node = oct * ka.sphere_octant_stride;
        // layouts storing (near, far) corners (sphere-only scenes, set by the host):
        // the plane constants paired the same way, so node_step can skip slab_hit's
        // min/max (rt_bvh_slab.h)
        if constexpr (!kTris)
            if (ka.sphere_boxes_ordered) slab_pair_by_octant(ts.slab);
    }
}

// kTris: the scene has objects (triangles); false compiles the triangle side out.
template <bool kTris>
__device__ __forceinline__ void trace_begin(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts) {
    if constexpr (kTris) {
        ts.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // ray_in_bounds (:407-419) needs the IEEE quotient
    } else {
        // sphere-only scenes use 1/d only in the culling slab test, whose error
        // budget (rt_bvh_slab.h: 16u X for rounding, orders under the margin)
        // covers v_rcp_f32's 1 ulp; the sign (the layout octant) and +-inf for
        // a zero component are exact
        ts.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    }
    const float a = dot(d, d);
    ts.a4 = 4.0f * a;
    ts.a2 = 2.0f * a;
    ts.sph = SphereHit{kF32Max, 0u, 0u};
    ts.tri = TriHit{kF32Max, 0u, 0u, 0u, false};
    ts.nan_hit = false;
    ts.node = 0;
    ts.pending = kNoLeaf;
    // brute-force sphere set: wave-uniform sweep over groups of 4, then the rest
    // one by one (a sphere's own test is exact, so the visiting order is free)
    // (the slots after the set up to the next group boundary are NaN padding:
    // a remainder of 2-3 spheres takes one group, a lone sphere a single test)
    uint32_t i = 0;
    for (; i + 4u <= ka.sphere_always; i += 4u) test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    if (ka.sphere_always - i >= 2u) {
        test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    } else if (ka.sphere_always - i == 1u) {
        float b;
        const float disc = sphere_disc(sv.sph[i], o, d, ts.a4, b);
        sphere_candidate(disc, b, ts.a2, sv.orig[i], i, ts.sph);
    }
    if constexpr (!kTris) {
        ts.phase = 1;
    } else if (!ka.tri_accel) {
        ts.tri = sweep_triangles(sv, ka, o, d);
        ts.phase = 1;
    } else {
        ts.phase = ka.tri_nodes != 0 ? 0u : 1u;
    }
    if (ts.phase == 1 && ka.sphere_nodes == 0) ts.phase = 2;
    phase_setup<kTris>(sv, ka, o, a, ts.phase, ts);
}

// The lane's index in its wave, computed where it is used: an opaque value, so that the compiler
// does not hoist it (and what is derived from it) out of the traversal loop into a register
// held across every node step.
__device__ __forceinline__ uint32_t lane_id_here() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// Ends the current BVH walk once its nodes are exhausted and no leaf is pending.
template <bool kTris>
__device__ __forceinline__ void phase_end(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts) {
    if (ts.pending != kNoLeaf) return;
    if (kTris && ts.phase == 0) {
        if (ts.node < ka.tri_nodes) return;
#ifdef RT_DIAG_TAIL
        if (ts.nan_hit) atomicAdd(ka.diag + 6, 1ull);
#endif
        if (ts.nan_hit) ts.tri = sweep_triangles(sv, ka, o, d);  // measure-zero case: the sweep decides
        ts.node = 0;
        ts.phase = ka.sphere_nodes != 0 ? 1u : 2u;
        phase_setup<kTris>(sv, ka, o, ts.a2 * 0.5f, 1, ts);
    } else if (ts.node >= ka.sphere_nodes) {
        ts.phase = 2;
    }
}

// Advances the walk by one BVH node. A reached leaf is not tested here but
// deferred (ts.pending) and the walk goes on past it: the wave tests leaves in
// batches (leaf_step), so the leaf body -- two box tests and up to 7 triangle
// tests with their global loads, or a sphere group -- runs for many lanes at
// once instead of for the few lanes that sit on a leaf in a given step. A lane
// that reaches a second leaf while one is deferred stays on it until the batch.
// Testing a leaf late only delays the pruning distance it would set: the result
// is the lexicographic minimum over the tested primitives either way.
template <bool kTris>
constexpr bool kDeferLeaves = kTris;
// Sphere-only scenes: a lane that reaches a leaf stops walking, and the group tests of the lanes
// waiting at a leaf run together after a block of the wave's unrolled node steps (kTravUnroll),
// once at least kBlockLeafShare eighths of the traversing lanes wait, instead of inside each node
// step for the few lanes at a leaf in that step. The lane resumes with its pruning distance
// updated, so it visits the nodes the on-the-spot test would, in the same order (C2 0.2820 ->
// 0.2481 ms per frame in one process; walking on past the leaf until a second one was slower;
// DESIGN §5.2).
template <bool kTris>
constexpr bool kBlockLeaves = !kTris;
#ifndef RT_BLOCK_LEAF_SHARE
#define RT_BLOCK_LEAF_SHARE 3
#endif
constexpr uint32_t kBlockLeafShare = RT_BLOCK_LEAF_SHARE;
// Node steps per wave-wide check of the traversal loop (the ballots of the
// threshold and leaf-batch tests, exec-mask updates). Lanes that finish inside
// the group idle for its remaining steps; the visit order is unchanged.
// Measured (1 -> 3): C2 -2.8%, C3 -10%, C4 -11%, C5 -7%. Round 4, per accelerator placement
// (profiles/r04/r04_z): global-memory walks 3 -> 4 / 5 / 6: C5 -4.0% / -4.3% / -1.6%;
// LDS-resident walks 3 -> 2: C3 -1.2%, C4 (4K) +0.5%. Sphere walks, with the block group tests
// (round 6, profiles/r06/r06l, r06o, r06p): blocks of 4 with the tests once 3/8 of the lanes wait,
// C2 0.2481 ms per frame; 3 / 5 / 6 steps 0.2522 / 0.2503 / 0.2503; every block tested (no
// share) at 3 / 4 / 6 / 8 / 12 steps 0.2675 / 0.2580 / 0.2575 / 0.2614 / 0.2658.
// Again with the group test's roots evaluated per candidate (rt_sphere_roots.h;
// profiles/sphere_roots/ab_c2_sweep.json, one process, 9 rounds, spreads <= 0.0023):
//   blocks of 4, share 3/8 (kept)   C2 0.2383 ms per frame
//   blocks of 3 / 5                 0.2394 / 0.2428
//   share 2/8 / 4/8                 0.2382 / 0.2393
// No setting beats the defaults by more than the 1% band (-DRT_SPHERE_TRAV_UNROLL=N,
// -DRT_BLOCK_LEAF_SHARE=N build the variants).
#ifndef RT_SPHERE_TRAV_UNROLL
#define RT_SPHERE_TRAV_UNROLL 4
#endif
template <int kMode, bool kTris>
constexpr int kTravUnroll = !kTris ? RT_SPHERE_TRAV_UNROLL : kMode <= 1 ? 5 : 3;
// Triangle walks: the leaf batch runs after the block's node steps in the same iteration (round 6)
// instead of in an iteration of its own in which the walking lanes idle: the LDS-resident walk
// (mode 2, C3 0.2645 -> 0.2463, C4 1.539 -> 1.416 ms per frame in one process with blocks of 3
// steps; 2 / 4 / 5 steps: C3 0.2492 / 0.2478 / 0.2527, C4 1.460 / 1.413 / 1.437; shares of
// 5/8-8/8 around the default 6/8 no better; profiles/r06/r06r-r06t).
// The walks from global memory keep their batches apart: fusing the cooperative batch the same
// way measured C5 +2.3% (profiles/r06/r06u).
template <int kMode, bool kTris>
constexpr bool kFusedLeaves = kTris && kMode == 2;

// Decoupled drain (see the kernel's step 4): triangle scenes whose accelerator
// is read from global memory (LDS modes 0 and 1).
template <int kMode, bool kTris>
constexpr bool kDrainDecouple = kTris && kMode < 2;

// Walks that read leaf certificates: from global memory only (see tri_leaf).
template <int kMode>
constexpr bool kCertWalk = kMode <= 1;

// A 16-B quantized node decoded (tri_qnode.h): the box exactly (a superset of the 32-B node's
// box), lo.w = the skip link (a leaf's: node + 1, or the end), hi.w = the leaf record or none.
__device__ __forceinline__ void qnode_decode(const SceneView& sv, uint4 q, uint32_t node, float4& lo, float4& hi) {
    lo = make_float4(fmaf((float)(q.x & 0xffffu), sv.qsx, sv.qox), fmaf((float)(q.x >> 16), sv.qsy, sv.qoy),
                     fmaf((float)(q.y & 0xffffu), sv.qsz, sv.qoz), 0.0f);
    hi = make_float4(fmaf((float)(q.y >> 16), sv.qsx, sv.qox), fmaf((float)(q.z & 0xffffu), sv.qsy, sv.qoy),
                     fmaf((float)(q.z >> 16), sv.qsz, sv.qoz), 0.0f);
    const bool is_leaf = (q.w & 0x80000000u) != 0u;
    // a leaf's skip link is node + 1 (pre-order), or the end for a layout's last leaf
    lo.w = __uint_as_float(is_leaf ? ((q.w & kTriQLastLeaf) ? kTriWalkEnd : node + 1u) : q.w);
    hi.w = __uint_as_float(is_leaf ? (q.w & 0xffffffu) : 0xffffffffu);
}

// One node's visit, given its box and links: the box test, the deferred leaf or the sphere
// group, the next node.
template <bool kTris, bool kCert>
__device__ __forceinline__ void node_visit(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                           bool tri, float4 lo, float4 hi) {
    float near_t, far_t;
    if (!kTris && ka.sphere_boxes_ordered)  // (near, far) corners: no min/max per axis (6 VALU per node step)
        slab_hit_ordered(ts.slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(ts.slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    // enters the inflated box and is not wholly behind the origin; on the sphere
    // side also not beyond the best sphere or the triangle hit (a sphere wins
    // only when strictly closer, :347); ts.slack / ts.limit are 0 / inf on the
    // triangle side
    const bool hit = near_t <= far_t && far_t >= -ts.slack && near_t <= ts.limit;
    const uint32_t leaf = __float_as_uint(hi.w);
    uint32_t skip = 0u;
    if constexpr (kTris && kCert) {
        // certified pruning: a leaf whose box is entered beyond the best triangle hit records
        // the gap of its box beyond that hit, for the leaf batch's certificate test
        if (tri && hit && leaf != 0xffffffffu && ka.tri_leafcert && near_t > ts.tri.t && ts.tri.t != kF32Max &&
            ts.pending == kNoLeaf) {
            const float tbs = ts.tri.t * (1.0f + 0x1p-20f);
            const SlabRay& sr = ts.slab;
            const float gx = (fminf(fmaf(lo.x, sr.ix, sr.lx), fmaf(hi.x, sr.ix, sr.hx)) - tbs) * fabsf(d.x);
            const float gy = (fminf(fmaf(lo.y, sr.iy, sr.ly), fmaf(hi.y, sr.iy, sr.hy)) - tbs) * fabsf(d.y);
            const float gz = (fminf(fmaf(lo.z, sr.iz, sr.lz), fmaf(hi.z, sr.iz, sr.hz)) - tbs) * fabsf(d.z);
            ts.cert_gap = fmaxf(fmaxf(gx, gy), gz) * (1.0f - 0x1p-20f);
            skip = ts.cert_gap > 0.0f ? 1u : 0u;  // (bit 24 of pending: test deferred)
        }
    }
    const bool at_leaf = hit && leaf != 0xffffffffu;
#ifdef RT_DIAG
    if constexpr (!kDeferLeaves<kTris>) {  // node steps and the sphere-group tests inside them, with their lanes
        const uint64_t act = __ballot(true), lf = __ballot(at_leaf);
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(act)) {
            atomicAdd(ka.diag + 22, 1ull);
            atomicAdd(ka.diag + 23, (unsigned long long)__popcll(act));
            if (lf) {
                atomicAdd(ka.diag + 24, 1ull);
                atomicAdd(ka.diag + 25, (unsigned long long)__popcll(lf));
            }
        }
    }
#endif
    if (at_leaf && !kDeferLeaves<kTris> && !kBlockLeaves<kTris>) {
        test_sphere_group(sv, leaf & 0xffffffu, o, d, ts.a4, ts.a2, ts.sph);
        ts.limit = prune_limit(ts);
    } else if (at_leaf) {
        if (ts.pending != kNoLeaf) return;  // blocked until the batch tests the deferred leaf
        ts.pending = (leaf & 0xffffffu) | (skip << 24);
    }
    ts.node = (hit && !at_leaf) ? ts.node + 1u : __float_as_uint(lo.w);
}

// kCert: the walk records leaf-certificate gaps (node_visit) when ka.tri_leafcert is set.
template <bool kTris, bool kCert = true>
__device__ __forceinline__ void node_step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts) {
    const bool tri = kTris && ts.phase == 0;
    if (kDeferLeaves<kTris> && ts.node >= (tri ? ka.tri_nodes : ka.sphere_nodes))
        return;  // walk over, a leaf still deferred
    if (kBlockLeaves<kTris> && ts.pending != kNoLeaf) return;  // waits for the block's group tests
    float4 lo, hi;
    if (kTris && tri && sv.tri_q) {
        qnode_decode(sv, sv.tri_q[ts.node], ts.node, lo, hi);
    } else {
        const float4* nodes = tri ? sv.tri_nodes : sv.nodes;
        lo = nodes[2u * ts.node];
        hi = nodes[2u * ts.node + 1u];
    }
    node_visit<kTris, kCert>(sv, ka, o, d, ts, tri, lo, hi);
}

template <bool kTris, bool kLazySub = false>
__device__ __forceinline__ void leaf_step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts) {
    if (kTris && ts.phase == 0) {
        tri_leaf<kLazySub>(sv, ka, o, d, ts, ts.pending);
        ts.limit = tri_limit(sv, ka, o, ts);
    } else {
        test_sphere_group(sv, ts.pending, o, d, ts.a4, ts.a2, ts.sph);
        ts.limit = prune_limit(ts);
    }
    ts.pending = kNoLeaf;
}

// ---- Cooperative leaf batches (walks from global memory) --------------------
//
// A per-lane leaf test loads its up-to-7 triangles with three lane-distinct 16-B loads each:
// 21 L1 tag lookups per leaf, and the L1's tag rate (about one line per cycle per CU) is what
// the global-memory walk is bound by. Here a leaf batch tests the wave's
// pending leaves together instead: the pending lanes publish their ray and leaf in a per-wave
// LDS scratch, and each round 8 lanes per leaf -- lane j the leaf's triangle j -- load the
// leaf's triangle block (KernelArgs::tri_leaftris: piece p of slots 0..7 in one 128-B line),
// so the 21 loads become 3 lines shared by 8 lanes, and 8 leaves are tested per round on all
// 64 lanes. Each lane runs the reference's test (compute_shader.wgsl:445-500) with the same
// f32 operations as tri_leaf; the group's candidates are reduced to the lexicographic minimum
// of (distance, sweep position) and an "any NaN distance" flag, which the leaf's lane then
// merges exactly as tri_leaf's sequential loop would: the sub-object box test (:441) runs if a
// candidate beats the lane's best hit or has a NaN distance; if it fails, nothing of the leaf
// counts; else the NaN flag and the best candidate are taken. (Within a leaf the sequential
// loop's result is that minimum: a candidate's test does not depend on the running best other
// than through "distance < best", which is the minimum's own comparison.)
template <int kMode, bool kTris>
constexpr bool kCoopLeaves = kTris && kMode <= 1;

// LDS written by some lanes of a wave and read by others: the wave's LDS operations complete in
// order, so only the compiler must not move them across this point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One step of the 8-lane (distance, sequence) minimum: the candidate of lane (DPP `ctrl`).
template <int kCtrl>
__device__ __forceinline__ void coop_min_step(float& cd, uint32_t& cs, uint32_t& ct) {
    const float od = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(cd), kCtrl, 0xf, 0xf, false));
    const uint32_t os = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cs, kCtrl, 0xf, 0xf, false);
    const uint32_t ot = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ct, kCtrl, 0xf, 0xf, false);
    const bool take = od < cd || (od == cd && os < cs);
    cd = take ? od : cd;
    cs = take ? os : cs;
    ct = take ? ot : ct;
}

// `active`: this lane traverses and holds a deferred leaf (a triangle leaf, or a sphere group in
// the sphere phase, which is tested on the spot as in leaf_step). Wave-uniform call; the scratch
// is this wave's 64 x 3 float4 of LDS at ka.lds_leafbatch_offset.
__device__ __forceinline__ void coop_leaf_batch(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                                bool active, unsigned char* lds) {
    bool want = false;
    uint32_t prim = 0u, range = 0u, seq0 = 0u, obj = 0u, sub = 0u;
    if (active) {
        if (ts.phase == 0) {
            prim = ts.pending & 0xffffffu;
            uint32_t skip = 0u;
            if ((ts.pending >> 24) & 1u) {  // the certificate test deferred by node_step
                const uint4* rec = reinterpret_cast<const uint4*>(ka.tri_leafcert + prim);
                const uint4 c0 = rec[0], c1 = rec[1];
                const uint32_t w[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                skip = tri_leafcert_skips_gap(w, tri_cone_ray(o.x, o.y, o.z, d.x, d.y, d.z), ts.tri.t, ts.cert_gap);
            }
            if (skip != kLeafCertAll) {
                const uint4 pr = sv.tri_prims[prim];  // object, sub, seq_base, range
                const RtObject& ob = sv.obj[pr.x];
                if (ray_in_bounds(o, ts.inv, ob.min_bounds, ob.max_bounds)) {  // :431
                    if (pr.w != kPrimRangeNone && (pr.w >> 27) < kLeafTriSlots) {
                        want = true;
                        range = pr.w;
                        seq0 = pr.z;
                        obj = pr.x;
                        sub = pr.y;
                    } else {  // a leaf of more than 7 triangles: the per-lane test (no certificate mask)
                        tri_leaf<true>(sv, ka, o, d, ts, prim);
                        ts.limit = tri_limit(sv, ka, o, ts);
                    }
                }
            }
        } else {
            test_sphere_group(sv, ts.pending, o, d, ts.a4, ts.a2, ts.sph);
            ts.limit = prune_limit(ts);
        }
        ts.pending = kNoLeaf;
    }
    const uint64_t wm = __ballot(want);
    if (wm == 0) return;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4* const scratch = reinterpret_cast<float4*>(lds + ka.lds_leafbatch_offset + wave * kLeafBatchWaveBytes);
    const uint32_t n = (uint32_t)__popcll(wm);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(wm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wm, 0u));
    if (want) {
        float4* sl = scratch + 3u * rank;
        sl[0] = make_float4(o.x, o.y, o.z, __uint_as_float(prim));
        sl[1] = make_float4(d.x, d.y, d.z, __uint_as_float(range));
        sl[2] = make_float4(__uint_as_float(seq0), __uint_as_float(obj), __uint_as_float(sub), 0.0f);
    }
    wave_lds_sync();
    const uint32_t lane = lane_id_here(), g = lane >> 3, j = lane & 7u;
    for (uint32_t base = 0; base < n; base += 8u) {
        const uint32_t kk = base + g;
        float cd = __builtin_inff();  // no candidate: never accepted (a distance is always < inf there)
        uint32_t cs = 0xffffffffu, ct = 0u;
        bool cnan = false;
        if (kk < n) {
            const float4* sl = scratch + 3u * kk;
            const float4 s0 = sl[0], s1 = sl[1];
            const uint32_t rg = __float_as_uint(s1.w);
            if (j < (rg >> 27)) {
                const uint4* blk = ka.tri_leaftris + (size_t)__float_as_uint(s0.w) * kLeafTriWords + j;
                const uint4 q0 = blk[0], q1 = blk[kLeafTriSlots], q2 = blk[2u * kLeafTriSlots];
                const float4 p0 = make_float4(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z),
                                              __uint_as_float(q0.w));
                const float4 p1 = make_float4(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z),
                                              __uint_as_float(q1.w));
                const float4 p2 = make_float4(__uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z),
                                              __uint_as_float(q2.w));
                const TriGeom tg{mk(p0.x, p0.y, p0.z), mk(p0.w, p1.x, p1.y), mk(p1.z, p1.w, p2.x),
                                 mk(p2.y, p2.z, p2.w)};
                const f3 ro = mk(s0.x, s0.y, s0.z), rd = mk(s1.x, s1.y, s1.z);
                // the reference's test, tri_leaf's operations (:449-481)
                const float det = -dot(rd, tg.cn);
                const float inv_det = 1.0f / det;
                const f3 ao = ro - tg.a;
                const float dist = dot(ao, tg.cn) * inv_det;
                const f3 dao = cross(ao, rd);
                const float v = -dot(tg.ab, dao) * inv_det;
                const float u = dot(tg.ac, dao) * inv_det;
                const float w = 1.0f - u - v;
                if (!(dist < 0.0f) && !(v < 0.0f) && !(u < 0.0f) && !(w < 0.0f)) {
                    if (dist != dist) {
                        cnan = true;
                    } else {
                        cd = dist;
                        cs = __float_as_uint(sl[2].x) + j;
                        ct = min((rg & ((1u << 27) - 1u)) + j, ka.triangle_count - 1u) | (det > 0.0f ? 0x80000000u : 0u);
                    }
                }
            }
        }
        // the group's minimum on every lane of it: xor 1, xor 2 (quad), then the other quad
        coop_min_step<0xB1>(cd, cs, ct);
        coop_min_step<0x4E>(cd, cs, ct);
        coop_min_step<0x141>(cd, cs, ct);
        const uint64_t nm = __ballot(cnan);
        if (j == 0u && kk < n)  // slot kk's ray is no longer needed: its result goes there
            scratch[3u * kk] = make_float4(cd, __uint_as_float(cs), __uint_as_float(ct),
                                           __uint_as_float(((nm >> (8u * g)) & 0xffu) != 0u ? 1u : 0u));
    }
    wave_lds_sync();
    if (want) {
        const float4 r = scratch[3u * rank];
        const float4 r2 = scratch[3u * rank + 2u];
        obj = __float_as_uint(r2.y);
        sub = __float_as_uint(r2.z);
        const float rd = r.x;
        const uint32_t rs = __float_as_uint(r.y), rt = __float_as_uint(r.z);
        const bool rnan = __float_as_uint(r.w) != 0u;
        const bool beats = rd < ts.tri.t || (rd == ts.tri.t && rs < ts.tri.seq);
        if (rnan || beats) {
            const RtSubObject so = sv.sub[sub];  // :441, run when the leaf would change the result
            if (ray_in_bounds(o, ts.inv, so.min_bounds, so.max_bounds)) {
                if (rnan) ts.nan_hit = true;
                if (beats) ts.tri = TriHit{rd, rs, rt & 0x7fffffffu, obj, (rt >> 31) != 0u};
            }
        }
        ts.limit = tri_limit(sv, ka, o, ts);
    }
}

}  // namespace
