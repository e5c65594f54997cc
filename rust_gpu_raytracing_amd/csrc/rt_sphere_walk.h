// rt_sphere_walk.h -- a block of node steps of the sphere BVH walk (sphere-only scenes, the BVH in
// LDS), shared by the path kernel (pathtrace.hip) and the CPU harness
// (tests/cpp/sphere_walk_block.cpp), so both run the same step.
//
// The walk is the stackless skip-link walk of rt_walk.h (node_visit with kBlockLeaves): a node
// whose inflated box the ray enters within [-slack, limit] is descended into (node + 1) when
// internal; a leaf so entered is recorded in `pending` (its sphere group's first slot) and the
// lane takes the leaf's skip link, then waits until the caller has tested the group and cleared
// `pending`; a node not entered is left by its skip link. The walk is over when
// pending == kSphereWalkNoLeaf && node >= node_end.
//
// A block is kSteps such steps as straight-line code: one predicate per step,
//     walk = pending == none && node < node_end,
// and everything a step changes is merged through selects on it, so a block holds no branch and no
// exec-mask update: a lane that waits at a leaf, or whose walk is over, runs the block's
// instructions with its node and pending kept. Its loads read node 0 (every such lane the same
// address: an LDS broadcast, no bank conflict) and the values are discarded. The generic
// node_step / phase_end sequence re-derived the lane's mode after every step with two exec-mask
// saves and five branches per step; in the sphere walk, which is bound by each wave's serial chain
// of LDS round trip and step rather than by VALU issue, those instructions are on
// the chain.
//
// kOrdered: the layout stores (near, far) corners for the ray's octant and the slab constants are
// paired the same way (slab_pair_by_octant), so the test needs no min/max per axis. It is
// launch-constant: the caller picks the instantiation once per block.
//
// Preconditions: nodes[0] and nodes[1] are readable (also when node_end == 0: no lane walks then,
// and what is read is discarded); skip links are > their node's index, so a walk ends.
// Vec4: four f32 members x, y, z, w (float4 on the device); a node is two of them, {bmin, skip}
// and {bmax, leaf} (SphereBvhNode), the integers read by bit pattern.
#pragma once

#include <stdint.h>

#include "rt_bvh_slab.h"

#if defined(__HIPCC__)
#define RT_SPHERE_WALK_FN __host__ __device__ __forceinline__
#else
#define RT_SPHERE_WALK_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr uint32_t kSphereWalkNoLeaf = 0xffffffffu;  // `pending`: no leaf recorded (rt_path_common.h: kNoLeaf)
constexpr uint32_t kSphereWalkInternal = 0xffffffffu;  // a node's leaf word: internal (sphere_bvh.h)

RT_SPHERE_WALK_FN uint32_t sphere_walk_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}

// Called once per step with the lane's predicates and the node it stands on (analysis builds count
// steps and lanes with it, the CPU harness records the visited nodes).
struct SphereWalkNoHook {
    RT_SPHERE_WALK_FN void operator()(bool /*walk*/, bool /*at_leaf*/, uint32_t /*node*/) const {}
};

// One step. hit, at_leaf, the next node and the leaf record are node_visit's expressions, with its
// comparison directions: a NaN near_t or far_t is a miss (the lane takes the skip link).
template <bool kOrdered, class Vec4, class Hook>
RT_SPHERE_WALK_FN void sphere_walk_step(const Vec4* nodes, uint32_t node_end, const SlabRay& slab, float slack,
                                        float limit, uint32_t& node, uint32_t& pending, const Hook& hook) {
    const bool walk = pending == kSphereWalkNoLeaf && node < node_end;
    const uint32_t at = walk ? node : 0u;
    const Vec4 lo = nodes[2u * at], hi = nodes[2u * at + 1u];
    float near_t, far_t;
    if (kOrdered)
        slab_hit_ordered(slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    const bool hit = near_t <= far_t && far_t >= -slack && near_t <= limit;
    const uint32_t leaf = sphere_walk_bits(hi.w);
    const bool at_leaf = hit && leaf != kSphereWalkInternal;
    hook(walk, walk && at_leaf, node);
    const uint32_t next = (hit && !at_leaf) ? node + 1u : sphere_walk_bits(lo.w);
    pending = (walk && at_leaf) ? (leaf & 0xffffffu) : pending;
    node = walk ? next : node;
}

template <int kSteps, bool kOrdered, class Vec4, class Hook = SphereWalkNoHook>
RT_SPHERE_WALK_FN void sphere_walk_block(const Vec4* nodes, uint32_t node_end, const SlabRay& slab, float slack,
                                         float limit, uint32_t& node, uint32_t& pending, const Hook& hook = Hook{}) {
    uint32_t n = node, p = pending;  // in registers across the block
#pragma unroll
    for (int k = 0; k < kSteps; ++k) sphere_walk_step<kOrdered>(nodes, node_end, slab, slack, limit, n, p, hook);
    node = n;
    pending = p;
}
