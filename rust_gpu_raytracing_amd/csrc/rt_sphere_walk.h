// rt_sphere_walk.h -- a block of node steps of the sphere BVH walk (sphere-only scenes, the BVH in
// LDS), shared by the path kernel (pathtrace.hip) and the CPU harnesses
// (tests/cpp/sphere_walk_block.cpp, tests/cpp/sphere_walk_links.cpp), so all run the same step.
// Two forms: sphere_walk_block on the node image as the host built it (node an index; the
// instance that reads the scene from global memory), and below it sphere_links_block on the image
// as the staging instances rewrite it into LDS (node an address).
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

// ---- The linked form: the walk of the instances that stage the nodes in LDS ---------------------
//
// Staging rewrites the nodes as it copies them (sphere_links_stage, the device-memory image is
// untouched), so that a step computes nothing that tests no box:
//   - `node` and the skip links are LDS byte addresses, nodes base + 32 * index: no shift and no
//     add between "the next node is known" and "its load is issued";
//   - the leaf word of a leaf is its sphere group's first slot alone (the flag bits masked off
//     once, in staging), 0xffffffff for an internal node as before;
//   - one more record follows the last node, the sentinel (sphere_links_sentinel): all six planes
//     NaN, so every ray misses it by the step's comparison directions; its skip link is its own
//     address; its leaf word is the internal marker. Every link that leaves the tree (>= node_end)
//     points to it, so a lane whose walk is over stands on it and stays there: no end comparison.
// One predicate per step remains, walk = pending == none. A waiting lane re-reads its own node and
// discards it; a finished lane reads the sentinel (all such lanes one address: a broadcast).
// The walk is over when pending == kSphereWalkNoLeaf && node == sentinel.
//
// `mem`: on the host, the byte image that the addresses index (the CPU harness: a stand-in for
// LDS); on the device it is not read, the address is the LDS address itself.
constexpr uint32_t kSphereNodeBytes = 32u;

RT_SPHERE_WALK_FN float sphere_walk_float(uint32_t b) {
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

RT_SPHERE_WALK_FN uint32_t sphere_links_addr(uint32_t base, uint32_t index) { return base + kSphereNodeBytes * index; }

// Half `i` of the node image (even: {bmin, skip}, odd: {bmax, leaf}) as staged at `base`.
template <class Vec4>
RT_SPHERE_WALK_FN Vec4 sphere_links_stage(Vec4 v, uint32_t i, uint32_t base, uint32_t node_end) {
    const uint32_t w = sphere_walk_bits(v.w);
    if (i & 1u)
        v.w = sphere_walk_float(w == kSphereWalkInternal ? w : (w & 0xffffffu));
    else
        v.w = sphere_walk_float(sphere_links_addr(base, w < node_end ? w : node_end));
    return v;
}

// Half `i` (0, 1) of the sentinel, the record at index node_end.
template <class Vec4>
RT_SPHERE_WALK_FN Vec4 sphere_links_sentinel(uint32_t i, uint32_t base, uint32_t node_end) {
    const float nan = sphere_walk_float(0x7fc00000u);
    Vec4 v;
    v.x = v.y = v.z = nan;
    v.w = sphere_walk_float(i ? kSphereWalkInternal : sphere_links_addr(base, node_end));
    return v;
}

template <class Vec4>
RT_SPHERE_WALK_FN void sphere_links_read(const unsigned char* mem, uint32_t addr, Vec4& lo, Vec4& hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float LdsVec4 __attribute__((ext_vector_type(4)));
    const __attribute__((address_space(3))) LdsVec4* p = (const __attribute__((address_space(3))) LdsVec4*)addr;
    const LdsVec4 a = p[0], b = p[1];
    lo.x = a.x, lo.y = a.y, lo.z = a.z, lo.w = a.w;
    hi.x = b.x, hi.y = b.y, hi.z = b.z, hi.w = b.w;
    (void)mem;
#else
    __builtin_memcpy(&lo, mem + addr, 16);
    __builtin_memcpy(&hi, mem + addr + 16, 16);
#endif
}

// One step: sphere_walk_step's hit and at_leaf, on the staged record at `node`.
template <bool kOrdered, class Vec4, class Hook>
RT_SPHERE_WALK_FN void sphere_links_step(const unsigned char* mem, uint32_t sentinel, const SlabRay& slab, float slack,
                                         float limit, uint32_t& node, uint32_t& pending, const Hook& hook) {
    Vec4 lo, hi;
    sphere_links_read(mem, node, lo, hi);
    float near_t, far_t;
    if (kOrdered)
        slab_hit_ordered(slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    const bool hit = near_t <= far_t && far_t >= -slack && near_t <= limit;
    const uint32_t leaf = sphere_walk_bits(hi.w);
    const bool at_leaf = hit && leaf != kSphereWalkInternal;
    const bool walk = pending == kSphereWalkNoLeaf;
    hook(walk && node != sentinel, walk && at_leaf, node);  // (the hook alone reads `sentinel`)
    const uint32_t next = (hit && !at_leaf) ? node + kSphereNodeBytes : sphere_walk_bits(lo.w);
    pending = (walk && at_leaf) ? leaf : pending;
    node = walk ? next : node;
}

// sphere_walk_block's contract with `node` an address: `sentinel` takes node_end's place.
// Preconditions: every staged record up to and including the sentinel is readable, and `node`
// is the address of one of them.
template <int kSteps, bool kOrdered, class Vec4, class Hook = SphereWalkNoHook>
RT_SPHERE_WALK_FN void sphere_links_block(const unsigned char* mem, uint32_t sentinel, const SlabRay& slab, float slack,
                                          float limit, uint32_t& node, uint32_t& pending, const Hook& hook = Hook{}) {
    uint32_t n = node, p = pending;  // in registers across the block
#pragma unroll
    for (int k = 0; k < kSteps; ++k) sphere_links_step<kOrdered, Vec4>(mem, sentinel, slab, slack, limit, n, p, hook);
    node = n;
    pending = p;
}
