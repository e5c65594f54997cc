// rt_sphere_roots.h -- the root half of the sphere group test (check_spheres,
// compute_shader.wgsl:380-391), shared by the kernels (rt_path_common.h:
// test_sphere_group) and the CPU harness (tests/cpp/sphere_group_select.cpp), so
// both run the same selection logic and the same f32 operation order.
//
// A group is 4 slots with their discriminants. A slot with disc >= 0 is a
// candidate: its near root t = (-b - sqrt(disc)) / 2a is evaluated (correctly
// rounded sqrt and division) and accepted as the lexicographic minimum of
// (t, original index) over roots with t > 0. That minimum does not depend on the
// order in which a lane evaluates its candidates, so the group is evaluated by
// candidate, not by slot position: in each pass every lane that still has an
// untested candidate evaluates one of them, and the passes end when no lane of
// the wave has one left. A wave whose lanes hold at most one candidate each --
// the common case at a BVH leaf, DESIGN.md §5.2 -- pays for one root evaluation,
// where four positional arms cost one evaluation per slot position that is a
// candidate in any lane. (The full-wave sweep of the brute-force set keeps the
// positional arms, sphere_group_roots_by_slot: there they are the cheaper form.)
//
// RT_SPHERE_ROOTS_FORM picks how the passes are laid out (same result):
//   0  lowest candidate slot; then the highest, where a lane has two or more;
//      then slots 1 and 2 where they lie strictly between (three or more).
//      Straight-line code, the compare results stay live as lane masks. The default:
//      C2 0.2446 -> 0.2383 ms per frame in one process.
//   1  a 4-bit candidate mask per lane; a loop evaluates the lowest set bit and
//      clears it until every lane's mask is empty. Fewer SGPRs and less code, but the
//      mask arithmetic and the loop cost the first pass more: C2 0.2440.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include "rt_device_math.h"
#define RT_ROOTS_FN __device__ __forceinline__
#else
#include <cmath>
#define RT_ROOTS_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#ifndef RT_SPHERE_ROOTS_FORM
#define RT_SPHERE_ROOTS_FORM 0
#endif

// check_spheres, compute_shader.wgsl:355-404.
//
// The reference sweeps spheres in index order keeping the first of equal
// distances (strict `<`, :391), i.e. it returns the lexicographic minimum of
// (t, index) over spheres with disc >= 0 and t > 0. Here spheres are visited
// in slot order (brute-force set, then BVH leaves), so acceptance compares
// (t, original index) lexicographically, which yields the same sphere in any
// visiting order. `orig` starts at 0 so that t == F32_MAX is never taken.
struct SphereHit {
    float t;
    uint32_t orig;
    uint32_t slot;
};

// Correctly rounded sqrt: the device's own form (rt_device_math.h), the IEEE one on the host.
RT_ROOTS_FN float sphere_root_sqrt(float x) {
#if defined(__HIPCC__)
    return rtk::sqrt_rn_any(x);
#else
    return std::sqrt(x);
#endif
}

RT_ROOTS_FN void sphere_candidate(float disc, float b, float two_a, uint32_t orig, uint32_t slot, SphereHit& best) {
    if (disc >= 0.0f) {
        const float t = (-b - sphere_root_sqrt(disc)) / two_a;
        if (t > 0.0f && (t < best.t || (t == best.t && orig < best.orig))) {
            best.t = t;
            best.orig = orig;
            best.slot = slot;
        }
    }
}

// The same candidates by slot position: arm k runs for the wave when any lane has disc[k] >= 0.
// For the wave-uniform sweep of the brute-force set, where every lane is active and each slot is
// a candidate in some lane: the passes below would run as often as the arms and pay their
// selection on top (C1, C3, C4 measured 1-2% slower with them there).
RT_ROOTS_FN void sphere_group_roots_by_slot(const float disc[4], const float b[4], const uint32_t orig[4],
                                            uint32_t slot, float two_a, SphereHit& best) {
    if (disc[0] >= 0.0f || disc[1] >= 0.0f || disc[2] >= 0.0f || disc[3] >= 0.0f) {
        sphere_candidate(disc[0], b[0], two_a, orig[0], slot, best);
        sphere_candidate(disc[1], b[1], two_a, orig[1], slot + 1u, best);
        sphere_candidate(disc[2], b[2], two_a, orig[2], slot + 2u, best);
        sphere_candidate(disc[3], b[3], two_a, orig[3], slot + 3u, best);
    }
}

// Called at the start of every root pass by the lanes that take it (diagnostic builds count
// passes and lanes with it; the default does nothing).
struct SphereRootsNoHook {
    RT_ROOTS_FN void operator()() const {}
};

// The candidates of the group of 4 slots at `slot` (disc[k] >= 0; NaN padding is none), each
// evaluated once and merged into `best`.
template <class PassHook = SphereRootsNoHook>
RT_ROOTS_FN void sphere_group_roots(const float disc[4], const float b[4], const uint32_t orig[4], uint32_t slot,
                                    float two_a, SphereHit& best, PassHook pass = PassHook{}) {
    // Read once into values: the selects below then pick among registers. (Selecting among the
    // array elements themselves lets the compiler turn the select into an indexed load, which
    // puts the arrays in scratch memory on the device.)
    const float d0 = disc[0], d1 = disc[1], d2 = disc[2], d3 = disc[3];
    const float b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    const uint32_t o0 = orig[0], o1 = orig[1], o2 = orig[2], o3 = orig[3];
    const bool c0 = d0 >= 0.0f, c1 = d1 >= 0.0f, c2 = d2 >= 0.0f, c3 = d3 >= 0.0f;
#if RT_SPHERE_ROOTS_FORM == 0
    if (c0 || c1 || c2 || c3) {
        // pass 1: the lowest candidate slot
        pass();
        const uint32_t lo = c0 ? 0u : c1 ? 1u : c2 ? 2u : 3u;
        sphere_candidate(c0 ? d0 : c1 ? d1 : c2 ? d2 : d3, c0 ? b0 : c1 ? b1 : c2 ? b2 : b3, two_a,
                         c0 ? o0 : c1 ? o1 : c2 ? o2 : o3, slot + lo, best);
        // pass 2: the highest, where it is another one
        const uint32_t hi = c3 ? 3u : c2 ? 2u : c1 ? 1u : 0u;
        if (hi != lo) {
            pass();
            sphere_candidate(c3 ? d3 : c2 ? d2 : d1, c3 ? b3 : c2 ? b2 : b1, two_a, c3 ? o3 : c2 ? o2 : o1, slot + hi,
                             best);
            // pass 3: slots 1 and 2 strictly between the two
            if (c1 && lo == 0u && hi >= 2u) {
                pass();
                sphere_candidate(d1, b1, two_a, o1, slot + 1u, best);
            }
            if (c2 && lo <= 1u && hi == 3u) {
                pass();
                sphere_candidate(d2, b2, two_a, o2, slot + 2u, best);
            }
        }
    }
#else
    uint32_t m = (c0 ? 1u : 0u) | (c1 ? 2u : 0u) | (c2 ? 4u : 0u) | (c3 ? 8u : 0u);
    while (m != 0u) {  // (on the device: until no lane of the wave has a candidate left)
        pass();
        const uint32_t low = m & (0u - m);  // the lowest candidate's bit
        m ^= low;
        const bool k0 = low == 1u, k1 = low == 2u, k2 = low == 4u;
        sphere_candidate(k0 ? d0 : k1 ? d1 : k2 ? d2 : d3, k0 ? b0 : k1 ? b1 : k2 ? b2 : b3, two_a,
                         k0 ? o0 : k1 ? o1 : k2 ? o2 : o3, slot + (k0 ? 0u : k1 ? 1u : k2 ? 2u : 3u), best);
    }
#endif
}
