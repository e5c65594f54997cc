// rt_nearest_math.h -- THE NEAREST-POINT CONTRACT of include/rt_abi.h as code, and the certified
// box bound of its accelerated walk. Plain C++ for the host and the device: the
// kernel (nearest.hip), the host's box check (rt_queries.cpp) and the CPU harness
// (tests/cpp/nearest_bound.cpp) compile this one text. Every operation is a single f32 operation:
// compile without contraction (-ffp-contract=off), with correctly rounded division and sqrt.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RTN_HD __host__ __device__ __forceinline__
#else
#define RTN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rtn {

constexpr float kMissDistance = 3.4028235e38f;
constexpr uint32_t kSphereOrder = 0x80000000u;  // order key of sphere i: kSphereOrder + i, after every triangle
constexpr uint32_t kNoOrder = 0xffffffffu;      // the order key of "nothing found yet"

struct V3 {
    float x, y, z;
};
RTN_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
RTN_HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RTN_HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RTN_HD V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
// the project's order (rt_device_math.h)
RTN_HD float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RTN_HD float sqrt_rn(float x) { return __builtin_sqrtf(x); }
RTN_HD float absf(float x) { return __builtin_fabsf(x); }
RTN_HD bool is_nan(float x) { return x != x; }

// ---- spheres ---------------------------------------------------------------------------------

// key = | sqrt(dot(c - p, c - p)) - |r| |; `l` receives the root.
RTN_HD float sphere_key(V3 c, float r_abs, V3 p, float& l) {
    const V3 v = c - p;
    l = sqrt_rn(dot(v, v));
    return absf(l - r_abs);
}

struct SphereNearest {
    V3 point, normal;
    uint32_t side;
};

RTN_HD SphereNearest sphere_nearest(V3 c, float r_abs, V3 p) {
    const V3 v = c - p;
    const float l = sqrt_rn(dot(v, v));
    SphereNearest s;
    if (l == 0.0f) {
        s.point = v3(c.x + r_abs, c.y, c.z);
        s.normal = v3(1.0f, 0.0f, 0.0f);
    } else {
        const float k = r_abs / l;
        s.point = c - v * k;
        s.normal = v3(-(v.x / l), -(v.y / l), -(v.z / l));
    }
    s.side = l >= r_abs ? 1u : 0u;
    return s;
}

// ---- triangles -------------------------------------------------------------------------------

// A weight as the contract takes it: NaN and negative values are 0, values above 1 are 1.
RTN_HD float weight01(float x) { return x >= 0.0f ? (x > 1.0f ? 1.0f : x) : 0.0f; }

struct TriNearest {
    V3 q;
    uint32_t feature;  // 1..7
};

// Ericson's seven regions in the contract's order, from the stored a, edge_ab, edge_ac.
RTN_HD TriNearest tri_nearest(V3 a, V3 ab, V3 ac, V3 p) {
    const V3 ap = p - a;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) return TriNearest{a, 1u};
    const V3 bp = ap - ab;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) return TriNearest{a + ab, 2u};
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = weight01(d1 / (d1 - d3));
        return TriNearest{a + ab * v, 3u};
    }
    const V3 cp = ap - ac;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) return TriNearest{a + ac, 4u};
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = weight01(d2 / (d2 - d6));
        return TriNearest{a + ac * w, 5u};
    }
    const float va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    if (va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
        const float w = weight01(e1 / (e1 + e2));
        return TriNearest{(a + ab * (1.0f - w)) + ac * w, 6u};
    }
    const float denom = 1.0f / ((va + vb) + vc);
    const float v = weight01(vb * denom);
    float w = weight01(vc * denom);
    const float rest = 1.0f - v;
    if (w > rest) w = rest;
    return TriNearest{(a + ab * v) + ac * w, 7u};
}

RTN_HD float point_key(V3 q, V3 p) {
    const V3 e = q - p;
    return sqrt_rn(dot(e, e));
}

// ---- candidates ------------------------------------------------------------------------------

// Whether the candidate (key, order) is accepted under max_distance and precedes the best so far
// (best_key, best_order): smaller key, then smaller order key (triangles by sweep position, then
// spheres by index). Nothing found yet: (+inf, kNoOrder).
RTN_HD bool candidate_wins(float key, uint32_t order, float max_distance, float best_key, uint32_t best_order) {
    if (!(key <= max_distance)) return false;  // (a NaN key, a NaN or negative max_distance)
    return key < best_key || (key == best_key && order < best_order);
}

// ---- the certified box bound -------------------------------------------------
//
// box_bound(corner, corner, p, abs_part) = d (1 - 2^-20) - abs_part, with d the f32 distance from p
// to the box: a value that never exceeds the contract key of a primitive below the node. With
// u = 2^-24: each difference in d has a relative error of u and the squares, sums and root add
// 3.5u, so d <= D (1 + 5u) for the real distance D; the key's own last steps (q - p or c - p, the
// dot, the root) lose at most 5u the other way; 1 - 2^-20 = 1 - 16u covers both. abs_part covers
// what is not relative to the distance. Triangles (tri_abs_part): the computed closest point is a
// convex combination of a, a + ab, a + ac up to 14u E per axis (E: the accelerator's extent), and
// the box check lets each of a, fl(a + ab), fl(a + ac) sit 32u E outside the box: at most 49u E
// per axis, 85u E in distance, covered by 2^-17 E = 128u E. Spheres (sphere_abs_part): the root is
// off by 4u |c - p| before |r| is subtracted, of which 4u |r| is not relative to the distance:
// covered by 2^-20 S = 16u S (S: the BVH spheres' extent). kTinyAbs is for squares that underflow.
// The corners may come in either order (the sphere layouts that store (near, far) corners).
constexpr float kBoundRel = 1.0f - 0x1p-20f;
constexpr float kTriAbsScale = 0x1p-17f;     // 128u: above sqrt(3) x (32u the box check allows + 14u + 3u)
constexpr float kTriCheckScale = 0x1p-19f;   // the box check: a vertex at most this x max |box coordinate| outside
constexpr float kSphereAbsScale = 0x1p-20f;  // 16u: above the 4u |r| that the root's rounding leaves
constexpr float kTinyAbs = 0x1p-60f;

RTN_HD float box_distance(float lx, float ly, float lz, float hx, float hy, float hz, V3 p) {
    const float ax = lx < hx ? lx : hx, bx = lx < hx ? hx : lx;
    const float ay = ly < hy ? ly : hy, by = ly < hy ? hy : ly;
    const float az = lz < hz ? lz : hz, bz = lz < hz ? hz : lz;
    float dx = ax - p.x, dy = ay - p.y, dz = az - p.z;
    const float ex = p.x - bx, ey = p.y - by, ez = p.z - bz;
    dx = dx > ex ? dx : ex;
    dy = dy > ey ? dy : ey;
    dz = dz > ez ? dz : ez;
    dx = dx > 0.0f ? dx : 0.0f;  // (a NaN difference counts as inside: never culled for it)
    dy = dy > 0.0f ? dy : 0.0f;
    dz = dz > 0.0f ? dz : 0.0f;
    return sqrt_rn((dx * dx + dy * dy) + dz * dz);
}

// The bound with the shrink. kShrink false is the mutant of the harness: the raw distance.
template <bool kShrink = true>
RTN_HD float box_bound(float lx, float ly, float lz, float hx, float hy, float hz, V3 p, float abs_part) {
    const float d = box_distance(lx, ly, lz, hx, hy, hz, p);
    if (!kShrink) return d;
    return d * kBoundRel - abs_part;
}

// The absolute parts. For spheres the rounding of l is relative to l <= distance + 2 |r|: the part
// relative to the distance is in kBoundRel, the rest scales with the spheres' extent.
RTN_HD float tri_abs_part(float tri_extent) { return kTriAbsScale * tri_extent + kTinyAbs; }
RTN_HD float sphere_abs_part(float sphere_extent) { return kSphereAbsScale * sphere_extent + kTinyAbs; }

// A node is skipped only when its bound is strictly beyond what can still win: a tie survives.
// kStrict false is the harness's second mutant.
template <bool kStrict = true>
RTN_HD bool bound_culls(float bound, float limit) {
    return kStrict ? bound > limit : bound >= limit;
}

// The visiting order: of the 8 direction-ordered layouts (sphere_bvh.h: bit k of a layout is set
// for rays that travel towards -axis k, and a layout lists first the child such a ray meets
// first) a point takes the one whose rays travel from it towards the root box's centre, which
// lists near children first for it. A heuristic: the bound is conservative under any order.
RTN_HD uint32_t point_octant(float lx, float ly, float lz, float hx, float hy, float hz, V3 p) {
    return (0.5f * (lx + hx) < p.x ? 1u : 0u) | (0.5f * (ly + hy) < p.y ? 2u : 0u) |
           (0.5f * (lz + hz) < p.z ? 4u : 0u);
}

// The box check of the host (one sub-object's box against one of its triangles): a, fl(a + ab) and
// fl(a + ac) lie in the box widened by kTriCheckScale x the box's largest |coordinate|. A
// non-finite box passes: the accelerator gives it an all-enclosing one. In a finite box a triangle
// with anything non-finite in a, ab, ac, fl(a + ab) or fl(a + ac) fails: its keys can still be
// finite (a = 0, ab = (inf, 0, 0), ac = (0, 1, 0) is at 1.41 from (-1, -1, 0) through region 1),
// so no finite box vouches for it.
RTN_HD bool box_holds_triangle(const float* mn, const float* mx, V3 a, V3 ab, V3 ac) {
    const V3 b = a + ab, c = a + ac;
    const float vs[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
    const float es[6] = {ab.x, ab.y, ab.z, ac.x, ac.y, ac.z};
    float big = 0.0f;
    for (int k = 0; k < 3; ++k)
        if (!(absf(mn[k]) <= kMissDistance) || !(absf(mx[k]) <= kMissDistance)) return true;
    for (int i = 0; i < 9; ++i)
        if (!(absf(vs[i]) <= kMissDistance)) return false;
    for (int i = 0; i < 6; ++i)
        if (!(absf(es[i]) <= kMissDistance)) return false;
    for (int k = 0; k < 3; ++k) {
        big = absf(mn[k]) > big ? absf(mn[k]) : big;
        big = absf(mx[k]) > big ? absf(mx[k]) : big;
    }
    const float m = kTriCheckScale * big;
    for (int i = 0; i < 9; ++i) {
        const int k = i % 3;
        const float lo = mn[k] < mx[k] ? mn[k] : mx[k], hi = mn[k] < mx[k] ? mx[k] : mn[k];
        if (!(vs[i] >= lo - m && vs[i] <= hi + m)) return false;
    }
    return true;
}

}  // namespace rtn
