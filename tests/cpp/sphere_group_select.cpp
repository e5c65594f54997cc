// CPU check of the sphere group test's root passes (csrc/rt_sphere_roots.h: sphere_group_roots,
// the code the kernels run, compiled here with -ffp-contract=off so that sqrt and / are the
// correctly rounded IEEE ones).
//
//   sphere_group_select select <n_random> <seed>
//     The candidate-compacted selection against two references written out below -- the four
//     positional arms, and a brute lexicographic (t, orig) minimum -- on structured cases (every
//     candidate mask, equal t with orig in every order, t <= 0 and t == +0, disc == 0 / -0 / NaN /
//     inf / below 2^-96 / denormal, an incoming best below, at and above every candidate) and on
//     n_random random groups: (t, orig, slot) must be bitwise equal, and every candidate must be
//     evaluated exactly once (passes == candidates).
//     -> "ok select groups <n> masks <bitmap of the 16 masks seen> by_count <n0> <n1> <n2> <n3> <n4>"
//   sphere_group_select scene <spheres.bin> <rays.bin>
//     Builds the slots of a scene (rt_scene_sphere records), walks its BVH for every ray (6 f32:
//     origin, direction) with the group test at the leaves, and compares with the reference's
//     brute-force scan (compute_shader.wgsl:355-404).
//     -> "ok scene rays <n> groups <visited> by_count <n0> <n1> <n2> <n3> <n4> mismatches 0"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rt_bvh_slab.h"
#include "rt_sphere_roots.h"
#include "sphere_bvh.h"

static const float kF32Max = 3.4028235e+38f;

static uint32_t bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
static bool same(const SphereHit& a, const SphereHit& b) {
    return bits(a.t) == bits(b.t) && a.orig == b.orig && a.slot == b.slot;
}

// Reference 1: the four positional arms (the form the kernels had).
static void ref_arm(float disc, float b, float two_a, uint32_t orig, uint32_t slot, SphereHit& best) {
    if (disc >= 0.0f) {
        const float t = (-b - std::sqrt(disc)) / two_a;
        if (t > 0.0f && (t < best.t || (t == best.t && orig < best.orig))) best = SphereHit{t, orig, slot};
    }
}
static void ref_arms(const float disc[4], const float b[4], const uint32_t orig[4], uint32_t slot, float two_a,
                     SphereHit& best) {
    for (uint32_t k = 0; k < 4; k++) ref_arm(disc[k], b[k], two_a, orig[k], slot + k, best);
}

// Reference 2: all roots first, then the lexicographic (t, orig) minimum of the accepted ones
// (t > 0; a NaN root is none), which replaces the incoming best only when lexicographically below.
static void ref_brute(const float disc[4], const float b[4], const uint32_t orig[4], uint32_t slot, float two_a,
                      SphereHit& best) {
    std::vector<SphereHit> c;
    for (uint32_t k = 0; k < 4; k++) {
        if (!(disc[k] >= 0.0f)) continue;
        const float s = std::sqrt(disc[k]);
        const float num = -b[k] - s;
        const float t = num / two_a;
        if (t > 0.0f) c.push_back(SphereHit{t, orig[k], slot + k});
    }
    if (c.empty()) return;
    const SphereHit m = *std::min_element(c.begin(), c.end(), [](const SphereHit& x, const SphereHit& y) {
        return x.t < y.t || (x.t == y.t && x.orig < y.orig);
    });
    if (m.t < best.t || (m.t == best.t && m.orig < best.orig)) best = m;
}

struct PassCounter {
    long* n;
    void operator()() const { ++*n; }
};

static long g_groups = 0, g_by_count[5] = {0, 0, 0, 0, 0};
static uint32_t g_masks = 0;

static bool check_group(const float disc[4], const float b[4], const uint32_t orig[4], uint32_t slot, float two_a,
                        SphereHit best) {
    SphereHit a = best, r1 = best, r2 = best;
    long passes = 0;
    sphere_group_roots(disc, b, orig, slot, two_a, a, PassCounter{&passes});
    SphereHit plain = best;  // the default (no hook) instantiation, as the product kernels call it
    sphere_group_roots(disc, b, orig, slot, two_a, plain);
    SphereHit by_slot = best;  // the header's positional form (the brute-force set's sweep)
    sphere_group_roots_by_slot(disc, b, orig, slot, two_a, by_slot);
    ref_arms(disc, b, orig, slot, two_a, r1);
    ref_brute(disc, b, orig, slot, two_a, r2);
    uint32_t mask = 0;
    for (int k = 0; k < 4; k++) mask |= (disc[k] >= 0.0f ? 1u : 0u) << k;
    const int n = __builtin_popcount(mask);
    g_groups++;
    g_by_count[n]++;
    g_masks |= 1u << mask;
    if (same(a, r1) && same(a, r2) && same(a, plain) && same(a, by_slot) && passes == n) return true;
    printf("MISMATCH mask %x passes %ld two_a %.9g best (%.9g %u %u)\n", mask, passes, two_a, best.t, best.orig,
           best.slot);
    for (int k = 0; k < 4; k++) printf("  slot %d disc %.9g b %.9g orig %u\n", k, disc[k], b[k], orig[k]);
    printf("  got (%.9g %u %u) arms (%.9g %u %u) brute (%.9g %u %u)\n", a.t, a.orig, a.slot, r1.t, r1.orig, r1.slot,
           r2.t, r2.orig, r2.slot);
    return false;
}

// One group against the incoming bests that matter: none yet, and for every candidate root a best
// just below, at (with a lower, the same and a higher original index) and just above it.
static bool check_with_bests(const float disc[4], const float b[4], const uint32_t orig[4], uint32_t slot, float two_a) {
    if (!check_group(disc, b, orig, slot, two_a, SphereHit{kF32Max, 0u, 0u})) return false;
    for (int k = 0; k < 4; k++) {
        if (!(disc[k] >= 0.0f)) continue;
        const float t = (-b[k] - std::sqrt(disc[k])) / two_a;
        if (!(t > 0.0f) || std::isinf(t)) continue;
        const SphereHit bests[5] = {{std::nextafter(t, 0.0f), 77u, 900u},
                                    {t, orig[k] - 1u, 901u},
                                    {t, orig[k], 902u},
                                    {t, orig[k] + 1u, 903u},
                                    {std::nextafter(t, INFINITY), 0u, 904u}};
        for (const SphereHit& bs : bests)
            if (!check_group(disc, b, orig, slot, two_a, bs)) return false;
    }
    return true;
}

static int select_cases(long n_random, unsigned seed) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // discriminants: not a candidate (negative, NaN), zero of either sign, the slow side of the
    // sqrt (below 2^-96, denormal), ordinary, huge, infinite
    const float dpool[] = {-1.0f, nan, 0.0f, -0.0f, 1e-30f, 1e-40f, 0x1p-96f, 1.0f, 4.0f, 2.25f, 3.0e38f, INFINITY};
    // b: roots behind the origin (t <= 0), t == +0 with disc 4 or 1, in front, far in front
    const float bpool[] = {3.0f, -2.0f, -1.0f, 0.0f, -4.0f, -1.0e20f, -5.5f};
    const int nd = sizeof(dpool) / sizeof(*dpool), nb = sizeof(bpool) / sizeof(*bpool);
    static const int perm[24][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1},
                                    {1, 0, 2, 3}, {1, 0, 3, 2}, {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0},
                                    {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0}, {2, 3, 0, 1}, {2, 3, 1, 0},
                                    {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};
    // 1. every combination of discriminant kinds over the four slots (every mask among them)
    uint32_t h = 0x9e3779b9u;
    for (int i = 0; i < nd * nd * nd * nd; i++) {
        const int id[4] = {i % nd, (i / nd) % nd, (i / nd / nd) % nd, i / nd / nd / nd};
        float disc[4], b[4];
        uint32_t orig[4];
        h = h * 747796405u + 2891336453u;
        const int* pm = perm[(h >> 8) % 24];
        for (int k = 0; k < 4; k++) {
            disc[k] = dpool[id[k]];
            b[k] = bpool[(h >> (4 * k + 12)) % nb];
            orig[k] = 10u + (uint32_t)pm[k];
        }
        const float two_a = (i % 3 == 0) ? 2.0f : (i % 3 == 1) ? 0.73f : 5.0e-3f;
        if (!check_with_bests(disc, b, orig, 8u * (uint32_t)(i % 50), two_a)) return 1;
    }
    // 2. equal roots: every mask x the original indices in every order x the same (disc, b) in
    // every candidate slot (t > 0, t == +0, t < 0), the others negative or NaN padding
    const float eq[][2] = {{4.0f, -5.0f}, {4.0f, -2.0f}, {4.0f, 1.0f}, {0.0f, -3.0f}, {1e-30f, -1.0f}};
    for (uint32_t mask = 0; mask < 16; mask++)
        for (int p = 0; p < 24; p++)
            for (const auto& e : eq)
                for (int pad = 0; pad < 2; pad++) {
                    float disc[4], b[4];
                    uint32_t orig[4];
                    for (int k = 0; k < 4; k++) {
                        const bool c = (mask >> k) & 1u;
                        disc[k] = c ? e[0] : pad ? nan : -2.0f;
                        b[k] = c ? e[1] : pad ? nan : -7.0f;
                        orig[k] = (!c && pad) ? 0xffffffffu : 3u + (uint32_t)perm[p][k];
                    }
                    if (!check_with_bests(disc, b, orig, 4u * mask, 2.0f)) return 1;
                }
    // 3. two equal pairs at different distances (pairs 0.5 0.5 0.8 0.8 of the cluster scene), all orders
    for (int p = 0; p < 24; p++)
        for (int q = 0; q < 24; q++) {
            const float d2[2] = {9.0f, 2.25f}, b2[2] = {-6.0f, -6.0f};
            float disc[4], b[4];
            uint32_t orig[4];
            for (int k = 0; k < 4; k++) {
                disc[k] = d2[perm[q][k] >> 1];
                b[k] = b2[perm[q][k] >> 1];
                orig[k] = 40u + (uint32_t)perm[p][k];
            }
            if (!check_with_bests(disc, b, orig, 12u, 2.0f)) return 1;
        }
    // 4. random groups: values from the pools and random ones, mixed per slot
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    for (long r = 0; r < n_random; r++) {
        float disc[4], b[4];
        uint32_t orig[4];
        const bool ties = rng() % 4 == 0;
        const float td = 16.0f * U(rng), tb = -8.0f * U(rng);
        for (int k = 0; k < 4; k++) {
            const uint32_t kind = rng() % 8;
            if (kind == 0) {
                disc[k] = dpool[rng() % nd];
                b[k] = bpool[rng() % nb];
            } else if (ties && kind < 5) {
                disc[k] = td;
                b[k] = tb;
            } else {
                disc[k] = (U(rng) - 0.45f) * std::ldexp(1.0f, (int)(rng() % 40) - 20);
                b[k] = (U(rng) - 0.7f) * std::ldexp(1.0f, (int)(rng() % 24) - 12);
            }
            orig[k] = rng() % 8;  // (equal indices in two slots cannot occur in a scene; harmless here)
        }
        for (int k = 1; k < 4; k++)  // distinct original indices
            for (int j = 0; j < k; j++)
                if (orig[k] == orig[j]) orig[k] = 100u + (uint32_t)k;
        const float two_a = 2.0f * std::ldexp(0.5f + U(rng), (int)(rng() % 8) - 4);
        SphereHit best{kF32Max, 0u, 0u};
        const uint32_t bk = rng() % 4;
        if (bk == 1) best = SphereHit{4.0f * U(rng), (uint32_t)(rng() % 8), 999u};
        if (bk == 2) {  // exactly a candidate's root, with an index around that candidate's
            const int k = (int)(rng() % 4);
            const float t = (-b[k] - std::sqrt(disc[k])) / two_a;
            if (t > 0.0f) best = SphereHit{t, orig[k] + (uint32_t)(rng() % 3) - 1u, 998u};
        }
        if (!check_group(disc, b, orig, 4u * (uint32_t)(r % 1000), two_a, best)) return 1;
    }
    printf("ok select groups %ld masks %x by_count %ld %ld %ld %ld %ld\n", g_groups, g_masks, g_by_count[0],
           g_by_count[1], g_by_count[2], g_by_count[3], g_by_count[4]);
    return 0;
}

// ---- the cluster scene: the walk with the group test at its leaves against the brute scan ----
struct V {
    float x, y, z;
};
static V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static float dot(V a, V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// check_spheres, compute_shader.wgsl:355-404 (index order, first of equal distances).
static SphereHit brute(const std::vector<rt_scene_sphere>& s, V o, V d) {
    SphereHit r{kF32Max, 0xffffffffu, 0u};
    const float a = dot(d, d);
    for (size_t i = 0; i < s.size(); i++) {
        const V oc = sub(o, V{s[i].position[0], s[i].position[1], s[i].position[2]});
        const float b = 2.0f * dot(d, oc);
        const float c = dot(oc, oc) - s[i].radius * s[i].radius;
        const float disc = b * b - 4.0f * a * c;
        if (disc < 0.0f) continue;
        const float t = (-b - std::sqrt(disc)) / (2.0f * a);
        if (t > 0.0f && t < r.t) r = SphereHit{t, (uint32_t)i, 0u};
    }
    return r;
}

// sphere_disc of rt_path_common.h.
static float slot_disc(const SphereSlots& sl, uint32_t slot, V o, V d, float four_a, float& b) {
    const float* q = &sl.slot_sph[4 * slot];
    const V oc = sub(o, V{q[0], q[1], q[2]});
    b = 2.0f * dot(d, oc);
    const float c = dot(oc, oc) - q[3];
    return b * b - four_a * c;
}

// test_sphere_group of rt_path_common.h; `count`: tally the group's candidates (BVH leaves).
static void group(const SphereSlots& sl, uint32_t slot, V o, V d, float four_a, float two_a, SphereHit& best, bool count) {
    float disc[4], b[4];
    uint32_t orig[4];
    int n = 0;
    for (uint32_t k = 0; k < 4; k++) {
        disc[k] = slot_disc(sl, slot + k, o, d, four_a, b[k]);
        orig[k] = sl.slot_orig[slot + k];
        n += disc[k] >= 0.0f;
    }
    if (count) {
        g_groups++;
        g_by_count[n]++;
    }
    sphere_group_roots(disc, b, orig, slot, two_a, best);
}

// trace_begin's sweep of the brute-force set, then the skip-link walk (node_visit) with the
// culling bounds of rt_bvh_slab.h, as the kernels do.
static SphereHit walk(const SphereSlots& sl, V o, V d) {
    SphereHit best{kF32Max, 0u, 0u};
    const float a = dot(d, d), four_a = 4.0f * a, two_a = 2.0f * a;
    uint32_t i = 0;
    for (; i + 4u <= sl.n_always; i += 4u) group(sl, i, o, d, four_a, two_a, best, false);
    if (sl.n_always - i >= 2u) {
        group(sl, i, o, d, four_a, two_a, best, false);
    } else if (sl.n_always - i == 1u) {
        float b;
        const float disc = slot_disc(sl, i, o, d, four_a, b);
        sphere_candidate(disc, b, two_a, sl.slot_orig[i], i, best);
    }
    const uint32_t n = (uint32_t)sl.nodes.size();
    if (n) {
        float lateral, slack;
        sphere_cull_bounds(std::sqrt(dot(o, o)), sl.extent, sl.r_min, sl.r_max, 1.0f / std::sqrt(a), lateral, slack);
        const SlabRay sr = slab_ray(o.x, o.y, o.z, 1.0f / d.x, 1.0f / d.y, 1.0f / d.z, lateral);
        uint32_t node = 0;
        while (node < n) {
            const SphereBvhNode& nd = sl.nodes[node];
            float near_t, far_t;
            slab_hit(sr, nd.bmin[0], nd.bmin[1], nd.bmin[2], nd.bmax[0], nd.bmax[1], nd.bmax[2], near_t, far_t);
            const bool hit = near_t <= far_t && far_t >= -slack && near_t <= best.t * 1.00001f + slack;
            if (hit && nd.leaf != kSphereBvhInternal) group(sl, nd.leaf & 0xffffffu, o, d, four_a, two_a, best, true);
            node = (hit && nd.leaf == kSphereBvhInternal) ? node + 1 : nd.skip;
        }
    }
    return best;
}

static int scene(const char* sph_path, const char* rays_path) {
    FILE* f = fopen(sph_path, "rb");
    if (!f) return 2;
    std::vector<rt_scene_sphere> s;
    rt_scene_sphere sp;
    while (fread(&sp, sizeof(sp), 1, f) == 1) s.push_back(sp);
    fclose(f);
    SphereSlots sl;
    build_sphere_slots(s.data(), (uint32_t)s.size(), true, &sl);
    f = fopen(rays_path, "rb");
    if (!f) return 2;
    float q[6];
    long n = 0, bad = 0;
    while (fread(q, sizeof(q), 1, f) == 1) {
        const V o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
        const SphereHit want = brute(s, o, d), got = walk(sl, o, d);
        const bool hit = want.orig != 0xffffffffu;
        const bool ok = hit ? (bits(got.t) == bits(want.t) && got.orig == want.orig && sl.slot_orig[got.slot] == want.orig)
                            : bits(got.t) == bits(kF32Max);
        if (!ok && bad++ == 0)
            printf("MISMATCH ray %ld o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g) brute=(%u %.9g) walk=(%u %.9g)\n", n, o.x, o.y,
                   o.z, d.x, d.y, d.z, want.orig, want.t, got.orig, got.t);
        n++;
    }
    fclose(f);
    printf("%s scene rays %ld always %u nodes %zu groups %ld by_count %ld %ld %ld %ld %ld mismatches %ld\n",
           bad ? "FAILED" : "ok", n, sl.n_always, sl.nodes.size(), g_groups, g_by_count[0], g_by_count[1], g_by_count[2],
           g_by_count[3], g_by_count[4], bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 3 && strcmp(argv[1], "scene") == 0) return scene(argv[2], argv[3]);
    if (argc > 3 && strcmp(argv[1], "select") == 0) return select_cases(atol(argv[2]), (unsigned)atoi(argv[3]));
    fprintf(stderr, "usage: sphere_group_select select <n_random> <seed> | scene <spheres.bin> <rays.bin>\n");
    return 2;
}
