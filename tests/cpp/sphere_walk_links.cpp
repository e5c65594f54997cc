// CPU check of the linked form of the sphere walk (csrc/rt_sphere_walk.h: sphere_links_stage,
// sphere_links_sentinel, sphere_links_block -- the code the path kernel's staging instances run)
// against sphere_walk_block on the unstaged nodes.
//
//   sphere_walk_links walk <seed>
//     Each tree is staged the way the kernel stages it: every half rewritten by sphere_links_stage
//     into a byte image (the stand-in for LDS) whose nodes start at a non-zero base, the sentinel
//     after the last node, poison after the sentinel. Every lane is then walked twice in lockstep,
//     a block at a time: by sphere_walk_block over the original nodes (node an index) and by
//     sphere_links_block over the image (node an address). After every block the two must agree:
//     address == base + 32 * index while the index walk is inside the tree, the sentinel's address
//     once it is over; equal pending; the same nodes visited in the same order. Between blocks a
//     waiting lane is "tested" (pending cleared, the limit moved below / at / above the leaf's
//     entry, or kept) or left waiting; a finished lane runs two more blocks.
//     Trees: BVHs of sphere_bvh.cpp over a random and a clustered sphere set in the 8 octant
//     layouts with plain and ordered boxes, a one-node tree whose root is a leaf, an empty tree
//     (the image is the sentinel alone), a hand-made tree with NaN planes and links past node_end.
//     Lanes: all 8 octants, zero direction components, limits below / at / above the root's entry,
//     lanes that enter their first block waiting or finished (with and without a leaf), a start
//     in the middle of the tree. Blocks of 1 to 8 steps.
//     A lane left on the sentinel for 1000 steps must not move, visit or record a leaf.
//     -> "ok walk lanes <n> blocks <n> visits <n> ..." and the coverage counts it asserts on
//   sphere_walk_links mutants <seed>
//     The same comparison must fail for: an image whose sentinel links to the first node instead
//     of to itself; an image whose leaf words keep their high bits; a block walk whose waiting
//     lanes move. The unbroken copy of that block walk must pass. -> "ok mutants detected 3"
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
#include "rt_sphere_walk.h"
#include "sphere_bvh.h"

struct V4 {
    float x, y, z, w;
};
static const uint32_t kNone = 0xffffffffu;
static const uint32_t kBase = 0x1230u;  // the image's first node (16-byte aligned, not 0)

static float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

struct Tree {
    std::vector<V4> nodes;  // 2 per node, and one readable poisoned node after them (sphere_walk_block reads node 0)
    uint32_t node_end = 0;  // nodes of all layouts
    uint32_t stride = 0;    // nodes per octant layout (0: one layout)
    bool ordered = false;
    float extent = 30.0f, r_min = 0.2f, r_max = 1.0f;
    std::vector<unsigned char> image;  // the staged form: kBase bytes, the nodes, the sentinel, poison
    uint32_t sentinel = 0;
};

enum ImageMutant { kImageGood = 0, kSentinelToFirst = 1, kLeafHighBits = 2 };

// The kernel's staging loop (pathtrace.hip) on the host.
static void stage(Tree& t, ImageMutant m) {
    const V4 poison{-1e6f, -1e6f, -1e6f, from_bits(kBase)};
    const V4 poison_hi{1e6f, 1e6f, 1e6f, from_bits(20u)};  // a box every ray enters, a leaf
    t.image.assign(kBase + 32u * (t.node_end + 1u) + 64u, 0xa5);
    V4* img = reinterpret_cast<V4*>(t.image.data() + kBase);
    for (uint32_t i = 0; i < 2u * t.node_end; i++) {
        img[i] = sphere_links_stage(t.nodes[i], i, kBase, t.node_end);
        if (m == kLeafHighBits && (i & 1u)) img[i].w = t.nodes[i].w;
    }
    for (uint32_t i = 0; i < 2u; i++) img[2u * t.node_end + i] = sphere_links_sentinel<V4>(i, kBase, t.node_end);
    if (m == kSentinelToFirst) img[2u * t.node_end].w = from_bits(kBase);
    img[2u * t.node_end + 2u] = poison;
    img[2u * t.node_end + 3u] = poison_hi;
    t.sentinel = sphere_links_addr(kBase, t.node_end);
}

static void push_node(Tree& t, const float lo[3], uint32_t skip, const float hi[3], uint32_t leaf) {
    t.nodes.push_back(V4{lo[0], lo[1], lo[2], from_bits(skip)});
    t.nodes.push_back(V4{hi[0], hi[1], hi[2], from_bits(leaf)});
}
static void finish(Tree& t, uint32_t node_end) {
    t.node_end = node_end;
    if (t.nodes.size() == 2u * node_end) {  // what sphere_walk_block reads for a lane that does not walk
        const float lo[3] = {-1e6f, -1e6f, -1e6f}, hi[3] = {1e6f, 1e6f, 1e6f};
        push_node(t, lo, 0u, hi, 20u | (1u << 24));
    }
}

static Tree tree_of(const std::vector<rt_scene_sphere>& s, bool ordered) {
    SphereSlots sl;
    build_sphere_slots(s.data(), (uint32_t)s.size(), true, &sl);
    if (sl.nodes.empty() || (ordered && !box_layout_orderable(sl.nodes))) {
        printf("FAILED: the builder made no (orderable) BVH\n");
        exit(1);
    }
    std::vector<SphereBvhNode> all;
    order_bvh_by_octant(sl.nodes, &all, ordered);
    Tree t;
    for (const SphereBvhNode& n : all) push_node(t, n.bmin, n.skip, n.bmax, n.leaf);
    finish(t, (uint32_t)all.size());
    t.stride = (uint32_t)sl.nodes.size();
    t.ordered = ordered;
    t.extent = sl.extent;
    t.r_min = sl.r_min;
    t.r_max = sl.r_max;
    return t;
}

// ---- the two walks ----------------------------------------------------------------------------
struct Record {
    std::vector<uint32_t>* seq;
    void operator()(bool walk, bool, uint32_t node) const {
        if (walk) seq->push_back(node);
    }
};

template <int kSteps>
static void index_block_n(const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node, uint32_t& pending,
                          std::vector<uint32_t>& seq) {
    if (t.ordered)
        sphere_walk_block<kSteps, true>(t.nodes.data(), t.node_end, sr, slack, limit, node, pending, Record{&seq});
    else
        sphere_walk_block<kSteps, false>(t.nodes.data(), t.node_end, sr, slack, limit, node, pending, Record{&seq});
}
template <int kSteps>
static void links_block_n(const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node, uint32_t& pending,
                          std::vector<uint32_t>& seq) {
    if (t.ordered)
        sphere_links_block<kSteps, true, V4>(t.image.data(), t.sentinel, sr, slack, limit, node, pending, Record{&seq});
    else
        sphere_links_block<kSteps, false, V4>(t.image.data(), t.sentinel, sr, slack, limit, node, pending, Record{&seq});
}

// The header's step written out, with the waiting lane's select switchable (the `mutants` mode).
static bool g_waiting_moves = false;
static void copy_block(int steps, const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node,
                       uint32_t& pending, std::vector<uint32_t>& seq) {
    for (int k = 0; k < steps; k++) {
        V4 lo, hi;
        memcpy(&lo, t.image.data() + node, 16);
        memcpy(&hi, t.image.data() + node + 16, 16);
        float near_t, far_t;
        if (t.ordered)
            slab_hit_ordered(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
        else
            slab_hit(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
        const bool hit = near_t <= far_t && far_t >= -slack && near_t <= limit;
        const uint32_t leaf = bits(hi.w);
        const bool at_leaf = hit && leaf != 0xffffffffu;
        const bool walk = pending == kNone || g_waiting_moves;
        if (walk && node != t.sentinel) seq.push_back(node);
        const uint32_t next = (hit && !at_leaf) ? node + 32u : bits(lo.w);
        if (walk && at_leaf) pending = leaf;
        if (walk) node = next;
    }
}

typedef void (*BlockFn)(int, const Tree&, const SlabRay&, float, float, uint32_t&, uint32_t&, std::vector<uint32_t>&);

#define RT_STEP_CASES(fn)                                         \
    switch (steps) {                                              \
        case 1: return fn<1>(t, sr, slack, limit, node, pending, seq); \
        case 2: return fn<2>(t, sr, slack, limit, node, pending, seq); \
        case 3: return fn<3>(t, sr, slack, limit, node, pending, seq); \
        case 4: return fn<4>(t, sr, slack, limit, node, pending, seq); \
        case 5: return fn<5>(t, sr, slack, limit, node, pending, seq); \
        case 6: return fn<6>(t, sr, slack, limit, node, pending, seq); \
        case 7: return fn<7>(t, sr, slack, limit, node, pending, seq); \
        case 8: return fn<8>(t, sr, slack, limit, node, pending, seq); \
    }                                                             \
    printf("FAILED: no instantiation for %d steps\n", steps);     \
    exit(1);
static void index_block(int steps, const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node,
                        uint32_t& pending, std::vector<uint32_t>& seq) {
    RT_STEP_CASES(index_block_n)
}
static void links_block(int steps, const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node,
                        uint32_t& pending, std::vector<uint32_t>& seq) {
    RT_STEP_CASES(links_block_n)
}

// ---- coverage ---------------------------------------------------------------------------------
struct Coverage {
    long lanes = 0, blocks = 0, visits = 0;
    long enter_waiting = 0, enter_done = 0, leaves = 0, ends = 0, links_out = 0;
    long nan_box = 0, sentinel_steps = 0;
    uint32_t octants = 0, step_sizes = 0;
};

struct Lane {
    SlabRay sr;
    float slack, limit;
    uint32_t node, pending;  // node: an index (>= node_end: finished)
};

static uint32_t addr_of(const Tree& t, uint32_t index) {
    return index < t.node_end ? sphere_links_addr(kBase, index) : t.sentinel;
}

static float near_of(const Tree& t, const Lane& ln, uint32_t node) {
    const V4 lo = t.nodes[2u * node], hi = t.nodes[2u * node + 1u];
    float near_t, far_t;
    if (t.ordered)
        slab_hit_ordered(ln.sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(ln.sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    return near_t <= far_t ? near_t : std::numeric_limits<float>::quiet_NaN();
}

// Walks one lane with `block` over the image and with sphere_walk_block over the nodes.
static bool run_lane(const Tree& t, Lane ln, int steps, BlockFn block, uint32_t seed, Coverage& cv, bool quiet) {
    std::mt19937 rng(seed);
    uint32_t rn = ln.node, rp = ln.pending;  // the index walk
    uint32_t an = addr_of(t, ln.node), ap = ln.pending;
    float limit = ln.limit;
    std::vector<uint32_t> sa, sr;
    int after_done = 0;
    cv.lanes++;
    cv.step_sizes |= 1u << steps;
    const long max_blocks = 16L * (t.node_end + 16);
    for (long blk = 0;; blk++) {
        if (blk > max_blocks) {
            if (!quiet) printf("MISMATCH: the walk does not end\n");
            return false;
        }
        sa.clear();
        sr.clear();
        if (rp != kNone) cv.enter_waiting++;
        if (rp == kNone && rn >= t.node_end) cv.enter_done++;
        const uint32_t p0 = rp;
        index_block(steps, t, ln.sr, ln.slack, limit, rn, rp, sr);
        block(steps, t, ln.sr, ln.slack, limit, an, ap, sa);
        cv.blocks++;
        cv.visits += (long)sr.size();
        bool aligned = true;  // every visited address is a node's: at or after the base, a multiple of 32 from it
        for (uint32_t& a : sa) {
            if (a < kBase || (a - kBase) % 32u != 0u) aligned = false;
            a = (a - kBase) / 32u;
        }
        bool same = aligned && an == addr_of(t, rn) && ap == rp && sa == sr;
        if (same && an > t.sentinel) same = false;
        if (!same) {
            if (!quiet)
                printf("MISMATCH steps %d block %ld: linked walk (addr %x pending %x, %zu visits) index walk (node %u -> addr %x "
                       "pending %x, %zu visits)\n", steps, blk, an, ap, sa.size(), rn, addr_of(t, rn), rp, sr.size());
            return false;
        }
        if (p0 == kNone && rp != kNone) cv.leaves++;
        if (rp == kNone && rn >= t.node_end) {
            if (after_done == 0) {
                cv.ends++;
                if (rn > t.node_end) cv.links_out++;
            }
            if (++after_done == 3) return true;
            continue;
        }
        if (rp != kNone && rng() % 3u != 0u) {  // the group test: pending cleared, the limit moved
            const uint32_t leaf_node = sr.empty() ? 0u : sr.back();
            const float leaf_near = sr.empty() ? 0.0f : near_of(t, ln, leaf_node);
            if (!std::isnan(leaf_near)) switch (rng() % 5u) {
                    case 1: limit = std::fmin(limit, leaf_near); break;
                    case 2: limit = std::fmin(limit, std::nextafter(leaf_near, -INFINITY)); break;
                    case 3: limit = std::fmin(limit, std::nextafter(leaf_near, INFINITY)); break;
                    case 4: limit = std::fmin(limit, leaf_near * 1.5f + 0.1f); break;
                    default: break;
                }
            ap = rp = kNone;
        }
    }
}

// ---- lanes ------------------------------------------------------------------------------------
static uint32_t octant_of(const SlabRay& sr) {
    return (bits(sr.ix) >> 31) | ((bits(sr.iy) >> 31) << 1) | ((bits(sr.iz) >> 31) << 2);
}

static Lane make_lane(const Tree& t, const float o[3], const float d[3], Coverage& cv) {
    Lane ln;
    const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    float lateral;
    sphere_cull_bounds(std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]), t.extent, t.r_min, t.r_max,
                       1.0f / std::sqrt(a), lateral, ln.slack);
    if (!std::isfinite(lateral)) lateral = 0.01f;
    if (!std::isfinite(ln.slack)) ln.slack = 0.01f;
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};  // +-inf for a zero component
    ln.sr = slab_ray(o[0], o[1], o[2], inv[0], inv[1], inv[2], lateral);
    const uint32_t oct = octant_of(ln.sr);
    cv.octants |= 1u << oct;
    if (t.ordered) slab_pair_by_octant(ln.sr);
    ln.node = oct * t.stride;
    ln.pending = kNone;
    ln.limit = INFINITY;
    return ln;
}

static bool run_variants(const Tree& t, const Lane& base, BlockFn block, std::mt19937& rng, Coverage& cv, bool quiet) {
    const float near0 = t.node_end ? near_of(t, base, base.node) : std::numeric_limits<float>::quiet_NaN();
    for (int steps = 1; steps <= 8; steps++) {
        std::vector<Lane> v;
        v.push_back(base);
        if (!std::isnan(near0)) {  // the root's entry against the limit: below, at, above
            for (float lim : {std::nextafter(near0, -INFINITY), near0, std::nextafter(near0, INFINITY), near0 + 1.0f}) {
                Lane l = base;
                l.limit = lim;
                v.push_back(l);
            }
        }
        Lane l = base;  // enters its first block waiting at a leaf
        l.pending = 8u;
        v.push_back(l);
        l = base;  // enters finished, without and with a leaf
        l.node = t.node_end;
        v.push_back(l);
        l.pending = 4u;
        v.push_back(l);
        if (t.node_end > 1) {  // starts in the middle of the tree
            l = base;
            l.node = base.node + rng() % std::max(1u, (t.stride ? t.stride : t.node_end) - 1u);
            v.push_back(l);
        }
        for (const Lane& x : v)
            if (!run_lane(t, x, steps, block, (uint32_t)rng(), cv, quiet)) return false;
    }
    return true;
}

static bool run_tree(const Tree& t, BlockFn block, std::mt19937& rng, int n_rays, Coverage& cv, bool quiet) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (int r = 0; r < n_rays; r++) {
        float o[3], d[3];
        const int kind = r % 6;
        for (int k = 0; k < 3; k++) {
            o[k] = (kind == 1 ? 60.0f : 12.0f) * U(rng);
            d[k] = U(rng);
        }
        if (kind == 2) d[rng() % 3u] = 0.0f;
        if (kind == 3) d[rng() % 3u] = -0.0f;
        if (kind == 4) {  // axis-parallel: two zero components
            const int keep = (int)(rng() % 3u);
            for (int k = 0; k < 3; k++)
                if (k != keep) d[k] = (rng() & 1u) ? 0.0f : -0.0f;
        }
        if (kind == 5)  // pointing away from the scene
            for (int k = 0; k < 3; k++) {
                o[k] = 40.0f * (U(rng) > 0.0f ? 1.0f : -1.0f) + U(rng);
                d[k] = std::copysign(std::fabs(d[k]) + 0.05f, o[k]);
            }
        if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
        const Lane base = make_lane(t, o, d, cv);
        if (!run_variants(t, base, block, rng, cv, quiet)) return false;
    }
    // a lane on the sentinel: 1000 steps, one at a time, must leave it there
    {
        float o[3] = {0.5f, 0.25f, -0.125f}, d[3] = {0.3f, -0.5f, 0.8f};
        const Lane ln = make_lane(t, o, d, cv);
        uint32_t node = t.sentinel, pending = kNone;
        std::vector<uint32_t> seq;
        for (int k = 0; k < 1000; k++) {
            block(1, t, ln.sr, ln.slack, ln.limit, node, pending, seq);
            cv.sentinel_steps++;
            if (node != t.sentinel || pending != kNone || !seq.empty()) {
                if (!quiet) printf("MISMATCH: a lane on the sentinel moved at step %d (addr %x pending %x)\n", k, node, pending);
                return false;
            }
        }
    }
    return true;
}

// ---- scenes -----------------------------------------------------------------------------------
static std::vector<rt_scene_sphere> random_spheres(std::mt19937& rng, int n) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<rt_scene_sphere> s;
    for (int i = 0; i < n; i++) {
        rt_scene_sphere sp{};
        for (int k = 0; k < 3; k++) sp.position[k] = 10.0f * U(rng);
        sp.radius = 0.2f + 0.4f * std::fabs(U(rng));
        s.push_back(sp);
    }
    return s;
}
static std::vector<rt_scene_sphere> clustered_spheres(std::mt19937& rng, int clusters) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<rt_scene_sphere> s;
    for (int c = 0; c < clusters; c++) {
        const float cx = 9.0f * U(rng), cy = 9.0f * U(rng), cz = 9.0f * U(rng);
        for (int i = 0; i < 4; i++) {
            rt_scene_sphere sp{};
            sp.position[0] = cx + 0.3f * U(rng);
            sp.position[1] = cy + 0.3f * U(rng);
            sp.position[2] = cz + 0.3f * U(rng);
            sp.radius = 0.25f;
            s.push_back(sp);
        }
    }
    return s;
}

static Tree one_node_tree() {
    Tree t;
    const float lo[3] = {-1.0f, -1.0f, -1.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
    push_node(t, lo, 1u, hi, 0u | (1u << 24));
    finish(t, 1);
    return t;
}
static Tree empty_tree() {
    Tree t;
    finish(t, 0);
    return t;
}
// NaN planes: one, several, all of a box, in internal nodes and leaves; links past node_end.
static Tree nan_tree() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    Tree t;
    const float L[3] = {-8.0f, -8.0f, -8.0f}, H[3] = {8.0f, 8.0f, 8.0f};
    const float l1[3] = {nan, -8.0f, -8.0f}, h1[3] = {0.0f, 8.0f, 8.0f};
    const float l2[3] = {-8.0f, -8.0f, -8.0f}, h2[3] = {-4.0f, nan, 8.0f};
    const float l3[3] = {nan, nan, nan}, h3[3] = {nan, nan, nan};
    const float l4[3] = {0.0f, -8.0f, -8.0f}, h4[3] = {8.0f, 8.0f, 8.0f};
    const float l5[3] = {0.0f, nan, -8.0f}, h5[3] = {4.0f, nan, 8.0f};
    const float l6[3] = {4.0f, -8.0f, -8.0f}, h6[3] = {8.0f, 8.0f, nan};
    push_node(t, L, 9u, H, 0xffffffffu);         // 0 root
    push_node(t, l1, 5u, h1, 0xffffffffu);       // 1 internal, one NaN plane
    push_node(t, l2, 3u, h2, 0u | (4u << 24));   // 2 leaf, one NaN plane
    push_node(t, l3, 4u, h3, 4u | (4u << 24));   // 3 leaf, all NaN: never entered
    push_node(t, l1, 5u, h1, 8u | (2u << 24));   // 4 leaf
    push_node(t, l4, 72u, h4, 0xffffffffu);      // 5 internal, its link beyond node_end (a copy's "8x the node count")
    push_node(t, l5, 7u, h5, 12u | (4u << 24));  // 6 leaf, an axis all NaN: unconstrained
    push_node(t, l3, 8u, h3, 0xffffffffu);       // 7 internal, all NaN: skipped
    push_node(t, l6, 0xfffffff0u, h6, 16u | (3u << 24));  // 8 leaf, its link far beyond node_end
    finish(t, 9);
    return t;
}

static bool run_all(BlockFn block, ImageMutant m, unsigned seed, Coverage& cv, bool quiet) {
    std::mt19937 rng(seed);
    const std::vector<rt_scene_sphere> rnd = random_spheres(rng, 180), clu = clustered_spheres(rng, 30);
    for (int ordered = 0; ordered < 2; ordered++) {
        Tree a = tree_of(rnd, ordered != 0), b = tree_of(clu, ordered != 0);
        Tree one = one_node_tree(), none = empty_tree(), nn = nan_tree();
        one.ordered = none.ordered = nn.ordered = ordered != 0;
        for (Tree* t : {&a, &b, &one, &none, &nn}) stage(*t, m);
        if (!run_tree(a, block, rng, 96, cv, quiet)) return false;
        if (!run_tree(b, block, rng, 96, cv, quiet)) return false;
        if (!run_tree(one, block, rng, 48, cv, quiet)) return false;
        if (!run_tree(none, block, rng, 24, cv, quiet)) return false;
        const long v0 = cv.visits;
        if (!run_tree(nn, block, rng, 96, cv, quiet)) return false;
        cv.nan_box += cv.visits - v0;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc > 2 && strcmp(argv[1], "walk") == 0) {
        Coverage cv;
        if (!run_all(links_block, kImageGood, (unsigned)atoi(argv[2]), cv, false)) return 1;
        const bool covered = cv.octants == 0xffu && cv.step_sizes == 0x1feu && cv.enter_waiting > 0 && cv.enter_done > 0 &&
                             cv.leaves > 0 && cv.ends > 0 && cv.links_out > 0 && cv.nan_box > 0 &&
                             cv.sentinel_steps >= 10000;
        printf("%s walk lanes %ld blocks %ld visits %ld octants %x step_sizes %x enter_waiting %ld enter_done %ld leaves %ld "
               "ends %ld links_out %ld nan_box_visits %ld sentinel_steps %ld\n",
               covered ? "ok" : "FAILED (coverage)", cv.lanes, cv.blocks, cv.visits, cv.octants, cv.step_sizes,
               cv.enter_waiting, cv.enter_done, cv.leaves, cv.ends, cv.links_out, cv.nan_box, cv.sentinel_steps);
        return covered ? 0 : 1;
    }
    if (argc > 2 && strcmp(argv[1], "mutants") == 0) {
        const unsigned seed = (unsigned)atoi(argv[2]);
        int detected = 0;
        for (int m = 1; m <= 3; m++) {
            Coverage cv;
            g_waiting_moves = m == 3;
            const bool pass = m == 3 ? run_all(copy_block, kImageGood, seed, cv, true)
                                     : run_all(links_block, (ImageMutant)m, seed, cv, true);
            if (!pass)
                detected++;
            else
                printf("FAILED: mutant %d passes the comparison\n", m);
        }
        g_waiting_moves = false;
        Coverage cv;
        if (!run_all(copy_block, kImageGood, seed, cv, false)) {
            printf("FAILED: the unbroken copy of the walk does not pass\n");
            return 1;
        }
        printf("%s mutants detected %d\n", detected == 3 ? "ok" : "FAILED", detected);
        return detected == 3 ? 0 : 1;
    }
    fprintf(stderr, "usage: sphere_walk_links walk <seed> | mutants <seed>\n");
    return 2;
}
