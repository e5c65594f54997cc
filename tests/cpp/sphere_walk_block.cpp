// CPU check of the sphere walk's block of node steps (csrc/rt_sphere_walk.h: sphere_walk_block, the
// code the path kernel runs) against the one-node-at-a-time walk written out below (node_step /
// node_visit of rt_walk.h for a sphere-only scene: a lane that holds a leaf waits, a leaf takes its
// skip link).
//
//   sphere_walk_block walk <seed>
//     Every lane (a ray with its slab constants, slack and pruning limit, a start node and a start
//     `pending`) is walked twice in lockstep, a block of kSteps at a time: by sphere_walk_block and
//     by kSteps single steps of the reference. After every block (node, pending) must be equal and
//     so must the nodes visited in it, in order. Between blocks a lane that holds a leaf is either
//     "tested" (pending cleared, the limit moved to below / at / above that leaf's box entry or
//     kept) or left waiting into the next block; a finished lane runs two more blocks.
//     Trees: BVHs of sphere_bvh.cpp over a random and a clustered sphere set in the 8 octant
//     layouts with plain and (near, far) ordered boxes, a one-node tree, an empty tree
//     (node_end == 0, node 0 readable and poisoned), a hand-made tree with NaN box planes.
//     Rays: all 8 octants, zero direction components of either sign, origins with the tree behind
//     them (far_t < 0 inside and outside -slack), limits below / at / above the root's entry.
//     kSteps 1, 3, 4, 5, 6, 8.
//     -> "ok walk lanes <n> blocks <n> visits <n> ..." and the coverage counts it asserts on
//   sphere_walk_block mutants <seed>
//     The same comparison with two broken block walks in place of the header's -- a leaf that goes
//     on to node + 1 instead of its skip link, a waiting lane that is allowed to move -- must
//     report a mismatch for each. -> "ok mutants detected 2"
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
    std::vector<V4> nodes;  // 2 per node; at least one readable node
    uint32_t node_end = 0;  // nodes of all layouts
    uint32_t stride = 0;    // nodes per octant layout (0: one layout)
    bool ordered = false;   // (near, far) corners per layout
    float extent = 30.0f, r_min = 0.2f, r_max = 1.0f;
};

static void push_node(Tree& t, const float lo[3], uint32_t skip, const float hi[3], uint32_t leaf) {
    t.nodes.push_back(V4{lo[0], lo[1], lo[2], from_bits(skip)});
    t.nodes.push_back(V4{hi[0], hi[1], hi[2], from_bits(leaf)});
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
    t.node_end = (uint32_t)all.size();
    t.stride = (uint32_t)sl.nodes.size();
    t.ordered = ordered;
    t.extent = sl.extent;
    t.r_min = sl.r_min;
    t.r_max = sl.r_max;
    return t;
}

// ---- the reference: one node at a time (rt_walk.h: node_step, node_visit, kBlockLeaves) ------
struct StepInfo {
    bool walked = false, at_leaf = false, ended = false;
    float near_t = 0.0f, far_t = 0.0f;
};
static StepInfo ref_step(const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node, uint32_t& pending,
                         std::vector<uint32_t>& seq) {
    StepInfo si;
    if (pending != kNone) return si;     // waits for the block's group tests
    if (node >= t.node_end) return si;   // the walk is over
    const V4 lo = t.nodes[2u * node], hi = t.nodes[2u * node + 1u];
    float near_t, far_t;
    if (t.ordered)
        slab_hit_ordered(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    const bool hit = near_t <= far_t && far_t >= -slack && near_t <= limit;
    const uint32_t leaf = bits(hi.w);
    const bool at_leaf = hit && leaf != 0xffffffffu;
    seq.push_back(node);
    if (at_leaf) pending = leaf & 0xffffffu;
    node = (hit && !at_leaf) ? node + 1u : bits(lo.w);
    si.walked = true;
    si.at_leaf = at_leaf;
    si.ended = !at_leaf && node >= t.node_end;
    si.near_t = near_t;
    si.far_t = far_t;
    return si;
}

// ---- the block walks under test ---------------------------------------------------------------
struct Record {
    std::vector<uint32_t>* seq;
    void operator()(bool walk, bool, uint32_t node) const {
        if (walk) seq->push_back(node);
    }
};

template <int kSteps>
static void header_block_n(const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node, uint32_t& pending,
                           std::vector<uint32_t>& seq) {
    if (t.ordered)
        sphere_walk_block<kSteps, true>(t.nodes.data(), t.node_end, sr, slack, limit, node, pending, Record{&seq});
    else
        sphere_walk_block<kSteps, false>(t.nodes.data(), t.node_end, sr, slack, limit, node, pending, Record{&seq});
}
static void header_block(int steps, const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node,
                         uint32_t& pending, std::vector<uint32_t>& seq) {
    switch (steps) {
        case 1: return header_block_n<1>(t, sr, slack, limit, node, pending, seq);
        case 3: return header_block_n<3>(t, sr, slack, limit, node, pending, seq);
        case 4: return header_block_n<4>(t, sr, slack, limit, node, pending, seq);
        case 5: return header_block_n<5>(t, sr, slack, limit, node, pending, seq);
        case 6: return header_block_n<6>(t, sr, slack, limit, node, pending, seq);
        case 8: return header_block_n<8>(t, sr, slack, limit, node, pending, seq);
    }
    printf("FAILED: no instantiation for %d steps\n", steps);
    exit(1);
}

// Broken walks (the `mutants` mode): 1 = a leaf goes on to node + 1, 2 = a waiting lane moves.
static int g_mutant = 0;
static void mutant_block(int steps, const Tree& t, const SlabRay& sr, float slack, float limit, uint32_t& node,
                         uint32_t& pending, std::vector<uint32_t>& seq) {
    for (int k = 0; k < steps; k++) {
        const bool walk = (g_mutant == 2 || pending == kNone) && node < t.node_end;
        if (!walk) continue;
        const V4 lo = t.nodes[2u * node], hi = t.nodes[2u * node + 1u];
        float near_t, far_t;
        if (t.ordered)
            slab_hit_ordered(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
        else
            slab_hit(sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
        const bool hit = near_t <= far_t && far_t >= -slack && near_t <= limit;
        const uint32_t leaf = bits(hi.w);
        const bool at_leaf = hit && leaf != 0xffffffffu;
        seq.push_back(node);
        if (at_leaf) pending = leaf & 0xffffffu;
        node = (hit && (!at_leaf || g_mutant == 1)) ? node + 1u : bits(lo.w);
    }
}

typedef void (*BlockFn)(int, const Tree&, const SlabRay&, float, float, uint32_t&, uint32_t&, std::vector<uint32_t>&);

// ---- coverage ---------------------------------------------------------------------------------
struct Coverage {
    long lanes = 0, blocks = 0, visits = 0;
    long enter_waiting = 0, enter_done = 0;
    long leaf_at[3] = {0, 0, 0}, end_at[3] = {0, 0, 0};  // first / middle / last step of a block
    long far_neg_in = 0, far_neg_out = 0;                // far_t < 0: >= -slack, < -slack
    long near_below = 0, near_at = 0, near_above = 0;    // near_t against the limit (finite limits)
    long nan_box = 0, inf_slope = 0;
    uint32_t octants = 0;
};
static int pos_of(int k, int steps) { return k == 0 ? 0 : k == steps - 1 ? 2 : 1; }

struct Lane {
    SlabRay sr;
    float slack, limit;
    uint32_t node, pending;
};

// Walks one lane with `block` and with the reference; false (and a message) on the first difference.
static bool run_lane(const Tree& t, Lane ln, int steps, BlockFn block, uint32_t seed, Coverage& cv, bool quiet) {
    std::mt19937 rng(seed);
    uint32_t an = ln.node, ap = ln.pending, rn = ln.node, rp = ln.pending;
    float limit = ln.limit;
    std::vector<uint32_t> sa, sr;
    int after_done = 0;
    cv.lanes++;
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
        float leaf_near = 0.0f;
        for (int k = 0; k < steps; k++) {
            const StepInfo si = ref_step(t, ln.sr, ln.slack, limit, rn, rp, sr);
            if (!si.walked) continue;
            cv.visits++;
            if (si.at_leaf) {
                cv.leaf_at[pos_of(k, steps)]++;
                leaf_near = si.near_t;
            }
            if (si.ended) cv.end_at[pos_of(k, steps)]++;
            if (si.far_t < 0.0f) (si.far_t >= -ln.slack ? cv.far_neg_in : cv.far_neg_out)++;
            if (std::isfinite(limit) && si.near_t <= si.far_t)
                (si.near_t < limit ? cv.near_below : si.near_t == limit ? cv.near_at : cv.near_above)++;
        }
        block(steps, t, ln.sr, ln.slack, limit, an, ap, sa);
        cv.blocks++;
        if (an != rn || ap != rp || sa != sr) {
            if (!quiet) {
                printf("MISMATCH steps %d block %ld: block walk (node %u pending %x, %zu visits) reference (node %u pending %x, "
                       "%zu visits)\n", steps, blk, an, ap, sa.size(), rn, rp, sr.size());
                for (size_t i = 0; i < std::max(sa.size(), sr.size()); i++)
                    printf("  visit %zu: %d / %d\n", i, i < sa.size() ? (int)sa[i] : -1, i < sr.size() ? (int)sr[i] : -1);
            }
            return false;
        }
        if (rp == kNone && rn >= t.node_end) {
            if (++after_done == 3) return true;
            continue;
        }
        if (rp != kNone && rng() % 3u != 0u) {  // the group test: pending cleared, the limit moved
            switch (rng() % 5u) {
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
    for (int k = 0; k < 3; k++) cv.inf_slope += std::isinf(inv[k]);
    ln.sr = slab_ray(o[0], o[1], o[2], inv[0], inv[1], inv[2], lateral);
    const uint32_t oct = octant_of(ln.sr);
    cv.octants |= 1u << oct;
    if (t.ordered) slab_pair_by_octant(ln.sr);
    ln.node = oct * t.stride;
    ln.pending = kNone;
    ln.limit = INFINITY;
    return ln;
}

// near / far of a node for this lane.
static void node_range(const Tree& t, const Lane& ln, uint32_t node, float& near_t, float& far_t) {
    const V4 lo = t.nodes[2u * node], hi = t.nodes[2u * node + 1u];
    if (t.ordered)
        slab_hit_ordered(ln.sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(ln.sr, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
}

static const int kStepSizes[] = {1, 3, 4, 5, 6, 8};

// All block sizes over one lane and its variants of limit, slack, start node and start pending.
static bool run_variants(const Tree& t, const Lane& base, BlockFn block, std::mt19937& rng, Coverage& cv, bool quiet) {
    float near0 = 0.0f, far0 = 0.0f;
    if (t.node_end) node_range(t, base, base.node, near0, far0);
    for (int steps : kStepSizes) {
        std::vector<Lane> v;
        v.push_back(base);
        if (t.node_end && near0 <= far0) {  // the root's entry against the limit: below, at, above
            for (float lim : {std::nextafter(near0, -INFINITY), near0, std::nextafter(near0, INFINITY), near0 + 1.0f}) {
                Lane l = base;
                l.limit = lim;
                v.push_back(l);
            }
        }
        if (t.node_end && far0 < 0.0f) {  // the tree behind the origin: inside and outside -slack
            for (float s : {0.0f, -far0 * 0.5f, -far0, std::nextafter(-far0, 0.0f), -far0 * 2.0f, INFINITY}) {
                Lane l = base;
                l.slack = s;
                v.push_back(l);
            }
        }
        {  // enters its first block waiting at a leaf; already past the end (with and without a leaf)
            Lane l = base;
            l.pending = 8u;
            v.push_back(l);
            for (uint32_t n : {t.node_end, t.node_end + 7u, 0xfffffff0u}) {
                l = base;
                l.node = n;
                v.push_back(l);
                l.pending = 4u;
                v.push_back(l);
            }
            if (t.node_end > 1) {  // starts in the middle of the tree
                l = base;
                l.node = base.node + rng() % std::max(1u, (t.stride ? t.stride : t.node_end) - 1u);
                v.push_back(l);
            }
        }
        for (const Lane& l : v)
            if (!run_lane(t, l, steps, block, (uint32_t)rng(), cv, quiet)) return false;
    }
    return true;
}

static bool run_tree(const Tree& t, BlockFn block, std::mt19937& rng, int n_rays, Coverage& cv, bool quiet) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (int r = 0; r < n_rays; r++) {
        float o[3], d[3];
        const int kind = r % 8;
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
        if (kind == 5)  // pointing away from the scene: everything behind the origin
            for (int k = 0; k < 3; k++) {
                o[k] = 40.0f * (U(rng) > 0.0f ? 1.0f : -1.0f) + U(rng);
                d[k] = std::copysign(std::fabs(d[k]) + 0.05f, o[k]);
            }
        if (kind == 6)
            for (int k = 0; k < 3; k++) d[k] *= 1e-6f;
        if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
        const Lane base = make_lane(t, o, d, cv);
        if (!run_variants(t, base, block, rng, cv, quiet)) return false;
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
    t.node_end = 1;
    return t;
}
// node_end == 0; node 0 is readable and poisoned: a box every ray enters, a leaf record.
static Tree empty_tree() {
    Tree t;
    const float lo[3] = {-1e6f, -1e6f, -1e6f}, hi[3] = {1e6f, 1e6f, 1e6f};
    push_node(t, lo, 0u, hi, 20u | (1u << 24));
    t.node_end = 0;
    return t;
}
// NaN planes: one, several, all of a box, in internal nodes and leaves.
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
    push_node(t, L, 9u, H, 0xffffffffu);    // 0 root
    push_node(t, l1, 5u, h1, 0xffffffffu);  // 1 internal, one NaN plane
    push_node(t, l2, 3u, h2, 0u | (4u << 24));   // 2 leaf, one NaN plane
    push_node(t, l3, 4u, h3, 4u | (4u << 24));   // 3 leaf, all NaN: never entered
    push_node(t, l1, 5u, h1, 8u | (2u << 24));   // 4 leaf
    push_node(t, l4, 9u, h4, 0xffffffffu);  // 5 internal
    push_node(t, l5, 7u, h5, 12u | (4u << 24));  // 6 leaf, an axis all NaN: unconstrained
    push_node(t, l3, 8u, h3, 0xffffffffu);  // 7 internal, all NaN: skipped
    push_node(t, l6, 9u, h6, 16u | (3u << 24));  // 8 leaf
    t.node_end = 9;
    return t;
}

static bool run_all(BlockFn block, unsigned seed, Coverage& cv, bool quiet) {
    std::mt19937 rng(seed);
    const std::vector<rt_scene_sphere> rnd = random_spheres(rng, 180), clu = clustered_spheres(rng, 30);
    for (int ordered = 0; ordered < 2; ordered++) {
        if (!run_tree(tree_of(rnd, ordered != 0), block, rng, 160, cv, quiet)) return false;
        if (!run_tree(tree_of(clu, ordered != 0), block, rng, 160, cv, quiet)) return false;
        Tree one = one_node_tree(), none = empty_tree(), nn = nan_tree();
        one.ordered = none.ordered = nn.ordered = ordered != 0;
        if (!run_tree(one, block, rng, 64, cv, quiet)) return false;
        if (!run_tree(none, block, rng, 32, cv, quiet)) return false;
        const long v0 = cv.visits;
        if (!run_tree(nn, block, rng, 96, cv, quiet)) return false;
        cv.nan_box += cv.visits - v0;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc > 2 && strcmp(argv[1], "walk") == 0) {
        Coverage cv;
        if (!run_all(header_block, (unsigned)atoi(argv[2]), cv, false)) return 1;
        const bool covered = cv.octants == 0xffu && cv.enter_waiting > 0 && cv.enter_done > 0 &&
                             std::min({cv.leaf_at[0], cv.leaf_at[1], cv.leaf_at[2]}) > 0 &&
                             std::min({cv.end_at[0], cv.end_at[1], cv.end_at[2]}) > 0 &&
                             std::min(cv.far_neg_in, cv.far_neg_out) > 0 &&
                             std::min({cv.near_below, cv.near_at, cv.near_above}) > 0 && cv.nan_box > 0 &&
                             cv.inf_slope > 0;
        printf("%s walk lanes %ld blocks %ld visits %ld octants %x enter_waiting %ld enter_done %ld leaf_at %ld %ld %ld end_at "
               "%ld %ld %ld far_neg %ld %ld near_vs_limit %ld %ld %ld nan_box_visits %ld inf_slopes %ld\n",
               covered ? "ok" : "FAILED (coverage)", cv.lanes, cv.blocks, cv.visits, cv.octants, cv.enter_waiting,
               cv.enter_done, cv.leaf_at[0], cv.leaf_at[1], cv.leaf_at[2], cv.end_at[0], cv.end_at[1], cv.end_at[2],
               cv.far_neg_in, cv.far_neg_out, cv.near_below, cv.near_at, cv.near_above, cv.nan_box, cv.inf_slope);
        return covered ? 0 : 1;
    }
    if (argc > 2 && strcmp(argv[1], "mutants") == 0) {
        int detected = 0;
        for (g_mutant = 1; g_mutant <= 2; g_mutant++) {
            Coverage cv;
            if (!run_all(mutant_block, (unsigned)atoi(argv[2]), cv, true))
                detected++;
            else
                printf("FAILED: mutant %d passes the comparison\n", g_mutant);
        }
        g_mutant = 0;
        Coverage cv;
        if (!run_all(mutant_block, (unsigned)atoi(argv[2]), cv, false)) {  // the unbroken copy must pass
            printf("FAILED: the unbroken copy of the walk does not pass\n");
            return 1;
        }
        printf("%s mutants detected %d\n", detected == 2 ? "ok" : "FAILED", detected);
        return detected == 2 ? 0 : 1;
    }
    fprintf(stderr, "usage: sphere_walk_block walk <seed> | mutants <seed>\n");
    return 2;
}
