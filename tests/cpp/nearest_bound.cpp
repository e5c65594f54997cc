// nearest_bound.cpp -- CPU harness for the certified box bound of rt_nearest.
//
// Compiles rt_nearest_math.h, the text the kernel compiles, with sphere_bvh.cpp, the builder the
// library runs. On built sphere BVHs and triangle accelerators, over random and adversarial points
// (|p| from 1e-3 to 1e15, points inside boxes, on faces of boxes, on primitives; the primitives
// touch their boxes' walls by construction, and a vertex fl(a + ab) may sit an ulp outside):
//   bound   every node's and leaf's bound against the contract key of every primitive below it;
//   walk    the stackless skip walk's result, with and without the greedy descent before it (the
//           point's own octant layout and a random one, plain and ordered sphere boxes), against
//           the sweep's, and box_holds_triangle on every sub-object and on a triangle with an
//           infinite edge in a finite, wrong box (finite keys below the box's bound: refuted);
//   mutants a bound without the shrink must violate `bound`, and a non-strict cull must lose a tie
//           (shown with the tightest certified bound there is, the smallest key below the node:
//           with it ties at the bound are the rule, and the strict cull still finds the sweep's
//           winner).
// usage: nearest_bound walk|mutants SEED
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rt_abi.h"
#include "rt_nearest_math.h"
#include "sphere_bvh.h"

using rtn::V3;

namespace {

struct Best {
    float key = INFINITY;
    uint32_t order = rtn::kNoOrder;
    bool operator==(const Best& o) const { return std::memcmp(&key, &o.key, 4) == 0 && order == o.order; }
};

void offer(Best& b, float key, uint32_t order, float maxd) {
    if (rtn::candidate_wins(key, order, maxd, b.key, b.order)) {
        b.key = key;
        b.order = order;
    }
}

// A hierarchy with its primitives' keys behind one interface: spheres (leaves of 4 slots) or
// triangles (a leaf is one sub-object).
struct Tree {
    std::vector<SphereBvhNode> nodes;  // the layouts, concatenated (stride: one layout's nodes)
    uint32_t stride = 0;
    float abs_part = 0.0f;
    bool spheres = false;
    // spheres
    SphereSlots slots;
    std::vector<rt_scene_sphere> sph;
    // triangles
    TriangleAccel acc;
    std::vector<rt_scene_triangle> tris;
    std::vector<rt_sub_object_info> subs;

    // every primitive of leaf record `leaf` offered for p
    template <class F>
    void leaf_prims(uint32_t leaf, V3 p, F f) const {
        if (spheres) {
            const uint32_t slot = leaf & 0xffffffu;
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t orig = slots.slot_orig[slot + k];
                if (orig == kSphereDummyOrig) continue;
                float l;
                const float* s = &slots.slot_sph[4 * (slot + k)];
                f(rtn::sphere_key(rtn::v3(s[0], s[1], s[2]), std::fabs(sph[orig].radius), p, l), rtn::kSphereOrder + orig);
            }
        } else {
            const SubObjectPrim& pr = acc.prims[leaf & 0xffffffu];
            const rt_sub_object_info& sub = subs[pr.sub];
            for (uint32_t j = 0; j < sub.triangle_count; j++) {
                const rt_scene_triangle& t = tris[sub.first_triangle_index + j];
                const rtn::TriNearest r = rtn::tri_nearest(rtn::v3(t.a[0], t.a[1], t.a[2]),
                                                           rtn::v3(t.edge_ab[0], t.edge_ab[1], t.edge_ab[2]),
                                                           rtn::v3(t.edge_ac[0], t.edge_ac[1], t.edge_ac[2]), p);
                f(rtn::point_key(r.q, p), pr.seq_base + j);
            }
        }
    }

    // the smallest key below `node` (its subtree is [node, skip) in pre-order within its layout)
    float min_key_below(uint32_t node, V3 p) const {
        const uint32_t base = node - node % stride;
        uint32_t end = nodes[node].skip;
        if (end > base + stride) end = base + stride;
        float m = INFINITY;
        for (uint32_t i = node; i < end; i++)
            if (nodes[i].leaf != kSphereBvhInternal)
                leaf_prims(nodes[i].leaf, p, [&](float key, uint32_t) {
                    if (key < m) m = key;
                });
        return m;
    }

    Best sweep(V3 p, float maxd) const {
        Best b;
        for (uint32_t i = 0; i < stride; i++)
            if (nodes[i].leaf != kSphereBvhInternal)
                leaf_prims(nodes[i].leaf, p, [&](float key, uint32_t order) { offer(b, key, order, maxd); });
        return b;
    }

    float bound_of(uint32_t node, V3 p) const {
        const SphereBvhNode& n = nodes[node];
        return rtn::box_bound(n.bmin[0], n.bmin[1], n.bmin[2], n.bmax[0], n.bmax[1], n.bmax[2], p, abs_part);
    }

    // the kernel's walk (near_step) from the root of layout `oct`, after its greedy descent to one
    // leaf (near_descend) when `descend`; kTight: the smallest key below the node for a bound
    template <bool kTight, bool kStrict>
    Best walk(uint32_t oct, V3 p, float maxd, uint64_t* culled, bool descend = false) const {
        Best b;
        float limit = maxd;
        uint32_t node = oct * stride;
        const uint32_t total = (uint32_t)nodes.size();
        for (uint32_t depth = 0, at = node; descend && depth < 64u && at < total; ++depth) {
            const SphereBvhNode& n = nodes[at];
            if (n.leaf != kSphereBvhInternal) {
                leaf_prims(n.leaf, p, [&](float key, uint32_t order) {
                    offer(b, key, order, maxd);
                    limit = std::fmin(b.key, maxd);
                });
                break;
            }
            const uint32_t left = at + 1u;
            if (left >= total) break;
            const uint32_t right = nodes[left].skip;
            at = left;
            if (right > left && right < total && bound_of(right, p) < bound_of(left, p)) at = right;
        }
        uint64_t steps = 0;
        while (node < total) {
            if (++steps > 4u * total) {
                std::printf("FAIL walk does not terminate\n");
                std::exit(1);
            }
            const SphereBvhNode& n = nodes[node];
            const float bound = kTight ? min_key_below(node, p) : bound_of(node, p);
            const bool enter = !rtn::bound_culls<kStrict>(bound, limit);
            if (!enter && culled) ++*culled;
            const bool at_leaf = enter && n.leaf != kSphereBvhInternal;
            if (at_leaf)
                leaf_prims(n.leaf, p, [&](float key, uint32_t order) {
                    offer(b, key, order, maxd);
                    limit = std::fmin(b.key, maxd);
                });
            node = (enter && !at_leaf) ? node + 1u : n.skip;
        }
        return b;
    }
};

struct Rng {
    std::mt19937_64 g;
    float uni(float a, float b) { return a + (b - a) * (float)((g() >> 11) * (1.0 / 9007199254740992.0)); }
    uint32_t below(uint32_t n) { return (uint32_t)(g() % n); }
};

Tree sphere_tree(Rng& r, uint32_t n, float offset, bool ordered) {
    Tree t;
    t.spheres = true;
    for (uint32_t i = 0; i < n; i++) {
        rt_scene_sphere s{};
        if (i >= 6 && i % 9 < 6 && i % 9 != 0) {
            s = t.sph[i - i % 9];  // runs of six identical spheres: ties across leaves
        } else {
            for (int k = 0; k < 3; k++) s.position[k] = offset + r.uni(-10.f, 10.f);
            s.radius = r.uni(0.05f, 1.5f) * (i % 5 == 0 ? -1.0f : 1.0f);  // hollow shells too
        }
        t.sph.push_back(s);
    }
    build_sphere_slots(t.sph.data(), n, true, &t.slots);
    t.stride = (uint32_t)t.slots.nodes.size();
    order_bvh_by_octant(t.slots.nodes, &t.nodes, ordered && box_layout_orderable(t.slots.nodes));
    t.abs_part = rtn::sphere_abs_part(t.slots.extent);
    return t;
}

Tree triangle_tree(Rng& r, uint32_t n_subs, float offset, float size) {
    Tree t;
    std::vector<rt_object_info> objs;
    for (uint32_t s = 0; s < n_subs; s++) {
        rt_sub_object_info sub{};
        sub.first_triangle_index = (uint32_t)t.tris.size();
        sub.triangle_count = 1 + r.below(7);
        float c[3];
        for (int k = 0; k < 3; k++) c[k] = offset + r.uni(-10.f, 10.f);
        for (int k = 0; k < 3; k++) sub.min_bounds[k] = INFINITY, sub.max_bounds[k] = -INFINITY;
        for (uint32_t j = 0; j < sub.triangle_count; j++) {
            float v[3][3];
            for (int i = 0; i < 3; i++)
                for (int k = 0; k < 3; k++) v[i][k] = c[k] + r.uni(-size, size);
            const uint32_t kind = r.below(16);
            if (kind == 0) std::memcpy(v[2], v[1], 12);                                   // a zero edge
            if (kind == 1) for (int k = 0; k < 3; k++) v[2][k] = v[0][k] + 2.0f * (v[1][k] - v[0][k]);  // collinear
            if (kind == 2) std::memcpy(v[1], v[0], 12), std::memcpy(v[2], v[0], 12);      // a point
            rt_scene_triangle tr{};
            for (int k = 0; k < 3; k++) {
                tr.a[k] = v[0][k];
                tr.edge_ab[k] = v[1][k] - v[0][k];
                tr.edge_ac[k] = v[2][k] - v[0][k];
                // the box of the vertices as given: fl(a + ab) may sit an ulp outside
                for (int i = 0; i < 3; i++) {
                    sub.min_bounds[k] = std::fmin(sub.min_bounds[k], v[i][k]);
                    sub.max_bounds[k] = std::fmax(sub.max_bounds[k], v[i][k]);
                }
            }
            t.tris.push_back(tr);
        }
        t.subs.push_back(sub);
    }
    for (uint32_t s = 0; s < n_subs;) {  // objects of 1..4 sub-objects
        rt_object_info o{};
        o.first_sub_object_index = s;
        o.sub_object_count = std::min<uint32_t>(1 + r.below(4), n_subs - s);
        s += o.sub_object_count;
        objs.push_back(o);
    }
    build_triangle_accel(objs.data(), (uint32_t)objs.size(), t.subs.data(), (uint32_t)t.subs.size(), &t.acc);
    t.stride = (uint32_t)t.acc.nodes.size();
    order_bvh_by_octant(t.acc.nodes, &t.nodes, false);
    t.abs_part = rtn::tri_abs_part(t.acc.extent);
    return t;
}

struct Counts {
    uint64_t pairs = 0, nodes = 0, points = 0, culled = 0, walks = 0, ties = 0, inside = 0, on_face = 0, far = 0,
             bound_zero = 0, bound_pos = 0, violations = 0, mismatches = 0, boxes_ok = 0, degenerate_nan = 0;
};

// The points of one tree: the classes the header names.
std::vector<V3> points_for(const Tree& t, Rng& r, uint32_t n, Counts& c) {
    std::vector<V3> pts;
    for (uint32_t i = 0; i < n; i++) {
        const SphereBvhNode& nd = t.nodes[r.below(t.stride)];
        V3 p;
        switch (i % 5) {
            case 0: {  // any magnitude from 1e-3 to 1e15
                const float m = std::pow(10.0f, r.uni(-3.f, 15.f));
                p = rtn::v3(r.uni(-1.f, 1.f) * m, r.uni(-1.f, 1.f) * m, r.uni(-1.f, 1.f) * m);
                c.far += m > 1e6f;
                break;
            }
            case 1:  // inside a node's box
                p = rtn::v3(r.uni(nd.bmin[0], nd.bmax[0]), r.uni(nd.bmin[1], nd.bmax[1]), r.uni(nd.bmin[2], nd.bmax[2]));
                c.inside++;
                break;
            case 2: {  // on a face of a node's box
                p = rtn::v3(r.uni(nd.bmin[0], nd.bmax[0]), r.uni(nd.bmin[1], nd.bmax[1]), r.uni(nd.bmin[2], nd.bmax[2]));
                const uint32_t k = r.below(3);
                (&p.x)[k] = r.below(2) ? nd.bmin[k] : nd.bmax[k];
                c.on_face++;
                break;
            }
            case 3: {  // just off a node's box, by a few ulps to a few percent
                p = rtn::v3(r.uni(nd.bmin[0], nd.bmax[0]), r.uni(nd.bmin[1], nd.bmax[1]), r.uni(nd.bmin[2], nd.bmax[2]));
                const uint32_t k = r.below(3);
                const float w = nd.bmax[k] - nd.bmin[k] + 1e-3f;
                (&p.x)[k] = nd.bmax[k] + w * std::pow(10.0f, r.uni(-7.f, -1.f));
                break;
            }
            default:  // around the scene
                p = rtn::v3(r.uni(-25.f, 25.f), r.uni(-25.f, 25.f), r.uni(-25.f, 25.f));
        }
        pts.push_back(p);
    }
    return pts;
}

template <bool kShrink>
void check_bounds(const Tree& t, const std::vector<V3>& pts, Counts& c) {
    for (const V3& p : pts) {
        c.points++;
        for (uint32_t node = 0; node < t.stride; node++) {
            const SphereBvhNode& n = t.nodes[node];
            const float bound = rtn::box_bound<kShrink>(n.bmin[0], n.bmin[1], n.bmin[2], n.bmax[0], n.bmax[1], n.bmax[2], p, t.abs_part);
            const float m = t.min_key_below(node, p);  // (NaN keys are no candidates: min ignores them)
            c.nodes++;
            c.pairs += (n.skip < t.stride ? n.skip : t.stride) - node;
            c.bound_zero += bound <= 0.0f;
            c.bound_pos += bound > 0.0f;
            if (bound > m) c.violations++;
        }
    }
}

void check_walks(const Tree& t, const std::vector<V3>& pts, Rng& r, Counts& c) {
    for (const V3& p : pts) {
        const Best free = t.sweep(p, INFINITY);
        const float maxds[4] = {INFINITY, free.key, std::nextafter(free.key, -INFINITY), free.key * r.uni(0.5f, 4.f)};
        for (float maxd : maxds) {
            const Best want = t.sweep(p, maxd);
            const SphereBvhNode& root = t.nodes[0];
            const uint32_t own = rtn::point_octant(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], p);
            for (uint32_t oct : {own, (uint32_t)r.below(8)}) {  // the heuristic's layout, and any other
                const Best got = t.walk<false, true>(oct, p, maxd, nullptr);
                const Best head = t.walk<false, true>(oct, p, maxd, &c.culled, true);  // with the descent
                c.walks++;
                if (!(got == want) || !(head == want)) c.mismatches++;
            }
        }
        // ties: how many primitives share the winner's key
        uint32_t same = 0;
        for (uint32_t i = 0; i < t.stride; i++)
            if (t.nodes[i].leaf != kSphereBvhInternal)
                t.leaf_prims(t.nodes[i].leaf, p, [&](float key, uint32_t) { same += key == free.key; });
        c.ties += same > 1;
    }
}

void check_boxes(const Tree& t, Counts& c) {
    for (const rt_sub_object_info& sub : t.subs)
        for (uint32_t j = 0; j < sub.triangle_count; j++) {
            const rt_scene_triangle& tr = t.tris[sub.first_triangle_index + j];
            const V3 a = rtn::v3(tr.a[0], tr.a[1], tr.a[2]), ab = rtn::v3(tr.edge_ab[0], tr.edge_ab[1], tr.edge_ab[2]),
                     ac = rtn::v3(tr.edge_ac[0], tr.edge_ac[1], tr.edge_ac[2]);
            if (!rtn::box_holds_triangle(sub.min_bounds, sub.max_bounds, a, ab, ac)) c.mismatches++;
            c.boxes_ok++;
            // shrunk towards its centre by a tenth of its largest side (and at least a little): refuted
            float mn[3], mx[3], side = 0.0f;
            for (int k = 0; k < 3; k++) side = std::fmax(side, sub.max_bounds[k] - sub.min_bounds[k]);
            for (int k = 0; k < 3; k++) {
                const float mid = 0.5f * (sub.min_bounds[k] + sub.max_bounds[k]);
                mn[k] = mid - 0.4f * (sub.max_bounds[k] - sub.min_bounds[k]) + 0.01f * side + 1e-3f;
                mx[k] = mn[k];
            }
            if (rtn::box_holds_triangle(mn, mx, a, ab, ac) && side > 0.1f) c.mismatches++;
        }
}

// A triangle with an infinite edge inside a finite, wrong box: its keys are finite through the
// regions that do not touch the edge, the box's bound exceeds them, so the box check must refute it
// (and pass it in a non-finite box, which the accelerator replaces by an all-enclosing one).
void check_infinite_edge(Counts& c) {
    const V3 a = rtn::v3(0.f, 0.f, 0.f), ab = rtn::v3(INFINITY, 0.f, 0.f), ac = rtn::v3(0.f, 1.f, 0.f);
    const float mn[3] = {100.f, 100.f, 100.f}, mx[3] = {101.f, 101.f, 101.f};
    const float open_mx[3] = {101.f, INFINITY, 101.f};
    const V3 pts[3] = {rtn::v3(-1.f, -1.f, 0.f), rtn::v3(-1.f, 2.f, 0.f), rtn::v3(-0.5f, 0.5f, 0.2f)};
    const uint32_t regions[3] = {1u, 4u, 5u};
    for (int i = 0; i < 3; i++) {
        const rtn::TriNearest r = rtn::tri_nearest(a, ab, ac, pts[i]);
        const float key = rtn::point_key(r.q, pts[i]);
        const float bound = rtn::box_bound(mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], pts[i], rtn::tri_abs_part(101.f));
        if (!(r.feature == regions[i] && key < 2.0f && bound > 100.0f)) c.mismatches++;  // the premise
        c.degenerate_nan++;
    }
    if (rtn::box_holds_triangle(mn, mx, a, ab, ac)) c.mismatches++;
    if (!rtn::box_holds_triangle(mn, open_mx, a, ab, ac)) c.mismatches++;
    // anything non-finite in a, ab, ac or the rebuilt vertices refutes a finite box
    const V3 bad[4] = {rtn::v3(NAN, 0.f, 0.f), rtn::v3(0.f, -INFINITY, 0.f), rtn::v3(3e38f, 0.f, 0.f), rtn::v3(0.f, 0.f, NAN)};
    const V3 one = rtn::v3(100.5f, 100.5f, 100.5f), e = rtn::v3(0.1f, 0.f, 0.f), f = rtn::v3(0.f, 0.1f, 0.f);
    if (!rtn::box_holds_triangle(mn, mx, one, e, f)) c.mismatches++;
    for (const V3& v : bad) {
        if (rtn::box_holds_triangle(mn, mx, v, e, f)) c.mismatches++;
        if (rtn::box_holds_triangle(mn, mx, one, v, f)) c.mismatches++;
        if (rtn::box_holds_triangle(mn, mx, one, e, v)) c.mismatches++;
    }
    // (3e38 for an edge: finite itself, fl(a + ab) overflows)
    if (rtn::box_holds_triangle(mn, mx, rtn::v3(3e38f, 100.5f, 100.5f), rtn::v3(3e38f, 0.f, 0.f), f)) c.mismatches++;
}

int fail(const char* what, const Counts& c) {
    std::printf("FAIL %s violations %llu mismatches %llu\n", what, (unsigned long long)c.violations, (unsigned long long)c.mismatches);
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool mutants = std::strcmp(argv[1], "mutants") == 0;
    Rng r{std::mt19937_64(std::strtoull(argv[2], nullptr, 10))};
    std::vector<Tree> trees;
    trees.push_back(sphere_tree(r, 200, 0.0f, false));
    trees.push_back(sphere_tree(r, 120, 0.0f, true));
    trees.push_back(sphere_tree(r, 90, 3000.0f, false));  // far from the origin: coarse coordinates
    trees.push_back(triangle_tree(r, 80, 0.0f, 0.8f));
    trees.push_back(triangle_tree(r, 60, 0.0f, 0.01f));   // small triangles
    trees.push_back(triangle_tree(r, 50, 5000.0f, 0.5f));
    if (mutants) {
        int detected = 0;
        Counts c;
        for (const Tree& t : trees) check_bounds<false>(t, points_for(t, r, 150, c), c);
        detected += c.violations > 0;  // the raw box distance exceeds a key somewhere
        uint64_t lost = 0, kept = 0;
        for (const Tree& t : trees) {
            Counts d;
            for (const V3& p : points_for(t, r, 150, d)) {
                const Best want = t.sweep(p, INFINITY);
                for (uint32_t oct = 0; oct < 8; oct++) {
                    kept += t.walk<true, true>(oct, p, INFINITY, nullptr) == want;
                    lost += !(t.walk<true, false>(oct, p, INFINITY, nullptr) == want);
                }
            }
        }
        if (kept != 6u * 150u * 8u) return fail("the strict cull with the tightest bound loses a winner", c);
        detected += lost > 0;
        std::printf("no_shrink_violations %llu non_strict_lost %llu\n", (unsigned long long)c.violations, (unsigned long long)lost);
        std::printf(detected == 2 ? "ok mutants detected 2\n" : "FAIL mutants detected %d\n", detected);
        return detected == 2 ? 0 : 1;
    }
    Counts c;
    for (const Tree& t : trees) {
        const std::vector<V3> pts = points_for(t, r, 250, c);
        check_bounds<true>(t, pts, c);
        check_walks(t, pts, r, c);
        if (!t.spheres) check_boxes(t, c);
    }
    check_infinite_edge(c);
    if (c.violations || c.mismatches) return fail("walk", c);
    // the coverage this run must have had
    if (!(c.pairs > 1000000 && c.culled > 50000 && c.ties > 20 && c.inside >= 300 && c.on_face >= 300 && c.far > 100 &&
          c.bound_zero > 5000 && c.bound_pos > 100000 && c.boxes_ok > 500 && c.degenerate_nan == 3))
        return fail("coverage", c), std::printf("pairs %llu culled %llu ties %llu far %llu zero %llu pos %llu boxes %llu\n",
                                                 (unsigned long long)c.pairs, (unsigned long long)c.culled,
                                                 (unsigned long long)c.ties, (unsigned long long)c.far,
                                                 (unsigned long long)c.bound_zero, (unsigned long long)c.bound_pos,
                                                 (unsigned long long)c.boxes_ok), 1;
    std::printf("ok walk points %llu nodes %llu pairs %llu walks %llu culled %llu ties %llu inside %llu on_face %llu far %llu "
                "bound_zero %llu bound_pos %llu boxes %llu\n",
                (unsigned long long)c.points, (unsigned long long)c.nodes, (unsigned long long)c.pairs,
                (unsigned long long)c.walks, (unsigned long long)c.culled, (unsigned long long)c.ties,
                (unsigned long long)c.inside, (unsigned long long)c.on_face, (unsigned long long)c.far,
                (unsigned long long)c.bound_zero, (unsigned long long)c.bound_pos, (unsigned long long)c.boxes_ok);
    return 0;
}
