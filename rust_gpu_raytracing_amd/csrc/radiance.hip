// radiance.hip -- batched radiance queries for gfx950 (rt_radiance, rt_radiance_device; DESIGN.md
// §5.4e).
//
// rt_radiance_kernel answers "how much light arrives along this ray?" for arbitrary rays: per_pixel
// of the reference (compute_shader.wgsl:210-314) with the camera origin, the pixel's direction and
// the pixel index of the seed taken from a 32-B record, summed over `samples` samples. It stands on
// rt_query_kernel's frame (query.hip) -- one ray per lane, persistent wave64s claiming chunks of
// rays, ballot + mbcnt refill, the three scene placements, the walk of rt_walk.h -- and on the path
// kernel's shading (rt_path_common.h: trace_end, shade, Path). Nothing of the framebuffer is read
// or written. What differs from the closest-hit query:
//
//  * A lane keeps its ray for samples x (up to) bounces walks: when a walk finishes the lane
//    shades the hit (trace_end -> shade) and either starts the next segment of the path, or adds
//    the path's light to the ray's sum and starts the next sample, or writes the sum with one 16-B
//    store and goes idle. The samples of a ray run back to back on its lane, so the sum is added
//    in the contract's order.
//  * Shading runs in batches as in the path kernel (pathtrace.hip, step 4): lanes whose walk has
//    finished wait until at most trav_threshold lanes still traverse, then the wave shades and
//    refills them together.
//  * The scene image holds what shading reads too: in modes 1 and 2 the materials, their glass
//    constants and 1x1 texels, and the sRGB table are staged at the path kernel's offsets
//    (shade<true>); mode 0 reads materials and the table from global memory (shade<false>). Every
//    placement returns the same bits.
//  * Each wave's first chunk is its own, by its index in the launch, as in rt_occlusion_kernel.
//  * Counted ray segments (the rule of rt_ray_count: one per trace_ray call) are summed per lane,
//    reduced once per wave at exit and added to the caller's counter with one atomic per wave.
//
// Gather queries (rt_gather, rt_gather_device) run on the same kernel body,
// instantiated with kGather, and on rt_gather_resolve_kernel below. The contract, as in
// include/rt_abi.h:
//
// THE GATHER CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
// written order, with no contraction. For point i with record (x, stream, n):
//  1. Sample index and origin. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
//     o = x + n * 0.0001f per component: one multiply and one add (the reference's bounce
//     offset, as restated at oracle/pathtrace_oracle.c:511).
//  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
//     gx, gy, gz = normal_distribution(&dseed) three times, in that order
//     (compute_shader.wgsl:622-628, theta drawn before rho).
//     dir = normalize(n + (gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
//     dot(v, v) = (x*x + y*y) + z*z. n is used as given and is not normalised.
//  3. Path. L_s is the result rt_radiance defines for the record (o, stream, dir) with
//     first_sample = u, samples = 1 and the call's bounces: per_pixel with its own seed
//     stream * u * 326624u, its own jitter, and everything else of a frame.
//  4. Reduction. P_j (j = 0 .. 63) starts at +0.0f on all four channels. For s ascending,
//     P_{s mod 64} = P_{s mod 64} + L_s. Then, for off = 32, 16, 8, 4, 2, 1:
//     P_j = P_j + P_{j+off} for every j < off. radiance[i] = P_0. Lanes that got no sample
//     take part with +0.0f. (An xor butterfly gives the same bits on finite values, because
//     f32 addition commutes.)
// End of the gather contract.
//
//  * The work item is a (point, stripe) pair: stripe j of a point runs its samples j, j + 64, ...
//    back to back on one lane, which is step 4's P_j, and stores it among the point's 64
//    partials. Points with fewer than 64 samples have only `samples` stripes. Three places of
//    the body differ from a radiance query: the sample start (steps 1 and 2, then
//    start_sample_at), the sample stride, and where the sum goes.
//  * rt_gather_resolve_kernel runs step 4's tree: one wave per point, lane j loads P_j (one
//    coalesced 1 KB read; +0.0f for a stripe the point does not have), six shuffle levels in the
//    contract's order, one 16-B store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_path_common.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct RadianceArgs {
    const float4* __restrict__ rays;  // rt_radiance_ray[count]: {origin.xyz, stream}, {direction.xyz, pad}
    float4* __restrict__ radiance;    // one float4 per ray
    unsigned long long count;
    unsigned long long* __restrict__ next;      // the chunk counter (zero at launch)
    unsigned long long* __restrict__ segments;  // counted ray segments, added to (null: not counted)
    uint32_t wave_chunk;                        // rays per claim
    uint32_t first_chunk;                       // rays of each wave's own first chunk (no claim)
    unsigned long long claimed_from;            // first ray handed out by the counter: first_chunk x the launch's waves
    uint32_t first_sample;                      // random_index of a ray's first sample (:154)
    uint32_t samples;                           // samples per ray, >= 1 (ka.bounces >= 1 too: the host answers 0)
    uint32_t stripes;                           // kGather: stripes per point, min(samples, 64)
};

namespace {

// The wave's next chunk of rays, wave-uniform (called by whole waves): rt_occlusion_kernel's
// schedule (occlusion.hip). The first chunk is the wave's own, by its index in the launch; after
// it lane 0 claims from the counter, which hands out the rays from qa.claimed_from on.
__device__ __forceinline__ void claim_chunk(const RadianceArgs& qa, uint32_t wave, bool& first,
                                            unsigned long long& next, unsigned long long& end, bool& dry) {
    unsigned long long base = qa.count, chunk = qa.wave_chunk;
    if (first) {
        base = (unsigned long long)wave * qa.first_chunk;
        chunk = qa.first_chunk;
        first = false;
    }
    if (base >= qa.count && qa.claimed_from < qa.count) {
        unsigned long long got = qa.count;
        if ((threadIdx.x & 63u) == 0) got = atomicAdd(qa.next, (unsigned long long)qa.wave_chunk);
        const uint32_t b_lo = __builtin_amdgcn_readfirstlane((uint32_t)got);
        const uint32_t b_hi = __builtin_amdgcn_readfirstlane((uint32_t)(got >> 32));
        base = qa.claimed_from + (((unsigned long long)b_hi << 32) | b_lo);
        chunk = qa.wave_chunk;
    }
    dry = base >= qa.count;
    next = dry ? qa.count : base;
    end = (dry || base + chunk >= qa.count) ? qa.count : base + chunk;
}

}  // namespace

// kGather: the path kernel of a gather query (the contract above). A "ray" is then a (point,
// stripe) item: qa.rays holds rt_gather_point records, qa.count the launch's items (points x
// qa.stripes, below 2^32), and qa.radiance the partials, 64 float4 per point.
template <int kMode, bool kTris, uint32_t kThreads, bool kGather = false>
__global__ void __launch_bounds__(kThreads, 1) rt_radiance_kernel(KernelArgs ka, RadianceArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool kAux = kMode >= 1;
    const uint32_t tid = threadIdx.x;
    SceneView sv{ka.sphere_slots, ka.sphere_orig, ka.sphere_material, ka.sphere_bvh, ka.materials, nullptr,
                 ka.objects,      ka.srgb,        ka.tri_bvh,         ka.tri_prims,  kTris ? *ka.tri_extent : 0.0f,
                 ka.sub_objects};
    if constexpr (kTris && kMode <= 1) {
        if (ka.tri_qnodes) {
            const float4 g0 = ka.tri_qgrid[0], g1 = ka.tri_qgrid[1];
            if (g0.w != 0.0f) {
                sv.tri_q = ka.tri_qnodes;
                sv.qox = g0.x;
                sv.qoy = g0.y;
                sv.qoz = g0.z;
                sv.qsx = g1.x;
                sv.qsy = g1.y;
                sv.qsz = g1.z;
            }
        }
    }
    // The path kernel's LDS image at the same offsets, without the camera block.
    if constexpr (kMode >= 1) {
        float4* l_sph = reinterpret_cast<float4*>(lds);
        RtMaterial* l_mat = reinterpret_cast<RtMaterial*>(lds + ka.lds_mat_offset);
        float4* l_aux = reinterpret_cast<float4*>(lds + ka.lds_mat_aux_offset);
        RtObject* l_obj = reinterpret_cast<RtObject*>(lds + ka.lds_obj_offset);
        uint32_t* l_orig = reinterpret_cast<uint32_t*>(lds + ka.lds_orig_offset);
        uint32_t* l_smat = reinterpret_cast<uint32_t*>(lds + ka.lds_smat_offset);
        float4* l_nodes = reinterpret_cast<float4*>(lds + ka.lds_nodes_offset);
        float* l_srgb = reinterpret_cast<float*>(lds + ka.lds_srgb_offset);
        for (uint32_t i = tid; i < ka.sphere_slot_count; i += kThreads) {
            l_sph[i] = ka.sphere_slots[i];
            l_orig[i] = ka.sphere_orig[i];
        }
        for (uint32_t i = tid; i < ka.sphere_count; i += kThreads) l_smat[i] = ka.sphere_material[i];
        for (uint32_t i = tid; i < 2u * ka.sphere_nodes; i += kThreads) l_nodes[i] = ka.sphere_bvh[i];
        for (uint32_t i = tid; i < ka.material_count; i += kThreads) {
            const RtMaterial m = ka.materials[i];
            l_mat[i] = m;
            // shade()'s glass constants, by the same f32 operations (:320, :328-334, :307)
            const float ior_front = 1.0f / m.refraction_index;
            float r0f = (1.0f - ior_front) / (1.0f + ior_front);
            float r0b = (1.0f - m.refraction_index) / (1.0f + m.refraction_index);
            r0f = r0f * r0f;
            r0b = r0b * r0b;
            l_aux[2u * i] = make_float4(ior_front, r0f, r0b, div_const(m.roughness, 10.0f, kInv10));
            // the decoded texel a 1x1 texture layer gives every hit (sample_texture, :26-32)
            const f4 c = decode_texel(ka.textures[min(m.texture_index, ka.tex_layers - 1u)], ka.srgb);
            l_aux[2u * i + 1u] = make_float4(c.x, c.y, c.z, c.w);
        }
        if constexpr (kTris)
            for (uint32_t i = tid; i < ka.object_count; i += kThreads) l_obj[i] = ka.objects[i];
        for (uint32_t i = tid; i < 256u; i += kThreads) l_srgb[i] = ka.srgb[i];
        sv.sph = l_sph;
        sv.orig = l_orig;
        sv.sph_mat = l_smat;
        sv.nodes = l_nodes;
        sv.mat = l_mat;
        sv.mat_aux = l_aux;
        sv.obj = l_obj;
        sv.srgb = l_srgb;
    }
    if constexpr (kMode == 2) {
        float4* l_tn = reinterpret_cast<float4*>(lds + ka.lds_tri_nodes_offset);
        uint4* l_tp = reinterpret_cast<uint4*>(lds + ka.lds_tri_prims_offset);
        for (uint32_t i = tid; i < 2u * ka.tri_nodes; i += kThreads) l_tn[i] = ka.tri_bvh[i];
        for (uint32_t i = tid; i < ka.tri_prim_count; i += kThreads) l_tp[i] = ka.tri_prims[i];
        sv.tri_nodes = l_tn;
        sv.tri_prims = l_tp;
        if (ka.lds_sub_offset) {
            RtSubObject* l_sub = reinterpret_cast<RtSubObject*>(lds + ka.lds_sub_offset);
            for (uint32_t i = tid; i < ka.sub_object_count; i += kThreads) l_sub[i] = ka.sub_objects[i];
            sv.sub = l_sub;
        }
    }
    if constexpr (kMode >= 1) __syncthreads();

    // Lane states. A lane owns one ray at a time and one segment of its current sample's path.
    constexpr uint32_t kIdle = 0, kSetup = 1, kTrav = 2, kDone = 3;
    uint32_t mode = kIdle;
    unsigned long long ray = 0;
    uint32_t sample = 0;
    uint32_t segs = 0;  // trace_ray calls of this lane's rays (a lane runs far fewer than 2^32)
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    Path p;
    p.o = p.d = mk(0.f, 0.f, 0.f);
    p.light = p.contrib = f4{0.f, 0.f, 0.f, 0.f};
    p.seed = p.bounce = 0;
    TraceState ts;
    ts.inv = mk(0.f, 0.f, 0.f);
    ts.a4 = ts.a2 = 0.f;
    ts.node = 0;
    ts.phase = 2;
    ts.pending = kNoLeaf;
    ts.nan_hit = false;
    ts.sph = SphereHit{kF32Max, 0u, 0u};
    ts.tri = TriHit{kF32Max, 0u, 0u, 0u, false};

    // Sample `sample` of the lane's ray: the record is read again (two 16-B loads that hit the
    // cache) instead of holding origin, direction and stream in 7 registers through every walk.
    // kGather: `ray` is point * 64 + stripe (the item's slot among the partials) and `sample` the
    // sample index s; the origin and the direction are steps 1 and 2 of the contract.
    auto begin_sample = [&]() {
        if constexpr (kGather) {
            const float4 r0 = qa.rays[2ull * (ray >> 6)], r1 = qa.rays[2ull * (ray >> 6) + 1ull];
            const f3 n = mk(r1.x, r1.y, r1.z);
            const uint32_t stream = __float_as_uint(r0.w), u = qa.first_sample + sample;
            uint32_t dseed = (stream * u * 326624u) ^ 0x9E3779B9u;
            const float gx = normal01(dseed);
            const float gy = normal01(dseed);
            const float gz = normal01(dseed);
            start_sample_at(mk(r0.x, r0.y, r0.z) + n * 0.0001f, stream, u, normalize(n + mk(gx, gy, gz)), p);
        } else {
            const float4 r0 = qa.rays[2ull * ray], r1 = qa.rays[2ull * ray + 1ull];
            start_sample_at(mk(r0.x, r0.y, r0.z), __float_as_uint(r0.w), qa.first_sample + sample,
                            mk(r1.x, r1.y, r1.z), p);
        }
        mode = kSetup;
    };

    // The wave's chunk [next, end) of the ray array, wave-uniform.
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64u) + (tid >> 6));
    bool first = true;
    unsigned long long next = 0, end = 0;
    bool dry = false;  // no rays are left for this wave
    claim_chunk(qa, wave, first, next, end, dry);

    while (true) {
        // 1. Shade the lanes whose walk has finished (:228-311). A path that ends adds its light
        // to the ray's sum (one f32 add per channel); then the ray's next sample, or its result.
        if (mode == kDone) {
            const Hit h = trace_end<kTris>(sv, ka, p.o, p.d, ts);
            ++segs;
            if (shade<kAux>(sv, ka, p, h)) {
                sum.x = sum.x + p.light.x;
                sum.y = sum.y + p.light.y;
                sum.z = sum.z + p.light.z;
                sum.w = sum.w + p.light.w;
                bool more;
                if constexpr (kGather) {  // the stripe's next sample, 64 on (no wrap: samples - sample >= 1)
                    more = qa.samples - sample > 64u;
                    sample += 64u;
                } else {
                    sample += 1;
                    more = sample < qa.samples;
                }
                if (more) {
                    begin_sample();
                } else {
                    qa.radiance[ray] = sum;
                    mode = kIdle;
                }
            } else {
                mode = kSetup;
            }
        }
        // 2. Refill: idle lanes take the chunk's next rays, in order.
        while (true) {
            const uint64_t need = __ballot(mode == kIdle);
            if (need == 0 || dry) break;
            const uint32_t avail = (uint32_t)(end - next);
            if (mode == kIdle) {
                const uint32_t rank =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                if (rank < avail) {
                    if constexpr (kGather) {
                        const uint32_t item = (uint32_t)(next + rank), point = item / qa.stripes;
                        sample = item - point * qa.stripes;
                        ray = (unsigned long long)point * 64u + sample;
                    } else {
                        ray = next + rank;
                        sample = 0;
                    }
                    sum = make_float4(0.f, 0.f, 0.f, 0.f);
                    begin_sample();
                }
            }
            next += min((uint32_t)__popcll(need), avail);
            if (next == end) claim_chunk(qa, wave, first, next, end, dry);
        }
        // 3. Start the next segment of every lane that has one (ka.bounces >= 1: a path that
        // reached the limit ended in shade).
        if (mode == kSetup) {
            trace_begin<kTris>(sv, ka, p.o, p.d, ts);
            mode = ts.phase == 2 ? kDone : kTrav;
        }
        if (__ballot(mode != kIdle) == 0 && dry) break;
        // 4. Traverse, as the path kernel does (pathtrace.hip, step 4): lanes whose walk finishes
        // wait until at most trav_threshold lanes still traverse, then the wave shades and refills
        // them together. With no rays left the wave traverses to the end before it shades, except
        // the instances whose triangle accelerator stays in global memory, which decouple the
        // drain by the path kernel's rule (drain_threshold, drain_min_steps).
        uint32_t thresh = dry ? 0u : ka.trav_threshold;
        uint32_t n_active = 64u, min_steps = 0u;
        if constexpr (kDrainDecouple<kMode, kTris>) {
            if (dry) {
                thresh = ka.drain_threshold;
                n_active = (uint32_t)__popcll(__ballot(mode == kTrav || mode == kDone));
                min_steps = ka.drain_min_steps;
            }
        }
        while (true) {
            const uint64_t trav = __ballot(mode == kTrav);
            const uint32_t n_trav = (uint32_t)__popcll(trav);
            if constexpr (kDrainDecouple<kMode, kTris>) {
                if (trav == 0 || (n_trav <= thresh && n_trav < n_active && min_steps == 0)) break;
                min_steps -= min_steps != 0;
            } else {
                if (n_trav <= thresh || trav == 0) break;
            }
            bool leaves = false;
            if constexpr (kDeferLeaves<kTris> && !kFusedLeaves<kMode, kTris>) {
                const uint32_t n_pend = (uint32_t)__popcll(__ballot(mode == kTrav && ts.pending != kNoLeaf));
                leaves = 8u * n_pend >= ka.leaf_batch * n_trav;
            }
            bool batched = false;
            if constexpr (kCoopLeaves<kMode, kTris>) {
                if (leaves && ka.tri_leaftris) {  // the wave's deferred leaves, cooperatively
                    const bool act = mode == kTrav && ts.pending != kNoLeaf;
                    coop_leaf_batch(sv, ka, p.o, p.d, ts, act, lds);
                    if (act) {
                        phase_end<kTris>(sv, ka, p.o, p.d, ts);
                        if (ts.phase == 2) mode = kDone;
                    }
                    batched = true;
                }
            }
            if (!batched && mode == kTrav && (!leaves || ts.pending != kNoLeaf)) {
                if (kDeferLeaves<kTris> && leaves) {
                    leaf_step<kTris, (kMode <= 1)>(sv, ka, p.o, p.d, ts);
                } else {
                    node_step<kTris, kCertWalk<kMode>>(sv, ka, p.o, p.d, ts);
                }
                phase_end<kTris>(sv, ka, p.o, p.d, ts);
                if (ts.phase == 2) mode = kDone;
                if (!(kDeferLeaves<kTris> && leaves)) {
#pragma unroll
                    for (int k = 1; k < kTravUnroll<kMode, kTris>; ++k) {
                        if (mode == kTrav) {
                            node_step<kTris, kCertWalk<kMode>>(sv, ka, p.o, p.d, ts);
                            phase_end<kTris>(sv, ka, p.o, p.d, ts);
                            if (ts.phase == 2) mode = kDone;
                        }
                    }
                }
                if constexpr (kFusedLeaves<kMode, kTris>) {
                    // the leaf batch after the block's node steps: one kind of leaf per batch
                    const uint64_t mt = __ballot(mode == kTrav && ts.pending != kNoLeaf && ts.phase == 0);
                    const uint64_t ms = __ballot(mode == kTrav && ts.pending != kNoLeaf && ts.phase != 0);
                    const uint32_t n_p = (uint32_t)__popcll(mt | ms);
                    const uint32_t n_t = (uint32_t)__popcll(__ballot(mode == kTrav));
                    const bool tri_first = __popcll(mt) >= __popcll(ms);
                    if (8u * n_p >= ka.leaf_batch * n_t && mode == kTrav && ts.pending != kNoLeaf &&
                        (ts.phase == 0) == tri_first) {
                        leaf_step<kTris, (kMode <= 1)>(sv, ka, p.o, p.d, ts);
                        phase_end<kTris>(sv, ka, p.o, p.d, ts);
                        if (ts.phase == 2) mode = kDone;
                    }
                }
                if constexpr (kBlockLeaves<kTris>) {
                    // the block's group tests: every lane that reached a leaf in it, together
                    const uint32_t n_wait = (uint32_t)__popcll(__ballot(ts.pending != kNoLeaf));
                    const uint32_t n_tr = (uint32_t)__popcll(__ballot(true));
                    if (8u * n_wait >= kBlockLeafShare * n_tr && mode == kTrav && ts.pending != kNoLeaf) {
                        test_sphere_group(sv, ts.pending, p.o, p.d, ts.a4, ts.a2, ts.sph);
                        ts.limit = prune_limit(ts);
                        ts.pending = kNoLeaf;
                        phase_end<kTris>(sv, ka, p.o, p.d, ts);
                        if (ts.phase == 2) mode = kDone;
                    }
                }
            }
        }
    }
    // The wave's counted segments: one reduction and one atomic per wave (the loop's exit is
    // wave-uniform, so all 64 lanes are here).
    if (qa.segments) {
        unsigned long long total = segs;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
        if ((tid & 63u) == 0 && total != 0) atomicAdd(qa.segments, total);
    }
}

// Step 4's tree of a gather query: one wave per point. Lane j holds P_j; after the level `off`
// the lanes below `off` hold the contract's P_j + P_{j+off} (the lanes above hold sums that nothing
// reads). Stripes the point does not have (samples < 64) take part with +0.0f.
constexpr uint32_t kResolveThreads = 256;
__global__ void __launch_bounds__(kResolveThreads) rt_gather_resolve_kernel(const float4* __restrict__ partials,
                                                                           float4* __restrict__ radiance,
                                                                           uint32_t points, uint32_t stripes) {
    const uint32_t point = blockIdx.x * (kResolveThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (point >= points) return;  // wave-uniform
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < stripes) v = partials[(size_t)point * 64u + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.x = v.x + __shfl_down(v.x, off, 64);
        v.y = v.y + __shfl_down(v.y, off, 64);
        v.z = v.z + __shfl_down(v.z, off, 64);
        v.w = v.w + __shfl_down(v.w, off, 64);
    }
    if (lane == 0) radiance[point] = v;
}

// Workgroup size by placement. The global-memory instance has no image to share: small workgroups,
// as the closest-hit query's. The staged instances share one image among as many waves as their
// registers allow without spilling: the walks from global memory with the shading state live need
// about 150 VGPRs (the path kernel's figure), which 16 waves per workgroup (128 each) would spill.
uint32_t rt_radiance_threads(int mode, bool tris) { return mode == 0 ? 256u : (tris && mode == 1) ? 512u : 1024u; }

// (mode, triangles, threads); each also as the gather instance
#define RT_FOR_EACH_RADIANCE(X) \
    X(0, true, 256) X(1, true, 512) X(2, true, 1024) X(0, false, 256) X(1, false, 1024)

template <class K>
static hipError_t radiance_occupancy_of(K kernel, uint32_t threads, size_t lds_bytes, int* blocks_per_cu) {
    if (lds_bytes > 64u * 1024u) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, kernel, threads, lds_bytes);
}

// Resident workgroups per CU of the instance at this dynamic LDS size (0: it does not fit).
hipError_t rt_radiance_occupancy(int mode, bool tris, bool gather, size_t lds_bytes, int* blocks_per_cu) {
#define RT_ROCC(M, TR, T)                                                                                  \
    if (mode == M && tris == TR)                                                                           \
        return gather ? radiance_occupancy_of(&rt_radiance_kernel<M, TR, T, true>, T, lds_bytes, blocks_per_cu) \
                      : radiance_occupancy_of(&rt_radiance_kernel<M, TR, T, false>, T, lds_bytes, blocks_per_cu);
    RT_FOR_EACH_RADIANCE(RT_ROCC)
#undef RT_ROCC
    return hipErrorInvalidValue;
}

// `stripes` 0: a radiance query of `count` rays. Otherwise the path kernel of a gather query:
// `rays` holds rt_gather_point records, `count` is the launch's items (points x stripes) and
// `radiance` receives the partials, 64 float4 per point.
hipError_t rt_launch_radiance(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, uint32_t blocks,
                              const void* rays, void* radiance, uint64_t count, unsigned long long* counter,
                              unsigned long long* segments, uint32_t wave_chunk, uint32_t first_chunk,
                              uint32_t first_sample, uint32_t samples, uint32_t stripes, hipStream_t stream) {
    if (blocks == 0 || count == 0) return hipSuccess;
    const unsigned long long waves = (unsigned long long)blocks * (rt_radiance_threads(mode, tris) / 64u);
    const RadianceArgs qa{static_cast<const float4*>(rays), static_cast<float4*>(radiance), count, counter, segments,
                          wave_chunk, first_chunk, waves * first_chunk, first_sample, samples, stripes};
#define RT_RLAUNCH(M, TR, T)                                                                                  \
    if (mode == M && tris == TR) {                                                                            \
        if (stripes)                                                                                          \
            hipLaunchKernelGGL((rt_radiance_kernel<M, TR, T, true>), dim3(blocks), dim3(T), lds_bytes, stream, ka, qa); \
        else                                                                                                  \
            hipLaunchKernelGGL((rt_radiance_kernel<M, TR, T, false>), dim3(blocks), dim3(T), lds_bytes, stream, ka, qa); \
        return hipGetLastError();                                                                             \
    }
    RT_FOR_EACH_RADIANCE(RT_RLAUNCH)
#undef RT_RLAUNCH
    return hipErrorInvalidValue;
}

// Step 4's tree over the partials of `points` points (stream-ordered after the path kernel).
hipError_t rt_launch_gather_resolve(const void* partials, void* radiance, uint32_t points, uint32_t stripes,
                                    hipStream_t stream) {
    if (points == 0) return hipSuccess;
    const uint32_t per_block = kResolveThreads / 64u;
    hipLaunchKernelGGL(rt_gather_resolve_kernel, dim3((points + per_block - 1u) / per_block), dim3(kResolveThreads), 0,
                       stream, static_cast<const float4*>(partials), static_cast<float4*>(radiance), points, stripes);
    return hipGetLastError();
}
