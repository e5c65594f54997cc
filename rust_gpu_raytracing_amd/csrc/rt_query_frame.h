// rt_query_frame.h -- the frame the query kernels stand on (query.hip, occlusion.hip,
// radiance.hip): one ray per lane, persistent wave64s that take chunks of
// consecutive rays, the three scene placements of the path kernel, the traversal step, and the
// host-side occupancy and launch of an instance. The walk itself is rt_walk.h's.
//
// rt_occlusion_kernel keeps its own copy of the staging: the shared form costs SGPR spills there
// (DESIGN.md §5.4b has the figures, and those of the forms of query_traverse that were tried).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_abi.h"
#include "rt_path_common.h"
#include "rt_query_schedule.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

namespace {

// ---- the scene view and its LDS image ----------------------------------------------------------
//
// Mode 0 reads everything from global memory, mode 1 stages spheres / objects / the sphere BVH in
// LDS once per workgroup, mode 2 also the triangle accelerator: the path kernel's image at the
// path kernel's offsets (ka.lds_*), of which each kernel stages the tables it reads. Every piece
// is called by the whole workgroup and followed by one __syncthreads() in the kernel.

// The view of the scene in global memory, with the quantized triangle nodes of modes 0 and 1
// hooked up when the scene has them. `srgb`: the table shading reads (null: a kernel that does not
// shade).
template <int kMode, bool kTris>
__device__ __forceinline__ SceneView global_scene_view(const KernelArgs& ka, const float* srgb) {
    SceneView sv{ka.sphere_slots, ka.sphere_orig, ka.sphere_material, ka.sphere_bvh, ka.materials, nullptr,
                 ka.objects,      srgb,           ka.tri_bvh,         ka.tri_prims,  kTris ? *ka.tri_extent : 0.0f,
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
    return sv;
}

// Modes 1 and 2, what every walk reads: sphere slots and their original indices, the sphere BVH,
// the objects.
template <bool kTris, uint32_t kThreads>
__device__ __forceinline__ SceneView stage_walk_tables(const KernelArgs& ka, unsigned char* lds, SceneView sv) {
    const uint32_t tid = threadIdx.x;
    float4* l_sph = reinterpret_cast<float4*>(lds);
    RtObject* l_obj = reinterpret_cast<RtObject*>(lds + ka.lds_obj_offset);
    uint32_t* l_orig = reinterpret_cast<uint32_t*>(lds + ka.lds_orig_offset);
    float4* l_nodes = reinterpret_cast<float4*>(lds + ka.lds_nodes_offset);
    for (uint32_t i = tid; i < ka.sphere_slot_count; i += kThreads) {
        l_sph[i] = ka.sphere_slots[i];
        l_orig[i] = ka.sphere_orig[i];
    }
    for (uint32_t i = tid; i < 2u * ka.sphere_nodes; i += kThreads) l_nodes[i] = ka.sphere_bvh[i];
    if constexpr (kTris)
        for (uint32_t i = tid; i < ka.object_count; i += kThreads) l_obj[i] = ka.objects[i];
    sv.sph = l_sph;
    sv.orig = l_orig;
    sv.nodes = l_nodes;
    sv.obj = l_obj;
    return sv;
}

// Modes 1 and 2, what a hit record reads beyond the walk: the spheres' material indices.
template <uint32_t kThreads>
__device__ __forceinline__ SceneView stage_sphere_materials(const KernelArgs& ka, unsigned char* lds, SceneView sv) {
    uint32_t* l_smat = reinterpret_cast<uint32_t*>(lds + ka.lds_smat_offset);
    for (uint32_t i = threadIdx.x; i < ka.sphere_count; i += kThreads) l_smat[i] = ka.sphere_material[i];
    sv.sph_mat = l_smat;
    return sv;
}

// Modes 1 and 2, what shading reads (shade<true>): the materials, their glass constants and 1x1
// texels, and the sRGB table.
template <uint32_t kThreads>
__device__ __forceinline__ SceneView stage_shading_tables(const KernelArgs& ka, unsigned char* lds, SceneView sv) {
    const uint32_t tid = threadIdx.x;
    RtMaterial* l_mat = reinterpret_cast<RtMaterial*>(lds + ka.lds_mat_offset);
    float4* l_aux = reinterpret_cast<float4*>(lds + ka.lds_mat_aux_offset);
    float* l_srgb = reinterpret_cast<float*>(lds + ka.lds_srgb_offset);
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
    for (uint32_t i = tid; i < 256u; i += kThreads) l_srgb[i] = ka.srgb[i];
    sv.mat = l_mat;
    sv.mat_aux = l_aux;
    sv.srgb = l_srgb;
    return sv;
}

// Mode 2: the triangle accelerator's nodes and leaves, and the sub-objects when they fit.
template <uint32_t kThreads>
__device__ __forceinline__ SceneView stage_triangle_tables(const KernelArgs& ka, unsigned char* lds, SceneView sv) {
    const uint32_t tid = threadIdx.x;
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
    return sv;
}

// The search state of a lane that holds no ray: no walk in progress, both bests at `best`.
__device__ __forceinline__ TraceState idle_trace_state(float best) {
    TraceState ts;
    ts.inv = mk(0.f, 0.f, 0.f);
    ts.a4 = ts.a2 = 0.f;
    ts.node = 0;
    ts.phase = 2;
    ts.pending = kNoLeaf;
    ts.nan_hit = false;
    ts.sph = SphereHit{best, 0u, 0u};
    ts.tri = TriHit{best, 0u, 0u, 0u, false};
    return ts;
}

// ---- chunks of rays ----------------------------------------------------------------------------

// The chunk schedule of a launch (rt_query_schedule.h), as the kernels read it: embedded in
// QueryArgs and OcclusionArgs. RadianceArgs carries the same five fields by the same names in its
// own order (claim_chunk reads either): its instances' SGPR spills follow the order of the kernel
// arguments, and every order with this block embedded cost some instance spills.
struct ChunkArgs {
    unsigned long long count;               // rays of the launch
    unsigned long long* __restrict__ next;  // the chunk counter (zero at launch)
    uint32_t wave_chunk;                    // rays per claim
    uint32_t first_chunk;                   // rays of each wave's own first chunk (no claim)
    unsigned long long claimed_from;        // first ray handed out by the counter: first_chunk x the launch's waves
};

inline ChunkArgs chunk_args(uint64_t count, unsigned long long* counter, const rtq::QuerySchedule& s, uint32_t threads) {
    const unsigned long long waves = (unsigned long long)s.blocks * (threads / 64u);
    return ChunkArgs{count, counter, s.rest_chunk, s.first_chunk, waves * s.first_chunk};
}

// The wave's chunk [next, end) of the ray array, wave-uniform; `dry`: no rays are left for this
// wave. `first`: the wave has not taken its own first chunk yet.
struct WaveChunk {
    unsigned long long next, end;
    bool first, dry;
};

// The index of this wave in the launch.
template <uint32_t kThreads>
__device__ __forceinline__ uint32_t wave_in_launch() {
    return __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64u) + (threadIdx.x >> 6));
}

// The wave's next chunk of rays (called by whole waves). The first chunk is the wave's own, by its
// index in the launch: were it claimed, every resident wave's first claim would queue at one
// counter address while nothing else runs. After it lane 0 claims from the counter, which hands
// out the rays from ca.claimed_from on; a launch whose first chunks cover every ray claims nothing.
// (Reading the counter before claiming, to spare the claim that comes back empty, doubled the run
// time of 2M rays: a load of that line queues with the claims. DESIGN.md §5.4c.)
// kOwnFirst false: the closest-hit kernel's schedule, which has no first chunks: it enters with
// c.first false, its launch has claimed_from 0, and every call claims (the two are compile-time
// facts here so that the kernel does not hold claimed_from in registers).
// `ca`: a ChunkArgs, or an argument struct with its fields. The chunk state is updated in place and
// the fields are read where they are used: both kept every instance at its register figures.
template <bool kOwnFirst = true, class Args>
__device__ __forceinline__ void claim_chunk(const Args& ca, uint32_t wave, WaveChunk& c) {
    unsigned long long base = ca.count, chunk = ca.wave_chunk;
    if (kOwnFirst && c.first) {
        base = (unsigned long long)wave * ca.first_chunk;
        chunk = ca.first_chunk;
        c.first = false;
    }
    if (!kOwnFirst || (base >= ca.count && ca.claimed_from < ca.count)) {
        unsigned long long got = ca.count;
        if ((threadIdx.x & 63u) == 0) got = atomicAdd(ca.next, (unsigned long long)ca.wave_chunk);
        const uint32_t b_lo = __builtin_amdgcn_readfirstlane((uint32_t)got);
        const uint32_t b_hi = __builtin_amdgcn_readfirstlane((uint32_t)(got >> 32));
        base = (kOwnFirst ? ca.claimed_from : 0ull) + (((unsigned long long)b_hi << 32) | b_lo);
        chunk = ca.wave_chunk;
    }
    c.dry = base >= ca.count;
    c.next = c.dry ? ca.count : base;
    c.end = (c.dry || base + chunk >= ca.count) ? ca.count : base + chunk;
}

// The refill's rank of an idle lane: how many idle lanes (`need`: their ballot) are below it, so
// that the idle lanes take the chunk's next rays in order.
__device__ __forceinline__ uint32_t rank_among(uint64_t need) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
}

// ---- directions drawn on the device ------------------------------------------------------------

// Step 2 of the gather contract (and of the ambient contract, which refers to it): the direction
// of the sample with index u of a point with normal n, used as given. The gather instance of
// rt_radiance_kernel and rt_ambient_kernel both call this, so both hold the same bits.
__device__ __forceinline__ f3 gather_direction(f3 n, uint32_t stream, uint32_t u) {
    uint32_t dseed = (stream * u * 326624u) ^ 0x9E3779B9u;
    const float gx = normal01(dseed);
    const float gy = normal01(dseed);
    const float gz = normal01(dseed);
    return normalize(n + mk(gx, gy, gz));
}

// Steps A to D of the lens contract (include/rt_abi.h; radiance.hip repeats it): the ray (o, d) of
// pixel `pixel` of the descriptor's image for the sample index u of its stream. The lens instance
// of rt_radiance_kernel and rt_lens_rays_kernel both call this, so both hold the same bits. `cam`
// is device memory read at wave-uniform addresses; the host has checked kind, width and height.
// (The ray comes back by value from one exit: with two out-pointers and a return per kind the
// callers' o and d went through scratch memory.)
struct LensRay {
    f3 o, d;
};

__device__ __forceinline__ LensRay lens_ray(const rt_lens_camera* __restrict__ cam, uint32_t pixel, uint32_t stream,
                                            uint32_t u) {
    const uint32_t y = pixel / cam->width, x = pixel - y * cam->width;
    const f3 origin = mk(cam->origin[0], cam->origin[1], cam->origin[2]);
    if (cam->kind == RT_LENS_EQUIRECT) {
        const float uc = ((float)x + 0.5f) / (float)cam->width;
        const float vc = ((float)y + 0.5f) / (float)cam->height;
        const float az = (uc - 0.5f) * kTwoPiWgsl;
        const float el = (vc - 0.5f) * kWgslPi;
        const float ce = cosf_c(el);
        return LensRay{origin,
                       mk(ce * cosf_c(az), cosf_c(el - 1.5707963705062866f), ce * cosf_c(az - 1.5707963705062866f))};
    }
    const float xc = (float)x / (float)cam->width;
    const float yc = (float)y / (float)cam->height;
    const float nx = xc * 2.0f - 1.0f;
    const float ny = yc * 2.0f - 1.0f;
    const float ax = nx * cam->aspect;
    // in view space: the direction v and, for the kinds that leave the origin, the offset (px, py, 0)
    f3 v = mk(0.0f, 0.0f, -1.0f);
    float px = 0.0f, py = 0.0f;
    bool shifted = true;
    if (cam->kind == RT_LENS_ORTHOGRAPHIC) {
        px = ax * cam->ortho_half_height;
        py = ny * cam->ortho_half_height;
    } else {
        float tw;
        const f3 t = mat4_mul_xyz(cam->inverse_projection, ax, ny, 1.0f, 1.0f, tw);
        const f3 ws = normalize(mk(t.x / tw, t.y / tw, t.z / tw));
        if (cam->aperture == 0.0f) {  // camera_ray (rt_path_common.h), operation for operation
            v = ws;
            shifted = false;
        } else {
            uint32_t lseed = (stream * u * 326624u) ^ 0x85EBCA6Bu;
            const float r1 = random01(lseed);
            const float r2 = random01(lseed);
            const float rad = cam->aperture * sqrt_rn_any(r1);
            const float th = kBoxMullerTwoPi * r2;
            px = rad * cosf_c(th);
            py = rad * cosf_c(th - 1.5707963705062866f);
            const float k = cam->focus / (0.0f - ws.z);
            const f3 f = ws * k;
            v = normalize(mk(f.x - px, f.y - py, f.z));
        }
    }
    float unused;
    const f3 d = mat4_mul_xyz(cam->inverse_view, v.x, v.y, v.z, 0.0f, unused);
    const f3 off = mat4_mul_xyz(cam->inverse_view, px, py, 0.0f, 0.0f, unused);
    return LensRay{shifted ? origin + off : origin, d};
}

// ---- the traversal step --------------------------------------------------------------------------

// Lane states. A lane owns one ray at a time.
constexpr uint32_t kLaneIdle = 0, kLaneSetup = 1, kLaneTrav = 2, kLaneDone = 3;

// What a lane carries through the traversal: its search (TraceState, field by field, the bools as
// words: no padding, so that copies by value carry nothing else) and its state.
struct LaneWalk {
    f3 inv;
    float a4, a2;
    SlabRay slab;
    float slack, limit;
    uint32_t node, phase, pending;
    float cert_gap;
    uint32_t nan_hit;
    SphereHit sph;
    float tri_t;
    uint32_t tri_seq, tri_tri, tri_obj, tri_front;
    uint32_t mode;
};

__device__ __forceinline__ LaneWalk lane_walk(const TraceState& s, uint32_t mode) {
    static_assert(sizeof(TraceState) == 116, "a field was added to TraceState: carry it in LaneWalk");
    return LaneWalk{s.inv, s.a4, s.a2, s.slab, s.slack, s.limit, s.node, s.phase, s.pending, s.cert_gap,
                    s.nan_hit ? 1u : 0u, s.sph, s.tri.t, s.tri.seq, s.tri.tri, s.tri.obj, s.tri.front ? 1u : 0u, mode};
}

__device__ __forceinline__ void take_lane_walk(const LaneWalk& w, TraceState& ts, uint32_t& mode) {
    ts.inv = w.inv;
    ts.a4 = w.a4;
    ts.a2 = w.a2;
    ts.slab = w.slab;
    ts.slack = w.slack;
    ts.limit = w.limit;
    ts.node = w.node;
    ts.phase = w.phase;
    ts.pending = w.pending;
    ts.cert_gap = w.cert_gap;
    ts.nan_hit = w.nan_hit != 0u;
    ts.sph = w.sph;
    ts.tri.t = w.tri_t;
    ts.tri.seq = w.tri_seq;
    ts.tri.tri = w.tri_tri;
    ts.tri.obj = w.tri_obj;
    ts.tri.front = w.tri_front != 0u;
    mode = w.mode;
}

// What ends a step of a closest-hit search: phase_end, and the lane is done when its walks are.
struct WalkEnd {
    template <bool kTris>
    __device__ __forceinline__ void step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                         uint32_t& mode) const {
        phase_end<kTris>(sv, ka, o, d, ts);
        if (ts.phase == 2) mode = kLaneDone;
    }
};

// Step 4 of the query kernels, the path kernel's (pathtrace.hip, step 4): the wave traverses until
// at most trav_threshold lanes still do, so that finished lanes are written (or shaded) and
// refilled together; with no rays left (`dry`) it traverses to the end -- or, with kDrain on the
// instances whose triangle accelerator stays in global memory, decouples the drain by the path
// kernel's rule (drain_threshold, drain_min_steps). (o, d): the lane's ray. `end`: what ends a
// step (WalkEnd, or the any-hit search's own).
template <int kMode, bool kTris, bool kDrain, class End>
__device__ __forceinline__ LaneWalk query_traverse(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, LaneWalk in,
                                                   bool dry, unsigned char* lds, End end) {
    TraceState ts;
    uint32_t mode;
    take_lane_walk(in, ts, mode);
    uint32_t thresh = dry ? 0u : ka.trav_threshold;
    uint32_t n_active = 64u, min_steps = 0u;
    if constexpr (kDrain && kDrainDecouple<kMode, kTris>) {
        if (dry) {
            thresh = ka.drain_threshold;
            n_active = (uint32_t)__popcll(__ballot(mode == kLaneTrav || mode == kLaneDone));
            min_steps = ka.drain_min_steps;
        }
    }
    while (true) {
        const uint64_t trav = __ballot(mode == kLaneTrav);
        const uint32_t n_trav = (uint32_t)__popcll(trav);
        if constexpr (kDrain && kDrainDecouple<kMode, kTris>) {
            if (trav == 0 || (n_trav <= thresh && n_trav < n_active && min_steps == 0)) break;
            min_steps -= min_steps != 0;
        } else {
            if (n_trav <= thresh || trav == 0) break;
        }
        bool leaves = false;
        if constexpr (kDeferLeaves<kTris> && !kFusedLeaves<kMode, kTris>) {
            const uint32_t n_pend = (uint32_t)__popcll(__ballot(mode == kLaneTrav && ts.pending != kNoLeaf));
            leaves = 8u * n_pend >= ka.leaf_batch * n_trav;
        }
        bool batched = false;
        if constexpr (kCoopLeaves<kMode, kTris>) {
            if (leaves && ka.tri_leaftris) {  // the wave's deferred leaves, cooperatively
                const bool act = mode == kLaneTrav && ts.pending != kNoLeaf;
                coop_leaf_batch(sv, ka, o, d, ts, act, lds);
                if (act) end.template step<kTris>(sv, ka, o, d, ts, mode);
                batched = true;
            }
        }
        if (!batched && mode == kLaneTrav && (!leaves || ts.pending != kNoLeaf)) {
            if (kDeferLeaves<kTris> && leaves) {
                leaf_step<kTris, (kMode <= 1)>(sv, ka, o, d, ts);
            } else {
                node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
            }
            end.template step<kTris>(sv, ka, o, d, ts, mode);
            if (!(kDeferLeaves<kTris> && leaves)) {
#pragma unroll
                for (int k = 1; k < kTravUnroll<kMode, kTris>; ++k) {
                    if (mode == kLaneTrav) {
                        node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
                        end.template step<kTris>(sv, ka, o, d, ts, mode);
                    }
                }
            }
            if constexpr (kFusedLeaves<kMode, kTris>) {
                // the leaf batch after the block's node steps: one kind of leaf per batch
                const uint64_t mt = __ballot(mode == kLaneTrav && ts.pending != kNoLeaf && ts.phase == 0);
                const uint64_t ms = __ballot(mode == kLaneTrav && ts.pending != kNoLeaf && ts.phase != 0);
                const uint32_t n_p = (uint32_t)__popcll(mt | ms);
                const uint32_t n_t = (uint32_t)__popcll(__ballot(mode == kLaneTrav));
                const bool tri_first = __popcll(mt) >= __popcll(ms);
                if (8u * n_p >= ka.leaf_batch * n_t && mode == kLaneTrav && ts.pending != kNoLeaf &&
                    (ts.phase == 0) == tri_first) {
                    leaf_step<kTris, (kMode <= 1)>(sv, ka, o, d, ts);
                    end.template step<kTris>(sv, ka, o, d, ts, mode);
                }
            }
            if constexpr (kBlockLeaves<kTris>) {
                // the block's group tests: every lane that reached a leaf in it, together
                const uint32_t n_wait = (uint32_t)__popcll(__ballot(ts.pending != kNoLeaf));
                const uint32_t n_tr = (uint32_t)__popcll(__ballot(true));
                if (8u * n_wait >= kBlockLeafShare * n_tr && mode == kLaneTrav && ts.pending != kNoLeaf) {
                    test_sphere_group(sv, ts.pending, o, d, ts.a4, ts.a2, ts.sph);
                    ts.limit = prune_limit(ts);
                    ts.pending = kNoLeaf;
                    end.template step<kTris>(sv, ka, o, d, ts, mode);
                }
            }
        }
    }
    return lane_walk(ts, mode);
}

// ---- instances on the host ---------------------------------------------------------------------

// Resident workgroups per CU of a kernel instance at this dynamic LDS size (0: it does not fit).
template <class K>
hipError_t query_occupancy_of(K kernel, uint32_t threads, size_t lds_bytes, int* blocks_per_cu) {
    if (lds_bytes > 64u * 1024u) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, kernel, threads, lds_bytes);
}

template <class K, class A>
hipError_t query_launch_of(K kernel, uint32_t threads, uint32_t blocks, size_t lds_bytes, hipStream_t stream,
                           const KernelArgs& ka, const A& qa) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, ka, qa);
    return hipGetLastError();
}

}  // namespace
