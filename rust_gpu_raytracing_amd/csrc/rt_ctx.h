// rt_ctx.h — what the host translation units share (private: installed nowhere).
//
// The context behind the opaque rt_ctx of include/rt_abi.h, the entry macros, the error and
// device-buffer helpers, and the declarations of the helpers that cross files. Who defines what:
//   rt_abi.cpp      errors, pinned staging and uploads, accelerator refresh, launch timing slots
//   rt_frames.cpp   the frame queue and the scene as a launch sees it (SceneLaunch and its carve)
//   rt_queries.cpp  query_enter, run_query
// Everything shared lives in namespace rth with hidden visibility: the library exports only the
// entry points that rt_abi.h declares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_abi.h"
#include "rt_kernel_args.h"
#include "rt_scene_math.h"
#include "sphere_bvh.h"
#include "tri_cone.h"

namespace rth {

// The defaults and limits of the context's tuning fields (rt_set_tuning, rt_abi.cpp).
// Tile queue: counters per stripe (pathtrace.hip, claim_tile), 256 B apart;
// kQueueStripes = 4 per XCD by default (measured: C2 0.599 ms at 8, 0.595 at 32; C1
// 0.076 -> 0.058 ms), up to kQueueStripesMax (rt_kernel_args.h, with kQueueStride).
constexpr uint32_t kQueueStripes = 32;
// Instances with the triangle accelerator in global memory: the traverse threshold
// (trav_threshold_for, rt_frames.cpp) once the tile queue is empty, when the wave goes back to shading only if some lane
// has finished and after at least kDefaultDrainMinSteps traversal steps
// (threshold 0: traverse to the end, as the other instances do).
constexpr uint32_t kDefaultDrainThreshold = 32;
constexpr uint32_t kDefaultDrainMinSteps = 64;
// Tile claim order: 0 = tile index order, 1 = cost-ordered (most rays first,
// sorted on the device from the previous frame's per-tile ray counts).
constexpr uint32_t kDefaultTileSchedule = 1;
// Ray queries (query.hip). rt_trace_rays stages its rays and records through pinned memory in
// chunks of this many rays (96 B each: 6 MiB pinned, 6 MiB of device scratch); tuning "query_chunk".
constexpr uint32_t kDefaultQueryChunk = 65536;
constexpr uint32_t kMaxQueryChunk = 1u << 24;
// Gather queries (radiance.hip) run in launches of at most this many points, 1 KB of partials
// each (16 MiB of context-owned scratch); tuning "gather_chunk".
constexpr uint32_t kDefaultGatherChunk = 16384;
constexpr uint32_t kMaxGatherChunk = 1u << 20;
// Probe queries (radiance.hip) run in launches of at most this many paths, 16 B of scratch each
// (16 MiB of context-owned scratch), but of one whole probe at least; tuning "probe_chunk".
constexpr uint32_t kDefaultProbeChunk = 1048576;
constexpr uint32_t kMaxProbeChunk = 1u << 26;
// Feature buffers (denoise.hip): the frame's camera rays are traced in bands of this many pixels,
// so the scratch of a band -- its rays and records, 96 B per pixel: 48 MiB -- does not grow with
// the frame (3840x2160 would take 800 MB at once); tuning "feature_band".
constexpr uint32_t kDefaultFeatureBand = 1u << 19;
constexpr uint32_t kMaxFeatureBand = 1u << 24;
// rt_ctx::near_boxes
constexpr int kNearBoxesUnknown = 0, kNearBoxesVouched = 1, kNearBoxesRefuted = 2;

}  // namespace rth

// The entry points are global (C linkage by their declarations in rt_abi.h) and call the shared
// helpers unqualified.
using namespace rth;

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    uint64_t n_pixels = 0;
    uint32_t rank = 0, world = 1;
    uint32_t tiles_x = 0, tiles_y = 0, owned_tiles = 0;

    rt_params params{};  // shadow of binding 0
    uint32_t k = 1;      // Renderer::accumulation_index (src/renderer.rs:37)
    rt_ray_camera camera{};
    // frame batching (rt_set_frame_batch): queued rt_compute_frame calls
    uint32_t frame_batch = RT_DEFAULT_FRAME_BATCH;  // frames per launch at most (1: one launch per frame)
    uint32_t pending_frames = 0;  // queued, not yet launched (their k already advanced)
    uint32_t pending_bounces = 0;
    bool frame_parallel = true;     // tuning "frame_parallel" 0: batches run frames back to back per lane
    float4* d_frame_light[2] = {};    // frame-parallel batch lights (by batch parity), owned px x frames x samples
    size_t frame_light_cap = 0;       // bytes, each
    // overlapped batches (dispatch_frames): batch i runs on streams[i % 2]
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_resolved[2] = {};   // after batch i's resolve (i % 2)
    hipEvent_t ev_aux_done = nullptr; // after the last work issued on aux_stream
    hipEvent_t ev_primary = nullptr;  // a point of the primary stream an aux batch waits for
    bool aux_outstanding = false;     // aux work the primary stream has not been ordered after yet
    bool primary_dirty = true;        // primary-stream work since then that an aux batch must follow
    uint64_t batches = 0;             // frame-parallel batches launched
    bool batch_overlap = true;        // tuning "batch_overlap" 0: every batch on the primary stream
    bool stage_subs = true;           // tuning "stage_subs" 0: mode 2 leaves read sub-objects from global
    // device memory the batch buffers (frame lights, primary records) may take: a batch that
    // would need more is rendered as several launches (dispatch_batch); tuning "batch_memory_mb"
    size_t batch_budget = 0;
    // 16-B quantized triangle nodes for walks from global memory (tuning "tri_qnodes" 0: the 32-B nodes)
    bool use_qnodes = true;
    bool qnodes_dirty = true;          // the binary accelerator changed since the copy was made
    bool derived_octants = false, derived_qnodes = false;  // what the last derivation produced
    uint4* d_tri_qnodes = nullptr;
    float4* d_tri_qgrid = nullptr;
    size_t qnodes_cap = 0;  // bytes
    bool batch_schedule = false;      // tuning "batch_schedule" 1: cost-ordered claims in batches too
    // tuning "frame_par_instance" 0: frame-parallel batches run the generic path kernel instance too
    bool frame_par_instance = true;
    // a tile's frames claimed one after another (C3 -12%, C4 -8%, C5 -4%, C2 -1.8% per frame
    // against frame-major, profiles/archive/r02_knobs2); tuning "unit_tile_major" 0: frame-major
    bool unit_tile_major = true;

    uint32_t cap_mat = 0, cap_sph = 0, cap_tri = 0, cap_obj = 0, cap_sub = 0;
    // extents the kernel clamps against (>= 1 so clamps never underflow)
    uint32_t n_mat_dev = 1, n_tri_dev = 1, n_sub_dev = 1;

    float4* d_rays = nullptr;
    float4* d_accum = nullptr;
    uint32_t* d_out = nullptr;
    unsigned long long* d_counter = nullptr;
    uint32_t* d_queue = nullptr;  // [stream][2] x kQueueStripesMax tile-queue counters, kQueueStride apart
    uint32_t queue_parity[2] = {0, 0};  // per stream: which half its next launch uses (the launch zeroes all of the other)
    uint32_t queue_stripes = kQueueStripes;  // tuning "queue_stripes"
    int n_cu = 0;
    bool force_global_scene = false;   // tuning "scene_in_lds" 0
    // the occupancy query's answer per path kernel instance (0 generic, 1 frame-parallel), so that a
    // context whose launches alternate instances (full batches and a one-frame remainder) asks once each
    struct OccKey {  // what the answer depends on (no padding: same_key compares the bytes)
        size_t lds_bytes = 0, stack_pt = 0;
        size_t line_bytes = 0;  // the environment line asked for; env_line: the same configuration holds it
        int mode = -1;
        uint32_t tris = 0, force_threads = 0, waves_cap = 0;
    };
    struct OccEntry {
        OccKey key;
        int blocks_per_cu = 0;
        uint32_t threads = 0;
        bool env_line = false;
    } occ_cache[2];
    int max_lds_mode = 2;               // tuning "lds_mode": highest staging mode allowed
    uint32_t force_threads = 0;        // tuning "block_threads"; 0 = pick by occupancy
    uint32_t waves_cap = 0;            // tuning "waves_per_cu"; 0 = default cap
    uint32_t trav_threshold = 0;  // tuning "trav_threshold"; 0 = by scene (trav_threshold_for)
    uint32_t drain_threshold = kDefaultDrainThreshold;  // tuning "drain_threshold"
    uint32_t drain_min_steps = kDefaultDrainMinSteps;   // tuning "drain_min_steps"
    uint32_t leaf_batch = 0;  // tuning "leaf_batch", in eighths; 0 = by scene (leaf_batch_for)
    // cost-ordered tile schedule (rt_set_tile_schedule), double-buffered by
    // launch parity: launch L records costs[L&1], reads order[L&1], and its
    // first idle workgroup sorts costs[~L&1] (launch L-1's) into order[~L&1]
    uint32_t tile_schedule = kDefaultTileSchedule;  // rt_set_tile_schedule / tuning "tile_schedule"
    // per stream (launches on the auxiliary stream keep their own history):
    uint32_t* d_tile_sched[2] = {};    // costs[2][n], orders[2][n], flags[2] (n = owned tiles)
    uint64_t sched_launches[2] = {};   // launches since the schedule was (re)set
    // the last launch (rt_launch_config): workgroups, dynamic LDS, workgroup size, and the
    // placement mode of the last path kernel launch (-1: none yet)
    uint32_t last_blocks = 0, last_lds = 0, last_threads = 0;
    int last_mode = -1;
    uint32_t last_passes = 0;  // RT_PASS_* of the last dispatch
    float4* d_slot_sph = nullptr;        // kernel-ordered spheres (sphere_bvh.h)
    uint32_t* d_slot_orig = nullptr;
    uint32_t* d_sph_mat = nullptr;       // by original index
    SphereBvhNode* d_bvh = nullptr;
    std::vector<rt_scene_sphere> h_sph;  // host copy: the BVH is rebuilt from it
    bool slots_dirty = true;
    uint32_t slots_count = 0xffffffffu;  // sphere_count the slots were built for
    bool use_bvh = true;                 // tuning "sphere_bvh" 0: the brute-force sweep only
    bool sphere_octants = true;          // tuning "sphere_octants" 0: one BVH layout
    bool sphere_box_order = true;        // tuning "sphere_box_order" 0: octant layouts keep bmin/bmax
    bool sphere_boxes_ordered = false;   // the uploaded layouts store (near, far) corners
    bool slots_sphere_only = false;      // the uploaded slots were laid out for the sphere-only kernels
    uint32_t sphere_leaf_max = 0;        // tuning "sphere_leaf"; 0 = default
    uint32_t n_always = 0, n_nodes = 0, n_slots = 0;
    float sphere_extent = 0.0f;
    float sphere_rmin = 0.0f, sphere_rmax = 0.0f;
    // triangle accelerator over (object, sub-object) pairs (sphere_bvh.h)
    SphereBvhNode* d_tri_bvh = nullptr;
    SubObjectPrim* d_tri_prims = nullptr;
    size_t tri_bvh_cap = 0, tri_prims_cap = 0;
    bool tri_dirty = true;
    uint32_t tri_count_built = 0xffffffffu;
    bool use_tri_bvh = true;  // tuning "tri_bvh" 0: the reference's sweep
    // Direction-ordered layouts of the binary accelerator for walks from global memory (LDS
    // modes 0/1; order_bvh_by_octant): per position of the 8 layouts the base node and the
    // layout's skip link (host-built with the tree), and the 32-B copy derived from the base
    // nodes on the device after every upload or refit (with the quantized copy).
    // tuning "tri_octants" 0: one layout.
    bool use_tri_octants = true;
    uint32_t* d_tri_src8 = nullptr;
    uint32_t* d_tri_skip8 = nullptr;
    SphereBvhNode* d_tri_bvh8 = nullptr;
    size_t tri_src8_cap = 0, tri_skip8_cap = 0, tri_bvh8_cap = 0;
    bool tri_octants_built = false;  // d_tri_src8 / d_tri_skip8 describe the current tree
    // rt_set_triangle_pruning: distance pruning of the triangle walk: 1 =
    // certified by the leaf certificates (default, exact), 0 = box culling only, 2 = the round-3
    // relative slack (not exact: only this explicit call selects it)
    int tri_prune_mode = 1;
    // certified pruning (tri_cone.h): one certificate per leaf record, rebuilt on the device
    // after any change of the accelerator or the triangles
    TriLeafCert* d_tri_lcert = nullptr;
    size_t tri_lcert_cap = 0;
    bool cones_dirty = true;
    // cooperative leaf batches of the walks from global memory (pathtrace.hip coop_leaf_batch):
    // the leaves' triangle blocks, rebuilt with the certificates; tuning "coop_leaves" 0:
    // per-lane leaf tests
    bool use_coop_leaves = true;
    uint4* d_tri_ltris = nullptr;
    size_t tri_ltris_cap = 0;
    bool ltris_dirty = true;
    // rt_set_brute_force: the reference's own sweeps (BASELINE config 5): 0 off, 1 LDS-tiled, 2
    // through the scalar cache (rt_brute_wf_kernel<tris, stream>)
    int brute = 0;
    // coherent primary rays (rt_primary_kernel): tuning "primary_pass" 1 / 0 force on / off, -1 by scene
    int primary_pass = -1;
    // Workgroup size of the pre-pass where the accelerator is walked from global memory (modes
    // 0/1): its packet walks are chains of dependent node loads, so resident waves are what
    // count; at 1024 threads and ~69 VGPRs only one workgroup (16 waves) fits a CU, at 256 seven
    // (28 waves): C5 5.69 -> 5.24 ms per frame (profiles/r03_ai/ab_c5_pthreads.jsonl); held to
    // 64 VGPRs, eight waves per SIMD (32 per CU): 5.04 ms (profiles/r03_aj/ab_c5_pthreads.jsonl).
    // tunings "primary_threads" 64 / 128 / 256 / 512 / 1024 and "primary_waves" 0 / 8.
    uint32_t primary_threads = 256;
    uint32_t primary_min_waves = 8;
    // a tile's frames on consecutive pre-pass waves, whose packets walk nearly the same nodes:
    // C5 5.02 -> 4.93 ms (profiles/r03_al/ab_c5_ptm.jsonl); tuning "primary_tile_major" 0: frame-major
    bool primary_tile_major = true;
    uint4* d_primary[2] = {};   // per batch parity (overlapped batches), owned px x frames x samples records
    size_t primary_cap = 0;     // bytes, each
    // sub-object bytes of the brute-force launches: [0] SURVEY §8d's tile-streaming convention,
    // [1] what the sweeps read from L2
    unsigned long long* d_stream = nullptr;
    // the brute-force wavefront (rt_brute_wf_kernel)
    float4* d_brute_paths = nullptr;
    uint32_t* d_brute_queue = nullptr;
    uint32_t* d_brute_counts = nullptr;
    size_t brute_paths_cap = 0, brute_queue_cap = 0, brute_counts_cap = 0;
    uint32_t tri_nodes = 0, tri_prim_count = 0;
    float* d_tri_extent = nullptr;   // margin extent, in device memory (refit updates it)
    uint32_t* d_tri_order = nullptr; // node indices by depth, deepest level first (refit)
    uint32_t* d_tri_level_off = nullptr;
    size_t tri_order_cap = 0, tri_level_cap = 0;
    uint32_t tri_levels = 0;
    // device-side edit path (scene_edit.hip): normalised points per triangle,
    // triangle/sub-object -> object maps, per-object triangle ranges, placements
    float* d_model = nullptr;
    uint32_t model_tris = 0;
    bool models_valid = false;  // rt_set_object_models since the last object / sub-object range change
    uint32_t* d_tri_object = nullptr;
    uint32_t* d_sub_object = nullptr;
    uint2* d_object_tris = nullptr;
    rt_scene::Placement* d_place = nullptr;
    float4* d_tri_bounds = nullptr;   // per-triangle min/max (SceneTriangle's host-only fields)
    bool geom_on_device = false;      // device edits are newer than h_obj / h_sub
    RtMaterial* d_mat = nullptr;
    RtObject* d_obj = nullptr;
    RtSubObject* d_sub = nullptr;
    RtTriangleHot* d_tri = nullptr;
    uint32_t* d_tex = nullptr;
    uint32_t tex_w = 0, tex_h = 0, tex_layers = 0;
    uint32_t* d_env = nullptr;
    uint32_t env_w = 0, env_h = 0;
    uint32_t env_uniform = 3;  // bit 0: every row one colour, bit 1: every column (sample_env skips u / v)
    float* d_srgb = nullptr;

    // host-side copies used for validation of index ranges
    std::vector<rt_object_info> h_obj;
    std::vector<rt_sub_object_info> h_sub;

    // pinned staging (one buffer, reused after its last copy completes)
    void* pinned = nullptr;
    size_t pinned_cap = 0;
    hipEvent_t staging_done = nullptr;
    bool staging_busy = false;

    // timing
    bool timing = false;
    bool gen_rays = false;  // rt_update_camera_matrices: primary rays computed on the device
    float inv_proj[16] = {}, inv_view[16] = {};
    // launch timing (rt_set_timing): each timed launch's kernel span on the device
    // clock -- the first workgroup's start to the last one's end (s_memrealtime) --
    // in a ring of slots read back in bulk; HIP events would time each launch from
    // the moment its stream reached it, which overlapped batches make meaningless
    unsigned long long* d_clock = nullptr;  // kClockSlots x {path: ~min start, max end; resolve: the same}
    std::vector<uint32_t> clock_pending;    // slots of timed launches not yet read back
    uint32_t clock_next = 0;
    double wall_khz = 100000.0;             // device wall clock rate (hipDeviceAttributeWallClockRate)
    double total_ms = 0.0;
    uint64_t n_timed = 0;
    double resolve_total_ms = 0.0;  // rt_resolve_frames_kernel spans of the timed batches
    uint64_t n_resolve_timed = 0;
    float last_ms = 0.0f;

    // ray queries (rt_trace_rays, rt_trace_rays_device, rt_pick; query.hip)
    uint32_t query_chunk = kDefaultQueryChunk;  // tuning "query_chunk": rays per staged chunk of rt_trace_rays
    int query_lds_mode = -1;                    // tuning "query_lds_mode": -1 by batch size, else the highest placement
    unsigned long long* d_query_next = nullptr; // the kernel's chunk counter
    void* d_query_buf = nullptr;                // rt_trace_rays / rt_pick scratch: rays, then records
    size_t query_buf_rays = 0, query_buf_bytes = 0;
    void* query_pinned = nullptr;               // the same on the host, pinned
    size_t query_pinned_rays = 0;
    unsigned long long* d_radiance_segs = nullptr;  // rt_radiance: the batch's counted segments
    uint32_t gather_chunk = kDefaultGatherChunk;    // tuning "gather_chunk": points per gather launch
    void* d_gather_partials = nullptr;              // rt_gather: 64 float4 per point of a launch
    size_t gather_partials_bytes = 0;
    uint32_t probe_chunk = kDefaultProbeChunk;      // tuning "probe_chunk": paths per probe launch
    void* d_probe_lights = nullptr;                 // rt_probe_sh: one float4 per path of a launch
    size_t probe_lights_bytes = 0;
    unsigned long long* d_probe_next = nullptr;     // the chunk counters of the two launches in flight
    uint4* d_lens_cam = nullptr;                    // rt_lens: the descriptor the launches of a call read
    // proximity queries (rt_nearest; nearest.hip)
    int nearest_walk = 1;                           // tuning "nearest_walk" 0: the sweep instance, 2: the walk without its descent
    float* d_near_radius = nullptr;                 // |radius| as uploaded, by original sphere index
    size_t near_radius_bytes = 0;
    bool near_radius_dirty = true;                  // the sphere slots were rebuilt since the table was written
    // whether every non-empty sub-object box encloses its triangles within the margin of the walk's
    // bound (rt_nearest_math.h): established by one host pass, until the next triangle, sub-object
    // or object-range upload
    int near_boxes = 0;                             // kNearBoxes*
    struct QueryOccKey {                        // the last query instance (kind: which kernel's, QueryKind)
        int mode = -1, kind = 0;
        uint32_t tris = 0, lds_bytes = 0;
    } q_occ_key;
    int q_occ_blocks = 0;                       // its resident workgroups per CU

    // first-hit feature buffers and the denoiser (rt_compute_features, rt_denoise; denoise.hip).
    // scene_epoch counts the calls that can change what a camera ray hits or what it looks up
    // there (camera, geometry, materials, textures, Params); the planes are rebuilt when the
    // epoch they were built at is stale. Everything is allocated on first use.
    uint64_t scene_epoch = 1;
    uint64_t feat_epoch = 0;                      // 0: never built
    float4* d_feat[2] = {};                       // plane A: normal.xyz, t; plane B: albedo.rgb, hit
    uint2* d_feat_ids = nullptr;                  // the ID plane: rt_hit.kind, rt_hit.index
    void* d_feat_scratch = nullptr;               // one band's rays, then its records
    size_t feat_scratch_bytes = 0;
    uint32_t feature_band = kDefaultFeatureBand;  // tuning "feature_band": pixels per band
    float4* d_dn[2] = {};                         // the filter's ping-pong colour planes
    uint32_t* d_dn_out = nullptr;                 // the packed denoised output
    int dn_result = -1;                           // which of d_dn holds the last rt_denoise's result; -1: none yet
    bool denoise_lds = true;                      // tuning "denoise_lds" 0: the passes with step 1, 2 load directly
    // temporal reprojection (rt_denoise_temporal): two history slots of three float4 planes (C: rgba;
    // X: xyz, hit; Nn: normal.xyz, n), each with the world_to_pixel matrix it was written with and
    // the accumulation generation it was written in. accum_gen counts rt_reset_accumulation calls.
    struct TemporalSlot {
        float4* plane[3] = {};
        float matrix[16] = {};
        uint64_t gen = 0;
        bool valid = false;
        uint2* ids = nullptr;   // the I plane, allocated at the first rt_denoise_temporal_motion
        bool has_ids = false;   // the call that wrote this slot wrote ids too
    } t_slot[2];
    void* d_motion = nullptr;   // rt_denoise_temporal_motion: the object records, then the sphere records
    size_t motion_bytes = 0;
    int t_cur = 0;            // the slot the last rt_denoise_temporal wrote (when valid)
    int t_prev = -1;          // the slot it read; -1: none
    uint64_t accum_gen = 0;   // G
    // the display transform (rt_display; display.hip), allocated on first use
    uint32_t* d_disp_out = nullptr;    // the packed display plane
    uint32_t* d_disp_meter = nullptr;  // kDispBins live bins, kDispBins kept bins, kDispStateWords of state
    bool disp_valid = false;           // an rt_display has written d_disp_out
    bool disp_exposure_valid = false;  // the state's exposure word holds an adapted exposure

    std::string err;
};

namespace rth {

// Orders the primary stream after everything issued on the auxiliary stream
// (overlapped batches): every call other than rt_compute_frame runs this first.
hipError_t join_aux(rt_ctx* ctx);

// Launches the queued frames (rt_frames.cpp).
int flush_frames(rt_ctx* ctx);

int fail(rt_ctx* ctx, int code, const std::string& msg);
int hip_fail(rt_ctx* ctx, const char* what, hipError_t e);

#define RT_HIP(ctx, call)                                \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return hip_fail(ctx, #call, e_); \
    } while (0)

// A device buffer of at least `bytes` -- or `n` of them under one capacity: the pairs by batch
// parity -- reallocated when smaller, after both streams have drained: nothing may still read
// it. The capacity stays 0 until every allocation has succeeded. `what` names the buffer in the
// out-of-memory message; *stale is set when it was reallocated (what the caller derived into it
// is gone).
template <typename T>
int grow_buffer(rt_ctx* ctx, const char* what, T** p, size_t* cap, size_t bytes, bool* stale = nullptr, size_t n = 1) {
    if (p[0] && *cap >= bytes) return RT_OK;
    RT_HIP(ctx, join_aux(ctx));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) {
        if (p[i]) RT_HIP(ctx, hipFree(p[i]));
        p[i] = nullptr;
    }
    *cap = 0;
    const size_t alloc = bytes < 256 ? 256 : bytes;
    for (size_t i = 0; i < n; i++) {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p[i]), alloc);
        if (e != hipSuccess) return fail(ctx, RT_E_NOMEM, std::string(what) + ": " + hipGetErrorString(e));
    }
    *cap = alloc;
    if (stale) *stale = true;
    return RT_OK;
}

// Cache keys are plain structs without padding, compared as a whole.
template <typename K>
bool same_key(const K& a, const K& b) {
    static_assert(std::has_unique_object_representations_v<K>, "the key's bytes must be its value");
    return std::memcmp(&a, &b, sizeof(K)) == 0;
}

// A caller's device pointer, as an entry point requires it.
struct DevicePtr {
    const void* p;
    const char* name;
    uintptr_t alignment;  // in bytes, a power of two
    bool may_be_null;
};

// RT_OK when every pointer is device memory of the context's device at its alignment (or NULL
// where that is allowed); else RT_E_INVALID with a message naming `entry` and the argument.
int check_device_ptrs(rt_ctx* ctx, const char* entry, std::initializer_list<DevicePtr> ptrs);

template <typename T>
int dev_alloc(rt_ctx* ctx, T** p, size_t count) {
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;  // keep every binding a valid pointer
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
    if (e != hipSuccess) return fail(ctx, RT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemsetAsync(*p, 0, bytes, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "hipMemsetAsync", e);
    ctx->primary_dirty = true;
    return RT_OK;
}

// Pinned staging and uploads, accelerator refresh, launch timing slots (rt_abi.cpp).
uint32_t owned_tile_count(uint32_t n_tiles, uint32_t rank, uint32_t world);
int staging(rt_ctx* ctx, size_t bytes, void** out);
int staged_copy(rt_ctx* ctx, void* dst, size_t bytes);
int upload_raw(rt_ctx* ctx, void* dst, const void* src, size_t bytes);
int refresh_sphere_slots(rt_ctx* ctx, uint32_t count, bool sphere_only);
int sync_host_geometry(rt_ctx* ctx);
int refresh_tri_accel(rt_ctx* ctx, uint32_t object_count);
hipError_t follow_primary(rt_ctx* ctx, hipStream_t S);
int claim_clock_slot(rt_ctx* ctx, hipStream_t S, KernelArgs& ka);

// ---- the scene as a launch sees it ------------------------------------------------------------
//
// The scene-view part of the kernel arguments, shared by the frame launches (dispatch_batch) and
// the ray queries (run_query): the scene and camera fields, the LDS carve-up with the placement
// mode it allows (0: everything read from global memory, 1: spheres / materials / objects / sphere
// BVH staged in LDS, 2: also the triangle accelerator), and what the accelerators' walks read in
// that mode (direction-ordered and quantized nodes, leaf certificates, leaf triangle blocks),
// derived on the device when stale.
struct SceneLaunch {
    bool tris = false;      // the scene has objects: else the sphere-only kernels
    int mode = 0;           // LDS placement mode
    uint32_t layouts = 1;   // sphere BVH layouts staged (1 or 8)
    size_t mode1_bytes = 0, mode2_bytes = 0;  // the LDS images of modes 1 and 2, tail included
    size_t lds_bytes = 0;   // the image of `mode`
    bool coop = false;      // cooperative leaf batches: per-wave LDS scratch after the image
};

inline size_t al16(size_t x) { return (x + 15) & ~size_t(15); }
void scene_base_args(rt_ctx* ctx, KernelArgs& ka);
void scene_carve(rt_ctx* ctx, KernelArgs& ka, int max_mode, SceneLaunch& sl);
int scene_accel_args(rt_ctx* ctx, KernelArgs& ka, SceneLaunch& sl);
int copy_plane_to_device(rt_ctx* ctx, const char* entry, const uint32_t* src, const char* missing,
                         void* dst_device, uint32_t bytes_per_row);

// Ray queries (rt_queries.cpp), which the feature buffers run too.
int query_enter(rt_ctx* ctx);
int run_query(rt_ctx* ctx, const void* rays, void* hits, uint64_t count, bool any_hit = false);

}  // namespace rth

#define RT_ENTER_NOFLUSH(ctx)                                       \
    do {                                                            \
        if (!(ctx)) return RT_E_INVALID;                            \
        (ctx)->err.clear();                                         \
        hipError_t e0_ = hipSetDevice((ctx)->device);               \
        if (e0_ != hipSuccess) return hip_fail(ctx, "hipSetDevice", e0_); \
    } while (0)

// Every entry point but rt_compute_frame: launch the queued frames, order the
// primary stream after the auxiliary one, and note that primary-stream work may
// follow (a later overlapped batch then waits for it).
#define RT_ENTER(ctx)                                                   \
    do {                                                                \
        RT_ENTER_NOFLUSH(ctx);                                          \
        const int rcf_ = flush_frames(ctx);                             \
        if (rcf_ != RT_OK) return rcf_;                                 \
        const hipError_t ej_ = join_aux(ctx);                           \
        if (ej_ != hipSuccess) return hip_fail(ctx, "join_aux", ej_);   \
        (ctx)->primary_dirty = true;                                    \
    } while (0)
