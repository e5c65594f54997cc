// rt_abi.cpp — host implementation of include/rt_abi.h.
//
// Replaces the wgpu side of the reference's per-frame path:
//   DataBuffers (src/buffers.rs:140-596)  -> hipMalloc'd device buffers, updated
//                                            through a pinned staging buffer with
//                                            hipMemcpyAsync on the context stream
//   Renderer::compute_frame (src/renderer.rs:201-252)
//                                         -> Params shadow + hipLaunchKernelGGL
// Stream order gives the same visibility guarantees as wgpu's queue order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rt_abi.h"
#include "rt_kernel_args.h"
#include "rt_launch.h"
#include "rt_query_schedule.h"
#include "rt_scene_math.h"
#include "sphere_bvh.h"
#include "tri_cone.h"
#include "tri_qnode.h"

static_assert(sizeof(rt_params) == 48, "Params is 48 bytes (src/buffers.rs:9-22)");
static_assert(sizeof(rt_ray_camera) == 16, "RayCamera is 16 bytes");
static_assert(sizeof(rt_ray) == 16, "Ray is 16 bytes");
static_assert(sizeof(rt_scene_sphere) == 32, "SceneSphere is 32 bytes");
static_assert(sizeof(rt_scene_triangle) == 112, "SceneTriangle is 112 bytes");
static_assert(sizeof(rt_scene_material) == 32, "SceneMaterial is 32 bytes");
static_assert(sizeof(rt_object_info) == 48, "ObjectInfo is 48 bytes");
static_assert(sizeof(rt_sub_object_info) == 32, "SubObjectInfo is 32 bytes");
static_assert(sizeof(rt_query_ray) == 32, "rt_query_ray is two 16-B loads");
static_assert(sizeof(rt_hit) == 64, "rt_hit is four 16-B stores");
static_assert(sizeof(rt_denoise_params) == 16, "rt_denoise_params is 16 bytes");
static_assert(sizeof(rt_temporal_params) == 80, "rt_temporal_params is 80 bytes");
static_assert(sizeof(rt_motion) == 64 && offsetof(rt_motion, normal_scale) == 48, "rt_motion is four 16-B rows");
static_assert(sizeof(rt_display_params) == 48, "rt_display_params is 48 bytes");
static_assert(sizeof(rt_occlusion_ray) == sizeof(rt_query_ray), "rt_occlusion_ray is an rt_query_ray with t_max for _pad1");
static_assert(sizeof(rt_radiance_ray) == sizeof(rt_query_ray), "rt_radiance_ray is an rt_query_ray with the stream for _pad0");
static_assert(offsetof(rt_radiance_ray, stream) == 12 && offsetof(rt_radiance_ray, direction) == 16,
              "rt_radiance_ray: {origin, stream}, {direction, pad} as two 16-B loads");
static_assert(sizeof(rt_gather_point) == sizeof(rt_radiance_ray), "rt_gather_point has the layout of rt_radiance_ray");
static_assert(offsetof(rt_gather_point, stream) == 12 && offsetof(rt_gather_point, normal) == 16,
              "rt_gather_point: {position, stream}, {normal, pad} as two 16-B loads");
static_assert(sizeof(rt_ambient_point) == sizeof(rt_gather_point), "rt_ambient_point is an rt_gather_point with t_max for _pad1");
static_assert(offsetof(rt_ambient_point, stream) == 12 && offsetof(rt_ambient_point, normal) == 16 &&
                  offsetof(rt_ambient_point, t_max) == 28,
              "rt_ambient_point: {position, stream}, {normal, t_max} as two 16-B loads");
static_assert(sizeof(rt_probe) == 16 && offsetof(rt_probe, stream) == 12, "rt_probe: {position, stream} as one 16-B load");
static_assert(sizeof(rt_scene_material) == sizeof(RtMaterial), "material record");
static_assert(sizeof(rt_object_info) == sizeof(RtObject), "object record");
static_assert(sizeof(rt_sub_object_info) == sizeof(RtSubObject), "sub-object record");

namespace {

constexpr size_t kLdsSceneBudget = 64 * 1024;    // mode 1: spheres/materials/objects/sphere BVH per workgroup
constexpr size_t kLdsAccelBudget = 150 * 1024;   // mode 2: + triangle accelerator (one 1024-thread workgroup per CU)
// d_counter: [0] the ray counter, [1, 1 + kDiagCounters) the diagnostic
// counters of RT_DIAG / RT_DIAG_TAIL builds (KernelArgs::diag), then the
// per-wave (queue dry, end) records of RT_DIAG_TAIL builds: room for 65,536 waves.
constexpr size_t kDiagCounters = kDiagHeaderWords;
constexpr size_t kDiagWaveRecords = 2 * 65536;
constexpr size_t kCounterWords = 1 + kDiagCounters + kDiagWaveRecords;
// Tile queue: counters per stripe (pathtrace.hip, claim_tile), 256 B apart;
// kQueueStripes = 4 per XCD by default (measured: C2 0.599 ms at 8, 0.595 at 32; C1
// 0.076 -> 0.058 ms), up to kQueueStripesMax (rt_kernel_args.h, with kQueueStride).
constexpr uint32_t kQueueStripes = 32;
// Triangle-walk distance pruning: a node is skipped once its (inflated) box
// is entered beyond best * (1 + kTriPruneRho) + kTriPruneAbs * (|o| + extent) / |d|.
constexpr float kTriPruneRho = 1.0f / 64.0f;
// A wave goes back to shading once at most this many of its 64 lanes are still
// traversing (pathtrace.hip, step 4 of the kernel loop). The longer a trace is
// against a shading pass, the earlier it pays to shade the finished lanes
// (measured: sphere scenes 8, C2 slower at 12+ until round 6's block group tests, since then 12:
// C2 0.2474 -> 0.2448 ms, 10 / 14 / 20: 0.2456 / 0.2444 / 0.2468, profiles/r06/r06v, r06w;
// triangle accelerator in LDS
// 24, C3/C4 -2%; in global memory 32, C5 -10%; with the pruned octant walk of round 3,
// 48: C5 5.95 -> 5.72 ms, profiles/r03_ah/knobs_c5b.jsonl; C3 unchanged at 24-32).
// certified: walks from global memory with the certified pruning, whose
// traces visit the box-culling node set (about twice the relative slack's): they return to
// shading later and batch their leaves earlier (C5 13.0 -> 11.1 ms per frame at 56 / 3, 10.7 at 56 / 4
// once the certificate test moved into the leaf batch;
// profiles/r04/r04_f/ab.jsonl; the slack keeps round 3's 48 / 5).
uint32_t trav_threshold_for(int lds_mode, bool tris, bool certified) {
    if (!tris) return 12;
    return lds_mode == 2 ? 24 : certified ? 56 : 48;
}
// Triangle scenes test deferred leaves once this many eighths of the
// traversing lanes hold one (pathtrace.hip, leaf_step): later for an LDS
// accelerator, earlier when the leaf's loads go to global memory anyway.
// Re-measured with 20-frame launches (profiles/archive/r02_s4/r02_s4k, r02_s4l):
// mode 2 at 6 (C4 -2.3% against 7, C3 within 0.3%), modes 0/1 at 5 (C5 -2.9%
// against 6; 4 and 3 within 0.4% of 5); certified walks at 4 (above; 3 before the certificate
// test moved into the leaf batch, profiles/r04/r04_k).
uint32_t leaf_batch_for(int lds_mode, bool certified) { return lds_mode == 2 ? 6 : certified ? 4 : 5; }
// Instances with the triangle accelerator in global memory: the same once the
// tile queue is empty, when the wave goes back to shading only if some lane
// has finished and after at least kDefaultDrainMinSteps traversal steps
// (threshold 0: traverse to the end, as the other instances do).
constexpr uint32_t kDefaultDrainThreshold = 32;
constexpr uint32_t kDefaultDrainMinSteps = 64;
// Tile claim order: 0 = tile index order, 1 = cost-ordered (most rays first,
// sorted on the device from the previous frame's per-tile ray counts).
constexpr uint32_t kDefaultTileSchedule = 1;
constexpr uint64_t kSchedMinTilesPerWave = 4;
// Frame batching (rt_set_frame_batch): at most this many frames per launch.
constexpr uint32_t kMaxFrameBatch = 64;
// Frame-parallel batches (every (frame, tile) its own queue unit, lights resolved
// in order afterwards) up to this many frames x samples; larger batches run each
// pixel's frames back to back on one lane.
constexpr uint32_t kMaxParallelLights = 64;
// Ray queries (query.hip). rt_trace_rays stages its rays and records through pinned memory in
// chunks of this many rays (96 B each: 6 MiB pinned, 6 MiB of device scratch); tuning "query_chunk".
constexpr uint32_t kDefaultQueryChunk = 65536;
constexpr uint32_t kMaxQueryChunk = 1u << 24;
// A query of fewer rays than this launches the mode-0 instance (the scene read from global
// memory) instead of staging the LDS image in every workgroup: measured crossover, DESIGN.md §5.4b.
constexpr uint64_t kQueryStageMinRays = 262144;
// Gather queries (radiance.hip) run in launches of at most this many points, 1 KB of partials
// each (16 MiB of context-owned scratch); tuning "gather_chunk".
constexpr uint32_t kDefaultGatherChunk = 16384;
constexpr uint32_t kMaxGatherChunk = 1u << 20;
// Probe queries (radiance.hip) run in launches of at most this many paths, 16 B of scratch each
// (16 MiB of context-owned scratch), but of one whole probe at least; tuning "probe_chunk".
constexpr uint32_t kDefaultProbeChunk = 1048576;
constexpr uint32_t kMaxProbeChunk = 1u << 26;
// The most samples a probe takes: one probe's scratch is then 256 MiB.
constexpr uint32_t kMaxProbeSamples = 1u << 24;
constexpr size_t kMaxProbeScratchBytes = (size_t)kMaxProbeSamples * 16u;
// Feature buffers (denoise.hip): the frame's camera rays are traced in bands of this many pixels,
// so the scratch of a band -- its rays and records, 96 B per pixel: 48 MiB -- does not grow with
// the frame (3840x2160 would take 800 MB at once); tuning "feature_band".
constexpr uint32_t kDefaultFeatureBand = 1u << 19;
constexpr uint32_t kMaxFeatureBand = 1u << 24;
constexpr uint32_t kMaxDenoiseIterations = 8;
// The display transform's metering buffer (display.hip): live bins | kept bins | {E, -, metered lo, hi}.
constexpr uint32_t kDispBins = 256;
constexpr uint32_t kDispStateWords = 4;

}  // namespace

// The last error of a call without a context (rt_create, the scene builders).
thread_local std::string g_create_error;
void rt_set_global_error(const std::string& msg) { g_create_error = msg; }

namespace {

constexpr uint32_t kClockSlots = 4096;
constexpr uint32_t kClockWords = 4;  // per timed launch: path kernel {~start, end}, resolve kernel {~start, end}

}  // namespace

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

static int flush_frames(rt_ctx* ctx);

// Orders the primary stream after everything issued on the auxiliary stream
// (overlapped batches): every call other than rt_compute_frame runs this first.
static hipError_t join_aux(rt_ctx* ctx) {
    if (!ctx->aux_outstanding) return hipSuccess;
    ctx->aux_outstanding = false;
    return hipStreamWaitEvent(ctx->stream, ctx->ev_aux_done, 0);
}

namespace {

int fail(rt_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

int hip_fail(rt_ctx* ctx, const char* what, hipError_t e) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return fail(ctx, RT_E_HIP, m);
}

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
int check_device_ptrs(rt_ctx* ctx, const char* entry, std::initializer_list<DevicePtr> ptrs) {
    auto bad = [&](const DevicePtr& a, const std::string& why) {
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": " + a.name + " " + why);
    };
    for (const DevicePtr& a : ptrs) {
        if (!a.p) {
            if (a.may_be_null) continue;
            return bad(a, "is NULL");
        }
        hipPointerAttribute_t attr{};
        const hipError_t ea = hipPointerGetAttributes(&attr, a.p);
        if (ea != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
            (void)hipGetLastError();
            return bad(a, "must be device memory of the context's device");
        }
        if ((uintptr_t)a.p & (a.alignment - 1u))
            return bad(a, "must be " + std::to_string(a.alignment) + "-byte aligned");
    }
    return RT_OK;
}

void srgb_table(float out[256]) {
    // IEC 61966-2-1 decode of an 8-bit Rgba8UnormSrgb channel, rounded to f32.
    for (int i = 0; i < 256; i++) {
        const double c = (double)i / 255.0;
        const double l = c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        out[i] = (float)l;
    }
}

uint32_t owned_tile_count(uint32_t n_tiles, uint32_t rank, uint32_t world) {
    if (rank >= n_tiles) return 0;
    return (n_tiles - rank + world - 1) / world;
}

// Returns a pinned host region of at least `bytes`, waiting for any copy
// still reading the previous contents.
int staging(rt_ctx* ctx, size_t bytes, void** out) {
    if (ctx->staging_busy) {
        RT_HIP(ctx, hipEventSynchronize(ctx->staging_done));
        ctx->staging_busy = false;
    }
    if (bytes > ctx->pinned_cap) {
        if (ctx->pinned) RT_HIP(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_cap = 0;
        size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;
        RT_HIP(ctx, hipHostMalloc(&ctx->pinned, cap, hipHostMallocDefault));
        ctx->pinned_cap = cap;
    }
    *out = ctx->pinned;
    return RT_OK;
}

int staged_copy(rt_ctx* ctx, void* dst, size_t bytes) {
    if (bytes == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(dst, ctx->pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipEventRecord(ctx->staging_done, ctx->stream));
    ctx->primary_dirty = true;  // an overlapped batch issued later must follow this copy
    ctx->staging_busy = true;
    return RT_OK;
}

int upload_raw(rt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return RT_OK;
    void* p;
    int rc = staging(ctx, bytes, &p);
    if (rc) return rc;
    std::memcpy(p, src, bytes);
    return staged_copy(ctx, dst, bytes);
}

int upload_spheres(rt_ctx* ctx, const rt_scene_sphere* s, uint32_t n) {
    if (n == 0) return RT_OK;
    std::copy(s, s + n, ctx->h_sph.begin());
    ctx->slots_dirty = true;  // slots + BVH are rebuilt at the next dispatch
    return RT_OK;
}

// Rebuild the kernel's sphere slots (brute-force set + BVH) for the first
// `count` spheres and upload them, stream-ordered before the next launch.
int refresh_sphere_slots(rt_ctx* ctx, uint32_t count, bool sphere_only) {
    if (!ctx->slots_dirty && ctx->slots_count == count && ctx->slots_sphere_only == sphere_only) return RT_OK;
    SphereSlots sl;
    build_sphere_slots(ctx->h_sph.data(), count, ctx->use_bvh, &sl, ctx->sphere_leaf_max);
    std::vector<uint32_t> mat(count);
    for (uint32_t i = 0; i < count; i++) mat[i] = ctx->h_sph[i].material_index;
    std::vector<SphereBvhNode> oct;  // 8 direction-ordered copies; layout 0 alone is a complete walk too
    // boxes stored as (near, far) corners per octant when that is exact (rt_bvh_slab.h);
    // only the sphere-only kernels read them that way, so only for scenes without objects
    const bool box_order = ctx->sphere_box_order && sphere_only && box_layout_orderable(sl.nodes);
    order_bvh_by_octant(sl.nodes, &oct, box_order);
    int rc;
    if ((rc = upload_raw(ctx, ctx->d_slot_sph, sl.slot_sph.data(), sl.slot_sph.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_slot_orig, sl.slot_orig.data(), sl.slot_orig.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_sph_mat, mat.data(), mat.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_bvh, oct.data(), oct.size() * sizeof(SphereBvhNode))))
        return rc;
    ctx->n_always = sl.n_always;
    ctx->n_slots = (uint32_t)sl.slot_orig.size();
    ctx->n_nodes = (uint32_t)sl.nodes.size();
    ctx->sphere_boxes_ordered = box_order;
    ctx->sphere_extent = sl.extent;
    ctx->sphere_rmin = sl.r_min;
    ctx->sphere_rmax = sl.r_max;
    ctx->slots_dirty = false;
    ctx->slots_count = count;
    ctx->slots_sphere_only = sphere_only;
    return RT_OK;
}

// After device-side edits (rt_update_objects) the host copies of the object and
// sub-object records are stale; read them back before anything host-side uses
// their bounds.
int sync_host_geometry(rt_ctx* ctx) {
    if (!ctx->geom_on_device) return RT_OK;
    if (!ctx->h_obj.empty())
        RT_HIP(ctx, hipMemcpyAsync(ctx->h_obj.data(), ctx->d_obj, ctx->h_obj.size() * 48, hipMemcpyDeviceToHost,
                                   ctx->stream));
    if (!ctx->h_sub.empty())
        RT_HIP(ctx, hipMemcpyAsync(ctx->h_sub.data(), ctx->d_sub, ctx->h_sub.size() * 32, hipMemcpyDeviceToHost,
                                   ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->geom_on_device = false;
    return RT_OK;
}

// Rebuild the triangle accelerator for the first `object_count` objects when
// objects or sub-objects changed (the boxes it culls with are theirs).
int refresh_tri_accel(rt_ctx* ctx, uint32_t object_count) {
    if (!ctx->use_tri_bvh || object_count == 0) return RT_OK;
    if (!ctx->tri_dirty && ctx->tri_count_built == object_count) return RT_OK;
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    int rc;
    TriangleAccel acc;
    build_triangle_accel(ctx->h_obj.data(), object_count, ctx->h_sub.data(), (uint32_t)ctx->h_sub.size(), &acc);
    const size_t nb = acc.nodes.size() * sizeof(SphereBvhNode), pb = acc.prims.size() * sizeof(SubObjectPrim);
    if ((rc = grow_buffer(ctx, "triangle accelerator nodes", &ctx->d_tri_bvh, &ctx->tri_bvh_cap, nb)) ||
        (rc = grow_buffer(ctx, "triangle accelerator leaves", &ctx->d_tri_prims, &ctx->tri_prims_cap, pb)) ||
        (rc = upload_raw(ctx, ctx->d_tri_bvh, acc.nodes.data(), nb)) ||
        (rc = upload_raw(ctx, ctx->d_tri_prims, acc.prims.data(), pb)))
        return rc;
    ctx->qnodes_dirty = true;
    ctx->cones_dirty = true;
    ctx->ltris_dirty = true;
    ctx->tri_nodes = (uint32_t)acc.nodes.size();
    ctx->tri_prim_count = (uint32_t)acc.prims.size();
    ctx->tri_octants_built = false;
    if (ctx->use_tri_octants && acc.nodes.size() > 1 && acc.nodes.size() * 8 < (size_t)kTriWalkEnd) {
        std::vector<SphereBvhNode> oct;
        std::vector<uint32_t> src;
        order_bvh_by_octant(acc.nodes, &oct, false, &src);
        std::vector<uint32_t> skip(oct.size());
        for (size_t i = 0; i < oct.size(); i++) skip[i] = oct[i].skip;
        const size_t b8 = oct.size() * 4;
        if ((rc = grow_buffer(ctx, "octant layout sources", &ctx->d_tri_src8, &ctx->tri_src8_cap, b8)) ||
            (rc = grow_buffer(ctx, "octant layout links", &ctx->d_tri_skip8, &ctx->tri_skip8_cap, b8)) ||
            (rc = grow_buffer(ctx, "octant layout nodes", &ctx->d_tri_bvh8, &ctx->tri_bvh8_cap, oct.size() * sizeof(SphereBvhNode))) ||
            (rc = upload_raw(ctx, ctx->d_tri_src8, src.data(), b8)) ||
            (rc = upload_raw(ctx, ctx->d_tri_skip8, skip.data(), b8)))
            return rc;
        ctx->tri_octants_built = true;
    }
    // depth levels for the device refit (preorder: a node precedes its children)
    std::vector<uint32_t> depth(acc.nodes.size(), 0);
    uint32_t max_depth = 0;
    for (size_t i = 0; i < acc.nodes.size(); i++) {
        max_depth = std::max(max_depth, depth[i]);
        if (acc.nodes[i].leaf == kSphereBvhInternal) {
            depth[i + 1] = depth[i] + 1;
            depth[acc.nodes[i + 1].skip] = depth[i] + 1;
        }
    }
    std::vector<uint32_t> off(max_depth + 2, 0), order(acc.nodes.size());
    for (uint32_t d : depth) off[max_depth - d + 1]++;  // deepest level first
    for (size_t l = 1; l < off.size(); l++) off[l] += off[l - 1];
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (size_t i = 0; i < acc.nodes.size(); i++) order[fill[max_depth - depth[i]]++] = (uint32_t)i;
    if ((rc = grow_buffer(ctx, "refit order", &ctx->d_tri_order, &ctx->tri_order_cap, order.size() * 4)) ||
        (rc = grow_buffer(ctx, "refit levels", &ctx->d_tri_level_off, &ctx->tri_level_cap, off.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_order, order.data(), order.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_level_off, off.data(), off.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_extent, &acc.extent, 4)))
        return rc;
    ctx->tri_levels = max_depth + 1;
    ctx->tri_dirty = false;
    ctx->tri_count_built = object_count;
    return RT_OK;
}

int upload_triangles(rt_ctx* ctx, const rt_scene_triangle* t, uint32_t n) {
    if (n == 0) return RT_OK;
    ctx->cones_dirty = true;
    ctx->ltris_dirty = true;
    void* p;
    int rc = staging(ctx, (size_t)n * sizeof(RtTriangleHot), &p);
    if (rc) return rc;
    RtTriangleHot* hot = static_cast<RtTriangleHot*>(p);
    for (uint32_t i = 0; i < n; i++) {
        const rt_scene_triangle& s = t[i];
        hot[i] = pack_triangle(s.a, s.edge_ab, s.edge_ac, s.calc_normal, s.face_normal);
    }
    if ((rc = staged_copy(ctx, ctx->d_tri, (size_t)n * sizeof(RtTriangleHot))) ||
        (rc = staging(ctx, (size_t)n * 32, &p)))
        return rc;
    float4* b = static_cast<float4*>(p);
    for (uint32_t i = 0; i < n; i++) {
        const rt_scene_triangle& s = t[i];
        b[2 * i] = make_float4(s.min_bounds[0], s.min_bounds[1], s.min_bounds[2], 0.f);
        b[2 * i + 1] = make_float4(s.max_bounds[0], s.max_bounds[1], s.max_bounds[2], 0.f);
    }
    return staged_copy(ctx, ctx->d_tri_bounds, (size_t)n * 32);
}

// Index ranges the kernel walks must lie inside the buffers (the reference's
// fixed-size WGSL arrays would clamp; here they are rejected up front).
int validate_ranges(rt_ctx* ctx) {
    for (size_t i = 0; i < ctx->h_obj.size(); i++) {
        const rt_object_info& o = ctx->h_obj[i];
        if ((uint64_t)o.first_sub_object_index + o.sub_object_count > ctx->cap_sub)
            return fail(ctx, RT_E_INVALID, "object " + std::to_string(i) + " sub-object range exceeds sub_object_count");
    }
    for (size_t i = 0; i < ctx->h_sub.size(); i++) {
        const rt_sub_object_info& s = ctx->h_sub[i];
        if (s.triangle_count != 0 && (uint64_t)s.first_triangle_index + s.triangle_count > ctx->cap_tri)
            return fail(ctx, RT_E_INVALID, "sub-object " + std::to_string(i) + " triangle range exceeds triangle_count");
    }
    return RT_OK;
}

int check_params(rt_ctx* ctx, const rt_params* p) {
    if (!p) return fail(ctx, RT_E_INVALID, "params is NULL");
    if (p->screen_width != ctx->width)
        return fail(ctx, RT_E_INVALID, "params.screen_width must equal the framebuffer width");
    if (p->sphere_count > ctx->cap_sph) return fail(ctx, RT_E_INVALID, "params.sphere_count exceeds sphere buffer");
    if (p->object_count > ctx->cap_obj) return fail(ctx, RT_E_INVALID, "params.object_count exceeds object buffer");
    return RT_OK;
}

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

int collect_timing(rt_ctx* ctx) {
    if (ctx->clock_pending.empty()) return RT_OK;
    RT_HIP(ctx, join_aux(ctx));
    std::vector<unsigned long long> c(kClockWords * (size_t)kClockSlots);
    RT_HIP(ctx, hipMemcpyAsync(c.data(), ctx->d_clock, c.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t slot : ctx->clock_pending) {
        const unsigned long long* w = c.data() + kClockWords * (size_t)slot;
        const unsigned long long t0 = ~w[0], t1 = w[1];
        if (w[0] != 0 && t1 >= t0) {  // else no workgroup ran
            const float ms = (float)((double)(t1 - t0) / ctx->wall_khz);
            ctx->total_ms += ms;
            ctx->n_timed += 1;
            ctx->last_ms = ms;
        }
        const unsigned long long r0 = ~w[2], r1 = w[3];
        if (w[2] != 0 && r1 >= r0) {  // the batch's resolve pass
            ctx->resolve_total_ms += (double)(r1 - r0) / ctx->wall_khz;
            ctx->n_resolve_timed += 1;
        }
    }
    ctx->clock_pending.clear();
    // the slots start the next launches at zero (the kernels atomicMax into them): cleared
    // here, off the launch path, instead of by a memset ahead of every timed launch
    RT_HIP(ctx, hipMemsetAsync(ctx->d_clock, 0, c.size() * 8, ctx->stream));
    ctx->primary_dirty = true;  // an auxiliary-stream batch waits for it
    return RT_OK;
}

// The auxiliary stream follows the primary stream: what S runs next waits for everything issued
// on the primary stream so far (nothing to do when S is the primary stream).
hipError_t follow_primary(rt_ctx* ctx, hipStream_t S) {
    if (S == ctx->stream) return hipSuccess;
    const hipError_t e = hipEventRecord(ctx->ev_primary, ctx->stream);
    return e != hipSuccess ? e : hipStreamWaitEvent(S, ctx->ev_primary, 0);
}

// ka.launch_clock: the timing slot of a launch on stream S, null unless timing is on
// (rt_set_timing, which also allocates the ring ahead of the launches).
int claim_clock_slot(rt_ctx* ctx, hipStream_t S, KernelArgs& ka) {
    ka.launch_clock = nullptr;
    if (!ctx->timing) return RT_OK;
    int rc;
    if (ctx->clock_pending.size() >= kClockSlots && (rc = collect_timing(ctx))) return rc;
    if (!ctx->d_clock) {
        if ((rc = dev_alloc(ctx, &ctx->d_clock, kClockWords * (size_t)kClockSlots))) return rc;
        RT_HIP(ctx, follow_primary(ctx, S));  // the zeroed slots must be in place before an aux launch
    }
    const uint32_t slot = ctx->clock_next;
    ctx->clock_next = (ctx->clock_next + 1) % kClockSlots;
    ka.launch_clock = ctx->d_clock + kClockWords * (size_t)slot;  // zero: dev_alloc / collect_timing
    ctx->clock_pending.push_back(slot);
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

#ifndef RT_BUILD_HASH
#define RT_BUILD_HASH "unknown"
#endif
const char* rt_build_hash(void) { return RT_BUILD_HASH; }

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rt_srgb_table(float out[256]) {
    if (!out) return RT_E_INVALID;
    srgb_table(out);
    return RT_OK;
}

int rt_create(const rt_create_info* info, rt_ctx** out_ctx) {
    g_create_error.clear();
    if (!info || !out_ctx) return fail(nullptr, RT_E_INVALID, "rt_create: NULL argument");
    *out_ctx = nullptr;
    if (info->width == 0 || info->height == 0) return fail(nullptr, RT_E_INVALID, "width and height must be > 0");
    if (info->world_size == 0 || info->rank >= info->world_size)
        return fail(nullptr, RT_E_INVALID, "rank must be < world_size (world_size >= 1)");
    const uint64_t n_pixels = (uint64_t)info->width * info->height;
    if (n_pixels > 0xffffffffull) return fail(nullptr, RT_E_INVALID, "pixel index must fit in u32 (:148)");
    if (!info->camera_rays) return fail(nullptr, RT_E_INVALID, "camera_rays is NULL");
    if ((info->material_count && !info->materials) || (info->sphere_count && !info->spheres) ||
        (info->triangle_count && !info->triangles) || (info->object_count && !info->objects) ||
        (info->sub_object_count && !info->sub_objects))
        return fail(nullptr, RT_E_INVALID, "NULL scene array with a non-zero count");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return fail(nullptr, RT_E_NODEVICE, "no HIP device available");
    if (info->device < 0 || info->device >= n_dev) return fail(nullptr, RT_E_NODEVICE, "device ordinal out of range");

    rt_ctx* ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return fail(nullptr, RT_E_NOMEM, "out of host memory");
    auto bail = [&](int rc) {
        g_create_error = ctx->err;
        rt_destroy(ctx);
        return rc;
    };
    ctx->device = info->device;
    ctx->width = info->width;
    ctx->height = info->height;
    ctx->n_pixels = n_pixels;
    ctx->rank = info->rank;
    ctx->world = info->world_size;
    ctx->tiles_x = (info->width + 7) / 8;
    ctx->tiles_y = (info->height + 7) / 8;
    ctx->owned_tiles = owned_tile_count(ctx->tiles_x * ctx->tiles_y, ctx->rank, ctx->world);
    ctx->camera = info->camera;
    ctx->cap_mat = info->material_count;
    ctx->cap_sph = info->sphere_count;
    ctx->cap_tri = info->triangle_count;
    ctx->cap_obj = info->object_count;
    ctx->cap_sub = info->sub_object_count;
    ctx->n_mat_dev = info->material_count ? info->material_count : 1;
    ctx->n_tri_dev = info->triangle_count ? info->triangle_count : 1;
    ctx->n_sub_dev = info->sub_object_count ? info->sub_object_count : 1;
    ctx->h_obj.assign(info->objects, info->objects + info->object_count);
    ctx->h_sph.resize(info->sphere_count);
    ctx->h_sub.assign(info->sub_objects, info->sub_objects + info->sub_object_count);

    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipSetDevice", e));
    {
        int n_cu = 0;
        e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipDeviceGetAttribute", e));
        ctx->n_cu = n_cu;
        // the batch buffers' share of device memory: an eighth of the device
        size_t free_b = 0, total_b = 0;
        e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipMemGetInfo", e));
        ctx->batch_budget = total_b / 8;
    }
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamCreate", e));
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) == hipSuccess && khz > 0)
            ctx->wall_khz = (double)khz;
    }
    e = hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamCreate (aux)", e));
    for (hipEvent_t* ev : {&ctx->staging_done, &ctx->ev_resolved[0], &ctx->ev_resolved[1], &ctx->ev_aux_done,
                           &ctx->ev_primary}) {
        e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipEventCreate", e));
    }

    int rc;
    if ((rc = check_params(ctx, &info->params))) return bail(rc);
    if ((rc = validate_ranges(ctx))) return bail(rc);
    ctx->params = info->params;
    ctx->k = 1;  // src/renderer.rs:96

    if ((rc = dev_alloc(ctx, &ctx->d_rays, n_pixels)) || (rc = dev_alloc(ctx, &ctx->d_accum, n_pixels)) ||
        (rc = dev_alloc(ctx, &ctx->d_out, n_pixels)) || (rc = dev_alloc(ctx, &ctx->d_counter, kCounterWords)) ||
        (rc = dev_alloc(ctx, &ctx->d_queue, 4 * kQueueStripesMax * kQueueStride)) ||  // 2 streams x 2 halves
        (rc = dev_alloc(ctx, &ctx->d_slot_sph, 4 * (size_t)info->sphere_count + 4)) ||  // padded groups
        (rc = dev_alloc(ctx, &ctx->d_slot_orig, 4 * (size_t)info->sphere_count + 4)) ||
        (rc = dev_alloc(ctx, &ctx->d_sph_mat, info->sphere_count)) ||
        (rc = dev_alloc(ctx, &ctx->d_bvh, 16 * (size_t)info->sphere_count + 8)) ||  // 8 ordered layouts
        (rc = dev_alloc(ctx, &ctx->d_mat, ctx->n_mat_dev)) || (rc = dev_alloc(ctx, &ctx->d_obj, info->object_count)) ||
        (rc = dev_alloc(ctx, &ctx->d_sub, ctx->n_sub_dev)) || (rc = dev_alloc(ctx, &ctx->d_tri, ctx->n_tri_dev)) ||
        (rc = dev_alloc(ctx, &ctx->d_tri_bounds, 2 * (size_t)ctx->n_tri_dev)) ||
        (rc = dev_alloc(ctx, &ctx->d_tri_extent, 1)) || (rc = dev_alloc(ctx, &ctx->d_stream, 2)) ||
        (rc = dev_alloc(ctx, &ctx->d_srgb, 256)) || (rc = dev_alloc(ctx, &ctx->d_tex, 1)) ||
        (rc = dev_alloc(ctx, &ctx->d_env, 1)))
        return bail(rc);
    ctx->tex_w = ctx->tex_h = ctx->tex_layers = 1;  // a black 1x1 placeholder until textures arrive
    ctx->env_w = ctx->env_h = 1;

    if ((rc = upload_raw(ctx, ctx->d_rays, info->camera_rays, n_pixels * 16)) ||
        (rc = upload_raw(ctx, ctx->d_mat, info->materials, (size_t)info->material_count * 32)) ||
        (rc = upload_spheres(ctx, info->spheres, info->sphere_count)) ||
        (rc = upload_triangles(ctx, info->triangles, info->triangle_count)) ||
        (rc = upload_raw(ctx, ctx->d_obj, info->objects, (size_t)info->object_count * 48)) ||
        (rc = upload_raw(ctx, ctx->d_sub, info->sub_objects, (size_t)info->sub_object_count * 32)))
        return bail(rc);
    float lut[256];
    srgb_table(lut);
    if ((rc = upload_raw(ctx, ctx->d_srgb, lut, sizeof(lut)))) return bail(rc);
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamSynchronize", e));
    ctx->staging_busy = false;
    *out_ctx = ctx;
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)flush_frames(ctx);  // queued frames were submitted: they run before teardown
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    void* bufs[] = {ctx->d_rays, ctx->d_accum, ctx->d_out, ctx->d_counter, ctx->d_queue, ctx->d_slot_sph,
                    ctx->d_slot_orig, ctx->d_bvh, ctx->d_sph_mat, ctx->d_tri_bvh, ctx->d_tri_prims,
                    ctx->d_mat,  ctx->d_obj,   ctx->d_sub, ctx->d_tri,     ctx->d_tex,     ctx->d_env,
                    ctx->d_srgb, ctx->d_tri_extent, ctx->d_tri_order, ctx->d_tri_level_off, ctx->d_model,
                    ctx->d_tri_object, ctx->d_sub_object, ctx->d_object_tris, ctx->d_place, ctx->d_tri_bounds,
                    ctx->d_tile_sched[0], ctx->d_tile_sched[1], ctx->d_frame_light[0], ctx->d_frame_light[1],
                    ctx->d_clock, ctx->d_stream, ctx->d_primary[0], ctx->d_primary[1], ctx->d_tri_qnodes,
                    ctx->d_tri_qgrid, ctx->d_tri_src8, ctx->d_tri_skip8, ctx->d_tri_bvh8, ctx->d_tri_lcert,
                    ctx->d_tri_ltris, ctx->d_brute_paths, ctx->d_brute_queue, ctx->d_brute_counts,
                    ctx->d_query_next, ctx->d_query_buf, ctx->d_radiance_segs, ctx->d_gather_partials, ctx->d_probe_lights, ctx->d_probe_next, ctx->d_lens_cam, ctx->d_feat[0], ctx->d_feat[1], ctx->d_feat_scratch,
                    ctx->d_dn[0], ctx->d_dn[1], ctx->d_dn_out, ctx->d_disp_out, ctx->d_disp_meter,
                    ctx->t_slot[0].plane[0], ctx->t_slot[0].plane[1], ctx->t_slot[0].plane[2],
                    ctx->t_slot[1].plane[0], ctx->t_slot[1].plane[1], ctx->t_slot[1].plane[2],
                    ctx->d_feat_ids, ctx->t_slot[0].ids, ctx->t_slot[1].ids, ctx->d_motion};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->query_pinned) (void)hipHostFree(ctx->query_pinned);
    for (hipEvent_t ev : {ctx->staging_done, ctx->ev_resolved[0], ctx->ev_resolved[1], ctx->ev_aux_done,
                          ctx->ev_primary})
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    delete ctx;
}

static int dispatch_frames(rt_ctx* ctx, uint32_t bounces, uint32_t frames);

// Frame batching (rt_set_frame_batch): rt_compute_frame queues frames and one
// launch renders the whole batch (each pixel's frames back to back on one lane,
// every frame's accumulation and output written). The batch is launched when it
// is full and before anything else touches the context, so every other entry
// point sees exactly the state the sequence of single-frame dispatches leaves.
static int flush_frames(rt_ctx* ctx) {
    if (ctx->pending_frames == 0) return RT_OK;
    const uint32_t n = ctx->pending_frames;
    ctx->pending_frames = 0;
    return dispatch_frames(ctx, ctx->pending_bounces, n);
}

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

int rt_upload_textures(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t layers) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!rgba8 || width == 0 || height == 0 || layers == 0)
        return fail(ctx, RT_E_INVALID, "textures: need non-empty RGBA8 data");
    const size_t texels = (size_t)width * height * layers;
    if (texels != (size_t)ctx->tex_w * ctx->tex_h * ctx->tex_layers || !ctx->d_tex) {
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_tex) RT_HIP(ctx, hipFree(ctx->d_tex));
        ctx->d_tex = nullptr;
        RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_tex), texels * 4));
    }
    ctx->tex_w = width;
    ctx->tex_h = height;
    ctx->tex_layers = layers;
    return upload_raw(ctx, ctx->d_tex, rgba8, texels * 4);
}

int rt_upload_env_map(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!rgba8 || width == 0 || height == 0) return fail(ctx, RT_E_INVALID, "env map: need non-empty RGBA8 data");
    const size_t texels = (size_t)width * height;
    if (texels != (size_t)ctx->env_w * ctx->env_h || !ctx->d_env) {
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_env) RT_HIP(ctx, hipFree(ctx->d_env));
        ctx->d_env = nullptr;
        RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_env), texels * 4));
    }
    ctx->env_w = width;
    ctx->env_h = height;
    // A map whose rows (columns) are each one colour returns the same texel for
    // any u (v): the kernel then skips that coordinate's atan2 (asin).
    const uint32_t* t = reinterpret_cast<const uint32_t*>(rgba8);
    bool rows = true, cols = true;
    for (size_t y = 0; y < height && rows; y++)
        for (size_t x = 1; x < width; x++)
            if (t[y * width + x] != t[y * width]) {
                rows = false;
                break;
            }
    for (size_t y = 1; y < height && cols; y++)
        for (size_t x = 0; x < width; x++)
            if (t[y * width + x] != t[x]) {
                cols = false;
                break;
            }
    ctx->env_uniform = (rows ? 1u : 0u) | (cols ? 2u : 0u);
    return upload_raw(ctx, ctx->d_env, rgba8, texels * 4);
}

int rt_update_params(rt_ctx* ctx, const rt_params* params) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    int rc = check_params(ctx, params);
    if (rc) return rc;
    ctx->params = *params;
    return RT_OK;
}

int rt_reset_accumulation(rt_ctx* ctx, const rt_params* params) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    int rc = check_params(ctx, params);
    if (rc) return rc;
    RT_HIP(ctx, hipMemsetAsync(ctx->d_accum, 0, ctx->n_pixels * 16, ctx->stream));
    ctx->params = *params;
    ctx->k = params->accumulation_index;
    ++ctx->accum_gen;  // rt_denoise_temporal: a new accumulation generation
    return RT_OK;
}

int rt_update_ray_directions(rt_ctx* ctx, const rt_ray* rays, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !rays) return fail(ctx, RT_E_INVALID, "rays is NULL");
    if (count > ctx->n_pixels) return fail(ctx, RT_E_CAPACITY, "more rays than pixels");
    ctx->gen_rays = false;
    return upload_raw(ctx, ctx->d_rays, rays, (size_t)count * 16);
}

int rt_update_camera_matrices(rt_ctx* ctx, const float inverse_projection[16], const float inverse_view[16]) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!inverse_projection || !inverse_view) return fail(ctx, RT_E_INVALID, "matrix is NULL");
    std::memcpy(ctx->inv_proj, inverse_projection, sizeof(ctx->inv_proj));
    std::memcpy(ctx->inv_view, inverse_view, sizeof(ctx->inv_view));
    ctx->gen_rays = true;
    return RT_OK;
}

int rt_update_camera(rt_ctx* ctx, const rt_ray_camera* camera) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!camera) return fail(ctx, RT_E_INVALID, "camera is NULL");
    ctx->camera = *camera;  // passed by value to the next launch
    return RT_OK;
}

int rt_update_spheres(rt_ctx* ctx, const rt_scene_sphere* spheres, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !spheres) return fail(ctx, RT_E_INVALID, "spheres is NULL");
    if (count > ctx->cap_sph) return fail(ctx, RT_E_CAPACITY, "more spheres than the buffer holds");
    return upload_spheres(ctx, spheres, count);
}

int rt_update_triangles(rt_ctx* ctx, const rt_scene_triangle* triangles, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !triangles) return fail(ctx, RT_E_INVALID, "triangles is NULL");
    if (count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    return upload_triangles(ctx, triangles, count);
}

int rt_update_object_info(rt_ctx* ctx, const rt_object_info* objects, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !objects) return fail(ctx, RT_E_INVALID, "objects is NULL");
    if (count > ctx->cap_obj) return fail(ctx, RT_E_CAPACITY, "more objects than the buffer holds");
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    std::vector<rt_object_info> saved = ctx->h_obj;
    std::copy(objects, objects + count, ctx->h_obj.begin());
    int rc = validate_ranges(ctx);
    if (rc) {
        ctx->h_obj.swap(saved);
        return rc;
    }
    // the accelerator culls with the object boxes and walks the sub-object
    // ranges; the device edit path's maps follow the ranges. A change of the
    // other fields (material_index) invalidates neither.
    bool boxes = false, ranges = false;
    for (uint32_t i = 0; i < count; i++) {
        const rt_object_info &a = saved[i], &b = objects[i];
        boxes |= std::memcmp(a.min_bounds, b.min_bounds, 12) != 0 || std::memcmp(a.max_bounds, b.max_bounds, 12) != 0;
        ranges |= a.first_sub_object_index != b.first_sub_object_index || a.sub_object_count != b.sub_object_count;
    }
    if (boxes || ranges) ctx->tri_dirty = true;
    if (ranges) ctx->models_valid = false;
    return upload_raw(ctx, ctx->d_obj, objects, (size_t)count * 48);
}

int rt_update_sub_object_info(rt_ctx* ctx, const rt_sub_object_info* sub_objects, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !sub_objects) return fail(ctx, RT_E_INVALID, "sub_objects is NULL");
    if (count > ctx->cap_sub) return fail(ctx, RT_E_CAPACITY, "more sub-objects than the buffer holds");
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    std::vector<rt_sub_object_info> saved = ctx->h_sub;
    std::copy(sub_objects, sub_objects + count, ctx->h_sub.begin());
    int rc = validate_ranges(ctx);
    if (rc) {
        ctx->h_sub.swap(saved);
        return rc;
    }
    for (uint32_t i = 0; i < count; i++)
        if (saved[i].first_triangle_index != sub_objects[i].first_triangle_index ||
            saved[i].triangle_count != sub_objects[i].triangle_count)
            ctx->models_valid = false;  // the device edit path's triangle maps are stale
    ctx->tri_dirty = true;
    return upload_raw(ctx, ctx->d_sub, sub_objects, (size_t)count * 32);
}

int rt_update_materials(rt_ctx* ctx, const rt_scene_material* materials, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !materials) return fail(ctx, RT_E_INVALID, "materials is NULL");
    if (count > ctx->cap_mat) return fail(ctx, RT_E_CAPACITY, "more materials than the buffer holds");
    return upload_raw(ctx, ctx->d_mat, materials, (size_t)count * 32);
}

static int dispatch_frames(rt_ctx* ctx, uint32_t bounces, uint32_t frames);

int rt_dispatch(rt_ctx* ctx, uint32_t bounces) {
    RT_ENTER(ctx);
    return dispatch_frames(ctx, bounces, 1);
}

static int dispatch_batch(rt_ctx* ctx, uint32_t bounces, uint32_t frames);

// Renders `frames` frames starting at Params.accumulation_index: one launch (dispatch_batch),
// or, when the batch's buffers -- the frame lights and the primary records, 32 B per owned
// pixel, frame and sample each -- would outgrow the batch budget (an eighth of the device's
// memory by default), consecutive launches of as many frames as fit, which render the same
// bits: frames are independent but for the accumulation, which every launch adds to in order.
static int dispatch_frames(rt_ctx* ctx, uint32_t bounces, uint32_t frames) {
    const rt_params& p = ctx->params;
    const uint64_t samples = std::max<uint32_t>(1u, p.accumulate == 1u ? p.compute_per_frame : 1u);
    const uint64_t per_frame = (uint64_t)ctx->owned_tiles * 64u * samples * 2u * 2u * sizeof(float4);
    const uint64_t fit = std::max<uint64_t>(1u, ctx->batch_budget / std::max<uint64_t>(1u, per_frame));
    if (frames <= fit) return dispatch_batch(ctx, bounces, frames);
    const uint32_t k0 = ctx->params.accumulation_index;
    int rc = RT_OK;
    for (uint32_t done = 0; done < frames && rc == RT_OK;) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(fit, frames - done);
        if (p.accumulate == 1u) ctx->params.accumulation_index = k0 + done;
        rc = dispatch_batch(ctx, bounces, n);
        done += n;
    }
    ctx->params.accumulation_index = k0;  // the batch's Params, as one launch leaves them
    return rc;
}

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

static size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

static void scene_base_args(rt_ctx* ctx, KernelArgs& ka) {
    const rt_params& p = ctx->params;
    ka.sphere_slots = ctx->d_slot_sph;
    ka.sphere_orig = ctx->d_slot_orig;
    ka.sphere_material = ctx->d_sph_mat;
    ka.sphere_bvh = reinterpret_cast<const float4*>(ctx->d_bvh);
    ka.sphere_always = ctx->n_always;
    ka.sphere_nodes = ctx->n_nodes;
    ka.sphere_extent = ctx->sphere_extent;
    ka.sphere_rmin = ctx->sphere_rmin;
    ka.sphere_rmax = ctx->sphere_rmax;
    ka.tri_accel = (ctx->use_tri_bvh && p.object_count != 0) ? 1u : 0u;
    ka.tri_nodes = ka.tri_accel ? ctx->tri_nodes : 0u;
    ka.tri_prim_count = ka.tri_accel ? ctx->tri_prim_count : 0u;
    ka.tri_extent = ctx->d_tri_extent;
    ka.tri_bvh = reinterpret_cast<const float4*>(ctx->d_tri_bvh);
    ka.tri_prims = reinterpret_cast<const uint4*>(ctx->d_tri_prims);
    ka.materials = ctx->d_mat;
    ka.objects = ctx->d_obj;
    ka.sub_objects = ctx->d_sub;
    ka.triangles = ctx->d_tri;
    ka.textures = ctx->d_tex;
    ka.env = ctx->d_env;
    ka.srgb = ctx->d_srgb;
    ka.camera_origin[0] = ctx->camera.origin[0];
    ka.camera_origin[1] = ctx->camera.origin[1];
    ka.camera_origin[2] = ctx->camera.origin[2];
    ka.width = ctx->width;
    ka.accumulation_index = p.accumulation_index;
    ka.accumulate = p.accumulate;
    ka.sphere_count = p.sphere_count;
    ka.sphere_slot_count = ctx->n_slots;
    ka.object_count = p.object_count;
    ka.compute_per_frame = p.compute_per_frame;
    ka.texture_width = p.texture_width;
    ka.texture_height = p.texture_height;
    ka.env_map_width = p.env_map_width;
    ka.env_map_height = p.env_map_height;
    ka.material_count = ctx->n_mat_dev;
    ka.sub_object_count = ctx->n_sub_dev;
    ka.triangle_count = ctx->n_tri_dev;
    ka.tex_w = ctx->tex_w;
    ka.tex_h = ctx->tex_h;
    ka.tex_layers = ctx->tex_layers;
    ka.env_w = ctx->env_w;
    ka.env_h = ctx->env_h;
    ka.env_uniform = ctx->env_uniform;
    ka.height = ctx->height;
    ka.gen_rays = ctx->gen_rays ? 1u : 0u;
    ka.aspect = (float)ctx->width / (float)ctx->height;  // src/camera.rs:142
    std::memcpy(ka.inv_proj, ctx->inv_proj, sizeof(ka.inv_proj));
    std::memcpy(ka.inv_view, ctx->inv_view, sizeof(ka.inv_view));
}

// Lays out the LDS image for `layouts` sphere BVH layouts and returns the highest placement mode
// up to `max_mode` that it fits.
// dynamic LDS carve-up: sphere slots | materials | objects | slot->orig | sphere materials | BVH | srgb
static int scene_carve_layouts(rt_ctx* ctx, KernelArgs& ka, uint32_t layouts, size_t mode1_budget, int max_mode,
                               SceneLaunch& sl) {
    const rt_params& p = ctx->params;
    size_t off = al16((size_t)ctx->n_slots * 16);
    ka.lds_mat_offset = (uint32_t)off;
    off = al16(off + (size_t)ctx->n_mat_dev * sizeof(RtMaterial));
    ka.lds_mat_aux_offset = (uint32_t)off;
    off = al16(off + (size_t)ctx->n_mat_dev * 32);
    ka.lds_obj_offset = (uint32_t)off;
    off = al16(off + (size_t)p.object_count * sizeof(RtObject));
    ka.lds_orig_offset = (uint32_t)off;
    off = al16(off + (size_t)ctx->n_slots * 4);
    ka.lds_smat_offset = (uint32_t)off;
    off = al16(off + (size_t)p.sphere_count * 4);
    ka.lds_nodes_offset = (uint32_t)off;
    off = al16(off + (size_t)layouts * ctx->n_nodes * sizeof(SphereBvhNode));
    // sphere-only scenes: one more record, the sentinel that ends the path kernel's walk
    // (rt_sphere_walk.h). Every kernel that lays out its image here (the query, occlusion, radiance,
    // ambient and lens kernels, which neither write nor read it) inherits the 32 bytes, also where
    // this decides between eight layouts and one or between placement modes.
    if (p.object_count == 0) off += sizeof(SphereBvhNode);
    sl.mode1_bytes = off + kLdsTailBytes;
    ka.lds_tri_nodes_offset = (uint32_t)off;
    off = al16(off + (size_t)ka.tri_nodes * sizeof(SphereBvhNode));
    ka.lds_tri_prims_offset = (uint32_t)off;
    off = al16(off + (size_t)ka.tri_prim_count * sizeof(SubObjectPrim));
    // the sub-object records the leaves read, when they fit the mode-2 budget too
    // (one dependent global load less per leaf test; tuning "stage_subs" 0 switches it off)
    ka.lds_sub_offset = 0;
    if (ctx->stage_subs && ka.sub_object_count != 0) {
        const size_t with = al16(off + (size_t)ka.sub_object_count * sizeof(RtSubObject));
        if (with + kLdsTailBytes <= kLdsAccelBudget) {
            ka.lds_sub_offset = (uint32_t)off;
            off = with;
        }
    }
    sl.mode2_bytes = off + kLdsTailBytes;
    if (ka.tri_accel && ka.tri_nodes != 0 && sl.mode2_bytes <= kLdsAccelBudget && max_mode >= 2)
        return 2;
    if (sl.mode1_bytes <= mode1_budget && max_mode >= 1) return 1;
    return 0;
}

// Direction-ordered sphere BVH layouts (order_bvh_by_octant) when all eight
// fit the LDS mode that one layout gets (up to the mode-2 budget, in fewer,
// larger workgroups); otherwise layout 0 alone.
static void scene_carve(rt_ctx* ctx, KernelArgs& ka, int max_mode, SceneLaunch& sl) {
    sl.tris = ctx->params.object_count != 0;
    sl.mode = scene_carve_layouts(ctx, ka, 1, kLdsSceneBudget, max_mode, sl);
    sl.layouts = 1;
    if (ctx->sphere_octants && ctx->n_nodes != 0) {
        if (scene_carve_layouts(ctx, ka, 8, kLdsAccelBudget, max_mode, sl) == sl.mode)
            sl.layouts = 8;
        else
            scene_carve_layouts(ctx, ka, 1, kLdsSceneBudget, max_mode, sl);
    }
}

// What the walks of placement sl.mode read, derived when stale (primary stream), the walk's batch
// thresholds, and the image size.
static int scene_accel_args(rt_ctx* ctx, KernelArgs& ka, SceneLaunch& sl) {
    ka.sphere_nodes = sl.layouts * ctx->n_nodes;
    ka.sphere_octant_stride = sl.layouts == 8 ? ctx->n_nodes : 0u;
    ka.sphere_boxes_ordered = (sl.layouts == 8 && ctx->sphere_boxes_ordered && !sl.tris) ? 1u : 0u;
    const bool certified = sl.tris && sl.mode <= 1 && ka.tri_accel && ctx->tri_prune_mode == 1;
    ka.trav_threshold = ctx->trav_threshold ? ctx->trav_threshold : trav_threshold_for(sl.mode, sl.tris, certified);
    ka.leaf_batch = ctx->leaf_batch ? ctx->leaf_batch : leaf_batch_for(sl.mode, certified);
    // walks of the binary triangle accelerator from global memory read its direction-ordered
    // layouts (8 x tri_nodes positions, 32-B and 16-B quantized copies), else the single one
    ka.tri_qnodes = nullptr;
    ka.tri_qgrid = nullptr;
    ka.tri_octant_stride = 0;
    const bool global_walk = sl.tris && sl.mode <= 1 && ka.tri_accel && ka.tri_nodes != 0;
    const bool octants = global_walk && ctx->tri_octants_built;
    const bool qnodes = global_walk && ctx->use_qnodes;
    int rc;
    if (octants || qnodes) {
        const uint32_t n_out = octants ? 8u * ka.tri_nodes : ka.tri_nodes;
        if (qnodes && (rc = grow_buffer(ctx, "quantized triangle nodes", &ctx->d_tri_qnodes, &ctx->qnodes_cap,
                                        (size_t)n_out * sizeof(uint4), &ctx->qnodes_dirty)))
            return rc;
        if (!ctx->d_tri_qgrid) RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_tri_qgrid), 2 * sizeof(float4)));
        if (ctx->qnodes_dirty || ctx->derived_octants != octants || ctx->derived_qnodes != qnodes) {
            // after the accelerator's upload or refit (primary stream)
            RT_HIP(ctx, rt_launch_quantize_tri_nodes(reinterpret_cast<const SphereBvhNode*>(ctx->d_tri_bvh),
                                                     ka.tri_nodes, octants ? ctx->d_tri_src8 : nullptr,
                                                     octants ? ctx->d_tri_skip8 : nullptr, n_out,
                                                     octants ? ctx->d_tri_bvh8 : nullptr,
                                                     qnodes ? ctx->d_tri_qnodes : nullptr, ctx->d_tri_qgrid,
                                                     ctx->stream));
            ctx->qnodes_dirty = false;
            ctx->derived_octants = octants;
            ctx->derived_qnodes = qnodes;
            ctx->primary_dirty = true;  // an auxiliary-stream batch waits for it
        }
        if (qnodes) {
            ka.tri_qnodes = ctx->d_tri_qnodes;
            ka.tri_qgrid = ctx->d_tri_qgrid;
        }
        if (octants) {
            ka.tri_bvh = reinterpret_cast<const float4*>(ctx->d_tri_bvh8);
            ka.tri_octant_stride = ka.tri_nodes;
            ka.tri_nodes = n_out;
        }
    }
    // distance pruning of the binary walk: certified (the leaf certificates,
    // rebuilt on the device after any change), or the round-3 relative slack, or none
    ka.tri_prune_mode = (sl.tris && ka.tri_accel && ka.tri_nodes != 0) ? (uint32_t)ctx->tri_prune_mode : 0u;
    ka.tri_prune = ka.tri_prune_mode == 2u ? kTriPruneRho : 0.0f;
    ka.tri_leafcert = nullptr;
    if (ka.tri_prune_mode == 1u && ka.tri_prim_count != 0 && sl.mode <= 1) {  // (mode 2 culls by box alone)
        if ((rc = grow_buffer(ctx, "leaf certificates", &ctx->d_tri_lcert, &ctx->tri_lcert_cap,
                              (size_t)ka.tri_prim_count * sizeof(TriLeafCert), &ctx->cones_dirty)))
            return rc;
        if (ctx->cones_dirty) {
            RT_HIP(ctx, rt_launch_tri_leafcert(ctx->d_tri_prims, ka.tri_prim_count, ctx->d_sub, ctx->d_tri,
                                               ctx->n_tri_dev, ctx->d_tri_lcert, ctx->stream));
            ctx->cones_dirty = false;
            ctx->primary_dirty = true;  // an auxiliary-stream batch waits for it
        }
        ka.tri_leafcert = ctx->d_tri_lcert;
    }
    // cooperative leaf batches (walks from global memory): the leaves' triangle blocks
    ka.tri_leaftris = nullptr;
    sl.coop = sl.tris && sl.mode <= 1 && ka.tri_accel && ka.tri_nodes != 0 && ka.tri_prim_count != 0 &&
                      ctx->use_coop_leaves;
    if (sl.coop) {
        if ((rc = grow_buffer(ctx, "leaf triangle blocks", &ctx->d_tri_ltris, &ctx->tri_ltris_cap,
                              (size_t)ka.tri_prim_count * kLeafTriWords * sizeof(uint4), &ctx->ltris_dirty)))
            return rc;
        if (ctx->ltris_dirty) {
            RT_HIP(ctx, rt_launch_tri_leaftris(ctx->d_tri_prims, ka.tri_prim_count, ctx->d_tri, ctx->n_tri_dev,
                                               ctx->d_tri_ltris, ctx->stream));
            ctx->ltris_dirty = false;
            ctx->primary_dirty = true;  // an auxiliary-stream batch waits for it
        }
        ka.tri_leaftris = ctx->d_tri_ltris;
    }
    if (sl.mode == 2) {
        ka.lds_srgb_offset = (uint32_t)(sl.mode2_bytes - kLdsTailBytes);
        sl.lds_bytes = sl.mode2_bytes;
    } else if (sl.mode == 1) {
        ka.lds_srgb_offset = (uint32_t)(sl.mode1_bytes - kLdsTailBytes);
        sl.lds_bytes = sl.mode1_bytes;
    } else {
        ka.lds_srgb_offset = 0;
        sl.lds_bytes = kLdsTailBytes;
    }
    return RT_OK;
}

// Which instance of the path kernel a launch runs (the one place that decides it): the
// frame-parallel instance (pathtrace.hip, kFramePar) for a frame-parallel batch -- accumulating,
// its lights within kMaxParallelLights -- that traces at least one segment per sample; the
// generic instance for every other launch (non-accumulating, "frame_parallel" 0, a batch past
// the light limit, bounces == 0: its samples end in setup, which only the generic instance
// handles) and when the tuning key "frame_par_instance" is 0.
static bool rt_path_frame_par_instance(bool frame_par_batch, uint32_t accumulate, uint32_t bounces, bool enabled) {
    return enabled && frame_par_batch && accumulate == 1u && bounces >= 1u;
}

// ---- a batch launch, stage by stage (dispatch_batch) --------------------------------------------

// What the stages hand to each other.
struct BatchLaunch {
    uint32_t bounces = 0, frames = 0;
    uint64_t owned_px = 0;
    bool frame_par = false;    // a frame-parallel batch: (frame, tile) units, lights resolved afterwards
    bool fp_instance = false;  // the path kernel runs as its frame-parallel instance
    SceneLaunch sl;
    const rt_ctx::OccEntry* occ = nullptr;  // the path launch's workgroup size and residency
    size_t lds_bytes = 0;      // the path launch's dynamic LDS
    uint32_t blocks = 0;       // its workgroups
    bool sched = false;        // it claims tiles in cost order
    int si = 0;                // the stream it runs on: 0 the primary, 1 the auxiliary one
    hipStream_t S = nullptr;
    bool primary = false;      // the pre-pass runs ahead of it
};

// The arguments every frame launch starts from.
static void batch_base_args(rt_ctx* ctx, const BatchLaunch& b, KernelArgs& ka) {
    ka.camera_rays = ctx->d_rays;
    ka.accum = ctx->d_accum;
    ka.output = ctx->d_out;
    ka.ray_counter = ctx->d_counter;
    ka.diag = ctx->d_counter + 1;
    ka.queue_stripes = ctx->queue_stripes;  // (queue counters: per stream, set at launch)
    scene_base_args(ctx, ka);
    ka.bounces = b.bounces;
    ka.tiles_x = ctx->tiles_x;
    ka.owned_tiles = ctx->owned_tiles;
    ka.rank = ctx->rank;
    ka.world_size = ctx->world;
    ka.drain_threshold = ctx->drain_threshold;
    ka.drain_min_steps = ctx->drain_min_steps;
    ka.frames = b.frames;
}

// Batch plan. Frame-parallel batch: one queue unit per (frame, tile), lights resolved in order
// by rt_resolve_frames_kernel (accumulating renders; non-accumulating frames are
// all the same frame and keep the per-lane sequence).
static int plan_batch(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    const rt_params& p = ctx->params;
    b.owned_px = (uint64_t)ctx->owned_tiles * 64u;
    b.frame_par = b.frames > 1 && p.accumulate == 1u && ctx->frame_parallel &&
                  (uint64_t)b.frames * p.compute_per_frame <= kMaxParallelLights && p.compute_per_frame > 0;
    ka.frame_light = nullptr;
    ka.queue_units = ctx->owned_tiles;
    if (b.frame_par) {
        const size_t need = (size_t)b.owned_px * b.frames * p.compute_per_frame;  // float4 entries
        if (need * sizeof(float4) > ctx->frame_light_cap) {
            // sized for the configured batch too, so a short first batch (a warmup)
            // does not leave a reallocation for a later, timed launch; two buffers,
            // one per batch parity (overlapped batches), within the batch budget
            const size_t want = std::max<size_t>(
                need, std::min<size_t>(ctx->batch_budget / (2 * sizeof(float4)),
                                       (size_t)b.owned_px * std::min<uint64_t>((uint64_t)ctx->frame_batch *
                                                                                   p.compute_per_frame,
                                                                               kMaxParallelLights)));
            const int rc = grow_buffer(ctx, "frame lights", ctx->d_frame_light, &ctx->frame_light_cap,
                                       want * sizeof(float4), nullptr, 2);
            if (rc) return rc;
        }
        ka.queue_units = ctx->owned_tiles * b.frames;
        ka.unit_tile_major = ctx->unit_tile_major ? 1u : 0u;
        ka.light_plane = (uint32_t)b.owned_px;
    }
    b.fp_instance = rt_path_frame_par_instance(b.frame_par, p.accumulate, b.bounces, ctx->frame_par_instance);
    return RT_OK;
}

// Brute-force launch: the reference's sweeps as a wavefront (rt_brute_wf_kernel): the mode-1 scene
// image, then the sub-object tiles (mode 1) or the hit lists (mode 2: the records through the
// scalar cache; a scene without triangles has no records to stream and sweeps its
// spheres in the LDS-tiled kernel); every pass (frame, sample) in order, one launch per
// bounce level
static int launch_brute(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    SceneLaunch& sl = b.sl;
    scene_carve_layouts(ctx, ka, 1, kLdsSceneBudget, ctx->force_global_scene ? 0 : ctx->max_lds_mode, sl);
    ka.lds_srgb_offset = (uint32_t)(sl.mode1_bytes - kLdsTailBytes);
    ka.lds_stack_offset = (uint32_t)al16(sl.mode1_bytes);
    const uint32_t samples = ka.accumulate == 1u ? ka.compute_per_frame : 1u;
    const uint64_t passes = (uint64_t)b.frames * samples;
    const bool scalar_stream = sl.tris && ctx->brute == 2;
    const size_t lds = ka.lds_stack_offset + rt_brute_wf_tile_bytes(scalar_stream);
    int dev = 0, max_optin = 0;
    RT_HIP(ctx, hipGetDevice(&dev));
    RT_HIP(ctx, hipDeviceGetAttribute(&max_optin, hipDeviceAttributeSharedMemPerBlockOptin, dev));
    if (lds > (size_t)max_optin - 256)
        return fail(ctx, RT_E_CAPACITY, "brute-force mode: spheres, materials and objects must fit in LDS");
    ka.sphere_octant_stride = 0;
    ka.sphere_boxes_ordered = 0;
    ka.stream_bytes = ctx->d_stream;
    ka.l2_stream_bytes = ctx->d_stream + 1;
    ka.frame_light = nullptr;
    RT_HIP(ctx, join_aux(ctx));
    int rc = claim_clock_slot(ctx, ctx->stream, ka);
    if (rc) return rc;
    const size_t n_slots = (size_t)ctx->owned_tiles * 64u;
    // per pass one counter per bounce level: the entries of each level's queue
    ka.brute_levels = std::max(1u, b.bounces) + 1u;
    const size_t n_counts = (size_t)passes * ka.brute_levels;
    if ((rc = grow_buffer(ctx, "brute-force paths", &ctx->d_brute_paths, &ctx->brute_paths_cap,
                          4 * n_slots * sizeof(float4))) ||
        (rc = grow_buffer(ctx, "brute-force queue", &ctx->d_brute_queue, &ctx->brute_queue_cap,
                          2 * n_slots * sizeof(uint32_t))) ||
        (rc = grow_buffer(ctx, "brute-force counters", &ctx->d_brute_counts, &ctx->brute_counts_cap,
                          n_counts * sizeof(uint32_t))))
        return rc;
    RT_HIP(ctx, hipMemsetAsync(ctx->d_brute_counts, 0, n_counts * sizeof(uint32_t), ctx->stream));
    ka.brute_paths = ctx->d_brute_paths;
    ka.brute_queue = ctx->d_brute_queue;
    ka.brute_counts = ctx->d_brute_counts;
    // workgroups per launch: enough for every chunk of queue entries, at most 16 per CU
    const uint32_t chunks = (uint32_t)((n_slots + rt_brute_wf_chunk() - 1u) / rt_brute_wf_chunk());
    const uint32_t blocks = std::min<uint32_t>(chunks, 16u * (uint32_t)std::max<int>(1, (int)ctx->n_cu));
    for (uint64_t pass = 0; pass < passes; ++pass)
        for (uint32_t level = 0; level < std::max(1u, b.bounces); ++level) {
            ka.brute_pass = (uint32_t)pass;
            ka.brute_level = level;
            RT_HIP(ctx, rt_launch_brute_wf(ka, sl.tris, scalar_stream, lds, blocks, ctx->stream));
        }
    ctx->last_blocks = blocks;
    ctx->last_passes = RT_PASS_BRUTE | (scalar_stream ? RT_PASS_BRUTE_STREAM : 0u);
    ctx->last_lds = (uint32_t)lds;
    ctx->last_threads = 256;  // (last_mode: the last path launch's, as rt_launch_config has always reported)
    ctx->primary_dirty = true;
    return RT_OK;
}

// Path occupancy. Persistent grid: as many workgroups as can be resident (never more than
// one wave per tile); waves then pull tiles from the queue.
static int path_occupancy(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    const SceneLaunch& sl = b.sl;
    // per-thread LDS after the scene image: the cooperative leaf batch's per-wave scratch
    const size_t lane_pt = sl.coop ? (size_t)kLeafBatchWaveBytes / 64u : 0u;
    // The environment line (rt_kernel_args.h): the decoded texels of a rows- or columns-uniform
    // environment map, staged after the scene image's tail by the instances that stage the scene.
    size_t line_bytes = 0;
    if (sl.mode >= 1) {
        const uint32_t n = env_line_texels(ka.env_uniform, ka.env_w, ka.env_h);
        if (n != 0 && n <= kEnvLineMax) line_bytes = (size_t)n * sizeof(float4);
    }
    const rt_ctx::OccKey key{sl.lds_bytes, lane_pt, line_bytes, sl.mode, sl.tris ? 1u : 0u, ctx->force_threads,
                             ctx->waves_cap};
    rt_ctx::OccEntry& oc = ctx->occ_cache[b.fp_instance ? 1 : 0];
    if (oc.blocks_per_cu == 0 || !same_key(oc.key, key)) {
        int per_cu = 0;
        uint32_t threads = 0;
        hipError_t oe = rt_pathtrace_pick_config(sl.mode, sl.tris, b.fp_instance, sl.lds_bytes, lane_pt,
                                                 ctx->force_threads, ctx->waves_cap, &threads, &per_cu);
        if (oe != hipSuccess) return hip_fail(ctx, "rt_pathtrace_pick_config (occupancy query)", oe);
        // the line is staged only where the launch keeps its workgroup size and its workgroups per CU with it
        oc.env_line = false;
        if (line_bytes != 0) {
            int per_cu_line = 0;
            uint32_t threads_line = 0;
            oe = rt_pathtrace_pick_config(sl.mode, sl.tris, b.fp_instance, sl.lds_bytes + line_bytes, lane_pt,
                                          ctx->force_threads, ctx->waves_cap, &threads_line, &per_cu_line);
            if (oe != hipSuccess) (void)hipGetLastError();  // no configuration holds it: the global path
            oc.env_line = oe == hipSuccess && threads_line == threads && per_cu_line == per_cu;
        }
        oc.key = key;
        oc.blocks_per_cu = per_cu;
        oc.threads = threads;
    }
    b.occ = &oc;
    // this launch's configuration (rt_launch_config reports it)
    ctx->last_threads = oc.threads;
    ctx->last_mode = sl.mode;
    b.lds_bytes = sl.lds_bytes;
    if (oc.env_line) {  // right after the tail (a multiple of 16 bytes, as the image before it)
        ka.env_uniform |= kEnvLineStaged;
        b.lds_bytes += line_bytes;
    }
    // the leaf batch scratch after the scene image, its tail and the environment line
    ka.lds_leafbatch_offset = (uint32_t)al16(b.lds_bytes);
    if (sl.coop) b.lds_bytes = ka.lds_leafbatch_offset + (size_t)oc.threads * lane_pt;
    const uint32_t waves_per_block = oc.threads / 64;
    const uint64_t resident = (uint64_t)oc.blocks_per_cu * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 1);
    const uint64_t wanted = ((uint64_t)ka.queue_units + waves_per_block - 1) / waves_per_block;
    b.blocks = (uint32_t)(wanted < resident ? wanted : resident);
    return RT_OK;
}

// Stream and queue selection.
// Overlapped batches: frame-parallel batches alternate between
// the primary and the auxiliary stream. Batch i's path kernel depends on no
// other batch (it writes its own light buffer, i % 2), so it starts on the CUs
// that batch i-1's drain frees; only its resolve waits for batch i-1's resolve
// (the accumulation order). Everything else stays on the primary stream.
static int select_stream(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    b.si = (b.frame_par && ctx->batch_overlap) ? (int)(ctx->batches & 1u) : 0;
    b.S = b.si ? ctx->aux_stream : ctx->stream;
    if (!b.frame_par) RT_HIP(ctx, join_aux(ctx));  // a plain launch follows every earlier batch
    if (b.si && ctx->primary_dirty) {  // primary-stream work (uploads, resets) the batch must follow
        RT_HIP(ctx, follow_primary(ctx, b.S));
        ctx->primary_dirty = false;
    }
    const uint32_t parity = ctx->queue_parity[b.si];
    ka.queue = ctx->d_queue + (size_t)(2 * b.si + parity) * kQueueStripesMax * kQueueStride;
    ka.queue_next = ctx->d_queue + (size_t)(2 * b.si + (parity ^ 1u)) * kQueueStripesMax * kQueueStride;
    if (b.frame_par) ka.frame_light = ctx->d_frame_light[ctx->batches & 1u];
    return RT_OK;
}

// Schedule state.
static int schedule_state(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    // Cost-ordered schedule, when each wave takes several tiles per launch (with
    // about one tile per wave the claim order cannot shorten the drain, and the
    // sort would sit on a short launch's critical path).
    // Frame-parallel batches claim in index order: with the drain paid once per batch
    // (and overlapped) the cost order's recording and sort cost more than they save,
    // and index order keeps neighbouring tiles together (C2 -5.2%, C3 -2.7% per frame
    // measured, profiles/archive/r02_knobs); RT_BATCH_SCHEDULE=1 sorts them too (A/B switch).
    const uint32_t waves_per_block = b.occ->threads / 64;
    b.sched = ctx->tile_schedule && (!b.frame_par || ctx->batch_schedule) &&
              (uint64_t)ka.queue_units >= kSchedMinTilesPerWave * b.blocks * waves_per_block;
    if (!b.sched) return RT_OK;
    const size_t n = ctx->owned_tiles;
    uint32_t*& state = ctx->d_tile_sched[b.si];
    if (!state) {
        int rc = dev_alloc(ctx, &state, 4 * n + 2);
        if (rc) return rc;
        RT_HIP(ctx, hipMemsetAsync(state, 0, (4 * n + 2) * 4, ctx->stream));
        ctx->primary_dirty = true;
        RT_HIP(ctx, follow_primary(ctx, b.S));
        ctx->sched_launches[b.si] = 0;
    }
    ka.sched = state;
    // orders[parity] was written by this stream's previous launch
    ka.sched_bits = (uint32_t)(ctx->sched_launches[b.si] & 1u);
    ka.tile_cost = ka.sched + ka.sched_bits * (size_t)n;
    ka.tile_order = ctx->sched_launches[b.si] ? ka.sched + (2u + ka.sched_bits) * (size_t)n : nullptr;
    return RT_OK;
}

// Primary pre-pass.
// Coherent primary rays: the first segment of every (frame, sample, pixel) of the launch
// traced by rt_primary_kernel as 8x8 packets, stream-ordered before the path kernel
// (scene image in LDS, binary triangle accelerator). By default only where the triangle
// accelerator stays in global memory (mode 1 with triangles, C5: wall -12%); with the
// accelerator in LDS (C3, C4) or no triangles (C2) the pass costs more wall time than it
// takes off the path kernel (+13%, +13%, +23%: profiles/r03_i/ab_primary.jsonl)
// (within the batch budget: a batch too large for it traces its first segments in the path kernel)
static int primary_prepass(rt_ctx* ctx, BatchLaunch& b, KernelArgs& ka) {
    const rt_params& p = ctx->params;
    const SceneLaunch& sl = b.sl;
    const size_t need =  // records
        (size_t)b.owned_px * b.frames * std::max<uint32_t>(1u, p.accumulate == 1u ? p.compute_per_frame : 1u);
    b.primary = b.bounces > 0 && sl.mode >= 1 && sl.tris && ka.compute_per_frame > 0 &&
                (ctx->primary_pass == 1 || (ctx->primary_pass == -1 && sl.mode == 1)) &&
                2 * need * sizeof(uint4) <= ctx->batch_budget;
    ka.primary = nullptr;
    if (!b.primary) return RT_OK;
    if (need * sizeof(uint4) > ctx->primary_cap) {
        const size_t want = std::max<size_t>(
            need, std::min<size_t>(ctx->batch_budget / (2 * sizeof(uint4)), (size_t)b.owned_px * ctx->frame_batch));
        const int rc = grow_buffer(ctx, "primary records", ctx->d_primary, &ctx->primary_cap, want * sizeof(uint4),
                                   nullptr, 2);
        if (rc) return rc;
    }
    KernelArgs pka = ka;
    pka.primary = ctx->d_primary[ctx->batches & 1u];
    pka.queue_units = ctx->owned_tiles * b.frames;  // one unit per (frame, tile)
    pka.primary_tile_major = ctx->primary_tile_major ? 1u : 0u;
    const size_t image = sl.mode == 2 ? sl.mode2_bytes : sl.mode1_bytes;
    // (the 64-VGPR variant is built at 256 threads only)
    const uint32_t min_waves = (sl.mode == 2 || ctx->primary_threads != 256u) ? 0u : ctx->primary_min_waves;
    RT_HIP(ctx, rt_launch_primary(pka, sl.mode, sl.tris, image, sl.mode == 2 ? 1024u : ctx->primary_threads, min_waves,
                                  b.S));
    ka.primary = pka.primary;
    return RT_OK;
}

// The path kernel, the batch's resolve, and the end-of-launch bookkeeping.
static int launch_path_and_resolve(rt_ctx* ctx, const BatchLaunch& b, const KernelArgs& ka) {
    const rt_params& p = ctx->params;
    hipError_t e = rt_launch_pathtrace(ka, b.sl.mode, b.sl.tris, b.fp_instance, b.occ->threads, b.lds_bytes, b.blocks,
                                       b.S);
    ctx->last_blocks = b.blocks;
    ctx->last_passes = RT_PASS_PATH | (b.primary ? RT_PASS_PRIMARY : 0u) | (b.frame_par ? RT_PASS_RESOLVE : 0u) |
                       (b.fp_instance ? RT_PASS_PATH_FRAME_PAR : 0u);
    ctx->last_lds = (uint32_t)b.lds_bytes;
    if (e != hipSuccess) return hip_fail(ctx, "rt_pathtrace_kernel launch", e);
    if (b.frame_par) {
        // the accumulation is summed in frame order: after the previous batch's resolve
        if (ctx->batches > 0) RT_HIP(ctx, hipStreamWaitEvent(b.S, ctx->ev_resolved[(ctx->batches - 1) & 1u], 0));
        e = rt_launch_resolve(ctx->d_accum, ctx->d_out, ka.frame_light, ctx->width, ctx->height, ctx->tiles_x,
                              ctx->owned_tiles, ctx->rank, ctx->world, p.accumulation_index, p.compute_per_frame,
                              b.frames, ka.launch_clock ? ka.launch_clock + 2 : nullptr, b.S);
        if (e != hipSuccess) return hip_fail(ctx, "rt_resolve_frames_kernel launch", e);
        RT_HIP(ctx, hipEventRecord(ctx->ev_resolved[ctx->batches & 1u], b.S));
        ctx->batches += 1;
    }
    // every tile is claimed once and every wave makes one final failing claim
    ctx->queue_parity[b.si] ^= 1u;  // this launch zeroes the other half for the stream's next one
    if (b.si) {
        RT_HIP(ctx, hipEventRecord(ctx->ev_aux_done, b.S));
        ctx->aux_outstanding = true;
    }
    // A plain launch (not frame-parallel) reads and writes the accumulation and
    // the output on the primary stream; a later overlapped batch on the auxiliary
    // stream must follow it (its resolve writes both), not just the previous batch.
    if (!b.frame_par) ctx->primary_dirty = true;
    if (b.sched) ++ctx->sched_launches[b.si];
    return RT_OK;
}

// One launch rendering `frames` frames starting at Params.accumulation_index.
static int dispatch_batch(rt_ctx* ctx, uint32_t bounces, uint32_t frames) {
    const rt_params& p = ctx->params;
    int rc;
    if ((rc = refresh_sphere_slots(ctx, p.sphere_count, p.object_count == 0)) ||
        (rc = refresh_tri_accel(ctx, p.object_count)))
        return rc;
    KernelArgs ka{};
    BatchLaunch b;
    b.bounces = bounces;
    b.frames = frames;
    batch_base_args(ctx, b, ka);
    if ((rc = plan_batch(ctx, b, ka))) return rc;
    scene_carve(ctx, ka, ctx->force_global_scene ? 0 : ctx->max_lds_mode, b.sl);
    if (ctx->brute) return launch_brute(ctx, b, ka);
    if ((rc = scene_accel_args(ctx, ka, b.sl)) || (rc = path_occupancy(ctx, b, ka))) return rc;
    if (b.blocks == 0) return RT_OK;
    if ((rc = select_stream(ctx, b, ka)) || (rc = schedule_state(ctx, b, ka)) ||
        (rc = claim_clock_slot(ctx, b.S, ka)) || (rc = primary_prepass(ctx, b, ka)))
        return rc;
    return launch_path_and_resolve(ctx, b, ka);
}

// Queueing a frame is host bookkeeping only: the device is selected (a HIP call)
// only when the call launches the batch.
int rt_compute_frame(rt_ctx* ctx, uint32_t bounces) {
    if (!ctx || ctx->frame_batch <= 1) return rt_compute_frames(ctx, bounces, 1);
    if (ctx->pending_frames && bounces != ctx->pending_bounces) {
        RT_ENTER_NOFLUSH(ctx);
        const int rc = flush_frames(ctx);
        if (rc) return rc;
    }
    if (ctx->pending_frames == 0) {
        ctx->pending_bounces = bounces;
        if (ctx->params.accumulate) ctx->params.accumulation_index = ctx->k;  // src/renderer.rs:216-235
    }
    if (ctx->params.accumulate) ctx->k += 1;
    ctx->pending_frames += 1;
    if (ctx->pending_frames < ctx->frame_batch) return RT_OK;
    RT_ENTER_NOFLUSH(ctx);
    return flush_frames(ctx);
}

int rt_submit_frames(rt_ctx* ctx, uint32_t bounces, uint32_t count) {
    if (!ctx) return RT_E_INVALID;
    for (uint32_t i = 0; i < count; i++) {
        const int rc = rt_compute_frame(ctx, bounces);
        if (rc) return rc;
    }
    return RT_OK;
}

int rt_set_frame_batch(rt_ctx* ctx, uint32_t max_frames) {
    RT_ENTER(ctx);
    if (max_frames == 0 || max_frames > kMaxFrameBatch)
        return fail(ctx, RT_E_INVALID, "frame batch must be in [1, " + std::to_string(kMaxFrameBatch) + "]");
    ctx->frame_batch = max_frames;
    return RT_OK;
}

int rt_frame_batch(const rt_ctx* ctx, uint32_t* max_frames, uint32_t* pending) {
    if (!ctx || !max_frames || !pending) return RT_E_INVALID;
    *max_frames = ctx->frame_batch;
    *pending = ctx->pending_frames;
    return RT_OK;
}

int rt_flush(rt_ctx* ctx) {
    RT_ENTER(ctx);
    return RT_OK;
}

int rt_compute_frames(rt_ctx* ctx, uint32_t bounces, uint32_t frames) {
    RT_ENTER(ctx);
    if (frames == 0) return fail(ctx, RT_E_INVALID, "frames must be >= 1");
    if (ctx->params.accumulate) {  // src/renderer.rs:216-235 (`accumulate` is a bool there)
        ctx->params.accumulation_index = ctx->k;
        ctx->k += frames;
    }
    return dispatch_frames(ctx, bounces, frames);
}

int rt_synchronize(rt_ctx* ctx) {
    RT_ENTER(ctx);
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// rt_copy_{output,denoised,display}_to_device: the RGBA8 plane `src` into the caller's pitched
// rows, stream-ordered. `missing`: why the entry point has no plane to copy (null: it has one).
static int copy_plane_to_device(rt_ctx* ctx, const char* entry, const uint32_t* src, const char* missing,
                                void* dst_device, uint32_t bytes_per_row) {
    if (dst_device && missing) return fail(ctx, RT_E_INVALID, std::string(entry) + ": " + missing);
    const int rc = check_device_ptrs(ctx, entry, {{dst_device, "dst_device", 1, false}});
    if (rc) return rc;
    if ((uint64_t)bytes_per_row < 4ull * ctx->width)
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": bytes_per_row < 4 * width");
    RT_HIP(ctx, hipMemcpy2DAsync(dst_device, bytes_per_row, src, 4u * (size_t)ctx->width, 4u * (size_t)ctx->width,
                                 ctx->height, hipMemcpyDeviceToDevice, ctx->stream));
    return RT_OK;
}

int rt_copy_output_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row) {
    RT_ENTER(ctx);  // queued frames launched first: the copy sees the last frame's output
    // a rank's output holds only its own tiles: gather first (rt_gather_frame)
    return copy_plane_to_device(ctx, "rt_copy_output_to_device", ctx->d_out,
                                ctx->world > 1 ? "a rank context (world_size > 1) has no full frame" : nullptr,
                                dst_device, bytes_per_row);
}

// ---- ray queries (query.hip) -------------------------------------------------------------------
//
// A query reads the scene and writes the caller's records, nothing else: the queued frames stay
// queued (nothing changed the scene since they were queued -- every update launches them first --
// so they render the same bits before or after the query), and the accumulation, the output, the
// counters, the timing totals and the tile schedule are not touched. The accelerators are
// prepared exactly as a frame launch prepares them (the same refresh and derivation, whichever
// comes first does the work), on the primary stream after everything the auxiliary stream runs.
static int query_enter(rt_ctx* ctx) {
    RT_HIP(ctx, join_aux(ctx));
    if (!ctx->d_query_next) {
        const int rc = dev_alloc(ctx, &ctx->d_query_next, 1);
        if (rc) return rc;
    }
    const rt_params& p = ctx->params;
    int rc = refresh_sphere_slots(ctx, p.sphere_count, p.object_count == 0);
    if (rc) return rc;
    return refresh_tri_accel(ctx, p.object_count);
}

// The scene view of a query of `count` rays: the frame launches' carve, with the placement capped
// by tuning "query_lds_mode", or by default at mode 0 for batches too small to repay staging.
// `kind`: the kernel the view is for -- rt_query_kernel, rt_occlusion_kernel (occlusion.hip) or
// rt_radiance_kernel (radiance.hip), whose `count` is its walks' lower bound, rays x samples, or
// its gather instance (points x samples) or its probe instance (probes x samples), or
// rt_ambient_kernel (ambient.hip; points x samples), or the radiance kernel's lens instance
// (pixels x samples), or rt_hits_kernel (hits.hip).
enum QueryKind {
    kQueryClosest = 0,
    kQueryAnyHit = 1,
    kQueryRadiance = 2,
    kQueryGather = 3,
    kQueryProbe = 4,
    kQueryAmbient = 5,
    kQueryLens = 6,
    kQueryHits = 7
};

// Per kind: the workgroup size of the instance for a placement, and its resident workgroups per CU.
static const struct {
    uint32_t (*threads)(int mode, bool tris);
    hipError_t (*occupancy)(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
} kQueryKernels[8] = {{rt_query_threads, rt_query_occupancy},
                      {rt_occlusion_threads, rt_occlusion_occupancy},
                      {rt_radiance_threads, rt_radiance_occupancy},
                      {rt_radiance_threads, rt_gather_occupancy},
                      {rt_radiance_threads, rt_probe_occupancy},
                      {rt_ambient_threads, rt_ambient_occupancy},
                      {rt_radiance_threads, rt_lens_occupancy},
                      {rt_hits_threads, rt_hits_occupancy}};

struct QueryLaunch {
    KernelArgs ka{};
    SceneLaunch sl;
    size_t lds_bytes = 0;
    uint32_t waves_per_block = 0;
    uint64_t resident = 0;  // workgroups of the instance that the device holds at once
};

static int query_scene(rt_ctx* ctx, uint64_t count, int kind, QueryLaunch& q) {
    KernelArgs& ka = q.ka;
    SceneLaunch& sl = q.sl;
    scene_base_args(ctx, ka);
    ka.camera_rays = ctx->d_rays;
    int max_mode = ctx->force_global_scene ? 0 : ctx->max_lds_mode;
    if (ctx->query_lds_mode >= 0)
        max_mode = ctx->query_lds_mode;
    else if (count < kQueryStageMinRays)
        max_mode = 0;
    for (;; --max_mode) {
        // (the carve reads ka.tri_nodes of the single layout: scene_accel_args may have scaled it)
        ka.tri_nodes = ka.tri_accel ? ctx->tri_nodes : 0u;
        ka.tri_bvh = reinterpret_cast<const float4*>(ctx->d_tri_bvh);
        scene_carve(ctx, ka, max_mode, sl);
        const int rc = scene_accel_args(ctx, ka, sl);
        if (rc) return rc;
        const uint32_t threads = kQueryKernels[kind].threads(sl.mode, sl.tris);
        ka.lds_leafbatch_offset = (uint32_t)al16(sl.lds_bytes);
        q.lds_bytes = sl.coop ? ka.lds_leafbatch_offset + (size_t)(threads / 64u) * kLeafBatchWaveBytes : sl.lds_bytes;
        const rt_ctx::QueryOccKey key{sl.mode, kind, sl.tris ? 1u : 0u, (uint32_t)q.lds_bytes};
        if (ctx->q_occ_blocks == 0 || !same_key(ctx->q_occ_key, key)) {
            int n = 0;
            const hipError_t e = kQueryKernels[kind].occupancy(sl.mode, sl.tris, q.lds_bytes, &n);
            if (e != hipSuccess) (void)hipGetLastError();
            ctx->q_occ_key = key;
            ctx->q_occ_blocks = e == hipSuccess ? n : 0;
        }
        if (ctx->q_occ_blocks > 0) break;
        // an image this instance cannot take: the next lower placement (mode 0 fits every scene)
        if (sl.mode == 0) return fail(ctx, RT_E_HIP, "ray query: the kernel does not fit the device");
        max_mode = sl.mode;
    }
    q.waves_per_block = kQueryKernels[kind].threads(sl.mode, sl.tris) / 64u;
    q.resident = (uint64_t)ctx->q_occ_blocks * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 1);
    return RT_OK;
}

// Traces `count` rays at device pointer `rays` into `hits`, stream-ordered on the primary stream:
// rt_hit records, or with `any_hit` one occlusion byte per rt_occlusion_ray.
static int run_query(rt_ctx* ctx, const void* rays, void* hits, uint64_t count, bool any_hit = false) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    const int rc = query_scene(ctx, count, any_hit ? kQueryAnyHit : kQueryClosest, q);
    if (rc) return rc;
    // the closest-hit kernel takes every chunk from the counter; an any-hit wave owns its first
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident,
                                                     any_hit ? rtq::kNoChunkCap : 0u, rtq::kWalkChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = (any_hit ? rt_launch_occlusion : rt_launch_query)(
        q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, hits, count, ctx->d_query_next, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, any_hit ? "rt_occlusion_kernel launch" : "rt_query_kernel launch", e);
    return RT_OK;
}

// The staging of the host entry points and rt_pick: `n` rays then `n` records, on the device and
// pinned.
static int query_buffers(rt_ctx* ctx, size_t n) {
    if (ctx->query_buf_rays < n) {
        const int rc = grow_buffer(ctx, "query scratch", &ctx->d_query_buf, &ctx->query_buf_bytes, n * (sizeof(rt_query_ray) + sizeof(rt_hit)));
        if (rc) return rc;
        ctx->query_buf_rays = n;
    }
    if (ctx->query_pinned_rays < n) {
        if (ctx->query_pinned) RT_HIP(ctx, hipHostFree(ctx->query_pinned));
        ctx->query_pinned = nullptr;
        ctx->query_pinned_rays = 0;
        RT_HIP(ctx, hipHostMalloc(&ctx->query_pinned, n * (sizeof(rt_query_ray) + sizeof(rt_hit)), hipHostMallocDefault));
        ctx->query_pinned_rays = n;
    }
    return RT_OK;
}

// What the two entry points of a query family differ in from those of the other families; the rest
// of an entry point is staged_query (the host form) or device_query (the device form) around the
// family's run(device in, device out, n, device segment counter or null).
struct QueryFamily {
    const char* host;      // the entry points, as the messages name them
    const char* device;
    const char* in;        // the record arguments, as the messages name them
    const char* out;
    size_t in_bytes;       // per record
    size_t out_bytes;
    uintptr_t out_align;   // of the device form's `out` (its `in` is 16-byte aligned, `segments` 8)
    uint32_t max_samples;  // 0: the family takes no `samples`
    bool segments;         // the family counts ray segments
};
constexpr uint32_t kAnySamples = UINT32_MAX;

// The checks on `samples`, which come first: an entry point refuses them whatever `count` is.
static int check_samples(rt_ctx* ctx, const QueryFamily& f, const char* entry, uint32_t samples) {
    if (f.max_samples == 0) return RT_OK;
    if (samples == 0) return fail(ctx, RT_E_INVALID, std::string(entry) + ": samples is 0");
    if (samples > f.max_samples)
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": samples above " + std::to_string(f.max_samples));
    return RT_OK;
}

// The device form of a family's entry point: `count` records at device pointer `in` answered into
// `out`, stream-ordered on the primary stream; `segments` (device memory too) may be null.
extern "C++" template <class Run>  // (a template inside the extern "C" block of the entry points)
static int device_query(rt_ctx* ctx, const QueryFamily& f, const void* in, void* out, uint64_t count, uint32_t samples,
                        void* segments, Run run) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, f, f.device, samples);
    if (rc || count == 0) return rc;
    rc = check_device_ptrs(ctx, f.device,
                           {{in, f.in, 16, false}, {out, f.out, f.out_align, false}, {segments, "segments", 8, true}});
    if (rc || (rc = query_enter(ctx))) return rc;
    return run(in, out, count, static_cast<unsigned long long*>(segments));
}

// The host form of a family's entry point: the `count` records of `in_bytes` each at host pointer
// `in` go through the pinned and the device scratch in chunks of "query_chunk"; run answers a
// chunk, and `out_bytes` per record come back to `out`. Both scratch buffers hold the inputs at
// their base and the results at capacity x 32 bytes (where the records of a closest-hit chunk go);
// a call whose results exceed 32 bytes per record (rt_probe_sh: 144) sizes both by that many
// records more. In a family that counts segments the context's segment counter is zeroed first and
// read back after the last chunk, into the pinned bytes after a chunk's results, for `segments`
// (which may be null).
extern "C++" template <class Run>
static int staged_query(rt_ctx* ctx, const QueryFamily& f, const void* in, void* out, uint64_t count, uint32_t samples,
                        uint64_t* segments, Run run) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, f, f.host, samples);
    if (rc) return rc;
    if (count == 0) {
        if (segments) *segments = 0;
        return RT_OK;
    }
    if (!in || !out) return fail(ctx, RT_E_INVALID, std::string(f.host) + ": " + f.in + " or " + f.out + " is NULL");
    if ((rc = query_enter(ctx))) return rc;
    if (f.segments && !ctx->d_radiance_segs && (rc = dev_alloc(ctx, &ctx->d_radiance_segs, 1))) return rc;
    const size_t in_bytes = f.in_bytes, out_bytes = f.out_bytes;
    const size_t chunk = (size_t)std::min<uint64_t>(count, ctx->query_chunk);
    if ((rc = query_buffers(ctx, chunk * ((out_bytes + 31u) / 32u)))) return rc;
    unsigned char* d_in = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* d_out = d_in + ctx->query_buf_rays * sizeof(rt_query_ray);
    unsigned char* h_in = static_cast<unsigned char*>(ctx->query_pinned);
    unsigned char* h_out = h_in + ctx->query_pinned_rays * sizeof(rt_query_ray);
    unsigned long long* h_segs = reinterpret_cast<unsigned long long*>(h_out + chunk * out_bytes);
    unsigned long long* d_segs = f.segments ? ctx->d_radiance_segs : nullptr;
    if (d_segs) RT_HIP(ctx, hipMemsetAsync(d_segs, 0, sizeof(unsigned long long), ctx->stream));
    for (uint64_t done = 0; done < count;) {
        const size_t n = (size_t)std::min<uint64_t>(chunk, count - done);
        std::memcpy(h_in, static_cast<const unsigned char*>(in) + done * in_bytes, n * in_bytes);
        RT_HIP(ctx, hipMemcpyAsync(d_in, h_in, n * in_bytes, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = run(d_in, d_out, n, d_segs))) return rc;
        RT_HIP(ctx, hipMemcpyAsync(h_out, d_out, n * out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (d_segs && done + n == count)
            RT_HIP(ctx, hipMemcpyAsync(h_segs, d_segs, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(static_cast<unsigned char*>(out) + done * out_bytes, h_out, n * out_bytes);
        done += n;
    }
    if (d_segs && segments) *segments = *h_segs;
    return RT_OK;
}

// The run of a path family (run_radiance, run_gather, run_probe_sh) with a call's scalars bound.
extern "C++" template <class PathRun>
static auto bind_path_run(PathRun run, rt_ctx* ctx, uint32_t bounces, uint32_t first_sample, uint32_t samples) {
    return [=](const void* in, void* out, uint64_t n, unsigned long long* segs) {
        return run(ctx, in, out, n, bounces, first_sample, samples, segs);
    };
}

constexpr QueryFamily kTraceRays = {"rt_trace_rays", "rt_trace_rays_device", "rays", "hits", sizeof(rt_query_ray),
                                    sizeof(rt_hit), 16, 0, false};

int rt_trace_rays_device(rt_ctx* ctx, const void* rays_device, void* hits_device, uint64_t count) {
    return device_query(ctx, kTraceRays, rays_device, hits_device, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n); });
}

int rt_trace_rays(rt_ctx* ctx, const rt_query_ray* rays, rt_hit* hits, uint64_t count) {
    return staged_query(ctx, kTraceRays, rays, hits, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n); });
}

int rt_pick(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hit) {
    RT_ENTER_NOFLUSH(ctx);
    if (!hit) return fail(ctx, RT_E_INVALID, "rt_pick: hit is NULL");
    if (x >= ctx->width || y >= ctx->height) return fail(ctx, RT_E_INVALID, "rt_pick: pixel outside the framebuffer");
    int rc = query_enter(ctx);
    if (rc) return rc;
    if ((rc = query_buffers(ctx, 1))) return rc;
    unsigned char* d_ray = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* d_hit = d_ray + ctx->query_buf_rays * sizeof(rt_query_ray);
    {
        // the pixel's un-jittered camera ray, as the kernels read or compute it (pixel_ray)
        KernelArgs ka{};
        scene_base_args(ctx, ka);
        ka.camera_rays = ctx->d_rays;
        RT_HIP(ctx, rt_launch_pick_ray(ka, x, y, d_ray, ctx->stream));
    }
    if ((rc = run_query(ctx, d_ray, d_hit, 1))) return rc;
    unsigned char* h_hit = static_cast<unsigned char*>(ctx->query_pinned);
    RT_HIP(ctx, hipMemcpyAsync(h_hit, d_hit, sizeof(rt_hit), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(hit, h_hit, sizeof(rt_hit));
    return RT_OK;
}

// ---- feature buffers and the denoiser (denoise.hip) ---------------------------------------------
//
// The feature planes are a whole-frame ray query: rt_feature_rays_kernel writes a band's un-jittered
// camera rays (rt_pick's ray for every pixel), run_query traces them with the unchanged query
// kernel, rt_feature_resolve_kernel looks up albedo or environment and writes the planes. Like a
// query it reads the scene and writes only its own buffers.
static int build_features(rt_ctx* ctx) {
    if (ctx->feat_epoch == ctx->scene_epoch && ctx->d_feat[0]) return RT_OK;
    int rc = query_enter(ctx);
    if (rc) return rc;
    for (float4*& plane : ctx->d_feat)
        if (!plane && (rc = dev_alloc(ctx, &plane, ctx->n_pixels))) return rc;
    if (!ctx->d_feat_ids && (rc = dev_alloc(ctx, &ctx->d_feat_ids, ctx->n_pixels))) return rc;
    const uint64_t band = std::min<uint64_t>(ctx->n_pixels, ctx->feature_band);
    if ((rc = grow_buffer(ctx, "feature scratch", &ctx->d_feat_scratch, &ctx->feat_scratch_bytes,
                          band * (sizeof(rt_query_ray) + sizeof(rt_hit)))))
        return rc;
    unsigned char* d_rays = static_cast<unsigned char*>(ctx->d_feat_scratch);
    unsigned char* d_hits = d_rays + band * sizeof(rt_query_ray);
    KernelArgs kb{};
    scene_base_args(ctx, kb);
    kb.camera_rays = ctx->d_rays;
    for (uint64_t first = 0; first < ctx->n_pixels; first += band) {  // bands reuse the scratch in stream order
        const uint32_t n = (uint32_t)std::min<uint64_t>(band, ctx->n_pixels - first);
        RT_HIP(ctx, rt_launch_feature_rays(kb, (uint32_t)first, n, d_rays, ctx->stream));
        if ((rc = run_query(ctx, d_rays, d_hits, n))) return rc;
        RT_HIP(ctx, rt_launch_feature_resolve(kb, (uint32_t)first, n, d_rays, d_hits, ctx->d_feat[0], ctx->d_feat[1],
                                              ctx->d_feat_ids, ctx->stream));
    }
    ctx->feat_epoch = ctx->scene_epoch;
    ctx->primary_dirty = true;
    return RT_OK;
}

int rt_compute_features(rt_ctx* ctx) {
    RT_ENTER_NOFLUSH(ctx);  // like a query: the queued frames stay queued
    return build_features(ctx);
}

int rt_read_features(rt_ctx* ctx, float* normal_depth, float* albedo_hit) {
    RT_ENTER_NOFLUSH(ctx);
    const int rc = build_features(ctx);
    if (rc) return rc;
    float* dst[2] = {normal_depth, albedo_hit};
    for (int i = 0; i < 2; i++)
        if (dst[i])
            RT_HIP(ctx, hipMemcpyAsync(dst[i], ctx->d_feat[i], ctx->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_features_device(rt_ctx* ctx, const void** normal_depth, const void** albedo_hit) {
    RT_ENTER_NOFLUSH(ctx);
    if (!normal_depth || !albedo_hit) return fail(ctx, RT_E_INVALID, "rt_features_device: NULL argument");
    const int rc = build_features(ctx);
    if (rc) return rc;
    *normal_depth = ctx->d_feat[0];
    *albedo_hit = ctx->d_feat[1];
    return RT_OK;
}

int rt_read_feature_ids(rt_ctx* ctx, uint32_t* ids) {
    RT_ENTER_NOFLUSH(ctx);
    if (!ids) return fail(ctx, RT_E_INVALID, "rt_read_feature_ids: NULL argument");
    const int rc = build_features(ctx);
    if (rc) return rc;
    RT_HIP(ctx, hipMemcpyAsync(ids, ctx->d_feat_ids, ctx->n_pixels * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_feature_ids_device(rt_ctx* ctx, const void** ids) {
    RT_ENTER_NOFLUSH(ctx);
    if (!ids) return fail(ctx, RT_E_INVALID, "rt_feature_ids_device: NULL argument");
    const int rc = build_features(ctx);
    if (rc) return rc;
    *ids = ctx->d_feat_ids;
    return RT_OK;
}

int rt_denoise_default_params(rt_denoise_params* out) {
    if (!out) return RT_E_INVALID;
    *out = rt_denoise_params{4u, 1.0f, 0.1f, 0.05f};
    return RT_OK;
}

int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params) {
    RT_ENTER(ctx);  // an observation point: the queued frames are launched first
    rt_denoise_params dp;
    (void)rt_denoise_default_params(&dp);
    if (params) dp = *params;
    if (ctx->world > 1)
        return fail(ctx, RT_E_INVALID, "rt_denoise: a rank context (world_size > 1) has no full frame");
    if (ctx->params.accumulate != 1u)
        return fail(ctx, RT_E_INVALID, "rt_denoise: Params.accumulate != 1 never writes the accumulation");
    if (ctx->k - 1u == 0u || (ctx->k - 1u) * ctx->params.compute_per_frame == 0u)  // D would be 0
        return fail(ctx, RT_E_INVALID, "rt_denoise: no frame since the last reset");
    if (dp.iterations > kMaxDenoiseIterations)
        return fail(ctx, RT_E_INVALID, "rt_denoise: iterations must be <= " + std::to_string(kMaxDenoiseIterations));
    for (float sgm : {dp.sigma_color, dp.sigma_albedo, dp.sigma_depth})
        if (!std::isfinite(sgm) || !(sgm > 0.0f))
            return fail(ctx, RT_E_INVALID, "rt_denoise: every sigma must be finite and > 0");
    int rc = build_features(ctx);
    if (rc) return rc;
    for (float4*& plane : ctx->d_dn)
        if (!plane && (rc = dev_alloc(ctx, &plane, ctx->n_pixels))) return rc;
    if (!ctx->d_dn_out && (rc = dev_alloc(ctx, &ctx->d_dn_out, ctx->n_pixels))) return rc;
    // the host-side constants of the contract (denoise.hip), in f32
    const uint32_t n_samples = (ctx->k - 1u) * ctx->params.compute_per_frame;
    const float div = (float)n_samples;
    const float s0 = dp.sigma_color / sqrtf((float)n_samples);
    const float k_a = 1.0f / (dp.sigma_albedo * dp.sigma_albedo);
    RT_HIP(ctx, rt_launch_denoise_init(ctx->d_accum, ctx->d_dn[0], dp.iterations == 0 ? ctx->d_dn_out : nullptr,
                                       ctx->n_pixels, div, ctx->stream));
    float scale = 1.0f;
    for (uint32_t i = 0; i < dp.iterations; i++, scale *= 0.5f) {
        const float s_i = s0 * scale;
        const float k_c = 1.0f / (s_i * s_i);
        const bool last = i + 1 == dp.iterations;
        RT_HIP(ctx, rt_launch_denoise_pass(ctx->d_feat[0], ctx->d_feat[1], ctx->d_dn[i & 1u], ctx->d_dn[(i + 1u) & 1u],
                                           last ? ctx->d_dn_out : nullptr, ctx->width, ctx->height, 1u << i, k_a, k_c,
                                           dp.sigma_depth, ctx->denoise_lds, ctx->stream));
    }
    ctx->dn_result = (int)(dp.iterations & 1u);
    return RT_OK;
}

int rt_read_denoised(rt_ctx* ctx, uint32_t* rgba8_out, float* rgba_f32_out) {
    RT_ENTER_NOFLUSH(ctx);
    if (ctx->dn_result < 0) return fail(ctx, RT_E_INVALID, "rt_read_denoised: no rt_denoise yet");
    if (rgba8_out)
        RT_HIP(ctx, hipMemcpyAsync(rgba8_out, ctx->d_dn_out, ctx->n_pixels * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (rgba_f32_out)
        RT_HIP(ctx, hipMemcpyAsync(rgba_f32_out, ctx->d_dn[ctx->dn_result], ctx->n_pixels * 16, hipMemcpyDeviceToHost,
                                   ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_copy_denoised_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row) {
    RT_ENTER_NOFLUSH(ctx);
    return copy_plane_to_device(ctx, "rt_copy_denoised_to_device", ctx->d_dn_out,
                                ctx->dn_result < 0 ? "no rt_denoise yet" : nullptr, dst_device, bytes_per_row);
}

// ---- temporal reprojection (denoise.hip) --------------------------------------------------------
int rt_temporal_default_params(rt_temporal_params* out) {
    if (!out) return RT_E_INVALID;
    *out = rt_temporal_params{};
    out->max_history = 32u;
    out->sigma_position = 0.02f;
    out->normal_min = 0.9f;
    return RT_OK;
}

// The two motion tables of an rt_denoise_temporal_motion; null for a plain rt_denoise_temporal.
struct MotionTables {
    const rt_motion* objects;
    uint32_t object_count;
    const rt_motion* spheres;
    uint32_t sphere_count;
};

// rt_denoise_temporal and rt_denoise_temporal_motion after RT_ENTER: every argument is checked
// before the first allocation or launch, so a failing call leaves the history as it was.
static int denoise_temporal(rt_ctx* ctx, const std::string& who, const rt_temporal_params* tparams,
                            const rt_denoise_params* params, const MotionTables* mt) {
    rt_denoise_params dp;
    (void)rt_denoise_default_params(&dp);
    if (params) dp = *params;
    if (ctx->world > 1)
        return fail(ctx, RT_E_INVALID, who + "a rank context (world_size > 1) has no full frame");
    if (ctx->params.accumulate != 1u)
        return fail(ctx, RT_E_INVALID, who + "Params.accumulate != 1 never writes the accumulation");
    if (ctx->k - 1u == 0u || (ctx->k - 1u) * ctx->params.compute_per_frame == 0u)  // D would be 0
        return fail(ctx, RT_E_INVALID, who + "no frame since the last reset");
    if (dp.iterations > kMaxDenoiseIterations)
        return fail(ctx, RT_E_INVALID,
                    who + "iterations must be <= " + std::to_string(kMaxDenoiseIterations));
    for (float sgm : {dp.sigma_color, dp.sigma_albedo, dp.sigma_depth})
        if (!std::isfinite(sgm) || !(sgm > 0.0f))
            return fail(ctx, RT_E_INVALID, who + "every sigma must be finite and > 0");
    if (!tparams) return fail(ctx, RT_E_INVALID, who + "rt_temporal_params is NULL (the matrix has no default)");
    const rt_temporal_params tp = *tparams;
    for (float m : tp.world_to_pixel)
        if (!std::isfinite(m)) return fail(ctx, RT_E_INVALID, who + "world_to_pixel is not finite");
    if (tp.max_history < 1u || tp.max_history > 65536u)
        return fail(ctx, RT_E_INVALID, who + "max_history must be in 1..65536");
    if (!std::isfinite(tp.sigma_position) || !(tp.sigma_position > 0.0f))
        return fail(ctx, RT_E_INVALID, who + "sigma_position must be finite and > 0");
    if (!std::isfinite(tp.normal_min) || tp.normal_min < -1.0f || tp.normal_min > 1.0f)
        return fail(ctx, RT_E_INVALID, who + "normal_min must be in [-1, 1]");
    if (mt) {
        for (const auto& [table, count] : {std::pair{mt->objects, mt->object_count}, std::pair{mt->spheres, mt->sphere_count}}) {
            if (count && !table) return fail(ctx, RT_E_INVALID, who + "a motion table is NULL with a count > 0");
            for (uint32_t i = 0; i < count; i++) {
                const rt_motion& r = table[i];
                if (r.flags & ~(RT_MOTION_MOVED | RT_MOTION_DROP))
                    return fail(ctx, RT_E_INVALID, who + "unknown rt_motion flags");
                if (!(r.flags & RT_MOTION_MOVED)) continue;
                bool finite = std::isfinite(r.normal_scale);
                for (float v : r.m) finite = finite && std::isfinite(v);
                if (!finite) return fail(ctx, RT_E_INVALID, who + "a MOVED rt_motion record is not finite");
            }
        }
    }
    int rc = build_features(ctx);
    if (rc) return rc;
    for (float4*& plane : ctx->d_dn)
        if (!plane && (rc = dev_alloc(ctx, &plane, ctx->n_pixels))) return rc;
    if (!ctx->d_dn_out && (rc = dev_alloc(ctx, &ctx->d_dn_out, ctx->n_pixels))) return rc;
    for (rt_ctx::TemporalSlot& slot : ctx->t_slot)
        for (float4*& plane : slot.plane)
            if (!plane && (rc = dev_alloc(ctx, &plane, ctx->n_pixels))) return rc;
    if (mt) {
        for (rt_ctx::TemporalSlot& slot : ctx->t_slot)
            if (!slot.ids && (rc = dev_alloc(ctx, &slot.ids, ctx->n_pixels))) return rc;
        // the records as the caller wrote them (64 B each: three rows of A, then normal_scale, flags),
        // objects first; copied through the pinned staging area, so the caller's arrays are free on return
        const size_t ob = (size_t)mt->object_count * sizeof(rt_motion), sb = (size_t)mt->sphere_count * sizeof(rt_motion);
        if (ob + sb) {
            if ((rc = grow_buffer(ctx, "motion records", &ctx->d_motion, &ctx->motion_bytes, ob + sb))) return rc;
            void* p;
            if ((rc = staging(ctx, ob + sb, &p))) return rc;
            if (ob) std::memcpy(p, mt->objects, ob);
            if (sb) std::memcpy(static_cast<unsigned char*>(p) + ob, mt->spheres, sb);
            if ((rc = staged_copy(ctx, ctx->d_motion, ob + sb))) return rc;
        }
    }
    // the slot rule: within one accumulation generation the history stays the last result of the
    // generation before it, so the past is never counted twice
    int cur = ctx->t_cur, prev = ctx->t_prev;
    if (ctx->t_slot[cur].valid && ctx->t_slot[cur].gen != ctx->accum_gen) {
        prev = cur;
        cur ^= 1;
    } else if (!ctx->t_slot[cur].valid) {
        prev = -1;
    }
    const bool has_prev = prev >= 0 && ctx->t_slot[prev].valid;
    rt_ctx::TemporalSlot& sc = ctx->t_slot[cur];
    const uint32_t n_samples = (ctx->k - 1u) * ctx->params.compute_per_frame;
    KernelArgs kb{};
    scene_base_args(ctx, kb);
    kb.camera_rays = ctx->d_rays;
    const bool zero = dp.iterations == 0;
    TemporalMotion tm{};
    if (mt) {
        const float4* records = static_cast<const float4*>(ctx->d_motion);
        tm.ids = ctx->d_feat_ids;
        tm.prev_i = has_prev && ctx->t_slot[prev].has_ids ? ctx->t_slot[prev].ids : nullptr;
        tm.cur_i = sc.ids;
        tm.objects = records;
        tm.spheres = records ? records + 4u * (size_t)mt->object_count : nullptr;
        tm.object_count = mt->object_count;
        tm.sphere_count = mt->sphere_count;
    }
    RT_HIP(ctx, rt_launch_temporal(kb, ctx->d_accum, ctx->d_feat[0], ctx->d_feat[1],
                                   has_prev ? ctx->t_slot[prev].plane : nullptr, sc.plane,
                                   has_prev ? ctx->t_slot[prev].matrix : nullptr, zero ? ctx->d_dn[0] : nullptr,
                                   zero ? ctx->d_dn_out : nullptr, (float)n_samples, (float)tp.max_history,
                                   tp.sigma_position * tp.sigma_position, tp.normal_min, ctx->stream,
                                   mt ? &tm : nullptr));
    // the current slot is being rewritten from here on: the bookkeeping follows the launch
    std::memcpy(sc.matrix, tp.world_to_pixel, sizeof(sc.matrix));
    sc.gen = ctx->accum_gen;
    sc.valid = true;
    sc.has_ids = mt != nullptr;
    ctx->t_cur = cur;
    ctx->t_prev = has_prev ? prev : -1;
    const float k_a = 1.0f / (dp.sigma_albedo * dp.sigma_albedo);
    float scale = 1.0f;
    for (uint32_t i = 0; i < dp.iterations; i++, scale *= 0.5f) {
        const float s_i = dp.sigma_color * scale;
        const float k_i = 1.0f / (s_i * s_i);
        const bool last = i + 1 == dp.iterations;
        RT_HIP(ctx, rt_launch_denoise_pass(ctx->d_feat[0], ctx->d_feat[1], i == 0 ? sc.plane[0] : ctx->d_dn[(i - 1u) & 1u],
                                           ctx->d_dn[i & 1u], last ? ctx->d_dn_out : nullptr, ctx->width, ctx->height,
                                           1u << i, k_a, k_i, dp.sigma_depth, ctx->denoise_lds, ctx->stream,
                                           sc.plane[2]));
    }
    ctx->dn_result = zero ? 0 : (int)((dp.iterations - 1u) & 1u);
    return RT_OK;
}

int rt_denoise_temporal(rt_ctx* ctx, const rt_temporal_params* tparams, const rt_denoise_params* params) {
    RT_ENTER(ctx);  // an observation point: the queued frames are launched first
    return denoise_temporal(ctx, "rt_denoise_temporal: ", tparams, params, nullptr);
}

int rt_denoise_temporal_motion(rt_ctx* ctx, const rt_temporal_params* tparams, const rt_denoise_params* params,
                               const rt_motion* objects, uint32_t object_count, const rt_motion* spheres,
                               uint32_t sphere_count) {
    RT_ENTER(ctx);  // an observation point, like rt_denoise_temporal
    const MotionTables mt{objects, object_count, spheres, sphere_count};
    return denoise_temporal(ctx, "rt_denoise_temporal_motion: ", tparams, params, &mt);
}

int rt_temporal_reset(rt_ctx* ctx) {
    RT_ENTER_NOFLUSH(ctx);
    for (rt_ctx::TemporalSlot& slot : ctx->t_slot) slot.valid = false;
    ctx->t_prev = -1;
    return RT_OK;
}

int rt_read_temporal(rt_ctx* ctx, float* rgba, float* history) {
    RT_ENTER_NOFLUSH(ctx);
    const rt_ctx::TemporalSlot& slot = ctx->t_slot[ctx->t_cur];
    if (!slot.valid) return fail(ctx, RT_E_INVALID, "rt_read_temporal: no rt_denoise_temporal since the last reset");
    if (rgba) RT_HIP(ctx, hipMemcpyAsync(rgba, slot.plane[0], ctx->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> nn;
    if (history) {
        nn.resize((size_t)ctx->n_pixels * 4);
        RT_HIP(ctx, hipMemcpyAsync(nn.data(), slot.plane[2], ctx->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
    }
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (history)
        for (size_t i = 0; i < (size_t)ctx->n_pixels; i++) history[i] = nn[4 * i + 3];
    return RT_OK;
}

// ---- the display transform (display.hip) ---------------------------------------------------------
//
// Radiance to display codes on the device: meter the source into 256 integer bins, solve and adapt
// the exposure in one wave, tone-map and encode. Three stream-ordered launches and no host wait:
// the exposure lives in d_disp_meter and the tone kernel reads it there. Every argument is checked
// before the first launch, so a failing call leaves the exposure state and the display plane alone.
int rt_display_default_params(rt_display_params* out) {
    if (!out) return RT_E_INVALID;
    *out = rt_display_params{RT_DISPLAY_ACCUMULATION, RT_TONE_REINHARD, RT_ENCODE_SRGB, 1u, 1.0f, 0.18f,
                             1.0f / 64.0f, 64.0f, 1.0f, 4.0f, 100u, 50u};
    return RT_OK;
}

int rt_display(rt_ctx* ctx, const rt_display_params* params, const void* plane_device) {
    RT_ENTER_NOFLUSH(ctx);
    rt_display_params dp;
    (void)rt_display_default_params(&dp);
    if (params) dp = *params;
    auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
    if (ctx->world > 1)
        return fail(ctx, RT_E_INVALID, "rt_display: a rank context (world_size > 1) has no full frame");
    if (dp.source > RT_DISPLAY_PLANE) return fail(ctx, RT_E_INVALID, "rt_display: unknown source");
    if (dp.tone_operator > RT_TONE_ACES) return fail(ctx, RT_E_INVALID, "rt_display: unknown tone operator");
    if (dp.encode > RT_ENCODE_SRGB) return fail(ctx, RT_E_INVALID, "rt_display: unknown encode");
    if (dp.auto_exposure > 1u) return fail(ctx, RT_E_INVALID, "rt_display: auto_exposure must be 0 or 1");
    if (dp.source != RT_DISPLAY_PLANE && plane_device)
        return fail(ctx, RT_E_INVALID, "rt_display: plane_device must be NULL unless the source is RT_DISPLAY_PLANE");
    if (dp.auto_exposure) {
        if (!positive(dp.key) || !positive(dp.min_exposure) || !positive(dp.max_exposure))
            return fail(ctx, RT_E_INVALID, "rt_display: key, min_exposure and max_exposure must be finite and > 0");
        if (dp.min_exposure > dp.max_exposure)
            return fail(ctx, RT_E_INVALID, "rt_display: min_exposure > max_exposure");
        if (!(dp.adaptation > 0.0f && dp.adaptation <= 1.0f))
            return fail(ctx, RT_E_INVALID, "rt_display: adaptation must be in (0, 1]");
        if ((uint64_t)dp.low_permille + dp.high_permille >= 1000u)
            return fail(ctx, RT_E_INVALID, "rt_display: low_permille + high_permille must be < 1000");
    } else if (!positive(dp.exposure)) {
        return fail(ctx, RT_E_INVALID, "rt_display: exposure must be finite and > 0");
    }
    if (dp.tone_operator == RT_TONE_REINHARD && !positive(dp.white))
        return fail(ctx, RT_E_INVALID, "rt_display: white must be finite and > 0");
    const float4* src = nullptr;
    float div = 1.0f;
    if (dp.source == RT_DISPLAY_ACCUMULATION) {
        // an observation point, like rt_denoise: the queued frames are launched first
        const int rcf = flush_frames(ctx);
        if (rcf != RT_OK) return rcf;
        RT_HIP(ctx, join_aux(ctx));
        ctx->primary_dirty = true;
        if (ctx->params.accumulate != 1u)
            return fail(ctx, RT_E_INVALID, "rt_display: Params.accumulate != 1 never writes the accumulation");
        if (ctx->k - 1u == 0u || (ctx->k - 1u) * ctx->params.compute_per_frame == 0u)  // D would be 0
            return fail(ctx, RT_E_INVALID, "rt_display: no frame since the last reset");
        src = ctx->d_accum;
        div = (float)((ctx->k - 1u) * ctx->params.compute_per_frame);
    } else if (dp.source == RT_DISPLAY_DENOISED) {
        if (ctx->dn_result < 0) return fail(ctx, RT_E_INVALID, "rt_display: no rt_denoise or rt_denoise_temporal yet");
        src = ctx->d_dn[ctx->dn_result];
    } else {
        const int rcp = check_device_ptrs(ctx, "rt_display", {{plane_device, "plane_device", 16, false}});
        if (rcp) return rcp;
        src = static_cast<const float4*>(plane_device);
    }
    int rc;
    if (!ctx->d_disp_out && (rc = dev_alloc(ctx, &ctx->d_disp_out, ctx->n_pixels))) return rc;
    if (!ctx->d_disp_meter && (rc = dev_alloc(ctx, &ctx->d_disp_meter, 2u * kDispBins + kDispStateWords))) return rc;
    uint32_t* bins = ctx->d_disp_meter;
    uint32_t* kept = bins + kDispBins;
    uint32_t* state = kept + kDispBins;
    if (dp.auto_exposure) {
        RT_HIP(ctx, rt_launch_display_meter(src, ctx->n_pixels, div, bins, ctx->stream));
        RT_HIP(ctx, rt_launch_display_solve(bins, kept, state, dp.low_permille, dp.high_permille, dp.key, dp.min_exposure,
                                            dp.max_exposure, dp.adaptation, ctx->disp_exposure_valid, ctx->stream));
        ctx->disp_exposure_valid = true;
    }
    const float iw2 = dp.tone_operator == RT_TONE_REINHARD ? 1.0f / (dp.white * dp.white) : 0.0f;
    RT_HIP(ctx, rt_launch_display_tone(src, ctx->d_disp_out, ctx->n_pixels, div, dp.auto_exposure ? state : nullptr,
                                       dp.exposure, iw2, ctx->d_srgb, dp.tone_operator, dp.encode, ctx->stream));
    ctx->disp_valid = true;
    return RT_OK;
}

int rt_read_display(rt_ctx* ctx, uint32_t* rgba8_out) {
    RT_ENTER_NOFLUSH(ctx);
    if (!ctx->disp_valid) return fail(ctx, RT_E_INVALID, "rt_read_display: no rt_display yet");
    if (rgba8_out)
        RT_HIP(ctx, hipMemcpyAsync(rgba8_out, ctx->d_disp_out, ctx->n_pixels * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_copy_display_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row) {
    RT_ENTER_NOFLUSH(ctx);
    return copy_plane_to_device(ctx, "rt_copy_display_to_device", ctx->d_disp_out,
                                ctx->disp_valid ? nullptr : "no rt_display yet", dst_device, bytes_per_row);
}

int rt_display_state(rt_ctx* ctx, float* exposure, uint32_t* histogram, uint64_t* metered) {
    RT_ENTER_NOFLUSH(ctx);
    uint32_t words[kDispBins + kDispStateWords] = {};  // kept bins, then the state; zeros before the first auto call
    if (ctx->d_disp_meter) {
        RT_HIP(ctx, hipMemcpyAsync(words, ctx->d_disp_meter + kDispBins, sizeof(words), hipMemcpyDeviceToHost,
                                   ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (exposure) {
        *exposure = 0.0f;  // no adapted exposure
        if (ctx->disp_exposure_valid) std::memcpy(exposure, &words[kDispBins], sizeof(float));
    }
    if (histogram) std::memcpy(histogram, words, kDispBins * sizeof(uint32_t));
    if (metered) *metered = (uint64_t)words[kDispBins + 2] | ((uint64_t)words[kDispBins + 3] << 32);
    return RT_OK;
}

int rt_display_reset(rt_ctx* ctx) {
    RT_ENTER_NOFLUSH(ctx);
    ctx->disp_exposure_valid = false;
    return RT_OK;
}

// ---- occlusion queries (occlusion.hip) ---------------------------------------------------------
//
// The any-hit counterpart of the calls above, with the same scene visibility and the same absence
// of side effects; rt_occluded stages through the same buffers (32 B in, 1 B out per ray: the
// bytes go where the records of a closest-hit chunk would).
constexpr QueryFamily kOccluded = {"rt_occluded", "rt_occluded_device", "rays", "occluded", sizeof(rt_occlusion_ray),
                                   1, 1, 0, false};

int rt_occluded_device(rt_ctx* ctx, const void* rays_device, void* occluded_device, uint64_t count) {
    return device_query(ctx, kOccluded, rays_device, occluded_device, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n, true); });
}

int rt_occluded(rt_ctx* ctx, const rt_occlusion_ray* rays, uint8_t* occluded, uint64_t count) {
    return staged_query(ctx, kOccluded, rays, occluded, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n, true); });
}

// ---- hit-list queries (hits.hip) ---------------------------------------------------------------
//
// The K nearest hits of each ray, with the scene visibility and the absence of side effects of the
// calls above: `count` rt_occlusion_ray at device pointer `rays` into count x max_hits rt_hit at
// `hits` and, unless null, one count per ray at `counts`. `pick`: the rays are rt_pick's (no t_max).
static int run_hits(rt_ctx* ctx, const void* rays, void* hits, void* counts, uint64_t count, uint32_t max_hits,
                    bool pick = false) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    const int rc = query_scene(ctx, count, kQueryHits, q);
    if (rc) return rc;
    // every chunk from the counter, as the closest-hit kernel takes them
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, 0u, rtq::kWalkChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = rt_launch_hits(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, hits, counts, count, max_hits,
                                        pick, ctx->d_query_next, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_hits_kernel launch", e);
    return RT_OK;
}

// The check on max_hits, which comes first: an entry point refuses it whatever `count` is.
static int check_max_hits(rt_ctx* ctx, const char* entry, uint32_t max_hits) {
    if (max_hits == 0 || max_hits > RT_HITS_MAX)
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": max_hits must be in [1, " + std::to_string(RT_HITS_MAX) + "]");
    return RT_OK;
}

int rt_trace_hits_device(rt_ctx* ctx, const void* rays_device, void* hits_device, void* counts_device, uint64_t count,
                         uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_trace_hits_device", max_hits);
    if (rc || count == 0) return rc;
    rc = check_device_ptrs(ctx, "rt_trace_hits_device",
                           {{rays_device, "rays", 16, false}, {hits_device, "hits", 16, false}, {counts_device, "counts", 4, true}});
    if (rc || (rc = query_enter(ctx))) return rc;
    return run_hits(ctx, rays_device, hits_device, counts_device, count, max_hits);
}

// Staged through the buffers of rt_trace_rays in chunks of max(1, query_chunk / max_hits) rays: a
// chunk's rays at the base, then its records, then its counts.
int rt_trace_hits(rt_ctx* ctx, const rt_occlusion_ray* rays, rt_hit* hits, uint32_t* counts, uint64_t count,
                  uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_trace_hits", max_hits);
    if (rc || count == 0) return rc;
    if (!rays || !hits) return fail(ctx, RT_E_INVALID, "rt_trace_hits: rays or hits is NULL");
    if ((rc = query_enter(ctx))) return rc;
    const size_t chunk = (size_t)std::min<uint64_t>(count, std::max<uint32_t>(1u, ctx->query_chunk / max_hits));
    const size_t ray_bytes = sizeof(rt_occlusion_ray), list_bytes = (size_t)max_hits * sizeof(rt_hit);
    // (a scratch "ray" is 96 bytes: chunk x max_hits of them hold the records, chunk more the rays and counts)
    if ((rc = query_buffers(ctx, chunk * max_hits + chunk))) return rc;
    unsigned char* d_in = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* h_in = static_cast<unsigned char*>(ctx->query_pinned);
    const size_t hits_at = chunk * ray_bytes, counts_at = hits_at + chunk * list_bytes;
    for (uint64_t done = 0; done < count;) {
        const size_t n = (size_t)std::min<uint64_t>(chunk, count - done);
        std::memcpy(h_in, rays + done, n * ray_bytes);
        RT_HIP(ctx, hipMemcpyAsync(d_in, h_in, n * ray_bytes, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = run_hits(ctx, d_in, d_in + hits_at, d_in + counts_at, n, max_hits))) return rc;
        RT_HIP(ctx, hipMemcpyAsync(h_in + hits_at, d_in + hits_at, n * list_bytes, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipMemcpyAsync(h_in + counts_at, d_in + counts_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(hits + done * max_hits, h_in + hits_at, n * list_bytes);
        if (counts) std::memcpy(counts + done, h_in + counts_at, n * sizeof(uint32_t));
        done += n;
    }
    return RT_OK;
}

int rt_pick_hits(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hits, uint32_t* n, uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_pick_hits", max_hits);
    if (rc) return rc;
    if (!hits || !n) return fail(ctx, RT_E_INVALID, "rt_pick_hits: hits or n is NULL");
    if (x >= ctx->width || y >= ctx->height)
        return fail(ctx, RT_E_INVALID, "rt_pick_hits: pixel outside the framebuffer");
    if ((rc = query_enter(ctx)) || (rc = query_buffers(ctx, (size_t)max_hits + 1u))) return rc;
    unsigned char* d_ray = static_cast<unsigned char*>(ctx->d_query_buf);
    const size_t hits_at = sizeof(rt_query_ray), list_bytes = (size_t)max_hits * sizeof(rt_hit);
    {
        // rt_pick's ray (its record carries no t_max: the kernel takes +inf)
        KernelArgs ka{};
        scene_base_args(ctx, ka);
        ka.camera_rays = ctx->d_rays;
        RT_HIP(ctx, rt_launch_pick_ray(ka, x, y, d_ray, ctx->stream));
    }
    if ((rc = run_hits(ctx, d_ray, d_ray + hits_at, d_ray + hits_at + list_bytes, 1, max_hits, true))) return rc;
    unsigned char* h_out = static_cast<unsigned char*>(ctx->query_pinned);
    RT_HIP(ctx, hipMemcpyAsync(h_out, d_ray + hits_at, list_bytes + sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(hits, h_out, list_bytes);
    std::memcpy(n, h_out + list_bytes, sizeof(uint32_t));
    return RT_OK;
}

// ---- radiance queries (radiance.hip) -----------------------------------------------------------
//
// per_pixel for arbitrary rays, with the scene visibility and the absence of side effects of the
// calls above. rt_radiance stages through the same buffers (32 B in, 16 B out per ray: the sums go
// where the records of a closest-hit chunk would).

// The answer of a path query of zero bounces, `out_bytes` per record: the bounce loop does not run
// (:226), so there is no light and there are no segments.
static int answer_zero_bounces(rt_ctx* ctx, void* out, uint64_t count, size_t out_bytes) {
    RT_HIP(ctx, hipMemsetAsync(out, 0, (size_t)count * out_bytes, ctx->stream));
    return RT_OK;
}

// The walks of `count` records of `samples` each, for the placement threshold of the other queries.
static uint64_t query_walks(uint64_t count, uint32_t samples) {
    return count > UINT64_MAX / samples ? UINT64_MAX : count * samples;
}

// The head of a radiance, gather or probe launch (`kind`) of `count` records, `bounces` > 0: `q`
// receives the scene view, placed by the walks the call runs at least, and the shading arguments.
static int path_query_scene(rt_ctx* ctx, uint64_t count, uint32_t bounces, uint32_t samples, int kind, QueryLaunch& q) {
    const int rc = query_scene(ctx, query_walks(count, samples), kind, q);
    if (rc) return rc;
    q.ka.bounces = bounces;
    q.ka.drain_threshold = ctx->drain_threshold;
    q.ka.drain_min_steps = ctx->drain_min_steps;
    return RT_OK;
}

// Path-traces `count` rays at device pointer `rays` into `radiance`, stream-ordered on the primary
// stream; the batch's counted segments are added to the device counter `segments` (null: not
// counted).
static int run_radiance(rt_ctx* ctx, const void* rays, void* radiance, uint64_t count, uint32_t bounces,
                        uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryRadiance, q);
    if (rc) return rc;
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, rtq::kRadianceFirstChunkMax,
                                                     rtq::kRadianceChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = rt_launch_radiance(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, radiance, count,
                                            ctx->d_query_next, segments, first_sample, samples, 0u, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_radiance_kernel launch", e);
    return RT_OK;
}

constexpr QueryFamily kRadiance = {"rt_radiance", "rt_radiance_device", "rays", "radiance", sizeof(rt_radiance_ray),
                                   16, 16, kAnySamples, true};

int rt_radiance_device(rt_ctx* ctx, const void* rays_device, void* radiance_device, uint64_t count, uint32_t bounces,
                       uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kRadiance, rays_device, radiance_device, count, samples, segments_device,
                        bind_path_run(run_radiance, ctx, bounces, first_sample, samples));
}

int rt_radiance(rt_ctx* ctx, const rt_radiance_ray* rays, float* radiance, uint64_t count, uint32_t bounces,
                uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kRadiance, rays, radiance, count, samples, segments,
                        bind_path_run(run_radiance, ctx, bounces, first_sample, samples));
}

// ---- gather queries (radiance.hip, kGather) -----------------------------------------------------
//
// Per point, the tree-reduced light of `samples` paths through the diffuse lobe (the contract in
// include/rt_abi.h). The path kernel is the radiance kernel's gather instance over (point, stripe)
// items; rt_gather_resolve_kernel reduces each point's partials.

// The launches of a gather or an ambient call, which differ in their kernel: `count` points (32-byte
// records) at device pointer `points` in launches of at most "gather_chunk" points, each
// launch(schedule, its points, items, stripes) over (point, stripe) items into the context's
// partials, which rt_gather_resolve_kernel reduces into `out`. `what` names the launch in an error.
extern "C++" template <class Launch>
static int run_striped(rt_ctx* ctx, const QueryLaunch& q, const void* points, void* out, uint64_t count,
                       uint32_t samples, const char* what, Launch launch) {
    const uint32_t stripes = std::min<uint32_t>(samples, 64u);
    const uint64_t chunk = std::min<uint64_t>(count, ctx->gather_chunk);
    const int rc = grow_buffer(ctx, "gather partials", &ctx->d_gather_partials, &ctx->gather_partials_bytes, (size_t)chunk * 1024u);
    if (rc) return rc;
    for (uint64_t done = 0; done < count;) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, count - done);
        // the launch is sized by its items, (point, stripe) pairs: at most 2^20 x 64
        const uint64_t items = (uint64_t)n * stripes;
        const rtq::QuerySchedule s = rtq::query_schedule(items, q.waves_per_block, q.resident,
                                                         rtq::kRadianceFirstChunkMax, rtq::kRadianceChunkMax);
        RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
        hipError_t e = launch(s, static_cast<const unsigned char*>(points) + done * sizeof(rt_gather_point), items, stripes);
        if (e != hipSuccess) return hip_fail(ctx, what, e);
        e = rt_launch_gather_resolve(ctx->d_gather_partials, static_cast<unsigned char*>(out) + done * 16u, n, stripes,
                                     ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, "rt_gather_resolve_kernel launch", e);
        done += n;
    }
    return RT_OK;
}

// Gathers at `count` points at device pointer `points` into `radiance`, stream-ordered on the
// primary stream, in launches of at most "gather_chunk" points; the counted segments are added to
// the device counter `segments` (null: not counted).
static int run_gather(rt_ctx* ctx, const void* points, void* radiance, uint64_t count, uint32_t bounces,
                      uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryGather, q);
    if (rc) return rc;
    return run_striped(ctx, q, points, radiance, count, samples, "rt_radiance_kernel (gather) launch",
                       [&](const rtq::QuerySchedule& s, const void* records, uint64_t items, uint32_t stripes) {
                           return rt_launch_radiance(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records,
                                                     ctx->d_gather_partials, items, ctx->d_query_next, segments,
                                                     first_sample, samples, stripes, ctx->stream);
                       });
}

constexpr QueryFamily kGather = {"rt_gather", "rt_gather_device", "points", "radiance", sizeof(rt_gather_point),
                                 16, 16, kAnySamples, true};

int rt_gather_device(rt_ctx* ctx, const void* points_device, void* radiance_device, uint64_t count, uint32_t bounces,
                     uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kGather, points_device, radiance_device, count, samples, segments_device,
                        bind_path_run(run_gather, ctx, bounces, first_sample, samples));
}

int rt_gather(rt_ctx* ctx, const rt_gather_point* points, float* radiance, uint64_t count, uint32_t bounces,
              uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kGather, points, radiance, count, samples, segments,
                        bind_path_run(run_gather, ctx, bounces, first_sample, samples));
}

// ---- ambient queries (ambient.hip) ---------------------------------------------------------------
//
// Per point, the open count and the sum of the open directions among `samples` any-hit searches
// through the gather's lobe (the contract in include/rt_abi.h), with the scene visibility and the
// absence of side effects of rt_occluded. rt_ambient_kernel runs (point, stripe) items into the
// gather's partials; rt_gather_resolve_kernel reduces each point's partials.

// The most samples per point: `open` stays an exactly represented integer (2^24).
constexpr uint32_t kMaxAmbientSamples = 1u << 24;

// Answers `count` points at device pointer `points` into `out`, stream-ordered on the primary
// stream, in launches of at most "gather_chunk" points.
static int run_ambient(rt_ctx* ctx, const void* points, void* out, uint64_t count, uint32_t first_sample,
                       uint32_t samples) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    // the placement threshold of the other queries, on the walks the call runs at most
    const int rc = query_scene(ctx, query_walks(count, samples), kQueryAmbient, q);
    if (rc) return rc;
    return run_striped(ctx, q, points, out, count, samples, "rt_ambient_kernel launch",
                       [&](const rtq::QuerySchedule& s, const void* records, uint64_t items, uint32_t stripes) {
                           return rt_launch_ambient(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records,
                                                    ctx->d_gather_partials, items, ctx->d_query_next, first_sample,
                                                    samples, stripes, ctx->stream);
                       });
}

constexpr QueryFamily kAmbient = {"rt_ambient", "rt_ambient_device", "points", "out", sizeof(rt_ambient_point),
                                  16, 16, kMaxAmbientSamples, false};

int rt_ambient_device(rt_ctx* ctx, const void* points_device, void* out_device, uint64_t count, uint32_t first_sample,
                      uint32_t samples) {
    return device_query(ctx, kAmbient, points_device, out_device, count, samples, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) {
                            return run_ambient(ctx, in, out, n, first_sample, samples);
                        });
}

int rt_ambient(rt_ctx* ctx, const rt_ambient_point* points, float* out, uint64_t count, uint32_t first_sample,
               uint32_t samples) {
    return staged_query(ctx, kAmbient, points, out, count, samples, nullptr,
                        [=](const void* d_in, void* d_out, uint64_t n, unsigned long long*) {
                            return run_ambient(ctx, d_in, d_out, n, first_sample, samples);
                        });
}

// ---- probe queries (radiance.hip, kPathProbe) ---------------------------------------------------
//
// Per probe, the second-order spherical-harmonic projection of the light of `samples` paths that
// leave the point in uniform directions (the contract in include/rt_abi.h). The path kernel is the
// radiance kernel's probe instance over (probe, sample) items, which stores every path's light;
// rt_probe_resolve_kernel projects and reduces each probe's lights.

// Bakes `count` probes at device pointer `probes` into `sh`, stream-ordered on the primary stream,
// in launches of whole probes, max(1, "probe_chunk" / samples) of them, two of them in flight (the
// primary stream is ordered after both on return); the counted segments are added to the device
// counter `segments` (null: not counted).
static int run_probe_sh(rt_ctx* ctx, const void* probes, void* sh, uint64_t count, uint32_t bounces,
                        uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, sh, count, 144u);
    QueryLaunch q;
    int rc = path_query_scene(ctx, count, bounces, samples, kQueryProbe, q);
    if (rc) return rc;
    // whole probes per launch: at most max("probe_chunk", samples) <= 2^26 items, 16 B each
    const uint64_t chunk = std::min<uint64_t>(count, std::max<uint32_t>(1u, ctx->probe_chunk / samples));
    const size_t bytes = (size_t)chunk * samples * 16u;
    // A call of several launches alternates them between the primary and the auxiliary stream, each
    // with its own half of the scratch and its own chunk counter: a launch of a million paths is
    // mostly fill and drain (four items per resident lane), and the next launch's workgroups take
    // the CUs the draining one gives up. Not where that would take the scratch beyond its cap.
    const bool overlap = count > chunk && 2u * bytes <= kMaxProbeScratchBytes;
    if ((rc = grow_buffer(ctx, "probe lights", &ctx->d_probe_lights, &ctx->probe_lights_bytes, overlap ? 2u * bytes : bytes))) return rc;
    if (overlap) {
        if (!ctx->d_probe_next && (rc = dev_alloc(ctx, &ctx->d_probe_next, 2))) return rc;
        RT_HIP(ctx, hipEventRecord(ctx->ev_primary, ctx->stream));  // the probes are there, the scratch is free
        RT_HIP(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_primary, 0));
    }
    // orders the primary stream after the auxiliary one again (on every way out)
    auto join = [&]() -> hipError_t {
        if (!overlap) return hipSuccess;
        const hipError_t e = hipEventRecord(ctx->ev_aux_done, ctx->aux_stream);
        if (e != hipSuccess) return e;
        ctx->aux_outstanding = true;
        return join_aux(ctx);
    };
    uint32_t group = 0;
    for (uint64_t done = 0; done < count; ++group) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, count - done);
        const uint64_t items = (uint64_t)n * samples;
        const rtq::QuerySchedule s = rtq::query_schedule(items, q.waves_per_block, q.resident,
                                                         rtq::kRadianceFirstChunkMax, rtq::kRadianceChunkMax);
        const uint32_t slot = overlap ? group & 1u : 0u;
        hipStream_t S = slot ? ctx->aux_stream : ctx->stream;
        unsigned long long* next = overlap ? ctx->d_probe_next + slot : ctx->d_query_next;
        unsigned char* lights = static_cast<unsigned char*>(ctx->d_probe_lights) + slot * bytes;
        const unsigned char* records = static_cast<const unsigned char*>(probes) + done * sizeof(rt_probe);
        hipError_t e = hipMemsetAsync(next, 0, sizeof(unsigned long long), S);
        if (e == hipSuccess)
            e = rt_launch_probe_paths(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records, lights, items, next, segments,
                                      first_sample, samples, S);
        if (e == hipSuccess)
            e = rt_launch_probe_resolve(lights, records, static_cast<unsigned char*>(sh) + done * 144u, n, first_sample,
                                        samples, S);
        if (e != hipSuccess) {
            (void)join();
            return hip_fail(ctx, "rt_probe_sh launch", e);
        }
        done += n;
    }
    RT_HIP(ctx, join());
    return RT_OK;
}

constexpr QueryFamily kProbeSh = {"rt_probe_sh", "rt_probe_sh_device", "probes", "sh", sizeof(rt_probe),
                                  144, 16, kMaxProbeSamples, true};

int rt_probe_sh_device(rt_ctx* ctx, const void* probes_device, void* sh_device, uint64_t count, uint32_t bounces,
                       uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kProbeSh, probes_device, sh_device, count, samples, segments_device,
                        bind_path_run(run_probe_sh, ctx, bounces, first_sample, samples));
}

int rt_probe_sh(rt_ctx* ctx, const rt_probe* probes, float* sh, uint64_t count, uint32_t bounces, uint32_t first_sample,
                uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kProbeSh, probes, sh, count, samples, segments,
                        bind_path_run(run_probe_sh, ctx, bounces, first_sample, samples));
}

// ---- lens queries (radiance.hip, kPathLens) -----------------------------------------------------
//
// Per pixel of a range of the descriptor's image, the summed light of `samples` paths whose first
// ray is drawn on the device from the descriptor (the contract in include/rt_abi.h). The path
// kernel is the radiance kernel's lens instance over the range's pixels; rt_lens_rays_kernel writes
// the same rays as records. The launches read the descriptor from the context's copy
// (d_lens_cam), which rt_lens_store_kernel writes on the primary stream from a kernel argument:
// every lens launch runs on that stream too, so the copy changes only after the launches that read
// the earlier one and before those that follow, whatever the host does in between. (The chunks of
// a host form share the copy of their call; the auxiliary stream runs no lens launch.)

constexpr QueryFamily kLens = {"rt_lens", "rt_lens_device", "cam", "radiance", 0, 16, 16, kAnySamples, true};
constexpr QueryFamily kLensRays = {"rt_lens_rays", "rt_lens_rays_device", "cam", "rays", 0, 32, 16, 0, false};

// Consequence 6 of the lens contract, for the range [first_pixel, first_pixel + count), count > 0.
static int check_lens(rt_ctx* ctx, const char* entry, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count) {
    auto bad = [&](const char* why) { return fail(ctx, RT_E_INVALID, std::string(entry) + ": " + why); };
    if (!cam) return bad("cam is NULL");
    if (cam->kind > RT_LENS_EQUIRECT) return bad("unknown kind");
    if (cam->width == 0 || cam->height == 0) return bad("width or height is 0");
    const uint64_t pixels = (uint64_t)cam->width * cam->height;  // (below 2^64)
    if (pixels > (1ull << 32)) return bad("width * height above 2^32");
    if (first_pixel > pixels || count > pixels - first_pixel) return bad("the range lies outside the image");
    if (!(cam->aperture >= 0.0f) || std::isinf(cam->aperture)) return bad("aperture is negative or not finite");
    if (cam->kind == RT_LENS_PERSPECTIVE && cam->aperture > 0.0f && !(cam->focus > 0.0f))
        return bad("focus must be > 0 when aperture > 0");
    if (cam->kind == RT_LENS_ORTHOGRAPHIC && !(cam->ortho_half_height > 0.0f)) return bad("ortho_half_height must be > 0");
    return RT_OK;
}

// The context's copy of `cam` for the launches that follow on the primary stream.
static int stage_lens_camera(rt_ctx* ctx, const rt_lens_camera* cam) {
    if (!ctx->d_lens_cam) {
        const int rc = dev_alloc(ctx, &ctx->d_lens_cam, sizeof(rt_lens_camera) / sizeof(uint4));
        if (rc) return rc;
    }
    const hipError_t e = rt_launch_lens_camera(*cam, ctx->d_lens_cam, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_lens_store_kernel launch", e);
    return RT_OK;
}

// Path-traces the `count` pixels from `first_pixel` on of the staged descriptor's image into
// `radiance`, stream-ordered on the primary stream; the counted segments are added to the device
// counter `segments` (null: not counted).
static int run_lens(rt_ctx* ctx, uint64_t first_pixel, void* radiance, uint64_t count, uint32_t bounces,
                    uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryLens, q);
    if (rc) return rc;
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, rtq::kRadianceFirstChunkMax,
                                                     rtq::kRadianceChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    // (first_pixel < width * height <= 2^32 with count > 0: check_lens)
    const hipError_t e = rt_launch_lens(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, ctx->d_lens_cam, radiance,
                                        (uint32_t)first_pixel, count, ctx->d_query_next, segments, first_sample,
                                        samples, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_radiance_kernel (lens) launch", e);
    return RT_OK;
}

// The host form of a lens entry point, which has no input records: the range runs in chunks of
// "query_chunk" pixels, run(first pixel, device out, n, device segment counter or null) answers a
// chunk into the device scratch where the results of a closest-hit chunk go, and `out_bytes` per
// pixel come back to `out` through the pinned buffer. The segment counter as in staged_query.
extern "C++" template <class Run>
static int staged_pixels(rt_ctx* ctx, const QueryFamily& f, uint64_t first_pixel, void* out, uint64_t count,
                         uint64_t* segments, Run run) {
    int rc;
    if (f.segments && !ctx->d_radiance_segs && (rc = dev_alloc(ctx, &ctx->d_radiance_segs, 1))) return rc;
    const size_t out_bytes = f.out_bytes;
    const size_t chunk = (size_t)std::min<uint64_t>(count, ctx->query_chunk);
    if ((rc = query_buffers(ctx, chunk))) return rc;
    unsigned char* d_out = static_cast<unsigned char*>(ctx->d_query_buf) + ctx->query_buf_rays * sizeof(rt_query_ray);
    unsigned char* h_out = static_cast<unsigned char*>(ctx->query_pinned) + ctx->query_pinned_rays * sizeof(rt_query_ray);
    unsigned long long* h_segs = reinterpret_cast<unsigned long long*>(h_out + chunk * out_bytes);
    unsigned long long* d_segs = f.segments ? ctx->d_radiance_segs : nullptr;
    if (d_segs) RT_HIP(ctx, hipMemsetAsync(d_segs, 0, sizeof(unsigned long long), ctx->stream));
    for (uint64_t done = 0; done < count;) {
        const size_t n = (size_t)std::min<uint64_t>(chunk, count - done);
        if ((rc = run(first_pixel + done, d_out, n, d_segs))) return rc;
        RT_HIP(ctx, hipMemcpyAsync(h_out, d_out, n * out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (d_segs && done + n == count)
            RT_HIP(ctx, hipMemcpyAsync(h_segs, d_segs, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(static_cast<unsigned char*>(out) + done * out_bytes, h_out, n * out_bytes);
        done += n;
    }
    if (d_segs && segments) *segments = *h_segs;
    return RT_OK;
}

int rt_lens_device(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, void* radiance_device,
                   uint32_t bounces, uint32_t first_sample, uint32_t samples, void* segments_device) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, kLens, kLens.device, samples);
    if (rc || count == 0) return rc;
    if ((rc = check_lens(ctx, kLens.device, cam, first_pixel, count))) return rc;
    rc = check_device_ptrs(ctx, kLens.device, {{radiance_device, kLens.out, 16, false}, {segments_device, "segments", 8, true}});
    if (rc || (rc = query_enter(ctx)) || (rc = stage_lens_camera(ctx, cam))) return rc;
    return run_lens(ctx, first_pixel, radiance_device, count, bounces, first_sample, samples,
                    static_cast<unsigned long long*>(segments_device));
}

int rt_lens(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, float* radiance,
            uint32_t bounces, uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, kLens, kLens.host, samples);
    if (rc) return rc;
    if (count == 0) {
        if (segments) *segments = 0;
        return RT_OK;
    }
    if ((rc = check_lens(ctx, kLens.host, cam, first_pixel, count))) return rc;
    if (!radiance) return fail(ctx, RT_E_INVALID, "rt_lens: radiance is NULL");
    if ((rc = query_enter(ctx)) || (rc = stage_lens_camera(ctx, cam))) return rc;
    return staged_pixels(ctx, kLens, first_pixel, radiance, count, segments,
                         [=](uint64_t first, void* out, uint64_t n, unsigned long long* segs) {
                             return run_lens(ctx, first, out, n, bounces, first_sample, samples, segs);
                         });
}

// The records of the range's rays (steps A to D for the sample index u): no scene, nothing but the
// descriptor is read.
static int run_lens_rays(rt_ctx* ctx, uint64_t first_pixel, void* rays, uint64_t count, uint32_t u) {
    const hipError_t e = rt_launch_lens_rays(ctx->d_lens_cam, rays, (uint32_t)first_pixel, count, u, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_lens_rays_kernel launch", e);
    return RT_OK;
}

int rt_lens_rays_device(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count,
                        uint32_t sample_index, void* rays_device) {
    RT_ENTER_NOFLUSH(ctx);
    if (count == 0) return RT_OK;
    int rc = check_lens(ctx, kLensRays.device, cam, first_pixel, count);
    if (rc) return rc;
    rc = check_device_ptrs(ctx, kLensRays.device, {{rays_device, kLensRays.out, 16, false}});
    if (rc || (rc = stage_lens_camera(ctx, cam))) return rc;
    return run_lens_rays(ctx, first_pixel, rays_device, count, sample_index);
}

int rt_lens_rays(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, uint32_t sample_index,
                 rt_radiance_ray* rays) {
    RT_ENTER_NOFLUSH(ctx);
    if (count == 0) return RT_OK;
    int rc = check_lens(ctx, kLensRays.host, cam, first_pixel, count);
    if (rc) return rc;
    if (!rays) return fail(ctx, RT_E_INVALID, "rt_lens_rays: rays is NULL");
    if ((rc = stage_lens_camera(ctx, cam))) return rc;
    return staged_pixels(ctx, kLensRays, first_pixel, rays, count, nullptr,
                         [=](uint64_t first, void* out, uint64_t n, unsigned long long*) {
                             return run_lens_rays(ctx, first, out, n, sample_index);
                         });
}

int rt_read_output(rt_ctx* ctx, uint32_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_out, ctx->n_pixels * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_output_pitched(rt_ctx* ctx, uint8_t* dst, uint32_t bytes_per_row) {
    RT_ENTER(ctx);
    if (!dst) return fail(ctx, RT_E_INVALID, "dst is NULL");
    if ((uint64_t)bytes_per_row < 4ull * ctx->width) return fail(ctx, RT_E_INVALID, "bytes_per_row < 4 * width");
    RT_HIP(ctx, hipMemcpy2DAsync(dst, bytes_per_row, ctx->d_out, 4ull * ctx->width, 4ull * ctx->width, ctx->height,
                                 hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

uint32_t rt_bytes_per_row(uint32_t width, uint32_t alignment) {
    if (alignment == 0 || (alignment & (alignment - 1)) != 0) return 0;
    const uint64_t v = 4ull * width;
    const uint64_t r = (v + alignment - 1) & ~(uint64_t)(alignment - 1);
    return r > 0xffffffffull ? 0u : (uint32_t)r;
}

// ---- device-side edit path (scene_edit.hip) --------------------------------

int rt_set_object_models(rt_ctx* ctx, const float* points, uint32_t triangle_count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (triangle_count && !points) return fail(ctx, RT_E_INVALID, "normalized_points is NULL");
    if (triangle_count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    int rc = sync_host_geometry(ctx);
    if (rc) return rc;
    // triangle -> object and sub-object -> object maps, per-object triangle ranges
    const uint32_t n_obj = (uint32_t)ctx->h_obj.size(), n_sub = (uint32_t)ctx->h_sub.size();
    std::vector<uint32_t> tri_obj(std::max<uint32_t>(triangle_count, 1), 0xffffffffu);
    std::vector<uint32_t> sub_obj(std::max<uint32_t>(n_sub, 1), 0xffffffffu);
    std::vector<uint2> obj_tris(std::max<uint32_t>(n_obj, 1), make_uint2(0, 0));
    for (uint32_t o = 0; o < n_obj; o++) {
        const rt_object_info& ob = ctx->h_obj[o];
        uint32_t first = 0, count = 0;
        for (uint32_t i = 0; i < ob.sub_object_count; i++) {
            const uint32_t si = ob.first_sub_object_index + i;
            const rt_sub_object_info& so = ctx->h_sub[si];
            if (count == 0) first = so.first_triangle_index;
            if (so.triangle_count && so.first_triangle_index != first + count)
                return fail(ctx, RT_E_INVALID, "object " + std::to_string(o) + ": sub-object triangles not contiguous");
            if ((uint64_t)so.first_triangle_index + so.triangle_count > triangle_count)
                return fail(ctx, RT_E_INVALID, "object " + std::to_string(o) + " has triangles without model points");
            sub_obj[si] = o;
            for (uint32_t t = 0; t < so.triangle_count; t++) tri_obj[so.first_triangle_index + t] = o;
            count += so.triangle_count;
        }
        obj_tris[o] = make_uint2(first, count);
    }
    auto alloc = [&](auto** p, size_t count) -> int {
        if (*p) return RT_OK;
        return dev_alloc(ctx, p, count);
    };
    if ((rc = alloc(&ctx->d_model, 9 * (size_t)ctx->n_tri_dev)) || (rc = alloc(&ctx->d_tri_object, ctx->n_tri_dev)) ||
        (rc = alloc(&ctx->d_sub_object, ctx->n_sub_dev)) || (rc = alloc(&ctx->d_object_tris, std::max(ctx->cap_obj, 1u))) ||
        (rc = alloc(&ctx->d_place, std::max(ctx->cap_obj, 1u))) ||
        (rc = upload_raw(ctx, ctx->d_model, points, (size_t)triangle_count * 36)) ||
        (rc = upload_raw(ctx, ctx->d_tri_object, tri_obj.data(), (size_t)triangle_count * 4)) ||
        (rc = upload_raw(ctx, ctx->d_sub_object, sub_obj.data(), (size_t)n_sub * 4)) ||
        (rc = upload_raw(ctx, ctx->d_object_tris, obj_tris.data(), (size_t)n_obj * 8)))
        return rc;
    ctx->model_tris = triangle_count;
    ctx->models_valid = true;
    return RT_OK;
}

int rt_update_objects(rt_ctx* ctx, const rt_object_transform* transforms, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !transforms) return fail(ctx, RT_E_INVALID, "transforms is NULL");
    if (count > ctx->h_obj.size()) return fail(ctx, RT_E_CAPACITY, "more transforms than objects");
    if (count == 0) return RT_OK;
    if (!ctx->d_model || !ctx->models_valid)
        return fail(ctx, RT_E_INVALID,
                    "object models missing or stale (object / sub-object ranges changed): call rt_set_object_models");
    void* p;
    int rc = staging(ctx, (size_t)count * sizeof(rt_scene::Placement), &p);
    if (rc) return rc;
    rt_scene::Placement* pl = static_cast<rt_scene::Placement*>(p);
    for (uint32_t o = 0; o < count; o++)
        rt_scene::placement(*reinterpret_cast<const rt_scene::ObjectTransform*>(&transforms[o]), pl[o]);
    if ((rc = staged_copy(ctx, ctx->d_place, (size_t)count * sizeof(rt_scene::Placement)))) return rc;
    RT_HIP(ctx, rt_launch_edit(ctx->d_model, ctx->d_tri_object, ctx->d_sub_object, ctx->d_object_tris, ctx->d_place,
                               count, ctx->model_tris, (uint32_t)ctx->h_sub.size(), ctx->d_tri, ctx->d_tri_bounds,
                               ctx->d_sub, ctx->d_obj, ctx->stream));
    ctx->geom_on_device = true;
    // the accelerator keeps its topology; its boxes (and the margin extent) follow the new bounds
    if (ctx->d_tri_bvh && ctx->tri_nodes && !ctx->tri_dirty) {
        RT_HIP(ctx, rt_launch_refit(ctx->d_tri_bvh, ctx->d_tri_prims, ctx->d_sub, ctx->d_tri_order,
                                    ctx->d_tri_level_off, ctx->tri_levels, ctx->d_tri_extent, ctx->stream));
        ctx->qnodes_dirty = true;
    }
    ctx->cones_dirty = true;  // the triangles changed
    ctx->ltris_dirty = true;
    return RT_OK;
}

int rt_read_triangles(rt_ctx* ctx, rt_scene_triangle* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    if (count == 0) return RT_OK;
    std::vector<RtTriangleHot> hot(count);
    std::vector<float4> b(2 * (size_t)count);
    RT_HIP(ctx, hipMemcpyAsync(hot.data(), ctx->d_tri, (size_t)count * sizeof(RtTriangleHot), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(b.data(), ctx->d_tri_bounds, (size_t)count * 32, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    auto put = [](float* dst, const float4& v) {
        dst[0] = v.x;
        dst[1] = v.y;
        dst[2] = v.z;
    };
    for (uint32_t i = 0; i < count; i++) {
        rt_scene_triangle& t = out[i];
        std::memset(&t, 0, sizeof(t));
        unpack_triangle(hot[i], t.a, t.edge_ab, t.edge_ac, t.calc_normal, t.face_normal);
        put(t.min_bounds, b[2 * i]);
        put(t.max_bounds, b[2 * i + 1]);
    }
    return RT_OK;
}

int rt_read_object_info(rt_ctx* ctx, rt_object_info* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_obj) return fail(ctx, RT_E_CAPACITY, "more objects than the buffer holds");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_obj, (size_t)count * 48, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_sub_object_info(rt_ctx* ctx, rt_sub_object_info* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_sub) return fail(ctx, RT_E_CAPACITY, "more sub-objects than the buffer holds");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_sub, (size_t)count * 32, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_accumulation(rt_ctx* ctx, float* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_accum, ctx->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_ray_count(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v = 0;
    RT_HIP(ctx, hipMemcpyAsync(&v, ctx->d_counter, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v;
    return RT_OK;
}

int rt_set_brute_force(rt_ctx* ctx, int enable) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (enable < 0 || enable > 2) return fail(ctx, RT_E_INVALID, "brute-force mode must be 0, 1 or 2");
    ctx->brute = enable;
    return RT_OK;
}

int rt_set_triangle_pruning(rt_ctx* ctx, int mode) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (mode < 0 || mode > 2) return fail(ctx, RT_E_INVALID, "triangle pruning mode must be 0, 1 or 2");
    ctx->tri_prune_mode = mode;
    return RT_OK;
}

int rt_streamed_bytes(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v[2] = {0, 0};
    RT_HIP(ctx, hipMemcpyAsync(v, ctx->d_stream, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v[0];
    return RT_OK;
}

int rt_streamed_bytes_l2(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v[2] = {0, 0};
    RT_HIP(ctx, hipMemcpyAsync(v, ctx->d_stream, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v[1];
    return RT_OK;
}

// rt_set_tile_schedule and the tuning key "tile_schedule": the claim order, with the recorded costs
// and orders of both streams discarded (after RT_ENTER: the primary stream follows the auxiliary one).
static int set_tile_schedule(rt_ctx* ctx, uint32_t schedule) {
    ctx->tile_schedule = schedule;
    for (int si = 0; si < 2; si++) {
        if (ctx->d_tile_sched[si])
            RT_HIP(ctx, hipMemsetAsync(ctx->d_tile_sched[si], 0, (4 * (size_t)ctx->owned_tiles + 2) * 4, ctx->stream));
        ctx->sched_launches[si] = 0;
    }
    return RT_OK;
}

// Exact variants of the schedule and the acceleration structures, for A/B measurements (the
// product reads no environment): every setting renders the same bits.
int rt_set_tuning(rt_ctx* ctx, const char* key, int32_t value) {
    RT_ENTER(ctx);
    if (!key) return fail(ctx, RT_E_INVALID, "rt_set_tuning: key is NULL");
    const std::string k(key);
    const int32_t v = value;
    auto range = [&](int32_t lo, int32_t hi) {
        return v >= lo && v <= hi ? RT_OK
                                  : fail(ctx, RT_E_INVALID, "rt_set_tuning: " + k + " must be in [" + std::to_string(lo) +
                                                                ", " + std::to_string(hi) + "]");
    };
    auto flag = [&](bool& field) {
        const int rc = range(0, 1);
        if (rc == RT_OK) field = v != 0;
        return rc;
    };
    int rc = RT_OK;
    if (k == "scene_in_lds") {
        if ((rc = range(0, 1)) == RT_OK) ctx->force_global_scene = v == 0;
    } else if (k == "lds_mode") {
        if ((rc = range(0, 2)) == RT_OK) ctx->max_lds_mode = v;
    } else if (k == "block_threads") {
        if (v != 0 && v != 256 && v != 512 && v != 1024)
            return fail(ctx, RT_E_INVALID, "rt_set_tuning: block_threads must be 0, 256, 512 or 1024");
        ctx->force_threads = (uint32_t)v;
    } else if (k == "waves_per_cu") {
        if ((rc = range(0, 32)) == RT_OK) ctx->waves_cap = (uint32_t)v;
    } else if (k == "tri_bvh") {
        if ((rc = flag(ctx->use_tri_bvh)) == RT_OK) ctx->tri_dirty = true;
    } else if (k == "tri_octants") {
        if ((rc = flag(ctx->use_tri_octants)) == RT_OK) ctx->tri_dirty = true;
    } else if (k == "tri_qnodes") {
        rc = flag(ctx->use_qnodes);
    } else if (k == "coop_leaves") {
        rc = flag(ctx->use_coop_leaves);
    } else if (k == "stage_subs") {
        rc = flag(ctx->stage_subs);
    } else if (k == "primary_pass") {
        if ((rc = range(-1, 1)) == RT_OK) ctx->primary_pass = v;
    } else if (k == "primary_threads") {
        if (v != 64 && v != 128 && v != 256 && v != 512 && v != 1024)
            return fail(ctx, RT_E_INVALID, "rt_set_tuning: primary_threads must be 64, 128, 256, 512 or 1024");
        ctx->primary_threads = (uint32_t)v;
    } else if (k == "primary_waves") {
        if (v != 0 && v != 8) return fail(ctx, RT_E_INVALID, "rt_set_tuning: primary_waves must be 0 or 8");
        ctx->primary_min_waves = (uint32_t)v;
    } else if (k == "primary_tile_major") {
        rc = flag(ctx->primary_tile_major);
    } else if (k == "sphere_bvh") {
        if ((rc = flag(ctx->use_bvh)) == RT_OK) ctx->slots_dirty = true;
    } else if (k == "sphere_leaf") {
        if ((rc = range(0, 64)) == RT_OK) {
            ctx->sphere_leaf_max = (uint32_t)v;
            ctx->slots_dirty = true;
        }
    } else if (k == "sphere_octants") {
        rc = flag(ctx->sphere_octants);
    } else if (k == "sphere_box_order") {
        if ((rc = flag(ctx->sphere_box_order)) == RT_OK) ctx->slots_dirty = true;
    } else if (k == "queue_stripes") {
        if ((rc = range(1, (int32_t)kQueueStripesMax)) == RT_OK) ctx->queue_stripes = (uint32_t)v;
    } else if (k == "trav_threshold") {
        if ((rc = range(0, 63)) == RT_OK) ctx->trav_threshold = (uint32_t)v;
    } else if (k == "drain_threshold") {
        if ((rc = range(0, 63)) == RT_OK) ctx->drain_threshold = (uint32_t)v;
    } else if (k == "drain_min_steps") {
        if ((rc = range(0, 1 << 20)) == RT_OK) ctx->drain_min_steps = (uint32_t)v;
    } else if (k == "leaf_batch") {
        if ((rc = range(0, 8)) == RT_OK) ctx->leaf_batch = (uint32_t)v;
    } else if (k == "tile_schedule") {
        if ((rc = range(0, 1)) == RT_OK) rc = set_tile_schedule(ctx, (uint32_t)v);
    } else if (k == "frame_parallel") {
        rc = flag(ctx->frame_parallel);
    } else if (k == "batch_overlap") {
        rc = flag(ctx->batch_overlap);
    } else if (k == "batch_schedule") {
        rc = flag(ctx->batch_schedule);
    } else if (k == "unit_tile_major") {
        rc = flag(ctx->unit_tile_major);
    } else if (k == "frame_par_instance") {
        rc = flag(ctx->frame_par_instance);
    } else if (k == "query_chunk") {
        if ((rc = range(1, (int32_t)kMaxQueryChunk)) == RT_OK) ctx->query_chunk = (uint32_t)v;
    } else if (k == "gather_chunk") {
        if ((rc = range(1, (int32_t)kMaxGatherChunk)) == RT_OK) ctx->gather_chunk = (uint32_t)v;
    } else if (k == "probe_chunk") {
        if ((rc = range(1, (int32_t)kMaxProbeChunk)) == RT_OK) ctx->probe_chunk = (uint32_t)v;
    } else if (k == "query_lds_mode") {
        if ((rc = range(-1, 2)) == RT_OK) ctx->query_lds_mode = v;
    } else if (k == "feature_band") {
        if ((rc = range(64, (int32_t)kMaxFeatureBand)) == RT_OK) ctx->feature_band = (uint32_t)v;
    } else if (k == "denoise_lds") {
        rc = flag(ctx->denoise_lds);
    } else if (k == "batch_memory_mb") {
        if ((rc = range(1, 1 << 30)) == RT_OK) ctx->batch_budget = (size_t)v << 20;
    } else {
        return fail(ctx, RT_E_INVALID, "rt_set_tuning: unknown key " + k);
    }
    return rc;
}

int rt_set_tile_schedule(rt_ctx* ctx, uint32_t schedule) {
    RT_ENTER(ctx);
    if (schedule > 1) return fail(ctx, RT_E_INVALID, "tile schedule must be 0 (index order) or 1 (cost-ordered)");
    return set_tile_schedule(ctx, schedule);
}

int rt_tile_schedule_state(rt_ctx* ctx, uint32_t* order, uint32_t* costs) {
    RT_ENTER(ctx);
    // the primary stream's schedule: the one every single-frame launch and every
    // other overlapped batch follows
    const size_t n = ctx->owned_tiles;
    const uint32_t* st = ctx->d_tile_sched[0];
    const uint64_t launches = ctx->sched_launches[0];
    const bool on = ctx->tile_schedule && st;
    const uint32_t par = (uint32_t)(launches & 1u);  // the next launch's parity
    for (size_t i = 0; i < n && order; i++) order[i] = (uint32_t)i;
    if (order && on && launches)
        RT_HIP(ctx, hipMemcpyAsync(order, st + 2 * n + par * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (costs) {
        if (on && launches)  // what the last launch recorded
            RT_HIP(ctx, hipMemcpyAsync(costs, st + (par ^ 1u) * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        else
            std::memset(costs, 0, n * 4);
    }
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_reset_ray_count(rt_ctx* ctx) {
    RT_ENTER(ctx);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_counter, 0, (1 + kDiagCounters) * sizeof(unsigned long long), ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(ctx->d_stream, 0, 2 * sizeof(unsigned long long), ctx->stream));
    return RT_OK;
}

int rt_accumulation_index(const rt_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return RT_E_INVALID;
    *out = ctx->k;
    return RT_OK;
}

int rt_set_timing(rt_ctx* ctx, int enable) {
    RT_ENTER(ctx);
    ctx->timing = enable != 0;
    // The launch-clock slots are allocated (and zeroed) here rather than by the first timed
    // launch: callers switch timing on ahead of the region they time (bench.py), which then
    // holds no hipMalloc on its launch path.
    if (ctx->timing && !ctx->d_clock) {
        const int rc = dev_alloc(ctx, &ctx->d_clock, kClockWords * (size_t)kClockSlots);
        if (rc) return rc;
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RT_OK;
}

int rt_last_dispatch_ms(rt_ctx* ctx, float* out_ms) {
    RT_ENTER(ctx);
    if (!out_ms) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *out_ms = ctx->last_ms;
    return RT_OK;
}

int rt_dispatch_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed) {
    RT_ENTER(ctx);
    if (!total_ms || !n_timed) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *total_ms = ctx->total_ms;
    *n_timed = ctx->n_timed;
    return RT_OK;
}

int rt_resolve_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed) {
    RT_ENTER(ctx);
    if (!total_ms || !n_timed) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *total_ms = ctx->resolve_total_ms;
    *n_timed = ctx->n_resolve_timed;
    return RT_OK;
}

int rt_reset_timing(rt_ctx* ctx) {
    RT_ENTER(ctx);
    int rc = collect_timing(ctx);
    if (rc) return rc;
    ctx->total_ms = 0.0;
    ctx->n_timed = 0;
    ctx->resolve_total_ms = 0.0;
    ctx->n_resolve_timed = 0;
    ctx->last_ms = 0.0f;
    return RT_OK;
}

int rt_owned_pixel_count(const rt_ctx* ctx, uint32_t rank, uint32_t world_size, uint64_t* out) {
    if (!ctx || !out || world_size == 0 || rank >= world_size) return RT_E_INVALID;
    *out = (uint64_t)owned_tile_count(ctx->tiles_x * ctx->tiles_y, rank, world_size) * 64u;
    return RT_OK;
}

int rt_pack_owned_accumulation(rt_ctx* ctx, void* dst_device) {
    RT_ENTER(ctx);
    if (!dst_device) return fail(ctx, RT_E_INVALID, "dst is NULL");
    if (ctx->owned_tiles == 0) return RT_OK;
    hipError_t e = rt_launch_pack(ctx->d_accum, static_cast<float4*>(dst_device), ctx->width, ctx->height,
                                  ctx->tiles_x, ctx->owned_tiles, ctx->rank, ctx->world, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_pack_tiles_kernel launch", e);
    return RT_OK;
}

int rt_unpack_accumulation(rt_ctx* ctx, const void* src_device, uint32_t src_rank, uint32_t world_size,
                           uint32_t divisor) {
    RT_ENTER(ctx);
    if (!src_device || world_size == 0 || src_rank >= world_size || divisor == 0)
        return fail(ctx, RT_E_INVALID, "unpack: bad arguments");
    hipError_t e = rt_launch_unpack(static_cast<const float4*>(src_device), ctx->d_accum, ctx->d_out, ctx->width,
                                    ctx->height, ctx->tiles_x, ctx->tiles_x * ctx->tiles_y, src_rank, 1, world_size,
                                    0, 0xffffffffu, (float)divisor, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_unpack_tiles_kernel launch", e);
    return RT_OK;
}

int rt_unpack_accumulation_ranks(rt_ctx* ctx, const void* src_device, uint64_t stride_px, uint32_t world_size,
                                 uint32_t skip_rank, uint32_t divisor) {
    RT_ENTER(ctx);
    const uint64_t cap = (uint64_t)owned_tile_count(ctx->tiles_x * ctx->tiles_y, 0, world_size ? world_size : 1) * 64u;
    if (!src_device || world_size == 0 || divisor == 0 || stride_px < cap)
        return fail(ctx, RT_E_INVALID, "unpack: bad arguments (stride below the largest rank's block?)");
    hipError_t e = rt_launch_unpack(static_cast<const float4*>(src_device), ctx->d_accum, ctx->d_out, ctx->width,
                                    ctx->height, ctx->tiles_x, ctx->tiles_x * ctx->tiles_y, 0, world_size, world_size,
                                    stride_px, skip_rank, (float)divisor, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_unpack_tiles_kernel launch", e);
    return RT_OK;
}

int rt_pack_owned_output(rt_ctx* ctx, void* dst_device) {
    RT_ENTER(ctx);
    if (!dst_device) return fail(ctx, RT_E_INVALID, "dst is NULL");
    if (ctx->owned_tiles == 0) return RT_OK;
    hipError_t e = rt_launch_pack_output(ctx->d_out, static_cast<uint32_t*>(dst_device), ctx->width, ctx->height,
                                         ctx->tiles_x, ctx->tiles_x * ctx->tiles_y, ctx->rank, 1, ctx->world, 0,
                                         0xffffffffu, false, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_pack_output_kernel launch", e);
    return RT_OK;
}

int rt_unpack_output(rt_ctx* ctx, const void* src_device, uint32_t src_rank, uint32_t world_size) {
    RT_ENTER(ctx);
    if (!src_device || world_size == 0 || src_rank >= world_size) return fail(ctx, RT_E_INVALID, "unpack: bad arguments");
    hipError_t e = rt_launch_pack_output(ctx->d_out, const_cast<uint32_t*>(static_cast<const uint32_t*>(src_device)),
                                         ctx->width, ctx->height, ctx->tiles_x, ctx->tiles_x * ctx->tiles_y, src_rank, 1,
                                         world_size, 0, 0xffffffffu, true, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_pack_output_kernel launch", e);
    return RT_OK;
}

int rt_unpack_output_ranks(rt_ctx* ctx, const void* src_device, uint64_t stride_px, uint32_t world_size,
                           uint32_t skip_rank) {
    RT_ENTER(ctx);
    const uint64_t cap = (uint64_t)owned_tile_count(ctx->tiles_x * ctx->tiles_y, 0, world_size ? world_size : 1) * 64u;
    if (!src_device || world_size == 0 || stride_px < cap)
        return fail(ctx, RT_E_INVALID, "unpack: bad arguments (stride below the largest rank's block?)");
    hipError_t e = rt_launch_pack_output(ctx->d_out, const_cast<uint32_t*>(static_cast<const uint32_t*>(src_device)),
                                         ctx->width, ctx->height, ctx->tiles_x, ctx->tiles_x * ctx->tiles_y, 0,
                                         world_size, world_size, stride_px, skip_rank, true, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_pack_output_kernel launch", e);
    return RT_OK;
}

int rt_debug_counters(rt_ctx* ctx, uint64_t* out, uint32_t n) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    const size_t m = std::min<size_t>(n, kDiagCounters + kDiagWaveRecords);
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_counter + 1, m * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_check_leaf_certificates(rt_ctx* ctx, uint32_t* mismatches, uint32_t* valid, uint32_t* total) {
    RT_ENTER(ctx);
    if (!mismatches || !valid || !total) return fail(ctx, RT_E_INVALID, "NULL output");
    *mismatches = *valid = *total = 0;
    RT_HIP(ctx, join_aux(ctx));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n = ctx->tri_prim_count;
    if (!ctx->d_tri_lcert || ctx->cones_dirty || n == 0 || ctx->tri_lcert_cap < (size_t)n * sizeof(TriLeafCert))
        return RT_OK;
    std::vector<TriLeafCert> dev(n);
    std::vector<SubObjectPrim> prims(n);
    std::vector<RtSubObject> subs(ctx->n_sub_dev);
    std::vector<RtTriangleHot> tris(ctx->n_tri_dev);
    RT_HIP(ctx, hipMemcpy(dev.data(), ctx->d_tri_lcert, n * sizeof(TriLeafCert), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(prims.data(), ctx->d_tri_prims, n * sizeof(SubObjectPrim), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(subs.data(), ctx->d_sub, subs.size() * sizeof(RtSubObject), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(tris.data(), ctx->d_tri, tris.size() * sizeof(RtTriangleHot), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        const RtSubObject& s = subs[std::min<uint32_t>(prims[i].sub, (uint32_t)subs.size() - 1u)];
        float lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(s.min_bounds[k], s.max_bounds[k]);
            hi[k] = std::fmax(s.min_bounds[k], s.max_bounds[k]);
        }
        const uint32_t n_tri = (uint32_t)tris.size();
        const uint32_t cnt = (s.triangle_count <= kLeafCertSlots && n_tri != 0u) ? s.triangle_count : 0u;
        float a[kLeafCertSlots][3], ab[kLeafCertSlots][3], ac[kLeafCertSlots][3], cn[kLeafCertSlots][3];
        for (uint32_t j = 0; j < cnt; ++j) {
            float fn[3];
            unpack_triangle(tris[std::min(s.first_triangle_index + j, n_tri - 1u)], a[j], ab[j], ac[j], cn[j], fn);
        }
        const TriLeafCert h = tricone::leafcert_build(cnt, a, ab, ac, cn, lo, hi);
        *mismatches += std::memcmp(&h, &dev[i], sizeof(h)) != 0;
        *valid += dev[i].w[7] != kLeafCertNone;
    }
    *total = n;
    return RT_OK;
}

int rt_launch_config(rt_ctx* ctx, uint32_t* threads, uint32_t* blocks, uint32_t* lds_bytes,
                     uint32_t* scene_in_lds) {
    RT_ENTER(ctx);  // the last launch: queued frames launched first
    if (!threads || !blocks || !lds_bytes || !scene_in_lds) return RT_E_INVALID;
    *threads = ctx->last_threads;
    *blocks = ctx->last_blocks;
    *lds_bytes = ctx->last_lds;
    *scene_in_lds = ctx->last_mode < 0 ? 0u : (uint32_t)ctx->last_mode;
    return RT_OK;
}

int rt_last_launch_passes(rt_ctx* ctx, uint32_t* passes) {
    RT_ENTER(ctx);  // the last launch: queued frames launched first
    if (!passes) return RT_E_INVALID;
    *passes = ctx->last_passes;
    return RT_OK;
}

void* rt_stream(rt_ctx* ctx) {
    if (!ctx) return nullptr;
    // flush_frames may launch and allocate: on the context's device
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    // work the caller orders on this stream follows every frame submitted so far
    if (flush_frames(ctx) != RT_OK || join_aux(ctx) != hipSuccess) return nullptr;
    ctx->primary_dirty = true;
    return (void*)ctx->stream;
}

}  // extern "C"

int rt_math_selftest(uint32_t which, uint64_t* mismatches, uint32_t* first_bad) {
    if (!mismatches || !first_bad || which > 6) return RT_E_INVALID;
    unsigned long long* d_bad = nullptr;
    uint32_t* d_first = nullptr;
    hipError_t e = hipMalloc(&d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&d_first, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_first, 0xff, sizeof(uint32_t));
    if (e == hipSuccess) e = rt_launch_math_selftest(which, d_bad, d_first, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_bad, d_first, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (d_first) (void)hipFree(d_first);
    if (e != hipSuccess) return RT_E_HIP;
    *mismatches = bad;
    return RT_OK;
}
