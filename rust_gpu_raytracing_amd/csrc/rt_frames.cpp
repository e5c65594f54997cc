// rt_frames.cpp — the frame launches of include/rt_abi.h.
//
// rt_dispatch, rt_compute_frame(s), rt_submit_frames, rt_set_frame_batch, rt_frame_batch, rt_flush,
// rt_synchronize and rt_copy_output_to_device, the frame queue behind them (flush_frames), the
// scene as a launch sees it (the carve that the queries of rt_queries.cpp share), and the
// multi-rank pack and unpack calls. It launches pathtrace.hip (the path kernel, the primary
// pre-pass, the resolve, the brute-force wavefront, the tile packs) and scene_edit.hip's
// derivations of what the triangle walks read.
#include <algorithm>

#include "rt_ctx.h"
#include "rt_launch.h"

namespace {

constexpr size_t kLdsSceneBudget = 64 * 1024;    // mode 1: spheres/materials/objects/sphere BVH per workgroup
constexpr size_t kLdsAccelBudget = 150 * 1024;   // mode 2: + triangle accelerator (one 1024-thread workgroup per CU)
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
// The cost-ordered tile schedule is used where a wave takes at least this many tiles (schedule_state).
constexpr uint64_t kSchedMinTilesPerWave = 4;
// Frame batching (rt_set_frame_batch): at most this many frames per launch.
constexpr uint32_t kMaxFrameBatch = 64;
// Frame-parallel batches (every (frame, tile) its own queue unit, lights resolved
// in order afterwards) up to this many frames x samples; larger batches run each
// pixel's frames back to back on one lane.
constexpr uint32_t kMaxParallelLights = 64;

}  // namespace

// ---- the scene as a launch sees it (SceneLaunch, rt_ctx.h) -------------------------------------

void rth::scene_base_args(rt_ctx* ctx, KernelArgs& ka) {
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
void rth::scene_carve(rt_ctx* ctx, KernelArgs& ka, int max_mode, SceneLaunch& sl) {
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
int rth::scene_accel_args(rt_ctx* ctx, KernelArgs& ka, SceneLaunch& sl) {
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

// Frame batching (rt_set_frame_batch): rt_compute_frame queues frames and one
// launch renders the whole batch (each pixel's frames back to back on one lane,
// every frame's accumulation and output written). The batch is launched when it
// is full and before anything else touches the context, so every other entry
// point sees exactly the state the sequence of single-frame dispatches leaves.
int rth::flush_frames(rt_ctx* ctx) {
    if (ctx->pending_frames == 0) return RT_OK;
    const uint32_t n = ctx->pending_frames;
    ctx->pending_frames = 0;
    return dispatch_frames(ctx, ctx->pending_bounces, n);
}

int rt_dispatch(rt_ctx* ctx, uint32_t bounces) {
    RT_ENTER(ctx);
    return dispatch_frames(ctx, bounces, 1);
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
int rth::copy_plane_to_device(rt_ctx* ctx, const char* entry, const uint32_t* src, const char* missing,
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
