// rt_post.cpp — what include/rt_abi.h does to a rendered frame.
//
// The first-hit feature buffers (rt_compute_features and its read-backs), rt_denoise, the temporal
// reprojection (rt_denoise_temporal, rt_denoise_temporal_motion) and the display transform
// (rt_display). It launches denoise.hip and display.hip, and traces the feature rays with
// run_query (rt_queries.cpp).
#include <algorithm>
#include <cmath>
#include <utility>

#include "rt_ctx.h"
#include "rt_launch.h"

namespace {

constexpr uint32_t kMaxDenoiseIterations = 8;
// The display transform's metering buffer (display.hip): live bins | kept bins | {E, -, metered lo, hi}.
constexpr uint32_t kDispBins = 256;
constexpr uint32_t kDispStateWords = 4;

}  // namespace

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
