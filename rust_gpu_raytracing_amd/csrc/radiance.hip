// radiance.hip -- batched radiance queries for gfx950 (rt_radiance, rt_radiance_device; DESIGN.md
// §5.4e).
//
// rt_radiance_kernel answers "how much light arrives along this ray?" for arbitrary rays: per_pixel
// of the reference (compute_shader.wgsl:210-314) with the camera origin, the pixel's direction and
// the pixel index of the seed taken from a 32-B record, summed over `samples` samples. It stands on
// the query kernels' frame (rt_query_frame.h) -- one ray per lane, persistent wave64s taking chunks
// of rays, ballot + mbcnt refill, the three scene placements, the walk of rt_walk.h -- and on the path
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
//  * Each wave's first chunk is its own, by its index in the launch (claim_chunk).
//  * Counted ray segments (the rule of rt_ray_count: one per trace_ray call) are summed per lane,
//    reduced once per wave at exit and added to the caller's counter with one atomic per wave.
//
// Gather queries (rt_gather, rt_gather_device) run on the same kernel body,
// instantiated with kPathGather, and on rt_gather_resolve_kernel below. The contract, as in
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
//
// Probe queries (rt_probe_sh, rt_probe_sh_device) run on the same kernel body,
// instantiated with kPathProbe, and on rt_probe_resolve_kernel below. The contract, as in
// include/rt_abi.h:
//
// THE PROBE CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
// written order, with no contraction. For probe i with record (x, stream):
//  1. Sample index. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
//  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
//     gx, gy, gz = normal_distribution(&dseed) three times, in that order
//     (compute_shader.wgsl:622-628, theta drawn before rho).
//     dir = normalize((gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
//     dot(v, v) = (x*x + y*y) + z*z: a uniform direction on the sphere.
//  3. Path. L_s is the result rt_radiance defines for the record (x, stream, dir) with
//     first_sample = u, samples = 1 and the call's bounces. The origin is x as given (no offset).
//  4. Basis, on dir = (dx, dy, dz) of step 2 (before per_pixel's jitter):
//     b0 = 0.28209479f                       b1 = 0.48860251f * dy
//     b2 = 0.48860251f * dz                  b3 = 0.48860251f * dx
//     b4 = 1.09254843f * (dx*dy)             b5 = 1.09254843f * (dy*dz)
//     b6 = 0.31539157f * (3.0f*(dz*dz) - 1.0f)
//     b7 = 1.09254843f * (dx*dz)             b8 = 0.54627422f * (dx*dx - dy*dy)
//     T_{s,k} = L_s * b_k: one multiply per channel, all four channels.
//  5. Reduction, for each k = 0 .. 8 on its own: P_j (j = 0 .. 63) starts at +0.0f. For s ascending,
//     P_{s mod 64} = P_{s mod 64} + T_{s,k}. Then, for off = 32, 16, 8, 4, 2, 1:
//     P_j = P_j + P_{j+off} for every j < off. sh[i][k] = P_0. Lanes that got no sample take part
//     with +0.0f.
// End of the probe contract.
//
//  * The work item is a (probe, sample) pair: item t of a launch is sample t % samples of probe
//    t / samples, dealt in chunks as a radiance query's rays are. The lane runs that one path and
//    stores L_s to slot t of the launch's scratch (one 16-B store): no sample loop, no sum, so a
//    lane that finishes a short path takes the next item instead of waiting for a stripe.
//  * rt_probe_resolve_kernel runs steps 4 and 5: one wave per probe, lane j walks s = j, j + 64,
//    ... (step 5's P_j), loads L_s (1 KB per step across the wave), draws step 2's direction
//    again from (stream, u) with the path kernel's own function -- the scratch holds no
//    directions: 16 B per path, not 32 -- and adds the 36 products in sample order; then six
//    shuffle levels on each of the 36 values and nine 16-B stores.
//
// Lens queries (rt_lens, rt_lens_device, rt_lens_rays, rt_lens_rays_device) run on
// the same kernel body, instantiated with kPathLens, and on rt_lens_rays_kernel below. The contract,
// as in include/rt_abi.h:
//
// THE LENS CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
// written order, with no contraction. For pixel index i = y*width + x of the descriptor's image,
// stream = stream_base + i (u32, wrapping) and sample index u:
//  A. Screen point, as in camera_ray. xc = f32(x)/f32(width), yc = f32(y)/f32(height).
//     nx = xc*2.0f - 1.0f, ny = yc*2.0f - 1.0f, ax = nx*aspect.
//  B. PERSPECTIVE. t = P^-1 * (ax, ny, 1, 1) with glam's Mat4 * Vec4 =
//     ((c0*x + c1*y) + c2*z) + c3*w per component (P^-1 = inverse_projection, V^-1 = inverse_view).
//     ws = normalize(t.xyz / t.w) with normalize(v) = v * (1.0f / sqrt((x*x + y*y) + z*z)).
//     If aperture == 0: o = origin, d = (V^-1 * (ws, 0)).xyz: the very bits of camera_ray.
//     Otherwise: lseed = (stream * u * 326624u) ^ 0x85EBCA6Bu (u32, wrapping).
//     r1 = random(&lseed), r2 = random(&lseed), in that order (compute_shader.wgsl:587-599).
//     rad = aperture * sqrt(r1), th = 6.2831850051879883f * r2.
//     lx = rad * cos(th), ly = rad * cos(th - 1.5707963705062866f).
//     k = focus / (0.0f - ws.z), f = ws * k.
//     dv = normalize((f.x - lx, f.y - ly, f.z)), d = (V^-1 * (dv, 0)).xyz.
//     o = origin + (V^-1 * (lx, ly, 0, 0)).xyz.
//     cos is the oracle's oracle_cosf (cosf_c on the device; its arguments stay within
//     |x| <= 2 pi) and sqrt is correctly rounded.
//  C. ORTHOGRAPHIC. o = origin + (V^-1 * (ax*ortho_half_height, ny*ortho_half_height, 0, 0)).xyz.
//     d = (V^-1 * (0, 0, -1, 0)).xyz.
//  D. EQUIRECT. The inverse of environment_map_coords at pixel centres, world-aligned.
//     uc = (f32(x) + 0.5f)/f32(width), vc = (f32(y) + 0.5f)/f32(height).
//     az = (uc - 0.5f) * (2.0f*WGSL_PI), el = (vc - 0.5f) * WGSL_PI, ce = cos(el), with
//     WGSL_PI = 3.1415926536f.
//     d = (ce*cos(az), cos(el - 1.5707963705062866f), ce*cos(az - 1.5707963705062866f)). o = origin.
//  E. Path and sum. R = +0.0f on all four channels. For s = 0 .. samples-1 ascending,
//     u = first_sample + s (u32, wrapping); L_s is the result rt_radiance defines for the record
//     (o, stream, d) of step B, C or D at u with first_sample = u, samples = 1 and the call's
//     bounces, per_pixel's own jitter included. R = R + L_s per channel. radiance[i] = R.
// End of the lens contract.
//
//  * The work item is a pixel of the call's range, and the control flow is a radiance query's: the
//    samples of a pixel run back to back on its lane and are summed in order. One place differs:
//    the sample start, which draws the ray (lens_ray of rt_query_frame.h, steps A to D) instead of
//    loading a record, then start_sample_at.
//  * The descriptor is not a kernel argument (RadianceArgs and the other kinds' code stay as they
//    are): qa.rays points to a copy of it in device memory the context owns, read at wave-uniform
//    addresses, and qa.stripes carries the launch's first pixel. The copy is written on the launch's
//    stream by rt_lens_store_kernel, which takes the descriptor by value: stream order keeps a
//    launch in flight from seeing the next call's descriptor.
//  * rt_lens_rays_kernel writes the records of steps A to D, one thread per pixel, two 16-B stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "rt_launch.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct RadianceArgs {
    const float4* __restrict__ rays;  // rt_radiance_ray[count]: {origin.xyz, stream}, {direction.xyz, pad}
    float4* __restrict__ radiance;    // one float4 per ray
    // the fields of ChunkArgs (rt_query_frame.h: rt_launch_radiance fills them from chunk_args), in
    // the order this kernel's registers were tuned at
    unsigned long long count;
    unsigned long long* __restrict__ next;      // the chunk counter (zero at launch)
    unsigned long long* __restrict__ segments;  // counted ray segments, added to (null: not counted)
    uint32_t wave_chunk;                        // rays per claim
    uint32_t first_chunk;                       // rays of each wave's own first chunk (no claim)
    unsigned long long claimed_from;            // first ray handed out by the counter: first_chunk x the launch's waves
    uint32_t first_sample;                      // random_index of a ray's first sample (:154)
    uint32_t samples;                           // samples per ray, >= 1 (ka.bounces >= 1 too: the host answers 0)
    uint32_t stripes;                           // kPathGather: stripes per point, min(samples, 64)
                                                // kPathLens: the launch's first pixel (below 2^32)
};

// What the body of rt_radiance_kernel answers.
enum PathKind : int { kPathRadiance = 0, kPathGather = 1, kPathProbe = 2, kPathLens = 3 };

// Step 2 of the probe contract: the direction of the sample with index u of a probe's stream. The
// path kernel and the resolve kernel both call this, so both hold the same bits.
__device__ __forceinline__ f3 probe_direction(uint32_t stream, uint32_t u) {
    uint32_t dseed = (stream * u * 326624u) ^ 0x9E3779B9u;
    const float gx = normal01(dseed);
    const float gy = normal01(dseed);
    const float gz = normal01(dseed);
    return normalize(mk(gx, gy, gz));
}

// kPathGather: the path kernel of a gather query (the gather contract above). A "ray" is then a
// (point, stripe) item: qa.rays holds rt_gather_point records, qa.count the launch's items (points x
// qa.stripes, below 2^32), and qa.radiance the partials, 64 float4 per point.
// kPathProbe: the path kernel of a probe query (the probe contract above). A "ray" is a (probe,
// sample) item: qa.rays holds rt_probe records, 16 B each, qa.count the launch's items (probes x
// qa.samples, below 2^32), and qa.radiance the scratch, one float4 per item.
// kPathLens: the path kernel of a lens query (the lens contract above). A "ray" is a pixel of the
// launch's range: qa.rays points to the context's copy of the rt_lens_camera, qa.stripes is the
// range's first pixel, qa.count its pixels and qa.radiance one float4 per pixel of the range.
template <int kMode, bool kTris, uint32_t kThreads, PathKind kKind = kPathRadiance>
__global__ void __launch_bounds__(kThreads, 1) rt_radiance_kernel(KernelArgs ka, RadianceArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool kAux = kMode >= 1;
    constexpr bool kGather = kKind == kPathGather, kProbe = kKind == kPathProbe, kLens = kKind == kPathLens;
    // The path kernel's LDS image without the camera block: what the walk, the record and shading
    // read.
    SceneView sv = global_scene_view<kMode, kTris>(ka, ka.srgb);
    if constexpr (kMode >= 1) {
        sv = stage_walk_tables<kTris, kThreads>(ka, lds, sv);
        sv = stage_sphere_materials<kThreads>(ka, lds, sv);
        sv = stage_shading_tables<kThreads>(ka, lds, sv);
    }
    if constexpr (kMode == 2) sv = stage_triangle_tables<kThreads>(ka, lds, sv);
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
    TraceState ts = idle_trace_state(kF32Max);

    // Sample `sample` of the lane's ray: the record is read again (two 16-B loads that hit the
    // cache) instead of holding origin, direction and stream in 7 registers through every walk.
    // kGather: `ray` is point * 64 + stripe (the item's slot among the partials) and `sample` the
    // sample index s; the origin and the direction are steps 1 and 2 of the contract.
    // kProbe: `ray` is the item t; one 16-B load reads the probe's record.
    // kLens: `ray` is the pixel's position in the range; the ray is drawn from the descriptor.
    auto begin_sample = [&]() {
        if constexpr (kLens) {
            const rt_lens_camera* __restrict__ cam = reinterpret_cast<const rt_lens_camera*>(qa.rays);
            const uint32_t pixel = qa.stripes + (uint32_t)ray;
            const uint32_t stream = cam->stream_base + pixel, u = qa.first_sample + sample;
            const LensRay r = lens_ray(cam, pixel, stream, u);
            start_sample_at(r.o, stream, u, r.d, p);
        } else if constexpr (kProbe) {
            const uint32_t probe = (uint32_t)ray / qa.samples, s = (uint32_t)ray - probe * qa.samples;
            const float4 r0 = qa.rays[probe];
            const uint32_t stream = __float_as_uint(r0.w), u = qa.first_sample + s;
            start_sample_at(mk(r0.x, r0.y, r0.z), stream, u, probe_direction(stream, u), p);
        } else if constexpr (kGather) {
            const float4 r0 = qa.rays[2ull * (ray >> 6)], r1 = qa.rays[2ull * (ray >> 6) + 1ull];
            const f3 n = mk(r1.x, r1.y, r1.z);
            const uint32_t stream = __float_as_uint(r0.w), u = qa.first_sample + sample;
            start_sample_at(mk(r0.x, r0.y, r0.z) + n * 0.0001f, stream, u, gather_direction(n, stream, u), p);
        } else {
            const float4 r0 = qa.rays[2ull * ray], r1 = qa.rays[2ull * ray + 1ull];
            start_sample_at(mk(r0.x, r0.y, r0.z), __float_as_uint(r0.w), qa.first_sample + sample,
                            mk(r1.x, r1.y, r1.z), p);
        }
        mode = kSetup;
    };

    const uint32_t wave = wave_in_launch<kThreads>();
    WaveChunk c{0, 0, true, false};
    claim_chunk(qa, wave, c);

    while (true) {
        // 1. Shade the lanes whose walk has finished (:228-311). A path that ends adds its light
        // to the ray's sum (one f32 add per channel); then the ray's next sample, or its result.
        if (mode == kDone) {
            const Hit h = trace_end<kTris>(sv, ka, p.o, p.d, ts);
            ++segs;
            if constexpr (kProbe) {
                // the item's one path: L_s = +0.0f + light, the sum of a radiance query of one sample
                if (shade<kAux>(sv, ka, p, h)) {
                    qa.radiance[ray] = make_float4(0.0f + p.light.x, 0.0f + p.light.y, 0.0f + p.light.z, 0.0f + p.light.w);
                    mode = kIdle;
                } else {
                    mode = kSetup;
                }
            } else if (shade<kAux>(sv, ka, p, h)) {
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
            if (need == 0 || c.dry) break;
            const uint32_t avail = (uint32_t)(c.end - c.next);
            if (mode == kIdle) {
                const uint32_t rank = rank_among(need);
                if (rank < avail) {
                    if constexpr (kProbe) {
                        ray = c.next + rank;
                    } else if constexpr (kGather) {
                        const uint32_t item = (uint32_t)(c.next + rank), point = item / qa.stripes;
                        sample = item - point * qa.stripes;
                        ray = (unsigned long long)point * 64u + sample;
                    } else {
                        ray = c.next + rank;
                        sample = 0;
                    }
                    sum = make_float4(0.f, 0.f, 0.f, 0.f);
                    begin_sample();
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk(qa, wave, c);
        }
        // 3. Start the next segment of every lane that has one (ka.bounces >= 1: a path that
        // reached the limit ended in shade).
        if (mode == kSetup) {
            trace_begin<kTris>(sv, ka, p.o, p.d, ts);
            mode = ts.phase == 2 ? kDone : kTrav;
        }
        if (__ballot(mode != kIdle) == 0 && c.dry) break;
        // 4. Traverse (query_traverse, with the drain rule): finished lanes wait for the wave, which
        // then shades and refills them together.
        take_lane_walk(query_traverse<kMode, kTris, true>(sv, ka, p.o, p.d, lane_walk(ts, mode), c.dry, lds, WalkEnd{}), ts,
                       mode);
    }
    // The wave's counted segments: one reduction and one atomic per wave (the loop's exit is
    // wave-uniform, so all 64 lanes are here).
    if (qa.segments) {
        unsigned long long total = segs;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
        if ((threadIdx.x & 63u) == 0 && total != 0) atomicAdd(qa.segments, total);
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

// Steps 4 and 5 of a probe query: one wave per probe. Lane j adds the products of the samples
// j, j + 64, ... in ascending order into its 36 accumulators (step 5's P_j of the nine
// coefficients, four channels each), drawing each sample's direction again (probe_direction: the
// path kernel's bits). Then the tree as in rt_gather_resolve_kernel, on each of the 36 values, and
// lane 0 stores the probe's nine float4. `lights`: the launch's scratch, L_s of probe p at
// p * samples + s (points * samples is below 2^32).
__global__ void __launch_bounds__(kResolveThreads) rt_probe_resolve_kernel(const float4* __restrict__ lights,
                                                                          const float4* __restrict__ probes,
                                                                          float4* __restrict__ sh, uint32_t count,
                                                                          uint32_t first_sample, uint32_t samples) {
    const uint32_t probe = blockIdx.x * (kResolveThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (probe >= count) return;  // wave-uniform
    const uint32_t stream = __float_as_uint(probes[probe].w);
    const float4* __restrict__ mine = lights + (size_t)probe * samples;
    float acc[9][4];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u) {
        const float4 l = mine[s];
        const f3 d = probe_direction(stream, first_sample + s);
        const float b[9] = {0.28209479f,
                            0.48860251f * d.y,
                            0.48860251f * d.z,
                            0.48860251f * d.x,
                            1.09254843f * (d.x * d.y),
                            1.09254843f * (d.y * d.z),
                            0.31539157f * (3.0f * (d.z * d.z) - 1.0f),
                            1.09254843f * (d.x * d.z),
                            0.54627422f * (d.x * d.x - d.y * d.y)};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            acc[k][0] = acc[k][0] + l.x * b[k];
            acc[k][1] = acc[k][1] + l.y * b[k];
            acc[k][2] = acc[k][2] + l.z * b[k];
            acc[k][3] = acc[k][3] + l.w * b[k];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[k][ch] = acc[k][ch] + __shfl_down(acc[k][ch], off, 64);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) sh[(size_t)probe * 9u + k] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
    }
}

// The context's copy of a call's descriptor: the descriptor arrives by value, as a kernel argument,
// so the write is ordered on the stream like the launches that read the copy, and nothing of the
// caller's memory is read after the call. One lane, eleven 16-B stores at constant offsets.
struct LensWords {
    uint4 q[sizeof(rt_lens_camera) / 16u];
};
static_assert(sizeof(LensWords) == sizeof(rt_lens_camera), "rt_lens_camera is a whole number of 16-B words");
__global__ void __launch_bounds__(64) rt_lens_store_kernel(LensWords cam, uint4* __restrict__ slot) {
    if (threadIdx.x != 0) return;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(LensWords) / 16u; ++k) slot[k] = cam.q[k];
}

// rt_lens_rays: the records (o, stream, d, +0.0f) of steps A to D of the lens contract for the
// pixels first_pixel .. first_pixel + count - 1 and the sample index u, one thread per pixel.
__global__ void __launch_bounds__(kResolveThreads) rt_lens_rays_kernel(const rt_lens_camera* __restrict__ cam,
                                                                      float4* __restrict__ rays, uint32_t first_pixel,
                                                                      unsigned long long count, uint32_t u) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kResolveThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t pixel = first_pixel + (uint32_t)i, stream = cam->stream_base + pixel;
    const LensRay r = lens_ray(cam, pixel, stream, u);
    rays[2ull * i] = make_float4(r.o.x, r.o.y, r.o.z, __uint_as_float(stream));
    rays[2ull * i + 1ull] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

// The instances, (mode, triangles, threads), each for the four kinds: f(kernel, threads) for the
// one of (mode, tris, kind). Workgroup size by placement: the global-memory instance has
// no image to share: small workgroups, as the closest-hit query's. The staged instances share one
// image among as many waves as their registers allow without spilling: the walks from global
// memory with the shading state live need about 150 VGPRs (the path kernel's figure), which 16
// waves per workgroup (128 each) would spill.
template <PathKind kKind, class F>
static hipError_t with_radiance_instance(int mode, bool tris, F f) {
    if (mode == 0 && tris) return f(&rt_radiance_kernel<0, true, 256, kKind>, 256u);
    if (mode == 1 && tris) return f(&rt_radiance_kernel<1, true, 512, kKind>, 512u);
    if (mode == 2 && tris) return f(&rt_radiance_kernel<2, true, 1024, kKind>, 1024u);
    if (mode == 0 && !tris) return f(&rt_radiance_kernel<0, false, 256, kKind>, 256u);
    if (mode == 1 && !tris) return f(&rt_radiance_kernel<1, false, 1024, kKind>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance, as rt_query_threads)
uint32_t rt_radiance_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_radiance_instance<kPathRadiance>(mode, tris, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_radiance_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_radiance_instance<kPathRadiance>(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_gather_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_radiance_instance<kPathGather>(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_probe_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_radiance_instance<kPathProbe>(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_lens_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_radiance_instance<kPathLens>(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

// The launch of the instance of `kKind`: `count` items of `rays` into `radiance`.
template <PathKind kKind>
static hipError_t launch_path_kind(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                                   const void* rays, void* radiance, uint64_t count, unsigned long long* counter,
                                   unsigned long long* segments, uint32_t first_sample, uint32_t samples, uint32_t stripes,
                                   hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_radiance_instance<kKind>(mode, tris, [&](auto kernel, uint32_t t) {
        const ChunkArgs ca = chunk_args(count, counter, s, t);
        const RadianceArgs qa{static_cast<const float4*>(rays), static_cast<float4*>(radiance),
                              ca.count, ca.next, segments, ca.wave_chunk, ca.first_chunk, ca.claimed_from,
                              first_sample, samples, stripes};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, qa);
    });
}

// `stripes` 0: a radiance query of `count` rays. Otherwise the path kernel of a gather query:
// `rays` holds rt_gather_point records, `count` is the launch's items (points x stripes) and
// `radiance` receives the partials, 64 float4 per point.
hipError_t rt_launch_radiance(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                              const void* rays, void* radiance, uint64_t count, unsigned long long* counter,
                              unsigned long long* segments, uint32_t first_sample, uint32_t samples, uint32_t stripes,
                              hipStream_t stream) {
    return stripes ? launch_path_kind<kPathGather>(ka, mode, tris, lds_bytes, s, rays, radiance, count, counter, segments,
                                                   first_sample, samples, stripes, stream)
                   : launch_path_kind<kPathRadiance>(ka, mode, tris, lds_bytes, s, rays, radiance, count, counter, segments,
                                                     first_sample, samples, 0u, stream);
}

// The path kernel of a probe query: `probes` holds rt_probe records, `count` is the launch's items
// (probes x samples, below 2^32) and `lights` receives L_s of item t at slot t.
hipError_t rt_launch_probe_paths(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                                 const void* probes, void* lights, uint64_t count, unsigned long long* counter,
                                 unsigned long long* segments, uint32_t first_sample, uint32_t samples,
                                 hipStream_t stream) {
    return launch_path_kind<kPathProbe>(ka, mode, tris, lds_bytes, s, probes, lights, count, counter, segments,
                                        first_sample, samples, 0u, stream);
}

// Writes the context's copy `slot` (device memory, 16-byte aligned) of a lens descriptor,
// stream-ordered: after every launch that reads the previous copy, before those that follow.
hipError_t rt_launch_lens_camera(const rt_lens_camera& cam, void* slot, hipStream_t stream) {
    LensWords w;
    memcpy(&w, &cam, sizeof(w));
    hipLaunchKernelGGL(rt_lens_store_kernel, dim3(1), dim3(64), 0, stream, w, static_cast<uint4*>(slot));
    return hipGetLastError();
}

// The path kernel of a lens query: the `count` pixels from `first_pixel` on of the image of the
// descriptor at `cam` (the context's copy, device memory) into `radiance`, one float4 per pixel.
hipError_t rt_launch_lens(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                          const void* cam, void* radiance, uint32_t first_pixel, uint64_t count,
                          unsigned long long* counter, unsigned long long* segments, uint32_t first_sample,
                          uint32_t samples, hipStream_t stream) {
    return launch_path_kind<kPathLens>(ka, mode, tris, lds_bytes, s, cam, radiance, count, counter, segments,
                                       first_sample, samples, first_pixel, stream);
}

// The records of the same pixels for the sample index u into `rays`, 32 bytes per pixel.
hipError_t rt_launch_lens_rays(const void* cam, void* rays, uint32_t first_pixel, uint64_t count, uint32_t u,
                               hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const uint64_t blocks = (count + kResolveThreads - 1u) / kResolveThreads;  // count <= 2^32: at most 2^24
    hipLaunchKernelGGL(rt_lens_rays_kernel, dim3((uint32_t)blocks), dim3(kResolveThreads), 0, stream,
                       static_cast<const rt_lens_camera*>(cam), static_cast<float4*>(rays), first_pixel,
                       (unsigned long long)count, u);
    return hipGetLastError();
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

// Steps 4 and 5 over the lights of `count` probes (stream-ordered after the path kernel).
hipError_t rt_launch_probe_resolve(const void* lights, const void* probes, void* sh, uint32_t count, uint32_t first_sample,
                                   uint32_t samples, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const uint32_t per_block = kResolveThreads / 64u;
    hipLaunchKernelGGL(rt_probe_resolve_kernel, dim3((count + per_block - 1u) / per_block), dim3(kResolveThreads), 0,
                       stream, static_cast<const float4*>(lights), static_cast<const float4*>(probes),
                       static_cast<float4*>(sh), count, first_sample, samples);
    return hipGetLastError();
}
