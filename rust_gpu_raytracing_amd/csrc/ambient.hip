// ambient.hip -- batched ambient queries for gfx950 (rt_ambient, rt_ambient_device; DESIGN.md
// §5.4j).
//
// rt_ambient_kernel answers "which part of the hemisphere over this surface point is open within
// t_max?": per point the count of unoccluded sample directions and their sum (the bent normal),
// with the directions drawn on the device as a gather query draws them and every direction
// answered by the any-hit search of the occlusion queries (rt_occlusion_walk.h). It stands on the
// query kernels' frame (rt_query_frame.h): persistent wave64s taking chunks of items, ballot +
// mbcnt refill, the three scene placements, the walk of rt_walk.h. Nothing is shaded: no
// materials, textures or environment are read. The contract, as in include/rt_abi.h:
//
// THE AMBIENT CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
// written order, with no contraction. For point i with record (x, stream, n, t_max):
//  1. Sample index and origin: step 1 of the gather contract. For s = 0 .. samples-1,
//     u = first_sample + s (u32, wrapping). o = x + n * 0.0001f per component: one multiply and
//     one add.
//  2. Direction: step 2 of the gather contract. dseed = (stream * u * 326624u) ^ 0x9E3779B9u
//     (u32, wrapping). gx, gy, gz = normal_distribution(&dseed) three times, in that order.
//     dir = normalize(n + (gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
//     dot(v, v) = (x*x + y*y) + z*z. n is used as given and is not normalised. There is no
//     jitter: dir is the ray's direction as is.
//  3. Visibility. B_s is the byte rt_occluded defines for the record (o, dir, t_max): 1 iff a
//     primitive is accepted at a non-NaN distance t < t_max (strictly); t_max <= 0 or NaN
//     gives 0. V_s = 1 - B_s.
//  4. Term. T_s = (dir.x, dir.y, dir.z, 1.0f) where V_s == 1, and
//     T_s = (+0.0f, +0.0f, +0.0f, +0.0f) where V_s == 0.
//  5. Reduction: step 4 of the gather contract on T_s. P_j (j = 0 .. 63) starts at +0.0f on all
//     four channels. For s ascending, P_{s mod 64} = P_{s mod 64} + T_s. Then, for
//     off = 32, 16, 8, 4, 2, 1: P_j = P_j + P_{j+off} for every j < off. out[i] = P_0. Lanes
//     that got no sample take part with +0.0f.
// End of the ambient contract.
//
//  * The work item is a (point, stripe) pair, as in the gather instance of rt_radiance_kernel:
//    stripe j of a point runs its samples j, j + 64, ... back to back on one lane, which is step
//    5's P_j, and stores it among the point's 64 partials. Points with fewer than 64 samples have
//    only `samples` stripes. rt_gather_resolve_kernel (radiance.hip) runs step 5's tree.
//  * A lane whose search ends adds T_s into four registers and starts the stripe's next sample in
//    the same pass of the wave loop: it does not go idle between samples. An occluded sample adds
//    nothing: P + (+0.0f) has the bits of P, since no P is ever -0.0f (a sum is -0.0f only when
//    both terms are, and P starts at +0.0f).
//  * The record is read again at every sample (two 16-B loads that hit the cache): the lane
//    carries origin, direction and bound through the walk, not the normal and the stream.
//  * With no items left the wave traverses to the end, as the other query kernels do, except
//    while a lane has a further sample to start and more than trav_threshold lanes traverse: then
//    it still stops at the threshold, so that finished lanes start their next samples together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_occlusion_walk.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct AmbientArgs {
    const float4* __restrict__ points;  // rt_ambient_point[points]: {position.xyz, stream}, {normal.xyz, t_max}
    float4* __restrict__ partials;      // 64 float4 per point: {sum of open directions, open count} per stripe
    ChunkArgs chunks;                   // over the launch's items, points x stripes (below 2^32)
    uint32_t first_sample;              // sample index u of a point's first sample
    uint32_t samples;                   // samples per point, >= 1
    uint32_t stripes;                   // stripes per point, min(samples, 64)
};

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_ambient_kernel(KernelArgs ka, AmbientArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    SceneView sv = global_scene_view<kMode, kTris>(ka, nullptr);
    // The walk's tables of the LDS image (nothing is shaded: materials are left out).
    if constexpr (kMode >= 1) sv = stage_walk_tables<kTris, kThreads>(ka, lds, sv);
    if constexpr (kMode == 2) sv = stage_triangle_tables<kThreads>(ka, lds, sv);
    if constexpr (kMode >= 1) __syncthreads();

    // Lane states. A lane owns one (point, stripe) item at a time and one sample of it.
    constexpr uint32_t kIdle = 0, kSetup = 1, kTrav = 2, kDone = 3;
    uint32_t mode = kIdle;
    uint32_t slot = 0;    // point * 64 + stripe: the item's place among the partials (points <= 2^20)
    uint32_t sample = 0;  // the sample index s of the lane's current search
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    float bound = 0.0f;  // the seed: min(t_max, F32_MAX), or 0 for a t_max that nothing is closer than
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    TraceState ts = idle_trace_state(0.0f);

    // Sample `sample` of the lane's item: steps 1 and 2 of the contract and the search's seed.
    auto begin_sample = [&]() {
        const float4 r0 = qa.points[2u * (size_t)(slot >> 6)], r1 = qa.points[2u * (size_t)(slot >> 6) + 1u];
        const f3 n = mk(r1.x, r1.y, r1.z);
        o = mk(r0.x, r0.y, r0.z) + n * 0.0001f;
        d = gather_direction(n, __float_as_uint(r0.w), qa.first_sample + sample);
        // t_max <= 0 or NaN: nothing is closer (the search is skipped)
        bound = r1.w > 0.0f ? fminf(r1.w, kF32Max) : 0.0f;
        mode = kSetup;
    };

    const uint32_t wave = wave_in_launch<kThreads>();
    WaveChunk c{0, 0, true, false};
    claim_chunk(qa.chunks, wave, c);

    while (true) {
        // 1. The terms of the lanes whose search has finished (step 4), then the stripe's next
        // sample (64 on; no wrap: samples - sample >= 1) or its partial.
        if (mode == kDone) {
            if (!occluder_found(ts, bound)) {
                sum.x = sum.x + d.x;
                sum.y = sum.y + d.y;
                sum.z = sum.z + d.z;
                sum.w = sum.w + 1.0f;
            }
            const bool more = qa.samples - sample > 64u;
            sample += 64u;
            if (more) {
                begin_sample();
            } else {
                qa.partials[slot] = sum;
                mode = kIdle;
            }
        }
        // 2. Refill: idle lanes take the chunk's next items, in order.
        while (true) {
            const uint64_t need = __ballot(mode == kIdle);
            if (need == 0 || c.dry) break;
            const uint32_t avail = (uint32_t)(c.end - c.next);
            if (mode == kIdle) {
                const uint32_t rank = rank_among(need);
                if (rank < avail) {
                    const uint32_t item = (uint32_t)(c.next + rank), point = item / qa.stripes;
                    sample = item - point * qa.stripes;
                    slot = point * 64u + sample;
                    sum = make_float4(0.f, 0.f, 0.f, 0.f);
                    begin_sample();
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk(qa.chunks, wave, c);
        }
        // 3. Start the search of every lane that has a sample.
        if (mode == kSetup) {
            if (bound > 0.0f) {
                occlusion_begin<kTris>(sv, ka, o, d, bound, ts);
                mode = ts.phase == 2 ? kDone : kTrav;
            } else {
                ts.sph.t = ts.tri.t = 0.0f;
                mode = kDone;
            }
        }
        if (__ballot(mode != kIdle) == 0 && c.dry) break;
        // 4. Traverse (query_traverse): finished lanes wait for the wave, which then takes their
        // terms and starts their next samples together. With no items left it traverses to the
        // end -- unless a lane has a further sample to start and more than trav_threshold lanes
        // traverse: then it stops at the threshold, as with items left. (At or below the
        // threshold query_traverse would return without a step; with items left the refill
        // raises the count, without them nothing would, and the wave would spin.)
        const bool drain = c.dry && (__ballot(mode != kIdle && qa.samples - sample > 64u) == 0 ||
                                     (uint32_t)__popcll(__ballot(mode == kTrav)) <= ka.trav_threshold);
        take_lane_walk(query_traverse<kMode, kTris, false>(sv, ka, o, d, lane_walk(ts, mode), drain, lds, OccluderEnd{bound}),
                       ts, mode);
    }
}

// The instances, (mode, triangles, threads): f(kernel, threads) for the one of (mode, tris). The
// workgroup sizes are rt_occlusion_kernel's.
template <class F>
static hipError_t with_ambient_instance(int mode, bool tris, F f) {
    if (mode == 0 && tris) return f(&rt_ambient_kernel<0, true, 256>, 256u);
    if (mode == 1 && tris) return f(&rt_ambient_kernel<1, true, 1024>, 1024u);
    if (mode == 2 && tris) return f(&rt_ambient_kernel<2, true, 1024>, 1024u);
    if (mode == 0 && !tris) return f(&rt_ambient_kernel<0, false, 256>, 256u);
    if (mode == 1 && !tris) return f(&rt_ambient_kernel<1, false, 1024>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance, as rt_query_threads)
uint32_t rt_ambient_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_ambient_instance(mode, tris, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_ambient_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_ambient_instance(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

// `points` holds rt_ambient_point records, `count` is the launch's items (points x stripes, below
// 2^32) and `partials` receives 64 float4 per point, of which the first `stripes` are written.
hipError_t rt_launch_ambient(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                             const void* points, void* partials, uint64_t count, unsigned long long* counter,
                             uint32_t first_sample, uint32_t samples, uint32_t stripes, hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_ambient_instance(mode, tris, [&](auto kernel, uint32_t t) {
        const AmbientArgs qa{static_cast<const float4*>(points), static_cast<float4*>(partials),
                             chunk_args(count, counter, s, t), first_sample, samples, stripes};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, qa);
    });
}
