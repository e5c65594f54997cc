// display.hip -- the display transform for gfx950: metered auto-exposure, tone curves and the
// encode to display codes (rt_display, rt_read_display, rt_copy_display_to_device, rt_display_state,
// rt_display_reset).
//
// THE DISPLAY CONTRACT (tests/display_ref.py restates it from here; include/rt_abi.h carries the
// same text).
//
// Everything is f32 unless marked integer. Each written operation is one IEEE operation, in the
// written order, with no contraction and correctly rounded division. No exp, log or pow is used.
//
// S(p) is the source pixel, with four channels: accumulation(p) / D on all four channels (exactly
// rt_denoise's c0) for RT_DISPLAY_ACCUMULATION, the f32 result of the last denoise call for
// RT_DISPLAY_DENOISED, the caller's plane for RT_DISPLAY_PLANE.
//
// 1. Metering (only when auto_exposure == 1).
//   Per pixel, L = (0.2126f*S.r + 0.7152f*S.g) + 0.0722f*S.b.
//   The pixel is metered iff L > 0 && L < +inf. Both tests are false for NaN.
//   Its bin is an integer: j = clamp((int)(bits(L) >> 20) - 888, 0, 255).
//     This gives 8 bins per octave over [2^-16, 2^16). 888 = (127-16)*8.
//     Smaller values go to bin 0, larger ones to bin 255.
//   hist[j] += 1.
//   The histogram is a set of integer counts, so it is independent of schedule and order.
//
// 2. Exposure solve (integer until the last line; u64).
//   total = sum of hist.
//   lo = total*low_permille/1000.
//   hi = total - total*high_permille/1000.
//   Walking j ascending with a running sum cum, n_j = |[cum, cum+hist[j]) intersected with [lo, hi)|.
//   Nn = sum of n_j and Sn = sum of n_j*(2j+1).
//   If total == 0: there is no target.
//   Otherwise:
//     a = (2*Sn + Nn) / (2*Nn). This is the mean bin centre in 1/16 octaves, rounded. It is in 1..511.
//     n = 256 - a, q = floor(n / 16), r = n - 16*q.
//     E_t = key * ldexpf(T16[r], q).
//     E_t = min(max(E_t, min_exposure), max_exposure).
//   T16[r] is 2^(r/16) rounded to f32. Its bits are:
//     0x3f800000, 0x3f85aac3, 0x3f8b95c2, 0x3f91c3d3, 0x3f9837f0, 0x3f9ef532, 0x3fa5fed7, 0x3fad583f,
//     0x3fb504f3, 0x3fbd08a4, 0x3fc5672a, 0x3fce248c, 0x3fd744fd, 0x3fe0ccdf, 0x3feac0c7, 0x3ff5257d.
//
// 3. Adaptation. E_prev is the state.
//   State none, target none: E = min(max(1.0f, min_exposure), max_exposure).
//   State none, target E_t: E = E_t.
//   State E_prev, target none: E = E_prev.
//   State E_prev, target E_t: E = E_prev + (E_t - E_prev)*adaptation.
//   The state becomes E.
//   With auto_exposure == 0: E = params.exposure. The state and the stored histogram are left untouched.
//
// 4. Tone curve, per colour channel.
//   x = S.c * E.
//   x = x > 0 ? x : 0. NaN and -0 give +0.
//   x = min(x, 65536.0f).
//   LINEAR: y = x.
//   REINHARD: iw2 = 1.0f/(white*white), computed on the host in f32; y = (x*(1.0f + x*iw2)) / (1.0f + x).
//   ACES: y = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f).
//   Then y = min(y, 1.0f).
//   Alpha is clamp01(S.a) with no exposure and no curve (NaN gives 0, as in the frame's clamp). It is
//   always packed as the frame packs it.
//
// 5. Encode.
//   NONE: code = (uint32_t)(y*255.0f) & 0xff, which is pack_rgba8.
//   SRGB: code is the largest j in 0..255 with srgb_table[j] <= y.
//     The table is the 256-entry table of rt_srgb_table.
//     It is strictly increasing, so a branch-free 8-step search finds j.
//   The packed word is r | g<<8 | b<<16 | a<<24.
// End of the display contract.
//
// What is MI355X-specific. Three kernels, all with plain vector stores, no scratch:
//   rt_display_meter_kernel: grid-stride over at most kMeterBlocks workgroups of 256 threads, four
//     16-B loads per lane in flight per trip. Each wave owns one 256-bin histogram in LDS (4 KB per
//     workgroup) and counts with non-returning LDS integer adds; a wave whose 64 lanes all fall into
//     one bin (a flat region, where 64 adds to one LDS address would serialise) adds the count once
//     from one lane. At exit lane t of the workgroup sums bin t of the four copies and, when it is
//     not zero, adds it to the context's bins with one global integer atomic: a workgroup's merge is
//     contiguous dwords. Integer sums: exact under any order.
//   rt_display_solve_kernel: one wave. Lane l owns bins 4l..4l+3 (one 16-B load), a shuffle scan gives
//     each lane its running sum, the clipped counts are reduced with xor shuffles and lane 0 runs the
//     f32 lines of steps 2 and 3. The same wave keeps a copy of the histogram for rt_display_state and
//     zeroes the live bins for the next call.
//   rt_display_tone_kernel<op, encode>: one pixel per lane, one 16-B load and one 4-B store; E is a
//     uniform load from device memory (auto) or a kernel argument (manual). The sRGB table is staged
//     into 1 KB of LDS, where the 3 x 8 divergent search reads cost no vector-cache traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_path_common.h"

#pragma clang fp contract(off)

using namespace rtk;

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64, kBins = 256;
constexpr uint32_t kMeterBlocks = 512;  // one pass of the metering grid covers 512 x 256 x 4 pixels
constexpr uint32_t kMeterUnroll = 4;

__constant__ uint32_t kT16[16] = {0x3f800000u, 0x3f85aac3u, 0x3f8b95c2u, 0x3f91c3d3u, 0x3f9837f0u, 0x3f9ef532u,
                                  0x3fa5fed7u, 0x3fad583fu, 0x3fb504f3u, 0x3fbd08a4u, 0x3fc5672au, 0x3fce248cu,
                                  0x3fd744fdu, 0x3fe0ccdfu, 0x3feac0c7u, 0x3ff5257du};

// S(p): the plane divided by `div` on all four channels (div is 1.0f, an exact identity, for the
// denoised and the caller's planes).
__device__ __forceinline__ float4 source_pixel(const float4* __restrict__ src, uint64_t i, float div) {
    const float4 v = src[i];
    return make_float4(v.x / div, v.y / div, v.z / div, v.w / div);
}

// Step 1: the pixel's bin, or -1 when it is not metered.
__device__ __forceinline__ int meter_bin(float4 s) {
    const float l = (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z;
    if (!(l > 0.0f && l < __builtin_inff())) return -1;
    const int j = (int)(__float_as_uint(l) >> 20) - 888;
    return min(max(j, 0), (int)kBins - 1);
}

}  // namespace

// ---- metering --------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) rt_display_meter_kernel(const float4* __restrict__ src, uint64_t n, float div,
                                                                    uint32_t* __restrict__ bins) {
    __shared__ uint32_t hist[kWaves * kBins];
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) hist[i * kBins + tid] = 0u;
    __syncthreads();
    uint32_t* mine = hist + (tid >> 6) * kBins;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    // the trip count is uniform over the workgroup: every lane stays active for the wave votes
    for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n; base += kMeterUnroll * stride) {
        float4 s[kMeterUnroll];
        bool ok[kMeterUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kMeterUnroll; ++u) {
            const uint64_t i = base + u * stride + tid;
            ok[u] = i < n;
            s[u] = source_pixel(src, ok[u] ? i : 0, div);  // pixel 0 always exists; dropped below
        }
#pragma unroll
        for (uint32_t u = 0; u < kMeterUnroll; ++u) {
            const int j = ok[u] ? meter_bin(s[u]) : -1;
            const int first = __builtin_amdgcn_readfirstlane(j);
            if (__all(j == first)) {  // one bin (or nothing) for the whole wave: one add of 64
                if (first >= 0 && (tid & 63u) == 0u)
                    (void)__hip_atomic_fetch_add(&mine[first], 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if (j >= 0) {
                (void)__hip_atomic_fetch_add(&mine[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) sum += hist[i * kBins + tid];
    if (sum != 0u) (void)__hip_atomic_fetch_add(&bins[tid], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- exposure solve and adaptation -----------------------------------------------------------------

struct DisplaySolveArgs {
    uint32_t* __restrict__ bins;   // the live bins: read, then zeroed for the next call
    uint32_t* __restrict__ kept;   // their copy for rt_display_state
    uint32_t* __restrict__ state;  // [0]: E (f32 bits), [2..3]: the metered count (u64)
    uint32_t low_permille, high_permille;
    float key, min_exposure, max_exposure, adaptation;
    uint32_t has_state;            // 1: state[0] holds E_prev
};

__global__ void __launch_bounds__(64) rt_display_solve_kernel(DisplaySolveArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint4 h = reinterpret_cast<const uint4*>(a.bins)[lane];
    reinterpret_cast<uint4*>(a.kept)[lane] = h;
    reinterpret_cast<uint4*>(a.bins)[lane] = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t c[4] = {h.x, h.y, h.z, h.w};
    const uint64_t own = ((uint64_t)h.x + h.y) + ((uint64_t)h.z + h.w);
    uint64_t incl = own;  // inclusive scan over the lanes
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, off, 64);
        if (lane >= off) incl += t;
    }
    const uint64_t total = __shfl((unsigned long long)incl, 63, 64);
    const uint64_t lo = total * a.low_permille / 1000u;
    const uint64_t hi = total - total * a.high_permille / 1000u;
    uint64_t cum = incl - own, nn = 0, sn = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t b0 = cum > lo ? cum : lo, e = cum + c[k], b1 = e < hi ? e : hi;
        const uint64_t nj = b1 > b0 ? b1 - b0 : 0;
        nn += nj;
        sn += nj * (2u * (4u * lane + k) + 1u);
        cum = e;
    }
#pragma unroll
    for (uint32_t off = 32; off >= 1; off >>= 1) {
        nn += __shfl_xor((unsigned long long)nn, off, 64);
        sn += __shfl_xor((unsigned long long)sn, off, 64);
    }
    if (lane != 0) return;
    float e_out;
    if (total != 0) {
        const uint64_t am = (2u * sn + nn) / (2u * nn);  // nn >= 1: low_permille + high_permille < 1000
        const int m = 256 - (int)am;
        const int q = m >> 4, r = m & 15;                // floor division: m may be negative
        const float scale = __uint_as_float((uint32_t)(127 + q) << 23);  // 2^q, q in -16..15
        float e_t = a.key * (__uint_as_float(kT16[r]) * scale);          // the inner product is exact: ldexpf
        e_t = e_t > a.min_exposure ? e_t : a.min_exposure;
        e_t = e_t < a.max_exposure ? e_t : a.max_exposure;
        if (a.has_state) {
            const float e_prev = __uint_as_float(a.state[0]);
            e_out = e_prev + (e_t - e_prev) * a.adaptation;
        } else {
            e_out = e_t;
        }
    } else if (a.has_state) {
        e_out = __uint_as_float(a.state[0]);
    } else {
        e_out = 1.0f > a.min_exposure ? 1.0f : a.min_exposure;
        e_out = e_out < a.max_exposure ? e_out : a.max_exposure;
    }
    a.state[0] = __float_as_uint(e_out);
    a.state[2] = (uint32_t)total;
    a.state[3] = (uint32_t)(total >> 32);
}

// ---- tone curve and encode -------------------------------------------------------------------------

struct DisplayToneArgs {
    const float4* __restrict__ src;
    uint32_t* __restrict__ dst;
    uint64_t n;
    float div;
    const uint32_t* __restrict__ state;  // auto: E is state[0]; null: E is `exposure`
    float exposure;
    float iw2;                           // RT_TONE_REINHARD: 1.0f/(white*white)
    const float* __restrict__ srgb;      // the 256-entry decode table (RT_ENCODE_SRGB)
};

namespace {

template <uint32_t kOp>
__device__ __forceinline__ float tone(float c, float e, float iw2) {
    float x = c * e;
    x = x > 0.0f ? x : 0.0f;
    x = x < 65536.0f ? x : 65536.0f;
    float y;
    if constexpr (kOp == 1u)
        y = (x * (1.0f + x * iw2)) / (1.0f + x);
    else if constexpr (kOp == 2u)
        y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    else
        y = x;
    return y < 1.0f ? y : 1.0f;
}

// The largest j with tab[j] <= y (tab[0] is 0 and y >= 0): eight steps, no branch.
__device__ __forceinline__ uint32_t srgb_code(const float* tab, float y) {
    uint32_t j = 0u;
#pragma unroll
    for (uint32_t step = 128u; step >= 1u; step >>= 1) j += tab[j + step] <= y ? step : 0u;
    return j;
}

}  // namespace

template <uint32_t kOp, uint32_t kEncode>
__global__ void __launch_bounds__(kThreads) rt_display_tone_kernel(DisplayToneArgs a) {
    __shared__ float tab[kBins];
    if constexpr (kEncode == 1u) {
        tab[threadIdx.x] = a.srgb[threadIdx.x];
        __syncthreads();
    }
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const float e = a.state ? __uint_as_float(a.state[0]) : a.exposure;
    const float4 s = source_pixel(a.src, i, a.div);
    const float r = tone<kOp>(s.x, e, a.iw2), g = tone<kOp>(s.y, e, a.iw2), b = tone<kOp>(s.z, e, a.iw2);
    const float al = clamp01(s.w);
    uint32_t word;
    if constexpr (kEncode == 1u)
        word = srgb_code(tab, r) | (srgb_code(tab, g) << 8) | (srgb_code(tab, b) << 16) |
               (pack_rgba8(0.0f, 0.0f, 0.0f, al) & 0xff000000u);
    else
        word = pack_rgba8(r, g, b, al);
    a.dst[i] = word;
}

// ---- launches --------------------------------------------------------------------------------------

static uint32_t rt_display_meter_blocks(uint64_t n) {
    const uint64_t need = (n + kThreads - 1u) / kThreads;
    return (uint32_t)(need < kMeterBlocks ? need : kMeterBlocks);
}

hipError_t rt_launch_display_meter(const float4* src, uint64_t n, float div, uint32_t* bins, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_display_meter_kernel, dim3(rt_display_meter_blocks(n)), dim3(kThreads), 0, stream, src, n, div,
                       bins);
    return hipGetLastError();
}

hipError_t rt_launch_display_solve(uint32_t* bins, uint32_t* kept, uint32_t* state, uint32_t low_permille,
                                   uint32_t high_permille, float key, float min_exposure, float max_exposure,
                                   float adaptation, bool has_state, hipStream_t stream) {
    const DisplaySolveArgs a{bins, kept, state, low_permille, high_permille, key, min_exposure, max_exposure, adaptation,
                             has_state ? 1u : 0u};
    hipLaunchKernelGGL(rt_display_solve_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t rt_launch_display_tone(const float4* src, uint32_t* dst, uint64_t n, float div, const uint32_t* state,
                                  float exposure, float iw2, const float* srgb, uint32_t op, uint32_t encode,
                                  hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const DisplayToneArgs a{src, dst, n, div, state, exposure, iw2, srgb};
    const dim3 grid((uint32_t)((n + kThreads - 1u) / kThreads)), block(kThreads);
    switch (op * 2u + encode) {
        case 0u: hipLaunchKernelGGL((rt_display_tone_kernel<0u, 0u>), grid, block, 0, stream, a); break;
        case 1u: hipLaunchKernelGGL((rt_display_tone_kernel<0u, 1u>), grid, block, 0, stream, a); break;
        case 2u: hipLaunchKernelGGL((rt_display_tone_kernel<1u, 0u>), grid, block, 0, stream, a); break;
        case 3u: hipLaunchKernelGGL((rt_display_tone_kernel<1u, 1u>), grid, block, 0, stream, a); break;
        case 4u: hipLaunchKernelGGL((rt_display_tone_kernel<2u, 0u>), grid, block, 0, stream, a); break;
        case 5u: hipLaunchKernelGGL((rt_display_tone_kernel<2u, 1u>), grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
