// denoise.hip -- first-hit feature buffers and the guided a-trous filter for gfx950
// (rt_compute_features, rt_denoise).
//
// FEATURES. Two float4 planes of width*height pixels, row-major:
//   plane A: normal.xyz, t          plane B: albedo.rgb, hit (1.0f or 0.0f)
// Per pixel, the un-jittered camera ray exactly as rt_pick defines it (the camera origin plus the
// ray-buffer direction, or pixel_ray while rt_update_camera_matrices is in effect) and the record
// rt_trace_rays would return for it.
//   Hit:  normal, t straight from the record; albedo = sample_texture(materials[min(material_index,
//         material_count-1)].texture_index, u, v).rgb with the clamp, sRGB table and layer clamp of
//         the path kernel's shading (compute_shader.wgsl:26-40). Emission is ignored.
//   Miss: normal = 0, t = 3.4028235e38f, hit = 0; albedo = the environment texel at
//         environment_map_coords(direction) (compute_shader.wgsl:580-585), through the kernel's
//         exact atan2 / asin helpers.
// Construction: rt_feature_rays_kernel writes rt_query_ray records for a band of pixels (it
// generalises rt_pick_ray_kernel), the unchanged rt_query_kernel traces them into scratch rt_hit
// records, rt_feature_resolve_kernel turns records into the planes. Exact by construction.
//
// THE FILTER. The arithmetic below is the contract (tests/denoise_ref.py restates it from here).
//
// Everything is f32, one IEEE operation per written operation, in the written order. The build's
// numeric flags guarantee no contraction and correctly rounded `/` and `sqrt`.
//
// Inputs. Per pixel p:
//   c0(p) = accumulation(p) / D, all four channels;
//   D = (float)((k-1) * compute_per_frame);
//   k is the context's accumulation counter, as reported by rt_accumulation_index;
//   n(p), z(p), a(p), hit(p) from the feature planes.
//
// Host-side constants, computed in f32:
//   N = (k-1)*compute_per_frame;
//   s0 = sigma_color / sqrtf((float)N);
//   k_a = 1.0f / (sigma_albedo*sigma_albedo);
//   for iteration i: s_i = s0 * 0.5f^i (exact scaling) and k_c = 1.0f / (s_i*s_i).
//
// Iteration i = 0 .. iterations-1:
//   step s = 1<<i;
//   h = {1/16, 1/4, 3/8, 1/4, 1/16};
//   taps q = p + s*(dx,dy);
//   dy is the outer loop and dx the inner loop, each running -2..2 ascending.
//
// Centre tap. w = h[2]*h[2] (that is 9/64). It is always taken and evaluates no guide.
//
// Other taps. A tap is skipped (it adds nothing to either sum) if q is outside the image. Otherwise:
//   Guide g:
//     If hit(p) and hit(q) are both 0, then g = 1.
//     If exactly one of them is 0, then g = 0.
//     Otherwise g = wn*wz, with:
//       d = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z);
//       wn = d^32, by five squarings;
//       x = |z_p - z_q| / (sigma_depth*(z_p + z_q) + 1e-30f);
//       wz = 1/(1 + x*x).
//   Albedo:
//     da = a_p - a_q;
//     xa = ((da.r*da.r + da.g*da.g) + da.b*da.b) * k_a;
//     ra = 1/(1+xa).
//   Colour, on the current iteration's input:
//     dc = c_p.rgb - c_q.rgb;
//     xc = ((dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b) * k_c;
//     rc = 1/(1+xc).
//   Weight: w = (((h[dy]*h[dx]) * g) * (ra*ra)) * (rc*rc).
//   The tap is skipped unless w > 0. That test is false for NaN.
//
// Result per iteration. Per channel, num = num + w*c_q and den = den + w, in tap order starting
// from 0. The result is num/den.
//
// After the last iteration the f32 RGBA result is kept. Its clamp01 then pack_to_u32 (the
// truncating pack the frame output uses) goes to a separate denoised-output buffer.
// iterations == 0 is just c0 and its pack. That pack equals rt_read_output of the same frame.
// Pixels whose accumulation is not finite give unspecified values there only.
//
// What is MI355X-specific: one pixel per lane, 256-thread workgroups over a 32x8 pixel tile (a
// wave64 covers two 32-pixel row segments: every plane access of a wave is two 512-B runs of 16-B
// vector loads). The three input planes (two guides and the ping-pong colour) of the passes with
// step 1 and 2 can be staged as tile + halo in LDS (kLds: 3 x (32+4s) x (8+4s) x 16 B, 20 / 30 KB),
// each texel then read from L2 once per workgroup instead of up to 25 times from the vector cache;
// steps >= 4 load their taps directly (a tile + halo would be larger than the taps it serves).
// Clamp and pack are fused into the last pass. No atomics; plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_path_common.h"

#pragma clang fp contract(off)

using namespace rtk;

namespace {

constexpr uint32_t kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;

__device__ __forceinline__ float4 ld_f4(const float4* __restrict__ p, size_t i) { return p[i]; }

}  // namespace

// ---- features ------------------------------------------------------------------------------------

// The un-jittered camera rays of pixels [first, first + count) as rt_query_ray records.
__global__ void __launch_bounds__(256) rt_feature_rays_kernel(KernelArgs ka, uint32_t first, uint32_t count,
                                                              float4* __restrict__ rays) {
    __shared__ float cam[33];
    const uint32_t tid = threadIdx.x;
    if (tid < 16) {
        cam[tid] = ka.inv_proj[tid];
        cam[16 + tid] = ka.inv_view[tid];
    }
    if (tid == 16) cam[32] = ka.aspect;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    if (i >= count) return;
    const uint32_t p = first + i;
    const uint32_t y = p / ka.width, x = p - y * ka.width;
    const f3 d = pixel_ray(ka, cam, p, x, y);
    rays[2 * (size_t)i] = make_float4(ka.camera_origin[0], ka.camera_origin[1], ka.camera_origin[2], 0.0f);
    rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

// rt_hit records of pixels [first, first + count) -> the two feature planes.
__global__ void __launch_bounds__(256) rt_feature_resolve_kernel(KernelArgs ka, uint32_t first, uint32_t count,
                                                                 const float4* __restrict__ rays,
                                                                 const uint4* __restrict__ hits,
                                                                 float4* __restrict__ plane_a,
                                                                 float4* __restrict__ plane_b) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint4 q0 = hits[4 * (size_t)i], q1 = hits[4 * (size_t)i + 1], q2 = hits[4 * (size_t)i + 2];
    const float t = __uint_as_float(q0.x);
    const uint32_t kind = q2.w;
    float4 a, b;
    if (kind != 0u) {
        const float u = __uint_as_float(q1.w), v = __uint_as_float(q2.x);
        const uint32_t mi = min(q2.y, ka.material_count - 1u);
        const f4 c = decode_texel(fetch_texture(ka, ka.materials[mi].texture_index, u, v), ka.srgb);
        a = make_float4(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z), t);
        b = make_float4(c.x, c.y, c.z, 1.0f);
    } else {
        const float4 dr = rays[2 * (size_t)i + 1];
        const f4 c = sample_env(ka, ka.srgb, mk(dr.x, dr.y, dr.z));
        a = make_float4(0.0f, 0.0f, 0.0f, kF32Max);
        b = make_float4(c.x, c.y, c.z, 0.0f);
    }
    plane_a[(size_t)first + i] = a;
    plane_b[(size_t)first + i] = b;
}

hipError_t rt_launch_feature_rays(const KernelArgs& ka, uint32_t first, uint32_t count, void* rays,
                                  hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_feature_rays_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, ka, first, count,
                       static_cast<float4*>(rays));
    return hipGetLastError();
}

hipError_t rt_launch_feature_resolve(const KernelArgs& ka, uint32_t first, uint32_t count, const void* rays,
                                     const void* hits, float4* plane_a, float4* plane_b, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_feature_resolve_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, ka, first, count,
                       static_cast<const float4*>(rays), static_cast<const uint4*>(hits), plane_a, plane_b);
    return hipGetLastError();
}

// ---- the filter ----------------------------------------------------------------------------------

struct DenoiseArgs {
    const float4* __restrict__ nd;    // plane A: normal.xyz, t
    const float4* __restrict__ ah;    // plane B: albedo.rgb, hit
    const float4* __restrict__ src;   // this iteration's input colour
    float4* __restrict__ dst;         // its result
    uint32_t* __restrict__ packed;    // the last pass: clamp01 + pack of the result; else null
    uint32_t width, height;
    uint32_t step;
    float k_a, k_c, sigma_depth;
};

namespace {

struct Px {
    float4 nd, ah, c;
};

// The weight of tap q for centre p, without the kernel factor h[dy]*h[dx] (`hh`) folded in any
// other order than the contract's: (((hh * g) * (ra*ra)) * (rc*rc)).
__device__ __forceinline__ float tap_weight(const Px& p, const Px& q, float hh, const DenoiseArgs& a) {
    float g;
    const bool hp = p.ah.w != 0.0f, hq = q.ah.w != 0.0f;
    if (!hp && !hq) {
        g = 1.0f;
    } else if (hp != hq) {
        g = 0.0f;
    } else {
        const float dn = (p.nd.x * q.nd.x + p.nd.y * q.nd.y) + p.nd.z * q.nd.z;
        const float d = dn > 0.0f ? dn : 0.0f;
        const float d2 = d * d, d4 = d2 * d2, d8 = d4 * d4, d16 = d8 * d8, wn = d16 * d16;
        const float x = __builtin_fabsf(p.nd.w - q.nd.w) / (a.sigma_depth * (p.nd.w + q.nd.w) + 1e-30f);
        const float wz = 1.0f / (1.0f + x * x);
        g = wn * wz;
    }
    const float ar = p.ah.x - q.ah.x, ag = p.ah.y - q.ah.y, ab = p.ah.z - q.ah.z;
    const float xa = ((ar * ar + ag * ag) + ab * ab) * a.k_a;
    const float ra = 1.0f / (1.0f + xa);
    const float cr = p.c.x - q.c.x, cg = p.c.y - q.c.y, cb = p.c.z - q.c.z;
    const float xc = ((cr * cr + cg * cg) + cb * cb) * a.k_c;
    const float rc = 1.0f / (1.0f + xc);
    return ((hh * g) * (ra * ra)) * (rc * rc);
}

__device__ __forceinline__ void store_result(const DenoiseArgs& a, size_t idx, float4 num, float den) {
    const float4 r = make_float4(num.x / den, num.y / den, num.z / den, num.w / den);
    a.dst[idx] = r;
    if (a.packed) a.packed[idx] = pack_rgba8(clamp01(r.x), clamp01(r.y), clamp01(r.z), clamp01(r.w));
}

}  // namespace

// One a-trous iteration. kLds: the three planes' tile + halo (2*step pixels) staged in LDS.
template <bool kLds>
__global__ void __launch_bounds__(kThreads) rt_denoise_pass_kernel(DenoiseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 tile[];
    const uint32_t tid = threadIdx.x;
    const uint32_t tx = tid & (kTileW - 1u), ty = tid / kTileW;
    const int x = (int)(blockIdx.x * kTileW + tx), y = (int)(blockIdx.y * kTileH + ty);
    const int w = (int)a.width, h = (int)a.height, s = (int)a.step;
    const int halo = 2 * s;
    const uint32_t pitch = kTileW + 2u * (uint32_t)halo, rows = kTileH + 2u * (uint32_t)halo;
    const uint32_t plane = pitch * rows;
    if constexpr (kLds) {
        const int x0 = (int)(blockIdx.x * kTileW) - halo, y0 = (int)(blockIdx.y * kTileH) - halo;
        for (uint32_t i = tid; i < plane; i += kThreads) {
            const uint32_t ly = i / pitch, lx = i - ly * pitch;
            const int gx = x0 + (int)lx, gy = y0 + (int)ly;
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {  // texels outside the image are never read
                const size_t gi = (size_t)gy * a.width + (size_t)gx;
                tile[i] = ld_f4(a.nd, gi);
                tile[plane + i] = ld_f4(a.ah, gi);
                tile[2u * plane + i] = ld_f4(a.src, gi);
            }
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;
    const size_t idx = (size_t)y * a.width + (size_t)x;
    auto load = [&](int qx, int qy, int dx, int dy) {
        Px q;
        if constexpr (kLds) {
            const uint32_t li = (uint32_t)((int)ty + halo + s * dy) * pitch + (uint32_t)((int)tx + halo + s * dx);
            q.nd = tile[li];
            q.ah = tile[plane + li];
            q.c = tile[2u * plane + li];
        } else {
            const size_t qi = (size_t)qy * a.width + (size_t)qx;
            q.nd = ld_f4(a.nd, qi);
            q.ah = ld_f4(a.ah, qi);
            q.c = ld_f4(a.src, qi);
        }
        return q;
    };
    const Px p = load(x, y, 0, 0);
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float4 num = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float den = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float hh = hk[dy + 2] * hk[dx + 2];
            float wgt;
            float4 c;
            if (dx == 0 && dy == 0) {
                wgt = hh;
                c = p.c;
            } else {
                const int qx = x + s * dx, qy = y + s * dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const Px q = load(qx, qy, dx, dy);
                wgt = tap_weight(p, q, hh, a);
                if (!(wgt > 0.0f)) continue;
                c = q.c;
            }
            num.x = num.x + wgt * c.x;
            num.y = num.y + wgt * c.y;
            num.z = num.z + wgt * c.z;
            num.w = num.w + wgt * c.w;
            den = den + wgt;
        }
    }
    store_result(a, idx, num, den);
}

// c0 = accumulation / D into the first colour plane; with `packed` (iterations == 0) also its pack.
__global__ void __launch_bounds__(256) rt_denoise_init_kernel(const float4* __restrict__ accum, float4* __restrict__ dst,
                                                              uint32_t* __restrict__ packed, uint64_t n, float div) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 v = accum[i];
    const float4 r = make_float4(v.x / div, v.y / div, v.z / div, v.w / div);
    dst[i] = r;
    if (packed) packed[i] = pack_rgba8(clamp01(r.x), clamp01(r.y), clamp01(r.z), clamp01(r.w));
}

hipError_t rt_launch_denoise_init(const float4* accum, float4* dst, uint32_t* packed, uint64_t n, float div,
                                  hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_denoise_init_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, accum, dst,
                       packed, n, div);
    return hipGetLastError();
}

// LDS bytes of a tiled pass at this step (the passes with step <= 2 may be tiled).
size_t rt_denoise_tile_bytes(uint32_t step) {
    return 3u * (size_t)(kTileW + 4u * step) * (kTileH + 4u * step) * sizeof(float4);
}

hipError_t rt_launch_denoise_pass(const float4* nd, const float4* ah, const float4* src, float4* dst, uint32_t* packed,
                                  uint32_t width, uint32_t height, uint32_t step, float k_a, float k_c,
                                  float sigma_depth, bool lds, hipStream_t stream) {
    const DenoiseArgs a{nd, ah, src, dst, packed, width, height, step, k_a, k_c, sigma_depth};
    const dim3 grid((width + kTileW - 1u) / kTileW, (height + kTileH - 1u) / kTileH);
    if (lds && step <= 2u)
        hipLaunchKernelGGL(rt_denoise_pass_kernel<true>, grid, dim3(kThreads), rt_denoise_tile_bytes(step), stream, a);
    else
        hipLaunchKernelGGL(rt_denoise_pass_kernel<false>, grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}
