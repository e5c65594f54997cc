// denoise.hip -- first-hit feature buffers, the guided a-trous filter and its temporal
// reprojection stage for gfx950 (rt_compute_features, rt_denoise, rt_denoise_temporal,
// rt_denoise_temporal_motion).
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
//
// THE TEMPORAL STAGE (rt_denoise_temporal; tests/temporal_ref.py restates it from here).
//
// Everything is f32, one IEEE operation per written operation, in the written order, with no
// contraction and correctly rounded division. W and H are (float)width and (float)height.
//
// Per pixel p = (x, y):
//
// 1. Current estimate.
//   c = accumulation(p) / D on all four channels;
//   N = (float)((k-1)*compute_per_frame), exactly the c0 and N of rt_denoise (D is N);
//   (o, d) is the pixel's un-jittered ray as rt_pick defines it;
//   n_p, t_p and hit_p come from the feature planes.
//
// 2. World point.
//   Hit: X_p = o + d*t_p per component (one multiply, one add), and wv = 1.
//   Miss: X_p = d, and wv = 0.
//
// 3. Projection through the previous slot's matrix M. This step runs only if a previous slot exists.
//   For rows i = 0, 1, 3: c_i = (M[i]*X.x + M[4+i]*X.y) + M[8+i]*X.z. On a hit, c_i = c_i + M[12+i] follows.
//   There is no history unless c_3 > 0.
//   fx = c_0/c_3 and fy = c_1/c_3.
//   There is no history unless fx > -1 && fx < W && fy > -1 && fy < H. Every one of these tests is false for NaN.
//
// 4. Bilinear taps.
//   x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0, bx = 1 - ax, by = 1 - ay.
//   The taps q, in this order:
//     (x0, y0) with w = bx*by;
//     (x0+1, y0) with w = ax*by;
//     (x0, y0+1) with w = bx*ay;
//     (x0+1, y0+1) with w = ax*ay.
//   A tap counts only if q is inside the image, w > 0, and hit_q == hit_p.
//   On a hit, two further tests apply:
//     the normal: (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_min;
//     the position: e2 <= (sigma_position*sigma_position) * r2, with
//       e = X_p - X_q,
//       e2 = (e.x*e.x + e.y*e.y) + e.z*e.z,
//       f = X_p - o,
//       r2 = (f.x*f.x + f.y*f.y) + f.z*f.z.
//   Misses need nothing further.
//
// 5. History sums.
//   sw = sw + w, hc = hc + w*C_q (per channel) and hn = hn + w*n_q, in tap order starting from 0.
//   There is no history unless sw > 0.
//   Otherwise h = hc/sw and nh = min(hn/sw, (float)max_history).
//
// 6. Blend.
//   Without history: out = c and n_out = N.
//   With history: tot = nh + N, a = N/tot, out = h + (c - h)*a per channel, and n_out = tot.
//
// 7. Store. The current slot gets C = out, X = (X_p, hit_p) and Nn = (n_p, n_out). Its matrix becomes
//   params->world_to_pixel and its tag becomes G.
//
// 8. Filter. The a-trous iterations of rt_denoise run on c0 := out. The colour scale is per pixel:
//   s_i = sigma_color * 0.5f^i (exact scaling);
//   K_i = 1.0f/(s_i*s_i);
//   k_c(p) = n_out(p) * K_i, using the centre pixel's count.
//   Everything else is word for word the pass above. iterations == 0 gives out and its pack.
//
// Because k_c rounds differently (n_out*K_i here, 1/(s_i*s_i) with s0 = sigma_color/sqrtf(N) above), a
// call without history is close to rt_denoise of the same frame but is not promised bit-equal.
// End of the temporal contract.
//
// The temporal kernel: one pixel per lane over the same 32x8 tile, 256-thread workgroups. The camera
// block of pixel_ray is read from the kernel arguments (scalar registers), so there is no LDS and no
// barrier; the instance is chosen by where the camera ray comes from (ray buffer or matrices). Every
// plane access is a 16-B vector load or store: 16 B of accumulation, 32 B of features (and 16 B of
// ray buffer in that instance), then for a pixel that reprojects on screen 4 x 48 B gathered from
// the previous slot -- neighbouring pixels reproject to neighbouring taps, so a wave's gathers
// fall into a few rows -- and 48 B written to the current slot. The two slots are distinct buffers:
// no hazard, no atomics. The four taps' loads are issued together (indices clamped into the image)
// and the invalid ones dropped with selects, never multiplied by zero.
//
// THE MOTION STAGE (rt_denoise_temporal_motion; tests/temporal_motion_ref.py restates it from here).
//
// This is the temporal contract above, word for word, with the changes below. Everything is f32, one
// IEEE operation per written operation, in the written order, with no contraction.
//
// 2m. Record lookup.
//   id_p comes from the ID plane.
//   The record R is objects[id.y] if id.x == 2 && id.y < object_count.
//   R is spheres[id.y] if id.x == 1 && id.y < sphere_count.
//   Otherwise there is no record. Misses never have one.
//   X_p is as in step 2.
//   If R has DROP, the pixel has no history.
//   If R has MOVED, for i = 0..2:
//     Y_i = ((m[4i]*X.x + m[4i+1]*X.y) + m[4i+2]*X.z) + m[4i+3];
//     g_i = ((m[4i]*n.x + m[4i+1]*n.y) + m[4i+2]*n.z) * normal_scale.
//   Otherwise Y = X_p and g = n_p, chosen by selection. The pixel does no arithmetic.
//
// 3m. Projection. Step 3 projects Y instead of X_p.
//
// 4m. Tap tests.
//   The tap tests are those of step 4, with g in the normal test and e = Y - X_q in the position test.
//   f = X_p - o and r2 are unchanged. The tolerance scales with the current distance.
//   On a hit, and only when the previous slot has an I plane, one further test applies: both words of
//   I_q equal id_p.
//
// 7m. Store. Store as step 7: X = (X_p, hit_p) and Nn = (n_p, n_out). In addition I = id_p.
//
// Steps 1, 5, 6 and 8 are unchanged.
// End of the motion contract.
//
// The motion instance (kMotion) of the temporal kernel adds, per pixel: 8 B of ID plane, one guarded
// 64-B record gather (four 16-B loads; neighbouring pixels share ids, so the lanes of a wave mostly
// read one and the same record), 4 x 8 B of I taps issued with the other tap loads (indices clamped,
// dropped by selects) and 8 B of I written. The instances without it compile to the code they had
// before it existed (profiles/temporal_motion/kernel_regs.txt).
// The ID plane: rt_feature_resolve_kernel stores (rt_hit.kind, rt_hit.index) of the record planes A
// and B are resolved from, (0, 0) on a miss: one extra 8-B store per pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
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

// rt_hit records of pixels [first, first + count) -> the two feature planes and the ID plane.
__global__ void __launch_bounds__(256) rt_feature_resolve_kernel(KernelArgs ka, uint32_t first, uint32_t count,
                                                                 const float4* __restrict__ rays,
                                                                 const uint4* __restrict__ hits,
                                                                 float4* __restrict__ plane_a,
                                                                 float4* __restrict__ plane_b,
                                                                 uint2* __restrict__ plane_i) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint4 q0 = hits[4 * (size_t)i], q1 = hits[4 * (size_t)i + 1], q2 = hits[4 * (size_t)i + 2];
    const float t = __uint_as_float(q0.x);
    const uint32_t kind = q2.w;
    float4 a, b;
    uint2 id = make_uint2(0u, 0u);
    if (kind != 0u) {
        id = make_uint2(kind, reinterpret_cast<const uint32_t*>(hits)[16 * (size_t)i + 12]);  // rt_hit.index
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
    plane_i[(size_t)first + i] = id;
}

hipError_t rt_launch_feature_rays(const KernelArgs& ka, uint32_t first, uint32_t count, void* rays,
                                  hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_feature_rays_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, ka, first, count,
                       static_cast<float4*>(rays));
    return hipGetLastError();
}

hipError_t rt_launch_feature_resolve(const KernelArgs& ka, uint32_t first, uint32_t count, const void* rays,
                                     const void* hits, float4* plane_a, float4* plane_b, uint2* plane_i,
                                     hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_feature_resolve_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, ka, first, count,
                       static_cast<const float4*>(rays), static_cast<const uint4*>(hits), plane_a, plane_b, plane_i);
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
    const float4* __restrict__ nn;    // kPix (rt_denoise_temporal): the current slot's Nn plane, k_c(p) = nn(p).w * k_c
};

namespace {

struct Px {
    float4 nd, ah, c;
};

// The weight of tap q for centre p, without the kernel factor h[dy]*h[dx] (`hh`) folded in any
// other order than the contract's: (((hh * g) * (ra*ra)) * (rc*rc)).
__device__ __forceinline__ float tap_weight(const Px& p, const Px& q, float hh, const DenoiseArgs& a, float k_c) {
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
    const float xc = ((cr * cr + cg * cg) + cb * cb) * k_c;
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
// kPix: the temporal filter's per-pixel colour scale (one extra scalar load at the centre pixel).
template <bool kLds, bool kPix>
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
    float k_c = a.k_c;
    if constexpr (kPix) k_c = reinterpret_cast<const float*>(a.nn)[4u * idx + 3u] * a.k_c;
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
                wgt = tap_weight(p, q, hh, a, k_c);
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
                                  float sigma_depth, bool lds, hipStream_t stream, const float4* nn) {
    const DenoiseArgs a{nd, ah, src, dst, packed, width, height, step, k_a, k_c, sigma_depth, nn};
    const dim3 grid((width + kTileW - 1u) / kTileW, (height + kTileH - 1u) / kTileH);
    const bool tiled = lds && step <= 2u;
    const size_t bytes = tiled ? rt_denoise_tile_bytes(step) : 0;
    if (nn) {  // rt_denoise_temporal: k_c is K_i, scaled per pixel by nn(p).w
        if (tiled)
            hipLaunchKernelGGL((rt_denoise_pass_kernel<true, true>), grid, dim3(kThreads), bytes, stream, a);
        else
            hipLaunchKernelGGL((rt_denoise_pass_kernel<false, true>), grid, dim3(kThreads), bytes, stream, a);
    } else if (tiled) {
        hipLaunchKernelGGL((rt_denoise_pass_kernel<true, false>), grid, dim3(kThreads), bytes, stream, a);
    } else {
        hipLaunchKernelGGL((rt_denoise_pass_kernel<false, false>), grid, dim3(kThreads), bytes, stream, a);
    }
    return hipGetLastError();
}

// ---- the temporal stage --------------------------------------------------------------------------

struct TemporalArgs {
    const float4* __restrict__ accum;
    const float4* __restrict__ nd;      // plane A: normal.xyz, t
    const float4* __restrict__ ah;      // plane B: albedo.rgb, hit
    const float4* __restrict__ prev_c;  // the previous slot's planes; null: there is none
    const float4* __restrict__ prev_x;
    const float4* __restrict__ prev_nn;
    float4* __restrict__ cur_c;         // the current slot's planes
    float4* __restrict__ cur_x;
    float4* __restrict__ cur_nn;
    float4* __restrict__ dn;            // iterations == 0: `out` and its pack as the denoised result; else null
    uint32_t* __restrict__ packed;
    float m[16];                        // the previous slot's world_to_pixel
    float n;                            // N = D
    float max_history, sigma2, normal_min;  // (float)max_history, sigma_position*sigma_position
    // kMotion (rt_denoise_temporal_motion) only; the plain instances never read past this line
    const uint2* __restrict__ ids;      // the ID plane: rt_hit.kind, rt_hit.index
    const uint2* __restrict__ prev_i;   // the previous slot's I plane; null: that slot has no ids
    uint2* __restrict__ cur_i;          // the current slot's I plane
    const float4* __restrict__ objects; // motion records, four float4 each: m[0..3], m[4..7], m[8..11],
    const float4* __restrict__ spheres; //   (normal_scale, flags, 0, 0)
    uint32_t object_count, sphere_count;
};

namespace {

// Step 2m: the motion record of the primitive (kind, index), or a static one (flags 0) where the
// tables have none. The index is used only behind its bounds test.
__device__ __forceinline__ void load_motion(const TemporalArgs& t, uint32_t kind, uint32_t index, float4 (&r)[4]) {
    const bool obj = kind == 2u && index < t.object_count, sph = kind == 1u && index < t.sphere_count;
    r[0] = r[1] = r[2] = r[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (obj || sph) {
        const float4* __restrict__ rec = (obj ? t.objects : t.spheres) + 4u * (size_t)index;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = rec[k];
    }
}

}  // namespace

// Steps 1-7 of the temporal contract. kGen: the camera ray is computed from the matrices
// (rt_update_camera_matrices in effect); else it is read from the ray buffer. kMotion: the motion
// contract's steps 2m, 3m, 4m and 7m (rt_denoise_temporal_motion); the instances without it hold
// none of that code.
template <bool kGen, bool kMotion>
__global__ void __launch_bounds__(kThreads) rt_temporal_kernel(KernelArgs ka, TemporalArgs t) {
    const uint32_t tid = threadIdx.x;
    const uint32_t x = blockIdx.x * kTileW + (tid & (kTileW - 1u)), y = blockIdx.y * kTileH + tid / kTileW;
    if (x >= ka.width || y >= ka.height) return;
    const int w = (int)ka.width, h = (int)ka.height;
    const size_t idx = (size_t)y * ka.width + (size_t)x;
    // 1. current estimate
    const float4 acc = ld_f4(t.accum, idx);
    const float4 c = make_float4(acc.x / t.n, acc.y / t.n, acc.z / t.n, acc.w / t.n);
    const float4 nd = ld_f4(t.nd, idx);
    const float hit_p = ld_f4(t.ah, idx).w;
    const bool hit = hit_p != 0.0f;
    f3 d;
    if constexpr (kGen) {
        float cam[33];  // constant indices into the kernel arguments: scalar registers, not scratch
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            cam[i] = ka.inv_proj[i];
            cam[16 + i] = ka.inv_view[i];
        }
        cam[32] = ka.aspect;
        d = camera_ray(ka, cam, x, y);
    } else {
        const float4 cr = ld_f4(ka.camera_rays, idx);
        d = mk(cr.x, cr.y, cr.z);
    }
    const f3 o = mk(ka.camera_origin[0], ka.camera_origin[1], ka.camera_origin[2]);
    // 2. world point
    const f3 xp = hit ? mk(o.x + d.x * nd.w, o.y + d.y * nd.w, o.z + d.z * nd.w) : d;
    float4 out = c;
    float n_out = t.n;
    // 2m. the record of this pixel's primitive: yp and g are X_p and n_p carried to the previous call
    f3 yp = xp, g = mk(nd.x, nd.y, nd.z);
    uint2 id = make_uint2(0u, 0u);
    bool keep = true;
    if constexpr (kMotion) {
        id = t.ids[idx];
        // neighbouring pixels share ids: the lanes of a wave mostly gather one and the same 64 B
        float4 r[4];
        load_motion(t, id.x, id.y, r);
        const uint32_t flags = __float_as_uint(r[3].y);
        const float ns = r[3].x;
        const f3 ym = mk(((r[0].x * xp.x + r[0].y * xp.y) + r[0].z * xp.z) + r[0].w,
                         ((r[1].x * xp.x + r[1].y * xp.y) + r[1].z * xp.z) + r[1].w,
                         ((r[2].x * xp.x + r[2].y * xp.y) + r[2].z * xp.z) + r[2].w);
        const f3 gm = mk(((r[0].x * nd.x + r[0].y * nd.y) + r[0].z * nd.z) * ns,
                         ((r[1].x * nd.x + r[1].y * nd.y) + r[1].z * nd.z) * ns,
                         ((r[2].x * nd.x + r[2].y * nd.y) + r[2].z * nd.z) * ns);
        const bool moved = (flags & 1u) != 0u;
        yp = mk(moved ? ym.x : xp.x, moved ? ym.y : xp.y, moved ? ym.z : xp.z);  // per component: registers
        g = mk(moved ? gm.x : nd.x, moved ? gm.y : nd.y, moved ? gm.z : nd.z);
        keep = (flags & 2u) == 0u;
    }
    if (t.prev_c && keep) {
        // 3. projection
        float c0 = (t.m[0] * yp.x + t.m[4] * yp.y) + t.m[8] * yp.z;
        float c1 = (t.m[1] * yp.x + t.m[5] * yp.y) + t.m[9] * yp.z;
        float c3 = (t.m[3] * yp.x + t.m[7] * yp.y) + t.m[11] * yp.z;
        if (hit) {
            c0 = c0 + t.m[12];
            c1 = c1 + t.m[13];
            c3 = c3 + t.m[15];
        }
        const float fx = c0 / c3, fy = c1 / c3;
        if (c3 > 0.0f && fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h) {
            // 4. bilinear taps: fx in (-1, W) puts x0 in [-1, W-1]; indices are clamped into the
            // image so that all loads can be issued, and `inside` drops the clamped ones
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float ax = fx - x0, ay = fy - y0, bx = 1.0f - ax, by = 1.0f - ay;
            const int ix = (int)x0, iy = (int)y0;
            const float wt[4] = {bx * by, ax * by, bx * ay, ax * ay};
            float4 qc[4], qx[4], qn[4];
            uint2 qid[4];
            bool inside[4];
            bool with_ids = false;
            if constexpr (kMotion) with_ids = t.prev_i != nullptr;  // uniform: a kernel argument
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qxi = ix + (k & 1), qyi = iy + (k >> 1);
                inside[k] = qxi >= 0 && qxi < w && qyi >= 0 && qyi < h;
                const int cx = min(max(qxi, 0), w - 1), cy = min(max(qyi, 0), h - 1);
                const size_t qi = (size_t)cy * ka.width + (size_t)cx;
                qc[k] = ld_f4(t.prev_c, qi);
                qx[k] = ld_f4(t.prev_x, qi);
                qn[k] = ld_f4(t.prev_nn, qi);
                if constexpr (kMotion) {
                    qid[k] = make_uint2(id.x, id.y);  // a slot without ids hands back id itself
                    if (with_ids) qid[k] = t.prev_i[qi];
                }
            }
            const float fx_ = xp.x - o.x, fy_ = xp.y - o.y, fz_ = xp.z - o.z;
            const float r2 = (fx_ * fx_ + fy_ * fy_) + fz_ * fz_;
            const float lim = t.sigma2 * r2;
            float sw = 0.0f, hn = 0.0f;
            float4 hc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool ok = inside[k] && wt[k] > 0.0f && qx[k].w == hit_p;
                if (hit) {
                    const float dn = (g.x * qn[k].x + g.y * qn[k].y) + g.z * qn[k].z;
                    const float ex = yp.x - qx[k].x, ey = yp.y - qx[k].y, ez = yp.z - qx[k].z;
                    const float e2 = (ex * ex + ey * ey) + ez * ez;
                    ok = ok && dn >= t.normal_min && e2 <= lim;
                    // 4m. a slot without ids hands back id itself
                    if constexpr (kMotion) ok = ok && qid[k].x == id.x && qid[k].y == id.y;
                }
                // 5. history sums
                sw = ok ? sw + wt[k] : sw;
                hc.x = ok ? hc.x + wt[k] * qc[k].x : hc.x;
                hc.y = ok ? hc.y + wt[k] * qc[k].y : hc.y;
                hc.z = ok ? hc.z + wt[k] * qc[k].z : hc.z;
                hc.w = ok ? hc.w + wt[k] * qc[k].w : hc.w;
                hn = ok ? hn + wt[k] * qn[k].w : hn;
            }
            if (sw > 0.0f) {
                // 6. blend
                const float4 hh = make_float4(hc.x / sw, hc.y / sw, hc.z / sw, hc.w / sw);
                const float nq = hn / sw;
                const float nh = nq < t.max_history ? nq : t.max_history;
                const float tot = nh + t.n;
                const float a = t.n / tot;
                out = make_float4(hh.x + (c.x - hh.x) * a, hh.y + (c.y - hh.y) * a, hh.z + (c.z - hh.z) * a,
                                  hh.w + (c.w - hh.w) * a);
                n_out = tot;
            }
        }
    }
    // 7. store
    t.cur_c[idx] = out;
    t.cur_x[idx] = make_float4(xp.x, xp.y, xp.z, hit_p);
    t.cur_nn[idx] = make_float4(nd.x, nd.y, nd.z, n_out);
    if constexpr (kMotion) t.cur_i[idx] = id;
    if (t.dn) {
        t.dn[idx] = out;
        t.packed[idx] = pack_rgba8(clamp01(out.x), clamp01(out.y), clamp01(out.z), clamp01(out.w));
    }
}

hipError_t rt_launch_temporal(const KernelArgs& ka, const float4* accum, const float4* nd, const float4* ah,
                              float4* const prev[3], float4* const cur[3], const float* prev_matrix, float4* dn,
                              uint32_t* packed, float n, float max_history, float sigma2, float normal_min,
                              hipStream_t stream, const TemporalMotion* motion) {
    TemporalArgs t{};
    t.accum = accum;
    t.nd = nd;
    t.ah = ah;
    if (prev) {
        t.prev_c = prev[0];
        t.prev_x = prev[1];
        t.prev_nn = prev[2];
        for (int i = 0; i < 16; ++i) t.m[i] = prev_matrix[i];
    }
    t.cur_c = cur[0];
    t.cur_x = cur[1];
    t.cur_nn = cur[2];
    t.dn = dn;
    t.packed = packed;
    t.n = n;
    t.max_history = max_history;
    t.sigma2 = sigma2;
    t.normal_min = normal_min;
    const dim3 grid((ka.width + kTileW - 1u) / kTileW, (ka.height + kTileH - 1u) / kTileH);
    if (motion) {  // rt_denoise_temporal_motion
        t.ids = motion->ids;
        t.prev_i = prev ? motion->prev_i : nullptr;
        t.cur_i = motion->cur_i;
        t.objects = motion->objects;
        t.spheres = motion->spheres;
        t.object_count = motion->object_count;
        t.sphere_count = motion->sphere_count;
        if (ka.gen_rays)
            hipLaunchKernelGGL((rt_temporal_kernel<true, true>), grid, dim3(kThreads), 0, stream, ka, t);
        else
            hipLaunchKernelGGL((rt_temporal_kernel<false, true>), grid, dim3(kThreads), 0, stream, ka, t);
    } else if (ka.gen_rays) {
        hipLaunchKernelGGL((rt_temporal_kernel<true, false>), grid, dim3(kThreads), 0, stream, ka, t);
    } else {
        hipLaunchKernelGGL((rt_temporal_kernel<false, false>), grid, dim3(kThreads), 0, stream, ka, t);
    }
    return hipGetLastError();
}
