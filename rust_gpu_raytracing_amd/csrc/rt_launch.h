// rt_launch.h — what the translation units of the library call in one another: the kernel
// launchers and launch queries that the .hip files define for the host files (rt_abi.cpp,
// rt_frames.cpp, rt_queries.cpp, rt_post.cpp; rt_ctx.h is what those share), and rt_abi.cpp's
// rt_set_global_error. Every file that defines one of these includes this header, so a signature
// that drifts is seen where it is defined, and the library is linked with --no-undefined, so one
// that is declared and called but nowhere defined fails the build.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_kernel_args.h"
#include "rt_query_schedule.h"
#include "rt_scene_math.h"
#include "sphere_bvh.h"
#include "tri_cone.h"
#include "tri_qnode.h"

// rt_abi.cpp, for scene_build.cpp and rt_multi.cpp: the last error of a call without a context, rt_last_error(NULL)
void rt_set_global_error(const std::string& msg);

// pathtrace.hip, for rt_frames.cpp (the self-test: rt_abi.cpp)
hipError_t rt_launch_math_selftest(uint32_t which, unsigned long long* mismatches, uint32_t* first_bad,
                                   hipStream_t stream);
hipError_t rt_launch_pathtrace(const KernelArgs& ka, int mode, bool tris, bool frame_par, uint32_t threads,
                               size_t lds_bytes, uint32_t blocks, hipStream_t stream);
hipError_t rt_pathtrace_pick_config(int mode, bool tris, bool frame_par, size_t lds_bytes,
                                    size_t lds_bytes_per_thread, uint32_t force_threads, uint32_t waves_cap,
                                    uint32_t* threads, int* blocks_per_cu);
hipError_t rt_launch_primary(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, uint32_t threads,
                             uint32_t min_waves, hipStream_t stream);
hipError_t rt_launch_brute_wf(const KernelArgs& ka, bool tris, bool scalar_stream, size_t lds_bytes, uint32_t blocks,
                              hipStream_t stream);
size_t rt_brute_wf_tile_bytes(bool scalar_stream);
uint32_t rt_brute_wf_chunk();
hipError_t rt_launch_resolve(float4* accum, uint32_t* output, const float4* light, uint32_t width, uint32_t height,
                             uint32_t tiles_x, uint32_t owned_tiles, uint32_t rank, uint32_t world, uint32_t k0,
                             uint32_t samples, uint32_t frames, unsigned long long* clock, hipStream_t stream);
hipError_t rt_launch_pack_output(uint32_t* output, uint32_t* packed, uint32_t width, uint32_t height, uint32_t tiles_x,
                                 uint32_t n_tiles, uint32_t first_rank, uint32_t ranks, uint32_t world,
                                 uint64_t stride_px, uint32_t skip_rank, bool unpack, hipStream_t stream);
hipError_t rt_launch_pack(const float4* accum, float4* dst, uint32_t width, uint32_t height, uint32_t tiles_x,
                          uint32_t owned_tiles, uint32_t rank, uint32_t world, hipStream_t stream);
hipError_t rt_launch_unpack(const float4* src, float4* accum, uint32_t* output, uint32_t width, uint32_t height,
                            uint32_t tiles_x, uint32_t n_tiles, uint32_t first_rank, uint32_t ranks, uint32_t world,
                            uint64_t stride_px, uint32_t skip_rank, float divisor, hipStream_t stream);

// scene_edit.hip, for rt_abi.cpp (edit, refit) and rt_frames.cpp (what the triangle walks read, derived)
hipError_t rt_launch_edit(const float* model, const uint32_t* tri_object, const uint32_t* sub_object,
                          const uint2* object_tris, const rt_scene::Placement* place, uint32_t object_count,
                          uint32_t n_tri, uint32_t n_sub, RtTriangleHot* tris, float4* bounds, RtSubObject* subs,
                          RtObject* objects, hipStream_t stream);
hipError_t rt_launch_quantize_tri_nodes(const SphereBvhNode* nodes, uint32_t n, const uint32_t* src,
                                        const uint32_t* skip, uint32_t n_out, SphereBvhNode* out32, uint4* q,
                                        float4* grid, hipStream_t stream);
hipError_t rt_launch_refit(SphereBvhNode* nodes, const SubObjectPrim* prims, const RtSubObject* subs,
                           const uint32_t* order, const uint32_t* level_offsets, uint32_t n_levels, float* extent_out,
                           hipStream_t stream);
hipError_t rt_launch_tri_leafcert(const SubObjectPrim* prims, uint32_t n_prims, const RtSubObject* subs,
                                  const RtTriangleHot* tris, uint32_t n_tri, TriLeafCert* out, hipStream_t stream);
hipError_t rt_launch_tri_leaftris(const SubObjectPrim* prims, uint32_t n_prims, const RtTriangleHot* tris,
                                  uint32_t n_tri, uint4* out, hipStream_t stream);

// the query kernels (query.hip, occlusion.hip, radiance.hip, ambient.hip), for rt_queries.cpp: per kernel the workgroup size of a
// placement, the resident workgroups per CU, and the launch on a schedule of rt_query_schedule.h
uint32_t rt_query_threads(int mode, bool tris);
hipError_t rt_query_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_query(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                           const void* rays, void* hits, uint64_t count, unsigned long long* counter,
                           hipStream_t stream);
hipError_t rt_launch_pick_ray(const KernelArgs& ka, uint32_t x, uint32_t y, void* ray_out, hipStream_t stream);
uint32_t rt_occlusion_threads(int mode, bool tris);
hipError_t rt_occlusion_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_occlusion(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                               const void* rays, void* occluded, uint64_t count, unsigned long long* counter,
                               hipStream_t stream);
// hits.hip: `counts` may be null; `pick`: the rays carry no t_max (rt_launch_pick_ray's record)
uint32_t rt_hits_threads(int mode, bool tris);
hipError_t rt_hits_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_hits(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                          const void* rays, void* hits, void* counts, uint64_t count, uint32_t max_hits, bool pick,
                          unsigned long long* counter, hipStream_t stream);
// nearest.hip: `sweep`: the instance that tests every candidate; `radius`: |radius| by original sphere
// index; `descend`: the walk instance makes its greedy descent before each walk
uint32_t rt_nearest_threads(int mode, bool tris);
hipError_t rt_nearest_occupancy(int mode, bool tris, bool sweep, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_nearest(const KernelArgs& ka, int mode, bool tris, bool sweep, size_t lds_bytes,
                             const rtq::QuerySchedule& s, const void* points, void* out, const float* radius,
                             bool descend, uint64_t count, unsigned long long* counter, hipStream_t stream);
uint32_t rt_radiance_threads(int mode, bool tris);
hipError_t rt_radiance_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_gather_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_probe_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_radiance(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                              const void* rays, void* radiance, uint64_t count, unsigned long long* counter,
                              unsigned long long* segments, uint32_t first_sample, uint32_t samples, uint32_t stripes,
                              hipStream_t stream);
hipError_t rt_launch_gather_resolve(const void* partials, void* radiance, uint32_t points, uint32_t stripes,
                                    hipStream_t stream);
hipError_t rt_launch_probe_paths(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                                 const void* probes, void* lights, uint64_t count, unsigned long long* counter,
                                 unsigned long long* segments, uint32_t first_sample, uint32_t samples,
                                 hipStream_t stream);
hipError_t rt_launch_probe_resolve(const void* lights, const void* probes, void* sh, uint32_t count, uint32_t first_sample,
                                   uint32_t samples, hipStream_t stream);
hipError_t rt_lens_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_lens_camera(const rt_lens_camera& cam, void* slot, hipStream_t stream);
hipError_t rt_launch_lens(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                          const void* cam, void* radiance, uint32_t first_pixel, uint64_t count,
                          unsigned long long* counter, unsigned long long* segments, uint32_t first_sample,
                          uint32_t samples, hipStream_t stream);
hipError_t rt_launch_lens_rays(const void* cam, void* rays, uint32_t first_pixel, uint64_t count, uint32_t u,
                               hipStream_t stream);
uint32_t rt_ambient_threads(int mode, bool tris);
hipError_t rt_ambient_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
hipError_t rt_launch_ambient(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                             const void* points, void* partials, uint64_t count, unsigned long long* counter,
                             uint32_t first_sample, uint32_t samples, uint32_t stripes, hipStream_t stream);

// denoise.hip, for rt_post.cpp
hipError_t rt_launch_feature_rays(const KernelArgs& ka, uint32_t first, uint32_t count, void* rays, hipStream_t stream);
hipError_t rt_launch_feature_resolve(const KernelArgs& ka, uint32_t first, uint32_t count, const void* rays,
                                     const void* hits, float4* plane_a, float4* plane_b, uint2* plane_i,
                                     hipStream_t stream);
hipError_t rt_launch_denoise_init(const float4* accum, float4* dst, uint32_t* packed, uint64_t n, float div,
                                  hipStream_t stream);
hipError_t rt_launch_denoise_pass(const float4* nd, const float4* ah, const float4* src, float4* dst, uint32_t* packed,
                                  uint32_t width, uint32_t height, uint32_t step, float k_a, float k_c,
                                  float sigma_depth, bool lds, hipStream_t stream, const float4* nn = nullptr);
// What rt_denoise_temporal_motion adds to a temporal launch: the ID plane, the slots' I planes
// (prev_i null: the previous slot was written without ids) and the motion tables, 64 B per record.
struct TemporalMotion {
    const uint2* ids;
    const uint2* prev_i;
    uint2* cur_i;
    const float4* objects;
    const float4* spheres;
    uint32_t object_count, sphere_count;
};
hipError_t rt_launch_temporal(const KernelArgs& ka, const float4* accum, const float4* nd, const float4* ah,
                              float4* const prev[3], float4* const cur[3], const float* prev_matrix, float4* dn,
                              uint32_t* packed, float n, float max_history, float sigma2, float normal_min,
                              hipStream_t stream, const TemporalMotion* motion = nullptr);

// display.hip, for rt_post.cpp
hipError_t rt_launch_display_meter(const float4* src, uint64_t n, float div, uint32_t* bins, hipStream_t stream);
hipError_t rt_launch_display_solve(uint32_t* bins, uint32_t* kept, uint32_t* state, uint32_t low_permille,
                                   uint32_t high_permille, float key, float min_exposure, float max_exposure,
                                   float adaptation, bool has_state, hipStream_t stream);
hipError_t rt_launch_display_tone(const float4* src, uint32_t* dst, uint64_t n, float div, const uint32_t* state,
                                  float exposure, float iw2, const float* srgb, uint32_t op, uint32_t encode,
                                  hipStream_t stream);
