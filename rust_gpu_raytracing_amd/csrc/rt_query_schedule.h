// rt_query_schedule.h -- how a ray-query launch is cut into workgroups and chunks of rays (host
// only, plain C++). One function for the four query paths, so that the
// arithmetic is written, and tested (tests/cpp/query_schedule.cpp), once.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace rtq {

constexpr uint64_t kNoChunkCap = UINT64_MAX;

// Rays per chunk of a radiance or gather launch: the cap of a wave's own first chunk and of the
// chunks the counter deals. A ray there is a whole path, so a chunk of consecutive rays is
// uniformly dear or cheap and larger chunks end the launch on the waves that drew the dear ones
// (DESIGN.md §5.4e has the measurement behind the values).
#ifndef RT_RADIANCE_FIRST_CHUNK_MAX
#define RT_RADIANCE_FIRST_CHUNK_MAX 128u
#endif
#ifndef RT_RADIANCE_CHUNK_MAX
#define RT_RADIANCE_CHUNK_MAX 128u
#endif
constexpr uint64_t kRadianceFirstChunkMax = RT_RADIANCE_FIRST_CHUNK_MAX;
constexpr uint64_t kRadianceChunkMax = RT_RADIANCE_CHUNK_MAX;
// The closest-hit and any-hit kernels' rays are single walks: dealt in chunks of at most 256.
constexpr uint64_t kWalkChunkMax = 256;

struct QuerySchedule {
    uint32_t blocks;       // workgroups launched: what the batch needs, at most what is resident
    uint32_t first_chunk;  // rays of each wave's own first chunk, taken without a claim (0: it has none)
    uint32_t rest_chunk;   // rays per claim from the counter, which deals the rays the first chunks leave
};

// The schedule of `count` >= 1 rays (or items) on a kernel of `waves_per_block` wave64s per
// workgroup, `resident_blocks` >= 1 of which the device holds at once.
//
// Each wave's own first chunk is about half the wave's share, rounded down to whole waves of rays,
// at least 64 and at most `first_chunk_max`: taken by the wave's index, because the resident waves'
// first claims would queue at one counter address (about 20 ns each) while nothing else runs. The
// counter deals the other half, which evens out what the first chunks cost, in chunks of about half
// a wave's share of it (two claims per wave), rounded up to whole waves of rays, at least 64 and at
// most `chunk_max`. A batch of at most one wave of rays per wave claims nothing.
// `first_chunk_max` 0: no own first chunks (the closest-hit kernel), every ray is dealt.
inline QuerySchedule query_schedule(uint64_t count, uint32_t waves_per_block, uint64_t resident_blocks,
                                    uint64_t first_chunk_max, uint64_t chunk_max) {
    const uint64_t per_block = 64ull * waves_per_block;
    const uint64_t wanted = (count + per_block - 1) / per_block;
    QuerySchedule s;
    s.blocks = (uint32_t)std::min<uint64_t>(wanted, resident_blocks);
    const uint64_t waves = (uint64_t)s.blocks * waves_per_block;
    s.first_chunk = first_chunk_max == 0
                        ? 0u
                        : (uint32_t)std::min<uint64_t>(first_chunk_max,
                                                       std::max<uint64_t>(64u, (count / waves / 2u) & ~63ull));
    const uint64_t rest = count > waves * s.first_chunk ? count - waves * s.first_chunk : 0;
    s.rest_chunk = (uint32_t)std::min<uint64_t>(chunk_max, std::max<uint64_t>(64u, (rest / (waves * 2u) + 63u) & ~63ull));
    return s;
}

}  // namespace rtq
