// CPU harness of csrc/rt_query_schedule.h (tests/test_query_schedule_cpu.py): query_schedule against
// the three formulas the query paths carried before they shared it, written out below as they
// stood in run_query (closest hit, any hit) and in run_radiance / run_gather.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "rt_query_schedule.h"

namespace {

struct Triple {
    uint32_t blocks, first_chunk, rest_chunk;
};

uint32_t blocks_of(uint64_t count, uint32_t waves_per_block, uint64_t resident) {
    const uint64_t wanted = (count + 64ull * waves_per_block - 1) / (64ull * waves_per_block);
    return (uint32_t)std::min<uint64_t>(wanted, resident);
}

// run_query, closest hit: rays per claim, about two claims per wave, whole waves of rays, at most 256
Triple closest_formula(uint64_t count, uint32_t waves_per_block, uint64_t resident) {
    const uint32_t blocks = blocks_of(count, waves_per_block, resident);
    const uint64_t per_wave = count / ((uint64_t)blocks * waves_per_block * 2u);
    const uint32_t wave_chunk = (uint32_t)std::min<uint64_t>(256u, std::max<uint64_t>(64u, (per_wave + 63u) & ~63ull));
    return {blocks, 0u, wave_chunk};
}

// run_query, any hit
Triple any_hit_formula(uint64_t count, uint32_t waves_per_block, uint64_t resident) {
    const uint32_t blocks = blocks_of(count, waves_per_block, resident);
    const uint64_t waves = (uint64_t)blocks * waves_per_block;
    const uint32_t first_chunk = (uint32_t)std::max<uint64_t>(64u, (count / waves / 2u) & ~63ull);
    const uint64_t rest = count > waves * first_chunk ? count - waves * first_chunk : 0;
    const uint32_t rest_chunk =
        (uint32_t)std::min<uint64_t>(256u, std::max<uint64_t>(64u, (rest / (waves * 2u) + 63u) & ~63ull));
    return {blocks, first_chunk, rest_chunk};
}

// run_radiance, and run_gather over items
Triple radiance_formula(uint64_t count, uint32_t waves_per_block, uint64_t resident, uint64_t first_max,
                        uint64_t chunk_max) {
    const uint32_t blocks = blocks_of(count, waves_per_block, resident);
    const uint64_t waves = (uint64_t)blocks * waves_per_block;
    const uint32_t first_chunk =
        (uint32_t)std::min<uint64_t>(first_max, std::max<uint64_t>(64u, (count / waves / 2u) & ~63ull));
    const uint64_t rest = count > waves * first_chunk ? count - waves * first_chunk : 0;
    const uint32_t rest_chunk =
        (uint32_t)std::min<uint64_t>(chunk_max, std::max<uint64_t>(64u, (rest / (waves * 2u) + 63u) & ~63ull));
    return {blocks, first_chunk, rest_chunk};
}

int failures = 0;

void require(bool ok, const char* what, const char* set, uint64_t count, uint32_t wpb, uint64_t resident) {
    if (ok) return;
    ++failures;
    printf("FAIL %s: %s count %llu waves_per_block %u resident %llu\n", what, set, (unsigned long long)count, wpb,
           (unsigned long long)resident);
}

}  // namespace

int main() {
    const uint64_t rad_first = rtq::kRadianceFirstChunkMax, rad_chunk = rtq::kRadianceChunkMax;
    const uint64_t counts[] = {1, 63, 64, 65, 777, 10000, (1ull << 20) + 77, (1ull << 32) + 5};
    const uint32_t waves_per_block[] = {4, 8, 16};
    const uint64_t residents[] = {1, 256, 2048};
    // the four cap sets: closest hit, any hit, radiance, gather (the last two share their caps)
    const struct {
        const char* name;
        uint64_t first_max, chunk_max;
    } sets[] = {{"closest", 0, rtq::kWalkChunkMax},
                {"any_hit", rtq::kNoChunkCap, rtq::kWalkChunkMax},
                {"radiance", rad_first, rad_chunk},
                {"gather", rad_first, rad_chunk}};
    unsigned cases = 0, with_dealt = 0, with_first_only = 0;
    for (const auto& set : sets)
        for (uint64_t count : counts)
            for (uint32_t wpb : waves_per_block)
                for (uint64_t resident : residents) {
                    const rtq::QuerySchedule s = rtq::query_schedule(count, wpb, resident, set.first_max, set.chunk_max);
                    const Triple want = set.first_max == 0 ? closest_formula(count, wpb, resident)
                                        : set.first_max == rtq::kNoChunkCap
                                            ? any_hit_formula(count, wpb, resident)
                                            : radiance_formula(count, wpb, resident, set.first_max, set.chunk_max);
                    ++cases;
                    require(s.blocks == want.blocks && s.first_chunk == want.first_chunk &&
                                s.rest_chunk == want.rest_chunk,
                            "equal triples", set.name, count, wpb, resident);
                    require(s.rest_chunk >= 64u && s.rest_chunk % 64u == 0, "dealt chunk whole waves, >= 64", set.name,
                            count, wpb, resident);
                    if (set.first_max != 0)  // (the closest-hit kernel has no first chunk)
                        require(s.first_chunk >= 64u && s.first_chunk % 64u == 0, "first chunk whole waves, >= 64",
                                set.name, count, wpb, resident);
                    else
                        require(s.first_chunk == 0u, "no first chunk", set.name, count, wpb, resident);
                    require(s.blocks >= 1u, "blocks >= 1", set.name, count, wpb, resident);
                    require((uint64_t)s.blocks * wpb * 64u >= std::min<uint64_t>(count, resident * wpb * 64u),
                            "the launch covers the batch or fills the device", set.name, count, wpb, resident);
                    const uint64_t own = (uint64_t)s.blocks * wpb * s.first_chunk;
                    if (own < count) ++with_dealt; else ++with_first_only;
                }
    // both halves of the schedule occur among the cases
    if (with_dealt == 0 || with_first_only == 0) {
        ++failures;
        printf("FAIL coverage: dealt %u first-only %u\n", with_dealt, with_first_only);
    }
    if (failures) return 1;
    printf("ok schedule cases %u dealt %u first_only %u\n", cases, with_dealt, with_first_only);
    return 0;
}
