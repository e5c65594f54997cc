/* The radiance query records of the gather contract (include/rt_abi.h, steps 1 and 2), made on the
 * host: what a caller without rt_gather has to generate by hand. Built by tools/query_bench.py
 * --gather against the CPU oracle's library, whose oracle_random, oracle_logf and oracle_cosf are
 * the RNG, the logarithm and the cosine (tests/gather_ref.py is the same arithmetic in NumPy).
 * Compile with -ffp-contract=off: every operation below is one f32 operation. */
#include <math.h>
#include <stdint.h>
#include <string.h>

float oracle_random(uint32_t* seed);
float oracle_logf(float x);
float oracle_cosf(float x);

static float normal_distribution(uint32_t* seed) { /* compute_shader.wgsl:622-628 */
    float theta = 6.2831850051879883f * oracle_random(seed);
    float rho = sqrtf(-2.0f * oracle_logf(oracle_random(seed)));
    return rho * oracle_cosf(theta);
}

/* points: n records of 8 floats {position, stream bits, normal, pad}. out: samples * n records of
 * 8 floats {origin, stream bits, direction, 0}: sample-major (record s * n + i is sample s of
 * point i) or, with point_major, record i * samples + s. The stream written is stream * u (u32,
 * wrapping): rt_radiance takes first_sample per call, and seeds with stream * first_sample *
 * 326624u, so with first_sample = 1 the folded stream gives every record the contract's seed
 * stream * u * 326624u and all the records go through one call. */
void gather_records(const float* points, uint64_t n, uint32_t first_sample, uint32_t samples, int point_major,
                    float* out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float* p = points + 8 * i;
        uint32_t stream;
        memcpy(&stream, p + 3, 4);
        const float nx = p[4], ny = p[5], nz = p[6];
        const float ox = p[0] + nx * 0.0001f, oy = p[1] + ny * 0.0001f, oz = p[2] + nz * 0.0001f;
        for (uint32_t s = 0; s < samples; s++) {
            const uint32_t u = first_sample + s;
            uint32_t dseed = (stream * u * 326624u) ^ 0x9E3779B9u;
            const float gx = normal_distribution(&dseed);
            const float gy = normal_distribution(&dseed);
            const float gz = normal_distribution(&dseed);
            const float vx = nx + gx, vy = ny + gy, vz = nz + gz;
            const float inv = 1.0f / sqrtf((vx * vx + vy * vy) + vz * vz);
            float* q = out + 8 * (point_major ? (uint64_t)i * samples + s : (uint64_t)s * n + (uint64_t)i);
            const uint32_t folded = stream * u;
            q[0] = ox; q[1] = oy; q[2] = oz;
            memcpy(q + 3, &folded, 4);
            q[4] = vx * inv; q[5] = vy * inv; q[6] = vz * inv;
            q[7] = 0.0f;
        }
    }
}
