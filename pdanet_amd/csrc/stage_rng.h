// stage_rng.h -- the randomness of the data stages' seeded modes (input_stage.hip, voxel_stage.hip): stream keys, a keyed
// bijection on [0, m) for samples without replacement and shuffles, a counter hash for draws with replacement.
#pragma once
#include "pda_common.h"

namespace pda {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The key of one stream of draws of one scene: purpose 0 = pick, 1 = perm1, 2 = perm2.
__device__ __forceinline__ uint64_t stream_key(uint64_t seed, int b, int purpose) {
    return splitmix64(seed ^ splitmix64((uint64_t)b * 3u + (uint64_t)purpose));
}

// x in [0, m) -> a bijection of [0, m) selected by key.  m <= 2^30, so 2h <= 30 bits; cycle walking needs fewer than 4
// rounds of the network on average (4^h < 4m).
__device__ inline uint32_t keyed_bijection(uint64_t key, uint32_t m, uint32_t x) {
    int h = 1;
    while ((1ull << (2 * h)) < (uint64_t)m) ++h;
    const uint32_t mask = (1u << h) - 1u;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    do {
        uint32_t l = x >> h, r = x & mask;
#pragma unroll
        for (int round = 0; round < 6; ++round) {
            const uint32_t f = mix32(r ^ mix32((round & 1 ? k1 : k0) + 0x9e3779b9u * (uint32_t)(round + 1))) & mask;
            const uint32_t nl = r;
            r = l ^ f;
            l = nl;
        }
        x = (l << h) | r;
    } while (x >= m);
    return x;
}

// draw i with replacement from [0, m): the high half of a 64-bit hash scaled to m (bias below m / 2^32)
__device__ __forceinline__ uint32_t draw_below(uint64_t key, uint32_t i, uint32_t m) {
    const uint64_t hsh = splitmix64(key ^ splitmix64(i));
    return (uint32_t)(((hsh >> 32) * (uint64_t)m) >> 32);
}

}  // namespace pda
