// kbin_hash.h -- the mmer -> destination hash, host and device: the one
// statement of what routing (ranks), split passes (kb_set_partition) and the
// local buckets must agree on.  (kbin/dist.py and the tests restate it.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kb {

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// odd constants with users besides the salts below, written once
constexpr uint64_t GOLDEN64 = 0x9E3779B97F4A7C15ull;  // 2^64 / phi: splitmix64's increment, Fibonacci hashing
constexpr uint64_t XSTAR64 = 0x2545F4914F6CDD1Dull;   // xorshift64*'s multiplier

constexpr uint64_t OWNER_SALT = 0x5851F42D4C957F2Dull;  // rank of a mmer
constexpr uint64_t BUCKET_SALT = XSTAR64;               // bucket of a mmer inside one rank (independent)
constexpr uint64_t PART_SALT = GOLDEN64;                // pass of a mmer (kb_set_partition; independent)

__host__ __device__ __forceinline__ uint32_t dest_of(uint32_t mmer, uint32_t G, uint64_t salt) {
    return (uint32_t)((mix64((uint64_t)mmer + salt) >> 32) % G);
}

}  // namespace kb
