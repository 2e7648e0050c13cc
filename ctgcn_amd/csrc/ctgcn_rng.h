// ctgcn_rng.h — the counter-based RNG of the walk / negative-sampling draws (splitmix64 of seed/key/counter).  Shared by
// ctgcn_walks.hip and ctgcn_epoch.hip: the batched sampler must reproduce the single-batch draws bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ uint64_t ctgcn_mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double ctgcn_u01(uint64_t a, uint64_t b, uint64_t c)
{
    return (double)(ctgcn_mix64(ctgcn_mix64(a) ^ ctgcn_mix64(b * 0x100000001b3ull + c)) >> 11) * (1.0 / 9007199254740992.0);
}
