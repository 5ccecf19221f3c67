// k_xxh64.hip -- XXH64 (xxHash, 64-bit; the low 32 bits are the content checksum of a Zstandard frame) over whole blocks: the twin of
// k_xxh32.hip, and the device code the Zstandard reader (k_zstd.hip) checks a frame's content with.
//
// NOT a function of the reference crate.  The checker is a plain-Python XXH64 in tests/zstd_ref.py, written from the algorithm's
// description, and libzstd's frames, which carry the hash.
//
// The algorithm: four 64-bit accumulators run over 32-byte stripes, acc_j = rotl(acc_j + word_j * P2, 31) * P1; they are folded and
// merged, the length is added, the < 32 tail bytes go in by 8, by 4 and by bytes, a multiply-xorshift avalanche finishes.  Inputs under
// 32 bytes start from seed + P5 instead of the fold.  As with XXH32 the round has no closed form across chunks: one stream is a serial
// chain.  FOUR LANES PER STREAM (lane j of a quad owns accumulator j and loads word j of every stripe, so a quad's load covers a
// whole stripe), SIXTEEN STREAMS PER WAVE in the batch kernel; the Zstandard reader hashes one stream on the first quad of its wave.
// No LDS tile as in k_xxh32.hip: the 64-bit multiplies (four 32-bit ones and the carries) outweigh the loads here.
// Any in_off alignment, any length up to 2^32 - 1.  The hash of block b comes back in out_len[b] (eight bytes, the one 64-bit result
// word of the descriptors: rcx_xxh64_batch hands the caller's array in as out_len).
#pragma once
#include "rcx_dev.h"

#define RCX_XXH64_P1 11400714785074694791ull
#define RCX_XXH64_P2 14029467366897019727ull
#define RCX_XXH64_P3 1609587929392839161ull
#define RCX_XXH64_P4 9650029242287828579ull
#define RCX_XXH64_P5 2870177450012600261ull

__device__ __forceinline__ uint64_t rcx_xxh64_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t rcx_xxh64_round(uint64_t acc, uint64_t w) { return rcx_xxh64_rotl(acc + w * RCX_XXH64_P2, 31) * RCX_XXH64_P1; }
__device__ __forceinline__ uint64_t rcx_xxh64_merge(uint64_t h, uint64_t acc) { return (h ^ rcx_xxh64_round(0, acc)) * RCX_XXH64_P1 + RCX_XXH64_P4; }
__device__ __forceinline__ uint64_t rcx_xxh64_shfl(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// XXH64 of in[0 .. n) by the quad the calling lane belongs to; EVERY lane of the wave calls (the fold shuffles), a quad whose stream
// is empty passes n = 0.  The result is valid in the quad's first lane.
__device__ __forceinline__ uint64_t rcx_xxh64_quad(const uint8_t* in, uint64_t n, uint64_t seed, unsigned lane)
{
    const unsigned j = lane & 3u;
    uint64_t acc = j == 0 ? seed + RCX_XXH64_P1 + RCX_XXH64_P2 : j == 1 ? seed + RCX_XXH64_P2 : j == 2 ? seed : seed - RCX_XXH64_P1;
    const uint64_t nstripes = n / 32;
    const uint8_t* p = in + 8 * j;
    for (uint64_t s = 0; s < nstripes; s++) acc = rcx_xxh64_round(acc, *(const rcx_u64_u*)(p + 32 * s));
    const int q0 = (int)(lane & ~3u);
    const uint64_t a1 = rcx_xxh64_shfl(acc, q0 + 1), a2 = rcx_xxh64_shfl(acc, q0 + 2), a3 = rcx_xxh64_shfl(acc, q0 + 3);
    uint64_t h = 0;
    if (j == 0) {
        if (n >= 32) {
            h = rcx_xxh64_rotl(acc, 1) + rcx_xxh64_rotl(a1, 7) + rcx_xxh64_rotl(a2, 12) + rcx_xxh64_rotl(a3, 18);
            h = rcx_xxh64_merge(h, acc); h = rcx_xxh64_merge(h, a1); h = rcx_xxh64_merge(h, a2); h = rcx_xxh64_merge(h, a3);
        } else h = seed + RCX_XXH64_P5;
        h += n;
        uint64_t i = n & ~31ull;
        for (; i + 8 <= n; i += 8) h = rcx_xxh64_rotl(h ^ rcx_xxh64_round(0, *(const rcx_u64_u*)(in + i)), 27) * RCX_XXH64_P1 + RCX_XXH64_P4;
        if (i + 4 <= n) { h = rcx_xxh64_rotl(h ^ ((uint64_t)*(const rcx_u32_u*)(in + i) * RCX_XXH64_P1), 23) * RCX_XXH64_P2 + RCX_XXH64_P3; i += 4; }
        for (; i < n; i++) h = rcx_xxh64_rotl(h ^ ((uint64_t)in[i] * RCX_XXH64_P5), 11) * RCX_XXH64_P1;
        h ^= h >> 33; h *= RCX_XXH64_P2; h ^= h >> 29; h *= RCX_XXH64_P3; h ^= h >> 32;
    }
    return h;
}

__global__ __launch_bounds__(64) void k_xxh64(rcx_kargs a, uint64_t seed)
{
    const unsigned lane = rcx_lane(), q = lane >> 2;
    const uint32_t b = blockIdx.x * 16u + q;
    const bool have = b < a.nblocks;
    const uint8_t* in = have ? a.in_base + a.in_off[b] : a.in_base;
    const uint64_t n = have ? a.in_len[b] : 0;
    const uint64_t h = rcx_xxh64_quad(in, n, seed, lane);
    if (have && (lane & 3u) == 0) {
        if (a.out_len) a.out_len[b] = h;
        if (a.status) a.status[b] = RCX_OK;
        if (a.in_used) a.in_used[b] = n;
    }
}

static void launch_xxh64(hipStream_t s, rcx_kargs& k, uint64_t seed)
{
    hipLaunchKernelGGL(k_xxh64, dim3((k.nblocks + 15) / 16), dim3(64), 0, s, k, seed);
}
