// k_xxh32.hip -- XXH32 (xxHash, 32-bit; the header, block and content checksum of the LZ4 frame format) over whole blocks.
//
// NOT a function of the reference crate: its LZ4 frame types skip every checksum (src/lz4.rs:383-402, 445-456).  This is the device
// side of rust_compress_amd/lz4frame.py, the conforming frame codec.  The checker is tests/lz4_frame_ref.py (written from the format
// description) and, where it is installed, libxxhash.
//
// The algorithm: four accumulators run over 16-byte stripes, acc_j = rotl(acc_j + word_j * P2, 13) * P1; they are folded, the length is
// added, the < 16 tail bytes go in by dwords and bytes, three multiply-xorshift steps finish.  Inputs under 16 bytes start from
// seed + P5 instead of the fold.
//
// Unlike CRC-32 and Adler-32 (k_crc32.hip, k_inflate.hip) the round is NOT combinable across chunks: rotl(x + c, 13) * P1 has no
// closed form for "the state after n more bytes", so one stream is a serial chain of one multiply-add-rotate-multiply per stripe and
// accumulator, and the 32-bit multiplies on that chain are quarter-rate.  Parallelism is the batch and the four accumulators:
//   FOUR LANES PER STREAM, SIXTEEN STREAMS PER WAVE, one wave per workgroup (a batch of 4096 streams is 256 waves: one per CU).
//   Lane j of a quad owns accumulator j.  A tile is 256 bytes of a stream = 16 stripes: lane j fetches stripes j, j+4, j+8, j+12
//   with 16-byte loads (a quad's load instruction covers 64 consecutive bytes; a dword per stripe per lane would be a quarter of
//   that per request), parks them in the quad's LDS row and reads back word j of all 16 stripes (rows padded to 272 bytes: the
//   quads' dword reads fall into different banks).  The next tile's loads are in flight while the current one is hashed.
//   The < 16 whole stripes behind the last tile are read a dword per lane, the tail by the quad's first lane.
// Any in_off alignment (the 16-byte loads are unaligned global loads), any length up to 2^32 - 1.
//
// MEASURED on MI355X (benchmarks/lz4_frame_rate.py, device-resident, the host clock around the synchronous call, median of 10;
// DESIGN.md 3.14): 4096 x 64 KiB in 0.151 ms a call = 1659 GiB/s; ONE 256 MiB stream in 368.7 ms = 0.68 GiB/s, i.e. 352 ns (about
// 840 cycles) per tile of 16 dependent rounds.  A single large stream is slow, slower than a host thread: the rate is in the batch.
#pragma once
#include "rcx_dev.h"

#define RCX_XXH_P1 2654435761u
#define RCX_XXH_P2 2246822519u
#define RCX_XXH_P3 3266489917u
#define RCX_XXH_P4 668265263u
#define RCX_XXH_P5 374761393u

__device__ __forceinline__ uint32_t rcx_xxh_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t rcx_xxh_round(uint32_t acc, uint32_t w) { return rcx_xxh_rotl(acc + w * RCX_XXH_P2, 13) * RCX_XXH_P1; }

static constexpr int XXH_TILE = 256;          // bytes of a stream per tile
static constexpr int XXH_ROW = XXH_TILE + 16; // LDS bytes per quad: 68 dwords, so quad q's word j sits in bank (4 q + j) mod 64 + const

__global__ __launch_bounds__(64) void k_xxh32(rcx_kargs a, uint32_t seed)
{
    __shared__ __align__(16) uint8_t s_tile[16 * XXH_ROW];
    const unsigned lane = rcx_lane(), j = lane & 3u, q = lane >> 2;
    const uint32_t b = blockIdx.x * 16u + q;
    const bool have = b < a.nblocks;
    const uint8_t* in = have ? a.in_base + a.in_off[b] : a.in_base;
    const uint64_t n = have ? a.in_len[b] : 0;
    const uint64_t ntiles = n / XXH_TILE;                      // whole tiles
    const uint32_t nstripes = (uint32_t)((n % XXH_TILE) / 16); // whole stripes behind them
    uint32_t acc = j == 0 ? seed + RCX_XXH_P1 + RCX_XXH_P2 : j == 1 ? seed + RCX_XXH_P2 : j == 2 ? seed : seed - RCX_XXH_P1;
    uint8_t* row = s_tile + q * XXH_ROW;

    rcx_u32x4 v0 = {0, 0, 0, 0}, v1 = v0, v2 = v0, v3 = v0;
    if (ntiles) {
        const uint8_t* p = in + 16 * j;
        v0 = *(const rcx_u32x4_u*)(p); v1 = *(const rcx_u32x4_u*)(p + 64); v2 = *(const rcx_u32x4_u*)(p + 128); v3 = *(const rcx_u32x4_u*)(p + 192);
    }
    for (uint64_t t = 0; __any(t < ntiles); t++) {             // (uniform trip count: the wave's longest stream; a quad that is done idles)
        const bool on = t < ntiles;
        if (on) {
            *(rcx_u32x4*)(row + 16 * j) = v0; *(rcx_u32x4*)(row + 64 + 16 * j) = v1;
            *(rcx_u32x4*)(row + 128 + 16 * j) = v2; *(rcx_u32x4*)(row + 192 + 16 * j) = v3;
        }
        if (t + 1 < ntiles) {                                  // the next tile's bytes travel while this one is hashed
            const uint8_t* p = in + (t + 1) * XXH_TILE + 16 * j;
            v0 = *(const rcx_u32x4_u*)(p); v1 = *(const rcx_u32x4_u*)(p + 64); v2 = *(const rcx_u32x4_u*)(p + 128); v3 = *(const rcx_u32x4_u*)(p + 192);
        }
        rcx_wave_sync();
        if (on) {
            const uint32_t* w = (const uint32_t*)row + j;
#pragma unroll
            for (int s = 0; s < 16; s++) acc = rcx_xxh_round(acc, w[4 * s]);
        }
        rcx_wave_sync();
    }
    {
        const uint8_t* p = in + ntiles * XXH_TILE + 4 * j;
        for (uint32_t s = 0; s < nstripes; s++) acc = rcx_xxh_round(acc, *(const rcx_u32_u*)(p + 16 * s));
    }
    // fold: the quad's first lane collects the four accumulators (every lane takes part in the shuffles)
    const int q0 = (int)(lane & ~3u);
    const uint32_t a1 = (uint32_t)__shfl((int)acc, q0 + 1), a2 = (uint32_t)__shfl((int)acc, q0 + 2), a3 = (uint32_t)__shfl((int)acc, q0 + 3);
    if (have && j == 0) {
        uint32_t h = n >= 16 ? rcx_xxh_rotl(acc, 1) + rcx_xxh_rotl(a1, 7) + rcx_xxh_rotl(a2, 12) + rcx_xxh_rotl(a3, 18) : seed + RCX_XXH_P5;
        h += (uint32_t)n;
        uint64_t i = n & ~15ull;
        for (; i + 4 <= n; i += 4) h = rcx_xxh_rotl(h + *(const rcx_u32_u*)(in + i) * RCX_XXH_P3, 17) * RCX_XXH_P4;
        for (; i < n; i++) h = rcx_xxh_rotl(h + in[i] * RCX_XXH_P5, 11) * RCX_XXH_P1;
        h ^= h >> 15; h *= RCX_XXH_P2; h ^= h >> 13; h *= RCX_XXH_P3; h ^= h >> 16;
        if (a.aux) a.aux[b] = h;
        if (a.status) a.status[b] = RCX_OK;
        if (a.out_len) a.out_len[b] = 0;
        if (a.in_used) a.in_used[b] = n;
    }
}

static void launch_xxh32(hipStream_t s, rcx_kargs& k, uint32_t seed)
{
    hipLaunchKernelGGL(k_xxh32, dim3((k.nblocks + 15) / 16), dim3(64), 0, s, k, seed);
}
