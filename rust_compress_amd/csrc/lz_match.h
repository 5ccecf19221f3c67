// lz_match.h -- what the segment-parallel LZ77 encoders share (k_lz4_hc.hip, k_deflate_hc.hip, k_deflate_encode.hip): the flattened
// segment list (plan, owner search, descriptor) and the exact hash-chain match finder (chain build, chain search).  The kernels stay in
// the encoders' files, each a body that declares its __shared__ arrays, loops over its segments and calls the code here; what differs
// between the formats (window, segment size, the longest allowed match, how a candidate is packed) is a template parameter, never a
// run-time branch.
#pragma once
#include "rcx_dev.h"

#define LZC_HBITS 15                   /* buckets of the chain build's table: 2^15 */
#define LZC_CHUNK 8192u                /* hashes staged in LDS at a time by lzc_links */

__device__ __forceinline__ uint32_t lzc_ld32(const uint8_t* p) { return *(const rcx_u32_u*)p; }
__device__ __forceinline__ uint32_t lzc_hash(uint32_t x) { return (x * 2654435761u) >> (32 - LZC_HBITS); }

// common prefix of in[p..] and in[q..], at most maxl bytes (in[p + maxl - 1] is the last byte read)
__device__ __forceinline__ uint32_t lzc_extend(const uint8_t* in, uint32_t p, uint32_t q, uint32_t maxl)
{
    uint32_t l = 0;
    for (;;) {
        if (l + 4 > maxl) { while (l < maxl && in[p + l] == in[q + l]) l++; return l; }
        const uint32_t x = lzc_ld32(in + p + l) ^ lzc_ld32(in + q + l);
        if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
        l += 4;
    }
}

// exclusive scan of v over the workgroup (whole waves; s_ws: a word per wave), and the workgroup's total
__device__ uint32_t lzc_block_excl_scan(uint32_t v, uint32_t* s_ws, uint32_t& total)
{
    const uint32_t lane = rcx_lane(), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_ws[wv] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (uint32_t w = 0; w < nw; w++) { const uint32_t x = s_ws[w]; if (w < wv) off += x; tot += x; }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

// the plan kernel's body, one workgroup: seg_first[b] = the segments of the blocks before b (nseg(b) each), seg_first[n] = the total;
// 1024 blocks at a time with a carry.  s_ws: 16 words, s_carry: one
template <class NSEG>
__device__ __forceinline__ void lzc_plan(uint32_t n, uint32_t* seg_first, uint32_t* s_ws, uint32_t* s_carry, NSEG nseg)
{
    if (threadIdx.x == 0) *s_carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n; b0 += blockDim.x) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n ? nseg(b) : 0u;
        uint32_t tot;
        const uint32_t ex = lzc_block_excl_scan(v, s_ws, tot);
        const uint32_t c = *s_carry;
        if (b < n) seg_first[b] = c + ex;
        __syncthreads();
        if (threadIdx.x == 0) *s_carry = c + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_first[n] = *s_carry;
}

// which block (stream) a flattened segment belongs to: the last b with sf[b] <= g
__device__ __forceinline__ uint32_t lzc_owner_of(const uint32_t* sf, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n;                          // sf[lo] <= g < sf[hi]
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sf[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

// the flattened segment g: its block b, the block's first segment f0, input and length, the segment's start in the block and length
struct LzcSeg { uint32_t b, f0, s0, L, len; const uint8_t* in; };
template <uint32_t SEG>
__device__ __forceinline__ LzcSeg lzc_seg(const rcx_kargs& a, const uint32_t* seg_first, uint32_t g)
{
    LzcSeg s;
    s.b = lzc_owner_of(seg_first, a.nblocks, g);
    s.f0 = seg_first[s.b];
    s.in = a.in_base + a.in_off[s.b];
    s.len = (uint32_t)a.in_len[s.b];
    s.s0 = (g - s.f0) * SEG;
    s.L = s.len - s.s0 < SEG ? s.len - s.s0 : SEG;
    return s;
}
// the segments a per-segment kernel loops over: all of them, or as many as the scratch holds (the scan kernel then says so)
__device__ __forceinline__ uint32_t lzc_lim(const rcx_kargs& a, const uint32_t* seg_first, uint32_t cap)
{
    const uint32_t total = seg_first[a.nblocks];
    return total < cap ? total : cap;
}

// Chain build of segment s by its workgroup: exact hash chains over the WIN bytes before the segment and the segment itself.  The table
// (s_head: 2^LZC_HBITS buckets of 4-byte prefixes, position + 1) is filled with the window (atomicMax: the latest position per bucket,
// order-free), then one wave walks the segment 64 positions at a time: a position's link is the distance to the nearest earlier position
// of its bucket (inside the 64 from the hashes staged in s_hc [LZC_CHUNK], else the table), 0 = none within WIN.  16-bit links, indexed
// by the position in the block: `link` is the block's, so the window's links are the previous segment's.
template <uint32_t WIN>
__device__ __forceinline__ void lzc_links(const LzcSeg& s, uint16_t* link, uint32_t* s_head, uint16_t* s_hc)
{
    const uint32_t tid = threadIdx.x, lane = rcx_lane();
    for (uint32_t i = tid; i < (1u << LZC_HBITS); i += blockDim.x) s_head[i] = 0;
    __syncthreads();
    const uint32_t h0 = s.s0 > WIN ? s.s0 - WIN : 0;
    for (uint32_t x = h0 + tid; x < s.s0; x += blockDim.x)
        if (s.len - x >= 4) atomicMax(&s_head[lzc_hash(lzc_ld32(s.in + x))], x + 1);
    __syncthreads();
    for (uint32_t c0 = 0; c0 < s.L; c0 += LZC_CHUNK) {
        const uint32_t cn = s.L - c0 < LZC_CHUNK ? s.L - c0 : LZC_CHUNK;
        for (uint32_t i = tid; i < cn; i += blockDim.x) {
            const uint32_t p = s.s0 + c0 + i;                 // (0xffff: fewer than 4 bytes left in the block)
            s_hc[i] = s.len - p >= 4 ? (uint16_t)lzc_hash(lzc_ld32(s.in + p)) : (uint16_t)0xffffu;
        }
        __syncthreads();
        if (tid < 64) {
            for (uint32_t r0 = 0; r0 < cn; r0 += 64) {
                const uint32_t i = r0 + lane, p = s.s0 + c0 + i;
                const bool live = i < cn;
                const uint32_t h = live ? s_hc[i] : 0xffffu;
                uint32_t lk = 0;
                if (h != 0xffffu) {
                    for (uint32_t j = i; j > r0; j--) if (s_hc[j - 1] == h) { lk = i - (j - 1); break; }
                    if (!lk) {
                        const uint32_t q = s_head[h];
                        if (q && p - (q - 1) <= WIN) lk = p - (q - 1);
                    }
                }
                if (live) link[p] = (uint16_t)lk;
                __builtin_amdgcn_wave_barrier();
                if (h != 0xffffu) atomicMax(&s_head[h], p + 1);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

// Chain search of segment s by its workgroup: every position walks its chain (`link`: the block's) up to `depth` links and keeps the
// longest match (the nearest among equals) of at least 4 bytes in cand[position in the segment], 0 = none; a candidate whose byte after
// the best length so far differs is skipped without a compare, and the walk stops at a match of the longest allowed length.  M supplies
//   WIN                      the window
//   maxl(s, i)               the longest match allowed at position i of segment s (less than 4: none)
//   pack(length, distance)   the candidate word
template <class M>
__device__ __forceinline__ void lzc_search(const LzcSeg& s, const uint16_t* link, uint32_t* cand, uint32_t depth)
{
    for (uint32_t i = threadIdx.x; i < s.L; i += blockDim.x) {
        const uint32_t p = s.s0 + i;
        const uint32_t maxl = M::maxl(s, i);
        uint32_t best = 0, bd = 0;
        if (maxl >= 4) {
            uint32_t dist = 0;
            for (uint32_t k = 0; k < depth; k++) {
                const uint32_t lk = link[p - dist];
                if (!lk) break;
                dist += lk;
                if (dist > M::WIN) break;
                const uint32_t q = p - dist;
                if (best >= 4 && s.in[q + best] != s.in[p + best]) continue;
                const uint32_t l = lzc_extend(s.in, p, q, maxl);
                if (l > best) { best = l; bd = dist; if (best == maxl) break; }
            }
        }
        cand[i] = best >= 4 ? M::pack(best, bd) : 0u;
    }
}
