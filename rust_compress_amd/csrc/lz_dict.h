// lz_dict.h -- SHARED DICTIONARIES for the segment-parallel LZ77 encoders (k_lz4_hc_dict.hip, k_deflate_hc_dict.hip): a block's history
// is a range anywhere in the input buffer, and blocks that name the same range share one set of hash chains, built once.
//
// The match finder still works on the block's VIRTUAL block, the dictionary (D bytes, virtual positions 0 .. D-1) followed by the
// block (virtual position D + p for the block's position p), as k_lz4_hc_hist.hip and k_deflate_hc_hist.hip do -- and computes what
// they compute on a buffer that holds the dictionary directly in front of the block.  What differs is where things come from:
//   bytes      of a virtual position below D from the dictionary, else from the block; a match that starts in the dictionary and runs
//              past its last byte goes on in the block's first bytes (lzd_extend), never in what follows the dictionary in memory
//   links      of the virtual positions 0 .. D-4 from the dictionary's shared array, built once by lzd_build (lzc_links over the
//              dictionary alone, one segment); of D-3 .. D-1 from three words of the block's own (`tail`); of D + p from the block's
//              link array, indexed by p as in the encoders without history
//   the table  a block's first segment starts from the dictionary's final bucket table (stored by lzd_build next to the links)
//              instead of from zero and a window fill.  It holds a bucket's latest position among 0 .. D-4, which is what the fill
//              of the contiguous encoder leaves of them.
// THE DICTIONARY'S LAST THREE POSITIONS have 4-byte prefixes that reach into the block: their hashes, their links and their place in
// the table depend on the block, so lzc_links over the dictionary alone leaves them out (fewer than 4 bytes left) and every block
// inserts them for itself, in front of its own positions (lzd_links_first).
// LATER SEGMENTS of a long block never see the dictionary: their window fill starts at D + s0 - WIN >= D + SEG - WIN > D, and no chain
// leads farther back than WIN.  lzd_sees says so from the numbers; where it is false the kernels call lzc_links / lzc_search on the
// block as the encoders without history do.
// No byte below a dictionary's first, beyond its last, or outside the block is read.
//
// The words of a batch (k.aux, from rcx_plan_dict of rcx_plan.h; n = nblocks):
//   aux[b]           D, the dictionary's length after the clamp, 0 = none (where k_de_scan<DE_ZDICT> and k_dh_hist_head look for it)
//   aux[n + b]       the zlib DICTID
//   aux[2n + b]      the index of block b's dictionary among the distinct ones
//   aux[3n + b], aux[4n + b]   the dictionary's offset from in_base, low and high word
//   aux[5n + j]      a block that names dictionary j
#pragma once
#include "lz_match.h"

#define LZD_GRID 1024u                 /* workgroups of the build launch at the most: one fits a CU (its LDS), four rounds of them */

struct LzdScratch {
    uint32_t* table;       // [ndict << LZC_HBITS]: a dictionary's final bucket table: the latest position + 1 of each bucket, 0 = none
    uint16_t* dlink;       // [ndict * lslot]: a dictionary's chain links by position
    uint16_t* tail;        // [n * 4]: block b's links of its dictionary's last three positions (virtual D-3, D-2, D-1)
    uint32_t ndict, lslot;
};

static inline uint64_t lzd_al(uint64_t x) { return (x + 255u) & ~255ull; }
// lslot: link entries per dictionary (the longest dictionary, a multiple of 128)
static inline uint64_t lzd_bytes(uint32_t n, uint64_t ndict, uint32_t lslot)
{
    return 256 + lzd_al((ndict * 4ull) << LZC_HBITS) + lzd_al(ndict * 2ull * lslot) + lzd_al(8ull * n);
}
// the arrays at the front of `scratch`; *rest = the first byte behind them (256-byte aligned).  The caller checked the size.
static inline LzdScratch lzd_carve(void* scratch, uint32_t n, uint32_t ndict, uint32_t lslot, uint8_t** rest)
{
    LzdScratch z;
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 255u) & ~(uintptr_t)255u);
    z.table = (uint32_t*)p; p += lzd_al(((uint64_t)ndict * 4ull) << LZC_HBITS);
    z.dlink = (uint16_t*)p; p += lzd_al((uint64_t)ndict * 2ull * lslot);
    z.tail = (uint16_t*)p; p += lzd_al(8ull * n);
    z.ndict = ndict; z.lslot = lslot;
    *rest = p;
    return z;
}

// block b's dictionary: its bytes, length (0: none), shared links and table
struct LzdDict { const uint8_t* at; uint32_t D; const uint16_t* link; const uint32_t* table; };
template <uint32_t WIN>
__device__ __forceinline__ LzdDict lzd_of(const rcx_kargs& a, const LzdScratch& z, uint32_t b)
{
    LzdDict t = {nullptr, 0, nullptr, nullptr};
    if (!a.aux) return t;
    const uint32_t n = a.nblocks, D = a.aux[b], j = a.aux[2 * (uint64_t)n + b];
    if (!D || D > WIN || D > z.lslot || j >= z.ndict) return t;            // (the plan never says so: nothing is indexed by a word unchecked)
    t.at = a.in_base + (a.aux[3 * (uint64_t)n + b] | ((uint64_t)a.aux[4 * (uint64_t)n + b] << 32));
    t.D = D;
    t.link = z.dlink + (uint64_t)j * z.lslot;
    t.table = z.table + ((uint64_t)j << LZC_HBITS);
    return t;
}

// does the segment that starts at the block's position s0 see a dictionary of D bytes: its window fill starts below virtual position D
template <uint32_t WIN>
__device__ __forceinline__ bool lzd_sees(uint32_t D, uint32_t s0)
{
    const uint64_t v0 = (uint64_t)D + s0;                                 // the segment's start, virtual
    return D && (v0 > WIN ? v0 - WIN : 0) < D;
}

// the byte / the four bytes (little-endian) at virtual position v of the dictionary t followed by the block `in`
__device__ __forceinline__ uint32_t lzd_byte(const LzdDict& t, const uint8_t* in, uint32_t v) { return v < t.D ? t.at[v] : in[v - t.D]; }
__device__ __forceinline__ uint32_t lzd_ld32(const LzdDict& t, const uint8_t* in, uint32_t v)
{
    return lzd_byte(t, in, v) | (lzd_byte(t, in, v + 1) << 8) | (lzd_byte(t, in, v + 2) << 16) | (lzd_byte(t, in, v + 3) << 24);
}

// common prefix of the block at p and the dictionary at qd (< D), at most maxl bytes: behind the dictionary's last byte the source goes
// on at the block's first
__device__ __forceinline__ uint32_t lzd_extend(const LzdDict& t, const uint8_t* in, uint32_t p, uint32_t qd, uint32_t maxl)
{
    const uint32_t room = t.D - qd;                                       // dictionary bytes from qd on
    uint32_t l = 0;
    while (l + 4 <= maxl && l + 4 <= room) {
        const uint32_t x = lzc_ld32(t.at + qd + l) ^ lzc_ld32(in + p + l);
        if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
        l += 4;
    }
    while (l < maxl && l < room) { if (t.at[qd + l] != in[p + l]) return l; l++; }
    if (l == maxl) return l;
    return room + lzc_extend(in, p + room, 0, maxl - room);
}

// One work item per distinct dictionary: its chains (lzc_links over the dictionary alone, one segment: the last three positions get no
// link and stay out of the table), then the final bucket table next to them.
template <uint32_t WIN>
__device__ __forceinline__ void lzd_build(const rcx_kargs& a, const LzdScratch& z, uint32_t* s_head, uint16_t* s_hc)
{
    const uint32_t n = a.nblocks;
    for (uint32_t j = blockIdx.x; j < z.ndict; j += gridDim.x) {
        const uint32_t b = a.aux[5 * (uint64_t)n + j];
        if (b >= n) continue;                                              // (uniform: the whole workgroup moves on)
        const LzdDict t = lzd_of<WIN>(a, z, b);
        if (!t.D) continue;
        LzcSeg s;
        s.b = b; s.f0 = 0; s.in = t.at; s.len = t.D; s.s0 = 0; s.L = t.D;
        lzc_links<WIN>(s, z.dlink + (uint64_t)j * z.lslot, s_head, s_hc);    // (ends behind a barrier)
        uint32_t* table = z.table + ((uint64_t)j << LZC_HBITS);
        for (uint32_t i = threadIdx.x; i < (1u << LZC_HBITS); i += blockDim.x) table[i] = s_head[i];
        __syncthreads();
    }
}

// Chain build of the FIRST segment s (s0 == 0; the block's own geometry) of a block behind dictionary t: lzc_links with the table
// started from the dictionary's and the dictionary's last three positions inserted in front.  link: the block's, by its positions.
template <uint32_t WIN>
__device__ __forceinline__ void lzd_links_first(const LzcSeg& s, const LzdDict& t, uint16_t* tail, uint16_t* link, uint32_t* s_head, uint16_t* s_hc)
{
    const uint32_t tid = threadIdx.x, lane = rcx_lane(), D = t.D;
    for (uint32_t i = tid; i < (1u << LZC_HBITS); i += blockDim.x) s_head[i] = t.table[i];
    __syncthreads();
    if (tid == 0) {
        // virtual positions D-3, D-2, D-1 in order: the link is the distance to the bucket's latest earlier position
        for (uint32_t k = 0; k < 3; k++) {
            uint32_t lk = 0;
            if (D + k >= 3 && s.len + 3 - k >= 4) {                        // the position exists, and 4 bytes from it on do
                const uint32_t x = D - 3 + k;
                const uint32_t h = lzc_hash(lzd_ld32(t, s.in, x));
                const uint32_t q = s_head[h];
                if (q && x - (q - 1) <= WIN) lk = x - (q - 1);
                s_head[h] = x + 1;                                         // (later than anything in the table)
            }
            tail[k] = (uint16_t)lk;
        }
    }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < s.L; c0 += LZC_CHUNK) {
        const uint32_t cn = s.L - c0 < LZC_CHUNK ? s.L - c0 : LZC_CHUNK;
        for (uint32_t i = tid; i < cn; i += blockDim.x) {
            const uint32_t p = c0 + i;                                     // (0xffff: fewer than 4 bytes left in the block)
            s_hc[i] = s.len - p >= 4 ? (uint16_t)lzc_hash(lzc_ld32(s.in + p)) : (uint16_t)0xffffu;
        }
        __syncthreads();
        if (tid < 64) {
            for (uint32_t r0 = 0; r0 < cn; r0 += 64) {
                const uint32_t i = r0 + lane, p = c0 + i, v = D + p;
                const bool live = i < cn;
                const uint32_t h = live ? s_hc[i] : 0xffffu;
                uint32_t lk = 0;
                if (h != 0xffffu) {
                    for (uint32_t j = i; j > r0; j--) if (s_hc[j - 1] == h) { lk = i - (j - 1); break; }
                    if (!lk) {
                        const uint32_t q = s_head[h];
                        if (q && v - (q - 1) <= WIN) lk = v - (q - 1);
                    }
                }
                if (live) link[p] = (uint16_t)lk;
                __builtin_amdgcn_wave_barrier();
                if (h != 0xffffu) atomicMax(&s_head[h], v + 1);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

// Chain search of the FIRST segment s (s0 == 0) of a block behind dictionary t: lzc_search on the virtual block.  M as for lzc_search;
// M::maxl measures from the end, so it takes the block's own geometry.
template <class M>
__device__ __forceinline__ void lzd_search_first(const LzcSeg& s, const LzdDict& t, const uint16_t* tail, const uint16_t* link, uint32_t* cand,
                                                 uint32_t depth)
{
    const uint32_t D = t.D;
    for (uint32_t i = threadIdx.x; i < s.L; i += blockDim.x) {
        const uint32_t p = i;
        const uint32_t maxl = M::maxl(s, i);
        uint32_t best = 0, bd = 0;
        if (maxl >= 4) {
            uint32_t dist = 0;
            for (uint32_t k = 0; k < depth; k++) {
                const uint32_t v = D + p - dist;                           // where the walk stands, virtual
                const uint32_t lk = v >= D ? link[v - D] : v + 3 >= D ? tail[v + 3 - D] : t.link[v];
                if (!lk) break;
                dist += lk;
                if (dist > M::WIN) break;
                uint32_t l;
                if (dist <= p) {                                           // the candidate lies in the block
                    const uint32_t q = p - dist;
                    if (best >= 4 && s.in[q + best] != s.in[p + best]) continue;
                    l = lzc_extend(s.in, p, q, maxl);
                } else {
                    const uint32_t qd = D + p - dist;                      // ... in the dictionary (chains never lead below 0)
                    if (best >= 4 && lzd_byte(t, s.in, qd + best) != s.in[p + best]) continue;
                    l = lzd_extend(t, s.in, p, qd, maxl);
                }
                if (l > best) { best = l; bd = dist; if (best == maxl) break; }
            }
        }
        cand[i] = best >= 4 ? M::pack(best, bd) : 0u;
    }
}
