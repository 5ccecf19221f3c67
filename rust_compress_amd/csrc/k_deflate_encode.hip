// k_deflate_encode.hip -- batched DEFLATE (RFC 1951) encoder, with zlib (RFC 1950) and gzip (RFC 1952) framing.
//
// NOT in the reference crate (it has no DEFLATE encoder): an extension, like k_gzip.hip.  The checkers are
// any RFC 1951 decoder: Python's zlib, the reference-faithful oracle and this library's own inflate kernels (see the tests).
//
// Segment-parallel.  Every stream is cut into DE_SEG-byte segments and the segments of the whole batch are flattened; each
// segment becomes exactly one DEFLATE block (two for a stored 64 KiB segment: a stored block holds at most 65535 bytes), so no
// block is empty and the pieces are joined at bit offsets, never with empty stored blocks (the reference decoder stops at an
// empty block in mid-stream, rcx.h RCX_W_EMPTY_BLOCK_MIDSTREAM).  Launches, in stream order:
//   k_de_plan            one workgroup: exclusive scan of the streams' segment counts
//   k_de_segs            (zlib / gzip) the flattened segments as blocks of input, and the existing k_adler32 / k_crc32 over them: a
//                        wave per SEGMENT, so one long stream is checksummed by as many waves as it has segments
//   k_de_segment         a workgroup per segment (grid-stride over the flattened list):
//                          1. a 2^14-entry hash table of 4-byte prefixes in LDS: the 32 KiB before the segment are inserted at once
//                             (atomicMax keeps the latest position), then the segment 512 positions at a time -- query, then insert:
//                             one candidate per position, the most recent one of an earlier round (order-independent: atomicMax)
//                          2. every candidate extended to at most 258 bytes (4-byte compares) into a per-position word in scratch
//                          3. greedy parse p += max(1, len[p]) walked by one wave over 64-position register windows (readlane)
//                          4. literal/length and distance histograms with LDS atomics
//                          5. length-limited codes (15 / 15 / 7 bits) built by one lane: symbols rank-sorted by (frequency, index)
//                             by the whole workgroup, Moffat-Katajainen code lengths, the Kraft overflow moved down, canonical codes
//                          6. the cheapest block by exact bit count: stored, fixed or dynamic Huffman of the greedy parse, or
//                             dynamic Huffman of every byte as a literal (DNA-like data: short far matches cost more than the
//                             literals they replace).  Stored is counted with the largest padding its header can need, 7 bits:
//                             its real padding depends on where the segment lands
//                          7. Huffman blocks bit-packed into LDS (a thread per 128 positions, offsets from a block-wide scan, words
//                             merged with ds_or), then copied to the segment's staging in scratch
//   k_de_scan            a wave per stream: segment bit offsets (a stored segment's length depends on its start modulo 8: a
//                        segmented scan), the segments' checksums joined (Adler-32: b = b1 + b2 + n2 (a1 - 1); CRC-32:
//                        crc(A B) = crc(A) x^(8|B|) xor crc(B) mod P), the size check against out_cap, header and trailer bytes,
//                        status / out_len / in_used
//   k_de_place           a workgroup per segment: every 32-bit word of the stream whose first bit lies in the segment is built
//                        from the segment's staging (or, for stored segments, from the input) and the next segment's first bits,
//                        and stored: no word is written twice, and nothing but the stream's own bytes (no read-modify-write)
// Workgroups never talk to each other inside a launch.  Scratch is carved in de_carve; nothing in it is assumed zero.
// The segment list (plan body, owner search, segment descriptor), the prefix extension and the block-wide scan are lz_match.h's,
// shared with k_lz4_hc.hip and k_deflate_hc.hip.
#include "lz_match.h"
#include "k_crc32.hip"                // rcx_crc_mulmod / rcx_crc_xpow: the per-segment CRC-32s joined per stream

#define DE_SEG 65536u                  /* bytes per segment (one block) */
#define DE_WIN 32768u                  /* DEFLATE window */
#define DE_HBITS 14
#ifndef DE_FAR4
#define DE_FAR4 1024u                  /* a 4-byte match farther back than this is not taken (it costs about what 4 literals do) */
#endif
#define DE_T 512                       /* threads of k_de_segment */
#define DE_RANGE (DE_SEG / DE_T)       /* positions a thread histograms / packs */
#define DE_BIGW 16448u                 /* LDS words: the hash table, then the packed block (<= 8 * DE_SEG + 84 bits + slack) */
#define DE_STG_BYTES (DE_SEG + 256u)   /* a segment's packed bits in scratch */

enum { DE_RAW = 0, DE_ZLIB = 1, DE_GZIP = 2,
       DE_ZDICT = 3 };   // zlib whose stream b carries FDICT and four DICTID bytes when a.aux[b] != 0 (k_deflate_hc_hist.hip fills them in)
// the bytes in front of stream b's DEFLATE data and behind it
template <int FMT> __device__ __forceinline__ uint32_t de_hdr(const rcx_kargs& a, uint32_t b)
{
    return FMT == DE_ZDICT ? (a.aux[b] ? 6u : 2u) : FMT == DE_ZLIB ? 2u : FMT == DE_GZIP ? 10u : 0u;
}
template <int FMT> __device__ __forceinline__ uint32_t de_trl() { return FMT == DE_ZLIB || FMT == DE_ZDICT ? 4u : FMT == DE_GZIP ? 8u : 0u; }
static constexpr uint8_t DE_ORD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // code-length code order

struct DeScratch {
    uint32_t* seg_first;   // [n + 1]: first flattened segment of each stream; [n] = total
    uint32_t* sflag;       // [n]: 1 = the stream is written by k_de_place
    uint32_t* seg_bits;    // [cap]: bits of the segment (Huffman: from k_de_segment; stored: from k_de_scan)
    uint32_t* seg_type;    // [cap]: 0 stored, 1 fixed, 2 dynamic
    uint64_t* seg_off;     // [cap]: bit offset of the segment in its stream's DEFLATE data
    uint64_t* seg_ioff;    // [cap]: the segment as a block of input (in_base offset, length; 0 past the last segment) ...
    uint64_t* seg_ilen;
    uint32_t* seg_cks;     // [cap]: ... and its Adler-32 / CRC-32 (zlib / gzip)
    uint32_t* pos;         // [cap * DE_SEG]: per position: match length << 16 | (distance - 1), 0 = no match
    uint8_t* stg;          // [cap * DE_STG_BYTES]: packed Huffman blocks
    uint32_t cap;          // segments the scratch holds
};

static inline uint64_t de_al(uint64_t x) { return (x + 255u) & ~255ull; }
static inline uint64_t de_base_bytes(uint32_t n) { return de_al(4ull * (n + 1)) + de_al(4ull * n) + 256; }
static inline uint64_t de_seg_bytes() { return 4ull + 4ull + 8ull + 8ull + 8ull + 4ull + 4ull * DE_SEG + DE_STG_BYTES; }
static inline uint64_t de_scratch_bytes(uint32_t n, uint64_t nsegs) { return de_base_bytes(n) + nsegs * de_seg_bytes() + 4096; }

static inline DeScratch de_carve(void* scratch, uint64_t bytes, uint32_t n)
{
    DeScratch d;
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 255u) & ~(uintptr_t)255u);
    const uint64_t used = (uint64_t)(p - (uint8_t*)scratch);
    d.seg_first = (uint32_t*)p; p += de_al(4ull * (n + 1));
    d.sflag = (uint32_t*)p; p += de_al(4ull * n);
    const uint64_t fixed = used + de_base_bytes(n) + 6 * 256;        // (+ the alignment of the six segment arrays)
    uint64_t cap = bytes > fixed ? (bytes - fixed) / de_seg_bytes() : 0;
    if (cap > 0xffffffffull) cap = 0xffffffffull;
    d.cap = (uint32_t)cap;
    d.seg_off = (uint64_t*)p; p += de_al(8ull * cap);
    d.seg_bits = (uint32_t*)p; p += de_al(4ull * cap);
    d.seg_type = (uint32_t*)p; p += de_al(4ull * cap);
    d.seg_ioff = (uint64_t*)p; p += de_al(8ull * cap);
    d.seg_ilen = (uint64_t*)p; p += de_al(8ull * cap);
    d.seg_cks = (uint32_t*)p; p += de_al(4ull * cap);
    d.pos = (uint32_t*)p; p += 4ull * DE_SEG * cap;
    d.stg = p;
    return d;
}

__device__ __forceinline__ uint32_t de_hash(uint32_t x) { return (x * 2654435761u) >> (32 - DE_HBITS); }
__device__ __forceinline__ uint32_t de_rev(uint32_t c, uint32_t len) { return __brev(c) >> (32 - len); }

// length 3..258 -> symbol 257..285, extra bits and their value
__device__ __forceinline__ void de_len_sym(uint32_t len, uint32_t& sym, uint32_t& eb, uint32_t& ev)
{
    if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
    const uint32_t l = len - 3;
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    eb = 31 - __clz(l) - 2;
    sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
}
// distance 1..32768 -> symbol 0..29, extra bits and their value
__device__ __forceinline__ void de_dist_sym(uint32_t d, uint32_t& sym, uint32_t& eb, uint32_t& ev)
{
    const uint32_t dd = d - 1;
    if (dd < 4) { sym = dd; eb = 0; ev = 0; return; }
    const uint32_t k = 31 - __clz(dd);
    eb = k - 1;
    sym = 2 * k + ((dd >> (k - 1)) & 1u);
    ev = dd & ((1u << eb) - 1u);
}
__device__ __forceinline__ uint32_t de_fixed_llen(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// the bits of one thread's contiguous range, merged into LDS words (ds_or: the boundary words are shared with neighbours)
struct DeBits {
    uint32_t* w; uint32_t wi; uint32_t n; uint64_t acc;
    __device__ void start(uint32_t* words, uint32_t bit) { w = words; wi = bit >> 5; n = bit & 31u; acc = 0; }
    __device__ void put(uint32_t v, uint32_t nb)        // nb <= 32, v < 2^nb
    {
        acc |= (uint64_t)v << n;
        n += nb;
        if (n >= 32) { atomicOr(&w[wi], (uint32_t)acc); wi++; acc >>= 32; n -= 32; }
    }
    __device__ void flush() { if (n) atomicOr(&w[wi], (uint32_t)acc); }
};

// code lengths of the symbols sorted[0..nu) (ascending by frequency, ties by index), at most `lim` bits (one lane)
__device__ void de_code_lengths(const uint32_t* freq, const uint16_t* sorted, uint32_t nu, uint32_t lim, uint8_t* lens, uint32_t* A)
{
    for (uint32_t i = 0; i < nu; i++) A[i] = freq[sorted[i]];
    // Moffat & Katajainen, in place: A[i] becomes the depth of the i-th least frequent symbol
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < (int)nu - 1; next++) {
        if (leaf >= (int)nu || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= (int)nu || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[nu - 2] = 0;
    for (next = (int)nu - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = (int)nu - 2; next = (int)nu - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
    // counts per length, the overflow above `lim` pushed down until the Kraft sum is exactly 1
    uint32_t cnt[33];
    for (int i = 0; i < 33; i++) cnt[i] = 0;
    for (uint32_t i = 0; i < nu; i++) cnt[A[i] < 32 ? A[i] : 32]++;
    for (uint32_t i = lim + 1; i <= 32; i++) { cnt[lim] += cnt[i]; cnt[i] = 0; }
    uint32_t total = 0;
    for (uint32_t i = lim; i > 0; i--) total += cnt[i] << (lim - i);
    while (total != (1u << lim)) {
        cnt[lim]--;
        for (uint32_t i = lim - 1; i > 0; i--) if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
        total--;
    }
    // the most frequent symbols get the shortest codes
    uint32_t j = nu;
    for (uint32_t i = 1; i <= lim; i++) for (uint32_t c = cnt[i]; c > 0; c--) lens[sorted[--j]] = (uint8_t)i;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first output (one lane)
__device__ void de_canon(const uint8_t* lens, uint32_t nsym, uint16_t* codes)
{
    uint32_t bl[16], nc[16];
    for (int i = 0; i < 16; i++) bl[i] = 0;
    for (uint32_t s = 0; s < nsym; s++) bl[lens[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; b++) { c = (c + bl[b - 1]) << 1; nc[b] = c; }
    for (uint32_t s = 0; s < nsym; s++) codes[s] = lens[s] ? (uint16_t)de_rev(nc[lens[s]]++, lens[s]) : 0;
}

// rank sort of the used symbols by (frequency, index), all threads
__device__ void de_rank_sort(const uint32_t* freq, uint32_t nsym, uint16_t* sorted)
{
    for (uint32_t t = threadIdx.x; t < nsym; t += blockDim.x) {
        const uint32_t f = freq[t];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t s = 0; s < nsym; s++) {
            const uint32_t g = freq[s];
            r += (g && (g < f || (g == f && s < t))) ? 1u : 0u;
        }
        sorted[r] = (uint16_t)t;
    }
}

__device__ __forceinline__ uint32_t de_nseg(uint64_t len) { return len >> 32 ? 0u : (uint32_t)((len + DE_SEG - 1) / DE_SEG); }

__device__ __forceinline__ LzcSeg de_seg(const rcx_kargs& a, const DeScratch& d, uint32_t g) { return lzc_seg<DE_SEG>(a, d.seg_first, g); }
__device__ __forceinline__ uint32_t de_lim(const rcx_kargs& a, const DeScratch& d) { return lzc_lim(a, d.seg_first, d.cap); }

__global__ __launch_bounds__(1024) void k_de_plan(rcx_kargs a, DeScratch d)
{
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_carry;
    lzc_plan(a.nblocks, d.seg_first, s_ws, &s_carry, [&](uint32_t b) { return de_nseg(a.in_len[b]); });
}

// the flattened segments as blocks of input for the checksum kernels (entries past the last segment: empty blocks)
__global__ __launch_bounds__(256) void k_de_segs(rcx_kargs a, DeScratch d)
{
    const uint32_t total = d.seg_first[a.nblocks];
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < d.cap; g += gridDim.x * blockDim.x) {
        uint64_t o = 0, l = 0;
        if (g < total) {
            const LzcSeg s = de_seg(a, d, g);
            o = a.in_off[s.b] + s.s0;
            l = s.L;
        }
        d.seg_ioff[g] = o; d.seg_ilen[g] = l;
    }
}

__global__ __launch_bounds__(DE_T) void k_de_segment(rcx_kargs a, DeScratch d)
{
    __shared__ uint32_t s_big[DE_BIGW];                   // hash table (phases 1-2), then the packed block (phase 7)
    __shared__ uint64_t s_start[DE_SEG / 64];             // token starts of the greedy parse
    __shared__ uint32_t s_lf[288], s_df[32];              // frequencies of the greedy parse
    __shared__ uint8_t s_ll[2][288], s_dl[2][32], s_cl[2][19];   // code lengths of the two parses
    __shared__ uint16_t s_rle[2][320];                    // their code-length code items: symbol | extra value << 5
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_x[24];                          // extra bits, header bits, choice; per parse: hlit hdist hclen items cost
    // one region, three lives: the round's candidate distances (phase 2); byte histogram + tree building (phases 4-5); codes (phase 7)
    __shared__ uint32_t s_tmp[256 + 339 + 288 + 170];
    uint32_t* const s_cd = s_tmp;                         // [8 + DE_T]: [0, 8) the previous round's last
    uint32_t* const s_bf = s_tmp;                         // [256] every byte of the segment
    uint32_t* const s_tf = s_tmp + 256;                   // [288 + 32 + 19] frequencies that shape the trees (two symbols at least)
    uint32_t* const s_A = s_tmp + 256 + 339;              // [288]
    uint16_t* const s_sort = (uint16_t*)(s_tmp + 256 + 339 + 288);   // [339]
    uint16_t* const s_lc = (uint16_t*)s_tmp;              // [288 + 32 + 19] the chosen codes
    uint16_t* const s_dc = s_lc + 288;
    uint16_t* const s_cc = s_lc + 320;
    const uint32_t tid = threadIdx.x, lane = rcx_lane();
    const uint32_t n = a.nblocks;
    const uint32_t total = d.seg_first[n];
    const uint32_t lim = total < d.cap ? total : d.cap;

    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        // (lzc_seg's lines, written out: with de_seg(a, d, g) here this kernel compiled to 215 VGPRs and took 2-6 % longer)
        const uint32_t b = lzc_owner_of(d.seg_first, n, g);
        const uint8_t* in = a.in_base + a.in_off[b];
        const uint32_t len = (uint32_t)a.in_len[b];
        const uint32_t s0 = (g - d.seg_first[b]) * DE_SEG;
        const uint32_t s1 = len - s0 < DE_SEG ? len : s0 + DE_SEG;
        const uint32_t L = s1 - s0;
        uint32_t* pos = d.pos + (uint64_t)g * DE_SEG;

        // 1. the table: empty, then the window before the segment (atomicMax: the latest position per bucket wins)
        for (uint32_t i = tid; i < (1u << DE_HBITS); i += DE_T) s_big[i] = 0;
        for (uint32_t i = tid; i < 288; i += DE_T) s_lf[i] = 0;
        if (tid < 32) s_df[tid] = 0;
        if (tid < 24) s_x[tid] = 0;
        if (tid < 8) s_cd[tid] = 0;
        __syncthreads();
        // (positions run to len - 1 <= 2^32 - 2: every loop counts segment-relative offsets and every guard compares distances to
        //  the end, len - x, so that nothing wraps in 32 bits; a position's table value x + 1 is at most 2^32 - 1)
        const uint32_t ws0 = s0 > DE_WIN ? s0 - DE_WIN : 0;
        for (uint32_t r = tid; r < s0 - ws0; r += DE_T) {
            const uint32_t x = ws0 + r;
            if (len - x >= 4) atomicMax(&s_big[de_hash(lzc_ld32(in + x))], x + 1);
        }
        __syncthreads();
        // 2. the segment 512 positions a round: the table's candidate for every position, then the longest match among it, distance 1
        //    and the candidates of the three positions before (a repeat the table lost to a collision, a run inside the round), then
        //    the round's positions go into the table
        for (uint32_t c0 = 0; c0 < L; c0 += DE_T) {
            const uint32_t rel = c0 + tid, p = s0 + rel;                   // (p is used only where rel < L: then p < s1 <= len)
            uint32_t h = 0, dh = 0;
            const bool hashed = rel < L && len - p >= 4;
            if (hashed) {
                const uint32_t x = lzc_ld32(in + p);
                h = de_hash(x);
                const uint32_t q1 = s_big[h];
                if (q1 && p - (q1 - 1) <= DE_WIN && lzc_ld32(in + q1 - 1) == x) dh = p - (q1 - 1);
            }
            s_cd[8 + tid] = dh;
            __syncthreads();
            uint32_t m = 0;
            if (hashed && s1 - p >= 4) {
                const uint32_t maxl = s1 - p < 258 ? s1 - p : 258;
                uint32_t cand[5] = {dh, 1u, s_cd[7 + tid], s_cd[6 + tid], s_cd[5 + tid]};
                uint32_t bl = 0, bd = 0;
                for (int i = 0; i < 5; i++) {
                    const uint32_t dd = cand[i];
                    if (!dd || dd > p || dd > DE_WIN) continue;
                    bool seen = false;
                    for (int j = 0; j < i; j++) seen |= cand[j] == dd;
                    if (seen) continue;
                    const uint32_t l = lzc_extend(in, p, p - dd, maxl);
                    if (l > bl || (l == bl && dd < bd)) { bl = l; bd = dd; }
                }
                if (bl >= 5 || (bl == 4 && bd <= DE_FAR4)) m = (bl << 16) | (bd - 1);
            }
            if (rel < L) pos[rel] = m;
            __syncthreads();
            if (hashed) atomicMax(&s_big[h], p + 1);
            if (tid < 8) s_cd[tid] = s_cd[DE_T + tid];
            __syncthreads();
        }
        // 3. greedy parse, one wave: lane i holds the match length at window position i, the walk reads it with readlane
        if (tid < 64) {
            uint32_t ptr = 0;
            for (uint32_t base = 0; base < L; base += 64) {
                const uint32_t p = base + lane;
                const uint32_t ml = p < L ? (pos[p] >> 16) : 0u;
                uint64_t vis = 0;
                while (ptr < base + 64 && ptr < L) {
                    const uint32_t r = ptr - base;
                    vis |= 1ull << r;
                    const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)ml, (int)r);
                    ptr += l ? l : 1u;
                }
                if (lane == 0) s_start[base >> 6] = vis;
            }
        }
        __syncthreads();
        // 4. histograms (the end-of-block symbol once), and of every byte (the second parse: all literals)
        const uint32_t r0 = tid * DE_RANGE, r1 = r0 + DE_RANGE < L ? r0 + DE_RANGE : L;
        for (uint32_t i = tid; i < 256; i += DE_T) s_bf[i] = 0;
        __syncthreads();
        {
            uint32_t extra = 0;
            for (uint32_t p = r0; p < r1; p++) {
                const uint32_t c = in[s0 + p];
                atomicAdd(&s_bf[c], 1u);
                if (!((s_start[p >> 6] >> (p & 63)) & 1ull)) continue;
                const uint32_t m = pos[p];
                if (m) {
                    uint32_t ls, le, lv, ds, de, dv;
                    de_len_sym(m >> 16, ls, le, lv);
                    de_dist_sym((m & 0xffffu) + 1, ds, de, dv);
                    atomicAdd(&s_lf[ls], 1u); atomicAdd(&s_df[ds], 1u);
                    extra += le + de;
                } else atomicAdd(&s_lf[c], 1u);
            }
            if (extra) atomicAdd(&s_x[0], extra);
            if (tid == 0) atomicAdd(&s_lf[256], 1u);
        }
        for (uint32_t i = tid; i < DE_BIGW; i += DE_T) s_big[i] = 0;     // (the table is done with: the packed block goes here)
        __syncthreads();
        // 5. the trees of both parses and their exact dynamic-block cost
        for (uint32_t v = 0; v < 2; v++) {
            uint32_t* const X = s_x + 8 + 8 * v;                          // hlit hdist hclen items cost
            if (tid == 0) {
                for (int i = 0; i < 288; i++) s_tf[i] = v ? (i < 256 ? s_bf[i] : i == 256 ? 1u : 0u) : s_lf[i];
                for (int i = 0; i < 32; i++) s_tf[288 + i] = (!v && i < 30) ? s_df[i] : 0u;
                uint32_t nl = 0, nd = 0;
                for (int i = 0; i < 286; i++) nl += s_tf[i] ? 1u : 0u;
                for (int i = 0; i < 30; i++) nd += s_tf[288 + i] ? 1u : 0u;
                if (nl < 2) s_tf[s_tf[0] ? 1 : 0] = 1;
                if (nd < 2) { if (!s_tf[288]) s_tf[288] = 1; else s_tf[289] = 1; }
                if (nd == 0) s_tf[289] = 1;
            }
            __syncthreads();
            de_rank_sort(s_tf, 286, s_sort);
            de_rank_sort(s_tf + 288, 30, s_sort + 288);
            __syncthreads();
            if (tid == 0) {
                uint8_t* ll = s_ll[v]; uint8_t* dl = s_dl[v]; uint16_t* rle = s_rle[v];
                uint32_t nl = 0, nd = 0;
                for (int i = 0; i < 286; i++) nl += s_tf[i] ? 1u : 0u;
                for (int i = 0; i < 30; i++) nd += s_tf[288 + i] ? 1u : 0u;
                for (int i = 0; i < 288; i++) ll[i] = 0;
                for (int i = 0; i < 32; i++) dl[i] = 0;
                de_code_lengths(s_tf, s_sort, nl, 15, ll, s_A);
                de_code_lengths(s_tf + 288, s_sort + 288, nd, 15, dl, s_A);
                uint32_t hlit = 286, hdist = 30;
                while (hlit > 257 && !ll[hlit - 1]) hlit--;
                while (hdist > 1 && !dl[hdist - 1]) hdist--;
                // run-length code of the hlit + hdist lengths (16: previous 3-6 times, 17: zero 3-10 times, 18: zero 11-138 times)
                uint32_t nr = 0, i = 0;
                const uint32_t tot = hlit + hdist;
                while (i < tot) {
                    const uint32_t x = i < hlit ? ll[i] : dl[i - hlit];
                    uint32_t run = 1;
                    while (i + run < tot && (i + run < hlit ? ll[i + run] : dl[i + run - hlit]) == x) run++;
                    i += run;
                    if (x == 0) {
                        while (run >= 11) { const uint32_t r = run < 138 ? run : 138; rle[nr++] = (uint16_t)(18 | (r - 11) << 5); run -= r; }
                        if (run >= 3) { rle[nr++] = (uint16_t)(17 | (run - 3) << 5); run = 0; }
                        while (run) { rle[nr++] = 0; run--; }
                    } else {
                        rle[nr++] = (uint16_t)x; run--;
                        while (run >= 3) { const uint32_t r = run < 6 ? run : 6; rle[nr++] = (uint16_t)(16 | (r - 3) << 5); run -= r; }
                        while (run) { rle[nr++] = (uint16_t)x; run--; }
                    }
                }
                for (int k = 0; k < 19; k++) s_tf[320 + k] = 0;
                for (uint32_t k = 0; k < nr; k++) s_tf[320 + (rle[k] & 31u)]++;
                uint32_t nc = 0;
                for (int k = 0; k < 19; k++) nc += s_tf[320 + k] ? 1u : 0u;
                uint32_t dyn = 0;                                          // (the code-length symbols' own bits are added below)
                for (uint32_t k = 0; k < nr; k++) { const uint32_t sy = rle[k] & 31u; dyn += sy == 16 ? 2 : sy == 17 ? 3 : sy == 18 ? 7 : 0; }
                if (v == 0) {
                    uint32_t fix = 3 + s_x[0];
                    dyn += s_x[0];
                    for (int k = 0; k < 286; k++) { dyn += s_lf[k] * ll[k]; fix += s_lf[k] * de_fixed_llen(k); }
                    for (int k = 0; k < 30; k++) { dyn += s_df[k] * dl[k]; fix += s_df[k] * 5u; }
                    s_x[2] = fix;
                } else {
                    for (int k = 0; k < 256; k++) dyn += s_bf[k] * ll[k];
                    dyn += ll[256];
                }
                if (nc < 2) s_tf[320 + (s_tf[320] ? 1 : 0)] = 1;
                X[0] = hlit; X[1] = hdist; X[3] = nr; X[4] = dyn;
            }
            __syncthreads();
            de_rank_sort(s_tf + 320, 19, s_sort + 320);
            __syncthreads();
            if (tid == 0) {
                uint32_t nc = 0;
                for (int k = 0; k < 19; k++) nc += s_tf[320 + k] ? 1u : 0u;
                uint8_t* cl = s_cl[v];
                for (int k = 0; k < 19; k++) cl[k] = 0;
                de_code_lengths(s_tf + 320, s_sort + 320, nc, 7, cl, s_A);
                uint32_t hclen = 19;
                while (hclen > 4 && !cl[DE_ORD[hclen - 1]]) hclen--;
                uint32_t dyn = X[4] + 3 + 5 + 5 + 4 + 3 * hclen;
                for (uint32_t k = 0; k < X[3]; k++) dyn += cl[s_rle[v][k] & 31u];
                X[2] = hclen; X[4] = dyn;
            }
            __syncthreads();
        }
        // 6. the cheapest block: stored (counted with the most padding), fixed or dynamic for the greedy parse, dynamic for all literals
        if (tid == 0) {
            uint32_t type = 0, var = 0;
            uint64_t best = 42ull * ((L + 65534u) / 65535u) + 8ull * L;
            if (s_x[2] < best) { type = 1; var = 0; best = s_x[2]; }
            if (s_x[12] < best) { type = 2; var = 0; best = s_x[12]; }
            if (s_x[20] < best) { type = 2; var = 1; best = s_x[20]; }
            s_x[5] = type; s_x[6] = var;
        }
        __syncthreads();
        const uint32_t type = s_x[5], var = s_x[6];
        if (tid == 0 && type) {
            uint8_t* ll = s_ll[var]; uint8_t* dl = s_dl[var]; const uint8_t* cl = s_cl[var];
            if (type == 1) {
                for (int k = 0; k < 288; k++) ll[k] = (uint8_t)de_fixed_llen(k);
                for (int k = 0; k < 32; k++) dl[k] = 5;
            }
            de_canon(ll, 288, s_lc);
            de_canon(dl, 32, s_dc);
            DeBits w; w.start(s_big, 0);
            w.put(0, 1);                                      // BFINAL: set by k_de_place on the stream's last block
            w.put(type, 2);
            if (type == 2) {
                const uint32_t* X = s_x + 8 + 8 * var;
                de_canon(cl, 19, s_cc);
                w.put(X[0] - 257, 5); w.put(X[1] - 1, 5); w.put(X[2] - 4, 4);
                for (uint32_t k = 0; k < X[2]; k++) w.put(cl[DE_ORD[k]], 3);
                for (uint32_t k = 0; k < X[3]; k++) {
                    const uint32_t sy = s_rle[var][k] & 31u, ev = s_rle[var][k] >> 5;
                    w.put(s_cc[sy], cl[sy]);
                    if (sy >= 16) w.put(ev, sy == 16 ? 2 : sy == 17 ? 3 : 7);
                }
            }
            w.flush();
            s_x[4] = w.wi * 32 + w.n;
        }
        __syncthreads();
        if (type) {
            // 7. pack: the bits of every thread's range, offsets from a block-wide scan
            const uint8_t* ll = s_ll[var]; const uint8_t* dl = s_dl[var];
            uint32_t nb = 0;
            for (uint32_t p = r0; p < r1; p++) {
                if (var == 0 && !((s_start[p >> 6] >> (p & 63)) & 1ull)) continue;
                const uint32_t m = var ? 0u : pos[p];
                if (m) {
                    uint32_t ls, le, lv, ds, de, dv;
                    de_len_sym(m >> 16, ls, le, lv);
                    de_dist_sym((m & 0xffffu) + 1, ds, de, dv);
                    nb += ll[ls] + le + dl[ds] + de;
                } else nb += ll[in[s0 + p]];
            }
            uint32_t tot;
            const uint32_t off = lzc_block_excl_scan(nb, s_ws, tot) + s_x[4];
            DeBits w; w.start(s_big, off);
            for (uint32_t p = r0; p < r1; p++) {
                if (var == 0 && !((s_start[p >> 6] >> (p & 63)) & 1ull)) continue;
                const uint32_t m = var ? 0u : pos[p];
                if (m) {
                    uint32_t ls, le, lv, ds, de, dv;
                    de_len_sym(m >> 16, ls, le, lv);
                    de_dist_sym((m & 0xffffu) + 1, ds, de, dv);
                    w.put(s_lc[ls], ll[ls]);
                    if (le) w.put(lv, le);
                    w.put(s_dc[ds], dl[ds]);
                    if (de) w.put(dv, de);
                } else { const uint32_t c = in[s0 + p]; w.put(s_lc[c], ll[c]); }
            }
            w.flush();
            const uint32_t end = s_x[4] + tot;
            if (tid == DE_T - 1) { DeBits e; e.start(s_big, end); e.put(s_lc[256], ll[256]); e.flush(); }
            __syncthreads();
            const uint32_t bits = end + ll[256];
            uint32_t* stg = (uint32_t*)(d.stg + (uint64_t)g * DE_STG_BYTES);
            const uint32_t nw = (bits + 31) / 32 + 2;                       // (+ zero words: k_de_place reads 8 bytes at a time)
            for (uint32_t i = tid; i < nw; i += DE_T) stg[i] = s_big[i];
            if (tid == 0) { d.seg_bits[g] = bits; d.seg_type[g] = type; }
        } else if (tid == 0) { d.seg_bits[g] = 0; d.seg_type[g] = 0; }
        __syncthreads();
    }
}

// a stored segment of L bytes starting at bit m (mod 8) of the stream: its length in bits
__device__ __forceinline__ uint64_t de_stored_bits(uint32_t L, uint32_t m)
{
    const uint32_t nblk = (L + 65534u) / 65535u;
    const uint32_t h = 3 + ((8u - ((m + 3u) & 7u)) & 7u);
    return (uint64_t)h + 32u + 8ull * L + 40ull * (nblk - 1);
}

// a wave per stream: bit offsets of its segments, the size check, header, trailer and per-stream results
template <int FMT>
__global__ __launch_bounds__(256) void k_de_scan(rcx_kargs a, DeScratch d)
{
    const uint32_t lane = rcx_lane();
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (b >= a.nblocks) return;
    const uint32_t HDR = de_hdr<FMT>(a, b), TRL = de_trl<FMT>();
    constexpr bool ZL = FMT == DE_ZLIB || FMT == DE_ZDICT;
    const uint64_t len = a.in_len[b];
    const uint32_t f0 = d.seg_first[b], f1 = d.seg_first[b + 1];
    int st = RCX_OK;
    if (len >> 32) st = RCX_E_MALFORMED;                                   // (blocks are limited to 2^32 - 1 bytes, as everywhere)
    else if (f1 > d.cap) st = RCX_E_MALFORMED;                             // scratch smaller than rcx_scratch_bytes asked for
    uint64_t off = 0;
    if (!st && len == 0) off = 10;                                         // a lone final fixed block: 1, 01, end-of-block
    uint32_t ck = ZL ? 1u : 0u;                                            // the checksum of nothing; then segment by segment
    const uint32_t K64 = FMT == DE_GZIP && !st && f1 - f0 > 1 ? RCX_UNI(rcx_crc_xpow(8ull * DE_SEG)) : 0u;
    if (!st) {
        for (uint32_t c0 = f0; c0 < f1; c0 += 64) {
            const uint32_t g = c0 + lane;
            const bool live = g < f1;
            const uint32_t ty = live ? d.seg_type[g] : 1u;
            const uint32_t hb = live && ty ? d.seg_bits[g] : 0u;           // Huffman bits (0 for a stored segment)
            const uint32_t Lg = live ? (g + 1 < f1 ? DE_SEG : (uint32_t)(len - (uint64_t)(g - f0) * DE_SEG)) : 0u;
            const bool sto = live && ty == 0;
            // start modulo 8: a stored segment ends byte-aligned, so a lane's start is the Huffman bits since the last stored segment
            // before it (or since the chunk's start) -- a max-scan for that segment, a plain scan of the Huffman bits
            uint32_t incl = hb;
            for (uint32_t dd = 1; dd < 64; dd <<= 1) { const uint32_t t = __shfl_up(incl, dd); if (lane >= dd) incl += t; }
            const uint32_t excl = incl - hb;
            int last = sto ? (int)lane : -1;
            for (uint32_t dd = 1; dd < 64; dd <<= 1) { const int t = __shfl_up(last, dd); if (lane >= dd && t > last) last = t; }
            int prev = __shfl_up(last, 1);
            if (lane == 0) prev = -1;
            const uint32_t incl_prev = __shfl((int)incl, prev < 0 ? 0 : prev);
            const uint32_t m = prev >= 0 ? (excl - incl_prev) & 7u : (uint32_t)(off + excl) & 7u;
            const uint64_t bits = sto ? de_stored_bits(Lg, m) : (uint64_t)hb;
            // offsets: a scan of the bits (u64 across the chunk, stream totals reach 2^35)
            uint64_t inc = bits;
            for (uint32_t dd = 1; dd < 64; dd <<= 1) {
                const uint32_t lo = __shfl_up((uint32_t)inc, dd), hi = __shfl_up((uint32_t)(inc >> 32), dd);
                if (lane >= dd) inc += ((uint64_t)hi << 32) | lo;
            }
            if (live) { d.seg_off[g] = off + inc - bits; if (sto) d.seg_bits[g] = (uint32_t)bits; }
            if (FMT != DE_RAW) {
                const uint32_t sc = live ? d.seg_cks[g] : 0u;
                const uint32_t nl = f1 - c0 < 64 ? f1 - c0 : 64;
                for (uint32_t i = 0; i < nl; i++) {
                    const uint32_t c2 = (uint32_t)__shfl((int)sc, (int)i), l2 = (uint32_t)__shfl((int)Lg, (int)i);
                    if (FMT == DE_GZIP) ck = rcx_crc_mulmod(l2 == DE_SEG ? K64 : rcx_crc_xpow(8ull * l2), ck) ^ c2;
                    else {
                        const uint64_t a1 = ck & 0xffffu, b1 = ck >> 16, a2 = c2 & 0xffffu, b2 = c2 >> 16;
                        const uint32_t ra = (uint32_t)((a1 + a2 + 65520u) % 65521u);
                        const uint32_t rb = (uint32_t)((b1 + b2 + (uint64_t)l2 * (a1 + 65520u)) % 65521u);
                        ck = (rb << 16) | ra;
                    }
                }
            }
            const uint32_t tl = __shfl((uint32_t)inc, 63), th = __shfl((uint32_t)(inc >> 32), 63);
            off += ((uint64_t)th << 32) | tl;
        }
    }
    const uint64_t dbytes = (off + 7) / 8;
    const uint64_t total = HDR + dbytes + TRL;
    if (!st && total > a.out_cap[b]) st = RCX_E_OUTPUT_TOO_SMALL;
    if (lane == 0) {
        d.sflag[b] = st == RCX_OK && len != 0;
        a.status[b] = st;
        a.out_len[b] = st ? 0 : total;
        if (a.in_used) a.in_used[b] = st ? 0 : len;
        if (!st) {
            uint8_t* o = a.out_base + a.out_off[b];
            if (ZL) { o[0] = 0x78; o[1] = 0x01; }                           // deflate, 32 KiB window, fastest; (0x7801 % 31 == 0)
            if (FMT == DE_GZIP) {
                o[0] = 0x1f; o[1] = 0x8b; o[2] = 8;
                for (int i = 3; i < 9; i++) o[i] = 0;                       // FLG, MTIME, XFL
                o[9] = 0xff;                                                // OS: unknown
            }
            if (len == 0) { o[HDR] = 0x03; o[HDR + 1] = 0x00; }
            uint8_t* t = o + HDR + dbytes;
            if (ZL) { t[0] = (uint8_t)(ck >> 24); t[1] = (uint8_t)(ck >> 16); t[2] = (uint8_t)(ck >> 8); t[3] = (uint8_t)ck; }
            if (FMT == DE_GZIP) {
                const uint32_t isz = (uint32_t)len;
                for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(ck >> (8 * i)); t[4 + i] = (uint8_t)(isz >> (8 * i)); }
            }
        }
    }
}

// byte k of a stored segment's data after its first header bits: [LEN NLEN data] then [header LEN NLEN data] per further block
__device__ __forceinline__ uint32_t de_stored_byte(const uint8_t* src, uint32_t L, uint64_t k, bool fin)
{
    const uint32_t nblk = (L + 65534u) / 65535u;
    uint64_t start = 0;
    for (uint32_t i = 0; i < nblk; i++) {
        const uint32_t bl = L - i * 65535u < 65535u ? L - i * 65535u : 65535u;
        const uint32_t hd = i ? 5u : 4u;
        if (k < start + hd + bl) {
            uint64_t r = k - start;
            if (i) { if (r == 0) return (fin && i == nblk - 1) ? 1u : 0u; r--; }
            if (r == 0) return bl & 0xffu;
            if (r == 1) return bl >> 8;
            if (r == 2) return ~bl & 0xffu;
            if (r == 3) return (~bl >> 8) & 0xffu;
            return src[i * 65535u + (r - 4)];
        }
        start += hd + bl;
    }
    return 0;
}

// 32 bits of segment g from its bit r on (fin: the stream's last segment, BFINAL set); bits past the segment's end read as zero
__device__ __forceinline__ uint32_t de_seg_bits32(const DeScratch& d, const uint8_t* in, uint32_t f0, uint32_t g, uint64_t len, bool fin, uint64_t r)
{
    if (d.seg_type[g]) {
        const uint8_t* s = d.stg + (uint64_t)g * DE_STG_BYTES + (r >> 3);
        const uint64_t v = *(const rcx_u64_u*)s;
        uint32_t x = (uint32_t)(v >> (r & 7));
        if (r == 0 && fin) x |= 1u;
        return x;
    }
    const uint32_t j = g - f0;
    const uint32_t L = (uint32_t)(len - (uint64_t)j * DE_SEG < DE_SEG ? len - (uint64_t)j * DE_SEG : DE_SEG);
    const uint8_t* src = in + (uint64_t)j * DE_SEG;
    const uint32_t m = (uint32_t)(d.seg_off[g] & 7u);
    const uint32_t h = 3 + ((8u - ((m + 3u) & 7u)) & 7u);
    const bool fin0 = fin && L <= 65535u;
    if (r < h) {
        uint64_t acc = (r == 0 && fin0) ? 1u : 0u;
        uint32_t v = 0;
        for (int i = 0; i < 4; i++) v |= de_stored_byte(src, L, i, fin) << (8 * i);
        acc |= (uint64_t)v << (h - r);
        return (uint32_t)acc;
    }
    const uint64_t q = r - h, k = q >> 3;
    uint64_t v = 0;
    for (int i = 0; i < 5; i++) v |= (uint64_t)de_stored_byte(src, L, k + i, fin) << (8 * i);
    return (uint32_t)(v >> (q & 7));
}

template <int FMT>
__global__ __launch_bounds__(256) void k_de_place(rcx_kargs a, DeScratch d)
{
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        const uint32_t b = s.b;
        if (!d.sflag[b]) continue;
        const uint32_t f0 = s.f0, f1 = d.seg_first[b + 1];
        const uint8_t* in = s.in;
        const uint64_t len = s.len;                                        // (a stream that has segments is shorter than 2^32)
        const bool last = g + 1 == f1;
        const uint64_t o0 = d.seg_off[g], o1 = o0 + d.seg_bits[g];
        const uint32_t HDR = de_hdr<FMT>(a, b);
        const uint64_t dbytes = a.out_len[b] - HDR - de_trl<FMT>();
        uint8_t* o = a.out_base + a.out_off[b] + HDR;
        const uint64_t t0 = (o0 + 31) / 32, t1 = (o1 + 31) / 32;          // the words whose first bit lies in [o0, o1)
        for (uint64_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) {
            const uint64_t r = 32 * t - o0;
            uint32_t x = de_seg_bits32(d, in, f0, g, len, last, r);
            const uint64_t have = o1 - 32 * t;                             // bits of this segment in the word
            if (have < 32) {
                x &= (1u << have) - 1u;
                if (!last) x |= de_seg_bits32(d, in, f0, g + 1, len, g + 2 == f1, 0) << have;   // (a segment that is not the last is >= 32 bits long)
            }
            const uint64_t at = 4 * t;
            if (at + 4 <= dbytes) *(rcx_u32_u*)(o + at) = x;
            else for (uint64_t i = at; i < dbytes; i++) o[i] = (uint8_t)(x >> (8 * (i - at)));
        }
    }
}

// the whole encode on stream s.  cks launches the checksum kernel of the framing (k_crc32 / k_adler32) over the segments, with aux
// pointed at the scratch's per-segment checksum array; k.scratch holds de_scratch_bytes(n, segments) bytes.
static int launch_deflate_encode(hipStream_t s, rcx_kargs& k, int fmt, std::string& err, void (*cks)(hipStream_t, rcx_kargs&))
{
    const uint32_t n = k.nblocks;
    if (!k.scratch || k.scratch_bytes < de_scratch_bytes(n, 0)) { err = "deflate encode: scratch too small"; return RCX_RC_BAD_ARG; }
    const DeScratch d = de_carve(k.scratch, k.scratch_bytes, n);
    hipLaunchKernelGGL(k_de_plan, dim3(1), dim3(1024), 0, s, k, d);
    if (fmt != DE_RAW && d.cap) {
        hipLaunchKernelGGL(k_de_segs, dim3(d.cap < 65536u * 4u ? (d.cap + 255) / 256 : 1024u), dim3(256), 0, s, k, d);
        rcx_kargs kc = k;                                 // a wave per segment
        kc.in_off = d.seg_ioff; kc.in_len = d.seg_ilen; kc.nblocks = d.cap;
        kc.out_len = nullptr; kc.in_used = nullptr; kc.status = nullptr; kc.aux = d.seg_cks;
        cks(s, kc);
    }
    if (d.cap) hipLaunchKernelGGL(k_de_segment, dim3(d.cap < 2048u ? d.cap : 2048u), dim3(DE_T), 0, s, k, d);
    const dim3 gs((n + 3) / 4), gp(d.cap < 4096u ? d.cap : 4096u);
    if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_scan<DE_RAW>, gs, dim3(256), 0, s, k, d);
    else if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_de_scan<DE_ZLIB>, gs, dim3(256), 0, s, k, d);
    else hipLaunchKernelGGL(k_de_scan<DE_GZIP>, gs, dim3(256), 0, s, k, d);
    if (d.cap) {
        if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_place<DE_RAW>, gp, dim3(256), 0, s, k, d);
        else if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_de_place<DE_ZLIB>, gp, dim3(256), 0, s, k, d);
        else hipLaunchKernelGGL(k_de_place<DE_GZIP>, gp, dim3(256), 0, s, k, d);
    }
    return RCX_RC_OK;
}
