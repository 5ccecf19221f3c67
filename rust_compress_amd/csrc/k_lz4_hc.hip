// k_lz4_hc.hip -- batched LZ4 high-compression (HC) block encoder: hash chains searched to a level-dependent depth and a
// cost-based parse.  Every input block becomes one LZ4 block (the format of src/lz4.rs:67-110, what rcx_lz4_decode_batch reads).
//
// NOT in the reference crate (its only compressor is the greedy BlockEncoder, k_lz4_encode.hip, whose bytes stay the contract of
// rcx_lz4_encode_batch): an extension, checked by round trips through the reference-faithful decoder and by a structural check of
// the block format (tests).  The output is deterministic: no step depends on the order in which threads or workgroups run.
//
// Segment-parallel, as k_deflate_encode.hip.  Every block is cut into HC_SEG-byte segments, the segments of the batch are flattened;
// matches reach back up to 65535 bytes, across segment boundaries; a segment's parse ends at the segment's end.  Launches:
//   k_hc_plan    one workgroup: exclusive scan of the blocks' segment counts (0 for a block that gets a status of its own)
//   k_hc_links   a workgroup per segment: exact hash chains over the 65535 bytes before the segment and the segment (lzc_links of
//                lz_match.h, shared with DEFLATE's levels 2..9): 16-bit links, per position, 0 = none within 65535
//   k_hc_search  a workgroup per segment: every position walks its chain up to the level's depth and keeps the longest match
//                (the nearest among equals; lzc_search), at most HC_MAXM bytes, ending at least 5 bytes before the block's end and
//                starting at least 12 bytes before it
//   k_hc_parse   a wave per segment: forward min-cost parse.  The cheapest way to reach each position is relaxed in a 64-position
//                register ring (lane = position mod 64; a literal costs 1 byte plus the length byte its run needs at 15, 270, ...;
//                a match of length 4..min(L, 63) 3 bytes plus its length bytes), matches of 64 bytes or more through a 2048-entry LDS
//                ring (u64 atomicMin).  Then the parse is walked back from the segment's end and its matches listed in order; a match
//                that ends where the next starts, at the same distance, is joined with it (runs longer than HC_MAXM)
//   k_hc_scan    a thread per block: serially over its segments, the literal run each segment's first token carries in from the
//                segments before it, the byte offset of each segment's tokens, where each literal byte goes, the final literal-only
//                token; the block falls back to literals only if the parse came out larger than that; statuses
//   k_hc_place   a workgroup per segment: the tokens (a thread per run of tokens, offsets from a block-wide scan), the literals before
//                the first and after the last match (the whole workgroup), the final token's header (the block's last segment)
// Scratch is carved in hc_carve; nothing in it is assumed zero.  Workgroups never talk to each other inside a launch.
#include "lz_match.h"

#define HC_SEG 65536u                  /* bytes per segment */
#define HC_WIN 65535u                  /* largest LZ4 offset */
#define HC_RING 2048u                  /* k_hc_parse's ring of long-match arrivals */
#define HC_MAXM (HC_RING - 64u)        /* longest match the search reports and the parse relaxes (the parse's walk joins adjacent pieces of one run) */
#define HC_TOKCAP 16384u               /* matches a segment can hold (each is >= 4 bytes) */
#define HC_ELEN (HC_SEG + 64u)         /* per-segment entries of the parse's arrival record (positions 0..L) */
#define HC_INF 0xffffffffu

// chain depth per level (1..12): never decreasing
__host__ __device__ static inline uint32_t hc_depth(int level)
{
    return level <= 4 ? (uint32_t)(level < 1 ? 1 : level) : level == 5 ? 6u : level == 6 ? 8u : level == 7 ? 12u : level == 8 ? 16u
         : level == 9 ? 24u : level == 10 ? 64u : level == 11 ? 128u : 256u;
}

struct HcScratch {
    uint32_t* seg_first;   // [n + 1]: first flattened segment of each block; [n] = total
    uint32_t* sflag;       // [n]: 0 = nothing to place, 1 = the parse, 2 = literals only
    uint64_t* blk_ofin;    // [n]: offset of the final literal-only token
    uint64_t* blk_rf;      // [n]: its literal count
    uint32_t* seg_nm;      // [cap]: matches of the segment
    uint32_t* seg_fm;      // [cap]: start of its first match (segment-relative)
    uint32_t* seg_le;      // [cap]: end of its last match
    uint32_t* seg_fx;      // [cap]: its bytes that do not depend on the literals carried in (see k_hc_scan)
    uint64_t* seg_o;       // [cap]: output offset of its first token
    uint64_t* seg_c;       // [cap]: literals carried into its first token
    int64_t* seg_dfirst;   // [cap]: output position - input position of the literals of its first token
    int64_t* seg_dtail;    // [cap]: the same for the literals after its last match
    uint16_t* link;        // [cap * HC_SEG]: chain links, indexed by the block's first segment * HC_SEG + position in the block
    uint32_t* cand;        // [cap * HC_SEG]: longest match per position, length << 16 | distance; later the segment's matches (u64 each)
    uint32_t* elen;        // [cap * HC_ELEN]: the parse's arrival at each position: edge length | distance << 16
    uint32_t cap;          // segments the scratch holds
};

static inline uint64_t hc_al(uint64_t x) { return (x + 255u) & ~255ull; }
static inline uint64_t hc_base_bytes(uint32_t n) { return hc_al(4ull * (n + 1)) + hc_al(4ull * n) + 2 * hc_al(8ull * n) + 256; }
static inline uint64_t hc_seg_bytes() { return 4ull * 4 + 8ull * 4 + 2ull * HC_SEG + 4ull * HC_SEG + 4ull * HC_ELEN; }
static inline uint64_t hc_scratch_bytes(uint32_t n, uint64_t nsegs) { return hc_base_bytes(n) + nsegs * hc_seg_bytes() + 4096; }
__host__ __device__ static inline uint64_t hc_segments(uint64_t len) { return (len + HC_SEG - 1) / HC_SEG; }

static inline HcScratch hc_carve(void* scratch, uint64_t bytes, uint32_t n)
{
    HcScratch d;
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 255u) & ~(uintptr_t)255u);
    const uint64_t used = (uint64_t)(p - (uint8_t*)scratch);
    d.seg_first = (uint32_t*)p; p += hc_al(4ull * (n + 1));
    d.sflag = (uint32_t*)p; p += hc_al(4ull * n);
    d.blk_ofin = (uint64_t*)p; p += hc_al(8ull * n);
    d.blk_rf = (uint64_t*)p; p += hc_al(8ull * n);
    const uint64_t fixed = used + hc_base_bytes(n) + 11 * 256;        // (+ the alignment of the eleven segment arrays)
    uint64_t cap = bytes > fixed ? (bytes - fixed) / hc_seg_bytes() : 0;
    if (cap > 0xffffffffull) cap = 0xffffffffull;
    d.cap = (uint32_t)cap;
    d.seg_nm = (uint32_t*)p; p += hc_al(4ull * cap);
    d.seg_fm = (uint32_t*)p; p += hc_al(4ull * cap);
    d.seg_le = (uint32_t*)p; p += hc_al(4ull * cap);
    d.seg_fx = (uint32_t*)p; p += hc_al(4ull * cap);
    d.seg_o = (uint64_t*)p; p += hc_al(8ull * cap);
    d.seg_c = (uint64_t*)p; p += hc_al(8ull * cap);
    d.seg_dfirst = (int64_t*)p; p += hc_al(8ull * cap);
    d.seg_dtail = (int64_t*)p; p += hc_al(8ull * cap);
    d.cand = (uint32_t*)p; p += hc_al(4ull * HC_SEG * cap);
    d.elen = (uint32_t*)p; p += hc_al(4ull * HC_ELEN * cap);
    d.link = (uint16_t*)p;
    return d;
}

// length bytes of a literal run / of a match of length l (the token's nibble holds 0..14, then 255s and a remainder byte)
__host__ __device__ __forceinline__ uint64_t hc_lext(uint64_t r) { return r >= 15 ? 1 + (r - 15) / 255 : 0; }
__device__ __forceinline__ uint32_t hc_mext(uint32_t l) { return l >= 19 ? 1 + (l - 19) / 255 : 0; }

// why a block gets a status of its own and no segments: too large for LZ4, or a slot smaller than the compression bound
__device__ __forceinline__ int hc_block_status(const rcx_kargs& a, uint32_t b)
{
    const uint64_t len = a.in_len[b];
    return len > 0x7e000000ull ? RCX_E_LZ4_INPUT_TOO_LARGE : a.out_cap[b] < len + len / 255 + 20 ? RCX_E_OUTPUT_TOO_SMALL : RCX_OK;
}

__device__ __forceinline__ LzcSeg hc_seg(const rcx_kargs& a, const HcScratch& d, uint32_t g) { return lzc_seg<HC_SEG>(a, d.seg_first, g); }
__device__ __forceinline__ uint32_t hc_lim(const rcx_kargs& a, const HcScratch& d) { return lzc_lim(a, d.seg_first, d.cap); }

__global__ __launch_bounds__(1024) void k_hc_plan(rcx_kargs a, HcScratch d)
{
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_carry;
    lzc_plan(a.nblocks, d.seg_first, s_ws, &s_carry,
             [&](uint32_t b) { return hc_block_status(a, b) == RCX_OK ? (uint32_t)hc_segments(a.in_len[b]) : 0u; });
}

__global__ __launch_bounds__(256) void k_hc_links(rcx_kargs a, HcScratch d)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        lzc_links<HC_WIN>(s, d.link + (uint64_t)s.f0 * HC_SEG, s_head, s_hc);
    }
}

// LZ4's matches: at most HC_MAXM bytes, the last one starts 12 bytes before the block's end at the latest and ends 5 bytes before it
struct HcMatch {
    static constexpr uint32_t WIN = HC_WIN;
    static __device__ __forceinline__ uint32_t maxl(const LzcSeg& s, uint32_t i)
    {
        const uint32_t left = s.len - s.s0 - i;
        return left < 12 ? 0u : left - 5 < HC_MAXM ? left - 5 : HC_MAXM;
    }
    static __device__ __forceinline__ uint32_t pack(uint32_t len, uint32_t dist) { return (len << 16) | dist; }
};

__global__ __launch_bounds__(256) void k_hc_search(rcx_kargs a, HcScratch d, uint32_t depth)
{
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        lzc_search<HcMatch>(s, d.link + (uint64_t)s.f0 * HC_SEG, d.cand + (uint64_t)g * HC_SEG, depth);
    }
}

// one wave per segment (a workgroup of 64 threads)
__global__ __launch_bounds__(64) void k_hc_parse(rcx_kargs a, HcScratch d)
{
    __shared__ uint64_t s_far[HC_RING];                   // arrivals of matches of 64 bytes or more: key << 32 | distance
    const uint32_t lane = rcx_lane();
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        const uint32_t L = s.L;
        uint32_t* cand = d.cand + (uint64_t)g * HC_SEG;
        uint32_t* elen = d.elen + (uint64_t)g * HC_ELEN;
        for (uint32_t i = lane; i < HC_RING; i += 64) s_far[i] = ~0ull;
        __builtin_amdgcn_wave_barrier();
        // key = cost << 13 | (8191 - edge length): the cheapest arrival, the longer edge among equals; run = literals since the last match
        uint32_t key = lane == 0 ? 0u : HC_INF, run = 0, dis = 0;
        uint32_t cn = lane < L ? cand[lane] : 0u;
        for (uint32_t W = 0; W <= L; W += 64) {
            const uint32_t cw = cn;
            cn = W + 64 + lane < L ? cand[W + 64 + lane] : 0u;               // (the next window's, early)
            {
                const uint32_t slot = (W + lane) & (HC_RING - 1);
                const uint64_t fw = s_far[slot];
                __builtin_amdgcn_wave_barrier();
                s_far[slot] = ~0ull;
                __builtin_amdgcn_wave_barrier();
                if ((uint32_t)(fw >> 32) < key) { key = (uint32_t)(fw >> 32); run = 0; dis = (uint32_t)fw; }
            }
            uint32_t er = 0;                                                  // this lane's position's arrival edge
            const uint32_t jn = L - W < 63 ? L - W : 63;
            for (uint32_t j = 0; j <= jn; j++) {
                const uint32_t p = W + j;
                const uint32_t bk = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)j);
                const uint32_t br = (uint32_t)__builtin_amdgcn_readlane((int)run, (int)j);
                if (lane == j) { er = (8191u - (key & 8191u)) | (dis << 16); key = HC_INF; run = 0; }
                if (p == L) break;
                const uint32_t cost = bk >> 13;
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cw, (int)j);
                uint32_t ml = c >> 16;
                if (ml > L - p) ml = L - p;                                   // (segments parse independently)
                const uint32_t dd = (lane - j) & 63u;
                uint32_t nk = HC_INF, nr = 0;
                if (dd == 1) {
                    const uint32_t r1 = br + 1;
                    nk = ((cost + 1 + (r1 >= 15 && (r1 - 15) % 255 == 0 ? 1u : 0u)) << 13) | (8191u - 1);
                    nr = r1;
                } else if (dd >= 4 && dd <= ml) nk = ((cost + 3 + hc_mext(dd)) << 13) | (8191u - dd);
                if (nk < key) { key = nk; run = nr; dis = c & 0xffffu; }
                if (ml >= 64 && lane == 0) {
                    const uint64_t v = ((uint64_t)(((cost + 3 + hc_mext(ml)) << 13) | (8191u - ml)) << 32) | (c & 0xffffu);
                    atomicMin(&s_far[(p + ml) & (HC_RING - 1)], v);
                }
            }
            if (W + lane <= L) elen[W + lane] = er;
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                                      // (the arrivals, written above, are read below)
        // walk back from L: a run of literal arrivals is skipped a window at a time; every match is listed from the end of the region
        uint64_t* tok = (uint64_t*)cand;                                      // (the candidates are done with)
        uint32_t q = L, nm = 0, fx = 0, le = 0, nxt = 0, nl = 0, nd = 0;   // (nl, nd: the length and distance of the match listed last)
        while (q > 0) {
            const uint32_t Wq = q & ~63u;
            const uint32_t e = Wq + lane <= q ? elen[Wq + lane] : 0u;
            const unsigned long long mm = __ballot((e & 0xffffu) > 1 && Wq + lane >= 1);
            if (!mm) { q = Wq ? Wq - 1 : 0; continue; }
            const uint32_t x = Wq + 63 - (uint32_t)__clzll(mm);
            const uint32_t ex = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)(x - Wq));
            const uint32_t el = ex & 0xffffu, st = x - el, dist = ex >> 16;
            if (nm && x == nxt && dist == nd && nl + el <= 0xffffu) {
                // the match ends where the next one starts, at the same distance: one match (a run longer than HC_MAXM, whose pieces
                // would cost a token, an offset and length bytes each), as long as its length fits the token's 16 bits (a whole
                // segment, 65536 bytes, does not)
                fx -= 3 + hc_mext(nl);
                nl += el;
                fx += 3 + hc_mext(nl);
                if (lane == 0) tok[HC_TOKCAP - nm] = (uint64_t)st | ((uint64_t)nl << 16) | ((uint64_t)dist << 32);
            } else {
                fx += 3 + hc_mext(el);
                if (nm) { const uint32_t r = nxt - x; fx += r + (uint32_t)hc_lext(r); }
                else le = x;
                if (lane == 0) tok[HC_TOKCAP - 1 - nm] = (uint64_t)st | ((uint64_t)el << 16) | ((uint64_t)dist << 32);
                nm++;
                nl = el; nd = dist;
            }
            nxt = st;
            q = st;
        }
        if (lane == 0) { d.seg_nm[g] = nm; d.seg_fm[g] = nxt; d.seg_le[g] = le; d.seg_fx[g] = fx; }
        __syncthreads();
    }
}

// a thread per block
__global__ __launch_bounds__(64) void k_hc_scan(rcx_kargs a, HcScratch d)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint64_t len = a.in_len[b];
    int st = hc_block_status(a, b);
    const uint32_t f0 = d.seg_first[b], f1 = d.seg_first[b + 1];
    if (!st && f1 > d.cap) st = RCX_E_MALFORMED;                      // scratch smaller than rcx_lz4_hc_scratch_bytes asked for
    uint64_t total = 0;
    uint32_t flag = 0;
    if (!st) {
        uint64_t o = 0, c = 0;
        for (uint32_t g = f0; g < f1; g++) {
            const uint64_t L = len - (uint64_t)(g - f0) * HC_SEG < HC_SEG ? len - (uint64_t)(g - f0) * HC_SEG : HC_SEG;
            d.seg_o[g] = o; d.seg_c[g] = c;
            if (d.seg_nm[g]) {
                const uint64_t r0 = c + d.seg_fm[g];
                o += d.seg_fx[g] + r0 + hc_lext(r0);
                c = L - d.seg_le[g];
            } else c += L;
        }
        total = o + 1 + hc_lext(c) + c;
        const uint64_t lits = 1 + hc_lext(len) + len;
        flag = 1;
        if (total > lits) { flag = 2; total = lits; o = 0; c = len; }     // (never larger than the block as literals)
        d.blk_ofin[b] = o; d.blk_rf[b] = c;
        int64_t dc = (int64_t)(o + 1 + hc_lext(c)) - (int64_t)(len - c);
        for (uint32_t g = f1; g-- > f0;) {
            d.seg_dtail[g] = dc;
            if (flag == 1 && d.seg_nm[g]) {
                const uint64_t cg = d.seg_c[g], r0 = cg + d.seg_fm[g];
                dc = (int64_t)(d.seg_o[g] + 1 + hc_lext(r0)) - (int64_t)((uint64_t)(g - f0) * HC_SEG - cg);
                d.seg_dfirst[g] = dc;
            }
        }
        if (len == 0) a.out_base[a.out_off[b]] = 0;                    // an empty block: one token, no literals
    }
    d.sflag[b] = st ? 0u : len ? flag : 0u;
    a.status[b] = st;
    a.out_len[b] = st ? 0 : total;
    if (a.in_used) a.in_used[b] = st ? 0 : len;
}

// a literal run's length bytes at o (r >= 15), by the whole workgroup
__device__ __forceinline__ void hc_put_ext(uint8_t* o, uint64_t r)
{
    const uint64_t x = r - 15, n255 = x / 255;
    for (uint64_t i = threadIdx.x; i < n255; i += blockDim.x) o[i] = 255;
    if (threadIdx.x == 0) o[n255] = (uint8_t)(x - n255 * 255);
}

__global__ __launch_bounds__(256) void k_hc_place(rcx_kargs a, HcScratch d)
{
    __shared__ uint32_t s_ws[8];
    const uint32_t tid = threadIdx.x;
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        const uint32_t flag = d.sflag[s.b];
        if (!flag) continue;                                               // (uniform: the whole workgroup moves on)
        uint8_t* out = a.out_base + a.out_off[s.b];
        const uint32_t nm = flag == 1 ? d.seg_nm[g] : 0u;
        const uint64_t* tok = (const uint64_t*)(d.cand + (uint64_t)g * HC_SEG) + (HC_TOKCAP - nm);
        if (nm) {
            // the tokens: thread t writes tokens [k0, k1); the first token's literals (partly carried in) and their length bytes are below
            const uint32_t per = (nm + blockDim.x - 1) / blockDim.x;
            const uint32_t k0 = tid * per < nm ? tid * per : nm, k1 = k0 + per < nm ? k0 + per : nm;
            const uint64_t c = d.seg_c[g];
            uint64_t sz = 0;
            for (uint32_t k = k0; k < k1; k++) {
                const uint64_t t = tok[k];
                const uint32_t m = (uint32_t)t & 0xffffu, l = (uint32_t)(t >> 16) & 0xffffu;
                const uint64_t r = k ? m - ((uint32_t)tok[k - 1] & 0xffffu) - ((uint32_t)(tok[k - 1] >> 16) & 0xffffu) : c + m;
                sz += 3 + r + hc_lext(r) + hc_mext(l);
            }
            uint32_t tot;
            uint64_t o = d.seg_o[g] + lzc_block_excl_scan((uint32_t)sz, s_ws, tot);    // (a segment's tokens: < 2^32 bytes, the first one's literals aside)
            for (uint32_t k = k0; k < k1; k++) {
                const uint64_t t = tok[k];
                const uint32_t m = (uint32_t)t & 0xffffu, l = (uint32_t)(t >> 16) & 0xffffu, dist = (uint32_t)(t >> 32);
                const uint32_t pe = k ? ((uint32_t)tok[k - 1] & 0xffffu) + ((uint32_t)(tok[k - 1] >> 16) & 0xffffu) : 0u;
                const uint64_t r = k ? m - pe : c + m;
                out[o] = (uint8_t)(((r > 14 ? 15u : (uint32_t)r) << 4) | (l - 4 > 14 ? 15u : l - 4));
                o += 1;
                if (k) {
                    if (r >= 15) { uint64_t x = r - 15; while (x >= 255) { out[o++] = 255; x -= 255; } out[o++] = (uint8_t)x; }
                    for (uint32_t i = 0; i < r; i++) out[o + i] = s.in[s.s0 + pe + i];
                } else o += hc_lext(r);
                o += r;
                out[o] = (uint8_t)dist; out[o + 1] = (uint8_t)(dist >> 8);
                o += 2;
                if (l >= 19) { uint32_t x = l - 19; while (x >= 255) { out[o++] = 255; x -= 255; } out[o++] = (uint8_t)x; }
            }
            // the first token: its run's length bytes, the run's bytes that lie in this segment
            const uint64_t r0 = c + ((uint32_t)tok[0] & 0xffffu);
            if (r0 >= 15) hc_put_ext(out + d.seg_o[g] + 1, r0);
            const int64_t df = d.seg_dfirst[g];
            const uint32_t fm = (uint32_t)tok[0] & 0xffffu;
            for (uint32_t i = tid; i < fm; i += blockDim.x) out[(uint64_t)((int64_t)(s.s0 + i) + df)] = s.in[s.s0 + i];
        }
        // the literals after the last match (all of them without a match) go to the next token that has a match, or to the final token
        const uint32_t le = nm ? d.seg_le[g] : 0u;
        const int64_t dt = d.seg_dtail[g];
        for (uint32_t i = le + tid; i < s.L; i += blockDim.x) out[(uint64_t)((int64_t)(s.s0 + i) + dt)] = s.in[s.s0 + i];
        if (g + 1 == d.seg_first[s.b + 1]) {                               // the block's last segment: the final token's header
            const uint64_t of = d.blk_ofin[s.b], rf = d.blk_rf[s.b];
            if (tid == 0) out[of] = (uint8_t)((rf > 14 ? 15u : (uint32_t)rf) << 4);
            if (rf >= 15) hc_put_ext(out + of + 1, rf);
        }
        __syncthreads();
    }
}

// the whole encode on stream s at `level` (1..12); k.scratch holds hc_scratch_bytes(n, segments) bytes
static int launch_lz4_hc(hipStream_t s, rcx_kargs& k, int level, std::string& err)
{
    const uint32_t n = k.nblocks;
    if (level < 1 || level > 12) { err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < hc_scratch_bytes(n, 0)) { err = "lz4 hc: scratch too small"; return RCX_RC_BAD_ARG; }
    const HcScratch d = hc_carve(k.scratch, k.scratch_bytes, n);
    hipLaunchKernelGGL(k_hc_plan, dim3(1), dim3(1024), 0, s, k, d);
    if (d.cap) {
        const uint32_t gs = d.cap < 8192u ? d.cap : 8192u;
        hipLaunchKernelGGL(k_hc_links, dim3(gs), dim3(256), 0, s, k, d);
        hipLaunchKernelGGL(k_hc_search, dim3(gs), dim3(256), 0, s, k, d, hc_depth(level));
        hipLaunchKernelGGL(k_hc_parse, dim3(gs), dim3(64), 0, s, k, d);
    }
    hipLaunchKernelGGL(k_hc_scan, dim3((n + 63) / 64), dim3(64), 0, s, k, d);
    if (d.cap) hipLaunchKernelGGL(k_hc_place, dim3(d.cap < 8192u ? d.cap : 8192u), dim3(256), 0, s, k, d);
    return RCX_RC_OK;
}
