// k_deflate_hc.hip -- compression levels 2..9 of the batched DEFLATE / zlib / gzip encoder: hash chains searched to a level-dependent
// depth and a min-cost parse priced by Huffman code lengths.  Level 1 is k_deflate_encode.hip's encoder, byte for byte.
//
// NOT in the reference crate (it has no DEFLATE encoder): an extension, checked like k_deflate_encode.hip by any RFC 1951 decoder.
// Include it after k_deflate_encode.hip: it reuses that file's plan, checksum, scan and place kernels and its DeScratch staging, and
// builds each block as k_de_segment does (dh_block, a copy of its phases 3-7: histograms, trees, the cheapest block type by exact bit
// count, the packed bits).  Only the per-segment parse is new.  Launches, in stream order (the ones of k_deflate_encode.hip in brackets):
//   [k_de_plan, k_de_segs + k_adler32 / k_crc32]
//   k_dh_links   a workgroup per segment: exact hash chains over the 32 KiB before the segment and the segment itself (lzc_links of
//                lz_match.h, shared with LZ4 HC): 16-bit links, 0 = none within 32768, indexed by the stream's first segment *
//                DE_SEG + position in the stream, so the window's links are the previous segment's
//   k_dh_search  a workgroup per segment: every position walks its chain up to the level's depth and keeps the longest match (the
//                nearest among equals; lzc_search) of at least 4 bytes, at most 258 and not past the segment's end; it stops at a
//                258-byte match
//   k_dh_price   a workgroup per segment: a parse walked from the segment's start (the greedy one over the longest matches, or the
//                previous min-cost parse), its literal/length and distance histograms, and from them code lengths (15 bits at most)
//                of frequencies 8 f + 1 -- every symbol gets a price, the unseen ones a high one
//   k_dh_parse   a wave per segment: forward min-cost parse in bits.  Every position relaxes its literal and every match length
//                3..L at its longest match's distance (RFC 1951 allows any length at a distance that matches L bytes): lengths up to 63
//                in a 64-position register ring (lane = position mod 64), lengths 64..258 through a 512-entry LDS ring of arrivals
//                (u64 atomicMin).  Then the parse is walked back from the segment's end and written into DeScratch.pos at its token
//                starts (length << 16 | distance - 1, 0 = a literal)
//   (levels 7..9 price and parse a second time, priced by the first parse's own histograms)
//   k_dh_block   a workgroup per segment: dh_block over the parse -- the block is the cheapest of stored, fixed, dynamic Huffman of the
//                parse and dynamic Huffman of every byte as a literal, so rcx_deflate_compression_bound holds at every level
//   [k_de_scan, k_de_place]
//   k_dh_head    a thread per stream: the header fields of the level (zlib FLEVEL, gzip XFL) in every stream that was written
// The output is deterministic: no step depends on the order in which threads or workgroups run (atomicMax / atomicMin pick the same
// entry in any order).  Scratch is carved in dh_carve; nothing in it is assumed zero.

#define DH_RING 512u                   /* k_dh_parse's ring of long-match arrivals (> 63 + 258 positions ahead) */
#define DH_ELEN (DE_SEG + 64u)         /* per-segment entries of the parse's arrival record (positions 0..L) */
#define DH_INF 0xffffffffu

// chain depth per level (2..9) and the parses (levels from DH_ITER on price and parse twice)
__host__ __device__ static inline uint32_t dh_depth(int level)
{
    return level <= 2 ? 4u : level == 3 ? 8u : level == 4 ? 16u : level == 5 ? 32u : level == 6 ? 64u : level == 7 ? 96u
         : level == 8 ? 160u : 256u;
}
#define DH_ITER 7

struct DhScratch {
    uint16_t* link;        // [cap * DE_SEG]: chain links, indexed by the stream's first segment * DE_SEG + position in the stream
    uint32_t* cand;        // [cap * DE_SEG]: longest match per position: length << 16 | distance - 1, 0 = none
    uint32_t* elen;        // [cap * DH_ELEN]: the parse's arrival at each position: edge length | distance - 1 << 16
    uint8_t* price;        // [cap * 320]: code lengths that price the parse, literal/length [288] then distance [32]
};

static inline uint64_t dh_seg_bytes() { return 2ull * DE_SEG + 4ull * DE_SEG + 4ull * DH_ELEN + 320; }
// DeScratch for nsegs segments, then the chains, matches, arrivals and prices (+ their alignment)
static inline uint64_t dh_scratch_bytes(uint32_t n, uint64_t nsegs) { return de_scratch_bytes(n, nsegs) + nsegs * dh_seg_bytes() + 1024; }

static inline DeScratch dh_carve(void* scratch, uint64_t bytes, uint32_t n, DhScratch& h)
{
    const uint64_t fixed = dh_scratch_bytes(n, 0);
    uint64_t cap = bytes > fixed ? (bytes - fixed) / (de_seg_bytes() + dh_seg_bytes()) : 0;
    if (cap > 0xffffffffull) cap = 0xffffffffull;
    const uint64_t de = de_scratch_bytes(n, cap);
    const DeScratch d = de_carve(scratch, de, n);             // (d.cap == cap: de_scratch_bytes leaves less than a segment over)
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + de + 255u) & ~(uintptr_t)255u);
    h.link = (uint16_t*)p; p += de_al(2ull * DE_SEG * cap);
    h.cand = (uint32_t*)p; p += de_al(4ull * DE_SEG * cap);
    h.elen = (uint32_t*)p; p += de_al(4ull * DH_ELEN * cap);
    h.price = p;
    return d;
}

// k_dh_block's LDS and block builder: phases 3-7 of k_de_segment, copied -- a fix to one must be made in the other.  (Factored into
// one __device__ function that both kernels called, in two forms, k_de_segment compiled to different code and took 1.7-11 % longer on
// an MI355X; so it keeps its own.  DESIGN 3.12 has the forms and their times.)
struct DhLds {
    uint32_t big[DE_BIGW];                                // hash table (phases 1-2), then the packed block (phase 7)
    uint64_t start[DE_SEG / 64];                          // token starts of the parse
    uint32_t lf[288], df[32];                             // frequencies of the parse
    uint8_t ll[2][288], dl[2][32], cl[2][19];             // code lengths of the two parses
    uint16_t rle[2][320];                                 // their code-length code items: symbol | extra value << 5
    uint32_t ws[16];
    uint32_t x[24];                                       // extra bits, header bits, choice; per parse: hlit hdist hclen items cost
    // one region, three lives: the round's candidate distances (phase 2); byte histogram + tree building (phases 4-5); codes (phase 7)
    uint32_t tmp[256 + 339 + 288 + 170];
};

// the token starts of the parse p += max(1, pos[p] >> 16) from 0 as a bitmap, by the first wave: lane i holds the match length at
// window position i, the walk reads it with readlane
__device__ __forceinline__ void dh_walk(uint64_t* s_start, const uint32_t* pos, uint32_t L)
{
    const uint32_t lane = rcx_lane();
    if (threadIdx.x < 64) {
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
}

// phases 3-7 of k_de_segment: the parse (pos[p] at every token start: length << 16 | distance - 1, 0 = a literal) walked,
// histograms, trees, the cheapest block type, the packed bits staged.  S.lf, S.df and S.x hold zeros when it starts.
__device__ __forceinline__ void dh_block(DhLds& S, const DeScratch& d, uint32_t g, const uint8_t* in, uint32_t s0, uint32_t L,
                                         const uint32_t* pos)
{
    uint32_t* const s_big = S.big;
    uint64_t* const s_start = S.start;
    uint32_t* const s_lf = S.lf; uint32_t* const s_df = S.df;
    uint8_t (*const s_ll)[288] = S.ll; uint8_t (*const s_dl)[32] = S.dl; uint8_t (*const s_cl)[19] = S.cl;
    uint16_t (*const s_rle)[320] = S.rle;
    uint32_t* const s_ws = S.ws; uint32_t* const s_x = S.x;
    uint32_t* const s_tmp = S.tmp;
    uint32_t* const s_bf = s_tmp;                         // [256] every byte of the segment
    uint32_t* const s_tf = s_tmp + 256;                   // [288 + 32 + 19] frequencies that shape the trees (two symbols at least)
    uint32_t* const s_A = s_tmp + 256 + 339;              // [288]
    uint16_t* const s_sort = (uint16_t*)(s_tmp + 256 + 339 + 288);   // [339]
    uint16_t* const s_lc = (uint16_t*)s_tmp;              // [288 + 32 + 19] the chosen codes
    uint16_t* const s_dc = s_lc + 288;
    uint16_t* const s_cc = s_lc + 320;
    const uint32_t tid = threadIdx.x, lane = rcx_lane();

    // 3. greedy parse
    dh_walk(s_start, pos, L);
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
}

__global__ __launch_bounds__(256) void k_dh_links(rcx_kargs a, DeScratch d, DhScratch h)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        lzc_links<DE_WIN>(s, h.link + (uint64_t)s.f0 * DE_SEG, s_head, s_hc);
    }
}

// DEFLATE's matches: at most 258 bytes and not past the segment's end (its block); the distance is stored less one
struct DhMatch {
    static constexpr uint32_t WIN = DE_WIN;
    static __device__ __forceinline__ uint32_t maxl(const LzcSeg& s, uint32_t i) { return s.L - i < 258 ? s.L - i : 258; }
    static __device__ __forceinline__ uint32_t pack(uint32_t len, uint32_t dist) { return (len << 16) | (dist - 1); }
};

__global__ __launch_bounds__(256) void k_dh_search(rcx_kargs a, DeScratch d, DhScratch h, uint32_t depth)
{
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        lzc_search<DhMatch>(s, h.link + (uint64_t)s.f0 * DE_SEG, h.cand + (uint64_t)g * DE_SEG, depth);
    }
}

// from_parse 0: the greedy parse of the longest matches (h.cand); 1: the min-cost parse in d.pos
__global__ __launch_bounds__(DE_T) void k_dh_price(rcx_kargs a, DeScratch d, DhScratch h, uint32_t from_parse)
{
    __shared__ uint64_t s_start[DE_SEG / 64];
    __shared__ uint32_t s_f[288 + 32];                    // literal/length then distance frequencies, then the weights
    __shared__ uint32_t s_A[288];
    __shared__ uint16_t s_sort[288 + 32];
    __shared__ uint8_t s_len[288 + 32];
    const uint32_t tid = threadIdx.x;
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        const uint32_t* src = (from_parse ? d.pos : h.cand) + (uint64_t)g * DE_SEG;
        for (uint32_t i = tid; i < 288 + 32; i += DE_T) { s_f[i] = 0; s_len[i] = 0; }
        __syncthreads();
        dh_walk(s_start, src, s.L);
        __syncthreads();
        const uint32_t r0 = tid * DE_RANGE, r1 = r0 + DE_RANGE < s.L ? r0 + DE_RANGE : s.L;
        for (uint32_t p = r0; p < r1; p++) {
            if (!((s_start[p >> 6] >> (p & 63)) & 1ull)) continue;
            const uint32_t m = src[p];
            if (m) {
                uint32_t ls, le, lv, ds, de, dv;
                de_len_sym(m >> 16, ls, le, lv);
                de_dist_sym((m & 0xffffu) + 1, ds, de, dv);
                atomicAdd(&s_f[ls], 1u); atomicAdd(&s_f[288 + ds], 1u);
            } else atomicAdd(&s_f[s.in[s.s0 + p]], 1u);
        }
        if (tid == 0) atomicAdd(&s_f[256], 1u);
        __syncthreads();
        for (uint32_t i = tid; i < 288 + 32; i += DE_T) s_f[i] = (i < 286 || (i >= 288 && i < 318)) ? 8 * s_f[i] + 1 : 0u;
        __syncthreads();
        de_rank_sort(s_f, 286, s_sort);
        de_rank_sort(s_f + 288, 30, s_sort + 288);
        __syncthreads();
        if (tid == 0) {
            de_code_lengths(s_f, s_sort, 286, 15, s_len, s_A);
            de_code_lengths(s_f + 288, s_sort + 288, 30, 15, s_len + 288, s_A);
        }
        __syncthreads();
        uint8_t* pr = h.price + (uint64_t)g * 320;
        for (uint32_t i = tid; i < 320; i += DE_T) pr[i] = s_len[i];
        __syncthreads();
    }
}

// one wave per segment (a workgroup of 64 threads)
__global__ __launch_bounds__(64) void k_dh_parse(rcx_kargs a, DeScratch d, DhScratch h)
{
    __shared__ uint64_t s_far[DH_RING];                   // arrivals of matches of 64 bytes or more: key << 32 | distance - 1
    __shared__ uint16_t s_lc[259];                        // bits of a match length: its code + extra bits
    __shared__ uint8_t s_lit[256], s_dl[32];
    const uint32_t lane = rcx_lane();
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        const uint32_t L = s.L;
        const uint8_t* in = s.in + s.s0;
        const uint32_t* cand = h.cand + (uint64_t)g * DE_SEG;
        uint32_t* elen = h.elen + (uint64_t)g * DH_ELEN;
        uint32_t* pos = d.pos + (uint64_t)g * DE_SEG;
        const uint8_t* pr = h.price + (uint64_t)g * 320;
        for (uint32_t i = lane; i < DH_RING; i += 64) s_far[i] = ~0ull;
        for (uint32_t i = lane; i < 256; i += 64) s_lit[i] = pr[i];
        if (lane < 32) s_dl[lane] = pr[288 + lane];
        for (uint32_t l = lane; l < 259; l += 64) {
            uint32_t ls = 0, le = 0, lv;
            if (l >= 3) de_len_sym(l, ls, le, lv);
            s_lc[l] = (uint16_t)(l >= 3 ? pr[ls] + le : 0u);
        }
        __syncthreads();
        uint32_t lcf[4];                                  // this lane's long lengths 64 (k + 1) + lane and their bits
        for (int k = 0; k < 4; k++) { const uint32_t l = 64 * (k + 1) + lane; lcf[k] = l <= 258 ? s_lc[l] : 0u; }
        // key = cost << 9 | (511 - edge length): the cheapest arrival, the longer edge among equals
        uint32_t key = lane == 0 ? 511u : DH_INF, dis = 0;
        uint32_t cn = lane < L ? cand[lane] : 0u;
        for (uint32_t W = 0; W <= L; W += 64) {
            const uint32_t cw = cn;
            cn = W + 64 + lane < L ? cand[W + 64 + lane] : 0u;               // (the next window's, early)
            const uint32_t litw = W + lane < L ? s_lit[in[W + lane]] : 0u;   // this lane's position: its literal's bits ...
            uint32_t dcw = 0;                                                 // ... and its match distance's
            if (cw) { uint32_t ds, de, dv; de_dist_sym((cw & 0xffffu) + 1, ds, de, dv); dcw = s_dl[ds] + de; }
            {
                const uint32_t slot = (W + lane) & (DH_RING - 1);
                const uint64_t fw = s_far[slot];
                __builtin_amdgcn_wave_barrier();
                s_far[slot] = ~0ull;
                __builtin_amdgcn_wave_barrier();
                if ((uint32_t)(fw >> 32) < key) { key = (uint32_t)(fw >> 32); dis = (uint32_t)fw; }
            }
            uint32_t er = 0;                                                  // this lane's position's arrival edge
            const uint32_t jn = L - W < 63 ? L - W : 63;
            for (uint32_t j = 0; j <= jn; j++) {
                const uint32_t p = W + j;
                const uint32_t bk = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)j);
                if (lane == j) { er = (511u - (key & 511u)) | (dis << 16); key = DH_INF; }
                if (p == L) break;
                const uint32_t cost = bk >> 9;
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cw, (int)j);
                const uint32_t ml = c >> 16;
                const uint32_t dc = cost + (uint32_t)__builtin_amdgcn_readlane((int)dcw, (int)j);
                const uint32_t lc = cost + (uint32_t)__builtin_amdgcn_readlane((int)litw, (int)j);
                const uint32_t dd = (lane - j) & 63u;
                uint32_t nk = DH_INF;
                if (dd == 1) nk = (lc << 9) | 510u;
                else if (dd >= 3 && dd <= ml) nk = ((dc + s_lc[dd]) << 9) | (511u - dd);
                if (nk < key) { key = nk; dis = dd == 1 ? 0u : c & 0xffffu; }
                if (ml >= 64) {
                    for (int k = 0; k < 4; k++) {
                        const uint32_t l = 64 * (k + 1) + lane;
                        if (l <= ml) atomicMin(&s_far[(p + l) & (DH_RING - 1)], ((uint64_t)(((dc + lcf[k]) << 9) | (511u - l)) << 32) | (c & 0xffffu));
                    }
                }
            }
            if (W + lane <= L) elen[W + lane] = er;
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                                      // (the arrivals, written above, are read below)
        // walk back from L: the arrivals from q down to the highest match arrival x are literals (bytes x..q-1: pos 0), the match
        // arriving at x starts at x - its length (pos: the match); a window's arrivals are loaded once
        uint32_t q = L, Wc = ~0u, e = 0;
        while (q > 0) {
            const uint32_t Wq = q & ~63u;
            if (Wq != Wc) { e = elen[Wq + lane]; Wc = Wq; }                   // (Wq + lane <= Wq + 63 < DH_ELEN)
            const bool arr = Wq + lane <= q && Wq + lane >= 1;
            const unsigned long long mm = __ballot(arr && (e & 0xffffu) > 1);
            const uint32_t x = mm ? Wq + 63 - (uint32_t)__clzll(mm) : (Wq ? Wq - 1 : 0);
            if (arr && Wq + lane > x) pos[Wq + lane - 1] = 0;                 // (literal bytes)
            if (!mm) { q = x; continue; }
            const uint32_t ex = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)(x - Wq));
            const uint32_t el = ex & 0xffffu, st = x - el;
            if (lane == 0) pos[st] = (el << 16) | (ex >> 16);
            q = st;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DE_T) void k_dh_block(rcx_kargs a, DeScratch d)
{
    __shared__ DhLds S;
    const uint32_t tid = threadIdx.x;
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        for (uint32_t i = tid; i < 288; i += DE_T) S.lf[i] = 0;
        if (tid < 32) S.df[tid] = 0;
        if (tid < 24) S.x[tid] = 0;
        __syncthreads();
        dh_block(S, d, g, s.in, s.s0, s.L, d.pos + (uint64_t)g * DE_SEG);
        __syncthreads();
    }
}

// the level's header fields in every stream k_de_scan passed (level 2..9): zlib FLEVEL (78 5E / 78 9C / 78 DA), gzip XFL (2 at 9)
template <int FMT>
__global__ __launch_bounds__(256) void k_dh_head(rcx_kargs a, uint32_t level)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks || a.status[b] != RCX_OK) return;
    uint8_t* o = a.out_base + a.out_off[b];
    if (FMT == DE_ZLIB) o[1] = level <= 5 ? 0x5e : level == 6 ? 0x9c : 0xda;   // (0x785e, 0x789c, 0x78da: each % 31 == 0)
    if (FMT == DE_GZIP) o[8] = level == 9 ? 2 : 0;
}

// the whole encode on stream s at `level` (1..9; 1 is launch_deflate_encode); k.scratch holds dh_scratch_bytes(n, segments) bytes
static int launch_deflate_level(hipStream_t s, rcx_kargs& k, int fmt, int level, std::string& err, void (*cks)(hipStream_t, rcx_kargs&))
{
    const uint32_t n = k.nblocks;
    if (level < 1 || level > 9) { err = "deflate encode: level must be 1..9"; return RCX_RC_BAD_ARG; }
    if (level == 1) return launch_deflate_encode(s, k, fmt, err, cks);
    if (!k.scratch || k.scratch_bytes < dh_scratch_bytes(n, 0)) { err = "deflate encode: scratch too small"; return RCX_RC_BAD_ARG; }
    DhScratch h;
    const DeScratch d = dh_carve(k.scratch, k.scratch_bytes, n, h);
    hipLaunchKernelGGL(k_de_plan, dim3(1), dim3(1024), 0, s, k, d);
    if (fmt != DE_RAW && d.cap) {
        hipLaunchKernelGGL(k_de_segs, dim3(d.cap < 65536u * 4u ? (d.cap + 255) / 256 : 1024u), dim3(256), 0, s, k, d);
        rcx_kargs kc = k;                                 // a wave per segment
        kc.in_off = d.seg_ioff; kc.in_len = d.seg_ilen; kc.nblocks = d.cap;
        kc.out_len = nullptr; kc.in_used = nullptr; kc.status = nullptr; kc.aux = d.seg_cks;
        cks(s, kc);
    }
    if (d.cap) {
        const dim3 gs(d.cap < 8192u ? d.cap : 8192u);
        hipLaunchKernelGGL(k_dh_links, gs, dim3(256), 0, s, k, d, h);
        hipLaunchKernelGGL(k_dh_search, gs, dim3(256), 0, s, k, d, h, dh_depth(level));
        for (uint32_t it = 0; it < (level >= DH_ITER ? 2u : 1u); it++) {
            hipLaunchKernelGGL(k_dh_price, gs, dim3(DE_T), 0, s, k, d, h, it);
            hipLaunchKernelGGL(k_dh_parse, gs, dim3(64), 0, s, k, d, h);
        }
        hipLaunchKernelGGL(k_dh_block, dim3(d.cap < 2048u ? d.cap : 2048u), dim3(DE_T), 0, s, k, d);
    }
    const dim3 gs((n + 3) / 4), gp(d.cap < 4096u ? d.cap : 4096u), gh((n + 255) / 256);
    if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_scan<DE_RAW>, gs, dim3(256), 0, s, k, d);
    else if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_de_scan<DE_ZLIB>, gs, dim3(256), 0, s, k, d);
    else hipLaunchKernelGGL(k_de_scan<DE_GZIP>, gs, dim3(256), 0, s, k, d);
    if (d.cap) {
        if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_place<DE_RAW>, gp, dim3(256), 0, s, k, d);
        else if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_de_place<DE_ZLIB>, gp, dim3(256), 0, s, k, d);
        else hipLaunchKernelGGL(k_de_place<DE_GZIP>, gp, dim3(256), 0, s, k, d);
    }
    if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_dh_head<DE_ZLIB>, gh, dim3(256), 0, s, k, (uint32_t)level);
    if (fmt == DE_GZIP) hipLaunchKernelGGL(k_dh_head<DE_GZIP>, gh, dim3(256), 0, s, k, (uint32_t)level);
    return RCX_RC_OK;
}
