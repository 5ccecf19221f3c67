// k_bzip2.hip -- batched DECODE of .bz2 files (rcx_bzip2_decode_batch).  Block i of the batch is one whole file.
//
//   k_bz2_scan     every bit position of every file against the two 48-bit marks, every byte position against BZh1..9: a counting launch,
//                  the host's prefix sum over the 4 KiB chunks, an emitting launch -- the candidates of a file lie in increasing position
//                  whatever the scheduling
//   k_bz2_entropy  one wave per block mark, speculatively: header, selectors, coding tables, then Huffman + MTF + RUNA/RUNB into the
//                  candidate's slot of scratch (100 000 bytes x the highest level a header of the call names).  Safe on arbitrary bits: a mark can occur inside compressed data
//   (host)         rcx_plan_bz2_chain strings the candidates into streams and drops the ones off the chain
//   (tu_bwt)       rcx_tu_bwt_inverse(minimal) on the live blocks: for bzip2's rotation-sorted L and origPtr the n-step LF walk IS the inverse
//   k_bz2_count    which bytes of a block's text are run counts (a wave scan of 5-state functions), the expanded length
//   k_bz2_crc      the block CRC over the expanded bytes WITHOUT expanding them: 64 slices a block, merged with k_crc32.hip's x^n mod P
//                  machinery on bit-mirrored bytes
//   k_bz2_unrle    the expansion into the file's slot, for the blocks that passed their CRC and fit
//
// The launch loop (launch_bzip2_decode) is in this file and runs unmodified on the wave simulator.  It is synchronous: it reads the
// chunk counts, the candidates, the blocks' records and their lengths and CRCs back between the stages.
#pragma once
#include <string>
#include <vector>
#include "rcx_dev.h"
#include "rcx_plan.h"
#include "k_crc32.hip"

// the inverse BWT lives in tu_bwt.hip (k_bwt_inverse.hip): called, not copied
int rcx_tu_bwt_inverse(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool minimal);
uint64_t rcx_tu_bwt_inverse_scratch(uint32_t nblocks, uint64_t max_block);

#define BZ2_ROUND 1536u                  /* block candidates a round unless the caller says otherwise: the waves the LDS lets live at once (six a CU); bounds the scratch */
#define BZ2_ROUND_MIN 64u
#define BZ2_ROUND_MAX 4096u
#define BZ2_MAX_FILES 65535u             /* the file index rides on a grid dimension */
#define BZ2_BWT_BYTES (2ull << 30)       /* the inverse BWT's scratch at the most: about 110 blocks of 900 000 bytes a launch, smaller blocks more */
#define BZ2_CHUNK 4096u                  /* bytes per counter of the scan */
#define BZ2_SCAN_GRID 2048u
#define BZ2_RUN_WAVE 256u                /* a run at least this long is stored by the whole wave */
#define BZ2_MARK_BLOCK 0x314159265359ull
#define BZ2_MARK_END 0x177245385090ull

// ---- stage 1: the scan -------------------------------------------------------------------------------------------------------------------
// four bytes at q of a file of n bytes as a big-endian word, zeros behind the file's end
__device__ __forceinline__ uint32_t bz2_be32(const uint8_t* d, uint64_t n, uint64_t q)
{
    if (q + 4 <= n) return __builtin_bswap32(*(const rcx_u32_u*)(d + q));
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; j++) v = (v << 8) | (q + j < n ? (uint32_t)d[q + j] : 0u);
    return v;
}
// Workgroup (x, y): file y, the chunks x, x + gridDim.x, ... of it, one wave a chunk.  A lane takes 4 bytes a step: the 32 bit positions
// in them against both marks (64-bit funnel shifts over the 16 bytes from its own), its 4 byte positions against the header.
// EMIT false: cnt[chunk_base[y] + chunk] = the chunk's candidates.  EMIT true: the candidates go to cand[off[...] ...] in position order
// (a step without a candidate, nearly every one, is passed by one ballot).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_bz2_scan(const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, const uint64_t* chunk_base,
                                                  uint32_t* cnt, const uint64_t* off, rcx_bz2_cand* cand)
{
    const uint32_t f = blockIdx.y, lane = rcx_lane(), wave = threadIdx.x >> 6;
    const uint8_t* d = in_base + in_off[f];
    const uint64_t n = in_len[f], nbits = n * 8;
    const uint64_t nchunks = (n + BZ2_CHUNK - 1) / BZ2_CHUNK;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wave; ch < nchunks; ch += (uint64_t)gridDim.x * 4) {
        uint64_t at = EMIT ? off[chunk_base[f] + ch] : 0;
        uint32_t total = 0;
        for (uint32_t step = 0; step < BZ2_CHUNK / 256; step++) {
            const uint64_t base = ch * BZ2_CHUNK + step * 256u;
            if (base >= n) break;                                           // (wave-uniform)
            const uint64_t p = base + lane * 4u;
            const uint32_t w0 = bz2_be32(d, n, p);
            const uint32_t e0 = bz2_be32(d, n, base + 256), e1 = bz2_be32(d, n, base + 260), e2 = bz2_be32(d, n, base + 264);
            const uint32_t s1 = (uint32_t)__shfl_down((int)w0, 1), s2 = (uint32_t)__shfl_down((int)w0, 2), s3 = (uint32_t)__shfl_down((int)w0, 3);
            const uint32_t w1 = lane < 63 ? s1 : e0;
            const uint32_t w2 = lane < 62 ? s2 : (lane == 62 ? e0 : e1);
            const uint32_t w3 = lane < 61 ? s3 : (lane == 61 ? e0 : lane == 62 ? e1 : e2);
            const uint64_t hi = ((uint64_t)w0 << 32) | w1, lo = ((uint64_t)w2 << 32) | w3;
            uint32_t mb = 0, me = 0, mh = 0;
#pragma unroll
            for (uint32_t o = 0; o < 32; o++) {
                const uint64_t t = o ? (hi << o) | (lo >> (64 - o)) : hi;    // the 64 bits from bit o of the lane's window
                const bool inside = p * 8 + o + 48 <= nbits;                 // the whole mark lies in the file
                mb |= (inside && (t >> 16) == BZ2_MARK_BLOCK) ? 1u << o : 0u;
                me |= (inside && (t >> 16) == BZ2_MARK_END) ? 1u << o : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t v = (uint32_t)(((hi << (8 * j)) | (j ? lo >> (64 - 8 * j) : 0)) >> 32);
                const uint32_t lv = v & 0xffu;
                mh |= (p + j + 4 <= n && (v >> 8) == 0x425a68u && lv >= '1' && lv <= '9') ? 1u << j : 0u;
            }
            const uint32_t mine = (uint32_t)(__popc(mb) + __popc(me) + __popc(mh));
            if (__ballot(mine != 0) == 0) continue;                         // (wave-uniform)
            const uint32_t incl = rcx_wave_incl_scan(mine);
            if (EMIT && mine) {
                uint64_t w = at + total + incl - mine;
                for (uint32_t o = 0; o < 32; o++) {
                    const uint64_t bit = p * 8 + o;
                    if ((o & 7u) == 0 && ((mh >> (o >> 3)) & 1u)) {
                        const uint32_t j = o >> 3;
                        const uint32_t v = (uint32_t)(((hi << (8 * j)) | (j ? lo >> (64 - 8 * j) : 0)) >> 32);
                        cand[w++] = rcx_bz2_cand{bit, RCX_BZ2_HEAD, (v & 0xffu) - '0'};
                    }
                    if ((mb >> o) & 1u) cand[w++] = rcx_bz2_cand{bit, RCX_BZ2_BLOCK, 0u};
                    if ((me >> o) & 1u) {
                        const uint64_t t = o ? (hi << o) | (lo >> (64 - o)) : hi;
                        const uint32_t tail = (uint32_t)(((lo << o) >> 48) & 0xffffu);      // bits o + 64 .. o + 79 of the window
                        cand[w++] = rcx_bz2_cand{bit, RCX_BZ2_END, (uint32_t)((t & 0xffffu) << 16) | tail};
                    }
                }
            }
            total += (uint32_t)__shfl((int)incl, 63);
        }
        if (!EMIT && lane == 0) cnt[chunk_base[f] + ch] = total;
    }
}

// ---- stage 2: the entropy decoder ------------------------------------------------------------------------------------------------------
struct bz2_item { uint64_t bit; uint32_t file, pad; };      // a block candidate of the round: where its mark starts

// MSB-first bit reader over a file, one lane's.  Reads never leave the file: bytes behind its end read as zero and set `past`; whoever
// consumed one of them finds position() > nbits.
struct Bz2Bits {
    const uint8_t* d; uint64_t n;            // the file
    uint64_t next;                           // the next byte to load
    uint64_t acc; uint32_t have;             // the low `have` bits of acc are unread
    bool past;
    __device__ __forceinline__ void start(const uint8_t* data, uint64_t len, uint64_t bit)
    {
        d = data; n = len; next = bit >> 3; acc = 0; have = 0; past = false;
        if (bit & 7u) { acc = next < n ? d[next] : 0u; if (next >= n) past = true; next++; have = 8 - (uint32_t)(bit & 7u); }
    }
    __device__ __forceinline__ uint32_t get(uint32_t k)                      // k = 0 .. 24
    {
        if (have < k) {
            uint32_t w;
            if (next + 4 <= n) w = __builtin_bswap32(*(const rcx_u32_u*)(d + next));
            else { w = 0; for (uint32_t j = 0; j < 4; j++) w = (w << 8) | (next + j < n ? (uint32_t)d[next + j] : 0u); past = true; }
            acc = (acc << 32) | w; have += 32; next += 4;
        }
        have -= k;
        return (uint32_t)(acc >> have) & ((1u << k) - 1u);
    }
    __device__ __forceinline__ uint64_t position() const { return next * 8 - have; }
    __device__ __forceinline__ bool overran() const { return past && position() > n * 8; }
};

// One wave per block candidate (a workgroup of one wave: its 24 KiB of LDS -- 18 002 selectors among them -- let six live on a CU, and a
// round has at most 512).  Lane 0 parses the header, lanes 0..5 build one decoding table each exactly as libbz2 does (so that accept
// and reject agree on incomplete and over-subscribed tables), lane 0 runs the symbol loop -- serial by nature -- and the wave stores the
// long runs.  Every read is bounded by the file (Bz2Bits), every write by the slot (nblock <= cap, what the slot holds, is tested in
// front of each), and every loop by a count the header fixes: a symbol costs a bit at least and there are at most 50 a selector.
__global__ __launch_bounds__(64) void k_bz2_entropy(const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, const bz2_item* items,
                                                    rcx_bz2_rec* recs, uint8_t* slots, uint32_t slot_bytes, uint32_t cap, uint32_t count)
{
    __shared__ uint8_t s_sel[RCX_BZ2_MAX_SELECTORS + 6];
    __shared__ uint8_t s_len[6][260];
    __shared__ uint16_t s_perm[6][260];
    __shared__ int32_t s_limit[6][24], s_base[6][24];
    __shared__ uint32_t s_minlen[6];
    __shared__ uint8_t s_mtf[256];
    __shared__ uint32_t s_hdr[4];            // status, nGroups, alphaSize, nSelectors
    __shared__ uint32_t s_run[4];            // a long run for the wave: byte, count, start; [3] = the block is over
    const uint32_t c = blockIdx.x, lane = rcx_lane();
    if (c >= count) return;
    const bz2_item it = items[c];
    const uint8_t* d = in_base + in_off[it.file];
    const uint64_t n = in_len[it.file];
    uint8_t* L = slots + (size_t)c * slot_bytes;
    Bz2Bits br;
    br.start(d, n, it.bit + 48);
    uint32_t status = RCX_OK, crc = 0, orig = 0, nblock = 0, ngroups = 0, alpha = 0, nsel = 0;
    // ---- the header, lane 0
    if (lane == 0) {
        crc = br.get(16) << 16; crc |= br.get(16);
        const uint32_t randomised = br.get(1);
        orig = br.get(24);
        const uint32_t top = br.get(16);
        uint32_t used = 0;
        for (uint32_t i = 0; i < 16; i++) {
            if (!((top >> (15 - i)) & 1u)) continue;
            const uint32_t m = br.get(16);
            for (uint32_t j = 0; j < 16; j++) if ((m >> (15 - j)) & 1u) s_mtf[used++] = (uint8_t)(i * 16 + j);
        }
        alpha = used + 2;
        ngroups = br.get(3);
        nsel = br.get(15);
        if (randomised) status = RCX_E_BZ2_RANDOMISED;
        else if (used == 0 || ngroups < 2 || ngroups > 6 || nsel < 1 || nsel > RCX_BZ2_MAX_SELECTORS) status = RCX_E_BZ2_DATA;
        if (!status) {
            uint8_t order[6] = {0, 1, 2, 3, 4, 5};
            for (uint32_t i = 0; i < nsel && !status; i++) {
                uint32_t j = 0;
                while (br.get(1)) { if (++j >= ngroups) { status = RCX_E_BZ2_DATA; break; } }
                if (status) break;
                const uint8_t v = order[j];
                for (; j > 0; j--) order[j] = order[j - 1];
                order[0] = v;
                s_sel[i] = v;
                if (br.overran()) status = RCX_E_EOF;
            }
        }
        for (uint32_t t = 0; t < ngroups && !status; t++) {
            int32_t curr = (int32_t)br.get(5);
            for (uint32_t i = 0; i < alpha && !status; i++) {
                // (every turn reads a bit: at most as many turns as the file has bits)
                for (;;) {
                    if (curr < 1 || curr > 20) { status = RCX_E_BZ2_DATA; break; }
                    if (!br.get(1)) break;
                    curr += br.get(1) ? -1 : 1;
                    if (br.overran()) { status = RCX_E_EOF; break; }
                }
                s_len[t][i] = (uint8_t)curr;
            }
        }
        if (!status && br.overran()) status = RCX_E_EOF;
        s_hdr[0] = status; s_hdr[1] = ngroups; s_hdr[2] = alpha; s_hdr[3] = nsel;
        s_run[3] = 0;
    }
    rcx_wave_sync();
    status = s_hdr[0]; ngroups = s_hdr[1]; alpha = s_hdr[2]; nsel = s_hdr[3];
    // ---- the decoding tables, lane t builds table t (libbz2's BZ2_hbCreateDecodeTables)
    if (!status && lane < ngroups) {
        const uint32_t t = lane;
        uint32_t minl = 32, maxl = 0;
        for (uint32_t i = 0; i < alpha; i++) { const uint32_t l = s_len[t][i]; minl = l < minl ? l : minl; maxl = l > maxl ? l : maxl; }
        uint32_t pp = 0;
        for (uint32_t l = minl; l <= maxl; l++)
            for (uint32_t i = 0; i < alpha; i++) if (s_len[t][i] == l) s_perm[t][pp++] = (uint16_t)i;
        for (; pp < 260; pp++) s_perm[t][pp] = 0;
        for (uint32_t l = 0; l < 24; l++) { s_base[t][l] = 0; s_limit[t][l] = 0; }
        for (uint32_t i = 0; i < alpha; i++) s_base[t][s_len[t][i] + 1]++;
        for (uint32_t l = 1; l < 24; l++) s_base[t][l] += s_base[t][l - 1];
        int32_t vec = 0;
        for (uint32_t l = minl; l <= maxl; l++) { vec += s_base[t][l + 1] - s_base[t][l]; s_limit[t][l] = vec - 1; vec <<= 1; }
        for (uint32_t l = minl + 1; l <= maxl; l++) s_base[t][l] = ((s_limit[t][l - 1] + 1) << 1) - s_base[t][l];
        s_minlen[t] = minl;
    }
    rcx_wave_sync();
    // ---- the symbols: lane 0 decodes until the block ends, fails or has a long run for the wave.  Each turn of this loop decodes a
    // symbol at least, and there are at most 50 * nsel of them
    const uint32_t eob = alpha - 1;
    uint32_t group_no = 0xffffffffu, group_pos = 0, g = 0;
    uint32_t sym = 0xffffu;                                                 // the symbol in hand (0xffff: none yet)
    auto next_sym = [&]() -> uint32_t {                                      // libbz2's GET_MTF_VAL; 0xffff with `status` set
        if (group_pos == 0) {
            group_no++;
            if (group_no >= nsel) { status = RCX_E_BZ2_DATA; return 0xffffu; }
            group_pos = 50; g = s_sel[group_no];
        }
        group_pos--;
        uint32_t zn = s_minlen[g];
        int32_t zvec = (int32_t)br.get(zn);
        for (;;) {
            if (zn > 20) { status = RCX_E_BZ2_DATA; return 0xffffu; }
            if (zvec <= s_limit[g][zn]) break;
            zn++;
            zvec = (zvec << 1) | (int32_t)br.get(1);
        }
        const int32_t idx = zvec - s_base[g][zn];
        if (idx < 0 || idx >= 258) { status = RCX_E_BZ2_DATA; return 0xffffu; }
        if (br.overran()) { status = RCX_E_EOF; return 0xffffu; }
        return s_perm[g][idx];
    };
    const uint32_t max_turns = 50u * RCX_BZ2_MAX_SELECTORS + 2u;
    for (uint32_t turn = 0; turn < max_turns; turn++) {
        if (lane == 0) {
            s_run[1] = 0;
            bool over = status != RCX_OK;
            if (!over && sym == 0xffffu) { sym = next_sym(); over = status != RCX_OK; }
            while (!over) {
                if (sym == eob) { over = true; break; }
                if (sym <= 1) {                                             // RUNA / RUNB: a count in bijective base 2
                    int32_t es = -1, N = 1;
                    do {
                        if (N >= 2 * 1024 * 1024) { status = RCX_E_BZ2_DATA; break; }
                        es += sym == 0 ? N : 2 * N;
                        N *= 2;
                        sym = next_sym();
                    } while (!status && sym <= 1);
                    if (status) { over = true; break; }
                    es++;
                    if ((uint32_t)es > cap - nblock) { status = RCX_E_BZ2_DATA; over = true; break; }
                    const uint8_t uc = s_mtf[0];
                    if ((uint32_t)es >= BZ2_RUN_WAVE) { s_run[0] = uc; s_run[1] = (uint32_t)es; s_run[2] = nblock; nblock += (uint32_t)es; break; }
                    for (int32_t i = 0; i < es; i++) L[nblock++] = uc;
                    continue;
                }
                if (nblock >= cap) { status = RCX_E_BZ2_DATA; over = true; break; }
                const uint32_t j = sym - 1;                                 // (< alpha - 2 = the used bytes: perm holds symbols below alpha)
                const uint8_t uc = s_mtf[j];
                for (uint32_t q = j; q > 0; q--) s_mtf[q] = s_mtf[q - 1];
                s_mtf[0] = uc;
                L[nblock++] = uc;
                sym = next_sym();
                if (status) { over = true; break; }
            }
            s_run[3] = over ? 1u : 0u;
        }
        rcx_wave_sync();
        const uint32_t rb = s_run[0], rn = s_run[1], r0 = s_run[2], over = s_run[3];
        for (uint32_t i = lane; i < rn; i += 64) L[r0 + i] = (uint8_t)rb;   // (r0 + rn <= cap: tested by lane 0)
        rcx_wave_sync();
        if (over) break;
    }
    if (lane == 0) {
        if (status && br.overran()) status = RCX_E_EOF;                     // (what was read behind the file's end were zeros: the failure is the end)
        if (!status && sym != eob) status = RCX_E_BZ2_DATA;                 // (the turn bound: cannot happen)
        if (!status && orig >= nblock) status = RCX_E_BZ2_DATA;             // (an empty block too)
        rcx_bz2_rec r;
        r.status = (int32_t)status; r.nblock = nblock; r.orig = orig; r.crc = crc; r.end_bit = br.position();
        recs[c] = r;
    }
}

// ---- stage 5: the run-length step undone ---------------------------------------------------------------------------------------------------
// The step's decoder is a machine of five states -- the equal bytes seen in a row, 0 after a count, 4: the next byte is a count -- and a
// byte moves it by one of two functions, depending only on whether it equals the byte before it.  A function is five 3-bit entries;
// composing them is associative, so a tile of 64 bytes is a wave scan and the tiles of a block follow each other by one carried state.
#define BZ2_F_ID 0x4688u        /* 0 1 2 3 4 */
#define BZ2_F_EQ 0x08d1u        /* 1 2 3 4 0 */
#define BZ2_F_NE 0x0249u        /* 1 1 1 1 0 */
__device__ __forceinline__ uint32_t bz2_f_apply(uint32_t f, uint32_t x) { return (f >> (3 * x)) & 7u; }
__device__ __forceinline__ uint32_t bz2_f_then(uint32_t first, uint32_t second)      // x -> second(first(x))
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) r |= bz2_f_apply(second, bz2_f_apply(first, x)) << (3 * x);
    return r;
}
// One wave per live block.  mask[t_off / 64 + tile] = which of the tile's 64 bytes are counts; xlen[j] = the expanded length (at most
// 900 000 / 5 * 259 bytes), or ~0: the block ends after four equal bytes, where a count is due.
__global__ __launch_bounds__(64) void k_bz2_count(const uint8_t* t_base, const uint64_t* t_off, const uint64_t* t_len, uint64_t* mask,
                                                  uint32_t* xlen, uint32_t count)
{
    const uint32_t j = blockIdx.x, lane = rcx_lane();
    if (j >= count) return;
    const uint8_t* T = t_base + t_off[j];
    const uint32_t n = (uint32_t)t_len[j];
    uint64_t* m = mask + t_off[j] / 64;
    uint32_t state = 0, prev = 0x100u, acc = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t b = i < n ? T[i] : 0x200u;
        const uint32_t up = (uint32_t)__shfl_up((int)b, 1);
        const uint32_t pb = lane ? up : prev;
        uint32_t f = i < n ? (b == pb ? BZ2_F_EQ : BZ2_F_NE) : BZ2_F_ID;
#pragma unroll
        for (uint32_t dlt = 1; dlt < 64; dlt <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)f, dlt);
            if (lane >= dlt) f = bz2_f_then(o, f);
        }
        const uint32_t ex = (uint32_t)__shfl_up((int)f, 1);
        const uint32_t before = bz2_f_apply(lane ? ex : BZ2_F_ID, state);
        const bool is_count = i < n && before == 4;
        const unsigned long long cm = __ballot(is_count);
        if (lane == 0) m[i0 / 64] = cm;
        acc += i < n ? (is_count ? b : 1u) : 0u;
        state = bz2_f_apply((uint32_t)__shfl((int)f, 63), state);
        prev = (uint32_t)__shfl((int)b, 63);
    }
    acc = rcx_wave_sum(acc);
    // a text that ends where a count is due: libbz2 reads the count behind the block's end and calls the block corrupt
    if (lane == 0) xlen[j] = state == 4 ? 0xffffffffu : acc;
}

// One wave per live block: the bzip2 CRC (polynomial 0x04C11DB7, MSB first, all-ones in and out) of the EXPANDED bytes, read off the
// text and the count masks.  It is the bit-mirrored twin of CRC-32: crc_bz2(d) = bitrev32(crc32(bitrev8 of every byte)), so every lane
// runs k_crc32's table recurrence over mirrored bytes of its share of tiles, a count byte k being k more steps of the byte before
// it, and the 64 slices -- of unequal expanded lengths -- are merged by crc(A || B) = crc(A) * x^(8|B|) mod P xor crc(B).
__global__ __launch_bounds__(64) void k_bz2_crc(const uint8_t* t_base, const uint64_t* t_off, const uint64_t* t_len, const uint64_t* mask,
                                                uint32_t* crc_out, uint32_t count)
{
    __shared__ uint32_t s_tab[256];
    for (unsigned i = threadIdx.x; i < 256; i += 64) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? RCX_CRC_POLY : 0u);
        s_tab[i] = c;
    }
    __syncthreads();
    const uint32_t j = blockIdx.x, lane = rcx_lane();
    if (j >= count) return;
    const uint8_t* T = t_base + t_off[j];
    const uint32_t n = (uint32_t)t_len[j];
    const uint64_t* m = mask + t_off[j] / 64;
    const uint32_t ntiles = (n + 63) / 64, per = (ntiles + 63) / 64;
    const uint32_t t0 = lane * per < ntiles ? lane * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    uint32_t c = 0xffffffffu;
    uint64_t len = 0;
    for (uint32_t t = t0; t < t1; t++) {
        const uint64_t cm = m[t];
        const uint32_t e = (t + 1) * 64 < n ? (t + 1) * 64 : n;
        for (uint32_t i = t * 64; i < e; i++) {
            const uint32_t b = T[i];
            if ((cm >> (i & 63u)) & 1u) {
                const uint32_t x = __brev((uint32_t)T[i - 1]) >> 24;        // (a count is never a block's first byte)
                for (uint32_t k = 0; k < b; k++) c = s_tab[(c ^ x) & 0xffu] ^ (c >> 8);
                len += b;
            } else {
                c = s_tab[(c ^ (__brev(b) >> 24)) & 0xffu] ^ (c >> 8);
                len += 1;
            }
        }
    }
    c = ~c;
#pragma unroll 1
    for (int dd = 0; dd < 6; dd++) {
        const uint32_t right = (uint32_t)__shfl_down((int)c, 1 << dd);
        const uint32_t rlo = (uint32_t)__shfl_down((int)(uint32_t)len, 1 << dd), rhi = (uint32_t)__shfl_down((int)(uint32_t)(len >> 32), 1 << dd);
        const uint64_t rlen = ((uint64_t)rhi << 32) | rlo;
        if ((lane & ((2u << dd) - 1u)) == 0) {
            c = rcx_crc_mulmod(rcx_crc_xpow(8 * rlen), c) ^ right;
            len += rlen;
        }
    }
    if (lane == 0) crc_out[j] = __brev(c);
}

// One wave per live block: the expansion.  dst[j] = where the block's bytes start in out_base, or ~0: not this one.
__global__ __launch_bounds__(64) void k_bz2_unrle(const uint8_t* t_base, const uint64_t* t_off, const uint64_t* t_len, const uint64_t* mask,
                                                  uint8_t* out_base, const uint64_t* dst, uint32_t count)
{
    const uint32_t j = blockIdx.x, lane = rcx_lane();
    if (j >= count || dst[j] == ~0ull) return;
    const uint8_t* T = t_base + t_off[j];
    const uint32_t n = (uint32_t)t_len[j];
    const uint64_t* m = mask + t_off[j] / 64;
    uint8_t* o = out_base + dst[j];
    uint64_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool is_count = ((m[i0 / 64] >> lane) & 1ull) != 0;
        const uint32_t b = i < n ? T[i] : 0u;
        const uint32_t mine = i < n ? (is_count ? b : 1u) : 0u;
        const uint32_t incl = rcx_wave_incl_scan(mine);
        uint8_t* w = o + run + incl - mine;
        if (i < n) {
            if (is_count) { const uint8_t pb = T[i - 1]; for (uint32_t k = 0; k < b; k++) w[k] = pb; }
            else w[0] = (uint8_t)b;
        }
        run += (uint32_t)__shfl((int)incl, 63);
    }
}

// ---- the call -----------------------------------------------------------------------------------------------------------------------------------
// h_in_len / h_out_cap: the batch's lengths and capacities on the host (k's arrays are the device's).  Results go to k.out_len, k.in_used
// and k.status by a copy at the end.
// round: block candidates a round (0: BZ2_ROUND).  watch: somebody who wants to see the scan's candidates, the accepted blocks and the
// rounds as they happen (rcx_plan.h), or null.
static int launch_bzip2_decode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_len, const uint64_t* h_out_off, const uint64_t* h_out_cap,
                               const rcx_bz2_alloc& alloc, uint32_t round, std::string& err, const rcx_bz2_watch* watch = nullptr)
{
    const uint32_t n = k.nblocks;
    if (!n) return RCX_RC_OK;
    if (!h_in_len || !h_out_off || !h_out_cap || !alloc.get) { err = "bzip2 decode: use rcx_bzip2_decode_batch"; return RCX_RC_BAD_ARG; }
    if (n > BZ2_MAX_FILES) { err = "bzip2 decode: at most 65535 files a call"; return RCX_RC_BAD_ARG; }
    if (round && (round < BZ2_ROUND_MIN || round > BZ2_ROUND_MAX)) { err = "bzip2 decode: candidates a round must be 0 (default) or 64..4096"; return RCX_RC_BAD_ARG; }
#define BZ2_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return RCX_RC_HIP_ERROR; } } while (0)
// behind every launch whose results the host reads back and acts on: a refused launch must not leave it reading scratch nobody wrote
#define BZ2_LAUNCHED() BZ2_HIP(hipGetLastError())
    auto up = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    // ---- the scan: count, prefix (here), emit
    std::vector<uint64_t> chunk_base(n + 1, 0);
    uint64_t max_chunks = 1;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t c = (h_in_len[i] + BZ2_CHUNK - 1) / BZ2_CHUNK;
        chunk_base[i + 1] = chunk_base[i] + c;
        max_chunks = std::max(max_chunks, c);
    }
    const uint64_t nchunks = chunk_base[n];
    const dim3 sgrid((uint32_t)std::min<uint64_t>((max_chunks + 3) / 4, BZ2_SCAN_GRID), n);
    std::vector<uint32_t> h_cnt(nchunks);
    std::vector<uint64_t> h_off(nchunks + 1, 0);
    {
        uint8_t* base = (uint8_t*)alloc.get(alloc.self, 0, up((n + 1) * 8ull) + up(nchunks * 4) + 512);
        if (!base) { err = "bzip2 decode: no scratch"; return RCX_RC_NO_MEMORY; }
        base = (uint8_t*)(((uintptr_t)base + 255u) & ~(uintptr_t)255u);
        uint64_t* d_cb = (uint64_t*)base;
        uint32_t* d_cnt = (uint32_t*)(base + up((n + 1) * 8ull));
        BZ2_HIP(hipMemcpyAsync(d_cb, chunk_base.data(), (n + 1) * 8ull, hipMemcpyHostToDevice, s));
        if (nchunks) {
            hipLaunchKernelGGL((k_bz2_scan<false>), sgrid, dim3(256), 0, s, k.in_base, k.in_off, k.in_len, d_cb, d_cnt, (const uint64_t*)nullptr, (rcx_bz2_cand*)nullptr);
            BZ2_LAUNCHED();
            BZ2_HIP(hipMemcpyAsync(h_cnt.data(), d_cnt, nchunks * 4, hipMemcpyDeviceToHost, s));
        }
        BZ2_HIP(hipStreamSynchronize(s));
    }
    for (uint64_t i = 0; i < nchunks; i++) h_off[i + 1] = h_off[i] + h_cnt[i];
    const uint64_t ncand = h_off[nchunks];
    if (ncand > 0x7fffffffull) { err = "bzip2 decode: too many marks"; return RCX_RC_BAD_ARG; }
    // ---- the emitting launch, in a buffer of its own: the candidates are the host's from here on
    std::vector<rcx_bz2_cand> cands(ncand);
    if (ncand) {
        const uint64_t o_off = up((n + 1) * 8ull), o_cand = o_off + up((nchunks + 1) * 8);
        uint8_t* eb = (uint8_t*)alloc.get(alloc.self, 0, o_cand + up(ncand * sizeof(rcx_bz2_cand)) + 512);
        if (!eb) { err = "bzip2 decode: no scratch"; return RCX_RC_NO_MEMORY; }
        eb = (uint8_t*)(((uintptr_t)eb + 255u) & ~(uintptr_t)255u);
        BZ2_HIP(hipMemcpyAsync(eb, chunk_base.data(), (n + 1) * 8ull, hipMemcpyHostToDevice, s));
        BZ2_HIP(hipMemcpyAsync(eb + o_off, h_off.data(), (nchunks + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL((k_bz2_scan<true>), sgrid, dim3(256), 0, s, k.in_base, k.in_off, k.in_len, (const uint64_t*)eb, (uint32_t*)nullptr,
                           (const uint64_t*)(eb + o_off), (rcx_bz2_cand*)(eb + o_cand));
        BZ2_LAUNCHED();
        BZ2_HIP(hipMemcpyAsync(cands.data(), eb + o_cand, ncand * sizeof(rcx_bz2_cand), hipMemcpyDeviceToHost, s));
        BZ2_HIP(hipStreamSynchronize(s));
    }
    // ---- the scratch of the rounds.  A slot holds what the highest level any header of the call names allows: a block beyond that is
    // one every walk refuses (a header that merely occurred inside data only makes the slots larger)
    uint32_t nblk = 0, level = 1;
    for (const rcx_bz2_cand& c : cands) { if (c.kind == RCX_BZ2_BLOCK) nblk++; if (c.kind == RCX_BZ2_HEAD && c.extra > level) level = c.extra; }
    const uint32_t cap = 100000u * level, slot_bytes = (uint32_t)up(cap);
    const uint32_t R = std::min(std::max(nblk, 1u), round ? round : BZ2_ROUND);
    struct { uint64_t items, recs, L, T, mask, desc, xlen, crc, dst, end; } lay;
    lay.items = 0;
    lay.recs = lay.items + up((uint64_t)R * sizeof(bz2_item));
    lay.L = lay.recs + up((uint64_t)R * sizeof(rcx_bz2_rec));
    lay.T = lay.L + (uint64_t)R * slot_bytes;
    lay.mask = lay.T + (uint64_t)R * slot_bytes;
    lay.desc = lay.mask + up((uint64_t)R * slot_bytes / 8 + 8);
    lay.xlen = lay.desc + up((uint64_t)R * 56);                             // in_off in_len out_off out_cap out_len in_used | status aux
    lay.crc = lay.xlen + up((uint64_t)R * 4);
    lay.dst = lay.crc + up((uint64_t)R * 4);
    lay.end = lay.dst + up((uint64_t)R * 8);
    uint8_t* base = (uint8_t*)alloc.get(alloc.self, 0, lay.end + 512);
    if (!base) { err = "bzip2 decode: no scratch"; return RCX_RC_NO_MEMORY; }
    base = (uint8_t*)(((uintptr_t)base + 255u) & ~(uintptr_t)255u);
    // ---- per file: its candidates, its walk, its output so far
    struct file_state { uint64_t c0; uint32_t nc; uint32_t avail; rcx_bz2_chain chain; uint64_t out_pos; int32_t fail; };
    std::vector<file_state> fs(n);
    std::vector<rcx_bz2_rec> recs(ncand);
    for (uint32_t i = 0; i < n; i++) {
        fs[i].c0 = h_off[chunk_base[i]]; fs[i].nc = (uint32_t)(h_off[chunk_base[i + 1]] - fs[i].c0);
        fs[i].avail = 0; fs[i].out_pos = 0; fs[i].fail = RCX_OK;
        if (watch) for (uint32_t q = 0; q < fs[i].nc; q++) watch->candidate(watch->self, i, &cands[fs[i].c0 + q]);
    }
    std::vector<bz2_item> items(R);
    std::vector<uint64_t> item_cand(R);
    std::vector<uint32_t> live;
    std::vector<rcx_bz2_rec> round_recs(R);
    struct live_block { uint32_t file, slot, nblock, orig, crc; };
    std::vector<live_block> lb;
    std::vector<uint64_t> d64; std::vector<uint32_t> d32, h_xlen(R), h_crc(R);
    std::vector<uint64_t> h_dst(R);
    uint32_t f = 0, ci = 0;                                                 // the next candidate to look at: file f's ci-th
    for (;;) {
        // a round: the next block candidates no walk has passed yet, R at the most
        uint32_t cnt = 0;
        const uint32_t f_first = f;
        while (f < n) {
            file_state& F = fs[f];
            if (ci >= F.nc || F.chain.done) { F.avail = F.nc; f++; ci = 0; continue; }
            const rcx_bz2_cand& c = cands[F.c0 + ci];
            if (c.kind == RCX_BZ2_BLOCK && c.bit >= F.chain.expect) {
                if (cnt == R) break;                                        // the next round's first
                items[cnt] = bz2_item{c.bit, f, 0}; item_cand[cnt] = F.c0 + ci; cnt++;
            }
            ci++;
            F.avail = ci;
        }
        if (cnt) {
            BZ2_HIP(hipMemcpyAsync(base + lay.items, items.data(), cnt * sizeof(bz2_item), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_bz2_entropy, dim3(cnt), dim3(64), 0, s, k.in_base, k.in_off, k.in_len, (const bz2_item*)(base + lay.items),
                               (rcx_bz2_rec*)(base + lay.recs), base + lay.L, slot_bytes, cap, cnt);
            BZ2_LAUNCHED();
            BZ2_HIP(hipMemcpyAsync(round_recs.data(), base + lay.recs, cnt * sizeof(rcx_bz2_rec), hipMemcpyDeviceToHost, s));
            BZ2_HIP(hipStreamSynchronize(s));
            for (uint32_t q = 0; q < cnt; q++) recs[item_cand[q]] = round_recs[q];
        }
        // the walks of the files this round touched, as far as the records reach
        lb.clear();
        const uint32_t f_last = f < n ? f : n - 1;
        for (uint32_t i = f_first; i <= f_last; i++) {
            file_state& F = fs[i];
            if (F.chain.done) continue;
            live.clear();
            rcx_plan_bz2_chain(h_in_len[i], cands.data() + F.c0, F.nc, recs.data() + F.c0, F.avail, F.chain, live);
            for (uint32_t li : live) {
                uint32_t slot = 0;
                while (slot < cnt && item_cand[slot] != F.c0 + li) slot++;  // (a live block was decoded in this round: the walk stops at `avail`)
                if (slot >= cnt) { err = "bzip2 decode: a live block outside its round"; return RCX_RC_BAD_ARG; }
                const rcx_bz2_rec& r = recs[F.c0 + li];
                lb.push_back(live_block{i, slot, r.nblock, r.orig, r.crc});
                if (watch) watch->live(watch->self, i, cands[F.c0 + li].bit);
            }
        }
        const uint32_t nl = (uint32_t)lb.size();
        if (nl) {
            // the inverse BWT: kargs that point into the scratch, in as many launches as its budget takes
            d64.assign((size_t)6 * nl, 0); d32.assign((size_t)2 * nl, 0);
            uint64_t tpos = 0;
            for (uint32_t j = 0; j < nl; j++) {
                d64[j] = (uint64_t)lb[j].slot * slot_bytes; d64[nl + j] = lb[j].nblock;
                d64[2 * nl + j] = tpos; d64[3 * nl + j] = lb[j].nblock;
                d32[nl + j] = lb[j].orig;
                tpos += up(lb[j].nblock);
            }
            uint64_t* dd = (uint64_t*)(base + lay.desc);
            uint32_t* dw = (uint32_t*)(dd + (size_t)6 * nl);
            BZ2_HIP(hipMemcpyAsync(dd, d64.data(), (size_t)6 * nl * 8, hipMemcpyHostToDevice, s));
            BZ2_HIP(hipMemcpyAsync(dw, d32.data(), (size_t)2 * nl * 4, hipMemcpyHostToDevice, s));
            // (its scratch is a buffer of its own, sized by what the blocks of this round turned out to be: BZ2_BWT_BYTES at the most,
            //  and one block of any size always goes)
            std::vector<uint32_t> cuts(1, 0);
            uint64_t bwt_bytes = 0;
            for (uint32_t j0 = 0; j0 < nl;) {
                uint32_t j1 = j0; uint64_t maxn = 0, need = 0;
                while (j1 < nl) {
                    const uint64_t m = std::max<uint64_t>(maxn, lb[j1].nblock), b = rcx_tu_bwt_inverse_scratch(j1 - j0 + 1, m);
                    if (j1 > j0 && b > BZ2_BWT_BYTES) break;
                    maxn = m; need = b; j1++;
                }
                bwt_bytes = std::max(bwt_bytes, need);
                cuts.push_back(j1);
                j0 = j1;
            }
            uint8_t* bwt = (uint8_t*)alloc.get(alloc.self, 1, bwt_bytes + 512);
            if (!bwt) { err = "bzip2 decode: no scratch for the inverse BWT"; return RCX_RC_NO_MEMORY; }
            bwt = (uint8_t*)(((uintptr_t)bwt + 255u) & ~(uintptr_t)255u);
            for (size_t q = 0; q + 1 < cuts.size(); q++) {
                const uint32_t j0 = cuts[q], j1 = cuts[q + 1];
                rcx_kargs kb;
                memset(&kb, 0, sizeof kb);
                kb.in_base = base + lay.L; kb.in_off = dd + j0; kb.in_len = dd + nl + j0;
                kb.out_base = base + lay.T; kb.out_off = dd + 2 * nl + j0; kb.out_cap = dd + 3 * nl + j0;
                kb.out_len = dd + 4 * nl + j0; kb.in_used = dd + 5 * nl + j0; kb.status = (int32_t*)dw + j0; kb.aux = dw + nl + j0;
                kb.scratch = bwt; kb.scratch_bytes = bwt_bytes; kb.nblocks = j1 - j0;
                const int rc = rcx_tu_bwt_inverse(s, kb, 0, err, true);
                if (rc) return rc;
                BZ2_LAUNCHED();
            }
            const uint64_t* t_off = dd + 2 * nl; const uint64_t* t_len = dd + nl;
            hipLaunchKernelGGL(k_bz2_count, dim3(nl), dim3(64), 0, s, base + lay.T, t_off, t_len, (uint64_t*)(base + lay.mask), (uint32_t*)(base + lay.xlen), nl);
            hipLaunchKernelGGL(k_bz2_crc, dim3(nl), dim3(64), 0, s, base + lay.T, t_off, t_len, (const uint64_t*)(base + lay.mask), (uint32_t*)(base + lay.crc), nl);
            BZ2_LAUNCHED();
            BZ2_HIP(hipMemcpyAsync(h_xlen.data(), base + lay.xlen, nl * 4ull, hipMemcpyDeviceToHost, s));
            BZ2_HIP(hipMemcpyAsync(h_crc.data(), base + lay.crc, nl * 4ull, hipMemcpyDeviceToHost, s));
            BZ2_HIP(hipStreamSynchronize(s));
            // offsets by a running sum per file; the cap is checked here: a block is expanded when it and everything before it is good and fits
            bool any = false;
            for (uint32_t j = 0; j < nl; j++) {
                file_state& F = fs[lb[j].file];
                h_dst[j] = ~0ull;
                if (F.fail) continue;
                // (a file that has failed is over: its walk is marked done, so no later round decodes another block of it)
                if (h_xlen[j] == 0xffffffffu) { F.fail = RCX_E_BZ2_DATA; F.chain.done = true; continue; }
                if (h_crc[j] != lb[j].crc) { F.fail = RCX_E_BZ2_BLOCK_CRC; F.chain.done = true; continue; }
                if (F.out_pos + h_xlen[j] <= h_out_cap[lb[j].file]) { h_dst[j] = h_out_off[lb[j].file] + F.out_pos; any = true; }
                F.out_pos += h_xlen[j];
            }
            if (any) {
                BZ2_HIP(hipMemcpyAsync(base + lay.dst, h_dst.data(), nl * 8ull, hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(k_bz2_unrle, dim3(nl), dim3(64), 0, s, base + lay.T, t_off, t_len, (const uint64_t*)(base + lay.mask), k.out_base,
                                   (const uint64_t*)(base + lay.dst), nl);
                BZ2_LAUNCHED();
                BZ2_HIP(hipStreamSynchronize(s));                           // (h_dst and the T area are the next round's)
            }
        }
        if (watch) watch->round(watch->self);
        if (f >= n) break;
    }
    // ---- the files' results
    std::vector<uint64_t> r_len(n), r_used(n);
    std::vector<int32_t> r_st(n);
    for (uint32_t i = 0; i < n; i++) {
        file_state& F = fs[i];
        if (!F.chain.done) {                                                // (every candidate has been offered: cannot happen)
            live.clear();
            rcx_plan_bz2_chain(h_in_len[i], cands.data() + F.c0, F.nc, recs.data() + F.c0, F.nc, F.chain, live);
        }
        const int32_t st = F.fail ? F.fail : F.chain.status;
        if (st) { r_st[i] = st; r_len[i] = 0; r_used[i] = 0; }
        else if (F.out_pos > h_out_cap[i]) { r_st[i] = RCX_E_OUTPUT_TOO_SMALL; r_len[i] = F.out_pos; r_used[i] = 0; }
        else { r_st[i] = RCX_OK; r_len[i] = F.out_pos; r_used[i] = F.chain.in_used; }
    }
    BZ2_HIP(hipMemcpyAsync(k.out_len, r_len.data(), n * 8ull, hipMemcpyHostToDevice, s));
    if (k.in_used) BZ2_HIP(hipMemcpyAsync(k.in_used, r_used.data(), n * 8ull, hipMemcpyHostToDevice, s));
    BZ2_HIP(hipMemcpyAsync(k.status, r_st.data(), n * 4ull, hipMemcpyHostToDevice, s));
    BZ2_HIP(hipStreamSynchronize(s));
#undef BZ2_LAUNCHED
#undef BZ2_HIP
    return RCX_RC_OK;
}
