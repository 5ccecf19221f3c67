// k_zstd.hip -- Zstandard (RFC 8878) DECODE of whole .zst files: rcx_zstd_decode_batch (include/rcx.h).  Block b of the batch is one
// file: one or more concatenated frames, skippable frames skipped wherever they stand, a raw-content dictionary (a range anywhere in
// the input buffer, the words of rcx_plan_dict) as history in front of every frame.
// NOT a function of the reference crate, which has no Zstandard.  The checkers are tests/zstd_ref.py (a plain-Python decoder written
// from the format) and libzstd 1.4.8, whose accept / reject this follows where it differs from the RFC (DESIGN.md 3.22 lists where).
//
// ONE WAVE PER FILE, waves persistent over the files of a call (file = blockIdx.x, + gridDim.x, ...): frames and blocks are taken in
// order, because a block inherits the previous block's repeat offsets, Huffman table and FSE tables.  The wave's state lives in LDS
// (struct ZsLds, 12.0 KiB; the kernel's 129 VGPRs allow three waves a SIMD, twelve a CU); a block's literals (at most 128 KiB) go to the wave's buffer in scratch.
//   headers    wave-uniform: every lane reads the same bytes (uniform addresses, one request a load)
//   tables     the normalised counts are a serial variable-width read that every lane does alike.  The spread is one lane's loop of
//              stores (no load depends on them); the per-cell bit count and baseline come from a cell's rank among the cells of its
//              symbol, found 64 cells at a time with one ballot per distinct symbol of the group.  The predefined tables are built
//              once per wave.  Huffman weights: direct 4-bit or from the FSE pair of interleaved states (one lane); the ranks of
//              equal weights by ballots, the 2^tableLog cells filled by all lanes, symbol after symbol.
//   literals   raw (read in place from the input), RLE (one value), or Huffman with one or four backward bitstreams: a lane a stream, a
//              64-bit container refilled from the stream's end downward, tableLog-bit lookups in LDS, byte stores to scratch.
//   sequences  lane 0 decodes up to 64 sequences: three FSE states, extra bits in the order offset, match length, literal length, the
//              repeat offsets resolved (the shift when the literal length is 0, offset_value 3 as rep1 - 1), literals left and history
//              checked; it pushes (literal length, match length, offset) into the ring.
//   execution  the wave drains the ring FLATTENED: a prefix sum gives every sequence its place in the batch's output, and a lane takes an
//              output byte of the batch: it finds the byte's sequence (a binary search over the 64 ends in LDS); a literal is
//              copied; a match byte lies q = offset - (j mod offset) behind the match's start in the virtual stream dictionary ||
//              frame output || this sequence's literals (period handling keeps q >= 1), and where that is a byte of THIS batch the
//              lane hops to it and asks again -- every hop lands in an earlier sequence, 64 at the most -- until it stands on a
//              literal, on output from before the batch or in the dictionary.  No copy of a batch waits for another.
//              (The form built first took a sequence at a time, k_lz4_dict.hip's direct form with its `settled` rule inside the
//              batch; it is kept as an A/B variant and measured 11 to 21 % slower.)
//   ordering   `settled` is the output position up to which the wave has waited for its own stores (RCX_WAIT_VMEM between
//              rcx_wave_sync()s): once in front of a batch, whose loads from out[] all lie below the batch.  The literal buffer is
//              waited for once, behind the literal stage.
// A slot too small: parsing and counting go on, nothing at or beyond the capacity is stored or loaded, the content checksum (which
// needs the bytes) is left to the retry.  Every loop is bounded by the bits left in its stream, the declared counts or the slot.
// Nothing below the slot is dereferenced, nothing outside [out_off, out_off + out_cap) is written.
//
// What bounds it: the serial symbol work -- four lanes in the literal stage, one in the sequence stage.
#pragma once
#include "rcx_dev.h"
#include "k_xxh64.hip"

#define ZS_MAGIC 0xFD2FB528u
#define ZS_BLOCK_MAX 131072u
#define ZS_LIT_SLOT (ZS_BLOCK_MAX + 64u)     /* a wave's literal buffer in scratch */
#define ZS_MAX_WAVES 2048u
#define ZS_RING 64u
#define ZS_HUF_LOG 11u
#define ZS_ERR 0xffffffffu

// code -> baseline | extra bits << 24 (RFC 8878 3.1.1.3.2.1.1); an offset code c has the baseline 1 << c and c extra bits
__device__ static const uint32_t ZS_LL_CODE[36] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
    16 | 1u << 24, 18 | 1u << 24, 20 | 1u << 24, 22 | 1u << 24, 24 | 2u << 24, 28 | 2u << 24, 32 | 3u << 24, 40 | 3u << 24,
    48 | 4u << 24, 64 | 6u << 24, 128 | 7u << 24, 256 | 8u << 24, 512 | 9u << 24, 1024 | 10u << 24, 2048 | 11u << 24, 4096 | 12u << 24,
    8192 | 13u << 24, 16384 | 14u << 24, 32768 | 15u << 24, 65536 | 16u << 24};
__device__ static const uint32_t ZS_ML_CODE[53] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
    35 | 1u << 24, 37 | 1u << 24, 39 | 1u << 24, 41 | 1u << 24, 43 | 2u << 24, 47 | 2u << 24, 51 | 3u << 24, 59 | 3u << 24,
    67 | 4u << 24, 83 | 4u << 24, 99 | 5u << 24, 131 | 7u << 24, 259 | 8u << 24, 515 | 9u << 24, 1027 | 10u << 24, 2051 | 11u << 24,
    4099 | 12u << 24, 8195 | 13u << 24, 16387 | 14u << 24, 32771 | 15u << 24, 65539 | 16u << 24};
// the predefined distributions (RFC 8878 3.1.1.3.2.2), accuracy logs 6, 6, 5
__device__ static const int8_t ZS_LL_DEF[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__device__ static const int8_t ZS_ML_DEF[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__device__ static const int8_t ZS_OF_DEF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

// An FSE cell: symbol | bits to read << 8 | baseline of the next state << 16
struct ZsLds {
    uint16_t huf[1u << ZS_HUF_LOG];          // symbol | code length << 8, indexed by the next tableLog bits
    uint32_t ll[512], ml[512], of[256];      // this file's own tables (FSE-described or RLE)
    uint32_t pre_ll[64], pre_ml[64], pre_of[32];
    uint32_t wt[64];                         // the FSE table of the Huffman weights
    uint32_t ll_code[36], ml_code[53];
    union {                                  // a block builds its tables before its first sequence: the ring lies over the builds' temporaries
        struct {
            uint32_t ring_ll[ZS_RING], ring_ml[ZS_RING], ring_of[ZS_RING];
            uint32_t ring_end[ZS_RING], ring_lit[ZS_RING];   // the flattened executor: a sequence's end in the batch's output, its first literal
        };
        struct {
            int16_t norm[256];               // table builds: the normalised counts,
            uint16_t next[256];              // ... a symbol's next state (FSE) / first cell (Huffman),
            uint8_t spread[512];             // ... the symbol of every cell,
            uint8_t w[256];                  // ... the Huffman weights
        };
    };
};

// A backward bitstream (RFC 8878 4.1): read from the last byte's highest set bit downward.  One lane's.
struct ZsBits {
    const uint8_t* s; uint32_t ptr; uint64_t c; uint32_t nb; bool over;    // c: the next bits at its top, nb of them valid; s[0 .. ptr) not loaded yet
    __device__ __forceinline__ bool init(const uint8_t* start, uint32_t len)
    {
        s = start; ptr = 0; c = 0; nb = 0; over = false;
        if (!len) return false;
        const uint32_t lb = start[len - 1];
        if (!lb) return false;                                             // no end mark
        nb = 31u - (uint32_t)__clz(lb);
        c = nb ? (uint64_t)lb << (64u - nb) : 0;                           // (the mark itself leaves at the top)
        ptr = len - 1;
        return true;
    }
    __device__ __forceinline__ void refill()
    {
        if (nb <= 32u && ptr >= 4u) { ptr -= 4; c |= (uint64_t)(*(const rcx_u32_u*)(s + ptr)) << (32u - nb); nb += 32; }
        while (nb <= 56u && ptr) { ptr--; c |= (uint64_t)s[ptr] << (56u - nb); nb += 8; }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) { if (nb < n) refill(); return (uint32_t)(c >> (64u - n)); }        // 1 <= n <= 32; zeros behind the stream's first bit
    __device__ __forceinline__ void skip(uint32_t n) { if (n > nb) { over = true; c = 0; nb = 0; } else { c <<= n; nb -= n; } }   // after peek(>= n)
    __device__ __forceinline__ uint32_t read(uint32_t n) { if (!n) return 0; const uint32_t v = peek(n); skip(n); return v; }
    __device__ __forceinline__ bool done() const { return !over && nb == 0 && ptr == 0; }
};

struct Zstd {
    ZsLds* L;
    const uint8_t* in; uint32_t n;           // the file
    uint8_t* out; uint64_t cap;              // its slot
    const uint8_t* dict; uint64_t D;
    uint8_t* litbuf;
    uint32_t lane;
    // frame state
    uint64_t opos, fstart, settled;          // decoded bytes of the file so far; where the frame began; stores waited for
    bool have_huf, have_fse;
    const uint32_t* t_ll; const uint32_t* t_ml; const uint32_t* t_of;
    uint32_t log_ll, log_ml, log_of;
    uint32_t rep0, rep1, rep2;               // (lane 0's copies count)
    uint32_t huf_log;
    bool flat;                               // the flattened executor, what ships: a lane per output byte of a batch (false: a sequence at a time, an A/B variant)
    bool lit_only;                           // a profiling build's launch (RCX_AB_VARIANTS): a compressed block ends behind its literals
    // the block's literals
    const uint8_t* lit; uint32_t lit_n; bool lit_rle; uint32_t lit_val;

    __device__ __forceinline__ uint32_t rd8(uint32_t p) const { return in[p]; }
    __device__ __forceinline__ uint32_t rd16(uint32_t p) const { return in[p] | (uint32_t)in[p + 1] << 8; }
    __device__ __forceinline__ uint32_t rd24(uint32_t p) const { return rd16(p) | (uint32_t)in[p + 2] << 16; }
    __device__ __forceinline__ uint32_t rd32(uint32_t p) const { return rd16(p) | rd16(p + 2) << 16; }
    __device__ __forceinline__ uint32_t bcast(uint32_t v) const { return (uint32_t)__shfl((int)v, 0); }

    // ---- FSE table description (FSE_readNCount): counts into L->norm.  Every lane alike.  -> bytes consumed, 0: corrupt
    __device__ uint32_t read_ncount(uint32_t p, uint32_t len, uint32_t max_sym, uint32_t max_log, uint32_t& log, uint32_t& nsym)
    {
        // bits [at, at + k) of the description, k <= 16, zeros behind its end
        auto bits = [&](uint32_t at, uint32_t k) -> uint32_t {
            const uint32_t b = at >> 3;
            uint32_t v = 0;
            for (uint32_t i = 0; i < 3; i++) if (b + i < len) v |= rd8(p + b + i) << (8 * i);
            return (v >> (at & 7u)) & ((1u << k) - 1u);
        };
        uint32_t at = 4;
        log = bits(0, 4) + 5;
        if (log > 15u || log > max_log) return 0;
        int remaining = (1 << log) + 1, threshold = 1 << log;
        uint32_t nbits = log + 1, sym = 0;
        bool prev0 = false;
        while (remaining > 1 && sym <= max_sym) {
            if (prev0) {
                uint32_t n0 = sym;
                while (bits(at, 16) == 0xffffu) { n0 += 24; at += 16; }
                while (bits(at, 2) == 3u) { n0 += 3; at += 2; }
                n0 += bits(at, 2); at += 2;
                if (n0 > max_sym) return 0;
                if (lane == 0) for (uint32_t i = sym; i < n0; i++) L->norm[i] = 0;
                sym = n0;
            }
            const int max = (2 * threshold - 1) - remaining;
            const uint32_t v = bits(at, nbits);
            int count;
            if ((int)(v & (uint32_t)(threshold - 1)) < max) { count = (int)(v & (uint32_t)(threshold - 1)); at += nbits - 1; }
            else { count = (int)(v & (uint32_t)(2 * threshold - 1)); if (count >= threshold) count -= max; at += nbits; }
            count--;
            remaining -= count < 0 ? -count : count;
            if (lane == 0) L->norm[sym] = (int16_t)count;
            sym++;
            prev0 = !count;
            while (remaining < threshold) { nbits--; threshold >>= 1; }
        }
        if (remaining != 1 || at > 8 * len) return 0;
        nsym = sym;
        rcx_wave_sync();
        return (at + 7) >> 3;
    }

    // ---- the decoding table of L->norm[0 .. nsym) at accuracy `log` into tab[0 .. 1 << log)
    __device__ void build_fse(uint32_t* tab, uint32_t nsym, uint32_t log)
    {
        const uint32_t size = 1u << log;
        if (lane == 0) {
            uint32_t high = size - 1;
            for (uint32_t s = 0; s < nsym; s++) {
                const int c = L->norm[s];
                if (c == -1) { L->spread[high--] = (uint8_t)s; L->next[s] = 1; } else L->next[s] = (uint16_t)c;
            }
            const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
            uint32_t pos = 0;
            for (uint32_t s = 0; s < nsym; s++) {
                const int c = L->norm[s];
                for (int i = 0; i < c; i++) {
                    L->spread[pos] = (uint8_t)s;
                    do pos = (pos + step) & mask; while (pos > high);
                }
            }
        }
        rcx_wave_sync();
        for (uint32_t u0 = 0; u0 < size; u0 += 64) {
            const uint32_t u = u0 + lane;
            const bool valid = u < size;
            const uint32_t s = valid ? L->spread[u] : 0x100u + lane;
            const uint32_t base = valid ? L->next[s] : 0;
            rcx_wave_sync();
            uint64_t todo = __ballot(valid);
            uint32_t r = 0;
            while (todo) {                                                 // one turn per distinct symbol of the 64 cells
                const int l0 = __ffsll((unsigned long long)todo) - 1;
                const uint32_t s0 = (uint32_t)__shfl((int)s, l0);
                const uint64_t m = __ballot(valid && s == s0);
                if (valid && s == s0) {
                    r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if ((int)lane == l0) L->next[s] = (uint16_t)(base + (uint32_t)__popcll(m));
                }
                todo &= ~m;
            }
            if (valid) {
                const uint32_t ns = base + r;                              // >= 1: every cell's symbol has a count
                const uint32_t nb = log - (31u - (uint32_t)__clz(ns | 1u));
                tab[u] = s | nb << 8 | (((ns << nb) - size) & 0xffffu) << 16;
            }
            rcx_wave_sync();
        }
    }
    __device__ void build_default(uint32_t* tab, const int8_t* def, uint32_t nsym, uint32_t log)
    {
        if (lane < nsym) L->norm[lane] = def[lane];
        rcx_wave_sync();
        build_fse(tab, nsym, log);
    }

    // ---- the Huffman table from the description at in[p .. p + len).  -> bytes consumed, 0: corrupt
    __device__ uint32_t build_huf(uint32_t p, uint32_t len)
    {
        if (!len) return 0;
        const uint32_t hb = rd8(p);
        uint32_t nw, used;
        if (hb >= 128u) {                                                  // direct: 4 bits a weight, the high nibble first
            nw = hb - 127u;
            used = 1 + (nw + 1) / 2;
            if (used > len) return 0;
            for (uint32_t i = lane; i < nw; i += 64) { const uint32_t b = rd8(p + 1 + i / 2); L->w[i] = (uint8_t)((i & 1u) ? b & 15u : b >> 4); }
        } else {                                                           // FSE: two interleaved states over one backward bitstream
            used = 1 + hb;
            if (used > len || hb < 2u) return 0;
            uint32_t log, nsym;
            const uint32_t hdr = read_ncount(p + 1, hb, 255, 6, log, nsym);
            if (!hdr || hdr >= hb) return 0;
            build_fse(L->wt, nsym, log);
            uint32_t cnt = ZS_ERR;
            if (lane == 0) {
                ZsBits b;
                if (b.init(in + p + 1 + hdr, hb - hdr)) {
                    uint32_t s1 = b.read(log), s2 = b.read(log);
                    cnt = 0;
                    if (b.over) cnt = ZS_ERR;
                    while (cnt != ZS_ERR) {                                // (ends when a state's update runs off the stream, or at 255 weights)
                        if (cnt > 253u) { cnt = ZS_ERR; break; }
                        const uint32_t e1 = L->wt[s1];
                        L->w[cnt++] = (uint8_t)e1;
                        s1 = (e1 >> 16) + b.read((e1 >> 8) & 255u);
                        if (b.over) { L->w[cnt++] = (uint8_t)L->wt[s2]; break; }
                        if (cnt > 253u) { cnt = ZS_ERR; break; }
                        const uint32_t e2 = L->wt[s2];
                        L->w[cnt++] = (uint8_t)e2;
                        s2 = (e2 >> 16) + b.read((e2 >> 8) & 255u);
                        if (b.over) { L->w[cnt++] = (uint8_t)L->wt[s1]; break; }
                    }
                }
            }
            nw = bcast(cnt);
            if (nw == ZS_ERR) return 0;
        }
        rcx_wave_sync();
        // the last weight completes a power of two; weights of 12 and more, a total beyond 2^11 and an odd count of weight 1 are refused
        uint32_t tot = 0;
        bool bad = false;
        for (uint32_t i = lane; i < nw; i += 64) { const uint32_t w = L->w[i]; bad |= w > ZS_HUF_LOG; tot += (1u << w) >> 1; }
        if (__any(bad)) return 0;
        tot = rcx_wave_sum(tot);
        if (!tot) return 0;
        const uint32_t log = 32u - (uint32_t)__clz(tot);
        if (log > ZS_HUF_LOG) return 0;
        const uint32_t rest = (1u << log) - tot;
        if (rest & (rest - 1u)) return 0;
        if (lane == 0) L->w[nw] = (uint8_t)(32u - (uint32_t)__clz(rest));
        rcx_wave_sync();
        const uint32_t nsym = nw + 1;
        uint32_t start = 0;                                                // the first cell of weight w: the longest codes lie lowest
        for (uint32_t w = 1; w <= log; w++) {
            uint32_t running = 0;
            for (uint32_t i0 = 0; i0 < nsym; i0 += 64) {
                const uint32_t i = i0 + lane;
                const bool mine = i < nsym && L->w[i] == w;
                const uint64_t m = __ballot(mine);
                if (mine) L->next[i] = (uint16_t)(start + ((running + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) << (w - 1)));
                running += (uint32_t)__popcll(m);
            }
            if (w == 1 && (running < 2u || (running & 1u))) return 0;
            start += running << (w - 1);
        }
        rcx_wave_sync();
        for (uint32_t i = 0; i < nsym; i++) {
            const uint32_t w = L->w[i];
            if (!w) continue;
            const uint32_t len1 = 1u << (w - 1), st = L->next[i], e = i | (log + 1 - w) << 8;
            for (uint32_t u = lane; u < len1; u += 64) L->huf[st + u] = (uint16_t)e;
        }
        rcx_wave_sync();
        huf_log = log;
        return used;
    }

    // ---- the literals section of the block at in[p .. p + len).  -> bytes consumed, 0: corrupt
    __device__ uint32_t literals(uint32_t p, uint32_t len)
    {
        const uint32_t b0 = rd8(p), type = b0 & 3u, sf = (b0 >> 2) & 3u;
        lit_rle = false; lit_val = 0;
        if (type < 2u) {
            uint32_t hs, size;
            if (!(sf & 1u)) { hs = 1; size = b0 >> 3; }
            else if (sf == 1u) { hs = 2; if (len < 2u) return 0; size = rd16(p) >> 4; }
            else { hs = 3; if (len < 3u) return 0; size = rd24(p) >> 4; }
            if (size > ZS_BLOCK_MAX) return 0;
            lit_n = size;
            if (type == 0) { if (hs + size > len) return 0; lit = in + p + hs; return hs + size; }
            if (hs + 1 > len) return 0;
            lit_rle = true; lit_val = rd8(p + hs); lit = in;
            return hs + 1;
        }
        if (len < 5u) return 0;
        uint32_t hs, size, csize, streams = 4;
        const uint32_t h = rd32(p);
        if (sf < 2u) { hs = 3; size = (h >> 4) & 0x3ffu; csize = (h >> 14) & 0x3ffu; if (!sf) streams = 1; }
        else if (sf == 2u) { hs = 4; size = (h >> 4) & 0x3fffu; csize = h >> 18; }
        else { hs = 5; size = (h >> 4) & 0x3ffffu; csize = (h >> 22) + (rd8(p + 4) << 10); }
        if (size > ZS_BLOCK_MAX || hs + csize > len || !size) return 0;
        uint32_t q = p + hs, left = csize;
        if (type == 2u) {
            const uint32_t used = build_huf(q, left);
            if (!used) return 0;
            have_huf = true;
            q += used; left -= used;
        } else if (!have_huf) return 0;
        // a lane a stream
        uint32_t s_off = 0, s_len = left, d_off = 0, d_len = size;
        bool bad = false;
        if (streams == 4u) {
            if (left < 10u) return 0;
            const uint32_t l1 = rd16(q), l2 = rd16(q + 2), l3 = rd16(q + 4), seg = (size + 3) / 4;
            if (6u + l1 + l2 + l3 > left || 3u * seg > size) return 0;
            const uint32_t l4 = left - 6u - l1 - l2 - l3;
            s_off = 6u + (lane > 0 ? l1 : 0) + (lane > 1 ? l2 : 0) + (lane > 2 ? l3 : 0);
            s_len = lane == 0 ? l1 : lane == 1 ? l2 : lane == 2 ? l3 : l4;
            d_off = lane * seg; d_len = lane < 3u ? seg : size - 3u * seg;
        }
        rcx_wave_sync();                                                   // (the lanes that still copy the last block's literals out of the buffer come first)
        if (lane < streams) {
            ZsBits b;
            if (!b.init(in + q + s_off, s_len)) bad = true;
            else {
                const uint32_t log = huf_log;
                uint8_t* dst = litbuf + d_off;
                for (uint32_t i = 0; i < d_len && !b.over; i++) {
                    const uint32_t e = L->huf[b.peek(log)];
                    b.skip(e >> 8);
                    dst[i] = (uint8_t)e;
                }
                bad = !b.done();
            }
        }
        if (__any(bad)) return 0;
        rcx_wave_sync();
        RCX_WAIT_VMEM();
        rcx_wave_sync();
        lit = litbuf; lit_n = size;
        return hs + csize;
    }
    __device__ __forceinline__ uint8_t lit_at(uint32_t i) const { return lit_rle ? (uint8_t)lit_val : lit[i]; }

    // ---- one of the three sequence tables by its mode.  -> bytes consumed + 1, 0: corrupt
    __device__ uint32_t seq_table(uint32_t mode, uint32_t p, uint32_t len, uint32_t max_sym, uint32_t max_log, uint32_t* own,
                                  const uint32_t* pre, uint32_t pre_log, const uint32_t*& tab, uint32_t& log)
    {
        if (mode == 0) { tab = pre; log = pre_log; return 1; }
        if (mode == 1) {
            if (!len || rd8(p) > max_sym) return 0;
            rcx_wave_sync();
            if (lane == 0) own[0] = rd8(p);
            rcx_wave_sync();
            tab = own; log = 0;
            return 2;
        }
        if (mode == 3) return have_fse ? 1 : 0;
        uint32_t nsym, lg;
        const uint32_t used = read_ncount(p, len, max_sym, max_log, lg, nsym);
        if (!used) return 0;
        build_fse(own, nsym, lg);
        tab = own; log = lg;
        return used + 1;
    }


    // ---- a compressed block at in[p .. p + len): literals, sequences, execution.  -> RCX_OK or the status
    __device__ int block(uint32_t p, uint32_t len)
    {
        if (len < 3u || len >= ZS_BLOCK_MAX) return RCX_E_ZSTD_DATA;
        const uint32_t lused = literals(p, len);
        if (!lused) return RCX_E_ZSTD_DATA;
        if (lit_only) { opos += lit_n; return RCX_OK; }
        uint32_t q = p + lused, left = len - lused;
        if (!left) return RCX_E_ZSTD_DATA;
        uint32_t nseq = rd8(q); q++; left--;
        const bool none = nseq == 0;                                       // (libzstd: the one-byte 0 alone ends the section; 80 00 goes on to the modes)
        if (nseq >= 128u) {
            if (nseq == 255u) { if (left < 2u) return RCX_E_ZSTD_DATA; nseq = rd16(q) + 0x7f00u; q += 2; left -= 2; }
            else { if (left < 1u) return RCX_E_ZSTD_DATA; nseq = ((nseq - 128u) << 8) + rd8(q); q++; left--; }
        }
        uint32_t litpos = 0;
        if (none) { if (left) return RCX_E_ZSTD_DATA; }
        else {
            if (!left) return RCX_E_ZSTD_DATA;
            const uint32_t modes = rd8(q); q++; left--;
            uint32_t u = seq_table(modes >> 6, q, left, 35, 9, L->ll, L->pre_ll, 6, t_ll, log_ll);
            if (!u) return RCX_E_ZSTD_DATA;
            q += u - 1; left -= u - 1;
            u = seq_table((modes >> 4) & 3u, q, left, 31, 8, L->of, L->pre_of, 5, t_of, log_of);
            if (!u) return RCX_E_ZSTD_DATA;
            q += u - 1; left -= u - 1;
            u = seq_table((modes >> 2) & 3u, q, left, 52, 9, L->ml, L->pre_ml, 6, t_ml, log_ml);
            if (!u) return RCX_E_ZSTD_DATA;
            q += u - 1; left -= u - 1;
            if (nseq) have_fse = true;
            // lane 0's reader, states and counts live across the rounds of the ring
            ZsBits b;
            uint32_t s_ll = 0, s_of = 0, s_ml = 0, bad = 0, vlit = 0;
            uint64_t vpos = opos - fstart;                                 // the frame's bytes so far, for the history check
            b.init(in, 0);
            if (lane == 0 && nseq) {
                if (!b.init(in + q, left)) bad = 1;
                else { s_ll = b.read(log_ll); s_of = b.read(log_of); s_ml = b.read(log_ml); bad = b.over; }
            }
            if (bcast(bad)) return RCX_E_ZSTD_DATA;
            for (uint32_t done = 0; done < nseq;) {
                const uint32_t cnt = nseq - done < ZS_RING ? nseq - done : ZS_RING;
                if (lane == 0) {
                    for (uint32_t k = 0; k < cnt && !bad; k++) {
                        const uint32_t e_ll = t_ll[s_ll], e_ml = t_ml[s_ml], e_of = t_of[s_of];
                        const uint32_t c_ll = L->ll_code[e_ll & 255u], c_ml = L->ml_code[e_ml & 255u], oc = e_of & 255u;
                        const uint32_t ov = b.read(oc);                    // the extra bits: offset, match length, literal length
                        const uint32_t mlen = (c_ml & 0xffffffu) + b.read(c_ml >> 24);
                        const uint32_t llen = (c_ll & 0xffffffu) + b.read(c_ll >> 24);
                        uint32_t off;
                        if (oc > 1u) { off = (1u << oc) + ov - 3u; rep2 = rep1; rep1 = rep0; rep0 = off; }
                        else if (oc == 0) {                                // offset_value 1: the first repeat offset, the second behind no literals
                            if (llen) off = rep0;
                            else { off = rep1; rep1 = rep0; rep0 = off; }
                        } else {                                           // offset_value 2, 3: one further behind no literals, and 4 is rep1 - 1
                            const uint32_t idx = 1u + (llen ? 0u : 1u) + ov;
                            off = idx == 3u ? rep0 - 1u : idx == 1u ? rep1 : rep2;
                            if (!off) off = 1;                             // (libzstd reads a zero as 1)
                            if (idx != 1u) rep2 = rep1;
                            rep1 = rep0; rep0 = off;
                        }
                        if (llen > lit_n - vlit || (uint64_t)off > vpos + llen + D) { bad = 1; break; }
                        vlit += llen; vpos += (uint64_t)llen + mlen;
                        L->ring_ll[k] = llen; L->ring_ml[k] = mlen; L->ring_of[k] = off;
                        if (done + k + 1 < nseq) {                         // the last sequence updates no state
                            s_ll = (e_ll >> 16) + b.read((e_ll >> 8) & 255u);
                            s_ml = (e_ml >> 16) + b.read((e_ml >> 8) & 255u);
                            s_of = (e_of >> 16) + b.read((e_of >> 8) & 255u);
                        }
                        if (b.over) bad = 1;
                    }
                    if (done + cnt == nseq && !b.done()) bad = 1;          // bits left over, or read past the stream's first bit
                }
                rcx_wave_sync();
                if (bcast(bad)) return RCX_E_ZSTD_DATA;
                if (flat) {
                    // a lane per output byte: every byte is chased to a literal or to a byte that was there before the batch, so no
                    // copy of the batch waits for another
                    const uint32_t l_k = lane < cnt ? L->ring_ll[lane] : 0, m_k = lane < cnt ? L->ring_ml[lane] : 0;
                    const uint32_t e_k = rcx_wave_incl_scan(l_k + m_k), f_k = rcx_wave_incl_scan(l_k);
                    L->ring_end[lane] = e_k; L->ring_lit[lane] = f_k - l_k;
                    rcx_wave_sync();
                    if (opos > settled) { RCX_WAIT_VMEM(); rcx_wave_sync(); settled = opos; }
                    const uint32_t total = L->ring_end[cnt - 1], lits = L->ring_lit[cnt - 1] + L->ring_ll[cnt - 1];
                    const uint64_t have = opos - fstart, room = cap > opos ? cap - opos : 0;
                    const uint32_t lim = total < room ? total : (uint32_t)room;
                    #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                    for (uint32_t t = lane; t < lim; t += 64) {
                        uint32_t cur = t;
                        uint8_t x = 0;
                        for (uint32_t hop = 0; hop <= ZS_RING; hop++) {    // (a hop lands in an earlier sequence)
                            uint32_t k = 0;
                            for (uint32_t s = 32; s; s >>= 1) if (L->ring_end[k + s - 1] <= cur) k += s;
                            const uint32_t l = L->ring_ll[k], m = L->ring_ml[k], off = L->ring_of[k], st = L->ring_end[k] - l - m;
                            const uint32_t i = cur - st, lp = litpos + L->ring_lit[k];
                            if (i < l) { x = lit_at(lp + i); break; }
                            uint32_t j = i - l;
                            if (off < m) j %= off;
                            const uint32_t qd = off - j;
                            if (qd <= l) { x = lit_at(lp + l - qd); break; }
                            const uint32_t back = qd - l;
                            if (back <= st) { cur = st - back; continue; }
                            const uint64_t b2 = (uint64_t)(back - st);
                            x = b2 <= have ? out[opos - b2] : dict[D - (b2 - have)];
                            break;
                        }
                        out[opos + t] = x;
                    }
                    opos += total; litpos += lits;
                } else
                for (uint32_t k = 0; k < cnt; k++) {
                    const uint32_t l = L->ring_ll[k], m = L->ring_ml[k], off = L->ring_of[k];
                    // k_lz4_dict.hip's rule: a source in out[] above what the wave has waited for waits first
                    if (off > l && opos > settled) {
                        const uint32_t span = off < m ? off : m;
                        const uint32_t qmin = off - span + 1;
                        const uint32_t back = qmin > l ? qmin - l : 1u;
                        if ((uint64_t)back <= opos - fstart && opos - back >= settled) {
                            rcx_wave_sync();
                            RCX_WAIT_VMEM();
                            rcx_wave_sync();
                            settled = opos;
                        }
                    }
                    const uint64_t total = (uint64_t)l + m, have = opos - fstart;
                    const uint64_t room = cap > opos ? cap - opos : 0;
                    const uint64_t lim = total < room ? total : room;
                    #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                    for (uint64_t i = lane; i < lim; i += 64) {
                        uint8_t x;
                        if (i < l) x = lit_at(litpos + (uint32_t)i);
                        else {
                            uint32_t j = (uint32_t)(i - l);
                            if (off < m) j %= off;
                            const uint32_t qd = off - j;
                            if (qd <= l) x = lit_at(litpos + l - qd);
                            else if ((uint64_t)(qd - l) <= have) x = out[opos - (qd - l)];
                            else x = dict[D - ((uint64_t)(qd - l) - have)];
                        }
                        out[opos + i] = x;
                    }
                    opos += total; litpos += l;
                }
                rcx_wave_sync();
                done += cnt;
            }
        }
        // the literals behind the last sequence
        const uint32_t rest = lit_n - litpos;
        const uint64_t room = cap > opos ? cap - opos : 0;
        const uint32_t lim = rest < room ? rest : (uint32_t)room;
        for (uint32_t i = lane; i < lim; i += 64) out[opos + i] = lit_at(litpos + i);
        opos += rest;
        return RCX_OK;
    }

    // ---- the file: frames until what follows is no frame.  -> the status; *olen the decoded size, *used the byte behind the last frame
    __device__ int run(uint64_t* olen, uint64_t* used)
    {
        opos = 0; settled = 0; fstart = 0;
        huf_log = 0; lit_n = 0; lit = in; lit_rle = false; lit_val = 0;
        uint32_t pos = 0, frames = 0;
        for (;;) {
            if (n - pos < 4u) { if (frames) break; return RCX_E_EOF; }
            const uint32_t magic = rd32(pos);
            if ((magic & 0xfffffff0u) == 0x184D2A50u) {                    // a skippable frame
                if (n - pos < 8u) return RCX_E_EOF;
                const uint32_t sz = rd32(pos + 4);
                if (sz > n - pos - 8u) return RCX_E_EOF;
                pos += 8u + sz; frames++;
                continue;
            }
            if (magic != ZS_MAGIC) { if (frames) break; return RCX_E_ZSTD_MAGIC; }
            if (n - pos < 5u) return RCX_E_EOF;
            const uint32_t fhd = rd8(pos + 4), fcsf = fhd >> 6, single = (fhd >> 5) & 1u, didf = fhd & 3u;
            const uint32_t dids = didf == 3u ? 4u : didf, fcss = fcsf == 0 ? single : fcsf == 1u ? 2u : fcsf == 2u ? 4u : 8u;
            const uint32_t hsize = 5u + (single ? 0u : 1u) + dids + fcss;
            if (n - pos < hsize) return RCX_E_EOF;
            if (fhd & 8u) return RCX_E_ZSTD_HEADER;
            uint32_t q = pos + 5;
            if (!single) { if ((rd8(q) >> 3) + 10u > 31u) return RCX_E_ZSTD_HEADER; q++; }
            uint32_t did = 0;
            for (uint32_t i = 0; i < dids; i++) did |= rd8(q + i) << (8 * i);
            q += dids;
            if (did) return RCX_E_ZSTD_DICT;
            uint64_t fcs = 0;
            for (uint32_t i = 0; i < fcss; i++) fcs |= (uint64_t)rd8(q + i) << (8 * i);
            if (fcss == 2u) fcs += 256;
            pos += hsize;
            fstart = opos; have_huf = false; have_fse = false;
            rep0 = 1; rep1 = 4; rep2 = 8;
            for (;;) {
                if (n - pos < 3u) return RCX_E_EOF;
                const uint32_t bh = rd24(pos), type = (bh >> 1) & 3u, bsize = bh >> 3;
                pos += 3;
                if (type == 3u) return RCX_E_ZSTD_DATA;
                const uint32_t csz = type == 1u ? 1u : bsize;
                if (csz > n - pos) return RCX_E_EOF;
                if (type == 2u) {
                    const int st = block(pos, bsize);
                    if (st) return st;
                } else {                                                   // raw: the bytes; RLE: one byte, bsize times
                    const uint64_t room = cap > opos ? cap - opos : 0;
                    const uint32_t lim = bsize < room ? bsize : (uint32_t)room;
                    if (type == 0) for (uint32_t i = lane; i < lim; i += 64) out[opos + i] = in[pos + i];
                    else { const uint8_t v = in[pos]; for (uint32_t i = lane; i < lim; i += 64) out[opos + i] = v; }
                    opos += bsize;
                }
                pos += csz;
                if (bh & 1u) break;
            }
            if (fcss && opos - fstart != fcs && !lit_only) return RCX_E_ZSTD_DATA;
            if (fhd & 4u) {
                if (n - pos < 4u) return RCX_E_EOF;
                if (opos <= cap && !lit_only) {                                         // (the bytes are all there; a slot too small leaves the check to the retry)
                    rcx_wave_sync();
                    RCX_WAIT_VMEM();
                    rcx_wave_sync();
                    settled = opos;
                    const uint64_t h = rcx_xxh64_quad(out + fstart, lane < 4u ? opos - fstart : 0, 0, lane);
                    if (bcast((uint32_t)h) != rd32(pos)) return RCX_E_ZSTD_CHECKSUM;
                }
                pos += 4;
            }
            frames++;
        }
        *olen = opos; *used = pos;
        return opos > cap ? RCX_E_OUTPUT_TOO_SMALL : RCX_OK;
    }
};

// aux: the words of rcx_plan_dict (rcx_plan_zstd: lengths unclamped): aux[b] = D, aux[3n + b] / aux[4n + b] = the dictionary's offset
// LIT_ONLY: the profiling instantiation that stops every compressed block behind its literals (benchmarks/zstd_decode_rate.py takes the
// stages' shares from it and from a size query, which runs everything but the copies); its results are not a decode's
template <bool LIT_ONLY, bool FLAT>
__global__ __launch_bounds__(64) void k_zstd_decode(rcx_kargs a)
{
    __shared__ ZsLds lds;
    Zstd z;
    z.L = &lds; z.lane = rcx_lane(); z.lit_only = LIT_ONLY; z.flat = FLAT;
    for (uint32_t i = z.lane; i < 36u; i += 64) lds.ll_code[i] = ZS_LL_CODE[i];
    for (uint32_t i = z.lane; i < 53u; i += 64) lds.ml_code[i] = ZS_ML_CODE[i];
    rcx_wave_sync();
    z.build_default(lds.pre_ll, ZS_LL_DEF, 36, 6);
    z.build_default(lds.pre_ml, ZS_ML_DEF, 53, 6);
    z.build_default(lds.pre_of, ZS_OF_DEF, 29, 5);
    z.litbuf = (uint8_t*)a.scratch + (uint64_t)blockIdx.x * ZS_LIT_SLOT;
    const uint64_t n = a.nblocks;
    for (uint32_t f = blockIdx.x; f < a.nblocks; f += gridDim.x) {
        z.in = a.in_base + a.in_off[f];
        z.n = (uint32_t)a.in_len[f];
        z.out = a.out_base + a.out_off[f];
        z.cap = a.out_cap[f];
        z.D = a.aux[f];
        z.dict = a.in_base + ((uint64_t)a.aux[3 * n + f] | ((uint64_t)a.aux[4 * n + f] << 32));
        uint64_t olen = 0, used = 0;
        const int st = z.run(&olen, &used);
        rcx_wave_sync();
        if (z.lane == 0) {
            const bool ok = st == RCX_OK || st == RCX_E_OUTPUT_TOO_SMALL;
            a.status[f] = st;
            a.out_len[f] = ok ? olen : 0;
            if (a.in_used) a.in_used[f] = ok ? used : 0;
        }
    }
}

// waves of a launch: one per file up to ZS_MAX_WAVES, each with ZS_LIT_SLOT bytes of k.scratch (rcx_plan_zstd sizes it)
// variants of a library built with RCX_AB_VARIANTS alone: 1 the LIT_ONLY instantiation, 2 the executor that takes a sequence at a time
// (the form built first; the flattened one measured 11 to 21 % faster and ships: DESIGN.md 3.22)
static int launch_zstd_decode(hipStream_t s, rcx_kargs& k, uint32_t waves, int variant, std::string& err)
{
    if (!k.aux) { err = "zstd decode: use rcx_zstd_decode_batch"; return RCX_RC_BAD_ARG; }
    if (!waves || waves > ZS_MAX_WAVES || k.scratch_bytes < (uint64_t)waves * ZS_LIT_SLOT || !k.scratch) { err = "zstd decode: scratch too small"; return RCX_RC_BAD_ARG; }
#ifdef RCX_AB_VARIANTS
    if (variant == 1) { hipLaunchKernelGGL((k_zstd_decode<true, true>), dim3(waves), dim3(64), 0, s, k); return RCX_RC_OK; }
    if (variant == 2) { hipLaunchKernelGGL((k_zstd_decode<false, false>), dim3(waves), dim3(64), 0, s, k); return RCX_RC_OK; }
#endif
    if (variant) { err = "zstd decode: unknown variant"; return RCX_RC_BAD_ARG; }
    hipLaunchKernelGGL((k_zstd_decode<false, true>), dim3(waves), dim3(64), 0, s, k);
    return RCX_RC_OK;
}
