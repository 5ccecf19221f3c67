// k_bzip2_enc.hip -- batched ENCODE of whole .bz2 files (rcx_bzip2_encode_batch).  Block i of the batch is one FILE and
// becomes one stream; its input is cut into chunks (rcx_plan.h: how long), and every chunk is one bzip2 block.  The
// bytes are those of the specification in DESIGN.md 3.21 and of its serial reference (tests/bz2_enc_ref.py), not libbz2's.
//
//   k_bz2e_rle_len  the length of a chunk's run-length form: run starts from a neighbour compare, the place inside a run from a max-scan
//                   of the starts, what a byte contributes a closed form of (place in run) mod 255 -- every lane works
//   k_bz2e_rle      the same walk, storing: T twice (T || T) for the sort, the used-byte map, the block CRC over the chunk's input bytes
//                   (k_crc32.hip's recurrence on mirrored bytes, 256 slices merged by x^n mod P as k_bz2_crc merges its 64)
//   (tu_bwt)        rcx_tu_bwt_forward(sa_words) on the T || T blocks: a suffix of T || T that starts below n orders its rotation, a
//                   proper prefix sorts first, so equal rotations come by DESCENDING start
//   k_bz2e_pick     the suffix array's entries below n, compacted in order: L[j] = T[(sa - 1) mod n], origPtr where sa == 0
//   k_bz2e_mtf      MTF ranks, chunk-parallel: a chunk's starting list is the used bytes by their last occurrence before it (a last-place
//                   table per chunk, a running maximum per symbol, a rank sort), then a lane walks its chunk with its list in LDS
//   k_bz2e_syms     zero runs (they cross the chunks freely now: this pass is per position) to RUNA / RUNB digits, the other ranks to
//                   symbols, compacted; the end symbol, nMTF
//   k_bz2e_fit      one workgroup a block: histogram, libbz2's initial partition, four iterations of choose-and-refit over length tables
//                   in LDS, lengths by Moffat-Katajainen limited to 17 (de_code_lengths restated: DEFLATE's output does not depend on
//                   this file), the groups' bit costs and the block's length in bits
//   k_bz2e_pack     the block MSB-first from bit 0 of its slot of the store: one lane the header, the selectors and the tables, a thread
//                   per group of 50 its symbols at the offset a scan of the costs gives; shared words meet by atomicOr on zeroed words
//   k_bz2e_join     every output byte of a file's slot gathered from the one or two sources that cover it (the 32 header bits, the
//                   blocks' slots, the 80 trailer bits and the padding): no atomics on the caller's buffer, and a slot that is too small
//                   is not written at all
//
// The launch loop (launch_bzip2_encode) is in this file and runs unmodified on the wave simulator.  It is synchronous: it reads the
// chunks' lengths and the blocks' records back between the stages, and the blocks go in rounds so that the scratch of the sort and the
// stages -- some 70 bytes per input byte of a round -- does not grow with the file.  Only the packed blocks wait for their file to be
// complete, because its size is known only then and a slot that is too small must stay untouched: at most 2.2 bytes per input byte.
#pragma once
#include <string>
#include <vector>
#include "rcx_dev.h"
#include "rcx_plan.h"
#include "k_crc32.hip"

// the suffix sorter lives in tu_bwt.hip (k_bwt.hip, k_bwt_sort.hip): called, not copied
int rcx_tu_bwt_forward(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool sa_words);
uint64_t rcx_tu_bwt_forward_scratch(uint32_t nblocks, uint64_t max_block);

#define BZ2E_MAX_FILES 65535u            /* the file index rides on a grid dimension */
#define BZ2E_STAGE_BYTES (4ull << 30)    /* the stages' scratch of a round at the most (one block of any size always goes) */
#define BZ2E_MTF_CHUNKS 128u             /* MTF chunks a block at the most: a lane each, 256 bytes of LDS each */
#define BZ2E_MTF_MIN 32u                 /* bytes a chunk at the least */
#define BZ2E_LIMIT 17u                   /* the longest code, as libbz2 writes */
#define BZ2E_ALPHA 258u
#define BZ2E_MARK_BLOCK 0x314159265359ull
#define BZ2E_MARK_END 0x177245385090ull

struct bz2e_desc {                       // a block of the call
    uint64_t in_at;                      // its input bytes in in_base
    uint32_t len, n;                     // input bytes; the bytes of the run-length form
    uint64_t store;                      // its bits in the store (a byte offset, a multiple of 256)
};
// the scratch of a round: slot j of every area belongs to block b0 + j
struct bz2e_round {
    uint8_t* tt; uint8_t* sa; uint8_t* l; uint8_t* rk; uint8_t* sym; uint8_t* lp; uint8_t* sel; uint8_t* gcost; uint8_t* lens;
    uint64_t st_tt, st_sa, st_l, st_rk, st_sym, st_lp, st_sel, st_gcost, st_lens;      // bytes a slot
    uint32_t b0, count;
};

// ---- workgroup scans (256 threads): inclusive, sum or maximum; every thread calls, under uniform control flow -------------------------------
template <bool MAX>
__device__ __forceinline__ uint32_t bz2e_wg_scan(uint32_t v, uint32_t* s_w, uint32_t& total)
{
    const uint32_t lane = rcx_lane(), wave = threadIdx.x >> 6;
    uint32_t incl = v;
    if (MAX) {
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d && o > incl) incl = o;
        }
    } else incl = rcx_wave_incl_scan(v);
    __syncthreads();                                                        // (s_w may still be read from the scan before)
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t x = s_w[w];
        if (MAX) { if (w < wave && x > before) before = x; if (x > total) total = x; }
        else { if (w < wave) before += x; total += x; }
    }
    return MAX ? (before > incl ? before : incl) : before + incl;
}

// ---- stage 1: the run-length step ------------------------------------------------------------------------------------------------------
// Within a chunk maximal runs are taken 255 bytes at a time; a piece of 4..255 bytes becomes four bytes and a count.  With r = (place in
// run) mod 255 a byte is stored when r < 4, and the last byte of a piece (r == 254, or the next byte differs, or the chunk ends) with
// r >= 3 adds the count r - 3.  -> the length.  EMIT: T[0 .. n) and T[n .. 2n) are written and the used bytes marked (every store below n:
// n is what the counting launch returned for the same bytes).
template <bool EMIT>
__device__ uint32_t bz2e_rle_walk(const uint8_t* in, uint32_t len, uint8_t* T, uint32_t n, uint32_t* s_w, uint32_t* s_used)
{
    const uint32_t tid = threadIdx.x;
    uint32_t last_start = 0, out = 0;                                       // (starts are kept as index + 1: 0 is none)
    for (uint32_t base = 0; base < len; base += 256) {
        const uint32_t i = base + tid;
        const bool valid = i < len;
        const uint32_t b = valid ? in[i] : 0x100u;
        const uint32_t pb = (valid && i) ? in[i - 1] : 0x1ffu;
        const uint32_t nb = (valid && i + 1 < len) ? in[i + 1] : 0x2ffu;
        const bool start = valid && b != pb;
        uint32_t tot;
        uint32_t st = bz2e_wg_scan<true>(start ? i + 1 : 0u, s_w, tot);
        if (last_start > st) st = last_start;
        if (tot > last_start) last_start = tot;
        const uint32_t r = valid ? (i + 1 - st) % 255u : 0u;
        const bool last = valid && (r == 254u || nb != b);
        const bool count = last && r >= 3u;
        const uint32_t c = valid ? (r < 4u ? 1u : 0u) + (count ? 1u : 0u) : 0u;
        uint32_t o = bz2e_wg_scan<false>(c, s_w, tot) - c + out;
        out += tot;
        if (EMIT && valid) {
            if (r < 4u) {
                if (o < n) { T[o] = (uint8_t)b; T[n + o] = (uint8_t)b; }
                if (r == 0) atomicOr(&s_used[b >> 5], 1u << (b & 31u));
                o++;
            }
            if (count) {
                const uint32_t k = r - 3u;
                if (o < n) { T[o] = (uint8_t)k; T[n + o] = (uint8_t)k; }
                atomicOr(&s_used[k >> 5], 1u << (k & 31u));
            }
        }
    }
    return out;
}
// one workgroup per chunk of the list: lens[j] = the length of its run-length form
__global__ __launch_bounds__(256) void k_bz2e_rle_len(const uint8_t* in_base, const bz2e_desc* desc, uint32_t* lens, uint32_t count)
{
    __shared__ uint32_t s_w[4];
    const uint32_t j = blockIdx.x;
    if (j >= count) return;
    const uint32_t n = bz2e_rle_walk<false>(in_base + desc[j].in_at, desc[j].len, nullptr, 0, s_w, nullptr);
    if (threadIdx.x == 0) lens[j] = n;
}
// the bzip2 CRC (polynomial 0x04C11DB7, MSB first, all-ones in and out) of `len` bytes: crc_bz2(d) = bitrev32(crc32(bitrev8 of every
// byte)), 256 slices merged by crc(A || B) = crc(A) * x^(8|B|) mod P xor crc(B).  Thread 0 returns it.
__device__ uint32_t bz2e_crc(const uint8_t* in, uint32_t len, const uint32_t* s_tab, uint32_t* s_m)
{
    const uint32_t tid = threadIdx.x, lane = rcx_lane(), wave = tid >> 6;
    const uint32_t per = (len + 255u) / 256u;
    const uint32_t i0 = (uint64_t)tid * per < len ? tid * per : len, i1 = i0 + per < len ? i0 + per : len;
    uint32_t c = 0xffffffffu;
    for (uint32_t i = i0; i < i1; i++) c = s_tab[(c ^ (__brev((uint32_t)in[i]) >> 24)) & 0xffu] ^ (c >> 8);
    c = ~c;
    uint32_t sl = i1 - i0;
#pragma unroll 1
    for (int dd = 0; dd < 6; dd++) {
        const uint32_t right = (uint32_t)__shfl_down((int)c, 1 << dd);
        const uint32_t rlen = (uint32_t)__shfl_down((int)sl, 1 << dd);
        if ((lane & ((2u << dd) - 1u)) == 0) {
            c = rcx_crc_mulmod(rcx_crc_xpow(8ull * rlen), c) ^ right;
            sl += rlen;
        }
    }
    __syncthreads();
    if (lane == 0) { s_m[wave] = c; s_m[4 + wave] = sl; }
    __syncthreads();
    if (tid) return 0;
    c = s_m[0];
    for (uint32_t w = 1; w < 4; w++) c = rcx_crc_mulmod(rcx_crc_xpow(8ull * s_m[4 + w]), c) ^ s_m[w];
    return __brev(c);
}
// one workgroup per block of the round: T || T, the used-byte map and the CRC
__global__ __launch_bounds__(256) void k_bz2e_rle(const uint8_t* in_base, const bz2e_desc* desc, rcx_bz2e_hdr* hdr, bz2e_round R)
{
    __shared__ uint32_t s_w[4], s_used[8], s_m[8], s_tab[256];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= R.count) return;
    const bz2e_desc d = desc[R.b0 + j];
    if (tid < 8) s_used[tid] = 0;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? RCX_CRC_POLY : 0u);
        s_tab[tid] = c;
    }
    __syncthreads();
    const uint8_t* in = in_base + d.in_at;
    bz2e_rle_walk<true>(in, d.len, R.tt + (size_t)j * R.st_tt, d.n, s_w, s_used);
    const uint32_t crc = bz2e_crc(in, d.len, s_tab, s_m);
    __syncthreads();
    rcx_bz2e_hdr* h = hdr + R.b0 + j;
    if (tid < 8) h->used[tid] = s_used[tid];
    if (tid == 0) h->crc = crc;
}

// ---- stage 3: L and origPtr from the suffix array of T || T ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bz2e_pick(const bz2e_desc* desc, rcx_bz2e_hdr* hdr, bz2e_round R)
{
    __shared__ uint32_t s_w[4];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= R.count) return;
    const uint32_t n = desc[R.b0 + j].n;
    const uint8_t* T = R.tt + (size_t)j * R.st_tt;
    const uint32_t* sa = (const uint32_t*)(R.sa + (size_t)j * R.st_sa);
    uint8_t* L = R.l + (size_t)j * R.st_l;
    uint32_t run = 0;
    for (uint32_t base = 0; base < 2u * n; base += 256) {
        const uint32_t i = base + tid;
        const uint32_t v = i < 2u * n ? sa[i] : 0xffffffffu;
        const uint32_t keep = v < n ? 1u : 0u;
        uint32_t tot;
        const uint32_t o = bz2e_wg_scan<false>(keep, s_w, tot) - keep + run;
        run += tot;
        if (keep && o < n) {
            L[o] = T[v ? v - 1 : n - 1];
            if (v == 0) hdr[R.b0 + j].orig = o;
        }
    }
}

// ---- stage 4: MTF ranks, chunk-parallel -----------------------------------------------------------------------------------------------------
// L is cut into at most 128 chunks of at least 32 bytes, a lane each.  lp[s][t] first holds where byte s last occurs in chunk t (+ 1), then
// -- a running maximum over the chunks, one lane per byte value -- where it last occurs BEFORE chunk t.  A chunk's starting list is the
// used bytes by that place, the latest first, and the bytes not seen yet behind them in ascending order: the state the serial MTF has
// there.  rk[i] = the rank of L[i].
__global__ __launch_bounds__(BZ2E_MTF_CHUNKS) void k_bz2e_mtf(const bz2e_desc* desc, const rcx_bz2e_hdr* hdr, bz2e_round R)
{
    __shared__ uint8_t s_list[256 * BZ2E_MTF_CHUNKS];                       // [place][lane]: a lane's list lies across the banks
    __shared__ uint32_t s_used[8];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    if (j >= R.count) return;
    const uint32_t n = desc[R.b0 + j].n;
    const uint8_t* L = R.l + (size_t)j * R.st_l;
    uint8_t* rk = R.rk + (size_t)j * R.st_rk;
    uint32_t* lp = (uint32_t*)(R.lp + (size_t)j * R.st_lp);
    const uint32_t per = (n + BZ2E_MTF_CHUNKS - 1) / BZ2E_MTF_CHUNKS, ch = per > BZ2E_MTF_MIN ? per : BZ2E_MTF_MIN;
    const uint32_t nch = (n + ch - 1) / ch;                                 // (<= 128)
    const uint32_t i0 = (uint64_t)t * ch < n ? t * ch : n, i1 = i0 + ch < n ? i0 + ch : n;
    if (t < 8) s_used[t] = hdr[R.b0 + j].used[t];
    for (uint32_t s = 0; s < 256; s++) lp[s * BZ2E_MTF_CHUNKS + t] = 0;
    __syncthreads();
    for (uint32_t i = i0; i < i1; i++) lp[(uint32_t)L[i] * BZ2E_MTF_CHUNKS + t] = i + 1;
    __syncthreads();
    for (uint32_t s = t; s < 256; s += BZ2E_MTF_CHUNKS) {
        uint32_t carry = 0;
        for (uint32_t c = 0; c < nch; c++) {
            const uint32_t v = lp[s * BZ2E_MTF_CHUNKS + c];
            lp[s * BZ2E_MTF_CHUNKS + c] = carry;
            if (v > carry) carry = v;
        }
    }
    __syncthreads();
    if (t < nch) {
        auto used = [&](uint32_t s) { return (s_used[s >> 5] >> (s & 31u)) & 1u; };
        uint32_t nseen = 0;
        for (uint32_t s = 0; s < 256; s++) if (used(s) && lp[s * BZ2E_MTF_CHUNKS + t]) nseen++;
        uint32_t unseen = 0;
        for (uint32_t s = 0; s < 256; s++) {
            if (!used(s)) continue;
            const uint32_t key = lp[s * BZ2E_MTF_CHUNKS + t];
            uint32_t rank;
            if (!key) rank = nseen + unseen++;
            else {
                rank = 0;
                for (uint32_t s2 = 0; s2 < 256; s2++) if (used(s2) && lp[s2 * BZ2E_MTF_CHUNKS + t] > key) rank++;
            }
            s_list[rank * BZ2E_MTF_CHUNKS + t] = (uint8_t)s;                // (rank < the used bytes <= 256)
        }
        // the walk: every byte of L is a used byte, so it is in the list
        for (uint32_t i = i0; i < i1; i++) {
            const uint8_t b = L[i];
            uint8_t tmp = s_list[t];
            uint32_t q = 0;
            while (tmp != b && q < 255u) {
                q++;
                const uint8_t nx = s_list[q * BZ2E_MTF_CHUNKS + t];
                s_list[q * BZ2E_MTF_CHUNKS + t] = tmp;
                tmp = nx;
            }
            s_list[t] = b;
            rk[i] = (uint8_t)q;
        }
    }
}

// ---- stage 5: symbols ---------------------------------------------------------------------------------------------------------------------------
// Rank r >= 1 is symbol r + 1; a run of z zeros is floor(log2(z + 1)) digits RUNA / RUNB in bijective base 2, least significant first,
// written by the lane of the run's last zero, which knows z from the max-scan of the runs' starts; then the end symbol.
__global__ __launch_bounds__(256) void k_bz2e_syms(const bz2e_desc* desc, rcx_bz2e_hdr* hdr, bz2e_round R)
{
    __shared__ uint32_t s_w[4];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= R.count) return;
    const uint32_t n = desc[R.b0 + j].n;
    const uint8_t* rk = R.rk + (size_t)j * R.st_rk;
    uint16_t* sym = (uint16_t*)(R.sym + (size_t)j * R.st_sym);              // n + 1 of them at the most: a symbol a byte of L, and the end
    uint32_t last_start = 0, out = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + tid;
        const bool valid = i < n;
        const uint32_t r = valid ? rk[i] : 1u;
        const uint32_t pr = (valid && i) ? rk[i - 1] : 1u, nr = (valid && i + 1 < n) ? rk[i + 1] : 1u;
        const bool z = valid && r == 0, zstart = z && pr != 0, zlast = z && nr != 0;
        uint32_t tot;
        uint32_t st = bz2e_wg_scan<true>(zstart ? i + 1 : 0u, s_w, tot);
        if (last_start > st) st = last_start;
        if (tot > last_start) last_start = tot;
        uint32_t zn = zlast ? i + 2 - st : 0u;                              // the run's length
        const uint32_t c = !valid ? 0u : !z ? 1u : zlast ? 31u - (uint32_t)__clz(zn + 1u) : 0u;
        uint32_t o = bz2e_wg_scan<false>(c, s_w, tot) - c + out;
        out += tot;
        if (valid && !z) { if (o < n) sym[o] = (uint16_t)(r + 1u); }
        else if (zlast) {
            while (zn && o < n) {
                if (zn & 1u) { sym[o++] = 0; zn = (zn - 1u) >> 1; }
                else { sym[o++] = 1; zn = (zn - 2u) >> 1; }
            }
        }
    }
    if (tid == 0) {
        rcx_bz2e_hdr* h = hdr + R.b0 + j;
        uint32_t u = 0;
        for (uint32_t w = 0; w < 8; w++) u += (uint32_t)__popc(h->used[w]);
        h->alpha = u + 2u;
        if (out <= n) sym[out] = (uint16_t)(u + 1u);
        h->nmtf = out + 1u;
    }
}

// ---- stage 6: the tables -----------------------------------------------------------------------------------------------------------------------------
// MSB-first bits of one thread's contiguous range, merged into zeroed words (the boundary words are shared with neighbours).  Word w holds
// the stream's bits 32w .. 32w + 31, the first in its top bit: the joiner reads them the same way.
struct Bz2eBits {
    uint32_t* w; uint32_t wi, n; uint64_t acc;                              // the top n bits of acc are pending
    __device__ void start(uint32_t* words, uint32_t bit) { w = words; wi = bit >> 5; n = bit & 31u; acc = 0; }
    __device__ void put(uint32_t v, uint32_t nb)                            // nb <= 32, v < 2^nb
    {
        if (!nb) return;
        acc |= (uint64_t)v << (64u - n - nb);
        n += nb;
        if (n >= 32) { atomicOr(&w[wi], (uint32_t)(acc >> 32)); wi++; acc <<= 32; n -= 32; }
    }
    __device__ void flush() { if (n) atomicOr(&w[wi], (uint32_t)(acc >> 32)); }
};
// Everything of a block in front of its symbols: the mark, the CRC, origPtr, the used-byte map, the selectors (MTF, unary) and the tables
// (delta-coded).  One lane.  WRITE false only counts, by the same walk: the fit's length and the packer's bits cannot differ.
template <bool WRITE>
__device__ uint32_t bz2e_head(Bz2eBits* w, const rcx_bz2e_hdr* h, uint32_t ngroups, uint32_t nsel, uint32_t alpha, const uint8_t* sel,
                              const uint8_t* lens /* [6][258] */)
{
    uint32_t bits = 0;
    auto put = [&](uint32_t v, uint32_t nb) { if (WRITE) w->put(v, nb); bits += nb; };
    put((uint32_t)(BZ2E_MARK_BLOCK >> 24), 24); put((uint32_t)(BZ2E_MARK_BLOCK & 0xffffffu), 24);
    put(h->crc >> 16, 16); put(h->crc & 0xffffu, 16);
    put(0, 1);
    put(h->orig, 24);
    uint32_t top = 0;
    for (uint32_t i = 0; i < 16; i++) if ((h->used[i >> 1] >> ((i & 1u) * 16u)) & 0xffffu) top |= 1u << (15u - i);
    put(top, 16);
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t m = (h->used[i >> 1] >> ((i & 1u) * 16u)) & 0xffffu;
        if (m) put(__brev(m) >> 16, 16);                                    // (byte 16 i + j is bit 15 - j)
    }
    put(ngroups, 3);
    put(nsel, 15);
    uint8_t order[6] = {0, 1, 2, 3, 4, 5};
    for (uint32_t i = 0; i < nsel; i++) {
        const uint8_t v = sel[i];
        uint32_t q = 0;
        while (q < 5 && order[q] != v) q++;
        for (uint32_t x = q; x > 0; x--) order[x] = order[x - 1];
        order[0] = v;
        put((1u << (q + 1)) - 2u, q + 1);                                   // q ones, a zero
    }
    for (uint32_t t = 0; t < ngroups; t++) {
        const uint8_t* ln = lens + t * BZ2E_ALPHA;
        uint32_t cur = ln[0];
        put(cur, 5);
        for (uint32_t s = 0; s < alpha; s++) {
            while (cur < ln[s]) { put(2, 2); cur++; }
            while (cur > ln[s]) { put(3, 2); cur--; }
            put(0, 1);
        }
    }
    return bits;
}
// code lengths of the symbols sorted[0 .. nu) (ascending by weight max(count, 1), ties by index), at most 17 bits: k_deflate_encode.hip's
// de_code_lengths restated (one lane; nu >= 3: a used byte, RUNA / RUNB and the end symbol)
__device__ void bz2e_code_lengths(const uint32_t* cnt, const uint16_t* sorted, uint32_t nu, uint8_t* lens, uint32_t* A)
{
    const uint32_t lim = BZ2E_LIMIT;
    for (uint32_t i = 0; i < nu; i++) { const uint32_t c = cnt[sorted[i]]; A[i] = c ? c : 1u; }
    // Moffat & Katajainen, in place: A[i] becomes the depth of the i-th lightest symbol
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
    // counts per length, what lies above the limit folded into it and pushed down until the Kraft sum is exactly 1
    uint32_t cl[33];
    for (int i = 0; i < 33; i++) cl[i] = 0;
    for (uint32_t i = 0; i < nu; i++) cl[A[i] < 32 ? A[i] : 32]++;
    for (uint32_t i = lim + 1; i <= 32; i++) { cl[lim] += cl[i]; cl[i] = 0; }
    uint32_t total = 0;
    for (uint32_t i = lim; i > 0; i--) total += cl[i] << (lim - i);
    while (total != (1u << lim)) {
        cl[lim]--;
        for (uint32_t i = lim - 1; i > 0; i--) if (cl[i]) { cl[i]--; cl[i + 1] += 2; break; }
        total--;
    }
    // the heaviest symbols get the shortest codes
    uint32_t j = nu;
    for (uint32_t i = 1; i <= lim; i++) for (uint32_t c = cl[i]; c > 0; c--) lens[sorted[--j]] = (uint8_t)i;
}
// symbol i of a block, kept below alpha whatever the scratch holds: it indexes LDS tables
__device__ __forceinline__ uint32_t bz2e_sym(const uint16_t* sym, uint32_t i, uint32_t alpha) { const uint32_t s = sym[i]; return s < alpha ? s : alpha - 1u; }
// One workgroup a block.  Leaves the lengths (lens[6][258]), the selectors of the fourth iteration, the groups' bit costs under the tables
// computed after it, and in the record nGroups, nSelectors, the header's bits and the block's.
__global__ __launch_bounds__(256) void k_bz2e_fit(const bz2e_desc* desc, rcx_bz2e_hdr* hdr, bz2e_round R)
{
    __shared__ uint32_t s_freq[BZ2E_ALPHA];
    __shared__ uint32_t s_cnt[6][BZ2E_ALPHA];
    __shared__ uint32_t s_A[6][BZ2E_ALPHA];
    __shared__ uint16_t s_sorted[6][BZ2E_ALPHA];
    __shared__ uint8_t s_len[6 * BZ2E_ALPHA];
    __shared__ uint32_t s_bits;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= R.count) return;
    rcx_bz2e_hdr* h = hdr + R.b0 + j;
    const uint32_t nmtf = h->nmtf, alpha = h->alpha;
    const uint16_t* sym = (const uint16_t*)(R.sym + (size_t)j * R.st_sym);
    uint8_t* sel = R.sel + (size_t)j * R.st_sel;
    uint16_t* gcost = (uint16_t*)(R.gcost + (size_t)j * R.st_gcost);
    const uint32_t ng = nmtf < 200 ? 2u : nmtf < 600 ? 3u : nmtf < 1200 ? 4u : nmtf < 2400 ? 5u : 6u;
    const uint32_t nsel = (nmtf + 49u) / 50u;
    for (uint32_t s = tid; s < BZ2E_ALPHA; s += 256) s_freq[s] = 0;
    if (tid == 0) s_bits = 0;
    __syncthreads();
    for (uint32_t i = tid; i < nmtf; i += 256) atomicAdd(&s_freq[bz2e_sym(sym, i, alpha)], 1u);
    __syncthreads();
    if (tid == 0) {                                                         // libbz2's initial partition: length 0 inside a table's range, 15 outside
        uint32_t rem = nmtf;
        int gs = 0;
        for (uint32_t part = ng; part > 0; part--) {
            const uint32_t target = rem / part;
            int ge = gs - 1;
            uint32_t acc = 0;
            while (acc < target && ge < (int)alpha - 1) { ge++; acc += s_freq[ge]; }
            if (ge > gs && part != ng && part != 1 && ((ng - part) & 1u)) { acc -= s_freq[ge]; ge--; }
            for (int v = 0; v < (int)alpha; v++) s_len[(part - 1) * BZ2E_ALPHA + v] = (v >= gs && v <= ge) ? 0 : 15;
            gs = ge + 1;
            rem -= acc;
        }
    }
    __syncthreads();
    for (int it = 0; it < 4; it++) {
        for (uint32_t s = tid; s < 6 * BZ2E_ALPHA; s += 256) (&s_cnt[0][0])[s] = 0;
        __syncthreads();
        for (uint32_t g = tid; g < nsel; g += 256) {                        // every group of 50 takes the cheapest table, the lowest on ties
            const uint32_t a = g * 50u, e = a + 50u < nmtf ? a + 50u : nmtf;
            uint32_t cost[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t i = a; i < e; i++) {
                const uint32_t s = bz2e_sym(sym, i, alpha);
#pragma unroll
                for (uint32_t t = 0; t < 6; t++) cost[t] += s_len[t * BZ2E_ALPHA + s];
            }
            uint32_t best = 0;
            for (uint32_t t = 1; t < ng; t++) if (cost[t] < cost[best]) best = t;
            sel[g] = (uint8_t)best;
            for (uint32_t i = a; i < e; i++) atomicAdd(&s_cnt[best][bz2e_sym(sym, i, alpha)], 1u);
        }
        __syncthreads();
        // every table, chosen or not, gets new lengths: the symbols by (weight, index) -- a rank sort, all threads --, then a lane a table
        for (uint32_t x = tid; x < ng * alpha; x += 256) {
            const uint32_t t = x / alpha, s = x - t * alpha;
            const uint32_t w = s_cnt[t][s] ? s_cnt[t][s] : 1u;
            uint32_t rank = 0;
            for (uint32_t s2 = 0; s2 < alpha; s2++) {
                const uint32_t w2 = s_cnt[t][s2] ? s_cnt[t][s2] : 1u;
                rank += (w2 < w || (w2 == w && s2 < s)) ? 1u : 0u;
            }
            s_sorted[t][rank] = (uint16_t)s;
        }
        __syncthreads();
        if (tid < ng) bz2e_code_lengths(s_cnt[tid], s_sorted[tid], alpha, s_len + tid * BZ2E_ALPHA, s_A[tid]);
        __syncthreads();
    }
    // the groups' costs under the tables as they are written
    for (uint32_t g = tid; g < nsel; g += 256) {
        const uint32_t a = g * 50u, e = a + 50u < nmtf ? a + 50u : nmtf;
        const uint8_t* ln = s_len + (uint32_t)sel[g] * BZ2E_ALPHA;
        uint32_t c = 0;
        for (uint32_t i = a; i < e; i++) c += ln[bz2e_sym(sym, i, alpha)];
        gcost[g] = (uint16_t)c;                                             // (<= 50 x 17)
        atomicAdd(&s_bits, c);
    }
    uint8_t* lens = R.lens + (size_t)j * R.st_lens;
    for (uint32_t s = tid; s < 6 * BZ2E_ALPHA; s += 256) lens[s] = s_len[s];
    __syncthreads();
    if (tid == 0) {
        const uint32_t head = bz2e_head<false>(nullptr, h, ng, nsel, alpha, sel, s_len);
        h->ngroups = ng; h->nsel = nsel; h->head_bits = head; h->bits = head + s_bits;
    }
}

// ---- stage 7: the block's bits --------------------------------------------------------------------------------------------------------------------
// store: the call's packed blocks, zeroed for this round's.  Codes are canonical in (length, symbol) order.
__global__ __launch_bounds__(256) void k_bz2e_pack(const bz2e_desc* desc, const rcx_bz2e_hdr* hdr, bz2e_round R, uint8_t* store)
{
    __shared__ uint32_t s_code[6 * BZ2E_ALPHA];
    __shared__ uint8_t s_len[6 * BZ2E_ALPHA];
    __shared__ uint32_t s_w[4];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= R.count) return;
    const rcx_bz2e_hdr* h = hdr + R.b0 + j;
    const uint32_t nmtf = h->nmtf, alpha = h->alpha, ng = h->ngroups, nsel = h->nsel, head = h->head_bits;
    const uint16_t* sym = (const uint16_t*)(R.sym + (size_t)j * R.st_sym);
    const uint8_t* sel = R.sel + (size_t)j * R.st_sel;
    const uint16_t* gcost = (const uint16_t*)(R.gcost + (size_t)j * R.st_gcost);
    const uint8_t* lens = R.lens + (size_t)j * R.st_lens;
    uint32_t* words = (uint32_t*)(store + desc[R.b0 + j].store);
    for (uint32_t s = tid; s < 6 * BZ2E_ALPHA; s += 256) s_len[s] = lens[s];
    __syncthreads();
    if (tid < ng) {
        const uint8_t* ln = s_len + tid * BZ2E_ALPHA;
        uint32_t* code = s_code + tid * BZ2E_ALPHA;
        uint32_t c = 0;
        for (uint32_t l = 1; l <= BZ2E_LIMIT; l++) {
            for (uint32_t s = 0; s < alpha; s++) if (ln[s] == l) code[s] = c++;
            c <<= 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        Bz2eBits w;
        w.start(words, 0);
        bz2e_head<true>(&w, h, ng, nsel, alpha, sel, s_len);
        w.flush();
    }
    uint32_t run = 0;
    for (uint32_t base = 0; base < nsel; base += 256) {
        const uint32_t g = base + tid;
        const bool valid = g < nsel;
        const uint32_t cost = valid ? gcost[g] : 0u;
        uint32_t tot;
        const uint32_t o = bz2e_wg_scan<false>(cost, s_w, tot) - cost + run;
        run += tot;
        if (valid) {
            const uint32_t a = g * 50u, e = a + 50u < nmtf ? a + 50u : nmtf, t = sel[g];
            Bz2eBits w;
            w.start(words, head + o);                                       // (head + o + cost <= the block's bits <= what its slot of the store holds)
            for (uint32_t i = a; i < e; i++) { const uint32_t s = bz2e_sym(sym, i, alpha); w.put(s_code[t * BZ2E_ALPHA + s], s_len[t * BZ2E_ALPHA + s]); }
            w.flush();
        }
    }
}

// ---- stage 8: the files ----------------------------------------------------------------------------------------------------------------------------
struct bz2e_file {
    uint64_t out_at, out_len;            // the slot in out_base, the stream's bytes
    uint64_t tail_bit;                   // where the end mark starts
    uint32_t first, count;               // its blocks
    uint32_t crc, level;
    int32_t status; uint32_t pad;
};
// k <= 8 bits at bit o of MSB-first words (the word behind the last one a block uses is its slot's slack)
__device__ __forceinline__ uint32_t bz2e_get(const uint32_t* words, uint64_t o, uint32_t k)
{
    const uint64_t two = ((uint64_t)words[o >> 5] << 32) | words[(o >> 5) + 1];
    return (uint32_t)(two >> (64u - (uint32_t)(o & 31u) - k)) & ((1u << k) - 1u);
}
// Workgroup (x, y): file y, a thread per output byte.  A byte is put together from the sources that cover its 8 bits: nothing is read from
// the caller's buffer and nothing of it is written twice.
__global__ __launch_bounds__(256) void k_bz2e_join(const bz2e_file* files, const bz2e_desc* desc, const rcx_bz2e_hdr* hdr, const uint64_t* bit_off,
                                                   const uint8_t* store, uint8_t* out_base)
{
    const bz2e_file F = files[blockIdx.y];
    if (F.status != RCX_OK) return;
    const uint32_t head = 0x425a6830u + F.level;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < F.out_len; q += (uint64_t)gridDim.x * 256) {
        uint64_t pos = q * 8;
        uint32_t need = 8, val = 0;
        while (need) {
            uint32_t k, v;
            if (pos < RCX_BZ2E_HEAD_BITS) {
                k = need < 32u - (uint32_t)pos ? need : 32u - (uint32_t)pos;
                v = (head >> (32u - (uint32_t)pos - k)) & ((1u << k) - 1u);
            } else if (pos >= F.tail_bit) {
                k = need; v = 0;
                for (uint32_t x = 0; x < k; x++) {
                    const uint64_t idx = pos + x - F.tail_bit;
                    const uint32_t bit = idx < 48 ? (uint32_t)((BZ2E_MARK_END >> (47 - idx)) & 1ull) : idx < 80 ? (F.crc >> (79 - idx)) & 1u : 0u;
                    v = (v << 1) | bit;
                }
            } else {
                uint32_t lo = F.first, hi = F.first + F.count - 1;         // the last block whose bits start at or before pos
                while (lo < hi) { const uint32_t mid = (lo + hi + 1) / 2; if (bit_off[mid] <= pos) lo = mid; else hi = mid - 1; }
                const uint64_t o = pos - bit_off[lo], left = hdr[lo].bits - o;
                k = need < left ? need : (uint32_t)left;
                v = bz2e_get((const uint32_t*)(store + desc[lo].store), o, k);
            }
            val = (val << k) | v; pos += k; need -= k;
        }
        out_base[F.out_at + q] = (uint8_t)val;
    }
}

// ---- the call -----------------------------------------------------------------------------------------------------------------------------------
// h_*: the batch's offsets, lengths and capacities on the host (k's arrays are the device's).  level: the digit of the header, 1..9.  C:
// the bytes of run-length form a block holds; the C entry point passes 100000 * level - 19, a test harness may pass less.  round: blocks a round (0:
// RCX_BZ2E_ROUND).  alloc: buffer 0 the stages', 1 the sort's, 2 what lasts for the call (the blocks' records and the store).  Results go to
// k.out_len, k.in_used and k.status by a copy at the end.
static int launch_bzip2_encode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_off, const uint64_t* h_in_len, const uint64_t* h_out_off,
                               const uint64_t* h_out_cap, const rcx_bz2_alloc& alloc, int level, uint32_t C, uint32_t round, std::string& err,
                               const rcx_bz2e_watch* watch = nullptr)
{
    const uint32_t n = k.nblocks;
    if (!n) return RCX_RC_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_cap || !alloc.get) { err = "bzip2 encode: use rcx_bzip2_encode_batch"; return RCX_RC_BAD_ARG; }
    if (level < 1 || level > 9) { err = "bzip2 encode: level must be 1..9"; return RCX_RC_BAD_ARG; }
    if (n > BZ2E_MAX_FILES) { err = "bzip2 encode: at most 65535 files a call"; return RCX_RC_BAD_ARG; }
    if (C < 1 || C > 100000u * (uint32_t)level - 19u) { err = "bzip2 encode: a chunk's block holds 1 .. 100000 x level - 19 bytes"; return RCX_RC_BAD_ARG; }
    if (round > RCX_BZ2E_ROUND_MAX) { err = "bzip2 encode: blocks a round must be 0 (default) or 1..4096"; return RCX_RC_BAD_ARG; }
#define BZ2E_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return RCX_RC_HIP_ERROR; } } while (0)
#define BZ2E_LAUNCHED() BZ2E_HIP(hipGetLastError())
    auto up = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    auto aligned = [](void* p) { return (uint8_t*)(((uintptr_t)p + 255u) & ~(uintptr_t)255u); };
    // ---- the blocks: the pieces of C input bytes, measured; the chunks of every file, measured
    std::vector<rcx_bz2e_block> chunks, blocks;
    if (!rcx_plan_bz2e_chunks(n, h_in_len, C, chunks, err)) return RCX_RC_BAD_ARG;
    std::vector<bz2e_desc> h_desc;
    std::vector<uint32_t> h_n;
    auto measure = [&](std::vector<rcx_bz2e_block>& v) -> int {            // fills in n where it is 0
        h_desc.clear();
        for (const rcx_bz2e_block& b : v) if (!b.n) h_desc.push_back(bz2e_desc{h_in_off[b.file] + b.off, b.len, 0u, 0ull});
        const uint32_t cnt = (uint32_t)h_desc.size();
        if (!cnt) return RCX_RC_OK;
        uint8_t* base = (uint8_t*)alloc.get(alloc.self, 0, up((uint64_t)cnt * sizeof(bz2e_desc)) + up((uint64_t)cnt * 4) + 512);
        if (!base) { err = "bzip2 encode: no scratch"; return RCX_RC_NO_MEMORY; }
        base = aligned(base);
        uint32_t* d_n = (uint32_t*)(base + up((uint64_t)cnt * sizeof(bz2e_desc)));
        h_n.resize(cnt);
        BZ2E_HIP(hipMemcpyAsync(base, h_desc.data(), (uint64_t)cnt * sizeof(bz2e_desc), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bz2e_rle_len, dim3(cnt), dim3(256), 0, s, k.in_base, (const bz2e_desc*)base, d_n, cnt);
        BZ2E_LAUNCHED();
        BZ2E_HIP(hipMemcpyAsync(h_n.data(), d_n, (uint64_t)cnt * 4, hipMemcpyDeviceToHost, s));
        BZ2E_HIP(hipStreamSynchronize(s));
        uint32_t q = 0;
        for (rcx_bz2e_block& b : v) if (!b.n) b.n = h_n[q++];
        return RCX_RC_OK;
    };
    { const int rc = measure(chunks); if (rc) return rc; }
    // every file's chunk length: from the pieces' forms, then lowered while a chunk's form is over C (rcx_plan.h)
    std::vector<uint64_t> step(n, 0);
    std::vector<uint8_t> settled(n, 0);
    {
        std::vector<uint64_t> sum(n, 0);
        for (const rcx_bz2e_block& c : chunks) sum[c.file] += c.n;
        for (uint32_t f = 0; f < n; f++) { settled[f] = h_in_len[f] ? 0 : 1; if (h_in_len[f]) step[f] = rcx_plan_bz2e_step(h_in_len[f], sum[f], C); }
    }
    std::vector<std::vector<rcx_bz2e_block>> file_blocks(n);
    std::vector<rcx_bz2e_block> probe;
    for (uint32_t turn = 0; turn < RCX_BZ2E_TURNS; turn++) {              // (rcx_plan.h has the bound; two probes at the most for ordinary files)
        probe.clear();
        for (uint32_t f = 0; f < n; f++) if (!settled[f]) rcx_plan_bz2e_cut(f, h_in_len[f], step[f], probe);
        if (probe.empty()) break;
        { const int rc = measure(probe); if (rc) return rc; }
        for (size_t q = 0; q < probe.size();) {
            const uint32_t f = probe[q].file;
            size_t e = q;
            uint32_t longest = 0;
            while (e < probe.size() && probe[e].file == f) { longest = std::max(longest, probe[e].n); e++; }
            if (longest <= C) { file_blocks[f].assign(probe.begin() + q, probe.begin() + e); settled[f] = 1; }
            else step[f] = rcx_plan_bz2e_less(step[f], longest, C, turn);
            q = e;
        }
    }
    for (uint32_t f = 0; f < n; f++) {
        if (!settled[f]) { err = "bzip2 encode: internal: a file's chunk length did not settle"; return RCX_RC_BAD_ARG; }   // (cannot happen: a chunk of one byte fits, and RCX_BZ2E_TURNS reach it)
        blocks.insert(blocks.end(), file_blocks[f].begin(), file_blocks[f].end());
    }
    const uint32_t nb = (uint32_t)blocks.size();
    uint32_t max_n = 1;
    for (const rcx_bz2e_block& b : blocks) {
        if (b.n < 1 || b.n > C) { err = "bzip2 encode: a block's run-length form does not fit its block"; return RCX_RC_HIP_ERROR; }   // (cannot happen: the chunks were measured)
        max_n = std::max(max_n, b.n);
    }
    // ---- what lasts for the call: the blocks' descriptors and records, their bit offsets, the files, the store
    std::vector<bz2e_desc> desc(nb);
    uint64_t store_bytes = 0;
    for (uint32_t b = 0; b < nb; b++) {
        desc[b] = bz2e_desc{h_in_off[blocks[b].file] + blocks[b].off, blocks[b].len, blocks[b].n, store_bytes};
        store_bytes += up(rcx_plan_bz2e_block_bound(blocks[b].n));
    }
    struct { uint64_t desc, hdr, bit_off, files, store, end; } keep;
    keep.desc = 0;
    keep.hdr = keep.desc + up((uint64_t)nb * sizeof(bz2e_desc));
    keep.bit_off = keep.hdr + up((uint64_t)nb * sizeof(rcx_bz2e_hdr));
    keep.files = keep.bit_off + up((uint64_t)nb * 8);
    keep.store = keep.files + up((uint64_t)n * sizeof(bz2e_file));
    keep.end = keep.store + store_bytes;
    uint8_t* kb = (uint8_t*)alloc.get(alloc.self, 2, keep.end + 512);
    if (!kb) { err = "bzip2 encode: no scratch for the packed blocks"; return RCX_RC_NO_MEMORY; }
    kb = aligned(kb);
    const bz2e_desc* d_desc = (const bz2e_desc*)(kb + keep.desc);
    rcx_bz2e_hdr* d_hdr = (rcx_bz2e_hdr*)(kb + keep.hdr);
    uint8_t* d_store = kb + keep.store;
    std::vector<rcx_bz2e_hdr> h_hdr(nb);
    if (nb) {
        BZ2E_HIP(hipMemcpyAsync(kb + keep.desc, desc.data(), (uint64_t)nb * sizeof(bz2e_desc), hipMemcpyHostToDevice, s));
        BZ2E_HIP(hipMemsetAsync(d_hdr, 0, (uint64_t)nb * sizeof(rcx_bz2e_hdr), s));
    }
    // ---- the rounds.  A slot of every area holds the largest block of the call
    const uint64_t max_sel = ((uint64_t)max_n + 1 + 49) / 50;
    bz2e_round R;
    memset(&R, 0, sizeof R);
    R.st_tt = up(2ull * max_n); R.st_sa = up(8ull * max_n); R.st_l = up(max_n); R.st_rk = up(max_n); R.st_sym = up(2ull * max_n + 2);
    R.st_lp = 256ull * BZ2E_MTF_CHUNKS * 4; R.st_sel = up(max_sel); R.st_gcost = up(2 * max_sel); R.st_lens = up(6 * BZ2E_ALPHA);
    const uint64_t per_block = R.st_tt + R.st_sa + R.st_l + R.st_rk + R.st_sym + R.st_lp + R.st_sel + R.st_gcost + R.st_lens + 64;
    uint32_t per_round = std::min(std::max(nb, 1u), round ? round : RCX_BZ2E_ROUND);
    if ((uint64_t)per_round * per_block > BZ2E_STAGE_BYTES) per_round = (uint32_t)std::max<uint64_t>(1, BZ2E_STAGE_BYTES / per_block);
    std::vector<uint32_t> cuts;
    rcx_plan_bz2e_rounds(nb, per_round, cuts);
    uint8_t* base = nullptr;
    uint64_t o_args = 0;
    if (nb) {
        o_args = (uint64_t)per_round * (per_block - 64);
        base = (uint8_t*)alloc.get(alloc.self, 0, o_args + up((uint64_t)per_round * 56) + 512);
        if (!base) { err = "bzip2 encode: no scratch"; return RCX_RC_NO_MEMORY; }
        base = aligned(base);
        uint8_t* p = base;
        R.tt = p; p += per_round * R.st_tt; R.sa = p; p += per_round * R.st_sa; R.l = p; p += per_round * R.st_l; R.rk = p; p += per_round * R.st_rk;
        R.sym = p; p += per_round * R.st_sym; R.lp = p; p += per_round * R.st_lp; R.sel = p; p += per_round * R.st_sel;
        R.gcost = p; p += per_round * R.st_gcost; R.lens = p;
    }
    std::vector<uint64_t> d64; std::vector<uint32_t> d32; std::vector<int32_t> h_st;
    for (size_t r = 0; r + 1 < cuts.size(); r++) {
        const uint32_t b0 = cuts[r], cnt = cuts[r + 1] - b0;
        R.b0 = b0; R.count = cnt;
        uint32_t round_max = 1;
        for (uint32_t j = 0; j < cnt; j++) round_max = std::max(round_max, blocks[b0 + j].n);
        // the store of this round's blocks starts as zeros: the packer merges into it
        const uint64_t s0 = desc[b0].store, s1 = b0 + cnt < nb ? desc[b0 + cnt].store : store_bytes;
        BZ2E_HIP(hipMemsetAsync(d_store + s0, 0, s1 - s0, s));
        hipLaunchKernelGGL(k_bz2e_rle, dim3(cnt), dim3(256), 0, s, k.in_base, d_desc, d_hdr, R);
        BZ2E_LAUNCHED();
        // the sort: kargs that point at the T || T blocks, the suffix arrays as 32-bit words into their slots
        d64.assign((size_t)6 * cnt, 0); d32.assign((size_t)2 * cnt, 0);
        for (uint32_t j = 0; j < cnt; j++) {
            d64[j] = (uint64_t)j * R.st_tt; d64[cnt + j] = 2ull * blocks[b0 + j].n;
            d64[2 * cnt + j] = (uint64_t)j * R.st_sa; d64[3 * cnt + j] = 8ull * blocks[b0 + j].n;
        }
        uint64_t* dd = (uint64_t*)(base + o_args);
        uint32_t* dw = (uint32_t*)(dd + (size_t)6 * cnt);
        BZ2E_HIP(hipMemcpyAsync(dd, d64.data(), (size_t)6 * cnt * 8, hipMemcpyHostToDevice, s));
        BZ2E_HIP(hipMemcpyAsync(dw, d32.data(), (size_t)2 * cnt * 4, hipMemcpyHostToDevice, s));
        const uint64_t sort_bytes = rcx_tu_bwt_forward_scratch(cnt, 2ull * round_max);
        uint8_t* sort = (uint8_t*)alloc.get(alloc.self, 1, sort_bytes + 512);
        if (!sort) { err = "bzip2 encode: no scratch for the sort"; return RCX_RC_NO_MEMORY; }
        rcx_kargs ks;
        memset(&ks, 0, sizeof ks);
        ks.in_base = R.tt; ks.in_off = dd; ks.in_len = dd + cnt;
        ks.out_base = R.sa; ks.out_off = dd + 2 * cnt; ks.out_cap = dd + 3 * cnt;
        ks.out_len = dd + 4 * cnt; ks.in_used = dd + 5 * cnt; ks.status = (int32_t*)dw; ks.aux = dw + cnt;
        ks.scratch = aligned(sort); ks.scratch_bytes = sort_bytes; ks.nblocks = cnt;
        { const int rc = rcx_tu_bwt_forward(s, ks, 0, err, true); if (rc) return rc; }
        BZ2E_LAUNCHED();
        hipLaunchKernelGGL(k_bz2e_pick, dim3(cnt), dim3(256), 0, s, d_desc, d_hdr, R);
        hipLaunchKernelGGL(k_bz2e_mtf, dim3(cnt), dim3(BZ2E_MTF_CHUNKS), 0, s, d_desc, (const rcx_bz2e_hdr*)d_hdr, R);
        hipLaunchKernelGGL(k_bz2e_syms, dim3(cnt), dim3(256), 0, s, d_desc, d_hdr, R);
        hipLaunchKernelGGL(k_bz2e_fit, dim3(cnt), dim3(256), 0, s, d_desc, d_hdr, R);
        hipLaunchKernelGGL(k_bz2e_pack, dim3(cnt), dim3(256), 0, s, d_desc, (const rcx_bz2e_hdr*)d_hdr, R, d_store);
        BZ2E_LAUNCHED();
        h_st.resize(cnt);
        BZ2E_HIP(hipMemcpyAsync(h_hdr.data() + b0, d_hdr + b0, (uint64_t)cnt * sizeof(rcx_bz2e_hdr), hipMemcpyDeviceToHost, s));
        BZ2E_HIP(hipMemcpyAsync(h_st.data(), dw, (uint64_t)cnt * 4, hipMemcpyDeviceToHost, s));
        BZ2E_HIP(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < cnt; j++) {
            if (h_st[j] != RCX_OK) { err = "bzip2 encode: the sort refused a block"; return RCX_RC_HIP_ERROR; }
            if ((uint64_t)(h_hdr[b0 + j].bits + 31) / 32 * 4 + 16 > rcx_plan_bz2e_block_bound(blocks[b0 + j].n)) { err = "bzip2 encode: a block outgrew its bound"; return RCX_RC_HIP_ERROR; }   // (cannot happen)
        }
        if (watch)
            for (uint32_t j = 0; j < cnt; j++)
                watch->block(watch->self, b0 + j, &blocks[b0 + j], R.tt + (size_t)j * R.st_tt, R.l + (size_t)j * R.st_l, &h_hdr[b0 + j],
                             (const uint16_t*)(R.sym + (size_t)j * R.st_sym), R.lens + (size_t)j * R.st_lens, R.sel + (size_t)j * R.st_sel);
        if (watch) watch->round(watch->self);
    }
    // ---- the files: bit offsets, combined CRCs, sizes against the capacities; then the gather
    std::vector<uint64_t> bits(nb), bit_off;
    std::vector<uint32_t> crc(nb);
    for (uint32_t b = 0; b < nb; b++) { bits[b] = h_hdr[b].bits; crc[b] = h_hdr[b].crc; }
    std::vector<rcx_bz2e_file> files;
    rcx_plan_bz2e_layout(n, blocks, bits.data(), crc.data(), h_out_cap, bit_off, files);
    std::vector<bz2e_file> h_files(n);
    uint64_t max_out = 0;
    for (uint32_t i = 0; i < n; i++) {
        const rcx_bz2e_file& F = files[i];
        h_files[i] = bz2e_file{h_out_off[i], F.out_len, F.bits - RCX_BZ2E_TAIL_BITS, F.first, F.count, F.crc, (uint32_t)level, F.status, 0u};
        if (F.status == RCX_OK) max_out = std::max(max_out, F.out_len);
    }
    if (max_out) {
        if (nb) BZ2E_HIP(hipMemcpyAsync(kb + keep.bit_off, bit_off.data(), (uint64_t)nb * 8, hipMemcpyHostToDevice, s));
        BZ2E_HIP(hipMemcpyAsync(kb + keep.files, h_files.data(), (uint64_t)n * sizeof(bz2e_file), hipMemcpyHostToDevice, s));
        const uint32_t gx = (uint32_t)std::min<uint64_t>((max_out + 255) / 256, 4096);
        hipLaunchKernelGGL(k_bz2e_join, dim3(gx, n), dim3(256), 0, s, (const bz2e_file*)(kb + keep.files), d_desc, (const rcx_bz2e_hdr*)d_hdr,
                           (const uint64_t*)(kb + keep.bit_off), (const uint8_t*)d_store, k.out_base);
        BZ2E_LAUNCHED();
    }
    std::vector<uint64_t> r_len(n), r_used(n);
    std::vector<int32_t> r_st(n);
    for (uint32_t i = 0; i < n; i++) { r_st[i] = files[i].status; r_len[i] = files[i].out_len; r_used[i] = files[i].status == RCX_OK ? h_in_len[i] : 0; }
    BZ2E_HIP(hipMemcpyAsync(k.out_len, r_len.data(), n * 8ull, hipMemcpyHostToDevice, s));
    if (k.in_used) BZ2E_HIP(hipMemcpyAsync(k.in_used, r_used.data(), n * 8ull, hipMemcpyHostToDevice, s));
    BZ2E_HIP(hipMemcpyAsync(k.status, r_st.data(), n * 4ull, hipMemcpyHostToDevice, s));
    BZ2E_HIP(hipStreamSynchronize(s));
#undef BZ2E_LAUNCHED
#undef BZ2E_HIP
    return RCX_RC_OK;
}
