// Drives the planning arithmetic of the encoders behind shared dictionaries on the CPU, as a program of its own so that it can be built
// with -fsanitize=address,undefined (tests/test_host_plan_dict.py does):
//   test_plan_dict plan      rcx_plan_dict of rust_compress_amd/csrc/rcx_plan.h: the clamp, the deduplication, the kernels' words, the
//                            refusals and their texts
//   test_plan_dict carve     hc_dict_scratch_bytes / dh_dict_scratch_bytes and lzd_carve in front of hc_carve / dh_carve: every array
//                            lies inside a scratch of exactly the bytes the host path allocates (each array's first and last byte is
//                            written in a heap block of that size), and what the dictionaries cost beyond the encoders without history
// Built with  g++ -include tests/wavesim/wavesim.h  (the .hip files' host code; no kernel runs).  Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#define hipStream_t int
static inline int hipMemsetAsync(void*, int, size_t, int) { return 0; }
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) do { } while (0)
#include "k_lz4_hc.hip"
#include "k_lz4_hc_dict.hip"
#include "k_inflate.hip"
#include "k_crc32.hip"
#include "k_deflate_encode.hip"
#include "k_deflate_hc.hip"
#include "k_deflate_hc_hist.hip"
#include "k_deflate_hc_dict.hip"
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<uint64_t> V64;
typedef std::vector<uint32_t> V32;

static uint64_t off_of(const rcx_dict_plan& p, uint32_t n, uint32_t i) { return p.aux[3 * (size_t)n + i] | ((uint64_t)p.aux[4 * (size_t)n + i] << 32); }

static void t_plan()
{
    rcx_dict_plan p; std::string err;
    // six blocks: none; a range; the same range; a range that overlaps it but differs; the first range again, its offset ignored where
    // the length is 0; a range beyond 4 GiB
    V64 off = {999, 100, 100, 150, 12345, (1ull << 33) + 7}, len = {0, 500, 500, 500, 0, 32768};
    V32 ids = {1, 2, 3, 4, 5, 6};
    CHECK(rcx_plan_dict(6, off.data(), len.data(), 32768, 32768, nullptr, "x", p, err));
    CHECK(p.aux.size() == 6 * RCX_DICT_WORDS && p.ndict == 3 && p.span == (1ull << 33) + 7 + 32768);
    CHECK(p.aux[0] == 0 && p.aux[1] == 500 && p.aux[2] == 500 && p.aux[3] == 500 && p.aux[4] == 0 && p.aux[5] == 32768);
    for (uint32_t i = 0; i < 6; i++) CHECK(p.aux[6 + i] == 0);                                  // (no ids)
    CHECK(p.aux[12 + 1] == p.aux[12 + 2] && p.aux[12 + 1] != p.aux[12 + 3] && p.aux[12 + 3] != p.aux[12 + 5] && p.aux[12 + 1] != p.aux[12 + 5]);
    CHECK(off_of(p, 6, 1) == 100 && off_of(p, 6, 2) == 100 && off_of(p, 6, 3) == 150 && off_of(p, 6, 5) == (1ull << 33) + 7);
    for (uint32_t j = 0; j < 3; j++) {                                                          // dictionary j's block names dictionary j
        const uint32_t b = p.aux[30 + j];
        CHECK(b < 6 && p.aux[b] && p.aux[12 + b] == j);
    }
    for (uint32_t j = 3; j < 6; j++) CHECK(p.aux[30 + j] == 6);                                 // (no block)
    CHECK(p.aux[30 + p.aux[12 + 1]] == 1);                                                      // (the lowest block that names it)
    CHECK(rcx_plan_dict(6, off.data(), len.data(), 32768, 32768, ids.data(), "x", p, err));
    for (uint32_t i = 0; i < 6; i++) CHECK(p.aux[6 + i] == ids[i]);
    // the clamp comes BEFORE ranges are compared: of 65536 LZ4 bytes the last 65535 count, and so [10, 65546) and [11, 65546) are one
    V64 o2 = {10, 11, 10}, l2 = {65536, 65535, 65535};
    CHECK(rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err));
    CHECK(p.ndict == 2 && p.aux[0] == 65535 && p.aux[1] == 65535 && p.aux[2] == 65535 && p.span == 65546);
    CHECK(off_of(p, 3, 0) == 11 && off_of(p, 3, 1) == 11 && off_of(p, 3, 2) == 10);
    CHECK(p.aux[6 + 0] == p.aux[6 + 1] && p.aux[6 + 0] != p.aux[6 + 2]);
    // DEFLATE: all 32768 bytes count
    V64 o3 = {10, 11}, l3 = {32768, 32767};
    CHECK(rcx_plan_dict(2, o3.data(), l3.data(), 32768, 32768, nullptr, "deflate encode", p, err) && p.ndict == 2 && p.aux[0] == 32768);
    // refusals name the block, behind the caller's prefix
    l3[1] = 32769;
    CHECK(!rcx_plan_dict(2, o3.data(), l3.data(), 32768, 32768, nullptr, "deflate encode", p, err));
    CHECK(err.find("deflate encode: block 1:") == 0 && err.find("a dictionary of 32769 bytes") != std::string::npos && err.find("at most 32768") != std::string::npos);
    l2[2] = 65537;
    CHECK(!rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err));
    CHECK(err.find("lz4 hc: block 2:") == 0 && err.find("at most 65536") != std::string::npos);
    l2[2] = ~0ull;
    CHECK(!rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err) && err.find("lz4 hc: block 2:") == 0);
    l2[2] = (1ull << 32) + 5;                                                                   // (no wrap into a small 32-bit word)
    CHECK(!rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err) && err.find("lz4 hc: block 2:") == 0);
    l2[2] = 100; o2[2] = ~0ull - 50;                                                            // a range that wraps
    CHECK(!rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err));
    CHECK(err.find("lz4 hc: block 2:") == 0 && err.find("wraps") != std::string::npos);
    o2[2] = ~0ull; l2[2] = 0;                                                                   // (an offset without a length is ignored)
    CHECK(rcx_plan_dict(3, o2.data(), l2.data(), 65536, 65535, nullptr, "lz4 hc", p, err) && p.ndict == 1 && p.span == 65546);
    // n = 0: nothing is read
    CHECK(rcx_plan_dict(0, nullptr, nullptr, 65536, 65535, nullptr, "x", p, err) && p.ndict == 0 && p.aux.empty() && p.span == 0);
    // many blocks over few dictionaries, and every block its own
    const uint32_t N = 5000;
    V64 o(N), l(N);
    for (uint32_t i = 0; i < N; i++) { o[i] = 1000 * (i % 7); l[i] = i % 7 == 3 ? 0 : 2048; }
    CHECK(rcx_plan_dict(N, o.data(), l.data(), 32768, 32768, nullptr, "x", p, err) && p.ndict == 6);
    for (uint32_t i = 0; i < N; i++) {
        if (!l[i]) { CHECK(p.aux[i] == 0); continue; }
        const uint32_t j = p.aux[2 * (size_t)N + i], b = p.aux[5 * (size_t)N + j];
        CHECK(j < 6 && b < N && off_of(p, N, b) == o[i] && p.aux[b] == 2048 && b == (i % 7));
    }
    for (uint32_t i = 0; i < N; i++) { o[i] = 3 * i; l[i] = 1 + i % 5; }
    CHECK(rcx_plan_dict(N, o.data(), l.data(), 32768, 32768, nullptr, "x", p, err) && p.ndict == N);
    std::vector<uint8_t> seen(N, 0);
    for (uint32_t i = 0; i < N; i++) { const uint32_t j = p.aux[2 * (size_t)N + i]; CHECK(j < N && !seen[j] && p.aux[5 * (size_t)N + j] == i); seen[j] = 1; }
}

template <class T> static void touch(T* p, uint64_t count, const uint8_t* lo, const uint8_t* hi)
{
    if (!count) return;
    CHECK((const uint8_t*)p >= lo && (const uint8_t*)(p + count) <= hi);
    p[0] = T(); p[count - 1] = T();                                       // (out of the heap block: AddressSanitizer says so)
}

static void t_carve()
{
    const uint32_t ns[] = {1, 2, 63, 64, 1000, 8212}, nds[] = {0, 1, 3, 64};
    for (uint32_t n : ns) for (uint32_t ndict : nds) for (uint32_t per = 0; per <= 2; per++) for (uint32_t sh = 0; sh < 4; sh++) {
        if (ndict > n) continue;
        if ((uint64_t)n * per > 128) continue;                            // (keeps the heap blocks small)
        const uint64_t segs = (uint64_t)n * per;
        {   // LZ4
            const uint64_t sb = hc_dict_scratch_bytes(n, segs, ndict);
            std::vector<uint8_t> heap(sb + 64);
            uint8_t* s = heap.data() + 1 + 85 * sh; uint8_t* hi = s + sb; uint8_t* rest;
            const LzdScratch z = lzd_carve(s, n, ndict, HC_DSLOT, &rest);
            CHECK(rest <= hi && ((uintptr_t)rest & 255) == 0);
            touch(z.table, (uint64_t)ndict << LZC_HBITS, s, rest); touch(z.dlink, (uint64_t)ndict * HC_DSLOT, s, rest); touch(z.tail, 4ull * n, s, rest);
            CHECK((uint8_t*)z.dlink >= (uint8_t*)(z.table + ((uint64_t)ndict << LZC_HBITS)) && (uint8_t*)z.tail >= (uint8_t*)(z.dlink + (uint64_t)ndict * HC_DSLOT));
            const HcScratch d = hc_carve(rest, sb - (uint64_t)(rest - s), n);
            CHECK(d.cap >= segs);
            touch(d.seg_first, n + 1, rest, hi); touch(d.blk_rf, n, rest, hi); touch(d.seg_dtail, d.cap, rest, hi);
            touch(d.cand, (uint64_t)HC_SEG * d.cap, rest, hi); touch(d.elen, (uint64_t)HC_ELEN * d.cap, rest, hi); touch(d.link, (uint64_t)HC_SEG * d.cap, rest, hi);
            // what the dictionaries cost beyond the encoder without history: a table and a link array each, a few words per block
            CHECK(sb - hc_scratch_bytes(n, segs) <= (uint64_t)ndict * 262144 + 32ull * n + 4096);
        }
        {   // DEFLATE
            const uint64_t sb = dh_dict_scratch_bytes(n, segs, ndict);
            std::vector<uint8_t> heap(sb + 64);
            uint8_t* s = heap.data() + 1 + 85 * sh; uint8_t* hi = s + sb; uint8_t* rest;
            const LzdScratch z = lzd_carve(s, n, ndict, DH_DSLOT, &rest);
            CHECK(rest <= hi && ((uintptr_t)rest & 255) == 0);
            touch(z.table, (uint64_t)ndict << LZC_HBITS, s, rest); touch(z.dlink, (uint64_t)ndict * DH_DSLOT, s, rest); touch(z.tail, 4ull * n, s, rest);
            DhScratch h;
            const DeScratch d = dh_carve(rest, sb - (uint64_t)(rest - s), n, h);
            CHECK(d.cap >= segs);
            touch(d.seg_first, n + 1, rest, hi); touch(d.pos, (uint64_t)DE_SEG * d.cap, rest, hi);
            touch(h.link, (uint64_t)DE_SEG * d.cap, rest, hi); touch(h.cand, (uint64_t)DE_SEG * d.cap, rest, hi);
            touch(h.elen, (uint64_t)DH_ELEN * d.cap, rest, hi); touch(h.price, 320ull * d.cap, rest, hi);
            CHECK(sb - dh_scratch_bytes(n, segs) <= (uint64_t)ndict * 262144 + 32ull * n + 4096);
        }
    }
    // the formula's point, on the dictionary workload: 65536 records of 2 KiB behind ONE dictionary.  The history calls take 128 KiB
    // more per record; these 256 KiB at the most for the dictionary and 8 bytes per record
    const uint32_t n = 65536;
    const uint64_t shared = hc_dict_scratch_bytes(n, n, 1) - hc_scratch_bytes(n, n);
    CHECK(shared <= 262144 + 32ull * n + 4096 && shared >= 262144);
    CHECK(dh_dict_scratch_bytes(n, n, 1) - dh_scratch_bytes(n, n) <= 262144 + 32ull * n + 4096);
}

int main(int argc, char** argv)
{
    const std::string w = argc > 1 ? argv[1] : "";
    if (w == "plan") t_plan();
    else if (w == "carve") t_carve();
    else { printf("usage: test_plan_dict plan|carve\n"); return 2; }
    printf("HOST_PLAN_OK %s\n", w.c_str());
    return 0;
}
