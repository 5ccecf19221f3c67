// Drives the planning arithmetic of the DEFLATE calls with history on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_host_plan_hist.py does):
//   test_plan_hist args      rcx_plan_hist of rust_compress_amd/csrc/rcx_plan.h: the argument checks and the aux words
//   test_plan_hist slots     dh_hist_scratch_bytes / dh_hist_carve of k_deflate_hc_hist.hip: every array of the carve, the history
//                            slots of the link array among them, lies inside a scratch of exactly the bytes the host path allocates
//                            (each array's first and last byte is written in a heap block of that size)
// Built with  g++ -include tests/wavesim/wavesim.h  (the .hip files' host code; no kernel runs).  Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#define hipStream_t int
static inline int hipMemsetAsync(void*, int, size_t, int) { return 0; }
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) do { } while (0)
#include "k_inflate.hip"
#include "k_crc32.hip"
#include "k_deflate_encode.hip"
#include "k_deflate_hc.hip"
#include "k_deflate_hc_hist.hip"
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<uint64_t> V64;
typedef std::vector<uint32_t> V32;

static void t_args()
{
    V32 aux; uint32_t nhist = 99; std::string err;
    V64 hist = {0, 5, 32768, 1}, off = {0, 5, 40000, 1ull << 40};
    V32 ids = {11, 22, 33, 0xffffffffu};
    CHECK(rcx_plan_hist(4, hist.data(), off.data(), 32768, nullptr, "x", aux, nhist, err));
    CHECK(aux == (V32{0, 5, 32768, 1}) && nhist == 3);
    CHECK(rcx_plan_hist(4, hist.data(), off.data(), 32768, ids.data(), "x", aux, nhist, err));
    CHECK(aux == (V32{0, 5, 32768, 1, 11, 22, 33, 0xffffffffu}) && nhist == 3);
    hist[2] = 32769;                                         // more than the window
    CHECK(!rcx_plan_hist(4, hist.data(), off.data(), 32768, nullptr, "deflate encode", aux, nhist, err));
    CHECK(err.find("deflate encode: block 2:") == 0 && err.find("at most 32768") != std::string::npos);
    hist[2] = 32768; hist[1] = 6;                            // more than lies in front of the block
    CHECK(!rcx_plan_hist(4, hist.data(), off.data(), 32768, ids.data(), "inflate", aux, nhist, err));
    CHECK(err.find("inflate: block 1:") == 0 && err.find("offset 5") != std::string::npos);
    hist[1] = 5; hist[0] = 1;                                // block 0 at offset 0 has nothing in front of it
    CHECK(!rcx_plan_hist(4, hist.data(), off.data(), 32768, nullptr, "x", aux, nhist, err) && err.find("x: block 0:") == 0);
    hist[0] = 0; hist[3] = ~0ull;                            // (no wrap into a small 32-bit word)
    CHECK(!rcx_plan_hist(4, hist.data(), off.data(), 32768, nullptr, "x", aux, nhist, err) && err.find("x: block 3:") == 0);
    hist[3] = (1ull << 32) + 5;
    CHECK(!rcx_plan_hist(4, hist.data(), off.data(), 32768, nullptr, "x", aux, nhist, err) && err.find("x: block 3:") == 0);
    // all zero: no block has a history
    V64 z(1000, 0), o(1000, 7);
    CHECK(rcx_plan_hist(1000, z.data(), o.data(), 32768, nullptr, "x", aux, nhist, err) && nhist == 0 && aux.size() == 1000);
    for (uint32_t i = 0; i < 1000; i++) { z[i] = i % 3 ? (i * 37u) % 32769u : 0; o[i] = 40000; }
    V32 id2(1000);
    for (uint32_t i = 0; i < 1000; i++) id2[i] = i * 2654435761u;
    CHECK(rcx_plan_hist(1000, z.data(), o.data(), 32768, id2.data(), "x", aux, nhist, err) && aux.size() == 2000);
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < 1000; i++) { CHECK(aux[i] == z[i] && aux[1000 + i] == id2[i]); cnt += z[i] != 0; }
    CHECK(cnt == nhist);
}

template <class T> static void touch(T* p, uint64_t count, const uint8_t* lo, const uint8_t* hi)
{
    if (!count) return;
    CHECK((const uint8_t*)p >= lo && (const uint8_t*)(p + count) <= hi);
    ((volatile uint8_t*)p)[0] = 1;
    ((volatile uint8_t*)(p + count))[-1] = 1;
}

static void t_slots()
{
    const uint32_t ns[] = {1, 2, 63, 64, 65, 1000, 8212};
    const uint32_t segs_per[] = {0, 1, 2, 3};
    for (uint32_t n : ns) for (uint32_t sp : segs_per) for (uint32_t hmode = 0; hmode < 3; hmode++) for (uint32_t mis = 0; mis < 256; mis += 85) {
        const uint64_t segs = (uint64_t)n * sp > 40 ? 40 : (uint64_t)n * sp;      // (the heap block below is written at its arrays' ends only)
        const uint32_t nhist = hmode == 0 ? 0 : hmode == 1 ? 1 : n;
        const uint64_t bytes = dh_hist_scratch_bytes(n, segs, nhist);
        CHECK(bytes >= dh_scratch_bytes(n, segs) + (uint64_t)nhist * 2 * DE_SEG);
        uint8_t* raw = (uint8_t*)malloc(bytes + 256);
        CHECK(raw);
        uint8_t* scratch = raw + mis;                       // the carve aligns to 256 itself
        const uint8_t* hi = scratch + bytes;
        DhScratch h; DhHist hh;
        const DeScratch d = dh_hist_carve(scratch, bytes, n, nhist, h, hh);
        CHECK(d.cap >= segs && hh.cap == nhist);
        const uint64_t cap = d.cap;
        touch(hh.hslot, n + 1, scratch, hi);
        touch(d.seg_first, n + 1, scratch, hi); touch(d.sflag, n, scratch, hi);
        touch(d.seg_off, cap, scratch, hi); touch(d.seg_bits, cap, scratch, hi); touch(d.seg_type, cap, scratch, hi);
        touch(d.seg_ioff, cap, scratch, hi); touch(d.seg_ilen, cap, scratch, hi); touch(d.seg_cks, cap, scratch, hi);
        touch(d.pos, cap * DE_SEG, scratch, hi); touch(d.stg, cap * DE_STG_BYTES, scratch, hi);
        touch(h.cand, cap * DE_SEG, scratch, hi); touch(h.elen, cap * DH_ELEN, scratch, hi); touch(h.price, cap * 320, scratch, hi);
        touch(h.link, (cap + nhist) * DE_SEG, scratch, hi);
        // the arrays do not overlap: ascending, each ends where the next begins or before
        const uint8_t* order[] = {(uint8_t*)hh.hslot, (uint8_t*)d.seg_first, (uint8_t*)d.sflag, (uint8_t*)d.seg_off, (uint8_t*)d.seg_bits,
                                  (uint8_t*)d.seg_type, (uint8_t*)d.seg_ioff, (uint8_t*)d.seg_ilen, (uint8_t*)d.seg_cks, (uint8_t*)d.pos, d.stg,
                                  (uint8_t*)h.cand, (uint8_t*)h.elen, h.price, (uint8_t*)h.link};
        const uint64_t size[] = {4ull * (n + 1), 4ull * (n + 1), 4ull * n, 8 * cap, 4 * cap, 4 * cap, 8 * cap, 8 * cap, 4 * cap, 4ull * DE_SEG * cap,
                                 (uint64_t)DE_STG_BYTES * cap, 4ull * DE_SEG * cap, 4ull * DH_ELEN * cap, 320 * cap, 2ull * DE_SEG * (cap + nhist)};
        for (int i = 0; i + 1 < 15; i++) CHECK(order[i] + size[i] <= order[i + 1]);
        // a block's virtual position 0: hist entries before its own links, never before the link array
        // (block b, first segment f0, hslot[b] slots before it: the lowest is block 0 with f0 = 0, slot 0 and 32768 bytes of history)
        if (nhist) CHECK(h.link + ((uint64_t)0 + 0 + 1) * DE_SEG - DE_WIN >= h.link);
        free(raw);
    }
    // less than the fixed part: no segments, and nothing carved past the end is ever used (cap 0)
    DhScratch h; DhHist hh;
    uint8_t small[4096];
    const DeScratch d = dh_hist_carve(small, sizeof small, 4, 2, h, hh);
    CHECK(d.cap == 0);
}

int main(int argc, char** argv)
{
    const std::string sec = argc > 1 ? argv[1] : "";
    if (sec == "args") t_args();
    else if (sec == "slots") t_slots();
    else { printf("usage: test_plan_hist args|slots\n"); return 2; }
    printf("HOST_PLAN_OK %s\n", sec.c_str());
    return 0;
}
