// Drives the planning arithmetic of the decoders behind shared dictionaries on the CPU, as a program of its own so that it can be built
// with -fsanitize=address,undefined (tests/test_host_plan_slots.py does):
//   test_plan_slots copies   rcx_plan_slot_copies of rust_compress_amd/csrc/rcx_plan.h: what travels back to a host-memory batch -- the
//                            bytes the blocks produced and no byte between the slots
//   test_plan_slots words    the words of rcx_plan_dict the decoders read (k_lz4_dict.hip, k_inflate_dict.hip): the clamped length, the
//                            offset, the DICTID; the span that travels in
//   test_plan_slots dense    rcx_plan_out_dense: the layouts whose used span may travel back in one copy, because every byte of it lies
//                            in a slot
// Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<uint64_t> V64;
typedef std::vector<std::pair<uint64_t, uint64_t>> Ranges;

static void t_copies()
{
    // contiguous full slots: one range; the workload of benchmarks/dict_decode_rate.py
    { V64 off, cap, len; for (uint64_t i = 0; i < 1000; i++) { off.push_back(2048 * i); cap.push_back(2048); len.push_back(2048); }
      const Ranges r = rcx_plan_slot_copies(1000, off.data(), cap.data(), len.data());
      CHECK(r.size() == 1 && r[0].first == 0 && r[0].second == 2048 * 1000); }
    // gaps, a failed block (length 0), a short block, a length beyond the capacity (never copied beyond the slot)
    { V64 off = {5, 105, 205, 300, 400, 1ull << 40}, cap = {100, 100, 95, 100, 50, 7}, len = {100, 0, 95, 40, 60, 7};
      const Ranges r = rcx_plan_slot_copies(6, off.data(), cap.data(), len.data());
      CHECK(r.size() == 4);
      CHECK(r[0].first == 5 && r[0].second == 105);
      CHECK(r[1].first == 205 && r[1].second == 340);              // 205..300 touches 300..340
      CHECK(r[2].first == 400 && r[2].second == 450);
      CHECK(r[3].first == 1ull << 40 && r[3].second == (1ull << 40) + 7); }
    // a short block does not merge with the next slot: the bytes between its end and the next slot are the caller's
    { V64 off = {0, 100}, cap = {100, 100}, len = {99, 100};
      const Ranges r = rcx_plan_slot_copies(2, off.data(), cap.data(), len.data());
      CHECK(r.size() == 2 && r[0].second == 99 && r[1].first == 100 && r[1].second == 200); }
    // any order of the slots; nothing produced; no blocks
    { V64 off = {200, 100, 0}, cap = {100, 100, 100}, len = {100, 100, 100};
      CHECK(rcx_plan_slot_copies(3, off.data(), cap.data(), len.data()).size() == 3);
      V64 none = {0, 0, 0};
      CHECK(rcx_plan_slot_copies(3, off.data(), cap.data(), none.data()).empty());
      CHECK(rcx_plan_slot_copies(0, nullptr, nullptr, nullptr).empty()); }
    // every byte a block produced is covered exactly once, no other byte is (random layouts, checked on a map of the buffer)
    uint32_t seed = 12345;
    auto rnd = [&](uint32_t m) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % m; };
    for (int it = 0; it < 200; it++) {
        const uint32_t n = 1 + rnd(40);
        V64 off(n), cap(n), len(n);
        uint64_t at = rnd(4);
        for (uint32_t i = 0; i < n; i++) { at += rnd(3) ? 0 : rnd(5); off[i] = at; cap[i] = rnd(30); len[i] = rnd(4) ? cap[i] : rnd(40); at += cap[i]; }
        std::vector<uint8_t> want(at + 64, 0), got(at + 64, 0);
        for (uint32_t i = 0; i < n; i++) for (uint64_t k = 0; k < (len[i] < cap[i] ? len[i] : cap[i]); k++) want[off[i] + k]++;
        for (const auto& r : rcx_plan_slot_copies(n, off.data(), cap.data(), len.data())) { CHECK(r.second > r.first && r.second <= at); for (uint64_t k = r.first; k < r.second; k++) got[k]++; }
        CHECK(want == got);
    }
}

static void t_words()
{
    rcx_dict_plan p; std::string err;
    // LZ4: 65536 bytes count as their last 65535; the offset moves with the clamp; a length of 0 leaves the words 0 whatever the offset
    V64 off = {10, (1ull << 33) + 7, 1ull << 60}, len = {65536, 300, 0};
    CHECK(rcx_plan_dict(3, off.data(), len.data(), 65536, 65535, nullptr, "lz4 decode", p, err));
    const size_t N = 3;
    CHECK(p.aux[0] == 65535 && p.aux[3 * N] == 11 && p.aux[4 * N] == 0);
    CHECK(p.aux[1] == 300 && p.aux[3 * N + 1] == 7 && p.aux[4 * N + 1] == 2);
    CHECK(p.aux[2] == 0 && p.aux[3 * N + 2] == 0 && p.aux[4 * N + 2] == 0);
    CHECK(p.span == (1ull << 33) + 7 + 300);                                   // what travels in covers the highest dictionary byte
    // DEFLATE: all 32768 within reach, the DICTIDs behind the lengths; one byte more is refused by the block's number
    std::vector<uint32_t> ids = {0xAABBCCDDu, 5, 6};
    len = {32768, 300, 0};
    CHECK(rcx_plan_dict(3, off.data(), len.data(), 32768, 32768, ids.data(), "inflate", p, err));
    CHECK(p.aux[0] == 32768 && p.aux[3 * N] == 10 && p.aux[N] == 0xAABBCCDDu && p.aux[N + 2] == 6);
    len[1] = 32769;
    CHECK(!rcx_plan_dict(3, off.data(), len.data(), 32768, 32768, ids.data(), "inflate", p, err) && err.find("inflate: block 1:") == 0 && err.find("32768") != std::string::npos);
    len = {0, 0, 65537};
    CHECK(!rcx_plan_dict(3, off.data(), len.data(), 65536, 65535, nullptr, "lz4 decode", p, err) && err.find("lz4 decode: block 2:") == 0);
}

static void t_dense()
{
    // fixed power-of-two slots in index order (bench.py, benchmarks/host_path_rate.py): dense
    { V64 off, cap; for (uint64_t i = 0; i < 4096; i++) { off.push_back(65536 * i); cap.push_back(65536); }
      CHECK(rcx_plan_out_dense(4096, off.data(), cap.data(), 65536 * 4096ull));
      std::reverse(off.begin(), off.end());                                       // any order of the same slots
      CHECK(rcx_plan_out_dense(4096, off.data(), cap.data(), 65536 * 4096ull));
      off[7] += 1;                                                                // one byte of a gap (and one of overlap)
      CHECK(!rcx_plan_out_dense(4096, off.data(), cap.data(), 65536 * 4096ull)); }
    // a slot that does not start at 0; slots padded to 16; empty slots between full ones; no blocks; one empty block
    { V64 off = {1}, cap = {10}; CHECK(!rcx_plan_out_dense(1, off.data(), cap.data(), 11)); }
    { V64 off = {0, 16}, cap = {10, 10}; CHECK(!rcx_plan_out_dense(2, off.data(), cap.data(), 26)); }
    { V64 off = {0, 999, 10, 3}, cap = {10, 0, 10, 0}; CHECK(rcx_plan_out_dense(4, off.data(), cap.data(), 20)); }
    { CHECK(rcx_plan_out_dense(0, nullptr, nullptr, 0)); V64 off = {5}, cap = {0}; CHECK(rcx_plan_out_dense(1, off.data(), cap.data(), 5) == false); }
    // a gap in index order that a later slot fills
    { V64 off = {0, 20, 10}, cap = {10, 10, 10}; CHECK(rcx_plan_out_dense(3, off.data(), cap.data(), 30)); }
    // random layouts against a map of the buffer: dense exactly when no byte of [0, out_span) is outside every slot
    uint32_t seed = 777;
    auto rnd = [&](uint32_t m) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % m; };
    int ndense = 0;
    for (int it = 0; it < 2000; it++) {
        const uint32_t n = 1 + rnd(12);
        V64 off(n), cap(n);
        uint64_t at = rnd(3) ? 0 : rnd(3);
        for (uint32_t i = 0; i < n; i++) {
            if (!rnd(4)) at += rnd(3);                                            // sometimes a gap
            else if (!rnd(6) && at) at -= 1;                                      // sometimes an overlap
            off[i] = at; cap[i] = rnd(5) ? 1 + rnd(20) : 0; at += cap[i];
        }
        for (uint32_t i = n - 1; i > 0; i--) if (it & 1) { const uint32_t j = rnd(i + 1); std::swap(off[i], off[j]); std::swap(cap[i], cap[j]); }
        rcx_spans sp; std::string err;
        CHECK(rcx_plan_spans(n, off.data(), cap.data(), off.data(), cap.data(), sp, err));
        std::vector<uint8_t> in_slot(sp.out_span + 1, 0);
        for (uint32_t i = 0; i < n; i++) for (uint64_t k = 0; k < cap[i]; k++) in_slot[off[i] + k] = 1;
        bool want = true;
        for (uint64_t k = 0; k < sp.out_span; k++) want = want && in_slot[k];
        CHECK(rcx_plan_out_dense(n, off.data(), cap.data(), sp.out_span) == want);
        ndense += want;
    }
    CHECK(ndense > 100 && ndense < 1900);
}

int main(int argc, char** argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "copies") t_copies();
    else if (s == "words") t_words();
    else if (s == "dense") t_dense();
    else { printf("usage: test_plan_slots copies|words|dense\n"); return 2; }
    printf("HOST_PLAN_OK %s\n", s.c_str());
    return 0;
}
