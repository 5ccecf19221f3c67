// Drives the chain plan of the bzip2 decoder on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_host_plan_bz2.py does):
//   test_plan_bz2 chain    rcx_plan_bz2_chain of rust_compress_amd/csrc/rcx_plan.h on hand-written candidate lists: a candidate off the
//                          chain, a gap, an overlap, a block over its stream's level, two streams of different levels, trailing bytes, a
//                          missing stream end, zero blocks, the magic, failures of a block's own
//   test_plan_bz2 rounds   the same walks fed their records a few at a time: the results and the live blocks do not depend on the rounds
// Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<rcx_bz2_cand> Cands;
typedef std::vector<rcx_bz2_rec> Recs;
typedef std::vector<uint32_t> Live;

static rcx_bz2_cand head(uint64_t byte, uint32_t level) { return {byte * 8, RCX_BZ2_HEAD, level}; }
static rcx_bz2_cand blk(uint64_t bit) { return {bit, RCX_BZ2_BLOCK, 0}; }
static rcx_bz2_cand end(uint64_t bit, uint32_t crc) { return {bit, RCX_BZ2_END, crc}; }
static rcx_bz2_rec rec(uint64_t end_bit, uint32_t nblock, uint32_t crc, int32_t status = RCX_OK) { return {status, nblock, 0, crc, end_bit}; }
static uint32_t rotl(uint32_t c) { return (c << 1) | (c >> 31); }

struct Outcome { int32_t status; uint64_t in_used; Live live; };
// `step`: the records become available `step` candidates at a time (0: all at once)
static Outcome walk(uint64_t len, const Cands& c, const Recs& r, uint32_t step = 0)
{
    CHECK(c.size() == r.size());
    rcx_bz2_chain st;
    Outcome o;
    const uint32_t n = (uint32_t)c.size();
    uint32_t avail = step ? 0 : n;
    for (int turn = 0; turn < 1000; turn++) {
        // the records beyond `avail` are poisoned: a walk that read one would fail or trip the sanitizer's eye
        Recs seen(r.begin(), r.begin() + avail);
        seen.resize(n, rec(0, 0xffffffffu, 0xdeadbeefu, 12345));
        if (rcx_plan_bz2_chain(len, c.data(), n, seen.data(), avail, st, o.live)) break;
        CHECK(avail < n);
        avail = avail + step < n ? avail + step : n;
    }
    CHECK(st.done);
    o.status = st.status; o.in_used = st.in_used;
    return o;
}

// the scenarios: (file length, candidates, records, expected status, expected in_used, expected live)
struct Case { const char* name; uint64_t len; Cands c; Recs r; int32_t status; uint64_t in_used; Live live; };
static std::vector<Case> cases()
{
    std::vector<Case> v;
    const uint32_t A = 0x11111111u, B = 0x2222u, AB = rotl(A) ^ B;
    const Recs none1(1, rec(0, 0, 0)), none2(2, rec(0, 0, 0));
    // one stream, two blocks, the second bit-unaligned; the end at bit 1001: 1001 + 80 = 1081 bits -> 136 bytes
    v.push_back({"two blocks", 136, {head(0, 9), blk(32), blk(500), end(1001, AB)}, {rec(0, 0, 0), rec(500, 900000, A), rec(1001, 7, B), rec(0, 0, 0)}, RCX_OK, 136, {1, 2}});
    // a candidate off the chain: a block mark at bit 300 inside the first block's data (its speculative decode failed -- or not: both are dropped)
    v.push_back({"off the chain", 136, {head(0, 9), blk(32), blk(300), blk(500), end(1001, AB)},
                 {rec(0, 0, 0), rec(500, 10, A), rec(9999, 5, 77, RCX_E_BZ2_DATA), rec(1001, 7, B), rec(0, 0, 0)}, RCX_OK, 136, {1, 3}});
    v.push_back({"off the chain, decoded", 136, {head(0, 9), blk(32), blk(300), end(400, 5), head(60, 3), blk(500), end(1001, AB)},
                 {rec(0, 0, 0), rec(500, 10, A), rec(480, 5, 77), rec(0, 0, 0), rec(0, 0, 0), rec(1001, 7, B), rec(0, 0, 0)}, RCX_OK, 136, {1, 5}});
    // a gap: the first block ended at bit 490, the next mark stands at 500
    v.push_back({"gap", 136, {head(0, 9), blk(32), blk(500), end(1001, AB)}, {rec(0, 0, 0), rec(490, 10, A), rec(1001, 7, B), rec(0, 0, 0)}, RCX_E_BZ2_DATA, 0, {1}});
    // an overlap: the first block ended at bit 510, behind the next mark
    v.push_back({"overlap", 136, {head(0, 9), blk(32), blk(500), end(1001, AB)}, {rec(0, 0, 0), rec(510, 10, A), rec(1001, 7, B), rec(0, 0, 0)}, RCX_E_BZ2_DATA, 0, {1}});
    // a block over its stream's level: 100 001 bytes at level 1; exactly 100 000 pass
    v.push_back({"over the level", 136, {head(0, 1), blk(32), end(500, A)}, {rec(0, 0, 0), rec(500, 100001, A), rec(0, 0, 0)}, RCX_E_BZ2_DATA, 0, {}});
    v.push_back({"at the level", 73, {head(0, 1), blk(32), end(500, A)}, {rec(0, 0, 0), rec(500, 100000, A), rec(0, 0, 0)}, RCX_OK, 73, {1}});
    // two streams with different levels: the second starts at byte 73 and its block of 300 000 bytes needs its level 3
    v.push_back({"two streams", 200, {head(0, 1), blk(32), end(500, A), head(73, 3), blk(73 * 8 + 32), end(1200, B)},
                 {rec(0, 0, 0), rec(500, 100000, A), rec(0, 0, 0), rec(0, 0, 0), rec(1200, 300000, B), rec(0, 0, 0)}, RCX_OK, 160, {1, 4}});
    v.push_back({"second stream over ITS level", 200, {head(0, 3), blk(32), end(500, A), head(73, 1), blk(73 * 8 + 32), end(1200, B)},
                 {rec(0, 0, 0), rec(500, 300000, A), rec(0, 0, 0), rec(0, 0, 0), rec(1200, 300000, B), rec(0, 0, 0)}, RCX_E_BZ2_DATA, 0, {1}});
    // trailing bytes: what follows is no header (a header a byte later does not count either)
    v.push_back({"trailing bytes", 90, {head(0, 1), blk(32), end(500, A), head(74, 9)}, {rec(0, 0, 0), rec(500, 5, A), rec(0, 0, 0), rec(0, 0, 0)}, RCX_OK, 73, {1}});
    // a header and nothing behind it; a header and a mark cut short
    v.push_back({"header then nothing", 77, {head(0, 1), blk(32), end(500, A), head(73, 9)}, {rec(0, 0, 0), rec(500, 5, A), rec(0, 0, 0), rec(0, 0, 0)}, RCX_E_EOF, 0, {1}});
    // a missing stream end: the last block ends 10 bits before the file does / well before it
    v.push_back({"missing end, file over", 64, {head(0, 1), blk(32)}, {rec(0, 0, 0), rec(502, 5, A)}, RCX_E_EOF, 0, {1}});
    v.push_back({"missing end, data instead", 640, {head(0, 1), blk(32)}, {rec(0, 0, 0), rec(502, 5, A)}, RCX_E_BZ2_DATA, 0, {1}});
    // the end mark is there but its CRC is cut off; the combined CRC is wrong
    v.push_back({"end cut off", 70, {head(0, 1), blk(32), end(500, A)}, {rec(0, 0, 0), rec(500, 5, A), rec(0, 0, 0)}, RCX_E_EOF, 0, {1}});
    v.push_back({"combined crc", 73, {head(0, 1), blk(32), end(500, A ^ 1)}, {rec(0, 0, 0), rec(500, 5, A), rec(0, 0, 0)}, RCX_E_BZ2_STREAM_CRC, 0, {1}});
    // zero blocks: the 14 bytes of an empty stream; twice
    v.push_back({"zero blocks", 14, {head(0, 9), end(32, 0)}, none2, RCX_OK, 14, {}});
    v.push_back({"zero blocks twice", 28, {head(0, 9), end(32, 0), head(14, 9), end(14 * 8 + 32, 0)}, Recs(4, rec(0, 0, 0)), RCX_OK, 28, {}});
    // the magic; files shorter than a header; no candidates at all
    v.push_back({"magic", 100, {head(1, 9), blk(40)}, none2, RCX_E_BZ2_MAGIC, 0, {}});
    v.push_back({"no candidates", 100, {}, {}, RCX_E_BZ2_MAGIC, 0, {}});
    v.push_back({"short file", 3, {}, {}, RCX_E_EOF, 0, {}});
    v.push_back({"empty file", 0, {}, {}, RCX_E_EOF, 0, {}});
    v.push_back({"header alone", 4, {head(0, 5)}, none1, RCX_E_EOF, 0, {}});
    // a block's own failure is the file's, in stream order: the second block's status wins over the bad end behind it
    v.push_back({"block failure", 136, {head(0, 9), blk(32), blk(500), end(1001, 1)}, {rec(0, 0, 0), rec(500, 10, A), rec(0, 0, 0, RCX_E_BZ2_RANDOMISED), rec(0, 0, 0)},
                 RCX_E_BZ2_RANDOMISED, 0, {1}});
    // a block that ends where it began would never let the walk advance
    v.push_back({"no progress", 136, {head(0, 9), blk(32)}, {rec(0, 0, 0), rec(32, 10, A)}, RCX_E_BZ2_DATA, 0, {}});
    return v;
}

static void t_chain(uint32_t step_lo, uint32_t step_hi)
{
    for (const Case& k : cases())
        for (uint32_t step = step_lo; step <= step_hi; step++) {
            const Outcome o = walk(k.len, k.c, k.r, step);
            if (o.status != k.status || o.in_used != k.in_used || o.live != k.live) {
                printf("FAILED case '%s' (records %u at a time): status %d (want %d), in_used %llu (want %llu), %zu live (want %zu)\n", k.name, step,
                       o.status, k.status, (unsigned long long)o.in_used, (unsigned long long)k.in_used, o.live.size(), k.live.size());
                exit(1);
            }
        }
}

int main(int argc, char** argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "chain") t_chain(0, 0);
    else if (s == "rounds") t_chain(1, 3);
    else { printf("usage: test_plan_bz2 chain|rounds\n"); return 2; }
    printf("HOST_PLAN_OK %s\n", s.c_str());
    return 0;
}
