// Drives the host plan of the bzip2 ENCODER on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_host_plan_bz2_enc.py does):
//   test_plan_bz2_enc chunks   rcx_plan_bz2e_chunks / _step / _less / _cut of rust_compress_amd/csrc/rcx_plan.h at the boundaries: len = C,
//                              C + 1, 2C, empty files between others, a form over C by one byte, a last chunk of one byte, a file of 4 GiB
//   test_plan_bz2_enc layout   rcx_plan_bz2e_layout: bit offsets and padding, the combined CRC against known values, the capacity check,
//                              the bound of a block's bits
//   test_plan_bz2_enc rounds   rcx_plan_bz2e_rounds: rounds of 1, 2 and 3 blocks cover the same blocks once, and the layout does not know them
// Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<rcx_bz2e_block> Blocks;

static bool is(const rcx_bz2e_block& b, uint32_t file, uint64_t off, uint32_t len)
{
    return b.file == file && b.off == off && b.len == len && b.n == 0;
}

static void chunks()
{
    const uint32_t C = 1000;
    std::string err;
    Blocks ch, bl;
    // the measuring pieces: C input bytes each, the last one shorter, none for an empty file
    const uint64_t lens[] = {0, 1000, 1001, 2000, 0, 999, 1};
    CHECK(rcx_plan_bz2e_chunks(7, lens, C, ch, err));
    CHECK(ch.size() == 7);                                                  // 0 + 1 + 2 + 2 + 0 + 1 + 1
    CHECK(is(ch[0], 1, 0, 1000));
    CHECK(is(ch[1], 2, 0, 1000) && is(ch[2], 2, 1000, 1));
    CHECK(is(ch[3], 3, 0, 1000) && is(ch[4], 3, 1000, 1000));
    CHECK(is(ch[5], 5, 0, 999) && is(ch[6], 6, 0, 1));
    // the chunk a file starts with: q = floor(C L / R), less a 64th; never more than the file, never less than a byte
    CHECK(rcx_plan_bz2e_step(2000, 2000, C) == 985 && rcx_plan_bz2e_step(1, 1, C) == 1 && rcx_plan_bz2e_step(985, 985, C) == 985);
    CHECK(rcx_plan_bz2e_step(2000, 2400, C) == 820);                        // five bytes become six: 833 - 13
    CHECK(rcx_plan_bz2e_step(120000, 144000, 99981) == 82016);              // 83317 - 1301
    CHECK(rcx_plan_bz2e_step(5000, 100, C) == 5000);                        // long runs: the whole file
    CHECK(rcx_plan_bz2e_step(4294967295ull, 4294967295ull, 899981) == 885919);
    CHECK(rcx_plan_bz2e_step(4294967295ull, 100000ull, 899981) == (1ull << 30) && rcx_plan_bz2e_step(1ull << 29, 1000, 899981) == (1ull << 29));
    CHECK(rcx_plan_bz2e_step(3, 4, 1) == 1);
    // ... and the next one: smaller by a byte at least, in proportion otherwise, a byte at the least
    CHECK(rcx_plan_bz2e_less(993, 1001, C, 0) == 977);                      // over by one byte: 992 - 15
    CHECK(rcx_plan_bz2e_less(985, 1231, C, 3) == 788);                      // 800 - 12
    CHECK(rcx_plan_bz2e_less(2, 3, 2, 0) == 1 && rcx_plan_bz2e_less(1, 5, 4, 0) == 1 && rcx_plan_bz2e_less(1, 5, 4, 9) == 1);
    CHECK(rcx_plan_bz2e_less(4294967295ull, 899982, 899981, 0) < 4294967295ull);
    // from the fifth shortening on s is halved at least: a form barely over C no longer costs a 64th a turn
    CHECK(rcx_plan_bz2e_less(993, 1001, C, 4) == 496 && rcx_plan_bz2e_less(985, 2500, C, 4) == 388);
    // the bound: from 2^30, forms that are over C by a byte every time, RCX_BZ2E_TURNS probes reach a chunk of one byte
    {
        uint64_t st = RCX_BZ2E_MAX_CHUNK;
        uint32_t turn = 0;
        while (st > 1) { st = rcx_plan_bz2e_less(st, 899982, 899981, turn); turn++; }
        CHECK(turn + 1 <= RCX_BZ2E_TURNS && turn == 33);                       // (34 in theory: four turns of a 64th are worth one halving here)
    }
    // the cut: chunks of s bytes, the last one shorter; they tile the file
    rcx_plan_bz2e_cut(3, 2000, 820, bl);
    CHECK(bl.size() == 3 && is(bl[0], 3, 0, 820) && is(bl[1], 3, 820, 820) && is(bl[2], 3, 1640, 360));
    rcx_plan_bz2e_cut(5, 1971, 985, bl);                                    // (appends; a last chunk of one byte)
    CHECK(bl.size() == 6 && is(bl[3], 5, 0, 985) && is(bl[4], 5, 985, 985) && is(bl[5], 5, 1970, 1));
    bl.clear();
    rcx_plan_bz2e_cut(0, 1970, 985, bl);
    CHECK(bl.size() == 2 && is(bl[1], 0, 985, 985));
    for (uint64_t L : {1ull, 2ull, 999ull, 1000ull, 1001ull, 4294967295ull}) {
        for (uint64_t st : {1ull, 7ull, 985ull, 4294967295ull}) {
            if (L / st > 5000) continue;
            bl.clear();
            rcx_plan_bz2e_cut(9, L, st, bl);
            uint64_t at = 0;
            for (const auto& b : bl) { CHECK(b.off == at && b.len > 0 && b.len <= st); at += b.len; }
            CHECK(bl.size() == (L + st - 1) / st && at == L);
        }
    }
    // the real block size; 4 GiB is refused and names its file
    const uint64_t big[] = {899981ull * 2 + 5};
    CHECK(rcx_plan_bz2e_chunks(1, big, 899981, ch, err) && ch.size() == 3 && ch[2].len == 5 && ch[2].off == 2 * 899981ull);
    const uint64_t huge[] = {5, 1ull << 32};
    CHECK(!rcx_plan_bz2e_chunks(2, huge, 899981, ch, err) && err.find("block 1") != std::string::npos);
    const uint64_t none[] = {0, 0};
    CHECK(rcx_plan_bz2e_chunks(2, none, C, ch, err) && ch.empty());
    printf("HOST_PLAN_OK chunks\n");
}

static Blocks three_files()
{
    // file 0: blocks 0, 1, 2; file 1: none; file 2: block 3
    Blocks bl;
    bl.push_back(rcx_bz2e_block{0, 10, 0, 10, 0});
    bl.push_back(rcx_bz2e_block{0, 10, 10, 10, 0});
    bl.push_back(rcx_bz2e_block{0, 3, 20, 3, 0});
    bl.push_back(rcx_bz2e_block{2, 7, 0, 7, 0});
    return bl;
}

static void layout()
{
    const Blocks bl = three_files();
    const uint64_t bits[] = {181, 200, 163, 184};
    const uint32_t crc[] = {0x12345678u, 0x9abcdef0u, 0xffffffffu, 0xdeadbeefu};
    std::vector<uint64_t> off;
    std::vector<rcx_bz2e_file> files;
    // file 0: 32 + 544 + 80 = 656 bits = 82 bytes exactly; file 1: 112 bits = 14 bytes; file 2: 32 + 184 + 80 = 296 bits = 37 bytes
    const uint64_t cap[] = {82, 14, 37};
    rcx_plan_bz2e_layout(3, bl, bits, crc, cap, off, files);
    CHECK(off.size() == 4 && off[0] == 32 && off[1] == 32 + 181 && off[2] == 32 + 381 && off[3] == 32);
    CHECK(files[0].first == 0 && files[0].count == 3 && files[0].bits == 656 && files[0].out_len == 82 && files[0].status == RCX_OK);
    CHECK(files[1].first == 3 && files[1].count == 0 && files[1].bits == 112 && files[1].out_len == 14 && files[1].status == RCX_OK);
    CHECK(files[2].first == 3 && files[2].count == 1 && files[2].bits == 296 && files[2].out_len == 37 && files[2].status == RCX_OK);
    // the combined CRC: c = rotl(c, 1) ^ crc, against values worked out by hand
    CHECK(files[0].crc == 0x82571bfeu && files[1].crc == 0 && files[2].crc == 0xdeadbeefu);
    {
        Blocks two(bl.begin(), bl.begin() + 2);
        rcx_plan_bz2e_layout(1, two, bits, crc, cap, off, files);
        CHECK(files[0].crc == 0xbed47200u);
        const uint32_t edge[] = {0x80000000u, 0x00000001u};
        rcx_plan_bz2e_layout(1, two, bits, edge, cap, off, files);
        CHECK(files[0].crc == 0);
        Blocks five;
        const uint32_t same[] = {0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu};
        const uint64_t b5[] = {100, 100, 100, 100, 100};
        for (uint32_t i = 0; i < 5; i++) five.push_back(rcx_bz2e_block{0, 1, i, 1, 0});
        rcx_plan_bz2e_layout(1, five, b5, same, cap, off, files);
        CHECK(files[0].crc == 0x06f6210cu && off[4] == 432);
    }
    // padding: one bit more is one byte more
    const uint64_t bits1[] = {181, 200, 164, 184};
    rcx_plan_bz2e_layout(3, bl, bits1, crc, cap, off, files);
    CHECK(files[0].bits == 657 && files[0].out_len == 83 && files[0].status == RCX_E_OUTPUT_TOO_SMALL && files[2].status == RCX_OK);
    // capacities: exact, one less, zero -- the size is reported either way, and a file's status is its own
    const uint64_t cap2[] = {81, 0, 36};
    rcx_plan_bz2e_layout(3, bl, bits, crc, cap2, off, files);
    CHECK(files[0].status == RCX_E_OUTPUT_TOO_SMALL && files[0].out_len == 82);
    CHECK(files[1].status == RCX_E_OUTPUT_TOO_SMALL && files[1].out_len == 14);
    CHECK(files[2].status == RCX_E_OUTPUT_TOO_SMALL && files[2].out_len == 37);
    const uint64_t cap3[] = {1000, 13, 37};
    rcx_plan_bz2e_layout(3, bl, bits, crc, cap3, off, files);
    CHECK(files[0].status == RCX_OK && files[1].status == RCX_E_OUTPUT_TOO_SMALL && files[2].status == RCX_OK);
    // the bound of a block's bits: above 17 bits a symbol and the tables, a multiple of 4, with slack for a word behind the last
    for (uint32_t n : {1u, 50u, 12000u, 899981u}) {
        const uint64_t b = rcx_plan_bz2e_block_bound(n);
        CHECK(b % 4 == 0 && b * 8 >= 17ull * (n + 1) + 6ull * ((n + 50) / 50) + 51114 + 395 + 64);
        CHECK(b <= (uint64_t)n * 22 / 10 + 8000);
    }
    printf("HOST_PLAN_OK layout\n");
}

static void rounds()
{
    std::vector<uint32_t> cuts;
    for (uint32_t nb : {0u, 1u, 2u, 3u, 7u, 64u, 65u}) {
        for (uint32_t per : {1u, 2u, 3u, 64u, 1000u}) {
            rcx_plan_bz2e_rounds(nb, per, cuts);
            CHECK(cuts.size() == (nb + per - 1) / per + 1 && cuts.front() == 0 && cuts.back() == nb);
            for (size_t r = 0; r + 1 < cuts.size(); r++) CHECK(cuts[r + 1] > cuts[r] && cuts[r + 1] - cuts[r] <= per);
        }
    }
    rcx_plan_bz2e_rounds(5, 0, cuts);                                       // (0 is taken as 1)
    CHECK(cuts.size() == 6);
    // the records of the blocks arrive round by round; the layout sees the same arrays whatever the rounds were
    const Blocks bl = three_files();
    const uint64_t bits[] = {181, 200, 163, 184};
    const uint32_t crc[] = {0x12345678u, 0x9abcdef0u, 0xffffffffu, 0xdeadbeefu};
    const uint64_t cap[] = {82, 14, 37};
    std::vector<uint64_t> off0, off;
    std::vector<rcx_bz2e_file> f0, f;
    rcx_plan_bz2e_layout(3, bl, bits, crc, cap, off0, f0);
    for (uint32_t per : {1u, 2u, 3u}) {
        std::vector<uint64_t> got_bits(4, ~0ull);
        std::vector<uint32_t> got_crc(4, 0x55555555u);
        rcx_plan_bz2e_rounds(4, per, cuts);
        for (size_t r = 0; r + 1 < cuts.size(); r++)
            for (uint32_t b = cuts[r]; b < cuts[r + 1]; b++) { got_bits[b] = bits[b]; got_crc[b] = crc[b]; }
        rcx_plan_bz2e_layout(3, bl, got_bits.data(), got_crc.data(), cap, off, f);
        CHECK(off == off0 && f.size() == f0.size());
        for (size_t i = 0; i < f.size(); i++) CHECK(f[i].out_len == f0[i].out_len && f[i].crc == f0[i].crc && f[i].status == f0[i].status && f[i].first == f0[i].first);
    }
    printf("HOST_PLAN_OK rounds\n");
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "chunks") chunks();
    else if (what == "layout") layout();
    else if (what == "rounds") rounds();
    else { printf("usage: test_plan_bz2_enc chunks|layout|rounds\n"); return 2; }
    return 0;
}
