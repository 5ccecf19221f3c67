// Drives the plan of the Zstandard decoder on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_host_plan_zstd.py does):
//   test_plan_zstd plan     rcx_plan_zstd of rust_compress_amd/csrc/rcx_plan.h: the waves and the scratch by the number of files, the
//                           dictionary words with both arrays null, with lengths of 0, with one range shared and with a dictionary
//                           longer than an LZ4 or DEFLATE window (nothing is clamped), what it refuses
//   test_plan_zstd retry    rcx_plan_zstd_retry: the files of a size query that are decoded again, with the capacities they asked for
// Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static void plan()
{
    rcx_zstd_plan p;
    std::string err;
    // no dictionaries: words that say so, a wave a file
    CHECK(rcx_plan_zstd(3, nullptr, nullptr, p, err));
    CHECK(p.waves == 3 && p.scratch_bytes == 3ull * RCX_ZSTD_LIT_SLOT && p.dict.ndict == 0 && p.dict.span == 0);
    CHECK(p.dict.aux.size() == 3 * RCX_DICT_WORDS);
    for (uint32_t i = 0; i < 3; i++) CHECK(p.dict.aux[i] == 0 && p.dict.aux[9 + i] == 0 && p.dict.aux[12 + i] == 0);
    // more files than waves: the waves are persistent
    std::vector<uint64_t> off(5000, 0), len(5000, 0);
    CHECK(rcx_plan_zstd(5000, nullptr, nullptr, p, err));
    CHECK(p.waves == RCX_ZSTD_MAX_WAVES && p.scratch_bytes == (uint64_t)RCX_ZSTD_MAX_WAVES * RCX_ZSTD_LIT_SLOT);
    // tests/test_gpu_zstd.py's 4160 files: every wave takes two, 64 of them three
    CHECK(rcx_plan_zstd(4160, nullptr, nullptr, p, err) && p.waves == 2048 && 4160 == 2 * p.waves + 64);
    // one range shared by many files, one file with none, one with a dictionary of 1 MiB beyond 4 GiB: nothing is clamped
    for (uint32_t i = 0; i < 5000; i++) { off[i] = 64; len[i] = 32768; }
    len[7] = 0; off[7] = 0xdeadbeef;
    off[9] = (5ull << 32) + 3; len[9] = 1u << 20;
    CHECK(rcx_plan_zstd(5000, off.data(), len.data(), p, err));
    CHECK(p.dict.ndict == 2 && p.dict.span == (5ull << 32) + 3 + (1u << 20));
    CHECK(p.dict.aux[0] == 32768 && p.dict.aux[3 * 5000 + 0] == 64 && p.dict.aux[4 * 5000 + 0] == 0);
    CHECK(p.dict.aux[7] == 0 && p.dict.aux[3 * 5000 + 7] == 0);
    CHECK(p.dict.aux[9] == (1u << 20) && p.dict.aux[3 * 5000 + 9] == 3 && p.dict.aux[4 * 5000 + 9] == 5);
    // refused: one array without the other, too many files, a dictionary of 4 GiB, a range that wraps
    CHECK(!rcx_plan_zstd(2, off.data(), nullptr, p, err) && err.find("together") != std::string::npos);
    CHECK(!rcx_plan_zstd(2, nullptr, len.data(), p, err));
    CHECK(!rcx_plan_zstd(RCX_ZSTD_MAX_FILES + 1, nullptr, nullptr, p, err) && err.find("65535") != std::string::npos);
    CHECK(rcx_plan_zstd(RCX_ZSTD_MAX_FILES, nullptr, nullptr, p, err) && p.waves == RCX_ZSTD_MAX_WAVES);
    uint64_t o2[2] = {0, ~0ull - 5}, l2[2] = {1ull << 32, 100};
    CHECK(!rcx_plan_zstd(1, o2, l2, p, err) && err.find("block 0") != std::string::npos);
    l2[0] = 10;
    CHECK(!rcx_plan_zstd(2, o2, l2, p, err) && err.find("block 1") != std::string::npos);
    printf("HOST_PLAN_OK plan\n");
}

static void retry()
{
    const int32_t status[6] = {RCX_OK, RCX_E_OUTPUT_TOO_SMALL, RCX_E_ZSTD_DATA, RCX_E_OUTPUT_TOO_SMALL, RCX_E_EOF, RCX_OK};
    const uint64_t out_len[6] = {10, 300000, 0, 0, 0, 0};
    const auto r = rcx_plan_zstd_retry(6, status, out_len);
    CHECK(r.size() == 2 && r[0].first == 1 && r[0].second == 300000 && r[1].first == 3 && r[1].second == 0);
    CHECK(rcx_plan_zstd_retry(0, status, out_len).empty());
    printf("HOST_PLAN_OK retry\n");
}

int main(int argc, char** argv)
{
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "plan") plan();
    else if (which == "retry") retry();
    else { printf("usage: test_plan_zstd plan|retry\n"); return 2; }
    return 0;
}
