// Drives the planning arithmetic of dictionary training on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_host_plan_train.py does):
//   test_plan_train epochs   rcx_train_epoch_plan at the edge sizes (n = 0, n < k, n = k, the 10 k branch, a remainder), dead jobs, the
//                            round bound, and the words rcx_plan_train hands to the kernels
//   test_plan_train refuse   every refusal of rcx_plan_train and the job its text names
//   test_plan_train carve    every array of every job's region and the head in front of them lies inside a heap block of exactly
//                            plan.scratch_bytes (its first and last byte are written), the regions do not overlap, and
//                            rcx_plan_train_scratch with every job at the largest sizes is no smaller
// rcx_plan.h alone: plain C++, no kernel.  Prints HOST_PLAN_OK <section>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<uint64_t> V64;
typedef std::vector<uint32_t> V32;

static void t_epochs()
{
    rcx_train_epochs e = rcx_train_epoch_plan(0, 32768, 256);
    CHECK(e.E == 1 && e.size == 0);
    e = rcx_train_epoch_plan(100, 32768, 256);                     // n < 10 k: one epoch of n
    CHECK(e.E == 1 && e.size == 100);
    e = rcx_train_epoch_plan(256, 32768, 256);
    CHECK(e.E == 1 && e.size == 256);
    e = rcx_train_epoch_plan(524288, 32768, 256);                  // C / k / 4 = 32 epochs of 16384
    CHECK(e.E == 32 && e.size == 16384);
    e = rcx_train_epoch_plan(524288 + 31, 32768, 256);             // a remainder of 31 positions that are never starts
    CHECK(e.E == 32 && e.size == 16384);
    e = rcx_train_epoch_plan(65536, 32768, 64);                    // 128 epochs of 512 < 640: epochs of 640, 102 of them, 256 left over
    CHECK(e.E == 102 && e.size == 640);
    e = rcx_train_epoch_plan(420, 1024, 16);
    CHECK(e.E == 2 && e.size == 160);
    e = rcx_train_epoch_plan(0xffffffffull, 100, 4096);            // the largest corpus in one epoch
    CHECK(e.E == 1 && e.size == 0xffffffffull);
    e = rcx_train_epoch_plan(0xffffffffull, 0xffffffffull, 6);
    CHECK(e.E * e.size <= 0xffffffffull && e.size >= 60);
    CHECK(rcx_train_dead(255, 1000, 256, 8) && !rcx_train_dead(256, 1000, 256, 8) && rcx_train_dead(1000, 7, 256, 8) &&
          !rcx_train_dead(1000, 8, 256, 8) && rcx_train_dead(0, 0, 6, 6));
    CHECK(rcx_train_round_bound(32768, 8) == (4096 + 2) * 11 && rcx_train_round_bound(0, 6) == 22);

    // three jobs: a live one of three samples (one empty), an n = 0 job without samples, a live one
    V64 in_len = {3000, 0, 700}, cap = {1024, 512, 64}, sl = {1000, 0, 2000, 700};
    V32 ns = {3, 0, 1};
    rcx_train_plan p; std::string err;
    CHECK(rcx_plan_train(3, in_len.data(), cap.data(), ns.data(), sl.data(), 64, 8, 12, p, err));
    CHECK(p.aux_words == (3 * 9 + 4 + 2) / 3 && p.aux.size() == (size_t)p.aux_words * 3 && p.live == 2);
    CHECK(p.max_n == 3000 && p.max_cap == 1024 && p.max_rounds == rcx_train_round_bound(1024, 8));
    const uint32_t* h = p.aux.data() + 3;
    CHECK(h[0] == 0 && h[1] == 3 && h[6] == 0 && h[8 + 0] == 3 && h[8 + 1] == 0 && h[8 + 6] == 1 && h[16 + 0] == 3 && h[16 + 1] == 1 && h[16 + 6] == 0);
    const uint32_t* ends = p.aux.data() + 27;
    CHECK(ends[0] == 1000 && ends[1] == 1000 && ends[2] == 3000 && ends[3] == 700);
    CHECK(h[2] == rcx_train_epoch_plan(3000, 1024, 64).E && h[3] == rcx_train_epoch_plan(3000, 1024, 64).size);
    // no job at all, and null arrays with it
    CHECK(rcx_plan_train(0, nullptr, nullptr, nullptr, nullptr, 256, 8, 20, p, err) && p.aux.empty() && p.live == 0 && p.max_rounds == 0);
    printf("HOST_PLAN_OK epochs\n");
}

static void t_refuse()
{
    V64 in_len = {100, 200}, cap = {64, 64}, sl = {60, 40, 200};
    V32 ns = {2, 1};
    rcx_train_plan p; std::string err;
    CHECK(rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 16, 8, 20, p, err));
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 16, 7, 20, p, err) && err.find("d must be") != std::string::npos);
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 7, 8, 20, p, err) && err.find("k must be") != std::string::npos);
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 4097, 8, 20, p, err));
    CHECK(rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 4096, 6, 10, p, err));
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 16, 8, 9, p, err) && err.find("f must be") != std::string::npos);
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 16, 8, 23, p, err));
    CHECK(rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), sl.data(), 16, 8, 22, p, err));
    CHECK(!rcx_plan_train(2, nullptr, cap.data(), ns.data(), sl.data(), 16, 8, 20, p, err) && !rcx_plan_train(2, in_len.data(), nullptr, ns.data(), sl.data(), 16, 8, 20, p, err) &&
          !rcx_plan_train(2, in_len.data(), cap.data(), nullptr, sl.data(), 16, 8, 20, p, err) && !rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), nullptr, 16, 8, 20, p, err));
    V64 bad = {60, 40, 199};
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), bad.data(), 16, 8, 20, p, err) && err.find("job 1") != std::string::npos);
    bad = {60, 41, 200};
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), bad.data(), 16, 8, 20, p, err) && err.find("job 0") != std::string::npos);
    bad = {60, ~0ull, 200};                                        // (a sum that would wrap)
    CHECK(!rcx_plan_train(2, in_len.data(), cap.data(), ns.data(), bad.data(), 16, 8, 20, p, err) && err.find("job 0") != std::string::npos);
    V64 huge = {100, 1ull << 32}, hs = {60, 40, 1ull << 32};       // arithmetic only: no buffer of that size
    CHECK(!rcx_plan_train(2, huge.data(), cap.data(), ns.data(), hs.data(), 16, 8, 20, p, err) && err.find("job 1") != std::string::npos);
    V64 hcap = {64, 1ull << 32};
    CHECK(!rcx_plan_train(2, in_len.data(), hcap.data(), ns.data(), sl.data(), 16, 8, 20, p, err) && err.find("job 1") != std::string::npos);
    V64 top = {100, 0xffffffffull}, ts = {60, 40, 0xffffffffull};  // the largest corpus there is plans (nothing is allocated here)
    CHECK(rcx_plan_train(2, top.data(), cap.data(), ns.data(), ts.data(), 16, 8, 20, p, err) && p.max_n == 0xffffffffull);
    printf("HOST_PLAN_OK refuse\n");
}

static void t_carve()
{
    uint32_t seed = 12345;
    auto rnd = [&](uint32_t m) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % m; };
    for (int it = 0; it < 200; it++) {
        const uint32_t n = 1 + rnd(it < 150 ? 6 : 300), k = 6 + rnd(it % 3 ? 300 : 4091), d = rnd(2) ? 6 : 8, f = 10 + rnd(it % 5 ? 3 : 13);
        if (k < d) continue;
        V64 in_len(n), cap(n), sl(n);
        V32 ns(n, 1);
        uint64_t max_n = 0, max_c = 0;
        for (uint32_t i = 0; i < n; i++) {
            in_len[i] = rnd(8) ? rnd(40000) : 0; cap[i] = rnd(6) ? rnd(9000) : rnd(8); sl[i] = in_len[i];
            max_n = std::max(max_n, in_len[i]); max_c = std::max(max_c, cap[i]);
        }
        rcx_train_plan p; std::string err;
        CHECK(rcx_plan_train(n, in_len.data(), cap.data(), ns.data(), sl.data(), k, d, f, p, err));
        CHECK(p.scratch_bytes <= rcx_plan_train_scratch(n, max_n, max_c, k, f));
        uint8_t* raw = (uint8_t*)malloc(p.scratch_bytes + 256);
        CHECK(raw);
        for (int shift = 0; shift < 256; shift += 85) {            // the caller's pointer at four alignments; the kernels align it up
            uint8_t* ptr = raw + shift;                            // plan.scratch_bytes from here are the call's
            uint8_t* base = (uint8_t*)(((uintptr_t)ptr + 255) & ~(uintptr_t)255);
            const uint64_t room = p.scratch_bytes - (uint64_t)(base - ptr);
            auto touch = [&](uint64_t at, uint64_t bytes) { if (bytes) { CHECK(at + bytes <= room); base[at] = 1; base[at + bytes - 1] = 1; } };
            touch(0, 256);
            touch(rcx_train_state_at(n), (uint64_t)n * RCX_TRAIN_STATE_WORDS * 4);
            touch(rcx_train_partial_at(n), (uint64_t)n * RCX_TRAIN_SCAN_BLOCKS * 4);
            CHECK(rcx_train_state_at(n) >= 256 && rcx_train_partial_at(n) >= rcx_train_state_at(n) + (uint64_t)n * RCX_TRAIN_STATE_WORDS * 4);
            uint64_t prev_end = rcx_train_head_bytes(n);
            CHECK(prev_end >= rcx_train_partial_at(n) + (uint64_t)n * RCX_TRAIN_SCAN_BLOCKS * 4);
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t* h = p.aux.data() + n + RCX_TRAIN_HDR * i;
                CHECK((h[6] != 0) == rcx_train_dead(in_len[i], cap[i], k, d));
                if (h[6]) continue;
                const uint64_t at = h[4] | ((uint64_t)h[5] << 32);
                CHECK(at == prev_end && at % 256 == 0);
                const rcx_train_carve c = rcx_train_job_carve(in_len[i], cap[i], h[3], f);
                CHECK(c.hash == 0 && c.back >= 4 * in_len[i] && c.freq >= c.back + 2 * in_len[i] && c.diff >= c.freq + ((uint64_t)4 << f) &&
                      c.stage >= c.diff + 4 * ((uint64_t)h[3] + 1) && c.end >= c.stage + cap[i]);
                touch(at + c.hash, 4 * in_len[i]); touch(at + c.back, 2 * in_len[i]); touch(at + c.freq, (uint64_t)4 << f);
                touch(at + c.diff, 4 * ((uint64_t)h[3] + 1)); touch(at + c.stage, cap[i]);
                prev_end = at + c.end;
            }
            CHECK(prev_end + 256 == p.scratch_bytes);
        }
        free(raw);
    }
    CHECK(rcx_plan_train_scratch(1, 1000, 100, 5, 20) == 0 && rcx_plan_train_scratch(1, 1000, 100, 64, 9) == 0);
    CHECK(rcx_plan_train_scratch(256, 1 << 20, 32768, 256, 20) >= 256ull * ((10ull << 20) + (4ull << 20) + 32768));
    printf("HOST_PLAN_OK carve\n");
}

int main(int argc, char** argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "epochs") t_epochs();
    else if (s == "refuse") t_refuse();
    else if (s == "carve") t_carve();
    else { printf("usage: test_plan_train epochs|refuse|carve\n"); return 2; }
    return 0;
}
