// dict_train_ref.cpp -- the serial reference of dictionary training (TEST INFRASTRUCTURE), written from the specification of DESIGN.md
// 3.19 BY DEFINITION: the frequencies are counted position by position, the score of a start is summed over its segment with a stamp
// per hash for distinctness, and every round scores every start of its epoch afresh: O(n k) a round.  It shares nothing with the
// kernels (rust_compress_amd/csrc/k_dict_train.hip) or the host's plan (rcx_plan.h): no range-add, no array of previous occurrences.
// Built by tests/dict_train_cases.py with g++ as a shared library.
#include <stdint.h>
#include <string.h>
#include <vector>

static const uint32_t PASSES = 4, ZERO_RUNS = 10;

// S[0..n): the corpus, the concatenation of m samples of lengths len[0..m); dict: C bytes.  Returns out_len, the dictionary in
// dict[0..out_len); -1: arguments the specification does not allow.  rounds (or null): the rounds that ran.
extern "C" int64_t ref_dict_train(const uint8_t* S, uint64_t n, const uint64_t* len, uint32_t m, uint32_t k, uint32_t d, uint32_t f,
                                  uint8_t* dict, uint64_t C, uint64_t* rounds)
{
    if ((d != 6 && d != 8) || k < d || k > 4096 || f < 10 || f > 22 || n >> 32) return -1;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < m; i++) sum += len[i];
    if (sum != n) return -1;
    // validity and hashes
    std::vector<uint8_t> valid(n, 0);
    std::vector<uint32_t> h(n, 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < m; i++) {
        for (uint64_t p = at; p + d <= at + len[i]; p++) {
            uint64_t v = 0;
            for (uint32_t b = 0; b < d; b++) v |= (uint64_t)S[p + b] << (8 * b);
            valid[p] = 1;
            h[p] = (uint32_t)((v * 0x9E3779B185EBCA87ull) >> (64 - f));
        }
        at += len[i];
    }
    std::vector<uint32_t> freq((size_t)1 << f, 0);
    for (uint64_t p = 0; p < n; p++) if (valid[p]) freq[h[p]]++;
    // epochs
    uint64_t E = C / k / PASSES;
    if (E < 1) E = 1;
    uint64_t size = n / E;
    if (size < (uint64_t)10 * k) {
        size = (uint64_t)10 * k < n ? (uint64_t)10 * k : n;
        E = size ? n / size : 1;
        if (E < 1) E = 1;
    }
    std::vector<uint64_t> stamp((size_t)1 << f, 0);
    std::vector<uint8_t> buf(C, 0);
    uint64_t tail = C, zero = 0, tick = 0, r = 0;
    for (; tail > 0; r++) {
        const uint64_t e = r % E, lo = e * size;
        uint64_t hi = (e + 1) * size;
        if (n < k) hi = lo;
        else if (hi > n - k + 1) hi = n - k + 1;
        uint64_t best = 0, best_s = 0;
        bool any = false;
        for (uint64_t s = lo; s < hi; s++) {
            uint64_t score = 0;
            tick++;
            for (uint64_t p = s; p <= s + k - d; p++) {
                if (!valid[p] || stamp[h[p]] == tick) continue;
                stamp[h[p]] = tick;
                score += freq[h[p]];
            }
            if (!any || score > best) { any = true; best = score; best_s = s; }
        }
        if (!any || best == 0) {
            if (++zero >= ZERO_RUNS) { r++; break; }
            continue;
        }
        zero = 0;
        const uint64_t s = best_s;
        uint64_t b = 0, l = 0;
        bool have = false;
        for (uint64_t p = s; p <= s + k - d; p++)
            if (valid[p] && freq[h[p]] != 0) { if (!have) b = p; have = true; l = p; }
        for (uint64_t p = s; p <= s + k - d; p++) if (valid[p]) freq[h[p]] = 0;
        uint64_t g = l + d - b;
        if (g > tail) g = tail;
        if (g < d) { r++; break; }
        tail -= g;
        memcpy(buf.data() + tail, S + b, g);
    }
    if (rounds) *rounds = r;
    memcpy(dict, buf.data() + tail, C - tail);
    return (int64_t)(C - tail);
}
