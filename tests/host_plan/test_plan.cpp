// Drives rust_compress_amd/csrc/rcx_plan.h -- the integer planning of the host-descriptor batch path -- on the CPU.
//   test_plan <section>      spans | ranges | reversed | chains | copies
// Prints HOST_PLAN_OK and exits 0 when every check of the section holds; the first failure names its line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>

#include "rcx_plan.h"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
typedef std::vector<uint64_t> V64;
typedef std::vector<uint32_t> V32;

// ---- spans ---------------------------------------------------------------------------------------------------------------------------
static void t_spans()
{
    rcx_spans sp; std::string err;
    V64 off = {10, 100, 5}, len = {20, 0, 300}, ooff = {0, 50, 20}, ocap = {50, 7, 0};
    CHECK(rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err));
    CHECK(sp.in_span == 305 && sp.out_span == 57 && sp.max_in == 300 && sp.max_block == 300);
    CHECK(rcx_plan_spans(3, off.data(), len.data(), nullptr, nullptr, sp, err));
    CHECK(sp.in_span == 305 && sp.out_span == 0 && sp.max_block == 300);
    ocap[1] = 4000;
    CHECK(rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && sp.max_block == 4000 && sp.max_in == 300 && sp.out_span == 4050);
    // 2^32 - 1 is the longest block, 2^32 is not a block
    len[1] = 0xffffffffull;
    CHECK(rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && sp.max_in == 0xffffffffull && sp.in_span == 100 + 0xffffffffull);
    len[1] = 1ull << 32;
    CHECK(!rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && err.find("block 1:") == 0);
    len[1] = 0; ocap[2] = 1ull << 32;
    CHECK(!rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && err.find("block 2:") == 0);
    CHECK(rcx_plan_spans(3, off.data(), len.data(), nullptr, nullptr, sp, err));          // (no output: its arrays are not looked at)
    ocap[2] = 0xffffffffull;
    CHECK(rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err));
    // off + len wraps
    off[2] = ~0ull - 10; len[2] = 11;
    CHECK(!rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && err.find("block 2:") == 0);
    len[2] = 10;
    CHECK(rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && sp.in_span == ~0ull);
    ooff[0] = ~0ull; ocap[0] = 1;
    CHECK(!rcx_plan_spans(3, off.data(), len.data(), ooff.data(), ocap.data(), sp, err) && err.find("block 0:") == 0);
}

// ---- ranges ----------------------------------------------------------------------------------------------------------------------------
// n blocks of `len` bytes back to back
static V32 bounds_of(uint32_t n, uint32_t pieces_knob, uint32_t fdiv_knob, bool* ranged = nullptr)
{
    V64 off(n), len(n, 1000);
    for (uint32_t i = 0; i < n; i++) off[i] = 1000ull * i;
    rcx_range_plan p;
    const uint32_t pieces = rcx_plan_piece_count(n, pieces_knob);
    if (pieces <= 1) { if (ranged) *ranged = false; return V32{0, n}; }
    const bool ok = rcx_plan_ranges(n, pieces, fdiv_knob, off.data(), len.data(), 1000ull * n, p);
    if (ranged) *ranged = ok;
    return p.bnd;
}
struct Layout { V64 off, len; uint64_t span; };
// what rcx_plan_ranges is to return for these boundaries, the slow way
static bool naive_ranges(const Layout& L, const V32& bnd, V64& lo, V64& hi)
{
    const uint32_t pieces = (uint32_t)bnd.size() - 1;
    lo.assign(pieces, 0); hi.assign(pieces, 0);
    uint64_t moved = 0, last_lo = 0;
    bool ascending = true;                                          // (the ranges' spans, one after the other, never start lower)
    for (uint32_t r = 0; r < pieces; r++) {
        bool any = false;
        uint64_t a = 0, b = 0;
        for (uint32_t i = bnd[r]; i < bnd[r + 1]; i++) {
            if (!L.len[i]) continue;
            const uint64_t s = L.off[i], e = L.off[i] + L.len[i];
            if (!any || s < a) a = s;
            if (!any || e > b) b = e;
            any = true;
        }
        if (!any) continue;
        lo[r] = a / 256 * 256; hi[r] = std::min((b + 255) / 256 * 256, L.span);
        moved += hi[r] - lo[r];
        if (lo[r] < last_lo) ascending = false;
        last_lo = lo[r];
    }
    return pieces > 1 && ascending && moved <= L.span + L.span / 4;
}
static void check_ranges(const Layout& L, uint32_t pieces_knob, uint32_t fdiv_knob, int want_ranged /* -1: whatever the threshold says */)
{
    const uint32_t n = (uint32_t)L.off.size();
    const uint32_t pieces = rcx_plan_piece_count(n, pieces_knob);
    CHECK(pieces >= 1 && pieces <= 16 && (pieces == 1 || pieces <= n / 128));
    if (pieces <= 1) { CHECK(want_ranged <= 0); return; }
    rcx_range_plan p;
    const bool ranged = rcx_plan_ranges(n, pieces, fdiv_knob, L.off.data(), L.len.data(), L.span, p);
    // every block is in exactly one range
    CHECK(p.bnd.size() >= 2 && p.bnd.front() == 0 && p.bnd.back() == n && p.pieces() <= pieces);
    for (size_t r = 0; r + 1 < p.bnd.size(); r++) CHECK(p.bnd[r] < p.bnd[r + 1]);
    CHECK(p.lo.size() == p.pieces() && p.hi.size() == p.pieces());
    for (uint32_t r = 0; r < p.pieces(); r++) {
        if (p.hi[r] <= p.lo[r]) {                                   // (a range of empty blocks moves nothing)
            for (uint32_t i = p.bnd[r]; i < p.bnd[r + 1]; i++) CHECK(L.len[i] == 0);
            continue;
        }
        CHECK(p.lo[r] % 256 == 0 && (p.hi[r] % 256 == 0 || p.hi[r] == L.span) && p.hi[r] <= L.span);
        for (uint32_t i = p.bnd[r]; i < p.bnd[r + 1]; i++)
            if (L.len[i]) CHECK(L.off[i] >= p.lo[r] && L.off[i] + L.len[i] <= p.hi[r]);
    }
    V64 lo, hi;
    const bool want = naive_ranges(L, p.bnd, lo, hi);
    for (uint32_t r = 0; r < p.pieces(); r++) if (hi[r] > lo[r]) CHECK(p.lo[r] == lo[r] && p.hi[r] == hi[r]);
    CHECK(ranged == want);
    if (want_ranged >= 0) CHECK(ranged == (want_ranged != 0));
}
static Layout random_layout(std::mt19937& g, uint32_t n, bool ragged)
{
    Layout L; L.off.resize(n); L.len.resize(n); L.span = 0;
    uint64_t at = g() % 300;
    for (uint32_t i = 0; i < n; i++) {
        L.len[i] = g() % 5 == 0 ? 0 : 1 + g() % 3000;
        L.off[i] = at;
        at += L.len[i] + (ragged ? g() % 100 : 0);
        if (L.len[i]) L.span = std::max(L.span, L.off[i] + L.len[i]);
        else if (g() % 2) L.off[i] = g();                           // (an empty block's offset means nothing)
    }
    return L;
}
static Layout reversed(const Layout& L)
{
    Layout R = L;
    std::reverse(R.off.begin(), R.off.end()); std::reverse(R.len.begin(), R.len.end());
    return R;
}
static void t_ranges()
{
    // the default knobs: 16 ranges at the most, 128 blocks a range at least, the first range n / 64 blocks and 64 at least
    bool ranged = true;
    CHECK(rcx_plan_piece_count(255, 0) == 1 && bounds_of(255, 0, 0, &ranged) == (V32{0, 255}) && !ranged);
    CHECK(bounds_of(256, 0, 0, &ranged) == (V32{0, 64, 256}) && ranged);
    CHECK(bounds_of(700, 0, 0) == (V32{0, 64, 223, 382, 541, 700}));
    const V32 b4096 = bounds_of(4096, 0, 0);
    CHECK(b4096.size() == 17 && b4096[1] == 64 && b4096[2] == 332 && b4096[16] == 4096);
    CHECK(rcx_plan_piece_count(1u << 20, 200) == 16 && rcx_plan_piece_count(1u << 20, 0) == 16 && rcx_plan_piece_count(1u << 20, 3) == 3);
    CHECK(rcx_plan_piece_count(700, 16) == 5 && rcx_plan_piece_count(700, 2) == 2 && rcx_plan_piece_count(127, 4) == 1 && rcx_plan_piece_count(0, 0) == 1);
    CHECK(bounds_of(1u << 16, 0, 0)[1] == 1024 && bounds_of(1u << 16, 0, 8)[1] == 8192 && bounds_of(1u << 16, 3, 0) == (V32{0, 1024, 1024 + (65536 - 1024) / 2, 65536}));
    // the threshold: in_span + in_span / 4 bytes may move, not one line more.  Two ranges of 256 blocks, all but four of them empty:
    // range 0 takes [0, A), range 1 the whole span
    for (int over = 0; over < 2; over++) {
        Layout L; L.off.assign(256, 0); L.len.assign(256, 0); L.span = 262144;
        const uint64_t A = 65536 + 256 * over;
        L.len[0] = 256; L.off[63] = A - 256; L.len[63] = 256;
        L.len[64] = 256; L.off[255] = L.span - 256; L.len[255] = 256;
        check_ranges(L, 0, 0, over ? 0 : 1);
    }
    std::mt19937 g(20261017);
    for (int it = 0; it < 300; it++) {
        const uint32_t n = it < 8 ? 250 + it : 1 + g() % 5000;
        const Layout L = random_layout(g, n, it % 3 != 0);
        check_ranges(L, it % 4 == 3 ? g() % 256 : 0, it % 5 == 4 ? g() % 256 : 0, -1);
        if (n >= 256 && L.span >= 65536 && it % 4 != 3) check_ranges(L, 0, 0, 1);       // (blocks in order: the lines two ranges share are all that moves twice)
        // blocks dealt out like cards (even indices from the front half, odd ones from the back): every range spans half the input
        if (n >= 512 && L.span >= 65536) {
            Layout D = L;
            for (uint32_t i = 0; i < n; i++) { const uint32_t j = i % 2 ? n / 2 + i / 2 : i / 2; D.off[i] = L.off[j]; D.len[i] = L.len[j]; }
            check_ranges(D, 0, 0, 0);
        }
        check_ranges(reversed(L), 0, 0, n >= 512 ? 0 : -1);         // (several ranges of blocks against input order: one copy)
    }
}
// the blocks of a batch listed in reverse input order
static void t_reversed()
{
    std::mt19937 g(7);
    int ranged_batches = 0;
    for (int it = 0; it < 20; it++) {
        const uint32_t n = 512 + g() % 4000;
        const Layout R = reversed(random_layout(g, n, true));
        rcx_range_plan p;
        const bool ranged = rcx_plan_ranges(n, rcx_plan_piece_count(n, 0), 0, R.off.data(), R.len.data(), R.span, p);
        uint64_t moved = 0;
        for (uint32_t r = 0; r < p.pieces(); r++) if (p.hi[r] > p.lo[r]) moved += p.hi[r] - p.lo[r];
        printf("n %u ranges %u in_span %llu moved %llu limit %llu -> %s\n", n, p.pieces(), (unsigned long long)R.span, (unsigned long long)moved,
               (unsigned long long)(R.span + R.span / 4), ranged ? "ranges" : "one range");
        ranged_batches += ranged;
    }
    CHECK(ranged_batches == 0);
}

// ---- chains ----------------------------------------------------------------------------------------------------------------------------
static void check_chains(const std::vector<uint8_t>& link, const V32& want_head, const V32& want_depth)
{
    const uint32_t n = (uint32_t)link.size();
    V64 ooff(n), ocap(n), dict(n);
    for (uint32_t i = 0; i < n; i++) { ooff[i] = 100000ull * (i + 1); ocap[i] = 1000 + i; dict[i] = i % 3 ? 70000 : i; }
    rcx_chain_plan p; std::string err;
    CHECK(rcx_plan_chains(n, link.empty() ? nullptr : link.data(), dict.data(), ooff.data(), ocap.data(), p, err));
    CHECK(p.n() == n && p.tab.size() == 3 * (size_t)n);
    uint32_t maxd = 0;
    for (uint32_t i = 0; i < n; i++) {
        CHECK(p.head()[i] == want_head[i] && p.depth[i] == want_depth[i]);
        maxd = std::max(maxd, want_depth[i]);
        const bool is_head = want_head[i] == i;
        CHECK(p.out_off[i] == (is_head ? ooff[i] : 0) && p.out_cap[i] == (is_head ? ocap[i] : 0));
        CHECK(p.dict()[i] == (is_head ? std::min<uint64_t>(dict[i], 65536) : 0));
    }
    CHECK(p.nrounds == maxd + 1 && p.rounds_off.size() == p.nrounds + 1 && p.rounds_off[0] == 0 && p.rounds_off[p.nrounds] == n);
    // order: a permutation, by depth, by index within a depth; rounds_off cuts it where the depth changes
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t r = 0; r < p.nrounds; r++) {
        CHECK(p.rounds_off[r] < p.rounds_off[r + 1]);
        for (uint32_t j = p.rounds_off[r]; j < p.rounds_off[r + 1]; j++) {
            const uint32_t i = p.order()[j];
            CHECK(i < n && !seen[i] && p.depth[i] == r);
            seen[i] = 1;
            if (j > p.rounds_off[r]) CHECK(p.order()[j - 1] < i);
        }
    }
}
static void t_chains()
{
    const uint32_t n = 37;
    V32 head(n), depth(n);
    std::vector<uint8_t> link(n, 0);
    for (uint32_t i = 0; i < n; i++) { head[i] = i; depth[i] = 0; }
    check_chains(link, head, depth);                                // all independent
    {                                                               // (and a null link array says the same)
        rcx_chain_plan p; std::string err; V64 o(n, 5), cp(n, 9);
        CHECK(rcx_plan_chains(n, nullptr, nullptr, o.data(), cp.data(), p, err) && p.nrounds == 1 && p.rounds_off == (V32{0, n}));
        for (uint32_t i = 0; i < n; i++) CHECK(p.order()[i] == i && p.head()[i] == i && p.dict()[i] == 0 && p.out_off[i] == 5 && p.out_cap[i] == 9);
    }
    for (uint32_t i = 0; i < n; i++) { link[i] = i > 0; head[i] = 0; depth[i] = i; }
    check_chains(link, head, depth);                                // one chain of n
    for (uint32_t i = 0; i < n; i++) { link[i] = i % 2; head[i] = i & ~1u; depth[i] = i % 2; }
    check_chains(link, head, depth);                                // pairs
    for (uint32_t i = 0; i < n; i++) { link[i] = i % 4 != 0; head[i] = i & ~3u; depth[i] = i % 4; }
    check_chains(link, head, depth);                                // fours, the last one cut short
    const uint8_t mixed[] = {0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0};
    check_chains(std::vector<uint8_t>(mixed, mixed + 11), V32{0, 0, 0, 3, 4, 4, 6, 6, 6, 6, 10}, V32{0, 1, 2, 0, 0, 1, 0, 1, 2, 3, 0});
    std::mt19937 g(99);
    for (int it = 0; it < 200; it++) {
        const uint32_t m = 1 + g() % 300;
        std::vector<uint8_t> lk(m); V32 h(m), d(m);
        for (uint32_t i = 0; i < m; i++) { lk[i] = i && g() % 3; h[i] = lk[i] ? h[i - 1] : i; d[i] = lk[i] ? d[i - 1] + 1 : 0; }
        check_chains(lk, h, d);
    }
    // the errors
    rcx_chain_plan p; std::string err;
    V64 ooff = {100, 0, 500}, ocap = {50, 0, 50}, dict = {100, 0, 0};
    uint8_t lk[3] = {1, 0, 0};
    CHECK(!rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && err.find("block 0 cannot continue a chain") != std::string::npos);
    lk[0] = 0; lk[1] = 1;
    CHECK(rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && p.dict()[0] == 100);     // a dictionary down to out_base itself
    dict[0] = 101;
    CHECK(!rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && err.find("block 0: dict_len reaches below out_base") == 0);
    dict[0] = 0; dict[1] = 1ull << 40;                                                                        // (a continuing block's dict_len is not looked at)
    CHECK(rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && p.dict()[1] == 0);
    dict[2] = 501;
    CHECK(!rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && err.find("block 2:") == 0);
    ooff[2] = 1u << 20; dict[2] = 70000;
    CHECK(rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && p.dict()[2] == 65536);
    dict[2] = 65536;
    CHECK(rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && p.dict()[2] == 65536);
    dict[2] = 65535;
    CHECK(rcx_plan_chains(3, lk, dict.data(), ooff.data(), ocap.data(), p, err) && p.dict()[2] == 65535);
}

// ---- what travels back ------------------------------------------------------------------------------------------------------------------
static void t_copies()
{
    {   // the used span: the last byte any block wrote, a block's out_len capped at its slot
        V64 ooff = {0, 100, 300, 1000}, ocap = {100, 200, 50, 500}, olen = {10, 250, 0, 0};
        CHECK(rcx_plan_used_span(4, ooff.data(), ocap.data(), olen.data()) == 300);
        olen[1] = 0; CHECK(rcx_plan_used_span(4, ooff.data(), ocap.data(), olen.data()) == 10);
        olen[0] = 0; CHECK(rcx_plan_used_span(4, ooff.data(), ocap.data(), olen.data()) == 0);
        olen[3] = 1; CHECK(rcx_plan_used_span(4, ooff.data(), ocap.data(), olen.data()) == 1001);
    }
    {   // chains that touch travel as one copy, an empty chain is no copy, a chain's sum is capped at its head's slot
        const V32 head = {0, 0, 2, 3, 3, 5, 6};
        V64 ooff = {10, 0, 40, 60, 0, 100, 130}, ocap = {30, 0, 20, 25, 0, 30, 10}, olen = {20, 10, 0, 20, 20, 30, 5};
        typedef std::vector<std::pair<uint64_t, uint64_t>> R;
        CHECK(rcx_plan_chain_copies(7, head.data(), ooff.data(), ocap.data(), olen.data()) == (R{{10, 40}, {60, 85}, {100, 135}}));
        olen[2] = 20;
        CHECK(rcx_plan_chain_copies(7, head.data(), ooff.data(), ocap.data(), olen.data()) == (R{{10, 85}, {100, 135}}));
        for (auto& l : olen) l = 0;
        CHECK(rcx_plan_chain_copies(7, head.data(), ooff.data(), ocap.data(), olen.data()).empty());
    }
    std::mt19937 g(4242);
    for (int it = 0; it < 300; it++) {
        const uint32_t n = 1 + g() % 200;
        std::vector<uint8_t> lk(n);
        V64 ooff(n), ocap(n), olen(n);
        uint64_t at = g() % 50;
        for (uint32_t i = 0; i < n; i++) {
            lk[i] = i && g() % 2;
            olen[i] = g() % 4 == 0 ? 0 : g() % 500;
            if (!lk[i]) { ooff[i] = at; ocap[i] = g() % 1200; at += ocap[i] + (g() % 3 ? 0 : g() % 40); }       // (slots in ascending order, some of them touching)
        }
        rcx_chain_plan p; std::string err;
        CHECK(rcx_plan_chains(n, lk.data(), nullptr, ooff.data(), ocap.data(), p, err));
        const auto got = rcx_plan_chain_copies(n, p.head(), p.out_off.data(), p.out_cap.data(), olen.data());
        // every chain's [out_off, out_off + min(sum, cap)), byte by byte
        std::vector<uint8_t> want(at + 1, 0), have(at + 1, 0);
        for (uint32_t i = 0; i < n; i++) {
            if (lk[i]) continue;
            uint64_t sum = 0;
            for (uint32_t j = i; j < n && (j == i || lk[j]); j++) sum += olen[j];
            sum = std::min(sum, ocap[i]);
            for (uint64_t x = ooff[i]; x < ooff[i] + sum; x++) want[x] = 1;
        }
        for (size_t r = 0; r < got.size(); r++) {
            CHECK(got[r].first < got[r].second && got[r].second <= at);
            if (r) CHECK(got[r - 1].second < got[r].first);         // ascending, disjoint, and merged where they touch
            for (uint64_t x = got[r].first; x < got[r].second; x++) have[x] = 1;
        }
        CHECK(want == have);
    }
}

int main(int argc, char** argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "spans") t_spans();
    else if (s == "ranges") t_ranges();
    else if (s == "reversed") t_reversed();
    else if (s == "chains") t_chains();
    else if (s == "copies") t_copies();
    else { printf("usage: test_plan spans|ranges|reversed|chains|copies\n"); return 2; }
    printf("HOST_PLAN_OK %s\n", s.c_str());
    return 0;
}
