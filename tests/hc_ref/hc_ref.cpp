// hc_ref.cpp -- plain serial references of the stages of the two high-compression encoders (TEST INFRASTRUCTURE), written from the
// definitions in the header comments of k_deflate_hc.hip and k_lz4_hc.hip: no waves, no rings, no staging.  They share with the kernels
// only what is part of the definition: the bucket function, the windows, the length limits and the RFC 1951 symbol tables.  Built by
// tests/hc_stages.py with g++; every function works on one stream (block) of n bytes.
#include <cstdint>
#include <cstring>
#include <vector>

static const uint32_t SEG = 65536;

static uint32_t bucket(const uint8_t* p)
{
    const uint32_t x = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return (uint32_t)(x * 2654435761u) >> 17;
}

// Chains: link[p] = the distance to the nearest earlier position of p's bucket if that is at most `win`, else 0; a position with fewer
// than 4 bytes left has no bucket (0).
extern "C" void ref_links(const uint8_t* in, uint64_t n, uint32_t win, uint16_t* link)
{
    std::vector<int64_t> last(1u << 15, -1);
    for (uint64_t p = 0; p < n; p++) {
        link[p] = 0;
        if (n - p < 4) continue;
        const uint32_t b = bucket(in + p);
        if (last[b] >= 0 && p - (uint64_t)last[b] <= win) link[p] = (uint16_t)(p - (uint64_t)last[b]);
        last[b] = (int64_t)p;
    }
}

// Search: from p, at most `depth` chain entries, until the summed distance passes `win`; the longest common prefix of at least 4 bytes,
// the first (nearest) among equals.
//   lz4 0: at most 258 bytes and not past the end of p's 64 KiB segment               -> cand = length << 16 | distance - 1
//   lz4 1: at most maxm bytes, starting >= 12 and ending >= 5 bytes before the end    -> cand = length << 16 | distance
extern "C" void ref_search(const uint8_t* in, uint64_t n, const uint16_t* link, uint32_t win, uint32_t depth, int lz4, uint32_t maxm,
                           uint32_t* cand)
{
    for (uint64_t p = 0; p < n; p++) {
        uint64_t maxl;
        if (lz4) maxl = n - p >= 12 ? n - 5 - p : 0;
        else { const uint64_t end = (p / SEG + 1) * SEG < n ? (p / SEG + 1) * SEG : n; maxl = end - p; }
        if (maxl > maxm) maxl = maxm;
        uint32_t best = 0, bd = 0;
        uint64_t dist = 0;
        for (uint32_t k = 0; k < depth && maxl >= 4; k++) {
            const uint32_t lk = link[p - dist];
            if (!lk) break;
            dist += lk;
            if (dist > win) break;
            uint32_t l = 0;
            while (l < maxl && in[p - dist + l] == in[p + l]) l++;
            if (l > best) { best = l; bd = (uint32_t)dist; }
            if (best == maxl) break;                       // (nothing is longer, and the nearest of equals is kept: the result stands)
        }
        cand[p] = best >= 4 ? best << 16 | (lz4 ? bd : bd - 1) : 0;
    }
}

// RFC 1951, 3.2.5
static const uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                   8193, 12289, 16385, 24577};
static const uint8_t DEXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static int len_sym(uint32_t l) { int s = 28; while (LBASE[s] > l) s--; return s; }     // (258 is symbol 285 = index 28, not 284 + extra)
static int dist_sym(uint32_t d) { int s = 29; while (DBASE[s] > d) s--; return s; }

// DEFLATE parse: the minimum, in bits under price[320] (literal/length lengths [288], distance lengths [32]), of any parse of the segment
// in[0..L) that takes at each position its literal or a match of 3..length bytes at the distance of cand (length << 16 | distance - 1).
extern "C" uint64_t ref_deflate_min_cost(const uint8_t* in, uint32_t L, const uint32_t* cand, const uint8_t* price)
{
    const uint64_t INF = ~0ull;
    std::vector<uint64_t> cost(L + 1, INF);
    uint32_t lbits[259];
    for (uint32_t l = 3; l <= 258; l++) { const int s = len_sym(l); lbits[l] = price[257 + s] + LEXTRA[s]; }
    cost[0] = 0;
    for (uint32_t p = 0; p < L; p++) {
        const uint64_t c = cost[p];                        // (never INF: the literals reach every position)
        if (c + price[in[p]] < cost[p + 1]) cost[p + 1] = c + price[in[p]];
        if (!cand[p]) continue;
        const uint32_t ml = cand[p] >> 16, d = (cand[p] & 0xffff) + 1;
        const int ds = dist_sym(d);
        const uint64_t dc = c + price[288 + ds] + DEXTRA[ds];
        for (uint32_t l = 3; l <= ml && p + l <= L; l++)
            if (dc + lbits[l] < cost[p + l]) cost[p + l] = dc + lbits[l];
    }
    return cost[L];
}

static uint32_t mext(uint32_t l) { return l >= 19 ? 1 + (l - 19) / 255 : 0; }
static uint64_t lext(uint64_t r) { return r >= 15 ? 1 + (r - 15) / 255 : 0; }

// LZ4 lower bound of a segment: the minimum of a parse of in[0..L) that pays 1 byte for a literal and 3 bytes plus its length bytes for
// a match of 4..length bytes (cand = length << 16 | distance; no match crosses the segment's end).  It leaves out the length bytes of
// the literal runs, which no parse pays less than nothing for.
extern "C" uint64_t ref_lz4_min_cost(uint32_t L, const uint32_t* cand)
{
    std::vector<uint64_t> cost(L + 1, ~0ull);
    cost[0] = 0;
    for (uint32_t p = 0; p < L; p++) {
        const uint64_t c = cost[p];
        if (c + 1 < cost[p + 1]) cost[p + 1] = c + 1;
        const uint32_t ml = cand[p] >> 16;
        for (uint32_t l = 4; l <= ml && p + l <= L; l++)
            if (c + 3 + mext(l) < cost[p + l]) cost[p + l] = c + 3 + mext(l);
    }
    return cost[L];
}

// LZ4 greedy: the size of the block of n bytes that takes, in every 64 KiB segment, the candidate wherever one starts (cut at the
// segment's end; a cut below 4 bytes is a literal), else a literal; sized by the LZ4 token rules over the whole block (the literal runs
// carry across segments; the last token holds literals only).
extern "C" uint64_t ref_lz4_greedy_size(uint64_t n, const uint32_t* cand)
{
    uint64_t size = 0, run = 0, p = 0;
    while (p < n) {
        const uint64_t end = (p / SEG + 1) * SEG < n ? (p / SEG + 1) * SEG : n;
        uint64_t ml = cand[p] >> 16;
        if (ml > end - p) ml = end - p;
        if (ml >= 4) { size += 1 + lext(run) + run + 2 + mext((uint32_t)ml); run = 0; p += ml; }
        else { run++; p++; }
    }
    return size + 1 + lext(run) + run;
}
