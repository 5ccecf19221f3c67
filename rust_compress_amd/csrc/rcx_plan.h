// rcx_plan.h -- the integer planning of the host-descriptor batch path (rcx_api.hip run_batch): span limits, the input ranges of a
// gated launch, the chains of a linked LZ4 batch, and what travels back.  Plain C++17, no HIP: tests/host_plan drives it on the CPU.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

// ---- spans and limits ---------------------------------------------------------------------------------------------------------
struct rcx_spans {
    uint64_t in_span = 0, out_span = 0;          // one past the highest byte any block reads / may write
    uint64_t max_block = 0;                      // the longest in_len or out_cap
    uint64_t max_in = 0;                         // the longest in_len
};
// out_off / out_cap: null for a codec that writes no output.  false: `err` names the block.
inline bool rcx_plan_spans(uint32_t n, const uint64_t* in_off, const uint64_t* in_len, const uint64_t* out_off, const uint64_t* out_cap,
                           rcx_spans& sp, std::string& err)
{
    sp = rcx_spans();
    const bool needs_out = out_off && out_cap;
    for (uint32_t i = 0; i < n; i++) {
        // the kernels index a block with 32-bit offsets: a block of 4 GiB or more (or a range that wraps) is a caller error,
        // not something to decode a prefix of
        if (in_len[i] >> 32 || in_off[i] + in_len[i] < in_off[i] ||
            (needs_out && (out_cap[i] >> 32 || out_off[i] + out_cap[i] < out_off[i]))) {
            err = "block " + std::to_string(i) + ": lengths of 4 GiB or more are not supported (per-block limit 2^32 - 1 bytes)";
            return false;
        }
        const uint64_t e = in_off[i] + in_len[i];
        if (e > sp.in_span) sp.in_span = e;
        if (in_len[i] > sp.max_block) sp.max_block = in_len[i];
        if (in_len[i] > sp.max_in) sp.max_in = in_len[i];
        if (needs_out) {
            const uint64_t o = out_off[i] + out_cap[i];
            if (o > sp.out_span) sp.out_span = o;
            if (out_cap[i] > sp.max_block) sp.max_block = out_cap[i];
        }
    }
    return true;
}

// ---- the input ranges of a gated launch ------------------------------------------------------------------------------------------
// how many ranges to try for n blocks (`knob`: bits 8-15 of the decoder's parameter, 0 = the library's choice): 16 at the most (the
// gate words of rcx_kargs), and no range of fewer than 128 blocks
inline uint32_t rcx_plan_piece_count(uint32_t n, uint32_t knob)
{
    uint32_t pieces = knob ? knob : 16u;
    if (pieces > 16u) pieces = 16u;
    if (pieces > n / 128u) pieces = n / 128u ? n / 128u : 1u;
    return pieces;
}
struct rcx_range_plan {
    std::vector<uint32_t> bnd;                   // range r: blocks bnd[r] .. bnd[r + 1]
    std::vector<uint64_t> lo, hi;                // ... and its bytes of the input span (hi <= lo: none)
    uint32_t pieces() const { return (uint32_t)bnd.size() - 1; }
};
// The first range is small (n / fdiv blocks, 64 at least; `fdiv_knob`: bits 16-23 of the parameter, 0 = 64), the others share the rest.
// A range's compressed bytes are the span from its lowest to its highest input byte, widened to whole 256-byte lines of the staging
// buffer (a line two ranges share is complete the first time anybody reads it; what the widening copies early are the caller's own
// bytes).  Blocks that do not lie in index order make the spans overlap: more than a quarter of the input twice, or fewer than two
// ranges, and the answer is false -- one copy in front of the launch.  So it is when the ranges' spans do not ascend (blocks listed
// in reverse input order: the spans do not overlap, but the ranges are for a batch whose bytes arrive front to back).
inline bool rcx_plan_ranges(uint32_t n, uint32_t pieces, uint32_t fdiv_knob, const uint64_t* in_off, const uint64_t* in_len, uint64_t in_span,
                            rcx_range_plan& p)
{
    p.bnd.assign(1, 0);
    const uint32_t fdiv = fdiv_knob ? fdiv_knob : 64u;       // (tuning)
    const uint32_t first = n / fdiv > 64u ? n / fdiv : 64u;
    for (uint32_t pc = 1; pc < pieces; pc++) {
        const uint32_t at = first + (uint32_t)((uint64_t)(n - first) * (pc - 1) / (pieces - 1));
        if (at > p.bnd.back() && at < n) p.bnd.push_back(at);
    }
    p.bnd.push_back(n);
    pieces = p.pieces();
    p.lo.assign(pieces, ~0ull); p.hi.assign(pieces, 0);
    uint64_t moved = 0, last_lo = 0;
    bool ascending = true;
    for (uint32_t pc = 0; pc < pieces; pc++) {
        for (uint32_t i = p.bnd[pc]; i < p.bnd[pc + 1]; i++) {
            if (!in_len[i]) continue;
            if (in_off[i] < p.lo[pc]) p.lo[pc] = in_off[i];
            if (in_off[i] + in_len[i] > p.hi[pc]) p.hi[pc] = in_off[i] + in_len[i];
        }
        if (p.hi[pc] > p.lo[pc]) {
            p.lo[pc] &= ~255ull;
            p.hi[pc] = (p.hi[pc] + 255ull) & ~255ull; if (p.hi[pc] > in_span) p.hi[pc] = in_span;
            moved += p.hi[pc] - p.lo[pc];
            if (p.lo[pc] < last_lo) ascending = false;
            last_lo = p.lo[pc];
        }
    }
    return pieces > 1 && ascending && moved <= in_span + in_span / 4;
}

// ---- the chains of a linked LZ4 batch ------------------------------------------------------------------------------------------------
struct rcx_chain_plan {
    std::vector<uint32_t> tab;                   // order[n] | head[n] | dict[n]: one upload
    std::vector<uint32_t> depth;                 // block i's place in its chain (a head: 0)
    std::vector<uint32_t> rounds_off;            // order[rounds_off[r] .. rounds_off[r + 1]): the blocks at depth r
    uint32_t nrounds = 0;
    std::vector<uint64_t> out_off, out_cap;      // the caller's for a head, 0 / 0 for a block that continues a chain
    uint32_t n() const { return (uint32_t)depth.size(); }
    const uint32_t* order() const { return tab.data(); }           // the blocks sorted by depth, by index within a depth
    const uint32_t* head() const { return tab.data() + n(); }      // block i's chain head
    const uint32_t* dict() const { return tab.data() + 2 * (size_t)n(); }   // a head's dictionary bytes in front of its slot (65536 at the most)
};
// link: null or a flag per block (continues the chain of the block before it); dict_len: null or a length per head.  n > 0.
inline bool rcx_plan_chains(uint32_t n, const uint8_t* link, const uint64_t* dict_len, const uint64_t* out_off, const uint64_t* out_cap,
                            rcx_chain_plan& p, std::string& err)
{
    if (link && link[0]) { err = "lz4 linked decode: block 0 cannot continue a chain"; return false; }
    p.tab.assign(3 * (size_t)n, 0); p.depth.assign(n, 0); p.out_off.assign(n, 0); p.out_cap.assign(n, 0);
    uint32_t* order = p.tab.data(); uint32_t* head = order + n; uint32_t* dict = head + n;
    p.nrounds = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool cont = link && link[i];
        head[i] = cont ? head[i - 1] : i;
        p.depth[i] = cont ? p.depth[i - 1] + 1 : 0;
        if (p.depth[i] + 1 > p.nrounds) p.nrounds = p.depth[i] + 1;
        p.out_off[i] = cont ? 0 : out_off[i];
        p.out_cap[i] = cont ? 0 : out_cap[i];
        const uint64_t d = (!cont && dict_len) ? dict_len[i] : 0;
        if (d > p.out_off[i]) { err = "block " + std::to_string(i) + ": dict_len reaches below out_base"; return false; }
        dict[i] = (uint32_t)(d > 65536u ? 65536u : d);
    }
    std::vector<uint32_t> at(p.nrounds + 2, 0);                 // counting sort by depth
    for (uint32_t i = 0; i < n; i++) at[p.depth[i] + 2]++;
    for (uint32_t r = 2; r < p.nrounds + 2; r++) at[r] += at[r - 1];
    for (uint32_t i = 0; i < n; i++) order[at[p.depth[i] + 1]++] = i;
    at.resize(p.nrounds + 1);                                   // (the sort left at[r] at the first block of depth r, at[nrounds] = n)
    p.rounds_off.swap(at);
    return true;
}

// ---- histories (the DEFLATE calls with history) ---------------------------------------------------------------------------------------
// The kernels' aux words of n blocks with histories: aux[i] = hist_len[i], then (ids != null: the zlib forms) aux[n + i] = ids[i].
// hist_len[i] bytes lie directly before off[i] (in_off for an encoder, out_off for a decoder) in the same buffer: at most max_hist and
// at most off[i].  nhist: the blocks with a history.  false: `err` (prefixed with `what`) names the block.  n > 0, hist_len != null.
inline bool rcx_plan_hist(uint32_t n, const uint64_t* hist_len, const uint64_t* off, uint64_t max_hist, const uint32_t* ids,
                          const char* what, std::vector<uint32_t>& aux, uint32_t& nhist, std::string& err)
{
    aux.assign((ids ? 2 : 1) * (size_t)n, 0);
    nhist = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (hist_len[i] > off[i] || hist_len[i] > max_hist) {
            err = std::string(what) + ": block " + std::to_string(i) + ": a history of " + std::to_string(hist_len[i]) + " bytes "
                + (hist_len[i] > max_hist ? "(at most " + std::to_string(max_hist) + ")"
                                          : "does not fit in front of offset " + std::to_string(off[i]));
            return false;
        }
        aux[i] = (uint32_t)hist_len[i];
        nhist += hist_len[i] ? 1u : 0u;
        if (ids) aux[(size_t)n + i] = ids[i];
    }
    return true;
}

// ---- shared dictionaries (the encoders' *_shared_batch calls) -----------------------------------------------------------------------------
// Block i's history is the dict_len[i] bytes at dict_off[i] of the input buffer, anywhere in it; dict_len[i] == 0: none, dict_off[i]
// ignored.  At most max_dict bytes (false: `err`, prefixed with `what`, names the block), of which the last `reach` count: a longer one
// is clamped to them, and blocks whose ranges are equal AFTER the clamp share one dictionary (ranges that overlap but differ do not).
// aux: the kernels' words, RCX_DICT_WORDS per block, laid out by csrc/lz_dict.h: [0, n) the clamped length, [n, 2n) ids[i] (ids != null:
// the zlib form), [2n, 3n) the dictionary's index among the distinct ones, [3n, 5n) its offset (low words, then high words), [5n,
// 5n + ndict) a block that names dictionary j (the rest of [5n, 6n): n, no block).  span: one past the highest dictionary byte.  n > 0.
static const uint32_t RCX_DICT_WORDS = 6;
struct rcx_dict_plan {
    std::vector<uint32_t> aux;
    uint32_t ndict = 0;
    uint64_t span = 0;
};
inline bool rcx_plan_dict(uint32_t n, const uint64_t* dict_off, const uint64_t* dict_len, uint64_t max_dict, uint64_t reach, const uint32_t* ids,
                          const char* what, rcx_dict_plan& p, std::string& err)
{
    const size_t N = n;
    p.aux.assign(RCX_DICT_WORDS * N, 0);
    for (size_t i = 0; i < N; i++) p.aux[5 * N + i] = n;
    p.ndict = 0; p.span = 0;
    std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint32_t>> named;       // (offset, length) after the clamp, block
    for (uint32_t i = 0; i < n; i++) {
        if (ids) p.aux[N + i] = ids[i];
        uint64_t len = dict_len[i], off = len ? dict_off[i] : 0;
        if (len > max_dict || off + len < off) {
            err = std::string(what) + ": block " + std::to_string(i) + ": a dictionary of " + std::to_string(len) + " bytes "
                + (len > max_dict ? "(at most " + std::to_string(max_dict) + ")" : "at offset " + std::to_string(off) + " wraps");
            return false;
        }
        if (!len) continue;
        if (off + len > p.span) p.span = off + len;
        if (len > reach) { off += len - reach; len = reach; }
        p.aux[i] = (uint32_t)len;
        p.aux[3 * N + i] = (uint32_t)off; p.aux[4 * N + i] = (uint32_t)(off >> 32);
        named.push_back({{off, len}, i});
    }
    std::sort(named.begin(), named.end());                                        // equal ranges side by side, their lowest block first
    for (size_t k = 0; k < named.size(); k++) {
        if (!k || named[k].first != named[k - 1].first) p.aux[5 * N + p.ndict++] = named[k].second;
        p.aux[2 * N + named[k].second] = p.ndict - 1;
    }
    return true;
}

// ---- what travels back ------------------------------------------------------------------------------------------------------------------
// only what was produced: the span up to the last byte any block wrote, not the slots' capacity
inline uint64_t rcx_plan_used_span(uint32_t n, const uint64_t* out_off, const uint64_t* out_cap, const uint64_t* out_len)
{
    uint64_t used = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t l = out_len[i] < out_cap[i] ? out_len[i] : out_cap[i];
        if (l && out_off[i] + l > used) used = out_off[i] + l;
    }
    return used;
}
// what the blocks produced and nothing else: block i's first min(out_len, out_cap) bytes at out_off[i], blocks that touch (in batch order)
// as one range.  [first, second) byte ranges in batch order.  For the calls that promise the caller's bytes BETWEEN the slots without
// staging the output buffer in (the decoders behind shared dictionaries): contiguous slots travel as one copy, slots with gaps one each.
inline std::vector<std::pair<uint64_t, uint64_t>> rcx_plan_slot_copies(uint32_t n, const uint64_t* out_off, const uint64_t* out_cap, const uint64_t* out_len)
{
    std::vector<std::pair<uint64_t, uint64_t>> r;
    uint64_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t l = out_len[i] < out_cap[i] ? out_len[i] : out_cap[i];
        if (!l) continue;
        if (hi > lo && out_off[i] == hi) { hi += l; continue; }
        if (hi > lo) r.emplace_back(lo, hi);
        lo = out_off[i]; hi = lo + l;
    }
    if (hi > lo) r.emplace_back(lo, hi);
    return r;
}
// a chain's bytes lie behind its head's out_off, as many as its blocks' out_len add up to (its head's out_cap at the most); chains
// that touch travel as one copy.  [first, second) byte ranges in chain order.
inline std::vector<std::pair<uint64_t, uint64_t>> rcx_plan_chain_copies(uint32_t n, const uint32_t* head, const uint64_t* out_off,
                                                                         const uint64_t* out_cap, const uint64_t* out_len)
{
    std::vector<std::pair<uint64_t, uint64_t>> r;
    uint64_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < n;) {
        uint64_t sum = 0;
        uint32_t j = i;
        do { sum += out_len[j]; j++; } while (j < n && head[j] == i);
        if (sum > out_cap[i]) sum = out_cap[i];
        // (a chain whose last block failed may have written part of that block behind the sum: inside its slot, not reported)
        if (sum && out_off[i] == hi) hi += sum;
        else if (sum) {
            if (hi > lo) r.emplace_back(lo, hi);
            lo = out_off[i]; hi = lo + sum;
        }
        i = j;
    }
    if (hi > lo) r.emplace_back(lo, hi);
    return r;
}
