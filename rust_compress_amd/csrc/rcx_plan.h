// rcx_plan.h -- the integer planning of the host-descriptor batch path (rcx_api.hip run_batch): span limits, the input ranges of a
// gated launch, the chains of a linked LZ4 batch, and what travels back.  Plain C++17, no HIP: tests/host_plan drives it on the CPU.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rcx.h"

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
// Is every byte of [0, out_span) inside some block's slot [out_off[i], out_off[i] + out_cap[i])?  (out_span: rcx_plan_spans', one past
// the highest slot byte.)  Then one copy of the used span from a staging buffer touches nothing but slots, whose bytes beyond out_len
// are unspecified; otherwise it would replace the caller's bytes in front of, between and behind the slots (run_batch stages the output
// span in first for such a layout).  A dense layout in address order, which is how every packer lays its slots out, is recognised in
// one pass without an allocation; anything else by a sort of the slots.  Slots of capacity 0 cover nothing; overlapping slots cover
// their union.
inline bool rcx_plan_out_dense(uint32_t n, const uint64_t* out_off, const uint64_t* out_cap, uint64_t out_span)
{
    uint64_t at = 0;
    uint32_t i = 0;
    for (; i < n; i++) {
        if (!out_cap[i]) continue;
        if (out_off[i] > at) break;                            // a gap, unless a later slot fills it: the sort below decides
        if (out_off[i] + out_cap[i] > at) at = out_off[i] + out_cap[i];
    }
    if (i == n) return at == out_span;
    std::vector<std::pair<uint64_t, uint64_t>> s;
    for (uint32_t j = 0; j < n; j++) if (out_cap[j]) s.emplace_back(out_off[j], out_off[j] + out_cap[j]);
    std::sort(s.begin(), s.end());
    at = 0;
    for (const auto& r : s) {
        if (r.first > at) return false;
        if (r.second > at) at = r.second;
    }
    return at == out_span;
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

// ---- dictionary training (rcx_dict_train_batch, k_dict_train.hip) -------------------------------------------------------------------
// Job i trains one dictionary of out_cap[i] bytes from the corpus in_len[i], the concatenation of nsamples[i] samples.  The plan checks
// the arguments, does the epoch arithmetic of DESIGN.md 3.19, bounds the rounds and lays out the scratch; its words go to the kernels
// in the descriptors' aux array:
//   [0, N)                          comes back: the rounds job i ran
//   [N + RCX_TRAIN_HDR * i ...)     job i: first sample end (index), samples, E, size, scratch offset (low, high), dead, 0
//   [N * (1 + RCX_TRAIN_HDR) ...)   the sample ENDS of every job (prefix sums of its lengths, 32 bits: a corpus is shorter than 4 GiB)
// The carve below is constexpr so that the kernels compute a job's arrays from the same function.
#define RCX_TRAIN_PASSES 4u
#define RCX_TRAIN_ZERO_RUNS 10u
#define RCX_TRAIN_HDR 8u
#define RCX_TRAIN_SCAN_BLOCKS 128u            /* workgroups a job in the two scan launches: one partial sum each */
#define RCX_TRAIN_STATE_WORDS 16u             /* tail, zero, done, rounds, best (64 bits), padding */
#define RCX_TRAIN_MAX_JOBS 65535u             /* the job index rides on a grid dimension */
constexpr uint64_t rcx_train_up(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }
struct rcx_train_carve { uint64_t hash, back, freq, diff, stage, end; };      // byte offsets inside a job's region
// hash: a word per position; back: 16 bits per position; freq: 2^f words; diff: size + 1 words; stage: the dictionary, built from its end
constexpr rcx_train_carve rcx_train_job_carve(uint64_t n, uint64_t cap, uint64_t size, uint32_t f)
{
    rcx_train_carve c = {0, 0, 0, 0, 0, 0};
    c.back = c.hash + rcx_train_up(4 * n);
    c.freq = c.back + rcx_train_up(2 * n);
    c.diff = c.freq + rcx_train_up((uint64_t)4 << f);
    c.stage = c.diff + rcx_train_up(4 * (size + 1));
    c.end = c.stage + rcx_train_up(cap);
    return c;
}
// in front of the jobs' regions: 256 bytes of counters (word 0: the jobs that are done), the jobs' state, the scan's partial sums
constexpr uint64_t rcx_train_state_at(uint32_t) { return 256; }
constexpr uint64_t rcx_train_partial_at(uint32_t njobs) { return 256 + rcx_train_up((uint64_t)njobs * RCX_TRAIN_STATE_WORDS * 4); }
constexpr uint64_t rcx_train_head_bytes(uint32_t njobs) { return rcx_train_partial_at(njobs) + rcx_train_up((uint64_t)njobs * RCX_TRAIN_SCAN_BLOCKS * 4); }
struct rcx_train_epochs { uint64_t E, size; };
// E = max(1, C / k / PASSES), size = n / E; epochs shorter than 10 k are made 10 k long (or n), and E follows
constexpr rcx_train_epochs rcx_train_epoch_plan(uint64_t n, uint64_t cap, uint32_t k)
{
    rcx_train_epochs e = {cap / k / RCX_TRAIN_PASSES, 0};
    if (e.E < 1) e.E = 1;
    e.size = n / e.E;
    if (e.size < (uint64_t)10 * k) {
        e.size = (uint64_t)10 * k < n ? (uint64_t)10 * k : n;
        e.E = e.size ? n / e.size : 1;
        if (e.E < 1) e.E = 1;
    }
    return e;
}
// a job that cannot produce a byte (n < k: no start; C < d: no segment fits) runs no round and has no region
constexpr bool rcx_train_dead(uint64_t n, uint64_t cap, uint32_t k, uint32_t d) { return n < k || cap < d; }
// every round that picks a start takes d bytes or more off the tail or ends the job, and fewer than ZERO_RUNS rounds in a row pick none
constexpr uint64_t rcx_train_round_bound(uint64_t cap, uint32_t d) { return (cap / d + 2) * (RCX_TRAIN_ZERO_RUNS + 1); }
struct rcx_train_plan {
    std::vector<uint32_t> aux;
    uint32_t aux_words = 1;                      // words per job of aux (run_batch stages aux_words * n)
    uint32_t k = 0, d = 0, f = 0;
    uint64_t scratch_bytes = 0;                  // with 256 bytes of slack: the kernels align the base
    uint64_t max_rounds = 0, max_n = 0, max_size = 0, max_cap = 0;
    uint32_t live = 0;                           // jobs that run rounds
};
// false: `err` names the job
inline bool rcx_plan_train(uint32_t n, const uint64_t* in_len, const uint64_t* out_cap, const uint32_t* nsamples, const uint64_t* sample_len,
                           uint32_t k, uint32_t d, uint32_t f, rcx_train_plan& p, std::string& err)
{
    p = rcx_train_plan();
    p.k = k; p.d = d; p.f = f;
    if (d != 6 && d != 8) { err = "dict train: d must be 6 or 8"; return false; }
    if (k < d || k > 4096) { err = "dict train: k must be d..4096"; return false; }
    if (f < 10 || f > 22) { err = "dict train: f must be 10..22"; return false; }
    if (n > RCX_TRAIN_MAX_JOBS) { err = "dict train: at most 65535 jobs a call"; return false; }
    if (n && (!in_len || !out_cap || !nsamples)) { err = "dict train: null array"; return false; }
    const size_t N = n;
    uint64_t total = 0;
    for (size_t i = 0; i < N; i++) total += nsamples[i];
    if (total && !sample_len) { err = "dict train: null sample_len array"; return false; }
    const uint64_t words = (uint64_t)N * (1 + RCX_TRAIN_HDR) + total;
    p.aux_words = N ? (uint32_t)((words + N - 1) / N) : 1;
    p.aux.assign((size_t)p.aux_words * N, 0);
    uint64_t at = rcx_train_head_bytes(n), first = 0;
    for (size_t i = 0; i < N; i++) {
        if (in_len[i] >> 32 || out_cap[i] >> 32) {
            err = "dict train: job " + std::to_string(i) + ": a corpus or a capacity of 4 GiB or more";
            return false;
        }
        uint64_t sum = 0;
        uint32_t* ends = p.aux.data() + N * (1 + RCX_TRAIN_HDR) + first;
        for (uint32_t s = 0; s < nsamples[i]; s++) {
            const uint64_t l = sample_len[first + s];
            if (l > in_len[i] - sum) { sum = ~(uint64_t)0; break; }
            sum += l;
            ends[s] = (uint32_t)sum;
        }
        if (sum != in_len[i]) {
            err = "dict train: job " + std::to_string(i) + ": the sample lengths do not add up to in_len " + std::to_string(in_len[i]);
            return false;
        }
        const rcx_train_epochs e = rcx_train_epoch_plan(in_len[i], out_cap[i], k);
        const bool dead = rcx_train_dead(in_len[i], out_cap[i], k, d);
        uint32_t* h = p.aux.data() + N + RCX_TRAIN_HDR * i;
        h[0] = (uint32_t)first; h[1] = nsamples[i]; h[2] = (uint32_t)e.E; h[3] = (uint32_t)e.size;
        h[4] = (uint32_t)at; h[5] = (uint32_t)(at >> 32); h[6] = dead ? 1u : 0u;
        first += nsamples[i];
        if (dead) continue;
        at += rcx_train_job_carve(in_len[i], out_cap[i], e.size, f).end;
        p.live++;
        p.max_rounds = std::max(p.max_rounds, rcx_train_round_bound(out_cap[i], d));
        p.max_n = std::max(p.max_n, in_len[i]); p.max_size = std::max(p.max_size, e.size); p.max_cap = std::max(p.max_cap, out_cap[i]);
    }
    p.scratch_bytes = at + 256;
    return true;
}
// every job counted at max_corpus and max_cap, and its epoch at the whole corpus (a small capacity makes one epoch of it)
inline uint64_t rcx_plan_train_scratch(uint32_t njobs, uint64_t max_corpus, uint64_t max_cap, uint32_t k, uint32_t f)
{
    if (f < 10 || f > 22 || k < 6 || k > 4096) return 0;
    return rcx_train_head_bytes(njobs) + (uint64_t)njobs * rcx_train_job_carve(max_corpus, max_cap, max_corpus, f).end + 256;
}

// ---- bzip2 (rcx_bzip2_decode_batch, k_bzip2.hip) -------------------------------------------------------------------------------------
// The scan reports, per file and in increasing position, every place where one of the two 48-bit marks or a stream header stands; one
// wave decodes every block mark speculatively.  The chain below strings them into streams: from bit 32 the next item must be a candidate
// at exactly the expected bit, a block's successor is expected where its decode ended, and a mark that merely occurred inside data is
// never reached and drops out.  Pure host code (tests/host_plan/test_plan_bz2.cpp).
#define RCX_BZ2_BLOCK 0u                      /* the mark 0x314159265359 */
#define RCX_BZ2_END 1u                        /* the mark 0x177245385090; extra: the 32 bits behind it, the stream's combined CRC */
#define RCX_BZ2_HEAD 2u                       /* 'B' 'Z' 'h' '1'..'9' at a byte position; extra: the level 1..9 */
#define RCX_BZ2_MAX_BLOCK 900000u
#define RCX_BZ2_MAX_SELECTORS 18002u
struct rcx_bz2_cand { uint64_t bit; uint32_t kind, extra; };                           // bit: where the mark (the 'B') starts
struct rcx_bz2_rec { int32_t status; uint32_t nblock, orig, crc; uint64_t end_bit; };   // what the entropy stage left of a block candidate
// the launch loop's scratch: two buffers (0: the stages', 1: the inverse BWT's) that can be asked for again, larger -- the candidates are
// counted by the first launch, the blocks' sizes known after the entropy stage; what a buffer held is gone after the next call for it
struct rcx_bz2_alloc { void* (*get)(void* self, int which, uint64_t bytes); void* self; };
// somebody who watches a call (the tests' record): every candidate of the scan with its file, every block a walk accepts, every round
struct rcx_bz2_watch {
    void* self;
    void (*candidate)(void* self, uint32_t file, const struct rcx_bz2_cand* c);
    void (*live)(void* self, uint32_t file, uint64_t bit);
    void (*round)(void* self);
};
struct rcx_bz2_chain {                        // one file's walk; resumable: blocks are decoded in rounds
    uint64_t expect = 0;                      // the bit at which the next item must start
    uint32_t level = 0, crc = 0;              // of the stream the walk is in
    uint32_t next = 0;                        // the first candidate not passed yet
    uint32_t streams = 0;                     // streams accepted so far
    bool in_stream = false, done = false;
    int32_t status = RCX_OK;                  // enum rcx_status, valid when done
    uint64_t in_used = 0;                     // the byte just after the last accepted stream's padding
};
// Walks file `len` bytes long over its candidates c[0 .. n) (sorted by bit).  rec[i] is valid for the block candidates i < avail; the walk
// stops in front of the first block candidate it needs beyond that and returns false: call again with more.  Every accepted block's
// candidate index is appended to `live`, in stream order.  true: the walk is over, st.status and st.in_used are final.
inline bool rcx_plan_bz2_chain(uint64_t len, const rcx_bz2_cand* c, uint32_t n, const rcx_bz2_rec* rec, uint32_t avail, rcx_bz2_chain& st,
                               std::vector<uint32_t>& live)
{
    const uint64_t bits = len * 8;
    auto fail = [&](int32_t s) { st.status = s; st.done = true; st.in_used = 0; return true; };
    while (!st.done) {
        if (!st.in_stream) {
            // a stream header at byte expect / 8, or (behind an accepted stream) the end of what counts
            while (st.next < n && (c[st.next].bit < st.expect || (c[st.next].bit == st.expect && c[st.next].kind != RCX_BZ2_HEAD))) st.next++;
            if (st.next < n && c[st.next].bit == st.expect) {
                st.level = c[st.next].extra; st.crc = 0; st.in_stream = true; st.expect += 32; st.next++;
                continue;
            }
            if (st.streams) { st.done = true; st.status = RCX_OK; return true; }
            return fail(len < 4 ? RCX_E_EOF : RCX_E_BZ2_MAGIC);
        }
        while (st.next < n && (c[st.next].bit < st.expect || (c[st.next].bit == st.expect && c[st.next].kind == RCX_BZ2_HEAD))) st.next++;
        if (st.next >= n || c[st.next].bit != st.expect) return fail(st.expect + 48 > bits ? RCX_E_EOF : RCX_E_BZ2_DATA);
        const rcx_bz2_cand& k = c[st.next];
        if (k.kind == RCX_BZ2_END) {
            if (st.expect + 80 > bits) return fail(RCX_E_EOF);
            if (k.extra != st.crc) return fail(RCX_E_BZ2_STREAM_CRC);
            st.in_used = (st.expect + 80 + 7) / 8; st.expect = st.in_used * 8;
            st.in_stream = false; st.streams++; st.next++;
            continue;
        }
        if (st.next >= avail) return false;
        const rcx_bz2_rec& r = rec[st.next];
        if (r.status) return fail(r.status);
        if (r.nblock > 100000u * st.level || r.end_bit <= st.expect) return fail(RCX_E_BZ2_DATA);
        live.push_back(st.next);
        st.crc = ((st.crc << 1) | (st.crc >> 31)) ^ r.crc;
        st.expect = r.end_bit; st.next++;
    }
    return true;
}

// ---- bzip2 encode (rcx_bzip2_encode_batch, k_bzip2_enc.hip) ----------------------------------------------------------
// One file is one stream.  A block holds C bytes of run-length form (C = 100000 * level - 19; the tests pass smaller ones).  A file of L
// bytes is cut into chunks of s input bytes, the last one shorter, and every chunk is one block.  s is what fills a block on the file's
// average, less a 64th: q = floor(C L / R), R the sum of the run-length forms of the file's pieces of C input bytes, each measured on its
// own, and s = q - q / 64 -- about 0.98 C for text, 0.82 C where five bytes become six, many times C for long runs, as libbz2's
// greedy cut takes them.  While the longest form of a chunk is over C, s becomes min(s - 1, q' - q' / 64) with q' = floor(s C / longest),
// and from the fifth such turn on at most s / 2 as well: s starts at 2^30 or less, so 4 + 30 shortenings reach one byte, which always
// fits, and a file is measured 1 + 35 times at the very most (a file whose stretches differ wildly; two times is the rule).  The cut
// is not greedy: every block is known before any is encoded.
// Pure host code (tests/host_plan/test_plan_bz2_enc.cpp).
#define RCX_BZ2E_ROUND 1024u                  /* blocks a round unless the caller says otherwise */
#define RCX_BZ2E_ROUND_MAX 4096u
#define RCX_BZ2E_HEAD_BITS 32u                /* 'B' 'Z' 'h' level */
#define RCX_BZ2E_TAIL_BITS 80u                /* the end mark and the combined CRC */
struct rcx_bz2e_block {
    uint32_t file;
    uint32_t len;                             // input bytes
    uint64_t off;                             // where they start in the file
    uint32_t n;                               // the length of the run-length form (0: not measured yet)
    uint32_t pad;
};
// what the stages leave of a block: the CRC over its input bytes, origPtr, the symbols with the end symbol, the tables and selectors, the
// bits in front of the symbols and the block's bits in all, the used-byte map (bit b of word b / 32)
struct rcx_bz2e_hdr { uint32_t crc, orig, nmtf, ngroups, nsel, alpha, head_bits, bits; uint32_t used[8]; };
// somebody who watches a call (the tests' record): every block behind its round with the stage arrays -- T, L, the symbols, the lengths
// (6 x 258) and the selectors AS THE DEVICE HOLDS THEM, so only a harness whose device memory is the host's can read them -- and every round
struct rcx_bz2e_watch {
    void* self;
    void (*block)(void* self, uint32_t index, const struct rcx_bz2e_block* b, const uint8_t* T, const uint8_t* L, const struct rcx_bz2e_hdr* h,
                  const uint16_t* syms, const uint8_t* lens, const uint8_t* sel);
    void (*round)(void* self);
};
// the measuring pieces (C input bytes each, the last one shorter) of every file, in file order; an empty file has none.  false: a file
// of 4 GiB or more
inline bool rcx_plan_bz2e_chunks(uint32_t nfiles, const uint64_t* in_len, uint32_t C, std::vector<rcx_bz2e_block>& out, std::string& err)
{
    out.clear();
    for (uint32_t f = 0; f < nfiles; f++) {
        if (in_len[f] >> 32) { err = "block " + std::to_string(f) + ": lengths of 4 GiB or more are not supported (per-block limit 2^32 - 1 bytes)"; return false; }
        for (uint64_t o = 0; o < in_len[f]; o += C)
            out.push_back(rcx_bz2e_block{f, (uint32_t)std::min<uint64_t>(C, in_len[f] - o), o, 0u, 0u});
    }
    return true;
}
// input bytes a chunk of a file of len > 0 bytes starts with, from the sum of its pieces' run-length forms (rle_sum > 0): 2^30 at the
// most, whatever the runs (the kernels index a chunk with 32 bits, with room to step past its end)
#define RCX_BZ2E_MAX_CHUNK (1ull << 30)
inline uint64_t rcx_plan_bz2e_step(uint64_t len, uint64_t rle_sum, uint32_t C)
{
    const uint64_t q = (uint64_t)C * len / rle_sum, s = q - q / 64;
    return std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(s, 1), len), RCX_BZ2E_MAX_CHUNK);
}
// ... and the next, smaller one when the longest form of a chunk did not fit; turn: how often s has been shortened already
#define RCX_BZ2E_TURNS 36u                    /* probes of the chunk length at the most: the first, 4 in proportion, 30 halvings, one to spare */
inline uint64_t rcx_plan_bz2e_less(uint64_t s, uint32_t longest, uint32_t C, uint32_t turn)
{
    const uint64_t q = s * C / longest;
    uint64_t t = std::min<uint64_t>(s - 1, q - q / 64);
    if (turn >= 4) t = std::min<uint64_t>(t, s / 2);
    return std::max<uint64_t>(t, 1);
}
// appends the chunks of file f, len bytes long, at s input bytes a chunk, n = 0: to be measured
inline void rcx_plan_bz2e_cut(uint32_t f, uint64_t len, uint64_t s, std::vector<rcx_bz2e_block>& out)
{
    for (uint64_t o = 0; o < len; o += s) out.push_back(rcx_bz2e_block{f, (uint32_t)std::min<uint64_t>(s, len - o), o, 0u, 0u});
}
// rounds: cuts[r] .. cuts[r + 1] are the blocks of round r, `per_round` at the most
inline void rcx_plan_bz2e_rounds(uint32_t nblocks, uint32_t per_round, std::vector<uint32_t>& cuts)
{
    cuts.assign(1, 0u);
    if (!per_round) per_round = 1;
    for (uint32_t b = 0; b < nblocks;) { b = (uint32_t)std::min<uint64_t>((uint64_t)b + per_round, nblocks); cuts.push_back(b); }
}
struct rcx_bz2e_file {
    uint32_t first, count;                    // its blocks
    uint32_t crc;                             // the combined CRC: c = rotl(c, 1) ^ crc of every block in order
    int32_t status;                           // RCX_OK, or RCX_E_OUTPUT_TOO_SMALL: nothing of it is written
    uint64_t bits;                            // header, blocks and trailer, without the padding
    uint64_t out_len;                         // the stream's size in bytes
};
// Where every block's bits start in its file's stream (bit_off, behind the 32 header bits), and every file's size, combined CRC and
// status against its capacity.  bits / crc: per block, what the fit and the run-length stage left.
inline void rcx_plan_bz2e_layout(uint32_t nfiles, const std::vector<rcx_bz2e_block>& blocks, const uint64_t* bits, const uint32_t* crc,
                                 const uint64_t* out_cap, std::vector<uint64_t>& bit_off, std::vector<rcx_bz2e_file>& files)
{
    bit_off.assign(blocks.size(), 0);
    files.assign(nfiles, rcx_bz2e_file{0u, 0u, 0u, RCX_OK, 0ull, 0ull});
    size_t b = 0;
    for (uint32_t f = 0; f < nfiles; f++) {
        rcx_bz2e_file& F = files[f];
        F.first = (uint32_t)b;
        uint64_t at = RCX_BZ2E_HEAD_BITS;
        uint32_t c = 0;
        for (; b < blocks.size() && blocks[b].file == f; b++) {
            bit_off[b] = at;
            at += bits[b];
            c = ((c << 1) | (c >> 31)) ^ crc[b];
        }
        F.count = (uint32_t)b - F.first;
        F.crc = c;
        F.bits = at + RCX_BZ2E_TAIL_BITS;
        F.out_len = (F.bits + 7) / 8;
        F.status = F.out_len <= out_cap[f] ? RCX_OK : RCX_E_OUTPUT_TOO_SMALL;
    }
}
// what a block's bits take at the most, in bytes with the slack the packer's and the joiner's word accesses need: 17 bits a symbol (the
// block's bytes and the end symbol), a selector of 6 bits per 50 symbols, six tables of 258 delta-coded lengths, the fixed fields
inline uint64_t rcx_plan_bz2e_block_bound(uint32_t n)
{
    const uint64_t nsym = (uint64_t)n + 1, nsel = (nsym + 49) / 50;
    const uint64_t bits = 17 * nsym + 6 * nsel + 6ull * (5 + 258 * 33) + 48 + 32 + 1 + 24 + 16 + 256 + 3 + 15;
    return ((bits + 31) / 32) * 4 + 16;
}

// ---- Zstandard decode (rcx_zstd_decode_batch, k_zstd.hip) ---------------------------------------------------------
// One persistent wave per file, RCX_ZSTD_MAX_WAVES at the most, each with a buffer for one block's literals in the scratch.  The
// dictionaries are raw content, ranges anywhere in the input buffer: rcx_plan_dict's words with the lengths unclamped (an offset reaches
// as far as the frame's own output and the dictionary go); both arrays null: no file has one, and the words say so.
// Pure host code (tests/host_plan/test_plan_zstd.cpp).
#define RCX_ZSTD_MAX_FILES 65535u
#define RCX_ZSTD_MAX_WAVES 2048u
#define RCX_ZSTD_LIT_SLOT (131072u + 64u)
struct rcx_zstd_plan {
    rcx_dict_plan dict;                       // aux: RCX_DICT_WORDS a file
    uint32_t waves = 0;
    uint64_t scratch_bytes = 0;
};
// false: `err` names what is wrong.  n > 0.
inline bool rcx_plan_zstd(uint32_t n, const uint64_t* dict_off, const uint64_t* dict_len, rcx_zstd_plan& p, std::string& err)
{
    p = rcx_zstd_plan();
    if (n > RCX_ZSTD_MAX_FILES) { err = "zstd decode: at most 65535 files a call"; return false; }
    if (!dict_off != !dict_len) { err = "zstd decode: dict_off and dict_len come together or not at all"; return false; }
    const std::vector<uint64_t> none(dict_len ? 0 : n, 0);
    if (!rcx_plan_dict(n, dict_len ? dict_off : none.data(), dict_len ? dict_len : none.data(), 0xffffffffull, 0xffffffffull, nullptr,
                       "zstd decode", p.dict, err))
        return false;
    p.waves = n < RCX_ZSTD_MAX_WAVES ? n : RCX_ZSTD_MAX_WAVES;
    p.scratch_bytes = (uint64_t)p.waves * RCX_ZSTD_LIT_SLOT;
    return true;
}
// The size query and the retry: the files of a first call that must be decoded again, with the capacity each one asked for.  A file that
// reported RCX_E_OUTPUT_TOO_SMALL names its exact size in out_len; every other file is final.
inline std::vector<std::pair<uint32_t, uint64_t>> rcx_plan_zstd_retry(uint32_t n, const int32_t* status, const uint64_t* out_len)
{
    std::vector<std::pair<uint32_t, uint64_t>> r;
    for (uint32_t i = 0; i < n; i++) if (status[i] == RCX_E_OUTPUT_TOO_SMALL) r.emplace_back(i, out_len[i]);
    return r;
}
