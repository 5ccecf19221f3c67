// k_lz4_dict.hip -- LZ4 block decode behind SHARED DICTIONARIES: block b's history is a range anywhere in the INPUT buffer
// (rcx_lz4_decode_shared_batch, include/rcx.h), not the bytes in front of its slot.  What it computes is what k_lz4_linked.hip computes
// for the same block (link 0) with the same dictionary bytes copied directly in front of the slot: bytes, out_len, in_used, status.
// NOT a function of the reference crate; the block format, the checks and their precedence are BlockDecoder::decode's (src/lz4.rs:67-110,
// restated in oracle/o_lz4.c) with the dictionary counted into what an offset may reach.
//
// Lz4V4 reads its own output through `out` (repair, wide_match, solo, emit), which is what makes history in front of the slot free for
// k_lz4_linked and a history elsewhere impossible, and it is one of the headline kernel's sources.  So this is a decoder of its own, the
// DIRECT form: ONE WAVE PER BLOCK, nothing kept in LDS, two byte sources.
//   parse     wave-uniform.  The wave holds 64 input bytes in a register window (lane l: in[wbase + l]); token, extended lengths and
//             offset are read from it with v_readlane, and the window is loaded again where the cursor leaves it (once per ~64 input
//             bytes, or behind a run of literals that skipped past its end).
//   copy      literals and match of a sequence are ONE 64-lane copy over L + M destination bytes: destination byte i < L is the
//             literal in[lit + i]; byte L + j is the byte q = offset - (j mod offset) behind the match's destination in the VIRTUAL
//             stream dictionary || output.  j mod offset (period handling where offset < length) keeps q >= 1: bytes that existed
//             before the match began.
//               q <= L                  one of THIS sequence's literals: in[lit + L - q], read from the input instead of waiting for
//                                       the literal's store
//               q - L <= oend           out[oend - (q - L)], stored by an earlier sequence
//               beyond that             dict[D - (q - L - oend)]: the split may fall inside one match, lane by lane; a source that
//                                       runs past the dictionary's last byte goes on at the slot's first byte, never in what follows
//                                       the dictionary in memory
//             so no load of a sequence depends on a store of the same sequence, and a source wholly in the dictionary or in this
//             sequence's literals depends on no earlier output at all.
//   ordering  a byte of out[] that another lane stored in an earlier sequence must be visible to the lane that loads it.  `settled`
//             is the output length up to which the wave has waited for its stores; a match whose source in out[] ends above it
//             executes s_waitcnt vmcnt(0) (RCX_WAIT_VMEM: every store of the wave has been acknowledged by the L2, which every CU's
//             loads of lines it has not cached are served from; the CU's own L1 is write-through and sees its own stores in order)
//             between rcx_wave_sync()s, which keep the compiler from moving the loads across it.  Records behind a large dictionary
//             take most sources from the dictionary and seldom wait.
// Nothing below the slot is dereferenced (out_off may be 0, or less than D), nothing outside [out_off, out_off + out_cap) is written,
// no byte outside [dict, dict + D) is loaded on the dictionary's behalf.
// STATUS (o_lz4.c): an extended length or an offset that runs off the input, literals longer than the input left, an offset of 0 or
// beyond mdst + D: RCX_E_MALFORMED; literals or a match beyond the slot: RCX_E_OUTPUT_TOO_SMALL, in the reference's order (literal
// checks, offset checks, match length).  out_len is 0 on failure, in_used = in_len.  A failed block may have written earlier sequences
// into its slot.
//
// aux: the words of rcx_plan_dict (rcx_plan.h, laid out by lz_dict.h): aux[b] = D (at most 65535 after the clamp), aux[3n + b] /
// aux[4n + b] = the dictionary's offset from in_base.  The dictionary index and the per-dictionary words are not read.
#pragma once
#include "rcx_dev.h"

struct Lz4Dict {
    const uint8_t* in; uint32_t n;
    uint8_t* out; uint32_t cap;
    const uint8_t* dict; uint32_t D;
    uint32_t lane;
    uint32_t wv, wbase; bool wok;          // the input window: lane l holds in[wbase + l]

    // in[pos], wave-uniform; pos < n
    __device__ __forceinline__ uint32_t peek(uint32_t pos)
    {
        if (!wok || pos - wbase >= 64u) {
            wbase = pos; wok = true;
            wv = pos + lane < n ? (uint32_t)in[pos + lane] : 0u;
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)RCX_UNI(pos - wbase));
    }
    // length(), lz4.rs:112-122: the bytes behind a 15; false: the input ran out
    __device__ __forceinline__ bool more(uint32_t& cur, uint64_t& len)
    {
        for (;;) {
            if (cur >= n) return false;
            const uint32_t x = peek(cur); cur++;
            len += x;
            if (x != 255u) return true;
        }
    }

    __device__ int run(uint32_t* len_out)
    {
        lane = rcx_lane();
        wok = false; wv = 0; wbase = 0;
        uint32_t cur = 0, oend = 0, settled = 0;
        while (cur < n) {                                                  // :68
            const uint32_t code = peek(cur); cur++;                        // :69
            uint64_t L = code >> 4;                                        // :73
            if (L == 15u && !more(cur, L)) return RCX_E_MALFORMED;
            if (L > (uint64_t)(n - cur)) return RCX_E_MALFORMED;           // :75-85 reads past the input slice
            if (L > (uint64_t)(cap - oend)) return RCX_E_OUTPUT_TOO_SMALL;
            const uint32_t lit = cur, l = (uint32_t)L;
            cur += l;
            uint32_t off = 1, m = 0;
            if (cur < n) {                                                 // :87
                if (n - cur < 2u) return RCX_E_MALFORMED;
                off = peek(cur); off |= peek(cur + 1) << 8;                // :91
                cur += 2;
                if ((uint64_t)off > (uint64_t)oend + l + D || off == 0) return RCX_E_MALFORMED;   // :93
                uint64_t M = code & 15u;                                   // :98
                if (M == 15u && !more(cur, M)) return RCX_E_MALFORMED;
                M += 4;                                                    // :100-106
                if (M > (uint64_t)(cap - oend - l)) return RCX_E_OUTPUT_TOO_SMALL;
                m = (uint32_t)M;
            }
            // A source byte is q = offset - (j mod offset) bytes behind the match's destination (1 <= q <= offset <= 65535: written as
            // distances, nothing here can wrap): q <= l this sequence's literals, q - l <= oend out[], beyond that the dictionary.
            if (m && off > l && oend > settled) {
                const uint32_t span = off < m ? off : m;                   // the distinct source bytes
                const uint32_t qmin = off - span + 1;                      // the one closest to the destination ...
                const uint32_t back = qmin > l ? qmin - l : 1u;            // ... or the last byte of out[]: its distance behind oend
                if (back <= oend && oend - back >= settled) {              // in out[] above what the wave has waited for
                    rcx_wave_sync();
                    RCX_WAIT_VMEM();
                    rcx_wave_sync();
                    settled = oend;
                }
            }
            const uint32_t total = l + m;
            #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t i = lane; i < total; i += 64) {
                uint8_t x;
                if (i < l) x = in[lit + i];
                else {
                    uint32_t j = i - l;
                    if (off < m) j %= off;
                    const uint32_t q = off - j;
                    if (q <= l) x = in[lit + l - q];
                    else if (q - l <= oend) x = out[oend - (q - l)];
                    else x = dict[D - (q - l - oend)];
                }
                out[oend + i] = x;
            }
            oend += total;
        }
        *len_out = oend;
        return RCX_OK;
    }
};

__global__ __launch_bounds__(64) void k_lz4_decode_dict(rcx_kargs a)
{
    const uint32_t b = blockIdx.x;
    const uint64_t n = a.nblocks;
    if (b >= n) return;
    Lz4Dict s;
    s.in = a.in_base + a.in_off[b];
    s.n = (uint32_t)a.in_len[b];
    s.out = a.out_base + a.out_off[b];
    const uint64_t cap64 = a.out_cap[b];
    s.cap = cap64 > 0xffffffffull ? 0xffffffffu : (uint32_t)cap64;
    s.D = a.aux[b] < 65535u ? a.aux[b] : 65535u;                           // (an offset has 16 bits)
    s.dict = a.in_base + ((uint64_t)a.aux[3 * n + b] | ((uint64_t)a.aux[4 * n + b] << 32));
    uint32_t olen = 0;
    const int st = s.run(&olen);
    if ((threadIdx.x & 63u) == 0) {
        a.status[b] = st;
        a.out_len[b] = st ? 0u : olen;
        if (a.in_used) a.in_used[b] = s.n;
    }
}

// k.aux: the words of rcx_plan_dict, never null
static void launch_lz4_decode_dict(hipStream_t s, rcx_kargs& k)
{
    hipLaunchKernelGGL(k_lz4_decode_dict, dim3(k.nblocks), dim3(64), 0, s, k);
}
