// k_lz4_linked.hip -- LZ4 block decode with HISTORY: linked blocks (the LZ4 frame format's default, block-dependent mode) and
// dictionaries.  rcx_lz4_decode_linked_batch (include/rcx.h); NOT a function of the reference crate, whose frame decoder breaks on
// dependent blocks.
//
// A chain of linked blocks is serial: block i's output position and its history exist only when block i-1 is done.  Chains are
// independent.  So the batch runs in ROUNDS: round r is one launch over the blocks at depth r of their chains (the host sorts the block
// indices by depth, rcx_api.hip), the rounds are ordered by the stream, and a block reads where its predecessor started (eff), how
// much it produced (out_len) and whether it failed (status) from device memory.  A batch costs as many launches as its longest chain.
//
// The decoder is k_lz4_decode_v4's (one wave per block), started in the middle: `out` points at the FIRST HISTORY BYTE (what the chain
// has produced so far plus the head's dictionary, at most 64 KiB back), the block's own bytes begin `hist` bytes further on and `cap`
// counts from `out` too.  Positions stay offsets from `out`, so the bound of a match (off > mdst) is produced + history as it stands,
// and a match into the history is what a match into bytes drained long ago always was: a gather from HBM.  Nothing below out + hist
// is written: the drain starts there.  Lz4V4 itself is not changed, only its run() is restated here with that start.
// KNOWN COST: run_from() below repeats Lz4V4::run()'s loop (without the profiling lines), so a fix to one must be made in the other.
// A defaulted `hist` argument on run() would avoid that, but k_lz4_decode_v4.hip is one of the headline kernel's sources: bench.py
// quotes the measured HBM traffic of profiles/pmc_lz4_decode.json only while the hash of those files is the one it was measured on,
// and the headline decoders (k_lz4_decode_v5 / _v8) build on that struct.  Fold the two together when that figure is next re-measured.
// MEASURED on MI355X (benchmarks/lz4_frame_rate.py, device-resident, median of 10 calls): 4096 independent 64 KiB text
// blocks 0.943 ms a call (265 GiB/s; the two-wave headline decoder 0.501 ms on the same blocks), 256 chains of 16 linked blocks
// 10.1 ms (24.7 GiB/s): a round of 256 blocks takes what one wave needs for one block, 0.63 ms.
#pragma once
#include "k_lz4_decode_v4.hip"

template <int CB>
struct Lz4Linked : Lz4V4<CB> {
    typedef Lz4V4<CB> B;
    // Lz4V4::run with `hist` bytes of history in front of the block; *len_out = the block's own bytes
    __device__ void run_from(int32_t* st_out, uint32_t* len_out, uint32_t hist)
    {
        this->lane = rcx_lane();
        this->init_window();
        if (hist) {                                            // as after a wave-wide copy: everything so far is in HBM, its last RH bytes in the window too
            this->oend = RCX_U(hist); this->gflush = this->oend; this->mflush = this->oend;
            this->repair();
        }
        int st = RCX_OK;
        uint32_t cur = 0;
        if (this->n) this->stage(0); else { this->cbase = 0; this->cend = 0; }
        uint32_t s_L = 0, s_M = 0, s_off = 0, s_src = 0;
        for (;;) {
            const typename B::Batch bt = this->collect(cur, s_L, s_M, s_off, s_src);
            rcx_wave_sync();
            int lo = 0, e = 0;
            while (lo < bt.ns && !e) e = this->emit(bt.ns, lo, s_L, s_M, s_off, s_src);
            if (e) { st = e; break; }
            if (bt.why == B::STAGE_) { this->stage(cur); continue; }
            if (this->after_batch(bt, st)) break;
            if (bt.why == B::SOLO_ || bt.why == B::WIDE_) cur = bt.gnext;
        }
        if (!st) this->flush(this->oend, true);
        *st_out = st;
        *len_out = st ? 0u : this->oend - hist;
    }
};

template <int CB>
__global__ __launch_bounds__(64) void k_lz4_decode_linked(rcx_kargs a, const uint32_t* order, uint32_t count, const uint32_t* head,
                                                          const uint32_t* dict, uint64_t* eff)
{
    typedef Lz4Linked<CB> S;
    __shared__ __align__(16) uint8_t s_cbuf[CB + 96];
    __shared__ __align__(16) uint8_t s_wbuf[S::WBUF + 16];
    __shared__ uint32_t s_epos[64];
    if (blockIdx.x >= count) return;
    const uint32_t b = order[blockIdx.x];
    const uint32_t h = head[b];
    const uint64_t slot0 = a.out_off[h], slot_end = slot0 + a.out_cap[h];
    uint64_t start = slot0;
    if (h != b) {                                              // continues block b - 1 (decoded by the launch before this one)
        if (a.status[b - 1] != RCX_OK) {
            if ((threadIdx.x & 63u) == 0) {
                a.status[b] = RCX_E_LZ4_HISTORY; a.out_len[b] = 0; eff[b] = eff[b - 1];
                if (a.in_used) a.in_used[b] = 0;
            }
            return;
        }
        start = eff[b - 1] + a.out_len[b - 1];
    }
    uint64_t hist = start - slot0 + dict[h];
    if (hist > 65536u) hist = 65536u;                          // (an offset has 16 bits)
    const uint64_t cap64 = hist + (slot_end - start);
    S s;
    s.in = a.in_base + a.in_off[b];
    s.n = (uint32_t)a.in_len[b];
    s.out = a.out_base + (start - hist);
    s.cap = cap64 > 0xffffffffull ? 0xffffffffu : (uint32_t)cap64;
    s.cbuf = s_cbuf;
    s.wb_ = s_wbuf;
    s.epos = s_epos;
    int32_t st; uint32_t olen;
    s.run_from(&st, &olen, (uint32_t)hist);
    if ((threadIdx.x & 63u) == 0) {
        a.status[b] = st;
        a.out_len[b] = olen;
        eff[b] = start;
        if (a.in_used) a.in_used[b] = s.n;
    }
}

// rounds_off: HOST array of nrounds + 1 entries into `order`; everything else lives on the device
static void launch_lz4_decode_linked(hipStream_t s, rcx_kargs& k, const uint32_t* order, const uint32_t* rounds_off, uint32_t nrounds,
                                     const uint32_t* head, const uint32_t* dict, uint64_t* eff)
{
    for (uint32_t r = 0; r < nrounds; r++) {
        const uint32_t cnt = rounds_off[r + 1] - rounds_off[r];
        if (cnt) hipLaunchKernelGGL((k_lz4_decode_linked<1024>), dim3(cnt), dim3(64), 0, s, k, order + rounds_off[r], cnt, head, dict, eff);
    }
}
