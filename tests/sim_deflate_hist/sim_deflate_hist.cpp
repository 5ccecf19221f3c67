// sim_deflate_hist.cpp -- runs the UNMODIFIED DEFLATE encoder and decoder with history (k_deflate_hc_hist.hip behind k_deflate_hc.hip,
// k_inflate_hist.hip behind k_inflate2.hip) on the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by
// tests/sim_deflate_hist_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_deflate_hist/sim_deflate_hist.cpp tests/wavesim/wavesim.cpp
#include <string>
#define hipStream_t int
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
// every launch is counted; the launches past g_stop_after are skipped (the scratch as it stands after a stage)
static uint32_t g_launches = 0, g_stop_after = 0xffffffffu;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { if (g_launches++ < g_stop_after) ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); } while (0)
#include "../../rust_compress_amd/csrc/k_inflate.hip"
#include "../../rust_compress_amd/csrc/k_inflate2.hip"
#include "../../rust_compress_amd/csrc/k_inflate_hist.hip"
#include "../../rust_compress_amd/csrc/k_crc32.hip"
#include "../../rust_compress_amd/csrc/k_deflate_encode.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc_hist.hip"

// what the library's batch path allocates for n blocks of `segs` segments in all, `nhist` of them with history
extern "C" uint64_t sim_deflate_hist_scratch_bytes(uint32_t n, uint64_t segs, uint64_t nhist) { return dh_hist_scratch_bytes(n, segs, nhist); }

// The byte offsets, from `base`, of the stage arrays that dh_hist_carve places in a scratch of `bytes` bytes at the ADDRESS `base`
// (nothing is read or run).  layout: link cand elen price pos seg_first seg_type seg_bits cap hslot end.
extern "C" void sim_deflate_hist_layout(uint64_t base, uint64_t bytes, uint32_t n, uint32_t nhist, uint64_t* layout)
{
    DhScratch h;
    DhHist hh;
    const DeScratch d = dh_hist_carve((void*)(uintptr_t)base, bytes, n, nhist, h, hh);
    const uint8_t* b = (const uint8_t*)(uintptr_t)base;
    layout[0] = (uint64_t)((const uint8_t*)h.link - b); layout[1] = (uint64_t)((const uint8_t*)h.cand - b);
    layout[2] = (uint64_t)((const uint8_t*)h.elen - b); layout[3] = (uint64_t)(h.price - b);
    layout[4] = (uint64_t)((const uint8_t*)d.pos - b); layout[5] = (uint64_t)((const uint8_t*)d.seg_first - b);
    layout[6] = (uint64_t)((const uint8_t*)d.seg_type - b); layout[7] = (uint64_t)((const uint8_t*)d.seg_bits - b);
    layout[8] = d.cap; layout[9] = (uint64_t)((const uint8_t*)hh.hslot - b);
    layout[10] = (uint64_t)((const uint8_t*)(h.link + ((uint64_t)d.cap + nhist) * DE_SEG) - b);   // one past the link array, the carve's last
}

// The encode (fmt 0 raw, 1 zlib) at `level` in the caller's scratch (`scratch_bytes` bytes at `scratch`, what the caller filled it
// with), of which only the first `stop_after` kernel launches run (0xffffffff: all).  aux: n history lengths as the kernels get them
// (uint32) and, zlib, n DICTIDs behind them; or null.
extern "C" int sim_deflate_hist_stages(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t* aux,
                                       uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                                       int32_t* status, uint32_t n, uint32_t nhist, uint32_t stop_after, uint8_t* scratch,
                                       uint64_t scratch_bytes, uint64_t* layout)
{
    sim_deflate_hist_layout((uint64_t)(uintptr_t)scratch, scratch_bytes, n, nhist, layout);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = aux;
    k.scratch = scratch; k.scratch_bytes = scratch_bytes;
    std::string err;
    g_launches = 0; g_stop_after = stop_after;
    const int rc = launch_deflate_hist(0, k, fmt, level, nhist, err, launch_adler32);
    g_stop_after = 0xffffffffu;
    if (rc) fprintf(stderr, "sim_deflate_hist: %s\n", err.c_str());
    return rc;
}

// The decode: hist 1 -- k_inflate_hist (aux: n history lengths, then n DICTIDs when zlib; the flags come back in the first n);
// hist 0 -- k_inflate2 as launch_inflate2 launches it (aux: the flags).
extern "C" int sim_inflate_hist(int hist, int zlib, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t* aux,
                                uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                                int32_t* status, uint32_t n)
{
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = aux;
    g_launches = 0; g_stop_after = 0xffffffffu;
    if (hist) launch_inflate_hist(0, k, zlib != 0);
    else launch_inflate2(0, k, zlib ? 1 : 0, 0);
    return 0;
}
