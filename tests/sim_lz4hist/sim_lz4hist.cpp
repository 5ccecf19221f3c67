// sim_lz4hist.cpp -- runs the UNMODIFIED LZ4 HC encoder with history (k_lz4_hc.hip + k_lz4_hc_hist.hip) on the wave64 simulator of
// tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_lz4hist_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_lz4hist/sim_lz4hist.cpp tests/wavesim/wavesim.cpp
#include <string>
#define hipStream_t int
// every launch is counted; the launches past g_stop_after are skipped (the scratch as it stands after a stage)
static uint32_t g_launches = 0, g_stop_after = 0xffffffffu;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { if (g_launches++ < g_stop_after) ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); } while (0)
#include "../../rust_compress_amd/csrc/k_lz4_hc.hip"
#include "../../rust_compress_amd/csrc/k_lz4_hc_hist.hip"

// what the library's batch path allocates for n blocks of `segs` segments in all, `nhist` of them with history
extern "C" uint64_t sim_lz4hist_scratch_bytes(uint32_t n, uint64_t segs, uint64_t nhist) { return hc_hist_scratch_bytes(n, segs, nhist); }

// The byte offsets, from `base`, of the stage arrays that hc_hist_carve places in a scratch of `bytes` bytes at the ADDRESS `base`
// (nothing is read or run).  layout: link cand elen seg_first seg_nm seg_fm seg_le cap hslot.
extern "C" void sim_lz4hist_layout(uint64_t base, uint64_t bytes, uint32_t n, uint32_t nhist, uint64_t* layout)
{
    HcHist h;
    const HcScratch d = hc_hist_carve((void*)(uintptr_t)base, bytes, n, nhist, h);
    const uint8_t* b = (const uint8_t*)(uintptr_t)base;
    layout[0] = (uint64_t)((const uint8_t*)d.link - b); layout[1] = (uint64_t)((const uint8_t*)d.cand - b);
    layout[2] = (uint64_t)((const uint8_t*)d.elen - b); layout[3] = (uint64_t)((const uint8_t*)d.seg_first - b);
    layout[4] = (uint64_t)((const uint8_t*)d.seg_nm - b); layout[5] = (uint64_t)((const uint8_t*)d.seg_fm - b);
    layout[6] = (uint64_t)((const uint8_t*)d.seg_le - b); layout[7] = d.cap;
    layout[8] = (uint64_t)((const uint8_t*)h.hslot - b);
}

// The encode at `level` in the caller's scratch (`scratch_bytes` bytes at `scratch`, what the caller filled it with), of which only the
// first `stop_after` kernel launches run (0xffffffff: all).  hist: n history lengths as the kernels get them (uint32), or null.
extern "C" int sim_lz4hist_stages(int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t* hist, uint8_t* out,
                                  const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status,
                                  uint32_t n, uint32_t nhist, uint32_t stop_after, uint8_t* scratch, uint64_t scratch_bytes, uint64_t* layout)
{
    sim_lz4hist_layout((uint64_t)(uintptr_t)scratch, scratch_bytes, n, nhist, layout);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = hist;
    k.scratch = scratch; k.scratch_bytes = scratch_bytes;
    std::string err;
    g_launches = 0; g_stop_after = stop_after;
    const int rc = launch_lz4_hc_hist(0, k, level, nhist, err);
    g_stop_after = 0xffffffffu;
    if (rc) fprintf(stderr, "sim_lz4hist: %s\n", err.c_str());
    return rc;
}
