// sim_deflate_hc.cpp -- runs the UNMODIFIED DEFLATE encoder kernels of every level (k_deflate_encode.hip, k_deflate_hc.hip) on the
// wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_deflate_hc_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_deflate_hc/sim_deflate_hc.cpp tests/wavesim/wavesim.cpp
#include <string>
#define hipStream_t int
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
// every launch is counted; the launches past g_stop_after are skipped (sim_deflate_hc_stages: the scratch as it stands after a stage)
static uint32_t g_launches = 0, g_stop_after = 0xffffffffu;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { if (g_launches++ < g_stop_after) ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); } while (0)
#include "../../rust_compress_amd/csrc/k_inflate.hip"
#include "../../rust_compress_amd/csrc/k_crc32.hip"
#include "../../rust_compress_amd/csrc/k_deflate_encode.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc.hip"

// fmt: 0 raw DEFLATE, 1 zlib, 2 gzip; level 1..9.  Scratch: what the library's level batch path allocates, or `scratch_bytes` when not
// 0 (contents not zero: filled with 0xA5).
static int run_level(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                     const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t n,
                     uint8_t* scratch, uint64_t sb, uint32_t stop_after)
{
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n;
    k.scratch = scratch; k.scratch_bytes = sb;
    std::string err;
    g_launches = 0; g_stop_after = stop_after;
    const int rc = launch_deflate_level(0, k, fmt, level, err, fmt == DE_GZIP ? launch_crc32 : launch_adler32);
    g_stop_after = 0xffffffffu;
    if (rc) fprintf(stderr, "sim_deflate_hc: %s\n", err.c_str());
    return rc;
}

extern "C" int sim_deflate_hc_encode(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                                     const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                                     int32_t* status, uint32_t n, uint64_t scratch_bytes)
{
    uint64_t segs = 0;
    for (uint32_t i = 0; i < n; i++) segs += (in_len[i] + DE_SEG - 1) / DE_SEG;
    const uint64_t sb = scratch_bytes ? scratch_bytes : dh_scratch_bytes(n, segs);
    std::vector<uint8_t> scratch(sb + 64, 0xA5);
    return run_level(fmt, level, in, in_off, in_len, out, out_off, out_cap, out_len, in_used, status, n, scratch.data(), sb, 0xffffffffu);
}

// The byte offsets, from `base`, of the stage arrays that dh_carve / de_carve place in a scratch of `bytes` bytes at the ADDRESS `base`
// for n streams (the carve aligns relative to the address, so the layout of a device scratch comes from its device address; nothing is
// read or run).  layout: link cand elen price pos seg_first seg_type seg_bits cap.
extern "C" void sim_deflate_hc_layout(uint64_t base, uint64_t bytes, uint32_t n, uint64_t* layout)
{
    DhScratch h;
    const DeScratch d = dh_carve((void*)(uintptr_t)base, bytes, n, h);
    const uint8_t* b = (const uint8_t*)(uintptr_t)base;
    layout[0] = (uint64_t)((const uint8_t*)h.link - b); layout[1] = (uint64_t)((const uint8_t*)h.cand - b);
    layout[2] = (uint64_t)((const uint8_t*)h.elen - b); layout[3] = (uint64_t)(h.price - b);
    layout[4] = (uint64_t)((const uint8_t*)d.pos - b); layout[5] = (uint64_t)((const uint8_t*)d.seg_first - b);
    layout[6] = (uint64_t)((const uint8_t*)d.seg_type - b); layout[7] = (uint64_t)((const uint8_t*)d.seg_bits - b);
    layout[8] = d.cap;
}

// sim_deflate_hc_encode in the caller's scratch (`scratch_bytes` bytes at `scratch`, what the caller filled it with), of which only the
// first `stop_after` kernel launches run (k_de_plan is the first; 0xffffffff: all): the stage arrays as that launch left them.
extern "C" int sim_deflate_hc_stages(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                                     const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                                     int32_t* status, uint32_t n, uint32_t stop_after, uint8_t* scratch, uint64_t scratch_bytes,
                                     uint64_t* layout)
{
    sim_deflate_hc_layout((uint64_t)(uintptr_t)scratch, scratch_bytes, n, layout);
    return run_level(fmt, level, in, in_off, in_len, out, out_off, out_cap, out_len, in_used, status, n, scratch, scratch_bytes, stop_after);
}

// what the library's level batch path allocates for n streams of `segs` segments in all
extern "C" uint64_t sim_deflate_hc_scratch_bytes(uint32_t n, uint64_t segs) { return dh_scratch_bytes(n, segs); }
