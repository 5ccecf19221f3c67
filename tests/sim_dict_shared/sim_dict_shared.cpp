// sim_dict_shared.cpp -- runs the UNMODIFIED encoders behind shared dictionaries (k_lz4_hc_dict.hip behind k_lz4_hc.hip; k_deflate_hc_dict.hip
// behind k_deflate_hc.hip and k_deflate_hc_hist.hip) and the host's rcx_plan_dict on the wave64 simulator of tests/wavesim (TEST
// INFRASTRUCTURE).  Built twice by tests/sim_dict_shared_run.py, once per family (-DSIM_LZ4 / -DSIM_DEFLATE), with
//   g++ -include tests/wavesim/wavesim.h tests/sim_dict_shared/sim_dict_shared.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#define hipStream_t int
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
// every launch is counted; the launches past g_stop_after are skipped (the scratch as it stands after a stage)
static uint32_t g_launches = 0, g_stop_after = 0xffffffffu;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { if (g_launches++ < g_stop_after) ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); } while (0)
#include "../../rust_compress_amd/csrc/rcx_plan.h"
#ifdef SIM_LZ4
#include "../../rust_compress_amd/csrc/k_lz4_hc.hip"
#include "../../rust_compress_amd/csrc/k_lz4_hc_dict.hip"
#define SIM_SEG HC_SEG
#else
#include "../../rust_compress_amd/csrc/k_inflate.hip"
#include "../../rust_compress_amd/csrc/k_crc32.hip"
#include "../../rust_compress_amd/csrc/k_deflate_encode.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc_hist.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc_dict.hip"
#define SIM_SEG DE_SEG
#endif

// The encode at `level` (fmt 0 raw DEFLATE, 1 zlib with dict_id; LZ4: ignored) of n blocks behind the dictionaries dict_off / dict_len
// (as the C ABI takes them), in a scratch of the size the library's batch path allocates, filled with `fill`; only the first
// `stop_after` kernel launches run (0xffffffff: all).  cand (or null): the candidate word of every input position, the blocks' one after
// the other (valid when the run stopped behind the search; DEFLATE's later launches leave it alone).  info: ndict, scratch bytes, the
// plan's span.  -1: the plan refused (stderr has the text).
extern "C" int sim_dict_shared(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint64_t* dict_off,
                               const uint64_t* dict_len, const uint32_t* dict_id, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                               uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t n, uint32_t stop_after, int fill, uint32_t* cand,
                               uint64_t* info)
{
    rcx_dict_plan plan;
    std::string err;
#ifdef SIM_LZ4
    const uint64_t max_dict = 65536, reach = 65535;
#else
    const uint64_t max_dict = 32768, reach = 32768;
#endif
    if (!rcx_plan_dict(n, dict_off, dict_len, max_dict, reach, fmt ? dict_id : nullptr, "sim", plan, err)) { fprintf(stderr, "sim_dict_shared: %s\n", err.c_str()); return -1; }
    uint64_t segs = 0;
    for (uint32_t i = 0; i < n; i++) segs += (in_len[i] + SIM_SEG - 1) / SIM_SEG;
#ifdef SIM_LZ4
    const uint64_t sb = hc_dict_scratch_bytes(n, segs, plan.ndict);
#else
    const uint64_t sb = dh_dict_scratch_bytes(n, segs, plan.ndict);
#endif
    std::vector<uint8_t> scratch(sb + 64, (uint8_t)fill);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = plan.aux.data();
    k.scratch = scratch.data() + 1; k.scratch_bytes = sb;              // (an unaligned scratch, as any caller's may be)
    g_launches = 0; g_stop_after = stop_after;
    uint8_t* rest;
#ifdef SIM_LZ4
    const int rc = launch_lz4_hc_dict(0, k, level, plan.ndict, err);
    (void)lzd_carve(k.scratch, n, plan.ndict, HC_DSLOT, &rest);
    const HcScratch d = hc_carve(rest, sb - (uint64_t)(rest - (uint8_t*)k.scratch), n);
    const uint32_t* c0 = d.cand;
#else
    const int rc = launch_deflate_dict(0, k, fmt ? DE_ZLIB : DE_RAW, level, plan.ndict, err, launch_adler32);
    (void)lzd_carve(k.scratch, n, plan.ndict, DH_DSLOT, &rest);
    DhScratch h;
    const DeScratch d = dh_carve(rest, sb - (uint64_t)(rest - (uint8_t*)k.scratch), n, h);
    const uint32_t* c0 = h.cand;
#endif
    g_stop_after = 0xffffffffu;
    if (rc) { fprintf(stderr, "sim_dict_shared: %s\n", err.c_str()); return rc; }
    info[0] = plan.ndict; info[1] = sb; info[2] = plan.span;
    if (cand) {
        uint64_t at = 0;
        for (uint32_t b = 0; b < n; b++) {
            const uint32_t f0 = d.seg_first[b], f1 = d.seg_first[b + 1];
            for (uint64_t p = 0; p < in_len[b]; p++) cand[at + p] = f1 > f0 && f1 <= d.cap ? c0[(uint64_t)f0 * SIM_SEG + p] : 0u;
            at += in_len[b];
        }
    }
    return 0;
}
