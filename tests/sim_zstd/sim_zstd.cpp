// sim_zstd.cpp -- runs the UNMODIFIED Zstandard decoder (rust_compress_amd/csrc/k_zstd.hip with k_xxh64.hip) and the host's rcx_plan_zstd
// on the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_zstd_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_zstd/sim_zstd.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#define RCX_AB_VARIANTS 1            /* the executor built first (variant 2) runs here beside the shipped form */
#define hipStream_t int
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) ws::launch(grid, block, [&] { kern(__VA_ARGS__); })
#include "../../rust_compress_amd/csrc/rcx_plan.h"
#include "../../rust_compress_amd/csrc/k_zstd.hip"

// One call over n files behind the dictionaries dict_off / dict_len (as the C ABI takes them, or both null), with `waves` persistent
// waves (0: the plan's) and the scratch the library's batch path allocates, filled with 0xA5.  info: waves, scratch bytes, the plan's
// span.  -1: the plan refused (err has the text).
static int g_variant = 0;
extern "C" void sim_zstd_variant(int v) { g_variant = v; }

extern "C" int sim_zstd_decode(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint64_t* dict_off, const uint64_t* dict_len,
                               uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                               int32_t* status, uint32_t n, uint32_t waves, uint64_t* info, char* err, uint32_t err_cap)
{
    rcx_zstd_plan plan;
    std::string e;
    if (!rcx_plan_zstd(n, dict_off, dict_len, plan, e)) { snprintf(err, err_cap, "%s", e.c_str()); return -1; }
    if (waves && waves < plan.waves) plan.waves = waves;
    std::vector<uint8_t> scratch(plan.scratch_bytes + 64, 0xA5);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = plan.dict.aux.data();
    k.scratch = scratch.data() + 1; k.scratch_bytes = plan.scratch_bytes;         // (an unaligned scratch, as any caller's may be)
    const int rc = launch_zstd_decode(0, k, plan.waves, g_variant, e);
    if (rc) { snprintf(err, err_cap, "%s", e.c_str()); return rc; }
    info[0] = plan.waves; info[1] = plan.scratch_bytes; info[2] = plan.dict.span;
    return 0;
}

extern "C" int sim_xxh64(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint64_t seed, uint64_t* hash)
{
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_len = hash; k.nblocks = n;
    launch_xxh64(0, k, seed);
    return 0;
}
