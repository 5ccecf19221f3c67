// sim_deflate_hc.cpp -- runs the UNMODIFIED DEFLATE encoder kernels of every level (k_deflate_encode.hip, k_deflate_hc.hip) on the
// wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_deflate_hc_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_deflate_hc/sim_deflate_hc.cpp tests/wavesim/wavesim.cpp
#include <string>
#define hipStream_t int
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) ws::launch(grid, block, [&] { kern(__VA_ARGS__); })
#include "../../rust_compress_amd/csrc/k_inflate.hip"
#include "../../rust_compress_amd/csrc/k_crc32.hip"
#include "../../rust_compress_amd/csrc/k_deflate_encode.hip"
#include "../../rust_compress_amd/csrc/k_deflate_hc.hip"

// fmt: 0 raw DEFLATE, 1 zlib, 2 gzip; level 1..9.  Scratch: what the library's level batch path allocates, or `scratch_bytes` when not
// 0 (contents not zero: filled with 0xA5).
extern "C" int sim_deflate_hc_encode(int fmt, int level, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                                     const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used,
                                     int32_t* status, uint32_t n, uint64_t scratch_bytes)
{
    uint64_t segs = 0;
    for (uint32_t i = 0; i < n; i++) segs += (in_len[i] + DE_SEG - 1) / DE_SEG;
    const uint64_t sb = scratch_bytes ? scratch_bytes : dh_scratch_bytes(n, segs);
    std::vector<uint8_t> scratch(sb + 64, 0xA5);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n;
    k.scratch = scratch.data(); k.scratch_bytes = sb;
    std::string err;
    const int rc = launch_deflate_level(0, k, fmt, level, err, fmt == DE_GZIP ? launch_crc32 : launch_adler32);
    if (rc) fprintf(stderr, "sim_deflate_hc: %s\n", err.c_str());
    return rc;
}
