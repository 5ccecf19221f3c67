// sim_dict_decode.cpp -- runs the UNMODIFIED decoders behind shared dictionaries (k_lz4_dict.hip; k_inflate_dict.hip behind
// k_inflate2.hip) and the host's rcx_plan_dict on the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by
// tests/sim_dict_decode_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_dict_decode/sim_dict_decode.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#define hipStream_t int
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) ws::launch(grid, block, [&] { kern(__VA_ARGS__); })
#include "../../rust_compress_amd/csrc/rcx_plan.h"
#include "../../rust_compress_amd/csrc/k_inflate2.hip"
#include "../../rust_compress_amd/csrc/k_inflate_dict.hip"
#include "../../rust_compress_amd/csrc/k_lz4_dict.hip"

// `bytes` bytes between two pages that cannot be touched: front != 0 -- the first byte is a page's first (an access below the buffer
// ends the process), else the last byte is a page's last (an access beyond it does).  The buffer is never freed: a test process's.
extern "C" void* sim_guarded(uint64_t bytes, int front)
{
    const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
    const uint64_t body = (bytes + pg - 1) / pg * pg;
    uint8_t* p = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == (uint8_t*)MAP_FAILED) return nullptr;
    mprotect(p, pg, PROT_NONE);
    mprotect(p + pg + body, pg, PROT_NONE);
    return front ? p + pg : p + pg + body - bytes;
}

// family 0: LZ4 (rcx_lz4_decode_shared_batch's kernel), 1: raw DEFLATE, 2: zlib (dict_id).  dict_off / dict_len as the C ABI takes
// them; flags (DEFLATE, zlib): the streams' flags.  info: the plan's ndict and span.  -1: the plan refused (err_out has the text).
extern "C" int sim_dict_decode(int family, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint64_t* dict_off,
                               const uint64_t* dict_len, const uint32_t* dict_id, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                               uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t* flags, uint32_t n, uint64_t* info, char* err_out,
                               uint32_t err_cap)
{
    rcx_dict_plan plan;
    std::string err;
    const bool lz4 = family == 0;
    if (!rcx_plan_dict(n, dict_off, dict_len, lz4 ? 65536 : 32768, lz4 ? 65535 : 32768, family == 2 ? dict_id : nullptr, lz4 ? "lz4 decode" : "inflate",
                       plan, err)) {
        if (err_out && err_cap) { strncpy(err_out, err.c_str(), err_cap - 1); err_out[err_cap - 1] = 0; }
        return -1;
    }
    info[0] = plan.ndict; info[1] = plan.span;
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = plan.aux.data();
    if (lz4) launch_lz4_decode_dict(0, k);
    else launch_inflate_dict(0, k, family == 2);
    if (!lz4) for (uint32_t i = 0; i < n; i++) flags[i] = plan.aux[i];
    return 0;
}
