// sim_lz4frame.cpp -- runs the UNMODIFIED XXH32 and linked LZ4 decode kernels (k_xxh32.hip, k_lz4_linked.hip) on the wave64 simulator of
// tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_lz4frame_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_lz4frame/sim_lz4frame.cpp tests/wavesim/wavesim.cpp
#define hipStream_t int
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) ws::launch(grid, block, [&] { kern(__VA_ARGS__); })
#include "../../rust_compress_amd/csrc/k_xxh32.hip"
#include "../../rust_compress_amd/csrc/k_lz4_linked.hip"

extern "C" void sim_xxh32(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint32_t seed, uint32_t* hash,
                          uint64_t* in_used, int32_t* status)
{
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.in_used = in_used; k.status = status; k.aux = hash; k.nblocks = n;
    if (n) launch_xxh32(0, k, seed);
}

// the chains as rcx_lz4_decode_linked_batch lays them out (tests/sim_lz4frame_run.py does that part): order sorted by depth, rounds_off
// its nrounds + 1 bounds, head / dict per block; eff is written
extern "C" void sim_lz4_decode_linked(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out, const uint64_t* out_off,
                                      const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t n,
                                      const uint32_t* order, const uint32_t* rounds_off, uint32_t nrounds, const uint32_t* head,
                                      const uint32_t* dict, uint64_t* eff)
{
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n;
    launch_lz4_decode_linked(0, k, order, rounds_off, nrounds, head, dict, eff);
}
