// tu_bzip2_enc.hip -- bzip2 encode: the run-length step, the symbols, the table fit, the packer and the joiner behind
// rcx_bzip2_encode_batch (k_bzip2_enc.hip); the suffix sort between them is tu_bwt.hip's.
#include <new>
#include "rcx_tu.h"
#include "k_bzip2_enc.hip"

int rcx_tu_bzip2_encode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_off, const uint64_t* h_in_len, const uint64_t* h_out_off,
                        const uint64_t* h_out_cap, const rcx_bz2_alloc& alloc, int level, uint32_t round, std::string& err)
{
    // (the launch loop keeps its lists in vectors: running out of host memory is a status, not an exception across the C ABI)
    try { return launch_bzip2_encode(s, k, h_in_off, h_in_len, h_out_off, h_out_cap, alloc, level, 100000u * (uint32_t)level - 19u, round, err); }
    catch (const std::bad_alloc&) { err = "bzip2 encode: out of host memory"; return RCX_RC_NO_MEMORY; }
}
