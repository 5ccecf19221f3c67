// tu_bzip2.hip -- bzip2 decode: the scan, the entropy decoder and the run-length stage behind rcx_bzip2_decode_batch (k_bzip2.hip); the
// inverse BWT between them is tu_bwt.hip's.
#include <new>
#include "rcx_tu.h"
#include "k_bzip2.hip"

int rcx_tu_bzip2_decode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_len, const uint64_t* h_out_off, const uint64_t* h_out_cap,
                        const rcx_bz2_alloc& alloc, uint32_t round, std::string& err)
{
    // (the launch loop keeps its lists in vectors: running out of host memory is a status, not an exception across the C ABI)
    try { return launch_bzip2_decode(s, k, h_in_len, h_out_off, h_out_cap, alloc, round, err); }
    catch (const std::bad_alloc&) { err = "bzip2 decode: out of host memory"; return RCX_RC_NO_MEMORY; }
}
