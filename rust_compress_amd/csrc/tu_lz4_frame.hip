// tu_lz4_frame.hip -- the device side of the LZ4 frame format: XXH32 of every block, LZ4 block decode with history (in front of the
// slot: linked blocks, dictionaries; or a shared dictionary in the input buffer).
#include "rcx_tu.h"
#include "k_xxh32.hip"
#include "k_lz4_linked.hip"
#include "k_lz4_dict.hip"

void rcx_tu_xxh32(hipStream_t s, rcx_kargs& k, uint32_t seed) { launch_xxh32(s, k, seed); }
void rcx_tu_lz4_decode_linked(hipStream_t s, rcx_kargs& k, const uint32_t* order, const uint32_t* rounds_off, uint32_t nrounds,
                              const uint32_t* head, const uint32_t* dict, uint64_t* eff)
{
    launch_lz4_decode_linked(s, k, order, rounds_off, nrounds, head, dict, eff);
}
void rcx_tu_lz4_decode_dict(hipStream_t s, rcx_kargs& k) { launch_lz4_decode_dict(s, k); }
