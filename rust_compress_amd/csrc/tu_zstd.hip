// tu_zstd.hip -- Zstandard decode (k_zstd.hip) behind rcx_zstd_decode_batch, and XXH64 of every block (k_xxh64.hip), which the decoder
// checks a frame's content with.
#include "rcx_tu.h"
#include "k_zstd.hip"

void rcx_tu_xxh64(hipStream_t s, rcx_kargs& k, uint64_t seed) { launch_xxh64(s, k, seed); }
int rcx_tu_zstd_decode(hipStream_t s, rcx_kargs& k, uint32_t waves, int variant, std::string& err) { return launch_zstd_decode(s, k, waves, variant, err); }
