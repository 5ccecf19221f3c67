// tu_lz4_hc.hip -- the batched LZ4 high-compression block encoder, without history, with history and behind shared dictionaries, + its
// launch code (one translation unit).
#include "rcx_tu.h"
#include "k_lz4_hc.hip"
#include "k_lz4_hc_hist.hip"
#include "k_lz4_hc_dict.hip"

int rcx_tu_lz4_hc(hipStream_t s, rcx_kargs& k, int level, std::string& err) { return launch_lz4_hc(s, k, level, err); }
uint64_t rcx_tu_lz4_hc_scratch(uint32_t nblocks, uint64_t nsegs) { return hc_scratch_bytes(nblocks, nsegs); }
uint64_t rcx_tu_lz4_hc_segments(uint64_t len) { return hc_segments(len); }
int rcx_tu_lz4_hc_hist(hipStream_t s, rcx_kargs& k, int level, uint32_t nhist, std::string& err) { return launch_lz4_hc_hist(s, k, level, nhist, err); }
uint64_t rcx_tu_lz4_hc_hist_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t nhist) { return hc_hist_scratch_bytes(nblocks, nsegs, nhist); }
int rcx_tu_lz4_hc_dict(hipStream_t s, rcx_kargs& k, int level, uint32_t ndict, std::string& err) { return launch_lz4_hc_dict(s, k, level, ndict, err); }
uint64_t rcx_tu_lz4_hc_dict_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t ndict) { return hc_dict_scratch_bytes(nblocks, nsegs, ndict); }
