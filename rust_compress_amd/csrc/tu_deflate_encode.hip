// tu_deflate_encode.hip -- the batched DEFLATE / zlib / gzip encoder, without and with history, + its launch code (one translation unit).  The checksums of the
// framings come from the kernels of tu_inflate.hip (k_crc32, k_adler32).
#include "rcx_tu.h"
#include "k_deflate_encode.hip"
#include "k_deflate_hc.hip"              // levels 2..9 (after k_deflate_encode.hip, whose kernels it reuses)
#include "k_deflate_hc_hist.hip"         // ... with history
#include "k_deflate_hc_dict.hip"         // ... behind shared dictionaries

int rcx_tu_deflate_encode(hipStream_t s, rcx_kargs& k, int fmt, std::string& err)
{
    return launch_deflate_encode(s, k, fmt, err, fmt == DE_GZIP ? rcx_tu_crc32 : rcx_tu_adler32);
}
int rcx_tu_deflate_encode_level(hipStream_t s, rcx_kargs& k, int fmt, int level, std::string& err)
{
    return launch_deflate_level(s, k, fmt, level, err, fmt == DE_GZIP ? rcx_tu_crc32 : rcx_tu_adler32);
}
int rcx_tu_deflate_encode_hist(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t nhist, std::string& err)
{
    return launch_deflate_hist(s, k, fmt, level, nhist, err, rcx_tu_adler32);
}
int rcx_tu_deflate_encode_dict(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t ndict, std::string& err)
{
    return launch_deflate_dict(s, k, fmt, level, ndict, err, rcx_tu_adler32);
}
uint64_t rcx_tu_deflate_dict_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t ndict) { return dh_dict_scratch_bytes(nblocks, nsegs, ndict); }
uint64_t rcx_tu_deflate_hist_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t nhist) { return dh_hist_scratch_bytes(nblocks, nsegs, nhist); }
uint64_t rcx_tu_deflate_level_scratch(uint32_t nblocks, uint64_t nsegs) { return dh_scratch_bytes(nblocks, nsegs); }
uint64_t rcx_tu_deflate_encode_scratch(uint32_t nblocks, uint64_t nsegs) { return de_scratch_bytes(nblocks, nsegs); }
uint64_t rcx_tu_deflate_encode_segments(uint64_t len) { return (len + DE_SEG - 1) / DE_SEG; }
