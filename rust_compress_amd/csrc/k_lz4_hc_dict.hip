// k_lz4_hc_dict.hip -- the LZ4 HC block encoder of k_lz4_hc.hip behind SHARED DICTIONARIES: block b's matches may also reach into the D
// bytes (at most 65535) of a range anywhere in the input buffer, and the hash chains of a range are built once for all the blocks that
// name it (lz_dict.h has the method and the words of k.aux).  Included behind k_lz4_hc.hip (one translation unit): the plan, parse, scan
// and place kernels are that file's, launched unchanged.  Every block's bytes are those of k_lz4_hc_hist.hip for the same block with
// the same D bytes directly in front of it.
//
// Launches: k_hc_plan; k_hc_dict_build, a workgroup per distinct dictionary (grid-strided); k_hc_dict_links and k_hc_dict_search, a
// workgroup per segment: a block's first segment behind a dictionary by lzd_links_first / lzd_search_first, every other segment as
// k_hc_links / k_hc_search do it; then k_hc_parse, k_hc_scan, k_hc_place.  Scratch: lzd_carve's arrays (256 KiB per distinct dictionary,
// 8 bytes per block) in front of hc_carve's.
#include "lz_dict.h"

#define HC_DSLOT 65536u                /* link entries per dictionary */

static inline uint64_t hc_dict_scratch_bytes(uint32_t n, uint64_t nsegs, uint64_t ndict) { return hc_scratch_bytes(n, nsegs) + lzd_bytes(n, ndict, HC_DSLOT); }

__global__ __launch_bounds__(256) void k_hc_dict_build(rcx_kargs a, LzdScratch z)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    lzd_build<HC_WIN>(a, z, s_head, s_hc);
}

// Which segments take the dictionary's path: those lzd_sees says see it, in both kernels below.  A segment that starts at s0 >= HC_SEG
// has its window begin at D + s0 - HC_WIN > D, so the only one that can is the block's first (s0 == 0), which is what lzd_links_first
// and lzd_search_first take.
static_assert(HC_SEG > HC_WIN, "a later segment's window must begin inside the block");

__global__ __launch_bounds__(256) void k_hc_dict_links(rcx_kargs a, HcScratch d, LzdScratch z)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        const LzdDict t = lzd_of<HC_WIN>(a, z, s.b);
        uint16_t* link = d.link + (uint64_t)s.f0 * HC_SEG;
        if (lzd_sees<HC_WIN>(t.D, s.s0)) lzd_links_first<HC_WIN>(s, t, z.tail + 4 * (uint64_t)s.b, link, s_head, s_hc);   // (s0 == 0: above)
        else lzc_links<HC_WIN>(s, link, s_head, s_hc);
    }
}

__global__ __launch_bounds__(256) RCX_SGPR_CAP void k_hc_dict_search(rcx_kargs a, HcScratch d, LzdScratch z, uint32_t depth)
{
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = hc_seg(a, d, g);
        const LzdDict t = lzd_of<HC_WIN>(a, z, s.b);
        const uint16_t* link = d.link + (uint64_t)s.f0 * HC_SEG;
        uint32_t* cand = d.cand + (uint64_t)g * HC_SEG;
        if (lzd_sees<HC_WIN>(t.D, s.s0)) lzd_search_first<HcMatch>(s, t, z.tail + 4 * (uint64_t)s.b, link, cand, depth);
        else lzc_search<HcMatch>(s, link, cand, depth);
    }
}

// the whole encode on stream s at `level` (1..12); k.aux: the words of rcx_plan_dict (never null); k.scratch holds
// hc_dict_scratch_bytes(n, segments, ndict) bytes
static int launch_lz4_hc_dict(hipStream_t s, rcx_kargs& k, int level, uint32_t ndict, std::string& err)
{
    const uint32_t n = k.nblocks;
    if (level < 1 || level > 12) { err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    if (!k.aux) { err = "lz4 hc behind shared dictionaries: use rcx_lz4_encode_hc_shared_batch"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < hc_dict_scratch_bytes(n, 0, ndict)) { err = "lz4 hc: scratch too small"; return RCX_RC_BAD_ARG; }
    uint8_t* rest;
    const LzdScratch z = lzd_carve(k.scratch, n, ndict, HC_DSLOT, &rest);
    const HcScratch d = hc_carve(rest, k.scratch_bytes - (uint64_t)(rest - (uint8_t*)k.scratch), n);
    hipLaunchKernelGGL(k_hc_plan, dim3(1), dim3(1024), 0, s, k, d);
    if (d.cap) {
        const uint32_t gs = d.cap < 8192u ? d.cap : 8192u;
        if (ndict) hipLaunchKernelGGL(k_hc_dict_build, dim3(ndict < LZD_GRID ? ndict : LZD_GRID), dim3(256), 0, s, k, z);
        hipLaunchKernelGGL(k_hc_dict_links, dim3(gs), dim3(256), 0, s, k, d, z);
        hipLaunchKernelGGL(k_hc_dict_search, dim3(gs), dim3(256), 0, s, k, d, z, hc_depth(level));
        hipLaunchKernelGGL(k_hc_parse, dim3(gs), dim3(64), 0, s, k, d);
    }
    hipLaunchKernelGGL(k_hc_scan, dim3((n + 63) / 64), dim3(64), 0, s, k, d);
    if (d.cap) hipLaunchKernelGGL(k_hc_place, dim3(d.cap < 8192u ? d.cap : 8192u), dim3(256), 0, s, k, d);
    return RCX_RC_OK;
}
