// k_deflate_hc_dict.hip -- levels 2..9 of the DEFLATE / zlib encoder of k_deflate_hc.hip behind SHARED DICTIONARIES: block b's matches
// may also reach into the D bytes (at most 32768, all within reach) of a range anywhere in the input buffer, and the hash chains of a
// range are built once for all the blocks that name it (lz_dict.h has the method and the words of k.aux).  Included behind
// k_deflate_hc.hip and k_deflate_hc_hist.hip (one translation unit): the plan, checksum, price, parse, block, scan and place kernels
// are theirs and k_deflate_encode.hip's, launched unchanged; k_dh_hist_head and k_de_scan / k_de_place<DE_ZDICT> serve the zlib form as
// they are (aux[b] and aux[n + b] are where they look).  Every block's bytes are those of k_deflate_hc_hist.hip for the same block with
// the same D bytes directly in front of it.
//
// Launches as launch_deflate_hist's, with k_dh_dict_build (a workgroup per distinct dictionary, grid-strided) in front of
// k_dh_dict_links and k_dh_dict_search in the places of k_dh_hist_links and k_dh_hist_search.  Scratch: lzd_carve's arrays (192 KiB per
// distinct dictionary, 8 bytes per block) in front of dh_carve's.
#include "lz_dict.h"

#define DH_DSLOT 32768u                /* link entries per dictionary */

static inline uint64_t dh_dict_scratch_bytes(uint32_t n, uint64_t nsegs, uint64_t ndict) { return dh_scratch_bytes(n, nsegs) + lzd_bytes(n, ndict, DH_DSLOT); }

__global__ __launch_bounds__(256) void k_dh_dict_build(rcx_kargs a, LzdScratch z)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    lzd_build<DE_WIN>(a, z, s_head, s_hc);
}

// Which segments take the dictionary's path: those lzd_sees says see it, in both kernels below.  A segment that starts at s0 >= DE_SEG
// has its window begin at D + s0 - DE_WIN > D, so the only one that can is the block's first (s0 == 0), which is what lzd_links_first
// and lzd_search_first take.
static_assert(DE_SEG > DE_WIN, "a later segment's window must begin inside the block");

__global__ __launch_bounds__(256) void k_dh_dict_links(rcx_kargs a, DeScratch d, DhScratch h, LzdScratch z)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        const LzdDict t = lzd_of<DE_WIN>(a, z, s.b);
        uint16_t* link = h.link + (uint64_t)s.f0 * DE_SEG;
        if (lzd_sees<DE_WIN>(t.D, s.s0)) lzd_links_first<DE_WIN>(s, t, z.tail + 4 * (uint64_t)s.b, link, s_head, s_hc);   // (s0 == 0: above)
        else lzc_links<DE_WIN>(s, link, s_head, s_hc);
    }
}

__global__ __launch_bounds__(256) RCX_SGPR_CAP void k_dh_dict_search(rcx_kargs a, DeScratch d, DhScratch h, LzdScratch z, uint32_t depth)
{
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        const LzcSeg s = de_seg(a, d, g);
        const LzdDict t = lzd_of<DE_WIN>(a, z, s.b);
        const uint16_t* link = h.link + (uint64_t)s.f0 * DE_SEG;
        uint32_t* cand = h.cand + (uint64_t)g * DE_SEG;
        if (lzd_sees<DE_WIN>(t.D, s.s0)) lzd_search_first<DhMatch>(s, t, z.tail + 4 * (uint64_t)s.b, link, cand, depth);
        else lzc_search<DhMatch>(s, link, cand, depth);
    }
}

// the whole encode on stream s at `level` (2..9), fmt DE_RAW or DE_ZLIB (FDICT and aux[n + b] where aux[b] != 0); k.aux: the words of
// rcx_plan_dict (never null); k.scratch holds dh_dict_scratch_bytes(n, segments, ndict) bytes
static int launch_deflate_dict(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t ndict, std::string& err, void (*cks)(hipStream_t, rcx_kargs&))
{
    const uint32_t n = k.nblocks;
    if (level < 2 || level > 9) { err = "deflate encode behind shared dictionaries: level must be 2..9"; return RCX_RC_BAD_ARG; }
    if (fmt != DE_RAW && fmt != DE_ZLIB) { err = "deflate encode behind shared dictionaries: raw DEFLATE or zlib"; return RCX_RC_BAD_ARG; }
    if (!k.aux) { err = "deflate encode behind shared dictionaries: use rcx_deflate_encode_shared_batch / rcx_zlib_encode_shared_batch"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < dh_dict_scratch_bytes(n, 0, ndict)) { err = "deflate encode: scratch too small"; return RCX_RC_BAD_ARG; }
    uint8_t* rest;
    const LzdScratch z = lzd_carve(k.scratch, n, ndict, DH_DSLOT, &rest);
    DhScratch h;
    const DeScratch d = dh_carve(rest, k.scratch_bytes - (uint64_t)(rest - (uint8_t*)k.scratch), n, h);
    hipLaunchKernelGGL(k_de_plan, dim3(1), dim3(1024), 0, s, k, d);
    if (fmt != DE_RAW && d.cap) {
        hipLaunchKernelGGL(k_de_segs, dim3(d.cap < 65536u * 4u ? (d.cap + 255) / 256 : 1024u), dim3(256), 0, s, k, d);
        rcx_kargs kc = k;                                 // a wave per segment: the block's bytes alone
        kc.in_off = d.seg_ioff; kc.in_len = d.seg_ilen; kc.nblocks = d.cap;
        kc.out_len = nullptr; kc.in_used = nullptr; kc.status = nullptr; kc.aux = d.seg_cks;
        cks(s, kc);
    }
    if (d.cap) {
        const dim3 gs(d.cap < 8192u ? d.cap : 8192u);
        if (ndict) hipLaunchKernelGGL(k_dh_dict_build, dim3(ndict < LZD_GRID ? ndict : LZD_GRID), dim3(256), 0, s, k, z);
        hipLaunchKernelGGL(k_dh_dict_links, gs, dim3(256), 0, s, k, d, h, z);
        hipLaunchKernelGGL(k_dh_dict_search, gs, dim3(256), 0, s, k, d, h, z, dh_depth(level));
        for (uint32_t it = 0; it < (level >= DH_ITER ? 2u : 1u); it++) {
            hipLaunchKernelGGL(k_dh_price, gs, dim3(DE_T), 0, s, k, d, h, it);
            hipLaunchKernelGGL(k_dh_parse, gs, dim3(64), 0, s, k, d, h);
        }
        hipLaunchKernelGGL(k_dh_block, dim3(d.cap < 2048u ? d.cap : 2048u), dim3(DE_T), 0, s, k, d);
    }
    const dim3 gs((n + 3) / 4), gp(d.cap < 4096u ? d.cap : 4096u), gh((n + 255) / 256);
    if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_scan<DE_RAW>, gs, dim3(256), 0, s, k, d);
    else hipLaunchKernelGGL(k_de_scan<DE_ZDICT>, gs, dim3(256), 0, s, k, d);
    if (d.cap) {
        if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_place<DE_RAW>, gp, dim3(256), 0, s, k, d);
        else hipLaunchKernelGGL(k_de_place<DE_ZDICT>, gp, dim3(256), 0, s, k, d);
    }
    if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_dh_hist_head, gh, dim3(256), 0, s, k, (uint32_t)level);
    return RCX_RC_OK;
}
