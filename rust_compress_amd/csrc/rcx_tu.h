// rcx_tu.h -- host-side entry points of the per-codec translation units (tu_*.hip).  librcx.so is built from several
// TUs so that hipcc compiles them in parallel; each TU holds its kernels and the launch code next to them.
#pragma once
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <hip/hip_runtime.h>
#include <string>
#include "rcx_dev.h"

// tu_lz4.hip
int rcx_tu_lz4_decode(hipStream_t s, rcx_kargs& k, int variant, std::string& err);
int rcx_tu_lz4_encode(hipStream_t s, rcx_kargs& k, int variant, std::string& err);
void rcx_tu_lz4_decode_mirror_again(hipStream_t s, rcx_kargs& k);
uint64_t rcx_tu_lz4_encode_scratch(uint32_t nblocks);
// tu_inflate.hip
void rcx_tu_inflate(hipStream_t s, rcx_kargs& k, bool zlib, int variant);
// ... with history (k_inflate_hist.hip): k.aux = n history lengths (uint32), then n DICTIDs (zlib); flags come back in the first n
void rcx_tu_inflate_hist(hipStream_t s, rcx_kargs& k, bool zlib);
// ... behind shared dictionaries (k_inflate_dict.hip): k.aux = the words of rcx_plan_dict; flags come back in the first n
void rcx_tu_inflate_dict(hipStream_t s, rcx_kargs& k, bool zlib);
void rcx_tu_adler32(hipStream_t s, rcx_kargs& k);
void rcx_tu_crc32(hipStream_t s, rcx_kargs& k);
void rcx_tu_gzip_decode(hipStream_t s, rcx_kargs& k, int variant);
uint64_t rcx_tu_inflate_scratch(uint32_t nblocks);
bool rcx_tu_inflate_mirrors(uint32_t nblocks, int variant);     // would the launch store into a page-locked output buffer itself?
uint64_t rcx_tu_inflate_marks_offset(uint32_t nblocks);      // a mirrored launch: [count | 60 bytes | a byte per stream the first pass handed back]
uint64_t rcx_tu_gzip_scratch(uint32_t nblocks);
uint64_t rcx_tu_gzip_marks_offset(uint32_t nblocks);
// tu_bwt.hip
int rcx_tu_bwt_forward(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool sa_words);
int rcx_tu_bwt_inversion_table(hipStream_t s, rcx_kargs& k);
int rcx_tu_bwt_inverse(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool minimal);
uint64_t rcx_tu_bwt_forward_scratch(uint32_t nblocks, uint64_t max_block);
uint64_t rcx_tu_bwt_inverse_scratch(uint32_t nblocks, uint64_t max_block);
// tu_serial.hip
void rcx_tu_serial(hipStream_t s, int codec, rcx_kargs& k, int variant, uint32_t param);
uint64_t rcx_tu_dc_encode_scratch(uint32_t nblocks, uint64_t max_block);
// tu_deflate_encode.hip (fmt: 0 raw DEFLATE, 1 zlib, 2 gzip)
int rcx_tu_deflate_encode(hipStream_t s, rcx_kargs& k, int fmt, std::string& err);
uint64_t rcx_tu_deflate_encode_scratch(uint32_t nblocks, uint64_t nsegs);
uint64_t rcx_tu_deflate_encode_segments(uint64_t len);
int rcx_tu_deflate_encode_level(hipStream_t s, rcx_kargs& k, int fmt, int level, std::string& err);    // level 1..9 (1: as above)
uint64_t rcx_tu_deflate_level_scratch(uint32_t nblocks, uint64_t nsegs);
// ... levels 2..9 with history (k_deflate_hc_hist.hip), fmt 0 or 1: k.aux = n history lengths (uint32), then n DICTIDs (zlib), or null;
// nhist = the blocks that have one
int rcx_tu_deflate_encode_hist(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t nhist, std::string& err);
uint64_t rcx_tu_deflate_hist_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t nhist);
// ... levels 2..9 behind shared dictionaries (k_deflate_hc_dict.hip), fmt 0 or 1: k.aux = the words of rcx_plan_dict, ndict = the distinct dictionaries
int rcx_tu_deflate_encode_dict(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t ndict, std::string& err);
uint64_t rcx_tu_deflate_dict_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t ndict);
// tu_lz4_hc.hip (level 1..12)
int rcx_tu_lz4_hc(hipStream_t s, rcx_kargs& k, int level, std::string& err);
uint64_t rcx_tu_lz4_hc_scratch(uint32_t nblocks, uint64_t nsegs);
uint64_t rcx_tu_lz4_hc_segments(uint64_t len);
// ... with history (k_lz4_hc_hist.hip): k.aux = the history lengths (uint32) or null, nhist = the blocks that have one
int rcx_tu_lz4_hc_hist(hipStream_t s, rcx_kargs& k, int level, uint32_t nhist, std::string& err);
uint64_t rcx_tu_lz4_hc_hist_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t nhist);
// ... behind shared dictionaries (k_lz4_hc_dict.hip): k.aux = the words of rcx_plan_dict, ndict = the distinct dictionaries
int rcx_tu_lz4_hc_dict(hipStream_t s, rcx_kargs& k, int level, uint32_t ndict, std::string& err);
uint64_t rcx_tu_lz4_hc_dict_scratch(uint32_t nblocks, uint64_t nsegs, uint64_t ndict);
// tu_lz4_frame.hip: XXH32 of every block; LZ4 block decode with history (linked blocks, dictionaries), one launch per chain depth
void rcx_tu_xxh32(hipStream_t s, rcx_kargs& k, uint32_t seed);
// order[rounds_off[r] .. rounds_off[r + 1]): the blocks at depth r of their chains (rounds_off is a HOST array); head[i]: block i's chain
// head; dict[i]: a head's dictionary bytes; eff[i] (written): where block i's output starts in out_base.  Device arrays.
void rcx_tu_lz4_decode_linked(hipStream_t s, rcx_kargs& k, const uint32_t* order, const uint32_t* rounds_off, uint32_t nrounds,
                              const uint32_t* head, const uint32_t* dict, uint64_t* eff);
// LZ4 block decode behind shared dictionaries (k_lz4_dict.hip), one wave per block: k.aux = the words of rcx_plan_dict
void rcx_tu_lz4_decode_dict(hipStream_t s, rcx_kargs& k);
// tu_dict_train.hip: the batched dictionary trainer (k_dict_train.hip): k.aux = the words of rcx_plan_train; synchronous (it reads a
// count of finished jobs back every few rounds)
struct rcx_train_plan;
int rcx_tu_dict_train(hipStream_t s, rcx_kargs& k, const rcx_train_plan& plan, std::string& err);
// tu_bzip2.hip: .bz2 files (k_bzip2.hip).  Synchronous: it reads counts back between its stages and asks `alloc` for its scratch twice
// (the candidates are counted first).  h_*: the batch's lengths, slot offsets and capacities on the host.  Calls rcx_tu_bwt_inverse.
struct rcx_bz2_alloc;                        // rcx_plan.h
int rcx_tu_bzip2_decode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_len, const uint64_t* h_out_off, const uint64_t* h_out_cap,
                        const rcx_bz2_alloc& alloc, uint32_t round, std::string& err);          // round: candidates a round, 0 = the default
// tu_zstd.hip: XXH64 of every block (the hash comes back in out_len); .zst files (k_zstd.hip), one persistent wave per file up to `waves`
// (rcx_plan_zstd), k.aux = the words of rcx_plan_dict, k.scratch = a literal buffer per wave
void rcx_tu_xxh64(hipStream_t s, rcx_kargs& k, uint64_t seed);
int rcx_tu_zstd_decode(hipStream_t s, rcx_kargs& k, uint32_t waves, int variant, std::string& err);
// tu_bzip2_enc.hip: whole files to .bz2 streams (k_bzip2_enc.hip).  Synchronous: it reads the chunks' lengths and the blocks' records
// back and asks `alloc` for three buffers (0: the stages', 1: the sort's, 2: what lasts for the call).  Calls rcx_tu_bwt_forward.
int rcx_tu_bzip2_encode(hipStream_t s, rcx_kargs& k, const uint64_t* h_in_off, const uint64_t* h_in_len, const uint64_t* h_out_off,
                        const uint64_t* h_out_cap, const rcx_bz2_alloc& alloc, int level, uint32_t round, std::string& err);   // round: blocks a round, 0 = the default
