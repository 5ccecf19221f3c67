/*
 * rcx.h -- C ABI of the MI355X-native block-codec engine ("rcx" = rust-compress on CDNA).
 *
 * This is the drop-in boundary for the hot path of the Rust crate `compress`
 * (rusty-shell/rust-compress): every entry point below replaces one per-block
 * kernel that the crate's `Decoder<R: Read>` / `Encoder<W: Write>` types call
 * once per block; here it is called once per BATCH of independent blocks.
 * The reference interface each entry point replaces is cited as
 * `reference: <file>:<lines>` (paths relative to the crate root).
 *
 * Conventions (all entry points):
 *   - plain C99 types only; no C++/torch/HIP types cross the boundary
 *     (a HIP stream is passed as `void*`).
 *   - struct-of-arrays batch descriptors: block i reads
 *     in_base[in_off[i] .. in_off[i]+in_len[i]) and writes at most out_cap[i]
 *     bytes at out_base[out_off[i]..]; the callee allocates nothing the caller
 *     keeps, and retains no pointer after return.  No byte of `out_base`
 *     outside the slots is written, from either memory kind; inside a slot,
 *     bytes beyond `out_len[i]` are unspecified unless an entry point says
 *     otherwise.
 *   - `mem` says where the DATA buffers (in_base/out_base) live:
 *       RCX_MEM_DEVICE: HBM pointers (hipMalloc / torch.cuda tensors);
 *       RCX_MEM_HOST:   host pointers; the library stages them through HBM.
 *     The small descriptor arrays (offsets, lengths, status, ...) are ALWAYS
 *     host arrays; the library copies them to/from the device.
 *   - return value = batch-level status (bad arguments, HIP failure);
 *     per-block results go to status[i] (enum rcx_status). A failing block
 *     never affects another block. Nothing aborts or throws across the ABI.
 *   - the rcx_*_batch calls are synchronous from the caller's view (results are
 *     complete on return); rcx_launch_dev() only enqueues on the ctx stream.
 *   - there is NO CPU fallback: without a usable HIP device every call fails
 *     with RCX_E_NO_DEVICE.
 */
#ifndef RCX_H
#define RCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-block status: mirrors the reference's io::Error strings 1:1 ------ */
enum rcx_status {
    RCX_OK = 0,
    /* lib.rs:53-62,115-118 "unexpected end of file" / byteorder UnexpectedEof */
    RCX_E_EOF = 1,
    /* new: caller's out_cap[i] too small (the reference grows a Vec instead) */
    RCX_E_OUTPUT_TOO_SMALL = 2,
    /* input on which the reference panics (index OOB / assert!) or reads
     * uninitialised memory: lz4.rs:93,135,407; bwt/mod.rs:114,230; dc.rs:213;
     * flate.rs:297,432; ari/mod.rs:282 */
    RCX_E_MALFORMED = 3,
    /* flate.rs:56-65 */
    RCX_E_HUFFMAN_TREE_TOO_LARGE = 10,     /* "huffman tree too large" */
    RCX_E_INVALID_BLOCK_CODE = 11,         /* "invalid block code" */
    RCX_E_INVALID_HUFFMAN_HEADER_SYMBOL = 12, /* "invalid huffman header symbol" */
    RCX_E_INVALID_HUFFMAN_TREE = 13,       /* "invalid huffman tree" */
    RCX_E_INVALID_HUFFMAN_TREE_HEADER = 14,/* "invalid huffman tree header" */
    RCX_E_INVALID_HUFFMAN_CODE = 15,       /* "invalid huffman code" */
    RCX_E_INVALID_STATIC_SIZE = 16,        /* "invalid static size" */
    RCX_E_NOT_ENOUGH_BITS = 17,            /* "not enough bits" */
    /* zlib.rs:59-84,111-114 */
    RCX_E_ZLIB_FORMAT = 20,     /* "unsupported zlib stream format" */
    RCX_E_ZLIB_WINDOW = 21,     /* "unsupported zlib window size" */
    RCX_E_ZLIB_DICT = 22,       /* "unsupported initial dictionary in the output stream" */
    RCX_E_ZLIB_HEADER_CHECKSUM = 23, /* "invalid zlib header checksum" */
    RCX_E_ZLIB_CHECKSUM = 24,   /* "invalid checksum on zlib stream" */
    /* rcx_zlib_decode_dict_batch (extension): the stream's DICTID is not the caller's dict_id[i] */
    RCX_E_ZLIB_DICT_ID = 25,    /* "zlib dictionary id mismatch" */
    /* rle.rs:153 */
    RCX_E_RLE_LONG_RUN = 30,    /* "Overly long run" */
    /* lz4.rs:366,376: InvalidInput with empty message */
    RCX_E_LZ4_MAGIC = 40,
    RCX_E_LZ4_VERSION = 41,
    /* lz4.rs:229-230: compression_bound() == None -> encode returns 0 */
    RCX_E_LZ4_INPUT_TOO_LARGE = 42,
    /* rcx_lz4_decode_linked_batch: an earlier block of this block's chain failed, so its history does not exist */
    RCX_E_LZ4_HISTORY = 43,
    /* gzip member framing (RFC 1952; extension, see rcx_gzip_decode_batch) */
    RCX_E_GZIP_MAGIC = 50,          /* ID1 ID2 != 1f 8b */
    RCX_E_GZIP_METHOD = 51,         /* CM != 8 */
    RCX_E_GZIP_FLAGS = 52,          /* reserved FLG bits set */
    RCX_E_GZIP_CRC = 53,            /* CRC32 trailer mismatch */
    RCX_E_GZIP_ISIZE = 54,          /* ISIZE trailer mismatch */
    /* a limit of this implementation, not of the format: bwt::Encoder::new(w, block_size) takes any usize (bwt/mod.rs:451), the suffix
     * sorter keeps four flag bits beside a suffix index -- a block of 2^28 bytes or more gets this status (out_len 0) and the rest of
     * the batch is transformed.  The host mirrors turn it into io::ErrorKind::InvalidInput. */
    RCX_E_BWT_BLOCK_TOO_LARGE = 60, /* "bwt block of 2^28 bytes or more" */
    /* bzip2 files (extension, see rcx_bzip2_decode_batch) */
    RCX_E_BZ2_MAGIC = 70,           /* the first 4 bytes are not BZh1..BZh9 */
    RCX_E_BZ2_DATA = 71,            /* a malformed block or stream structure */
    RCX_E_BZ2_BLOCK_CRC = 72,       /* a block's CRC does not match */
    RCX_E_BZ2_STREAM_CRC = 73,      /* a stream's combined CRC does not match */
    RCX_E_BZ2_RANDOMISED = 74,      /* the obsolete randomised bit is set (bzip2 has not written it since 0.9.5): not supported */
    /* Zstandard files (extension, see rcx_zstd_decode_batch) */
    RCX_E_ZSTD_MAGIC = 80,          /* the first 4 bytes are no frame */
    RCX_E_ZSTD_HEADER = 81,         /* a reserved header bit, a window beyond 2^31 */
    RCX_E_ZSTD_DATA = 82,           /* everything else the format calls corrupt */
    RCX_E_ZSTD_CHECKSUM = 83,       /* the content checksum does not match */
    RCX_E_ZSTD_DICT = 84            /* a Dictionary_ID: the frame needs a formatted dictionary, which the call does not take */
};

/* ---- batch-level return codes --------------------------------------------- */
enum rcx_rc {
    RCX_RC_OK = 0,
    RCX_RC_BAD_ARG = -1,
    RCX_RC_NO_DEVICE = -2,   /* no HIP device / runtime: there is no CPU path */
    RCX_RC_HIP_ERROR = -3,
    RCX_RC_NO_MEMORY = -4
};

enum rcx_mem { RCX_MEM_HOST = 0, RCX_MEM_DEVICE = 1 };

/* inflate per-stream flag bits (out: flags[i]) */
#define RCX_W_EMPTY_BLOCK_MIDSTREAM 1u /* flate.rs:474-476 quirk: the reference's
                                          read() returns Ok(0) here; we decode on */

typedef struct rcx_ctx rcx_ctx;

/* ---- context ---------------------------------------------------------------- */
/* One ctx per caller thread and device (thread-compatible, not thread-safe).
 * device_id < 0 selects the current HIP device. */
int  rcx_ctx_create(int device_id, rcx_ctx** out);
void rcx_ctx_destroy(rcx_ctx* ctx);
/* Launch on the caller's HIP stream (hipStream_t passed as void*; NULL = the HIP
 * null stream).  A new ctx launches on its own non-blocking stream. */
int  rcx_ctx_set_stream(rcx_ctx* ctx, void* hip_stream);
const char* rcx_last_error(const rcx_ctx* ctx);
const char* rcx_status_string(int status);   /* the reference's error text */
int  rcx_version(void);

/* A batch descriptor shared by every codec (struct-of-arrays, host arrays). */
typedef struct rcx_batch {
    const uint8_t*  in_base;   /* mem */
    const uint64_t* in_off;    /* host [n] */
    const uint64_t* in_len;    /* host [n] */
    uint8_t*        out_base;  /* mem */
    const uint64_t* out_off;   /* host [n] */
    const uint64_t* out_cap;   /* host [n] */
    uint64_t*       out_len;   /* host [n], written */
    uint64_t*       in_used;   /* host [n] or NULL, written: bytes consumed */
    int32_t*        status;    /* host [n], written: enum rcx_status */
    uint32_t        nblocks;
    int             mem;       /* enum rcx_mem for in_base/out_base */
} rcx_batch;

/* ---- LZ4 -------------------------------------------------------------------- */
/* reference: src/lz4.rs:602-611 decode_block() -> BlockDecoder::decode :67-110
 * RCX_MEM_HOST with a PAGE-LOCKED out_base (hipHostMalloc / hipHostRegister): the decoder stores the decoded bytes straight into
 * the caller's buffer while it runs (nothing beyond out_len[i] of a block's slot is written for a block that decodes; a block that
 * fails, or one whose late input made the library decode it a second time, may leave bytes of its first attempt anywhere in its
 * slot -- never outside it) and, when in_base is page-locked
 * too, the compressed bytes arrive in block ranges under the launch; with pageable buffers one copy each way around the launch.
 * Same results either way.  rcx_ctx_set_param(ctx, RCX_LZ4_DECODE, 1) keeps the plain copies (A/B). */
int rcx_lz4_decode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/lz4.rs:616-627 encode_block() -> BlockEncoder::encode :226-310
 * (bit-exact: hash/skip/backtrack heuristics reproduced) */
int rcx_lz4_encode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/lz4.rs:175-181 compression_bound(); 0 == None */
uint64_t rcx_lz4_compression_bound(uint64_t in_len);
/* ---- extension beyond the reference (its frame Encoder stores every block, src/lz4.rs:543-545) ----
 * LZ4 high compression: one input block -> one LZ4 block that rcx_lz4_decode_batch (and the reference's BlockDecoder) reads, usually
 * smaller than rcx_lz4_encode_batch's.  Hash chains of 4-byte prefixes searched up to a depth that grows with `level`, then a min-cost
 * parse; matches reach back up to 65535 bytes (also across the encoder's internal 64 KiB segments).  Levels and chain depths:
 *     level  1  2  3  4  5  6   7   8   9   10   11   12
 *     depth  1  2  3  4  6  8  12  16  24   64  128  256
 * The block format's end rules hold: the last 5 bytes are literals, the last match starts 12 bytes before the end at the latest, the
 * final sequence is literals only.  Statuses and bound as rcx_lz4_encode_batch: a block longer than 0x7E000000 bytes gets
 * RCX_E_LZ4_INPUT_TOO_LARGE, a slot smaller than rcx_lz4_compression_bound(n) RCX_E_OUTPUT_TOO_SMALL (nothing of it is written); on
 * success in_used[i] = in_len[i].  The output is deterministic (the same bytes for the same input and level at any position of any
 * batch), and nothing outside [out_off[i], out_off[i] + out_len[i]) is written.  A level outside 1..12 returns RCX_RC_BAD_ARG.
 * rcx_launch_dev(ctx, RCX_LZ4_ENCODE, ...) runs this encoder when rcx_ctx_set_param(ctx, RCX_LZ4_ENCODE, level) set a level of 1..12
 * (0, the default, is the reference's encoder) and needs rcx_lz4_hc_scratch_bytes(nblocks, max_block) of scratch: too little and the
 * blocks it does not cover get RCX_E_MALFORMED. */
int rcx_lz4_encode_hc_batch(rcx_ctx*, const rcx_batch*, int level);
uint64_t rcx_lz4_hc_scratch_bytes(uint32_t nblocks, uint64_t max_block);

/* ---- extension beyond the reference: the LZ4 frame format's two device capabilities (lz4_Frame_format.md; the reference's frame
 * types skip every checksum and break on dependent blocks).  rust_compress_amd/lz4frame.py builds conforming frames on them.
 * XXH32 (the frame format's header, block and content checksum) of every block: hash[i] = XXH32(block i, seed); out_base, out_off,
 * out_cap and out_len are unused, in_used[i] = in_len[i].  Any length up to 2^32 - 1 and any alignment of in_off.  A stream is a serial
 * chain (the round does not combine across chunks the way CRC-32 and Adler-32 do): the rate comes from the batch.  Measured on MI355X,
 * device memory: 4096 x 64 KiB in 0.151 ms a call (1659 GiB/s), one 256 MiB stream 368.7 ms (0.68 GiB/s). */
int rcx_xxh32_batch(rcx_ctx*, const rcx_batch*, uint32_t seed, uint32_t* hash);
/* LZ4 block decode with HISTORY: linked blocks and dictionaries.  link and dict_len are host arrays of nblocks entries, or NULL (= all 0).
 *   link[i] == 0, a chain head: block i decodes into its slot as in rcx_lz4_decode_batch, and its matches may also reach into the
 *     dict_len[i] (at most 65536, at most out_off[i]) bytes that lie directly before out_base + out_off[i].  The caller put them there;
 *     they are read and never written.
 *   link[i] == 1 (not for i = 0): block i continues block i-1's chain.  out_off[i] and out_cap[i] are ignored: its output starts where
 *     block i-1's ended, the whole chain shares the head's out_cap, and its matches reach back up to 65535 bytes into what the chain has
 *     produced and the head's dictionary.  out_len[i] is the block's own byte count: the block's bytes start at the head's out_off plus
 *     the out_len of the chain's blocks before it (the library reports no offsets of its own).
 * status: a match offset of 0 or beyond produced + history is RCX_E_MALFORMED; the block of a chain that does not fit the rest of the
 * head's out_cap gets RCX_E_OUTPUT_TOO_SMALL; every block after a failed one of its chain gets RCX_E_LZ4_HISTORY and out_len 0; other
 * chains are not affected.  Nothing outside a head's [out_off, out_off + out_cap) is written.  With link and dict_len NULL the results
 * (bytes, out_len, in_used, status) are those of rcx_lz4_decode_batch.  A batch costs one launch per block of its longest chain, stream
 * ordered, no host wait in between; one wave decodes a block (k_lz4_decode_v4's decoder, started behind its history).  Measured on
 * MI355X, device memory: 4096 independent 64 KiB text blocks 0.943 ms a call (rcx_lz4_decode_batch: 0.501), 256 chains of 16 blocks
 * 10.1 ms.  From host memory only the dictionaries are copied in and only the bytes the chains wrote are copied back. */
int rcx_lz4_decode_linked_batch(rcx_ctx*, const rcx_batch*, const uint8_t* link, const uint64_t* dict_len);
/* LZ4 high compression with HISTORY: what writes linked blocks and blocks behind a dictionary.  hist_len is a host array of nblocks
 * entries, or NULL (= all 0).  Block i is encoded exactly as rcx_lz4_encode_hc_batch encodes it (levels, chain depths, end rules,
 * statuses, bound, in_used), and its matches may also reach into the hist_len[i] (at most 65536, at most in_off[i]) bytes that lie
 * directly before in_base + in_off[i] -- the mirror of dict_len above.  The caller put them there; they are read and never written, and
 * they may be another block's input: in a linked frame block k's history is block k-1, and every block of the frame is encoded at once
 * (all input is known up front: no rounds, no chains, no launch order).  Of 65536 history bytes the first is out of every match's reach
 * (65536 counts as 65535).  hist_len[i] > in_off[i] or > 65536 returns RCX_RC_BAD_ARG and rcx_last_error names the block.
 * No emitted offset exceeds position + hist_len[i] or 65535; no byte in front of the history influences the output; the output is
 * deterministic and does not depend on the block's place in the batch.  With hist_len NULL or all 0 every result (bytes, out_len,
 * in_used, status) is rcx_lz4_encode_hc_batch's at the same level.  The blocks decode with rcx_lz4_decode_linked_batch given
 * dict_len[i] = hist_len[i] and the history in front of the slot.
 * COST: the hash chains of a history are REBUILT for every block that names it, by one more workgroup per block (one more 64 KiB
 * segment of 16-bit links per block with history: rcx_lz4_hc_hist_scratch_bytes counts every block with one) -- up to twice the chain
 * work for linked 64 KiB blocks, 17 times for a 2 KiB record behind a 32 KiB dictionary.  A dictionary's table built once and attached
 * to many blocks, and history that is not contiguous with the block: rcx_lz4_encode_hc_shared_batch.  benchmarks/lz4_hist_rate.py
 * measures the rebuild. */
int rcx_lz4_encode_hc_hist_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* hist_len);
uint64_t rcx_lz4_hc_hist_scratch_bytes(uint32_t nblocks, uint64_t max_block);

/* ---- DEFLATE / zlib / Adler-32 ---------------------------------------------- */
/* reference: src/flate.rs:195-206,237-246,262-341,343-450 (one RFC-1951 stream
 * per block, decoded to BFINAL). flags may be NULL.
 * RCX_MEM_HOST with a PAGE-LOCKED out_base: as rcx_lz4_decode_batch -- rcx_inflate_batch, rcx_zlib_decode_batch and rcx_gzip_decode_batch
 * store the decoded bytes straight into the caller's buffer while the launch runs (streams the fast kernel hands to the exact one
 * arrive by a copy behind it); same results as with pageable buffers.  rcx_ctx_set_param(ctx, <codec>, 1) keeps the plain copies. */
int rcx_inflate_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags);
/* reference: src/zlib.rs:55-126 (header checks, inflate, Adler-32 BE trailer) */
int rcx_zlib_decode_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags);
/* reference: src/checksum/adler.rs:22-51; out_len/out_base unused,
 * adler[i] = State32::result() of block i */
int rcx_adler32_batch(rcx_ctx*, const rcx_batch*, uint32_t* adler);
/* ---- extension beyond the reference ("gzip members" of BASELINE config 3) ----
 * The reference has RFC 1950 (zlib) framing only, src/zlib.rs:55-126; these two follow its structure for RFC 1952.
 * crc[i] = CRC-32 (IEEE 802.3, as in the gzip trailer) of block i; out_len/out_base unused. */
int rcx_crc32_batch(rcx_ctx*, const rcx_batch*, uint32_t* crc);
/* one gzip member per block: header (FEXTRA/FNAME/FCOMMENT/FHCRC skipped), DEFLATE stream decoded to BFINAL,
 * CRC32 + ISIZE trailer verified; in_used[i] = bytes of the member.  flags as rcx_inflate_batch. */
int rcx_gzip_decode_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags);
/* ---- extension beyond the reference (it has no DEFLATE encoder) ----
 * One input block -> one complete raw DEFLATE stream (RFC 1951), zlib stream (RFC 1950: 78 01, Adler-32 big-endian) or gzip member
 * (RFC 1952: 10-byte header, no optional fields, MTIME 0, OS 255; CRC-32 and ISIZE little-endian).  Greedy LZ77 over a 32 KiB window
 * (also across the encoder's internal 64 KiB segments), one block per segment, each the cheapest of stored, fixed and dynamic Huffman;
 * no block decodes to zero bytes except the lone final block of an empty input.  The output is deterministic: the same bytes for the
 * same input at any position of any batch.  On success out_len[i] = bytes written, in_used[i] = in_len[i].  A slot smaller than the
 * stream gets RCX_E_OUTPUT_TOO_SMALL (out_len 0) and nothing of it is written.  rcx_launch_dev needs
 * rcx_scratch_bytes(codec, nblocks, max_block) of scratch: too little and the streams it does not cover get RCX_E_MALFORMED.
 * A block may be up to 2^32 - 1 bytes; a longer one gets RCX_E_MALFORMED through rcx_launch_dev (the batch calls refuse it). */
int rcx_deflate_encode_batch(rcx_ctx*, const rcx_batch*);
int rcx_zlib_encode_batch(rcx_ctx*, const rcx_batch*);
int rcx_gzip_encode_batch(rcx_ctx*, const rcx_batch*);
/* largest raw DEFLATE stream of n input bytes; a zlib stream needs 6 bytes more, a gzip member 18 */
uint64_t rcx_deflate_compression_bound(uint64_t n);
/* The same encoders at a compression level of 1..9.  Level 1 is rcx_*_encode_batch, byte for byte.  Levels 2..9 search hash chains
 * of 4-byte prefixes for every position's longest match (at most 258 bytes, 32 KiB back, also across the internal segments) up to a
 * depth that grows with the level, then choose the tokens by a min-cost parse priced in bits by Huffman code lengths of a first
 * parse (the greedy one); from level 7 on the parse runs a second time, priced by the first one's own code lengths:
 *     level   1       2  3   4   5   6   7   8    9
 *     depth   greedy  4  8  16  32  64  96  160  256
 *     parses  -       1  1   1   1   1   2   2    2
 * Each block is still the cheapest of stored, fixed, dynamic Huffman and dynamic all-literals, so rcx_deflate_compression_bound
 * holds at every level.  Header fields by level, as zlib sets them: zlib FLEVEL 78 01 (level 1), 78 5E (2-5), 78 9C (6), 78 DA
 * (7-9); gzip XFL 2 at level 9, else 0.  Statuses, slots, determinism and the 2^32 - 1 byte limit as above.  A level outside 1..9
 * returns RCX_RC_BAD_ARG.  rcx_launch_dev(ctx, RCX_{DEFLATE,ZLIB,GZIP}_ENCODE, ...) runs level rcx_ctx_set_param(ctx, codec, level):
 * 0 (the default) and 1 the level-1 encoder, 2..9 these, anything else RCX_RC_BAD_ARG; levels 2..9 need
 * rcx_deflate_level_scratch_bytes(nblocks, max_block) of scratch (enough for any level and framing): too little and the streams it
 * does not cover get RCX_E_MALFORMED. */
int rcx_deflate_encode_level_batch(rcx_ctx*, const rcx_batch*, int level);
int rcx_zlib_encode_level_batch(rcx_ctx*, const rcx_batch*, int level);
int rcx_gzip_encode_level_batch(rcx_ctx*, const rcx_batch*, int level);
uint64_t rcx_deflate_level_scratch_bytes(uint32_t nblocks, uint64_t max_block);
/* DEFLATE and zlib at levels 2..9 with HISTORY (extension): zlib's preset dictionary (deflateSetDictionary, Python's zdict=), and
 * chunks of one stream each primed with the 32 KiB before it.  hist_len is a host array of nblocks entries, or NULL (= all 0).  Block
 * i is encoded exactly as rcx_deflate_encode_level_batch encodes it at that level (depths, parses, block-type choice, statuses,
 * determinism, in_used, rcx_deflate_compression_bound), and its matches may also reach into the hist_len[i] (at most 32768, at most
 * in_off[i]) bytes that lie directly before in_base + in_off[i].  The caller put them there; they are read and never written, and
 * they may be another block's input.  ALL 32768 history bytes are within reach (DEFLATE's largest distance is 32768; LZ4's "65536
 * counts as 65535" does not apply).  hist_len[i] > in_off[i] or > 32768 returns RCX_RC_BAD_ARG and rcx_last_error names the block.
 * No emitted distance exceeds position + hist_len[i] or 32768; no byte in front of the history influences the output.  With hist_len
 * NULL or all 0 every result is rcx_deflate_encode_level_batch's at that level, byte for byte.
 * A level outside 2..9 returns RCX_RC_BAD_ARG: LEVEL 1 HAS NO HISTORY (its encoder has a hash finder of its own in LDS; as the
 * greedy LZ4 encoder has none).  gzip has no dictionary and no variant.
 * rcx_zlib_encode_dict_batch: where hist_len[i] > 0 the stream carries FDICT -- CMF/FLG with bit 5 set (FLEVEL as at that level,
 * FCHECK recomputed), dict_id[i] big-endian, the DEFLATE data, the Adler-32 of the BLOCK alone -- and the slot needs the raw bound
 * + 10; where hist_len[i] == 0 the stream is rcx_zlib_encode_level_batch's, byte for byte.  dict_id is the caller's: the Adler-32 of
 * whatever dictionary the decoder will be handed, which may be longer than the 32 KiB that count; the library does not compute it.
 * COST: the hash chains of a history are REBUILT for every block that names it, by one more workgroup per block, and take one more
 * 64 KiB segment of 16-bit links (128 KiB) per block with history: rcx_deflate_hist_scratch_bytes counts every block with one.  For
 * 64 KiB chunks linked by 32 KiB that is half as much chain work again, for a 2 KiB record behind a 32 KiB dictionary 17 times the
 * record's.  A dictionary's table built once and shared, and history that is not contiguous with the block: rcx_*_encode_shared_batch.
 * Measured on an MI355X, device memory, median of 10 calls at level 6: 4096 x 64 KiB blocks 224.3 ms with hist_len NULL (the level call:
 * 212.0), linked by 32 KiB 281.7 ms; 65536 x 2 KiB records 259.6 ms alone, 1033.2 ms behind a replicated 32 KiB dictionary
 * (benchmarks/deflate_hist_rate.py). */
int rcx_deflate_encode_hist_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* hist_len);
int rcx_zlib_encode_dict_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* hist_len, const uint32_t* dict_id);
uint64_t rcx_deflate_hist_scratch_bytes(uint32_t nblocks, uint64_t max_block);
/* The encoders behind SHARED DICTIONARIES (extension): many small records behind few dictionaries, without a copy of the dictionary in
 * front of every record and without rebuilding its hash chains for every record.  dict_off and dict_len are host arrays of nblocks
 * entries.  The history of block i is the dict_len[i] bytes at in_base + dict_off[i]: anywhere in the input buffer, before or after the
 * block, overlapping other blocks' input or other dictionaries; read and never written.  dict_len[i] == 0: no dictionary, dict_off[i] is
 * ignored.  Blocks that name the same range (the same offset and length after the clamp below) share one table, built once per call.
 * With both arrays NULL the results are rcx_lz4_encode_hc_batch's / rcx_{deflate,zlib}_encode_level_batch's; one NULL and the other not
 * is RCX_RC_BAD_ARG.
 * BYTES: every block's output bytes, out_len, in_used and status are exactly what rcx_lz4_encode_hc_hist_batch /
 * rcx_deflate_encode_hist_batch / rcx_zlib_encode_dict_batch produce at the same level for the same block with the same dict_len[i]
 * bytes copied directly in front of it -- levels (LZ4 1..12, DEFLATE and zlib 2..9, anything else RCX_RC_BAD_ARG), end rules, bounds,
 * statuses, determinism, the zlib form's FDICT, FCHECK, dict_id[i] big-endian and the block's own Adler-32 (the slot needs the raw bound
 * + 10) included.  Of 65536 LZ4 dictionary bytes the first is out of reach: a dictionary is clamped to its last 65535 bytes before
 * ranges are compared; all 32768 DEFLATE dictionary bytes are within reach.  dict_len[i] above 65536 (LZ4) or 32768 (DEFLATE) is
 * RCX_RC_BAD_ARG and rcx_last_error names the block.  No emitted distance exceeds position + dict_len[i]; the output depends neither on
 * the block's place in the batch nor on which other blocks share its dictionary; and NO NEIGHBOURING BYTE influences it, in front of a
 * dictionary or behind its end: a match whose source starts in the dictionary and runs past its last byte continues in the block's
 * first bytes.  From RCX_MEM_HOST the span that travels in covers the dictionaries' ranges as well as the blocks'.
 * SCRATCH: 256 KiB (LZ4; DEFLATE 192 KiB) per DISTINCT dictionary -- its bucket table and its 16-bit links -- and 8 bytes per block
 * beyond what the encoders without history take: rcx_*_shared_scratch_bytes(nblocks, max_block, ndict), ndict = the distinct
 * dictionaries.  The batch calls size it themselves.
 * COST PER BLOCK: the workgroup of a block's first segment copies its dictionary's whole bucket table, 128 KiB, from device memory
 * into LDS before it links the block (one workgroup a CU), however small the block; for 2 KiB records that copy, not the record, is
 * most of the call (the times below).  Records much smaller than the table would want several records a workgroup behind one copy,
 * which is not built.
 * The blocks decode behind the same ranges with rcx_lz4_decode_shared_batch / rcx_inflate_shared_batch / rcx_zlib_decode_shared_batch
 * below (or, given the dictionary in front of the slot, with rcx_lz4_decode_linked_batch / rcx_inflate_hist_batch /
 * rcx_zlib_decode_dict_batch).
 * NOT PROVIDED: lz4frame.encode_frames taking this call for independent blocks with a dictionary; level 1, gzip and the greedy LZ4
 * encoder.
 * The ids RCX_*_SHARED name the entry points to rcx_ctx_set_variant / rcx_ctx_set_param; rcx_launch_dev does not take them (the
 * dictionaries' words come from the host's plan).  Measured on an MI355X, device memory, 65536 x 2 KiB text records behind one 32 KiB
 * dictionary, median of 10 calls: LZ4 HC level 9 83.8 ms (the history call on the replicated layout: 795.5), DEFLATE level 6 272.5 ms
 * (1033.7); benchmarks/dict_shared_rate.py, DESIGN.md 3.17. */
int rcx_lz4_encode_hc_shared_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* dict_off, const uint64_t* dict_len);
int rcx_deflate_encode_shared_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* dict_off, const uint64_t* dict_len);
int rcx_zlib_encode_shared_batch(rcx_ctx*, const rcx_batch*, int level, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id);
uint64_t rcx_lz4_hc_shared_scratch_bytes(uint32_t nblocks, uint64_t max_block, uint32_t ndict);
uint64_t rcx_deflate_shared_scratch_bytes(uint32_t nblocks, uint64_t max_block, uint32_t ndict);
/* The decoders behind SHARED DICTIONARIES (extension): the mirror of the three encoders above -- many small records read behind few
 * dictionaries without a copy of the dictionary in front of every output slot.  dict_off and dict_len are host arrays of nblocks
 * entries.  The history of block i is the dict_len[i] bytes at in_base + dict_off[i], in the INPUT buffer beside the compressed blocks:
 * before or after them, overlapping other dictionaries or other blocks' input; read and never written.  dict_len[i] == 0: no
 * dictionary, dict_off[i] is ignored.  out_off[i] is free: it may be 0, or smaller than dict_len[i] (which the history calls refuse),
 * and no address below out_base + out_off[i] is dereferenced for block i.
 * BYTES: for every block the output bytes [out_off[i], out_off[i] + out_len[i]), out_len, in_used, status and (the DEFLATE forms)
 * flags are exactly what the history decoder produces for the same block with the same dictionary bytes copied directly in front of
 * its slot -- rcx_lz4_decode_linked_batch with link all 0 and the same dict_len[i], rcx_inflate_hist_batch, rcx_zlib_decode_dict_batch
 * with the same dict_id -- for malformed input too.  So: an LZ4 dictionary is at most 65536 bytes, of which the last 65535 count; a
 * DEFLATE dictionary at most 32768, all within reach; a longer dict_len[i] returns RCX_RC_BAD_ARG and rcx_last_error names the block.
 * A distance of exactly output so far + dictionary reaches the dictionary's first byte; one more is RCX_E_MALFORMED (LZ4) or
 * RCX_E_INVALID_HUFFMAN_CODE (DEFLATE), whatever lies in front of the dictionary in memory.  A match whose source starts in the
 * dictionary and runs past its last byte continues in the block's own first bytes (which may be the ones the match itself produces),
 * never in what follows the dictionary in the buffer: no byte outside [dict_off, dict_off + dict_len) and the block's own input is
 * loaded on the dictionary's behalf, and a dictionary may end at the buffer's last byte.  The zlib form: FDICT, DICTID,
 * RCX_E_ZLIB_DICT, RCX_E_ZLIB_DICT_ID, "no FDICT: the dictionary is ignored" and the Adler-32 of the block alone as in
 * rcx_zlib_decode_dict_batch.  Nothing outside [out_off[i], out_off[i] + out_cap[i]) is written; the results depend neither on a
 * block's place in the batch nor on which other blocks name its dictionary.
 * With both arrays NULL the call is rcx_lz4_decode_batch / rcx_inflate_batch / rcx_zlib_decode_batch; one NULL and the other not is
 * RCX_RC_BAD_ARG, and so is the zlib form with dictionaries and a NULL dict_id.
 * From RCX_MEM_HOST the span that travels in covers the dictionaries' ranges as well as the blocks'; nothing of the output buffer
 * travels in, and only what was produced travels back (the history calls stage the whole output buffer, or every replica of the
 * dictionary, in).  No scratch beyond the plain decoders': nothing is built per dictionary.
 * KERNELS: DEFLATE / zlib one lane per stream (k_inflate_hist's kernel with a split far source, k_inflate_dict.hip); LZ4 one wave per
 * block, parsed wave-uniformly and copied 64 lanes wide straight between device memory and registers, no LDS window
 * (k_lz4_dict.hip) -- rcx_lz4_decode_linked_batch runs k_lz4_decode_v4's windowed decoder.
 * NOT PROVIDED: LZ4 chains (`link`) whose head names a shared dictionary; lz4frame.py taking these calls; dictionary streams through
 * the wave-per-stream inflate kernel; rcx_launch_dev taking the ids RCX_*_DECODE_SHARED / RCX_INFLATE_SHARED (the dictionaries' words
 * come from the host's plan: a device-resident batch goes through these calls with RCX_MEM_DEVICE, as for the encoders).
 * Measured on an MI355X, 65536 x 2 KiB text records behind one 32 KiB dictionary (LZ4 HC level 9, DEFLATE level 6), median of 10
 * calls, the history call on the replicated layout against the shared call: from pageable host memory LZ4 1627.4 against 6.9 ms
 * (2.18 GB of replicas in 65536 copies against 35.4 MB) and DEFLATE 86.1 against 8.0 ms (2.31 GB in and 2.28 GB out against 28.5 MB
 * and 134 MB); output buffer 2 281 701 376 against 134 217 728 bytes.  DEVICE-RESIDENT THE SHARED CALLS ARE SLOWER: LZ4 2.504
 * against 0.920 ms (2.7 times: one sequence at a time, each behind an L2 round trip, where k_lz4_decode_v4 executes batches of 64
 * sequences in an LDS window), DEFLATE 4.832 against 4.213 ms (the position test in front of every far gather).  No LDS window was
 * built: it would not take the dictionary and literal loads out of a sequence's chain (benchmarks/dict_decode_rate.py, DESIGN.md
 * 3.18). */
int rcx_lz4_decode_shared_batch(rcx_ctx*, const rcx_batch*, const uint64_t* dict_off, const uint64_t* dict_len);
int rcx_inflate_shared_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags, const uint64_t* dict_off, const uint64_t* dict_len);
int rcx_zlib_decode_shared_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id);
/* Inflate with HISTORY (extension; the mirror of dict_len in rcx_lz4_decode_linked_batch).  Stream i decodes into its slot, and its
 * matches may reach into the hist_len[i] (at most 32768, at most out_off[i]; anything else RCX_RC_BAD_ARG naming the block) bytes
 * that lie directly before out_base + out_off[i].  The caller put them there; they are read and never written.  A distance beyond
 * output so far + hist_len[i], or beyond 32768, is RCX_E_INVALID_HUFFMAN_CODE (flate.rs:314 with the history counted in).  Every
 * other status, in_used, flags and out_len (the block's own bytes) is rcx_inflate_batch's; with hist_len NULL or all 0 so are all
 * results.  One lane per stream (the kernel of rcx_inflate_batch's exact path); the wave-per-stream kernel takes no history.
 * rcx_zlib_decode_dict_batch: FDICT set and hist_len[i] > 0 -- four DICTID bytes follow the header, count in in_used and must equal
 * dict_id[i] (big-endian), else RCX_E_ZLIB_DICT_ID with out_len 0; FDICT set and hist_len[i] == 0 -- RCX_E_ZLIB_DICT, as
 * rcx_zlib_decode_batch; FDICT clear -- the history is ignored (libz never asks for one) and the result is rcx_zlib_decode_batch's.
 * The Adler-32 trailer covers the decoded block only. */
int rcx_inflate_hist_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags, const uint64_t* hist_len);
int rcx_zlib_decode_dict_batch(rcx_ctx*, const rcx_batch*, uint32_t* flags, const uint64_t* hist_len, const uint32_t* dict_id);

/* ---- BWT / MTF / DC --------------------------------------------------------- */
/* reference: src/bwt/mod.rs:136-219 compute_suffixes + TransformIterator.
 * out block i receives L (n bytes); origin[i] = get_origin(). */
int rcx_bwt_forward_batch(rcx_ctx*, const rcx_batch*, uint32_t* origin);
/* reference: src/bwt/mod.rs:136-166 compute_suffixes (pub): the sorted suffix array itself.  out block i receives n
 * little-endian u32 suffix indices (out_cap >= 4n, the slot 4-byte aligned; out_len = 4n); origin[i] (may be NULL) =
 * the position of suffix 0, what TransformIterator::get_origin reports for the same array. */
int rcx_bwt_suffixes_batch(rcx_ctx*, const rcx_batch*, uint32_t* origin);
/* reference: src/bwt/mod.rs:223-239 compute_inversion_table (pub): in block i = L (n bytes), origin[i]; out block i receives
 * the n little-endian u32 table entries (out_cap >= 4n, 4-byte aligned; out_len = 4n): table[place(L[origin])] = 0, then
 * table[place(L[j])] = j + 1 for every other j in order.  status: origin >= n is RCX_E_MALFORMED (the index panic of :230,
 * also for an empty block). */
int rcx_bwt_inversion_table_batch(rcx_ctx*, const rcx_batch*, const uint32_t* origin);
/* reference: src/bwt/mod.rs:223-294 compute_inversion_table + InverseIterator */
int rcx_bwt_inverse_batch(rcx_ctx*, const rcx_batch*, const uint32_t* origin);
/* reference: src/bwt/mod.rs:298-315 decode_minimal, what bwt::Decoder runs with extra_mem = false (:397-399): n steps of
 * i <- C[L[i]] + #{k < i : L[k] == L[i]} from i = origin, the text written backwards.  Reproduced as the reference computes
 * it, which is NOT the inverse of rcx_bwt_forward_batch in general (wrong whenever T[n-1] also occurs in L[..origin]; right
 * for e.g. "abracadabra", the reference's only test of it, :549-551).  status: origin >= n is RCX_E_MALFORMED (:310),
 * n == 0 is RCX_OK only with origin == 0 (:300-302); there is no other failure. */
int rcx_bwt_inverse_minimal_batch(rcx_ctx*, const rcx_batch*, const uint32_t* origin);
/* reference: src/bwt/mtf.rs:63-90 with the stream codecs' identity start :103,141 */
int rcx_mtf_encode_batch(rcx_ctx*, const rcx_batch*);
int rcx_mtf_decode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/bwt/dc.rs:110-159 encode_simple::<u32> order: out block i =
 * little-endian u32 words: 256 x init, then k distances (out_len = 4*(256+k)).
 * The slot is the encoder's work array: it must hold 4*(256+n) bytes (n = in_len[i]; less: RCX_E_OUTPUT_TOO_SMALL) and be
 * 4-BYTE ALIGNED -- the kernels address the words as uint32_t.  With RCX_MEM_DEVICE that is the address out_base + out_off[i],
 * with RCX_MEM_HOST the offset out_off[i] (the bytes are staged at an aligned address).  The batch calls refuse a word buffer
 * anywhere else with RCX_RC_BAD_ARG and rcx_last_error names the block; through rcx_launch_dev such a block gets
 * RCX_E_OUTPUT_TOO_SMALL (encode) or RCX_E_MALFORMED (decode) and the rest of the batch is coded. */
int rcx_dc_encode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/bwt/dc.rs:162-252 decode_simple; in = the words above (4-byte aligned in the same sense: in_base + in_off[i],
 * or in_off[i] from host memory), n_out[i] = decoded length n (dc carries no length itself) */
int rcx_dc_decode_batch(rcx_ctx*, const rcx_batch*, const uint64_t* n_out);
/* The same two with the coding CONTEXT of every distance (reference: src/bwt/dc.rs:40-58 `Context`; yielded next to each
 * distance by EncodeIterator :88-103, handed to decode's distance callback :199-229; the reference's test :268-289 checks
 * that the two sides see the same contexts).  A context is 8 bytes: u32 LE symbol | last_rank << 8, u32 LE distance_limit.
 * The word buffers (the encoder's slot, the decoder's input) are 4-byte aligned as above, and a misaligned one is refused the same way.
 *   encode: block i's slot must hold 4*(256+n) + 8*n bytes (n = in_len[i]); words as above in its first 4*(256+k) bytes,
 *           the k contexts from byte 4*(256+n) on; out_len[i] = 4*(256+n) + 8*k.
 *   decode: the slot must be 8-byte aligned and hold ((n+7)&~7) + 8*(in_len[i]/4 - 256) bytes; the n decoded bytes first,
 *           one context per distance consumed from byte (n+7)&~7 on; out_len[i] = that offset + 8 * (distances consumed). */
int rcx_dc_encode_ctx_batch(rcx_ctx*, const rcx_batch*);
int rcx_dc_decode_ctx_batch(rcx_ctx*, const rcx_batch*, const uint64_t* n_out);

/* ---- adaptive byte range coder ---------------------------------------------- */
/* reference: src/entropy/ari/table.rs:185-224 ByteEncoder::write + finish
 * (RangeEncoder::process mod.rs:117-150, table::Model :69-117) */
int rcx_ari_byte_encode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/entropy/ari/table.rs:229-273 ByteDecoder::read (+ finish);
 * in_used[i] = bytes consumed so the next stream stays addressable */
int rcx_ari_byte_decode_batch(rcx_ctx*, const rcx_batch*);
uint64_t rcx_ari_byte_encode_bound(uint64_t in_len);
/* The crate's other two models have no stream codec; these entry points drive them exactly as the reference's
 * tests do.  reference: src/entropy/ari/bin.rs:17-103 bin::Model::new_flat(RANGE_DEFAULT_THRESHOLD >> 3, rate),
 * 8 decisions per byte LSB first (src/entropy/ari/test.rs:22-50).  rate must be 1..31.  The coding has no end
 * marker: the decoder produces exactly out_cap[i] bytes.  Encoded size <= rcx_ari_byte_encode_bound(n). */
int rcx_ari_binary_encode_batch(rcx_ctx*, const rcx_batch*, uint32_t rate);
int rcx_ari_binary_decode_batch(rcx_ctx*, const rcx_batch*, uint32_t rate);
/* reference: table::SumProxy (table.rs:127-180, weights 2:1 >> 0, update 10/5) for the high nibble + bin::SumProxy
 * (bin.rs:112-167, weights 1:1 >> 1, rates 3 and 5) for the low 4 bits, as src/entropy/ari/test.rs:91-148 */
int rcx_ari_proxy_encode_batch(rcx_ctx*, const rcx_batch*);
int rcx_ari_proxy_decode_batch(rcx_ctx*, const rcx_batch*);
/* reference: apm::Bit passed through an apm::Gate, update(rate 10, bias 0), 8 decisions per byte LSB first, as
 * src/entropy/ari/test.rs:150-182 (apm.rs:36-198).  The f32 ln / exp of Bit::to_wide / from_wide are evaluated on the
 * host with libm's logf / expf (what Rust's f32::ln / exp call) into a 4096-entry stretch table and the 17 initial
 * gate bins; the device code is integer only.  A status of RCX_E_MALFORMED on ENCODE means the reference panics on
 * that input (a skewed enough bit history drives the gate index out of its 17 bins, apm.rs:162-166).  The decoder
 * produces exactly out_cap[i] bytes. */
int rcx_ari_apm_encode_batch(rcx_ctx*, const rcx_batch*);
int rcx_ari_apm_decode_batch(rcx_ctx*, const rcx_batch*);

/* ---- RLE -------------------------------------------------------------------- */
/* reference: src/rle.rs:82-122 (one-shot write + finish) */
int rcx_rle_encode_batch(rcx_ctx*, const rcx_batch*);
/* reference: src/rle.rs:194-259 */
int rcx_rle_decode_batch(rcx_ctx*, const rcx_batch*);
uint64_t rcx_rle_encode_bound(uint64_t in_len);

/* ---- dictionary training (extension: the reference has no trainer) ------------------------------------------------------------
 * Makes the dictionaries the calls with history and behind shared dictionaries take as given: for each of many independent corpora
 * it selects the segments that cover the most frequent substrings -- COVER (Liao, Petri, Moffat, Wirth 2016) in the hashed form zstd
 * calls "fastcover" -- and writes a RAW-CONTENT dictionary, what LZ4 and zlib take.  Block i of the batch is job i: in_off / in_len the
 * corpus, the concatenation of nsamples[i] samples whose lengths are the next nsamples[i] entries of the flat host array sample_len
 * (job order; lengths of 0 are allowed); out_off / out_cap the dictionary's slot and its capacity C.  d is the length of the hashed
 * substrings (6 or 8), k the length of a segment (d .. 4096), f the log2 of the frequency table (10 .. 22).
 *   contract   the bytes are DEFINED by the specification in DESIGN.md 3.19 (epochs of max(1, C / k / 4), the start with the greatest
 *              sum of the frequencies of its segment's DISTINCT hashes, ties to the lowest start, trimmed, its frequencies zeroed,
 *              copied to the dictionary's end first; ten rounds in a row without a start end the job) and equal the serial reference of
 *              tests/dict_train_ref byte for byte.  The dictionary is delivered at the slot's START: out_len[i] <= C, in_used[i] =
 *              in_len[i], status RCX_OK.  A corpus shorter than k, a capacity below d or a corpus without a whole substring give
 *              out_len 0 with RCX_OK.  Slot bytes beyond out_len are unspecified; nothing outside the slots is written.  The result
 *              depends on the corpus, the sample lengths, k, d, f and C alone: not on the job's place, its neighbours or `mem`.
 *   limits     at most 65535 jobs a call; a corpus and a capacity below 4 GiB.  RCX_RC_BAD_ARG, with the job named by
 *              rcx_last_error: sample lengths that do not add up to in_len[i], in_len[i] >= 2^32, d other than 6 or 8, k or f out of
 *              range, a null array.  nblocks == 0 is RCX_RC_OK.
 *   scratch    rcx_dict_train_scratch_bytes(njobs, max_corpus, max_cap, k, f): per job 10 bytes per corpus byte (hash words, distances,
 *              score differences) + 4 << f for the frequencies + C; the batch call allocates what the real sizes take in the context.
 *   cost       one pass to hash and count, one to find every position's previous occurrence (k - d LDS reads a position), then four
 *              launches a ROUND for all live jobs together, each O(epoch), about C / k rounds and a few; the call is synchronous and
 *              reads one word back every eight rounds to stop when every job is done.  Measurements: DESIGN.md 3.19.
 *   not here   zstd's dictionary header and entropy tables; a search over k and d (batch the parameter sets as separate calls);
 *              rcx_launch_dev, which does not take RCX_DICT_TRAIN, as it takes none of the *_SHARED ids. */
int rcx_dict_train_batch(rcx_ctx*, const rcx_batch*, const uint32_t* nsamples, const uint64_t* sample_len, uint32_t k, uint32_t d, uint32_t f);
uint64_t rcx_dict_train_scratch_bytes(uint32_t njobs, uint64_t max_corpus, uint64_t max_cap, uint32_t k, uint32_t f);

/* ---- bzip2 (extension: the reference's block-sorting container is its own bwt | mtf/dc | ari pipeline, which no other tool reads) ----
 * DECODE of .bz2 files as bzip2 / libbz2 write them.  Block i of the batch is one whole FILE: one or more concatenated streams, optionally
 * followed by other bytes; its decoded bytes go to its output slot.
 *   results    success: RCX_OK, out_len[i] = the decoded size, in_used[i] = the byte just after the last accepted stream's padding (a
 *              following stream is one whose first 4 bytes are BZh1..BZh9, and its errors count; anything else ends the file with RCX_OK).
 *              The file decodes but out_cap[i] is too small: RCX_E_OUTPUT_TOO_SMALL and out_len[i] = the exact size needed -- every
 *              block and stream CRC has been checked by then, one retry suffices, and out_cap = 0 is a size query.  Any other failure:
 *              the first failure in stream order, out_len 0, in_used 0.  RCX_E_EOF: the input ends inside a stream (also a file
 *              shorter than 4 bytes).  RCX_E_BZ2_DATA: everything the format calls an error that has no status of its own, among
 *              them more than 18002 selectors.  Nothing outside a file's own slot is written, a failing file affects no other, and
 *              a slot is written only up to the blocks that had passed their CRC when the failure was found.
 *   oracle     bytes, out_len, in_used and accept / reject are libbz2's, with two exceptions: randomised blocks, which libbz2 still
 *              reads, are refused (RCX_E_BZ2_RANDOMISED); and a crafted block whose L is the BWT of nothing, with a cycle through
 *              origPtr that does not divide the block's length, is RCX_E_BZ2_BLOCK_CRC here where libbz2, which walks the cycle the
 *              other way round, accepts it when the CRC is that of its own walk (no encoder writes such a block).
 *   limits     a file and a slot below 4 GiB; at most 65535 files a call (more: RCX_RC_BAD_ARG).
 *   knob       rcx_ctx_set_param(ctx, RCX_BZIP2_DECODE, r): block candidates a round, 64..4096; 0 (the default) is 1536.  The one
 *              parameter of an extension id, and this call reads it.
 *   stages     a scan of every bit position for the two 48-bit marks and of every byte position for BZh1..9; one wave per block mark
 *              decodes speculatively (Huffman, selectors, MTF, RUNA/RUNB) into scratch; the host chains the candidates into streams
 *              (rcx_plan_bz2_chain) and drops the marks that occurred inside data; rcx_bwt_inverse_minimal_batch's kernel on the live
 *              blocks; the run-length step undone and the CRCs computed wave-parallel.  Candidates go in rounds of 1536, so
 *              the scratch (the context's: about 2.1 x 100 000 x the files' highest level bytes a candidate of a round -- 2.9 GB for a
 *              full round at level 9 -- and up to 2 GiB for the inverse BWT of large blocks) does not grow with the file.  The call is
 *              synchronous and reads counts back between the stages.  DESIGN.md 3.20 has the kernels and measurements.
 *   not here   rcx_launch_dev and rcx_multi_batch, which do not take RCX_BZIP2_DECODE. */
int rcx_bzip2_decode_batch(rcx_ctx*, const rcx_batch*);
/* ENCODE: block i of the batch is one whole FILE and becomes one stream in its slot -- BZh and the level digit, the blocks, the end mark,
 * the combined CRC, padding to a byte -- that bzip2, libbz2 and rcx_bzip2_decode_batch read.  level 1..9 is the digit of the header and
 * sets the blocks' size: a block holds C = 100000 * level - 19 bytes of run-length form, and a file is cut into chunks of as many input
 * bytes as fill a block on the file's average, less a 64th, shorter where a chunk's own form would not fit.  One large file is many
 * independent blocks and encodes in parallel.
 *   bytes      those of the specification in DESIGN.md 3.21 (equal rotations by descending start, libbz2's initial partition and four
 *              refits with Moffat-Katajainen lengths limited to 17 bits), byte for byte those of its serial reference; NOT libbz2's, whose
 *              sorter and Huffman builder break ties their own way.  The same input, level and library give the same bytes.
 *   results    success: RCX_OK, out_len[i] = the stream's size, in_used[i] = in_len[i].  out_cap[i] too small, 0 included:
 *              RCX_E_OUTPUT_TOO_SMALL, out_len[i] = the exact size and NOTHING of the slot is written -- a size query, but one at the full
 *              cost of encoding.  Nothing outside a file's own slot is ever written.  An empty file is a stream of 14 bytes.
 *   capacity   there is no proven bound for this fit and none is exported: use in_len + in_len / 64 + 1024 as a first capacity and retry
 *              the files that report RCX_E_OUTPUT_TOO_SMALL with the size they report (the sizes measured stay within 1 % + 8 bytes of
 *              libbz2's; random bytes grow by about half a per cent).
 *   limits     level outside 1..9, more than 65535 files a call: RCX_RC_BAD_ARG with rcx_last_error; a file of 4 GiB or more: the
 *              batch path's per-block limit.  RCX_MEM_HOST and RCX_MEM_DEVICE as the decoder.
 *   knob       rcx_ctx_set_param(ctx, RCX_BZIP2_ENCODE, r): blocks a round, 1..4096; 0 (the default) is 1024, and fewer where a round's
 *              scratch would pass 4 GiB.  The bytes do not depend on it.
 *   stages     the run-length step as a scan; rcx_bwt_suffixes_batch's sorter on every block doubled (T || T), of whose suffix array the
 *              entries below n are the rotations' order; MTF chunk-parallel from last-occurrence tables; RUNA / RUNB by a scan; the
 *              table fit, a workgroup a block; the bits MSB-first into a store; at the end every output byte gathered from the sources
 *              that cover it.  Blocks go in rounds: the sort and the stages take some 70 bytes of scratch per input byte of a round,
 *              the packed blocks wait for their file's end at up to 2.2 bytes per input byte of the call.  Synchronous.  DESIGN.md 3.21.
 *   not here   randomised blocks, more than one stream a file, rcx_launch_dev and rcx_multi_batch, which do not take RCX_BZIP2_ENCODE. */
int rcx_bzip2_encode_batch(rcx_ctx*, const rcx_batch*, int level);

/* ---- Zstandard (extension: the reference has no Zstandard) ----
 * DECODE of .zst files as zstd / libzstd write them (RFC 8878).  Block i of the batch is one whole FILE: one or more concatenated frames
 * (magic FD2FB528 little-endian), skippable frames (184D2A50..5F) skipped wherever they stand, optionally followed by other bytes; its
 * decoded bytes go to its output slot.
 *   dictionary dict_off / dict_len: both NULL, or a raw-content dictionary per file as a range anywhere in the input buffer (the
 *              convention of rcx_lz4_decode_shared_batch; dict_len[i] = 0: none; files may share a range).  It is history in front of
 *              EVERY frame of the file; repeat offsets start at 1, 4, 8.  A frame whose Dictionary_ID is not 0 needs a formatted
 *              dictionary with entropy tables, which this call does not take: RCX_E_ZSTD_DICT.
 *   results    success: RCX_OK, out_len[i] = the decoded size of all frames, in_used[i] = the byte just after the last accepted frame
 *              (the file ends, after at least one frame, where the next four bytes are neither magic or fewer than four remain).
 *              out_cap[i] too small, 0 included: RCX_E_OUTPUT_TOO_SMALL and out_len[i] = the exact size needed, so one retry
 *              suffices -- the kernel goes on parsing and counting without storing, which also sizes a frame without
 *              Frame_Content_Size; every structural check has been made by then, the content checksum, which needs the bytes, is
 *              checked by the retry.  Any other failure: the first failure in stream order, out_len 0, in_used 0.  RCX_E_EOF: the
 *              input ends inside a frame (also a file shorter than 4 bytes).  RCX_E_ZSTD_DATA: everything the format calls corrupt
 *              that has no status of its own, among it a decoded size that is not the declared Frame_Content_Size and block type 3.
 *              Nothing outside a file's own slot is written, a failing file affects no other, nothing below a slot is read.
 *   oracle     bytes, out_len, in_used and accept / reject are libzstd 1.4.8's one-shot decoder's, also where it is laxer or stricter
 *              than the RFC (a compressed block of fewer than 3 or of 128 KiB and more bytes is refused, a raw or RLE block is not held
 *              to the window's block maximum, a resolved offset of 0 reads as 1, the reserved bits of the sequence modes are ignored, a count of 0 sequences
 *              ends a block only when written in one byte: behind 80 00 the modes byte must follow and what follows it is not read).
 *              Three departures: a sequence or weight bitstream that is read past its first bit is refused (libzstd goes on with
 *              stale bits and may accept); Huffman codes longer than 11 bits are refused as the RFC asks (libzstd reads 12); four
 *              literal streams for fewer than 6 literals of sizes 1, 2, 3 and 5 are refused (libzstd writes past its segments).
 *   limits     a file and a slot below 4 GiB; at most 65535 files a call (more: RCX_RC_BAD_ARG).  RCX_MEM_HOST and RCX_MEM_DEVICE.
 *              Synchronous.
 *   stages     one wave per file, persistent over the files of a call, blocks in order: headers; the FSE and Huffman tables into
 *              12 KiB of LDS; literals, a lane per Huffman stream, into a 128 KiB buffer of the context's scratch; sequences by one
 *              lane into a ring of 64; execution by the wave, a lane per output byte of a batch, from three sources (literals, the
 *              frame's output, the dictionary); XXH64
 *              of a frame with a checksum.  DESIGN.md 3.22 has the kernel and what bounds it.
 *   not here   the writer, formatted dictionaries, legacy (pre-0.8) frames, rcx_launch_dev and rcx_multi_batch, which do not take
 *              RCX_ZSTD_DECODE or RCX_XXH64. */
int rcx_zstd_decode_batch(rcx_ctx*, const rcx_batch*, const uint64_t* dict_off, const uint64_t* dict_len);
/* XXH64 of every block, the twin of rcx_xxh32_batch: hash[i] = XXH64(block i, seed), eight bytes a hash; out_base, out_off, out_cap and
 * out_len may be NULL.  A Zstandard frame's content checksum is the low 32 bits; the decoder above uses the same device code. */
int rcx_xxh64_batch(rcx_ctx*, const rcx_batch*, uint64_t seed, uint64_t* hash);

/* ---- device-resident descriptors (benchmark / pipeline use) ------------------ */
/* Same kernels, but every array (offsets, lengths, status, ...) already lives
 * in HBM, nothing is copied and nothing is synchronised: the call enqueues on
 * the ctx stream and returns. This is what bench.py times.
 * ONE exception: RCX_BWT_FORWARD / RCX_BWT_SUFFIXES read in_len back and wait once per prefix-doubling round for a few counter words
 * (the host decides which of the sorter's kernels the next round needs, csrc/k_bwt.hip) -- the call returns when the last round has been
 * enqueued, with the transform's final kernels still running.  A caller that overlaps BWT batches gives each its own context and
 * thread (pipeline.PipelineLanes does). */
typedef struct rcx_dev_batch {
    const uint8_t*  in_base;
    const uint64_t* in_off;
    const uint64_t* in_len;
    uint8_t*        out_base;
    const uint64_t* out_off;
    const uint64_t* out_cap;
    uint64_t*       out_len;
    uint64_t*       in_used;   /* may be NULL */
    int32_t*        status;
    uint32_t*       aux;       /* codec extra (origin / adler / flags), may be NULL */
    uint32_t        nblocks;
} rcx_dev_batch;

enum rcx_codec {
    RCX_LZ4_DECODE = 0, RCX_LZ4_ENCODE, RCX_INFLATE, RCX_ZLIB_DECODE, RCX_ADLER32,
    RCX_BWT_FORWARD, RCX_BWT_INVERSE, RCX_MTF_ENCODE, RCX_MTF_DECODE,
    RCX_DC_ENCODE, RCX_DC_DECODE, RCX_ARI_BYTE_ENCODE, RCX_ARI_BYTE_DECODE,
    RCX_RLE_ENCODE, RCX_RLE_DECODE, RCX_CRC32, RCX_GZIP_DECODE,
    RCX_ARI_BINARY_ENCODE, RCX_ARI_BINARY_DECODE, RCX_ARI_PROXY_ENCODE, RCX_ARI_PROXY_DECODE,
    RCX_ARI_APM_ENCODE, RCX_ARI_APM_DECODE, RCX_BWT_INVERSE_MINIMAL,
    RCX_BWT_SUFFIXES, RCX_BWT_INVERSION_TABLE,
    RCX_DEFLATE_ENCODE, RCX_ZLIB_ENCODE, RCX_GZIP_ENCODE, RCX_CODEC_COUNT
};
/* Ids of the batch entry points that rcx_launch_dev, rcx_multi_* and rcx_scratch_bytes do not take (enum rcx_codec stays as it is for
 * those): they name the entry point to rcx_ctx_set_variant / rcx_ctx_set_param, neither of which has a setting for them yet, but for
 * RCX_BZIP2_DECODE's parameter (the candidates a round, see rcx_bzip2_decode_batch) and RCX_BZIP2_ENCODE's (the blocks a round, see
 * rcx_bzip2_encode_batch). */
enum rcx_xcodec { RCX_XXH32 = 32, RCX_LZ4_DECODE_LINKED = 33, RCX_LZ4_ENCODE_HIST = 34, RCX_DEFLATE_ENCODE_HIST = 35, RCX_ZLIB_ENCODE_DICT = 36,
                  RCX_INFLATE_HIST = 37, RCX_ZLIB_DECODE_DICT = 38, RCX_LZ4_ENCODE_SHARED = 39, RCX_DEFLATE_ENCODE_SHARED = 40,
                  RCX_ZLIB_ENCODE_SHARED = 41, RCX_LZ4_DECODE_SHARED = 42, RCX_INFLATE_SHARED = 43, RCX_ZLIB_DECODE_SHARED = 44,
                  RCX_DICT_TRAIN = 45, RCX_BZIP2_DECODE = 46, RCX_BZIP2_ENCODE = 47, RCX_ZSTD_DECODE = 48, RCX_XXH64 = 49,
                  RCX_XCODEC_END = 50 };
/* scratch bytes (HBM) the codec needs for nblocks blocks of <= max_block bytes.  Required for LZ4 encode, BWT and gzip
 * decode and the DEFLATE / zlib / gzip encoders; for RCX_INFLATE / RCX_ZLIB_DECODE it is what the default (wave-per-stream) decoder needs -- without it
 * rcx_launch_dev falls back to the lane-per-stream kernel (same results, slower on small batches). */
uint64_t rcx_scratch_bytes(int codec, uint32_t nblocks, uint64_t max_block);
int rcx_launch_dev(rcx_ctx*, int codec, const rcx_dev_batch*, void* scratch, uint64_t scratch_bytes);
/* Measurement aid (no counterpart in the reference): what a plain copy reaches on this device -- `bytes` read and `bytes` written per
 * pass by a kernel that moves 16 bytes a thread (a workgroup per 4 KiB), `reps` passes timed with events on the ctx stream; *gb_per_s =
 * 2 * bytes / time.  The "achievable" line next to the 8 TB/s spec peak in bench.py's roofline (hipMemcpy and torch's copy_ read 15-25 %
 * lower: benchmarks/micro/hbm_copy.hip). */
int rcx_hbm_copy_probe(rcx_ctx*, uint64_t bytes, int reps, double* gb_per_s);
/* kernel variant knob for A/B measurements (0 = default/best). */
int rcx_ctx_set_variant(rcx_ctx*, int codec, int variant);
/* codec parameter for rcx_launch_dev (the *_batch entry points take it as an argument and neither read nor write it): the rate of
 * RCX_ARI_BINARY_* (also what rcx_multi_batch, which has no argument for it, codes with);
 * RCX_LZ4_DECODE, RCX_INFLATE, RCX_ZLIB_DECODE, RCX_GZIP_DECODE: bit 0 = host-memory batches by plain copies (see rcx_lz4_decode_batch),
 * bits 8-15 / 16-23 tuning of the ranges -- the one parameter the batch calls do read;
 * RCX_LZ4_ENCODE: 0 = the reference's encoder, 1..12 = the HC level (see rcx_lz4_encode_hc_batch); the batch calls ignore it,
 * rcx_multi_batch included (it runs rcx_lz4_encode_batch's encoder);
 * RCX_DEFLATE_ENCODE / RCX_ZLIB_ENCODE / RCX_GZIP_ENCODE: 0 or 1..9 = the level (see rcx_deflate_encode_level_batch); the batch calls
 * ignore it, rcx_multi_batch included (level 1);
 * RCX_DC_ENCODE / RCX_DC_DECODE: 1 = with the coding contexts (rcx_dc_encode_ctx_batch); the batch calls ignore it */
int rcx_ctx_set_param(rcx_ctx*, int codec, uint32_t value);

/* ---- more than one device ---------------------------------
 * Blocks are independent in every codec (reference: src/lz4.rs:445-456 one block per frame block, src/bwt/mod.rs:373-401 one
 * record per block, src/entropy/ari/test.rs:52-89 self-terminating streams), so a batch shards by contiguous block ranges and
 * needs no collective: range g runs on device g.  An rcx_multi owns one rcx_ctx per listed device (a device may be listed more
 * than once: two ranges on one GPU).  Three layers, all without Python:
 *   rcx_partition        the ranges: contiguous, balanced by `weights` (decoded bytes), bounds[parts + 1], bounds[0] = 0
 *   rcx_multi_batch      a HOST-memory batch: every range is staged to its device, run and copied back by a host thread of its
 *                        own (one context each: contexts are thread-compatible, not thread-safe); per-block results land in the
 *                        caller's arrays exactly as the one-device entry point of that codec leaves them.  aux_in / aux_out /
 *                        n_out: what that entry point takes beside the batch (origins in, origins / flags / checksums out,
 *                        DC decode's lengths), or NULL.
 *   rcx_multi_launch_dev DEVICE-resident ranges: per_device[g] (arrays in device g's HBM, or NULL for none) is enqueued on device
 *                        g's context stream like rcx_launch_dev; rcx_multi_sync waits for every device.
 *   rcx_multi_scatter_dev / rcx_multi_gather_dev   the batch sits in the HBM of ONE device of the set (`root`): contiguous byte
 *                        ranges travel to the devices that work on them and the results come back DEVICE TO DEVICE, no host staging
 *                        ("RCCL only to scatter inputs and gather outputs").  range_off[g] .. range_off[g + 1] are device
 *                        g's bytes in root_buf (count + 1 host words; an empty range is skipped); peer_buf[g] is device g's buffer,
 *                        range-relative (its byte 0 is root_buf[range_off[g]]); peer_buf[root] may be NULL: that range stays where it
 *                        is.  Both calls only enqueue, each transfer ordered on the streams of the two contexts it connects:
 *                        scatter -> rcx_multi_launch_dev -> gather -> rcx_multi_sync needs no wait in between.
 *                        Transport: RCCL -- grouped ncclSend / ncclRecv, one communicator per device under ncclCommInitAll, librccl
 *                        loaded on first use -- when the set's devices are distinct; a set that lists a device twice (what a one-GPU
 *                        box can test), a host without librccl, or RCX_MULTI_TRANSPORT=peer in the environment use
 *                        hipMemcpyPeerAsync between the contexts' streams (events order it).  rcx_multi_transport() names the one
 *                        in use ("rccl" / "peer"; "" before the first transfer).  Measured on one device only: see DESIGN.md 4. */
typedef struct rcx_multi rcx_multi;
int  rcx_multi_create(const int* device_ids, int n, rcx_multi** out);
void rcx_multi_destroy(rcx_multi*);
int  rcx_multi_count(const rcx_multi*);
rcx_ctx* rcx_multi_ctx(rcx_multi*, int i);      /* device i's context: its stream, variant and parameter knobs, last error */
void rcx_partition(const uint64_t* weights, uint32_t nblocks, uint32_t parts, uint32_t* bounds);
int  rcx_multi_batch(rcx_multi*, int codec, const rcx_batch*, const uint32_t* aux_in, uint32_t* aux_out, const uint64_t* n_out);
int  rcx_multi_scatter_dev(rcx_multi*, int root, const uint8_t* root_buf, const uint64_t* range_off, uint8_t* const* peer_buf);
int  rcx_multi_gather_dev(rcx_multi*, int root, uint8_t* root_buf, const uint64_t* range_off, const uint8_t* const* peer_buf);
const char* rcx_multi_transport(const rcx_multi*);
int  rcx_multi_launch_dev(rcx_multi*, int codec, const rcx_dev_batch* const* per_device, void* const* scratch, const uint64_t* scratch_bytes);
int  rcx_multi_sync(rcx_multi*);
const char* rcx_multi_last_error(const rcx_multi*);

/* ---- page-locked host memory (no counterpart in the reference: its Vec<u8> buffers are pageable) ----------------------------------
 * rcx_lz4_decode_batch writes a page-locked output buffer directly and takes page-locked input in ranges under the launch (above).
 * A host language without the HIP headers pins its own allocation with these: rcx_host_register(ptr, bytes) page-locks
 * [ptr, ptr + bytes) for every device (hipHostRegister, portable + mapped; ~0.1 ms per MiB the first time), rcx_host_unregister
 * undoes it before the memory is freed.  Return enum rcx_rc. */
int rcx_host_register(void* ptr, uint64_t bytes);
int rcx_host_unregister(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* RCX_H */
