// rcx_api.hip -- the C-ABI of include/rcx.h over the gfx950 kernels.  Host side: descriptor staging,
// HBM staging for host-memory batches, kernel dispatch on the ctx stream.  There is no CPU code path:
// every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

#include "rcx_tu.h"
#include "rcx_plan.h"

struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = n + n / 8 + 4096;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct rcx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::string err;
    int variant[RCX_XCODEC_END] = {0};          // (indexed by enum rcx_codec and enum rcx_xcodec)
    uint32_t param[RCX_XCODEC_END] = {0};
    DevBuf d_link;                       // rcx_lz4_decode_linked_batch: the chains' tables (order | head | dict | eff)
    DevBuf d_in, d_out, d_desc, d_scratch;
    DevBuf d_scratch2;                   // rcx_bzip2_decode_batch: the inverse BWT's scratch, beside the stages' in d_scratch (rcx_bzip2_encode_batch: the sort's)
    DevBuf d_scratch3;                   // rcx_bzip2_encode_batch: what lasts for the call, the blocks' records and their packed bits
    DevBuf d_apm;                        // apm stretch table + gate bins (filled on first use)
    uint8_t* h_desc = nullptr; size_t h_desc_cap = 0;      // page-locked: the descriptors' way in and the results' way out are small copies the call waits for
    hipStream_t copy_stream = nullptr;   // the host-memory LZ4 decode: compressed ranges on their way in under the launch that decodes them
    std::vector<hipEvent_t> piece_ev;
    bool gate_bad = false;               // a gated launch ran into its time limit (the copies did not run beside it): one copy in front of the launch for the next GATE_RETRY calls, then ranges are tried again
    uint32_t gate_bad_calls = 0;         // calls left before the next try (rcx_ctx_set_param(ctx, codec, 0) of either decoder clears it at once)
    DevBuf d_gate; uint32_t* h_gate = nullptr; uint32_t gate_seq = 0;      // "range r has arrived" words (device; their page-locked source)
};

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return e_ == hipErrorOutOfMemory ? RCX_RC_NO_MEMORY : RCX_RC_HIP_ERROR;           \
        }                                                                                     \
    } while (0)

extern "C" int rcx_version(void) { return 1; }

extern "C" int rcx_ctx_create(int device_id, rcx_ctx** out)
{
    if (!out) return RCX_RC_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RCX_RC_NO_DEVICE;
    rcx_ctx* c = new rcx_ctx();
    if (device_id < 0) { if (hipGetDevice(&c->device) != hipSuccess) { delete c; return RCX_RC_NO_DEVICE; } }
    else { if (device_id >= ndev || hipSetDevice(device_id) != hipSuccess) { delete c; return RCX_RC_NO_DEVICE; } c->device = device_id; }
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RCX_RC_HIP_ERROR; }
    c->stream = c->own_stream;
    *out = c;
    return RCX_RC_OK;
}

extern "C" void rcx_ctx_destroy(rcx_ctx* c)
{
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    c->d_in.release(); c->d_out.release(); c->d_desc.release(); c->d_scratch.release(); c->d_apm.release(); c->d_link.release(); c->d_scratch2.release(); c->d_scratch3.release();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t e : c->piece_ev) (void)hipEventDestroy(e);
    c->d_gate.release();
    if (c->h_gate) (void)hipHostFree(c->h_gate);
    if (c->h_desc) (void)hipHostFree(c->h_desc);
    delete c;
}

extern "C" int rcx_ctx_set_stream(rcx_ctx* c, void* s)
{
    if (!c) return RCX_RC_BAD_ARG;
    c->stream = (hipStream_t)s;          // NULL = the HIP null (legacy default) stream
    return RCX_RC_OK;
}

static bool codec_id_ok(int codec) { return (codec >= 0 && codec < RCX_CODEC_COUNT) || (codec >= RCX_XXH32 && codec < RCX_XCODEC_END); }

extern "C" int rcx_ctx_set_variant(rcx_ctx* c, int codec, int variant)
{
    if (!c || !codec_id_ok(codec)) return RCX_RC_BAD_ARG;
    c->variant[codec] = variant;
    return RCX_RC_OK;
}

extern "C" int rcx_ctx_set_param(rcx_ctx* c, int codec, uint32_t value)
{
    if (!c || !codec_id_ok(codec)) return RCX_RC_BAD_ARG;
    c->param[codec] = value;
    if (codec == RCX_LZ4_DECODE || codec == RCX_INFLATE || codec == RCX_ZLIB_DECODE) { c->gate_bad = false; c->gate_bad_calls = 0; }   // (setting a decoder's host-path knobs also ends the back-off a late gate started)
    return RCX_RC_OK;
}

extern "C" const char* rcx_last_error(const rcx_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

extern "C" const char* rcx_status_string(int s)
{
    switch (s) {
    case RCX_OK: return "ok";
    case RCX_E_EOF: return "unexpected end of file";
    case RCX_E_OUTPUT_TOO_SMALL: return "output buffer too small";
    case RCX_E_MALFORMED: return "malformed input (the reference panics here)";
    case RCX_E_HUFFMAN_TREE_TOO_LARGE: return "huffman tree too large";
    case RCX_E_INVALID_BLOCK_CODE: return "invalid block code";
    case RCX_E_INVALID_HUFFMAN_HEADER_SYMBOL: return "invalid huffman header symbol";
    case RCX_E_INVALID_HUFFMAN_TREE: return "invalid huffman tree";
    case RCX_E_INVALID_HUFFMAN_TREE_HEADER: return "invalid huffman tree header";
    case RCX_E_INVALID_HUFFMAN_CODE: return "invalid huffman code";
    case RCX_E_INVALID_STATIC_SIZE: return "invalid static size";
    case RCX_E_NOT_ENOUGH_BITS: return "not enough bits";
    case RCX_E_ZLIB_FORMAT: return "unsupported zlib stream format";
    case RCX_E_ZLIB_WINDOW: return "unsupported zlib window size";
    case RCX_E_ZLIB_DICT: return "unsupported initial dictionary in the output stream";
    case RCX_E_ZLIB_DICT_ID: return "zlib dictionary id mismatch";
    case RCX_E_ZLIB_HEADER_CHECKSUM: return "invalid zlib header checksum";
    case RCX_E_ZLIB_CHECKSUM: return "invalid checksum on zlib stream";
    case RCX_E_RLE_LONG_RUN: return "Overly long run";
    case RCX_E_LZ4_MAGIC: return "";
    case RCX_E_LZ4_VERSION: return "";
    case RCX_E_LZ4_INPUT_TOO_LARGE: return "input too large";
    case RCX_E_LZ4_HISTORY: return "an earlier block of the chain failed";
    case RCX_E_BWT_BLOCK_TOO_LARGE: return "bwt block of 2^28 bytes or more";
    case RCX_E_GZIP_MAGIC: return "not a gzip member";
    case RCX_E_GZIP_METHOD: return "unsupported gzip compression method";
    case RCX_E_GZIP_FLAGS: return "reserved gzip flags set";
    case RCX_E_GZIP_CRC: return "invalid CRC-32 on gzip member";
    case RCX_E_GZIP_ISIZE: return "invalid length on gzip member";
    case RCX_E_BZ2_MAGIC: return "not a bzip2 file";
    case RCX_E_BZ2_DATA: return "invalid bzip2 data";
    case RCX_E_BZ2_BLOCK_CRC: return "invalid CRC on bzip2 block";
    case RCX_E_BZ2_STREAM_CRC: return "invalid combined CRC on bzip2 stream";
    case RCX_E_BZ2_RANDOMISED: return "randomised bzip2 block (not supported)";
    case RCX_E_ZSTD_MAGIC: return "not a zstd frame";
    case RCX_E_ZSTD_HEADER: return "unsupported zstd frame header";
    case RCX_E_ZSTD_DATA: return "invalid zstd data";
    case RCX_E_ZSTD_CHECKSUM: return "invalid content checksum on zstd frame";
    case RCX_E_ZSTD_DICT: return "zstd frame needs a formatted dictionary (not supported)";
    default: return "unknown status";
    }
}

extern "C" uint64_t rcx_lz4_compression_bound(uint64_t n) { return n > 0x7e000000ull ? 0 : n + n / 255 + 16 + 4; }
extern "C" uint64_t rcx_ari_byte_encode_bound(uint64_t n) { return 2 * n + 16; }
extern "C" uint64_t rcx_rle_encode_bound(uint64_t n) { return n + n / 2 + 16; }
// a 64 KiB segment is at worst two stored blocks: 2 x (3 header bits + 7 padding + 32 LEN/NLEN) = 84 bits <= 11 bytes; empty input: 2 bytes
extern "C" uint64_t rcx_deflate_compression_bound(uint64_t n) { return n + 11 * rcx_tu_deflate_encode_segments(n) + 2; }
extern "C" uint64_t rcx_deflate_level_scratch_bytes(uint32_t nblocks, uint64_t max_block)
{
    return rcx_tu_deflate_level_scratch(nblocks, (uint64_t)nblocks * rcx_tu_deflate_encode_segments(max_block));
}
extern "C" uint64_t rcx_lz4_hc_scratch_bytes(uint32_t nblocks, uint64_t max_block)
{
    return rcx_tu_lz4_hc_scratch(nblocks, (uint64_t)nblocks * rcx_tu_lz4_hc_segments(max_block));
}
// (every block counted with a history: one more segment of links each)
extern "C" uint64_t rcx_lz4_hc_hist_scratch_bytes(uint32_t nblocks, uint64_t max_block)
{
    return rcx_tu_lz4_hc_hist_scratch(nblocks, (uint64_t)nblocks * rcx_tu_lz4_hc_segments(max_block), nblocks);
}
// (every block counted with a history: one more segment of links each)
extern "C" uint64_t rcx_deflate_hist_scratch_bytes(uint32_t nblocks, uint64_t max_block)
{
    return rcx_tu_deflate_hist_scratch(nblocks, (uint64_t)nblocks * rcx_tu_deflate_encode_segments(max_block), nblocks);
}

// (ndict: the distinct dictionaries, 256 KiB each at the most; every block counted at max_block)
extern "C" uint64_t rcx_lz4_hc_shared_scratch_bytes(uint32_t nblocks, uint64_t max_block, uint32_t ndict)
{
    return rcx_tu_lz4_hc_dict_scratch(nblocks, (uint64_t)nblocks * rcx_tu_lz4_hc_segments(max_block), ndict);
}
extern "C" uint64_t rcx_deflate_shared_scratch_bytes(uint32_t nblocks, uint64_t max_block, uint32_t ndict)
{
    return rcx_tu_deflate_dict_scratch(nblocks, (uint64_t)nblocks * rcx_tu_deflate_encode_segments(max_block), ndict);
}

// ---- scratch requirements ---------------------------------------------------------------------
extern "C" uint64_t rcx_scratch_bytes(int codec, uint32_t nblocks, uint64_t max_block)
{
    switch (codec) {
    case RCX_LZ4_ENCODE: return rcx_tu_lz4_encode_scratch(nblocks);
    case RCX_BWT_FORWARD: return rcx_tu_bwt_forward_scratch(nblocks, max_block);
    case RCX_BWT_SUFFIXES: return rcx_tu_bwt_forward_scratch(nblocks, max_block);          // max_block: the longest INPUT block (the slot is 4n)
    case RCX_DC_ENCODE: return rcx_tu_dc_encode_scratch(nblocks, max_block);   // (optional: without it the wave-per-block kernel encodes every block; 0 when no block is long enough for the chunk path)
    case RCX_BWT_INVERSE: case RCX_BWT_INVERSE_MINIMAL: return rcx_tu_bwt_inverse_scratch(nblocks, max_block);
    case RCX_INFLATE: case RCX_ZLIB_DECODE: return rcx_tu_inflate_scratch(nblocks);
    case RCX_GZIP_DECODE: return rcx_tu_gzip_scratch(nblocks) + rcx_tu_inflate_scratch(nblocks) + 512;   // + the carve's alignment slack
    // every block counted at max_block: the per-segment staging of nblocks * segments(max_block) segments (the host batch path sizes it
    // from the real lengths instead)
    case RCX_DEFLATE_ENCODE: case RCX_ZLIB_ENCODE: case RCX_GZIP_ENCODE:
        return rcx_tu_deflate_encode_scratch(nblocks, (uint64_t)nblocks * rcx_tu_deflate_encode_segments(max_block));
    default: return 0;
    }
}

// ---- one call's record -------------------------------------------------------------------------------------------------------------
// rcx_lz4_decode_linked_batch: the chains of the batch (rcx_plan.h) and their tables in d_link
struct link_tables { const rcx_chain_plan* plan; const uint32_t* order; const uint32_t* head; const uint32_t* dict; uint64_t* eff; };
// What an entry point asks of run_batch and launch_codec.  Nothing of a call travels through the context: the context keeps the kernel
// variants and the decoders' host-path knobs (bit 0: plain copies, bits 8-23: range tuning), and rcx_launch_dev alone reads its parameter.
struct rcx_call {
    int codec;
    uint32_t param;                      // the EFFECTIVE parameter, resolved once by the entry point: LZ4 HC / DEFLATE level, DC withctx, ARI binary rate
    const uint32_t* aux_in; uint32_t* aux_out; const uint64_t* n_out;
    bool needs_out;
    uint32_t seed;                       // XXH32
    const link_tables* link;             // linked LZ4 decode, else null
    uint32_t nhist;                      // LZ4 HC / DEFLATE encode with history: the blocks that have one (their lengths are aux_in); behind shared dictionaries: the distinct dictionaries
    uint32_t aux_words;                  // words per block of aux_in: 1, or 2 (the zlib calls with history: lengths, then DICTIDs), or RCX_DICT_WORDS
    uint64_t dict_span;                  // shared dictionaries: one past their highest byte in the input buffer (it travels in with the blocks)
    const rcx_train_plan* train;         // dictionary training: the plan of the call (its words are aux_in), else null
    const rcx_batch* bz2;                // bzip2 decode and encode: the caller's batch (its host arrays steer the stages), else null
    uint64_t seed64;                     // XXH64
    const rcx_zstd_plan* zstd;           // Zstandard decode: the plan of the call (its dictionary words are aux_in), else null
};

// ---- per-codec traits of the host path ------------------------------------------------------------------------------------------------
enum mirror_kind { MIRROR_NONE, MIRROR_LZ4, MIRROR_INFLATE };          // may the launch store into a page-locked output buffer itself?
enum scratch_rule { SCRATCH_BY_CODEC,                                  // rcx_scratch_bytes
                    SCRATCH_DEFLATE_SEGS, SCRATCH_DEFLATE_LEVEL_SEGS,  // the staging of the real segments (+ chains, parse: levels 2..9)
                    SCRATCH_HC_SEGS,                                   // HC: the chains and parse of the real segments
                    SCRATCH_HC_HIST_SEGS,                              // ... and the chains of the real histories
                    SCRATCH_DEFLATE_HIST_SEGS,                         // DEFLATE levels 2..9: the real segments and the real histories
                    SCRATCH_HC_DICT_SEGS, SCRATCH_DEFLATE_DICT_SEGS,   // the real segments and the distinct dictionaries
                    SCRATCH_TRAIN,                                     // dictionary training: what the call's plan carved
                    SCRATCH_NONE,                                      // bzip2 decode: the launch reserves d_scratch itself
                    SCRATCH_ZSTD,                                      // Zstandard decode: a literal buffer per wave, by the call's plan
                    SCRATCH_DC_OPTIONAL };                             // chunk states: none with contexts, and none when they cannot be had
enum back_policy { BACK_USED_SPAN, BACK_INFLATE /* mirrored: the streams the first pass handed back */, BACK_CHAINS, BACK_SLOTS /* what the blocks produced, range by range */ };
struct codec_traits {
    bool needs_out;
    mirror_kind mirror;
    bool ranges;                         // may its input arrive in ranges under the launch?
    bool preload_out;                    // the staged output span starts as the caller's bytes
    scratch_rule scratch;
    back_policy back;
};
static codec_traits traits_of(int codec, uint32_t param)
{
    codec_traits t = {true, MIRROR_NONE, false, false, SCRATCH_BY_CODEC, BACK_USED_SPAN};
    switch (codec) {
    case RCX_LZ4_DECODE: t.mirror = MIRROR_LZ4; t.ranges = true; break;
    // (the inflate front end drains through the same window; the streams its first pass hands back are copied out behind the second)
    case RCX_INFLATE: case RCX_ZLIB_DECODE: t.mirror = MIRROR_INFLATE; t.ranges = true; t.back = BACK_INFLATE; break;
    // (gzip members: their headers are parsed by a kernel of its own in front of the decoder, which wants every member there)
    case RCX_GZIP_DECODE: t.mirror = MIRROR_INFLATE; t.back = BACK_INFLATE; break;
    // the DEFLATE encoders promise that no byte of the caller's buffer outside the streams they write changes: the copy back takes the
    // whole span, so the span starts as the caller's bytes
    case RCX_DEFLATE_ENCODE: case RCX_ZLIB_ENCODE: case RCX_GZIP_ENCODE:
        t.preload_out = true; t.scratch = param > 1 ? SCRATCH_DEFLATE_LEVEL_SEGS : SCRATCH_DEFLATE_SEGS; break;
    // (and so does the LZ4 HC encoder: a block's slot holds its bound, more than the block takes)
    case RCX_LZ4_ENCODE: if (param) { t.preload_out = true; t.scratch = SCRATCH_HC_SEGS; } break;
    case RCX_LZ4_ENCODE_HIST: t.preload_out = true; t.scratch = SCRATCH_HC_HIST_SEGS; break;
    case RCX_DEFLATE_ENCODE_HIST: case RCX_ZLIB_ENCODE_DICT: t.preload_out = true; t.scratch = SCRATCH_DEFLATE_HIST_SEGS; break;
    case RCX_LZ4_ENCODE_SHARED: t.preload_out = true; t.scratch = SCRATCH_HC_DICT_SEGS; break;
    case RCX_DEFLATE_ENCODE_SHARED: case RCX_ZLIB_ENCODE_SHARED: t.preload_out = true; t.scratch = SCRATCH_DEFLATE_DICT_SEGS; break;
    // the decoders with history read the bytes the caller put in front of the slots: the staged output span starts as the caller's
    case RCX_INFLATE_HIST: case RCX_ZLIB_DECODE_DICT: t.preload_out = true; break;
    // the decoders behind shared dictionaries read theirs from the input buffer: the input span, widened by the dictionaries' ranges,
    // travels in and nothing of the output buffer does.  They promise the caller's bytes between the slots all the same, so what the
    // blocks produced travels back range by range (rcx_plan_slot_copies: contiguous slots are one copy), never the span across the gaps
    case RCX_LZ4_DECODE_SHARED: case RCX_INFLATE_SHARED: case RCX_ZLIB_DECODE_SHARED: t.back = BACK_SLOTS; break;
    // dictionary training writes a slot's first out_len bytes and promises the rest of the caller's buffer: nothing of the output travels
    // in, and what the jobs produced travels back slot by slot
    case RCX_DICT_TRAIN: t.back = BACK_SLOTS; t.scratch = SCRATCH_TRAIN; break;
    // bzip2 files: a slot is written up to what the file decoded to, nothing of the output travels in; the scratch is asked for by the
    // launch itself, which learns how many candidates there are only from its first kernel
    case RCX_BZIP2_DECODE: t.back = BACK_SLOTS; t.scratch = SCRATCH_NONE; break;
    // ... and written: a slot holds its stream or, too small, nothing; the launch reserves its three buffers itself
    case RCX_BZIP2_ENCODE: t.back = BACK_SLOTS; t.scratch = SCRATCH_NONE; break;
    // .zst files: as bzip2's, a slot is written up to what the file decoded to and out_len of a slot too small is a size
    case RCX_ZSTD_DECODE: t.back = BACK_SLOTS; t.scratch = SCRATCH_ZSTD; break;
    case RCX_DC_ENCODE: t.scratch = SCRATCH_DC_OPTIONAL; break;
    case RCX_LZ4_DECODE_LINKED: t.back = BACK_CHAINS; break;
    case RCX_ADLER32: case RCX_CRC32: case RCX_XXH32: case RCX_XXH64: t.needs_out = false; break;
    default: break;
    }
    return t;
}
static rcx_call call_of(int codec, uint32_t param = 0, const uint32_t* aux_in = nullptr, uint32_t* aux_out = nullptr, const uint64_t* n_out = nullptr)
{
    return {codec, param, aux_in, aux_out, n_out, traits_of(codec, param).needs_out, 0, nullptr, 0, 1, 0, nullptr, nullptr, 0, nullptr};
}

// ---- kernel arguments: built here and nowhere else ---------------------------------------------------------------------------------------
struct gate_args { uint32_t* gate; const uint32_t* gate_host; uint32_t seq, ticks; const rcx_range_plan* ranges; };
static rcx_kargs make_kargs(const rcx_dev_batch& b, const uint64_t* n_out, void* scratch, uint64_t scratch_bytes,
                            uint8_t* out_mirror = nullptr, const gate_args* g = nullptr)
{
    rcx_kargs k = {};
    k.in_base = b.in_base; k.in_off = b.in_off; k.in_len = b.in_len;
    k.out_base = b.out_base; k.out_off = b.out_off; k.out_cap = b.out_cap;
    k.out_len = b.out_len; k.in_used = b.in_used; k.status = b.status; k.aux = b.aux;
    k.n_out = n_out; k.scratch = scratch; k.scratch_bytes = scratch_bytes; k.nblocks = b.nblocks; k.out_mirror = out_mirror;
    for (int i = 0; i < 15; i++) k.gate_bnd[i] = 0xffffffffu;
    if (g) {
        k.gate = g->gate; k.gate_host = g->gate_host; k.gate_seq = g->seq; k.gate_ticks = g->ticks;
        // (range 0 waits at a gate like the others: the launch is on its way to the device while the first bytes are)
        k.gate_all = 1;
        for (uint32_t pc = 1; pc < g->ranges->pieces(); pc++) k.gate_bnd[pc - 1] = g->ranges->bnd[pc];
    }
    return k;
}

// the stretch table and gate bins of the APM coder (apm.rs:53-59, 69-75, 144-154 through this host's libm), filled on first use
static int apm_tables(rcx_ctx* c)
{
    if (c->d_apm.p) return RCX_RC_OK;
    std::vector<uint16_t> h(4096 + 32, 0);
    for (uint32_t fp = 0; fp < 4096; fp++) {
        const float p = (float)fp / 4096.0f;
        const float w = logf(p / (1.0f - p)) * 2048.0f;
        h[fp] = (w > -32769.0f && w < 32768.0f) ? (uint16_t)(int16_t)w : (uint16_t)0x8000;
    }
    for (int i = 0; i < 17; i++) {
        const float rp = (float)i / 8.0f - 1.0f;
        const int16_t wp = (int16_t)(rp * 2048.0f);
        const float pr = 1.0f / (1.0f + expf(-((float)wp / 2048.0f)));
        h[4096 + i] = (uint16_t)(pr * 4096.0f);
    }
    HIPCHK(c, c->d_apm.reserve(h.size() * 2));
    HIPCHK(c, hipMemcpy(c->d_apm.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    return RCX_RC_OK;
}

// ---- kernel dispatch (the kernels and their launch code live in the tu_*.hip translation units) ------------------
static int launch_codec(rcx_ctx* c, const rcx_call& call, rcx_kargs& k)
{
    hipStream_t s = c->stream;
    const int codec = call.codec;
    const uint32_t n = k.nblocks;
    if (n == 0) return RCX_RC_OK;
    const int v = c->variant[codec];
    switch (codec) {
    case RCX_LZ4_DECODE: {
        int rc = rcx_tu_lz4_decode(s, k, v, c->err);
        if (rc) return rc;
        break; }
    case RCX_LZ4_ENCODE: {                                       // the codec parameter: 0 the reference's greedy encoder, 1..12 the HC level
        const uint32_t level = call.param;
        if (level > 12) { c->err = "lz4 encode: level must be 0 (reference encoder) or 1..12 (HC)"; return RCX_RC_BAD_ARG; }
        int rc = level ? rcx_tu_lz4_hc(s, k, (int)level, c->err) : rcx_tu_lz4_encode(s, k, v, c->err);
        if (rc) return rc;
        break; }
    case RCX_LZ4_ENCODE_HIST: {                                  // the codec parameter: the HC level; k.aux: the history lengths
        int rc = rcx_tu_lz4_hc_hist(s, k, (int)call.param, call.nhist, c->err);
        if (rc) return rc;
        break; }
    case RCX_LZ4_ENCODE_SHARED: {                                // the codec parameter: the HC level; k.aux: the words of rcx_plan_dict
        int rc = rcx_tu_lz4_hc_dict(s, k, (int)call.param, call.nhist, c->err);
        if (rc) return rc;
        break; }
    case RCX_DEFLATE_ENCODE_SHARED: case RCX_ZLIB_ENCODE_SHARED: {   // the codec parameter: the level, 2..9; k.aux: the words of rcx_plan_dict
        int rc = rcx_tu_deflate_encode_dict(s, k, codec == RCX_ZLIB_ENCODE_SHARED ? 1 : 0, (int)call.param, call.nhist, c->err);
        if (rc) return rc;
        break; }
    case RCX_INFLATE:
    case RCX_ZLIB_DECODE:
        rcx_tu_inflate(s, k, codec == RCX_ZLIB_DECODE, v);
        break;
    case RCX_LZ4_DECODE_SHARED:                                  // k.aux: the words of rcx_plan_dict, never null
        if (!k.aux || !call.aux_in) { c->err = "lz4 decode behind shared dictionaries: use rcx_lz4_decode_shared_batch"; return RCX_RC_BAD_ARG; }
        rcx_tu_lz4_decode_dict(s, k);
        break;
    case RCX_INFLATE_SHARED: case RCX_ZLIB_DECODE_SHARED:        // k.aux: the words of rcx_plan_dict, never null
        if (!k.aux || !call.aux_in) { c->err = "inflate behind shared dictionaries: use rcx_inflate_shared_batch / rcx_zlib_decode_shared_batch"; return RCX_RC_BAD_ARG; }
        rcx_tu_inflate_dict(s, k, codec == RCX_ZLIB_DECODE_SHARED);
        break;
    case RCX_DICT_TRAIN: {                                       // k.aux: the words of rcx_plan_train; returns when the last round has run
        if (!call.train || !k.aux) { c->err = "dict train: use rcx_dict_train_batch"; return RCX_RC_BAD_ARG; }
        int rc = rcx_tu_dict_train(s, k, *call.train, c->err);
        if (rc) return rc;
        break; }
    case RCX_BZIP2_DECODE: {                                     // synchronous; reserves the context's scratch itself, twice
        if (!call.bz2) { c->err = "bzip2 decode: use rcx_bzip2_decode_batch"; return RCX_RC_BAD_ARG; }
        const rcx_bz2_alloc alloc = {[](void* self, int which, uint64_t bytes) -> void* {
            rcx_ctx* cc = (rcx_ctx*)self;
            DevBuf& buf = which ? cc->d_scratch2 : cc->d_scratch;
            if (buf.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            return buf.p; }, c};
        int rc = rcx_tu_bzip2_decode(s, k, call.bz2->in_len, call.bz2->out_off, call.bz2->out_cap, alloc, c->param[RCX_BZIP2_DECODE], c->err);
        if (rc) return rc;
        break; }
    case RCX_BZIP2_ENCODE: {                                     // synchronous; the codec parameter: the level; reserves the context's scratch itself
        if (!call.bz2) { c->err = "bzip2 encode: use rcx_bzip2_encode_batch"; return RCX_RC_BAD_ARG; }
        const rcx_bz2_alloc alloc = {[](void* self, int which, uint64_t bytes) -> void* {
            rcx_ctx* cc = (rcx_ctx*)self;
            DevBuf& buf = which == 2 ? cc->d_scratch3 : which ? cc->d_scratch2 : cc->d_scratch;
            if (buf.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            return buf.p; }, c};
        int rc = rcx_tu_bzip2_encode(s, k, call.bz2->in_off, call.bz2->in_len, call.bz2->out_off, call.bz2->out_cap, alloc, (int)call.param,
                                     c->param[RCX_BZIP2_ENCODE], c->err);
        if (rc) return rc;
        break; }
    case RCX_INFLATE_HIST: case RCX_ZLIB_DECODE_DICT:            // k.aux: the history lengths (then the DICTIDs), never null
        if (!k.aux) { c->err = "inflate with history: use rcx_inflate_hist_batch / rcx_zlib_decode_dict_batch"; return RCX_RC_BAD_ARG; }
        rcx_tu_inflate_hist(s, k, codec == RCX_ZLIB_DECODE_DICT);
        break;
    case RCX_DEFLATE_ENCODE_HIST: case RCX_ZLIB_ENCODE_DICT: {   // the codec parameter: the level, 2..9; k.aux: the history lengths (then the DICTIDs)
        int rc = rcx_tu_deflate_encode_hist(s, k, codec == RCX_ZLIB_ENCODE_DICT ? 1 : 0, (int)call.param, call.nhist, c->err);
        if (rc) return rc;
        break; }
    case RCX_ADLER32:
        rcx_tu_adler32(s, k);
        break;
    case RCX_CRC32:
        rcx_tu_crc32(s, k);
        break;
    case RCX_XXH32:
        rcx_tu_xxh32(s, k, call.seed);
        break;
    case RCX_XXH64:
        rcx_tu_xxh64(s, k, call.seed64);
        break;
    case RCX_ZSTD_DECODE: {                                      // k.aux: the words of rcx_plan_dict, never null
        if (!call.zstd || !call.aux_in) { c->err = "zstd decode: use rcx_zstd_decode_batch"; return RCX_RC_BAD_ARG; }
        int rc = rcx_tu_zstd_decode(s, k, call.zstd->waves, v, c->err);
        if (rc) return rc;
        break; }
    case RCX_LZ4_DECODE_LINKED:
        if (!call.link) { c->err = "lz4 linked decode: use rcx_lz4_decode_linked_batch"; return RCX_RC_BAD_ARG; }
        rcx_tu_lz4_decode_linked(s, k, call.link->order, call.link->plan->rounds_off.data(), call.link->plan->nrounds, call.link->head,
                                 call.link->dict, call.link->eff);
        break;
    case RCX_GZIP_DECODE:
        if (k.scratch_bytes < rcx_tu_gzip_scratch(n)) { c->err = "gzip decode: scratch too small"; return RCX_RC_BAD_ARG; }
        rcx_tu_gzip_decode(s, k, v);
        break;
    case RCX_DEFLATE_ENCODE: case RCX_ZLIB_ENCODE: case RCX_GZIP_ENCODE: {   // the codec parameter: the level, 0 (as 1) or 1..9
        const uint32_t level = call.param;
        if (level > 9) { c->err = "deflate encode: level must be 0 or 1..9"; return RCX_RC_BAD_ARG; }
        const int fmt = codec == RCX_DEFLATE_ENCODE ? 0 : codec == RCX_ZLIB_ENCODE ? 1 : 2;
        int rc = level > 1 ? rcx_tu_deflate_encode_level(s, k, fmt, (int)level, c->err) : rcx_tu_deflate_encode(s, k, fmt, c->err);
        if (rc) return rc;
        break; }
    case RCX_BWT_FORWARD: case RCX_BWT_SUFFIXES: {
        int rc = rcx_tu_bwt_forward(s, k, v, c->err, codec == RCX_BWT_SUFFIXES);
        if (rc) return rc;
        break; }
    case RCX_BWT_INVERSION_TABLE: {
        int rc = rcx_tu_bwt_inversion_table(s, k);
        if (rc) return rc;
        break; }
    case RCX_BWT_INVERSE: case RCX_BWT_INVERSE_MINIMAL: {
        int rc = rcx_tu_bwt_inverse(s, k, v, c->err, codec == RCX_BWT_INVERSE_MINIMAL);
        if (rc) return rc;
        break; }
    case RCX_ARI_APM_ENCODE: case RCX_ARI_APM_DECODE: {
        const int rca = apm_tables(c);
        if (rca) return rca;
        k.scratch = c->d_apm.p; k.scratch_bytes = (4096 + 32) * 2;
        rcx_tu_serial(s, codec, k, v, 0);
        break; }
    case RCX_ARI_BINARY_ENCODE: case RCX_ARI_BINARY_DECODE:
        if (call.param < 1 || call.param > 31) { c->err = "ari binary: rate must be 1..31"; return RCX_RC_BAD_ARG; }
        [[fallthrough]];
    case RCX_MTF_ENCODE: case RCX_MTF_DECODE: case RCX_DC_ENCODE: case RCX_DC_DECODE:
    case RCX_ARI_PROXY_ENCODE: case RCX_ARI_PROXY_DECODE:
    case RCX_ARI_BYTE_ENCODE: case RCX_ARI_BYTE_DECODE: case RCX_RLE_ENCODE: case RCX_RLE_DECODE:
        rcx_tu_serial(s, codec, k, v, call.param);
        break;
    default:
        c->err = "unknown codec";
        return RCX_RC_BAD_ARG;
    }
    HIPCHK(c, hipGetLastError());
    return RCX_RC_OK;
}

extern "C" int rcx_launch_dev(rcx_ctx* c, int codec, const rcx_dev_batch* b, void* scratch, uint64_t scratch_bytes)
{
    if (!c || !b || codec < 0 || codec >= RCX_CODEC_COUNT) return RCX_RC_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (codec == RCX_DC_DECODE) { c->err = "dc decode needs n_out: use rcx_dc_decode_batch"; return RCX_RC_BAD_ARG; }
    rcx_kargs k = make_kargs(*b, nullptr, scratch, scratch_bytes);
    return launch_codec(c, call_of(codec, c->param[codec]), k);          // (the one place a codec's parameter comes from the context: include/rcx.h)
}

// ---- host-descriptor batch path -------------------------------------------------------------------
// run_batch is a sequence of stages over one batch_state; every stage enqueues on the context's stream in the order it is called.
// Descriptor block layout in HBM (all 8-byte aligned):
//   in_off[n] in_len[n] out_off[n] out_cap[n] n_out[n] | out_len[n] in_used[n] | status[n] aux[n]
static const uint32_t GATE_RETRY = 64;      // calls that go back to one copy in front of the launch after a gate ran into its limit (one descheduling of the calling thread is enough for that)
struct batch_state {
    const rcx_batch* b = nullptr;
    uint32_t n = 0;
    codec_traits t = {};
    rcx_spans sp;
    const uint8_t* d_in = nullptr; uint8_t* d_out = nullptr;        // the batch's bytes as the kernels see them
    uint8_t* mirror = nullptr;                                       // the caller's page-locked output buffer as the device sees it, or null
    uint32_t pieces = 1;                                             // input ranges (1: one copy in front of the launch)
    rcx_range_plan ranges;
    uint64_t* h64 = nullptr; int32_t* h_status = nullptr; uint32_t* h_aux = nullptr;     // the descriptor block, page-locked
    rcx_dev_batch dv = {};                                           // ... and in HBM
    const uint64_t* d_n_out = nullptr;
    void* scratch = nullptr; uint64_t scratch_bytes = 0;
    rcx_kargs k = {};
    bool gated = false;
    bool out_gaps = false;                                           // bytes of [0, out_span) lie outside every slot: they are the caller's
    bool out_staged = false;                                         // ... and were staged in, so that the span copy takes them back
    const uint64_t* out_len() const { return h64 + 5 * (size_t)n; }
};
#define STAGE(x) do { const int rc_ = (x); if (rc_ != RCX_RC_OK) return rc_; } while (0)

// The DC kernels address their words through uint32_t pointers (k_serial.hip; include/rcx.h asks for the alignment): a word buffer at
// another address is the caller's error and is refused by the block's number (the kernels themselves, reached through rcx_launch_dev,
// give such a block RCX_E_OUTPUT_TOO_SMALL / RCX_E_MALFORMED).  A host-memory batch is staged at an aligned address: there the
// offset alone decides.  rcx_multi_batch asks before it rebases its ranges' offsets, so that it refuses what one context refuses.
static bool dc_words_aligned(int codec, const rcx_batch* b, std::string& err)
{
    if (codec != RCX_DC_ENCODE && codec != RCX_DC_DECODE) return true;
    const bool enc = codec == RCX_DC_ENCODE;
    const uint64_t* off = enc ? b->out_off : b->in_off;
    if (!off) return true;
    const uintptr_t base = b->mem == RCX_MEM_HOST ? 0 : (uintptr_t)(enc ? (const uint8_t*)b->out_base : b->in_base);
    for (uint32_t i = 0; i < b->nblocks; i++)
        if ((base + off[i]) & 3u) {
            err = std::string(enc ? "dc encode" : "dc decode") + ": block " + std::to_string(i) + ": the word buffer is not 4-byte aligned ("
                + (enc ? "out_off" : "in_off") + (b->mem == RCX_MEM_HOST ? " must be a multiple of 4)" : ", added to the base address, must be a multiple of 4)");
            return false;
        }
    return true;
}

// stage 1: the arguments, the spans and the per-block limits
static int check_batch(rcx_ctx* c, const rcx_call& call, const rcx_batch* b, batch_state& st)
{
    if (!b || (b->nblocks && (!b->in_off || !b->in_len || !b->status))) { c->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    if (call.needs_out && b->nblocks && (!b->out_off || !b->out_cap || !b->out_len)) { c->err = "null output descriptor"; return RCX_RC_BAD_ARG; }
    st.b = b; st.n = b->nblocks; st.t = traits_of(call.codec, call.param);
    if (st.n == 0) return RCX_RC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!rcx_plan_spans(st.n, b->in_off, b->in_len, call.needs_out ? b->out_off : nullptr, call.needs_out ? b->out_cap : nullptr, st.sp, c->err))
        return RCX_RC_BAD_ARG;
    if (call.dict_span > st.sp.in_span) st.sp.in_span = call.dict_span;      // (the dictionaries' ranges travel in with the blocks')
    if ((st.sp.in_span && !b->in_base) || (st.sp.out_span && !b->out_base)) { c->err = "null data pointer"; return RCX_RC_BAD_ARG; }
    if (b->mem != RCX_MEM_HOST && b->mem != RCX_MEM_DEVICE) { c->err = "bad mem kind"; return RCX_RC_BAD_ARG; }
    if (!dc_words_aligned(call.codec, b, c->err)) return RCX_RC_BAD_ARG;
    // no byte of the caller's output buffer outside the slots is written (include/rcx.h).  The span that travels back from the staging
    // buffer covers slots alone when the layout is dense (rcx_plan_out_dense: bench.py's and every fixed-slot layout), and the call is
    // what it always was; any other layout is marked here, and stage_in_out / copy_back keep the caller's bytes
    st.out_gaps = b->mem == RCX_MEM_HOST && call.needs_out && !st.t.preload_out && (st.t.back == BACK_USED_SPAN || st.t.back == BACK_INFLATE) &&
                  !rcx_plan_out_dense(st.n, b->out_off, b->out_cap, st.sp.out_span);
    return RCX_RC_OK;
}

// (the WHOLE span must be page-locked and mapped as one range: a buffer registered only in part would take the kernel's stores
//  into unmapped addresses -- the last byte's attributes must continue the first's)
static bool page_locked(const void* base, uint64_t span, hipPointerAttribute_t& first)
{
    hipPointerAttribute_t last;
    if (hipPointerGetAttributes(&first, base) != hipSuccess || first.type != hipMemoryTypeHost || !first.devicePointer) return false;
    if (span <= 1) return true;
    if (hipPointerGetAttributes(&last, (const uint8_t*)base + span - 1) != hipSuccess || last.type != hipMemoryTypeHost || !last.devicePointer) return false;
    return (const uint8_t*)last.devicePointer == (const uint8_t*)first.devicePointer + (span - 1);
}

// stage 2: mirror and ranges.
// LZ4 decode from host memory into a PAGE-LOCKED output buffer (hipHostMalloc / hipHostRegister: the device can address it):
// the decoder stores every byte that leaves its window a second time straight into that buffer (k_lz4_decode_v4.hip, MIRROR),
// so the decoded bytes cross PCIe while the launch runs and no device-to-host copy follows it; and the compressed bytes travel in
// as block ranges on a copy stream while the launch already decodes the ranges before them (launch_gated).  One copy
// each way (what every other codec and a pageable buffer get) costs in + kernel + out = 1.8 + 0.5 + 4.9 ms on the headline
// workload; this is the outbound 4.9 ms and little else.  rcx_ctx_set_param(ctx, RCX_LZ4_DECODE, 1) keeps the plain copies.
static void decide_mirror(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    const uint32_t knobs = c->param[call.codec];
    st.mirror = nullptr; st.pieces = 1; st.gated = false;
    if (b->mem != RCX_MEM_HOST || st.t.mirror == MIRROR_NONE || (knobs & 1u) || c->variant[call.codec] != 0 || !st.sp.out_span) return;
    if (st.t.mirror == MIRROR_INFLATE && !rcx_tu_inflate_mirrors(st.n, 0)) return;
    if (c->gate_bad && c->gate_bad_calls && --c->gate_bad_calls == 0) c->gate_bad = false;
    hipPointerAttribute_t at, ai;
    if (!page_locked(b->out_base, st.sp.out_span, at)) { (void)hipGetLastError(); return; }
    st.mirror = (uint8_t*)at.devicePointer;
    // (ranges only from page-locked INPUT: a pageable buffer is staged piece by piece, by copies that may need the compute
    // units the waiting blocks would hold)
    if (st.t.ranges && st.sp.in_span && !c->gate_bad && page_locked(b->in_base, st.sp.in_span, ai)) st.pieces = rcx_plan_piece_count(st.n, (knobs >> 8) & 255u);
    else (void)hipGetLastError();
}

// stage 3: a host-memory batch's bytes on their way into HBM
static int stage_in_out(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    hipStream_t s = c->stream;
    st.d_in = b->in_base; st.d_out = b->out_base;
    if (b->mem != RCX_MEM_HOST) return RCX_RC_OK;
    const size_t out_shift = st.mirror ? (size_t)((uintptr_t)st.mirror & 255u) : 0;           // the copy in HBM and the host buffer: the same alignment
    HIPCHK(c, c->d_in.reserve(st.sp.in_span + 64));
    HIPCHK(c, c->d_out.reserve(st.sp.out_span + out_shift + 64));
    if (st.sp.in_span && st.pieces <= 1) HIPCHK(c, hipMemcpyAsync(c->d_in.p, b->in_base, st.sp.in_span, hipMemcpyHostToDevice, s));
    st.d_in = (const uint8_t*)c->d_in.p;
    st.d_out = (uint8_t*)c->d_out.p + out_shift;
    // a layout with gaps: the span copy back must return the caller's own bytes, so the span travels in first -- unless the launch
    // stores into the caller's page-locked buffer itself and no span travels back (copy_back takes the slots alone should the launch
    // decline the mirror after all)
    st.out_staged = st.out_gaps && !st.mirror;
    if ((st.t.preload_out || st.out_staged) && st.sp.out_span) HIPCHK(c, hipMemcpyAsync(st.d_out, b->out_base, st.sp.out_span, hipMemcpyHostToDevice, s));
    // the linked LZ4 decoder reads the dictionaries the caller put in front of the chain heads' slots: those ranges alone travel in
    // (and only what the chains wrote travels back, copy_back)
    if (call.link) {
        const uint32_t* head = call.link->plan->head(); const uint32_t* dict = call.link->plan->dict();
        for (uint32_t i = 0; i < st.n; i++)
            if (head[i] == i && dict[i]) {
                const uint64_t at = b->out_off[i] - dict[i];
                HIPCHK(c, hipMemcpyAsync(st.d_out + at, b->out_base + at, dict[i], hipMemcpyHostToDevice, s));
            }
    }
    return RCX_RC_OK;
}

// stage 4: the descriptors, through the page-locked block into HBM
static int pack_descriptors(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    const size_t N = st.n;
    const size_t AW = call.aux_in ? call.aux_words : 1;                                          // aux words per block (in; one comes back)
    const size_t desc_bytes = (5 * N + 2 * N) * 8 + (1 + AW) * N * 4 + 64;
    HIPCHK(c, c->d_desc.reserve(desc_bytes));
    if (desc_bytes > c->h_desc_cap) {
        if (c->h_desc) (void)hipHostFree(c->h_desc);
        c->h_desc = nullptr; c->h_desc_cap = 0;
        HIPCHK(c, hipHostMalloc((void**)&c->h_desc, desc_bytes + desc_bytes / 4, hipHostMallocDefault));
        c->h_desc_cap = desc_bytes + desc_bytes / 4;
    }
    uint64_t* h64 = st.h64 = (uint64_t*)c->h_desc;
    memcpy(h64 + 0 * N, b->in_off, N * 8);
    memcpy(h64 + 1 * N, b->in_len, N * 8);
    if (call.needs_out) { memcpy(h64 + 2 * N, b->out_off, N * 8); memcpy(h64 + 3 * N, b->out_cap, N * 8); }
    else memset(h64 + 2 * N, 0, 2 * N * 8);
    if (call.n_out) memcpy(h64 + 4 * N, call.n_out, N * 8); else memset(h64 + 4 * N, 0, N * 8);
    st.h_status = (int32_t*)(h64 + 7 * N);
    st.h_aux = (uint32_t*)(st.h_status + N);
    for (size_t i = 0; i < N; i++) st.h_status[i] = RCX_E_MALFORMED;
    if (call.aux_in) memcpy(st.h_aux, call.aux_in, AW * N * 4); else memset(st.h_aux, 0, N * 4);
    memset(h64 + 5 * N, 0, 2 * N * 8);
    HIPCHK(c, hipMemcpyAsync(c->d_desc.p, c->h_desc, (7 * N) * 8 + (1 + AW) * N * 4, hipMemcpyHostToDevice, c->stream));
    uint64_t* d64 = (uint64_t*)c->d_desc.p;
    int32_t* d_status = (int32_t*)(d64 + 7 * N);
    st.dv = {st.d_in, d64, d64 + N, st.d_out, d64 + 2 * N, d64 + 3 * N, d64 + 5 * N, d64 + 6 * N, d_status, (uint32_t*)(d_status + N), st.n};
    st.d_n_out = d64 + 4 * N;
    return RCX_RC_OK;
}

// stage 5: scratch, by the codec's rule
static int reserve_scratch(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    const uint32_t n = st.n;
    uint64_t sb = 0, segs = 0;
    switch (st.t.scratch) {
    case SCRATCH_BY_CODEC: sb = rcx_scratch_bytes(call.codec, n, call.codec == RCX_BWT_SUFFIXES ? st.sp.max_in : st.sp.max_block); break;
    case SCRATCH_DEFLATE_SEGS: case SCRATCH_DEFLATE_LEVEL_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_deflate_encode_segments(b->in_len[i]);
        sb = st.t.scratch == SCRATCH_DEFLATE_LEVEL_SEGS ? rcx_tu_deflate_level_scratch(n, segs) : rcx_tu_deflate_encode_scratch(n, segs);
        break;
    case SCRATCH_HC_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_lz4_hc_segments(b->in_len[i]);
        sb = rcx_tu_lz4_hc_scratch(n, segs);
        break;
    case SCRATCH_HC_HIST_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_lz4_hc_segments(b->in_len[i]);
        sb = rcx_tu_lz4_hc_hist_scratch(n, segs, call.nhist);
        break;
    case SCRATCH_DEFLATE_HIST_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_deflate_encode_segments(b->in_len[i]);
        sb = rcx_tu_deflate_hist_scratch(n, segs, call.nhist);
        break;
    case SCRATCH_HC_DICT_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_lz4_hc_segments(b->in_len[i]);
        sb = rcx_tu_lz4_hc_dict_scratch(n, segs, call.nhist);
        break;
    case SCRATCH_DEFLATE_DICT_SEGS:
        for (uint32_t i = 0; i < n; i++) segs += rcx_tu_deflate_encode_segments(b->in_len[i]);
        sb = rcx_tu_deflate_dict_scratch(n, segs, call.nhist);
        break;
    case SCRATCH_TRAIN: sb = call.train ? call.train->scratch_bytes : 0; break;
    case SCRATCH_ZSTD: sb = call.zstd ? call.zstd->scratch_bytes : 0; break;
    case SCRATCH_NONE: return RCX_RC_OK;
    case SCRATCH_DC_OPTIONAL:                                       // withctx: the wave-per-block kernel encodes, no chunk states
        sb = call.param ? 0 : rcx_scratch_bytes(call.codec, n, st.sp.max_block);
        break;
    }
    st.scratch = nullptr; st.scratch_bytes = 0;
    if (st.t.scratch == SCRATCH_DC_OPTIONAL && sb && c->d_scratch.reserve(sb + 64) != hipSuccess) {
        // the chunk states are optional (37 KiB a block): a batch too large for them falls back to the wave-per-block kernel
        (void)hipGetLastError();
        return RCX_RC_OK;
    }
    HIPCHK(c, c->d_scratch.reserve(sb + 64));
    if (st.t.scratch != SCRATCH_DC_OPTIONAL || sb) { st.scratch = c->d_scratch.p; st.scratch_bytes = c->d_scratch.cap; }
    return RCX_RC_OK;
}

// stage 6, ranges: the copy stream, the events and the gate words of this call
static int open_gates(rcx_ctx* c, const batch_state& st, gate_args& g)
{
    if (!c->copy_stream) {
        // a stream of ANOTHER priority than the launch's: HIP hands its few hardware queues to the streams of one priority in
        // turn, and a copy stream that shares the launch's queue stands behind the launch it is meant to feed (every gate ran into
        // its limit for one context in two: 66 ms a call).  The LOWEST priority: it carries copy-engine work only, and the
        // high-priority queues stay with whoever uses them for kernels (pipeline.PipelineLanes keeps its two lanes apart that way)
        int least = 0, greatest = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(c, hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, least));
    }
    while (c->piece_ev.size() < st.pieces) { hipEvent_t e; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->piece_ev.push_back(e); }
    const uint32_t seq = ++c->gate_seq ? c->gate_seq : ++c->gate_seq;       // (never 0)
    if (!c->h_gate) HIPCHK(c, hipHostMalloc((void**)&c->h_gate, 64, hipHostMallocDefault));
    // the gate words hold anything BUT this call's number before the launch: recycled page-locked or device memory is not zero, and a
    // stale word that happened to equal `seq` would let a range's blocks read input that has not arrived
    for (int w = 0; w < 16; w++) __atomic_store_n((volatile uint32_t*)(c->h_gate + w), seq - 1u, __ATOMIC_RELAXED);
    HIPCHK(c, c->d_gate.reserve(64));
    HIPCHK(c, hipMemsetAsync(c->d_gate.p, 0, 64, c->stream));                // (0 is never a call's number; in front of the launch on its stream)
    hipPointerAttribute_t ga;
    HIPCHK(c, hipPointerGetAttributes(&ga, c->h_gate));
    const uint64_t ticks = 1000000ull + st.sp.in_span / 50ull;               // 10 ms + the input at 5 GB/s (100 MHz ticks)
    g = {(uint32_t*)c->d_gate.p, (const uint32_t*)ga.devicePointer, seq, ticks > 0xffffffffull ? 0xffffffffu : (uint32_t)ticks, &st.ranges};
    return RCX_RC_OK;
}

// stage 6, ranges: ONE launch, the input in ranges.  The blocks of a range (the first one small: a sixty-fourth of the blocks) start when
// this thread has seen the range's copy complete and said so in a page-locked word (k_lz4_decode_v8, `gate`).  A launch per range
// was built first and measured: each one ends with the link drained and begins with nothing to send, 5.9 ms for three
// growing ranges, 6.6 for eight equal ones, against 7.0 for one launch behind one copy and 5.6 for this.
// A block whose input does not arrive in gate_ticks gives up with RCX_ST_GATE and is decoded by a second launch (run_batch; the copies
// cannot be held up by the waiting blocks as long as a copy engine moves them; a copy done by a kernel could be, and then this is what
// ends the wait).
static int launch_gated(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    hipStream_t s = c->stream;
    const uint32_t seq = st.k.gate_seq;
    // a failure behind the launch must not leave it spinning at its gates under the next call's copies: open every gate (the blocks
    // decode whatever has arrived; the call fails anyway), drain both streams, then return
    bool launched = false;
    auto bail = [&](hipError_t e, const char* what) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
        (void)hipGetLastError();
        if (launched) for (int w = 0; w < 16; w++) __atomic_store_n((volatile uint32_t*)(c->h_gate + w), seq, __ATOMIC_RELEASE);
        (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamSynchronize(s);
        return RCX_RC_HIP_ERROR;
    };
    for (uint32_t pc = 0; pc < st.pieces; pc++) {
        const uint64_t lo = st.ranges.lo[pc], hi = st.ranges.hi[pc];
        hipError_t e = hipSuccess;
        if (hi > lo) e = hipMemcpyAsync((uint8_t*)c->d_in.p + lo, b->in_base + lo, hi - lo, hipMemcpyHostToDevice, c->copy_stream);
        if (e != hipSuccess) return bail(e, "host path: range copy");
        if ((e = hipEventRecord(c->piece_ev[pc], c->copy_stream)) != hipSuccess) return bail(e, "host path: event record");
        if (pc == 0) {
            const int rcg = launch_codec(c, call, st.k);
            if (rcg) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamSynchronize(s); return rcg; }
            launched = true;
        }
    }
    // this thread tells the launch what has arrived (a word copied in behind each range would be the natural signal; such a small
    // copy is done by a kernel, and a kernel does not run while every slot of the device holds a waiting block: built, measured --
    // every gate ran into its time limit)
    for (uint32_t pc = 0; pc < st.pieces; pc++) {
        const hipError_t e = hipEventSynchronize(c->piece_ev[pc]);
        if (e != hipSuccess) return bail(e, "host path: event wait");
        __atomic_store_n((volatile uint32_t*)(c->h_gate + pc), seq, __ATOMIC_RELEASE);
    }
    st.gated = true;
    return RCX_RC_OK;
}

// stage 6: the launch, behind one copy of the input or with the input in ranges under it
static int launch(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    if (st.pieces > 1 && !rcx_plan_ranges(st.n, st.pieces, (c->param[call.codec] >> 16) & 255u, st.b->in_off, st.b->in_len, st.sp.in_span, st.ranges)) {
        st.pieces = 1;                                                 // (too few ranges, or ranges that overlap: rcx_plan.h)
        if (st.sp.in_span) HIPCHK(c, hipMemcpyAsync(c->d_in.p, st.b->in_base, st.sp.in_span, hipMemcpyHostToDevice, c->stream));
    }
    gate_args g = {};
    if (st.pieces > 1) { st.pieces = st.ranges.pieces(); STAGE(open_gates(c, st, g)); }
    st.k = make_kargs(st.dv, st.d_n_out, st.scratch, st.scratch_bytes, st.mirror, st.pieces > 1 ? &g : nullptr);
    STAGE(st.pieces > 1 ? launch_gated(c, call, st) : launch_codec(c, call, st.k));
    if (st.mirror && !st.k.out_mirror) st.mirror = nullptr;           // the launch says it did not store into the caller's buffer after all: the plain copy in copy_back
    return RCX_RC_OK;
}

// stage 7: the per-block results; true in `late` when a block's input did not arrive in time (a gated launch alone)
static int fetch_results(rcx_ctx* c, batch_state& st, bool& late)
{
    const size_t N = st.n;
    HIPCHK(c, hipMemcpyAsync(st.h64 + 5 * N, st.dv.out_len, 2 * N * 8 + 2 * N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    late = false;
    if (!st.gated) return RCX_RC_OK;
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    for (size_t i = 0; i < N && !late; i++) late = st.h_status[i] == (int32_t)RCX_ST_GATE;
    return RCX_RC_OK;
}

// stage 9, a mirrored inflate: the streams the first pass handed back were decoded into HBM alone -- a few, one copy each; many (a
// batch of corrupted streams), the span
static int copy_back_handed_back(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    const uint32_t n = st.n;
    const uint8_t* marks = (const uint8_t*)st.k.scratch + (call.codec == RCX_GZIP_DECODE ? rcx_tu_gzip_marks_offset(n) : rcx_tu_inflate_marks_offset(n));
    uint32_t nfb = 0;
    HIPCHK(c, hipMemcpy(&nfb, marks, 4, hipMemcpyDeviceToHost));
    if (!nfb) return RCX_RC_OK;
    const uint64_t* ol = st.out_len();
    if (nfb > n / 8u + 16u && !st.out_gaps) {                         // (the span only where it covers slots alone: rcx_plan_out_dense)
        const uint64_t used_span = rcx_plan_used_span(n, b->out_off, b->out_cap, ol);
        if (used_span) HIPCHK(c, hipMemcpy(b->out_base, st.d_out, used_span, hipMemcpyDeviceToHost));
        return RCX_RC_OK;
    }
    std::vector<uint8_t> fb(n);
    HIPCHK(c, hipMemcpy(fb.data(), marks + 64, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t l = ol[i] < b->out_cap[i] ? ol[i] : b->out_cap[i];
        if (fb[i] && l) HIPCHK(c, hipMemcpyAsync(b->out_base + b->out_off[i], st.d_out + b->out_off[i], l, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RCX_RC_OK;
}

// stage 9: the output bytes of a host-memory batch (unless the launch stored them itself), then the per-block results
static int copy_back(rcx_ctx* c, const rcx_call& call, batch_state& st)
{
    const rcx_batch* b = st.b;
    const size_t N = st.n;
    if (st.mirror && st.t.back == BACK_INFLATE && st.k.scratch) STAGE(copy_back_handed_back(c, call, st));
    if (b->mem == RCX_MEM_HOST && st.sp.out_span && !st.mirror) {
        if (st.t.back == BACK_CHAINS) {
            // nothing else of the caller's buffer changes (the staging buffer never held the caller's bytes between the slots)
            for (const auto& r : rcx_plan_chain_copies(st.n, call.link->plan->head(), b->out_off, b->out_cap, st.out_len()))
                HIPCHK(c, hipMemcpyAsync(b->out_base + r.first, st.d_out + r.first, r.second - r.first, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else if (st.t.back == BACK_SLOTS) {
            // (bzip2, zstd: out_len of a file that did not fit is the size it needs; its slot holds nothing to deliver)
            std::vector<uint64_t> made;
            if (call.codec == RCX_BZIP2_DECODE || call.codec == RCX_BZIP2_ENCODE || call.codec == RCX_ZSTD_DECODE) {
                made.assign(st.out_len(), st.out_len() + N);
                for (size_t i = 0; i < N; i++) if (st.h_status[i] == RCX_E_OUTPUT_TOO_SMALL) made[i] = 0;
            }
            for (const auto& r : rcx_plan_slot_copies(st.n, b->out_off, b->out_cap, made.empty() ? st.out_len() : made.data()))
                HIPCHK(c, hipMemcpyAsync(b->out_base + r.first, st.d_out + r.first, r.second - r.first, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else if (st.out_gaps && !st.out_staged) {
            // (a launch that declined the mirror on a layout with gaps: nothing of the caller's buffer was staged, so what the blocks produced)
            for (const auto& r : rcx_plan_slot_copies(st.n, b->out_off, b->out_cap, st.out_len()))
                HIPCHK(c, hipMemcpyAsync(b->out_base + r.first, st.d_out + r.first, r.second - r.first, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else {
            const uint64_t used_span = rcx_plan_used_span(st.n, b->out_off, b->out_cap, st.out_len());
            if (used_span) HIPCHK(c, hipMemcpy(b->out_base, st.d_out, used_span, hipMemcpyDeviceToHost));
        }
    }
    if (b->out_len) memcpy(b->out_len, st.h64 + 5 * N, N * 8);
    if (b->in_used) memcpy(b->in_used, st.h64 + 6 * N, N * 8);
    memcpy(b->status, st.h_status, N * 4);
    if (call.aux_out) memcpy(call.aux_out, st.h_aux, N * 4);
    return RCX_RC_OK;
}

static int run_batch(rcx_ctx* c, const rcx_call& call, const rcx_batch* b)
{
    if (!c) return RCX_RC_BAD_ARG;
    batch_state st;
    STAGE(check_batch(c, call, b, st));
    if (st.n == 0) return RCX_RC_OK;
    for (;;) {
        bool late = false;
        decide_mirror(c, call, st);
        STAGE(stage_in_out(c, call, st));
        STAGE(pack_descriptors(c, call, st));
        STAGE(reserve_scratch(c, call, st));
        STAGE(launch(c, call, st));
        STAGE(fetch_results(c, st, late));
        if (!late) break;
        // stage 8: a gate ran into its limit.  The next GATE_RETRY calls take one copy in front of the launch (decide_mirror)
        c->gate_bad = true; c->gate_bad_calls = GATE_RETRY;
        if (call.codec == RCX_LZ4_DECODE) {                      // the blocks that gave up, by a second launch
            st.k.gate = nullptr; st.gated = false;
            rcx_tu_lz4_decode_mirror_again(c->stream, st.k);
            HIPCHK(c, hipGetLastError());
            STAGE(fetch_results(c, st, late));
            break;
        }
        // (the inflate path's second pass and trailer check passed these streams by: the whole batch again, behind one copy -- gate_bad
        //  keeps this second pass from ranges, so there is no third)
    }
    return copy_back(c, call, st);
}

extern "C" int rcx_lz4_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_LZ4_DECODE), b); }
extern "C" int rcx_lz4_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_LZ4_ENCODE, 0), b); }
extern "C" int rcx_lz4_encode_hc_batch(rcx_ctx* c, const rcx_batch* b, int level)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (level < 1 || level > 12) { c->err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    return run_batch(c, call_of(RCX_LZ4_ENCODE, (uint32_t)level), b);
}
// The history travels in with the input (rcx_plan_spans stages [0, in_span), and a history lies below its block); its lengths go to
// the kernels as 32-bit words in the descriptors' aux array.
extern "C" int rcx_lz4_encode_hc_hist_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* hist_len)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (level < 1 || level > 12) { c->err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(RCX_LZ4_ENCODE_HIST, (uint32_t)level);
    if (!hist_len || !b || !b->nblocks) return run_batch(c, call, b);
    if (!b->in_off) { c->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    std::vector<uint32_t> hist(b->nblocks);
    for (uint32_t i = 0; i < b->nblocks; i++) {
        if (hist_len[i] > b->in_off[i] || hist_len[i] > 65536) {
            c->err = "lz4 hc: block " + std::to_string(i) + ": a history of " + std::to_string(hist_len[i]) + " bytes "
                   + (hist_len[i] > 65536 ? "(at most 65536)" : "does not fit in front of in_off " + std::to_string(b->in_off[i]));
            return RCX_RC_BAD_ARG;
        }
        hist[i] = hist_len[i] > 65535 ? 65535u : (uint32_t)hist_len[i];      // (of 65536 bytes the first is out of every match's reach)
        call.nhist += hist[i] ? 1u : 0u;
    }
    call.aux_in = hist.data();
    return run_batch(c, call, b);                                // (waits for the stream: the lengths above may go)
}
extern "C" int rcx_inflate_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags) { return run_batch(c, call_of(RCX_INFLATE, 0, nullptr, flags), b); }
extern "C" int rcx_zlib_decode_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags) { return run_batch(c, call_of(RCX_ZLIB_DECODE, 0, nullptr, flags), b); }
extern "C" int rcx_adler32_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* adler) { return run_batch(c, call_of(RCX_ADLER32, 0, nullptr, adler), b); }
extern "C" int rcx_crc32_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* crc) { return run_batch(c, call_of(RCX_CRC32, 0, nullptr, crc), b); }
extern "C" int rcx_xxh32_batch(rcx_ctx* c, const rcx_batch* b, uint32_t seed, uint32_t* hash)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (b && b->nblocks && !hash) { c->err = "xxh32: null hash array"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(RCX_XXH32, 0, nullptr, hash);
    call.seed = seed;
    return run_batch(c, call, b);
}
// The chains are laid out on the host -- every block's head, its depth, the blocks sorted by depth (rcx_plan.h) -- and the batch goes
// through run_batch like any other: launch_codec issues one launch per depth (k_lz4_linked.hip).  A linked block's out_off / out_cap
// are the caller's to leave unset: the batch run_batch sees has 0 / 0 there.
extern "C" int rcx_lz4_decode_linked_batch(rcx_ctx* c, const rcx_batch* b, const uint8_t* link, const uint64_t* dict_len)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (!b || (b->nblocks && (!b->out_off || !b->out_cap))) { c->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    const uint32_t n = b->nblocks;
    if (n == 0) return RCX_RC_OK;
    rcx_chain_plan plan;
    if (!rcx_plan_chains(n, link, dict_len, b->out_off, b->out_cap, plan, c->err)) return RCX_RC_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t tab_bytes = ((3 * (size_t)n * 4 + 7) & ~(size_t)7);
    HIPCHK(c, c->d_link.reserve(tab_bytes + (size_t)n * 8));
    HIPCHK(c, hipMemcpyAsync(c->d_link.p, plan.tab.data(), 3 * (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t* d_tab = (const uint32_t*)c->d_link.p;
    const link_tables lt = {&plan, d_tab, d_tab + n, d_tab + 2 * (size_t)n, (uint64_t*)((uint8_t*)c->d_link.p + tab_bytes)};
    rcx_batch bb = *b;
    bb.out_off = plan.out_off.data(); bb.out_cap = plan.out_cap.data();
    rcx_call call = call_of(RCX_LZ4_DECODE_LINKED);
    call.link = &lt;
    return run_batch(c, call, &bb);                              // (waits for the stream: the tables above may go)
}
extern "C" int rcx_gzip_decode_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags) { return run_batch(c, call_of(RCX_GZIP_DECODE, 0, nullptr, flags), b); }
extern "C" int rcx_deflate_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_DEFLATE_ENCODE, 1), b); }
extern "C" int rcx_zlib_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ZLIB_ENCODE, 1), b); }
extern "C" int rcx_gzip_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_GZIP_ENCODE, 1), b); }
static int deflate_level_batch(rcx_ctx* c, int codec, const rcx_batch* b, int level)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (level < 1 || level > 9) { c->err = "deflate encode: level must be 1..9"; return RCX_RC_BAD_ARG; }
    return run_batch(c, call_of(codec, (uint32_t)level), b);
}
extern "C" int rcx_deflate_encode_level_batch(rcx_ctx* c, const rcx_batch* b, int level) { return deflate_level_batch(c, RCX_DEFLATE_ENCODE, b, level); }
extern "C" int rcx_zlib_encode_level_batch(rcx_ctx* c, const rcx_batch* b, int level) { return deflate_level_batch(c, RCX_ZLIB_ENCODE, b, level); }
extern "C" int rcx_gzip_encode_level_batch(rcx_ctx* c, const rcx_batch* b, int level) { return deflate_level_batch(c, RCX_GZIP_ENCODE, b, level); }
// DEFLATE / zlib at levels 2..9 with history.  The history travels in with the input (rcx_plan_spans stages [0, in_span), and a history
// lies below its block); lengths and DICTIDs go to the kernels as 32-bit words in the descriptors' aux array (rcx_plan_hist).
static int deflate_hist_batch(rcx_ctx* c, int codec, const rcx_batch* b, int level, const uint64_t* hist_len, const uint32_t* dict_id)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (level < 2 || level > 9) { c->err = "deflate encode with history: level must be 2..9 (level 1 has none)"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(codec, (uint32_t)level);
    if (!hist_len || !b || !b->nblocks) return run_batch(c, call, b);
    if (!b->in_off) { c->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    if (codec == RCX_ZLIB_ENCODE_DICT && !dict_id) { c->err = "zlib encode with dictionary: null dict_id array"; return RCX_RC_BAD_ARG; }
    std::vector<uint32_t> aux;
    if (!rcx_plan_hist(b->nblocks, hist_len, b->in_off, 32768, dict_id, "deflate encode", aux, call.nhist, c->err)) return RCX_RC_BAD_ARG;
    call.aux_in = aux.data(); call.aux_words = dict_id ? 2 : 1;
    return run_batch(c, call, b);                                // (waits for the stream: the words above may go)
}
extern "C" int rcx_deflate_encode_hist_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* hist_len)
{
    return deflate_hist_batch(c, RCX_DEFLATE_ENCODE_HIST, b, level, hist_len, nullptr);
}
extern "C" int rcx_zlib_encode_dict_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* hist_len, const uint32_t* dict_id)
{
    return deflate_hist_batch(c, RCX_ZLIB_ENCODE_DICT, b, level, hist_len, dict_id);
}
// The encoders behind SHARED DICTIONARIES: block i's history is a range anywhere in the input buffer, and the chains of a range are built
// once for all the blocks that name it (csrc/lz_dict.h).  rcx_plan_dict checks the lengths, clamps and maps blocks to distinct ranges; its
// words go to the kernels in the descriptors' aux array, and the span of the ranges widens what travels in from host memory.
static int shared_batch(rcx_ctx* c, int codec, const rcx_batch* b, int level, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id)
{
    if (!c) return RCX_RC_BAD_ARG;
    const bool lz4 = codec == RCX_LZ4_ENCODE_SHARED;
    if (lz4 && (level < 1 || level > 12)) { c->err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    if (!lz4 && (level < 2 || level > 9)) { c->err = "deflate encode behind shared dictionaries: level must be 2..9 (level 1 has none)"; return RCX_RC_BAD_ARG; }
    if (!dict_off != !dict_len) { c->err = "shared dictionaries: dict_off and dict_len come together or not at all"; return RCX_RC_BAD_ARG; }
    if (!dict_len)                                               // the encoders without history
        return run_batch(c, call_of(lz4 ? RCX_LZ4_ENCODE : codec == RCX_ZLIB_ENCODE_SHARED ? RCX_ZLIB_ENCODE : RCX_DEFLATE_ENCODE, (uint32_t)level), b);
    rcx_call call = call_of(codec, (uint32_t)level);
    if (!b || !b->nblocks) return run_batch(c, call, b);
    if (codec == RCX_ZLIB_ENCODE_SHARED && !dict_id) { c->err = "zlib encode behind shared dictionaries: null dict_id array"; return RCX_RC_BAD_ARG; }
    rcx_dict_plan plan;
    if (!rcx_plan_dict(b->nblocks, dict_off, dict_len, lz4 ? 65536 : 32768, lz4 ? 65535 : 32768, dict_id, lz4 ? "lz4 hc" : "deflate encode", plan, c->err))
        return RCX_RC_BAD_ARG;
    call.aux_in = plan.aux.data(); call.aux_words = RCX_DICT_WORDS; call.nhist = plan.ndict; call.dict_span = plan.span;
    return run_batch(c, call, b);                                // (waits for the stream: the words above may go)
}
extern "C" int rcx_lz4_encode_hc_shared_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* dict_off, const uint64_t* dict_len)
{
    return shared_batch(c, RCX_LZ4_ENCODE_SHARED, b, level, dict_off, dict_len, nullptr);
}
extern "C" int rcx_deflate_encode_shared_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* dict_off, const uint64_t* dict_len)
{
    return shared_batch(c, RCX_DEFLATE_ENCODE_SHARED, b, level, dict_off, dict_len, nullptr);
}
extern "C" int rcx_zlib_encode_shared_batch(rcx_ctx* c, const rcx_batch* b, int level, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id)
{
    return shared_batch(c, RCX_ZLIB_ENCODE_SHARED, b, level, dict_off, dict_len, dict_id);
}
// Inflate with history: the history lies in front of the slot in the OUTPUT buffer and is staged with it (preload_out).  Without
// lengths the call is the plain one.
static int inflate_hist_batch(rcx_ctx* c, int codec, const rcx_batch* b, uint32_t* flags, const uint64_t* hist_len, const uint32_t* dict_id)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (!hist_len || !b || !b->nblocks) return run_batch(c, call_of(codec == RCX_ZLIB_DECODE_DICT ? RCX_ZLIB_DECODE : RCX_INFLATE, 0, nullptr, flags), b);
    if (!b->out_off) { c->err = "null output descriptor"; return RCX_RC_BAD_ARG; }
    if (codec == RCX_ZLIB_DECODE_DICT && !dict_id) { c->err = "zlib decode with dictionary: null dict_id array"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(codec, 0, nullptr, flags);
    std::vector<uint32_t> aux;
    if (!rcx_plan_hist(b->nblocks, hist_len, b->out_off, 32768, dict_id, "inflate", aux, call.nhist, c->err)) return RCX_RC_BAD_ARG;
    call.aux_in = aux.data(); call.aux_words = dict_id ? 2 : 1;
    return run_batch(c, call, b);
}
extern "C" int rcx_inflate_hist_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags, const uint64_t* hist_len)
{
    return inflate_hist_batch(c, RCX_INFLATE_HIST, b, flags, hist_len, nullptr);
}
extern "C" int rcx_zlib_decode_dict_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags, const uint64_t* hist_len, const uint32_t* dict_id)
{
    return inflate_hist_batch(c, RCX_ZLIB_DECODE_DICT, b, flags, hist_len, dict_id);
}
// The decoders behind SHARED DICTIONARIES: the mirror of shared_batch.  rcx_plan_dict as the encoders call it; of its words the kernels
// read the clamped length, the offset and the DICTID (nothing is built per dictionary: no scratch), and the span of the ranges widens
// what travels in from host memory.  The output buffer is not staged in: no slot has anything in front of it that a kernel reads.
static int shared_decode_batch(rcx_ctx* c, int codec, const rcx_batch* b, uint32_t* flags, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id)
{
    if (!c) return RCX_RC_BAD_ARG;
    const bool lz4 = codec == RCX_LZ4_DECODE_SHARED;
    if (!dict_off != !dict_len) { c->err = "shared dictionaries: dict_off and dict_len come together or not at all"; return RCX_RC_BAD_ARG; }
    if (!dict_len || !b || !b->nblocks)                          // the decoders without history
        return run_batch(c, lz4 ? call_of(RCX_LZ4_DECODE) : call_of(codec == RCX_ZLIB_DECODE_SHARED ? RCX_ZLIB_DECODE : RCX_INFLATE, 0, nullptr, flags), b);
    if (codec == RCX_ZLIB_DECODE_SHARED && !dict_id) { c->err = "zlib decode behind shared dictionaries: null dict_id array"; return RCX_RC_BAD_ARG; }
    rcx_dict_plan plan;
    if (!rcx_plan_dict(b->nblocks, dict_off, dict_len, lz4 ? 65536 : 32768, lz4 ? 65535 : 32768, dict_id, lz4 ? "lz4 decode" : "inflate", plan, c->err))
        return RCX_RC_BAD_ARG;
    rcx_call call = call_of(codec, 0, plan.aux.data(), flags);
    call.aux_words = RCX_DICT_WORDS; call.nhist = plan.ndict; call.dict_span = plan.span;
    return run_batch(c, call, b);                                // (waits for the stream: the words above may go)
}
extern "C" int rcx_lz4_decode_shared_batch(rcx_ctx* c, const rcx_batch* b, const uint64_t* dict_off, const uint64_t* dict_len)
{
    return shared_decode_batch(c, RCX_LZ4_DECODE_SHARED, b, nullptr, dict_off, dict_len, nullptr);
}
extern "C" int rcx_inflate_shared_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags, const uint64_t* dict_off, const uint64_t* dict_len)
{
    return shared_decode_batch(c, RCX_INFLATE_SHARED, b, flags, dict_off, dict_len, nullptr);
}
extern "C" int rcx_zlib_decode_shared_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* flags, const uint64_t* dict_off, const uint64_t* dict_len, const uint32_t* dict_id)
{
    return shared_decode_batch(c, RCX_ZLIB_DECODE_SHARED, b, flags, dict_off, dict_len, dict_id);
}
// DICTIONARY TRAINING: job i is block i.  rcx_plan_train checks the arguments, does the epoch arithmetic and carves the scratch; its words
// (the jobs' headers and the sample ends) go to the kernels in the descriptors' aux array, as many words per job as they take.
extern "C" int rcx_dict_train_batch(rcx_ctx* c, const rcx_batch* b, const uint32_t* nsamples, const uint64_t* sample_len, uint32_t k, uint32_t d, uint32_t f)
{
    if (!c) return RCX_RC_BAD_ARG;
    rcx_call call = call_of(RCX_DICT_TRAIN);
    rcx_train_plan plan;
    if (!b) { c->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    if (!rcx_plan_train(b->nblocks, b->in_len, b->out_cap, nsamples, sample_len, k, d, f, plan, c->err)) return RCX_RC_BAD_ARG;
    if (!b->nblocks) return RCX_RC_OK;
    call.aux_in = plan.aux.data(); call.aux_words = plan.aux_words; call.train = &plan;
    return run_batch(c, call, b);                                // (waits for the stream: the plan above may go)
}
// bzip2 files: block i is one whole file.  The stages and their read-backs are in k_bzip2.hip's launch loop; the batch goes through
// run_batch like any other.
extern "C" int rcx_bzip2_decode_batch(rcx_ctx* c, const rcx_batch* b)
{
    if (!c) return RCX_RC_BAD_ARG;
    rcx_call call = call_of(RCX_BZIP2_DECODE);
    call.bz2 = b;
    return run_batch(c, call, b);
}
// ... and written: block i is one whole file and becomes one stream.  The launch loop in k_bzip2_enc.hip plans the blocks from the host
// arrays of the caller's batch, whose offsets are the same in the staged copy.
extern "C" int rcx_bzip2_encode_batch(rcx_ctx* c, const rcx_batch* b, int level)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (level < 1 || level > 9) { c->err = "bzip2 encode: level must be 1..9"; return RCX_RC_BAD_ARG; }
    if (b && b->nblocks > 65535u) { c->err = "bzip2 encode: at most 65535 files a call"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(RCX_BZIP2_ENCODE, (uint32_t)level);
    call.bz2 = b;
    return run_batch(c, call, b);
}
// .zst files: block i is one whole file, one persistent wave each (k_zstd.hip).  rcx_plan_zstd checks the arguments, lays the dictionary
// words out and sizes the scratch; the span of the dictionaries' ranges widens what travels in from host memory.
extern "C" int rcx_zstd_decode_batch(rcx_ctx* c, const rcx_batch* b, const uint64_t* dict_off, const uint64_t* dict_len)
{
    if (!c) return RCX_RC_BAD_ARG;
    rcx_call call = call_of(RCX_ZSTD_DECODE);
    if (!b || !b->nblocks) return run_batch(c, call, b);
    rcx_zstd_plan plan;
    if (!rcx_plan_zstd(b->nblocks, dict_off, dict_len, plan, c->err)) return RCX_RC_BAD_ARG;
    call.aux_in = plan.dict.aux.data(); call.aux_words = RCX_DICT_WORDS; call.dict_span = plan.dict.span; call.zstd = &plan;
    return run_batch(c, call, b);                                // (waits for the stream: the plan above may go)
}
// XXH64 of every block.  The kernel leaves a hash in the descriptors' 64-bit result word, out_len: the caller's array stands in for it.
extern "C" int rcx_xxh64_batch(rcx_ctx* c, const rcx_batch* b, uint64_t seed, uint64_t* hash)
{
    if (!c) return RCX_RC_BAD_ARG;
    if (b && b->nblocks && !hash) { c->err = "xxh64: null hash array"; return RCX_RC_BAD_ARG; }
    rcx_call call = call_of(RCX_XXH64);
    call.seed64 = seed;
    if (!b) return run_batch(c, call, b);
    rcx_batch bb = *b;
    bb.out_len = hash;
    return run_batch(c, call, &bb);
}
extern "C" uint64_t rcx_dict_train_scratch_bytes(uint32_t njobs, uint64_t max_corpus, uint64_t max_cap, uint32_t k, uint32_t f)
{
    return rcx_plan_train_scratch(njobs, max_corpus, max_cap, k, f);
}
extern "C" int rcx_bwt_forward_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* origin) { return run_batch(c, call_of(RCX_BWT_FORWARD, 0, nullptr, origin), b); }
extern "C" int rcx_bwt_suffixes_batch(rcx_ctx* c, const rcx_batch* b, uint32_t* origin) { return run_batch(c, call_of(RCX_BWT_SUFFIXES, 0, nullptr, origin), b); }
extern "C" int rcx_bwt_inversion_table_batch(rcx_ctx* c, const rcx_batch* b, const uint32_t* origin) { return run_batch(c, call_of(RCX_BWT_INVERSION_TABLE, 0, origin), b); }
extern "C" int rcx_bwt_inverse_batch(rcx_ctx* c, const rcx_batch* b, const uint32_t* origin) { return run_batch(c, call_of(RCX_BWT_INVERSE, 0, origin), b); }
extern "C" int rcx_bwt_inverse_minimal_batch(rcx_ctx* c, const rcx_batch* b, const uint32_t* origin) { return run_batch(c, call_of(RCX_BWT_INVERSE_MINIMAL, 0, origin), b); }
extern "C" int rcx_mtf_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_MTF_ENCODE), b); }
extern "C" int rcx_mtf_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_MTF_DECODE), b); }
// the DC codecs' parameter is the kernels' `withctx`: the coding contexts behind the payload (include/rcx.h)
extern "C" int rcx_dc_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_DC_ENCODE, 0), b); }
extern "C" int rcx_dc_decode_batch(rcx_ctx* c, const rcx_batch* b, const uint64_t* n_out) { return run_batch(c, call_of(RCX_DC_DECODE, 0, nullptr, nullptr, n_out), b); }
extern "C" int rcx_dc_encode_ctx_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_DC_ENCODE, 1), b); }
extern "C" int rcx_dc_decode_ctx_batch(rcx_ctx* c, const rcx_batch* b, const uint64_t* n_out) { return run_batch(c, call_of(RCX_DC_DECODE, 1, nullptr, nullptr, n_out), b); }
extern "C" int rcx_ari_byte_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_BYTE_ENCODE), b); }
extern "C" int rcx_ari_byte_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_BYTE_DECODE), b); }
extern "C" int rcx_ari_binary_encode_batch(rcx_ctx* c, const rcx_batch* b, uint32_t rate) { return run_batch(c, call_of(RCX_ARI_BINARY_ENCODE, rate), b); }
extern "C" int rcx_ari_binary_decode_batch(rcx_ctx* c, const rcx_batch* b, uint32_t rate) { return run_batch(c, call_of(RCX_ARI_BINARY_DECODE, rate), b); }
extern "C" int rcx_ari_proxy_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_PROXY_ENCODE), b); }
extern "C" int rcx_ari_proxy_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_PROXY_DECODE), b); }
extern "C" int rcx_ari_apm_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_APM_ENCODE), b); }
extern "C" int rcx_ari_apm_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_ARI_APM_DECODE), b); }
extern "C" int rcx_rle_encode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_RLE_ENCODE), b); }
extern "C" int rcx_rle_decode_batch(rcx_ctx* c, const rcx_batch* b) { return run_batch(c, call_of(RCX_RLE_DECODE), b); }

// ---- more than one device -------------------------------------------------------------------------------------------------
// RCCL, loaded on first use (librcx.so itself does not link it: the library loads wherever HIP does, and a process that has torch's RCCL
// mapped already gets that one -- same SONAME).  Only what a grouped point-to-point exchange needs.
#include <dlfcn.h>
struct RcclApi {
    typedef void* comm_t;
    int (*CommInitAll)(comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
    static RcclApi& get()
    {
        static RcclApi a = [] {
            RcclApi r;
            void* h = nullptr;
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
            if (!h) return r;
            r.CommInitAll = (decltype(r.CommInitAll))dlsym(h, "ncclCommInitAll");
            r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
            r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
            r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
            r.Send = (decltype(r.Send))dlsym(h, "ncclSend");
            r.Recv = (decltype(r.Recv))dlsym(h, "ncclRecv");
            r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
            r.ok = r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv;
            return r;
        }();
        return a;
    }
};
static const int RCCL_UINT8 = 1;                 // ncclUint8 (nccl.h: ncclInt8 = 0, ncclUint8 = 1)

struct rcx_multi {
    std::vector<rcx_ctx*> ctx;
    std::string err;
    // the device-to-device shard path (rcx_multi_scatter_dev / rcx_multi_gather_dev)
    int transport = 0;                           // 0: not chosen yet, 1: RCCL, 2: peer copies
    std::vector<RcclApi::comm_t> comm;
    std::vector<hipEvent_t> ev;                  // peer copies: one event per context
};

extern "C" int rcx_multi_create(const int* device_ids, int n, rcx_multi** out)
{
    if (!out) return RCX_RC_BAD_ARG;
    *out = nullptr;
    if (!device_ids || n <= 0) return RCX_RC_BAD_ARG;
    rcx_multi* m = new rcx_multi();
    for (int i = 0; i < n; i++) {
        rcx_ctx* c = nullptr;
        const int rc = rcx_ctx_create(device_ids[i], &c);
        if (rc != RCX_RC_OK) { for (rcx_ctx* d : m->ctx) rcx_ctx_destroy(d); delete m; return rc; }
        m->ctx.push_back(c);
    }
    *out = m;
    return RCX_RC_OK;
}
extern "C" void rcx_multi_destroy(rcx_multi* m)
{
    if (!m) return;
    for (RcclApi::comm_t q : m->comm) if (q) (void)RcclApi::get().CommDestroy(q);
    for (size_t g = 0; g < m->ev.size(); g++) if (m->ev[g]) { (void)hipSetDevice(m->ctx[g]->device); (void)hipEventDestroy(m->ev[g]); }
    for (rcx_ctx* c : m->ctx) rcx_ctx_destroy(c);
    delete m;
}
extern "C" const char* rcx_multi_transport(const rcx_multi* m) { return !m ? "" : m->transport == 1 ? "rccl" : m->transport == 2 ? "peer" : ""; }

// choose and set up the transport once per set
static int multi_transport_init(rcx_multi* m)
{
    if (m->transport) return RCX_RC_OK;
    const size_t G = m->ctx.size();
    bool distinct = true;
    for (size_t a = 0; a < G; a++) for (size_t b = a + 1; b < G; b++) if (m->ctx[a]->device == m->ctx[b]->device) distinct = false;
    const char* want = getenv("RCX_MULTI_TRANSPORT");
    const bool force_peer = want && !strcmp(want, "peer"), force_rccl = want && !strcmp(want, "rccl");
    if (!force_peer && distinct && RcclApi::get().ok) {
        std::vector<int> devs(G);
        for (size_t g = 0; g < G; g++) devs[g] = m->ctx[g]->device;
        m->comm.assign(G, nullptr);
        const int e = RcclApi::get().CommInitAll(m->comm.data(), (int)G, devs.data());
        if (e == 0) { m->transport = 1; return RCX_RC_OK; }
        m->comm.clear();
        if (force_rccl) { m->err = std::string("ncclCommInitAll: ") + (RcclApi::get().GetErrorString ? RcclApi::get().GetErrorString(e) : "failed"); return RCX_RC_HIP_ERROR; }
    } else if (force_rccl) { m->err = distinct ? "RCX_MULTI_TRANSPORT=rccl: librccl could not be loaded" : "RCX_MULTI_TRANSPORT=rccl: the set lists a device more than once (RCCL wants one rank per device)"; return RCX_RC_BAD_ARG; }
    // peer copies: every device reads / writes every other's memory where the hardware allows (xGMI within a node); where it does not,
    // hipMemcpyPeerAsync stages through the host by itself
    for (size_t a = 0; a < G; a++) {
        if (hipSetDevice(m->ctx[a]->device) != hipSuccess) { (void)hipGetLastError(); m->err = "hipSetDevice failed"; return RCX_RC_HIP_ERROR; }
        for (size_t b = 0; b < G; b++) {
            if (m->ctx[a]->device == m->ctx[b]->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, m->ctx[a]->device, m->ctx[b]->device) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(m->ctx[b]->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                else (void)hipGetLastError();
            } else (void)hipGetLastError();
        }
    }
    m->ev.assign(G, nullptr);
    for (size_t g = 0; g < G; g++) {
        if (hipSetDevice(m->ctx[g]->device) != hipSuccess || hipEventCreateWithFlags(&m->ev[g], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); m->err = "cannot create an event"; return RCX_RC_HIP_ERROR; }
    }
    m->transport = 2;
    return RCX_RC_OK;
}

// ranges root -> peers (scatter) or peers -> root (gather); see include/rcx.h
static int multi_move(rcx_multi* m, int root, uint8_t* root_buf, const uint64_t* range_off, uint8_t* const* peer_buf, bool scatter)
{
    if (!m || m->ctx.empty()) return RCX_RC_BAD_ARG;
    m->err.clear();
    const int G = (int)m->ctx.size();
    if (root < 0 || root >= G || !range_off || !peer_buf) { m->err = "bad root / null range table"; return RCX_RC_BAD_ARG; }
    for (int g = 0; g < G; g++) {
        if (range_off[g + 1] < range_off[g]) { m->err = "ranges must not decrease"; return RCX_RC_BAD_ARG; }
        if (range_off[g + 1] > range_off[g] && (!root_buf || (!peer_buf[g] && g != root))) { m->err = "null buffer for a non-empty range"; return RCX_RC_BAD_ARG; }
    }
    const int rc = multi_transport_init(m);
    if (rc != RCX_RC_OK) return rc;
    rcx_ctx* R = m->ctx[(size_t)root];
    if (m->transport == 1) {
        RcclApi& N = RcclApi::get();
        int e = N.GroupStart();
        for (int g = 0; g < G && e == 0; g++) {
            const uint64_t bytes = range_off[g + 1] - range_off[g];
            if (!bytes || (g == root && !peer_buf[g])) continue;
            uint8_t* rp = root_buf + range_off[g];
            rcx_ctx* P = m->ctx[(size_t)g];
            if (scatter) { e = N.Send(rp, bytes, RCCL_UINT8, g, m->comm[(size_t)root], R->stream); if (!e) e = N.Recv(peer_buf[g], bytes, RCCL_UINT8, root, m->comm[(size_t)g], P->stream); }
            else { e = N.Send(peer_buf[g], bytes, RCCL_UINT8, root, m->comm[(size_t)g], P->stream); if (!e) e = N.Recv(rp, bytes, RCCL_UINT8, g, m->comm[(size_t)root], R->stream); }
        }
        const int e2 = N.GroupEnd();
        if (e || e2) { m->err = std::string(scatter ? "scatter" : "gather") + ": " + (N.GetErrorString ? N.GetErrorString(e ? e : e2) : "RCCL error"); return RCX_RC_HIP_ERROR; }
        return RCX_RC_OK;
    }
    // peer copies.  scatter: every receiving stream waits for what the root's stream has produced so far, then copies its range in;
    // gather: every sending stream copies its range out behind its own launches, and the root's stream waits for all of them.
#define MCHK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { (void)hipGetLastError(); m->err = std::string(#call) + ": " + hipGetErrorString(e_); return RCX_RC_HIP_ERROR; } } while (0)
    if (scatter) { MCHK(hipSetDevice(R->device)); MCHK(hipEventRecord(m->ev[(size_t)root], R->stream)); }
    for (int g = 0; g < G; g++) {
        const uint64_t bytes = range_off[g + 1] - range_off[g];
        if (!bytes || (g == root && !peer_buf[g])) continue;
        uint8_t* rp = root_buf + range_off[g];
        rcx_ctx* P = m->ctx[(size_t)g];
        MCHK(hipSetDevice(P->device));
        if (scatter) {
            if (g != root) MCHK(hipStreamWaitEvent(P->stream, m->ev[(size_t)root], 0));
            MCHK(hipMemcpyPeerAsync(peer_buf[g], P->device, rp, R->device, bytes, P->stream));
        } else {
            MCHK(hipMemcpyPeerAsync(rp, R->device, peer_buf[g], P->device, bytes, P->stream));
            if (g != root) { MCHK(hipEventRecord(m->ev[(size_t)g], P->stream)); MCHK(hipSetDevice(R->device)); MCHK(hipStreamWaitEvent(R->stream, m->ev[(size_t)g], 0)); }
        }
    }
#undef MCHK
    return RCX_RC_OK;
}
extern "C" int rcx_multi_scatter_dev(rcx_multi* m, int root, const uint8_t* root_buf, const uint64_t* range_off, uint8_t* const* peer_buf)
{
    return multi_move(m, root, const_cast<uint8_t*>(root_buf), range_off, peer_buf, true);
}
extern "C" int rcx_multi_gather_dev(rcx_multi* m, int root, uint8_t* root_buf, const uint64_t* range_off, const uint8_t* const* peer_buf)
{
    return multi_move(m, root, root_buf, range_off, const_cast<uint8_t* const*>(reinterpret_cast<const uint8_t* const*>(peer_buf)), false);
}
extern "C" int rcx_multi_count(const rcx_multi* m) { return m ? (int)m->ctx.size() : 0; }
extern "C" rcx_ctx* rcx_multi_ctx(rcx_multi* m, int i) { return (m && i >= 0 && (size_t)i < m->ctx.size()) ? m->ctx[(size_t)i] : nullptr; }
extern "C" const char* rcx_multi_last_error(const rcx_multi* m) { return m ? m->err.c_str() : "null multi"; }

// contiguous ranges balanced by weight: range g ends where the running sum first reaches g / parts of the total (what
// rust_compress_amd/dist.py `partition` and host/compress.hpp `partition` compute)
extern "C" void rcx_partition(const uint64_t* weights, uint32_t nblocks, uint32_t parts, uint32_t* bounds)
{
    if (!bounds || parts == 0) return;
    for (uint32_t g = 0; g <= parts; g++) bounds[g] = nblocks;
    bounds[0] = 0;
    if (!weights || nblocks == 0) return;
    long double total = 0, run = 0;
    for (uint32_t i = 0; i < nblocks; i++) total += (long double)weights[i];
    uint32_t g = 1;
    for (uint32_t i = 0; i < nblocks && g < parts; i++) {
        while (g < parts && run >= total * g / parts) bounds[g++] = i;
        run += (long double)weights[i];
    }
}

// one codec's host-descriptor entry point by its number (what rcx_multi_batch runs on a range)
static int run_codec(rcx_ctx* c, int codec, const rcx_batch* b, const uint32_t* aux_in, uint32_t* aux_out, const uint64_t* n_out)
{
    if (codec < 0 || codec >= RCX_CODEC_COUNT) { c->err = "unknown codec"; return RCX_RC_BAD_ARG; }
    // the parameter of the codec's one-device entry point: LZ4 encode the reference's encoder, DC without contexts (0), DEFLATE level 1;
    // the ARI binary rate, which those entry points take as an argument, is the context's (rcx_ctx_set_param)
    uint32_t param = 0;
    if (codec == RCX_DEFLATE_ENCODE || codec == RCX_ZLIB_ENCODE || codec == RCX_GZIP_ENCODE) param = 1;
    if (codec == RCX_ARI_BINARY_ENCODE || codec == RCX_ARI_BINARY_DECODE) param = c->param[codec];
    switch (codec) {
    case RCX_DC_DECODE: if (!n_out) { c->err = "dc decode: n_out missing"; return RCX_RC_BAD_ARG; } return run_batch(c, call_of(codec, param, nullptr, nullptr, n_out), b);
    case RCX_BWT_INVERSE: case RCX_BWT_INVERSE_MINIMAL: case RCX_BWT_INVERSION_TABLE:
        if (!aux_in) { c->err = "bwt inverse: origins missing"; return RCX_RC_BAD_ARG; }
        return run_batch(c, call_of(codec, param, aux_in), b);
    default: return run_batch(c, call_of(codec, param, nullptr, aux_out), b);
    }
}

extern "C" int rcx_multi_batch(rcx_multi* m, int codec, const rcx_batch* b, const uint32_t* aux_in, uint32_t* aux_out, const uint64_t* n_out)
{
    if (!m || m->ctx.empty()) return RCX_RC_BAD_ARG;
    if (!b || (b->nblocks && (!b->in_off || !b->in_len || !b->status))) { m->err = "null descriptor array"; return RCX_RC_BAD_ARG; }
    if (b->mem != RCX_MEM_HOST) { m->err = "rcx_multi_batch takes host-memory batches (device-resident ranges: rcx_multi_launch_dev)"; return RCX_RC_BAD_ARG; }
    if (!dc_words_aligned(codec, b, m->err)) return RCX_RC_BAD_ARG;      // (before the ranges' offsets are rebased: what one context refuses)
    const uint32_t n = b->nblocks, G = (uint32_t)m->ctx.size();
    if (n == 0) return RCX_RC_OK;
    const bool has_out = b->out_off && b->out_cap;
    m->err.clear();
    std::vector<uint32_t> bounds; std::vector<int> rcs; std::vector<std::thread> th;
    try { bounds.resize(G + 1); rcs.assign(G, RCX_RC_OK); th.reserve(G); } catch (...) { m->err = "out of memory"; return RCX_RC_NO_MEMORY; }
    rcx_partition(has_out ? b->out_cap : b->in_len, n, G, bounds.data());
    int spawn_rc = RCX_RC_OK;
    for (uint32_t g = 0; g < G && spawn_rc == RCX_RC_OK; g++) {
        const uint32_t a0 = bounds[g], a1 = bounds[g + 1];
        if (a1 <= a0) continue;
        try {
        th.emplace_back([&, g, a0, a1] {
          try {
            // the range's own view of the host buffers: offsets rebased to the range's first byte, so that only its span travels
            const uint32_t k = a1 - a0;
            uint64_t lo_in = ~0ull, lo_out = ~0ull;
            for (uint32_t i = a0; i < a1; i++) { if (b->in_off[i] < lo_in) lo_in = b->in_off[i]; if (has_out && b->out_off[i] < lo_out) lo_out = b->out_off[i]; }
            std::vector<uint64_t> io(k), oo(has_out ? k : 0);
            for (uint32_t i = 0; i < k; i++) { io[i] = b->in_off[a0 + i] - lo_in; if (has_out) oo[i] = b->out_off[a0 + i] - lo_out; }
            rcx_batch sb = *b;
            sb.in_base = b->in_base ? b->in_base + lo_in : nullptr; sb.in_off = io.data(); sb.in_len = b->in_len + a0;
            if (has_out) { sb.out_base = b->out_base ? b->out_base + lo_out : nullptr; sb.out_off = oo.data(); sb.out_cap = b->out_cap + a0; }
            if (b->out_len) sb.out_len = b->out_len + a0;
            if (b->in_used) sb.in_used = b->in_used + a0;
            sb.status = b->status + a0;
            sb.nblocks = k;
            rcs[g] = run_codec(m->ctx[g], codec, &sb, aux_in ? aux_in + a0 : nullptr, aux_out ? aux_out + a0 : nullptr, n_out ? n_out + a0 : nullptr);
          } catch (const std::bad_alloc&) { m->ctx[g]->err = "out of memory"; rcs[g] = RCX_RC_NO_MEMORY; }
            catch (...) { m->ctx[g]->err = "unexpected exception"; rcs[g] = RCX_RC_HIP_ERROR; }
        });
        } catch (...) { spawn_rc = RCX_RC_NO_MEMORY; }                       // (std::system_error: no thread to be had; the ones started are joined below)
    }
    for (std::thread& t : th) t.join();
    if (spawn_rc != RCX_RC_OK) { m->err = "cannot start a worker thread"; return spawn_rc; }
    for (uint32_t g = 0; g < G; g++)
        if (rcs[g] != RCX_RC_OK) { m->err = "device range " + std::to_string(g) + ": " + m->ctx[g]->err; return rcs[g]; }
    return RCX_RC_OK;
}

extern "C" int rcx_multi_launch_dev(rcx_multi* m, int codec, const rcx_dev_batch* const* per_device, void* const* scratch, const uint64_t* scratch_bytes)
{
    if (!m || !per_device) return RCX_RC_BAD_ARG;
    m->err.clear();
    for (size_t g = 0; g < m->ctx.size(); g++) {
        if (!per_device[g] || per_device[g]->nblocks == 0) continue;
        const int rc = rcx_launch_dev(m->ctx[g], codec, per_device[g], scratch ? scratch[g] : nullptr, scratch_bytes ? scratch_bytes[g] : 0);
        if (rc != RCX_RC_OK) { m->err = "device range " + std::to_string(g) + ": " + m->ctx[g]->err; return rc; }
    }
    return RCX_RC_OK;
}

extern "C" int rcx_multi_sync(rcx_multi* m)
{
    if (!m) return RCX_RC_BAD_ARG;
    for (size_t g = 0; g < m->ctx.size(); g++) {
        rcx_ctx* c = m->ctx[g];
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { m->err = "device range " + std::to_string(g) + ": synchronize failed"; return RCX_RC_HIP_ERROR; }
    }
    return RCX_RC_OK;
}

// ---- measurement aid: the device's own copy rate (include/rcx.h) ------------------------------------------------------------------
// ONE 16-byte chunk a thread, a workgroup per 4 KiB, the whole buffer in one launch: 6.23 TB/s on the MI355X box, what
// /opt/skills/guides/MI355X_MICROARCH.md measures with a float4 copy (6.29).  benchmarks/micro/hbm_copy.hip tried the shapes: grid-stride
// loops (4 .. 32 workgroups a CU, 1 / 4 / 8 chunks in flight a thread, nontemporal or not) reach 4.3 - 5.5 TB/s, hipMemcpy 4.7, torch's
// copy_ 5.4 -- more loads in flight per thread do not help a copy, more workgroups in flight do.
__global__ __launch_bounds__(256) void k_hbm_copy(const rcx_u32x4* __restrict__ src, rcx_u32x4* __restrict__ dst, uint64_t n16)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}
extern "C" int rcx_hbm_copy_probe(rcx_ctx* c, uint64_t bytes, int reps, double* gb_per_s)
{
    if (!c || !gb_per_s || bytes < 4096 || reps < 1) return RCX_RC_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n16 = bytes / 16;
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = RCX_RC_OK;
    if ((n16 + 255) / 256 > 0x7fffffffull) { c->err = "copy probe: buffer too large"; return RCX_RC_BAD_ARG; }
    const uint32_t grid = (uint32_t)((n16 + 255) / 256);
    float ms = 0;
    if (hipMalloc(&a, n16 * 16) != hipSuccess || hipMalloc(&b, n16 * 16) != hipSuccess) { (void)hipGetLastError(); c->err = "copy probe: out of device memory"; rc = RCX_RC_NO_MEMORY; }
    else if (hipMemsetAsync(a, 0x5a, n16 * 16, c->stream) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); c->err = "copy probe: setup failed"; rc = RCX_RC_HIP_ERROR; }
    else {
        hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, c->stream, (const rcx_u32x4*)a, (rcx_u32x4*)b, n16);      // warm-up
        (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps; r++) hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, c->stream, (const rcx_u32x4*)a, (rcx_u32x4*)b, n16);
        (void)hipEventRecord(e1, c->stream);
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0) { (void)hipGetLastError(); c->err = "copy probe: timing failed"; rc = RCX_RC_HIP_ERROR; }
        else *gb_per_s = 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    return rc;
}

// ---- page-locking a caller's buffers (include/rcx.h) -----------------------------------------------------------------------------
extern "C" int rcx_host_register(void* ptr, uint64_t bytes)
{
    if (!ptr || !bytes) return RCX_RC_BAD_ARG;
    const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable | hipHostRegisterMapped);
    if (e == hipSuccess) return RCX_RC_OK;
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? RCX_RC_NO_MEMORY : e == hipErrorNoDevice ? RCX_RC_NO_DEVICE : RCX_RC_HIP_ERROR;
}
extern "C" int rcx_host_unregister(void* ptr)
{
    if (!ptr) return RCX_RC_BAD_ARG;
    const hipError_t e = hipHostUnregister(ptr);
    if (e == hipSuccess) return RCX_RC_OK;
    (void)hipGetLastError();
    return RCX_RC_HIP_ERROR;
}
