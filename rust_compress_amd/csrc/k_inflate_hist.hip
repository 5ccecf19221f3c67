// k_inflate_hist.hip -- DEFLATE / zlib decode with HISTORY: stream b's matches may reach into the hist[b] bytes (at most 32768) that
// lie directly before its slot in the output buffer -- a preset dictionary (RFC 1950 FDICT, zlib's inflateSetDictionary), or the 32 KiB
// in front of a chunk of one long stream.  The mirror of dict_len in k_lz4_linked.hip.  Included behind k_inflate2.hip: one LANE per
// stream on that file's F2 machinery (tables, bit reader, ring, f2_stored / f2_fixed / f2_dynamic with the slot source policy).
//
// NOT in the reference crate (src/zlib.rs:71 refuses FDICT): an extension, checked against libz (zdict=).
//
// The stream is decoded as a VIRTUAL stream that starts hist bytes behind its slot: F2::out points at the first history byte, end and
// flushed start at hist, cap grows by hist.  The slot source policy's window rule (flate.rs:314: distance <= min(output so far, 32768))
// then counts the history in, far matches gather from out + (end - distance) whether that lies in the history or in the slot, and the
// drain stores [flushed, end) only: the history is read and never written; out_len is end - hist.  omis and the 16-byte drains follow
// the virtual pointer.  Distances below F2_NEAR are served from the 128-byte ring, so the ring is seeded with the last
// min(hist, 128) history bytes -- not through emit: the Adler-32 sums (the zlib trailer covers the decoded block alone) must not see
// them.
//
// aux[b] = hist[b] (uint32) when the kernel starts, the stream's flags when it ends; zlib form: aux[n + b] = the DICTID the caller
// expects.  zlib header (RFC 1950 2.2): FDICT clear -- the history is ignored (libz never asks for one) and the stream is
// k_inflate2's; FDICT set and no history -- RCX_E_ZLIB_DICT as there (checked before the header checksum); FDICT set and a history
// -- the four DICTID bytes behind the header count in in_used and must equal aux[n + b], else RCX_E_ZLIB_DICT_ID with nothing
// decoded; a stream that ends inside them is RCX_E_EOF with every byte used.

template <int SPW, int LG, int MINW>
__global__ __launch_bounds__(64, MINW) void k_inflate_hist(rcx_kargs a, int zlib)
{
    static_assert((1 << LG) == SPW && SPW <= 64, "streams per wave");
    __shared__ __align__(16) uint8_t s_mem[F2_LDS_PER_STREAM * SPW];
    const unsigned t = threadIdx.x;
    const uint32_t b = blockIdx.x * SPW + t;
    if (b >= a.nblocks) return;
    uint32_t hist = a.aux[b] < 32768u ? a.aux[b] : 32768u;
    F2 s;
    s.lg = LG;
    s.lsym = s_mem; s.lbit = (uint32_t*)(s_mem + 288 * SPW); s.dsym = s_mem + 288 * SPW + 9 * 4 * SPW;
    s.ring = (uint32_t*)(s_mem + 288 * SPW + 9 * 4 * SPW + 32 * SPW); s.t = t;
    s.in = a.in_base + a.in_off[b]; s.n = a.in_len[b]; s.p = 0;
    s.bb = 0; s.bc = 0; s.nx = 0; s.nxv = false; s.a = 1; s.b = 0; s.pend = 0;
    uint8_t lens[320];
    F2Huff HL, HD;
    int st = RCX_OK;
    uint32_t flags = 0;
    if (zlib) {                                                            // validate_header, zlib.rs:55-86, + FDICT
        if (s.n < 2) { st = RCX_E_EOF; s.p = s.n; }
        else {
            const uint32_t cmf = s.in[0], flg = s.in[1];
            s.p = 2;
            if ((cmf & 0xf) != 0x8) st = RCX_E_ZLIB_FORMAT;
            else if ((cmf & 0xf0) != 0x70) st = RCX_E_ZLIB_WINDOW;
            else if ((flg & 0x20) && !hist) st = RCX_E_ZLIB_DICT;
            else if ((cmf * 256 + flg) % 31 != 0) st = RCX_E_ZLIB_HEADER_CHECKSUM;
            else if (flg & 0x20) {
                if (s.n < 6) { st = RCX_E_EOF; s.p = s.n; }
                else {
                    const uint32_t id = ((uint32_t)s.in[2] << 24) | ((uint32_t)s.in[3] << 16) | ((uint32_t)s.in[4] << 8) | (uint32_t)s.in[5];
                    s.p = 6;
                    if (id != a.aux[a.nblocks + b]) st = RCX_E_ZLIB_DICT_ID;
                }
            } else hist = 0;                                               // no FDICT: the history is not this stream's
        }
    }
    // the virtual stream: hist bytes of history, then the slot
    s.out = a.out_base + a.out_off[b] - hist; s.cap = a.out_cap[b] + hist; s.end = hist; s.flushed = hist;
    s.omis = (uint32_t)((uintptr_t)s.out & 15u);
    if (!st) for (uint32_t i = hist < F2_W ? 0u : hist - F2_W; i < hist; i++) *s.RB(i) = s.out[i];
    bool eof = false;
    while (!st && !eof) {                                                  // Decoder::block :195-206, to BFINAL
        uint32_t x;
        const uint64_t before = s.end;
        if ((st = s.bits(1, x))) break;
        if (x == 1) eof = true;                                            // :198
        if ((st = s.bits(2, x))) break;                                    // :199
        if (x == 0) st = f2_stored(s);
        else if (x == 1) st = f2_fixed(s, HL, HD, lens, F2SlotSrc{});
        else if (x == 2) st = f2_dynamic(s, HL, HD, lens, F2SlotSrc{});
        else st = RCX_E_INVALID_BLOCK_CODE;                                // :203
        if (!st && s.end == before && !eof) flags |= RCX_W_EMPTY_BLOCK_MIDSTREAM;   // :474-476 quirk
    }
    uint64_t used = s.used();                                              // a dry bit reader leaves p == n, bc == 0
    if (zlib && !st) {                                                     // zlib.rs:108-118: the block's own bytes
        uint64_t q = s.used();
        if (s.n - q < 4) st = RCX_E_EOF;
        else {
            const uint32_t ck = ((uint32_t)s.in[q] << 24) | ((uint32_t)s.in[q + 1] << 16) |
                                ((uint32_t)s.in[q + 2] << 8) | (uint32_t)s.in[q + 3];
            used = q + 4;
            const uint32_t mine = ((s.b % 65521u) << 16) | (s.a % 65521u);
            if (ck != mine) st = RCX_E_ZLIB_CHECKSUM;
        }
    }
    s.drain(s.end);                                                        // what was produced is delivered, error or not
    a.status[b] = st;
    a.out_len[b] = s.end - hist;
    if (a.in_used) a.in_used[b] = used;
    a.aux[b] = flags;
}

// k.aux: n history lengths (+ n DICTIDs: zlib), never null
static void launch_inflate_hist(hipStream_t s, rcx_kargs& k, bool zlib)
{
    F2_LAUNCH(k_inflate_hist, f2_streams_per_wave(k.nblocks), s, k, zlib ? 1 : 0);
}
