// k_inflate_dict.hip -- DEFLATE / zlib decode behind SHARED DICTIONARIES: stream b's history is a range anywhere in the INPUT buffer
// (rcx_inflate_shared_batch / rcx_zlib_decode_shared_batch, include/rcx.h), not the bytes in front of its slot.  What it computes is
// what k_inflate_hist.hip computes for the same stream with the same dictionary bytes copied directly in front of the slot: bytes,
// out_len, in_used, status and flags, malformed streams included.  Included behind k_inflate2.hip: one LANE per stream on that
// file's F2 machinery (tables, bit reader, ring, drains, f2_stored / f2_fixed / f2_dynamic) with F2DictSrc as the source policy.
//
// POSITIONS ARE THE SLOT'S: F2::out is the slot, end and flushed start at 0 and cap is the slot's, so every address formed from them
// lies in the slot (k_inflate_hist's `out - hist` would point below an allocation whose first slot sits at offset 0).  The dictionary
// (D bytes after the clamp, at `dict`) stands for the positions -D .. -1:
//   the distance rule   flate.rs:314 with the history counted in: distance <= min(end + D, 32768)
//   the ring            RB() indexes modulo F2_W, so position end - distance is the same ring byte whether or not the subtraction
//                       wraps below 0; the ring is seeded with the dictionary's last min(D, F2_W) bytes at positions -1, -2, ... --
//                       not through emit: the Adler-32 (the zlib trailer covers the decoded block alone) must not see them
//   far sources         (distance >= F2_NEAR) are gathered 16 bytes at a time by F2DictSrc::gather: a position below 0 is
//                       dict[D + position], anything else the slot's.  A gather that straddles position 0 is put together byte by
//                       byte, its low bytes from the dictionary's end and its high bytes from the slot's start: no 16-byte load ever
//                       crosses the dictionary's last byte or begins below its first, so a dictionary may end at the input buffer's
//                       last byte and what lies around it in memory is never loaded.  (The slot bytes of a straddling gather are at
//                       most end - distance + 15 <= end - 97: drained long ago, as every far source is.)
//   omis, the drains    the slot's, as in k_inflate2.
//
// aux: the words of rcx_plan_dict (rcx_plan.h, laid out by lz_dict.h): aux[b] = D when the kernel starts and the stream's flags when
// it ends, aux[n + b] = the DICTID the caller expects (zlib), aux[3n + b] / aux[4n + b] = the dictionary's offset from in_base.  The
// dictionary index and the per-dictionary words are not read: nothing is built per dictionary.  zlib header as in k_inflate_hist.hip.

template <int SPW, int LG, int MINW>
__global__ __launch_bounds__(64, MINW) void k_inflate_dict(rcx_kargs a, int zlib)
{
    static_assert((1 << LG) == SPW && SPW <= 64, "streams per wave");
    __shared__ __align__(16) uint8_t s_mem[F2_LDS_PER_STREAM * SPW];
    const unsigned t = threadIdx.x;
    const uint32_t b = blockIdx.x * SPW + t;
    const uint64_t n = a.nblocks;
    if (b >= n) return;
    uint32_t D = a.aux[b] < 32768u ? a.aux[b] : 32768u;
    const uint8_t* dict = a.in_base + ((uint64_t)a.aux[3 * n + b] | ((uint64_t)a.aux[4 * n + b] << 32));
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
            else if ((flg & 0x20) && !D) st = RCX_E_ZLIB_DICT;
            else if ((cmf * 256 + flg) % 31 != 0) st = RCX_E_ZLIB_HEADER_CHECKSUM;
            else if (flg & 0x20) {
                if (s.n < 6) { st = RCX_E_EOF; s.p = s.n; }
                else {
                    const uint32_t id = ((uint32_t)s.in[2] << 24) | ((uint32_t)s.in[3] << 16) | ((uint32_t)s.in[4] << 8) | (uint32_t)s.in[5];
                    s.p = 6;
                    if (id != a.aux[n + b]) st = RCX_E_ZLIB_DICT_ID;
                }
            } else D = 0;                                                  // no FDICT: the dictionary is not this stream's
        }
    }
    s.out = a.out_base + a.out_off[b]; s.cap = a.out_cap[b]; s.end = 0; s.flushed = 0;
    s.omis = (uint32_t)((uintptr_t)s.out & 15u);
    if (!st) for (uint32_t i = 1; i <= D && i <= F2_W; i++) *s.RB((uint64_t)0 - i) = dict[D - i];
    bool eof = false;
    while (!st && !eof) {                                                  // Decoder::block :195-206, to BFINAL
        uint32_t x;
        const uint64_t before = s.end;
        if ((st = s.bits(1, x))) break;
        if (x == 1) eof = true;                                            // :198
        if ((st = s.bits(2, x))) break;                                    // :199
        if (x == 0) st = f2_stored(s);
        else if (x == 1) st = f2_fixed(s, HL, HD, lens, F2DictSrc{dict, D});
        else if (x == 2) st = f2_dynamic(s, HL, HD, lens, F2DictSrc{dict, D});
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
    a.out_len[b] = s.end;
    if (a.in_used) a.in_used[b] = used;
    a.aux[b] = flags;
}

// k.aux: the words of rcx_plan_dict, never null
static void launch_inflate_dict(hipStream_t s, rcx_kargs& k, bool zlib)
{
    F2_LAUNCH(k_inflate_dict, f2_streams_per_wave(k.nblocks), s, k, zlib ? 1 : 0);
}
