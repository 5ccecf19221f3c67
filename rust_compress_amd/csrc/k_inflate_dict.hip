// k_inflate_dict.hip -- DEFLATE / zlib decode behind SHARED DICTIONARIES: stream b's history is a range anywhere in the INPUT buffer
// (rcx_inflate_shared_batch / rcx_zlib_decode_shared_batch, include/rcx.h), not the bytes in front of its slot.  What it computes is
// what k_inflate_hist.hip computes for the same stream with the same dictionary bytes copied directly in front of the slot: bytes,
// out_len, in_used, status and flags, malformed streams included.  Included behind k_inflate2.hip: one LANE per stream on that file's
// F2 machinery (tables, bit reader, ring, drains, f2_stored), unchanged, with launch_inflate_hist's streams-per-wave choice.
//
// POSITIONS ARE THE SLOT'S: F2::out is the slot, end and flushed start at 0 and cap is the slot's, so every address formed from them
// lies in the slot (k_inflate_hist's `out - hist` would point below an allocation whose first slot sits at offset 0).  The dictionary
// (D bytes after the clamp, at `dict`) stands for the positions -D .. -1:
//   the distance rule   flate.rs:314 with the history counted in: distance <= min(end + D, 32768)
//   the ring            RB() indexes modulo F2_W, so position end - distance is the same ring byte whether or not the subtraction
//                       wraps below 0; the ring is seeded with the dictionary's last min(D, F2_W) bytes at positions -1, -2, ... --
//                       not through emit: the Adler-32 (the zlib trailer covers the decoded block alone) must not see them
//   far sources         (distance >= F2_NEAR) are gathered 16 bytes at a time by f2d_gather: a position below 0 is dict[D + position],
//                       anything else the slot's.  A gather that straddles position 0 is put together byte by byte, its low bytes
//                       from the dictionary's end and its high bytes from the slot's start: no 16-byte load ever crosses the
//                       dictionary's last byte or begins below its first, so a dictionary may end at the input buffer's last byte
//                       and what lies around it in memory is never loaded.  (The slot bytes of a straddling gather are at most
//                       end - distance + 15 <= end - 97: drained long ago, as every far source is.)
//   omis, the drains    the slot's, as in k_inflate2.
// KNOWN COST: f2d_codes, f2d_fixed and f2d_dynamic below repeat f2_codes, f2_fixed and f2_dynamic of k_inflate2.hip -- f2d_codes with
// the split source and the distance rule above, the other two because they end in a call of it -- so a fix to one must be made in the
// other.  A source-policy template parameter on f2_codes would avoid that, but it changes the text every other kernel of
// tu_inflate.hip is compiled from; fold them together when those kernels are next re-measured.
//
// aux: the words of rcx_plan_dict (rcx_plan.h, laid out by lz_dict.h): aux[b] = D when the kernel starts and the stream's flags when
// it ends, aux[n + b] = the DICTID the caller expects (zlib), aux[3n + b] / aux[4n + b] = the dictionary's offset from in_base.  The
// dictionary index and the per-dictionary words are not read: nothing is built per dictionary.  zlib header as in k_inflate_hist.hip.

// 16 bytes of the far source at slot position `src` (src + D >= 0: the distance rule), src + 16 <= end - 96
__device__ __forceinline__ rcx_u32x4 f2d_gather(const F2& s, const uint8_t* dict, uint32_t D, int64_t src)
{
    if (src >= 0 && (uint64_t)src + 16 <= s.cap) return *(const rcx_u32x4_u*)(s.out + src);
    if (src + 16 <= 0) return *(const rcx_u32x4_u*)(dict + ((int64_t)D + src));
    uint32_t t4[4] = {0, 0, 0, 0};                                         // straddles position 0 (or the slot's last bytes)
    for (int i = 0; i < 16; i++) {
        const int64_t p = src + i;
        uint32_t x = 0;
        if (p < 0) x = dict[(int64_t)D + p];
        else if ((uint64_t)p < s.end) x = s.out[p];
        t4[i >> 2] |= x << (8 * (i & 3));
    }
    return rcx_u32x4{t4[0], t4[1], t4[2], t4[3]};
}

// f2_codes (Decoder::codes, flate.rs:262-341) with the dictionary behind position 0
__device__ int f2d_codes(F2& s, const F2Huff& HL, const F2Huff& HD, const uint8_t* dict, uint32_t D)
{
    uint32_t pend = 0, dd = 0, w = 0;          // pending bytes of the current symbol; dd == 0: the literal in w
    rcx_u32x4 g = {0, 0, 0, 0};                // far-match gather buffer
    uint32_t gpos = 16;
    for (;;) {
        if (pend) {                                                        // :289 / :320-334
            const uint32_t k = pend < 4 ? pend : 4;
            uint32_t w4;
            if (dd == 0) w4 = w;
            else if (dd < F2_NEAR) {                                       // ring source; bytes repeat with period dd < 4
                const uint32_t i1 = dd > 1 ? 1u : 0u;
                const uint32_t i2 = dd > 2 ? 2u : 0u;
                const uint32_t i3 = dd > 3 ? 3u : (dd == 2 ? 1u : 0u);
                const uint64_t sp = s.end - dd;                            // (below 0: wraps, the same ring byte)
                const uint32_t b0 = *s.RB(sp), b1 = *s.RB(sp + i1), b2 = *s.RB(sp + i2), b3 = *s.RB(sp + i3);
                w4 = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            } else {                                                       // drained source or dictionary: 16-byte gather, 4 bytes a step
                if (gpos >= 16) { g = f2d_gather(s, dict, D, (int64_t)s.end - (int64_t)dd); gpos = 0; }
                w4 = gpos == 0 ? g[0] : gpos == 4 ? g[1] : gpos == 8 ? g[2] : g[3];
                gpos += 4;
            }
            const uint64_t e0 = s.end;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if ((uint32_t)u < k) { const uint32_t x = (w4 >> (8 * u)) & 0xffu; *s.RB(e0 + u) = (uint8_t)x; s.a += x; s.b += s.a; }
            }
            s.end = e0 + k; pend -= k;
            s.pend += k;
            if (s.pend >= 5548) { s.a %= 65521u; s.b %= 65521u; s.pend = 0; }
            const uint64_t al = s.end - (((uintptr_t)(s.out + s.end)) & 15u);   // last 16-byte boundary at or below end
            if (al > s.flushed && al <= s.end) s.drain(al);
        }
        if (pend) continue;
        uint32_t sym, x;
        int st = s.decode<0>(HL, sym);                                     // :287
        if (st) return st;
        if (sym < 256) {                                                   // :289
            if (s.end >= s.cap) return RCX_E_OUTPUT_TOO_SMALL;
            w = sym; dd = 0; pend = 1;
        } else if (sym == 256) {
            return RCX_OK;                                                 // :290
        } else if (sym < 290) {
            const uint32_t nn = sym - 257;
            if (nn > 29) return RCX_E_INVALID_HUFFMAN_CODE;                // :294 (off by one)
            if (nn == 29) return RCX_E_MALFORMED;                          // :297 index panic
            const uint32_t lb = nn < 8 ? 0u : (nn == 28 ? 0u : (nn - 4u) >> 2);
            const uint32_t lbase = nn < 8 ? 3u + nn : (nn == 28 ? 258u : 3u + ((4u + (nn & 3u)) << lb));
            st = s.bits(lb, x);
            if (st) return st;
            const uint32_t len = lbase + x;
            uint32_t d;
            st = s.decode<1>(HD, d);                                       // :302
            if (st) return st;
            if (d >= 30) return RCX_E_MALFORMED;
            const uint32_t db = d < 4 ? 0u : (d - 2u) >> 1;
            const uint32_t dbase = d < 4 ? 1u + d : 1u + ((2u + (d & 1u)) << db);
            st = s.bits(db, x);
            if (st) return st;
            const uint32_t dist = dbase + x;
            const uint64_t have = s.end + D;                               // output.len(), :314, the dictionary counted in
            if (dist > (have < 32768u ? have : 32768u)) return RCX_E_INVALID_HUFFMAN_CODE;
            if (len > s.cap - s.end) return RCX_E_OUTPUT_TOO_SMALL;
            pend = len; dd = dist; gpos = 16;
            if (dist >= F2_NEAR) {                                         // start the first gather now: its latency
                g = f2d_gather(s, dict, D, (int64_t)s.end - (int64_t)dist);   // overlaps the other lanes' work
                gpos = 0;
            }
        } else {
            return RCX_E_INVALID_HUFFMAN_CODE;                             // :336
        }
    }
}

// f2_fixed
__device__ int f2d_fixed(F2& s, F2Huff& HL, F2Huff& HD, uint8_t* lens, const uint8_t* dict, uint32_t D)
{
    for (unsigned i = 0; i < 144; i++) lens[i] = 8;
    for (unsigned i = 144; i < 256; i++) lens[i] = 9;
    for (unsigned i = 256; i < 280; i++) lens[i] = 7;
    for (unsigned i = 280; i < 288; i++) lens[i] = 8;
    bool e;
    s.construct<0>(HL, lens, 288, e);
    for (unsigned i = 0; i < 30; i++) lens[i] = 5;
    s.construct<1>(HD, lens, 30, e);
    return f2d_codes(s, HL, HD, dict, D);
}

// f2_dynamic (Decoder::dynamic, flate.rs:397-450)
__device__ int f2d_dynamic(F2& s, F2Huff& HL, F2Huff& HD, uint8_t* lens, const uint8_t* dict, uint32_t D)
{
    uint32_t x;
    int st;
    if ((st = s.bits(5, x))) return st;
    const uint32_t hlit = x + 257;
    if ((st = s.bits(5, x))) return st;
    const uint32_t hdist = x + 1;
    if ((st = s.bits(4, x))) return st;
    const uint32_t hclen = x + 4;
    if (hlit > 286 || hdist > 30) return RCX_E_HUFFMAN_TREE_TOO_LARGE;     // :401
    for (unsigned i = 0; i < 19; i++) lens[i] = 0;
    for (unsigned i = 0; i < hclen; i++) {                                 // :412-414
        if ((st = s.bits(3, x))) return st;
        lens[F2_ORDER[i]] = (uint8_t)x;
    }
    bool e;
    if ((st = s.construct<1>(HD, lens, 19, e))) return st;                 // code-length code in the dist slots, :415
    for (unsigned i = 0; i < 320; i++) lens[i] = 0;                        // :419
    uint32_t i = 0;
    while (i < hlit + hdist) {                                             // :421-441
        uint32_t symbol;
        if ((st = s.decode<1>(HD, symbol))) return st;
        if (symbol < 16) {
            lens[i++] = (uint8_t)symbol;
        } else if (symbol == 16) {
            if (i == 0) return RCX_E_INVALID_HUFFMAN_HEADER_SYMBOL;        // :428
            const uint8_t prev = lens[i - 1];
            if ((st = s.bits(2, x))) return st;
            const uint32_t rep = x + 3;
            for (uint32_t k = 0; k < rep; k++) {
                if (i >= 316) return RCX_E_MALFORMED;                      // :432 index panic
                lens[i++] = prev;
            }
        } else if (symbol == 17) {
            if ((st = s.bits(3, x))) return st;
            i += x + 3;
        } else if (symbol == 18) {
            if ((st = s.bits(7, x))) return st;
            i += x + 11;
        } else {
            return RCX_E_INVALID_HUFFMAN_HEADER_SYMBOL;                    // :439
        }
    }
    if (i > hlit + hdist) return RCX_E_INVALID_HUFFMAN_TREE_HEADER;        // :442
    if ((st = s.construct<0>(HL, lens, hlit, e))) return st;               // :445-446
    if ((st = s.construct<1>(HD, lens + hlit, hdist, e))) return st;       // :447-448
    return f2d_codes(s, HL, HD, dict, D);
}

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
        else if (x == 1) st = f2d_fixed(s, HL, HD, lens, dict, D);
        else if (x == 2) st = f2d_dynamic(s, HL, HD, lens, dict, D);
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

// k.aux: the words of rcx_plan_dict, never null.  Streams per wave as launch_inflate_hist chooses them.
static void launch_inflate_dict(hipStream_t s, rcx_kargs& k, bool zlib)
{
    const uint32_t n = k.nblocks;
    const int z = zlib ? 1 : 0;
    if (n >= 32u * 2048u) hipLaunchKernelGGL((k_inflate_dict<32, 5, 1>), dim3((n + 31) / 32), dim3(32), 0, s, k, z);
    else if (n >= 16u * 2048u) hipLaunchKernelGGL((k_inflate_dict<16, 4, 1>), dim3((n + 15) / 16), dim3(16), 0, s, k, z);
    else hipLaunchKernelGGL((k_inflate_dict<8, 3, 1>), dim3((n + 7) / 8), dim3(8), 0, s, k, z);
}
