// k_deflate_hc_hist.hip -- levels 2..9 of the DEFLATE / zlib encoder of k_deflate_hc.hip with HISTORY: block b's matches may also reach
// into the hist[b] bytes (at most 32768, DEFLATE's largest distance: all of them are within reach) that lie directly before its first
// byte in the input buffer -- a preset dictionary (RFC 1950 FDICT, zlib's deflateSetDictionary), or the 32 KiB in front of a chunk of
// one long stream.  Included behind k_deflate_hc.hip (one translation unit): the plan, checksum, price, parse, block, scan, place
// kernels are that file's and k_deflate_encode.hip's, launched unchanged on the unshifted segment geometry.
//
// NOT in the reference crate (it has no DEFLATE encoder): an extension, checked by libz (zdict=) and this library's own
// k_inflate_hist.hip.
//
// The match finder works on the block's VIRTUAL block, the history followed by the block, exactly as k_lz4_hc_hist.hip does: LzcSeg::in
// points at the first history byte, positions and len are shifted by hist, a segment of the block proper starts at hist + k * DE_SEG.
// DhMatch::maxl measures from the segment's END and the chains never lead below position 0, so lzc_links and lzc_search run as written
// and no byte in front of the history is ever read.  cand is indexed by the position in the segment, as before; it may now hold a
// distance larger than the position, which k_dh_price, k_dh_parse and dh_block never compare with anything (they copy it into the
// token), and dh_block and k_de_place read literals from the block itself.
//
// The history needs chain links of its own: one links-only work item per block with history, lzc_links over [0, hist) as a segment that
// is never searched, parsed or placed.  Its 16-bit links take one more DE_SEG of the link array per such block (half of it at the most
// is used), directly in front of the block's own: block b's links start at segment f0 + hslot[b] of the link array, hslot[b] = the
// blocks with history before b (k_dh_hist_plan), and virtual position 0 lies hist entries before the block's first link.  The chains of
// a history are rebuilt for every block that names it.
//
// aux[b] = hist[b] (uint32), aux[n + b] = the stream's DICTID (zlib form only).  With every hist 0 the launches do what
// launch_deflate_level's do.

struct DhHist {
    uint32_t* hslot;       // [n + 1]: blocks with history before block b; [n] = all of them
    uint32_t cap;          // history slots the link array holds beyond d.cap segments
};

static inline uint64_t dh_hist_extra_bytes(uint32_t n, uint64_t nhist) { return de_al(4ull * (n + 1)) + 512 + nhist * 2ull * DE_SEG; }
static inline uint64_t dh_hist_scratch_bytes(uint32_t n, uint64_t nsegs, uint64_t nhist) { return dh_scratch_bytes(n, nsegs) + dh_hist_extra_bytes(n, nhist); }

// hslot in front, then dh_carve's arrays in what is left less the history slots, with the link array LAST (dh_carve has it first): the
// slots extend it
static inline DeScratch dh_hist_carve(void* scratch, uint64_t bytes, uint32_t n, uint32_t nhist, DhScratch& h, DhHist& hh)
{
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 255u) & ~(uintptr_t)255u);
    hh.hslot = (uint32_t*)p; p += de_al(4ull * (n + 1));
    hh.cap = nhist;
    const uint64_t used = (uint64_t)(p - (uint8_t*)scratch) + 256 + (uint64_t)nhist * 2ull * DE_SEG;
    const uint64_t left = bytes > used ? bytes - used : 0;
    const uint64_t fixed = dh_scratch_bytes(n, 0);
    uint64_t cap = left > fixed ? (left - fixed) / (de_seg_bytes() + dh_seg_bytes()) : 0;
    if (cap > 0xffffffffull) cap = 0xffffffffull;
    const uint64_t de = de_scratch_bytes(n, cap);
    const DeScratch d = de_carve(p, de, n);                   // (d.cap == cap, as in dh_carve)
    uint8_t* q = (uint8_t*)(((uintptr_t)p + de + 255u) & ~(uintptr_t)255u);
    h.cand = (uint32_t*)q; q += de_al(4ull * DE_SEG * cap);
    h.elen = (uint32_t*)q; q += de_al(4ull * DH_ELEN * cap);
    h.price = q; q += de_al(320ull * cap);
    h.link = (uint16_t*)q;                                    // [(cap + nhist) * DE_SEG]
    return d;
}

__device__ __forceinline__ uint32_t dh_hist_of(const rcx_kargs& a, uint32_t b)
{
    const uint32_t h = a.aux ? a.aux[b] : 0u;
    return h > DE_WIN ? DE_WIN : h;
}
// does block b get a history pass and a slot: history, and segments to use it
__device__ __forceinline__ uint32_t dh_hist_slot(const rcx_kargs& a, uint32_t b)
{
    return dh_hist_of(a, b) && de_nseg(a.in_len[b]) ? 1u : 0u;
}

__global__ __launch_bounds__(1024) void k_dh_hist_plan(rcx_kargs a, DhHist hh)
{
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_carry;
    lzc_plan(a.nblocks, hh.hslot, s_ws, &s_carry, [&](uint32_t b) { return dh_hist_slot(a, b); });
}

// the virtual block of block s.b (first segment s.f0) and its links: s.in, s.len in virtual positions; s0, L are the caller's to set
__device__ __forceinline__ uint16_t* dh_hist_virtual(const DhScratch& h, const DhHist& hh, LzcSeg& s, uint32_t hist)
{
    const uint32_t slot = hh.hslot[s.b] < hh.cap ? hh.hslot[s.b] : hh.cap;   // (never past the slots the scratch holds)
    s.in -= hist;
    s.len += hist;
    return h.link + ((uint64_t)s.f0 + slot + (hist ? 1u : 0u)) * DE_SEG - hist;
}
// a block's history is used when its slot and all its segments lie inside the scratch (the host sized it: always; a block that a smaller
// scratch covers in part gets RCX_E_MALFORMED from k_de_scan, and no history before that)
__device__ __forceinline__ uint32_t dh_hist_usable(const rcx_kargs& a, const DeScratch& d, const DhHist& hh, uint32_t b)
{
    return dh_hist_slot(a, b) && hh.hslot[b] < hh.cap && d.seg_first[b + 1] <= d.cap ? dh_hist_of(a, b) : 0u;
}

// work items: the segments (as k_dh_links), then one per block: the links of its history, if it has one
__global__ __launch_bounds__(256) void k_dh_hist_links(rcx_kargs a, DeScratch d, DhScratch h, DhHist hh)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = de_lim(a, d);
    const uint64_t items = (uint64_t)lim + (hh.cap ? a.nblocks : 0u);
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        LzcSeg s;
        uint32_t hist;
        if (it < lim) {
            s = de_seg(a, d, (uint32_t)it);
            hist = dh_hist_usable(a, d, hh, s.b);
            s.s0 += hist;
        } else {
            const uint32_t b = (uint32_t)(it - lim);
            hist = dh_hist_usable(a, d, hh, b);
            if (!hist) continue;                                           // (uniform: the whole workgroup moves on)
            s.b = b; s.f0 = d.seg_first[b];
            s.in = a.in_base + a.in_off[b];
            s.len = (uint32_t)a.in_len[b];
            s.s0 = 0; s.L = hist;
        }
        uint16_t* link = dh_hist_virtual(h, hh, s, hist);
        lzc_links<DE_WIN>(s, link, s_head, s_hc);
    }
}

__global__ __launch_bounds__(256) RCX_SGPR_CAP void k_dh_hist_search(rcx_kargs a, DeScratch d, DhScratch h, DhHist hh, uint32_t depth)
{
    const uint32_t lim = de_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        LzcSeg s = de_seg(a, d, g);
        const uint32_t hist = dh_hist_usable(a, d, hh, s.b);
        s.s0 += hist;
        const uint16_t* link = dh_hist_virtual(h, hh, s, hist);
        lzc_search<DhMatch>(s, link, h.cand + (uint64_t)g * DE_SEG, depth);
    }
}

// the header of every zlib stream k_de_scan<DE_ZDICT> passed: FLEVEL of the level as k_dh_head writes it; with a history FDICT, FCHECK
// recomputed and the caller's DICTID (aux[n + b]) big-endian behind it
__global__ __launch_bounds__(256) void k_dh_hist_head(rcx_kargs a, uint32_t level)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks || a.status[b] != RCX_OK) return;
    uint8_t* o = a.out_base + a.out_off[b];
    if (!a.aux[b]) { o[1] = level <= 5 ? 0x5e : level == 6 ? 0x9c : 0xda; return; }
    const uint32_t flg = ((level <= 5 ? 1u : level == 6 ? 2u : 3u) << 6) | 0x20u;
    o[1] = (uint8_t)(flg + 31u - (0x7800u + flg) % 31u);                   // (0x7800 + flg is no multiple of 31 for these three)
    const uint32_t id = a.aux[a.nblocks + b];
    o[2] = (uint8_t)(id >> 24); o[3] = (uint8_t)(id >> 16); o[4] = (uint8_t)(id >> 8); o[5] = (uint8_t)id;
}

// the whole encode on stream s at `level` (2..9), fmt DE_RAW or DE_ZLIB; k.aux: the history lengths (then the DICTIDs: zlib) or null;
// k.scratch holds dh_hist_scratch_bytes(n, segments, nhist) bytes, nhist = the blocks with history
static int launch_deflate_hist(hipStream_t s, rcx_kargs& k, int fmt, int level, uint32_t nhist, std::string& err, void (*cks)(hipStream_t, rcx_kargs&))
{
    const uint32_t n = k.nblocks;
    if (level < 2 || level > 9) { err = "deflate encode with history: level must be 2..9"; return RCX_RC_BAD_ARG; }
    if (fmt != DE_RAW && fmt != DE_ZLIB) { err = "deflate encode with history: raw DEFLATE or zlib"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < dh_hist_scratch_bytes(n, 0, nhist)) { err = "deflate encode: scratch too small"; return RCX_RC_BAD_ARG; }
    DhScratch h;
    DhHist hh;
    const DeScratch d = dh_hist_carve(k.scratch, k.scratch_bytes, n, nhist, h, hh);
    const bool zdict = fmt == DE_ZLIB && k.aux;                // (without lengths every header is two bytes: the plain zlib form)
    hipLaunchKernelGGL(k_de_plan, dim3(1), dim3(1024), 0, s, k, d);
    hipLaunchKernelGGL(k_dh_hist_plan, dim3(1), dim3(1024), 0, s, k, hh);
    if (fmt != DE_RAW && d.cap) {
        hipLaunchKernelGGL(k_de_segs, dim3(d.cap < 65536u * 4u ? (d.cap + 255) / 256 : 1024u), dim3(256), 0, s, k, d);
        rcx_kargs kc = k;                                 // a wave per segment: the block's bytes alone
        kc.in_off = d.seg_ioff; kc.in_len = d.seg_ilen; kc.nblocks = d.cap;
        kc.out_len = nullptr; kc.in_used = nullptr; kc.status = nullptr; kc.aux = d.seg_cks;
        cks(s, kc);
    }
    if (d.cap) {
        const dim3 gs(d.cap < 8192u ? d.cap : 8192u);
        const uint64_t items = (uint64_t)d.cap + (nhist ? n : 0u);
        hipLaunchKernelGGL(k_dh_hist_links, dim3(items < 8192u ? (uint32_t)items : 8192u), dim3(256), 0, s, k, d, h, hh);
        hipLaunchKernelGGL(k_dh_hist_search, gs, dim3(256), 0, s, k, d, h, hh, dh_depth(level));
        for (uint32_t it = 0; it < (level >= DH_ITER ? 2u : 1u); it++) {
            hipLaunchKernelGGL(k_dh_price, gs, dim3(DE_T), 0, s, k, d, h, it);
            hipLaunchKernelGGL(k_dh_parse, gs, dim3(64), 0, s, k, d, h);
        }
        hipLaunchKernelGGL(k_dh_block, dim3(d.cap < 2048u ? d.cap : 2048u), dim3(DE_T), 0, s, k, d);
    }
    const dim3 gs((n + 3) / 4), gp(d.cap < 4096u ? d.cap : 4096u), gh((n + 255) / 256);
    if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_scan<DE_RAW>, gs, dim3(256), 0, s, k, d);
    else if (zdict) hipLaunchKernelGGL(k_de_scan<DE_ZDICT>, gs, dim3(256), 0, s, k, d);
    else hipLaunchKernelGGL(k_de_scan<DE_ZLIB>, gs, dim3(256), 0, s, k, d);
    if (d.cap) {
        if (fmt == DE_RAW) hipLaunchKernelGGL(k_de_place<DE_RAW>, gp, dim3(256), 0, s, k, d);
        else if (zdict) hipLaunchKernelGGL(k_de_place<DE_ZDICT>, gp, dim3(256), 0, s, k, d);
        else hipLaunchKernelGGL(k_de_place<DE_ZLIB>, gp, dim3(256), 0, s, k, d);
    }
    if (zdict) hipLaunchKernelGGL(k_dh_hist_head, gh, dim3(256), 0, s, k, (uint32_t)level);
    else if (fmt == DE_ZLIB) hipLaunchKernelGGL(k_dh_head<DE_ZLIB>, gh, dim3(256), 0, s, k, (uint32_t)level);
    return RCX_RC_OK;
}
