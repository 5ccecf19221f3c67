// k_lz4_hc_hist.hip -- the LZ4 HC block encoder of k_lz4_hc.hip with HISTORY: block b's matches may also reach into the hist[b] bytes
// (at most 65535) that lie directly before its first byte in the input buffer -- the previous block of a linked frame, or a dictionary.
// Included behind k_lz4_hc.hip (one translation unit): the plan, parse, scan and place kernels are that file's, launched unchanged.
//
// The match finder works on the block's VIRTUAL block, the history followed by the block: LzcSeg::in points at the first history byte,
// positions and len are shifted by hist, a segment of the block proper starts at hist + k * HC_SEG.  HcMatch::maxl measures from the END
// and the chains never lead below position 0, so lzc_links and lzc_search run as written: the window fill of the first segment starts at
// the first history byte, and no byte in front of the history is ever read.  cand is indexed by the position in the segment, as before;
// it may now hold a distance larger than the position, which the parse, scan and place kernels never compare with anything (they copy
// it into the token) -- so they see the segment geometry they always saw, and k_hc_place reads its literals from the block itself.
//
// The history needs chain links of its own (the search walks link[p - distance] through it): one links-only pass per block with
// history, lzc_links over [0, hist) as a segment that is never searched, parsed or placed.  Its 16-bit links take one more HC_SEG of
// the link array per such block, directly in front of the block's own: block b's links start at segment f0 + hslot[b] of the link
// array, hslot[b] = the blocks with history before b (a second scan of the plan kernel), and virtual position 0 lies hist entries before
// the block's first link.  The chains of the history are rebuilt for every block that names it: twice the links work for linked
// 64 KiB blocks, 33 times for a 2 KiB record behind a 64 KiB dictionary.
//
// aux[b] = hist[b] (uint32), or aux == null for no history at all.  With every hist 0 the launches do what launch_lz4_hc's do.

struct HcHist {
    uint32_t* hslot;       // [n + 1]: blocks with history (and segments) before block b; [n] = all of them
    uint32_t cap;          // history slots the link array holds beyond d.cap segments
};

static inline uint64_t hc_hist_extra_bytes(uint32_t n, uint64_t nhist) { return hc_al(4ull * (n + 1)) + 256 + nhist * 2ull * HC_SEG; }
static inline uint64_t hc_hist_scratch_bytes(uint32_t n, uint64_t nsegs, uint64_t nhist) { return hc_scratch_bytes(n, nsegs) + hc_hist_extra_bytes(n, nhist); }

// hslot in front, then hc_carve's layout in what is left less the history slots: the link array is the carve's last, so the slots extend it
static inline HcScratch hc_hist_carve(void* scratch, uint64_t bytes, uint32_t n, uint32_t nhist, HcHist& h)
{
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 255u) & ~(uintptr_t)255u);
    h.hslot = (uint32_t*)p; p += hc_al(4ull * (n + 1));
    h.cap = nhist;
    const uint64_t used = (uint64_t)(p - (uint8_t*)scratch) + (uint64_t)nhist * 2ull * HC_SEG;
    return hc_carve(p, bytes > used ? bytes - used : 0, n);
}

__device__ __forceinline__ uint32_t hc_hist_of(const rcx_kargs& a, uint32_t b)
{
    const uint32_t h = a.aux ? a.aux[b] : 0u;
    return h > HC_WIN ? HC_WIN : h;                                       // (of 65536 bytes the first is out of every match's reach)
}
// does block b get a history pass and a slot: history, and segments to use it
__device__ __forceinline__ uint32_t hc_hist_slot(const rcx_kargs& a, uint32_t b)
{
    return hc_hist_of(a, b) && a.in_len[b] && hc_block_status(a, b) == RCX_OK ? 1u : 0u;
}

__global__ __launch_bounds__(1024) void k_hc_hist_plan(rcx_kargs a, HcHist h)
{
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_carry;
    lzc_plan(a.nblocks, h.hslot, s_ws, &s_carry, [&](uint32_t b) { return hc_hist_slot(a, b); });
}

// the virtual block of block b (first segment f0) and its links: s.in, s.len in virtual positions; s0, L are the caller's to set
__device__ __forceinline__ uint16_t* hc_hist_virtual(const HcScratch& d, const HcHist& h, LzcSeg& s, uint32_t hist)
{
    const uint32_t slot = h.hslot[s.b] < h.cap ? h.hslot[s.b] : h.cap;   // (never past the slots the scratch holds)
    s.in -= hist;
    s.len += hist;
    return d.link + ((uint64_t)s.f0 + slot + (hist ? 1u : 0u)) * HC_SEG - hist;
}
// a block's history is used when its slot and all its segments lie inside the scratch (the host sized it: always; a block that a smaller
// scratch covers in part gets RCX_E_MALFORMED from k_hc_scan, and no history before that)
__device__ __forceinline__ uint32_t hc_hist_usable(const rcx_kargs& a, const HcScratch& d, const HcHist& h, uint32_t b)
{
    return hc_hist_slot(a, b) && h.hslot[b] < h.cap && d.seg_first[b + 1] <= d.cap ? hc_hist_of(a, b) : 0u;
}

// work items: the segments (as k_hc_links), then one per block: the links of its history, if it has one
__global__ __launch_bounds__(256) void k_hc_hist_links(rcx_kargs a, HcScratch d, HcHist h)
{
    __shared__ uint32_t s_head[1u << LZC_HBITS];
    __shared__ uint16_t s_hc[LZC_CHUNK];
    const uint32_t lim = hc_lim(a, d);
    const uint64_t items = (uint64_t)lim + (h.cap ? a.nblocks : 0u);
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        LzcSeg s;
        uint32_t hist;
        if (it < lim) {
            s = hc_seg(a, d, (uint32_t)it);
            hist = hc_hist_usable(a, d, h, s.b);
            s.s0 += hist;
        } else {
            const uint32_t b = (uint32_t)(it - lim);
            hist = hc_hist_usable(a, d, h, b);
            if (!hist) continue;                                           // (uniform: the whole workgroup moves on)
            s.b = b; s.f0 = d.seg_first[b];
            s.in = a.in_base + a.in_off[b];
            s.len = (uint32_t)a.in_len[b];
            s.s0 = 0; s.L = hist;
        }
        uint16_t* link = hc_hist_virtual(d, h, s, hist);
        lzc_links<HC_WIN>(s, link, s_head, s_hc);
    }
}

__global__ __launch_bounds__(256) RCX_SGPR_CAP void k_hc_hist_search(rcx_kargs a, HcScratch d, HcHist h, uint32_t depth)
{
    const uint32_t lim = hc_lim(a, d);
    for (uint32_t g = blockIdx.x; g < lim; g += gridDim.x) {
        LzcSeg s = hc_seg(a, d, g);
        const uint32_t hist = hc_hist_usable(a, d, h, s.b);
        s.s0 += hist;
        const uint16_t* link = hc_hist_virtual(d, h, s, hist);
        lzc_search<HcMatch>(s, link, d.cand + (uint64_t)g * HC_SEG, depth);
    }
}

// the whole encode on stream s at `level` (1..12); k.aux: the history lengths or null; k.scratch holds hc_hist_scratch_bytes(n, segments,
// nhist) bytes, nhist = the blocks with history
static int launch_lz4_hc_hist(hipStream_t s, rcx_kargs& k, int level, uint32_t nhist, std::string& err)
{
    const uint32_t n = k.nblocks;
    if (level < 1 || level > 12) { err = "lz4 hc: level must be 1..12"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < hc_hist_scratch_bytes(n, 0, nhist)) { err = "lz4 hc: scratch too small"; return RCX_RC_BAD_ARG; }
    HcHist h;
    const HcScratch d = hc_hist_carve(k.scratch, k.scratch_bytes, n, nhist, h);
    hipLaunchKernelGGL(k_hc_plan, dim3(1), dim3(1024), 0, s, k, d);
    hipLaunchKernelGGL(k_hc_hist_plan, dim3(1), dim3(1024), 0, s, k, h);
    if (d.cap) {
        const uint32_t gs = d.cap < 8192u ? d.cap : 8192u;
        const uint64_t items = (uint64_t)d.cap + (nhist ? n : 0u);
        hipLaunchKernelGGL(k_hc_hist_links, dim3(items < 8192u ? (uint32_t)items : 8192u), dim3(256), 0, s, k, d, h);
        hipLaunchKernelGGL(k_hc_hist_search, dim3(gs), dim3(256), 0, s, k, d, h, hc_depth(level));
        hipLaunchKernelGGL(k_hc_parse, dim3(gs), dim3(64), 0, s, k, d);
    }
    hipLaunchKernelGGL(k_hc_scan, dim3((n + 63) / 64), dim3(64), 0, s, k, d);
    if (d.cap) hipLaunchKernelGGL(k_hc_place, dim3(d.cap < 8192u ? d.cap : 8192u), dim3(256), 0, s, k, d);
    return RCX_RC_OK;
}
