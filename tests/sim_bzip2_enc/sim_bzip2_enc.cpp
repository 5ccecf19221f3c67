// sim_bzip2_enc.cpp -- runs the UNMODIFIED bzip2 encoder (k_bzip2_enc.hip: kernels and launch loop, the host's plan) and the suffix sorter
// it calls (k_bwt.hip, k_bwt_sort.hip) on the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_bzip2_enc_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_bzip2_enc/sim_bzip2_enc.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#define hipStream_t int
typedef int hipError_t;
static const int hipSuccess = 0, hipMemcpyDeviceToHost = 2, hipMemcpyHostToDevice = 1, hipHostMallocDefault = 0;
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
static inline int hipMemcpyAsync(void* d, const void* s, size_t n, int, int) { memcpy(d, s, n); return 0; }
static inline int hipStreamSynchronize(int) { return 0; }
static inline const char* hipGetErrorString(int) { return "hip error"; }
static inline int hipGetLastError() { return 0; }
static inline int hipHostMalloc(void** p, size_t n, int) { *p = malloc(n); return *p ? 0 : 1; }
#include <chrono>
#include <map>
static uint32_t g_launches = 0;
static std::map<std::string, double> g_seconds;          // per kernel, printed when SIM_BZ2_TIMES is set: where a slow test spends its time
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { g_launches++; const auto t0_ = std::chrono::steady_clock::now(); ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); \
         g_seconds[#kern] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); } while (0)
#include "../../rust_compress_amd/csrc/k_bwt.hip"
int rcx_tu_bwt_forward(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool sa_words) { return launch_bwt_forward(s, k, variant, err, sa_words); }
uint64_t rcx_tu_bwt_forward_scratch(uint32_t nblocks, uint64_t max_block) { return bwt_forward_scratch_bytes(nblocks, max_block); }
#include "../../rust_compress_amd/csrc/k_bzip2_enc.hip"

static std::vector<uint8_t> g_scratch[3];
static uint64_t g_scratch_peak = 0;
// the record of a call, through the launch loop's watcher: every block's stages, copied while its round's scratch still holds them
struct BlockRec { rcx_bz2e_block b; rcx_bz2e_hdr h; std::vector<uint8_t> T, L, lens, sel; std::vector<uint16_t> syms; };
struct Trace { std::vector<BlockRec> blocks; uint32_t rounds = 0; };
static Trace g_trace;
static const rcx_bz2e_watch g_watch = {
    nullptr,
    [](void*, uint32_t, const rcx_bz2e_block* b, const uint8_t* T, const uint8_t* L, const rcx_bz2e_hdr* h, const uint16_t* syms, const uint8_t* lens,
       const uint8_t* sel) {
        BlockRec r;
        r.b = *b; r.h = *h;
        r.T.assign(T, T + 2 * (size_t)b->n); r.L.assign(L, L + b->n); r.syms.assign(syms, syms + h->nmtf);
        r.lens.assign(lens, lens + 6 * 258); r.sel.assign(sel, sel + h->nsel);
        g_trace.blocks.push_back(r);
    },
    [](void*) { g_trace.rounds++; }};
static void* sim_get(void*, int which, uint64_t bytes)
{
    // (a fresh buffer of 0xA5 at an odd address each time: nothing may rely on what an earlier one held, or on zeros)
    std::vector<uint8_t>().swap(g_scratch[which]);
    g_scratch[which].assign(bytes + 1, 0xA5);
    g_scratch_peak = std::max<uint64_t>(g_scratch_peak, g_scratch[0].size() + g_scratch[1].size() + g_scratch[2].size());
    return g_scratch[which].data() + 1;
}

// One rcx_bzip2_encode_batch of n files, as the library's batch path runs it, but for the chunk size, which a test may choose.
// info: launches, rounds, blocks, the scratch's peak in bytes.
extern "C" int sim_bzip2_encode(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t n, int level, uint32_t chunk,
                                uint32_t round, uint64_t* info, char* errbuf, uint32_t errcap)
{
    std::string err;
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n;
    const rcx_bz2_alloc alloc = {sim_get, nullptr};
    g_launches = 0; g_scratch_peak = 0;
    g_trace = Trace();
    const int rc = launch_bzip2_encode(0, k, in_off, in_len, out_off, out_cap, alloc, level, chunk, round, err, &g_watch);
    for (auto& b : g_scratch) std::vector<uint8_t>().swap(b);
    if (getenv("SIM_BZ2_TIMES")) { for (const auto& kv : g_seconds) fprintf(stderr, "%9.3f s  %s\n", kv.second, kv.first.c_str()); g_seconds.clear(); }
    if (rc && errbuf && errcap) { strncpy(errbuf, err.c_str(), errcap - 1); errbuf[errcap - 1] = 0; }
    info[0] = g_launches; info[1] = g_trace.rounds; info[2] = g_trace.blocks.size(); info[3] = g_scratch_peak;
    return rc;
}
// the record of the last call.  sizes: per block (file, off, len, n, nmtf, nsel, ngroups, alpha, orig, crc, bits, head_bits)
extern "C" void sim_bzip2_enc_sizes(uint64_t* sizes)
{
    for (size_t i = 0; i < g_trace.blocks.size(); i++) {
        const BlockRec& r = g_trace.blocks[i];
        uint64_t* s = sizes + 12 * i;
        s[0] = r.b.file; s[1] = r.b.off; s[2] = r.b.len; s[3] = r.b.n; s[4] = r.h.nmtf; s[5] = r.h.nsel; s[6] = r.h.ngroups; s[7] = r.h.alpha;
        s[8] = r.h.orig; s[9] = r.h.crc; s[10] = r.h.bits; s[11] = r.h.head_bits;
    }
}
// block i's stage arrays: T || T (2n bytes), L (n), the symbols (nmtf 16-bit words), the lengths (6 x 258), the selectors (nsel), the used map (32 bytes)
extern "C" void sim_bzip2_enc_block(uint32_t i, uint8_t* tt, uint8_t* l, uint16_t* syms, uint8_t* lens, uint8_t* sel, uint32_t* used)
{
    const BlockRec& r = g_trace.blocks[i];
    memcpy(tt, r.T.data(), r.T.size()); memcpy(l, r.L.data(), r.L.size()); memcpy(syms, r.syms.data(), r.syms.size() * 2);
    memcpy(lens, r.lens.data(), r.lens.size()); memcpy(sel, r.sel.data(), r.sel.size()); memcpy(used, r.h.used, 32);
}
