// sim_bzip2.cpp -- runs the UNMODIFIED bzip2 decoder (k_bzip2.hip: kernels and launch loop, the host's rcx_plan_bz2_chain) and the inverse
// BWT it calls (k_bwt_inverse.hip) on the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_bzip2_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_bzip2/sim_bzip2.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#define hipStream_t int
typedef int hipError_t;
static const int hipSuccess = 0, hipMemcpyDeviceToHost = 2, hipMemcpyHostToDevice = 1;
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
static inline int hipMemcpyAsync(void* d, const void* s, size_t n, int, int) { memcpy(d, s, n); return 0; }
static inline int hipStreamSynchronize(int) { return 0; }
static inline const char* hipGetErrorString(int) { return "hip error"; }
static inline int hipGetLastError() { return 0; }
#include <chrono>
#include <map>
static uint32_t g_launches = 0;
static std::map<std::string, double> g_seconds;          // per kernel, printed when SIM_BZ2_TIMES is set: where a slow test spends its time
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { g_launches++; const auto t0_ = std::chrono::steady_clock::now(); ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); \
         g_seconds[#kern] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); } while (0)
#include "../../rust_compress_amd/csrc/k_bwt_inverse.hip"
int rcx_tu_bwt_inverse(hipStream_t s, rcx_kargs& k, int variant, std::string& err, bool minimal) { return launch_bwt_inverse(s, k, variant, err, minimal); }
uint64_t rcx_tu_bwt_inverse_scratch(uint32_t nblocks, uint64_t max_block) { return bwt_inverse_scratch_bytes(nblocks, max_block); }
#include "../../rust_compress_amd/csrc/k_bzip2.hip"

static std::vector<uint8_t> g_scratch[2];
static uint64_t g_scratch_peak = 0;
// the record of a call, through the launch loop's watcher: every candidate with its file, the accepted blocks, the rounds
struct Trace { std::vector<rcx_bz2_cand> cands; std::vector<uint32_t> cand_file; std::vector<uint64_t> live_file, live_bit; uint32_t rounds = 0; };
static Trace g_trace;
static const rcx_bz2_watch g_watch = {
    nullptr,
    [](void*, uint32_t file, const rcx_bz2_cand* c) { g_trace.cands.push_back(*c); g_trace.cand_file.push_back(file); },
    [](void*, uint32_t file, uint64_t bit) { g_trace.live_file.push_back(file); g_trace.live_bit.push_back(bit); },
    [](void*) { g_trace.rounds++; }};
static void* sim_get(void*, int which, uint64_t bytes)
{
    // (a fresh buffer of 0xA5 at an odd address each time: nothing may rely on what an earlier one held, or on zeros)
    std::vector<uint8_t>().swap(g_scratch[which]);
    g_scratch[which].assign(bytes + 1, 0xA5);
    g_scratch_peak = std::max<uint64_t>(g_scratch_peak, g_scratch[0].size() + g_scratch[1].size());
    return g_scratch[which].data() + 1;
}

// One rcx_bzip2_decode_batch of n files, as the library's batch path runs it.  info: launches, rounds, candidates, live blocks, the scratch's peak in bytes.
extern "C" int sim_bzip2_decode(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t n, uint32_t round, uint64_t* info,
                                char* errbuf, uint32_t errcap)
{
    std::string err;
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n;
    const rcx_bz2_alloc alloc = {sim_get, nullptr};
    g_launches = 0; g_scratch_peak = 0;
    g_trace = Trace();
    const int rc = launch_bzip2_decode(0, k, in_len, out_off, out_cap, alloc, round, err, &g_watch);
    std::vector<uint8_t>().swap(g_scratch[0]); std::vector<uint8_t>().swap(g_scratch[1]);
    if (getenv("SIM_BZ2_TIMES")) { for (const auto& kv : g_seconds) fprintf(stderr, "%9.3f s  %s\n", kv.second, kv.first.c_str()); g_seconds.clear(); }
    if (rc && errbuf && errcap) { strncpy(errbuf, err.c_str(), errcap - 1); errbuf[errcap - 1] = 0; }
    info[0] = g_launches; info[1] = g_trace.rounds; info[2] = g_trace.cands.size(); info[3] = g_trace.live_bit.size(); info[4] = g_scratch_peak;
    return rc;
}
// the record of the last call: the candidates (file, bit, kind, extra as four 64-bit words each) and the live blocks (file, bit)
extern "C" void sim_bzip2_trace(uint64_t* cands, uint64_t* live)
{
    for (size_t i = 0; i < g_trace.cands.size(); i++) {
        cands[4 * i] = g_trace.cand_file[i]; cands[4 * i + 1] = g_trace.cands[i].bit; cands[4 * i + 2] = g_trace.cands[i].kind; cands[4 * i + 3] = g_trace.cands[i].extra;
    }
    for (size_t i = 0; i < g_trace.live_bit.size(); i++) { live[2 * i] = g_trace.live_file[i]; live[2 * i + 1] = g_trace.live_bit[i]; }
}
