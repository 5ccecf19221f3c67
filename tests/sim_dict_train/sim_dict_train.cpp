// sim_dict_train.cpp -- runs the UNMODIFIED dictionary trainer (k_dict_train.hip: kernels and launch loop) and the host's rcx_plan_train on
// the wave64 simulator of tests/wavesim (TEST INFRASTRUCTURE).  Built by tests/sim_dict_train_run.py with
//   g++ -include tests/wavesim/wavesim.h tests/sim_dict_train/sim_dict_train.cpp tests/wavesim/wavesim.cpp
#include <string>
#include <vector>
#define hipStream_t int
typedef int hipError_t;
static const int hipSuccess = 0, hipMemcpyDeviceToHost = 2;
static inline int hipMemsetAsync(void* d, int v, size_t n, int) { memset(d, v, n); return 0; }
static inline int hipMemcpyAsync(void* d, const void* s, size_t n, int, int) { memcpy(d, s, n); return 0; }
static inline int hipStreamSynchronize(int) { return 0; }
static inline const char* hipGetErrorString(int) { return "hip error"; }
static uint32_t g_launches = 0;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) \
    do { g_launches++; ws::launch(grid, block, [&] { kern(__VA_ARGS__); }); } while (0)
#include "../../rust_compress_amd/csrc/k_dict_train.hip"

// One rcx_dict_train_batch of n jobs, as the library's batch path runs it: the plan, a scratch of the plan's size filled with `fill` at
// an odd address, the launch loop.  rounds[i]: the rounds job i ran.  info: scratch bytes, launches, the plan's round bound, live jobs.
// -1: the plan refused (errbuf has the text).
extern "C" int sim_dict_train(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint32_t* nsamples,
                              const uint64_t* sample_len, uint32_t kk, uint32_t d, uint32_t f, uint8_t* out, const uint64_t* out_off,
                              const uint64_t* out_cap, uint64_t* out_len, uint64_t* in_used, int32_t* status, uint32_t* rounds, uint32_t n,
                              int fill, uint64_t* info, char* errbuf, uint32_t errcap)
{
    rcx_train_plan plan;
    std::string err;
    auto fail = [&](int rc) { if (errbuf && errcap) { strncpy(errbuf, err.c_str(), errcap - 1); errbuf[errcap - 1] = 0; } return rc; };
    if (!rcx_plan_train(n, in_len, out_cap, nsamples, sample_len, kk, d, f, plan, err)) return fail(-1);
    std::vector<uint8_t> scratch(plan.scratch_bytes + 64, (uint8_t)fill);
    rcx_kargs k;
    memset(&k, 0, sizeof k);
    k.in_base = in; k.in_off = in_off; k.in_len = in_len; k.out_base = out; k.out_off = out_off; k.out_cap = out_cap;
    k.out_len = out_len; k.in_used = in_used; k.status = status; k.nblocks = n; k.aux = plan.aux.data();
    k.scratch = scratch.data() + 1; k.scratch_bytes = plan.scratch_bytes;
    g_launches = 0;
    const int rc = launch_dict_train(0, k, plan, err);
    if (rc) return fail(rc);
    for (uint32_t i = 0; i < n; i++) rounds[i] = plan.aux[i];
    info[0] = plan.scratch_bytes; info[1] = g_launches; info[2] = plan.max_rounds; info[3] = plan.live;
    return 0;
}
// the plan's arithmetic alone: in_len / out_cap may name sizes no buffer has
extern "C" int sim_dict_train_plan(const uint64_t* in_len, const uint64_t* out_cap, const uint32_t* nsamples, const uint64_t* sample_len,
                                   uint32_t kk, uint32_t d, uint32_t f, uint32_t n, char* errbuf, uint32_t errcap)
{
    rcx_train_plan plan;
    std::string err;
    const bool ok = rcx_plan_train(n, in_len, out_cap, nsamples, sample_len, kk, d, f, plan, err);
    if (!ok && errbuf && errcap) { strncpy(errbuf, err.c_str(), errcap - 1); errbuf[errcap - 1] = 0; }
    return ok ? 0 : -1;
}
