// k_dict_train.hip -- batched dictionary training (rcx_dict_train_batch): the hashed COVER selection of DESIGN.md 3.19, one job per
// corpus, the job index on gridDim.y.  Once per job: the hash word and validity of every position and the hash frequencies (k_dt_hash),
// the distance to the previous occurrence of a position's hash within a segment (k_dt_back).  Per round, for all live jobs at once:
// every position adds its frequency to the starts it counts for as a range (k_dt_add: two atomics on a difference array), a two-level
// prefix sum turns the differences into scores and keeps the best (k_dt_sums, k_dt_scanmax), and one workgroup per job trims, zeroes
// and copies the winner (k_dt_take).  No workgroup waits for another: every dependency is a launch boundary, every loop is bounded by
// the sizes.  All arithmetic is on integers, so the result does not depend on the order the atomics arrive in.
#pragma once
#include "rcx_dev.h"
#include "rcx_plan.h"

#define DT_THREADS 256u
#define DT_INVALID 0xffffffffu               /* the hash word of a position whose d-mer would leave its sample (f <= 22: never a hash) */
#define DT_GRID 512u                         /* workgroups a job at the most in the grid-strided launches (256 positions a sweep each) */
#define DT_BACK_TILE 2048u                   /* positions a workgroup resolves per LDS tile */
#define DT_BACK_GRID 64u
#define DT_MAX_HALO 4090u                    /* k - d at the most */
#define DT_SCAN_TILE 1024u                   /* 256 threads x 4 entries */
#define DT_FINISH_GRID 64u

struct DtArgs {
    const uint8_t* in_base; const uint64_t* in_off; const uint64_t* in_len;
    const uint64_t* out_cap; const uint32_t* aux;
    uint8_t* base;                           // the scratch, aligned to 256
    uint32_t njobs, k, d, f;
};
struct DtJob {
    const uint8_t* S; uint32_t n, cap, E, size, dead, nsamp;
    const uint32_t* ends;
    uint32_t* hash; uint16_t* back; uint32_t* freq; uint32_t* diff; uint8_t* stage;
    uint32_t* state; uint32_t* partial;
};
enum { DT_TAIL = 0, DT_ZERO = 1, DT_DONE = 2, DT_ROUNDS = 3, DT_BEST = 4 };

__device__ __forceinline__ DtJob dt_job(const DtArgs& a, uint32_t j)
{
    DtJob J;
    const uint32_t* h = a.aux + a.njobs + RCX_TRAIN_HDR * j;
    J.S = a.in_base + a.in_off[j]; J.n = (uint32_t)a.in_len[j]; J.cap = (uint32_t)a.out_cap[j];
    J.ends = a.aux + (size_t)a.njobs * (1 + RCX_TRAIN_HDR) + h[0]; J.nsamp = h[1]; J.E = h[2]; J.size = h[3]; J.dead = h[6];
    uint8_t* r = a.base + (((uint64_t)h[5] << 32) | h[4]);
    const rcx_train_carve c = rcx_train_job_carve(J.n, J.cap, J.size, a.f);
    J.hash = (uint32_t*)(r + c.hash); J.back = (uint16_t*)(r + c.back); J.freq = (uint32_t*)(r + c.freq);
    J.diff = (uint32_t*)(r + c.diff); J.stage = r + c.stage;
    J.state = (uint32_t*)(a.base + rcx_train_state_at(a.njobs)) + (size_t)RCX_TRAIN_STATE_WORDS * j;
    J.partial = (uint32_t*)(a.base + rcx_train_partial_at(a.njobs)) + (size_t)RCX_TRAIN_SCAN_BLOCKS * j;
    return J;
}
// the candidate starts of round r: [lo, hi), empty when hi <= lo (n >= k: a dead job never gets here)
__device__ __forceinline__ void dt_epoch(const DtJob& J, uint32_t k, uint64_t r, uint32_t& lo, uint32_t& hi)
{
    const uint64_t e = r % J.E, l = e * J.size, last = (uint64_t)J.n - k + 1;
    uint64_t h = (e + 1) * J.size;
    if (h > last) h = last;
    lo = (uint32_t)l; hi = h > l ? (uint32_t)h : (uint32_t)l;
}
// the scan launches' share of a job's len1 = hi - lo + 1 difference words: workgroup blk has [b0, b1)
__device__ __forceinline__ void dt_scan_range(uint32_t len1, uint32_t blk, uint32_t& b0, uint32_t& b1)
{
    const uint64_t chunk = (((uint64_t)len1 + RCX_TRAIN_SCAN_BLOCKS - 1) / RCX_TRAIN_SCAN_BLOCKS + DT_SCAN_TILE - 1) / DT_SCAN_TILE * DT_SCAN_TILE;
    const uint64_t x0 = chunk * blk, x1 = x0 + chunk;
    b0 = x0 < len1 ? (uint32_t)x0 : len1; b1 = x1 < len1 ? (uint32_t)x1 : len1;
}

// ---- once per call: the jobs' state, frequencies and differences start at zero ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt_clear(DtArgs a)
{
    const uint32_t j = blockIdx.y;
    const DtJob J = dt_job(a, j);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        J.state[DT_TAIL] = J.cap; J.state[DT_ZERO] = 0; J.state[DT_DONE] = J.dead ? 1u : 0u; J.state[DT_ROUNDS] = 0;
        J.state[DT_BEST] = 0; J.state[DT_BEST + 1] = 0;
        if (J.dead) atomicAdd((uint32_t*)a.base, 1u);
    }
    if (J.dead) return;
    const uint64_t nf = (uint64_t)1 << a.f, nd = (uint64_t)J.size + 1, step = (uint64_t)gridDim.x * DT_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DT_THREADS + threadIdx.x; i < nf; i += step) J.freq[i] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * DT_THREADS + threadIdx.x; i < nd; i += step) J.diff[i] = 0;
}

// ---- once per job: hash words and frequencies ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt_hash(DtArgs a)
{
    const DtJob J = dt_job(a, blockIdx.y);
    if (J.dead) return;
    const uint64_t step = (uint64_t)gridDim.x * DT_THREADS;
    for (uint64_t p = (uint64_t)blockIdx.x * DT_THREADS + threadIdx.x; p < J.n; p += step) {
        // the end of the sample that holds p: the first end beyond p (samples of length 0 repeat an end; the last end is n > p)
        uint32_t lo = 0, hi = J.nsamp;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (J.ends[mid] > p) hi = mid; else lo = mid + 1; }
        const uint64_t end = lo < J.nsamp ? J.ends[lo] : J.n;
        uint32_t w = DT_INVALID;
        if (p + a.d <= end) {
            const uint8_t* q = J.S + p;
            const uint64_t v = a.d == 8 ? *(const rcx_u64_u*)q
                                        : (uint64_t)*(const rcx_u32_u*)q | ((uint64_t)q[4] << 32) | ((uint64_t)q[5] << 40);
            w = (uint32_t)((v * 0x9E3779B185EBCA87ull) >> (64 - a.f));
            atomicAdd(&J.freq[w], 1u);
        }
        J.hash[p] = w;
    }
}

// ---- once per job: back(p), the distance to the nearest valid q < p with the same hash, if at most k - d (else 0) -----------------------
__global__ __launch_bounds__(256) void k_dt_back(DtArgs a)
{
    __shared__ uint32_t sh[DT_BACK_TILE + DT_MAX_HALO];
    const DtJob J = dt_job(a, blockIdx.y);
    if (J.dead) return;
    const uint32_t H = a.k - a.d;
    for (uint64_t t0 = (uint64_t)blockIdx.x * DT_BACK_TILE; t0 < J.n; t0 += (uint64_t)gridDim.x * DT_BACK_TILE) {
        for (uint32_t i = threadIdx.x; i < H + DT_BACK_TILE; i += DT_THREADS) {
            const uint64_t p = t0 + i;                                      // sh[i] is position t0 - H + i
            sh[i] = (p >= H && p - H < J.n) ? J.hash[p - H] : DT_INVALID;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < DT_BACK_TILE && t0 + i < J.n; i += DT_THREADS) {
            const uint32_t h = sh[H + i];
            uint32_t found = 0;
            if (h != DT_INVALID)
                for (uint32_t b = 1; b <= H; b++)
                    if (sh[H + i - b] == h) { found = b; break; }
            J.back[t0 + i] = (uint16_t)found;
        }
        __syncthreads();
    }
}

// ---- per round: the range of starts every position counts for -------------------------------------------------------------------------------
// A valid p with w = freq[h(p)] > 0 counts for the starts s in [lo, hi) with p - (k - d) <= s <= p whose segment holds no earlier
// occurrence of h(p): s > p - back(p).
__global__ __launch_bounds__(256) void k_dt_add(DtArgs a, uint64_t r)
{
    const DtJob J = dt_job(a, blockIdx.y);
    if (J.state[DT_DONE]) return;
    uint32_t lo, hi;
    dt_epoch(J, a.k, r, lo, hi);
    if (hi <= lo) return;
    const uint32_t H = a.k - a.d;
    const uint64_t pend = (uint64_t)hi - 1 + H;                             // <= n - d
    for (uint64_t p = (uint64_t)lo + (uint64_t)blockIdx.x * DT_THREADS + threadIdx.x; p <= pend; p += (uint64_t)gridDim.x * DT_THREADS) {
        const uint32_t h = J.hash[p];
        if (h == DT_INVALID) continue;
        const uint32_t w = J.freq[h];
        if (!w) continue;
        const uint32_t bk = J.back[p];
        uint64_t s0 = lo;
        if (p >= H && p - H > s0) s0 = p - H;
        if (bk && p - bk + 1 > s0) s0 = p - bk + 1;
        const uint64_t s1 = p < hi ? p : (uint64_t)hi - 1;
        if (s0 > s1) continue;
        atomicAdd(&J.diff[s0 - lo], w);
        atomicAdd(&J.diff[s1 + 1 - lo], 0u - w);
    }
}

// ---- per round: the sum of a workgroup's share of the differences ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt_sums(DtArgs a, uint64_t r)
{
    __shared__ uint32_t tot;
    const DtJob J = dt_job(a, blockIdx.y);
    if (J.state[DT_DONE]) return;
    uint32_t lo, hi, b0, b1;
    dt_epoch(J, a.k, r, lo, hi);
    dt_scan_range(hi > lo ? hi - lo + 1 : 0, blockIdx.x, b0, b1);
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    uint32_t s = 0;
    for (uint64_t i = (uint64_t)b0 + threadIdx.x; i < b1; i += DT_THREADS) s += J.diff[i];
    if (s) atomicAdd(&tot, s);
    __syncthreads();
    if (threadIdx.x == 0) J.partial[blockIdx.x] = tot;
}

// ---- per round: scores = the prefix sum of the differences; the greatest, lowest start first; the differences back to zero ---------------
__global__ __launch_bounds__(256) void k_dt_scanmax(DtArgs a, uint64_t r)
{
    __shared__ uint32_t carry, wsum[4];
    __shared__ unsigned long long top;
    const DtJob J = dt_job(a, blockIdx.y);
    if (J.state[DT_DONE]) return;
    uint32_t lo, hi, b0, b1;
    dt_epoch(J, a.k, r, lo, hi);
    const uint32_t len = hi > lo ? hi - lo : 0;                            // candidates; word `len` closes the last range
    dt_scan_range(len ? len + 1 : 0, blockIdx.x, b0, b1);
    if (b1 <= b0) return;
    if (threadIdx.x == 0) { carry = 0; top = 0; }
    __syncthreads();
    if (threadIdx.x < blockIdx.x) { const uint32_t v = J.partial[threadIdx.x]; if (v) atomicAdd(&carry, v); }     // (at most 128 workgroups)
    __syncthreads();
    uint32_t run = carry;
    unsigned long long best = 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t0 = b0; t0 < b1; t0 += DT_SCAN_TILE) {
        const uint64_t i0 = t0 + threadIdx.x * 4u;
        uint32_t v[4], t = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            v[q] = 0;
            if (i0 + q < b1) { v[q] = J.diff[i0 + q]; J.diff[i0 + q] = 0; }
            t += v[q];
        }
        const uint32_t incl = rcx_wave_incl_scan(t);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = run + incl - t, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) { if (w < wave) before += wsum[w]; all += wsum[w]; }
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            before += v[q];                                                 // the score of start lo + i0 + q
            if (i0 + q < len) {
                const unsigned long long pk = ((unsigned long long)before << 32) | (uint32_t)~(uint32_t)(lo + i0 + q);
                if (pk > best) best = pk;
            }
        }
        run += all;
        __syncthreads();
    }
    if (best) atomicMax(&top, best);
    __syncthreads();
    if (threadIdx.x == 0 && top) atomicMax((unsigned long long*)(J.state + DT_BEST), top);
}

// ---- per round: one workgroup per job takes the winner ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt_take(DtArgs a)
{
    __shared__ uint32_t first, last;
    const DtJob J = dt_job(a, blockIdx.x);
    const uint32_t done = J.state[DT_DONE], tail = J.state[DT_TAIL], zero = J.state[DT_ZERO];
    const unsigned long long best = *(const unsigned long long*)(J.state + DT_BEST);
    if (threadIdx.x == 0) { first = 0xffffffffu; last = 0; }
    __syncthreads();                                                        // every thread has the state before thread 0 changes it
    if (done) return;
    const uint32_t score = (uint32_t)(best >> 32), s = ~(uint32_t)best, H = a.k - a.d;
    if (!score) {                                                           // no start, or nothing left to cover in this epoch
        if (threadIdx.x == 0) {
            J.state[DT_ZERO] = zero + 1; J.state[DT_ROUNDS] += 1; J.state[DT_BEST] = 0; J.state[DT_BEST + 1] = 0;
            if (zero + 1 >= RCX_TRAIN_ZERO_RUNS) { J.state[DT_DONE] = 1; atomicAdd((uint32_t*)a.base, 1u); }
        }
        return;
    }
    // trim: the first and the last position of the segment whose frequency is not zero yet (score > 0: there is one)
    for (uint32_t i = threadIdx.x; i <= H; i += DT_THREADS) {
        const uint32_t h = J.hash[s + i];
        if (h != DT_INVALID && J.freq[h]) { atomicMin(&first, s + i); atomicMax(&last, s + i); }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= H; i += DT_THREADS) {
        const uint32_t h = J.hash[s + i];
        if (h != DT_INVALID) J.freq[h] = 0;
    }
    const uint32_t b = first, seg = last + a.d - b, g = seg < tail ? seg : tail;
    const bool stop = g < a.d;
    const uint32_t nt = stop ? tail : tail - g;
    if (!stop) for (uint32_t i = threadIdx.x; i < g; i += DT_THREADS) J.stage[nt + i] = J.S[b + i];
    if (threadIdx.x == 0) {
        J.state[DT_TAIL] = nt; J.state[DT_ZERO] = 0; J.state[DT_ROUNDS] += 1; J.state[DT_BEST] = 0; J.state[DT_BEST + 1] = 0;
        if (stop || nt == 0) { J.state[DT_DONE] = 1; atomicAdd((uint32_t*)a.base, 1u); }
    }
}

// ---- once per call: the dictionary to the slot's start, and the job's results ----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt_finish(DtArgs a, uint8_t* out_base, const uint64_t* out_off, uint64_t* out_len, uint64_t* in_used,
                                                   int32_t* status, uint32_t* aux_out)
{
    const uint32_t j = blockIdx.y;
    const DtJob J = dt_job(a, j);
    const uint32_t tail = J.state[DT_TAIL], len = J.cap - tail;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_len[j] = len; status[j] = RCX_OK; aux_out[j] = J.state[DT_ROUNDS];
        if (in_used) in_used[j] = J.n;
    }
    if (J.dead) return;
    uint8_t* o = out_base + out_off[j];
    for (uint64_t i = (uint64_t)blockIdx.x * DT_THREADS + threadIdx.x; i < len; i += (uint64_t)gridDim.x * DT_THREADS) o[i] = J.stage[tail + i];
}

// k.aux: the words of rcx_plan_train (the first njobs come back as the rounds run).  Synchronous: the host reads the count of finished
// jobs back every few rounds and stops when every job is done, by the plan's round bound at the latest.
#define DT_POLL 8u
static int launch_dict_train(hipStream_t s, rcx_kargs& k, const rcx_train_plan& plan, std::string& err)
{
    const uint32_t n = k.nblocks;
    if (!n) return RCX_RC_OK;
    if (!k.aux) { err = "dict train: use rcx_dict_train_batch"; return RCX_RC_BAD_ARG; }
    if (!k.scratch || k.scratch_bytes < plan.scratch_bytes) { err = "dict train: scratch too small"; return RCX_RC_BAD_ARG; }
    DtArgs a;
    a.in_base = k.in_base; a.in_off = k.in_off; a.in_len = k.in_len; a.out_cap = k.out_cap; a.aux = k.aux;
    a.base = (uint8_t*)(((uintptr_t)k.scratch + 255u) & ~(uintptr_t)255u);
    a.njobs = n; a.k = plan.k; a.d = plan.d; a.f = plan.f;
    auto grid = [](uint64_t items, uint64_t per, uint32_t cap) { const uint64_t g = (items + per - 1) / per; return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g); };
#define DT_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return RCX_RC_HIP_ERROR; } } while (0)
    DT_HIP(hipMemsetAsync(a.base, 0, 256, s));
    const uint64_t clear = std::max<uint64_t>((uint64_t)1 << plan.f, plan.max_size + 1);
    hipLaunchKernelGGL(k_dt_clear, dim3(grid(clear, DT_THREADS, DT_GRID), n), dim3(DT_THREADS), 0, s, a);
    if (plan.live) {
        hipLaunchKernelGGL(k_dt_hash, dim3(grid(plan.max_n, DT_THREADS, DT_GRID), n), dim3(DT_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_dt_back, dim3(grid(plan.max_n, DT_BACK_TILE, DT_BACK_GRID), n), dim3(DT_THREADS), 0, s, a);
        const uint32_t gadd = grid(plan.max_size + plan.k, DT_THREADS, DT_GRID);
        // (a share of the differences is a multiple of DT_SCAN_TILE words: workgroups beyond this many have none in any job)
        const uint32_t gscan = grid(plan.max_size + 1, DT_SCAN_TILE, RCX_TRAIN_SCAN_BLOCKS);
        for (uint64_t r = 0; r < plan.max_rounds; r++) {
            hipLaunchKernelGGL(k_dt_add, dim3(gadd, n), dim3(DT_THREADS), 0, s, a, r);
            hipLaunchKernelGGL(k_dt_sums, dim3(gscan, n), dim3(DT_THREADS), 0, s, a, r);
            hipLaunchKernelGGL(k_dt_scanmax, dim3(gscan, n), dim3(DT_THREADS), 0, s, a, r);
            hipLaunchKernelGGL(k_dt_take, dim3(n), dim3(DT_THREADS), 0, s, a);
            if (r % DT_POLL == DT_POLL - 1) {
                uint32_t ndone = 0;
                DT_HIP(hipMemcpyAsync(&ndone, a.base, 4, hipMemcpyDeviceToHost, s));
                DT_HIP(hipStreamSynchronize(s));
                if (ndone >= n) break;
            }
        }
    }
    hipLaunchKernelGGL(k_dt_finish, dim3(grid(plan.max_cap, DT_THREADS, DT_FINISH_GRID), n), dim3(DT_THREADS), 0, s, a, k.out_base, k.out_off,
                       k.out_len, k.in_used, k.status, k.aux);
#undef DT_HIP
    return RCX_RC_OK;
}
