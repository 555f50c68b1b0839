// core_observe.hip -- on-device field statistics (ffm_engine_set_field_stats): the
// time-summed occupancy of every cell and the evacuation curve N(tau), per class of envs.
// See DESIGN.md "Field statistics".
//
// The observer is a kernel of its own, launched after a step launch on that launch's stream.
// It reads what the step left -- pos, cnt, ep_start, the class array -- and writes only the
// statistics: no step kernel changes.  For env e with n = cnt[e] agents and
// tau = t - ep_start[e] (wrapping u32, the episode log's arithmetic):
//   n == 0 or tau == 0: nothing (tau == 0: this very step's auto-reset placed the env, and a
//   placement is never observed); else, with c the env's class and b = min(tau, bins - 1),
//   occupancy[c][pos[e][j]] += 1 for j < n, observed[c] += 1, remaining[c][b] += n,
//   alive[c][b] += 1.
// Every sum is an integer, so the result does not depend on the grid, the form, the slot
// count, step shards or the order of anything.
//
// One class's table is S = HW + 2 bins + 1 words: occupancy, remaining, alive, observed.  The
// device holds `slots` copies of the C tables as u64 (kernels.h ObserveArgs::tab); the host
// sums the copies when it reads.
//
// LDS form: the C tables as u32 in LDS.  A block walks contiguous runs of envs (grid-stride
// over runs), adds with LDS atomics whose result nobody reads (ds_add_u32, non-returning), and
// at its end adds its non-zero words to slot copy blockIdx % slots with u64 device-scope
// atomics.  Global form (tables beyond the LDS budget): the same walk, every add a u64 atomic
// straight into slot copy e % slots.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace ffm {

namespace {

// Large blocks: what a block pays once -- zeroing its tables and adding its non-zero words to the
// slot copies -- is paid by a quarter of the blocks that 256 threads would take for the same loads
// in flight (profiles/field_stats/).
constexpr int kObserveThreads = 1024, kObserveBatch = 4;

template <bool LDS>
__global__ __launch_bounds__(kObserveThreads) void core_observe_kernel(ObserveArgs o) {
    extern __shared__ uint32_t obs_lds[];
    const int tid = (int)threadIdx.x;
    const int words = o.C * o.S;
    if (LDS) {
        for (int i = tid; i < words; i += kObserveThreads) obs_lds[i] = 0;
        __syncthreads();
    }
    const int A = o.A, HW = o.HW, bins = o.bins;
    const uint32_t P = (uint32_t)(A + 1) >> 1;   // cell pairs (dwords) of an env's row
    const bool even = !(A & 1);                  // rows are whole dwords: one load per pair
    const uint32_t* pos32 = reinterpret_cast<const uint32_t*>(o.pos);
    for (long long r0 = (long long)blockIdx.x * o.run; r0 < o.E; r0 += (long long)gridDim.x * o.run) {
        const uint32_t ne = (uint32_t)(o.E - r0 < o.run ? o.E - r0 : o.run);
        const uint32_t items = ne * P;   // run * P < 2^31 (core_observe_run, and the override's bound)
        // kObserveBatch items per thread at a time: every load of a batch is issued before anything
        // that depends on one (the walk is bound by load latency, not by bytes), the pair's cells
        // whether or not the env counts -- the row is there either way.
        for (uint32_t l0 = (uint32_t)tid; l0 < items; l0 += kObserveBatch * kObserveThreads) {
            int nn[kObserveBatch], cc[kObserveBatch] = {};
            uint32_t st[kObserveBatch] = {}, w0[kObserveBatch] = {}, w1[kObserveBatch] = {};
#pragma unroll
            for (int u = 0; u < kObserveBatch; u++) {
                const uint32_t l = l0 + (uint32_t)u * kObserveThreads;
                nn[u] = 0;
                if (l >= items) continue;
                const uint32_t le = l / P, p = l - le * P;
                const long long e = r0 + le;
                nn[u] = o.cnt[e];
                st[u] = o.ep_start[e];
                cc[u] = o.cls ? o.cls[e] : 0;
                if (even) {
                    w0[u] = pos32[((size_t)e * A >> 1) + p];
                } else {
                    w0[u] = o.pos[(size_t)e * A + 2 * p];
                    w1[u] = 2 * p + 1 < (uint32_t)A ? o.pos[(size_t)e * A + 2 * p + 1] : 0xFFFFu;
                }
            }
#pragma unroll
            for (int u = 0; u < kObserveBatch; u++) {
                const uint32_t l = l0 + (uint32_t)u * kObserveThreads;
                const uint32_t le = l / P, p = l - le * P;
                const long long e = r0 + le;
                int n = nn[u];   // 0 past the run's end
                const uint32_t tau = o.t - st[u];
                if (n <= 0 || tau == 0) continue;
                if (n > A) n = A;
                const int c = cc[u];
                const int j = 2 * (int)p;
                uint32_t c0 = 0xFFFFu, c1 = 0xFFFFu;
                if (j < n) {
                    c0 = even ? w0[u] & 0xFFFFu : w0[u];
                    if (j + 1 < n) c1 = even ? w0[u] >> 16 : w1[u];
                }
                const uint32_t b = bins > 0 ? (tau < (uint32_t)bins - 1u ? tau : (uint32_t)bins - 1u) : 0u;
                // a stored cell is < HW (set_state checks, the kernels keep it); the comparisons
                // keep a stray value from writing outside the tables
                if (LDS) {
                    uint32_t* T = obs_lds + (size_t)c * o.S;
                    if (c0 < (uint32_t)HW) atomicAdd(&T[c0], 1u);
                    if (c1 < (uint32_t)HW) atomicAdd(&T[c1], 1u);
                    if (p == 0) {
                        atomicAdd(&T[HW + 2 * bins], 1u);
                        if (bins > 0) {
                            atomicAdd(&T[HW + b], (uint32_t)n);
                            atomicAdd(&T[HW + bins + b], 1u);
                        }
                    }
                } else {
                    unsigned long long* T = o.tab + (size_t)(e & (o.slots - 1)) * words + (size_t)c * o.S;
                    if (c0 < (uint32_t)HW) atomicAdd(&T[c0], 1ull);
                    if (c1 < (uint32_t)HW) atomicAdd(&T[c1], 1ull);
                    if (p == 0) {
                        atomicAdd(&T[HW + 2 * bins], 1ull);
                        if (bins > 0) {
                            atomicAdd(&T[HW + b], (unsigned long long)n);
                            atomicAdd(&T[HW + bins + b], 1ull);
                        }
                    }
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        unsigned long long* G = o.tab + (size_t)(blockIdx.x & (unsigned)(o.slots - 1)) * words;
        for (int i = tid; i < words; i += kObserveThreads) {
            const uint32_t v = obs_lds[i];
            if (v) atomicAdd(&G[i], (unsigned long long)v);
        }
    }
}

}  // namespace

// Envs per run: one batch of pairs per thread, so a block's loads of a run are a few KB of
// contiguous dwords, all in flight at once.
int core_observe_run(int A) {
    const int P = (A + 1) / 2;
    return std::max(1, kObserveBatch * kObserveThreads / P);
}

int core_observe_grid(long long E, int run, int max_blocks) {
    const long long runs = (E + run - 1) / run;
    return (int)std::max<long long>(1, std::min<long long>(runs, std::max(1, max_blocks)));
}

// The LDS form's u32 words cannot overflow within one launch: a word grows by at most A per
// env, and a block of this grid walks at most this many envs.
bool core_observe_lds_safe(long long E, int A, int run, int max_blocks) {
    const long long grid = core_observe_grid(E, run, max_blocks);
    const long long runs = (E + run - 1) / run;
    const long long per_block = (runs + grid - 1) / grid * run;
    return per_block * (long long)A < (1ll << 32);
}

hipError_t launch_core_observe(const ObserveArgs& o, bool lds, int max_blocks, hipStream_t s) {
    if (o.E <= 0) return hipSuccess;
    const unsigned grid = (unsigned)core_observe_grid(o.E, o.run, max_blocks);
    if (lds) {
        const size_t smem = (size_t)o.C * o.S * 4;
        core_observe_kernel<true><<<dim3(grid), dim3(kObserveThreads), smem, s>>>(o);
    } else {
        core_observe_kernel<false><<<dim3(grid), dim3(kObserveThreads), 0, s>>>(o);
    }
    return hipGetLastError();
}

}  // namespace ffm
