// core_flow.hip -- exit flow on the device (ffm_engine_set_exit_flow): which exit cell ("door")
// the agents leave through and when, per class of envs.  See DESIGN.md "Exit flow".
//
// Like the field statistics' observer this is a kernel of its own, launched after a step launch on
// that launch's stream; no step kernel changes.  It compares the env state the step left (P' =
// pos, n = cnt, ep_start) with the snapshot of the state before it (P = prev_pos, n0 = prev_cnt,
// prev_start) and then stores the new state into the snapshot, for the next step.
//
// The rule (model/ffm_core.py:66-72, 100-102: an agent with an exit among its free neighbours
// always requests the first exit in neighbour order, and whoever reaches an exit is dropped):
// door_from[room][c] is the door id of the first exit cell among c's neighbours, 0xFF for none
// (built on the host).  Agent i < n0 left in this step iff door_from[P[i]] != 0xFF and P[i] is not
// among P'[0 .. n): such an agent either leaves or stays put, and nobody else can enter a cell
// that was occupied before the step.  An env the step emptied -- re-placed by the auto-reset
// (ep_start == t) or left with n == 0 -- lost every agent of P.  An event adds, with c the env's
// class, tau = t - prev_start (wrapping u32) and b = min(tau, bins - 1),
//   exited[c][door] += 1,  outflow[c][door][b] += 1.
// Every sum is an integer: the result depends on no grid, form, slot count or order.
//
// One (class, door) record is 1 + bins words: exited, outflow[bins]; the device holds `slots`
// copies of the C * D records as u64 (kernels.h FlowArgs::tab), summed by the host at read.
// LDS form: a block's records as u32 in LDS, non-returning LDS adds, the non-zero words added to
// slot copy blockIdx % slots at the block's end.  Global form (tables beyond the LDS budget):
// every add a u64 atomic into slot copy e % slots.
//
// A wave owns one env at a time, or two (a half-wave each) where a row of A <= 32 cells fits 32
// lanes; a lane holds one agent of P and the agent of P' with the same index.  Lanes whose cell
// has a door are flagged; unless the env was emptied, each flagged cell (a handful per room: the
// cells next to an exit) is looked up in P' by one ballot -- the loop runs over the set bits of
// the flagged ballot, so it is wave-uniform, and the cell comes from v_readlane.  Rows of more
// than 64 agents go chunk by chunk, and a flagged cell is then looked up in every chunk of P'.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace ffm {

namespace {

constexpr int kFlowThreads = 256, kFlowWaves = kFlowThreads / 64;

// Diagnostic builds that the tests must catch (profiles/exit_flow/README.md; never the product):
// 1 drops the events of emptied and re-placed envs, 2 looks a flagged cell up in P instead of P'.
#ifndef FFM_FLOW_MUTATE
#define FFM_FLOW_MUTATE 0
#endif

template <bool LDS>
__global__ __launch_bounds__(kFlowThreads) void core_flow_kernel(FlowArgs f) {
    extern __shared__ uint32_t flow_lds[];
    const int tid = (int)threadIdx.x;
    const int rec = 1 + f.bins;
    const int words = f.C * f.D * rec;
    if (LDS) {
        for (int i = tid; i < words; i += kFlowThreads) flow_lds[i] = 0;
        __syncthreads();
    }
    const int A = f.A, HW = f.HW, bins = f.bins;
    const int lane = tid & 63;
    const int per = A <= 32 ? 2 : 1;          // envs a wave holds at a time
    const int width = 64 / per;               // lanes of an env
    const int sub = lane / width, li = lane - sub * width;
    const long long items = (f.E + per - 1) / per;
    const long long nwaves = (long long)gridDim.x * kFlowWaves;
    for (long long it = (long long)blockIdx.x * kFlowWaves + (tid >> 6); it < items; it += nwaves) {
        const long long e = it * per + sub;
        const bool live = e < f.E;
        int n0 = 0, n = 0, n_raw = 0, c = 0, room = 0;
        uint32_t s0 = 0, s1 = 0;
        if (live) {
            n0 = f.prev_cnt[e];
            n_raw = f.cnt[e];
            s0 = f.prev_start[e];
            s1 = f.ep_start[e];
            c = f.cls ? f.cls[e] : 0;
            room = f.room_of_env ? f.room_of_env[e] : 0;
        }
        n0 = n0 < 0 ? 0 : n0 > A ? A : n0;
        n = n_raw < 0 ? 0 : n_raw > A ? A : n_raw;
        // the step emptied the env: every agent of P left
        const bool all = n0 > 0 && (n == 0 || s1 == f.t);
        const uint32_t tau = f.t - s0;
        const uint32_t b = bins > 0 ? (tau < (uint32_t)bins - 1u ? tau : (uint32_t)bins - 1u) : 0u;
        const uint8_t* dfrom = f.door_from + (size_t)((unsigned)room < (unsigned)f.R ? room : 0) * HW;
        const size_t row = (size_t)(live ? e : 0) * A;
        for (int base = 0; base < A; base += width) {   // one trip unless A > 64
            const int i = base + li;
            uint32_t p = 0xFFFFu, q = 0xFFFFu;          // P[i], P'[i]
            if (live && i < A) {
                p = f.prev_pos[row + i];
                q = f.pos[row + i];
            }
            const uint32_t member = FFM_FLOW_MUTATE == 2 ? p : q;   // the row a flagged cell is looked up in
            // a stored cell is < HW; the comparison keeps a stray value from indexing the table
            uint32_t door = 0xFFu;
            if (i < n0 && p < (uint32_t)HW) door = dfrom[p];
            const bool flagged = door != 0xFFu && !(FFM_FLOW_MUTATE == 1 && all);
            unsigned long long todo = __ballot(flagged && !all), stay = 0;
            while (todo) {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                todo &= todo - 1;
                const uint32_t cell = (uint32_t)__builtin_amdgcn_readlane((int)p, l);
                bool found;
                if (A <= 64) {
                    const unsigned long long half = per == 2 ? (l < 32 ? 0xFFFFFFFFull : 0xFFFFFFFF00000000ull) : ~0ull;
                    found = (__ballot(i < n && member == cell) & half) != 0;
                } else {   // one env per wave: e, n are wave-uniform
                    found = false;
                    for (int b2 = 0; b2 < n && !found; b2 += 64) {
                        const int i2 = b2 + lane;
                        const uint32_t q2 = i2 < n ? (FFM_FLOW_MUTATE == 2 ? f.prev_pos : f.pos)[row + i2] : 0xFFFFu;
                        found = __ballot(q2 == cell) != 0;
                    }
                }
                if (found) stay |= 1ull << l;
            }
            if (flagged && !((stay >> lane) & 1) && (unsigned)c < (unsigned)f.C && door < (uint32_t)f.D) {
                const int at = (c * f.D + (int)door) * rec;
                if (LDS) {
                    atomicAdd(&flow_lds[at], 1u);
                    if (bins > 0) atomicAdd(&flow_lds[at + 1 + (int)b], 1u);
                } else {
                    unsigned long long* T = f.tab + (size_t)(e & (f.slots - 1)) * words;
                    atomicAdd(&T[at], 1ull);
                    if (bins > 0) atomicAdd(&T[at + 1 + (int)b], 1ull);
                }
            }
            // carry forward: what was just read as P' is the next step's P
            if (live && i < A) f.prev_pos[row + i] = (uint16_t)q;
        }
        if (live && li == 0) {
            f.prev_cnt[e] = n_raw;
            f.prev_start[e] = s1;
        }
    }
    if (LDS) {
        __syncthreads();
        unsigned long long* G = f.tab + (size_t)(blockIdx.x & (unsigned)(f.slots - 1)) * words;
        for (int i = tid; i < words; i += kFlowThreads) {
            const uint32_t v = flow_lds[i];
            if (v) atomicAdd(&G[i], (unsigned long long)v);
        }
    }
}

}  // namespace

// A wave per item (an env, or a pair where A <= 32), four waves per block, up to max_blocks.
int core_flow_grid(long long E, int A, int max_blocks) {
    const long long items = (E + (A <= 32 ? 1 : 0)) / (A <= 32 ? 2 : 1);
    const long long full = (items + kFlowWaves - 1) / kFlowWaves;
    return (int)std::max<long long>(1, std::min<long long>(full, std::max(1, max_blocks)));
}

// The LDS form's u32 words cannot overflow within one launch: a word grows by at most A per env.
bool core_flow_lds_safe(long long E, int A) { return E * (long long)A < (1ll << 32); }

hipError_t launch_core_flow(const FlowArgs& f, bool lds, int max_blocks, hipStream_t s) {
    if (f.E <= 0) return hipSuccess;
    const unsigned grid = (unsigned)core_flow_grid(f.E, f.A, max_blocks);
    if (lds) {
        const size_t smem = (size_t)f.C * f.D * (1 + f.bins) * 4;
        core_flow_kernel<true><<<dim3(grid), dim3(kFlowThreads), smem, s>>>(f);
    } else {
        core_flow_kernel<false><<<dim3(grid), dim3(kFlowThreads), 0, s>>>(f);
    }
    return hipGetLastError();
}

}  // namespace ffm
