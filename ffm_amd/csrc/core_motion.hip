// core_motion.hip -- motion statistics on the device (ffm_engine_set_motion_stats): the flow field
// (per cell, how often an agent stepped in each direction or stood still), mean speed against the
// time since placement, and the egress time by starting cell, per class of envs.  See DESIGN.md
// "Motion statistics".
//
// Like the exit flow's kernel this one is launched after a step launch on that launch's stream and
// compares the env state the step left (P' = pos, n = cnt, ep_start) with the snapshot of the
// state before it (P = prev_pos, n0 = prev_cnt, prev_start); no step kernel changes.  It runs
// before the flow kernel and stores the new state into the snapshot only where the flow is off
// (`carry`).
//
// Identity without ids.  The reference removes the agents that reached an exit order-preservingly
// (model/ffm_core.py:100-102), so agent i of P that did not leave is agent
//   i' = i - |{leavers l < i}|
// of P'.  The leavers are core_flow.hip's: agent i left iff P[i] has an exit among its neighbours
// (dir_from[room][P[i]] != 0xFF, built on the host: the index of the first exit cell in the
// reference's neighbour order) and P[i] is not among P'; a step that emptied the env (n == 0, or
// the auto-reset re-placed it: ep_start == t) took every agent.
//
// Direction d(i) in [0, NB]: a survivor's is the neighbour index of P'[i'] - P[i], NB for a stay; a
// leaver's is dir_from[P[i]].  Free cells never lie on the map's border, so the flat difference
// names the move; a difference that is no neighbour move (a state the caller made inconsistent)
// adds nothing for that agent.  origin[e][i] is the cell the agent now at index i was placed on,
// and origin_for[e] the ep_start of the episode the row belongs to.  Every placement path (reset,
// reset_envs, the auto-reset) sets ep_start to its own step index, so prev_start != origin_for
// says that the env was placed since the kernel last wrote the row: the origins of P are then P
// itself; otherwise they are read from the row.  (tau == 1 is not that test: reset_envs consumes a
// step index, so an env that another path placed in the step before it is first seen with
// tau == 2.)  The survivors' origins are stored back at i' (i' <= i, and a chunk is read before
// it is written: in place).  With c the env's class and b = min(tau, bins - 1):
//   flux[c][P[i]][d(i)] += 1;  present[c][b] += n0;  moved[c][b] += |{i : d(i) != NB}|;
//   for a leaver with origin o:  egress_count[c][o] += 1,  egress_steps[c][o] += tau.
// Every sum is an integer: the result depends on no grid, form, slot count or order.
//
// LDS form: a block's tables as u32 in LDS (a word grows by at most A per env:
// core_motion_lds_safe), the non-zero words added to slot copy blockIdx % slots at the block's end.
// egress_steps is not kept in LDS: tau is any u32, so its adds -- about 0.3 per env and step -- go
// straight to the u64 tables.  Global form (tables beyond the LDS budget): every add a u64 atomic
// into slot copy e % slots.
//
// A wave owns one env at a time, or two (a half-wave each) where a row of A <= 32 cells fits 32
// lanes.  The leaver mask is one ballot, i' a popcount of the mask's bits below the lane within
// the env's half, and P'[i'] comes from ds_bpermute.  Rows of more than 64 agents go in ascending
// chunks with a running leaver count; a chunk's successors may lie in the chunk before, so they
// are read from global memory.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace ffm {

namespace {

constexpr int kMotionThreads = 256, kMotionWaves = kMotionThreads / 64;

// Diagnostic builds that the tests must catch (profiles/motion_stats/README.md; never the
// product): 1 takes i' = i (no compaction), 2 drops the placement rule of the origins (the row is
// always read).
#ifndef FFM_MOTION_MUTATE
#define FFM_MOTION_MUTATE 0
#endif

// The neighbour index of the flat difference dd = P'[i'] - P[i] in a row of W cells: NB for a
// stay, 0xFF for no neighbour move.  Neumann up, down, left, right; Moore row-major.
__device__ __forceinline__ uint32_t direction_of(int dd, int W, int NB) {
    if (dd == 0) return (uint32_t)NB;
    if (NB == 4) return dd == -W ? 0u : dd == W ? 1u : dd == -1 ? 2u : dd == 1 ? 3u : 0xFFu;
    if (dd >= -W - 1 && dd <= -W + 1) return (uint32_t)(dd + W + 1);
    if (dd == -1) return 3u;
    if (dd == 1) return 4u;
    if (dd >= W - 1 && dd <= W + 1) return (uint32_t)(dd - W + 6);
    return 0xFFu;
}

template <bool LDS>
__global__ __launch_bounds__(kMotionThreads) void core_motion_kernel(MotionArgs m) {
    extern __shared__ uint32_t motion_lds[];
    const int tid = (int)threadIdx.x;
    const int A = m.A, HW = m.HW, W = m.W, bins = m.bins, NB = m.NB, ND = NB + 1;
    // a class: flux, present, moved, egress_count, egress_steps (the last not in LDS)
    const int oP = HW * ND, oM = oP + bins, oC = oM + bins, oS = oC + HW;
    const size_t S = (size_t)oS + HW, words = (size_t)m.C * S;
    const int lwords = m.C * oS;
    if (LDS) {
        for (int i = tid; i < lwords; i += kMotionThreads) motion_lds[i] = 0;
        __syncthreads();
    }
    const int lane = tid & 63;
    const int per = A <= 32 ? 2 : 1;          // envs a wave holds at a time
    const int width = 64 / per;               // lanes of an env
    const int sub = lane / width, li = lane - sub * width;
    const unsigned long long half = per == 2 ? (sub ? 0xFFFFFFFF00000000ull : 0xFFFFFFFFull) : ~0ull;
    const unsigned long long below = half & ((1ull << lane) - 1ull);
    const long long items = (m.E + per - 1) / per;
    const long long nwaves = (long long)gridDim.x * kMotionWaves;
    for (long long it = (long long)blockIdx.x * kMotionWaves + (tid >> 6); it < items; it += nwaves) {
        const long long e = it * per + sub;
        const bool live = e < m.E;
        int n0 = 0, n = 0, n_raw = 0, c = 0, room = 0;
        uint32_t s0 = 0, s1 = 0, of = 0;
        if (live) {
            n0 = m.prev_cnt[e];
            n_raw = m.cnt[e];
            s0 = m.prev_start[e];
            s1 = m.ep_start[e];
            of = m.origin_for[e];
            c = m.cls ? m.cls[e] : 0;
            room = m.room_of_env ? m.room_of_env[e] : 0;
        }
        n0 = n0 < 0 ? 0 : n0 > A ? A : n0;
        n = n_raw < 0 ? 0 : n_raw > A ? A : n_raw;
        // the step emptied the env: every agent of P left
        const bool all = n0 > 0 && (n == 0 || s1 == m.t);
        const uint32_t tau = m.t - s0;
        const uint32_t b = bins > 0 ? (tau < (uint32_t)bins - 1u ? tau : (uint32_t)bins - 1u) : 0u;
        const bool placed = FFM_MOTION_MUTATE != 2 && s0 != of;   // P is a placement the row has not seen: the origins are P
        const bool cok = (unsigned)c < (unsigned)m.C;
        const uint8_t* dfrom = m.dir_from + (size_t)((unsigned)room < (unsigned)m.R ? room : 0) * HW;
        const size_t row = (size_t)(live ? e : 0) * A;
        // the copy this env adds to, and the one its egress_steps go to in either form
        unsigned long long* T = m.tab + (size_t)((LDS ? (long long)blockIdx.x : e) & (m.slots - 1)) * words + (size_t)(cok ? c : 0) * S;
        uint32_t* L = motion_lds + (cok ? c : 0) * oS;
        int run = 0;                          // leavers in the chunks before this one
        uint32_t mv = 0;                      // agents of P that moved
        for (int base = 0; base < A; base += width) {   // one trip unless A > 64
            const int i = base + li;
            uint32_t p = 0xFFFFu, q = 0xFFFFu;          // P[i], P'[i]
            if (live && i < A) {
                p = m.prev_pos[row + i];
                q = m.pos[row + i];
            }
            const bool agent = i < n0;                  // (n0 == 0 off the end of the envs)
            uint32_t o = 0xFFFFu;                       // the agent's origin
            if (agent) o = placed ? p : m.origin[row + i];
            // a stored cell is < HW; the comparison keeps a stray value from indexing the tables
            uint32_t dl = 0xFFu;
            if (agent && p < (uint32_t)HW) dl = dfrom[p];
            const bool flagged = dl != 0xFFu;
            unsigned long long todo = __ballot(flagged && !all), stay = 0;
            while (todo) {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                todo &= todo - 1;
                const uint32_t cell = (uint32_t)__builtin_amdgcn_readlane((int)p, l);
                bool found;
                if (A <= 64) {
                    const unsigned long long h2 = per == 2 ? (l < 32 ? 0xFFFFFFFFull : 0xFFFFFFFF00000000ull) : ~0ull;
                    found = (__ballot(i < n && q == cell) & h2) != 0;
                } else {   // one env per wave: e, n are wave-uniform
                    found = false;
                    for (int b2 = 0; b2 < n && !found; b2 += 64) {
                        const int i2 = b2 + lane;
                        const uint32_t q2 = i2 < n ? m.pos[row + i2] : 0xFFFFu;
                        found = __ballot(q2 == cell) != 0;
                    }
                }
                if (found) stay |= 1ull << l;
            }
            const bool left = agent && (all || (flagged && !((stay >> lane) & 1)));
            const unsigned long long lm = __ballot(left) & half;
            // the survivor's index in P'
            const int ip = FFM_MOTION_MUTATE == 1 ? i : i - run - __popcll(lm & below);
            const bool survivor = agent && !left && ip >= 0 && ip < n;
            uint32_t qs;                                // P'[i']
            if (A <= 64) {
                const int src = sub * width + (survivor ? ip : li);
                qs = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)q);
            } else {
                qs = survivor ? m.pos[row + ip] : 0xFFFFu;
            }
            uint32_t d = 0xFFu;
            if (left) d = dl;
            else if (survivor && qs < (uint32_t)HW && p < (uint32_t)HW) d = direction_of((int)qs - (int)p, W, NB);
            if (agent && cok && d <= (uint32_t)NB) {
                if (LDS) atomicAdd(&L[(int)p * ND + (int)d], 1u);
                else atomicAdd(&T[(size_t)p * ND + d], 1ull);
            }
            mv += (uint32_t)__popcll(__ballot(agent && d < (uint32_t)NB) & half);
            if (left && cok && o < (uint32_t)HW) {
                if (LDS) atomicAdd(&L[oC + (int)o], 1u);
                else atomicAdd(&T[oC + (int)o], 1ull);
                atomicAdd(&T[oS + (int)o], (unsigned long long)tau);
            }
            // the origins follow the compaction (i' <= i, and this chunk has been read)
            if (survivor) m.origin[row + ip] = (uint16_t)o;
            // carry forward: what was just read as P' is the next step's P
            if (m.carry && live && i < A) m.prev_pos[row + i] = (uint16_t)q;
            run += __popcll(lm);
        }
        if (live && li == 0) {
            if (cok && bins > 0 && n0 > 0) {
                if (LDS) {
                    atomicAdd(&L[oP + (int)b], (uint32_t)n0);
                    if (mv) atomicAdd(&L[oM + (int)b], mv);
                } else {
                    atomicAdd(&T[oP + (int)b], (unsigned long long)n0);
                    if (mv) atomicAdd(&T[oM + (int)b], (unsigned long long)mv);
                }
            }
            if (s0 != of) m.origin_for[e] = s0;   // the row now holds this episode's survivors
            if (m.carry) {
                m.prev_cnt[e] = n_raw;
                m.prev_start[e] = s1;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        unsigned long long* G = m.tab + (size_t)(blockIdx.x & (unsigned)(m.slots - 1)) * words;
        for (int i = tid; i < lwords; i += kMotionThreads) {
            const uint32_t v = motion_lds[i];
            if (v) atomicAdd(&G[(size_t)(i / oS) * S + (size_t)(i % oS)], (unsigned long long)v);
        }
    }
}

}  // namespace

// A wave per item (an env, or a pair where A <= 32), four waves per block, up to max_blocks.
int core_motion_grid(long long E, int A, int max_blocks) {
    const long long items = (E + (A <= 32 ? 1 : 0)) / (A <= 32 ? 2 : 1);
    const long long full = (items + kMotionWaves - 1) / kMotionWaves;
    return (int)std::max<long long>(1, std::min<long long>(full, std::max(1, max_blocks)));
}

// The LDS form's u32 words cannot overflow within one launch: a word grows by at most A per env
// (a flux or egress_count word by one per agent, present and moved by n0 <= A).
bool core_motion_lds_safe(long long E, int A) { return E * (long long)A < (1ll << 32); }

hipError_t launch_core_motion(const MotionArgs& m, bool lds, int max_blocks, hipStream_t s) {
    if (m.E <= 0) return hipSuccess;
    const unsigned grid = (unsigned)core_motion_grid(m.E, m.A, max_blocks);
    if (lds) {
        const size_t smem = (size_t)m.C * core_motion_lds_stride(m.HW, m.NB, m.bins) * 4;
        core_motion_kernel<true><<<dim3(grid), dim3(kMotionThreads), smem, s>>>(m);
    } else {
        core_motion_kernel<false><<<dim3(grid), dim3(kMotionThreads), 0, s>>>(m);
    }
    return hipGetLastError();
}

}  // namespace ffm
