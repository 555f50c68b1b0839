// episode_log.h -- the core engine's evacuation-time log (ffm_engine_set_episode_log):
// one record per ended episode and an on-device histogram / summary of the lengths.
// See DESIGN.md "Episode log".
//
// An episode of env e ends at the step after which e holds no agents, having held some
// before it.  Its length is the difference of two step indices, t - ep_start[e] (wrapping
// u32): ep_start[e] is the index that keyed the env's current placement, written wherever
// an env is placed.  Nothing is counted per step.  Every sum is an integer atomic, so the
// statistics do not depend on launch geometry, shards or fused steps.
#pragma once
#include "core_common.h"
#include "kernels.h"

namespace ffm {

// An env placed with step index t (reset kernels, in-kernel auto-reset).
__device__ __forceinline__ void eplog_mark_start(const CoreStepArgs& a, long long e, uint32_t t) {
    if (a.ep_start) a.ep_start[e] = t;
}

// Histogram and summary of one ended episode.
__device__ __forceinline__ void eplog_stats(const CoreStepArgs& a, long long e, uint32_t steps) {
    if (!a.ephist) return;
    const uint32_t bin = steps < (uint32_t)a.ephist_bins - 1u ? steps : (uint32_t)a.ephist_bins - 1u;
    atomicAdd(&a.ephist[bin], 1ull);
    unsigned long long* s = a.epsum + (size_t)kEpSumStride * (size_t)(e & (kEpSumSlots - 1));
    atomicAdd(&s[0], 1ull);
    atomicAdd(&s[1], (unsigned long long)steps);
    atomicAdd(&s[2], (unsigned long long)steps * steps);
    atomicMax(&s[3], ~(unsigned long long)steps);   // the min, inverted
    atomicMax(&s[4], (unsigned long long)steps);
}

__device__ __forceinline__ void eplog_store(const CoreStepArgs& a, unsigned long long row, long long e, int k,
                                            uint32_t steps, uint32_t t) {
    if ((long long)row >= a.eplog_cap) return;   // counted, not stored: the drain reports it as dropped
    *reinterpret_cast<int4*>(a.eplog + 4 * row) = make_int4((int)(a.env_base + e), k, (int)steps, (int)t);
}

// Episode index of an episode that just ended: episodes[e] before this step's increment
// (the caller has already incremented it where auto_reset re-places the env).
__device__ __forceinline__ int eplog_index(const CoreStepArgs& a, long long e) {
    return a.auto_reset && a.episodes ? a.episodes[e] - 1 : 0;
}

// One thread, one ended episode of local env e at step index t (wave and block kernels).
__device__ __forceinline__ void eplog_end_one(const CoreStepArgs& a, long long e, uint32_t t) {
    const uint32_t steps = t - a.ep_start[e];
    a.ep_start[e] = t;
    if (a.eplog) eplog_store(a, atomicAdd(a.eplog_n, 1ull), e, eplog_index(a, e), steps, t);
    eplog_stats(a, e, steps);
}

// A whole wave: lanes with `ended` each end the episode of local env e at step index t;
// lanes with `placed` had env e re-placed by this step (the auto-reset: every ended env,
// and an env that was empty already).  One atomic on the record count per wave; the base
// is broadcast and every ending lane writes at base + its rank among the ending lanes.
// Call with a.ep_start != nullptr, all lanes converged.
__device__ __forceinline__ void eplog_end_wave(const CoreStepArgs& a, bool ended, bool placed, long long e, uint32_t t,
                                               int lane) {
    if (!__ballot(ended || placed)) return;   // wave-uniform, the common case
    const unsigned long long m = __ballot(ended);
    uint32_t steps = 0;
    if (ended) steps = t - a.ep_start[e];
    if (ended || placed) a.ep_start[e] = t;
    if (!m) return;
    if (a.eplog) {
        const int leader = (int)__builtin_ctzll(m);
        uint32_t lo = 0, hi = 0;
        if (lane == leader) {
            const unsigned long long b = atomicAdd(a.eplog_n, (unsigned long long)__popcll(m));
            lo = (uint32_t)b;
            hi = (uint32_t)(b >> 32);
        }
        lo = (uint32_t)__builtin_amdgcn_readlane((int)lo, leader);
        hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, leader);
        const unsigned long long base = ((unsigned long long)hi << 32) | lo;
        if (ended) eplog_store(a, base + (unsigned)lanes_below(m), e, eplog_index(a, e), steps, t);
    }
    if (ended) eplog_stats(a, e, steps);
}

}  // namespace ffm
