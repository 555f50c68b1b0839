// wave_reset.h -- Philox placement of one env by one wavefront (shared by the
// wave, pack and reset kernels).  See DESIGN.md 3.2 "placement".
#pragma once
#include "core_common.h"
#include "kernels.h"

namespace ffm {

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// Philox placement of one env, stored straight to its global positions gpos[0..N)
// (unpadded cell indices): all 64 lanes.
// fl = padded free-cell list (LDS).  F <= 128: the (key, j) pairs go to LDS and
// each lane ranks its two by broadcast reads (or, CAND, the one candidate pair the
// lane is handed: DESIGN.md 4, the placement tail) -- few registers, because this
// rarely-taken branch sits inside the step loop and would otherwise set the
// kernel's VGPR peak.  Larger F: threshold the keys into an LDS candidate list
// first (about 2N + 16 survive).
// PWK > 0: the padded row width as a constant (a kernel built for one map width).  SMALL: the
// caller's maps have at most 128 free cells, so the threshold path below is not built -- its
// divisions by F and PW are loop invariants the compiler otherwise sets up in every wave of a
// kernel that holds this call in a loop, whether or not an env is re-placed.
// CAND: the small-list path first tries the candidate pass below (a.reset_thr, set at create).
// N, thr: the agents placed and the candidate threshold -- a.N and a.reset_thr, or the env's own
// (per-env parameters, kernels.h EnvParams).  F: the length of fl -- a.F, or the env's own room's
// (per-env rooms: fl is then that room's list in the room table, keys still holds a.F pairs, the
// largest room's count).
template <int PWK = 0, bool SMALL = false, bool CAND = true>
__device__ inline void wave_reset_env(const CoreStepArgs& a, uint32_t genv, unsigned long long* keys, const uint16_t* fl,
                               uint16_t* gpos, int lane, int N, uint32_t thr, int F) {
    const int PW = PWK > 0 ? PWK : a.W + 2;
    if (SMALL || F <= 128) {
        // lane holds keys j0 = lane and j1 = lane + 64 and ranks both in one pass over
        // 16-B broadcast reads of the key list (two keys per read; keys is 16-B aligned)
        const int j0 = lane, j1 = lane + 64;
        const unsigned long long k0 =
            j0 < F ? ((unsigned long long)reset_key(a.key0, a.key1, a.t, genv, (uint32_t)j0) << 32) | (unsigned)j0
                   : ~0ull;
        const unsigned long long k1 =
            j1 < F ? ((unsigned long long)reset_key(a.key0, a.key1, a.t, genv, (uint32_t)j1) << 32) | (unsigned)j1
                   : ~0ull;
        if (CAND) {
            // Only the N smallest pairs are placed.  The pairs whose key is below reset_thr (about
            // M = N + max(8, (N + 1) / 2) of the F) are the candidates: every other key is >=
            // reset_thr and so above each of them, hence with C >= N candidates the N smallest
            // pairs are all candidates and their rank among the candidates is their rank among
            // all.  The C <= 64 of them are packed into keys[] (the j0 set, then the j1 set) and
            // lane i ranks the one word keys[i] over (C + 1) / 2 reads.  C outside [N, 64] (about
            // one placement in 1,150 at F = 100, N = 32), or reset_thr = 0: the full ranking below.
            // A pad lane's ~0 key is never below reset_thr.
            const bool c0 = (uint32_t)(k0 >> 32) < thr, c1 = (uint32_t)(k1 >> 32) < thr;
            const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
            const int C0 = __popcll(m0), C = C0 + __popcll(m1);
            if (C >= N && C <= 64) {
                // keys[C] <= keys[64] lies inside the list the full ranking writes: C <= F, and
                // an odd C equal to F is that path's own pad slot
                if (c0) keys[lanes_below(m0)] = k0;
                if (c1) keys[C0 + lanes_below(m1)] = k1;
                if (lane == 0 && (C & 1)) keys[C] = ~0ull;
                wave_sync();
                const unsigned long long ki = lane < C ? keys[lane] : ~0ull;
                int r = 0;
                const ulonglong2* kv = reinterpret_cast<const ulonglong2*>(keys);
#pragma unroll 4
                for (int q = 0; q < (C + 1) / 2; q++) {
                    const ulonglong2 p = kv[q];
                    r += (p.x < ki ? 1 : 0) + (p.y < ki ? 1 : 0);
                }
                if (lane < C && r < N) gpos[r] = (uint16_t)unpad(fl[(int)(ki & 0xFFu)], PW);
                wave_sync();
                return;
            }
        }
        if (j0 < F) keys[j0] = k0;
        if (j1 < F) keys[j1] = k1;
        if (lane == 0 && (F & 1)) keys[F] = ~0ull;   // pad to pairs: ~0 is never below a key
        wave_sync();
        int r0 = 0, r1 = 0;
        const ulonglong2* kv = reinterpret_cast<const ulonglong2*>(keys);
#pragma unroll 8
        for (int q = 0; q < (F + 1) / 2; q++) {
            const ulonglong2 p = kv[q];
            r0 += (p.x < k0 ? 1 : 0) + (p.y < k0 ? 1 : 0);
            r1 += (p.x < k1 ? 1 : 0) + (p.y < k1 ? 1 : 0);
        }
        if (j0 < F && r0 < N) gpos[r0] = (uint16_t)unpad(fl[j0], PW);
        if (j1 < F && r1 < N) gpos[r1] = (uint16_t)unpad(fl[j1], PW);
        wave_sync();
        return;
    }
    uint32_t T = reset_threshold(N, F);
    int C = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        C = 0;
        for (int j0 = 0; j0 < F; j0 += 64) {
            const int j = j0 + lane;
            uint32_t k = 0;
            bool cand = false;
            if (j < F) {
                k = reset_key(a.key0, a.key1, a.t, genv, (uint32_t)j);
                cand = k <= T;
            }
            const unsigned long long m = __ballot(cand);
            if (cand) keys[C + lanes_below(m)] = ((unsigned long long)k << 32) | (unsigned)j;
            C += __popcll(m);
        }
        if (C >= N || T == 0xFFFFFFFFu) break;
        T = 0xFFFFFFFFu;
    }
    wave_sync();
    for (int i = lane; i < C; i += 64) {
        const unsigned long long ki = keys[i];
        int rank = 0;
        for (int q = 0; q < C; q++) rank += keys[q] < ki ? 1 : 0;
        if (rank < N) gpos[rank] = (uint16_t)unpad(fl[(int)(ki & 0xFFFFu)], PW);
    }
    wave_sync();
}

// The engine's one room: a.F free cells.
template <int PWK = 0, bool SMALL = false, bool CAND = true>
__device__ inline void wave_reset_env(const CoreStepArgs& a, uint32_t genv, unsigned long long* keys, const uint16_t* fl,
                               uint16_t* gpos, int lane, int N, uint32_t thr) {
    wave_reset_env<PWK, SMALL, CAND>(a, genv, keys, fl, gpos, lane, N, thr, a.F);
}

// The engine-wide form: a.N agents, a.reset_thr.
template <int PWK = 0, bool SMALL = false, bool CAND = true>
__device__ inline void wave_reset_env(const CoreStepArgs& a, uint32_t genv, unsigned long long* keys, const uint16_t* fl,
                               uint16_t* gpos, int lane) {
    wave_reset_env<PWK, SMALL, CAND>(a, genv, keys, fl, gpos, lane, a.N, a.reset_thr);
}

}  // namespace ffm
