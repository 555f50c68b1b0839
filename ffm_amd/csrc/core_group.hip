// core_group.hip -- the production (Philox) ffm_core step for the small-room
// configs (12x12, A <= 32), with the live agents of G envs packed densely into
// the lanes of one wavefront.
//
// One launch advances every env by one FloorFieldModel.step()
// (model/ffm_core.py:36-117 of SoraKurihara/FFM), with the RNG definition and
// the semantics of core_lane_kernel and the same LDS
// picture per env: a padded direction-coded occupancy grid and a zero-halo DFF
// tile.  The lane kernel gives every env a fixed half-wave of 32 agent lanes and
// every pair a second DFF slot that only 8 lanes fill.  On MI355X that kernel is
// instruction-issue bound (occupancy 4..7 waves/SIMD all run within 2 %, and
// the waves' summed active-instruction cycles equal the kernel's wall time),
// and at steady state half its agent lanes are idle (16.9 of 32 agents live per
// env).  Here one wave steps a group of G consecutive envs per iteration:
//
//  * the group's cnt / pos / DFF rows are contiguous in HBM; the DFF streams as
//    ceil(G * HW / 256) float4 slots per lane (G = 8 at 12x12: 4.5 slots, 90 %
//    of the lanes busy, against 56 % in the lane kernel);
//  * the live agents of the G envs are concatenated in env order and packed 64
//    to a chunk: packed index j = 64 c + lane belongs to env s with
//    S[s] <= j < S[s+1] (S = exclusive prefix of the counts, wave-uniform);
//    chunks = ceil(live / 64), about 2.6 per 8 envs at steady state against
//    4 half-empty pair iterations;
//  * every phase (mark, decide, resolve, compaction) loops over the chunks, so
//    every agent of every env has decided before any resolves: the phases are
//    separated exactly as in the lane kernel;
//  * the order-preserving exit compaction (model/ffm_core.py:100-102) works on
//    the packed order: the exclusive kept-prefix of every packed index goes to
//    LDS, an agent's new index is its prefix minus the prefix at its env's
//    start, an env's new count the difference of the prefixes at its bounds (the
//    single-group form reads both from the lanes that hold them instead);
//  * the owner's friction bit (the top bit of its Philox word z) rides in bit 12
//    of its grid code, so the shared friction words are one dword per agent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "core_common.h"
#include "kernels.h"
#include "lane_common.h"
#include "episode_log.h"
#include "wave_reset.h"

namespace ffm {

namespace {

// Deferred auto-reset placements: 8 bits per group iteration (env s of the wave's
// i-th group = bit 8 i + s), so a wave steps at most kGroupMaxIters groups.
constexpr int kGroupMaxIters = 16;
constexpr int kGroupPendWords = 8 * kGroupMaxIters / 32;

struct GroupCarve {
    size_t grid, tile, words, posst, kp, keys, pend, dummy, per_wave;
};

// The staged positions are dead once the agents are marked, so the kept-prefix
// array reuses them; the placement keys are used only after the step loop (the
// single-group form: after the step's stencil), so they reuse the grids and tiles.  Both forms
// take this carve; the single-group form writes no kept prefixes and defers no placement, so of
// kp it uses the staged positions only and pend stays unused.
template <int G>
__host__ __device__ inline GroupCarve group_carve(int PHW, int TS, int F) {
    GroupCarve c;
    size_t o = 0;
    c.grid = o;  o += a16((size_t)G * PHW * 2);
    c.tile = o;  o += a16((size_t)G * TS * 4);
    c.keys = 0;
    const size_t keys_end = a16((size_t)(F > 0 ? F : 1) * 8);
    if (o < keys_end) o = keys_end;
    c.words = o; o += (size_t)G * 32 * 4;
    c.posst = o;
    // the compaction writes an entry for every lane of every agent chunk (idle lanes too: no
    // exec-mask branch), so the array spans whole chunks: (G * 32 + 63) / 64 * 64 + 1 entries
    c.kp = o;    o += a16((size_t)(((G * 32 + 63) / 64) * 64 + 1) * 2);
    c.pend = o;  o += kGroupPendWords * 4;
    c.dummy = o; o += 4;   // the target of the idle lanes' LDS writes (no exec-mask branch per write)
    c.per_wave = a16(o);
    return c;
}

// Block-shared: the map (u8), the staged SFF term (f32), the free-cell list (u16) and
// the map widened to the grid's u16 codes (each wave's grids are copied from it).
__host__ __device__ inline size_t group_shared_bytes(int PHW, int F) {
    return a16((size_t)PHW) + a16((size_t)PHW * 4) + a16((size_t)(F > 0 ? F : 1) * 2) + a16((size_t)PHW * 2);
}

// The room form's carve (per-env rooms, core_group_kernel<.., ROOM>).  No block-shared region: the
// wave holds every env's own grid (stride room_layout().gs codes), copied from the room table in
// whole 16-byte words; the SFFs stay in the table, where decide reads them.  The placement keys
// reuse the grids and tiles (dead past the stencil) and are sized by F, the largest room's count.
// The form is built on the single-group form: no kept-prefix array, and no placement is deferred.
template <int G>
__host__ __device__ inline GroupCarve group_room_carve(int PHW, int TS, int F) {
    const RoomLayout lay = room_layout(PHW, F);
    GroupCarve c;
    size_t o = 0;
    c.grid = o;  o += a16((size_t)G * lay.gs * 2);
    c.tile = o;  o += a16((size_t)G * TS * 4);
    c.keys = 0;
    const size_t keys_end = a16((size_t)(F > 0 ? F : 1) * 8);
    if (o < keys_end) o = keys_end;
    c.words = o; o += (size_t)G * 32 * 4;
    c.posst = o; o += a16((size_t)G * 16 * 4);   // the group's position dwords (A <= 32)
    c.kp = c.pend = o;                           // neither exists in this carve
    c.dummy = o; o += 4;
    c.per_wave = a16(o);
    return c;
}

// The stage image (CoreStepArgs::stage): the block-shared region above byte for byte (pads zero),
// then one table per group size of the per-lane slot geometry, which depends on (G, lane) only.
// A table is three arrays of 64 uint4, one entry per lane each (a 16-byte load):
//   A  x, y, z  toff[k]: the tile float index of the lane's k-th DFF float4 slot (-1: none)
//      w        bits 0-5   yfl: 2 bits per slot (the float4 starts / ends its row)
//               bits 8-19  senv: 4 bits per slot (its env, 15 = none)
//               bits 20-21 the scalar tail's cell starts / ends its row
//               bits 24-31 the float4 index of the tile-halo word this lane clears in the
//                          prologue (255: none)
//   B  lo[0], ro[0], lo[1], ro[1]: the tile float index of slot k's left and right neighbour
//      in its row, toff[k] - 1 and toff[k] + 4, or 0 (a zero word of the halo) across the
//      map's edge and for a missing slot
//   C  the same two of the scalar tail's cell, then lo[2], ro[2]
constexpr int kGeomWords = 12;
constexpr int kGeomTableBytes = 64 * kGeomWords * 4;

template <int H, int W, int G>
void group_lane_geom(int lane, int32_t (&w)[kGeomWords]) {
    constexpr int HW = H * W, TS = lane_tile_floats(H, W), Q4 = HW / 4, Q = G * Q4;
    constexpr int NS = (Q + 63) / 64, NSF = Q / 64, HQ = (4 + W) / 4;
    static_assert(NS <= 3 && (4 + W) % 4 == 0 && TS % 4 == 0 && G * 2 * HQ <= 64 && G * TS / 4 <= 255,
                  "geometry table entry");
    uint32_t yfl = 0, senv = 0, tail = 0;
    int lo[3] = {0, 0, 0}, ro[3] = {0, 0, 0}, tlo = 0, tro = 0;
    for (int k = 0; k < 3; k++) w[k] = -1;
    for (int k = 0; k < NS; k++) {
        const int q = k * 64 + lane;
        const int s = q / Q4, c = 4 * (q - s * Q4), y = c % W;
        w[k] = q < Q ? s * TS + 4 + W + c : -1;
        yfl |= (q < Q && y == 0 ? 1u : 0u) << (2 * k);
        yfl |= (q < Q && y == W - 4 ? 2u : 0u) << (2 * k);
        senv |= (uint32_t)(q < Q ? s : 15) << (4 * k);
        lo[k] = q < Q && y != 0 ? w[k] - 1 : 0;
        ro[k] = q < Q && y != W - 4 ? w[k] + 4 : 0;
    }
    if (Q % 64 != 0 && (Q % 64) * 4 == 64) {   // SCALAR_TAIL's cell (the kernel uses it with NB == 4)
        const int q = 4 * 64 * NSF + lane;
        const int s = q / HW, c = q - s * HW, y = c % W, off = s * TS + 4 + W + c;
        tail = (y == 0 ? 1u : 0u) | (y == W - 1 ? 2u : 0u);
        tlo = y != 0 ? off - 1 : 0;
        tro = y != W - 1 ? off + 1 : 0;
    }
    // the halo of env s's tile: its first and last HQ float4s (lane_tile_floats)
    const int s = lane / (2 * HQ), j = lane % (2 * HQ);
    const uint32_t halo = lane < G * 2 * HQ ? (uint32_t)(s * (TS / 4) + (j < HQ ? j : TS / 4 - 2 * HQ + j)) : 255u;
    w[3] = (int32_t)(yfl | (senv << 8) | (tail << 20) | (halo << 24));
    w[4] = lo[0]; w[5] = ro[0]; w[6] = lo[1]; w[7] = ro[1];
    w[8] = tlo; w[9] = tro; w[10] = lo[2]; w[11] = ro[2];
}

// Packed per-chunk state (one VGPR each):
//   cs: pp (bits 0-15) | al (16-20) | s (21-23) | live (24) | x + 1 (25-31)
//   cr: slot (0-3, 15 = no request) | to_exit (4)          -- after decide
//       np (0-15) | keep (16) | kept prefix (17-26)         -- after resolve
__device__ __forceinline__ int cs_pp(uint32_t v) { return (int)(v & 0xFFFFu); }
__device__ __forceinline__ int cs_al(uint32_t v) { return (int)((v >> 16) & 31u); }
__device__ __forceinline__ int cs_s(uint32_t v) { return (int)((v >> 21) & 7u); }
__device__ __forceinline__ bool cs_live(uint32_t v) { return ((v >> 24) & 1u) != 0u; }
__device__ __forceinline__ int cs_xp1(uint32_t v) { return (int)(v >> 25); }

__device__ __forceinline__ float lane_f32(float x, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}

// decide(), exact pass (lane_decide_exact, Neumann) for the chunk's pending lanes `pend`, one
// agent at a time across the wave: candidate k (0..3 neighbour, 4 stay) is evaluated on lane k,
// so the score, NumPy's exp and the f32 divide run once per candidate and side by side, and
// nothing is re-read from LDS.  Every rounding is the serial path's, in its order: the max,
// the f32 sum from -0 and the f64 cumsum are folded over the valid candidates in candidate
// order from the lanes' values (wave-uniform operands, dependent adds).  Called in wave-uniform
// control flow with all lanes active; csv is the chunk's cs word, wx / wy the decide draw.
// PEP: psff is the raw SFF, and lane s < G of kSv / kDv holds env s's f32(-k_S) / f32(k_D); the
// pending agent's env is wave-uniform here, so its two values are one readlane each.
// TABLE (the room form): PHW is the grids' stride and the SFF is read from the room table: psff is
// room 0's SFF there, lane s < G of roomv holds env s's room index and rstride is the record stride
// in floats.  Otherwise psff is the block's SFF in LDS.
template <int W, int PHW, int TS, bool PEP = false, bool TABLE = false>
__device__ __forceinline__ uint32_t group_exact_coop(unsigned long long pend, uint32_t slot, uint32_t csv, uint32_t wx,
                                                     uint32_t wy, const uint16_t* grid, const float* psff,
                                                     const float* tile, float kD, int lane, float kSv = 0.0f,
                                                     float kDv = 0.0f, int roomv = 0, int rstride = 0) {
    constexpr int NB = 4, PW = W + 2;
    while (pend) {
        const int L = __builtin_ctzll(pend);   // lowest pending lane first
        pend &= pend - 1ull;
        // candidate `lane`: its grid and tile offsets from the agent's cell (nb_dx / nb_dy<4>).
        // Opaque, so they are formed here, per pending agent: as loop invariants they are hoisted
        // out of the group loop and held through every iteration (G = 4: 78 VGPRs against 73).
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int off = ln == 0 ? -PW : ln == 1 ? PW : ln == 2 ? -1 : ln == 3 ? 1 : 0;
        const int doff = ln == 0 ? -W : ln == 1 ? W : ln == 2 ? -1 : ln == 3 ? 1 : 0;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)csv, L);
        const int pp = cs_pp(v), s = cs_s(v), dd0 = 3 - 2 * cs_xp1(v);
        const int cell = pp + off;   // lanes past the candidates: the agent's own cell
        const uint32_t g = grid[s * PHW + cell];
        // the valid candidates as a wave-uniform mask: free or exit neighbours, and the stay
        const unsigned vm = ((unsigned)__ballot(g == 0u || g == 3u) & ((1u << NB) - 1u)) | (1u << NB);   // :52-60
        const float* sf = psff;
        if constexpr (TABLE) sf = psff + (size_t)__builtin_amdgcn_readlane(roomv, s) * (size_t)rstride;
        const float sa = PEP ? lane_f32(kSv, s) * sf[cell] : psff[cell];
        const float sb = (PEP ? lane_f32(kDv, s) : kD) * tile[s * TS + pp + dd0 + doff];
        const float sc = sa + sb;                                                      // :77
        float mx = -__builtin_inff();
#pragma unroll
        for (int k = 0; k <= NB; k++) {
            const float sk = lane_f32(sc, k);
            mx = (((vm >> k) & 1u) && sk > mx) ? sk : mx;                              // :78
        }
        const float e = np_expf(sc - mx);                                              // :80
        float sum = -0.0f;                                                             // add.reduce, < 8 terms: left fold
#pragma unroll
        for (int k = 0; k <= NB; k++) {
            const float t = sum + lane_f32(e, k);
            sum = ((vm >> k) & 1u) ? t : sum;                                          // :81
        }
        const float p = e / sum;                                                       // :83
        // the f64 cumsum in choice: every lane folds the same terms, lane k through candidate k
        // (its mask is vm up to bit k), so lane NB ends with the total; the masks derive from
        // vm, not from the lane alone, and so are not held in SGPRs across the loop
        const unsigned vmk = vm & ((2u << (ln & 7)) - 1u);
        double run = 0.0;
#pragma unroll
        for (int k = 0; k <= NB; k++) {
            const double t = run + (double)lane_f32(p, k);
            run = ((vmk >> k) & 1u) ? t : run;
        }
        const unsigned long long rb = __builtin_bit_cast(unsigned long long, run);
        const double last = __builtin_bit_cast(
            double, ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rb >> 32), NB) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rb, NB));
        const double inv = 1.0 / last;
        const double u = u53((uint32_t)__builtin_amdgcn_readlane((int)wx, L),
                             (uint32_t)__builtin_amdgcn_readlane((int)wy, L));
        const unsigned gt = (unsigned)__ballot(cdf_gt(run, last, inv, u)) & vm & ((1u << NB) - 1u);
        const uint32_t pick = no_request_sum(last) ? (uint32_t)kNoReq                  // :82 (wave-uniform)
                              : gt ? (uint32_t)__builtin_ctz(gt) : (uint32_t)NB;       // cdf[-1] == 1 > u
        slot = lane == L ? pick : slot;
    }
    return slot;
}

}  // namespace

#ifndef FFM_GROUP_ABLATE
#define FFM_GROUP_ABLATE 0   // diagnostic builds only
#endif

// Skeleton ladder (diagnostic builds only; results invalid, timing only; profiles/r06/c2/):
//   0: the group loop streams the state in and stores it back unchanged (no prologue, no LDS)
//   1: + the block prologue (map / SFF term / free list staging, tile clears, grid init)
//   2: + the group staged in LDS and the DFF stencil (positions and counts stored back)
//   3: + count prefix, mark, unmark, compaction and stores (every agent stays: no decide,
//        no resolve)
//   4: the product kernel
#ifndef FFM_GROUP_LADDER
#define FFM_GROUP_LADDER 4
#endif

#ifndef FFM_GROUP_WAVES
#define FFM_GROUP_WAVES 6   // minimum waves per SIMD asked of the register allocator (G = 4 needs 73 VGPRs; the grid holds 6 per SIMD)
#endif

#ifndef FFM_GROUP_ONE_WAVES
// The same for the single-group form (ONE).  Every instantiation stays below the 64 VGPRs of
// eight waves per SIMD at 6 (tools/kernel_resources.py).  Asking for (8, 8) also cuts the SGPR
// budget: a build that did spilled 10 - 99 scalars to VGPR lanes (SQ_INSTS_VALU 671 -> 690 per
// wave in the headline kernel, profiles/lds_fit/).
#define FFM_GROUP_ONE_WAVES 6
#endif

#ifndef FFM_GROUP_G
#define FFM_GROUP_G 4
#endif
constexpr int kGroupG = FFM_GROUP_G;   // envs per group at large E
#ifndef FFM_GROUP_G_SMALL
#define FFM_GROUP_G_SMALL 2
#endif
constexpr int kGroupGSmall = FFM_GROUP_G_SMALL;   // envs per group when the large-E groups fill under half the waves

// EPL: the episode log (episode_log.h) as a kernel of its own, as KD1 is (group_op): behind a
// runtime pointer its code costs the step 4 VGPRs with the log off.
// ONE: the single-group form, for grids whose every wave steps at most one group (4 * blocks >=
// groups: every test-sized engine, every launch below the shard threshold at its default grid).
// The step is the loop form's one iteration, phase for phase and draw for draw, without the loop:
// the group's loads are issued at entry and nothing is prefetched (so no empty resource and no
// second group state), a wave without a group skips the step under one wave-uniform guard (it
// still meets the prologue's barrier), and the envs that emptied are re-placed straight from the
// step's ballot, in ascending env order as the loop form's deferred mask gives them, once the DFF
// is stored (no mask word in LDS).
// PEP: with per-env parameters (a.envp, kernels.h).  Lane s < G holds env s's record, loaded with
// the group's state; decide takes the agent's env's kS32 / kD32 on the raw SFF (a.stage is then the
// image built with multiplier 1), the stencil the c0 / c1 of each slot's env, the count store and
// the placements the env's N.  No KD1 variant: k_D * DFF with k_D == 1 is DFF exactly.
// ROOM (only with ONE and PEP): per-env rooms (a.rooms / a.room_of_env, kernels.h).  Lane s < G holds
// env s's room index, loaded with the group's state (a partial last group reads 0: room 0, always
// valid).  There is no block-shared region and no __syncthreads: the wave copies each env's grid codes
// from its room's record of the table into its own LDS (group_room_carve; 16-byte loads spread over
// the lanes, L2-resident), decide reads the agent's env's grid there and its room's raw SFF in the
// table (through L1 / L2: a few rooms of 784 bytes each; copying them into the wave's LDS measured
// slower at every size, profiles/env_rooms_group/ab.txt), and a placement takes the env's room's
// free list and F straight from the record.  Every index into a grid, an SFF or a tile comes from
// a position (< H * W) or a host-validated free-list entry, none from a map code: an env stepped in
// a room it was not placed in stays memory-safe (undefined for that env only).
template <int NB, int HT, int WT, int G, bool KD1, bool EPL, bool ONE, bool PEP = false, bool ROOM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ONE ? FFM_GROUP_ONE_WAVES : FFM_GROUP_WAVES, 8)))
void core_group_kernel(CoreStepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int H = HT, W = WT, HW = H * W, PW = W + 2, PHW = (H + 2) * PW;
    constexpr int TS = lane_tile_floats(H, W);
    constexpr int Q4 = HW / 4;                 // float4s per env
    constexpr int Q = G * Q4;                  // float4s per group
    constexpr int NS = (Q + 63) / 64;          // float4 slots per lane (staging)
    constexpr int NSF = Q / 64;                // full float4 slots
    // a partial last slot of at most 16 float4s is stepped as one cell per lane instead
    // (G = 4 at 12x12: 144 float4s = 2 full slots + 64 cells), so its stencil keeps every
    // lane busy (Neumann only: the Moore stencil keeps the float4 form)
    constexpr bool SCALAR_TAIL = NB == 4 && Q % 64 != 0 && (Q % 64) * 4 == 64;
    constexpr int MAXC = (G * 32 + 63) / 64;   // agent chunks per group (A <= 32)
    constexpr int PWORDS = G * 16;             // position dwords per group (A <= 32)
    static_assert(G >= 1 && G <= 8 && HW % 4 == 0 && H + 1 < 128, "group geometry");
    static_assert(!PEP || !KD1, "the per-env form multiplies by every env's own k_D");
    static_assert(!ROOM || (PEP && ONE), "the room form takes every env's record and is built on the single-group form");
    // the room form: grids strided per env as in the room table (whole 16-byte words)
    constexpr int GS = ROOM ? ((PHW + 7) & ~7) : PHW;
    static_assert(MAXC * 64 >= G * 32 && PWORDS * 4 <= (MAXC * 64 + 1) * 2, "kp spans the chunks; posst fits in it");
    // the single-group form has no kept-prefix array: its compaction reads the prefixes from the lanes
    static_assert(!ONE || MAXC <= 2, "the kept prefixes are read from the first or the last chunk");
    const int A = a.A;
    const int lane = (int)(threadIdx.x & 63);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    const GroupCarve cv = [&] {
        if constexpr (ROOM) return group_room_carve<G>(PHW, TS, a.F);
        else return group_carve<G>(PHW, TS, a.F);
    }();
    // block-shared (group_shared_bytes): the map and the widened map are in the image too, but
    // the kernel reads only the SFF term and the free list from LDS.  ROOM: neither is read.
    constexpr size_t kImgSff = ((size_t)PHW + 15) / 16 * 16, kImgFree = kImgSff + ((size_t)PHW * 4 + 15) / 16 * 16;
    const float* psff = reinterpret_cast<const float*>(smem + kImgSff);
    const uint16_t* pfree = reinterpret_cast<const uint16_t*>(smem + kImgFree);
    unsigned char* wbase = smem + (ROOM ? 0 : group_shared_bytes(PHW, a.F)) + (size_t)wv * cv.per_wave;
    uint16_t* const grid = reinterpret_cast<uint16_t*>(wbase + cv.grid);
    float* const tile = reinterpret_cast<float*>(wbase + cv.tile);
    uint32_t* const words = reinterpret_cast<uint32_t*>(wbase + cv.words);
    uint32_t* const posst32 = reinterpret_cast<uint32_t*>(wbase + cv.posst);
    const uint16_t* const posst = reinterpret_cast<const uint16_t*>(wbase + cv.posst);
    uint16_t* const kp = reinterpret_cast<uint16_t*>(wbase + cv.kp);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(wbase + cv.keys);
    uint32_t* const pend = reinterpret_cast<uint32_t*>(wbase + cv.pend);
    const int kDummy16 = (int)((cv.dummy - cv.grid) / 2);    // grid index of the dummy word
    const int kDummy32 = (int)((cv.dummy - cv.words) / 4);   // words index of the dummy word

    // The stage image (kernels.h): one resource over its block-shared part and both geometry tables.
    static_assert(G == kGroupG || G == kGroupGSmall, "a geometry table per built group size");
    const int sq4 = a.stage_q4;
    const __amdgpu_buffer_rsrc_t rS = pair_rsrc(a.stage, sq4 * 16 + 2 * kGeomTableBytes);
    // The lane's DFF float4 slots: q = 64 k + lane of the group's G * HW cells, env q / Q4,
    // cell 4 (q % Q4) of that env.  Their tile offsets and flags depend on (G, lane) only and
    // come from the image's table (group_lane_geom): 16-byte loads of the lane's entries.
    const int gtab = sq4 * 16 + (G == kGroupG ? kGeomTableBytes : 0);
    auto geom = [&](int j) {   // array j of the table: the lane's entry
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rS, lane * 16 + j * 1024, gtab, 0));
    };
    const uint4 gw = geom(0);
    static_assert(NS <= 3, "geometry table entry");
    int toff[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) toff[k] = (int)(k == 0 ? gw.x : k == 1 ? gw.y : gw.z);
    // yfl at bit 0 (2 bits per slot), senv at bit 8 (4 per slot), the halo word at bit 24
    const uint32_t geo = gw.w;
    // Neumann: the stencil's left / right neighbours by their own offsets (0: the halo's zero
    // word), so the float4 slots test and hold no edge flag in the loop.  Moore keeps the flags (yfl).
    int lo[NS], ro[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) lo[k] = ro[k] = 0;
    if (NB == 4) {
        const uint4 gb = geom(1);
        lo[0] = (int)gb.x; ro[0] = (int)gb.y;
        if (NS > 1) { lo[1] = (int)gb.z; ro[1] = (int)gb.w; }
        if (NS > 2 && !SCALAR_TAIL) {
            const uint4 gc = geom(2);
            lo[2] = (int)gc.z; ro[2] = (int)gc.w;
        }
    }

    const long long E = a.E;                   // host-checked: (E + 7) * HW * 4 < 2^31
    const uint32_t ebase = (uint32_t)a.env_base;
    // Whole-array buffer resources, built once.  The engine pads pos / cnt / DFF to whole groups
    // of 8 envs (zeroed), so a partial last group reads zero counts and DFF and its stores land
    // in the padding; every access takes its group's byte base as the scalar offset, and lanes
    // past the group's bytes use kOOB (dropped).
    // A launch may also be one env shard of the engine's arrays (engine.cpp, step shards): pos /
    // cnt / dff / episodes then point at the shard's first env and E is its env count.  Shards
    // start at multiples of 8 envs, so every shard but the last holds whole groups only (G divides
    // 8) and its Epad = E: the resources end at the shard's end, every store of a group is
    // addressed inside that group's envs, and the hardware drops what lies past a resource -- no
    // store reaches the next shard.  The last shard's partial group lands in the arrays' padding
    // as before.  Only the position load may read past a shard (G * 64 bytes whatever A is, cut
    // at the resource's 4 bytes of slack): read-only, of rows this launch does not step.
    const int Epad = (int)((E + 7) & ~7LL);
    const __amdgpu_buffer_rsrc_t rC = pair_rsrc(a.cnt, Epad * 4);
    const __amdgpu_buffer_rsrc_t rP = pair_rsrc(a.pos, Epad * A * 2 + 4);   // + the dword of slack
    const __amdgpu_buffer_rsrc_t rD = pair_rsrc(a.dff, Epad * HW * 4);
    // PEP: the records are not padded; what a partial last group reads past them is zero
    const __amdgpu_buffer_rsrc_t rE = pair_rsrc(PEP ? (const void*)a.envp : (const void*)a.dff,
                                                PEP ? (int)E * (int)sizeof(EnvParams) : 0);
    const int ngroups = (int)((E + G - 1) / G);
    const int wstride = (int)gridDim.x * 4;
    int g = (int)blockIdx.x * 4 + wv;

    struct GState {
        float4 d[NS];
        uint32_t p0, p1;
        int c;
        float4 pr;   // PEP, lane s < G: kS32, kD32, c0, c1 of env s
    };
    // past the last group (the loop's final prefetch) the loads go through empty resources:
    // every lane's access is out of range, no bytes move, and no value is conditionally
    // defined (a `return` there cost 8-14 VGPRs)
    const __amdgpu_buffer_rsrc_t rZ = pair_rsrc(a.dff, 0);
    auto load_rec = [&](int gg, GState& st) {   // PEP: the group's records, {kS32, kD32, c0, c1} of env `lane`
        constexpr int RB = (int)sizeof(EnvParams);
        // past the last group every lane's offset is out of range (no second resource to select).
        // The offset is formed here, per load (opaque): as a loop invariant it is held through every
        // iteration of the loop form (its G = 2 build with the episode log then spills 4 VGPRs).
        const bool ok = ONE || gg >= 0;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        st.pr = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rE, ok && ln < G ? ln * RB : kOOB,
                                                                                 (ok ? gg * G : 0) * RB, 0));
    };
    auto load = [&](int gg, GState& st) {
        const bool ok = ONE || gg >= 0;   // ONE loads its own group only
        const int e0 = ok ? gg * G : 0;
        const __amdgpu_buffer_rsrc_t rc = ok ? rC : rZ, rp = ok ? rP : rZ, rd = ok ? rD : rZ;
        st.c = (int)__builtin_amdgcn_raw_buffer_load_b32(rc, lane < G ? lane * 4 : kOOB, e0 * 4, 0);
        st.p0 = __builtin_amdgcn_raw_buffer_load_b32(rp, lane < PWORDS ? lane * 4 : kOOB, e0 * A * 2, 0);
        st.p1 = PWORDS > 64 ? __builtin_amdgcn_raw_buffer_load_b32(rp, 64 + lane < PWORDS ? 256 + lane * 4 : kOOB,
                                                                 e0 * A * 2, 0)
                            : 0u;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            const int q = k * 64 + lane;
            st.d[k] = __builtin_bit_cast(float4,
                                         __builtin_amdgcn_raw_buffer_load_b128(rd, q < Q ? q * 16 : kOOB, e0 * HW * 4, 0));
        }
        if constexpr (PEP) load_rec(gg, st);
    };
    // PEP: the value lane s holds (s < G, per lane: an agent's env, a DFF slot's env), one ds_bpermute
    auto env_val = [](float v, int s) {
        return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(s * 4, __builtin_bit_cast(int, v)));
    };
    // PEP: the placement of env e of this launch with its own N and threshold, read here: rare,
    // nothing of the step is live
    auto place = [&](long long e) {
        if constexpr (ROOM) {   // ... and its own room's free list and F, from the table (keys holds a.F pairs)
            const unsigned char* rec = a.rooms + (size_t)a.room_of_env[e] * (size_t)a.room_stride;
            wave_reset_env<PW, true>(a, ebase + (uint32_t)e, keys,
                                     reinterpret_cast<const uint16_t*>(rec + room_layout(PHW, a.F).free),
                                     a.pos + e * A, lane, a.envp[e].N, a.envp[e].reset_thr,
                                     min(*reinterpret_cast<const int*>(rec), a.F));
        } else if constexpr (PEP)
            wave_reset_env<PW, true>(a, ebase + (uint32_t)e, keys, pfree, a.pos + e * A, lane, a.envp[e].N,
                                     a.envp[e].reset_thr);
        else wave_reset_env<PW, true>(a, ebase + (uint32_t)e, keys, pfree, a.pos + e * A, lane);
    };
    constexpr int LAD = FFM_GROUP_LADDER;
    GState cur;
    if (!ONE) load(g < ngroups ? g : -1, cur);
    else if (g < ngroups) load(g, cur);   // wave-uniform; cur is read under the same guard only

    int roomv = 0;   // ROOM, lane s < G: env s's room index
    if constexpr (ROOM) {
        if (LAD >= 1 && g < ngroups) {   // wave-uniform: a wave without a group stages nothing
            // lane s < G: env s's room index.  One resource over the launch's E indices with the
            // group's base as the scalar offset: past the last env the load returns 0, room 0.
            roomv = (int)__builtin_amdgcn_raw_buffer_load_b32(pair_rsrc(a.room_of_env, (int)E * 4),
                                                                        lane < G ? lane * 4 : kOOB, g * G * 4, 0);
            // Every env's grid codes from its room's record (the host checked every index and that
            // room_stride is room_layout()'s): 16-byte word q of the G grids is word q % GQ of env
            // q / GQ's, and lands at byte 16 q of the wave's grids, whose stride is the record's.
            const RoomLayout lay = room_layout(PHW, a.F);
            constexpr int GQ = GS * 2 / 16;
            static_assert((GS * 2) % 16 == 0, "whole 16-byte words per env");
#pragma unroll
            for (int q0 = 0; q0 < G * GQ; q0 += 64) {
                const int q = q0 + lane, s = min(q / GQ, G - 1);
                // env s's index from the lane that holds it, taken with every lane active (s < G always)
                // (diagnostic: env 0's room for all)
                const int rb = __builtin_amdgcn_ds_bpermute(s * 4, roomv);
                const int r = (FFM_GROUP_ABLATE & 4) ? __builtin_amdgcn_readlane(roomv, 0) : rb;
                const unsigned char* rec = a.rooms + (size_t)r * (size_t)a.room_stride;
                if (q < G * GQ)
                    reinterpret_cast<uint4*>(grid)[q] = reinterpret_cast<const uint4*>(rec + lay.grid)[q - s * GQ];
            }
            // the tiles' halos, as below
            if ((geo >> 24) != 255u) reinterpret_cast<float4*>(tile)[geo >> 24] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // the wave's own grids and halos before its mark and decide read them: no block-wide barrier
        if (LAD >= 1) wave_sync();
    } else if (LAD >= 1) {
        // Block-shared region: the image's first sq4 float4s, one 16-byte load and LDS store per
        // thread (the host checks sq4 <= 256).  The map, f32(-k_S) * SFF, the free list and the
        // widened map are engine constants: nothing is recomputed per launch.
        if ((int)threadIdx.x < sq4)
            reinterpret_cast<uint4*>(smem)[threadIdx.x] = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(rS, (int)threadIdx.x * 16, 0, 0));
        // Every env's grid starts as the map: the widened map straight from the image (8 bytes per
        // lane, G LDS stores), so the wave's own state does not wait for the block's.
        static_assert((PHW * 2) % 8 == 0 && PHW * 2 / 8 <= 64, "8-B grid copies, one per lane");
        if (lane < PHW * 2 / 8) {
            const int pm16 = (int)(a16((size_t)PHW) + a16((size_t)PHW * 4) + a16((size_t)(a.F > 0 ? a.F : 1) * 2));
            const auto mw = __builtin_amdgcn_raw_buffer_load_b64(rS, lane * 8, pm16, 0);
#pragma unroll
            for (int s = 0; s < G; s++)
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(grid) + s * (PHW * 2) + lane * 8) =
                    __builtin_bit_cast(uint2, mw);
        }
        // Only the tiles' halos are cleared (the zero rows above and below the map with the 4 floats
        // before and after them, G * 8 float4s: one store).  The interior needs no clear: every
        // iteration stages all NS slots of its group before anything reads the tile, a partial
        // group's loads return the arrays' zeroed padding, and loads past the last group go through
        // the empty resource and return zero.  Nothing ever writes the halo.
        if ((geo >> 24) != 255u) reinterpret_cast<float4*>(tile)[geo >> 24] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ONE && lane < kGroupPendWords) pend[lane] = 0u;
        // the block-shared region is first read by decide (the SFF term) and by the placement tail
        __syncthreads();
    }

    unsigned c_steps = 0, c_exits = 0, c_resets = 0;
    constexpr uint32_t mW = (uint32_t)(((1ull << 32) + (unsigned)W - 1) / (unsigned)W);   // x = c / W, c < 2^16
    const int g_first = g;
    for (int iter = 0; g < ngroups; g += wstride, iter++) {
        const int e0 = g * G;
        const int nenv = (int)min((long long)G, E - e0);
        if (LAD <= 2) {   // ladder rungs 0-2: positions and counts stored back unchanged
            const __amdgpu_buffer_rsrc_t rq = pair_rsrc(a.pos + e0 * A, (nenv * A * 2 + 3) & ~3);
            __builtin_amdgcn_raw_buffer_store_b32(cur.p0, rq, lane < PWORDS ? lane * 4 : kOOB, 0, 0);
            if (PWORDS > 64)
                __builtin_amdgcn_raw_buffer_store_b32(cur.p1, rq, 64 + lane < PWORDS ? 256 + lane * 4 : kOOB, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)cur.c, pair_rsrc(a.cnt + e0, nenv * 4),
                                                  lane < G ? lane * 4 : kOOB, 0, 0);
            c_steps += (unsigned)A * (unsigned)nenv;
        }
        if (LAD <= 1) {   // rungs 0-1: the DFF stored back from registers
            const __amdgpu_buffer_rsrc_t rq = pair_rsrc(a.dff + e0 * HW, nenv * HW * 4);
#pragma unroll
            for (int k = 0; k < NS; k++) {
                const int q = k * 64 + lane;
                buf_st4(rq, q < Q ? q * 16 : kOOB, cur.d[k]);
            }
            if (ONE) break;
            GState nx;
            load(g + wstride < ngroups ? g + wstride : -1, nx);
            cur = nx;
            continue;
        }

        GState nxt;
        const int gn = g + wstride < ngroups ? g + wstride : -1;
        // ---- stage the group (prefetched by the previous iteration or the prologue) -------
#pragma unroll
        for (int k = 0; k < NS; k++)
            if (k < NSF || toff[k] >= 0) *reinterpret_cast<float4*>(tile + toff[k]) = cur.d[k];
        unsigned long long rsm = 0ull;   // envs re-placed at the end of this step
        if (LAD == 2) wave_sync();       // ladder rung 2: the staged tile before the stencil reads it
        if (LAD >= 3) {
            if (lane < PWORDS) posst32[lane] = cur.p0;
            if (PWORDS > 64 && 64 + lane < PWORDS) posst32[64 + lane] = cur.p1;
            int S[G + 1];   // exclusive prefix of the counts (wave-uniform)
            S[0] = 0;
#pragma unroll
            for (int s = 0; s < G; s++) S[s + 1] = S[s] + __builtin_amdgcn_readlane(cur.c, s);
            const int T = S[G];
            c_steps += (unsigned)T;
            wave_sync();   // posst before the mark reads it

            // ---- packed agents: cell and occupancy mark ------------------------------------
            uint32_t cs[MAXC], cr[MAXC];
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                cs[c] = (uint32_t)(PW + 1) | (1u << 25);   // idle: an in-bounds cell
                cr[c] = 15u;
                if (c * 64 < T) {
                    const int j = c * 64 + lane;
                    int s = 0, st = 0;
#pragma unroll
                    for (int q = 1; q < G; q++) {
                        const bool ge = j >= S[q];
                        s += ge ? 1 : 0;
                        st = ge ? S[q] : st;
                    }
                    const bool live = j < T;
                    const int al = live ? j - st : 0;
                    const uint32_t p = posst[live ? s * A + al : 0];
                    const int x = (int)__umulhi(p, mW);
                    const int y = (int)p - x * W;
                    const int pp = live ? (x + 1) * PW + y + 1 : PW + 1;
                    grid[live ? s * GS + pp : kDummy16] =
                        (uint16_t)(DirCodes::kAgent | (uint32_t)al | (DirCodes::kNoDir << 8));
                    cs[c] = (uint32_t)pp | ((uint32_t)al << 16) | ((uint32_t)s << 21) | ((live ? 1u : 0u) << 24) |
                            ((uint32_t)(live ? x + 1 : 1) << 25);
                }
            }
            wave_sync();

            // ---- decide (model/ffm_core.py:40-88) -------------------------------------------
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                if (LAD == 3) cr[c] = DirCodes::kNoDir;   // ladder: every agent stays, no request
                if (LAD >= 4 && c * 64 < T) {
                    const uint32_t v = cs[c];
                    const int pp = cs_pp(v), al = cs_al(v), s = cs_s(v);
                    const bool live = cs_live(v);
                    const uint32_t genv = ebase + (uint32_t)e0 + (uint32_t)s;
                    const uint4 pb = philox(make_uint4(a.t, genv, (uint32_t)al, kPurDecide << 28), a.key0, a.key1);
                    // the friction draw, if this agent owns a contested target
                    words[live ? s * 32 + al : kDummy32] = pb.w;
                    const uint16_t* gk = grid + s * GS;
                    const float* dk = tile + s * TS;
                    const int dd0 = 3 - 2 * cs_xp1(v);
                    bool to_exit = false;
                    // ROOM: the agent's env's room's SFF where it lies in the table (idle lanes: env 0's;
                    // every lane is active here)
                    const float* sk = psff;
                    if constexpr (ROOM) {
                        const int r = (FFM_GROUP_ABLATE & 2) ? __builtin_amdgcn_readlane(roomv, 0)
                                                             : __builtin_amdgcn_ds_bpermute(s * 4, roomv);
                        sk = reinterpret_cast<const float*>(a.rooms + (size_t)r * (size_t)a.room_stride +
                                                            room_layout(PHW, a.F).sff);
                    }
                    // PEP: the agent's env's k_S / k_D (idle lanes: env 0's), on the raw SFF
                    float kSe = a.kS32, kDe = a.kD32;
                    if constexpr (PEP) {
                        kSe = env_val(cur.pr.x, s);
                        kDe = env_val(cur.pr.y, s);
                    }
                    uint32_t slot =
                        PEP ? lane_decide<NB, false, false>(pp, PW, gk, sk, dk, dd0, kSe, kDe, pb.x, to_exit)
                            : lane_decide<NB, true, KD1>(pp, PW, gk, psff, dk, dd0, a.kS32, a.kD32, pb.x, to_exit);
                    slot = live ? slot : kNoReq;
                    // u near a cdf boundary: the exact NumPy arithmetic decides
                    if (NB == 4) {   // Neumann: one pending agent at a time across the wave
                        const unsigned long long pm = __ballot(slot == kPending);
                        if (pm) {   // wave-uniform, rare
                            if constexpr (ROOM)
                                slot = group_exact_coop<W, GS, TS, true, true>(
                                    pm, slot, v, pb.x, pb.y, grid,
                                    reinterpret_cast<const float*>(a.rooms + room_layout(PHW, a.F).sff), tile, 0.0f, lane,
                                    cur.pr.x, cur.pr.y, roomv, a.room_stride / 4);
                            else if constexpr (PEP)
                                slot = group_exact_coop<W, PHW, TS, true>(pm, slot, v, pb.x, pb.y, grid, psff, tile, 0.0f,
                                                                          lane, cur.pr.x, cur.pr.y);
                            else
                                slot = group_exact_coop<W, PHW, TS>(pm, slot, v, pb.x, pb.y, grid, psff, tile, a.kD32, lane);
                        }
                    } else if (slot == kPending)   // Moore: per lane
                        slot = lane_decide_exact_arr<NB, !PEP>(pp, PW, gk, sk, dk, dd0, kSe, kDe, u53(pb.x, pb.y));
                    const uint32_t sd = slot <= (uint32_t)NB ? slot : DirCodes::kNoDir;
                    grid[live ? s * GS + pp : kDummy16] =
                        (uint16_t)(DirCodes::kAgent | (uint32_t)al | (sd << 8) | ((pb.z >> 31) << 12));
                    cr[c] = sd | ((to_exit ? 1u : 0u) << 4);
                }
            }
            wave_sync();

            // ---- resolve (model/ffm_core.py:90-98), by each requester ------------------------
            unsigned long long km[MAXC];
            int kept = 0;
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                km[c] = 0ull;
                if (c * 64 < T) {
                    const uint32_t v = cs[c];
                    const int pp = cs_pp(v), al = cs_al(v), s = cs_s(v);
                    const bool live = cs_live(v);
                    const uint32_t sd = cr[c] & 15u;
                    const bool to_exit = (cr[c] & 16u) != 0u;
                    const uint32_t slot = sd == DirCodes::kNoDir ? (uint32_t)kNoReq : sd;
                    const uint16_t* gk = grid + s * GS;
                    const int r = (int)slot_cell_k<NB, PW>(slot, pp);
                    const bool req = slot <= (uint32_t)NB;
                    const bool moving = req && r != pp;
                    bool granted = req && !moving;   // a stay is always granted
                    if (LAD >= 4) {
                        const int rt = moving ? r : pp;
                        int m = 0, k = 0, o = 0x7F;
                        uint32_t zo = 0u;
#pragma unroll
                        for (int d = 0; d < NB; d++) {
                            const uint32_t cc = gk[rt - nb_dx<NB>(d) * PW - nb_dy<NB>(d)];
                            const bool is = (cc & DirCodes::kAgent) != 0u && ((cc >> 8) & 0xFu) == (uint32_t)d;
                            const int who = (int)(cc & DirCodes::kIdx);
                            m += is ? 1 : 0;
                            k += (is && who < al) ? 1 : 0;
                            const bool lower = is && who < o;
                            zo = lower ? (cc >> 12) & 1u : zo;
                            o = lower ? who : o;
                        }
                        granted = moving ? m == 1 : granted;   // an uncontested move is granted
                        if (moving && m > 1) {
                            const uint32_t w = words[s * 32 + o];
                            const uint32_t genv = ebase + (uint32_t)e0 + (uint32_t)s;
                            const int kk = philox_friction(zo << 31, w, (uint32_t)m, a.key0, a.key1, a.t, genv,
                                                           (uint32_t)o);
                            granted = kk == k;   // :95-96
                        }
                    }
                    // :91-98 -- the mover's source cell gains 1 (one agent per cell: no collisions)
                    if (granted)
                        __hip_atomic_fetch_add(tile + s * TS + pp + 3 - 2 * cs_xp1(v), 1.0f, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WAVEFRONT);
                    const int np = granted ? r : pp;
                    const bool keep = live && !(granted && to_exit);
                    km[c] = __ballot(keep);
                    const int kpv = kept + lanes_below(km[c]);
                    kept += __popcll(km[c]);
                    cr[c] = (uint32_t)np | ((keep ? 1u : 0u) << 16) | ((uint32_t)kpv << 17);
                }
            }

            // ---- exits: order-preserving compaction (model/ffm_core.py:100-102) ---------------
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                if (c * 64 < T) {
                    const uint32_t v = cs[c];
                    if (!ONE) kp[c * 64 + lane] = (uint16_t)(cr[c] >> 17);   // idle lanes' entries are never read
                    grid[cs_live(v) ? cs_s(v) * GS + cs_pp(v) : kDummy16] = 0;   // unmark: agents stand on free cells
                }
            }
            if (!ONE && lane == 0) kp[T] = (uint16_t)kept;
            c_exits += (unsigned)(T - kept);
            // ONE: the kept prefix at an env's start is the popcount of the resolve ballots below it
            // (the bits of idle lanes and of a chunk that did not run are zero, so base[G] = kept):
            // wave-uniform, and no LDS turn before the position stores
            int base[G + 1];
            base[0] = 0;
            base[G] = kept;
#pragma unroll
            for (int s = 1; s < G; s++) {
                base[s] = 0;
                if (ONE) {
                    // the lane at packed index S[s] holds that popcount as its own kept prefix (a live
                    // lane of a chunk that ran, whenever S[s] < T; past T every later env is empty)
                    int b = __builtin_amdgcn_readlane((int)(cr[0] >> 17), S[s] & 63);
                    if (MAXC > 1)
                        b = S[s] < 64 ? b : __builtin_amdgcn_readlane((int)(cr[MAXC - 1] >> 17), S[s] & 63);
                    base[s] = S[s] < T ? b : kept;
                }
            }
            if (!ONE) wave_sync();   // kp before the position stores read it
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                if (c * 64 < T) {
                    const uint32_t v = cs[c], w = cr[c];
                    const int j = c * 64 + lane;
                    const int s = cs_s(v);
                    const bool keep = ((w >> 16) & 1u) != 0u;
                    const int start = j - cs_al(v);
                    int bs = base[0];
#pragma unroll
                    for (int q = 1; q < G; q++) bs = s == q ? base[q] : bs;
                    const int newidx = (int)(w >> 17) - (ONE ? bs : (int)kp[cs_live(v) ? start : 0]);
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)unpad((int)(w & 0xFFFFu), PW), rP,
                                                          keep ? (s * A + newidx) * 2 : kOOB, e0 * A * 2, 0);
                }
            }
            int Sl = T, Sh = T;   // lane s < G: [S[s], S[s+1])
            int nk = 0;           // lane s < G: the env's new count
            bool had;             // ... and whether it had agents
            if (ONE) {
#pragma unroll
                for (int s = 0; s < G; s++) nk = lane == s ? base[s + 1] - base[s] : nk;
                had = cur.c > 0;
            } else {
#pragma unroll
                for (int s = 0; s < G; s++) {
                    Sl = lane == s ? S[s] : Sl;
                    Sh = lane == s ? S[s + 1] : Sh;
                }
                nk = (int)kp[Sh] - (int)kp[Sl];
                had = Sh > Sl;
            }
            const bool rs = a.auto_reset && lane < nenv && nk == 0;
            rsm = __ballot(rs);
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)(rs ? a.N : nk), rC,
                                                  lane < G && !(PEP && rs) ? lane * 4 : kOOB, e0 * 4, 0);
            if (rsm) {   // wave-uniform, rare
                // PEP: an emptied env's count is its own N, read here and stored by the env's lane in
                // place of the store above (nothing of the record is held for it through the step)
                if (PEP && rs) a.cnt[e0 + lane] = a.envp[e0 + lane].N;
                c_resets += (unsigned)__popcll(rsm);
                if (a.episodes && rs) a.episodes[e0 + lane] += 1;
                if (!ONE && lane == 0) pend[iter >> 2] |= (uint32_t)rsm << (8 * (iter & 3));
            }
            // episode log (episode_log.h): with auto_reset every ended env is in rsm, so the
            // ballot of ending lanes is taken inside that rare branch only
            if (EPL && (rsm || !a.auto_reset))
                eplog_end_wave(a, lane < nenv && nk == 0 && had, rs, e0 + lane, a.t, lane);
            // ONE: no wave_sync stands before the position stores, so resolve's adds to the tile (other
            // lanes' LDS atomics) are ordered before the stencil's reads here
            if (ONE) wave_sync();
        }

        // ---- next group's HBM loads, in flight across the stencil, the stores and the
        // next group's head ------------------------------------------------------------
        if (!ONE) load(gn, nxt);

        // ---- update_dff (model/ffm_core.py:106-117): B = c0 * D, A = B + sum c1 * B[nb],
        // then the DFF stores (an env reset this step starts its next episode at zero) ----
        if (SCALAR_TAIL) {     // the last, partial float4 slot as one cell per lane (all lanes busy)
            const int q = 4 * 64 * NSF + lane;                 // the group's cell
            // the 64 cells lie in one env (ts), so the tile offset is a constant plus the lane
            constexpr int ts = 4 * 64 * NSF / HW, tc = 4 * 64 * NSF - ts * HW;
            static_assert(!SCALAR_TAIL || (4 * 64 * NSF + 63) / HW == ts, "the scalar tail spans envs");
            const float* p = tile + (ts * TS + 4 + W + tc) + lane;
            // p[-1] / p[1] lie inside the tile at the map's edges too (the zero rows above and
            // below): read them unconditionally, select the edge's zero (no exec-mask branch; two
            // more offsets from the table instead cost the kernel two VGPRs)
            const float m0 = p[0], mu = p[-W], md = p[W], pl = p[-1], pr = p[1];
            const float ml = (geo & (1u << 20)) ? 0.0f : pl, mr = (geo & (2u << 20)) ? 0.0f : pr;
            // B = c0 * D per operand, then A = B + sum c1 * B[nb] in neighbour order (:106-117)
            // PEP: env ts's own c0 / c1, from the lane that holds its record
            const float c0 = PEP ? lane_f32(cur.pr.z, ts) : a.c0, c1 = PEP ? lane_f32(cur.pr.w, ts) : a.c1;
            const float b0 = c0 * m0, bu = c0 * mu, bd = c0 * md, bl = c0 * ml, br = c0 * mr;
            float acc = b0;
            acc = acc + c1 * bu;
            acc = acc + c1 * bd;
            acc = acc + c1 * bl;
            acc = acc + c1 * br;
            float o = acc < 1e-4f ? 0.0f : acc;
            if (rsm && ((rsm >> ts) & 1ull)) o = 0.0f;   // rsm wave-uniform and rare
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, o), rD, q * 4, e0 * HW * 4, 0);
        }
#pragma unroll
        for (int k = 0; k < (SCALAR_TAIL ? NSF : NS); k++) {
            const int tb = toff[k];
            // PEP: c0 / c1 of the slot's env (senv, not the lane's agent's env), taken with every lane
            // active; a missing slot's senv (15) names a lane whose record load was dropped: zeros
            float c0 = a.c0, c1 = a.c1;
            if constexpr (PEP) {
                const int se = (int)((geo >> (8 + 4 * k)) & 15u);
                c0 = env_val(cur.pr.z, se);
                c1 = env_val(cur.pr.w, se);
            }
            if (k >= NSF && tb < 0) continue;
            const bool yl = ((geo >> (2 * k)) & 1u) != 0u, yr = ((geo >> (2 * k)) & 2u) != 0u;
            const float* p = tile + tb;
            float b[3][6];   // rows dx = -1..1, columns -1..4 (B values)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const float4 u = *reinterpret_cast<const float4*>(p + dx * W);
                b[dx + 1][1] = c0 * u.x; b[dx + 1][2] = c0 * u.y;
                b[dx + 1][3] = c0 * u.z; b[dx + 1][4] = c0 * u.w;
                if (NB == 4 && dx != 0) continue;
                b[dx + 1][0] = c0 * tile[NB == 4 ? lo[k] : yl ? 0 : tb + dx * W - 1];   // tile[0] == 0
                b[dx + 1][5] = c0 * tile[NB == 4 ? ro[k] : yr ? 0 : tb + dx * W + 4];
            }
            if (NB == 8 && ONE) {
                // Moore, straight-line form: pin every B value to a register.  Without the loop
                // around it the compiler packs the sums below by passing b[][] through private
                // memory (80 bytes of scratch, re-read at shifted offsets).
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int cc = 0; cc < 6; cc++) asm volatile("" : "+v"(b[r][cc]));
            }
            float o[4];
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                float acc = b[1][jj + 1];
#pragma unroll
                for (int d = 0; d < NB; d++) {
                    const float t = c1 * b[1 + nb_dx<NB>(d)][jj + 1 + nb_dy<NB>(d)];   // :113
                    acc = acc + t;
                }
                o[jj] = acc < 1e-4f ? 0.0f : acc;                                     // :116-117
            }
            float4 out = make_float4(o[0], o[1], o[2], o[3]);
            if (rsm) {   // wave-uniform, rare: an env re-placed this step starts its next episode at zero
                if ((rsm >> ((geo >> (8 + 4 * k)) & 15u)) & 1ull) out = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, out),
                                                   rD, (k * 64 + lane) * 16, e0 * HW * 4, 0);
        }
        wave_sync();
        if (ONE) {
            // ---- auto-reset placements, from the step's own ballot: the grids
            // and tiles the keys reuse are dead past the stencil's wave_sync above
            static_assert((H - 2) * (W - 2) <= 128, "wave_reset_env<.., SMALL>");
            uint32_t m = (uint32_t)rsm;   // wave-uniform, rarely non-zero
            while (m) {
                const long long e = (long long)e0 + __builtin_ctz(m);
                m &= m - 1u;
                place(e);
                if (FFM_GROUP_ABLATE & 1) place(e);   // diagnostic: the same placement again (identical result)
            }
            break;
        }
        cur = nxt;
    }

    // ---- deferred auto-reset placements ------------------------------
    // c_resets (wave-uniform) counts the bits set in pend: most waves re-place no env and skip
    // the tail with its setup (the placement's loop invariants)
    if (!ONE && c_resets) wave_sync();
    for (int w = 0; w < (!ONE && LAD >= 1 && c_resets ? kGroupPendWords : 0); w++) {   // ladder rung 0: pend never initialised
        uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)pend[w]);
        while (m) {
            const int bit = w * 32 + __builtin_ctz(m);
            m &= m - 1u;
            const long long e = (long long)(g_first + (bit >> 3) * wstride) * G + (bit & 7);
            // at most (H - 2) * (W - 2) cells are free: the placement's small-list path only
            static_assert((H - 2) * (W - 2) <= 128, "wave_reset_env<.., SMALL>");
            place(e);
            if (FFM_GROUP_ABLATE & 1) place(e);   // diagnostic: the same placement again (identical result)
        }
    }

    if (lane == 0) {
        unsigned long long* ctr = a.counters + 4 * ((size_t)blockIdx.x * 4 + wv);
        if (c_steps) atomicAdd(&ctr[0], (unsigned long long)c_steps);
        if (c_exits) atomicAdd(&ctr[1], (unsigned long long)c_exits);
        if (c_resets) atomicAdd(&ctr[2], (unsigned long long)c_resets);
        if (blockIdx.x == 0 && wv == 0 && !a.no_step_count) atomicAdd(&ctr[3], 1ull);
    }
}

// Both forms of the kernel take the same size.
// room: the room form's (per-env rooms: its own carve, no block-shared region; F the largest room's).
size_t core_group_smem_bytes(int H, int W, int F, int waves, int G, bool room) {
    const int PHW = (H + 2) * (W + 2), TS = lane_tile_floats(H, W);
    if (room)
        return (size_t)waves * (G == kGroupGSmall ? group_room_carve<kGroupGSmall>(PHW, TS, F).per_wave
                                                  : group_room_carve<kGroupG>(PHW, TS, F).per_wave);
    const size_t per_wave = G == kGroupGSmall ? group_carve<kGroupGSmall>(PHW, TS, F).per_wave
                                              : group_carve<kGroupG>(PHW, TS, F).per_wave;
    return group_shared_bytes(PHW, F) + (size_t)waves * per_wave;
}

bool core_group_supported(int H, int W) { return H == 12 && W == 12; }

int core_group_max_iters() { return kGroupMaxIters; }

int core_group_stage_q4(int H, int W, int F) { return (int)(group_shared_bytes((H + 2) * (W + 2), F) / 16); }

size_t core_group_stage_bytes(int H, int W, int F) {
    return group_shared_bytes((H + 2) * (W + 2), F) + 2 * (size_t)kGeomTableBytes;
}

// The image on the host.  The SFF term is the one f32 product the kernel used to stage per launch,
// f32(-k_S) * SFF: a single IEEE multiply (this file is built without contraction), so the bits
// are the device's.
// kS32 = 1.0f gives the per-env forms' image: the product is exact, the region holds the SFF's own bits.
void core_group_stage_build(int H, int W, int F, const uint8_t* pmap, const float* psff, float kS32,
                            const uint16_t* free_padded, unsigned char* out) {
    const int PHW = (H + 2) * (W + 2);
    std::memset(out, 0, core_group_stage_bytes(H, W, F));
    unsigned char* p = out;
    std::memcpy(p, pmap, (size_t)PHW);
    p += a16((size_t)PHW);
    for (int i = 0; i < PHW; i++) {
        const float v = kS32 * psff[i];
        std::memcpy(p + 4 * (size_t)i, &v, 4);
    }
    p += a16((size_t)PHW * 4);
    if (F > 0) std::memcpy(p, free_padded, (size_t)F * 2);
    p += a16((size_t)(F > 0 ? F : 1) * 2);
    for (int i = 0; i < PHW; i++) {
        const uint16_t v = pmap[i];
        std::memcpy(p + 2 * (size_t)i, &v, 2);
    }
    p += a16((size_t)PHW * 2);
    if (!core_group_supported(H, W)) return;
    for (int lane = 0; lane < 64; lane++) {
        int32_t w[kGeomWords];
        group_lane_geom<12, 12, kGroupGSmall>(lane, w);
        for (int j = 0; j < kGeomWords / 4; j++) std::memcpy(p + j * 1024 + lane * 16, w + 4 * j, 16);
        group_lane_geom<12, 12, kGroupG>(lane, w);
        for (int j = 0; j < kGeomWords / 4; j++) std::memcpy(p + kGeomTableBytes + j * 1024 + lane * 16, w + 4 * j, 16);
    }
}

// KD1: k_D == 1 (the drivers' setting), where k_D * DFF is DFF itself: a kernel of its own
// rather than a runtime flag, which the register allocator would keep (and spill) all launch.
// PEP: the per-env form (a.envp set; a.stage is then the image built with multiplier 1).
template <int NB, bool KD1, int G, bool PEP = false>
static hipError_t group_op(const CoreStepArgs& a, int blocks, hipStream_t s, int op, int* occ, bool one) {
    const size_t smem = core_group_smem_bytes(a.H, a.W, a.F, 4, G);
    if (op) {   // the resident blocks per CU of the form `one` names
        *occ = 0;
        const hipError_t r =
            one ? hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, core_group_kernel<NB, 12, 12, G, KD1, false, true, PEP>, 256, smem)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, core_group_kernel<NB, 12, 12, G, KD1, false, false, PEP>, 256, smem);
        if (r != hipSuccess) *occ = 0;
        return hipSuccess;
    }
    const long long groups = (a.E + G - 1) / G;
    if (a.H != 12 || a.W != 12 || a.A > 32 || (groups + (long long)blocks * 4 - 1) / ((long long)blocks * 4) > kGroupMaxIters)
        return hipErrorInvalidConfiguration;   // shapes the kernel and its grid assume
    // the prologue copies the image's block-shared part with one 16-byte load per thread
    if (!a.stage || a.stage_q4 != core_group_stage_q4(a.H, a.W, a.F) || a.stage_q4 > 256)
        return hipErrorInvalidConfiguration;
    // the single-group form wherever no wave of the grid steps a second group
    const dim3 grid((unsigned)blocks), block(256);
    if (one && core_group_one_group(a.E, blocks, G)) {
        if (a.ep_start) core_group_kernel<NB, 12, 12, G, KD1, true, true, PEP><<<grid, block, smem, s>>>(a);
        else core_group_kernel<NB, 12, 12, G, KD1, false, true, PEP><<<grid, block, smem, s>>>(a);
    } else {
        if (a.ep_start) core_group_kernel<NB, 12, 12, G, KD1, true, false, PEP><<<grid, block, smem, s>>>(a);
        else core_group_kernel<NB, 12, 12, G, KD1, false, false, PEP><<<grid, block, smem, s>>>(a);
    }
    return hipGetLastError();
}

// The room form (a.rooms set): the single-group form only, so the grid holds a wave per group.
template <int NB, int G>
static hipError_t group_room_op(const CoreStepArgs& a, int blocks, hipStream_t s, int op, int* occ) {
    const size_t smem = core_group_smem_bytes(a.H, a.W, a.F, 4, G, true);
    if (op) {
        *occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, core_group_kernel<NB, 12, 12, G, false, false, true, true, true>,
                                                         256, smem) != hipSuccess)
            *occ = 0;
        return hipSuccess;
    }
    if (a.H != 12 || a.W != 12 || a.A > 32 || !a.envp || !a.room_of_env || !a.stage || a.stage_q4 <= 0 ||
        !core_group_one_group(a.E, blocks, G) || smem > 64 * 1024 ||
        (size_t)a.room_stride != room_layout((a.H + 2) * (a.W + 2), a.F).stride)
        return hipErrorInvalidConfiguration;   // shapes, tables and the grid the kernel assumes
    const dim3 grid((unsigned)blocks), block(256);
    if (a.ep_start) core_group_kernel<NB, 12, 12, G, false, true, true, true, true><<<grid, block, smem, s>>>(a);
    else core_group_kernel<NB, 12, 12, G, false, false, true, true, true><<<grid, block, smem, s>>>(a);
    return hipGetLastError();
}

template <int NB>
static hipError_t group_op_kd(const CoreStepArgs& a, int blocks, hipStream_t s, int op, int* occ, int G, bool one) {
    if (a.rooms)   // per-env rooms: the room form, whatever `one` says (it has no loop form)
        return G == kGroupGSmall ? group_room_op<NB, kGroupGSmall>(a, blocks, s, op, occ)
                                 : group_room_op<NB, kGroupG>(a, blocks, s, op, occ);
    if (a.envp)   // per-env parameters: every env's own k_D, so no KD1 variant
        return G == kGroupGSmall ? group_op<NB, false, kGroupGSmall, true>(a, blocks, s, op, occ, one)
                                 : group_op<NB, false, kGroupG, true>(a, blocks, s, op, occ, one);
    if (G == kGroupGSmall)
        return a.kD32 == 1.0f ? group_op<NB, true, kGroupGSmall>(a, blocks, s, op, occ, one)
                              : group_op<NB, false, kGroupGSmall>(a, blocks, s, op, occ, one);
    return a.kD32 == 1.0f ? group_op<NB, true, kGroupG>(a, blocks, s, op, occ, one)
                          : group_op<NB, false, kGroupG>(a, blocks, s, op, occ, one);
}

// Whether a launch of E envs on `blocks` blocks has every wave step at most one group.
bool core_group_one_group(long long E, int blocks, int G) { return 4ll * blocks >= (E + G - 1) / G; }

// one: the single-group form where the grid allows it (core_group_one_group); false keeps the
// loop form on every grid (FFM_GROUP_ONE=0).
hipError_t launch_core_group(const CoreStepArgs& a, int nb, int blocks, hipStream_t s, int G, bool one) {
    return nb == 4 ? group_op_kd<4>(a, blocks, s, 0, nullptr, G, one) : group_op_kd<8>(a, blocks, s, 0, nullptr, G, one);
}

// one: of the single-group form (diagnostic); the grid rules count with the loop form's.
// a.envp set: of the per-env forms.
int core_group_blocks_per_cu(const CoreStepArgs& a, int nb, int G, bool one) {
    int n = 0;
    (void)(nb == 4 ? group_op_kd<4>(a, 0, nullptr, 1, &n, G, one) : group_op_kd<8>(a, 0, nullptr, 1, &n, G, one));
    return n;
}

// Envs per group for E envs: the large-E size, unless its groups would fill less than half the
// resident waves -- then each wave's one group is the launch's critical path, and halving the
// group (one agent chunk, half the DFF slots) shortens it (E-sweep, profiles/r06/c2: 8,192 envs
// 13.8 -> 12.7 us; from 16,384 envs on G = 4 is faster).  FFM_GROUP_ENVS=2|4 forces it.
int core_group_pick_envs(const CoreStepArgs& a, int nb, long long E, int cus) {
    if (const char* ov = std::getenv("FFM_GROUP_ENVS")) {
        const int v = std::atoi(ov);
        if (v == kGroupGSmall || v == kGroupG) return v;
    }
    const long long waves = (long long)cus * std::max(1, core_group_blocks_per_cu(a, nb, kGroupG)) * 4;
    return 2 * ((E + kGroupG - 1) / kGroupG) <= waves ? kGroupGSmall : kGroupG;
}

}  // namespace ffm
