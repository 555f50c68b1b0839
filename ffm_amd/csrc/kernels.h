// kernels.h -- host-side launch interface of the FFM HIP kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ffm {

// ceil(2^32 / d): n / d == mulhi(n, magic_div(d)) whenever n * d < 2^32 (core_common.h mdiv).
// Callers check it on the host (magic_div_ok): the engine's padded cell indices, and the
// learner's cell indices and coordinates, all stay below it for maps of <= 65,536 cells.
__host__ __device__ inline uint32_t magic_div(uint32_t d) { return (uint32_t)((0x100000000ull + d - 1) / d); }
// every n < n_end divides exactly by magic_div(d)
__host__ __device__ inline bool magic_div_ok(uint64_t n_end, uint32_t d) { return n_end * (uint64_t)d <= 0x100000000ull; }

// Per-env parameters (ffm_engine_set_env_params): one 32-byte record per env, built on the host
// from the env's set with the expressions ffm_engine_create uses for the engine-wide values, so
// an env steps bit for bit like a homogeneous engine of its set.
struct EnvParams {
    float kS32, kD32;      // f32(-k_S), f32(k_D)
    float c0, c1;          // f32((1-decay)(1-diffuse)), f32(decay(1-diffuse)/|nb|)
    double kS64;           // -k_S (float64 SFF path)
    int N;                 // agents placed at the env's next placement
    uint32_t reset_thr;    // CoreStepArgs::reset_thr for this N
};
static_assert(sizeof(EnvParams) == 32, "EnvParams is one 32-byte record");

struct CoreStepArgs {
    int H, W, HW;          // map shape
    uint32_t mW, mPW;      // magic_div(W), magic_div(W + 2): row of a cell index by one multiply-high
    int A;                 // agent slots per env (stride of pos)
    int K;                 // envs per workgroup
    long long E;           // envs on this device
    long long env_base;    // global id of env 0 (RNG key)
    uint16_t* pos;         // [E][A] cell indices
    int* cnt;              // [E]
    float* dff;            // [E][HW]
    int* episodes;         // [E] or nullptr
    unsigned long long* counters;  // [slots][4] agent_steps, exits, resets, steps (one slot per wave/block)
    const uint8_t* pmap;   // [(H+2)*(W+2)] padded map codes: 0 free, 2 blocked, 3 exit
    const void* psff;      // [(H+2)*(W+2)] padded SFF, f32 or f64
    float kS32, kD32;      // f32(-k_S), f32(k_D)
    double kS64;           // -k_S (float64 SFF path)
    float c0, c1;          // f32((1-decay)(1-diffuse)), f32(decay(1-diffuse)/|nb|)
    uint32_t key0, key1;   // Philox key (seed)
    uint32_t t;            // step index (Philox counter word 0)
    int auto_reset, N;     // re-place N agents when an env empties
    const uint16_t* free_list;  // [F] row-major free cells
    const uint16_t* free_padded;  // [F] the same cells as padded indices (x+1)*(W+2)+y+1
    int F;
    uint32_t* mt_np;       // [E][625] MT mode
    uint32_t* mt_py;       // [E][625]
    unsigned long long* dbg;  // diagnostic builds: [16] per-phase cycle sums (else unused)
    unsigned char* scratch;   // big maps: [blocks][scratch_stride] block state (else nullptr)
    size_t scratch_stride;
    int no_step_count;        // group kernel: this launch leaves the `steps` counter alone (an env shard
                              // other than the step's first: engine.cpp, step shards)
    uint32_t reset_thr;       // placement with F <= 128 (wave_reset.h): keys below it are the candidates that
                              // get ranked; floor(M * 2^32 / F), set at create; 0: every key is ranked.
                              // (Kept away from F: next to it the two load as a pair at kernel entry and
                              // the threshold then holds a scalar register across the whole step loop.)
    // Group kernel: the engine-constant stage image (core_group_stage_build; 16-B aligned).  Its
    // first stage_q4 float4s are the block-shared LDS region byte for byte; the per-lane geometry
    // tables of both group sizes follow.  Built once at create: nothing in it has a setter.  The
    // group kernel's per-env forms (envp set) take a second image, built with multiplier 1 for the
    // SFF term: every env's own k_S is applied in the kernel.
    const void* stage;
    int stage_q4;
    // Episode log and statistics (ffm_engine_set_episode_log; episode_log.h).  All null / zero
    // while the feature is off: ep_start != nullptr is the switch the kernels test.
    uint32_t* ep_start;            // [E] step index that keyed each env's current placement
    int* eplog;                    // [eplog_cap][4] {global env, episode, steps, t_end} or nullptr
    unsigned long long* eplog_n;   // records appended (may pass eplog_cap: dropped)
    long long eplog_cap;
    unsigned long long* ephist;    // [ephist_bins] episodes by length (last bin: that long or longer) or nullptr
    int ephist_bins;
    unsigned long long* epsum;     // [kEpSumSlots][kEpSumStride] partial summaries (with ephist): count, sum of
                                   // steps, sum of steps^2, max of ~steps (the min, inverted: zero is its empty
                                   // value), max; an env adds to slot e % kEpSumSlots, the host sums the slots
    // Per-env parameters: [E] records, or nullptr (off: kS32 .. c1, N and reset_thr above hold for
    // every env).  The launchers pick the kernels' PEP instantiations when it is set.
    const EnvParams* envp;
    // Per-env rooms (ffm_engine_set_env_rooms): the room table (one record of room_stride bytes per
    // room, room_layout below) and the [E] room index of every env, or nullptr (off: pmap, psff and
    // the free lists above hold for every env).  While set, envp is set too, F above is the largest
    // room's (the LDS sizes) and the launchers pick the lane, group, block and reset kernels' ROOM
// instantiations (the group kernel's is its single-group form: a wave of the grid per group).
    const unsigned char* rooms;
    const int* room_of_env;
    int room_stride;
};

// One record of the room table: 16-byte aligned, every part a whole number of 16-byte words so a
// half-wave stages a room with 16-byte loads.  hdr: F, the room's free-cell count (one int, padded to
// 16 bytes); grid: the padded grid-initialisation codes as u16 (0 free, 2 blocked, 3 exit), gs of
// them; sff: the padded f32 SFF, ss floats; free: the padded free list, room for the largest F.
struct RoomLayout {
    int gs, ss;                 // u16 codes / floats per room in the record and in a half-wave's LDS
    size_t grid, sff, free;     // byte offsets in the record (F at 0)
    size_t stride;
};
__host__ __device__ inline RoomLayout room_layout(int PHW, int Fmax) {
    RoomLayout r;
    r.gs = (PHW + 7) & ~7;
    r.ss = (PHW + 3) & ~3;
    r.grid = 16;
    r.sff = r.grid + (size_t)r.gs * 2;
    r.free = r.sff + (size_t)r.ss * 4;
    r.stride = (r.free + (size_t)(Fmax > 0 ? Fmax : 1) * 2 + 15) & ~(size_t)15;
    return r;
}

// The summary is spread over slots of one 128-byte line each: a single contended word takes
// about 100 atomic adds per us, and C2 ends about 700 episodes per step.
constexpr int kEpSumSlots = 64, kEpSumStride = 16;

// Trajectory capture of the batched ffm_core step (ffm_engine_set_trajectory_capture):
// rows of {global env, episode, step in episode, count} + agent cells after every step.
struct CoreCapture {
    const int* envs;           // [n_sel] local env indices
    const int* phase;          // [n_sel] or nullptr
    int* state;                // [n_sel][3]: episode being logged, its steps so far, count after the last step
    int* meta;                 // [cap][4]
    uint16_t* cells;           // [cap][A]
    unsigned long long* n;     // rows appended (may pass cap: dropped)
    long long cap;
    int n_sel, period;
};

// Field statistics (ffm_engine_set_field_stats; core_observe.hip): what the observer launched after
// a step launch reads -- that launch's slices of pos, cnt, ep_start and the class array -- and the
// tables it adds to.  One class's table is S = HW + 2 bins + 1 words: occupancy[HW],
// remaining[bins], alive[bins], observed; `tab` holds `slots` (a power of two) copies of the C
// tables, summed by the host when it reads.
struct ObserveArgs {
    const uint16_t* pos;           // [E][A]
    const int* cnt;                // [E]
    const uint32_t* ep_start;      // [E]
    const int* cls;                // [E] class of every env, or nullptr (class 0)
    unsigned long long* tab;       // [slots][C][S]
    long long E;
    int A, HW, bins, C, S, slots;
    uint32_t t;                    // the step index that keyed the step launch
    int run;                       // envs per run (core_observe_run)
};
// The observer's LDS budget: the C tables as u32 take the LDS form where they fit it.  A workgroup
// may declare up to 160 KiB on gfx950, but 64 KiB keeps two blocks of the observer per CU next to
// whatever a neighbouring shard's step kernel holds, and needs no opt-in above the default limit.
constexpr size_t kObserveLdsBudget = 64 * 1024;
// Slot copies of the tables, the observer's largest grid and the envs of a run (FFM_FIELD_STATS_SLOTS,
// _BLOCKS and _RUN override them when the feature is set: A/B and test switches; profiles/field_stats/).
// Measured at C2 (two shards of 32,768 envs): 64 to 256 blocks per launch all add 7.1 - 7.7 us to the
// step, 512 blocks 12.7 us and 2,048 blocks 27.8 us (every block zeroes and flushes its tables);
// 1, 4, 16 and 64 slots are within 0.5 us of each other.
constexpr int kObserveSlots = 16, kObserveMaxBlocks = 256;
int core_observe_run(int A);   // the default run: one batch of cell pairs per thread
int core_observe_grid(long long E, int run, int max_blocks);
bool core_observe_lds_safe(long long E, int A, int run, int max_blocks);
hipError_t launch_core_observe(const ObserveArgs& o, bool lds, int max_blocks, hipStream_t s);

// Exit flow (ffm_engine_set_exit_flow; core_flow.hip): what the flow kernel launched after a step
// launch reads -- that launch's slices of pos, cnt, ep_start, the class array and the room indices,
// the snapshot of the same envs before the step (prev_*) and the door table -- and the tables it
// adds to.  One (class, door) record is 1 + bins words: exited, outflow[bins]; `tab` holds `slots`
// (a power of two) copies of the C * D records, summed by the host when it reads.  The kernel ends
// by storing pos, cnt and ep_start into prev_*: whoever else writes one of the three refreshes the
// snapshot on the same stream (engine.cpp refresh_flow_snapshot).
struct FlowArgs {
    const uint16_t* pos;           // [E][A] after the step
    const int* cnt;                // [E]
    const uint32_t* ep_start;      // [E]
    uint16_t* prev_pos;            // [E][A] before the step; after the kernel: pos
    int* prev_cnt;                 // [E]
    uint32_t* prev_start;          // [E]
    const int* cls;                // [E] class of every env, or nullptr (class 0)
    const int* room_of_env;        // [E] or nullptr (room 0)
    const uint8_t* door_from;      // [R][HW] door id of the first exit among a cell's neighbours, 0xFF: none
    unsigned long long* tab;       // [slots][C][D][1 + bins]
    long long E;
    int A, HW, R, bins, C, D, slots;
    uint32_t t;                    // the step index that keyed the step launch
};
// The flow kernel's LDS budget is the observer's; its slot copies and largest grid
// (FFM_EXIT_FLOW_BLOCKS overrides the grid when the feature is set; profiles/exit_flow/).
constexpr int kFlowSlots = 16, kFlowMaxBlocks = 1024;
int core_flow_grid(long long E, int A, int max_blocks);
bool core_flow_lds_safe(long long E, int A);
hipError_t launch_core_flow(const FlowArgs& f, bool lds, int max_blocks, hipStream_t s);

// Motion statistics (ffm_engine_set_motion_stats; core_motion.hip): what the motion kernel launched
// after a step launch reads -- the flow kernel's inputs, with the direction table in the place of
// the door table -- the origin row it compacts in place and the tables it adds to.  One class is
//   flux[HW][NB + 1], present[bins], moved[bins], egress_count[HW], egress_steps[HW]
// (core_motion_stride words); `tab` holds `slots` (a power of two) copies of the C classes, summed
// by the host when it reads.  The kernel runs before the flow kernel and carries the snapshot
// forward (as the flow kernel does) only where `carry` says the flow is off.
struct MotionArgs {
    const uint16_t* pos;           // [E][A] after the step
    const int* cnt;                // [E]
    const uint32_t* ep_start;      // [E]
    uint16_t* prev_pos;            // [E][A] before the step; with carry, after the kernel: pos
    int* prev_cnt;                 // [E]
    uint32_t* prev_start;          // [E]
    uint16_t* origin;              // [E][A] the cell the agent now at an index was placed on
    uint32_t* origin_for;          // [E] the ep_start of the episode the origin row belongs to
    const int* cls;                // [E] class of every env, or nullptr (class 0)
    const int* room_of_env;        // [E] or nullptr (room 0)
    const uint8_t* dir_from;       // [R][HW] neighbour index of the first exit among a cell's neighbours, 0xFF: none
    unsigned long long* tab;       // [slots][C][core_motion_stride]
    long long E;
    int A, HW, W, R, bins, C, NB, slots, carry;
    uint32_t t;                    // the step index that keyed the step launch
};
constexpr int kMotionSlots = 16, kMotionMaxBlocks = 1024;
// Words of one class: in the tables, and in the LDS form's block copy (egress_steps, the last
// part, is not kept there: its adds go straight to the u64 tables).
inline size_t core_motion_stride(int HW, int NB, int bins) { return (size_t)HW * (NB + 1) + 2 * (size_t)bins + 2 * (size_t)HW; }
inline size_t core_motion_lds_stride(int HW, int NB, int bins) { return core_motion_stride(HW, NB, bins) - (size_t)HW; }
int core_motion_grid(long long E, int A, int max_blocks);
bool core_motion_lds_safe(long long E, int A);
hipError_t launch_core_motion(const MotionArgs& m, bool lds, int max_blocks, hipStream_t s);

size_t core_wave_smem_bytes(int H, int W, int A, int F, bool mt, bool reset, int waves);
size_t core_block_smem_bytes(int H, int W, int A, int K, int F, bool f64, bool mt, bool reset);
hipError_t launch_core_wave(const CoreStepArgs& a, int nb, bool mt, int blocks, hipStream_t s);
int core_wave_blocks_per_cu(const CoreStepArgs& a, int nb, bool mt);
size_t core_lane_smem_bytes(int H, int W, int F, int waves, bool room = false);   // room: the per-env-rooms form's
hipError_t launch_core_lane(const CoreStepArgs& a, int nb, int blocks, hipStream_t s);
int core_lane_blocks_per_cu(const CoreStepArgs& a, int nb);
int core_lane_max_pairs_per_wave();
// room: the room form's (per-env rooms, F the largest room's)
size_t core_group_smem_bytes(int H, int W, int F, int waves, int G = 4, bool room = false);
bool core_group_supported(int H, int W);
int core_group_max_iters();
// The stage image of the group kernel (CoreStepArgs::stage): its size, the float4s of its
// block-shared part, and the host-side build from the padded map, the padded f32 SFF, f32(-k_S)
// and the padded free list.
size_t core_group_stage_bytes(int H, int W, int F);
int core_group_stage_q4(int H, int W, int F);
void core_group_stage_build(int H, int W, int F, const uint8_t* pmap, const float* psff, float kS32,
                            const uint16_t* free_padded, unsigned char* out);
int core_group_pick_envs(const CoreStepArgs& a, int nb, long long E, int cus);   // envs per group (2 or 4)
hipError_t launch_core_group(const CoreStepArgs& a, int nb, int blocks, hipStream_t s, int G, bool one = true);
bool core_group_one_group(long long E, int blocks, int G);   // every wave of the grid steps at most one group
// one: of the single-group form; a.rooms set: of the room form
int core_group_blocks_per_cu(const CoreStepArgs& a, int nb, int G, bool one = false);
size_t core_multi_smem_bytes(int H, int W, int F, int waves);
hipError_t launch_core_multi(const CoreStepArgs& a, int nb, int nsteps, int blocks, hipStream_t s);
int core_multi_blocks_per_cu(const CoreStepArgs& a, int nb);
hipError_t launch_core_block(const CoreStepArgs& a, int nb, bool f64, bool mt, int block, hipStream_t s);
hipError_t launch_core_reset(const CoreStepArgs& a, hipStream_t s, const uint8_t* mask = nullptr);
size_t core_big_scratch_bytes(int H, int W, int A, int F, bool mt);
hipError_t launch_core_block_reset(const CoreStepArgs& a, hipStream_t s, const uint8_t* mask = nullptr);
hipError_t launch_update_dff(const float* src, float* dst, long long E, int H, int W, int nb, float c0,
                             float c1, hipStream_t s);
// the same with each env's own c0, c1 (envp: [E] records)
hipError_t launch_update_dff_env(const float* src, float* dst, long long E, int H, int W, int nb,
                                 const EnvParams* envp, hipStream_t s);
// extra LDS of the block kernel's PEP form (the K staged records)
size_t core_block_pep_smem_bytes(int K);
// ... and of its room form (the K records and the K room indices)
size_t core_block_room_smem_bytes(int K);
// mask: nullptr = every selected env; else ([E] device bytes) only those with a nonzero byte
hipError_t launch_core_capture_init(const CoreStepArgs& a, const CoreCapture& c, hipStream_t s,
                                    const uint8_t* mask = nullptr);
hipError_t launch_core_capture(const CoreStepArgs& a, const CoreCapture& c, hipStream_t s);
hipError_t launch_np_expf(const float* x, float* y, long long n, hipStream_t s);

}  // namespace ffm
