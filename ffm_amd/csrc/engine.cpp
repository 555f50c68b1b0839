// engine.cpp -- C ABI (include/ffm_amd.h) over the HIP kernels.
//
// Owns the device state of E independent environments of one model class and
// drives the fused step kernel.  Mirrors the reference's FloorFieldModel
// (model/ffm_core.py:6-133): construction validates and uploads the map/SFF/
// params (:7-21), reset places agents (:23-26), step advances (:36-104),
// update_dff diffuses (:106-117).
#include "../../include/ffm_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace ffm {
// Shared with learn_engine.cpp: records the calling thread's last error.
int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace ffm

namespace {

int fail(int code, const std::string& msg) { return ffm::set_error(code, msg); }

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(FFM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

}  // namespace

// How a step is launched: the step kernel, its one-launch grid and, for the group kernel, the envs
// per group, its form, the step shards and the stage image.  The engine keeps one plan per form
// (create, per-env parameters on the lane / block kernel, per-env parameters on the group kernel,
// per-env rooms); plan() below picks the one in effect.
struct StepPlan {
    enum Kernel { kGroup = 0, kLane = 1, kWave = 2, kBlock = 3 };   // ffm_debug_launch_info's out[0]
    Kernel kernel = kBlock;
    int blocks = 0;              // the one-launch grid
    int g = 0;                   // group kernel: envs per group (core_group_pick_envs)
    bool one = false;            // ... the single-group form where a grid allows it (FFM_GROUP_ONE; the room
                                 // form has no other)
    // Step shards (group kernel, ffm_engine_step with n_steps > 1): disjoint env ranges, each
    // stepped by launches of its own on a stream of its own, so the fill and drain of one
    // shard's launch overlap the body of the others'.  Shard 0 runs on the caller's stream.
    struct Shard {
        long long e0 = 0, n = 0;   // first env, env count (e0 a multiple of 8)
        int blocks = 0, g = 4;     // its grid and envs per group
        size_t ctr0 = 0;           // its first counter slot
    };
    std::vector<Shard> shards;   // size() <= 1: off
    // The stage image (kernels.h): the engine's, or for the per-env form d_stage_raw.  Null on
    // engines not created on the group kernel; the other kernels do not read it.
    const unsigned char* stage = nullptr;
};

struct ffm_engine {
    ffm_engine_desc d{};
    int HW = 0, F = 0, K = 1, block = 256;
    int cus = 0;                 // the device's CUs (the persistent grids)
    bool f64 = false, mt = false;
    bool multi = false;     // multi-step kernel available (lane conditions): core_multi.hip
    int multi_blocks = 0;   // its persistent grid
    int fused = 1;          // steps per launch (ffm_engine_set_fused_steps)
    float kS32 = 0, kD32 = 0, c0 = 0, c1 = 0;
    double kS64 = 0;
    uint32_t t = 0;
    uint8_t* d_map = nullptr;    // padded map codes
    void* d_sff = nullptr;       // padded SFF
    uint16_t* d_free = nullptr;
    uint16_t* d_free_padded = nullptr;
    unsigned char* d_stage = nullptr;   // group kernel: the stage image (kernels.h), engine constants
    size_t stage_bytes = 0;
    int stage_q4 = 0;
    int reset_m = 0;             // placement candidates aimed at (0: every key is ranked) and their key
    uint32_t reset_thr = 0;      // threshold (CoreStepArgs::reset_thr); fixed at create
    uint16_t* d_pos = nullptr;
    int32_t* d_cnt = nullptr;
    float* d_dff = nullptr;
    float* d_tmp = nullptr;
    int32_t* d_eps = nullptr;
    unsigned long long* d_ctr = nullptr;   // [ctr_slots][4], summed on read
    size_t ctr_slots = 1;
    uint32_t* d_mt_np = nullptr;
    uint32_t* d_mt_py = nullptr;
    unsigned long long* d_dbg = nullptr;   // diagnostic counters (FFM_STAMPS builds)
    bool big = false;            // block kernel with its state in global scratch (maps beyond LDS)
    bool block_reset = false;    // placement by core_block_reset_kernel (free list beyond the wave reset's LDS)
    unsigned char* d_scratch = nullptr;    // [E][scratch_stride]
    size_t scratch_stride = 0;
    ffm::CoreCapture cap{};      // trajectory capture (n_sel = 0: off)
    // Episode log and statistics (ffm_engine_set_episode_log): all null / 0 while off.
    uint32_t* d_ep_start = nullptr;           // [n_envs padded to 8] step index of each env's placement
    int32_t* d_eplog = nullptr;               // [eplog_cap][4]
    unsigned long long* d_eplog_n = nullptr;  // records appended
    long long eplog_cap = 0;
    unsigned long long* d_ephist = nullptr;   // [ephist_bins] histogram, then the summary's slots
    int ephist_bins = 0;
    // Field statistics (ffm_engine_set_field_stats): null / 0 while off.  They share d_ep_start
    // with the episode log: it lives while either feature is on.
    unsigned long long* d_fs_tab = nullptr;   // [fs_slots][fs_classes][fs_stride] (kernels.h ObserveArgs)
    int32_t* d_fs_cls = nullptr;              // [n_envs] class of every env, or null (one class)
    int fs_classes = 0, fs_bins = 0, fs_slots = 0, fs_blocks = 0, fs_run = 0;
    bool fs_lds = false;                      // the observer's form
    // Exit flow (ffm_engine_set_exit_flow): null / 0 / empty while off.  It shares d_ep_start with
    // the episode log and the field statistics: it lives while any of the three is on.
    unsigned long long* d_xf_tab = nullptr;   // [xf_slots][xf_classes][xf_doors][1 + xf_bins] (kernels.h FlowArgs)
    int32_t* d_xf_cls = nullptr;              // [n_envs] class of every env, or null (one class)
    uint8_t* d_xf_door_from = nullptr;        // [rooms][HW] the door table
    uint16_t* d_prev_pos = nullptr;           // the snapshot of pos, cnt and ep_start before the next step,
    int32_t* d_prev_cnt = nullptr;            // sized like them
    uint32_t* d_prev_start = nullptr;
    int xf_classes = 0, xf_doors = 0, xf_bins = 0, xf_slots = 0, xf_blocks = 0, xf_rooms = 0;
    bool xf_lds = false;                      // the flow kernel's form
    std::vector<int32_t> xf_door_of_cell;     // [rooms][HW] the labels in effect, -1 off the exits
    // Motion statistics (ffm_engine_set_motion_stats): null / 0 while off.  They share d_ep_start
    // with the three features above, and the snapshot d_prev_* with the exit flow: it lives while
    // either of the two is on.
    unsigned long long* d_mo_tab = nullptr;   // [mo_slots][mo_classes][core_motion_stride] (kernels.h MotionArgs)
    int32_t* d_mo_cls = nullptr;              // [n_envs] class of every env, or null (one class)
    uint8_t* d_mo_dir_from = nullptr;         // [rooms][HW] the direction table
    uint16_t* d_origin = nullptr;             // sized like d_pos: the cell every agent was placed on
    uint32_t* d_origin_for = nullptr;         // sized like d_ep_start: the ep_start every origin row belongs to
    int mo_classes = 0, mo_bins = 0, mo_slots = 0, mo_blocks = 0, mo_rooms = 0;
    bool mo_lds = false;                      // the motion kernel's form
    std::vector<uint8_t> map0;                // the create-time map, row-major (0 free, 2 blocked, 3 exit)
    // The step plans, one per form (plan() picks), and when each is filled:
    StepPlan create_plan;      // ffm_engine_create: the lane, group, wave or block kernel
    StepPlan pep_plan;         // each ffm_engine_set_env_params: the lane kernel's per-env form on lane and group
                               // engines, the block kernel's on the others (the wave kernel has none)
    StepPlan pep_group_plan;   // the group kernel's own per-env form, when the feature moves to it (pep_group_setup)
    StepPlan room_plan;        // each ffm_engine_set_env_rooms: the lane, block or group form by room_kernel
    hipStream_t sh_stream[3] = {nullptr, nullptr, nullptr};   // step shards 1..3
    hipEvent_t sh_fork = nullptr;
    hipEvent_t sh_end[3] = {nullptr, nullptr, nullptr};
    // Per-env parameters (ffm_engine_set_env_params): null / empty while off.
    ffm::EnvParams* d_envp = nullptr;          // [n_envs] records (kernels.h)
    std::vector<ffm_env_params> pep_sets;      // the caller's tables, for ffm_engine_get_env_params
    std::vector<int32_t> pep_set_of_env;
    int pep_kernel = 0;                        // ffm_engine_set_env_params_kernel's mode (sticky)
    unsigned char* d_stage_raw = nullptr;      // the per-env group form's stage image: the SFF term with multiplier 1
                                               // (the raw SFF); built when the feature first moves to the group kernel
    // Per-env rooms (ffm_engine_set_env_rooms): null / empty while off.  While on, d_envp holds a
    // record per env: the caller's sets', or (pep_sets empty) the create-time values, each with
    // its room's placement threshold.
    bool lane_ok = false;                      // the lane kernel's conditions hold (create)
    unsigned char* d_rooms = nullptr;          // the room table (kernels.h room_layout)
    int32_t* d_room_of_env = nullptr;          // [n_envs]
    size_t room_stride = 0;
    int room_fmax = 0;                         // the largest room's free-cell count
    int room_kernel = 0;                       // ffm_engine_set_env_rooms_kernel's mode (sticky)
    std::vector<uint8_t> room_maps;            // the caller's tables, for ffm_engine_get_env_rooms
    std::vector<float> room_sffs;
    std::vector<int32_t> room_of_env;
    std::vector<int> room_f;                   // free cells of every room
};

// The two features.  Invariants the setters keep:
//   d_envp != nullptr  <=>  rooms_on || pep_on   (rooms keep a record per env even without sets);
//   pep_sets non-empty =>   d_envp != nullptr;
//   pep_on && pep_kernel == 1  =>  pep_group_plan is filled (and d_stage_raw built);
//   pep_on             =>   pep_plan is filled;   rooms_on  =>  room_plan is filled.
static bool rooms_on(const ffm_engine* e) { return e->d_rooms != nullptr; }
// Per-env parameters as the caller set them (the records of an engine with rooms only are the engine's own).
static bool pep_on(const ffm_engine* e) { return e->d_envp && !e->pep_sets.empty(); }

// The plan that steps the engine under its current settings.  Rooms go first: turning them off
// returns to the per-env plan computed earlier (or the create plan), never to a fresh one.
static const StepPlan& plan(const ffm_engine* e) {
    if (rooms_on(e)) return e->room_plan;
    if (pep_on(e)) return e->pep_kernel == 1 ? e->pep_group_plan : e->pep_plan;
    return e->create_plan;
}
static bool created_on(const ffm_engine* e, StepPlan::Kernel k) { return e->create_plan.kernel == k; }

// Counter slots the plan's launches add to: one per wave of a grid (per block of the block
// kernel's), the step shards a range each.
static size_t plan_slots(const StepPlan& p) {
    size_t n = (size_t)p.blocks * (p.kernel == StepPlan::kBlock ? 1 : 4);
    if (!p.shards.empty()) n = std::max(n, p.shards.back().ctr0 + (size_t)p.shards.back().blocks * 4);
    return n;
}

// Blocks per CU of the group kernel's largest grid (engine create, group_plan).
constexpr int kGroupGridPerCu = 8;

// A persistent grid for `units` (envs, env pairs or groups, one per wave at a time, 4 waves per
// block): min(ceil(units / 4), cus * per_cu) blocks.  FFM_WAVE_BLOCKS=<n> overrides the residency
// cap (diagnostic; read at create and when a form's geometry is taken).  per_wave > 0: the units a
// wave can step in one launch (its deferred-reset mask); beyond that the grid grows past one
// resident wave of blocks.
static int persistent_grid(long long units, int cus, int per_cu, long long per_wave = 0) {
    const long long full = (units + 3) / 4;
    long long b = std::max<long long>(1, std::min<long long>(full, (long long)cus * std::max(1, per_cu)));
    if (const char* ov = std::getenv("FFM_WAVE_BLOCKS")) {
        const long long v = std::atoll(ov);
        if (v > 0) b = std::min<long long>(v, full);
    }
    if (per_wave > 0) b = std::max<long long>(b, (units + 4 * per_wave - 1) / (4 * per_wave));
    return (int)b;
}

// The arguments the kernels' occupancy queries read, for the form that the tables name (envp set:
// the per-env form; rooms and room_of_env set as well: the room form) at F free cells (the LDS sizes).
static ffm::CoreStepArgs form_args(const ffm_engine* e, int F, const ffm::EnvParams* envp = nullptr,
                                   const unsigned char* rooms = nullptr, const int32_t* room_of_env = nullptr) {
    ffm::CoreStepArgs a{};
    a.H = e->d.H; a.W = e->d.W; a.A = e->d.agent_capacity; a.F = F;
    a.auto_reset = e->d.auto_reset && !e->mt;
    a.envp = envp; a.rooms = rooms; a.room_of_env = room_of_env;
    return a;
}

// The lane kernel's persistent grid, of the form `a` names.
static int lane_grid(const ffm_engine* e, const ffm::CoreStepArgs& a) {
    return persistent_grid((e->d.n_envs + 1) / 2, e->cus, ffm::core_lane_blocks_per_cu(a, e->d.neighborhood),
                           ffm::core_lane_max_pairs_per_wave());
}

// A plan of a kernel without group state: the grid only.
static StepPlan simple_plan(const ffm_engine* e, StepPlan::Kernel kernel, int blocks) {
    StepPlan p;
    p.kernel = kernel;
    p.blocks = blocks;
    p.stage = e->d_stage;
    return p;
}
static int block_grid(const ffm_engine* e) { return (int)((e->d.n_envs + e->K - 1) / e->K); }

// The placement's candidate count M and key threshold for N agents on F free cells (wave_reset.h):
// about M = N + max(8, (N + 1) / 2) of the F keys fall below thr = floor(M * 2^32 / F), 48 for 32
// agents.  FFM_RESET_CANDIDATES=<M> overrides M (A/B switch, read at create and when records are
// built; 0: rank every key).  The division is done here, once: in the kernel it would be a loop
// invariant that every wave sets up.
static uint32_t placement_threshold(int N, int F, int* m_out = nullptr) {
    int M = std::min(F, N + std::max(8, (N + 1) / 2));
    if (const char* ov = std::getenv("FFM_RESET_CANDIDATES")) M = std::max(0, std::min(F, std::atoi(ov)));
    if (m_out) *m_out = M;
    return M == 0 ? 0u : M == F ? 0xFFFFFFFFu : (uint32_t)(((uint64_t)M << 32) / (uint64_t)F);
}

// The wave reset's LDS for F free cells and n agents (launch_core_reset's carve, core_step.hip).
static size_t wave_reset_lds(int F, int n) {
    auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return al16(8 * (size_t)std::max(1, F)) + al16(2 * (size_t)std::max(1, n)) + al16(2 * (size_t)std::max(1, F));
}

// The free cells of a row-major H x W map as padded indices (x + 1)(W + 2) + y + 1 and, if asked
// for, as row-major ones.  False: a free cell on the border.  The reference indexes neighbours
// without bounds checks (model/ffm_core.py:45,52): agents must never stand on the outer ring.
static bool scan_free(const uint8_t* map, int H, int W, std::vector<uint16_t>* padded, std::vector<uint16_t>* rowmajor = nullptr) {
    for (int i = 0; i < H * W; i++) {
        const int x = i / W, y = i % W;
        if (map[i] != 0) continue;
        if (x == 0 || y == 0 || x == H - 1 || y == W - 1) return false;
        padded->push_back((uint16_t)((x + 1) * (W + 2) + y + 1));
        if (rowmajor) rowmajor->push_back((uint16_t)i);
    }
    return true;
}
static const char* const kBorderError = "free cell on the map border (walls must enclose the room)";

// Upper bound of FFM_STEP_SHARDS: the caller's stream + 3 of the engine's (a process has 4
// hardware queues by default; more streams than queues only serialise).
static constexpr int kMaxStepShards = 4;
// Default shard count where sharding engages (65,536 envs: 2 shards 26.9 us per step, 3 and 4
// shards 27.2 - 27.3, one launch 33.9; profiles/step_shards/).
// Shard 0 runs on the caller's stream, so the engine owns at most 3 streams.
static constexpr int kDefaultStepShards = 2;

// d_ephist: the histogram, then (on a 128-byte boundary) the summary's slots (kernels.h).
static size_t ep_sum_offset(int bins) { return ((size_t)bins + 15) & ~(size_t)15; }
static size_t ep_stats_words(int bins) { return ep_sum_offset(bins) + (size_t)ffm::kEpSumSlots * ffm::kEpSumStride; }

// Field statistics on: the observer follows every step launch, and d_ep_start stays.
static bool field_stats_on(const ffm_engine* e) { return e->d_fs_tab != nullptr; }
static size_t fs_stride(const ffm_engine* e) { return (size_t)e->HW + 2 * (size_t)e->fs_bins + 1; }
// Exit flow on: the flow kernel follows every step launch, and d_ep_start stays.
static bool exit_flow_on(const ffm_engine* e) { return e->d_xf_tab != nullptr; }
static size_t xf_words(const ffm_engine* e) { return (size_t)e->xf_classes * e->xf_doors * (1 + (size_t)e->xf_bins); }
// Motion statistics on: the motion kernel follows every step launch, and d_ep_start stays.
static bool motion_stats_on(const ffm_engine* e) { return e->d_mo_tab != nullptr; }
static size_t mo_stride(const ffm_engine* e) { return ffm::core_motion_stride(e->HW, e->d.neighborhood, e->mo_bins); }
// Each follows every step launch with a kernel of its own, which keeps the engine off the fused path.
static bool observers_on(const ffm_engine* e) { return field_stats_on(e) || exit_flow_on(e) || motion_stats_on(e); }

// ep_start_too: unless the field statistics, the exit flow or the motion statistics still need it.
static void free_episode_log(ffm_engine* e, bool ep_start_too) {
    (void)hipFree(e->d_eplog);
    (void)hipFree(e->d_eplog_n);
    (void)hipFree(e->d_ephist);
    e->d_eplog = nullptr;
    e->d_eplog_n = nullptr;
    e->d_ephist = nullptr;
    e->eplog_cap = 0;
    e->ephist_bins = 0;
    if (ep_start_too && !observers_on(e)) {
        (void)hipFree(e->d_ep_start);
        e->d_ep_start = nullptr;
    }
}

// The snapshot of pos, cnt and ep_start: the exit flow's and the motion statistics'.
static void free_snapshot(ffm_engine* e) {
    void* bufs[] = {e->d_prev_pos, e->d_prev_cnt, e->d_prev_start};
    for (void* p : bufs) (void)hipFree(p);
    e->d_prev_pos = nullptr;
    e->d_prev_cnt = nullptr;
    e->d_prev_start = nullptr;
}

// (the snapshot too, unless the motion statistics still need it)
static void free_exit_flow(ffm_engine* e) {
    void* bufs[] = {e->d_xf_tab, e->d_xf_cls, e->d_xf_door_from};
    for (void* p : bufs) (void)hipFree(p);
    e->d_xf_tab = nullptr;
    e->d_xf_cls = nullptr;
    e->d_xf_door_from = nullptr;
    if (!motion_stats_on(e)) free_snapshot(e);
    e->xf_classes = e->xf_doors = e->xf_bins = e->xf_slots = e->xf_blocks = e->xf_rooms = 0;
    e->xf_lds = false;
    e->xf_door_of_cell.clear();
}

// (the snapshot too, unless the exit flow still needs it)
static void free_motion_stats(ffm_engine* e) {
    void* bufs[] = {e->d_mo_tab, e->d_mo_cls, e->d_mo_dir_from, e->d_origin, e->d_origin_for};
    for (void* p : bufs) (void)hipFree(p);
    e->d_origin_for = nullptr;
    e->d_mo_tab = nullptr;
    e->d_mo_cls = nullptr;
    e->d_mo_dir_from = nullptr;
    e->d_origin = nullptr;
    if (!exit_flow_on(e)) free_snapshot(e);
    e->mo_classes = e->mo_bins = e->mo_slots = e->mo_blocks = e->mo_rooms = 0;
    e->mo_lds = false;
}

static void free_field_stats(ffm_engine* e) {
    (void)hipFree(e->d_fs_tab);
    (void)hipFree(e->d_fs_cls);
    e->d_fs_tab = nullptr;
    e->d_fs_cls = nullptr;
    e->fs_classes = e->fs_bins = e->fs_slots = e->fs_blocks = e->fs_run = 0;
    e->fs_lds = false;
}

// A plan of the group kernel: envs per group, the one-launch grid and the step shards (empty: one
// launch per step), from the resident blocks of the kernel form `a` names (a.envp set: the per-env
// form; a.rooms set: the room form), with the stage image and the FFM_GROUP_ONE setting it launches with.
// The room form is the single-group form only and not persistent, so every launch holds a wave
// per group, ceil(groups / 4) blocks: neither the residency cap nor FFM_WAVE_BLOCKS applies (a
// wave without a group skips the step).
static StepPlan group_plan(const ffm_engine* e, const ffm::CoreStepArgs& a, const unsigned char* stage, bool one) {
    const int nb = e->d.neighborhood, cus = e->cus;
    const long long n_envs = e->d.n_envs;
    const bool room = a.rooms != nullptr;
    StepPlan p;
    p.kernel = StepPlan::kGroup;
    p.stage = stage;
    p.one = one || room;
    // The grid of a launch of n envs: a wave per group up to kGroupGridPerCu blocks per CU
    // (2,048 on MI355X: each of the headline's two shards of 8,192 groups then takes the
    // single-group form, whose 56 VGPRs and 22.4 KB of LDS keep 7 blocks per CU
    // resident; profiles/one_group/), the persistent loop beyond; every wave steps at most
    // core_group_max_iters() groups (its deferred-reset mask).
    auto group_grid = [&](long long n, int G) {
        const long long groups = (n + G - 1) / G;
        if (room) return (int)std::max<long long>(1, (groups + 3) / 4);
        return persistent_grid(groups, cus, kGroupGridPerCu, ffm::core_group_max_iters());
    };
    p.g = ffm::core_group_pick_envs(a, nb, n_envs, cus);
    p.blocks = group_grid(n_envs, p.g);

    // Step shards.  FFM_STEP_SHARDS=1..4 forces the count (A/B switch, read at create and when
    // a form's geometry is taken);
    // unset, kDefaultStepShards shards wherever the one-launch grid has its waves step two
    // or more groups (on MI355X from 24,577 envs on; two shards measured faster from
    // 8,192 envs on, but below that size the engine keeps the single launch its callers
    // and the geometry tests know).  Every shard launches the persistent grid its env
    // count would get alone: the shards alternate on the GPU, and the slots a draining
    // launch frees take the next shard's blocks (1 / S of the resident blocks per shard
    // measured slower: profiles/step_shards/).
    // The rule counts with the loop form's resident blocks, at most 6 (6 waves per SIMD) per CU,
    // as the group-size picker does (as a one-launch grid, 7 per CU stepped slower and so did
    // fewer than 6: profiles/r06/c2/ab_grid_balance*.log, ab_occupancy7.log).
    int S = kDefaultStepShards;
    const long long groups = (n_envs + p.g - 1) / p.g;
    const int per_cu = std::max(1, ffm::core_group_blocks_per_cu(a, nb, p.g));
    if (groups <= (long long)cus * std::min(per_cu, 6) * 4) S = 1;
    if (const char* ov = std::getenv("FFM_STEP_SHARDS")) {
        const int v = std::atoi(ov);
        if (v >= 1 && v <= kMaxStepShards) S = v;
    }
    if (S > 1) {
        // contiguous shards whose boundaries are multiples of 8 envs: only the last can
        // hold a partial group, whose stores land in the arrays' zeroed padding
        // (core_group.hip); empty shards are skipped
        const long long per = ((n_envs + S - 1) / S + 7) & ~7ll;
        size_t ctr0 = 0;
        for (long long e0 = 0; e0 < n_envs; e0 += per) {
            StepPlan::Shard sh;
            sh.e0 = e0;
            sh.n = std::min<long long>(per, n_envs - e0);
            sh.g = ffm::core_group_pick_envs(a, nb, sh.n, cus);
            sh.blocks = group_grid(sh.n, sh.g);
            sh.ctr0 = ctr0;           // a slot range per shard: never contended on the device
            ctr0 += (size_t)sh.blocks * 4;
            p.shards.push_back(sh);
        }
        if (p.shards.size() <= 1) p.shards.clear();
    }
    return p;
}

// The shards' streams (shard 0 runs on the caller's) and the fork / join events, for n shards;
// what exists already is kept.
static hipError_t ensure_shard_streams(ffm_engine* e, size_t n) {
    hipError_t he = hipSuccess;
    if (n > 1 && !e->sh_fork) he = hipEventCreateWithFlags(&e->sh_fork, hipEventDisableTiming);
    for (size_t i = 0; he == hipSuccess && i + 1 < n; i++) {
        if (!e->sh_stream[i]) he = hipStreamCreateWithFlags(&e->sh_stream[i], hipStreamNonBlocking);
        if (he == hipSuccess && !e->sh_end[i]) he = hipEventCreateWithFlags(&e->sh_end[i], hipEventDisableTiming);
    }
    return he;
}

static void free_capture(ffm_engine* e) {
    void* bufs[] = {(void*)e->cap.envs, (void*)e->cap.phase, e->cap.state, e->cap.meta, e->cap.cells, e->cap.n};
    for (void* p : bufs) (void)hipFree(p);
    e->cap = ffm::CoreCapture{};
}

extern "C" {

const char* ffm_last_error(void) { return g_err.c_str(); }
int ffm_abi_version(void) { return FFM_ABI_VERSION; }

static void release(ffm_engine* e) {
    if (!e) return;
    for (int i = 0; i < 3; i++) {
        if (e->sh_stream[i]) {
            (void)hipStreamSynchronize(e->sh_stream[i]);
            (void)hipStreamDestroy(e->sh_stream[i]);
        }
        if (e->sh_end[i]) (void)hipEventDestroy(e->sh_end[i]);
    }
    if (e->sh_fork) (void)hipEventDestroy(e->sh_fork);
    (void)hipFree(e->d_map);
    (void)hipFree(e->d_sff);
    (void)hipFree(e->d_free);
    (void)hipFree(e->d_free_padded);
    (void)hipFree(e->d_stage);
    (void)hipFree(e->d_stage_raw);
    (void)hipFree(e->d_pos);
    (void)hipFree(e->d_cnt);
    (void)hipFree(e->d_dff);
    (void)hipFree(e->d_tmp);
    (void)hipFree(e->d_eps);
    (void)hipFree(e->d_ctr);
    (void)hipFree(e->d_mt_np);
    (void)hipFree(e->d_mt_py);
    (void)hipFree(e->d_dbg);
    (void)hipFree(e->d_scratch);
    (void)hipFree(e->d_envp);
    (void)hipFree(e->d_rooms);
    (void)hipFree(e->d_room_of_env);
    free_capture(e);
    free_field_stats(e);
    free_exit_flow(e);
    free_motion_stats(e);
    free_episode_log(e, true);
    delete e;
}

int ffm_engine_create(const ffm_engine_desc* desc, ffm_engine** out) {
    if (!desc || !out) return fail(FFM_E_INVALID, "null argument");
    *out = nullptr;
    const ffm_engine_desc& d = *desc;
    if (d.abi_version != FFM_ABI_VERSION) return fail(FFM_E_INVALID, "abi_version mismatch");
    if (d.variant != FFM_VARIANT_CORE) return fail(FFM_E_UNSUPPORTED, "only FFM_VARIANT_CORE is built");
    // Positions are u16 cell indices with 0xFFFF = none; a free cell is never on the
    // border, so up to 65,536 cells (256 x 256) every stored cell is < 0xFFFF.
    if (d.H < 3 || d.W < 3 || (long long)d.H * d.W > 65536)
        return fail(FFM_E_INVALID, "map must be at least 3x3 and at most 65536 cells");
    // the kernels divide padded cell indices (< (H + 2)(W + 2)) by W and W + 2 by multiply-high
    if (!ffm::magic_div_ok((uint64_t)(d.H + 2) * (d.W + 2), (uint32_t)d.W + 2u))
        return fail(FFM_E_INVALID, "map too large for the kernels' magic divisors");
    if (!d.map || !d.sff) return fail(FFM_E_INVALID, "map and sff are required");
    if (d.neighborhood != 4 && d.neighborhood != 8) return fail(FFM_E_INVALID, "neighborhood must be 4 or 8");
    if (d.sff_dtype != FFM_SFF_F32 && d.sff_dtype != FFM_SFF_F64) return fail(FFM_E_INVALID, "sff_dtype");
    if (d.n_envs < 1) return fail(FFM_E_INVALID, "n_envs must be >= 1");
    // the block kernel's grid codes hold a 15-bit agent index
    if (d.agent_capacity < 1 || d.agent_capacity > 32767) return fail(FFM_E_INVALID, "agent_capacity");
    if (d.n_agents < 0 || d.n_agents > d.agent_capacity) return fail(FFM_E_INVALID, "n_agents > agent_capacity");
    if (d.rng_mode != FFM_RNG_PHILOX && d.rng_mode != FFM_RNG_MT) return fail(FFM_E_INVALID, "rng_mode");
    const int H = d.H, W = d.W, HW = H * W;
    std::vector<uint16_t> fl, fp;   // the free list, row-major and as padded indices
    if (!scan_free(d.map, H, W, &fp, &fl)) return fail(FFM_E_INVALID, kBorderError);
    if (d.n_agents > (int)fl.size())
        return fail(FFM_E_INVALID, "Cannot take a larger sample than population when 'replace=False'");

    ffm_engine* e = new ffm_engine();
    e->d = d;
    e->d.map = nullptr;
    e->d.sff = nullptr;
    e->HW = HW;
    e->map0.resize((size_t)HW);
    for (int i = 0; i < HW; i++) e->map0[(size_t)i] = d.map[i] == 0 ? 0 : d.map[i] == 3 ? 3 : 2;
    e->F = (int)fl.size();
    e->reset_thr = placement_threshold(d.n_agents, e->F, &e->reset_m);
    e->f64 = d.sff_dtype == FFM_SFF_F64;
    e->mt = d.rng_mode == FFM_RNG_MT;
    // NumPy weak-scalar promotion (NEP 50): python numbers become float32 next
    // to a float32 array (model/ffm_core.py:77,109,113).
    e->kS32 = (float)(-d.k_S);
    e->kD32 = (float)d.k_D;
    e->kS64 = -d.k_S;
    e->c0 = (float)((1.0 - d.decay) * (1.0 - d.diffuse));
    e->c1 = (float)(d.decay * (1.0 - d.diffuse) / (double)d.neighborhood);

    auto cleanup = [&](int rc) {
        release(e);
        return rc;
    };
    hipError_t he = hipSetDevice(d.device);
    if (he != hipSuccess) return cleanup(fail(FFM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he)));

    // Kernel choice.  Small envs (A <= 64, float32 SFF): one wave per env or
    // env pair, persistent grid.  Otherwise (or when envs_per_block > 0 forces
    // it): K envs per workgroup, LDS-bounded.
    const int A = d.agent_capacity;
    const bool reset_lds = !e->mt && d.auto_reset;
    const int EW = A <= 32 ? 2 : 1;
    // envs_per_block: 0 = auto (lane kernel, else wave kernel, where they fit; else
    // block kernel), > 0 = block kernel with that many envs per workgroup,
    // -1 = wave kernel, -2 = lane kernel, -3 = group kernel.
    const bool lane_ok = !e->mt && !e->f64 && A <= 32 && W % 4 == 0 && HW <= 256 &&
                         ((long long)d.n_envs + 7) * HW * 4 < (1ll << 31);   // 32-bit buffer offsets (padded envs)
    e->lane_ok = lane_ok;
    const bool group = (d.envs_per_block == 0 || d.envs_per_block == -3) && lane_ok && ffm::core_group_supported(H, W) &&
                       ffm::core_group_smem_bytes(H, W, e->F, 4) <= 64 * 1024;
    e->multi = lane_ok && ffm::core_multi_smem_bytes(H, W, e->F, 4) <= 64 * 1024;
    const bool lane = !group && (d.envs_per_block == 0 || d.envs_per_block == -2) && lane_ok &&
                      ffm::core_lane_smem_bytes(H, W, e->F, 4) <= 64 * 1024;
    const bool wave = !lane && !group && (d.envs_per_block == 0 || d.envs_per_block == -1) && A <= 64 && !e->f64 && W % 4 == 0 && EW * HW <= 512 &&
                      ffm::core_wave_smem_bytes(H, W, A, e->F, e->mt, reset_lds, 4) <= 64 * 1024;
    e->block = A > 256 ? 512 : 256;
    if (const char* bs = getenv("FFM_BLOCK_BS"))     // A/B switch: the block kernel's workgroup size
        if (atoi(bs) == 256 || atoi(bs) == 512) e->block = atoi(bs);
    int K = d.envs_per_block > 0 ? d.envs_per_block : std::max(1, 256 / A);
    if (e->mt) K = 1;
    while (K > 1 && ffm::core_block_smem_bytes(H, W, A, K, e->F, e->f64, e->mt, reset_lds) > 64 * 1024) K--;
    e->K = K;
    // Maps whose env state exceeds the LDS, or whose padded cell indices exceed u16:
    // the block kernel keeps grid, DFF tile, cell lists and placement keys in a
    // global scratch region per block (one env per block).
    e->big = !wave && !lane && !group &&
             ((size_t)(H + 2) * (W + 2) > 65535 ||
              ffm::core_block_smem_bytes(H, W, A, K, e->F, e->f64, e->mt, reset_lds) > 64 * 1024);
    if (e->big) e->K = 1;
    // Philox placement of the whole free list in the wave reset's LDS, else by blocks
    e->block_reset = !e->mt && wave_reset_lds(e->F, d.n_agents) > 64 * 1024;

    const size_t E = (size_t)d.n_envs;
    const int PW = W + 2, PHW = (H + 2) * PW;
    const size_t sff_bytes = (size_t)PHW * (e->f64 ? 8 : 4);
    // Padded copies (one halo cell each side): map codes normalised to
    // 0 free / 2 blocked / 3 exit (only ==0 and ==3 matter, model/ffm_core.py:52-53,66,101).
    std::vector<uint8_t> pmap((size_t)PHW, 2);
    std::vector<double> psff64((size_t)PHW, 0.0);
    std::vector<float> psff32((size_t)PHW, 0.0f);
    for (int x = 0; x < H; x++)
        for (int y = 0; y < W; y++) {
            const int i = x * W + y, p = (x + 1) * PW + y + 1;
            pmap[p] = d.map[i] == 0 ? 0 : d.map[i] == 3 ? 3 : 2;
            if (e->f64) psff64[p] = reinterpret_cast<const double*>(d.sff)[i];
            else psff32[p] = reinterpret_cast<const float*>(d.sff)[i];
        }
#define ALLOC(p, n)                                                                                   \
    do {                                                                                              \
        he = hipMalloc((void**)&(p), (n));                                                            \
        if (he != hipSuccess) return cleanup(fail(FFM_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(he))); \
    } while (0)
    ALLOC(e->d_map, (size_t)PHW);
    ALLOC(e->d_sff, sff_bytes);
    ALLOC(e->d_free, std::max<size_t>(1, fl.size()) * 2);
    ALLOC(e->d_free_padded, std::max<size_t>(1, fl.size()) * 2);
    if (group) {
        e->stage_bytes = ffm::core_group_stage_bytes(H, W, e->F);
        e->stage_q4 = ffm::core_group_stage_q4(H, W, e->F);
        ALLOC(e->d_stage, e->stage_bytes);
    }
    // pos / cnt / DFF hold whole groups of 8 envs (zeroed padding beyond n_envs): the group kernel
    // reads and writes a partial last group through whole-array buffer resources (core_group.hip)
    const size_t Ep = (E + 7) & ~(size_t)7;
    // + a tail pad: the lane kernel streams positions as dwords, and the group kernel's position
    // load spans G * 64 bytes from its group's base whatever A is (a group holds G * A * 2), so
    // with few agents the last group's load reaches past Ep * A * 2 -- by at most 8 * 64 bytes
    const size_t pos_bytes = Ep * A * 2 + 512;
    ALLOC(e->d_pos, pos_bytes);
    ALLOC(e->d_cnt, Ep * 4);
    ALLOC(e->d_dff, Ep * HW * 4);
    ALLOC(e->d_eps, E * 4);
    if (e->big || e->block_reset) {
        e->scratch_stride = (ffm::core_big_scratch_bytes(H, W, A, e->F, e->mt) + 255) & ~(size_t)255;
        ALLOC(e->d_scratch, E * e->scratch_stride);
    }
    // The create plan.  Persistent wave, lane and multi-step kernels: CUs x resident blocks per CU.
    he = hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, d.device);
    if (he != hipSuccess) return cleanup(fail(FFM_E_HIP, "hipDeviceGetAttribute"));
    {
        const ffm::CoreStepArgs a = form_args(e, e->F);
        if (group) {
            // FFM_GROUP_ONE=0|1 (A/B and test switch, read at create): 0 keeps the loop form of
            // the group kernel on every grid; unset or 1, a launch whose waves step at most one
            // group each takes the single-group form (core_group.hip, ONE)
            const char* ov = std::getenv("FFM_GROUP_ONE");
            e->create_plan = group_plan(e, a, e->d_stage, !ov || std::atoi(ov) != 0);
        } else if (lane) {
            e->create_plan = simple_plan(e, StepPlan::kLane, lane_grid(e, a));
        } else if (wave) {
            e->create_plan = simple_plan(e, StepPlan::kWave,
                                         persistent_grid((d.n_envs + EW - 1) / EW, e->cus,
                                                         ffm::core_wave_blocks_per_cu(a, d.neighborhood, e->mt)));
        } else {
            e->create_plan = simple_plan(e, StepPlan::kBlock, block_grid(e));
        }
        if (e->multi)
            e->multi_blocks = persistent_grid((d.n_envs + 1) / 2, e->cus, ffm::core_multi_blocks_per_cu(a, d.neighborhood));
    }
    // One counter slot per wave (wave / lane / group kernel) or block (block kernel):
    // summed by ffm_engine_get_counters, never contended on the device.
    {
        const long long groups = (d.n_envs + EW - 1) / EW;
        const long long blocks = (d.n_envs + K - 1) / K;
        e->ctr_slots = (size_t)std::max<long long>(std::max<long long>(std::max<long long>(1, blocks), (groups + 3) / 4 * 4),
                                                   (long long)e->multi_blocks * 4);
        e->ctr_slots = std::max(e->ctr_slots, plan_slots(e->create_plan));
    }
    // the shards' streams (shard 0 runs on the caller's) and the fork / join events
    he = ensure_shard_streams(e, e->create_plan.shards.size());
    if (he != hipSuccess) return cleanup(fail(FFM_E_HIP, std::string("step shard streams: ") + hipGetErrorString(he)));
    ALLOC(e->d_ctr, e->ctr_slots * 32);
    ALLOC(e->d_dbg, 16 * 8);
    if (e->mt) {
        ALLOC(e->d_mt_np, E * 625 * 4);
        ALLOC(e->d_mt_py, E * 625 * 4);
    }
#undef ALLOC
    he = hipMemcpy(e->d_map, pmap.data(), PHW, hipMemcpyHostToDevice);
    if (he == hipSuccess)
        he = hipMemcpy(e->d_sff, e->f64 ? (const void*)psff64.data() : (const void*)psff32.data(), sff_bytes,
                       hipMemcpyHostToDevice);
    if (he == hipSuccess && !fl.empty()) he = hipMemcpy(e->d_free, fl.data(), fl.size() * 2, hipMemcpyHostToDevice);
    if (he == hipSuccess && !fl.empty()) he = hipMemcpy(e->d_free_padded, fp.data(), fp.size() * 2, hipMemcpyHostToDevice);
    if (he == hipSuccess && group) {
        // the map, the SFF term, k_S and the free list have no setter: the image is final
        std::vector<unsigned char> img(e->stage_bytes);
        ffm::core_group_stage_build(H, W, e->F, pmap.data(), psff32.data(), e->kS32, fp.data(), img.data());
        he = hipMemcpy(e->d_stage, img.data(), img.size(), hipMemcpyHostToDevice);
    }
    if (he == hipSuccess) he = hipMemset(e->d_pos, 0xFF, pos_bytes);
    if (he == hipSuccess) he = hipMemset(e->d_cnt, 0, Ep * 4);
    if (he == hipSuccess) he = hipMemset(e->d_dff, 0, Ep * HW * 4);
    if (he == hipSuccess) he = hipMemset(e->d_eps, 0, E * 4);
    if (he == hipSuccess) he = hipMemset(e->d_ctr, 0, e->ctr_slots * 32);
    if (he == hipSuccess) he = hipMemset(e->d_dbg, 0, 128);
    if (he == hipSuccess && e->mt) he = hipMemset(e->d_mt_np, 0, E * 625 * 4);
    if (he == hipSuccess && e->mt) he = hipMemset(e->d_mt_py, 0, E * 625 * 4);
    if (he != hipSuccess) return cleanup(fail(FFM_E_HIP, std::string("init: ") + hipGetErrorString(he)));
    *out = e;
    return FFM_OK;
}

int ffm_engine_destroy(ffm_engine* e) {
    if (!e) return FFM_OK;
    (void)hipSetDevice(e->d.device);
    (void)hipDeviceSynchronize();
    release(e);
    return FFM_OK;
}

static ffm::CoreStepArgs make_args(ffm_engine* e) {
    ffm::CoreStepArgs a{};
    a.mW = ffm::magic_div((uint32_t)e->d.W);
    a.mPW = ffm::magic_div((uint32_t)e->d.W + 2u);
    a.H = e->d.H;
    a.W = e->d.W;
    a.HW = e->HW;
    a.A = e->d.agent_capacity;
    a.K = e->K;
    a.E = e->d.n_envs;
    a.env_base = e->d.env_base;
    a.pos = e->d_pos;
    a.cnt = e->d_cnt;
    a.dff = e->d_dff;
    a.episodes = e->d_eps;
    a.counters = e->d_ctr;
    a.pmap = e->d_map;
    a.psff = e->d_sff;
    a.kS32 = e->kS32;
    a.kD32 = e->kD32;
    a.kS64 = e->kS64;
    a.c0 = e->c0;
    a.c1 = e->c1;
    a.key0 = (uint32_t)e->d.seed;
    a.key1 = (uint32_t)(e->d.seed >> 32);
    a.t = e->t;
    a.auto_reset = e->d.auto_reset && !e->mt;
    a.N = e->d.n_agents;
    a.free_list = e->d_free;
    a.free_padded = e->d_free_padded;
    a.F = rooms_on(e) ? e->room_fmax : e->F;   // per-env rooms: the largest room's (the LDS sizes)
    a.reset_thr = e->reset_thr;
    a.stage = plan(e).stage;   // (the group kernel's per-env form: the image that leaves k_S to the records)
    a.stage_q4 = e->stage_q4;
    a.mt_np = e->d_mt_np;
    a.mt_py = e->d_mt_py;
    a.dbg = e->d_dbg;
    a.scratch = e->big ? e->d_scratch : nullptr;
    a.scratch_stride = e->scratch_stride;
    a.ep_start = e->d_ep_start;
    a.eplog = e->d_eplog;
    a.eplog_n = e->d_eplog_n;
    a.eplog_cap = e->eplog_cap;
    a.ephist = e->d_ephist;
    a.ephist_bins = e->ephist_bins;
    a.epsum = e->d_ephist ? e->d_ephist + ep_sum_offset(e->ephist_bins) : nullptr;
    a.envp = e->d_envp;
    a.rooms = e->d_rooms;
    a.room_of_env = e->d_room_of_env;
    a.room_stride = (int)e->room_stride;
    return a;
}

// The field statistics' observer (core_observe.hip) after the step launch `a` describes: that
// launch's envs (e0: its first env, for the class array), its step index, its stream.
static hipError_t launch_observer(const ffm_engine* e, const ffm::CoreStepArgs& a, long long e0, hipStream_t s) {
    ffm::ObserveArgs o{};
    o.pos = a.pos;
    o.cnt = a.cnt;
    o.ep_start = a.ep_start;
    o.cls = e->d_fs_cls ? e->d_fs_cls + e0 : nullptr;
    o.tab = e->d_fs_tab;
    o.E = a.E;
    o.A = a.A;
    o.HW = a.HW;
    o.bins = e->fs_bins;
    o.C = e->fs_classes;
    o.S = (int)fs_stride(e);
    o.slots = e->fs_slots;
    o.t = a.t;
    o.run = e->fs_run;
    return ffm::launch_core_observe(o, e->fs_lds, e->fs_blocks, s);
}

// The exit flow's kernel (core_flow.hip) after the step launch `a` describes: that launch's envs
// (e0: its first env, for the class array and the snapshot), its step index, its stream.
static hipError_t launch_flow(const ffm_engine* e, const ffm::CoreStepArgs& a, long long e0, hipStream_t s) {
    ffm::FlowArgs f{};
    f.pos = a.pos;
    f.cnt = a.cnt;
    f.ep_start = a.ep_start;
    f.prev_pos = e->d_prev_pos + e0 * a.A;
    f.prev_cnt = e->d_prev_cnt + e0;
    f.prev_start = e->d_prev_start + e0;
    f.cls = e->d_xf_cls ? e->d_xf_cls + e0 : nullptr;
    f.room_of_env = a.room_of_env;
    f.door_from = e->d_xf_door_from;
    f.tab = e->d_xf_tab;
    f.E = a.E;
    f.A = a.A;
    f.HW = a.HW;
    f.R = e->xf_rooms;
    f.bins = e->xf_bins;
    f.C = e->xf_classes;
    f.D = e->xf_doors;
    f.slots = e->xf_slots;
    f.t = a.t;
    return ffm::launch_core_flow(f, e->xf_lds, e->xf_blocks, s);
}

// The motion statistics' kernel (core_motion.hip) after the step launch `a` describes, as
// launch_flow; before the flow's, and carrying the snapshot forward only where the flow is off.
static hipError_t launch_motion(const ffm_engine* e, const ffm::CoreStepArgs& a, long long e0, hipStream_t s) {
    ffm::MotionArgs m{};
    m.pos = a.pos;
    m.cnt = a.cnt;
    m.ep_start = a.ep_start;
    m.prev_pos = e->d_prev_pos + e0 * a.A;
    m.prev_cnt = e->d_prev_cnt + e0;
    m.prev_start = e->d_prev_start + e0;
    m.origin = e->d_origin + e0 * a.A;
    m.origin_for = e->d_origin_for + e0;
    m.cls = e->d_mo_cls ? e->d_mo_cls + e0 : nullptr;
    m.room_of_env = a.room_of_env;
    m.dir_from = e->d_mo_dir_from;
    m.tab = e->d_mo_tab;
    m.E = a.E;
    m.A = a.A;
    m.HW = a.HW;
    m.W = e->d.W;
    m.R = e->mo_rooms;
    m.bins = e->mo_bins;
    m.C = e->mo_classes;
    m.NB = e->d.neighborhood;
    m.slots = e->mo_slots;
    m.carry = exit_flow_on(e) ? 0 : 1;
    m.t = a.t;
    return ffm::launch_core_motion(m, e->mo_lds, e->mo_blocks, s);
}

// The snapshot invariant of the exit flow and the motion statistics: whoever writes pos, cnt or
// ep_start ends with this, on the same stream (the flow kernel, or without it the motion kernel,
// carries the snapshot forward itself).  Whole arrays: the envs a call left alone hold equal data
// already.  Nothing while both features are off.
static hipError_t refresh_flow_snapshot(ffm_engine* e, hipStream_t s) {
    if (!exit_flow_on(e) && !motion_stats_on(e)) return hipSuccess;
    const size_t Ep = ((size_t)e->d.n_envs + 7) & ~(size_t)7;
    hipError_t he = hipMemcpyAsync(e->d_prev_pos, e->d_pos, Ep * e->d.agent_capacity * 2, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(e->d_prev_cnt, e->d_cnt, Ep * 4, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(e->d_prev_start, e->d_ep_start, Ep * 4, hipMemcpyDeviceToDevice, s);
    return he;
}

// Shards a step(n > 1) call runs as, under the engine's current settings: 1 (one launch per
// step over all envs) with trajectory capture on (its kernel follows every step launch on the
// caller's stream), on the fused multi-step path and with per-env parameters on the lane kernel
// (only plans of the group kernel hold shards; its per-env and room forms hold their own).
// Field statistics, the exit flow and the motion statistics keep the shards (their kernels follow
// each shard's launch on that shard's stream) and keep the engine off the fused path.
static int shards_in_effect(const ffm_engine* e) {
    const size_t S = plan(e).shards.size();
    if (S <= 1 || e->cap.n_sel != 0 || (e->fused > 1 && e->multi && !rooms_on(e) && !observers_on(e))) return 1;
    return (int)S;
}

// n_steps steps as one launch per step and shard.  One fork and one join per call: the shard
// streams wait for what the caller's stream holds so far, the launches go out step-major (so
// the queues fill evenly from this one thread), and the caller's stream waits for every
// shard's last launch.  In between the shards drift freely: step t + 1 of a shard needs step t
// of that shard only (envs are independent, every draw is keyed by (t, global env)).  Whatever
// else the engine enqueues uses the caller's stream and is ordered by the join.
static int step_sharded(ffm_engine* e, int32_t n_steps, hipStream_t s) {
    const StepPlan& p = plan(e);
    const size_t S = p.shards.size();
    const int A = e->d.agent_capacity;
    HIP_TRY(hipEventRecord(e->sh_fork, s));
    for (size_t k = 1; k < S; k++) HIP_TRY(hipStreamWaitEvent(e->sh_stream[k - 1], e->sh_fork, 0));
    const ffm::CoreStepArgs base = make_args(e);
    hipError_t he = hipSuccess;
    int done = 0;
    for (; done < n_steps && he == hipSuccess; done++) {
        for (size_t k = 0; k < S && he == hipSuccess; k++) {
            const StepPlan::Shard& sh = p.shards[k];
            ffm::CoreStepArgs a = base;
            a.t = e->t + (uint32_t)done;
            a.E = sh.n;
            a.env_base = base.env_base + sh.e0;
            a.pos = base.pos + sh.e0 * A;
            a.cnt = base.cnt + sh.e0;
            a.dff = base.dff + sh.e0 * e->HW;
            a.episodes = base.episodes + sh.e0;
            if (base.ep_start) a.ep_start = base.ep_start + sh.e0;   // records carry global ids through env_base
            if (base.envp) a.envp = base.envp + sh.e0;
            if (base.room_of_env) a.room_of_env = base.room_of_env + sh.e0;
            a.counters = base.counters + 4 * sh.ctr0;
            a.no_step_count = k != 0;   // one shard per step counts the step
            he = ffm::launch_core_group(a, e->d.neighborhood, sh.blocks, k ? e->sh_stream[k - 1] : s, sh.g, p.one);
            // the shards add to the same slot copies: every add to them is an atomic
            if (he == hipSuccess && field_stats_on(e)) he = launch_observer(e, a, sh.e0, k ? e->sh_stream[k - 1] : s);
            if (he == hipSuccess && motion_stats_on(e)) he = launch_motion(e, a, sh.e0, k ? e->sh_stream[k - 1] : s);
            if (he == hipSuccess && exit_flow_on(e)) he = launch_flow(e, a, sh.e0, k ? e->sh_stream[k - 1] : s);
        }
    }
    // the join also after a failed launch: what was enqueued stays ordered before the caller's next work
    hipError_t hj = hipSuccess;
    for (size_t k = 1; k < S; k++) {
        hipError_t h1 = hipEventRecord(e->sh_end[k - 1], e->sh_stream[k - 1]);
        if (h1 == hipSuccess) h1 = hipStreamWaitEvent(s, e->sh_end[k - 1], 0);
        if (h1 != hipSuccess) hj = h1;
    }
    if (he != hipSuccess) return fail(FFM_E_HIP, std::string("launch_core_group (step shard): ") + hipGetErrorString(he));
    e->t += (uint32_t)n_steps;
    if (hj != hipSuccess) return fail(FFM_E_HIP, std::string("step shard join: ") + hipGetErrorString(hj));
    return FFM_OK;
}

int ffm_engine_step(ffm_engine* e, int32_t n_steps, void* stream) {
    if (!e || n_steps < 0) return fail(FFM_E_INVALID, "bad engine/n_steps");
    hipStream_t s = (hipStream_t)stream;
    if (e->fused > 1 && e->multi && e->cap.n_sel == 0 && !rooms_on(e) && !observers_on(e)) {
        // k steps per launch, the state of each env pair on chip (core_multi.hip)
        for (int done = 0; done < n_steps;) {
            const int k = std::min(e->fused, n_steps - done);
            ffm::CoreStepArgs a = make_args(e);
            HIP_TRY(ffm::launch_core_multi(a, e->d.neighborhood, k, e->multi_blocks, s));
            e->t += (uint32_t)k;
            done += k;
        }
        return FFM_OK;
    }
    if (shards_in_effect(e) > 1 && n_steps > 1) {
        // a stream under capture keeps today's single launch per step (no fork into streams
        // the capture does not know)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
            (void)hipGetLastError();
            cs = hipStreamCaptureStatusActive;
        }
        if (cs == hipStreamCaptureStatusNone) return step_sharded(e, n_steps, s);
    }
    const StepPlan& p = plan(e);
    for (int i = 0; i < n_steps; i++) {
        ffm::CoreStepArgs a = make_args(e);
        switch (p.kernel) {
        case StepPlan::kGroup: HIP_TRY(ffm::launch_core_group(a, e->d.neighborhood, p.blocks, s, p.g, p.one)); break;
        case StepPlan::kLane: HIP_TRY(ffm::launch_core_lane(a, e->d.neighborhood, p.blocks, s)); break;
        case StepPlan::kWave: HIP_TRY(ffm::launch_core_wave(a, e->d.neighborhood, e->mt, p.blocks, s)); break;
        case StepPlan::kBlock: HIP_TRY(ffm::launch_core_block(a, e->d.neighborhood, e->f64, e->mt, e->block, s)); break;
        }
        if (e->cap.n_sel) HIP_TRY(ffm::launch_core_capture(a, e->cap, s));
        if (field_stats_on(e)) HIP_TRY(launch_observer(e, a, 0, s));
        if (motion_stats_on(e)) HIP_TRY(launch_motion(e, a, 0, s));
        if (exit_flow_on(e)) HIP_TRY(launch_flow(e, a, 0, s));
        e->t++;
    }
    return FFM_OK;
}

int ffm_engine_set_fused_steps(ffm_engine* e, int32_t k) {
    if (!e || k < 1) return fail(FFM_E_INVALID, "fused steps must be >= 1");
    e->fused = k;
    return FFM_OK;
}

int ffm_engine_reset(ffm_engine* e, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)e->d.n_envs;
    HIP_TRY(hipMemsetAsync(e->d_dff, 0, E * e->HW * 4, s));
    HIP_TRY(hipMemsetAsync(e->d_cnt, 0, E * 4, s));
    HIP_TRY(hipMemsetAsync(e->d_pos, 0xFF, E * e->d.agent_capacity * 2, s));
    HIP_TRY(hipMemsetAsync(e->d_eps, 0, E * 4, s));   // episodes count from this reset
    if (e->mt) {   // the caller uploads positions drawn from its own MT stream
        if (e->cap.n_sel) HIP_TRY(ffm::launch_core_capture_init(make_args(e), e->cap, s));
        return FFM_OK;
    }
    // Philox placement, same stream as the in-kernel auto-reset (key: current t).
    if (e->block_reset) {
        ffm::CoreStepArgs a = make_args(e);
        a.scratch = e->d_scratch;
        HIP_TRY(ffm::launch_core_block_reset(a, s));
    } else {
        HIP_TRY(ffm::launch_core_reset(make_args(e), s));
    }
    e->t++;
    if (e->cap.n_sel) HIP_TRY(ffm::launch_core_capture_init(make_args(e), e->cap, s));
    HIP_TRY(refresh_flow_snapshot(e, s));
    // motion statistics: no origin row is of the episodes just placed (ep_start is the index consumed
    // above), whatever the step index was set to before the call
    if (motion_stats_on(e))
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)e->d_origin_for, (int)(e->t - 2u), ((size_t)E + 7) & ~(size_t)7, s));
    return FFM_OK;
}

int ffm_engine_reset_envs(ffm_engine* e, const uint8_t* mask, void* stream) {
    if (!e || !mask) return fail(FFM_E_INVALID, "null engine or mask");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "reset_envs: MT mode places agents on the host (set_state)");
    hipStream_t s = (hipStream_t)stream;
    // the masked envs only: Philox placement keyed by the current t (as ffm_engine_reset),
    // DFF row zeroed, count = N; the episode counters are left alone (not an episode end)
    if (e->block_reset) {
        ffm::CoreStepArgs a = make_args(e);
        a.scratch = e->d_scratch;
        HIP_TRY(ffm::launch_core_block_reset(a, s, mask));
    } else {
        HIP_TRY(ffm::launch_core_reset(make_args(e), s, mask));
    }
    e->t++;
    // trajectory capture: the masked envs' rows count from this placement (same episode index),
    // and one that had emptied logs again; nothing is launched while capture is off
    if (e->cap.n_sel) HIP_TRY(ffm::launch_core_capture_init(make_args(e), e->cap, s, mask));
    HIP_TRY(refresh_flow_snapshot(e, s));
    return FFM_OK;
}

int ffm_engine_update_dff(ffm_engine* e, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)e->d.n_envs * e->HW;
    if (!e->d_tmp) HIP_TRY(hipMalloc((void**)&e->d_tmp, n * 4));
    if (e->d_envp)
        HIP_TRY(ffm::launch_update_dff_env(e->d_dff, e->d_tmp, e->d.n_envs, e->d.H, e->d.W, e->d.neighborhood,
                                           e->d_envp, s));
    else
        HIP_TRY(ffm::launch_update_dff(e->d_dff, e->d_tmp, e->d.n_envs, e->d.H, e->d.W, e->d.neighborhood, e->c0,
                                       e->c1, s));
    HIP_TRY(hipMemcpyAsync(e->d_dff, e->d_tmp, n * 4, hipMemcpyDeviceToDevice, s));
    return FFM_OK;
}

static int check_range(ffm_engine* e, int64_t env0, int64_t n) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (env0 < 0 || n < 0 || env0 + n > e->d.n_envs) return fail(FFM_E_INVALID, "env range out of bounds");
    return FFM_OK;
}

int ffm_engine_set_state(ffm_engine* e, int64_t env0, int64_t n, const uint16_t* positions,
                         const int32_t* counts, const float* dff, void* stream) {
    int rc = check_range(e, env0, n);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int A = e->d.agent_capacity;
    if (counts) {
        for (int64_t i = 0; i < n; i++)
            if (counts[i] < 0 || counts[i] > A) return fail(FFM_E_INVALID, "count out of [0, agent_capacity]");
    }
    if (positions && counts) {
        // Positions must be distinct passable, non-exit cells (the reference never
        // holds an agent on an exit: model/ffm_core.py:101-102).
        const int PW = e->d.W + 2, PHW = (e->d.H + 2) * PW;
        std::vector<uint8_t> pmap(PHW);
        HIP_TRY(hipMemcpy(pmap.data(), e->d_map, PHW, hipMemcpyDeviceToHost));
        std::vector<uint8_t> seen(e->HW, 0);
        for (int64_t i = 0; i < n; i++) {
            for (int j = 0; j < counts[i]; j++) {
                const uint16_t c = positions[i * A + j];
                // per-env rooms: the env's own room's map
                if (c >= e->HW || (rooms_on(e) ? e->room_maps[(size_t)e->room_of_env[(size_t)(env0 + i)] * e->HW + c]
                                               : pmap[(c / e->d.W + 1) * PW + c % e->d.W + 1]) != 0)
                    return fail(FFM_E_INVALID, "agent on a non-free cell");
                if (seen[c]) return fail(FFM_E_INVALID, "two agents on one cell");
                seen[c] = 1;
            }
            for (int j = 0; j < counts[i]; j++) seen[positions[i * A + j]] = 0;
        }
    }
    if (positions)
        HIP_TRY(hipMemcpyAsync(e->d_pos + env0 * A, positions, (size_t)n * A * 2, hipMemcpyHostToDevice, s));
    if (counts) HIP_TRY(hipMemcpyAsync(e->d_cnt + env0, counts, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (dff)
        HIP_TRY(hipMemcpyAsync(e->d_dff + env0 * e->HW, dff, (size_t)n * e->HW * 4, hipMemcpyHostToDevice, s));
    if (positions || counts) HIP_TRY(refresh_flow_snapshot(e, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

int ffm_engine_get_state(ffm_engine* e, int64_t env0, int64_t n, uint16_t* positions, int32_t* counts,
                         float* dff, void* stream) {
    int rc = check_range(e, env0, n);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int A = e->d.agent_capacity;
    if (positions)
        HIP_TRY(hipMemcpyAsync(positions, e->d_pos + env0 * A, (size_t)n * A * 2, hipMemcpyDeviceToHost, s));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, e->d_cnt + env0, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (dff)
        HIP_TRY(hipMemcpyAsync(dff, e->d_dff + env0 * e->HW, (size_t)n * e->HW * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

int ffm_engine_set_mt_state(ffm_engine* e, int64_t env, const uint32_t* np_key, int32_t np_pos,
                            const uint32_t* py_key, int32_t py_pos, void* stream) {
    int rc = check_range(e, env, 1);
    if (rc) return rc;
    if (!e->mt) return fail(FFM_E_INVALID, "engine is not in MT mode");
    if (np_pos < 0 || np_pos > 624 || py_pos < 0 || py_pos > 624) return fail(FFM_E_INVALID, "MT position");
    hipStream_t s = (hipStream_t)stream;
    uint32_t buf[1250];
    std::memcpy(buf, np_key, 624 * 4);
    buf[624] = (uint32_t)np_pos;
    std::memcpy(buf + 625, py_key, 624 * 4);
    buf[1249] = (uint32_t)py_pos;
    HIP_TRY(hipMemcpyAsync(e->d_mt_np + env * 625, buf, 625 * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->d_mt_py + env * 625, buf + 625, 625 * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

int ffm_engine_get_mt_state(ffm_engine* e, int64_t env, uint32_t* np_key, int32_t* np_pos, uint32_t* py_key,
                            int32_t* py_pos, void* stream) {
    int rc = check_range(e, env, 1);
    if (rc) return rc;
    if (!e->mt) return fail(FFM_E_INVALID, "engine is not in MT mode");
    hipStream_t s = (hipStream_t)stream;
    uint32_t buf[1250];
    HIP_TRY(hipMemcpyAsync(buf, e->d_mt_np + env * 625, 625 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(buf + 625, e->d_mt_py + env * 625, 625 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(np_key, buf, 624 * 4);
    *np_pos = (int32_t)buf[624];
    std::memcpy(py_key, buf + 625, 624 * 4);
    *py_pos = (int32_t)buf[1249];
    return FFM_OK;
}

int ffm_engine_set_trajectory_capture(ffm_engine* e, const int32_t* envs, const int32_t* phases, int32_t n_sel,
                                      int32_t period, int64_t capacity_rows, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (n_sel < 0 || (n_sel > 0 && (!envs || period < 1 || capacity_rows < 1)))
        return fail(FFM_E_INVALID, "trajectory capture: envs, period >= 1 and capacity_rows >= 1 are required");
    for (int32_t i = 0; i < n_sel; i++) {
        if (envs[i] < 0 || envs[i] >= e->d.n_envs) return fail(FFM_E_INVALID, "trajectory capture: env out of range");
        if (phases && phases[i] < 0) return fail(FFM_E_INVALID, "trajectory capture: phase must be >= 0");
    }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));        // queued steps may still write the old buffers
    free_capture(e);
    if (n_sel == 0) return FFM_OK;
    ffm::CoreCapture& c = e->cap;
    const size_t A = (size_t)e->d.agent_capacity;
    int* de = nullptr; int* dp = nullptr;
    hipError_t he = hipMalloc((void**)&de, (size_t)n_sel * 4);
    if (he == hipSuccess && phases) he = hipMalloc((void**)&dp, (size_t)n_sel * 4);
    c.envs = de; c.phase = dp;
    if (he == hipSuccess) he = hipMalloc((void**)&c.state, (size_t)n_sel * 12);
    if (he == hipSuccess) he = hipMalloc((void**)&c.meta, (size_t)capacity_rows * 16);
    if (he == hipSuccess) he = hipMalloc((void**)&c.cells, (size_t)capacity_rows * A * 2);
    if (he == hipSuccess) he = hipMalloc((void**)&c.n, 8);
    if (he != hipSuccess) {
        free_capture(e);
        return fail(FFM_E_NOMEM, std::string("trajectory capture: ") + hipGetErrorString(he));
    }
    c.cap = capacity_rows; c.period = period;
    HIP_TRY(hipMemcpyAsync(de, envs, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
    if (dp) HIP_TRY(hipMemcpyAsync(dp, phases, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c.n, 0, 8, s));
    c.n_sel = n_sel;
    HIP_TRY(ffm::launch_core_capture_init(make_args(e), c, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

int ffm_engine_drain_trajectory(ffm_engine* e, int32_t* meta, uint16_t* cells, int64_t cap, int64_t* n,
                                int64_t* dropped, void* stream) {
    if (!e || !n) return fail(FFM_E_INVALID, "null argument");
    *n = 0;
    if (dropped) *dropped = 0;
    if (e->cap.n_sel == 0) return FFM_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, e->cap.n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const long long have = std::min<long long>((long long)c, e->cap.cap);
    if (have > cap) {
        *n = have;
        return fail(FFM_E_INVALID, "drain_trajectory: buffer too small (*n holds the count)");
    }
    const size_t A = (size_t)e->d.agent_capacity;
    if (have > 0 && meta) HIP_TRY(hipMemcpyAsync(meta, e->cap.meta, (size_t)have * 16, hipMemcpyDeviceToHost, s));
    if (have > 0 && cells) HIP_TRY(hipMemcpyAsync(cells, e->cap.cells, (size_t)have * A * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(e->cap.n, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = have;
    if (dropped) *dropped = (int64_t)c - have;
    return FFM_OK;
}

// The statistics' empty state is all zeros (the min is kept inverted).
static hipError_t clear_episode_stats(ffm_engine* e, hipStream_t s) {
    return hipMemsetAsync(e->d_ephist, 0, ep_stats_words(e->ephist_bins) * 8, s);
}

int ffm_engine_set_episode_log(ffm_engine* e, int64_t capacity_records, int32_t hist_bins, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "episode log: Philox engines only");
    if (capacity_records < 0 || hist_bins < 0) return fail(FFM_E_INVALID, "episode log: negative capacity or bins");
    if (e->d.env_base < 0 || e->d.env_base + e->d.n_envs > (int64_t)INT32_MAX)
        return fail(FFM_E_INVALID, "episode log: env_base + n_envs must fit int32 (records hold global env ids)");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));        // queued steps may still write the old buffers
    const bool off = capacity_records == 0 && hist_bins == 0;
    free_episode_log(e, off);   // (ep_start stays while the field statistics are on)
    if (off) return FFM_OK;
    hipError_t he = hipSuccess;
    const bool fresh = e->d_ep_start == nullptr;
    const size_t Ep = ((size_t)e->d.n_envs + 7) & ~(size_t)7;   // padded like d_cnt
    if (fresh) he = hipMalloc((void**)&e->d_ep_start, Ep * 4);
    if (he == hipSuccess && capacity_records > 0) {
        he = hipMalloc((void**)&e->d_eplog, (size_t)capacity_records * 16);
        if (he == hipSuccess) he = hipMalloc((void**)&e->d_eplog_n, 8);
    }
    if (he == hipSuccess && hist_bins > 0) he = hipMalloc((void**)&e->d_ephist, ep_stats_words(hist_bins) * 8);
    if (he != hipSuccess) {
        free_episode_log(e, true);
        return fail(FFM_E_NOMEM, std::string("episode log: ") + hipGetErrorString(he));
    }
    e->eplog_cap = e->d_eplog ? capacity_records : 0;
    e->ephist_bins = e->d_ephist ? hist_bins : 0;
    // Turned on mid-run: episodes in flight count from here.  The next step is keyed e->t, so
    // the index that "placed" every env is the one before it (a reset overwrites it anyway).
    if (fresh) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)e->d_ep_start, (int)(e->t - 1u), Ep, s));
    if (e->d_eplog_n) HIP_TRY(hipMemsetAsync(e->d_eplog_n, 0, 8, s));
    if (e->d_ephist) HIP_TRY(clear_episode_stats(e, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

int ffm_engine_drain_episodes(ffm_engine* e, int32_t* records, int64_t cap, int64_t* n, int64_t* dropped,
                              void* stream) {
    if (!e || !n) return fail(FFM_E_INVALID, "null argument");
    *n = 0;
    if (dropped) *dropped = 0;
    if (!e->d_eplog) return FFM_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, e->d_eplog_n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const long long have = std::min<long long>((long long)c, e->eplog_cap);
    if (have > cap || (have > 0 && !records)) {
        *n = have;
        return fail(FFM_E_INVALID, "drain_episodes: buffer too small (*n holds the count)");
    }
    if (have > 0) HIP_TRY(hipMemcpyAsync(records, e->d_eplog, (size_t)have * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(e->d_eplog_n, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = have;
    if (dropped) *dropped = (int64_t)c - have;
    return FFM_OK;
}

int ffm_engine_get_episode_stats(ffm_engine* e, uint64_t* hist, int32_t bins, uint64_t* summary, int32_t clear,
                                 void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (hist && bins != e->ephist_bins) return fail(FFM_E_INVALID, "episode stats: bins differs from the histogram's");
    if (summary) std::memset(summary, 0, 5 * sizeof(uint64_t));
    if (!e->d_ephist) return FFM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hist) HIP_TRY(hipMemcpyAsync(hist, e->d_ephist, (size_t)bins * 8, hipMemcpyDeviceToHost, s));
    std::vector<unsigned long long> slots((size_t)ffm::kEpSumSlots * ffm::kEpSumStride);
    if (summary)
        HIP_TRY(hipMemcpyAsync(slots.data(), e->d_ephist + ep_sum_offset(e->ephist_bins), slots.size() * 8,
                               hipMemcpyDeviceToHost, s));
    if (clear) HIP_TRY(clear_episode_stats(e, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (summary) {
        unsigned long long inv_min = 0;
        for (int j = 0; j < ffm::kEpSumSlots; j++) {
            const unsigned long long* q = slots.data() + (size_t)j * ffm::kEpSumStride;
            summary[0] += q[0];
            summary[1] += q[1];
            summary[2] += q[2];
            inv_min = std::max(inv_min, q[3]);
            summary[4] = std::max<uint64_t>(summary[4], q[4]);
        }
        summary[3] = summary[0] ? ~inv_min : 0;   // no episode yet: min reads 0
    }
    return FFM_OK;
}

// A/B switch of the field statistics with a positive integer value (read when the feature is set).
static int fs_env_int(const char* name, int dflt, int lo, int hi) {
    if (const char* ov = std::getenv(name)) {
        const int v = std::atoi(ov);
        if (v >= lo && v <= hi) return v;
    }
    return dflt;
}

int ffm_engine_set_field_stats(ffm_engine* e, const int32_t* class_of_env, int32_t n_classes, int32_t curve_bins,
                               void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "field statistics: Philox engines only");
    if (n_classes < 0 || curve_bins < 0) return fail(FFM_E_INVALID, "field statistics: negative class or bin count");
    hipStream_t s = (hipStream_t)stream;
    if (n_classes == 0) {
        HIP_TRY(hipStreamSynchronize(s));    // queued observers may still write the tables
        free_field_stats(e);
        if (!e->d_eplog && !e->d_ephist) free_episode_log(e, true);   // ep_start: the log is off too
        return FFM_OK;
    }
    const size_t E = (size_t)e->d.n_envs;
    if (class_of_env)
        for (size_t i = 0; i < E; i++)
            if (class_of_env[i] < 0 || class_of_env[i] >= n_classes)
                return fail(FFM_E_INVALID, "field statistics: class_of_env entry outside [0, n_classes)");
    // one copy of the tables as u64, against FFM_FIELD_STATS_MAX_BYTES
    const size_t S = (size_t)e->HW + 2 * (size_t)curve_bins + 1;
    const size_t words = (size_t)n_classes * S;
    if (words * 8 > (size_t)FFM_FIELD_STATS_MAX_BYTES)
        return fail(FFM_E_INVALID, "field statistics: n_classes * (H * W + 2 * curve_bins + 1) * 8 exceeds "
                                   "FFM_FIELD_STATS_MAX_BYTES");
    // The form.  FFM_FIELD_STATS_FORM=lds|global forces one (A/B and test switch, read here).
    const int blocks = fs_env_int("FFM_FIELD_STATS_BLOCKS", ffm::kObserveMaxBlocks, 1, 65535);
    const int run = fs_env_int("FFM_FIELD_STATS_RUN", ffm::core_observe_run(e->d.agent_capacity), 1, 4096);
    const bool fits = words * 4 <= ffm::kObserveLdsBudget &&
                      ffm::core_observe_lds_safe(e->d.n_envs, e->d.agent_capacity, run, blocks);
    bool lds = fits;
    if (const char* ov = std::getenv("FFM_FIELD_STATS_FORM")) {
        if (!std::strcmp(ov, "lds")) {
            if (!fits) return fail(FFM_E_INVALID, "field statistics: FFM_FIELD_STATS_FORM=lds, but the tables exceed the LDS budget");
            lds = true;
        } else if (!std::strcmp(ov, "global")) {
            lds = false;
        }
    }
    // slot copies: a power of two, fewer where the copies together would pass the limit
    int slots = 1;
    while (slots * 2 <= fs_env_int("FFM_FIELD_STATS_SLOTS", ffm::kObserveSlots, 1, 1024)) slots *= 2;
    while (slots > 1 && words * 8 * (size_t)slots > (size_t)FFM_FIELD_STATS_MAX_BYTES) slots /= 2;

    HIP_TRY(hipStreamSynchronize(s));        // queued observers may still write the old tables
    // Build into locals; the engine changes after the last call that can fail.
    unsigned long long* tab = nullptr;
    int32_t* cls = nullptr;
    uint32_t* ep_start = nullptr;
    const bool fresh = e->d_ep_start == nullptr;
    const size_t Ep = (E + 7) & ~(size_t)7;   // padded like d_cnt
    hipError_t he = hipMalloc((void**)&tab, words * 8 * (size_t)slots);
    if (he == hipSuccess && class_of_env) he = hipMalloc((void**)&cls, E * 4);
    if (he == hipSuccess && fresh) he = hipMalloc((void**)&ep_start, Ep * 4);
    const bool nomem = he != hipSuccess;
    if (he == hipSuccess) he = hipMemsetAsync(tab, 0, words * 8 * (size_t)slots, s);
    if (he == hipSuccess && cls) he = hipMemcpyAsync(cls, class_of_env, E * 4, hipMemcpyHostToDevice, s);
    // Turned on mid-run: episodes in flight count from here, as the episode log's do (the next
    // step is keyed e->t, so the index that "placed" every env is the one before it).
    if (he == hipSuccess && fresh) he = hipMemsetD32Async((hipDeviceptr_t)ep_start, (int)(e->t - 1u), Ep, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) {
        (void)hipFree(tab);
        (void)hipFree(cls);
        (void)hipFree(ep_start);
        return fail(nomem ? FFM_E_NOMEM : FFM_E_HIP, std::string("field statistics: ") + hipGetErrorString(he));
    }
    free_field_stats(e);
    e->d_fs_tab = tab;
    e->d_fs_cls = cls;
    if (fresh) e->d_ep_start = ep_start;
    e->fs_classes = n_classes;
    e->fs_bins = curve_bins;
    e->fs_slots = slots;
    e->fs_blocks = blocks;
    e->fs_run = run;
    e->fs_lds = lds;
    return FFM_OK;
}

int ffm_engine_get_field_stats(ffm_engine* e, uint64_t* occupancy, uint64_t* observed, uint64_t* remaining,
                               uint64_t* alive, int32_t clear, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (!field_stats_on(e)) return fail(FFM_E_INVALID, "field statistics are off");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = fs_stride(e), C = (size_t)e->fs_classes, HW = (size_t)e->HW, bins = (size_t)e->fs_bins;
    const size_t words = C * S;
    std::vector<unsigned long long> h(words * (size_t)e->fs_slots);
    HIP_TRY(hipMemcpyAsync(h.data(), e->d_fs_tab, h.size() * 8, hipMemcpyDeviceToHost, s));
    if (clear) HIP_TRY(hipMemsetAsync(e->d_fs_tab, 0, h.size() * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 1; k < e->fs_slots; k++)
        for (size_t i = 0; i < words; i++) h[i] += h[(size_t)k * words + i];
    for (size_t c = 0; c < C; c++) {
        const unsigned long long* T = h.data() + c * S;
        if (occupancy) std::copy(T, T + HW, occupancy + c * HW);
        if (remaining) std::copy(T + HW, T + HW + bins, remaining + c * bins);
        if (alive) std::copy(T + HW + bins, T + HW + 2 * bins, alive + c * bins);
        if (observed) observed[c] = T[HW + 2 * bins];
    }
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): the field statistics in effect.
//   out[0] 0 off, 1 the LDS form, 2 the global form;  out[1] blocks of the observer's grid over all
//   envs;  out[2] slot copies of the tables;  out[3] classes;  out[4] curve bins
int ffm_debug_field_stats_info(ffm_engine* e, int32_t* out, int n) {
    if (!e || !out || n < 0 || n > 5) return fail(FFM_E_INVALID, "bad args");
    const bool on = field_stats_on(e);
    const int32_t v[5] = {
        !on ? 0 : e->fs_lds ? 1 : 2,
        on ? ffm::core_observe_grid(e->d.n_envs, e->fs_run, e->fs_blocks) : 0,
        e->fs_slots,
        e->fs_classes,
        e->fs_bins,
    };
    for (int i = 0; i < n; i++) out[i] = v[i];
    return FFM_OK;
}

// The exit cells of room r's map in row-major order numbered 0, 1, ...: the default door labels.
// Returns the room's exit count.
static int default_doors(const uint8_t* map, int HW, int32_t* door_of_cell) {
    int n = 0;
    for (int i = 0; i < HW; i++) door_of_cell[i] = map[i] == 3 ? n++ : -1;
    return n;
}

// door_from of one room (kernels.h FlowArgs): for every free cell the door of the first exit cell
// among its neighbours in the reference's neighbour order (model/ffm_core.py:28-34: Neumann up,
// down, left, right; Moore row-major), 0xFF for none.
static void build_door_from(const uint8_t* map, const int32_t* door_of_cell, int H, int W, int nb, uint8_t* out) {
    static const int dx4[4] = {-1, 1, 0, 0}, dy4[4] = {0, 0, -1, 1};
    static const int dx8[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, dy8[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
    const int* dx = nb == 4 ? dx4 : dx8;
    const int* dy = nb == 4 ? dy4 : dy8;
    for (int x = 0; x < H; x++)
        for (int y = 0; y < W; y++) {
            uint8_t d = 0xFF;
            if (map[x * W + y] == 0)
                for (int k = 0; k < nb && d == 0xFF; k++) {
                    const int u = x + dx[k], v = y + dy[k];
                    if (u >= 0 && u < H && v >= 0 && v < W && map[u * W + v] == 3) d = (uint8_t)door_of_cell[u * W + v];
                }
            out[x * W + y] = d;
        }
}

int ffm_engine_set_exit_flow(ffm_engine* e, const int32_t* door_of_cell, int32_t n_doors, const int32_t* class_of_env,
                             int32_t n_classes, int32_t curve_bins, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "exit flow: Philox engines only");
    if (n_classes < 0 || curve_bins < 0 || n_doors < 0) return fail(FFM_E_INVALID, "exit flow: negative class, door or bin count");
    hipStream_t s = (hipStream_t)stream;
    if (n_classes == 0) {
        HIP_TRY(hipStreamSynchronize(s));    // queued flow kernels may still write the tables
        free_exit_flow(e);
        if (!e->d_eplog && !e->d_ephist) free_episode_log(e, true);   // ep_start, unless the field statistics need it
        return FFM_OK;
    }
    const size_t E = (size_t)e->d.n_envs;
    const int HW = e->HW, A = e->d.agent_capacity;
    if (class_of_env)
        for (size_t i = 0; i < E; i++)
            if (class_of_env[i] < 0 || class_of_env[i] >= n_classes)
                return fail(FFM_E_INVALID, "exit flow: class_of_env entry outside [0, n_classes)");
    // the doors of every room in effect
    const int R = rooms_on(e) ? (int)e->room_f.size() : 1;
    const uint8_t* maps = rooms_on(e) ? e->room_maps.data() : e->map0.data();
    std::vector<int32_t> doc((size_t)R * HW);
    int D = 0;
    for (int r = 0; r < R; r++) D = std::max(D, default_doors(maps + (size_t)r * HW, HW, doc.data() + (size_t)r * HW));
    if (door_of_cell) {
        if (n_doors < 1) return fail(FFM_E_INVALID, "exit flow: door_of_cell wants n_doors >= 1");
        for (size_t i = 0; i < doc.size(); i++) {
            if (doc[i] < 0) continue;            // only exit cells are read
            if (door_of_cell[i] < 0 || door_of_cell[i] >= n_doors)
                return fail(FFM_E_INVALID, "exit flow: an exit cell's door label outside [0, n_doors)");
            doc[i] = door_of_cell[i];
        }
        D = n_doors;
    }
    D = std::max(D, 1);
    if (D > 255) return fail(FFM_E_INVALID, "exit flow: more than 255 doors");
    // one copy of the tables as u64, against FFM_EXIT_FLOW_MAX_BYTES
    const size_t words = (size_t)n_classes * D * (1 + (size_t)curve_bins);
    if (words * 8 > (size_t)FFM_EXIT_FLOW_MAX_BYTES)
        return fail(FFM_E_INVALID, "exit flow: n_classes * doors * (1 + curve_bins) * 8 exceeds FFM_EXIT_FLOW_MAX_BYTES");
    // The form.  FFM_EXIT_FLOW_FORM=lds|global forces one, FFM_EXIT_FLOW_BLOCKS caps the grid (A/B
    // and test switches, read here).
    const int blocks = fs_env_int("FFM_EXIT_FLOW_BLOCKS", ffm::kFlowMaxBlocks, 1, 65535);
    const bool fits = words * 4 <= ffm::kObserveLdsBudget && ffm::core_flow_lds_safe(e->d.n_envs, A);
    bool lds = fits;
    if (const char* ov = std::getenv("FFM_EXIT_FLOW_FORM")) {
        if (!std::strcmp(ov, "lds")) {
            if (!fits) return fail(FFM_E_INVALID, "exit flow: FFM_EXIT_FLOW_FORM=lds, but the tables exceed the LDS budget");
            lds = true;
        } else if (!std::strcmp(ov, "global")) {
            lds = false;
        }
    }
    int slots = ffm::kFlowSlots;   // a power of two, fewer where the copies together would pass the limit
    while (slots > 1 && words * 8 * (size_t)slots > (size_t)FFM_EXIT_FLOW_MAX_BYTES) slots /= 2;
    std::vector<uint8_t> dfrom((size_t)R * HW);
    for (int r = 0; r < R; r++)
        build_door_from(maps + (size_t)r * HW, doc.data() + (size_t)r * HW, e->d.H, e->d.W, e->d.neighborhood,
                        dfrom.data() + (size_t)r * HW);

    HIP_TRY(hipStreamSynchronize(s));        // queued flow kernels may still write the old tables
    // Build into locals; the engine changes after the last call that can fail.
    unsigned long long* tab = nullptr;
    int32_t* cls = nullptr;
    uint8_t* d_dfrom = nullptr;
    uint16_t* ppos = nullptr;
    int32_t* pcnt = nullptr;
    uint32_t* pstart = nullptr;
    uint32_t* ep_start = nullptr;
    const bool fresh = e->d_ep_start == nullptr;
    const size_t Ep = (E + 7) & ~(size_t)7;   // padded like d_cnt
    hipError_t he = hipMalloc((void**)&tab, words * 8 * (size_t)slots);
    if (he == hipSuccess && class_of_env) he = hipMalloc((void**)&cls, E * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&d_dfrom, dfrom.size());
    if (he == hipSuccess) he = hipMalloc((void**)&ppos, Ep * A * 2 + 512);   // sized like d_pos
    if (he == hipSuccess) he = hipMalloc((void**)&pcnt, Ep * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&pstart, Ep * 4);
    if (he == hipSuccess && fresh) he = hipMalloc((void**)&ep_start, Ep * 4);
    const bool nomem = he != hipSuccess;
    if (he == hipSuccess) he = hipMemsetAsync(tab, 0, words * 8 * (size_t)slots, s);
    if (he == hipSuccess && cls) he = hipMemcpyAsync(cls, class_of_env, E * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_dfrom, dfrom.data(), dfrom.size(), hipMemcpyHostToDevice, s);
    // Turned on mid-run: episodes in flight count from here, as the episode log's do (the next
    // step is keyed e->t, so the index that "placed" every env is the one before it).
    if (he == hipSuccess && fresh) he = hipMemsetD32Async((hipDeviceptr_t)ep_start, (int)(e->t - 1u), Ep, s);
    // the snapshot: the state as it stands
    if (he == hipSuccess) he = hipMemcpyAsync(ppos, e->d_pos, Ep * A * 2, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(pcnt, e->d_cnt, Ep * 4, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(pstart, fresh ? ep_start : e->d_ep_start, Ep * 4, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) {
        void* bufs[] = {tab, cls, d_dfrom, ppos, pcnt, pstart, ep_start};
        for (void* p : bufs) (void)hipFree(p);
        return fail(nomem ? FFM_E_NOMEM : FFM_E_HIP, std::string("exit flow: ") + hipGetErrorString(he));
    }
    free_exit_flow(e);
    free_snapshot(e);                        // (shared with the motion statistics: the new one holds the same state)
    e->d_xf_tab = tab;
    e->d_xf_cls = cls;
    e->d_xf_door_from = d_dfrom;
    e->d_prev_pos = ppos;
    e->d_prev_cnt = pcnt;
    e->d_prev_start = pstart;
    if (fresh) e->d_ep_start = ep_start;
    e->xf_classes = n_classes;
    e->xf_doors = D;
    e->xf_bins = curve_bins;
    e->xf_slots = slots;
    e->xf_blocks = blocks;
    e->xf_rooms = R;
    e->xf_lds = lds;
    e->xf_door_of_cell = std::move(doc);
    return FFM_OK;
}

int ffm_engine_get_exit_flow(ffm_engine* e, uint64_t* exited, uint64_t* outflow, int32_t clear, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (!exit_flow_on(e)) return fail(FFM_E_INVALID, "the exit flow is off");
    hipStream_t s = (hipStream_t)stream;
    const size_t words = xf_words(e), bins = (size_t)e->xf_bins, CD = (size_t)e->xf_classes * e->xf_doors;
    std::vector<unsigned long long> h(words * (size_t)e->xf_slots);
    HIP_TRY(hipMemcpyAsync(h.data(), e->d_xf_tab, h.size() * 8, hipMemcpyDeviceToHost, s));
    if (clear) HIP_TRY(hipMemsetAsync(e->d_xf_tab, 0, h.size() * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 1; k < e->xf_slots; k++)
        for (size_t i = 0; i < words; i++) h[i] += h[(size_t)k * words + i];
    for (size_t cd = 0; cd < CD; cd++) {
        const unsigned long long* T = h.data() + cd * (1 + bins);
        if (exited) exited[cd] = T[0];
        if (outflow) std::copy(T + 1, T + 1 + bins, outflow + cd * bins);
    }
    return FFM_OK;
}

int ffm_engine_get_exit_doors(ffm_engine* e, int32_t* door_of_cell, int32_t* n_doors) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (!exit_flow_on(e)) return fail(FFM_E_INVALID, "the exit flow is off");
    if (door_of_cell) std::copy(e->xf_door_of_cell.begin(), e->xf_door_of_cell.end(), door_of_cell);
    if (n_doors) *n_doors = e->xf_doors;
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): the exit flow in effect.
//   out[0] 0 off, 1 the LDS form, 2 the global form;  out[1] blocks of the flow kernel's grid over
//   all envs;  out[2] slot copies of the tables;  out[3] classes;  out[4] doors;  out[5] curve bins;
//   out[6] rooms of the door table
int ffm_debug_exit_flow_info(ffm_engine* e, int32_t* out, int n) {
    if (!e || !out || n < 0 || n > 7) return fail(FFM_E_INVALID, "bad args");
    const bool on = exit_flow_on(e);
    const int32_t v[7] = {
        !on ? 0 : e->xf_lds ? 1 : 2,
        on ? ffm::core_flow_grid(e->d.n_envs, e->d.agent_capacity, e->xf_blocks) : 0,
        e->xf_slots,
        e->xf_classes,
        e->xf_doors,
        e->xf_bins,
        e->xf_rooms,
    };
    for (int i = 0; i < n; i++) out[i] = v[i];
    return FFM_OK;
}

// dir_from of one room (kernels.h MotionArgs): build_door_from's rule, but the neighbour index of
// the first exit cell instead of its door.
static void build_dir_from(const uint8_t* map, int H, int W, int nb, uint8_t* out) {
    static const int dx4[4] = {-1, 1, 0, 0}, dy4[4] = {0, 0, -1, 1};
    static const int dx8[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, dy8[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
    const int* dx = nb == 4 ? dx4 : dx8;
    const int* dy = nb == 4 ? dy4 : dy8;
    for (int x = 0; x < H; x++)
        for (int y = 0; y < W; y++) {
            uint8_t d = 0xFF;
            if (map[x * W + y] == 0)
                for (int k = 0; k < nb && d == 0xFF; k++) {
                    const int u = x + dx[k], v = y + dy[k];
                    if (u >= 0 && u < H && v >= 0 && v < W && map[u * W + v] == 3) d = (uint8_t)k;
                }
            out[x * W + y] = d;
        }
}

int ffm_engine_set_motion_stats(ffm_engine* e, const int32_t* class_of_env, int32_t n_classes, int32_t curve_bins,
                                void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "motion statistics: Philox engines only");
    if (n_classes < 0 || curve_bins < 0) return fail(FFM_E_INVALID, "motion statistics: negative class or bin count");
    hipStream_t s = (hipStream_t)stream;
    if (n_classes == 0) {
        HIP_TRY(hipStreamSynchronize(s));    // queued motion kernels may still write the tables
        free_motion_stats(e);
        if (!e->d_eplog && !e->d_ephist) free_episode_log(e, true);   // ep_start, unless another observer needs it
        return FFM_OK;
    }
    const size_t E = (size_t)e->d.n_envs;
    const int HW = e->HW, A = e->d.agent_capacity, NB = e->d.neighborhood;
    if (class_of_env)
        for (size_t i = 0; i < E; i++)
            if (class_of_env[i] < 0 || class_of_env[i] >= n_classes)
                return fail(FFM_E_INVALID, "motion statistics: class_of_env entry outside [0, n_classes)");
    // one copy of the tables as u64, against FFM_MOTION_STATS_MAX_BYTES
    const size_t words = (size_t)n_classes * ffm::core_motion_stride(HW, NB, curve_bins);
    if (words * 8 > (size_t)FFM_MOTION_STATS_MAX_BYTES)
        return fail(FFM_E_INVALID, "motion statistics: n_classes * (H * W * (neighbours + 3) + 2 * curve_bins) * 8 exceeds "
                                   "FFM_MOTION_STATS_MAX_BYTES");
    // The form.  FFM_MOTION_STATS_FORM=lds|global forces one, FFM_MOTION_STATS_BLOCKS caps the grid
    // (A/B and test switches, read here).
    const int blocks = fs_env_int("FFM_MOTION_STATS_BLOCKS", ffm::kMotionMaxBlocks, 1, 65535);
    const bool fits = (size_t)n_classes * ffm::core_motion_lds_stride(HW, NB, curve_bins) * 4 <= ffm::kObserveLdsBudget &&
                      ffm::core_motion_lds_safe(e->d.n_envs, A);
    bool lds = fits;
    if (const char* ov = std::getenv("FFM_MOTION_STATS_FORM")) {
        if (!std::strcmp(ov, "lds")) {
            if (!fits) return fail(FFM_E_INVALID, "motion statistics: FFM_MOTION_STATS_FORM=lds, but the tables exceed the LDS budget");
            lds = true;
        } else if (!std::strcmp(ov, "global")) {
            lds = false;
        }
    }
    int slots = ffm::kMotionSlots;   // a power of two, fewer where the copies together would pass the limit
    while (slots > 1 && words * 8 * (size_t)slots > (size_t)FFM_MOTION_STATS_MAX_BYTES) slots /= 2;
    // the direction table of every room in effect
    const int R = rooms_on(e) ? (int)e->room_f.size() : 1;
    const uint8_t* maps = rooms_on(e) ? e->room_maps.data() : e->map0.data();
    std::vector<uint8_t> dfrom((size_t)R * HW);
    for (int r = 0; r < R; r++) build_dir_from(maps + (size_t)r * HW, e->d.H, e->d.W, NB, dfrom.data() + (size_t)r * HW);

    HIP_TRY(hipStreamSynchronize(s));        // queued motion kernels may still write the old tables
    // Build into locals; the engine changes after the last call that can fail.
    unsigned long long* tab = nullptr;
    int32_t* cls = nullptr;
    uint8_t* d_dfrom = nullptr;
    uint16_t* origin = nullptr;
    uint32_t* origin_for = nullptr;
    uint16_t* ppos = nullptr;
    int32_t* pcnt = nullptr;
    uint32_t* pstart = nullptr;
    uint32_t* ep_start = nullptr;
    const bool fresh = e->d_ep_start == nullptr;
    const size_t Ep = (E + 7) & ~(size_t)7;   // padded like d_cnt
    hipError_t he = hipMalloc((void**)&tab, words * 8 * (size_t)slots);
    if (he == hipSuccess && class_of_env) he = hipMalloc((void**)&cls, E * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&d_dfrom, dfrom.size());
    if (he == hipSuccess) he = hipMalloc((void**)&origin, Ep * A * 2 + 512);   // sized like d_pos
    if (he == hipSuccess) he = hipMalloc((void**)&origin_for, Ep * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&ppos, Ep * A * 2 + 512);
    if (he == hipSuccess) he = hipMalloc((void**)&pcnt, Ep * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&pstart, Ep * 4);
    if (he == hipSuccess && fresh) he = hipMalloc((void**)&ep_start, Ep * 4);
    const bool nomem = he != hipSuccess;
    if (he == hipSuccess) he = hipMemsetAsync(tab, 0, words * 8 * (size_t)slots, s);
    if (he == hipSuccess && cls) he = hipMemcpyAsync(cls, class_of_env, E * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_dfrom, dfrom.data(), dfrom.size(), hipMemcpyHostToDevice, s);
    // Turned on mid-run: episodes in flight count from here, as the episode log's do (the next
    // step is keyed e->t, so the index that "placed" every env is the one before it) ...
    if (he == hipSuccess && fresh) he = hipMemsetD32Async((hipDeviceptr_t)ep_start, (int)(e->t - 1u), Ep, s);
    // ... and agents in flight originate where they stand now: rows of the episodes in flight
    if (he == hipSuccess) he = hipMemcpyAsync(origin, e->d_pos, Ep * A * 2, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(origin_for, fresh ? ep_start : e->d_ep_start, Ep * 4, hipMemcpyDeviceToDevice, s);
    // the snapshot: the state as it stands (with the exit flow on, what its snapshot holds already)
    if (he == hipSuccess) he = hipMemcpyAsync(ppos, e->d_pos, Ep * A * 2, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(pcnt, e->d_cnt, Ep * 4, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(pstart, fresh ? ep_start : e->d_ep_start, Ep * 4, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) {
        void* bufs[] = {tab, cls, d_dfrom, origin, origin_for, ppos, pcnt, pstart, ep_start};
        for (void* p : bufs) (void)hipFree(p);
        return fail(nomem ? FFM_E_NOMEM : FFM_E_HIP, std::string("motion statistics: ") + hipGetErrorString(he));
    }
    free_motion_stats(e);
    free_snapshot(e);                        // (shared with the exit flow: the new one holds the same state)
    e->d_mo_tab = tab;
    e->d_mo_cls = cls;
    e->d_mo_dir_from = d_dfrom;
    e->d_origin = origin;
    e->d_origin_for = origin_for;
    e->d_prev_pos = ppos;
    e->d_prev_cnt = pcnt;
    e->d_prev_start = pstart;
    if (fresh) e->d_ep_start = ep_start;
    e->mo_classes = n_classes;
    e->mo_bins = curve_bins;
    e->mo_slots = slots;
    e->mo_blocks = blocks;
    e->mo_rooms = R;
    e->mo_lds = lds;
    return FFM_OK;
}

int ffm_engine_get_motion_stats(ffm_engine* e, uint64_t* flux, uint64_t* present, uint64_t* moved, uint64_t* egress_count,
                                uint64_t* egress_steps, int32_t clear, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (!motion_stats_on(e)) return fail(FFM_E_INVALID, "the motion statistics are off");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = mo_stride(e), C = (size_t)e->mo_classes, HW = (size_t)e->HW, bins = (size_t)e->mo_bins;
    const size_t F = HW * ((size_t)e->d.neighborhood + 1), words = C * S;
    std::vector<unsigned long long> h(words * (size_t)e->mo_slots);
    HIP_TRY(hipMemcpyAsync(h.data(), e->d_mo_tab, h.size() * 8, hipMemcpyDeviceToHost, s));
    if (clear) HIP_TRY(hipMemsetAsync(e->d_mo_tab, 0, h.size() * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 1; k < e->mo_slots; k++)
        for (size_t i = 0; i < words; i++) h[i] += h[(size_t)k * words + i];
    for (size_t c = 0; c < C; c++) {
        const unsigned long long* T = h.data() + c * S;
        if (flux) std::copy(T, T + F, flux + c * F);
        if (present) std::copy(T + F, T + F + bins, present + c * bins);
        if (moved) std::copy(T + F + bins, T + F + 2 * bins, moved + c * bins);
        if (egress_count) std::copy(T + F + 2 * bins, T + F + 2 * bins + HW, egress_count + c * HW);
        if (egress_steps) std::copy(T + F + 2 * bins + HW, T + S, egress_steps + c * HW);
    }
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): the motion statistics in effect.
//   out[0] 0 off, 1 the LDS form, 2 the global form;  out[1] blocks of the motion kernel's grid over
//   all envs;  out[2] slot copies of the tables;  out[3] classes;  out[4] curve bins;  out[5] rooms
//   of the direction table;  out[6] directions per cell (neighbours + 1)
int ffm_debug_motion_stats_info(ffm_engine* e, int32_t* out, int n) {
    if (!e || !out || n < 0 || n > 7) return fail(FFM_E_INVALID, "bad args");
    const bool on = motion_stats_on(e);
    const int32_t v[7] = {
        !on ? 0 : e->mo_lds ? 1 : 2,
        on ? ffm::core_motion_grid(e->d.n_envs, e->d.agent_capacity, e->mo_blocks) : 0,
        e->mo_slots,
        e->mo_classes,
        e->mo_bins,
        e->mo_rooms,
        e->d.neighborhood + 1,
    };
    for (int i = 0; i < n; i++) out[i] = v[i];
    return FFM_OK;
}

// One env's record (kernels.h EnvParams) from its parameter set, with the expressions of
// ffm_engine_create (the same bits as a homogeneous engine).  F: the free cells of the env's room.
static ffm::EnvParams env_record(const ffm_env_params& q, int nb, int F) {
    ffm::EnvParams r{};
    r.kS32 = (float)(-q.k_S);
    r.kD32 = (float)q.k_D;
    r.kS64 = -q.k_S;
    r.c0 = (float)((1.0 - q.decay) * (1.0 - q.diffuse));
    r.c1 = (float)(q.decay * (1.0 - q.diffuse) / (double)nb);
    r.N = q.n_agents;
    r.reset_thr = placement_threshold(q.n_agents, F);
    return r;
}

// The create-time parameters as a set (the records of an engine with rooms but no sets).
static ffm_env_params create_set(const ffm_engine* e) {
    ffm_env_params q{};
    q.k_S = e->d.k_S; q.k_D = e->d.k_D; q.diffuse = e->d.diffuse; q.decay = e->d.decay;
    q.n_agents = e->d.n_agents;
    return q;
}

// Every env's record.  sets == nullptr: the create-time set for every env.  room_f == nullptr: the
// create-time room's F for every env, else room_f[room_of_env[i]].
static std::vector<ffm::EnvParams> env_records(const ffm_engine* e, const ffm_env_params* sets, const int32_t* set_of_env,
                                               const std::vector<int>* room_f, const int32_t* room_of_env) {
    const size_t E = (size_t)e->d.n_envs;
    const ffm_env_params base = create_set(e);
    std::vector<ffm::EnvParams> rec(E);
    for (size_t i = 0; i < E; i++)
        rec[i] = env_record(sets ? sets[set_of_env[i]] : base, e->d.neighborhood,
                            room_f ? (*room_f)[(size_t)room_of_env[i]] : e->F);
    return rec;
}

// The first env whose n_agents exceeds the free cells of its room, or -1 (same arguments).
static long long env_over_capacity(const ffm_engine* e, const ffm_env_params* sets, const int32_t* set_of_env,
                                   const std::vector<int>* room_f, const int32_t* room_of_env) {
    for (long long i = 0; i < e->d.n_envs; i++) {
        const int N = sets ? sets[set_of_env[i]].n_agents : e->d.n_agents;
        if (N > (room_f ? (*room_f)[(size_t)room_of_env[i]] : e->F)) return i;
    }
    return -1;
}

// Rewrites every env's record on stream s, after the steps queued there (which may still read the
// old ones), and waits for it (the off-paths of one feature while the other stays on).
static int rewrite_records(ffm_engine* e, const std::vector<ffm::EnvParams>& rec, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpyAsync(e->d_envp, rec.data(), rec.size() * sizeof(ffm::EnvParams), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FFM_OK;
}

// What the group kernel's per-env form needs beyond the records: its stage image (built once:
// the create-time image with the SFF term's multiplier 1, so the LDS region holds the raw SFF) and
// its plan, sized from that form's occupancy (envp: any non-null pointer, it only selects the
// form).  The caller commits *out to pep_group_plan.
static int pep_group_setup(ffm_engine* e, const ffm::EnvParams* envp, StepPlan* out) {
    const int H = e->d.H, W = e->d.W, PHW = (H + 2) * (W + 2);
    HIP_TRY(hipSetDevice(e->d.device));
    if (!e->d_stage_raw) {
        std::vector<uint8_t> pmap((size_t)PHW);
        std::vector<float> psff((size_t)PHW);
        std::vector<uint16_t> fp((size_t)std::max(1, e->F));
        HIP_TRY(hipMemcpy(pmap.data(), e->d_map, (size_t)PHW, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(psff.data(), e->d_sff, (size_t)PHW * 4, hipMemcpyDeviceToHost));
        if (e->F > 0) HIP_TRY(hipMemcpy(fp.data(), e->d_free_padded, (size_t)e->F * 2, hipMemcpyDeviceToHost));
        std::vector<unsigned char> img(e->stage_bytes);
        ffm::core_group_stage_build(H, W, e->F, pmap.data(), psff.data(), 1.0f, fp.data(), img.data());
        unsigned char* buf = nullptr;
        if (hipMalloc((void**)&buf, e->stage_bytes) != hipSuccess) return fail(FFM_E_NOMEM, "env params: stage image");
        const hipError_t he = hipMemcpy(buf, img.data(), img.size(), hipMemcpyHostToDevice);
        if (he != hipSuccess) {
            (void)hipFree(buf);
            return fail(FFM_E_HIP, std::string("env params: stage image: ") + hipGetErrorString(he));
        }
        e->d_stage_raw = buf;
    }
    StepPlan p = group_plan(e, form_args(e, e->F, envp), e->d_stage_raw, e->create_plan.one);
    // The counter slots were sized at create.  A geometry that needs more (the per-env form
    // resident in other numbers than the create-time form, so another group size or shard count)
    // gives way to the create-time one, which is valid for every form.
    if (plan_slots(p) > e->ctr_slots) {
        p = e->create_plan;
        p.stage = e->d_stage_raw;
    }
    const hipError_t he = ensure_shard_streams(e, p.shards.size());
    if (he != hipSuccess) return fail(FFM_E_HIP, std::string("step shard streams: ") + hipGetErrorString(he));
    *out = std::move(p);
    return FFM_OK;
}

int ffm_engine_set_env_params_kernel(ffm_engine* e, int32_t mode) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (mode != 0 && mode != 1) return fail(FFM_E_INVALID, "env params kernel: mode must be 0 (lane) or 1 (group)");
    if (mode == 1 && (!created_on(e, StepPlan::kGroup) || e->mt))
        return fail(FFM_E_UNSUPPORTED, "env params kernel: the engine was not created on the group kernel");
    if (mode == 1 && pep_on(e) && e->pep_kernel != 1) {   // the feature is on: move it now
        StepPlan p;
        const int rc = pep_group_setup(e, e->d_envp, &p);
        if (rc) return rc;
        e->pep_group_plan = std::move(p);
    }
    e->pep_kernel = mode;
    return FFM_OK;
}

int ffm_engine_set_env_params(ffm_engine* e, const ffm_env_params* sets, int32_t n_sets, const int32_t* set_of_env,
                              void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "env params: Philox engines only");
    if (n_sets < 0 || n_sets > e->d.n_envs) return fail(FFM_E_INVALID, "env params: n_sets must lie in [0, n_envs]");
    hipStream_t s = (hipStream_t)stream;
    if (n_sets == 0) {   // off: the create-time parameters, kernel and launch geometry
        if (!pep_on(e)) return FFM_OK;
        if (rooms_on(e)) {   // the rooms keep a record per env: the create-time values, each room's threshold
            if (env_over_capacity(e, nullptr, nullptr, &e->room_f, e->room_of_env.data()) >= 0)
                return fail(FFM_E_INVALID, "env params: the create-time n_agents exceeds the free cells of an env's room");
            const int rc = rewrite_records(e, env_records(e, nullptr, nullptr, &e->room_f, e->room_of_env.data()), s);
            if (rc) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(s));        // queued steps may still read the records
            (void)hipFree(e->d_envp);
            e->d_envp = nullptr;
        }
        e->pep_sets.clear();
        e->pep_set_of_env.clear();
        e->pep_plan = e->pep_group_plan = StepPlan{};
        return FFM_OK;
    }
    if (!sets || !set_of_env) return fail(FFM_E_INVALID, "env params: sets and set_of_env are required");
    const int A = e->d.agent_capacity;
    for (int32_t p = 0; p < n_sets; p++) {
        const ffm_env_params& q = sets[p];
        if (!std::isfinite(q.k_S) || !std::isfinite(q.k_D) || !std::isfinite(q.diffuse) || !std::isfinite(q.decay))
            return fail(FFM_E_INVALID, "env params: non-finite parameter");
        if (q.n_agents < 1 || q.n_agents > std::min(A, rooms_on(e) ? e->room_fmax : e->F))
            return fail(FFM_E_INVALID, "env params: n_agents must lie in [1, min(agent_capacity, free cells)]");
    }
    const size_t E = (size_t)e->d.n_envs;
    for (size_t i = 0; i < E; i++)
        if (set_of_env[i] < 0 || set_of_env[i] >= n_sets) return fail(FFM_E_INVALID, "env params: set_of_env out of range");
    // per-env rooms: every env's n_agents against the free cells of its own room
    const std::vector<int>* room_f = rooms_on(e) ? &e->room_f : nullptr;
    if (room_f && env_over_capacity(e, sets, set_of_env, room_f, e->room_of_env.data()) >= 0)
        return fail(FFM_E_INVALID, "env params: n_agents exceeds the free cells of an env's room");
    // The kernel while on.  Group engines: the lane kernel (the group kernel's conditions include
    // the lane kernel's); wave engines, and whatever else is not on the lane kernel: the block kernel.
    const bool lane = created_on(e, StepPlan::kLane) ||
                      (created_on(e, StepPlan::kGroup) && ffm::core_lane_smem_bytes(e->d.H, e->d.W, e->F, 4) <= 64 * 1024);
    if (!lane && !e->big &&
        ffm::core_block_smem_bytes(e->d.H, e->d.W, A, e->K, e->F, e->f64, false, e->d.auto_reset != 0) +
                ffm::core_block_pep_smem_bytes(e->K) > 64 * 1024)
        return fail(FFM_E_UNSUPPORTED, "env params: the block kernel's LDS has no room for the K records");
    // The records, with the expressions of ffm_engine_create (the same bits as a homogeneous engine)
    const std::vector<ffm::EnvParams> rec = env_records(e, sets, set_of_env, room_f, e->room_of_env.data());
    HIP_TRY(hipSetDevice(e->d.device));
    ffm::EnvParams* buf = e->d_envp;   // (per-env rooms: the engine's own records are there already)
    if (!buf) {
        hipError_t he = hipMalloc((void**)&buf, E * sizeof(ffm::EnvParams));
        if (he != hipSuccess) return fail(FFM_E_NOMEM, std::string("env params: ") + hipGetErrorString(he));
    }
    auto undo = [&](int rc) {
        if (!e->d_envp) (void)hipFree(buf);
        return rc;
    };
    // the occupancy of the per-env form (buf: any non-null pointer selects it)
    StepPlan pp = lane ? simple_plan(e, StepPlan::kLane, lane_grid(e, form_args(e, e->F, buf)))
                       : simple_plan(e, StepPlan::kBlock, block_grid(e));
    // the group kernel's own per-env form, if that is the engine's setting and the feature is not on it yet
    const bool to_group = e->pep_kernel == 1 && !pep_on(e);
    StepPlan gp;
    if (to_group) {
        const int rc = pep_group_setup(e, buf, &gp);
        if (rc) return undo(rc);
    }
    // stream-ordered after the steps queued so far; the tables are consumed before the return
    hipError_t he = hipMemcpyAsync(buf, rec.data(), E * sizeof(ffm::EnvParams), hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) return undo(fail(FFM_E_HIP, std::string("env params: ") + hipGetErrorString(he)));
    e->d_envp = buf;
    e->pep_sets.assign(sets, sets + n_sets);
    e->pep_set_of_env.assign(set_of_env, set_of_env + E);
    e->pep_plan = std::move(pp);
    if (to_group) e->pep_group_plan = std::move(gp);
    return FFM_OK;
}

int ffm_engine_get_env_params(ffm_engine* e, ffm_env_params* sets, int32_t cap, int32_t* n_sets, int32_t* set_of_env) {
    if (!e || !n_sets || cap < 0) return fail(FFM_E_INVALID, "null argument");
    *n_sets = (int32_t)e->pep_sets.size();
    if (*n_sets == 0) return FFM_OK;
    if (sets) {
        if (cap < *n_sets) return fail(FFM_E_INVALID, "get_env_params: buffer too small (*n_sets holds the count)");
        std::copy(e->pep_sets.begin(), e->pep_sets.end(), sets);
    }
    if (set_of_env) std::copy(e->pep_set_of_env.begin(), e->pep_set_of_env.end(), set_of_env);
    return FFM_OK;
}

int ffm_engine_set_env_rooms(ffm_engine* e, const uint8_t* maps, const float* sffs, int32_t n_rooms,
                             const int32_t* room_of_env, void* stream) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    // the door table is built from the rooms in effect when the flow is set: rooms first, the flow after
    if (exit_flow_on(e)) return fail(FFM_E_INVALID, "env rooms: the exit flow is on (turn it off, set the rooms, set it again)");
    if (motion_stats_on(e)) return fail(FFM_E_INVALID, "env rooms: the motion statistics are on (turn them off, set the rooms, set them again)");
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)e->d.n_envs;
    const bool pep = pep_on(e);
    if (n_rooms == 0) {   // off: the create-time room, kernel and launch geometry
        if (!rooms_on(e)) return FFM_OK;
        if (pep) {   // the sets stay: their records with the create-time room's threshold again
            if (env_over_capacity(e, e->pep_sets.data(), e->pep_set_of_env.data(), nullptr, nullptr) >= 0)
                return fail(FFM_E_INVALID, "env rooms: a parameter set's n_agents exceeds the create-time room's free cells");
            const int rc = rewrite_records(e, env_records(e, e->pep_sets.data(), e->pep_set_of_env.data(), nullptr, nullptr), s);
            if (rc) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(s));
            (void)hipFree(e->d_envp);
            e->d_envp = nullptr;
        }
        (void)hipFree(e->d_rooms);
        (void)hipFree(e->d_room_of_env);
        e->d_rooms = nullptr;
        e->d_room_of_env = nullptr;
        e->room_stride = 0;
        e->room_fmax = 0;
        e->room_plan = StepPlan{};
        e->room_maps.clear();
        e->room_sffs.clear();
        e->room_of_env.clear();
        e->room_f.clear();
        return FFM_OK;
    }
    if (e->mt) return fail(FFM_E_UNSUPPORTED, "env rooms: Philox engines only");
    if (e->f64) return fail(FFM_E_UNSUPPORTED, "env rooms: float32-SFF engines only");
    // the block kernel's room form (mode 1) or the group kernel's (mode 2) where the engine's setting asks
    // for it (ffm_engine_set_env_rooms_kernel, which accepted the engine); else the lane kernel's
    const bool block_form = e->room_kernel == 1, group_form = e->room_kernel == 2;
    if (!block_form && !e->lane_ok)
        return fail(FFM_E_UNSUPPORTED, "env rooms: engines of the lane kernel's shapes only (agent_capacity <= 32, W % 4 == 0, H*W <= 256)");
    if (n_rooms < 1 || n_rooms > e->d.n_envs) return fail(FFM_E_INVALID, "env rooms: n_rooms must lie in [0, n_envs]");
    if (!maps || !sffs || !room_of_env) return fail(FFM_E_INVALID, "env rooms: maps, sffs and room_of_env are required");
    const int H = e->d.H, W = e->d.W, HW = e->HW, PW = W + 2, PHW = (H + 2) * PW;
    // every room's free list, with the checks of ffm_engine_create
    std::vector<std::vector<uint16_t>> fp((size_t)n_rooms);   // padded indices
    std::vector<int> room_f((size_t)n_rooms);
    int fmax = 0;
    for (int32_t r = 0; r < n_rooms; r++) {
        if (!scan_free(maps + (size_t)r * HW, H, W, &fp[(size_t)r])) return fail(FFM_E_INVALID, kBorderError);
        room_f[(size_t)r] = (int)fp[(size_t)r].size();
        fmax = std::max(fmax, room_f[(size_t)r]);
    }
    for (size_t i = 0; i < E; i++)
        if (room_of_env[i] < 0 || room_of_env[i] >= n_rooms) return fail(FFM_E_INVALID, "env rooms: room_of_env out of range");
    if (group_form && std::max(ffm::core_group_smem_bytes(H, W, fmax, 4, 2, true),
                               ffm::core_group_smem_bytes(H, W, fmax, 4, 4, true)) > 64 * 1024)
        return fail(FFM_E_UNSUPPORTED, "env rooms: the group kernel's LDS has no room for the largest room");
    if (!block_form && !group_form && ffm::core_lane_smem_bytes(H, W, fmax, 4, true) > 64 * 1024)
        return fail(FFM_E_UNSUPPORTED, "env rooms: the lane kernel's LDS has no room for the largest room");
    if (block_form) {
        // the block kernel at the create-time K with the largest room's F, the K records and room indices
        if (ffm::core_block_smem_bytes(H, W, e->d.agent_capacity, e->K, fmax, false, false, e->d.auto_reset != 0) +
                ffm::core_block_room_smem_bytes(e->K) > 64 * 1024)
            return fail(FFM_E_UNSUPPORTED, "env rooms: the block kernel's LDS has no room for the largest room and the K records");
        // the placement of the largest room: in the block reset's scratch (sized at create), or in
        // the wave reset's LDS
        if (e->block_reset ? ffm::core_big_scratch_bytes(H, W, e->d.agent_capacity, fmax, false) > e->scratch_stride
                           : wave_reset_lds(fmax, e->d.agent_capacity) > 64 * 1024)
            return fail(FFM_E_UNSUPPORTED, "env rooms: the placement has no room for the largest room's free list");
        if ((size_t)block_grid(e) > e->ctr_slots)
            return fail(FFM_E_UNSUPPORTED, "env rooms: counter slots");
    }
    const ffm_env_params* sets = pep ? e->pep_sets.data() : nullptr;
    const int32_t* set_of_env = pep ? e->pep_set_of_env.data() : nullptr;
    if (env_over_capacity(e, sets, set_of_env, &room_f, room_of_env) >= 0)
        return fail(FFM_E_INVALID, "Cannot take a larger sample than population when 'replace=False' (an env's room "
                                   "has fewer free cells than its n_agents)");
    // the table (kernels.h room_layout) and the records
    const ffm::RoomLayout lay = ffm::room_layout(PHW, fmax);
    std::vector<unsigned char> table((size_t)n_rooms * lay.stride, 0);
    for (int32_t r = 0; r < n_rooms; r++) {
        unsigned char* rec = table.data() + (size_t)r * lay.stride;
        *reinterpret_cast<int32_t*>(rec) = room_f[(size_t)r];
        uint16_t* g = reinterpret_cast<uint16_t*>(rec + lay.grid);
        float* sf = reinterpret_cast<float*>(rec + lay.sff);
        uint16_t* fr = reinterpret_cast<uint16_t*>(rec + lay.free);
        for (int i = 0; i < lay.gs; i++) g[i] = 2;   // halo and padding: blocked
        for (int x = 0; x < H; x++)
            for (int y = 0; y < W; y++) {
                const int i = x * W + y, p = (x + 1) * PW + y + 1;
                const uint8_t c = maps[(size_t)r * HW + i];
                g[p] = c == 0 ? 0 : c == 3 ? 3 : 2;
                sf[p] = sffs[(size_t)r * HW + i];
            }
        // the list's tail up to the largest F: an in-bounds cell, never read (every loop stops at the room's F)
        for (int j = 0; j < std::max(1, fmax); j++)
            fr[j] = j < room_f[(size_t)r] ? fp[(size_t)r][(size_t)j] : (uint16_t)(PW + 1);
    }
    const std::vector<ffm::EnvParams> rec = env_records(e, sets, set_of_env, &room_f, room_of_env);

    HIP_TRY(hipSetDevice(e->d.device));
    unsigned char* d_rooms = nullptr;
    int32_t* d_roe = nullptr;
    ffm::EnvParams* d_envp = nullptr;
    unsigned long long* d_ctr = nullptr;   // the group form: a larger counter array, if its grids need one
    auto undo = [&](int rc) {
        (void)hipFree(d_rooms);
        (void)hipFree(d_roe);
        (void)hipFree(d_envp);
        (void)hipFree(d_ctr);
        return rc;
    };
    // room_of_env is read in pairs through buffer resources: whole pairs, zeroed padding
    const size_t roe_bytes = ((E + 7) & ~(size_t)7) * 4;
    hipError_t he = hipMalloc((void**)&d_rooms, table.size());
    if (he == hipSuccess) he = hipMalloc((void**)&d_roe, roe_bytes);
    if (he == hipSuccess) he = hipMalloc((void**)&d_envp, E * sizeof(ffm::EnvParams));
    if (he != hipSuccess) return undo(fail(FFM_E_NOMEM, std::string("env rooms: ") + hipGetErrorString(he)));
    // The room plan, from the occupancy of the room form (the tables select it).
    const ffm::CoreStepArgs fa = form_args(e, fmax, d_envp, d_rooms, d_roe);
    StepPlan rp;
    size_t ctr_slots = e->ctr_slots;
    if (group_form) {
        // The group kernel's room form: envs per group and step shards from that form's occupancy, as
        // the per-env form's (pep_group_setup); every launch's grid holds a wave per group.  The kernel
        // adds to one counter slot per wave of its grid, so a geometry with more waves than the slots
        // allocated at create gets a larger array, the sums carried over (below): the create-time
        // kernels keep their arguments and resources.
        rp = group_plan(e, fa, e->d_stage, true);
        ctr_slots = std::max(ctr_slots, plan_slots(rp));
        if (ctr_slots > e->ctr_slots) {
            he = hipMalloc((void**)&d_ctr, ctr_slots * 32);
            if (he != hipSuccess) return undo(fail(FFM_E_NOMEM, std::string("env rooms: counters: ") + hipGetErrorString(he)));
        }
        he = ensure_shard_streams(e, rp.shards.size());
        if (he != hipSuccess) return undo(fail(FFM_E_HIP, std::string("step shard streams: ") + hipGetErrorString(he)));
    } else if (block_form) {
        rp = simple_plan(e, StepPlan::kBlock, block_grid(e));
    } else {
        rp = simple_plan(e, StepPlan::kLane, lane_grid(e, fa));
        if (plan_slots(rp) > e->ctr_slots) return undo(fail(FFM_E_UNSUPPORTED, "env rooms: counter slots"));
    }
    // stream-ordered after the steps queued so far; the tables are consumed before the return
    he = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hipMemsetAsync(d_roe, 0, roe_bytes, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_roe, room_of_env, E * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_rooms, table.data(), table.size(), hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_envp, rec.data(), E * sizeof(ffm::EnvParams), hipMemcpyHostToDevice, s);
    if (he == hipSuccess && d_ctr) he = hipMemsetAsync(d_ctr, 0, ctr_slots * 32, s);
    if (he == hipSuccess && d_ctr) he = hipMemcpyAsync(d_ctr, e->d_ctr, e->ctr_slots * 32, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) return undo(fail(FFM_E_HIP, std::string("env rooms: ") + hipGetErrorString(he)));
    if (d_ctr) {   // the larger counter array stays for the engine's life (ffm_engine_device_buffers reports it)
        (void)hipFree(e->d_ctr);
        e->d_ctr = d_ctr;
        e->ctr_slots = ctr_slots;
    }
    (void)hipFree(e->d_rooms);
    (void)hipFree(e->d_room_of_env);
    (void)hipFree(e->d_envp);
    e->d_rooms = d_rooms;
    e->d_room_of_env = d_roe;
    e->d_envp = d_envp;
    e->room_stride = lay.stride;
    e->room_fmax = fmax;
    e->room_plan = std::move(rp);
    e->room_maps.assign(maps, maps + (size_t)n_rooms * HW);
    e->room_sffs.assign(sffs, sffs + (size_t)n_rooms * HW);
    e->room_of_env.assign(room_of_env, room_of_env + E);
    e->room_f = std::move(room_f);
    return FFM_OK;
}

int ffm_engine_set_env_rooms_kernel(ffm_engine* e, int32_t mode) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    if (mode != 0 && mode != 1 && mode != 2)
        return fail(FFM_E_INVALID, "env rooms kernel: mode must be 0 (lane), 1 (block) or 2 (group)");
    if (rooms_on(e)) return fail(FFM_E_INVALID, "env rooms kernel: rooms are on (turn them off first)");
    if (mode == 2 && (!created_on(e, StepPlan::kGroup) || e->mt || e->f64))
        return fail(FFM_E_UNSUPPORTED, "env rooms kernel: the engine was not created on the group kernel (12x12, "
                                       "agent_capacity <= 32, Philox, float32 SFF)");
    if (mode == 1) {
        if (e->mt) return fail(FFM_E_UNSUPPORTED, "env rooms kernel: Philox engines only");
        if (e->f64) return fail(FFM_E_UNSUPPORTED, "env rooms kernel: float32-SFF engines only");
        if (created_on(e, StepPlan::kLane) || created_on(e, StepPlan::kGroup))
            return fail(FFM_E_UNSUPPORTED, "env rooms kernel: lane and group engines have the lane kernel's room form");
        if (e->big)
            return fail(FFM_E_UNSUPPORTED, "env rooms kernel: engines with their state in global scratch (block_scratch) "
                                           "have no room form (u16 free lists, state outside the LDS)");
    }
    e->room_kernel = mode;
    return FFM_OK;
}

int ffm_engine_get_env_rooms(ffm_engine* e, uint8_t* maps, float* sffs, int32_t cap, int32_t* n_rooms,
                             int32_t* room_of_env) {
    if (!e || !n_rooms || cap < 0) return fail(FFM_E_INVALID, "null argument");
    *n_rooms = (int32_t)e->room_f.size();
    if (*n_rooms == 0) return FFM_OK;
    if ((maps || sffs) && cap < *n_rooms)
        return fail(FFM_E_INVALID, "get_env_rooms: buffer too small (*n_rooms holds the count)");
    if (maps) std::copy(e->room_maps.begin(), e->room_maps.end(), maps);
    if (sffs) std::copy(e->room_sffs.begin(), e->room_sffs.end(), sffs);
    if (room_of_env) std::copy(e->room_of_env.begin(), e->room_of_env.end(), room_of_env);
    return FFM_OK;
}

int ffm_engine_get_counters(ffm_engine* e, uint64_t* counters, void* stream) {
    if (!e || !counters) return fail(FFM_E_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    std::vector<unsigned long long> c(e->ctr_slots * 4);
    HIP_TRY(hipMemcpyAsync(c.data(), e->d_ctr, e->ctr_slots * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++) counters[i] = 0;
    for (size_t j = 0; j < e->ctr_slots; j++)
        for (int i = 0; i < 4; i++) counters[i] += c[j * 4 + i];
    return FFM_OK;
}

int ffm_engine_device_buffers(ffm_engine* e, ffm_device_buffers* out) {
    if (!e || !out) return fail(FFM_E_INVALID, "null argument");
    out->positions = e->d_pos;
    out->counts = e->d_cnt;
    out->dff = e->d_dff;
    out->episodes = e->d_eps;
    out->counters = reinterpret_cast<uint64_t*>(e->d_ctr);
    out->mt_np = e->d_mt_np;
    out->mt_py = e->d_mt_py;
    out->counter_slots = (int64_t)e->ctr_slots;
    return FFM_OK;
}

int ffm_engine_get_step_index(ffm_engine* e, uint32_t* t) {
    if (!e || !t) return fail(FFM_E_INVALID, "null argument");
    *t = e->t;
    return FFM_OK;
}

int ffm_engine_set_step_index(ffm_engine* e, uint32_t t) {
    if (!e) return fail(FFM_E_INVALID, "null engine");
    e->t = t;
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): read the FFM_STAMPS counters.
int ffm_debug_read(ffm_engine* e, uint64_t* out, int n) {
    if (!e || !out || n < 0 || n > 16) return fail(FFM_E_INVALID, "bad args");
    HIP_TRY(hipMemcpy(out, e->d_dbg, (size_t)n * 8, hipMemcpyDeviceToHost));
    return FFM_OK;
}

// Diagnostic: the group kernel's stage image (kernels.h), copied to the host.  *n gets its size in
// bytes (0 for engines of the other kernels); the copy is made when `out` holds that many.
int ffm_debug_stage_image(ffm_engine* e, void* out, int64_t cap, int64_t* n) {
    if (!e || !n || cap < 0) return fail(FFM_E_INVALID, "bad args");
    *n = (int64_t)e->stage_bytes;
    if (!out || e->stage_bytes == 0) return FFM_OK;
    if (cap < (int64_t)e->stage_bytes) return fail(FFM_E_INVALID, "stage_image: buffer too small (*n holds the size)");
    HIP_TRY(hipMemcpy(out, e->d_stage, e->stage_bytes, hipMemcpyDeviceToHost));
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): the blocks per CU the runtime reports resident
// (hipOccupancyMaxActiveBlocksPerMultiprocessor) for this engine's group kernel -- its
// neighbourhood, k_D and envs per group, the log-free instantiation -- in the single-group form
// (one != 0) or the loop form, each at its own shared-memory size.  0 for the other kernels.
int ffm_debug_group_occupancy(ffm_engine* e, int32_t one, int32_t* blocks_per_cu) {
    if (!e || !blocks_per_cu) return fail(FFM_E_INVALID, "bad args");
    *blocks_per_cu = 0;
    if (!created_on(e, StepPlan::kGroup)) return FFM_OK;
    HIP_TRY(hipSetDevice(e->d.device));
    ffm::CoreStepArgs a = make_args(e);
    // the form that steps the engine; while another kernel does (per-env parameters or rooms on
    // the lane kernel), the create-time form at the create-time group size
    const StepPlan* p = &plan(e);
    if (p->kernel != StepPlan::kGroup) {
        p = &e->create_plan;
        a.envp = nullptr;
        a.rooms = nullptr;
    }
    *blocks_per_cu = ffm::core_group_blocks_per_cu(a, e->d.neighborhood, p->g, one != 0);
    return FFM_OK;
}

// Diagnostic: the placement's candidate count M and key threshold in effect (fixed at create).
int ffm_debug_reset_candidates(ffm_engine* e, int32_t* m, uint32_t* thr) {
    if (!e || !m || !thr) return fail(FFM_E_INVALID, "bad args");
    *m = e->reset_m;
    *thr = e->reset_thr;
    return FFM_OK;
}

// Diagnostic (not part of the ABI header): the step plan in effect (plan(): the create plan, or with
// per-env parameters or rooms on, the kernel, grid and shards that step the engine meanwhile).
//   out[0] step kernel (0 group, 1 lane, 2 wave, 3 block, 4 block with global scratch)
//   out[1] envs per group of the group kernel (0 for the other kernels)
//   out[2] blocks of the step kernel's grid
//   out[3] K, envs per workgroup of the block kernel
//   out[4] threads per block of the step kernel
//   out[5] 1 if the fused multi-step kernel is available, out[6] its grid's blocks
//   out[7] env shards a step(n > 1) call runs as under the current settings (1: one launch per
//          step over all envs), out[8] blocks of one shard's grid (the first's; out[2] if one shard)
//   out[9] the group kernel's form in the launches of such a call (its out[7] shards, or the one
//          launch): 1 if every one of them takes the single-group form, 0 for the loop form (and
//          for the other kernels)
int ffm_debug_launch_info(ffm_engine* e, int32_t* out, int n) {
    if (!e || !out || n < 0 || n > 10) return fail(FFM_E_INVALID, "bad args");
    const StepPlan& p = plan(e);
    const bool block = p.kernel == StepPlan::kBlock;
    const int S = shards_in_effect(e);
    bool one = p.kernel == StepPlan::kGroup && p.one;
    if (one && S > 1) {
        for (const StepPlan::Shard& sh : p.shards) one = one && ffm::core_group_one_group(sh.n, sh.blocks, sh.g);
    } else if (one) {
        one = ffm::core_group_one_group(e->d.n_envs, p.blocks, p.g);
    }
    const int32_t v[10] = {
        block && e->big ? 4 : (int32_t)p.kernel,
        p.g,
        p.blocks,
        e->K,
        !block ? 256 : e->big ? 1024 : e->block,
        e->multi ? 1 : 0,
        e->multi ? e->multi_blocks : 0,
        S,
        S > 1 ? p.shards[0].blocks : p.blocks,
        one ? 1 : 0,
    };
    for (int i = 0; i < n; i++) out[i] = v[i];
    return FFM_OK;
}

int ffm_np_expf_device(const float* x, float* y, int64_t n, void* stream) {
    HIP_TRY(ffm::launch_np_expf(x, y, n, (hipStream_t)stream));
    return FFM_OK;
}

}  // extern "C"
