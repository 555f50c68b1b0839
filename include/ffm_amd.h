/*
 * ffm_amd.h -- C ABI of the MI355X-native batched floor-field stepper.
 *
 * The reference (SoraKurihara/FFM) has no native boundary: its "plugin" API
 * is the duck-typed model class consumed by the drivers.  Each entry point
 * below is what that class's methods bind to when a binding (ctypes stub in
 * INTEGRATION.md, or ffm_amd/engine.py) replaces the NumPy body:
 *
 *   ffm_engine_create      <- FloorFieldModel.__init__      model/ffm_core.py:7-21
 *   ffm_engine_reset       <- initialize_agents / reset     model/ffm_core.py:23-26
 *                                                           (reset(): model/ffm_ac_core.py:319-325)
 *   ffm_engine_step        <- FloorFieldModel.step          model/ffm_core.py:36-104
 *   ffm_engine_update_dff  <- FloorFieldModel.update_dff    model/ffm_core.py:106-117
 *   ffm_engine_{get,set}_state    <- .positions / .dff attributes (read by
 *                                    main.py:44-46, assigned by run_trained_ffm.py:235-236)
 *   ffm_engine_{get,set}_mt_state <- the process-global np.random / random
 *                                    streams the reference consumes
 *                                    (model/ffm_core.py:25,84,95,96)
 *
 * Conventions: plain pointers and sizes, no torch types.  Host pointers
 * unless the name says "device".  Every function returns 0 on success or a
 * negative FFM_E* code; ffm_last_error() describes the last failure of the
 * calling thread.  One engine per thread at a time (the engine is not
 * re-entrant, like the reference's process-global RNG).  Work is
 * stream-ordered on the hipStream_t passed as `stream` (NULL = null stream);
 * the get/set functions synchronise that stream.
 *
 * Agent positions are cell indices x*W + y stored as uint16 (maps up to
 * 65,536 cells); positions[e][0..count[e]) are the live agents of env e in
 * the reference's order (the row order of FloorFieldModel.positions).
 */
#ifndef FFM_AMD_H
#define FFM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFM_ABI_VERSION 2

enum {
    FFM_OK = 0,
    FFM_E_INVALID = -1,   /* bad argument / shape / map (ValueError in the reference) */
    FFM_E_HIP = -2,       /* HIP runtime failure */
    FFM_E_NOMEM = -3,
    FFM_E_UNSUPPORTED = -4
};

/* Which model class the engine steps. */
enum {
    FFM_VARIANT_CORE = 0,      /* model/ffm_core.py FloorFieldModel              (ffm_engine_*)  */
    FFM_VARIANT_AC = 1,        /* model/ffm_ac_core.py FloorFieldModel           (ffm_learner_*) */
    FFM_VARIANT_UNIFIED = 2,   /* model/ffm_unified.py FloorFieldModelUnified    (ffm_learner_*) */
    FFM_VARIANT_ACTOR_ONLY = 3, /* model/ffm_actor_only.py FloorFieldModelActorOnly (ffm_learner_*) */
    FFM_VARIANT_TRAINED = 4    /* model/ffm_trained_core.py FloorFieldModel: inference with a trained
                                  H (ffm_learner_*; import the table, nothing is learned) */
};

/* Where the random draws come from. */
enum {
    FFM_RNG_PHILOX = 0,       /* counter-based, keyed (seed, step, env, agent, purpose) */
    FFM_RNG_MT = 1            /* per-env NumPy-legacy + CPython MT19937 streams:
                                 reproduces the reference bit for bit */
};

enum { FFM_SFF_F32 = 0, FFM_SFF_F64 = 1 };

typedef struct {
    int32_t abi_version;      /* = FFM_ABI_VERSION */
    int32_t variant;          /* FFM_VARIANT_* */
    int32_t H, W;             /* map shape; H*W <= 65536 */
    const uint8_t* map;       /* host [H*W]: 0 free, 2 wall, 3 exit (others: blocked) */
    const void* sff;          /* host [H*W] static floor field */
    int32_t sff_dtype;        /* FFM_SFF_F32 / FFM_SFF_F64 (dtype of the .npy, model/ffm_core.py:17) */
    int32_t neighborhood;     /* 4 = "neumann", 8 = "moore" (model/ffm_core.py:28-34) */
    double k_S, k_D, diffuse, decay;   /* params, model/ffm_core.py:8-15 */
    int64_t n_envs;           /* E: independent environments on this device */
    int32_t agent_capacity;   /* A: slots per env (>= n_agents; learners: <= 16383 batched, <= 65535 MT) */
    int32_t n_agents;         /* N placed by reset / auto-reset */
    int32_t rng_mode;         /* FFM_RNG_* */
    int32_t auto_reset;       /* 1: an env emptied by a step is re-placed (Philox, keyed by that
                                 step) and its DFF zeroed at the end of that step */
    uint64_t seed;            /* Philox key */
    int64_t env_base;         /* global id of env 0 (multi-GPU sharding keys RNG by global id) */
    int32_t device;           /* HIP device ordinal */
    int32_t envs_per_block;   /* 0 = auto, > 0 = block kernel with that many envs per workgroup,
                                 -1 = wave kernel (core_step.hip), -2 = lane kernel (core_lane.hip),
                                 -3 = group kernel (core_group.hip; 12x12 only, the auto choice there);
                                 the negative values force a kernel for diagnostics and tests */
} ffm_engine_desc;

typedef struct {
    uint16_t* positions;      /* [E][A] */
    int32_t* counts;          /* [E] */
    float* dff;               /* [E][H*W] */
    int32_t* episodes;        /* [E] completed resets */
    uint64_t* counters;       /* [counter_slots][4]: agent_steps, exits, resets, steps;
                                 one slot per wave/workgroup (uncontended), sum over slots */
    uint32_t* mt_np;          /* [E][625] (MT mode only, else NULL) */
    uint32_t* mt_py;          /* [E][625] */
    int64_t counter_slots;
} ffm_device_buffers;

typedef struct ffm_engine ffm_engine;

const char* ffm_last_error(void);
int ffm_abi_version(void);

int ffm_engine_create(const ffm_engine_desc* desc, ffm_engine** out);
int ffm_engine_destroy(ffm_engine* eng);

/* Place n_agents in every env (Philox mode: keyed by the engine step counter,
 * which then advances), zero the DFF and the per-env episode counters.  MT mode places nothing: the caller
 * draws the placement from its own generator (initialize_agents) and uploads it. */
int ffm_engine_reset(ffm_engine* eng, void* stream);

/* Re-place the envs whose byte in `mask` is nonzero (reset(env_mask); the
 * reference's drivers reset one model per episode: run_unified_actor_training.py:263 ->
 * model/ffm_unified.py:800-812 reset()).  `mask` is a DEVICE pointer to n_envs bytes on the
 * engine's device, read on `stream`.  Philox only: the masked envs get the placement
 * ffm_engine_reset would give them (keyed by the step counter, which then advances), a zero
 * DFF and count n_agents; the other envs are untouched.  Episode counters are not changed
 * (an abandoned episode is not a completed one).  `mask` is read on `stream` and nowhere
 * else: whatever produces the bytes -- an upload, a conversion from another type -- must be
 * queued on `stream` before the call or be complete (the Python binding queues both there).
 * Trajectory capture: a masked env keeps its k and its rows restart at step 1 (see
 * ffm_engine_set_trajectory_capture); drain before the call.  With capture off the call
 * launches the placement only.  MT mode: FFM_E_UNSUPPORTED. */
int ffm_engine_reset_envs(ffm_engine* eng, const uint8_t* mask, void* stream);

/* Advance every env by n_steps steps (model/ffm_core.py:36-104 each).  With n_steps > 1 a
 * large 12x12 Philox engine may step disjoint env ranges on streams of its own between one
 * fork from and one join into `stream` (DESIGN.md section 4, step shards): whatever follows
 * on `stream` sees all n_steps steps of every env, and the state is the same bits either way.
 * A stream under capture always gets one launch per step on that stream. */
int ffm_engine_step(ffm_engine* eng, int32_t n_steps, void* stream);

/* Steps fused per launch by ffm_engine_step (default 1: one launch per step).
 * k > 1 lets Philox engines of the small-env kernels (A <= 32, W % 4 == 0,
 * H*W <= 256, float32 SFF) step each env pair k times with its state on chip;
 * results equal k single steps bit for bit.  Other engines keep one launch per
 * step.  Returns FFM_E_INVALID for k < 1. */
int ffm_engine_set_fused_steps(ffm_engine* eng, int32_t k);

/* Only the diffusion/decay of the DFF (model/ffm_core.py:106-117). */
int ffm_engine_update_dff(ffm_engine* eng, void* stream);

/* Copy envs [env0, env0+n) in/out.  Any pointer may be NULL to skip it.
 * positions: [n][A] uint16, counts: [n] int32, dff: [n][H*W] float32. */
int ffm_engine_set_state(ffm_engine* eng, int64_t env0, int64_t n, const uint16_t* positions,
                         const int32_t* counts, const float* dff, void* stream);
int ffm_engine_get_state(ffm_engine* eng, int64_t env0, int64_t n, uint16_t* positions,
                         int32_t* counts, float* dff, void* stream);

/* MT mode: per-env generator states, 624 words + position (NumPy
 * get_state()[1:3] / CPython getstate()[1]). */
int ffm_engine_set_mt_state(ffm_engine* eng, int64_t env, const uint32_t* np_key, int32_t np_pos,
                            const uint32_t* py_key, int32_t py_pos, void* stream);
int ffm_engine_get_mt_state(ffm_engine* eng, int64_t env, uint32_t* np_key, int32_t* np_pos,
                            uint32_t* py_key, int32_t* py_pos, void* stream);

/* Trajectory capture of the batched step (replaces the positions log of
 * model/ffm_core.py:119-133 run() and main.py:44-54, which keep a copy of `positions`
 * after every step until the room is empty).  For each selected env (local index) its
 * episode k (0-based, counted from the last ffm_engine_reset; one episode per auto-reset)
 * is captured iff (k + phases[i]) % period == 0 (phases NULL: 0).  After every step of a
 * captured episode one row is appended: meta {global env, k, step in the episode
 * (1-based), count} and the agent_capacity cells (x*W+y, live agents first in the
 * reference's order, 0xFFFF after); an episode's last row is the empty one of the step
 * that emptied the room.  An env that is already empty (auto_reset off) logs nothing.
 * The rule, per step and selected env e: one row iff its k at the start of the step passes
 * the period test, and none if e was empty before the step and is still empty after it.  The
 * row's step is the number of steps since the latest of e's current placement (by
 * ffm_engine_reset, ffm_engine_reset_envs or the auto-reset) and this call; count and cells
 * are e's state after the step, and a step that ended the episode gives the empty row (the
 * state before the re-placement).  ffm_engine_reset_envs changes no k: a masked env's rows
 * go on under the same k from step 1 again, and one that had emptied logs again (what the
 * learner's capture does as well).  The drain's consumers sort by (env, k, step), which
 * would interleave the two segments of one (env, k): drain before a masked reset.
 * Rows past capacity_rows are dropped and counted.  While capture is on, ffm_engine_step
 * makes one launch per step (fused steps are off).  n_sel = 0 turns capture off. */
int ffm_engine_set_trajectory_capture(ffm_engine* eng, const int32_t* envs, const int32_t* phases, int32_t n_sel,
                                      int32_t period, int64_t capacity_rows, void* stream);
/* Rows captured since the last drain, in no particular order (sort by env, k, step);
 * meta [cap][4] int32, cells [cap][agent_capacity] u16, host pointers. */
int ffm_engine_drain_trajectory(ffm_engine* eng, int32_t* meta, uint16_t* cells, int64_t cap, int64_t* n,
                                int64_t* dropped, void* stream);

/* Evacuation-time log and on-device statistics: what main.py:44-56 prints as "Simulation
 * finished in {step} steps" and model/ffm_core.py:119-133 run() loops for, from every env
 * without a host round trip per step.
 *
 * An episode of env e ends at the step after which e holds no agents, having held at least
 * one before it: with auto_reset the step that re-places it (the event that adds 1 to
 * episodes[e]), without it the one step that empties it.  Its length is
 * t_end - ep_start[e] in wrapping u32 arithmetic, where ep_start[e] is the step index that
 * keyed the env's current placement (written by ffm_engine_reset, by ffm_engine_reset_envs
 * for the masked envs, and by the in-kernel auto-reset): a reset keyed t = 0 and an emptying
 * step keyed t = 97 give 97, main.py's `step`.  Nothing is counted or written per step.
 *
 * capacity_records > 0 turns the record log on (0: off): one record of four int32 per ended
 * episode, {global env (env_base + e), episode index k, steps, t_end}, k = episodes[e]
 * before the increment (0-based from the last ffm_engine_reset; always 0 with auto_reset
 * off), in no particular order.  An env ends at most one episode per step, so a capacity of
 * 16 * n_envs is safe when the log is drained every 16 steps; records past the capacity are
 * dropped and counted.
 * hist_bins > 0 turns the statistics on (0: off): a histogram of u64, bin i = episodes of i
 * steps, the last bin every episode of hist_bins - 1 steps or more, and a summary {count,
 * sum of steps, sum of steps^2, min, max}.  They never drop anything and are integer
 * atomics: bitwise independent of launch geometry, step shards and fused steps.
 * Both 0 frees everything; with the feature off no kernel reads or writes anything new.
 *
 * ffm_engine_reset_envs is not an episode end: it logs nothing, leaves k alone and restarts
 * the masked envs' ep_start.  ffm_engine_reset clears neither the log nor the statistics
 * (a drain or `clear` does).  Turned on mid-run, episodes in flight count from the steps
 * taken after the call.  ffm_engine_set_step_index inside an episode, and
 * ffm_engine_set_state with new counts, leave the affected episodes' lengths undefined.
 * Works with step shards, fused steps, trajectory capture and on a stream under capture
 * (ffm_engine_step makes no host call for it).  Synchronises the stream.
 * Philox only (MT: FFM_E_UNSUPPORTED).  Needs env_base + n_envs <= INT32_MAX. */
int ffm_engine_set_episode_log(ffm_engine* eng, int64_t capacity_records, int32_t hist_bins, void* stream);
/* Like ffm_learner_drain_episodes: copies min(n, capacity) records [cap][4] int32 to the
 * host, then empties the log.  *dropped = records lost to a full log.  cap too small:
 * FFM_E_INVALID with *n = count needed, and the log is left as it was.  Log off: *n = 0. */
int ffm_engine_drain_episodes(ffm_engine* eng, int32_t* records, int64_t cap, int64_t* n, int64_t* dropped,
                              void* stream);
/* hist[bins] (bins = hist_bins) and summary[5] to the host (either may be NULL).  clear != 0
 * zeroes them afterwards (min is restored to its empty value).  min reads 0 while count is
 * 0; statistics off: summary reads zeros.  Synchronises the stream. */
int ffm_engine_get_episode_stats(ffm_engine* eng, uint64_t* hist, int32_t bins, uint64_t* summary, int32_t clear,
                                 void* stream);

/* Field statistics: where the crowd stands and how the room empties, summed on the device.
 * The reference gets both from the positions it logs after every step (main.py:44-54, read
 * back by visualize_trajectory.py and inspect_trajectory.py); here an observer kernel follows
 * every step launch and no position leaves the device.
 *
 * Env e has a class, class_of_env[e] in [0, n_classes) (NULL: every env in class 0).  Per class
 * c the engine keeps four arrays of u64:
 *   occupancy[c][H * W]   visits of every cell (row-major cell indices, as ffm_engine_get_state's)
 *   observed[c]           observed env states
 *   remaining[c][bins]    agents inside, by time since placement   (bins = curve_bins > 0)
 *   alive[c][bins]        observed env states, by time since placement
 * After every step launch keyed t, for every env e of it: n = counts[e], tau = t - ep_start[e]
 * in wrapping u32 (the episode log's ep_start and arithmetic).  n == 0 adds nothing; tau == 0
 * adds nothing (this step's auto-reset placed the env: a placement is never observed, whether
 * ffm_engine_reset, ffm_engine_reset_envs or the auto-reset made it, so an episode of T steps
 * adds exactly its states tau = 1 .. T - 1).  Otherwise, with b = min(tau, bins - 1):
 *   occupancy[c][positions[e][j]] += 1 for j < n;  observed[c] += 1;
 *   remaining[c][b] += n;  alive[c][b] += 1.
 * The mean density of a cell is occupancy / observed; the mean number inside at tau is
 * remaining[tau] divided by the number of episodes: both divisions are the caller's.  Every sum
 * is an integer: the same bits under any launch geometry, step shards, the fused-steps setting
 * and either form of the observer (FFM_FIELD_STATS_FORM=lds|global, read by this call, forces
 * one; lds on tables beyond the LDS budget: FFM_E_INVALID).  The step itself does not change.
 *
 * n_classes == 0 turns the feature off and frees everything.  FFM_E_INVALID, the engine exactly
 * as it was: n_classes < 0, curve_bins < 0, a class outside [0, n_classes), or tables of more
 * than FFM_FIELD_STATS_MAX_BYTES (one copy: n_classes * (H * W + 2 * curve_bins + 1) * 8 bytes).
 * Philox only (MT: FFM_E_UNSUPPORTED).  Setting it again replaces classes and bins and clears.
 *
 * While on, ffm_engine_step takes one launch per step (the fused multi-step path is not taken,
 * as with trajectory capture; the state is the same bits) and the observer follows each, on
 * each step shard's own stream where shards are in effect (measured on one MI355X at 65,536 envs
 * of 12x12 with 32 agents: 22.8 us per step off, 30.4 us with five classes and 128 bins, 87.9 us
 * with the global form forced; profiles/field_stats/).  ffm_engine_reset clears nothing
 * (`clear` below, or turning the feature off, does).  Turned on mid-run, episodes in flight
 * count from the steps taken after the call.  ffm_engine_set_step_index inside an episode, and
 * ffm_engine_set_state with new counts, leave the affected tau undefined.  Synchronises the
 * stream. */
#define FFM_FIELD_STATS_MAX_BYTES (256ll << 20)
int ffm_engine_set_field_stats(ffm_engine* eng, const int32_t* class_of_env, int32_t n_classes, int32_t curve_bins,
                               void* stream);
/* occupancy[C][H * W], observed[C], remaining[C][bins], alive[C][bins] to the host (any may be
 * NULL).  clear != 0 zeroes them afterwards.  Feature off: FFM_E_INVALID.  Synchronises the
 * stream. */
int ffm_engine_get_field_stats(ffm_engine* eng, uint64_t* occupancy, uint64_t* observed, uint64_t* remaining,
                               uint64_t* alive, int32_t clear, void* stream);

/* Exit flow: which exit the agents leave through, and when, summed on the device.  The reference
 * decides the door in model/ffm_core.py:66-72, 100-102: an agent with an exit among its free
 * neighbours always requests the first exit in neighbour order, and whoever reaches an exit is
 * dropped from `positions`.  That last move is invisible to ffm_engine_get_state (the agent is
 * removed in the same step, and the step that empties an env re-places it); here a kernel follows
 * every step launch, compares the positions before and after it, and nothing leaves the device.
 *
 * Doors.  Every exit cell of every room in effect (the create-time room, or the rooms of
 * ffm_engine_set_env_rooms) has a door id in [0, D).  door_of_cell == NULL: a room's exit cells
 * numbered in row-major order, D the largest count over the rooms (n_doors is ignored).  Else
 * door_of_cell[R][H * W] with D = n_doors >= 1: only the entries of exit cells are read, each in
 * [0, n_doors) -- a 4-wide exit can be one door.  D <= 255.
 * Per class c (class_of_env / n_classes as for the field statistics) the engine keeps, as u64,
 *   exited[c][d]           agents that left through door d
 *   outflow[c][d][bins]    the same by time since placement   (bins = curve_bins > 0)
 * After every step launch keyed t, for every env e of it and every agent that left in that step
 * through door d: tau = t - ep_start_before[e] in wrapping u32 (ep_start as it was before the
 * step: the auto-reset overwrites it), b = min(tau, bins - 1),
 *   exited[c][d] += 1;  outflow[c][d][b] += 1.
 * tau >= 1 always; the last agents of an episode are counted with the episode's length.  An agent
 * left iff its cell before the step has a door (the first exit cell among the cell's neighbours in
 * neighbour order) and is not among the positions after the step; a step that emptied the env
 * took every agent.  Every sum is an integer: the same bits under any launch geometry, step
 * shards, the fused-steps setting and either form of the kernel (FFM_EXIT_FLOW_FORM=lds|global
 * forces one and FFM_EXIT_FLOW_BLOCKS caps its grid, both read by this call; lds on tables beyond
 * the LDS budget: FFM_E_INVALID).  The step itself does not change.
 *
 * n_classes == 0 turns the feature off and frees everything.  FFM_E_INVALID, the engine exactly as
 * it was: a negative count, a class outside [0, n_classes), an exit cell's label outside
 * [0, n_doors), more than 255 doors, or tables of more than FFM_EXIT_FLOW_MAX_BYTES (one copy:
 * n_classes * D * (1 + curve_bins) * 8 bytes).  Philox only (MT: FFM_E_UNSUPPORTED).  Setting it
 * again replaces doors, classes and bins and clears.
 *
 * While on, the engine keeps a snapshot of positions, counts and ep_start (2 A + 8 bytes per env),
 * ffm_engine_step takes one launch per step (no fused steps, as for the field statistics; the
 * state is the same bits) and the flow kernel follows each, on each step shard's own stream where
 * shards are in effect.  ffm_engine_reset, ffm_engine_reset_envs and ffm_engine_set_state refresh
 * the snapshot on their stream; ffm_engine_reset clears nothing.  ep_start is shared with the
 * episode log and the field statistics; turned on mid-run, episodes in flight count from the
 * steps taken after the call.  Works with the log, trajectory capture and the field statistics
 * on.  Rooms first, the flow after: ffm_engine_set_env_rooms (on or off) while the flow is on
 * returns FFM_E_INVALID and leaves the engine as it was.  ffm_engine_set_step_index inside an
 * episode leaves the affected tau undefined.  Synchronises the stream. */
#define FFM_EXIT_FLOW_MAX_BYTES FFM_FIELD_STATS_MAX_BYTES
int ffm_engine_set_exit_flow(ffm_engine* eng, const int32_t* door_of_cell, int32_t n_doors, const int32_t* class_of_env,
                             int32_t n_classes, int32_t curve_bins, void* stream);
/* exited[C][D] and outflow[C][D][bins] to the host (either may be NULL).  clear != 0 zeroes them
 * afterwards.  Feature off: FFM_E_INVALID.  Synchronises the stream. */
int ffm_engine_get_exit_flow(ffm_engine* eng, uint64_t* exited, uint64_t* outflow, int32_t clear, void* stream);
/* The door labels in effect: door_of_cell[R][H * W] (-1 off the exits; R = 1 without per-env
 * rooms) and *n_doors = D (either may be NULL).  Feature off: FFM_E_INVALID. */
int ffm_engine_get_exit_doors(ffm_engine* eng, int32_t* door_of_cell, int32_t* n_doors);

/* Motion statistics: how the crowd moves, summed on the device -- the flow field, mean speed
 * against the time since placement, and the egress time by starting cell (what the reference's
 * users read off the per-step position log with visualize_trajectory.py and
 * inspect_trajectory.py).  A kernel follows every step launch and compares the positions before
 * (P, n0 agents) and after it (P', n agents); nothing leaves the device and no step kernel changes.
 *
 * Identity.  The reference removes the agents that reached an exit order-preservingly
 * (model/ffm_core.py:100-102), so agent i of P that did not leave is agent i - |{leavers l < i}|
 * of P'.  The leavers are the exit flow's: the cell before the step has an exit among its
 * neighbours and is not among the positions after it; a step that emptied the env took everybody.
 * Direction d in [0, NB] (NB = 4 or 8 neighbours): a survivor's is the index of its move in the
 * reference's neighbour order (Neumann up, down, left, right; Moore row-major), NB for a stay; a
 * leaver's is the index of the first exit cell among its cell's neighbours.  The origin of an
 * agent is the cell it was placed on (by ffm_engine_reset, ffm_engine_reset_envs or the
 * auto-reset; turned on mid-run: the cell it stood on then).
 * Per class c (class_of_env / n_classes as for the field statistics) the engine keeps, as u64,
 *   flux[c][cell][NB + 1]     agents that stepped out of `cell` in direction d, or stood still
 *   present[c][bins]          agents inside before a step, by time since placement
 *   moved[c][bins]            those of them that moved (leavers move); moved / present is the mean speed
 *   egress_count[c][cell]     agents placed on `cell` that have left
 *   egress_steps[c][cell]     the sum of their egress times; egress_steps / egress_count is the mean
 * After every step launch keyed t, for every env e of it with n0 > 0: tau = t - ep_start_before[e]
 * in wrapping u32, b = min(tau, bins - 1),
 *   flux[c][P[i]][d(i)] += 1 for i < n0;  present[c][b] += n0;  moved[c][b] += |{i : d(i) != NB}|;
 *   for every leaver with origin o:  egress_count[c][o] += 1;  egress_steps[c][o] += tau (not clamped).
 * A position pair that is no neighbour move (a state the caller made inconsistent) adds nothing
 * for that agent.  Every sum is an integer: the same bits under any launch geometry, step shards,
 * the fused-steps setting and either form of the kernel (FFM_MOTION_STATS_FORM=lds|global forces
 * one and FFM_MOTION_STATS_BLOCKS caps its grid, both read by this call; lds on tables beyond the
 * LDS budget: FFM_E_INVALID).  The step itself does not change.
 *
 * n_classes == 0 turns the feature off and frees everything.  FFM_E_INVALID, the engine exactly as
 * it was: a negative count, a class outside [0, n_classes), or tables of more than
 * FFM_MOTION_STATS_MAX_BYTES (one copy: n_classes * (H * W * (NB + 3) + 2 * curve_bins) * 8
 * bytes).  Philox only (MT: FFM_E_UNSUPPORTED).  Setting it again replaces classes and bins, clears,
 * and takes the agents' cells at that moment as their origins.
 *
 * While on, the engine keeps the exit flow's snapshot (shared with it: it lives while either is
 * on) and an origin per agent (2 A + 4 bytes per env); ffm_engine_step takes one launch per step (no
 * fused steps; the state is the same bits) and the motion kernel follows each, before the flow
 * kernel, on each step shard's own stream where shards are in effect.  ep_start is shared with the
 * episode log, the field statistics and the exit flow.  Rooms first, the motion statistics after:
 * ffm_engine_set_env_rooms (on or off) while they are on returns FFM_E_INVALID and leaves the
 * engine as it was.  Undefined: the affected tau after ffm_engine_set_step_index inside an
 * episode, and after ffm_engine_set_state the origins of the written envs until their next
 * placement (flux, present and moved stay defined: the snapshot is refreshed).  Synchronises the
 * stream. */
#define FFM_MOTION_STATS_MAX_BYTES FFM_FIELD_STATS_MAX_BYTES
int ffm_engine_set_motion_stats(ffm_engine* eng, const int32_t* class_of_env, int32_t n_classes, int32_t curve_bins,
                                void* stream);
/* flux[C][H * W][NB + 1], present[C][bins], moved[C][bins], egress_count[C][H * W] and
 * egress_steps[C][H * W] to the host (any may be NULL).  clear != 0 zeroes them afterwards (the
 * origins stay).  Feature off: FFM_E_INVALID.  Synchronises the stream. */
int ffm_engine_get_motion_stats(ffm_engine* eng, uint64_t* flux, uint64_t* present, uint64_t* moved,
                                uint64_t* egress_count, uint64_t* egress_steps, int32_t clear, void* stream);

/* Per-env parameters and agent counts: a whole sweep in one engine.  Replaces the user's loop
 * over FloorFieldModel(params=...) instances, one per point of an evacuation-time-against-N
 * curve (analyze_steps_by_n.py) or of the (k_S, k_D) plane -- each far too small to fill the
 * GPU, each with its own create and host loop -- by one engine and one launch per step.
 *
 * Env e (global id env_base + e) takes sets[set_of_env[e]] and from then on evolves bit for
 * bit like the env with the same global id of a homogeneous engine created with that set's
 * k_S, k_D, diffuse, decay and n_agents and the same map, SFF, neighbourhood, seed, auto_reset
 * and step indices: positions, counts, DFF bits, episodes and episode-log records.  (Every
 * Philox draw is keyed by (seed, t, global env, agent, purpose); the placement takes the
 * n_agents smallest of keys that do not depend on n_agents.)
 *
 * 1 <= n_sets <= n_envs; set_of_env is a host array [n_envs] of indices into sets.
 * n_sets = 0 turns the feature off: the engine goes back to its create-time parameters,
 * kernel and launch geometry, and the per-env buffer is freed (sets, set_of_env ignored).
 * May be called between steps at any time; stream-ordered on `stream`, the tables are copied
 * before it returns (it synchronises the stream).  Parameters take effect from the next step;
 * a new n_agents at the env's next placement (ffm_engine_reset, ffm_engine_reset_envs or the
 * auto-reset).  Episode indices and the episode log's start indices are untouched.
 * ffm_engine_update_dff uses each env's diffuse / decay.  Trajectory capture, the episode
 * log and fused steps work unchanged.
 *
 * Validated before anything changes: 1 <= n_agents <= min(agent_capacity, free cells),
 * finite parameters, set_of_env entries in [0, n_sets), non-null tables: FFM_E_INVALID.
 * MT engines: FFM_E_UNSUPPORTED.
 *
 * Kernels: the wave kernel has no per-env form.  While the feature is on, a wave engine steps
 * with the block kernel, and a group engine (12x12 default) by default with the lane kernel
 * (step shards, which belong to the group kernel, are then off); both return to their own
 * kernel at n_sets = 0.  ffm_engine_set_env_params_kernel(eng, 1) keeps a group engine on the
 * group kernel's own per-env form instead, step shards included.  Lane, fused and block
 * engines keep their kernel.  (A block engine whose LDS has no 32 bytes per env of its
 * workgroup left: FFM_E_UNSUPPORTED.) */
typedef struct {
    double k_S, k_D, diffuse, decay;
    int32_t n_agents;
    int32_t reserved;
} ffm_env_params;
int ffm_engine_set_env_params(ffm_engine* eng, const ffm_env_params* sets, int32_t n_sets,
                              const int32_t* set_of_env /* host [n_envs] */, void* stream);
/* The tables in effect: *n_sets = 0 while off.  sets (cap entries) and set_of_env ([n_envs])
 * may be NULL; cap < *n_sets: FFM_E_INVALID with *n_sets = count needed. */
int ffm_engine_get_env_params(ffm_engine* eng, ffm_env_params* sets, int32_t cap, int32_t* n_sets,
                              int32_t* set_of_env /* host [n_envs] or NULL */);
/* Which kernel steps a group engine while per-env parameters are on.
 * 0 (default): the lane kernel's per-env form, as before.  1: the group kernel's own per-env
 * form, with step shards.  Sticky; may be called with the feature on or off, between steps.
 * An engine not created on the group kernel, or an MT engine, with mode 1: FFM_E_UNSUPPORTED,
 * nothing changes.  Other modes: FFM_E_INVALID. */
int ffm_engine_set_env_params_kernel(ffm_engine* eng, int32_t mode);

/* Per-env rooms: a geometry sweep (exit width, exit position, obstacles) in one engine, where
 * the reference edits Create_Map.py / Create_SFF.py and re-runs main.py per room.
 *
 * While the feature is on, env e (global id env_base + e) runs in room rooms[room_of_env[e]] and
 * evolves bit for bit like the env with the same global id of a homogeneous engine created with
 * that room's map and SFF and the same neighbourhood, seed, auto_reset and step indices (and,
 * with per-env parameters on as well, that env's parameter set): positions, counts, DFF bits,
 * episodes, counters, episode-log records and trajectory rows.  (Every Philox draw is keyed by
 * (seed, t, global env, agent, purpose); the placement ranks keys indexed by the position in the
 * env's own room's free list, with that room's free-cell count.)
 *
 * maps: host [n_rooms][H*W] uint8 (0 free, 2 wall, 3 exit, as ffm_engine_desc.map);
 * sffs: host [n_rooms][H*W] float32; room_of_env: host [n_envs] indices into the rooms.
 * n_rooms = 0 turns the feature off (create-time room, kernel and launch geometry again).
 *
 * Validated before anything changes; a failed call leaves the engine exactly as it was.
 * FFM_E_INVALID: n_rooms outside 1 <= n_rooms <= n_envs; a free cell on a room's border; a
 * room_of_env entry out of range; null tables; an env whose n_agents -- the create-time one, or
 * its parameter set's while per-env parameters are on -- exceeds the free cells of its own room
 * (ffm_engine_set_env_params makes the same per-env check while rooms are on; turning rooms off
 * checks every set against the create-time room).  FFM_E_UNSUPPORTED: MT engines, float64-SFF
 * engines, and engines on which the lane kernel cannot run (agent_capacity > 32, W % 4 != 0,
 * H*W > 256, or its LDS at the largest room's free-cell count beyond 64 KB).
 *
 * Scope: 12x12 group engines and lane engines.  Wave and block engines take the block kernel's
 * room form, which is opt-in: ffm_engine_set_env_rooms_kernel(eng, 1) below.  Without it this
 * call refuses them as above.  12x12 group engines also have the group kernel's own room form,
 * opt-in as well: ffm_engine_set_env_rooms_kernel(eng, 2).
 *
 * May be called between steps; stream-ordered on `stream`, which it synchronises: the tables are
 * consumed before it returns.  The room holds from the next launch.  An env whose room changes
 * must be re-placed before it is stepped again (ffm_engine_reset, or ffm_engine_reset_envs over
 * those envs; the normal order is create, set_env_rooms, reset).  Stepping agents that were
 * placed in another room gives undefined results for that env but stays memory-safe: every access
 * a step makes stays inside the env's own padded grid, tile and position row, no index is derived
 * from a map code, and the envs stepped after it by the same wave see their own room unchanged.
 *
 * With per-env parameters: the two compose in either call order, with the same bits.  While rooms
 * are on the kernel has a parameter record per env; without ffm_engine_set_env_params the records
 * hold the create-time values.  Each env's placement-candidate threshold is computed with its
 * room's free-cell count by the expression create uses (FFM_RESET_CANDIDATES is honoured).
 * Turning either feature off rebuilds what the other needs.
 *
 * Kernel: while rooms are on the engine steps with the lane kernel's room form (or the block
 * kernel's or the group kernel's: ffm_engine_set_env_rooms_kernel), one launch per
 * step: step shards (but for the group kernel's form, below) and fused steps are off (ffm_engine_set_fused_steps(k > 1) is accepted and
 * ignored meanwhile, as under trajectory capture), and a sticky
 * ffm_engine_set_env_params_kernel(eng, 1) is remembered and resumes when rooms are turned off.
 * Trajectory capture, the episode log and statistics, ffm_engine_reset_envs,
 * ffm_engine_update_dff (map-independent), ffm_engine_get_state / ffm_engine_set_state (which
 * checks positions against the env's own room) and a stream under capture work unchanged. */
int ffm_engine_set_env_rooms(ffm_engine* eng, const uint8_t* maps, const float* sffs, int32_t n_rooms,
                             const int32_t* room_of_env, void* stream);
/* *n_rooms = 0 while off; maps / sffs (cap rooms) and room_of_env may be NULL;
 * cap < *n_rooms: FFM_E_INVALID with *n_rooms = the count needed. */
int ffm_engine_get_env_rooms(ffm_engine* eng, uint8_t* maps, float* sffs, int32_t cap, int32_t* n_rooms,
                             int32_t* room_of_env);
/* The kernel that steps the engine while rooms are on: mode 0 = lane (the create-time default:
 * ffm_engine_set_env_rooms behaves as described above), mode 1 = block -- the block kernel's room
 * form, for rooms beyond the lane kernel's shapes (the reference's 50x50 room, 64x64 with hundreds
 * of agents), mode 2 = group -- the group kernel's room form, the opt-in fast path for geometry
 * sweeps in 12x12 engines.  Sticky: read by the next ffm_engine_set_env_rooms, and independent of
 * ffm_engine_set_env_params_kernel.  FFM_E_INVALID: another value, or rooms are on (turn them off
 * first).
 *
 * Mode 1 is accepted on Philox, float32-SFF engines whose create-time kernel is the wave or the
 * block kernel.  FFM_E_UNSUPPORTED, nothing changed: lane and group engines (they have the lane
 * form), MT and float64-SFF engines, and engines whose block kernel keeps its state in a global
 * scratch region (maps beyond the LDS, `block_scratch`): their padded cell indices do not fit the
 * room table's u16 free lists, and their grid and tile live outside the LDS the room form fills.
 *
 * With mode 1 set, ffm_engine_set_env_rooms validates as above (everything before anything
 * changes), builds the same room table and per-env records, and instead of the lane kernel's
 * conditions checks the block kernel's: its LDS at the create-time K (envs per workgroup) with the
 * largest room's free-cell count plus K * 36 bytes (the K records and room indices), the
 * placement's room for the largest free list, and the counter slots; FFM_E_UNSUPPORTED with
 * nothing changed if one fails.  While on, the engine steps with the block kernel (a wave engine
 * moves to it, as under ffm_engine_set_env_params), fused steps do not apply, and everything
 * said above about composition, resets, the log, capture and update_dff holds.  n_rooms = 0
 * restores the create-time kernel and grid.
 *
 * Mode 2 is accepted on Philox, float32-SFF engines created on the group kernel (12x12,
 * agent_capacity <= 32).  FFM_E_UNSUPPORTED, nothing changed: lane, wave, block and block_scratch
 * engines, MT and float64-SFF engines.
 *
 * With mode 2 set, ffm_engine_set_env_rooms validates as above, builds the same room table and
 * per-env records, and takes the launch geometry of the group kernel's room form: envs per group
 * (2 or 4; FFM_GROUP_ENVS) and step shards (FFM_STEP_SHARDS) from that form's occupancy, as
 * ffm_engine_set_env_params_kernel(eng, 1) does for the per-env form.  The form is the kernel's
 * single-group form only: every launch's grid holds one wave per group, ceil(groups / 4) blocks,
 * whatever is resident, and the diagnostic FFM_WAVE_BLOCKS does not shrink it.  Where those grids
 * have more waves than the counter array has slots, the array is replaced by a larger one with the
 * sums carried over (ffm_engine_device_buffers then reports the new pointer and slot count; it
 * stays for the engine's life).  FFM_E_UNSUPPORTED with nothing changed only if the form's LDS at
 * the largest room's free-cell count exceeds 64 KB.  While on, the engine stays on the group kernel
 * with the bits of the lane form: step shards apply as on a homogeneous group engine (one shard
 * under trajectory capture), fused steps do not, ffm_engine_reset and ffm_engine_reset_envs place
 * from each env's room as in the other forms, and everything said above about composition with
 * ffm_engine_set_env_params (in either order; a remembered ffm_engine_set_env_params_kernel
 * choice stays as it was), the log, capture and update_dff holds.  n_rooms = 0 restores the
 * create-time kernel, grid and shards. */
int ffm_engine_set_env_rooms_kernel(ffm_engine* eng, int32_t mode);

/* counters[4] = {agent_steps, exits, resets, steps} accumulated since create. */
int ffm_engine_get_counters(ffm_engine* eng, uint64_t* counters, void* stream);
int ffm_engine_device_buffers(ffm_engine* eng, ffm_device_buffers* out);
/* Step counter (Philox key component); settable for replay. */
int ffm_engine_get_step_index(ffm_engine* eng, uint32_t* t);
int ffm_engine_set_step_index(ffm_engine* eng, uint32_t t);

/* ---- learning variants (ffm_ac_core / ffm_unified / ffm_actor_only) ----
 *
 * A learner owns E envs of one learning model class plus its V (state value)
 * and H (action preference) tables, shared by all E envs.  Reference entry
 * points each function replaces:
 *   ffm_learner_create        <- __init__   model/ffm_ac_core.py:9-38, model/ffm_unified.py:27-129,
 *                                           model/ffm_actor_only.py:21-79
 *   ffm_learner_reset         <- reset()    model/ffm_ac_core.py:319-325, model/ffm_unified.py:800-812
 *   ffm_learner_step          <- step()     model/ffm_ac_core.py:111-236, model/ffm_unified.py:271-606,
 *                                           model/ffm_actor_only.py:149-409
 *   ffm_learner_{export,import}_table <- get_v_table / set_v_table / get_h_table and the
 *                                        pretrained-critic loaders (model/ffm_unified.py:84-110)
 *   ffm_learner_table_size    <- get_v_table_size / get_h_table_size
 *   ffm_learner_set_epsilon   <- set_epsilon (model/ffm_unified.py:859-867)
 *
 * rng_mode FFM_RNG_MT: the reference's semantics bit for bit (per-env NumPy +
 * CPython streams, agents and table updates in the reference's order; envs are
 * stepped one after another).  FFM_RNG_PHILOX: the batched production step
 * (DESIGN.md section 9): all envs in parallel against the tables as they were at
 * the start of the step, increments summed in 2^-32 fixed point, on-device
 * episode ends (emptied or max_steps) with Philox placement.
 * Learning variants take neighborhood 4 ("neumann", every reference driver) or 8
 * ("moore": nine moves and nine-value H rows, model/ffm_unified.py:173-185,
 * model/ffm_actor_only.py:87-93; in both rng modes) and map values in 0..3.  Table keys are packed u64
 * (ffm_amd/learn_keys.py): 2 bits per cell / rank in [0,26), bx in [26,45),
 * by in [45,64).
 */
enum { FFM_LEARN_CRITIC_ONLY = 0, FFM_LEARN_ACTOR_ONLY = 1, FFM_LEARN_BOTH = 2 };
enum { FFM_TABLE_V = 0, FFM_TABLE_H = 1 };

typedef struct {
    int32_t mode;             /* FFM_LEARN_* (ffm_unified learning_mode; ignored otherwise) */
    double k_A;               /* actor logit scale */
    double alpha_v, alpha_h, gamma;
    double exit_reward, step_penalty, collision_penalty;
    double epsilon;           /* eps-greedy (actor modes) */
    double v_default;         /* value a V read inserts: 0.0 (-1.0 after ffm_ac_core.set_v_table) */
    int32_t block_size;       /* state-key block size (ffm_actor_only: always 5) */
    int32_t max_steps;        /* Philox mode: an episode also ends after this many steps (0 = never) */
    int32_t log2_v_capacity;  /* hash-table slots (0 = 21); hashed tables also keep up to 4
                                 copies of their fixed-point accumulators (V 16 B, H 40 B per
                                 slot and copy), fewer when the copies would pass 256 MiB */
    int32_t log2_h_capacity;
    /* Philox mode, eps_span > 0: each env explores with
     * clip(eps_start + (eps_end - eps_start) * (k + eps_offset) / eps_span, 0, 1) after k ended
     * episodes (run_actor_only_training.py:190-196: offset 0, span total episodes - 1;
     * run_unified_actor_training.py:253-259: offset 1, span episodes per configuration). */
    double eps_start, eps_end, eps_offset, eps_span;
} ffm_learn_desc;

typedef struct ffm_learner ffm_learner;

/* FFM_VARIANT_TRAINED: ffm_learner_import_table(FFM_TABLE_H, ...) loads the trained actor
 * (model/ffm_trained_core.py:51-68); steps read it and never change it. */
int ffm_learner_create(const ffm_engine_desc* desc, const ffm_learn_desc* learn, ffm_learner** out);
int ffm_learner_destroy(ffm_learner* l);
/* Philox: place n_agents in every env (keyed by the step counter, which advances),
 * zero the DFF and the per-env episode counters.  MT: zero the DFF and counts only (the caller uploads
 * positions drawn from its own generators, like ffm_engine_reset). */
int ffm_learner_reset(ffm_learner* l, void* stream);
/* reset(env_mask) of the batched learner (model/ffm_unified.py:800-812 per env; the drivers'
 * per-episode reset, run_unified_actor_training.py:263): the envs whose byte in the DEVICE
 * array `mask` (n_envs bytes) is nonzero are re-placed as ffm_learner_reset places them
 * (Philox keyed by the step counter, which then advances; an env past its episode quota
 * stays empty), their DFF zeroed and their episode step count cleared.  A masked env's
 * position row holds the new placement and 0xFFFF in every slot behind it (an env past its
 * quota: 0xFFFF only), as after ffm_learner_reset.  Not an episode end: nothing is logged or
 * counted, and the tables are untouched.  `mask` is read on `stream` and nowhere else
 * (ffm_engine_reset_envs).  Trajectory capture: a masked env keeps its k and its rows restart
 * at step 1 -- drain before the call.  Between steps only; MT mode: FFM_E_UNSUPPORTED. */
int ffm_learner_reset_envs(ffm_learner* l, const uint8_t* mask, void* stream);
/* Asynchronous: returns once the steps are queued on `stream`.  A hashed V / H
 * table that passes 7/8 load drops the updates that would insert (the step goes
 * on); that condition (FFM_E_NOMEM) is reported exactly at the next sync point
 * (counters, table export / size, get_state) and, without a sync, by the next
 * ffm_learner_step once the previous call's queued flag copy has landed. */
int ffm_learner_step(ffm_learner* l, int32_t n_steps, void* stream);
int ffm_learner_set_state(ffm_learner* l, int64_t env0, int64_t n, const uint16_t* positions,
                          const int32_t* counts, const float* dff, void* stream);
int ffm_learner_get_state(ffm_learner* l, int64_t env0, int64_t n, uint16_t* positions, int32_t* counts,
                          float* dff, void* stream);
/* episodes[n]: completed episodes per env; ep_steps[n]: steps into the current one. */
int ffm_learner_get_episodes(ffm_learner* l, int64_t env0, int64_t n, int32_t* episodes, int32_t* ep_steps,
                             void* stream);
int ffm_learner_set_mt_state(ffm_learner* l, int64_t env, const uint32_t* np_key, int32_t np_pos,
                             const uint32_t* py_key, int32_t py_pos, void* stream);
int ffm_learner_get_mt_state(ffm_learner* l, int64_t env, uint32_t* np_key, int32_t* np_pos,
                             uint32_t* py_key, int32_t* py_pos, void* stream);
int ffm_learner_get_counters(ffm_learner* l, uint64_t* counters, void* stream);
int ffm_learner_set_epsilon(ffm_learner* l, double epsilon);
int ffm_learner_set_v_default(ffm_learner* l, double v_default, void* stream);
int ffm_learner_table_size(ffm_learner* l, int32_t which, int64_t* n, void* stream);
/* Entries in insertion order (= the reference dict's order in MT mode).
 * vals: [cap][1] (V) or [cap][5] (H).  *n receives the entry count; fails if > cap. */
int ffm_learner_export_table(ffm_learner* l, int32_t which, uint64_t* keys, double* vals, int64_t cap,
                             int64_t* n, void* stream);
/* Replace the table by these entries, inserted in the given order. */
int ffm_learner_import_table(ffm_learner* l, int32_t which, const uint64_t* keys, const double* vals,
                             int64_t n, void* stream);
/* ffm_trained_core (FFM_VARIANT_TRAINED only): values of trained H rows the table cannot
 * hold -- rows whose length is not the move count (model/ffm_trained_core.py:228-249: such
 * a state scores as a missing row, zeros) -- that still join the whole-table min / max of
 * the normalisation (:242-267).  n_values values with these min / max (nonfinite: any of
 * them NaN or inf); n_values = 0 clears.  Kept across import_table. */
int ffm_learner_set_h_extra(ffm_learner* l, int64_t n_values, double min, double max, int32_t nonfinite);
/* The batched (Philox) step in phases, for multi-rank runs whose ranks share
 * the tables (ffm_amd/dist.py TableSync):
 *   step_local -> exchange V (and H unless unified actor_only) -> step_apply(V)
 *   -> [unified actor_only: exchange H] -> step_apply(H) (actor variants) -> step_end.
 * ffm_learner_step == the same phases with no exchange.  A delta record is a
 * key (u64) and its pending accumulators (i64 words: V 2 = the fixed-point sum of td
 * and the visit count, H 5 = the fixed-point alpha_h * td sums per action)
 * for every entry inserted or incremented during this step; a rank merges the
 * other ranks' records (inserting missing keys) before applying, so every rank
 * ends the step with the tables a single device holding all envs would have.
 * Record buffers are DEVICE pointers; export fails with *n = the count needed
 * when cap is too small. */
int ffm_learner_step_local(ffm_learner* l, void* stream);
int ffm_learner_step_apply(ffm_learner* l, int32_t which, void* stream);
int ffm_learner_step_end(ffm_learner* l, void* stream);
int ffm_learner_delta_export(ffm_learner* l, int32_t which, uint64_t* d_keys, int64_t* d_acc, int64_t cap,
                             int64_t* n, void* stream);
int ffm_learner_delta_merge(ffm_learner* l, int32_t which, const uint64_t* d_keys, const int64_t* d_acc,
                            int64_t n, void* stream);
/* The same exchange without host synchronisation (multi-rank steps issue no host
 * sync inside the loop): export writes the record count to the DEVICE int64 d_count
 * (records past cap are dropped; count > cap is reported as FFM_E_INVALID at the next
 * sync point or ffm_learner_step); merge reads min(*d_count, cap) records. */
int ffm_learner_delta_export_async(ffm_learner* l, int32_t which, uint64_t* d_keys, int64_t* d_acc, int64_t cap,
                                   int64_t* d_count, void* stream);
int ffm_learner_delta_merge_async(ffm_learner* l, int32_t which, const uint64_t* d_keys, const int64_t* d_acc,
                                  const int64_t* d_count, int64_t cap, void* stream);
/* The tiled step across ranks (ffm_unified, dense tables at block size 1 on large maps,
 * sync period 1): step_tiled_local runs the step and leaves one 16-B record
 * per agent (raster order) and per-env tile offsets in this learner's DEVICE buffers
 * (tiled_buffers: rec_bytes bytes of records, tstart_count uint16 offsets: agent ranks
 * below agent_capacity <= 16383); the ranks
 * all-gather both, rank-major; step_tiled_apply sums every rank's records per tile of
 * cells into the replicated tables (inserting the slots other ranks created) and ends the
 * step.  Every rank holds, bit for bit, the tables one device stepping all envs would hold.
 * Learners of other kinds return FFM_E_UNSUPPORTED. */
int ffm_learner_tiled_buffers(ffm_learner* l, void** d_recs, int64_t* rec_bytes, uint16_t** d_tstart,
                              int64_t* tstart_count);
int ffm_learner_step_tiled_local(ffm_learner* l, void* stream);
int ffm_learner_step_tiled_apply(ffm_learner* l, const void* d_recs_all, const uint16_t* d_tstart_all,
                                 int64_t n_envs_all, void* stream);
/* The owner-sharded tiled step: the tiles of cells are dealt to the ranks
 * (chunks of 64 tiles round-robin) and each rank sums only its own tiles' records, from all
 * ranks, so the per-rank table work does not grow with the rank count.  Every exchange has a
 * fixed size and the counts travel on the device, so the host queues a whole step without
 * waiting for the GPU (ffm_amd/dist.py TableSync).  Per step:
 *   step_owner_local: the step; the records packed tile-major by destination rank into
 *     fixed-capacity blocks (send_recs: rank q's records at [q * send_rec_capacity, + counts[q]);
 *     send_hdr row q: q's tiles' record offsets within its block, hdr_stride u32 per row);
 *   the ranks all-to-all the record blocks (equal splits) and header rows;
 *   step_owner_v: sums this rank's tiles' V (d_recs: the received blocks, rank-major, each
 *     send_rec_capacity records; d_hdrs: the received header rows) and writes the updated V
 *     values to v_slot / v_val (out_counts[0] of them, at most v_capacity);
 *   the ranks all-gather v_capacity entries and the count;
 *   step_owner_h: stores the other ranks' V values; actor modes sum this rank's tiles' H
 *     (h_key = slot (bits 0-23) | action << 24 (0-8: Moore's stay is 8), bit 31 on the first
 *     entry of a row another rank's step
 *     created; h_q = the fixed-point increment; out_counts[1] entries, at most h_capacity)
 *     and write the tiles' H summaries (tsum, tsum_count rows of 5 doubles);
 *   the ranks all-gather h_capacity entries, the count and the summaries;
 *   step_owner_end: inserts the flagged rows, applies the other ranks' H increments and
 *     summaries, the H statistics, ends the step.
 * Counts are DEVICE int64 arrays ([world], rank-major), as are every buffer; "_all"
 * buffers are rank-major with the given row stride in elements.  A count past its capacity
 * is reported at the next sync point (FFM_E_INVALID), never silently dropped.  Every rank
 * ends each step with the H table (keys and values) and the V values one device stepping
 * all envs would hold, bit for bit; the V slots other ranks inserted join a rank's key set
 * when the presence bitmaps are merged (ffm_learner_dense_buffers + dense_adopt, which a
 * shared learner accepts between steps as well): TableSync does so before every export or
 * size query.  set_owner_capacity sizes the buffers (records per destination, V and H output
 * entries); pointers change only there. */
typedef struct ffm_owner_buffers {
    int32_t world, rank;
    void* send_recs;                 /* 16-B records, world blocks of send_rec_capacity */
    int64_t send_rec_capacity;
    uint32_t* send_hdr;
    int64_t hdr_stride;
    int64_t* counts;                 /* [world] records per destination (device) */
    uint32_t* v_slot;
    double* v_val;
    uint32_t* h_key;
    int64_t* h_q;
    int64_t* out_counts;             /* [2] V values, H increments (device) */
    int64_t v_capacity, h_capacity;
    double* tsum;
    int64_t tsum_count;
} ffm_owner_buffers;
int ffm_learner_set_tile_owners(ffm_learner* l, int32_t world, int32_t rank);
int ffm_learner_set_owner_capacity(ffm_learner* l, int64_t rec_capacity, int64_t v_capacity, int64_t h_capacity);
int ffm_learner_owner_buffers(ffm_learner* l, ffm_owner_buffers* b);
int ffm_learner_step_owner_local(ffm_learner* l, void* stream);
/* src_stride: records between two sources' blocks in d_recs (0 = send_rec_capacity: the
 * all-to-all's receive buffer).  set_owner_send_buffer: pack into a caller's device buffer of
 * world * send_rec_capacity records instead (NULL: the learner's own), e.g. one allocation
 * shared by coupled shards, which then read each other's blocks in place. */
int ffm_learner_set_owner_send_buffer(ffm_learner* l, void* d_buf);
/* The V / H outputs written into caller buffers (v_capacity / h_capacity entries, the counts
 * as int64) instead of the learner's own, e.g. rows of the gathered buffers coupled shards
 * read in place; NULLs restore the learner's own.  owner_buffers keeps describing its own. */
int ffm_learner_set_owner_output_buffers(ffm_learner* l, uint32_t* v_slot, double* v_val, int64_t* v_count,
                                         uint32_t* h_key, int64_t* h_q, int64_t* h_count);
int ffm_learner_step_owner_v(ffm_learner* l, const void* d_recs, const uint32_t* d_hdrs, int64_t src_stride,
                             void* stream);
int ffm_learner_step_owner_h(ffm_learner* l, const uint32_t* d_v_slot, const double* d_v_val,
                             const int64_t* d_v_counts, int64_t v_stride, void* stream);
int ffm_learner_step_owner_end(ffm_learner* l, const uint32_t* d_h_key, const int64_t* d_h_q,
                               const int64_t* d_h_counts, int64_t h_stride, const double* d_tsum_all,
                               int64_t tsum_stride, void* stream);
/* Table sync period K >= 1 (default 1 = the reference's per-step updates): the fixed-point
 * increments of K steps accumulate and V / H (and the actor's H statistics) are applied
 * at every K-th step only; a multi-rank run exchanges deltas at those steps only, so
 * sharded == one device at the same K, bit for bit.  apply_due: 1 if the current (or
 * next) step's step_apply applies.  A table export / import or a new period between two
 * applies first applies the pending increments (the period ends at the last step) and
 * restarts the period. */
int ffm_learner_set_sync_period(ffm_learner* l, int32_t period);
int ffm_learner_apply_due(ffm_learner* l, int32_t* due);
/* A learner whose tables are shared with other ranks (TableSync sets it): an export is
 * read-only (the tables as of the last apply: the pending increments are only this rank's),
 * an import or a new period between two applies fails, and the pending increments are
 * applied collectively: flush_begin (*pending = 1 opens a phase in which the deltas are
 * exchanged as in a step) -> exchange V and H -> flush_end (applies them, restarts the
 * period).  *pending = 0: nothing pending, no phase opened. */
int ffm_learner_set_external_sync(ffm_learner* l, int32_t on);
int ffm_learner_flush_begin(ffm_learner* l, int32_t* pending);
int ffm_learner_flush_end(ffm_learner* l, void* stream);
/* Dense (ffm_unified rank-key) tables: the device fixed-point accumulators (acc_count
 * int64) and presence bitmap (present_words u32), for an all-reduce of the increments;
 * dense_adopt then takes the presence union of all ranks (a DEVICE bitmap): slots other
 * ranks inserted get their keys.  Between step_local and step_apply (or, for a tiled learner,
 * between steps). */
int ffm_learner_dense_buffers(ffm_learner* l, int32_t which, int64_t** d_acc, int64_t* acc_count,
                              uint32_t** d_present, int64_t* present_words);
int ffm_learner_dense_adopt(ffm_learner* l, int32_t which, const uint32_t* d_union, void* stream);
/* Philox placement candidates of later resets: `count` distinct free cells (x*W+y) and the
 * agents to place, <= count (the radius curriculum, model/ffm_unified.py:150-171:
 * actual_N = min(N, cells within the radius)).  count = 0 restores every free cell. */
int ffm_learner_set_placement(ffm_learner* l, const uint16_t* cells, int32_t count, int32_t n_agents);
int ffm_learner_set_epsilon_schedule(ffm_learner* l, double eps_start, double eps_end, double eps_offset,
                                     double eps_span);
/* period > 0: global env g explores as if g % period more episodes had ended (k + g % period
 * in the schedule above), so E >= P envs that each run one episode of a configuration cover a
 * P-episode per-configuration schedule (run_unified_actor_training.py:253-259) between them;
 * 0 = off (the default). */
int ffm_learner_set_epsilon_phase(ffm_learner* l, int32_t period);
/* stride >= 1 (default 1): global env g adds (g % period) * stride instead, so envs that each
 * run `stride` episodes cover a run-wide schedule with episodes numbered env-major (the single
 * linear schedule over all episodes of run_actor_only_training.py:186-196). */
int ffm_learner_set_epsilon_stride(ffm_learner* l, int64_t stride);
/* Per-env episode quota of the auto-reset (the drivers' episode counts,
 * run_actor_only_training.py:186-188 / run_unified_actor_training.py:247-252: the run stops
 * after P episodes): env e is re-placed until it has ended caps[e] episodes since the last
 * ffm_learner_reset, then stays empty (no agents, no table reads or increments) until the
 * next reset; caps[e] <= 0 leaves env e empty from the reset on.  n = n_envs (host array)
 * sets the quotas, n = 0 removes them (every env re-placed forever, the default). */
int ffm_learner_set_episode_caps(ffm_learner* l, const int32_t* caps, int64_t n);
/* Ended episodes since the last drain, in no particular order: records of 4 int32
 * {global env, episode index, steps, 1 = emptied / 0 = truncated at max_steps}
 * (the per-episode rows of run_*_training.py's steps_per_episode.csv).  *dropped counts
 * records lost because the log was full (capacity max(16 E, 4096): an env ends at most one
 * episode per step, so draining every 16 steps never loses one). */
int ffm_learner_drain_episodes(ffm_learner* l, int32_t* records, int64_t cap, int64_t* n, int64_t* dropped,
                               void* stream);
/* Trajectory capture of the batched step (replaces run(max_steps, return_trajectory=True),
 * model/ffm_unified.py:902-931 / model/ffm_actor_only.py, and the driver's every-100th-episode
 * trajectory files, run_actor_only_training.py:199-218).  For each selected env (local index)
 * its episode k (0-based, counted from the last ffm_learner_reset) is captured iff
 * (k + phases[i]) % period == 0 (phases NULL: 0).  After every step of a captured episode one
 * row is appended: meta {global env, k, step in the episode (1-based), count} and the
 * agent_capacity cells (x*W+y, live agents first in the reference's order, 0xFFFF after),
 * i.e. the reference's `positions` after that step.  The step counts from the env's current
 * placement; ffm_learner_reset_envs changes no k, so a masked env's rows go on under the same
 * k from step 1 again: drain before a masked reset (consumers sort by env, k, step).  Rows
 * past capacity_rows are dropped and counted.  n_sel = 0 turns capture off.  Batched (Philox)
 * learners only. */
int ffm_learner_set_trajectory_capture(ffm_learner* l, const int32_t* envs, const int32_t* phases, int32_t n_sel,
                                       int32_t period, int64_t capacity_rows, void* stream);
/* Rows captured since the last drain, in no particular order within a step (sort by
 * env, k, step); meta [cap][4] int32, cells [cap][agent_capacity] u16, host pointers. */
int ffm_learner_drain_trajectory(ffm_learner* l, int32_t* meta, uint16_t* cells, int64_t cap, int64_t* n,
                                 int64_t* dropped, void* stream);
int ffm_learner_get_step_index(ffm_learner* l, uint32_t* t);
int ffm_learner_set_step_index(ffm_learner* l, uint32_t t);

/* ---- numerics probes (used by the parity tests) ---------------------- */
/* y[i] = NumPy-exact float32 exp(x[i]) computed on the device; device pointers. */
int ffm_np_expf_device(const float* x, float* y, int64_t n, void* stream);

/* ---- diagnostics ------------------------------------------------------ */
/* The engine-constant stage image of the group step kernel (12x12 rooms, <= 32 agents), copied
 * to the host: the bytes every workgroup copies into its shared memory (the padded map as u8,
 * f32(-k_S) * SFF, the padded free list as u16, the padded map as u16; each region padded with
 * zeros to 16 bytes), then the per-lane geometry tables of the two group sizes.  *n receives
 * the size in bytes (0: the engine steps with another kernel); the copy is made when out is
 * not NULL and cap >= *n. */
int ffm_debug_stage_image(ffm_engine* eng, void* out, int64_t cap, int64_t* n);
/* The placement's candidate pass (free lists of <= 128 cells): only keys below *thr =
 * floor(*m * 2^32 / F) are ranked, *m = min(F, N + max(8, (N + 1) / 2)) unless the environment
 * variable FFM_RESET_CANDIDATES set another count when the engine was created (0: every key is
 * ranked, *thr = 0; *m = F: *thr = 2^32 - 1).  The placements are the same for every *m. */
int ffm_debug_reset_candidates(ffm_engine* eng, int32_t* m, uint32_t* thr);

#ifdef __cplusplus
}
#endif
#endif /* FFM_AMD_H */
