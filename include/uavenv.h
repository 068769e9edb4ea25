/*
 * uavenv.h -- C ABI of the MI355X-native PathPlan_City hot path (libuavenv.so).
 *
 * The reference (young-how/DQN-based-UAV-3D_path_planer) is pure Python and has
 * NO FFI of its own: its plugin boundary is reflection (FactoryClass/EnvFactory.py:12-25,
 * AgentFactory.py:11-27, TrainerFactory.py:10-22) over duck-typed Env/Agent/Trainer
 * objects.  This header is the boundary the build adds UNDER that surface; each entry
 * point names the reference interface it replaces.  The Python plugin classes in
 * dqn_based_uav_3d_path_planer_amd/plugins/ (PathPlan_City, UAV, building, *_Trainer) bind
 * these symbols with ctypes -- see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - every function returns 0 on success or a negative UAVENV_E* code; nothing throws
 *     across the ABI; uavenv_last_error() gives a message for the last failure.
 *   - "dev" pointers are device (HBM) pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); "host" pointers are ordinary host memory, copied synchronously.
 *   - hot-path calls only ENQUEUE work on the caller's stream (void* == hipStream_t,
 *     NULL = default stream); they never synchronise and create no threads.
 *   - agents are indexed i = env * uav_per_env + j  (PathPlan_City.py:59-62: UAV_j of env).
 */
#ifndef UAVENV_H
#define UAVENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVENV_ABI_VERSION 5
#define UAVENV_OBS_DIM 100          /* Agents/UAV.py:517  state_map = zeros(1,1,1,100) */
#define UAVENV_MAX_BUILDINGS 64     /* broad-phase masks are 64-bit */

/* error codes */
#define UAVENV_OK 0
#define UAVENV_EINVAL (-22)
#define UAVENV_ENOMEM (-12)
#define UAVENV_EHIP (-5)            /* a HIP runtime call failed; see uavenv_last_error() */
#define UAVENV_ENODEV (-19)         /* no gfx950 device visible -- there is no CPU fallback */
#define UAVENV_EP2P (-70)           /* the peer-to-peer gradient exchange raised its sticky error (uavenv_p2p_status): this
                                       rank's weights are frozen; fall back to the collective and re-broadcast the weights */

/* info codes written by uavenv_step (Agents/UAV.py:406,465,483,495,509,513) */
#define UAVENV_INFO_NORMAL 0
#define UAVENV_INFO_SUCCESS 1
#define UAVENV_INFO_LOSE 2
#define UAVENV_INFO_SKIPPED 3       /* agent was already done and UAVENV_STEP_SKIP_DONE was set */

/* action encodings accepted by uavenv_step */
#define UAVENV_ACT_STEER_F32 0      /* action[0] in [-1,1] as float  (SAC continuous, Trainer/SAC_Trainer.py:444-448) */
#define UAVENV_ACT_STEER_F64 1      /* same as double (parity tests) */
#define UAVENV_ACT_INDEX_I32 2      /* discrete a in [0,A): steer = -1 + 2a/(A-1)  (the
                                       reference leaves the discrete->steering map undefined; this is ours) */

/* observation storage */
#define UAVENV_OBS_F32 0
#define UAVENV_OBS_F16 1
/* Packed rows: 75 + 5 of the 100 columns are 0/1 occupancy flags and 5 are constant zeros (Agents/UAV.py:517,533-566),
 * so a row is 15 scalars + 80 bits.  20 dwords (80 B) per row, lossless with respect to the f32 row:
 *   dword 0..2 flag words (bit (c & 31) of word (c >> 5) = column c, c in 11..85 and 90..94), dword 3 = 0,
 *   dword 4..14 columns 0..10 (f32), dword 15..18 columns 86..89 (f32), dword 19 = 0.
 * uavenv_obs_unpack expands packed rows to f32 / f16 rows; the fused act / learner kernels read them directly. */
#define UAVENV_OBS_PACKED 2
#define UAVENV_OBS_PACKED_DWORDS 20

/* uavenv_step flags */
#define UAVENV_STEP_AUTO_RESET 1u   /* env whose agents are all done is reset from the scenario bank in the same
                                       launch (replaces PathPlan_City.py:416-417 Scene_Random_Reset per episode) */
#define UAVENV_STEP_SKIP_DONE 2u    /* agents with done==1 do not move (PathPlan_City.py:365-366) */
#define UAVENV_STEP_NO_OBS 4u       /* do not compute/write the observation */
#define UAVENV_STEP_ONE_WAVE 8u     /* diagnostics: small launches also take the one-wavefront-per-64-agents kernel (same results) */
#define UAVENV_STEP_APF_LANE 16u    /* diagnostics: Adjust_subgoal by one lane per agent inside the step kernel instead of the
                                     * separate k_apf_adjust launch (same results) */

typedef struct UavEnv UavEnv;       /* opaque; owns the per-agent state in HBM */

/* Construction parameters: BaseClass/BaseEnv.py:17-22, Agents/UAV.py:22-59, config/UAV.xml. */
typedef struct UavEnvConfig {
    int32_t abi_version;        /* UAVENV_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    int32_t n_envs;             /* independent environments resident on this device */
    int32_t uav_per_env;        /* num_UAV (PathPlan_City.py:55); power of two <= 64 */
    int32_t max_subgoals;       /* K: capacity of each agent's sub-goal list (reference: unbounded, observed <= 34) */
    int32_t max_step;           /* Max_Step */
    int32_t apf_enabled;        /* APF_Enabled (UAV.py:142,448) */
    int32_t obs_dtype;          /* UAVENV_OBS_F32 / UAVENV_OBS_F16 / UAVENV_OBS_PACKED */
    int32_t n_actions;          /* A for UAVENV_ACT_INDEX_I32 (>=2) */
    int32_t reserved0;
    double len, width, h;       /* world box; NOTE Threaten_rate bounds x AND y by `width` (PathPlan_City.py:218) */
    double max_v;               /* int(Max_V) */
    double steering_angle;      /* radians: Steering_angle/180*pi */
    double power[8];            /* P_i v_0 d_0 rho s A P_b F_b  (A gets +0.03 j, xi = 0.8+0.02 j per UAV j) */
    double cell_size;           /* broad-phase grid cell in metres; 0 -> 20 */
} UavEnvConfig;

/* ---- lifetime --------------------------------------------------------------------- */
int uavenv_abi_version(void);
const char *uavenv_last_error(void);
/* replaces PathPlan_City.__init__ + UAV.__init__ state allocation (PathPlan_City.py:31-69) */
int uavenv_create(const UavEnvConfig *cfg, UavEnv **out);
int uavenv_destroy(UavEnv *env);
int uavenv_num_agents(const UavEnv *env);

/* replaces the building list built from buildings.xml (PathPlan_City.py:41-51, building.py:6-11).
 * host_cxcyczRH: nb x 5 doubles; host_vxyz: nb x 3 doubles or NULL (static, stock config). */
int uavenv_set_buildings(UavEnv *env, const double *host_cxcyczRH, const double *host_vxyz, int32_t nb);

/* ---- reset ------------------------------------------------------------------------- */
/* Scenario bank = the part of UAV.reset() that cannot run per step on device yet: start/goal
 * and the RRT sub-goal list (UAV.py:353-360, PathPlan/RRT.py:63-105).
 * host_start_goal: M x 6 (sx,sy,sz,gx,gy,gz); host_subgoals: M x K x 3; host_nsub: M. */
int uavenv_load_scenarios(UavEnv *env, const double *host_start_goal, const double *host_subgoals,
                          const int32_t *host_nsub, int32_t m);
/* The same bank planned ON THE GPU: m scenarios, each = UAV.reset()'s start/goal draws (UAV.py:353-358) + the RRT
 * sub-goal planner (PathPlan/RRT.py:63-105, step 30 m, obstacle test every 5 m), one wavefront per scenario, Philox
 * stream (seed, scenario).  Replaces the env's bank.  The tree is capped at 2048 nodes whatever max_iter is (its nodes
 * live in LDS next to the world; the reference's list is unbounded): a search that fills it counts as "gave up" like one
 * that runs out of iterations.  Scenarios whose planner gave up or whose path does not fit K take the next valid
 * scenario's start / goal / path (this changes the reset distribution by that fraction: read it back with
 * uavenv_bank_stats).  Fails with UAVENV_EINVAL, leaving the old bank in place, when NO scenario could be planned.
 * Synchronises the stream. */
int uavenv_plan_scenarios(UavEnv *env, int32_t m, uint64_t seed, int32_t max_iter, void *stream);
/* Size of the scenario bank in use and how many of its scenarios are copies of a neighbour (0 for a loaded bank). */
int uavenv_bank_stats(const UavEnv *env, int32_t *m, int32_t *replaced);
/* Rolling refresh of the bank while a loop runs -- the reference plans a fresh path at EVERY reset (Agents/UAV.py:327-366 ->
 * PathPlan/RRT.py:63-105); the env kernels reset from a bank, and these calls keep that bank turning over:
 *   uavenv_replan_begin   plans `count` new scenarios for bank rows [first, first + count) into the env's staging area on
 *                         plan_stream.  It touches neither the bank nor an agent, so plan_stream may be a (low-priority) stream
 *                         BESIDE the one the step kernels run on.  Philox stream (seed, row): pass a new seed per refresh.
 *                         One slice in flight at a time (UAVENV_EINVAL otherwise); allocates on its first call.
 *   uavenv_replan_ready   1 = that planning has finished, 0 = still running, -1 = nothing pending (never blocks).
 *   uavenv_replan_commit  enqueues, on `stream` -- the stream of the step kernels, so that no reset runs meanwhile -- the
 *                         hand-over: a row takes its new start / goal / sub-goal list unless an agent currently flies it
 *                         (agents read their list from the bank) or the new plan is unusable (planner gave up / > K nodes);
 *                         such rows keep their old plan and are retried by the next refresh that covers them.  Waits (on the
 *                         stream, not the host) for the planning if it is still running.  force != 0: the caller is about to
 *                         reset EVERY agent (uavenv_reset_all: an episode boundary of the plugin path), so no list is in use
 *                         and every usable plan is taken.
 *   uavenv_replan_stats   out5 = {refreshes begun, rows planned, rows committed, rows skipped: in use, rows skipped: no plan}
 *                         (synchronises).  Every row of a committed slice is counted once; a row that is both in use and
 *                         without a usable plan counts as "in use" (under force no row is in use). */
int uavenv_replan_begin(UavEnv *env, int32_t first, int32_t count, uint64_t seed, int32_t max_iter, void *plan_stream);
int uavenv_replan_ready(UavEnv *env);
int uavenv_replan_commit(UavEnv *env, int32_t force, void *stream);
int uavenv_replan_stats(UavEnv *env, int64_t *out5);
/* "Did this step move anyone?" on the device.  After uavenv_set_moved_word(env, w) every step launch (uavenv_step /
 * uavenv_step_policy) that moves at least one agent -- valid = 1: not skipped as done, not masked out -- stores
 * (uint32_t)uavenv_tick(env) AS RETURNED AFTER THAT CALL into *w (device memory); a launch that moves nobody leaves *w alone.
 * uavenv_dqn_reduce_adam_gated / UavSacAdam.go_word take (w, that value): the learner update behind a step that moved nobody
 * changes nothing -- the reference has left its episode loop by then (Envs/PathPlan_City.py:456-459), the fused plugin path
 * only looks every <done_check> steps.  NULL turns it off. */
int uavenv_set_moved_word(UavEnv *env, uint32_t *dev_word);
uint64_t uavenv_tick(const UavEnv *env);             /* step launches enqueued so far (+ resets: see uavenv_reset_all) */
/* Rows [first, first + count) of the bank in use, into host memory (any pointer may be NULL): start/goal count x 6, sub-goal
 * lists count x K x 3, n_sub count.  Diagnostics / tests; synchronises the device. */
int uavenv_bank_read(UavEnv *env, int32_t first, int32_t count, double *host_start_goal, double *host_subgoals, int32_t *host_nsub);
/* The planner itself, for callers that bring their own start/goal (m x 6, nullable) and/or their own U[0,1) stream
 * (m x stream_len, nullable; parity tests replay CPython's Mersenne stream).  out_nsub < 0: path needs -n > K slots. */
int uavenv_rrt_plan(UavEnv *env, int32_t m, const double *start_goal_dev, const double *uniforms_dev,
                    int32_t stream_len, uint64_t seed, int32_t max_iter, double step_size, double obstacle_step,
                    double *out_start_goal_dev, double *out_sub_dev, int32_t *out_nsub_dev, int32_t *out_iters_dev,
                    void *stream);
/* UAV.reset() (UAV.py:327-366) for every agent: heading ~ U(0,2pi), scenario ~ U{0..M-1} from a
 * counter-based Philox stream keyed by (seed, agent); sub_goals[0] aliases the position as in the reference. */
int uavenv_reset_all(UavEnv *env, uint64_t seed, void *stream);

/* ---- parity injection (tests; synchronous, host pointers) ------------------------- */
/* kin: count x 8 doubles (px,py,pz,vx,vy,gx,gy,gz); V is recomputed with Calc_V semantics (UAV.py:246-253).
 * step/n_sub/alias: count int32 each (alias may be NULL = 0); sub: count x K x 3 doubles. */
int uavenv_set_state(UavEnv *env, int32_t first, int32_t count, const double *kin, const int32_t *step,
                     const int32_t *n_sub, const int32_t *alias, const double *sub);
/* out16: count x 16 doubles = [px,py,pz,vx,vy,V,gx,gy,gz,Step,done,n_sub,score,total_score,path_len,reach_goal];
 * out_sub (nullable): count x K x 3 remaining sub-goals, current first; out_alias (nullable): count int32. */
int uavenv_get_state(UavEnv *env, int32_t first, int32_t count, double *out16, double *out_sub, int32_t *out_alias);

/* ---- hot path ---------------------------------------------------------------------- */
/* One UAV.update_PathPlan(action) (UAV.py:397-513) + UAV.state_PathPlan() (UAV.py:515-567) for every
 * agent, i.e. BaseEnv.Move_Agent (BaseEnv.py:123-137) vectorised.  All output pointers are nullable.
 *   actions_dev   N elements of the type selected by action_kind
 *   obs_dev       N x 100 (f32 or f16 per cfg.obs_dtype): the state AFTER the step (after the reset if
 *                 AUTO_RESET fired) -- point it at replay frame t+1 to fuse ReplayMemory.add (replay_buffer.py:41-42)
 *   reward64/32   global_r as double / float (the reference stores FloatTensor([[reward]]), PathPlan_City.py:377)
 *   ret_done      the `done` RETURNED by update (goes into replay); agent_done = self.done (ends the episode)
 *   valid         0 for skipped agents, else 1
 *   energy64      Calc_Fly_Power at the post-step speed (UAV.py:239-245), J per unit-time step
 *   active        nullable N-byte mask; agents with 0 are left untouched (info SKIPPED, valid 0) -- this is how
 *                 BaseEnv.Move_Agent(index, action) moves ONE agent of the batch
 * Teams (uav_per_env = U > 1; agent i is UAV i mod U of env i / U; held to oracle/team_model.py by
 * tests/test_team_protocol_gpu.py): an agent that is done and waits (SKIP_DONE) or that `active` leaves out reports
 * info SKIPPED, valid 0, ret_done = agent_done = its done flag, reward 0, and its state is not written.  Under AUTO_RESET the
 * env restarts in the launch after which all U of its agents are done: a masked agent that is done counts towards that, a
 * masked agent that is not done blocks it.  The restart re-draws EVERY agent of the env in that launch -- waiting and masked
 * ones too (their outputs still describe them as skipped; obs is the fresh state's).  Without SKIP_DONE a done agent
 * steps on (and stays done); the env still restarts only when complete.  energy64 uses UAV (i mod U)'s A and xi.
 */
int uavenv_step(UavEnv *env, const void *actions_dev, int32_t action_kind, void *obs_dev, double *reward64_dev,
                float *reward32_dev, uint8_t *ret_done_dev, uint8_t *agent_done_dev, uint8_t *info_dev,
                uint8_t *valid_dev, double *energy64_dev, const uint8_t *active_dev, uint32_t flags, void *stream);
/* uavenv_dqn_act + uavenv_step in ONE launch: the actions are computed in the step kernel's prologue from the packed
 * observation rows of the current frame (obs_cur_dev: N x 20 dwords, e.g. replay frame t) with the same forward pass and
 * the same epsilon-greedy stream as uavenv_dqn_act(net, obs_cur, ..., seed, counter) -- bit-identical actions -- and are
 * also written to action_out_dev (N int32, e.g. the replay's action plane of frame t).  Everything else as uavenv_step.
 * Takes packed-row envs of <= 49 152 agents without APF and nets with <= 4 layer-2 outputs on the f32 MFMA; returns
 * UAVENV_EINVAL otherwise (callers then issue the two calls). */
struct UavDqnNet;
int uavenv_step_policy(UavEnv *env, const struct UavDqnNet *net, const void *obs_cur_dev, float eps, uint64_t seed,
                       uint64_t counter, int32_t *action_out_dev, void *obs_dev, double *reward64_dev, float *reward32_dev,
                       uint8_t *ret_done_dev, uint8_t *agent_done_dev, uint8_t *info_dev, uint8_t *valid_dev,
                       double *energy64_dev, const uint8_t *active_dev, uint32_t flags, void *stream);
/* Diagnostics: when dev_buf != NULL, wave w of uavenv_step writes 8 s_memtime stamps to dev_buf[8*w .. 8*w+7]
 * (start, world staged, state landed, step done, reset done, obs computed, stores issued, stores retired). */
int uavenv_set_debug_buffer(UavEnv *env, unsigned long long *dev_buf);
/* UAV.state_PathPlan() only (UAV.py:515-567), e.g. the first observation after a reset. */
int uavenv_observe(UavEnv *env, void *obs_dev, void *stream);
/* PathPlan_City.Threaten_rate (PathPlan_City.py:215-223) for n points: xyz_dev n x 3 doubles -> out_dev n bytes. */
int uavenv_threaten_rate(UavEnv *env, const double *xyz_dev, uint8_t *out_dev, int64_t n, void *stream);
/* BaseClass/CalMod.py:89-102 calculate_angle(a, b) (atan2 -> degrees -> (x + 360) % 360 -> radians, in [0, 2 pi)) and
 * :64-65 Eu_Loc_distance(a, b) for n point pairs, computed by the device functions the step kernels use.
 * ab_dev: n x 6 doubles (ax, ay, az, bx, by, bz); either output nullable. */
int uavenv_geometry(const double *ab_dev, double *angle_out_dev, double *dist_out_dev, int64_t n, void *stream);
/* Same, bypassing the broad-phase grid (all-pairs); used to prove the culling is exact. */
int uavenv_threaten_rate_allpairs(UavEnv *env, const double *xyz_dev, uint8_t *out_dev, int64_t n, void *stream);

/* ---- device replay ring + acting (BaseClass/replay_buffer.py:28-54) ----------------- */
/* The ring is caller-owned HBM, frame-major: frame t holds obs[t] = state BEFORE action t, plus
 * action/reward/done/valid of transition t; next_state of (t,i) is obs[(t+1) % frames][i]. */
typedef struct UavReplayRing {
    void *obs;            /* frames x N x 100, f32 or f16 -- or frames x N x 20 dwords, packed */
    void *action;         /* frames x N, float steer or int32 index */
    float *reward;        /* frames x N */
    uint8_t *done;        /* frames x N  (returned done) */
    uint8_t *valid;       /* frames x N */
    int32_t frames;
    int32_t n_agents;
    int32_t obs_dtype;
    int32_t action_is_index;
    void *meta;           /* ABI 5, nullable: frames x N transition records of 16 bytes {a1, a0, reward, flags} -- the action as the step
                             consumed it (int32 index or f32 steer bits; a1 = the second SAC action component or 0), the f32 reward, and
                             done | valid << 8 | info << 16 -- written by the step kernels next to the planes above (uavenv_set_step_meta).
                             A learner that finds it gathers ONE 16-byte record per sample instead of a line each from the action, reward,
                             done and valid planes (round 5: those four scattered loads were ~45 % of a gradient launch's HBM fetch);
                             the planes stay the source of truth for everything else.  NULL: the kernels read the planes. */
} UavReplayRing;
#define UAVENV_META_BYTES 16
/* The next step launch of this env (uavenv_step / uavenv_step_policy; ONE launch, then forgotten) also writes the transition records
 * of its N agents to meta_frame_dev (N x UAVENV_META_BYTES: the frame of a ring's `meta` that its reward / done pointers aim at);
 * action1_frame_dev (nullable, N floats): the second action component to put into the records (SAC_Trainer.get_action's
 * action[1], :444-448, which the step itself never reads).  NULL meta: nothing is written (the default). */
int uavenv_set_step_meta(UavEnv *env, void *meta_frame_dev, const float *action1_frame_dev);

/* ReplayMemory.sample2 = random.sample(memory, batch) (replay_buffer.py:48-51) on device: `batch` DISTINCT stored
 * transitions (frame, agent) out of the `filled` frames preceding `head` -- the first `batch` images of a keyed
 * pseudo-random permutation of the filled * n_agents transitions (Feistel network keyed by Philox(seed, counter);
 * batch > filled * n_agents wraps around, where the reference raises) -- gathered into
 * contiguous batch buffers: obs_b/next_obs_b batch x 100 (ring dtype; packed rings give packed rows), action_b batch (ring type),
 * reward_b batch f32, done_b batch f32 (0/1), valid_b batch f32 (0/1). */
int uavenv_replay_sample(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed,
                         uint64_t counter, void *obs_b, void *next_obs_b, void *action_b, float *reward_b,
                         float *done_b, float *valid_b, void *stream);

/* Expand n packed rows (UAVENV_OBS_PACKED) into n x 100 f32 (out_dtype UAVENV_OBS_F32) or f16 rows. */
int uavenv_obs_unpack(const void *packed_dev, int64_t n, void *out_dev, int32_t out_dtype, void *stream);

/* The draws alone: frame_agent_out_dev[2*s], [2*s+1] = (frame, agent) of sample s, s < batch -- exactly the
 * transitions uavenv_replay_sample / uavenv_dqn_grad use for the same (seed, counter, head, filled). */
int uavenv_replay_draw(int32_t frames, int32_t n_agents, int32_t head, int32_t filled, int32_t batch, uint64_t seed,
                       uint64_t counter, int32_t *frame_agent_out_dev, void *stream);
/* The same draws over VALID rows only -- the reference's buffers never hold a row of a finished agent (run_eposide stops pushing
 * for it, Envs/PathPlan_City.py:456-459; BaseClass/replay_buffer.py:41-51), the ring keeps such rows with valid = 0.  (frame, env)
 * pairs for n_slots UAV slots at once: slot first_slot + j takes draws [j * batch, (j + 1) * batch) and tests ITS row
 * valid_dev[(frame * n_envs + env) * uav_per_env + slot] (the ring's valid plane).  Try t of draw s looks at permutation position
 * (s mod D) + t S (D = filled * n_envs stored rows, S = n_slots * batch) while that is below D and t < max_tries, and the draw
 * takes the first valid row: rejection sampling over a bijection -- uniform over the valid rows, distinct within a slot while
 * batch <= D.  With every row valid the result equals uavenv_replay_draw(batch * n_slots) for every S and D: S > D wraps as
 * it does there (s mod D), so every pair names a stored row.  A draw that finds no valid row keeps the row of its try 0 (weight
 * 0 in the update through the valid plane). */
#define UAVENV_DRAW_MAX_TRIES 8
int uavenv_replay_draw_valid(int32_t frames, int32_t n_envs, int32_t head, int32_t filled, int32_t batch, int32_t n_slots,
                             int32_t uav_per_env, int32_t first_slot, const uint8_t *valid_dev, int32_t max_tries, uint64_t seed,
                             uint64_t counter, int32_t *frame_env_out_dev, void *stream);
/* The draws of all uav_per_env slots as (frame, AGENT) pairs, one launch: slot j's draws [j * batch, (j + 1) * batch) are written as
 * (frame, env * uav_per_env + j) -- uavenv_dqn_grad takes slice j as its explicit pairs.  Frame and env are those of
 * uavenv_replay_draw_valid(frames, n_envs, head, filled, batch, uav_per_env, uav_per_env, 0, valid_dev, max_tries, seed, counter)
 * with a valid plane, and of uavenv_replay_draw(frames, n_envs, head, filled, uav_per_env * batch, seed, counter) with
 * valid_dev NULL (max_tries is not looked at then). */
int uavenv_replay_draw_slots(int32_t frames, int32_t n_envs, int32_t head, int32_t filled, int32_t batch, int32_t uav_per_env,
                             const uint8_t *valid_dev, int32_t max_tries, uint64_t seed, uint64_t counter,
                             int32_t *frame_agent_out_dev, void *stream);

/* epsilon-greedy over Q-values (Trainer/DuelingDQN_Trainer.py:86-97): q_dev N x A f32 (row-major).
 * Writes the chosen index (int32, nullable) and its steering value (f32, nullable). */
int uavenv_select_actions(const float *q_dev, int32_t n, int32_t n_actions, float eps, uint64_t seed,
                          uint64_t counter, int32_t *index_out_dev, float *steer_out_dev, void *stream);

/* ---- prioritised replay (BaseClass/replay_buffer.py:57-223: SumTree + ReplayTree) on the device -------------------- */
/* Priorities are a flat f64 array, one per data slot (for the replay ring: slot = frame * N + agent); selection is a
 * two-level prefix search instead of a tree walk.  chunk_sum / chunk_prefix are scratch the caller allocates:
 * uavenv_per_num_chunks(capacity) and that + 1 doubles.  rot = uavenv_per_rotation(capacity): the flat-array SumTree
 * visits its leaves rotated by that many slots when the capacity is not a power of two (0 reproduces plain slot
 * order). */
typedef struct UavPer {
    double *prio;          /* [capacity] */
    double *chunk_sum;     /* [num_chunks] */
    double *chunk_prefix;  /* [num_chunks + 1]; the last entry is the total priority */
    int64_t capacity;
    int64_t rot;
    double *group_sum;     /* nullable [num_chunks * 64]: sums of 16 consecutive in-order leaves, written by the rebuild; with
                              it a sample reads 64 + 16 doubles instead of 1 024 (same selection, bit for bit) */
} UavPer;

int uavenv_per_num_chunks(int64_t capacity);
int uavenv_per_rotation(int64_t capacity);
/* Recompute the chunk sums and their prefix after priorities changed (SumTree.update's propagation, :68-79). */
int uavenv_per_rebuild(const UavPer *per, void *stream);
/* ReplayTree.sample (:146-180), selection part: sample i takes v_i = draws_dev[i], or -- draws_dev NULL --
 * uniform(seg*i, seg*(i+1)) with seg = int(total)/batch from Philox(seed, counter); out_slot_dev[i] = the slot whose
 * leaf the tree descent (:99-115) reaches, out_prio_dev[i] (nullable) its priority.  Needs a current rebuild. */
int uavenv_per_sample(const UavPer *per, int32_t batch, const double *draws_dev, uint64_t seed, uint64_t counter,
                      int64_t *out_slot_dev, double *out_prio_dev, void *stream);
/* prio[slots[i]] = min(|abs_err[i]| + epsilon, clip) ** alpha   (batch_update :215-222; clip <= 0: no clip = push :143).
 * With clip > 0 a slot whose priority is 0 -- an empty leaf: a retired or never-valid ring row -- is left at 0.
 * A slot listed several times takes the LAST of its errors, as the reference's sequential loop does.
 * PRECONDITION: equal entries of slots_dev are ADJACENT -- true of every list uavenv_per_sample returns (stratified draws come
 * back in prefix order).  Non-adjacent duplicates race (which error wins is undefined): a caller with an arbitrary list sorts it by
 * slot first, stably (replay.DevicePER.update does). */
int uavenv_per_set(const UavPer *per, const int64_t *slots_dev, const double *abs_err_dev, int32_t n, double epsilon,
                   double alpha, double clip, void *stream);
/* prio[first .. first+count) = priority where valid_dev[i] != 0 (or everywhere if NULL), 0 elsewhere: the slots of a
 * ring frame k_step has just written. */
int uavenv_per_fill(const UavPer *per, int64_t first, int64_t count, double priority, const uint8_t *valid_dev,
                    void *stream);
/* The two fills of a replay step in ONE launch: the frame k_step has just written ([first, first + count): `priority` where
 * valid_dev[i] != 0, 0 elsewhere) and the frame that became the ring's head ([retire_first, retire_first + count) <- 0). */
int uavenv_per_fill_frame(const UavPer *per, int64_t first, int64_t count, double priority, const uint8_t *valid_dev,
                          int64_t retire_first, void *stream);
/* uavenv_per_fill_frame with the valid flag of slot first + i at valid_dev[i * valid_stride]: one UAV slot's column of a frame's
 * valid plane (rows e * uav_per_env + slot; each SAC trainer keeps its own tree over its slot's transitions). */
int uavenv_per_fill_frame_strided(const UavPer *per, int64_t first, int64_t count, double priority, const uint8_t *valid_dev,
                                  int64_t valid_stride, int64_t retire_first, void *stream);
/* uavenv_per_fill_frame + uavenv_per_rebuild with the fills applied while the rebuild reads the priorities (one launch less). */
int uavenv_per_rebuild_frame(const UavPer *per, int64_t first, int64_t count, double priority, const uint8_t *valid_dev,
                             int64_t retire_first, void *stream);
/* uavenv_per_set with f32 errors (what uavenv_dqn_grad_w / uavenv_sac_critic_grad write). */
int uavenv_per_set_f32(const UavPer *per, const int64_t *slots_dev, const float *abs_err_dev, int32_t n, double epsilon,
                       double alpha, double clip, void *stream);
/* ... that leaves every priority alone unless *go_word_dev == go_value when it runs (uavenv_set_moved_word): batch_update belongs
 * to an update, and there is none behind a step that moved nobody. */
int uavenv_per_set_f32_gated(const UavPer *per, const int64_t *slots_dev, const float *abs_err_dev, int32_t n, double epsilon,
                             double alpha, double clip, const uint32_t *go_word_dev, uint32_t go_value, void *stream);
/* ReplayTree.sample (:163-178), the part after the selection: is_weights[i] = (n_entries * p_i / int(total)) ** -beta,
 * divided by their maximum (f32 out); a zero priority gets weight 0; int(total) < 1 counts as 1.  Also splits each slot
 * into the (frame, agent) pair uavenv_dqn_grad takes (frame_agent_out_dev nullable, batch x 2 int32; slot = frame *
 * n_agents + agent).  prio_dev: the batch priorities uavenv_per_sample returned FOLLOWED by (batch + 255) / 256 doubles of
 * scratch; the call overwrites all of it.  Needs the rebuild uavenv_per_sample used.  n_entries <= 0 has no meaning (the
 * reference never samples an empty tree, and 0 ** -beta would turn the whole batch into NaN): UAVENV_EINVAL, nothing is written. */
int uavenv_per_weights(const UavPer *per, const int64_t *slots_dev, double *prio_dev, int32_t batch,
                       int64_t n_entries, double beta, int32_t n_agents, float *is_weights_out_dev,
                       int32_t *frame_agent_out_dev, void *stream);
/* ---- the same for one tree per UAV slot in ONE launch per phase (grid x n_slots; tree j = pers[j], a HOST array of n_slots
 * pointers).  Slice j of each launch is the per-tree kernel on tree j: every result is bit for bit what the per-tree entry point
 * named below gives for pers[j].  UAVENV_EINVAL, with nothing enqueued (no device is touched), for: n_slots < 1 or
 * > UAVENV_DQN_MAX_SLOTS; a NULL tree or one the per-tree entry refuses; capacities that differ; rot != 0; group_sum on some trees
 * only; two trees sharing `prio`; batch <= 0; n_entries <= 0. */
/* uavenv_per_fill_frame_strided(pers[j], first, count, priority, valid_dev + j, n_slots, retire_first) for every j: slot j reads the
 * flag of tree slot first + i at valid_dev[i * n_slots + j] (its column of a frame's valid plane). */
int uavenv_per_fill_frame_slots(const UavPer *const *pers, int32_t n_slots, int64_t first, int64_t count, double priority,
                                const uint8_t *valid_dev, int64_t retire_first, void *stream);
/* uavenv_per_rebuild_frame for every tree, the flags read as above: two launches, grids (num_chunks, n_slots) and (1, n_slots).
 * count == 0: a plain uavenv_per_rebuild. */
int uavenv_per_rebuild_slots(const UavPer *const *pers, int32_t n_slots, int64_t first, int64_t count, double priority,
                             const uint8_t *valid_dev, int64_t retire_first, void *stream);
/* uavenv_per_sample(pers[j], batch, NULL, seed + j, counter, out_slot_dev + j * batch, out_prio_dev + j * (batch + (batch + 255) / 256))
 * for every j: out_slot_dev [n_slots][batch], out_prio_dev (nullable) [n_slots][batch + (batch + 255) / 256] -- the row uavenv_per_weights takes. */
int uavenv_per_sample_slots(const UavPer *const *pers, int32_t n_slots, int32_t batch, uint64_t seed, uint64_t counter,
                            int64_t *out_slot_dev, double *out_prio_dev, void *stream);
/* uavenv_per_weights for every tree on row j of slots_dev / prio_dev (the layouts above): weights normalised by slot j's own maximum
 * and the floor of slot j's own total, into is_weights_out_dev [n_slots][batch].  pairs_out_dev (nullable, [n_slots][batch][2]): tree j
 * covers UAV slot j's column of the ring (tree slot s = frame * n_envs + env), and the pair written is
 * (s / n_envs, (s % n_envs) * n_slots + j) -- (frame, AGENT), what uavenv_dqn_grad takes and uavenv_replay_draw_slots writes. */
int uavenv_per_weights_slots(const UavPer *const *pers, int32_t n_slots, const int64_t *slots_dev, double *prio_dev, int32_t batch,
                             int64_t n_entries, double beta, int32_t n_envs, float *is_weights_out_dev, int32_t *pairs_out_dev,
                             void *stream);
/* uavenv_per_set_f32_gated(pers[j], slots_dev + j * batch, abs_err_dev + j * batch, batch, ...) for every j, one gate word for all.
 * The last of a run of equal slots writes, and a run lies within one slot's batch entries: the last entry of slot j and the first of
 * slot j + 1 belong to different trees whatever numbers they hold. */
int uavenv_per_set_f32_slots_gated(const UavPer *const *pers, int32_t n_slots, const int64_t *slots_dev, const float *abs_err_dev,
                                   int32_t batch, double epsilon, double alpha, double clip, const uint32_t *go_word_dev,
                                   uint32_t go_value, void *stream);

/* ---- fused DQN-family learner for the reference's Q-MLPs (BaseClass/BaseCNN.py:93-139, w=100, hid=64) ---------- */
/* Flat f32 parameter blocks in HBM (16-byte aligned), layout [W1 hid*w][b1 hid][W2 n2*hid][b2 n2] with n2 = n_actions
 * (+1 value row for the dueling VAnet2: rows 0..A-1 = fc_A, row A = fc_V).  m / v are Adam's moments (same layout). */
#define UAVENV_MFMA_F32 0            /* f32 operands on v_mfma_f32_16x16x4_f32: the reference's precision */
#define UAVENV_MFMA_F16 1            /* f16 operands (fc1 weights, observations, H / dH of the gradient products) on
                                        v_mfma_f32_16x16x32_f16, f32 accumulate; master weights, Adam, layer 2, the TD target
                                        and the loss stay f32.  f16 / packed rings, at most 4 layer-2 outputs. */
typedef struct UavDqnNet {
    float *local;     /* q_local  */
    float *target;    /* q_target */
    float *m, *v;
    int32_t w, hid, n_actions, dueling;
    int32_t mfma_dtype;   /* UAVENV_MFMA_F32 / UAVENV_MFMA_F16: operand type of the fused kernels' matrix products */
    int32_t reserved0;
} UavDqnNet;

int uavenv_dqn_num_params(const UavDqnNet *net);
/* Diagnostics (UAVENV_PHASE_PROFILE builds): 8 s_memtime stamps per workgroup of uavenv_dqn_grad; NULL disables. */
int uavenv_dqn_set_debug_buffer(unsigned long long *dev_buf);
/* Partial-gradient scratch: uavenv_dqn_partial_rows(batch) rows of uavenv_dqn_partial_stride(net) floats (a multiple
 * of 32, so rows keep the base's alignment; base 16-byte aligned at least, 128 for the fewest fetches); row layout = the parameter layout, then loss sum and valid count at [num_params], [num_params + 1]. */
int uavenv_dqn_partial_stride(const UavDqnNet *net);
int uavenv_dqn_partial_rows(int32_t batch);
/* One learn_off_policy() gradient (Trainer/DQN_Trainer.py:93-121, DDQN_Trainer.py:84-105): draws `batch` transitions
 * (batch % 64 == 0) with the SAME permutation as uavenv_replay_sample (or takes explicit (frame, agent) pairs),
 * gathers them from the ring, forward/backward on the f32 MFMA.  kind 0: max_a Q_target(s'); 1: double-DQN.
 * Writes the partial rows described above (gradient sums, loss sum, valid count). */
int uavenv_dqn_grad(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed,
                    uint64_t counter, const int32_t *explicit_idx_dev, const UavDqnNet *net, int32_t kind, float gamma,
                    int32_t huber, float *partials_dev, void *stream);
/* The same with prioritised replay (BaseClass/replay_buffer.py:146-223, Trainer/SAC_Trainer.py:336-352 applied to the
 * DQN family): is_weights_dev (nullable, batch f32) = the importance-sampling weight of sample s -- the loss becomes
 * mean_s w_s loss_s --, abs_td_out_dev (nullable, batch f32) receives |Q(s, a) - y| of sample s for ReplayTree.batch_update.
 * With both NULL this IS uavenv_dqn_grad (bit for bit). */
int uavenv_dqn_grad_w(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed,
                      uint64_t counter, const int32_t *explicit_idx_dev, const UavDqnNet *net, int32_t kind, float gamma,
                      int32_t huber, const float *is_weights_dev, float *abs_td_out_dev, float *partials_dev, void *stream);
/* n_partials = uavenv_dqn_partial_rows(batch).  Sum the partial rows -> raw_out_dev[num_params + 2] = gradient sums, loss sum, valid-sample count.  This flat vector
 * is the RCCL all-reduce(sum) payload for multi-GPU (the mean is then over the valid samples of all ranks). */
int uavenv_dqn_reduce(const UavDqnNet *net, const float *partials_dev, int32_t n_partials, float *raw_out_dev,
                      void *stream);
/* grad = raw / max(count, 1); torch.optim.Adam step t (1-based) on q_local; hard_update != 0 also copies the new
 * weights into q_target (DQN_Trainer.py:121-130,138-141); loss_out_dev (nullable) receives the mean loss. */
int uavenv_dqn_adam(const UavDqnNet *net, const float *raw_dev, float lr, float beta1, float beta2, float eps,
                    int32_t step_t, int32_t hard_update, float *loss_out_dev, void *stream);
/* Single-GPU fast path: uavenv_dqn_reduce + uavenv_dqn_adam in ONE launch (raw_out_dev nullable). */
/* uavenv_dqn_reduce_adam that changes NOTHING (weights, moments, target, loss) unless *go_word_dev == go_value when it runs
 * (uavenv_set_moved_word); go_word_dev NULL = always. */
int uavenv_dqn_reduce_adam_gated(const UavDqnNet *net, const float *partials, int32_t n_partials, float lr, float beta1,
                                 float beta2, float eps, int32_t step_t, int32_t hard_update, float *loss_out, float *raw_out,
                                 const uint32_t *go_word_dev, uint32_t go_value, void *stream);
int uavenv_dqn_reduce_adam(const UavDqnNet *net, const float *partials_dev, int32_t n_partials, float lr, float beta1,
                           float beta2, float eps, int32_t step_t, int32_t hard_update, float *loss_out_dev,
                           float *raw_out_dev, void *stream);
/* Q(s) for n envs + epsilon-greedy in one launch (DuelingDQN_Trainer.py:86-97); q_out_dev nullable [n][A]. */
int uavenv_dqn_act(const UavDqnNet *net, const void *obs_dev, int32_t obs_dtype, int32_t n, float eps, uint64_t seed,
                   uint64_t counter, int32_t *index_out_dev, float *steer_out_dev, float *q_out_dev, void *stream);
/* The same for one net per UAV slot in ONE launch: obs_dev holds n_envs * n_nets packed rows (UAVENV_OBS_PACKED only), agent
 * e * n_nets + j is flown by nets[j] (host array).  index_out_dev [n_envs * n_nets] and q_out_dev (nullable, [n_envs * n_nets][A])
 * are indexed by agent.  For agent e * n_nets + j the action and the Q row are bit for bit what
 * uavenv_dqn_act(nets[j], rows j, j + n_nets, ... gathered contiguously, UAVENV_OBS_PACKED, n_envs, eps, seed + j, counter, ...)
 * gives at index e: the draw is Philox(seed + j (mod 2^64); e, counter, 0xac7).  UAVENV_EINVAL, with nothing enqueued, for
 * n_nets < 1 or > UAVENV_DQN_MAX_SLOTS, a NULL net, another obs_dtype, an f16-MFMA net, nets that differ in n_actions or dueling,
 * a head uavenv_dqn_act refuses, a `local` or obs_dev off 16 bytes, n_envs <= 0. */
#define UAVENV_DQN_MAX_SLOTS 8
int uavenv_dqn_act_slots(const UavDqnNet *const *nets, int32_t n_nets, const void *obs_dev, int32_t obs_dtype, int32_t n_envs,
                         float eps, uint64_t seed, uint64_t counter, int32_t *index_out_dev, float *q_out_dev, void *stream);
/* The learning half for one net per UAV slot: uavenv_dqn_grad for n_nets nets in ONE launch (grid rows x n_nets).  All slots read
 * the one packed ring; slot j trains nets[j] (host array) on ITS batch (frame, agent) pairs pairs_dev[j][batch][2] -- explicit and
 * mandatory, uavenv_replay_draw_slots' layout -- and writes partials[j] (host array of device pointers), each
 * uavenv_dqn_partial_rows(batch) x uavenv_dqn_partial_stride(net) floats.  Row x of partials[j] is bit for bit the row that
 * uavenv_dqn_grad(ring, head, filled, batch, seed, counter, pairs_dev + j * batch * 2, nets[j], kind, gamma, huber, partials[j])
 * writes.  UAVENV_EINVAL, with nothing enqueued, for whatever uavenv_dqn_grad refuses of any slot and for: n_nets < 1 or
 * > UAVENV_DQN_MAX_SLOTS; a ring that is not UAVENV_OBS_PACKED; an f16-MFMA net; more than 4 layer-2 outputs (n_actions + dueling);
 * nets that differ in n_actions or dueling; pairs_dev NULL or off 8 bytes; a partials entry NULL or off 16 bytes; two slots sharing
 * `local` or a partials buffer. */
int uavenv_dqn_grad_slots(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed, uint64_t counter,
                          const int32_t *pairs_dev, const UavDqnNet *const *nets, int32_t n_nets, int32_t kind, float gamma,
                          int32_t huber, float *const *partials, void *stream);
/* uavenv_dqn_grad_slots under prioritised replay: slot j also takes its importance weights is_weights_dev[j][batch] and writes
 * |Q(s, a) - y| of its samples to abs_td_out_dev[j][batch] (both mandatory, f32, slot-major).  Row x of partials[j] and row j of
 * abs_td_out_dev are bit for bit what uavenv_dqn_grad_w(ring, ..., pairs_dev + j * batch * 2, nets[j], kind, gamma, huber,
 * is_weights_dev + j * batch, abs_td_out_dev + j * batch, partials[j]) writes.  Refuses what uavenv_dqn_grad_slots refuses. */
int uavenv_dqn_grad_slots_w(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed, uint64_t counter,
                            const int32_t *pairs_dev, const UavDqnNet *const *nets, int32_t n_nets, int32_t kind, float gamma,
                            int32_t huber, const float *is_weights_dev, float *abs_td_out_dev, float *const *partials, void *stream);
/* uavenv_dqn_reduce_adam_gated for n_nets nets in ONE launch (grid (num_params + 2 + 31) / 32 x n_nets): slot j sums its
 * n_partials rows of partials[j] and takes Adam step step_t[j] (host array, each > 0: the slots' update counts may differ) with
 * the hard target copy where hard_update[j] != 0 (host array); loss_out (host array, nullable as a whole and per entry) holds
 * the slots' device loss cells.  One gate for all slots.  Parameters, moments, target and loss of slot j are bit for bit those of
 * uavenv_dqn_reduce_adam_gated(nets[j], partials[j], n_partials, ..., step_t[j], hard_update[j], loss_out[j], NULL, go_word_dev,
 * go_value).  UAVENV_EINVAL, with nothing enqueued, for whatever that entry refuses of any slot, n_nets out of range, differing
 * heads, a partials entry off 16 bytes, or two slots sharing `local` or a partials buffer. */
int uavenv_dqn_reduce_adam_slots(const UavDqnNet *const *nets, int32_t n_nets, float *const *partials, int32_t n_partials, float lr,
                                 float beta1, float beta2, float eps, const int32_t *step_t, const int32_t *hard_update,
                                 float *const *loss_out, const uint32_t *go_word_dev, uint32_t go_value, void *stream);

/* ---- greedy policy evaluation: whole episodes in one launch (Trainer/DuelingDQN_Trainer.py:90, Is_Train == 0) ----------------
 * Episode e (0 <= e < n) flies scenario row (first + e) mod m of a scenario set -- the env's bank (start_goal / sub / nsub NULL) or
 * caller arrays in the bank's layout (start_goal [m][6], sub [m][K][3], nsub [m], K = the env's max_subgoals) -- as UAV slot
 * j = e mod uav_per_env (whose power parameters price the energy).  The reset is UAV.reset() as the bank reset does it (non-APF;
 * alias = nsub >= 2).  Initial V_vector: v0 [n][2] (raw, before Calc_V) or Max_V (cos t, sin t) with t ~ U[0, 2 pi) from Philox
 * keyed by (seed; e, 0, 0, 0xe7a1) (the bank reset's key constant is 0x5eed).  Every step: state_PathPlan of the current state,
 * the packed row's Q(s) by the forward of uavenv_dqn_act on packed rows (f32 MFMA: bit-identical Q values), the first maximum
 * (strict >) -- with eps > 0 a uniform action where the 24-bit draw of Philox (seed; e, step, 0, 0xe75f) is < eps --, then
 * update_PathPlan (UAV.py:397-513).  The episode ends when the agent is done (success / lose), after max_steps > 0 steps
 * (truncated) or at the natural bound n_sub x Max_Step + 1; a popped sub-goal ("done" returned, agent not done) does not end it.
 * The call never reads or writes the env's agents, its tick, a pending uavenv_set_step_meta or the moved word: a training run is
 * the same with or without evaluations between its calls.  Calls on one env run in stream order (they share the env's layer-1
 * image scratch).  Takes non-APF envs with a world, f32-MFMA nets of the uavenv_step_policy shape (w 100, hid 64, the env's
 * n_actions >= 2, at most UAVENV_EVAL_MAX_OUTPUTS layer-2 outputs); UAVENV_EINVAL otherwise, and for n <= 0, first < 0, misaligned
 * pointers (16 bytes: net->local, records), caller scenarios with m <= 0 or only some of the three pointers, no scenarios at all,
 * traj_steps > 0 without both trajectory pointers (or >= 2^30), or n so large that n + the grid's lanes exceeds INT32_MAX.
 * Heads of more than 4 layer-2 outputs (n_actions + dueling: finer steering tables, a dueling net of 4 actions) run a second
 * instantiation of the same kernel whose layer 2 goes in groups of four outputs; every Q value, the dueling combination and the
 * first maximum are still bit for bit those of uavenv_dqn_act.  The narrower heads launch what they always launched. */
#define UAVENV_EVAL_MAX_OUTPUTS 14  /* layer-2 outputs uavenv_eval_episodes / _slots take: what uavenv_dqn_act / uavenv_dqn_grad take */
#define UAVENV_EVAL_SUCCESS 1       /* the agent reached the goal (or had no sub-goal left) */
#define UAVENV_EVAL_LOSE 2          /* Step reached Max_Step */
#define UAVENV_EVAL_TRUNCATED 4     /* stopped by max_steps (or the natural bound) before the agent was done */
#define UAVENV_EVAL_INVALID 5       /* the scenario row has nsub < 0 or nsub > K: not flown, 0 steps */
typedef struct UavEvalRecord {     /* 64 bytes per episode */
    double ret;                     /* sum of the rewards update_PathPlan returned, in step order from 0.0 */
    double total_score, path_len;   /* the agent's fields at the end (as uavenv_get_state reports them) */
    double energy;                  /* sum of Calc_Fly_Power over the steps (as uavenv_step's energy64) */
    double v0x, v0y;                /* the raw initial V_vector of the reset */
    int32_t steps;                  /* update_PathPlan calls */
    int32_t subgoals;               /* sub-goals popped */
    int32_t collisions;             /* steps that took the Threaten_rate == 1 branch (UAV.py:425-428) */
    uint8_t outcome;                /* UAVENV_EVAL_* */
    uint8_t reach_goal, slot, reserved;
} UavEvalRecord;
typedef struct UavEvalArgs {
    int32_t n, first;               /* episodes; scenario row of episode e = (first + e) mod m */
    const double *start_goal;       /* dev, nullable (all three NULL: the env's bank) [m][6] */
    const double *sub;              /* dev [m][K][3] */
    const int32_t *nsub;            /* dev [m] */
    int32_t m;                      /* rows of the caller's set (ignored for the bank) */
    int32_t max_steps;              /* > 0: truncate after this many steps */
    const double *v0;               /* dev, nullable [n][2] raw initial V_vector per episode */
    uint64_t seed;                  /* headings (v0 NULL) and exploration draws */
    float eps;                      /* <= 0: greedy, no draws; 1: the uniform random policy */
    int32_t traj_steps;             /* > 0: trajectory of the first traj_steps steps */
    UavEvalRecord *records;         /* dev [n], 16-byte aligned */
    double *traj_pos;               /* dev [n][traj_steps + 1][3]: the start, then the position after each step */
    int8_t *traj_act;               /* dev [n][traj_steps]: the action of each step */
    int32_t max_workgroups;         /* 0: as many as stay resident, at most ceil(n / 256); > 0: at most this many */
    int32_t reserved0;
} UavEvalArgs;
int uavenv_eval_episodes(UavEnv *env, const UavDqnNet *net, const UavEvalArgs *args, void *stream);

/* ---- the same for an f16-MFMA net (UAVENV_MFMA_F16: BASELINE configs[2]) ----------------------------------------------------------
 * uavenv_eval_episodes with the policy an f16 learner acts with: Q(s) by the f16-MFMA forward of uavenv_dqn_act (fc1, b1 and the
 * observation row rounded to f16, four v_mfma_f32_16x16x32_f16 per accumulator, f32 accumulation, fc2 / b2 in f32: bit-identical Q
 * values), not the f32 master weights under the f32 forward.  The row's halves are what the env's own launches feed the net: the
 * halves an UAVENV_OBS_F16 env stores, which are also the halves uavenv_dqn_act expands an UAVENV_OBS_PACKED row to.  Everything
 * else -- episodes, scenario rows, the reset, v0 / the heading draw, the first-maximum action, the eps draw, the end of an episode,
 * UavEvalArgs, UavEvalRecord, the trajectory, the grid, what is left untouched on the env -- is uavenv_eval_episodes'.
 * Takes a non-APF env with a world whose obs_dtype is UAVENV_OBS_F16 or UAVENV_OBS_PACKED, and an f16-MFMA net of w 100, hid 64, the
 * env's n_actions >= 2, at most 4 layer-2 outputs and a 16-byte aligned `local`.  UAVENV_EINVAL, with nothing allocated or enqueued,
 * otherwise (an f32-MFMA net, an UAVENV_OBS_F32 env, an APF env, more than 4 outputs) and for every argument uavenv_eval_episodes
 * refuses.  uavenv_eval_episodes and uavenv_eval_episodes_slots keep refusing f16-MFMA nets. */
int uavenv_eval_episodes_f16(UavEnv *env, const UavDqnNet *net, const UavEvalArgs *args, void *stream);

/* ---- greedy DQN evaluation with one net per UAV slot, APF on or off, in one launch ---------------------------------------------------
 * uavenv_eval_episodes for n_nets nets (n_nets = 1, or uav_per_env <= UAVENV_SAC_LOOP_MAX_SLOTS: one net per UAV slot,
 * Envs/PathPlan_City.py:59-69) and for envs with APF on as well as off.  Episode e is flown by net e mod n_nets as UAV slot
 * e mod uav_per_env; net j's workgroups fly only the episodes = j (mod n_nets).  Episodes, scenario rows, the reset, v0 / the heading
 * draw, the forward, the first-maximum action, the eps draw, the end of an episode, UavEvalArgs, UavEvalRecord and the trajectory are
 * those of uavenv_eval_episodes: with n_nets = 1 on a non-APF env the two entries write the same bytes.  With APF on, update_PathPlan
 * runs Adjust_subgoal and the force term (UAV.py:156-210, 448-453) on a private [K][3] f64 sub-goal list per resident lane, in the
 * env-owned workspace uavenv_eval_episodes_sac uses (24 K bytes per lane, grown on demand, freed by uavenv_destroy); the env's own
 * lists, agents, tick, pending uavenv_set_step_meta and moved word are never touched.  max_workgroups bounds the workgroups PER NET.
 * The nets' layer-1 images live in a buffer of this entry's own on the env (allocated on first use, grown when n_nets needs it).
 * Calls on one env run in stream order.  A record does not depend on the grid.
 * Takes f32-MFMA nets of w 100, hid 64, the env's n_actions >= 2 and at most UAVENV_EVAL_MAX_OUTPUTS layer-2 outputs, all with the same
 * `dueling`, each with a 16-byte aligned `local` (wide heads: as uavenv_eval_episodes). UAVENV_EINVAL, with nothing enqueued or allocated, otherwise and for: no world; nets NULL or a NULL
 * entry; n_nets other than 1 or uav_per_env (or > UAVENV_SAC_LOOP_MAX_SLOTS); and every argument uavenv_eval_episodes refuses. */
int uavenv_eval_episodes_slots(UavEnv *env, const UavDqnNet *const *nets, int32_t n_nets, const UavEvalArgs *args, void *stream);

/* ---- SAC policy evaluation: whole episodes of the continuous actor in one launch (Trainer/SAC_Trainer.py:444-448 get_action) -------
 * uavenv_eval_episodes with the SAC actor (PolicyNetContinuous_SAC 100-64-(2+2), BaseClass/BaseCNN.py:459-483) as the policy, for APF
 * and non-APF envs.  Episodes, scenario rows, the reset, v0 / the heading draw (Philox (seed; e, 0, 0, 0xe7a1)), the end of an episode,
 * UavEvalRecord and traj_pos are those of uavenv_eval_episodes.  Episode e is flown by actor e mod n_actors (n_actors = 1, or
 * uav_per_env <= UAVENV_SAC_LOOP_MAX_SLOTS: one actor per UAV slot) as UAV slot e mod uav_per_env.  Every step: state_PathPlan of the
 * current state, the packed row through the forward of uavenv_sac_act (bit-identical head outputs), the head with the reference's
 * quirks (std = tanh(softplus(.)), tanh applied twice), action = tanh(mu + std * eps) * action_bound in f32, steer = (double) of its
 * component 0 as uavenv_step reads UAVENV_ACT_STEER_F32, then update_PathPlan (UAV.py:397-513) -- with Adjust_subgoal and the force
 * term when the env has APF on.  get_action always samples (SAC has no greedy branch), so there are two modes:
 *   UAVENV_EVAL_SAC_MEAN    eps = 0: the action uavenv_sac_act gives for a zero noise tensor;
 *   UAVENV_EVAL_SAC_SAMPLE  eps ~ N(0, 1) per (episode, step, component): Box-Muller on the first two words of Philox keyed by
 *                           (seed; e, step, 0, 0x5ac0) -- cosine branch = component 0, sine branch = component 1.
 *                           uavenv_eval_noise_fill writes the same numbers to memory: out[(e * steps + t) * 2 + d].
 * Only component 0 steers; component 1 is evaluated only for the trajectory.  traj_act: float [n][traj_steps][2], the two values
 * uavenv_sac_act would have written to act0 / act1 (the caller pre-fills what lies past an episode's end, e.g. with NaN).
 * APF mutates sub-goal lists, so every resident lane flies on a private [K][3] f64 list in an env-owned workspace: 24 K bytes per lane
 * (1 152 B at K = 48; 256 lanes per workgroup, ~75 MB with one resident workgroup on each of 256 CUs -- max_workgroups bounds it),
 * allocated on first use, grown (after a device synchronisation) when a later call needs more lanes, freed by uavenv_destroy.  The
 * env's own lists are never touched, and as with uavenv_eval_episodes neither are its agents, tick, pending uavenv_set_step_meta or
 * moved word.  Non-APF envs use no workspace.  A record does not depend on the grid.
 * UAVENV_EINVAL, with nothing enqueued, for: no world; no scenarios at all; n <= 0; first < 0; n_actors other than 1 or uav_per_env
 * (or > UAVENV_SAC_LOOP_MAX_SLOTS); actors NULL, or an actor block NULL or not 16-byte aligned; action_bound not finite or <= 0; an
 * unknown mode; records NULL or not 16-byte aligned; traj_steps < 0 or >= 2^30, or > 0 without both trajectory pointers; f64 arrays
 * or traj_act not 8-byte, nsub not 4-byte aligned; only some of the three scenario pointers, or all three with m <= 0; max_steps or
 * max_workgroups < 0; n so large that n + the grid's lanes exceeds INT32_MAX. */
#define UAVENV_EVAL_SAC_MEAN 0
#define UAVENV_EVAL_SAC_SAMPLE 1
typedef struct UavSacEvalArgs {
    int32_t n, first;               /* as UavEvalArgs */
    const double *start_goal;       /* dev, nullable (all three NULL: the env's bank) [m][6] */
    const double *sub;              /* dev [m][K][3] */
    const int32_t *nsub;            /* dev [m] */
    int32_t m;
    int32_t max_steps;              /* > 0: truncate after this many steps */
    const double *v0;               /* dev, nullable [n][2] raw initial V_vector per episode */
    uint64_t seed;                  /* headings (v0 NULL) and the noise of UAVENV_EVAL_SAC_SAMPLE */
    const float *const *actors;     /* HOST array of n_actors device pointers: the actors' flat parameter blocks (16-byte aligned) */
    int32_t n_actors;               /* 1 or uav_per_env */
    float action_bound;             /* config/Trainer.xml <action_bound> */
    int32_t mode;                   /* UAVENV_EVAL_SAC_MEAN | UAVENV_EVAL_SAC_SAMPLE */
    int32_t traj_steps;             /* > 0: trajectory of the first traj_steps steps */
    UavEvalRecord *records;         /* dev [n], 16-byte aligned */
    double *traj_pos;               /* dev [n][traj_steps + 1][3] */
    float *traj_act;                /* dev [n][traj_steps][2] */
    int32_t max_workgroups;         /* per actor: 0 = as many as stay resident, at most one per 256 of its episodes; > 0: at most this many */
    int32_t reserved0;
} UavSacEvalArgs;
int uavenv_eval_episodes_sac(UavEnv *env, const UavSacEvalArgs *args, void *stream);
/* out_dev[(e * steps + t) * 2 + d], e < n, t < steps: the noise UAVENV_EVAL_SAC_SAMPLE uses for episode e, step t, component d.
 * UAVENV_EINVAL for n <= 0, steps <= 0, n * steps >= 2^31 or a NULL / misaligned (4 bytes) pointer. */
int uavenv_eval_noise_fill(uint64_t seed, int32_t n, int32_t steps, float *out_dev, void *stream);

/* ---- a scripted baseline policy: sub-goal pursuit with look-ahead (no learning; the yardstick the learned policies are held to) ------
 * The policy reads an agent's position, current sub-goal (with APF: its own shifted list head), cached heading
 * (calculate_angle(0, V_vector)), the number of sub-goals left and the world.  Candidate steers k = 0 .. C - 1:
 *   UAVENV_ACT_INDEX_I32  C = the env's n_actions (2..32), steer_k = -1 + 2k / (C - 1) as uavenv_step decodes index k; candidates = 0;
 *   UAVENV_ACT_STEER_F32  C = candidates (odd, 3..17), steer_k = (double)(float)(-1 + 2k / (C - 1)), as uavenv_step reads an f32 steer.
 * Rule: no sub-goal left -> candidate C / 2.  Otherwise err = calculate_angle(sub0 - pos) - heading wrapped into (-pi, pi],
 * s* = clamp(err / Steering_angle, -1, 1), cost_k = |steer_k - s*|.  Candidate k is blocked where Threaten_rate(pos + t V_k) = 1 for
 * some t = 1 .. lookahead, V_k being the V_vector update_PathPlan sets for steer_k (UAV.py:411-417, Calc_V's clamp included: the t = 1
 * point is bit for bit where the step moves to); lookahead = 0 blocks nothing.  The policy takes the unblocked candidate of least
 * cost, the lower k on equal cost; with every candidate blocked, the least cost among the candidates whose next point (t = 1) is
 * free; with none of those either, the least cost overall.  So with lookahead >= 1 a step takes the collision branch
 * (UAV.py:425-428) only when every candidate's next point was blocked.
 *
 * uavenv_scripted_act: the act launch alone, one lane per agent of the env: actions_out[i] (dev, [N], 4-byte aligned) = the int32
 * index or the f32 steer of agent i's candidate, the middle candidate C / 2 for a done agent -- what uavenv_step takes as
 * UAVENV_ACT_INDEX_I32 / UAVENV_ACT_STEER_F32.  The env is only read.
 *
 * uavenv_eval_episodes_scripted: uavenv_eval_episodes with this policy in the net's place, for APF and non-APF envs, in one launch
 * that stages nothing but the world.  Episodes, scenario rows, the reset, v0 / the heading draw, UavEvalArgs, UavEvalRecord, the end of
 * an episode, truncation, invalid rows, max_workgroups and what is left untouched on the env are uavenv_eval_episodes'; slot
 * j = e mod uav_per_env; with APF on the lanes fly on the env-owned workspace of uavenv_eval_episodes_sac / _slots.  Index kind:
 * args->eps > 0 replaces the choice by uavenv_eval_episodes' exploration draw (Philox (seed; e, step, 0, 0xe75f)), so eps = 1 is
 * that entry's random policy bit for bit; traj_act is int8 [n][traj_steps].  Steer kind: traj_act points to float [n][traj_steps]
 * (4-byte aligned), the f32 steer of every step.  A record does not depend on the grid.
 * UAVENV_EINVAL, with nothing enqueued or allocated, for: an action_kind other than the two; candidates even, outside 3..17 or (index
 * kind) non-zero; lookahead outside 0..16; the index kind on an env with more than 32 actions; eps > 0 with the steer kind; no world;
 * and every argument uavenv_eval_episodes refuses. */
#define UAVENV_SCRIPTED_MAX_LOOKAHEAD 16
#define UAVENV_SCRIPTED_MAX_STEER_CANDIDATES 17
#define UAVENV_SCRIPTED_MAX_INDEX_ACTIONS 32
typedef struct UavScriptedPolicy {
    int32_t action_kind;            /* UAVENV_ACT_INDEX_I32 | UAVENV_ACT_STEER_F32 */
    int32_t candidates;             /* steer kind: C, odd, 3..17; index kind: 0 (C = the env's n_actions) */
    int32_t lookahead;              /* H, 0..16 */
    int32_t reserved0;
} UavScriptedPolicy;
int uavenv_scripted_act(UavEnv *env, const UavScriptedPolicy *policy, void *actions_out, void *stream);
int uavenv_eval_episodes_scripted(UavEnv *env, const UavScriptedPolicy *policy, const UavEvalArgs *args, void *stream);

/* ---- multi-GPU: one-shot all-reduce of the gradient bucket over peer-mapped HBM (csrc/p2p.hip) ------------------- */
/* One UavP2P per rank (= per GPU / process).  create -> every rank publishes its UAVENV_P2P_HANDLE_BYTES handle
 * (uavenv_p2p_handle) -> the `world` handles, in rank order, go to uavenv_p2p_connect on every rank.  Then, per update,
 *     uavenv_dqn_grad -> uavenv_dqn_reduce_p2p -> uavenv_dqn_adam_p2p
 * replaces uavenv_dqn_reduce -> RCCL all-reduce -> uavenv_dqn_adam: the column sums are stored straight into every
 * rank's receive area (xGMI), flags tell the readers, every rank adds the `world` contributions in rank order (bit-
 * identical updates) and takes the Adam step -- all on the stream, no host round trip.  Waits are bounded: a timeout
 * raises a sticky error (uavenv_p2p_status) instead of hanging; see there. */
#define UAVENV_P2P_HANDLE_BYTES 64
#define UAVENV_P2P_ERR_TIMEOUT 1    /* a peer's flag did not arrive within the spin limit */
#define UAVENV_P2P_ERR_DIVERGED 2   /* the ranks' weight checksums differ */
typedef struct UavP2P UavP2P;
int uavenv_p2p_create(int32_t world, int32_t rank, int32_t bucket_floats, UavP2P **out);
int uavenv_p2p_handle(UavP2P *p2p, void *handle_out_host);
/* 1 when kernels on `device` may address memory of `peer_device` (hipDeviceCanAccessPeer; a device reaches itself): the
 * check to run on every rank before uavenv_p2p_connect maps anything. */
int uavenv_p2p_can_reach(int32_t device, int32_t peer_device);
int uavenv_p2p_connect(UavP2P *p2p, const void *all_handles_host);
int uavenv_p2p_destroy(UavP2P *p2p);
/* check_every: every that many updates the Adam kernel folds a 64-bit checksum of the new weights into the next bucket
 * and every rank compares the `world` checksums (0 = never; default 256).  spin_limit: polls before a wait gives up
 * (0 = keep; default 2^24, about four seconds).  Must be the same on every rank. */
int uavenv_p2p_configure(UavP2P *p2p, int32_t check_every, int32_t spin_limit);
int uavenv_p2p_errors(UavP2P *p2p, int32_t *timeouts_out);        /* synchronises */
/* Device address of the exchange's sticky error word (0 = healthy): what UavSacAdam.skip_word takes.  NULL for NULL. */
const uint32_t *uavenv_p2p_error_word(const UavP2P *p2p);
/* out4 = {sticky error code (0 = healthy, UAVENV_P2P_ERR_*), timeouts, checksum mismatches, checksums folded so far}.
 * synchronise == 0: only the code, read from host-mapped memory without touching the device (timeouts / mismatches = -1).
 * Once the code is non-zero the rank's Adam steps are skipped (its weights freeze rather than absorb stale or partial
 * sums) and uavenv_dqn_reduce_p2p / uavenv_dqn_adam_p2p / uavenv_loop_run return UAVENV_EP2P. */
int uavenv_p2p_status(UavP2P *p2p, int32_t synchronise, int32_t *out4);
/* Tests: raise the sticky error as a timeout / a mismatch would (code 0 clears it). */
int uavenv_p2p_inject_fault(UavP2P *p2p, int32_t code);
/* The same exchange for any float buffer (the SAC learners' per-phase gradient rows): buf_dev[i] <- sum over the ranks, in rank
 * order, of their buf_dev[i], i < count -- two launches on the stream.  count: a multiple of 4, <= bucket_floats; buf_dev 16-byte
 * aligned.  After a sticky error the buffer keeps this rank's own values and the call returns UAVENV_EP2P: stop stepping and
 * re-synchronise parameters and optimiser moments from one rank.  (Use a UavP2P of its own, not the one a DQN learner drives.) */
int uavenv_p2p_allreduce(UavP2P *p2p, float *buf_dev, int64_t count, void *stream);
/* Are the ranks' parameters still bit-identical?  Hashes the bit patterns of n_blocks flat f32 blocks (device pointers in a HOST
 * array, n_floats[b] each) on the device, sends the 64-bit result to every rank and compares the `world` results on the device
 * -- four small launches on the stream, no host round trip.  A difference raises the exchange's sticky error
 * (UAVENV_P2P_ERR_DIVERGED: uavenv_p2p_status, UAVENV_EP2P from then on), exactly like the DQN bucket's built-in checksum; the
 * generic exchange has no room for one in its buffers, so its owners call this every so many updates (uavenv_sac_loop_run:
 * UavSacLoopConfig.check_every).  Every rank must call it at the same point of the sequence. */
#define UAVENV_P2P_CHECK_MAX_BLOCKS 40
int uavenv_p2p_check_blocks(UavP2P *p2p, const float *const *blocks_dev, const int32_t *n_floats, int32_t n_blocks, void *stream);
int uavenv_dqn_reduce_p2p(const UavDqnNet *net, const float *partials_dev, int32_t n_partials, UavP2P *p2p, void *stream);
/* step_t == 0: only the rank-ordered sum, into raw_out_dev[num_params + 2] (self-test); otherwise Adam as uavenv_dqn_adam
 * (raw_out_dev nullable). */
int uavenv_dqn_adam_p2p(const UavDqnNet *net, UavP2P *p2p, float lr, float beta1, float beta2, float eps, int32_t step_t,
                        int32_t hard_update, float *loss_out_dev, float *raw_out_dev, void *stream);

/* ---- multi-GPU fallback: the same bucket through an RCCL all-reduce enqueued from C (csrc/coll.hip) ------------------ */
/* RCCL is dlopen'ed (rccl_path first -- e.g. PyTorch's own librccl.so --, then the loader's search path); the library
 * has no link-time dependency on it.  Rank 0: uavenv_coll_unique_id -> the UAVENV_COLL_ID_BYTES travel to every rank
 * (any channel) -> every rank: uavenv_coll_create with its HIP device current.  Per update, on the stream:
 *     uavenv_dqn_grad -> uavenv_dqn_reduce(raw) -> uavenv_coll_allreduce_sum(raw) -> uavenv_dqn_adam(raw)
 * which is what uavenv_loop_run issues when UavLoopConfig.coll is set.  All ranks receive bit-identical sums. */
#define UAVENV_COLL_ID_BYTES 128
typedef struct UavColl UavColl;
const char *uavenv_coll_last_error(void);
int uavenv_coll_unique_id(const char *rccl_path, void *id_out_host);
int uavenv_coll_create(const char *rccl_path, int32_t world, int32_t rank, const void *id_host, UavColl **out);
int uavenv_coll_destroy(UavColl *coll);
int uavenv_coll_allreduce_sum(UavColl *coll, float *buf_dev, int64_t n, void *stream);

/* ---- the whole off-policy loop, enqueued from C ------------------------------------------------------------------ */
/* PathPlan_City.run_thread_OffPolicy (Envs/PathPlan_City.py:364-385) for every env of the shard at once, K times:
 *     act     Q(s) + epsilon-greedy            -> ring.action[head]          (Choose_Action2, :346,370)
 *     step    update_PathPlan + state_PathPlan -> ring frame head / head+1   (Move_Agent + Push_Replay, :371-379)
 *     learn   learn_off_policy(): sample, TD target, loss, Adam, hard copy   (:380-383; skipped while the ring holds
 *             fewer than `learn_start` transitions or when batch == 0)
 * One call enqueues all 3 K launches on the stream (act rides in the step kernel's prologue when it can: uavenv_step_policy;
 * 4 K otherwise, + 1 K with the RCCL exchange); the host does nothing per step but those launches from C (no
 * interpreter, no per-step allocation).  The cursor (head, filled, counter, epoch) lives in the UavLoop and is
 * advanced by uavenv_loop_run; read it back with uavenv_loop_get. */
typedef struct UavLoop UavLoop;
typedef struct UavLoopConfig {
    UavEnv *env;
    UavReplayRing ring;          /* action_is_index must be 1 */
    UavDqnNet net;
    int32_t head, filled;        /* initial ring cursor */
    int32_t batch;               /* learner batch (multiple of 64); 0 = rollout only */
    int32_t kind;                /* 0 max_a Q_target(s'), 1 double-DQN */
    int32_t huber;
    int32_t update_loop;         /* hard target copy every update_loop updates */
    int32_t epoch;               /* learner updates done so far (Adam's step count) */
    int32_t learn_start;         /* transitions the ring must hold before the first update (>= batch) */
    uint64_t seed, counter;      /* Philox key / first step's counter (one counter value per step) */
    float eps, gamma, lr, beta1, beta2, adam_eps;
    uint32_t step_flags;         /* UAVENV_STEP_* for every step */
    float *partials_dev;         /* uavenv_dqn_partial_rows(batch) x uavenv_dqn_partial_stride(net) floats of scratch */
    float *loss_dev;             /* device scalar: mean loss of the last update */
    uint8_t *info_dev;           /* nullable: frames x N plane receiving uavenv_step's info codes (frame-major like reward) */
    UavP2P *p2p;                 /* nullable: multi-GPU -- gradients are summed over the ranks through csrc/p2p.hip */
    int32_t time_every;          /* > 0: bracket the step kernel of every time_every-th step with HIP events */
    int32_t sample_lag;          /* 0 = the reference's order (update t samples transitions <= t: act -> step -> learn, strictly
                                    serial).  1 = EXPERIMENT, a stated deviation from Envs/PathPlan_City.py:374-385: update t samples
                                    the transitions stored before step t (<= t - 1), so its gradient kernel depends on the
                                    previous Adam step only and runs on a second stream BESIDE step t; Adam t joins both.  Not
                                    with prioritised replay. */
    UavColl *coll;               /* nullable (used when p2p is NULL): multi-GPU -- RCCL all-reduce of raw_dev from C */
    float *raw_dev;              /* num_params + 2 floats of scratch for the coll path */
    /* prioritised replay (per.prio != NULL; capacity = frames * N, slot = frame * N + agent): per pass, after the step,
     * the frame just completed gets the new-transition priority (|0| + per_eps) ** per_alpha where valid and the ring's
     * new head frame gets 0; the update then is rebuild -> uavenv_per_sample (Philox(seed, counter)) -> uavenv_per_weights
     * -> uavenv_dqn_grad_w -> reduce + Adam -> uavenv_per_set_f32, all stream-ordered.  beta advances by per_beta_inc per
     * update (capped at 1) and is read back through uavenv_loop_get_per. */
    UavPer per;
    double per_alpha, per_beta, per_beta_inc, per_eps, per_clip;
    int64_t *per_slots_dev;      /* batch */
    double *per_prio_dev;        /* batch + (batch + 255) / 256 (priorities, then uavenv_per_weights' scratch) */
    float *per_w_dev;            /* batch */
    float *per_abs_dev;          /* batch */
    int32_t *per_idx_dev;        /* batch x 2 (frame, agent) pairs of the batch.  Without `per`: non-null + UAVENV_STEP_SKIP_DONE in
                                  * step_flags = uniform draws over the VALID rows only (uavenv_replay_draw_valid), handed to the
                                  * update as explicit pairs; null = the update draws for itself over every stored row */
    /* rolling refresh of the reset bank (uavenv_replan_*; 0 = off, the bank stays as planned): every replan_every passes the
     * loop commits the slice whose planning has finished and starts planning the next replan_count rows of the bank (rotating)
     * on a low-priority stream of its own, beside the passes. */
    int32_t replan_every, replan_count, replan_max_iter, reserved1;
    /* nullable device word: the loop registers it with the env (uavenv_set_moved_word) and gates every update on "this pass's
     * step moved at least one agent" (uavenv_dqn_reduce_adam_gated).  Single-GPU form only (no p2p / coll). */
    uint32_t *moved_dev;
} UavLoopConfig;
typedef struct UavLoopCursor {
    int32_t head, filled, epoch, reserved0;
    uint64_t counter;
} UavLoopCursor;

int uavenv_loop_create(const UavLoopConfig *cfg, UavLoop **out);
int uavenv_loop_destroy(UavLoop *loop);
int uavenv_loop_set_eps(UavLoop *loop, float eps);
/* Enqueue n_steps iterations on `stream`; never synchronises. */
int uavenv_loop_run(UavLoop *loop, int32_t n_steps, void *stream);
int uavenv_loop_get(const UavLoop *loop, UavLoopCursor *out);
/* Prioritised replay: the current beta. */
int uavenv_loop_get_per(const UavLoop *loop, double *beta_out);
/* Synchronises the recorded events; writes up to max_n step-kernel durations (ms) and returns their number in *n_out;
 * clears the record. */
int uavenv_loop_step_times(UavLoop *loop, float *ms_out, int32_t max_n, int32_t *n_out);

/* ---------------------------------------------------------------------------------------------------------------------
 * Fused SAC (continuous actions) update -- Trainer/SAC_Trainer.py:325-379 (update, continuous branch), :122-131
 * (calc_target), :145-147 (soft_update), nets BaseClass/BaseCNN.py:459-500 (PolicyNetContinuous_SAC 100-64-(2+2),
 * QValueNetContinuous_SAC 102-64-64-2, critics emitting action_dim = 2 values as in the reference).  csrc/sac.hip.
 * One update = critic_grad -> critic_adam -> actor_grad -> actor_adam on one stream (four launches, nothing synchronises).
 * Flat f32 parameter blocks, 16-byte aligned; the torch modules' parameters are views of them:
 *   actor : fc1.weight 64x100 | fc1.bias 64 | fc_mu.weight 2x64 | fc_std.weight 2x64 | fc_mu.bias 2 | fc_std.bias 2
 *   critic: fc1.weight 64x102 | fc1.bias 64 | fc2.weight 64x64 | fc2.bias 64 | fc_out.weight 2x64 | fc_out.bias 2
 * A partial-gradient row (one per workgroup, uavenv_sac_partial_rows(batch) of them) has the same layout:
 *   critic rows: critic 1 | critic 2 | loss 1 | loss 2 | valid / B | 0     actor rows: actor | actor loss | sum log pi | valid / B | 0 */
#define UAVENV_SAC_CRITIC_IN 102
#define UAVENV_SAC_ACTOR_PARAMS 6724
#define UAVENV_SAC_CRITIC_PARAMS 10882
#define UAVENV_SAC_ACTOR_STRIDE 6728
#define UAVENV_SAC_CRITIC_STRIDE 21768
typedef struct UavSacNets {
    float *actor, *critic1, *critic2, *target1, *target2;
    float *log_alpha;            /* device scalar */
} UavSacNets;
/* The sampled transitions, in place: packed observation rows (UAVENV_OBS_PACKED) + planes indexed by the row of s.
 * Rows either explicit (idx_s / idx_n: row of s and of s' per sample) or derived from uavenv_replay_draw's (frame, env)
 * pairs for UAV slot `slot` of a ring whose frames hold n_agents = n_envs * uav_per_env rows:
 * row(s) = frame * n_agents + env * uav_per_env + slot, s' one frame later. */
typedef struct UavSacBatch {
    const void *obs_packed;
    const int32_t *idx_s, *idx_n;        /* nullable when draws != NULL */
    const int32_t *draws;                /* nullable: batch x (frame, env) */
    int32_t n_agents, uav_per_env, slot, frames;
    const float *act0, *act1, *reward;   /* the two action components (:444-448), the reward */
    const uint8_t *done, *valid;         /* valid nullable (= all 1): rows with 0 (agents that only waited for their team-mates:
                                            not replay memory in the reference) carry weight 0 in EVERY loss -- critics, actor,
                                            log_alpha -- and all means are over the valid samples */
    const float *eps;                    /* batch x 2 N(0,1) draws standing for Normal.rsample() of this phase */
    int32_t batch;                       /* a multiple of 64 */
    int32_t tiles_per_wg;                /* 0: chosen per launch (uavenv_sac_partial_rows_n); > 0: this many 64-sample tiles per
                                            workgroup (at most 8) -- fixes the partition, and so the summation order, of the
                                            partial rows whatever else shares the launch */
    /* prioritised replay (Trainer/SAC_Trainer.py:336-352), both nullable: is_weights[s] multiplies sample s in the two critic
     * losses (mean_s w_s err_s^2: the per-sample form of `is_weights * critic_loss`); abs_td_out[s] receives
     * |min(Q1, Q2)(s, a) - td_target| of output column 0 (:351) -- written by uavenv_sac_critic_grad. */
    const float *is_weights;
    float *abs_td_out;
    const void *meta;                    /* ABI 5, nullable: the ring's transition records (UavReplayRing.meta), indexed by the row of s:
                                            when set, a0 / a1 / reward / done / valid of a sample come from its ONE record instead of
                                            a line each from the five planes above (which may then be NULL) */
    float *td_scratch;                   /* ABI 4, nullable: batch x 2 floats of device scratch.  With it uavenv_sac_critic_grad computes the
                                            td targets (:122-131) in a launch of its own -- two tiles in flight per workgroup, two
                                            wavefronts per SIMD -- and the gradient kernel reads them from here; without it the
                                            gradient kernel computes them itself.  Bit-identical either way. */
} UavSacBatch;
typedef struct UavSacAdam {
    float lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt;   /* 1 - beta1^t, sqrt(1 - beta2^t) */
    float tau;                           /* soft target update (critic_adam only) */
    float grad_scale;                    /* ignored since ABI 3: every column is divided by the summed valid-fraction column of the
                                            partial rows (1 / world size after an all-reduce SUM of all-valid batches) */
    const uint32_t *skip_word;           /* ABI 4, nullable device word: non-zero when the launch runs => it changes NOTHING (no
                                            parameter, moment, target or scalar).  uavenv_p2p_error_word(): an Adam launch enqueued
                                            behind a peer exchange that timed out must not step with rank-local sums */
    const uint32_t *go_word;             /* ABI 4, nullable: the launch changes nothing unless *go_word == go_value when it runs
                                            (uavenv_set_moved_word: no update behind a step that moved nobody) */
    uint32_t go_value, reserved0;
} UavSacAdam;
/* get_action (SAC_Trainer.py:444-448) for `count` agents whose packed rows are first_row + i * row_stride: the two
 * action components land in act0[row] / act1[row].  eps: count x 2 N(0,1) draws (Normal.rsample()). */
int uavenv_sac_act(const float *actor, const void *obs_packed, int32_t first_row, int32_t row_stride, int32_t count,
                   const float *eps, float action_bound, float *act0, float *act1, void *stream);
int uavenv_sac_partial_rows(int32_t batch);          /* = uavenv_sac_partial_rows_n(batch, 1, 0): never less than any launch writes */
/* Partial rows per slot that a grad launch over n_slots trainers writes (= workgroups per slot), tiles_per_wg as in UavSacBatch:
 * 0 = as many tiles per workgroup as bring the launch down to one workgroup per CU (at most 8).  What the Adam call behind
 * that launch must be told as `rows`. */
int uavenv_sac_partial_rows_n(int32_t batch, int32_t n_slots, int32_t tiles_per_wg);
const char *uavenv_sac_last_error(void);
/* Diagnostics (UAVENV_PHASE_PROFILE builds): 16 s_memtime stamps per workgroup of uavenv_sac_critic_grad; NULL disables. */
int uavenv_sac_set_debug_buffer(unsigned long long *dev_buf);
/* Batched forms: n <= UAVENV_SAC_LOOP_MAX_SLOTS independent trainers (one per UAV slot, Envs/PathPlan_City.py:59-69) in ONE launch
 * per phase (grid.y = slot); arrays of n entries each; results are bit-identical to n single launches.  At BASELINE
 * configs[3]'s batch one trainer fills the chip; in small runs a step is a chain of latency-bound launches and n slots side
 * by side cost what one does. */
#define UAVENV_SAC_LOOP_MAX_SLOTS 8
int uavenv_sac_act_multi(const float *const *actors, const void *obs_packed, const int32_t *first_rows, int32_t row_stride,
                         int32_t count, const float *const *eps, float action_bound, float *act0, float *act1, int32_t n,
                         void *stream);
int uavenv_sac_critic_grad_multi(const UavSacNets *nets, const UavSacBatch *batches, int32_t n, float gamma, float action_bound,
                                 float *const *partials, void *stream);
int uavenv_sac_actor_grad_multi(const UavSacNets *nets, const UavSacBatch *batches, int32_t n, float action_bound,
                                float *const *partials, void *stream);
int uavenv_sac_critic_adam_multi(const UavSacNets *nets, float *const *partials, int32_t rows, float *const *m1, float *const *v1,
                                 float *const *m2, float *const *v2, const UavSacAdam *h, float *const *losses_out, int32_t n,
                                 void *stream);
int uavenv_sac_actor_adam_multi(const UavSacNets *nets, float *const *partials, int32_t rows, int32_t batch, float *const *m,
                                float *const *v, float *const *alpha_mv, const UavSacAdam *h, float alpha_lr, float target_entropy,
                                float *const *scalars_out, int32_t n, void *stream);
/* eps = the draws of actor(next_states).  partials: rows x UAVENV_SAC_CRITIC_STRIDE floats. */
int uavenv_sac_critic_grad(const UavSacNets *nets, const UavSacBatch *batch, float gamma, float action_bound, float *partials,
                           void *stream);
/* Adam on both critics (m / v: UAVENV_SAC_CRITIC_PARAMS floats each) + target <- target (1 - tau) + critic tau.
 * losses_out (nullable, 4 floats): the two critic losses. */
int uavenv_sac_critic_adam(const UavSacNets *nets, const float *partials, int32_t rows, float *m1, float *v1, float *m2, float *v2,
                           const UavSacAdam *h, float *losses_out, void *stream);
/* Multi-GPU: column sums of the partial rows only -> raw[stride] (stride = one of the two UAVENV_SAC_*_STRIDE); all-reduce
 * (sum) raw over the ranks, then call the *_adam entry point with partials = raw, rows = 1: the valid-fraction column, summed
 * over the ranks, makes the update the mean over the valid samples of ALL ranks. */
int uavenv_sac_reduce(const float *partials, int32_t rows, int32_t stride, float *raw, void *stream);
/* eps = the draws of actor(states).  partials: rows x UAVENV_SAC_ACTOR_STRIDE floats. */
int uavenv_sac_actor_grad(const UavSacNets *nets, const UavSacBatch *batch, float action_bound, float *partials, void *stream);
/* Adam on the actor and on log_alpha (alpha_mv: its exp_avg, exp_avg_sq).  scalars_out (nullable, 4 floats): actor loss,
 * sum of log pi over [batch, 2]. */
int uavenv_sac_actor_adam(const UavSacNets *nets, const float *partials, int32_t rows, int32_t batch, float *m, float *v,
                          float *alpha_mv, const UavSacAdam *h, float alpha_lr, float target_entropy, float *scalars_out,
                          void *stream);

/* ---- the off-policy loop for SAC (continuous actions), one trainer per UAV slot, enqueued from C ----------------------
 * PathPlan_City.run_thread_OffPolicy (Envs/PathPlan_City.py:364-385) with SAC_Trainer for every env at once, K steps per
 * call.  Per step: one launch of N(0,1) draws (uavenv_randn) for every rsample() of the step, get_action of all U slots
 * (uavenv_sac_act_multi), uavenv_step (replay write included), one uavenv_replay_draw, and the four phases of the fused update
 * for all U slots at once (the *_multi entry points) -- what plugins/PathPlan_City._run_eposide_fused_sac issues from Python slot
 * by slot (~22 launches per step), bit for bit, in 8.  Uniform replay (over valid rows only when the step flags skip finished
 * agents: uavenv_replay_draw_valid) or prioritised replay per slot (UavSacLoopSlot.per). */
typedef struct UavSacLoopSlot {
    UavSacNets nets;
    float *m_actor, *v_actor, *alpha_mv;     /* Adam moments of the actor (UAVENV_SAC_ACTOR_PARAMS each) and of log_alpha (2) */
    float *m1, *v1, *m2, *v2;                /* Adam moments of the two critics (UAVENV_SAC_CRITIC_PARAMS each) */
    float *scalars;                          /* 8 floats: critic losses [0:4], actor loss / sum log pi [4:8] of the last update */
    float *partials_critic, *partials_actor; /* >= uavenv_sac_partial_rows_n(batch, n_slots, 0) rows x UAVENV_SAC_CRITIC_STRIDE / _ACTOR_STRIDE, per slot */
    int32_t epoch, adam_steps;               /* update() calls so far; Adam steps actually taken (bias correction) */
    /* prioritised replay (the reference's own use of ReplayTree, Trainer/SAC_Trainer.py:336-352); per.prio NULL = uniform.  One
     * tree per slot over ITS transitions: capacity = frames x n_envs, data slot = frame * n_envs + env.  All slots or none. */
    UavPer per;
    int64_t *per_slots_dev;                  /* batch */
    double *per_prio_dev;                    /* batch + (batch + 255) / 256 */
    float *per_w_dev, *per_abs_dev;          /* batch each: importance weights in, |TD| out */
    double per_beta;                         /* ReplayTree.beta when the loop is created */
    float *td_dev;                           /* nullable: batch x 2 floats (UavSacBatch.td_scratch of this slot's updates) */
} UavSacLoopSlot;
typedef struct UavSacLoopConfig {
    UavEnv *env;
    UavReplayRing ring;                      /* packed rows, action_is_index = 0 (action plane = first action component) */
    float *act1_plane;                       /* frames x N: the second action component (SAC_Trainer.py:444-448) */
    uint8_t *info_dev;                       /* nullable frames x N */
    int32_t n_slots;                         /* = uav_per_env: slot j trains on rows e * n_slots + j */
    int32_t batch;                           /* per slot; multiple of 64 */
    int32_t head, filled;
    int32_t is_train;
    int32_t valid_draws;                     /* != 0 (needs ring.valid): the uniform draws go over the VALID rows only
                                                (uavenv_replay_draw_valid) -- for loops that skip finished agents instead of
                                                restarting them; 0: over every stored row (rows with valid = 0 weigh 0) */
    uint64_t seed, counter;
    double beta1, beta2, adam_eps;           /* torch.optim.Adam's (doubles: the bias corrections are formed in double) */
    float gamma, tau, action_bound, actor_lr, critic_lr, alpha_lr, target_entropy, reserved1;
    uint32_t step_flags, reserved2;
    int32_t *draws_dev;                      /* n_slots x batch x 2 */
    float *noise_dev;                        /* uavenv_sac_loop_noise_floats(n_slots, n_envs, batch) floats */
    UavSacLoopSlot slot[UAVENV_SAC_LOOP_MAX_SLOTS];
    /* multi-GPU (all NULL on one GPU): every phase's column sums of all slots (uavenv_sac_reduce) are summed over the ranks on
     * the stream -- uavenv_p2p_allreduce on p2p (bucket >= n_slots x UAVENV_SAC_CRITIC_STRIDE) or, when p2p is NULL,
     * uavenv_coll_allreduce_sum on coll -- and the Adam kernels take that one row (the valid-fraction column normalises).
     * uavenv_sac_loop_run returns UAVENV_EP2P once the peer exchange has raised its sticky error. */
    struct UavP2P *p2p;
    struct UavColl *coll;
    float *xbuf_dev;                         /* n_slots x UAVENV_SAC_CRITIC_STRIDE floats */
    /* ReplayTree's hyper-parameters (replay_buffer.py:123-131) when the slots carry a UavPer: per step the loop enqueues, per
     * slot, new-frame priorities ((0 + eps) ** alpha where valid) + retiring the new head -> rebuild -> ReplayTree.sample (Philox
     * (seed + 7 + slot, counter)) -> importance weights -> the four update phases (weights into the critic losses, |TD| out) ->
     * batch_update.  The draws of a slot then come from its tree (draws_dev receives the (frame, env) pairs). */
    double per_alpha, per_beta_inc, per_eps, per_clip;
    uint32_t *moved_dev;                     /* as UavLoopConfig.moved_dev: no update of any slot behind a step that moved nobody */
    int32_t check_every, reserved3;          /* p2p only: compare the ranks' weight checksums (uavenv_p2p_check_blocks over every slot's
                                                actor, critics and targets) every that many updates; 0 = never */
} UavSacLoopConfig;
typedef struct UavSacLoopCursor {
    int32_t head, filled;
    uint64_t counter;
    int32_t epoch[UAVENV_SAC_LOOP_MAX_SLOTS], adam_steps[UAVENV_SAC_LOOP_MAX_SLOTS];
} UavSacLoopCursor;
typedef struct UavSacLoop UavSacLoop;
/* out[i] ~ N(0, 1) for i < n from Philox4x32-10(seed; counter, i / 4) + Box-Muller, one launch. */
int uavenv_randn(uint64_t seed, uint64_t counter, int64_t n, float *out_dev, void *stream);
/* Layout of noise_dev: [n_slots][n_envs][2] get_action draws, then [2][n_slots * batch][2] (rsample() of calc_target, of
 * the actor phase; slot j's rows are j * batch .. (j + 1) * batch of each half). */
int64_t uavenv_sac_loop_noise_floats(int32_t n_slots, int32_t n_envs, int32_t batch);
int uavenv_sac_loop_create(const UavSacLoopConfig *cfg, UavSacLoop **out);
int uavenv_sac_loop_destroy(UavSacLoop *loop);
int uavenv_sac_loop_run(UavSacLoop *loop, int32_t n_steps, void *stream);
int uavenv_sac_loop_get(const UavSacLoop *loop, UavSacLoopCursor *out);
/* ReplayTree.beta of every slot as the loop left it (n_slots doubles). */
int uavenv_sac_loop_get_per(const UavSacLoop *loop, double *beta_out);

/* ---- the off-policy loop for the DQN family with one learner per UAV slot, enqueued from C ------------------------------
 * PathPlan_City.run_thread_OffPolicy (Envs/PathPlan_City.py:364-385) with one Trainer per UAV index (:59-69) for every env at
 * once, K passes per call.  Pass t with counter c, on a packed discrete ring whose n_agents = n_envs * n_slots:
 *     uavenv_dqn_act_slots     all slots' Q(s) + epsilon-greedy from frame t's rows into frame t's action plane (key `seed`)
 *     uavenv_step              UAVENV_ACT_INDEX_I32, replay write into frame t + 1 (transition records included)
 *     while batch > 0 and filled * n_envs >= max(learn_start, batch):
 *     uavenv_replay_draw_slots (seed + 7, c) into draws_dev: over the valid rows with valid_draws, over every stored row otherwise
 *     per slot j               uavenv_dqn_grad on slice j of the draws with net j, epoch j += 1, hard copy every update_loop
 *                              updates, uavenv_dqn_reduce_adam_gated (gated on moved_dev when given)
 * -- 3 + 2 n_slots launches, bit for bit what the same entry points give when the caller issues them.  The loop owns one layer-1
 * image per slot (the split form its act and gradient launches stage): rebuilt from the parameters whenever a run with
 * n_steps > 0 starts, kept current by its own Adam launches, so parameters may be replaced BETWEEN runs (a federated merge).
 * One GPU only: no gradient exchange, no sample lag, no bank refresh.  Uniform replay unless uavenv_dqn_slots_loop_set_per gives every
 * slot a tree (below): then a learning pass is 10 launches whatever n_slots is, and a pass that does not learn 3. */
typedef struct UavDqnSlotsLoopSlot {
    UavDqnNet net;               /* f32 MFMA, w 100, hid 64; all slots one n_actions / dueling */
    float *partials_dev;         /* uavenv_dqn_partial_rows(batch) x uavenv_dqn_partial_stride(net) floats, this slot's own */
    float *loss_dev;             /* device scalar: mean loss of this slot's last update */
    int32_t epoch;               /* updates done so far (Adam's step count) */
    int32_t reserved0;
} UavDqnSlotsLoopSlot;
typedef struct UavDqnSlotsLoopConfig {
    UavEnv *env;
    UavReplayRing ring;          /* UAVENV_OBS_PACKED, action_is_index = 1, n_agents = n_envs * n_slots */
    uint8_t *info_dev;           /* nullable: frames x N plane of uavenv_step's info codes */
    uint32_t *moved_dev;         /* nullable, as UavLoopConfig.moved_dev: no update of any slot behind a step that moved nobody */
    int32_t *draws_dev;          /* n_slots x batch x 2 (frame, agent); may be NULL when batch == 0 */
    int32_t n_slots;             /* = uav_per_env: slot j acts for and learns from agents e * n_slots + j */
    int32_t batch;               /* per slot, multiple of 64; 0 = rollout only */
    int32_t head, filled;
    int32_t kind, huber, update_loop, learn_start;
    int32_t valid_draws;         /* != 0 (needs ring.valid): draws over the VALID rows only, for loops that skip finished agents */
    uint32_t step_flags;
    uint64_t seed, counter;
    float eps, gamma, lr, beta1, beta2, adam_eps;
    UavDqnSlotsLoopSlot slot[UAVENV_DQN_MAX_SLOTS];
} UavDqnSlotsLoopConfig;
typedef struct UavDqnSlotsLoopCursor {
    int32_t head, filled;
    uint64_t counter;
    int32_t epoch[UAVENV_DQN_MAX_SLOTS];
} UavDqnSlotsLoopCursor;
typedef struct UavDqnSlotsLoop UavDqnSlotsLoop;
int uavenv_dqn_slots_loop_create(const UavDqnSlotsLoopConfig *cfg, UavDqnSlotsLoop **out);
int uavenv_dqn_slots_loop_destroy(UavDqnSlotsLoop *loop);
int uavenv_dqn_slots_loop_set_eps(UavDqnSlotsLoop *loop, float eps);
/* on != 0: from the next run the learning phase of a pass is ONE uavenv_dqn_grad_slots and ONE uavenv_dqn_reduce_adam_slots for all
 * slots (a pass is 5 launches instead of 3 + 2 n_slots) -- same parameters, moments, losses and epochs, bit for bit.  Off by
 * default.  UAVENV_EINVAL, with the loop left as it was, when the loop's nets have more than 4 layer-2 outputs. */
int uavenv_dqn_slots_loop_set_multi_update(UavDqnSlotsLoop *loop, int32_t on);
/* Prioritised replay (IsPriority_Replay = 1), one tree per slot: per[j] covers slot j's column of the ring, tree slot
 * frame * n_envs + env <-> agent env * n_slots + j, capacity frames * n_envs, rot 0.  One beta for all slots (one Trainer.xml, and every
 * slot samples on every learning pass).  A pass then is, as in UavLoop and UavSacLoop:
 *     act, step                          as above
 *     not learning:                      uavenv_per_fill_frame_slots -- the frame just written gets (0 + eps) ** alpha where valid, the
 *                                        new head frame is retired
 *     learning (same condition):         beta = min(1, beta + beta_inc); uavenv_per_rebuild_slots with that fill fused in;
 *                                        uavenv_per_sample_slots (seed + 7, c) -- slot j draws under seed + 7 + j;
 *                                        uavenv_per_weights_slots with n_entries = filled * n_envs, the pairs into draws_dev;
 *                                        uavenv_dqn_grad_slots_w; uavenv_dqn_reduce_adam_slots; uavenv_per_set_f32_slots_gated on moved_dev
 * The learning phase is always the one-launch form (uavenv_dqn_slots_loop_set_multi_update(loop, 0) then returns UAVENV_EINVAL), and
 * valid_draws has no meaning: invalid rows carry priority 0.  Call it before the first run; cfg NULL turns prioritised replay off
 * (the one-launch update stays selected: same results; uavenv_dqn_slots_loop_set_multi_update changes it again).
 * UAVENV_EINVAL, with the loop left as it was, for: more than 4 layer-2 outputs; no ring.valid; batch == 0; a NULL buffer; a capacity
 * other than frames * n_envs; whatever uavenv_per_fill_frame_slots refuses of the trees. */
typedef struct UavDqnSlotsPer {
    UavPer per[UAVENV_DQN_MAX_SLOTS];
    int64_t *slots_dev;          /* [n_slots][batch]: the tree slots of the last draw */
    double *prio_dev;            /* [n_slots][batch + (batch + 255) / 256] */
    float *w_dev;                /* [n_slots][batch]: importance weights */
    float *abs_dev;              /* [n_slots][batch]: |TD| of the last gradient */
    double alpha, beta, beta_inc, eps, clip;
} UavDqnSlotsPer;
int uavenv_dqn_slots_loop_set_per(UavDqnSlotsLoop *loop, const UavDqnSlotsPer *cfg);
int uavenv_dqn_slots_loop_get_per(const UavDqnSlotsLoop *loop, double *beta_out);
/* Enqueue n_steps passes on `stream`; never synchronises. */
int uavenv_dqn_slots_loop_run(UavDqnSlotsLoop *loop, int32_t n_steps, void *stream);
int uavenv_dqn_slots_loop_get(const UavDqnSlotsLoop *loop, UavDqnSlotsLoopCursor *out);

/* ---- federated merge of the per-UAV trainers (Envs/PathPlan_City.py:469-475 -> Federated_Learning_AC :590-601) --------------
 * Every one of the n_blocks flat f32 parameter blocks (device pointers, 16-byte aligned, distinct, n_floats each; the array
 * itself is HOST memory) <- scale * (block[0] + block[1] + ... in that order), one launch.  scale = 1 is the reference AS
 * EXECUTED (its division at :597 assigns into a temporary dict and never reaches the model: every UAV receives the SUM of
 * the actors through replace_param, Trainer/SAC_Trainer.py:456-459; tests/golden/federated_ac.npz), scale = 1 / n_blocks the
 * mean its comment intends.  Adam moments are not touched (replace_param leaves the optimizers alone). */
#define UAVENV_FED_MAX_BLOCKS 8
int uavenv_fed_aggregate(float *const *blocks, int32_t n_blocks, int32_t n_floats, float scale, void *stream);

/* ---- selective federated merge of DQN-family slot learners (Federated_Learning_choice, Envs/PathPlan_City.py:644-684) ----------
 * For p = 0 .. n_nets-1 IN ORDER, each step on the blocks as the earlier steps left them: q_local of nets[p] (host array, as
 * uavenv_dqn_act_slots takes it) and of every other net are forwarded (f32 MFMA) on net p's n_states packed rows
 * obs_dev[frame][agent] named by pairs_dev[p][s] = (frame, agent) -- uavenv_replay_draw_slots' layout --,
 * d[p][j] = mean((q_p - q_j)^2) over all n_states x n_actions elements (f32), the others are sorted by d ascending, stably (ties
 * keep the index order), the first (n_nets - 1) / 2 are chosen, and nets[p]->local <- (w_p + w_c0 + w_c1 + ...) / (k + 1): f32
 * adds in chosen order, then a correctly rounded division.  Only `local` blocks are written (replace_param,
 * Trainer/DuelingDQN_Trainer.py:204-207): targets and Adam moments stay.  One launch of one workgroup; never synchronises.
 * dist_out_dev (nullable, [n_nets][n_nets] f32, row p as step p computed it, 0 on the diagonal) and chosen_out_dev (nullable,
 * [n_nets][n_nets] int32, row p = the chosen indices in order, padded with -1) are diagnostics.
 * *status_out_dev (mandatory) <- 0, or 1 when any pair is out of range (0 <= frame < frames, 0 <= agent < n_agents): then NO block
 * is written (nor dist / chosen) -- an out-of-range index never becomes an address.
 * UAVENV_EINVAL, with nothing enqueued, for: n_nets outside 1..UAVENV_DQN_MAX_SLOTS; n_states outside 1..16; a NULL net, obs, pairs
 * or status pointer; a `local` block or obs_dev off 16 bytes; two nets sharing a `local` block; an f16-MFMA net; nets that differ in
 * n_actions or dueling; a head uavenv_dqn_act_slots refuses; frames <= 0 or n_agents <= 0. */
int uavenv_fed_choice(const void *obs_dev, int32_t frames, int32_t n_agents, const int32_t *pairs_dev, int32_t n_states,
                      const UavDqnNet *const *nets, int32_t n_nets, float *dist_out_dev, int32_t *chosen_out_dev,
                      int32_t *status_out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UAVENV_H */
