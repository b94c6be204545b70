/*
 * wurm_hip.h — C ABI of libwurm_hip.so, the MI355X (gfx950) implementation of the batched environment step of
 * oscarknagg/wurm: wurm.envs.SingleSnake / SimpleGridworld / MultiSnake .step() / .reset() / ._observe().
 *
 * The reference exposes no FFI for this path — its boundary is the Python class API of wurm/envs
 * (wurm/envs/__init__.py:1-3).  Each entry point below names the reference method it replaces; the Python
 * classes in wurm_amd/envs/ (same constructor signatures, attributes and return conventions as the
 * reference's) are thin callers of this ABI, and INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add to call it from the wurm/envs modules directly.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HBM), caller-allocated and caller-owned.  Nothing is allocated, freed
 *    or synchronised here: each call enqueues kernels on `stream` (a hipStream_t passed as void*, NULL = the
 *    default stream) and returns.
 *  - State layout is the reference's: fp32 NCHW holding exact small integers.
 *      SingleSnake     envs (N,3,S,S) = [food, head, body]         (single_snake.py:87, config.py:7-9)
 *      SimpleGridworld envs (N,2,S,S) = [food, agent]              (simple_gridworld.py:74)
 *      MultiSnake      foods (N,1,S,S), heads/bodies (N*K,1,S,S), agent = env*K + i   (multi_snake.py:100-108)
 *  - done / info outputs are one byte per env holding 0 or 1 (torch.bool / torch.uint8 storage).
 *  - Return value: WURM_OK or a negative WURM_ERR_* code; the Python layer maps codes onto the reference's
 *    exception types (TypeError / RuntimeError / NotImplementedError / ValueError).
 *  - Randomness: the reference draws from torch's global RNG in a way no other implementation can restate
 *    (SURVEY.md §0 fact 6).  This ABI uses a counter-based generator, Philox4x32-10 keyed by `seed`, with
 *    counter (global env id = env_offset + i, `call`, purpose): results do not depend on how envs are
 *    sharded over GPUs.  `call` must be different for every step()/reset() call of one env object (the
 *    Python classes count calls).  Every `inject_*` argument is nullable; when non-NULL it supplies the
 *    random outcomes (used to replay outcomes recorded from the reference in parity tests).
 *  - Supported grid sizes: 3 <= S <= 64.  Env ids must be < 2^32.
 */
#ifndef WURM_HIP_H
#define WURM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WURM_OK 0
#define WURM_ERR_INVALID_ARG (-1) /* -> RuntimeError / ValueError   */
#define WURM_ERR_UNSUPPORTED (-2) /* -> NotImplementedError         */
#define WURM_ERR_HIP (-3)         /* a HIP launch failed            */
#define WURM_ERR_DTYPE (-4)       /* -> TypeError                   */
#define WURM_MIRROR_REFUSED 1     /* wurm_grid_step_reset only: the call ran; the mirror it was asked to build was refused */

/* observation modes: single_snake.py:130-195, simple_gridworld.py:111-133, multi_snake.py:283-334 */
#define WURM_OBS_DEFAULT 0     /* RGB/255, (N,3,S,S)  (MultiSnake: 'full', per agent)         */
#define WURM_OBS_RAW 1         /* clone of the state                                          */
#define WURM_OBS_ONE_CHANNEL 2 /* (N,1,S,S)                                                   */
#define WURM_OBS_POSITIONS 3   /* (N,4) head y,x food y,x                                     */
#define WURM_OBS_PARTIAL 4     /* (N,3*(2n+1)^2) crop around the head                         */
#define WURM_OBS_NONE 5        /* no observation written                                      */

/* element type of the `actions` tensor (single_snake.py:198-200 accepts short/int/long) */
#define WURM_ACT_I64 0
#define WURM_ACT_I32 1

/* Library / build identification: "wurm_hip <version> gfx950". */
const char *wurm_version(void);

/* Tuning / test knobs (wurm_amd/csrc/options.hpp lists them: WURM_LANE_ROLLOUT_MIN_ENVS, WURM_RESIDENT_MIN_ENVS, ...).
 * Each starts at its default, is overridden ONCE by the environment variable of the same name when the library is
 * loaded, and changes afterwards only through these calls — no launch path reads the environment.  None of them
 * changes results, only which kernel serves a call.  set / reset return WURM_ERR_INVALID_ARG for an unknown name,
 * get returns INT64_MIN.  The knobs are PROCESS-WIDE (every env object and thread sees them); an environment variable that
 * is not a whole decimal number leaves the default in place.  wurm_launch_count is an atomic diagnostic counter,
 * wurm_single_last_route and wurm_multi_last_route name the calling thread's last launch; none is state a later call
 * depends on. */
int wurm_set_option(const char *name, int64_t value);
int64_t wurm_get_option(const char *name);
int wurm_reset_option(const char *name);

/* Number of kernels the library has launched in this process so far (a plain counter: bench.py divides its growth by
 * the loop iterations to report launches per `step(a); reset(done)` iteration). */
int64_t wurm_launch_count(void);

/* Name of the row of the dispatch table (wurm_amd/csrc/single_launch.hpp: route_of) that served the last SingleSnake /
 * SimpleGridworld launch of this process: "generic", "grid_step", "lane_step", "lane_resident", "lane_wide_resident", "lane_wide", "grid_rollout",
 * "lane_rollout", "rollout_s9", "rollout_s9_injected", "rollout_lean", "rollout_generic_partial", "rollout_generic_none".
 * Diagnostic only (bench.py and tests/test_dispatch_table.py name a launch by it); a static string. */
const char *wurm_single_last_route(void);

/* Waves per env of that launch: 2 if it was rollout_s9_kernel's pair form ("rollout_s9" / "rollout_s9_injected" with at most
 * WURM_S9_PAIR_MAX_ENVS envs, default 1024: a workgroup of a stepping wave and a helper wave per env; 0 = never), 3 if it was
 * that kernel's trio form (where the helper wave would render the crops, see below: at most WURM_S9_TRIO_MAX_ENVS envs, default
 * 512, and at least WURM_S9_TRIO_MIN_STEPS steps, default 512, -1 = never: a second render wave beside the helper), else 1.
 * Results do not depend on the form.  Diagnostic only (tests/test_s9_pair_rollout.py tells the two forms apart by it). */
int wurm_single_last_waves_per_env(void);

/* Which wave of that launch rendered the partial_n crops: 1 if it was the pair form whose helper wave renders them (the pair
 * form above, partial_n, at least WURM_S9_CROP_HELPER_MIN_STEPS steps, default 256; -1 = never), else 0: the stepping wave,
 * or a kernel without that split; in the trio form wave 2 renders beside wave 1, and this stays 1.  Results do not depend on it.  Diagnostic only (tests/test_s9_crop_helper.py). */
int wurm_single_last_crop_wave(void);

/* The same for MultiSnake: the kernel instantiation that served the calling thread's last wurm_multi_* launch, by its row in
 * the list in wurm_amd/csrc/multi_snake.hip ("step_rng_full_k4_s25", "rollout_two_rng", "rollout_group_8215_rng", "reset_wg",
 * ...; "none" before the first), followed by how it was driven where one kernel is driven in several ways: "+emit_wave" /
 * "+emit_group" (the per-call step writing 'full' observations through class codes, WURM_MULTI_GROUP_STEP_WPB), "/tapes"
 * (recorded outcomes injected).  No geometry.  wurm_multi_resident_flush and wurm_multi_colours do not change it.  Diagnostic
 * only (tests/test_multi_dispatch_table.py pins the choice by it); the string is the thread's own, valid until its next call. */
const char *wurm_multi_last_route(void);

/* Number of fp32 elements one env's observation occupies (0 = invalid mode for that env family). */
int64_t wurm_single_obs_elems(int obs_mode, int obs_n, int size);
int64_t wurm_grid_obs_elems(int obs_mode, int obs_n, int size);

/* ------------------------------------------------------------------------------------------- SingleSnake */

/* SingleSnake.step (single_snake.py:197-304) + its _observe (:130-195) in one launch.
 *   envs            in/out (N,3,S,S) fp32
 *   actions         in/out (N) int64|int32 — reverse moves are rewritten in place (:221-222)
 *   reward          out (N) fp32; done, self_collision, edge_collision out (N) bytes
 *   obs             out, wurm_single_obs_elems() floats per env (ignored for WURM_OBS_NONE); the observation
 *                   of the post-step, pre-reset state (:304)
 *   inject_food     nullable (N) int32: flat cell (y*S+x) the respawned food goes to when env i eats, -1 = none */
int wurm_single_step(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                     uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                     int64_t num_envs, int size, uint64_t seed, uint64_t call, int64_t env_offset,
                     const int32_t *inject_food, void *stream);

/* SingleSnake.reset (single_snake.py:322-342) + _create_envs (:344-387): envs with done[i] != 0 are rebuilt
 * (3-segment snake at a random seed cell/direction, one food), then every env is observed.
 *   inject_reset    nullable (N,4) int32: seed_y, seed_x, direction, food_cell
 * Returns WURM_ERR_UNSUPPORTED for size <= 8 (:346-347). */
int wurm_single_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                      int size, uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_reset,
                      void *stream);

/* SingleSnake._observe (single_snake.py:130-195) */
int wurm_single_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                        void *stream);

/* T fused iterations of the caller loop of tests/test_single_snake_env.py:24-31 / experiments/main.py:212-227:
 *   for t: outputs[t] = step(actions[t]) with call = call0 + 2t;  reset(done[t]) with call = call0 + 2t + 1
 * in ONE launch with the env resident on chip.  actions (T,N) in/out; reward/done/... (T,N); obs (T,N,elems);
 * inject_food (T,N), inject_reset (T,N,4) nullable.  Bit-identical to T calls of the two entry points above. */
int wurm_single_rollout(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                        uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                        int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                        int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream);

/* wurm_single_rollout (RNG mode) for a caller that keeps the mirror of wurm_single_call.resident (wurm_single_resident_bytes;
 * *resident_valid / resident_lazy as the fields of wurm_single_call).  Grids of 12 x 12 and larger: an env the mirror's record
 * describes is read from its clock grid (2 bytes per cell instead of 12) and written back there — the planes only while the
 * mirror is not lazy — and *resident_valid = 1 afterwards (round 6: a 16-step launch of BASELINE configs[4] no longer reads
 * 127 MB of planes).  9 x 9 and every launch the clock-grid rollout does not serve: wurm_single_rollout on the planes after
 * writing a lazy valid mirror out; *resident_valid = 0.  resident == NULL: wurm_single_rollout. */
int wurm_single_rollout_resident(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                                 uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                                 int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                 int64_t env_offset, void *resident, int *resident_valid, int resident_lazy, void *stream);

/* Arguments of wurm_single_step_reset / wurm_grid_step_reset (a HOST struct of device pointers and sizes; the fields
 * shared with wurm_single_step / wurm_single_reset mean the same). */
typedef struct wurm_single_call {
    float *envs;                     /* in/out (N,3,S,S) [SimpleGridworld: (N,2,S,S)]                            */
    void *actions;                   /* in/out (N) int64|int32 (SimpleGridworld: read only)                      */
    float *reward;                   /* out (N)                                                                  */
    uint8_t *done;                   /* out (N)                                                                  */
    uint8_t *self_collision;         /* out (N), SingleSnake only                                                */
    uint8_t *edge_collision;         /* out (N)                                                                  */
    float *obs;                      /* out: observation of the post-step, PRE-reset state (single_snake.py:304) */
    float *obs_after;                /* nullable out: what reset(done) returns (:342) — the observation of every
                                        env once the envs that just finished are rebuilt with call + 1          */
    uint8_t *done_copy;              /* nullable out (N): second copy of `done`                                  */
    const uint8_t *pre_done;         /* nullable in (N): envs flagged here are rebuilt BEFORE the step, exactly as
                                        wurm_single_reset(done = pre_done, call = pre_call) would               */
    const int32_t *inject_food;      /* nullable, as wurm_single_step                                            */
    const int32_t *inject_reset;     /* nullable (N,4) [grid: (N)]: outcomes of the reset that follows the step  */
    const int32_t *inject_pre_reset; /* nullable (N,4) [grid: (N)]: outcomes of the reset in front of the step   */
    int64_t num_envs;
    int64_t env_offset;
    uint64_t seed;
    uint64_t call;                   /* counter of the step; the reset that follows it uses call + 1             */
    uint64_t pre_call;               /* counter of the reset in front of the step                                */
    int actions_dtype, obs_mode, obs_n, size;
    int post_reset;                  /* != 0: envs that finished are rebuilt (call + 1) and STORED after `obs`   */
    int start_y, start_x;            /* SimpleGridworld start location (simple_gridworld.py:254-262)             */
    void *resident;                  /* nullable in/out: wurm_single_resident_bytes() (SimpleGridworld:
                                        wurm_grid_resident_bytes()) bytes the caller owns — a compact mirror of `envs` that
                                        the step reads INSTEAD of envs and keeps current (envs itself is still written
                                        every call)                                                                */
    int resident_valid;              /* != 0: nothing but calls that were given `resident` has written envs since
                                        the mirror was last maintained; 0: it is rebuilt from envs first.
                                        SimpleGridworld also knows 2 = REFUSED: the launch that built the mirror found envs
                                        outside the lane kernel's domain; the planes stay the state and the mirror unused
                                        until the caller clears the field again (wurm_grid_resident_bytes)          */
    int resident_lazy;               /* != 0: the step does not write envs at all; envs is brought up to date by
                                        wurm_single_resident_flush (call it before anything else reads or writes
                                        envs, and before clearing resident_valid)                                 */
    uint32_t *check_mask;            /* nullable out (N), SingleSnake: wurm_single_check's mask of the POST-STEP state of
                                        every env, computed inside the step launch where the launch holds all there is to
                                        check (the resident step: an env in its domain is a well-formed snake — what is
                                        left to say is WURM_CHK_MIN_LENGTH / WURM_CHK_ONE_FOOD); WURM_CHK_NOT_COMPUTED for
                                        an env that finished in this step or that the launch cannot vouch for, and for
                                        every env when another kernel served the call.  experiments/main.py:214-215 checks
                                        `env.envs[~done]` every step: with this the check is one any() over N words       */
} wurm_single_call;

/* One launch for one iteration of the caller loop of tests/test_single_snake_env.py:24-31 /
 * experiments/main.py:212-227,
 *     obs, reward, done, info = env.step(actions);  env.reset(done)
 * in either grouping: post_reset != 0 = [step, observe, reset] (what wurm_single_rollout does per iteration); pre_done
 * given = [the reset the caller postponed, step, observe] — the host class defers reset(done) into the next step's
 * launch and flushes it with wurm_single_reset if the state is looked at in between, so `envs` is always what the
 * reference would show.  Bit-identical to the wurm_single_step / wurm_single_reset pair with the same counters. */
int wurm_single_step_reset(const wurm_single_call *c, void *stream);

/* Size in bytes of the mirror of wurm_single_call.resident for this batch, 0 if the shape is not served by it (then pass
 * resident = NULL).  Served: size 9 with observation none or partial_2 from 4096 envs on (32 bytes per env,
 * wurm_amd/csrc/lane_resident.hpp), sizes 10 and 11 with observation default, one_channel, partial_2, partial_3, positions or
 * none from 4096 envs on (48 bytes per env, lane_wide_resident.hpp; maintained by calls with resident_lazy != 0 only: a call with
 * resident_lazy == 0 steps envs without the mirror and leaves it stale — wurm_single_step_slot clears resident_valid, a caller
 * of wurm_single_step_reset does so itself), and 12 <= size <= 64 with any observation from 2^20 cells in the batch on (the 16-bit
 * clock grid of the LDS step + 48 bytes per env, grid_rollout.hip); WURM_RESIDENT_MIN_ENVS replaces the thresholds by
 * a number of envs.  With the mirror the per-call step of a large batch does not read the (N,3,S,S) state at all.  Protocol: a call of
 * wurm_single_step_reset with `resident` given leaves the mirror current unless it had inject_* / post_reset set;
 * wurm_single_step_slot maintains c->resident_valid itself after each call, the caller only CLEARS it whenever anything
 * else writes `envs` (another entry point, the caller's own code).  A call that cannot use the mirror (inject_* /
 * post_reset) flushes a lazy mirror into envs first by itself. */
int64_t wurm_single_resident_bytes(int64_t num_envs, int size, int obs_mode, int obs_n);
/* the same without the batch-size threshold: the size of the mirror whenever the SHAPE is served (a caller that asked for
 * the mirror explicitly, `resident_mirror=True` of the Python classes), 0 if it is not */
int64_t wurm_single_resident_size(int64_t num_envs, int size, int obs_mode, int obs_n);

/* resident_lazy: writes envs from the mirror (every env the mirror describes, whole; the others — states outside the
 * lane kernels' domain, which the step keeps in envs itself — are left as they are).  A no-op returning WURM_OK unless
 * c->resident, c->resident_lazy and c->resident_valid are all set.  Leaves the mirror valid. */
int wurm_single_resident_flush(const wurm_single_call *c, void *stream);

/* The same for SimpleGridworld (simple_gridworld.py:135-202,225-268). */
int wurm_grid_step_reset(const wurm_single_call *c, void *stream);

/* SimpleGridworld's mirror (round 6; wurm_amd/csrc/gridworld_lane.hip): 16 bytes of header + one 32-bit record per env (agent
 * cell | food cell << 16) — an env in the reference's own invariant IS two cell indices, so with the mirror the per-call
 * step of a large batch neither scans the (N,2,S,S) planes nor (while the mirror is lazy) writes them, and it is ONE launch:
 * the lane kernel's domain (at most one agent, at most one food, values 0 / 1) is closed under this library's own launches,
 * so once a launch has built the mirror without meeting an env outside it, none can appear until something else writes the
 * state — which is when the caller clears resident_valid.  The launch that BUILDS the mirror (resident_valid == 0) reads
 * that verdict back synchronously (4 bytes, one stream synchronisation): resident_valid becomes 1, or 2 = refused (then the
 * planes are the state, every call takes the two-launch path, and the mirror is tried again when the caller clears the
 * field).  Served: 5 <= size <= 64, observation default / raw / positions / none, from WURM_LANE_STEP_MIN_ENVS envs on
 * (WURM_RESIDENT_MIN_ENVS overrides); wurm_grid_resident_size: without the batch-size threshold.  Protocol otherwise as
 * wurm_single_resident_bytes: wurm_grid_step_slot maintains c->resident_valid (wurm_grid_step_reset, whose block is const,
 * returns WURM_MIRROR_REFUSED instead of WURM_OK from the call that was to build the mirror: the caller sets the field to 2),
 * the caller clears it whenever anything else writes envs, and wurm_grid_resident_flush writes envs from a lazy valid mirror
 * (a no-op otherwise).  0 also for an image observation whose run of four envs exceeds the lane kernel's 16 KB byte slab. */
int64_t wurm_grid_resident_bytes(int64_t num_envs, int size, int obs_mode);
int64_t wurm_grid_resident_size(int64_t num_envs, int size, int obs_mode);
int wurm_grid_resident_flush(const wurm_single_call *c, void *stream);

/* Caller-allocated output slabs holding the fresh output tensors of the next `steps` step() calls (the host classes
 * carve the tensors they return out of them; a slab is never written twice).  Layouts: obs, obs_after
 * (steps, N, elems) fp32; reward (steps, N) fp32; flags (3, steps, N) bytes = done, self_collision, edge_collision. */
typedef struct wurm_single_slabs {
    float *obs;
    float *obs_after; /* nullable */
    float *reward;
    uint8_t *flags;
    int64_t steps;
} wurm_single_slabs;

/* wurm_single_step_reset with the per-call bookkeeping of the host class done here instead of in Python (at 512 envs
 * the loop of experiments/main.py:212-227 is bound by host time per call): fills c->actions / actions_dtype / call and
 * the output pointers of slot `slot` of the slabs (obs_after only if want_obs_after), sets c->pre_done = c->done_copy
 * and c->pre_call when `apply_pending` (the reset the caller postponed), else clears c->pre_done, and launches.
 * Everything else in *c (envs, sizes, seed, modes, done_copy, injections) is left as the caller set it. */
int wurm_single_step_slot(wurm_single_call *c, const wurm_single_slabs *slabs, int64_t slot, void *actions,
                          int actions_dtype, uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after,
                          void *stream);

/* The same for SimpleGridworld (the self_collision plane of `flags` is not written). */
int wurm_grid_step_slot(wurm_single_call *c, const wurm_single_slabs *slabs, int64_t slot, void *actions,
                        int actions_dtype, uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after,
                        void *stream);

/* The acting half of the single-agent loop, experiments/main.py:207-212,227, T iterations in ONE launch:
 *   probs, value = model(state)            FeedforwardAgent, wurm/agents/feedforward.py:8-28: E -> 64 -> 64 -> {4, 1}
 *   action = Categorical(probs).sample()   main.py:208-210
 *   state, reward, done, info = env.step(action);  env.reset(done)     (`state`: the PRE-reset observation, :212)
 * obs0 (N,E): the observation the policy acts on at step 0 (the caller's `state`), E = 3 (2 obs_n + 1)^2.
 * params: W1 (64,E) b1 (64) W2 (64,64) b2 (64) Wp (4,64) bp (4) Wv (64) bv (1), fp32, torch Linear layout,
 * concatenated.  Outputs (T,N,..): actions int64 (sanitised by step as in the reference), probs (4), values, reward,
 * done, collision flags, obs (E) = the observation step t returned = the policy input of step t+1.
 * status (N) uint8: 0 = rolled out; 1 = the env's state is outside the kernel's domain (not a well-formed snake):
 * it is left untouched and its outputs are not written.  Step t uses call0 + 2t (env step and the sampling draw),
 * its reset call0 + 2t + 1.  Arithmetic order of the policy: see wurm_amd/csrc/policy_rollout.hpp.
 * Supported: 9 <= size <= 64, 0 <= obs_n <= 6 (sizes 9-11 with obs_n <= 3 on policy_rollout.hpp's kernels, the rest on
 * policy_wide.hpp's; WURM_POLICY_WIDE = 1 sends every shape to the latter).  Outside: WURM_ERR_UNSUPPORTED. */
int wurm_single_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                               float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                               uint8_t *edge_collision, float *obs, uint8_t *status, int obs_n, int64_t num_envs,
                               int size, int64_t num_steps, uint64_t seed, uint64_t call0, int64_t env_offset,
                               void *stream);

/* wurm_single_policy_rollout with the observation mode as an argument: WURM_OBS_PARTIAL (obs_n as there) or
 * WURM_OBS_POSITIONS (E = 4: head row, head column, food row, food column; obs_n ignored), 9 <= size <= 64.  The image
 * modes and WURM_OBS_NONE return WURM_ERR_UNSUPPORTED: the reference's feed-forward agent takes a flat observation
 * (experiments/main.py:129-137). */
int wurm_single_policy_rollout_mode(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                    float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                                    uint8_t *edge_collision, float *obs, uint8_t *status, int obs_mode, int obs_n,
                                    int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                    int64_t env_offset, void *stream);

/* wurm_single_policy_rollout_mode for a POPULATION: the num_envs envs are num_members members of M = num_envs /
 * num_members consecutive envs each, member m owns envs [m M, (m + 1) M) and acts with row m of params
 * (num_members, num_params), each row packed as above.  Still one launch, the same kernels' arithmetic and the same
 * routes; every draw is keyed by env_offset + env, so member m's columns of every output and its rows of envs are bit
 * for bit those of a stand-alone call on its M envs with env_offset + m M.  num_members <= 0 or num_envs % num_members
 * != 0: WURM_ERR_INVALID_ARG; every other refusal is wurm_single_policy_rollout_mode's.  num_members == 1 is that call. */
int wurm_single_policy_rollout_pop(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                   float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                                   uint8_t *edge_collision, float *obs, uint8_t *status, int obs_mode, int obs_n,
                                   int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                   int64_t env_offset, void *stream, int64_t num_members);

/* Name of the kernel that served the calling thread's last policy rollout: "policy_s9", "policy_generic" (both
 * policy_rollout.hpp), "policy_wide" (policy_wide.hpp), or "none". */
const char *wurm_policy_last_route(void);

/* wurm.utils.env_consistency / snake_consistency (wurm/utils.py:113-178) as a per-env error bitmask
 * (bit i = i-th check failed, WURM_CHK_*; 0 = consistent).  err out (N) uint32. */
#define WURM_CHK_FOOD_VALUE 1u
#define WURM_CHK_ONE_HEAD 2u
#define WURM_CHK_HAS_SNAKE 4u
#define WURM_CHK_HEAD_AT_END 8u
#define WURM_CHK_BODY_RANGE 16u
#define WURM_CHK_MIN_LENGTH 32u
#define WURM_CHK_HEAD_ON_FOOD 64u
#define WURM_CHK_ONE_FOOD 128u
int wurm_single_check(const float *envs, uint32_t *err, int64_t num_envs, int size, void *stream);

/* ------------------------------------------------------------------------------------------- SimpleGridworld */

/* SimpleGridworld.step (simple_gridworld.py:135-202) + _observe (:111-133); actions are read only. */
int wurm_grid_step(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                   uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                   uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_food, void *stream);

/* SimpleGridworld.reset (simple_gridworld.py:225-268): agent at (start_y,start_x), one food.
 *   inject_reset nullable (N) int32 food cell.  WURM_ERR_UNSUPPORTED for size <= 4 or no start location (:249-260). */
int wurm_grid_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                    int size, int start_y, int start_x, uint64_t seed, uint64_t call, int64_t env_offset,
                    const int32_t *inject_reset, void *stream);

int wurm_grid_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      void *stream);

int wurm_grid_rollout(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                      uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0,
                      int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream);

/* The fused acting loop of wurm_single_policy_rollout for SimpleGridworld, 'positions' observations (E = 4), start
 * location as wurm_grid_rollout's, 5 <= size <= 64.  Same outputs minus self_collision.  status (N): 1 = the env does not
 * hold exactly one agent and one food (left untouched, its outputs not written). */
int wurm_grid_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                             float *values, float *reward, uint8_t *done, uint8_t *edge_collision, float *obs,
                             uint8_t *status, int64_t num_envs, int size, int64_t num_steps, int start_y, int start_x,
                             uint64_t seed, uint64_t call0, int64_t env_offset, void *stream);

/* wurm_grid_policy_rollout for a population: params (num_members, num_params), member m owns the envs
 * [m M, (m + 1) M), M = num_envs / num_members — as wurm_single_policy_rollout_pop. */
int wurm_grid_policy_rollout_pop(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                 float *values, float *reward, uint8_t *done, uint8_t *edge_collision, float *obs,
                                 uint8_t *status, int64_t num_envs, int size, int64_t num_steps, int start_y,
                                 int start_x, uint64_t seed, uint64_t call0, int64_t env_offset, void *stream,
                                 int64_t num_members);

/* wurm_grid_rollout (RNG mode) for a caller that keeps SimpleGridworld's mirror (wurm_grid_resident_bytes; *resident_valid and
 * resident_lazy as the fields of wurm_single_call): where the one-env-per-lane kernel serves the launch, the state comes from
 * the records when *resident_valid == 1 — no scan of the planes, no flag pass behind the launch, and (lazy) no write to the
 * planes — and the records describe the final state afterwards.  A launch that BUILDS the mirror reads its verdict back
 * (one stream synchronisation): *resident_valid = 1, or 2 = refused.  Any other launch runs wurm_grid_rollout on the planes
 * after writing a lazy valid mirror out, and leaves *resident_valid = 0 (2 stays 2).  resident == NULL: wurm_grid_rollout. */
int wurm_grid_rollout_resident(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                               uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                               int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0, int64_t env_offset,
                               void *resident, int *resident_valid, int resident_lazy, void *stream);

/* ------------------------------------------------------------------------------------------- MultiSnake */

/* Dynamics parameters of MultiSnake (attributes the reference lets callers change after construction,
 * multi_snake.py:121-129; tests/test_multi_snake_env.py:180,288,401-403 set them).  A HOST struct. */
typedef struct wurm_multi_config {
    int boost;             /* self.boost                                           multi_snake.py:123 */
    int food_on_death;     /* self.food_on_death_prob > 0                          :565,662           */
    float death_threshold; /* (float)(1 - food_on_death_prob): food where u > threshold   :424        */
    float boost_cost_prob; /* boost cost where u < boost_cost_prob                 :579               */
    int food_mode;         /* 0 = 'only_one', 1 = 'random_rate'                    :369,380           */
    float food_rate;       /* rate food where u < food_rate                        :403               */
    int max_food;          /* num_snakes * 8                                       :127               */
    float reward_on_death; /*                                                      :684               */
    int respawn_any;       /* respawn_mode == 'any'                                :805               */
    int colour_random;     /* colour_mode == 'random'                              :800               */
} wurm_multi_config;

/* Recorded random outcomes for wurm_multi_step (all DEVICE pointers; pass the struct pointer as NULL for RNG mode). */
typedef struct wurm_multi_inject {
    const uint8_t *death_a;   /* (N,S,S) outcome of `rand_like > 1-p`, boost phase    :424 via :574 */
    const uint8_t *cost;      /* (N*K)   outcome of `rand < boost_cost_prob`          :579          */
    const uint8_t *death_b;   /* (N,S,S) outcome of `rand_like > 1-p`, regular phase  :424 via :671 */
    const uint8_t *rate;      /* (N,S,S) outcome of `rand < food_rate`                :401-403      */
    const int32_t *food_cell; /* (N)     'only_one' respawn cell, -1 = none           :374-379      */
} wurm_multi_inject;

/* Recorded random outcomes for wurm_multi_reset (DEVICE pointers; NULL struct pointer = RNG mode). */
typedef struct wurm_multi_reset_inject {
    const int32_t *create;      /* (N,K,2) seed cell, direction of every snake of a rebuilt env    :996-1019 */
    const int32_t *create_food; /* (N)     food cell of a rebuilt env                               :1016     */
    const int16_t *colours;     /* (N*K,3) colour given to snakes still dead after the reset        :800-803  */
    const int32_t *respawn;     /* (N,2)   respawn_mode 'any': seed cell (-1 = no room), direction  :805-829  */
} wurm_multi_reset_inject;

/* floats per (agent, env) of an observation: 'full' (WURM_OBS_DEFAULT) 3*S*S, 'partial_n' 3*(2n+1)^2 */
int64_t wurm_multi_obs_elems(int obs_mode, int obs_n, int size);

/* MultiSnake.step (multi_snake.py:462-731) + _observe (:283-334) in one launch.
 *   foods (N,1,S,S), heads/bodies (N*K,1,S,S) fp32 in/out; dones (N*K) bytes in/out; orientations (N*K) int64
 *   in/out; actions (K,N) int64: actions[i*N + e] = agent_i's action (0..7) in env e (the reference stacks its
 *   dict the same way, :492); colours (N*K,3) int16 (agent_colours, read by 'partial_n').
 *   Outputs, (N*K) in the reference's agent order env*K + i: boost_this_step, rewards, snake_collision,
 *   edge_collision, food_consumed (info 'food_i'), sizes (info 'size_i'); all_done (N) = dones['__all__'].
 *   obs (K,N,elems): obs[i] is agent_i's tensor.
 *   agent_major_f32 / agent_major_u8: nullable.  The same per-agent outputs transposed to agent-major (K,N) rows, so
 *   that the per-agent dicts of :701-729 are plain row views: f32 (3,K,N) = rewards, food_consumed, sizes;
 *   u8 (4,K,N) = dones, boost_this_step, snake_collision, edge_collision. */
int wurm_multi_step(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                    const int64_t *actions, uint8_t *boost_this_step, float *rewards, uint8_t *snake_collision,
                    uint8_t *edge_collision, float *food_consumed, float *sizes, uint8_t *all_done,
                    const int16_t *colours, float *obs, int obs_mode, int obs_n, int64_t num_envs, int num_snakes,
                    int size, const wurm_multi_config *cfg, uint64_t seed, uint64_t call, int64_t env_offset,
                    const wurm_multi_inject *inject, float *agent_major_f32, uint8_t *agent_major_u8, void *stream);

/* Arguments of wurm_multi_step_reset: the pointers and sizes of wurm_multi_step (same meaning), plus the postponed
 * reset.  A HOST struct of device pointers. */
typedef struct wurm_multi_call {
    float *foods, *heads, *bodies;
    uint8_t *dones;
    int64_t *orientations;
    int16_t *colours;                 /* in/out when pre_done is given (re-rolled colours), else read ('partial_n')   */
    const int64_t *actions;           /* (K,N)                                                                         */
    uint8_t *boost_this_step;
    float *rewards;
    uint8_t *snake_collision, *edge_collision;
    float *food_consumed, *sizes;
    uint8_t *all_done;                /* out (N) = dones['__all__']                                                    */
    uint8_t *all_done_copy;           /* nullable out (N): second copy of all_done                                     */
    float *obs;
    float *obs_after;                 /* nullable out, shaped like obs: what wurm_multi_reset(done_env = all_done,
                                         call = call + 1) would return — the observation of every agent after the
                                         envs that just finished are rebuilt, dead snakes' colours re-rolled and
                                         (respawn_any) one dead snake respawned.  Only written: that reset is NOT
                                         applied to the state tensors (pass all_done_copy as the next pre_done)         */
    float *agent_major_f32;           /* nullable, as wurm_multi_step                                                  */
    uint8_t *agent_major_u8;
    const uint8_t *pre_done;          /* nullable in (N): wurm_multi_reset(done_env = pre_done, call = pre_call, no
                                         observation) is applied to every env BEFORE the step                         */
    const wurm_multi_inject *inject;            /* nullable: outcomes of the step                                      */
    const wurm_multi_reset_inject *pre_inject;  /* nullable: outcomes of the reset in front of it                      */
    int64_t num_envs, env_offset;
    uint64_t seed, call, pre_call;
    int num_snakes, size, obs_mode, obs_n;
    wurm_multi_config cfg;
    void *resident;                   /* nullable in/out: wurm_multi_resident_bytes() bytes the caller owns — a compact
                                         mirror of foods / heads / bodies that the step reads INSTEAD of them and keeps
                                         current (dones, orientations, colours are always read and written in place)      */
    int resident_valid;               /* != 0: nothing but calls that were given `resident` has written foods / heads /
                                         bodies since the mirror was last maintained; 0: the step reads them            */
    int resident_lazy;                /* != 0: the step does not write foods / heads / bodies; wurm_multi_resident_flush
                                         brings them up to date (before anything else reads or writes them, and before
                                         resident_valid is cleared)                                                     */
    uint32_t *check_mask;             /* nullable out (N): wurm_multi_check's mask of the post-step state, computed from
                                         the on-chip image inside the step launch — for an env whose image came from the
                                         mirror or from a rebuild; 0xffffffff = not computed (the env was read from the
                                         fp32 tensors, which can hold more than the image: run wurm_multi_check)         */
    uint32_t *check_mask_after;       /* nullable out (N), with obs_after: the same for the state obs_after observes   */
} wurm_multi_call;

/* One launch for one iteration of the caller loop of experiments/speeds.py:30-37 / tests/test_multi_snake_env.py:78-89,
 *     obs, rewards, dones, info = env.step(actions);  env.reset(dones['__all__'])
 * as [the reset the caller postponed, step, observe]: the host class defers reset(...) into the next step's launch and
 * flushes it with wurm_multi_reset if the state is looked at in between.  Bit-identical to the wurm_multi_reset (without
 * observation) / wurm_multi_step pair with the same counters.  pre_done = NULL: plain wurm_multi_step. */
int wurm_multi_step_reset(const wurm_multi_call *c, void *stream);

/* wurm_multi_step_reset for a host loop that keeps ONE call block alive (state pointers, sizes, seed, configuration,
 * all_done_copy) and hands over only what changes from step to step; the output pointers of the block are filled from
 * two packed buffers (so that the Python class allocates twice per step, not six times, and unbinds them into the
 * per-agent dicts of multi_snake.py:701-729); obs_after (nullable) as in wurm_multi_call:
 *   out_f32 (6*K*N floats): [0,KN) rewards, [KN,2KN) food_consumed, [2KN,3KN) sizes, env-major [env*K + i];
 *                           then the same three agent-major, (3,K,N), [i*N + env]
 *   out_u8 (7*K*N + N bytes): boost_this_step, snake_collision, edge_collision env-major; then agent-major (4,K,N)
 *                           dones, boost, snake_collision, edge_collision; then all_done (N)
 *   apply_pending != 0: the postponed reset with pre_done = c->all_done_copy (the previous step's all_done) and
 *                           counter pre_call goes in front of the step.
 * c->inject / c->pre_inject are used as they stand.  Bit-identical to wurm_multi_step_reset on the same pointers. */
int wurm_multi_step_packed(wurm_multi_call *c, float *out_f32, uint8_t *out_u8, float *obs, float *obs_after,
                           const int64_t *actions, uint64_t call, int apply_pending, uint64_t pre_call, void *stream);

/* Caller-allocated output slabs holding the fresh output tensors of the next `steps` step() calls of MultiSnake (as
 * wurm_single_slabs: the host class carves the tensors of its per-agent dicts, multi_snake.py:701-729, out of them ONCE per
 * slab; a slab is never written twice).  Per step the layouts of wurm_multi_step_packed:
 * out_f32 (steps, 6 K N) floats; out_u8 (steps, 7 K N + N) bytes; obs, obs_after (steps, K, N, elems) floats. */
typedef struct wurm_multi_slabs {
    float *out_f32;
    uint8_t *out_u8;
    float *obs;
    float *obs_after; /* nullable */
    int64_t steps;
    int64_t obs_elems; /* floats per (agent, env) of an observation: wurm_multi_obs_elems(c->obs_mode, c->obs_n, c->size) */
} wurm_multi_slabs;

/* wurm_multi_step_packed on slot `slot` of the slabs (obs_after only if want_obs_after): one C call per
 * `env.step(actions)` with nothing to allocate or to compute on the host (wurm_amd/csrc/fastcall.c: Stepper.step_multi). */
int wurm_multi_step_slot(wurm_multi_call *c, const wurm_multi_slabs *slabs, int64_t slot, const int64_t *actions,
                         uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after, void *stream);

/* The mirror of wurm_multi_call.resident: per env the 16-bit clock grids of the K bodies, the food grid as bytes and three
 * ints per snake — (2 K + 1) S^2 bytes and change instead of (1 + 2 K) S^2 fp32 read every call
 * (wurm_amd/csrc/multi_device.hpp).  Returns its size in bytes, 0 if it is not offered for this batch (fewer than 2^20
 * cells num_envs * num_snakes * size^2; WURM_RESIDENT_MIN_ENVS replaces that by a number of envs).  Protocol as for
 * wurm_single_call.resident: wurm_multi_step_packed sets c->resident_valid after a launch that maintained the mirror
 * (not with inject / pre_inject: such a call writes a lazy mirror out first and steps the fp32 state), the caller clears it
 * whenever anything else writes the state — after wurm_multi_resident_flush if the mirror is lazy. */
int64_t wurm_multi_resident_bytes(int64_t num_envs, int num_snakes, int size);
int64_t wurm_multi_resident_size(int64_t num_envs, int num_snakes, int size); /* without the batch-size threshold */
int wurm_multi_resident_flush(const wurm_multi_call *c, void *stream);

/* MultiSnake.reset (multi_snake.py:771-836): envs flagged in done_env (N bytes) are rebuilt (_create_envs
 * :996-1019: K snakes placed one after another on free cells away from everything, one food); colours of
 * snakes that are still dead are re-rolled (colour_random); respawn_any: the first dead snake of every env
 * respawns if there is room; then every agent is observed (obs may be NULL / WURM_OBS_NONE).
 *   status: nullable, 1 int32, incremented for every env in which a rebuilt snake found no room (the reference
 *   raises RuntimeError at :946-947). */
int wurm_multi_reset(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                     int16_t *colours, const uint8_t *done_env, int32_t *status, const uint8_t *boost_this_step,
                     float *obs, int obs_mode, int obs_n, int64_t num_envs, int num_snakes, int size,
                     const wurm_multi_config *cfg, uint64_t seed, uint64_t call, int64_t env_offset,
                     const wurm_multi_reset_inject *inject, void *stream);

/* T fused iterations of the caller loop of experiments/speeds.py:30-37 / tests/test_multi_snake_env.py:78-89:
 *   for t: outputs[t], obs[t] = step(actions[t]) with call = call0 + 2t;  reset(dones['__all__']) with call0 + 2t + 1
 * in ONE launch with the env resident on chip (LDS).  Bit-identical to T calls of wurm_multi_step / wurm_multi_reset
 * (the latter without observation).
 *   actions (T,K,N) int64;  out_f32 (T,3,K,N) = rewards, food_consumed, sizes;  out_u8 (T,4,K,N) = dones,
 *   boost_this_step, snake_collision, edge_collision (agent-major rows, as the agent_major_* outputs of
 *   wurm_multi_step);  all_done (T,N);  obs (T,K,N,elems).  State tensors, dones, orientations, colours and
 *   boost_this_step (nullable) are updated in place to the state after the last reset.
 *   inject / reset_inject: both NULL (RNG mode) or both given, each array with a leading T dimension. */
int wurm_multi_rollout(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                       int16_t *colours, uint8_t *boost_this_step, const int64_t *actions, float *out_f32,
                       uint8_t *out_u8, uint8_t *all_done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                       int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg, uint64_t seed,
                       uint64_t call0, int64_t env_offset, const wurm_multi_inject *inject,
                       const wurm_multi_reset_inject *reset_inject, void *stream);

/* wurm_multi_rollout (RNG mode) for a caller that keeps the compact mirror of wurm_multi_call (`resident`,
 * wurm_multi_resident_bytes() bytes; same meaning of *resident_valid / resident_lazy as there): where the launch is served by
 * the kernel that can keep it ('full' observations of at most 10 snakes, more than one step, a large batch) the state is
 * read from the mirror when *resident_valid != 0 — 2 K + 1 bytes per cell instead of (1 + 2 K) fp32 planes — and the mirror
 * describes the final state afterwards (*resident_valid = 1); foods / heads / bodies are then written only if
 * resident_lazy == 0.  Any other shape runs wurm_multi_rollout on the fp32 planes: a lazy valid mirror is written out to
 * them first (wurm_multi_resident_flush) and *resident_valid = 0 afterwards.  resident == NULL: wurm_multi_rollout.
 * Replaces nothing in the reference (MultiSnake has no fused loop); it is to `env.rollout` what wurm_multi_step_packed's
 * mirror is to `env.step` (multi_snake.py:462-731, 771-836 over T iterations). */
int wurm_multi_rollout_resident(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                                int16_t *colours, uint8_t *boost_this_step, const int64_t *actions, float *out_f32,
                                uint8_t *out_u8, uint8_t *all_done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                                int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg, uint64_t seed,
                                uint64_t call0, int64_t env_offset, void *resident, int *resident_valid, int resident_lazy,
                                void *stream);

/* MultiSnake._observe (multi_snake.py:283-334) */
int wurm_multi_observe(const float *foods, const float *heads, const float *bodies, const uint8_t *dones,
                       const uint8_t *boost_this_step, const int16_t *colours, float *obs, int obs_mode, int obs_n,
                       int64_t num_envs, int num_snakes, int size, void *stream);

/* MultiSnake.check_consistency (multi_snake.py:733-769) as a per-env bitmask: bits 0-6 = WURM_CHK_* of any living
 * snake, WURM_MCHK_OVERLAP, WURM_MCHK_DEAD_NONZERO. */
#define WURM_CHK_NOT_COMPUTED 0xFFFFFFFFu /* wurm_single_call.check_mask / wurm_multi_call.check_mask: run the checker */
#define WURM_MCHK_OVERLAP 0x100u
#define WURM_MCHK_DEAD_NONZERO 0x200u
int wurm_multi_check(const float *foods, const float *heads, const float *bodies, const uint8_t *dones, uint32_t *err,
                     int64_t num_envs, int num_snakes, int size, void *stream);

/* MultiSnake.get_n_colours (multi_snake.py:163-169) at construction: random colour per agent (fixed = 0) or one
 * colour per snake index shared by all envs (fixed = 1; :146-148).  colours out (N*K,3) int16. */
int wurm_multi_colours(int16_t *colours, int64_t num_envs, int num_snakes, int fixed, uint64_t seed, uint64_t call,
                       int64_t env_offset, void *stream);

/* The acting half of the multi-agent loop (experiments/multiagent.py:354-364) for every snake and every species in ONE
 * launch: per (snake k, env i) row  probs, value = model_s(obs[k][i]);  action = Categorical(probs).sample()  with the
 * 2 x 64 feed-forward actor-critic of species s = k * num_species / num_snakes (integer division, multiagent.py:356).
 * Kernel: wurm_amd/csrc/multi_act.hpp.  The arithmetic is wurm_single_policy_rollout's, bit for bit.
 *   params  (num_species, P) fp32, row s as pack_policy_params, P = 64 E + 64 + 4096 + 64 + 256 + 4 + 64 + 1
 *   obs     (num_snakes, num_envs, E) fp32, contiguous: MultiSnake's 'partial_n' observations, agent-major as `step`
 *           lays them out;  E = num_inputs = 3 (2n+1)^2, n <= 6
 *   actions (num_snakes, num_envs) int64, written: 0..3 — the agent-major block wurm_multi_step reads
 *   probs   (num_snakes, num_envs, 4) fp32, written, nullable;  values (num_snakes, num_envs) fp32, written, nullable
 *   The uniform of row (k, i) is u01 of word 0 of Philox(seed; env = (env_offset + i) * num_snakes + k, call, purpose 8):
 *   `call` is a POLICY call counter the caller keeps beside the env's own; this entry point consumes none of the latter.
 * Refused before any HIP call: negative sizes, num_species < 1 or > num_snakes (so num_snakes = 0 is refused), and — with
 * num_envs > 0 — null params, obs or actions (WURM_ERR_INVALID_ARG); a num_inputs that is not 3 (2n+1)^2 with n <= 6
 * (WURM_ERR_UNSUPPORTED).  num_envs = 0 is a successful no-op without a launch.  Otherwise exactly one launch on
 * `stream`, whatever the sizes; no atomics. */
int wurm_multi_act(const float *params, const float *obs, int64_t *actions, float *probs, float *values,
                   int64_t num_envs, int num_snakes, int num_species, int num_inputs, uint64_t seed, uint64_t call,
                   int64_t env_offset, void *stream);

/* wurm_multi_act with a LINE-UP per env: a league of num_policies policies in one batch, every (snake k, env i) row
 * r = k * num_envs + i played by the policy the caller's lists name (experiments/eval.py: random matchups of agents out
 * of a folder of checkpoints, one process each there).  Kernel: wurm_amd/csrc/multi_league.hpp.  The arithmetic, the
 * outputs and the draw of a row are wurm_multi_act's, bit for bit: they do not depend on who plays the other rows.
 *   params  (>= num_policies, P) fp32, row a as pack_policy_params;  obs, actions, probs, values as for wurm_multi_act
 *   order   (num_snakes * num_envs) int32, device: the rows sorted by policy
 *   offsets (num_policies + 1) int64, device: policy a plays the rows order[offsets[a] .. offsets[a + 1]).  Neither is read
 *           on the host.  The kernel clamps the offsets to [0, num_snakes * num_envs] and skips an entry of `order` outside
 *           [0, num_snakes * num_envs): it reads and writes in bounds whatever the two hold.  A row no list names is not
 *           written.  num_policies may exceed num_snakes, and 256; a policy without rows is legal.
 * Refused before any HIP call: negative sizes, num_policies < 1 and — with num_envs > 0 and num_snakes > 0 — null params,
 * obs, order, offsets or actions (WURM_ERR_INVALID_ARG); a num_inputs that is not 3 (2n+1)^2 with n <= 6, and
 * num_snakes * num_envs >= 2^31 (WURM_ERR_UNSUPPORTED).  num_envs = 0 (or num_snakes = 0) is a successful no-op without a
 * launch.  Otherwise exactly one launch on `stream`, its grid sized from num_snakes, num_envs and num_policies alone; no
 * atomics. */
int wurm_multi_act_league(const float *params, const float *obs, const int32_t *order, const int64_t *offsets,
                          int64_t *actions, float *probs, float *values, int64_t num_envs, int num_snakes,
                          int num_policies, int num_inputs, uint64_t seed, uint64_t call, int64_t env_offset, void *stream);

/* The per-policy results of one window of such a league, added to a persistent device table.
 *   rewards (T, R) fp32, dones (T, R) bytes: R = num_rows = num_snakes * num_envs columns k * num_envs + i, T = num_steps
 *   food, size (T, R) fp32, boost, snake_collision, edge_collision (T, R) bytes: each nullable (its column gets nothing)
 *   order, offsets: as for wurm_multi_act_league, with the same clamping and skipping
 *   table   (num_policies, 8) doubles, added to.  Row a, over the rows of policy a and the T steps: [0] steps (row-steps:
 *           T per row), [1] the sum of rewards, [2] deaths (steps with done set), [3] food, [4] snake_collisions,
 *           [5] edge_collisions, [6] boost (steps with the flag set), [7] the sum of size.
 * One workgroup per policy; per thread its list entries in order, then a fixed wave butterfly and the waves in order, in
 * double: no atomics, the same bits every run (and sums of integers and of rewards in {-1, 0, 1} are exact).
 * Refused before any HIP call: negative sizes, num_policies < 1 and — with num_rows > 0 and num_steps > 0 — null rewards,
 * dones, order, offsets or table (WURM_ERR_INVALID_ARG); num_rows >= 2^31 (WURM_ERR_UNSUPPORTED).  num_rows = 0 or
 * num_steps = 0 is a successful no-op without a launch.  Otherwise exactly one launch on `stream`. */
int wurm_multi_league_scores(const float *rewards, const uint8_t *dones, const float *food, const float *size,
                             const uint8_t *boost, const uint8_t *snake_collision, const uint8_t *edge_collision,
                             const int32_t *order, const int64_t *offsets, double *table, int64_t num_rows,
                             int64_t num_steps, int num_policies, void *stream);

/* Matchmaking on the device: the line-up of such a league DRAWN from integer tickets, and the order / offsets lists of any
 * line-up BUILT, both without a host read (kernels: wurm_amd/csrc/multi_matchmaking.hpp).  Each of the two calls takes ONE
 * argument block whose last member is the stream, the calling style of wurm_single_call / wurm_multi_call for calls of
 * many arguments.  The prototypes therefore have no `stream` parameter: the table of stream cases (tests/stream_cases.py,
 * which tests/test_stream_inventory.py holds against the prototypes that have one) does not list them, and their stream
 * cases are in tests/test_league_draw_gpu.py; a later change may move them into the table.
 *
 * wurm_league_draw.  Per env i (global id env_offset + i), seats k = 0 .. num_snakes - 1 in order:
 *   a seat with pinned[k] >= 0 goes to that policy, without a draw;
 *   else the pool is every policy — with replacement = 0 less the pinned ones (all of them, before any seat is drawn) and
 *   those already seated in this env;  t[a] = max(tickets[a], 0) (1 with tickets = NULL), total = the sum of t over the
 *   pool;  if total = 0 every member of the pool counts 1 and total = the size of the pool;
 *   w = Philox(seed; env = env_offset + i, call, purpose 10, sub = k);  x = w[0] << 32 | w[1];
 *   r = the high 64 bits of x * total;  the seat goes to the smallest a of the pool whose running sum of t, over the pool
 *   in ascending order, exceeds r.
 * Exact integer arithmetic: an env's seats depend on seed, call, env_offset + i, the tickets and the arguments, not on
 * num_envs nor on another env.  `call` is a counter of LINE-UP draws the caller keeps beside the env's own and the policy
 * call counter; this entry point consumes neither of those.
 *   tickets (num_policies) int32, device, nullable;  lineup (num_snakes, num_envs) int64, device, written
 *   pinned  HOST pointer to num_snakes ints, nullable (= all -1); read during the call only
 * Refused before any HIP call: a null block; negative num_envs or env_offset, num_snakes < 1, num_policies < 1, a pinned
 * entry outside [-1, num_policies), with replacement = 0 num_policies < num_snakes or a policy pinned twice, and — with
 * num_envs > 0 — a null lineup (WURM_ERR_INVALID_ARG); num_snakes > 64, num_snakes * num_envs >= 2^31 and env_offset +
 * num_envs > 2^32 (WURM_ERR_UNSUPPORTED).  num_envs = 0 is a successful no-op without a launch.  Otherwise exactly ONE
 * launch on `stream`, one env per lane; no atomics, no scratch. */
typedef struct wurm_league_draw {
    const int32_t *tickets;
    int64_t *lineup;
    const int32_t *pinned;
    int64_t num_envs, env_offset;
    uint64_t seed, call;
    int num_snakes, num_policies, replacement;
    void *stream;
} wurm_league_draw;
int wurm_multi_league_draw(const wurm_league_draw *args);

/* wurm_league_plan: what MultiSnake.league_plan computes with torch ops, bit for bit, in WURM_LEAGUE_PLAN_LAUNCHES launches.
 *   lineup  (num_rows) integers of lineup_dtype, device: entry r = k * num_envs + i names the policy of row r
 *   order   (num_rows) int32, written: the rows with an entry in [0, num_policies) sorted by policy, ascending within a
 *           policy (a stable counting sort); the entries behind offsets[num_policies] are set to -1
 *   offsets (num_policies + 1) int64, written: the cumulative counts
 *   dropped int32 scalar, written: the number of rows whose entry lies outside [0, num_policies); they are in no list
 *   workspace: wurm_multi_league_plan_workspace_bytes(num_rows, num_policies) bytes, 8-byte aligned, contents ignored.
 *           Sized from the two numbers alone (a (chunks, num_policies) int32 table of counts, at most 256 chunks, and a
 *           sum per 256 policies); 0 from the query = refused sizes.  Any num_policies: above 256, above num_rows.
 * The launches: counts per (chunk of rows, policy) — integer atomic adds, whose sum does not depend on their order —, a
 * scan over the chunks per policy, a scan over the policies, and the placement of every row by ballot within its wave,
 * the waves of a chunk in order.  No grid-wide barrier, no floating point: the same bits every run.
 * Refused before any HIP call: a null block; negative num_rows, num_policies < 1, a lineup_dtype that is none of the five
 * below and — with num_rows > 0 — null lineup, order, offsets, dropped or workspace, a workspace that is too small or not
 * 8-byte aligned (WURM_ERR_INVALID_ARG); num_rows >= 2^31 (WURM_ERR_UNSUPPORTED).  num_rows = 0 is a successful no-op
 * without a launch (the caller zeroes offsets and dropped).  Otherwise exactly WURM_LEAGUE_PLAN_LAUNCHES launches on
 * `stream`, their grids sized from num_rows and num_policies alone. */
#define WURM_LEAGUE_PLAN_LAUNCHES 4
#define WURM_LINEUP_I64 0
#define WURM_LINEUP_I32 1
#define WURM_LINEUP_I16 2
#define WURM_LINEUP_I8 3
#define WURM_LINEUP_U8 4
typedef struct wurm_league_plan {
    const void *lineup;
    int32_t *order;
    int64_t *offsets;
    int32_t *dropped;
    void *workspace;
    int64_t workspace_bytes, num_rows;
    int num_policies, lineup_dtype;
    void *stream;
} wurm_league_plan;
int64_t wurm_multi_league_plan_workspace_bytes(int64_t num_rows, int num_policies);
int wurm_multi_league_plan(const wurm_league_plan *args);

/* wurm.utils.determine_orientations (wurm/utils.py:36-65) over a (n,3,S,S) batch; out (n) int64. */
int wurm_orientations(const float *envs, int64_t *out, int64_t n, int size, void *stream);

/* ------------------------------------------------------------------------------------------- learner-side glue
 * (the consumers of the env's outputs in experiments/main.py) */

/* Return computation of wurm.rl.A2C.loss (wurm/rl/a2c.py:49-66): reverse scan over time per env.
 *   rewards, values, returns (T,N) fp32 row-major; dones (T,N) bytes; bootstrap (N) fp32.
 *   use_gae = 0: R = bootstrap * !done[T-1]; R_t = r_t + gamma * R_{t+1} * !done_t            (:60-64; values unused)
 *   use_gae = 1: delta_t = r_t + gamma * v_{t+1} * !done_t - v_t; gae_t = delta_t + gamma_lambda * !done_t * gae_{t+1};
 *                R_t = gae_t + v_t, with gamma_lambda = (float)(gamma * gae_lambda)            (:50-59)
 * fp32 in the reference's operation order: bit-identical to its torch-CPU path. */
int wurm_a2c_returns(const float *bootstrap, const float *rewards, const float *values, const uint8_t *dones,
                     float gamma, int use_gae, float gamma_lambda, float *returns, int64_t num_steps, int64_t num_envs,
                     void *stream);

/* Gradient of the scan above: given grad_returns (T,N), writes grad_values (T,N; nullable) and grad_bootstrap (N;
 * nullable) — what torch autograd computes through the reference's op-by-op construction of `returns`. */
int wurm_a2c_returns_backward(const float *grad_returns, const uint8_t *dones, float gamma, int use_gae,
                              float gamma_lambda, float *grad_values, float *grad_bootstrap, int64_t num_steps,
                              int64_t num_envs, void *stream);

/* The per-step logging reductions of experiments/main.py:252-274 in one launch: adds to accum (5 doubles on the
 * device, zeroed by the caller) the batch sums of done, reward, edge_collision, self_collision and snake length
 * (max of the body channel of envs (N,3,S,S)). */
int wurm_single_stats(const float *envs, const float *reward, const uint8_t *done, const uint8_t *self_collision,
                      const uint8_t *edge_collision, double *accum, int64_t num_envs, int size, void *stream);

/* ------------------------------------------------------------------------------------------- fused A2C learner
 * One update of the 2 x 64 feed-forward actor-critic (wurm_amd/agents.py) from the outputs of a policy rollout:
 * batched forward, the return scan of wurm_a2c_returns (n-step, or GAE through the _gae entry points), the loss of experiments/main.py:236-242
 * with A2C(gamma) defaults, its gradient, clip_grad_norm_ and torch.optim.Adam — three launches, no host
 * synchronisation, no atomics (bit-identical from run to run).  Kernels: wurm_amd/csrc/a2c_learner.hpp.
 *   params (P) as pack_policy_params, P = 64 E + 64 + 4096 + 64 + 256 + 4 + 64 + 1;  obs0 (N,E) the input of step 0;
 *   obs (T,N,E) what step t returned (the input of step t + 1; obs[T-1] is the bootstrap input and gets no gradient);
 *   actions (T,N) int64 in 0..3;  rewards (T,N) fp32;  dones (T,N) bytes.
 *   loss = mean l(v - R) - mean((R - v) log p~[a]) - entropy_coef * mean H, l = value_loss_kind, log p~ =
 *   log(clamp(p, eps32, 1 - eps32)), H = - sum_k p_k log p~_k, means over the N T samples, R and R - v constants.
 *   num_inputs: 3 (2n+1)^2 for n <= 6 ('partial_n') or 4 ('positions'); anything else is WURM_ERR_UNSUPPORTED.
 * The PARAMETER NAMES of the wurm_a2c_ff_* prototypes (this section and the next two) are read by the Python loader:
 * wurm_amd/_lib.py keeps them (`fn.argnames`) and the learners place their arguments by them (`_lib.call_named`), so
 * these prototypes are the one statement of the argument order.  The same value has the same name in every prototype;
 * renaming a parameter here renames what the callers must supply. */
#define WURM_A2C_SMOOTH_L1 0 /* F.smooth_l1_loss, beta = 1 */
#define WURM_A2C_MSE 1       /* (v - R)^2 */

/* Bytes of the caller-owned workspace of the two calls below (0 for an unsupported shape): one partial gradient per
 * workgroup (at most 256 of them) and eight parked floats (32 bytes) per row.  The workspace must be 16-byte aligned. */
int64_t wurm_a2c_ff_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs);

/* grad (P): the unclipped gradient;  losses (3): value loss, policy loss, mean entropy;  values_out: nullable, (T,N),
 * the value of every policy input (what the rollout's own `values` are to fp32 rounding). */
int wurm_a2c_ff_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                     const float *rewards, const uint8_t *dones, float gamma, float entropy_coef, int value_loss_kind,
                     float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                     int64_t num_envs, int64_t num_steps, int num_inputs, void *stream);

/* clip_grad_norm_(max_grad_norm) + one torch.optim.Adam step (no weight decay, no amsgrad) in place, `step` counting
 * from 1.  grad is not modified; grad_norm (1, nullable) receives ||grad||_2 before clipping; max_grad_norm <= 0: no
 * clipping.  lr, beta1, beta2 and eps are taken as the shortest decimal that rounds to the float given (0.999f means
 * 0.999), so that 1 - beta2 and the bias corrections are those of torch's double-valued hyper-parameters. */
int wurm_a2c_ff_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                      int64_t step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                      int64_t num_params, void *stream);

/* The double that wurm_a2c_ff_apply / _update compute with for the float hyper-parameter x: the shortest decimal (at
 * most 9 digits) that rounds to x, x itself if there is none or x is not finite.  A caller whose value really is
 * 0.99900001287460327 cannot say so through a float; it gets the arithmetic of 0.999. */
int wurm_a2c_ff_hyper_parameter(float x, double *value);

/* wurm_a2c_ff_grad followed by wurm_a2c_ff_apply in one call: the same kernels, bit-identical results, grad and
 * losses still written. */
int wurm_a2c_ff_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                       const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                       int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                       int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, float *exp_avg,
                       float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1, float beta2, float eps,
                       float max_grad_norm, void *stream);

/* The same two calls with generalised advantage estimation (A2C(gamma, use_gae=True, gae_lambda), wurm/rl/a2c.py:50-59):
 * the same three launches and workspace, the arguments of wurm_a2c_ff_grad / _update followed by
 *   gamma_lambda: (float)(gamma * gae_lambda), the product rounded by the caller as for wurm_a2c_returns; finite and
 *                 >= 0, anything else is WURM_ERR_INVALID_ARG;
 *   returns_out:  nullable, (T,N): R, bit for bit what wurm_a2c_returns(use_gae = 1) makes of values_out and the value of
 *                 obs[T-1].
 *   delta_t = r_t + gamma * v_{t+1} * !done_t - v_t (v_T: the value of obs[T-1]);  gae_t = delta_t + gamma_lambda *
 *   !done_t * gae_{t+1};  R_t = gae_t + v_t.  The loss is the one above with this R; R - v in the policy term is still a
 *   constant, but R in the value term is NOT (the reference does not detach it): with G_t = -l'(v_t - R_t) / (N T) and
 *   A_t = G_t + gamma_lambda * !done_{t-1} * A_{t-1} (the adjoint of wurm_a2c_returns_backward),
 *   dloss/dv_t = l'(v_t - R_t) / (N T) + G_t - A_t + gamma * !done_{t-1} * A_{t-1}.  v_T carries no gradient
 *   (experiments/main.py:233-234 computes it under no_grad).  At gae_lambda = 1 the added term vanishes and R is the
 *   n-step return, to rounding. */
int wurm_a2c_ff_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                         int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                         int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, void *stream,
                         float gamma_lambda, float *returns_out);

int wurm_a2c_ff_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                           int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                           int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs,
                           float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1,
                           float beta2, float eps, float max_grad_norm, void *stream, float gamma_lambda,
                           float *returns_out);

/* ------------------------------------------------------------------------------------------- fused A2C population
 * The calls above for num_members INDEPENDENT agents at once, still three launches: the num_envs envs of the (T,N,.)
 * inputs are num_members members of M = num_envs / num_members consecutive envs, member m learns from the columns
 * [m M, (m + 1) M) only (means over its own M T samples) with row m of params / grad / exp_avg / exp_avg_sq
 * (num_members, P), of losses (num_members, 3) and of grad_norm (num_members).  The grids gain a member dimension; a
 * member's sub-grid has the workgroups, env ranges, tile order and summation order of a stand-alone call with
 * num_envs = M, so every result is bit for bit that call's on contiguous copies of the member's columns.
 *
 * hyper: DEVICE table (num_members, 4) of doubles — lr, gamma, entropy_coef, gamma_lambda of each member — filled on
 * the host by wurm_a2c_ff_pop_hyper and copied to the device once by the caller; nothing about the hyper-parameters is
 * copied or allocated per update.  beta1, beta2, eps, max_grad_norm, value_loss_kind and step are shared.
 * Refused before any HIP call: null pointers, num_members <= 0, num_envs % num_members != 0 (WURM_ERR_INVALID_ARG),
 * more than 65535 members (WURM_ERR_UNSUPPORTED), and whatever the stand-alone call refuses for num_envs = M. */

/* num_members times wurm_a2c_ff_workspace_bytes(num_envs / num_members, ...); 0 for an unsupported shape or a
 * num_envs that num_members does not divide. */
int64_t wurm_a2c_ff_pop_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members);

/* Fills the HOST table (num_members, 4) from host arrays of num_members floats: lr as wurm_a2c_ff_hyper_parameter reads
 * it (the double a stand-alone apply divides by 1 - beta1^step), the others as the floats they are.  gamma_lambda is
 * nullable (n-step returns: zeros); as for wurm_a2c_ff_grad_gae each must be finite and >= 0, and each lr >= 0:
 * anything else is WURM_ERR_INVALID_ARG and the table is not written.  No HIP call. */
int wurm_a2c_ff_pop_hyper(const float *lr, const float *gamma, const float *entropy_coef, const float *gamma_lambda,
                          int64_t num_members, double *table);

int wurm_a2c_ff_pop_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                         float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                         int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream);

int wurm_a2c_ff_pop_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                             const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                             float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                             int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                             float *returns_out);

/* num_params: of ONE member.  Member m's step size is (float)(hyper[m][0] / (1 - beta1^step)), divided in double on the
 * device and rounded once, as wurm_a2c_ff_apply rounds it on the host. */
int wurm_a2c_ff_pop_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                          const double *hyper, int64_t step, float beta1, float beta2, float eps, float max_grad_norm,
                          int64_t num_params, int64_t num_members, void *stream);

int wurm_a2c_ff_pop_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                           float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                           int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                           float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                           float max_grad_norm, void *stream);

int wurm_a2c_ff_pop_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                               const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                               float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                               int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members,
                               float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                               float beta2, float eps, float max_grad_norm, void *stream, float *returns_out);

/* ------------------------------------------------------------------------------------------- fused A2C league
 * The population calls for a LEAGUE: member a learns from an index list of columns of any length instead of a consecutive
 * block of num_envs / num_members.  The (T, R, .) inputs are a MultiSnake window of R = num_rows = num_snakes * num_envs
 * columns k * num_envs + i (obs0 (R, E) the observations it started from), and
 *   order   (R) int32, DEVICE;  offsets (num_members + 1) int64, DEVICE: member a owns the columns
 *           order[offsets[a] .. offsets[a + 1]), M_a of them — what MultiSnake.league_plan makes for wurm_multi_act_league.
 *           Neither is read on the host.
 *   learn   (num_members) bytes, DEVICE, nullable: learn[a] == 0 keeps member a out of this update.
 * Still three launches, sized from R and num_members alone: (min(R, 256), num_members) workgroups for the main kernel.
 * Member a's workgroups form M_a, G_a = min(M_a, 256) and 1 / (M_a T) from `offsets` themselves; those with
 * blockIdx.x >= G_a return at once.  Member a's sub-grid then has the workgroups, ranges (over LIST POSITIONS), tile order
 * and summation order of a stand-alone call with num_envs = M_a, so every result of member a is bit for bit that call's on
 * contiguous copies of its columns taken in list order (means over its own M_a T samples).
 *   A member with learn[a] == 0 or M_a == 0: its rows of params, exp_avg and exp_avg_sq are not touched, its rows of grad
 *   and losses and its grad_norm are written as zeros, and its columns of values_out / returns_out are not written (nor
 *   is any column that no list names): the caller zeroes the two beforehand.  `step` is shared by all members as in the
 *   population, so a member that sat windows out is stepped with the bias corrections of the shared count.
 *   Bounds: the kernels clamp the offsets to [0, R] and make them non-decreasing (a running maximum), and give an entry of
 *   `order` outside [0, R) a row with zero input and zero loss derivative (it still counts in M_a): they read and write in
 *   bounds whatever the two arrays hold.
 *   hyper, beta1, beta2, eps, max_grad_norm, value_loss_kind: as for the population.
 * Refused before any HIP call: null pointers (learn and the optional outputs aside), num_members <= 0, num_rows <= 0, a
 * workspace that is too small or not 16-byte aligned (WURM_ERR_INVALID_ARG); more than 65535 members, num_rows >= 2^31
 * (WURM_ERR_UNSUPPORTED); and whatever the stand-alone call refuses for num_steps, num_inputs and value_loss_kind. */

/* Bytes of the workspace, from host-known bounds: min(num_rows, 256 * num_members) partial gradients (member a's
 * min(M_a, 256) start at group index sum over b < a of min(M_b, 256), which its workgroups and the reduce kernel form from
 * `offsets`), then eight parked floats for each of the num_rows * (num_steps + 1) rows, by list position.  0 for an
 * unsupported shape. */
int64_t wurm_a2c_ff_league_workspace_bytes(int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members);

int wurm_a2c_ff_league_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                            const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                            const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                            float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                            int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream);

int wurm_a2c_ff_league_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                                const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                                float *returns_out);

/* num_params: of ONE member; offsets, learn and num_rows say who steps (the lists themselves are not needed). */
int wurm_a2c_ff_league_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                             const double *hyper, const int64_t *offsets, const uint8_t *learn, int64_t step,
                             float beta1, float beta2, float eps, float max_grad_norm, int64_t num_params,
                             int64_t num_rows, int64_t num_members, void *stream);

int wurm_a2c_ff_league_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                              const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                              const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                              float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                              int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                              float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                              float max_grad_norm, void *stream);

int wurm_a2c_ff_league_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                                  const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                  const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                  float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                  int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members,
                                  float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                                  float beta2, float eps, float max_grad_norm, void *stream, float *returns_out);

/* Population-based training, the exploit / explore step, in two launches on `stream` (kernels: wurm_amd/csrc/a2c_pbt.hpp):
 * no atomics, no grid-wide barrier, nothing read back.
 *   scores  DEVICE (num_members) doubles, only read; a NaN counts as -infinity.  rank(p) = #{q : score_q > score_p or
 *           (score_q == score_p and q < p)}: best first, ties to the lower index.
 *   order   DEVICE (num_members) int32, written: order[rank(p)] = p, the members best to worst.
 *   parent  DEVICE (num_members) int32, written: p itself for a member of rank < num_members - num_replace, which keeps
 *           everything; else src = order[mulhi(w0, num_replace)], one of the best num_replace, with w the Philox4x32-10
 *           block of (seed; env = p, call = generation, purpose 9, sub 0).  Such a member's rows of params, exp_avg and
 *           exp_avg_sq (num_members, num_params) become copies of row src, and its row of hyper becomes
 *             lr           = min(max(hyper[src][0] * (w1 >> 31 ? lr_up : lr_down), lr_lo), lr_hi), a double;
 *             entropy_coef = (double)(float)min(max(hyper[src][2] * (w2 >> 31 ? e_up : e_down), e_lo), e_hi): the
 *                            table holds it as a float;
 *             gamma and gamma_lambda: those of src.
 *   perturb HOST, 8 doubles: lr_down, lr_up, lr_lo, lr_hi, e_down, e_up, e_lo, e_hi; read before the call returns.
 * No row that is read as a source is written by the same call (sources have rank < num_replace, destinations rank >=
 * num_members - num_replace).  num_replace = 0 still writes order and parent = identity.  step is shared and untouched.
 * Refused before any HIP call: a null pointer, num_params <= 0, num_members <= 0, num_replace < 0, 2 num_replace >
 * num_members, generation < 0, a factor that is not finite or <= 0, bounds with lo < 0, lo > hi or a NaN (hi = +infinity
 * is allowed) (WURM_ERR_INVALID_ARG); more than 65535 members (WURM_ERR_UNSUPPORTED). */
int wurm_a2c_ff_pop_exploit(float *params, float *exp_avg, float *exp_avg_sq, double *hyper, const double *scores,
                            int32_t *order, int32_t *parent, int64_t num_params, int64_t num_members,
                            int64_t num_replace, const double *perturb, uint64_t seed, int64_t generation, void *stream);

/* ------------------------------------------------------------------------------------------- rollout statistics
 * The log columns of experiments/main.py:252-316 from the (T,N) outputs of a policy rollout, carried from window to
 * window: two launches, no host synchronisation, no atomics (bit-identical from run to run).  Kernels:
 * wurm_amd/csrc/rollout_stats.hpp.
 *   rewards (T,N) fp32;  dones, edge_collision (T,N) bytes;  self_collision (T,N) bytes, nullable (SimpleGridworld: the
 *   column stays 0);  probs (T,N,4) fp32, 16-byte aligned, nullable (the entropy column stays 0).
 *   Per step and env: episode_return += reward, episode_length += 1; grown = size + (reward == 1) (single_snake.py:268-271);
 *   on done the episode's (return, length, grown) join the episode sums and return and length are cleared; size becomes
 *   initial_size on done and grown otherwise — the length of the snake main.py:273 reads after env.reset(done).
 *   initial_size = 0 says that the env has no snake (SimpleGridworld): nothing grows, every size stays 0.
 *   H = - sum_k p_k log(clamp(p_k, eps32, 1 - eps32)) in fp32, the learner's expression.
 * carry    (3, N) 4-byte words, read and written: row 0 episode_return (fp32), row 1 episode_length (int32), row 2 size
 *          (int32).  The caller seeds size with the current length of every snake (zeros for SimpleGridworld).
 * accum    (num_members, 12) doubles, added to: [0] env steps (T M per call), the sums over steps and envs of [1] done
 *          (= finished episodes), [2] reward, [3] edge_collision, [4] self_collision, [5] size, [6] H, the sums over
 *          finished episodes of [7] return, [8] length, [9] final size (grown), and the maxima over them of [10] return
 *          and [11] final size, folded in with fmax: the caller initialises the two to -infinity.
 * table    nullable, (num_members, T, 6) doubles, written: the batch sums of step t in the order of accum[1..6].
 * smooth   (num_members, 6) doubles, read and written: ExponentialMovingAverageTracker(alpha) (wurm/utils.py:323-337)
 *          over the per-step batch MEANS (the table's rows / M) in step order, in double: a NaN entry is "nothing seen
 *          yet" and takes the first mean; after that s = alpha x + (1 - alpha) s.  The caller initialises it to NaN.
 * num_members > 1: member m owns the envs [m M, (m + 1) M), M = num_envs / num_members, and row m of accum, table and
 * smooth; its numbers are bit for bit those of a stand-alone call on contiguous copies of its M columns.
 * Refused before any HIP call: a null required pointer, num_envs <= 0, num_steps <= 0, num_members <= 0, num_envs %
 * num_members != 0, alpha outside [0, 1], a workspace that is too small or not 16-byte aligned (WURM_ERR_INVALID_ARG);
 * more than 65535 members (WURM_ERR_UNSUPPORTED). */

/* Bytes of the caller-owned workspace (0 for arguments the call refuses): 6 T + 5 doubles per workgroup of 256 envs of a
 * member, and the per-step sums. */
int64_t wurm_rollout_stats_workspace_bytes(int64_t num_envs, int64_t num_steps, int64_t num_members);

int wurm_rollout_stats(const float *rewards, const uint8_t *dones, const uint8_t *edge_collision,
                       const uint8_t *self_collision, const float *probs, void *carry, double *accum, double *smooth,
                       double *table, void *workspace, int64_t workspace_bytes, int64_t num_envs, int64_t num_steps,
                       int64_t num_members, int initial_size, double alpha, void *stream);

/* ---- the multi-agent log columns (wurm_amd/csrc/multi_rollout_stats.hpp) -----------------------------------------------
 * The per-agent columns of experiments/multiagent.py:486-505 (reward_i, policy_entropy_i, food_i, edge_collisions_i,
 * snake_collisions_i, boost_i, size_i, done_i, return_i, their ExponentialMovingAverageTracker versions, episodes) from the
 * (T, K N) outputs of a MultiSnake window (MultiSnake.act_window(..., info=True) or MultiSnake.rollout), carried from
 * window to window: two launches (a scan and a reduce), no host synchronisation, no atomics, no scratch (bit-identical
 * from run to run).  A row is one (snake k, env i) pair, column k N + i, N = num_envs, K = num_snakes.
 *   rewards, food, size (T, K N) fp32 (size is a snake's length: an integer, read as one);  dones, boost,
 *   snake_collision, edge_collision (T, K N) bytes;  probs (T, K N, 4) fp32, 16-byte aligned, nullable (H = 0);
 *   all_done (T, N) bytes, nullable (episodes stays 0).
 *   H = - sum_k p_k log(clamp(p_k, eps32, 1 - eps32)) in fp32, the learner's expression (wurm_rollout_stats above).
 *   With alive = !done, the ten batch sums over the N envs of agent k at step t, in this order: [0] alive, [1] done,
 *   [2] reward alive, [3] H alive, [4] food alive, [5] boost alive, [6] size alive, [7] edge_collision,
 *   [8] snake_collision, [9] size done.  All but [2], [3] and [4] are sums of integers: exact.
 *   Per step and row: life_return += reward, life_length += 1; on every step where done is set the pair joins the agent's
 *   sums over deaths, feeds the maximum of the life return beside the size at death, and is cleared.  A snake that stays
 *   done for several steps counts on each of them, as the reference's size_i[done_i] column does.
 * carry    (2, K N) 4-byte words, read and written: row 0 life_return (fp32), row 1 life_length (int32).  Zeros at first.
 * accum    (K, 16) doubles, added to: [0] env steps (T N per call), [1..10] the ten sums over the window's steps,
 *          [11] the sum of life_return over deaths, [12] of life_length, the maxima of [13] size at death and [14]
 *          life_return over deaths, folded in with fmax (the caller initialises the two to -infinity), [15] episodes =
 *          the sum of all_done over the window, the same number in every agent's row.
 * table    nullable, (K, T, 10) doubles, written: the ten sums of step t.
 * smooth   (K, 9) doubles, read and written: ExponentialMovingAverageTracker(alpha) (wurm/utils.py:323-337) in step
 *          order, in double, over the per-step values reward [2]/[0], policy_entropy [3]/[0], food [4]/[0],
 *          edge_collisions [7]/N, snake_collisions [8]/N, boost [5]/[0], size [6]/[0], done [1]/N, return [9]/[1]: a NaN
 *          entry is "nothing seen yet" and takes the first value; after that s = alpha x + (1 - alpha) s.  The caller
 *          initialises it to NaN.  DEVIATION: a step whose mask is empty ([0] or [1] is 0) gives the reference a NaN mean
 *          that its tracker never recovers from (return_i on the first step without a death); here such a step leaves
 *          that column's smoother as it was.
 * Agent k owns row k of accum, table and smooth; its numbers are bit for bit those of a call with num_snakes = 1 on
 * contiguous copies of its N columns.
 * Refused before any HIP call: a null required pointer, num_envs <= 0, num_snakes <= 0, num_steps <= 0, alpha outside
 * [0, 1], a workspace that is too small or not 16-byte aligned, probs not 16-byte aligned (WURM_ERR_INVALID_ARG); more
 * than 65535 snakes (WURM_ERR_UNSUPPORTED). */

/* Bytes of the caller-owned workspace (0 for arguments the call refuses): 10 T + 5 doubles per wave of 64 envs of an agent
 * (four to a workgroup), and the per-step sums. */
int64_t wurm_multi_rollout_stats_workspace_bytes(int64_t num_envs, int64_t num_snakes, int64_t num_steps);

int wurm_multi_rollout_stats(const float *rewards, const float *food, const float *size, const uint8_t *dones,
                             const uint8_t *boost, const uint8_t *snake_collision, const uint8_t *edge_collision,
                             const float *probs, const uint8_t *all_done, void *carry, double *accum, double *smooth,
                             double *table, void *workspace, int64_t workspace_bytes, int64_t num_envs,
                             int64_t num_snakes, int64_t num_steps, double alpha, void *stream);

/* ---- frames of a fused window, after the fact (wurm_amd/csrc/rollout_frames.hpp) --------------------------------------
 * A window of wurm_single_rollout / wurm_*_policy_rollout* (and the SimpleGridworld forms) is a pure function of an env's
 * start state, its id env_offset + index, seed, the window's first call counter call0 and the SANITISED actions the launch
 * returned.  These entry points re-run it for num_select chosen envs, one wave each, in one launch, and write what
 * `_get_rgb()` shows in front of every step; the window's own kernels are untouched and pay nothing.
 *   start        (num_select, C, S, S) float planes of the chosen envs before the window (C = 3; SimpleGridworld 2), read
 *   select       (num_select) int64 env indices within the object; random draws use env_offset + select[j], never j
 *   actions      (num_steps, num_envs) int64 as the window returned them; column select[j] is read (nullable if num_steps == 0)
 *   frames       (num_steps + 1, num_select, 3, S, S) uint8, written: frame t is the env before step t (after step t - 1
 *                and its reset); frame num_steps is the state the window leaves behind
 *   final_state  (num_select, C, S, S) float planes after the last step and its reset, written
 *   status       (num_select) bytes, written: 0 = replayed; 1 = select[j] is outside [0, num_envs): nothing of that env is
 *                read, its frames and final planes are zeros
 * Refused before any HIP call: a null required pointer, num_select <= 0, num_envs <= 0, num_steps < 0, size < 3
 * (WURM_ERR_INVALID_ARG); size > 64, a size the class cannot reset (<= 8; SimpleGridworld <= 4), a start location off the
 * grid, more than 2^31 - 1 selected envs (WURM_ERR_UNSUPPORTED).  One launch on `stream`. */
int wurm_single_rollout_frames(const float *start, const int64_t *select, const int64_t *actions, uint8_t *frames,
                               float *final_state, uint8_t *status, int64_t num_select, int64_t num_envs, int size,
                               int64_t num_steps, uint64_t seed, uint64_t call0, int64_t env_offset, void *stream);

int wurm_grid_rollout_frames(const float *start, const int64_t *select, const int64_t *actions, uint8_t *frames,
                             float *final_state, uint8_t *status, int64_t num_select, int64_t num_envs, int size,
                             int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0,
                             int64_t env_offset, void *stream);

/* ---- frames of a MultiSnake window, after the fact (wurm_amd/csrc/multi_frames.hpp) ------------------------------------
 * A window of T iterations of step / reset(dones['__all__']) — wurm_multi_rollout, or the per-call launches of
 * MultiSnake.act_window — is for one env a pure function of its start state, its id env_offset + index, seed, the
 * configuration block, the window's first call counter call0 (step t uses call0 + 2 t, its reset call0 + 2 t + 1) and the
 * actions AS GIVEN to the step (it sanitises them itself; the policy's draws come from another counter).  This entry point
 * re-runs it for num_select chosen envs, one wave each, in one launch, with the loop body of wurm_multi_rollout's kernel, and
 * writes what `MultiSnake._get_env_images()` shows in front of every step, bit for bit; the window's own kernels are untouched
 * and pay nothing.
 *   foods .. boost_this_step   the GATHERED state of the chosen envs before the window, read: foods (num_select, 1, S, S),
 *                heads / bodies (num_select K, 1, S, S) float, dones / boost_this_step (num_select K) bytes, orientations
 *                (num_select K) int64, colours (num_select K, 3) int16; env j of them is select[j]'s
 *   select       (num_select) int64 env indices within the object; random draws use env_offset + select[j], never j
 *   actions      (num_steps, K, num_envs) int64, the tape of wurm_multi_rollout or `out['actions']` of act_window (column
 *                k N + i); column select[j] of every snake is read (nullable if num_steps == 0)
 *   frames       (num_steps + 1, num_select, 3, S, S) int16, written: frame t is the env before step t (after step t - 1
 *                and its reset); frame num_steps is the state the window leaves behind
 *   final_*      the state after the last step and its reset, in the layout of the gathered start state, written
 *   status       (num_select) bytes, written: 0 = replayed; 1 = select[j] is outside [0, num_envs): nothing of that env is
 *                read, its frames and final state are zeros
 *   cfg          as wurm_multi_rollout takes it
 * Refused before any HIP call: a null required pointer, a pointer not aligned to its element, num_select <= 0,
 * num_envs <= 0, num_steps < 0, num_snakes < 1, size < 3 (WURM_ERR_INVALID_ARG); more than 64 snakes, size > 64 or < 5, an env
 * whose grids do not fit 160 KB of LDS, more than 2^31 - 1 selected envs (WURM_ERR_UNSUPPORTED): what wurm_multi_rollout
 * serves is served.  num_steps == 0 writes the one frame and the state back.  One launch on `stream`. */
int wurm_multi_rollout_frames(const float *foods, const float *heads, const float *bodies, const uint8_t *dones,
                              const int64_t *orientations, const int16_t *colours, const uint8_t *boost_this_step,
                              const int64_t *select, const int64_t *actions, int16_t *frames, float *final_foods,
                              float *final_heads, float *final_bodies, uint8_t *final_dones, int64_t *final_orientations,
                              int16_t *final_colours, uint8_t *final_boost, uint8_t *status, int64_t num_select,
                              int64_t num_envs, int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg,
                              uint64_t seed, uint64_t call0, int64_t env_offset, void *stream);

/* ---- MultiSnake.policy_window: act, step and reset a whole window in one launch (wurm_amd/csrc/multi_policy_window.hpp) ---
 * num_steps iterations of  a = wurm_multi_act(params, state); step(a); reset(dones['__all__']); state = observation  for
 * every env, with the env on chip for the whole window — what MultiSnake.act_window does with two launches per step, bit
 * for bit.  Step t draws at call0 + 2 t, its reset at call0 + 2 t + 1, the policy at policy_call0 + t from the stream
 * (env_offset + i) K + k of snake k of env i; snake k acts with row k * num_species / num_snakes of params.  Columns /
 * rows are agent-major: k * num_envs + i.  A HOST struct of device pointers. */
typedef struct wurm_multi_policy_window_call {
    float *foods, *heads, *bodies;    /* in/out: the state, as wurm_multi_rollout takes it; after the call the state behind */
    uint8_t *dones;                   /*         the last step AND its reset                                                */
    int64_t *orientations;
    int16_t *colours;
    uint8_t *boost_this_step;
    const uint8_t *pre_done;          /* nullable in (N): wurm_multi_reset(done_env = pre_done, call = pre_call, no
                                         observation) is applied to every env BEFORE step 0 (wurm_multi_call.pre_done)      */
    const float *params;              /* (num_species, num_params) fp32, rows in pack_policy_params order                   */
    const float *obs0;                /* (K, N, E): what the policy acts on at step 0                                       */
    int64_t *actions;                 /* out (T, K N): as sampled (the step sanitises them itself)                          */
    float *probs, *values;            /* out (T, K N, 4), (T, K N)                                                          */
    float *observations;              /* out (T, K N, E): what step t returned, before its reset                            */
    float *rewards;                   /* out (T, K N)                                                                       */
    uint8_t *dones_out;               /* out (T, K N)                                                                       */
    uint8_t *all_done;                /* out (T, N)                                                                         */
    float *food, *sizes;              /* out (T, K N): info['food_k'], info['size_k']                                       */
    uint8_t *boost, *snake_collision, *edge_collision; /* out (T, K N)                                                      */
    int64_t num_envs, num_steps, env_offset, num_params; /* num_params: the row length of params                            */
    uint64_t seed, call0, pre_call, policy_call0;
    int num_snakes, size, obs_n, num_species;
    int waves_per_group;              /* envs per workgroup, 1 .. 4; 0 = chosen by batch size (same results either way)     */
    wurm_multi_config cfg;
} wurm_multi_policy_window_call;

/* Which form serves (num_snakes, size, 'partial_<obs_n>', num_species) at num_envs envs: 0 = none (the call would be
 * refused), 1 = the species' first layers resident in LDS and their heads in registers, 2 = one slot, reloaded whenever
 * the species changes from one snake to the next (more than 4 species, or first layers that do not fit LDS together).
 * No HIP call. */
int wurm_multi_policy_window_plan(int num_snakes, int size, int obs_n, int num_species, int64_t num_envs);

/* Refused before any HIP call: c or a required pointer null (the outputs only when num_steps > 0), a pointer not aligned
 * to its element, num_envs < 0, num_steps < 0, num_snakes < 1, size < 3, num_species outside [1, num_snakes], num_params
 * other than the row length for E = 3 (2 obs_n + 1)^2 inputs, waves_per_group outside [0, 4] (WURM_ERR_INVALID_ARG); more
 * than 64 snakes, size > 64 or < 5, obs_n outside [0, 3], an env whose LDS image does not fit beside one first layer, more
 * than 2^31 - 1 workgroups (WURM_ERR_UNSUPPORTED).  num_envs == 0 or num_steps == 0: WURM_OK, nothing launched, nothing
 * read or written (pre_done is NOT applied).  Otherwise ONE launch on `stream`. */
int wurm_multi_policy_window(const wurm_multi_policy_window_call *c, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WURM_HIP_H */
