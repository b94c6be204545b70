// single_snake.hip — the C-ABI entry points of SingleSnake and SimpleGridworld, and the SingleSnake half of the kernels
// (launch<true>; single_grid.hip holds launch<false>).
#include "single_launch.hpp"
#include "policy_rollout.hpp"

namespace wurm {

thread_local Route last_route = R_GENERIC;
thread_local int last_waves_per_env = 1;
thread_local int last_crop_wave = 0;

template int launch<true>(Kind, StepArgs, void *);
extern template int launch<false>(Kind, StepArgs, void *); // single_grid.hip

static long long obs_elems(bool snake, int mode, int n, int S)
{
    const long long C = (long long)S * S;
    switch (mode) {
    case WURM_OBS_DEFAULT: return 3 * C;
    case WURM_OBS_RAW: return (snake ? 3 : 2) * C;
    case WURM_OBS_ONE_CHANNEL: return snake ? C : 0;
    case WURM_OBS_POSITIONS: return 4;
    case WURM_OBS_PARTIAL: return (snake && n >= 0) ? 3ll * (2 * n + 1) * (2 * n + 1) : 0;
    default: return 0;
    }
}

static int check_common(bool snake, const void *envs, long long N, int S, const void *obs, int mode, int n, int dtype)
{
    if (N < 0 || S < 3 || S > 64) return S > 64 ? WURM_ERR_UNSUPPORTED : WURM_ERR_INVALID_ARG;
    if (N > 0 && envs == nullptr) return WURM_ERR_INVALID_ARG;
    if (dtype != WURM_ACT_I64 && dtype != WURM_ACT_I32) return WURM_ERR_DTYPE;
    if (mode != WURM_OBS_NONE) {
        if (obs_elems(snake, mode, n, S) == 0) return WURM_ERR_INVALID_ARG;
        if (N > 0 && obs == nullptr) return WURM_ERR_INVALID_ARG;
    }
    return WURM_OK;
}

// check_common, then the part of the argument block every entry point and fused_entry share
static int checked_args(bool snake, StepArgs &p, float *envs, float *obs, int obs_mode, int obs_n, long long N, int S,
                        int dtype, u64 seed, u64 call, long long env_offset)
{
    p = {};
    p.envs = envs; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n; p.obs_elems = obs_elems(snake, obs_mode, obs_n, S);
    p.N = N; p.S = S; p.seed = seed; p.call = call; p.env_offset = env_offset;
    return check_common(snake, envs, N, S, obs, obs_mode, obs_n, dtype);
}

// ... and the per-step outputs (SimpleGridworld has no self collision: selfc is null)
static void step_outputs(StepArgs &p, const void *actions, int dtype, float *reward, uint8_t *done, uint8_t *selfc, uint8_t *edgec)
{
    p.actions = const_cast<void *>(actions); p.act_dtype = dtype; p.reward = reward; p.done = done; p.selfc = selfc; p.edgec = edgec;
}

static bool start_ok(int size, int y, int x) { return y >= 0 && x >= 0 && y < size && x < size; } // simple_gridworld.py:254-260

// The validation of the four rollout entry points, in the order their callers see, and their argument block.  WURM_OK with
// num_steps == 0 is "nothing to do"; the _resident forms have nothing to do at num_envs == 0 either, the plain ones leave that to launch.
static int rollout_args(bool snake, StepArgs &p, float *envs, const void *actions, int dtype, float *reward, uint8_t *done,
                        uint8_t *selfc, uint8_t *edgec, float *obs, int obs_mode, int obs_n, long long N, int S, long long T,
                        int start_y, int start_x, u64 seed, u64 call0, long long env_offset)
{
    int rc = checked_args(snake, p, envs, obs, obs_mode, obs_n, N, S, dtype, seed, call0, env_offset);
    if (rc) return rc;
    if (T < 0) return WURM_ERR_INVALID_ARG;
    if (S <= (snake ? 8 : 4)) return WURM_ERR_UNSUPPORTED;
    if (!snake && !start_ok(S, start_y, start_x)) return WURM_ERR_UNSUPPORTED;
    if (N > 0 && T > 0 && (!actions || !reward || !done || !edgec || (snake && !selfc))) return WURM_ERR_INVALID_ARG;
    step_outputs(p, actions, dtype, reward, done, selfc, edgec);
    p.T = T; p.start_y = start_y; p.start_x = start_x;
    return WURM_OK;
}

static int launch_kind(bool snake, Kind kind, const StepArgs &p, void *stream)
{
    return snake ? launch<true>(kind, p, stream) : launch<false>(kind, p, stream);
}

// "This call cannot use the mirror" (and the flush entry points): a lazy valid mirror is written out to envs, by the kernel
// of the family that keeps it.  WURM_ERR_INVALID_ARG: no SingleSnake mirror exists at this size (nothing was launched).
static int write_out_lazy_mirror(bool snake, StepArgs p, void *resident, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    hipError_t err;
    p.resident = resident;
    if (!snake) err = launch_gridworld_lane_flush(p, st);
    else if (p.S == 9) err = launch_lane_resident_flush(p, resident, st);
    else if (p.S == 10 || p.S == 11) err = launch_lane_wide_resident_flush(p, resident, st);
    else if (grid_step_eligible(p)) err = launch_grid_resident_flush(p, st);
    else return WURM_ERR_INVALID_ARG;
    return err == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

// A SimpleGridworld launch on the caller's mirror (gridworld_lane.hip; valid: 0 = build it in this launch, 1 = current).
// *state: 1 = the mirror describes the state, 2 = refused, 0 = the launch failed; left alone if nothing was launched.
// A launch that BUILT the mirror (and wrote the planes whatever `lazy` says) is valid only if it could describe every env:
// one synchronous 4-byte read per build — the first launch of an env object, and the one after something else wrote the
// state — is what lets every other call be a single launch.
static int launch_gridworld_on_mirror(Kind kind, StepArgs p, void *resident, int valid, int lazy, void *stream, int *state)
{
    hipStream_t st = (hipStream_t)stream;
    p.resident = resident;
    p.resident_valid = valid == 1;
    p.resident_lazy = lazy != 0;
    if (!p.resident_valid && hipMemsetAsync(resident, 0, 16, st) != hipSuccess) return WURM_ERR_HIP;
    const int rc = launch<false>(kind, p, stream);
    if (rc != WURM_OK) { *state = 0; return rc; }
    int odd = 0;
    if (!p.resident_valid && (hipMemcpyAsync(&odd, resident, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                              hipStreamSynchronize(st) != hipSuccess))
        return WURM_ERR_HIP;
    *state = odd != 0 ? 2 : 1;
    return WURM_OK;
}

// `go(kernel<CPL>)` for the cells per lane pick_cpl chose (the ladder of launch and of policy_wide.hpp)
#define WURM_CPL_LADDER(cpl, go, kernel) \
    switch (cpl) { \
    case 2: go(kernel<2>); break; \
    case 4: go(kernel<4>); break; \
    case 8: go(kernel<8>); break; \
    case 16: go(kernel<16>); break; \
    case 24: go(kernel<24>); break; \
    case 32: go(kernel<32>); break; \
    case 48: go(kernel<48>); break; \
    default: go(kernel<64>); break; \
    }

// policy_wide.hip: the fused actor beyond policy_rollout.hpp's domain, and the route of the last policy launch
// (members == 0: one set of weights; members >= 1: a population, params (members, num_params), p.N % members == 0)
int launch_policy_wide(const PolicyArgs &p, int obs_mode, int obs_n, void *stream, long long members);
extern thread_local int policy_route;

// the fused actor on policy_rollout.hpp's domain (S <= 11, partial_n with n <= 3); arguments already validated
static int launch_policy_rollout(const PolicyArgs &p, int obs_n, void *stream, long long members)
{
    const int W2 = (2 * obs_n + 1) * (2 * obs_n + 1), EP = (3 * W2 + 3) & ~3;
    const size_t lds = (size_t)(EP + 64) * sizeof(float);
    dim3 grid((unsigned)p.N), block(64);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    const bool s9 = p.S == 9 && !opt.policy_generic; // (debug switch: time / test the generic loop on 9x9 grids)
    auto go = [&](auto s9_kernel, auto kernel) {
        if (s9) WURM_LAUNCH(s9_kernel, grid, block, lds, st, p);
        else WURM_LAUNCH(kernel, grid, block, lds, st, p);
    };
    if (members > 0) {
        PolicyPopArgs pp = {};
        static_cast<PolicyArgs &>(pp) = p;
        pp.M = p.N / members;
        auto go_pop = [&](auto s9_kernel, auto kernel) {
            if (s9) WURM_LAUNCH(s9_kernel, grid, block, lds, st, pp);
            else WURM_LAUNCH(kernel, grid, block, lds, st, pp);
        };
        switch (obs_n) {
        case 0: go_pop(policy_rollout_s9_kernel<0, true>, policy_rollout_kernel<0, true>); break;
        case 1: go_pop(policy_rollout_s9_kernel<1, true>, policy_rollout_kernel<1, true>); break;
        case 2: go_pop(policy_rollout_s9_kernel<2, true>, policy_rollout_kernel<2, true>); break;
        case 3: go_pop(policy_rollout_s9_kernel<3, true>, policy_rollout_kernel<3, true>); break;
        default: return WURM_ERR_UNSUPPORTED;
        }
        return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
    }
    switch (obs_n) {
    case 0: go(policy_rollout_s9_kernel<0>, policy_rollout_kernel<0>); break;
    case 1: go(policy_rollout_s9_kernel<1>, policy_rollout_kernel<1>); break;
    case 2: go(policy_rollout_s9_kernel<2>, policy_rollout_kernel<2>); break;
    case 3: go(policy_rollout_s9_kernel<3>, policy_rollout_kernel<3>); break;
    default: return WURM_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

// wurm_single_policy_rollout (members == 0) and the WURM_OBS_PARTIAL half of wurm_single_policy_rollout_pop
int single_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                          float *values, float *reward, uint8_t *done, uint8_t *self_collision, uint8_t *edge_collision,
                          float *obs, uint8_t *status, int obs_n, int64_t num_envs, int size, int64_t num_steps,
                          uint64_t seed, uint64_t call0, int64_t env_offset, void *stream, long long members)
{
    if (num_envs < 0 || num_steps < 0 || size < 3) return WURM_ERR_INVALID_ARG;
    // the reset draw needs 9 x 9; 64 x 64 is the largest grid; n <= 6 is what the crop machinery covers (CROP_NI)
    if (size <= 8 || size > 64 || obs_n < 0 || obs_n > 6) return WURM_ERR_UNSUPPORTED;
    if (num_envs == 0 || num_steps == 0) return WURM_OK;
    if (!envs || !obs0 || !params || !actions || !probs || !values || !reward || !done || !self_collision ||
        !edge_collision || !obs || !status)
        return WURM_ERR_INVALID_ARG;
    const PolicyArgs p = make_policy_args(envs, obs0, params, actions, probs, values, reward, done, self_collision,
                                          edge_collision, obs, status, num_envs, size, num_steps, seed, call0, env_offset);
    // policy_rollout.hpp's kernels on their domain (WURM_POLICY_WIDE = 1 moves it to policy_wide_kernel), policy_wide.hpp beyond
    if (size > 11 || obs_n > 3 || opt.policy_wide) return launch_policy_wide(p, WURM_OBS_PARTIAL, obs_n, stream, members);
    policy_route = size == 9 && !opt.policy_generic ? 1 : 2;
    return launch_policy_rollout(p, obs_n, stream, members);
}

} // namespace wurm

using namespace wurm;

extern "C" {

const char *wurm_version(void) { return "wurm_hip 0.1 gfx950"; }
const char *wurm_single_last_route(void) { return route_name(last_route); }
int wurm_single_last_crop_wave(void) { return (last_route == R_S9 || last_route == R_S9_INJ) ? last_crop_wave : 0; }
int wurm_single_last_waves_per_env(void) { return (last_route == R_S9 || last_route == R_S9_INJ) ? last_waves_per_env : 1; }

int64_t wurm_single_obs_elems(int obs_mode, int obs_n, int size) { return obs_elems(true, obs_mode, obs_n, size); }
int64_t wurm_grid_obs_elems(int obs_mode, int obs_n, int size) { return obs_elems(false, obs_mode, obs_n, size); }

int wurm_single_step(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                     uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                     int64_t num_envs, int size, uint64_t seed, uint64_t call, int64_t env_offset,
                     const int32_t *inject_food, void *stream)
{
    StepArgs p;
    int rc = checked_args(true, p, envs, obs, obs_mode, obs_n, num_envs, size, actions_dtype, seed, call, env_offset);
    if (rc) return rc;
    if (num_envs > 0 && (!actions || !reward || !done || !self_collision || !edge_collision)) return WURM_ERR_INVALID_ARG;
    step_outputs(p, actions, actions_dtype, reward, done, self_collision, edge_collision);
    p.inject_food = inject_food;
    return launch<true>(K_STEP, p, stream);
}

int wurm_single_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                      int size, uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_reset,
                      void *stream)
{
    StepArgs p;
    int rc = checked_args(true, p, envs, obs, obs_mode, obs_n, num_envs, size, WURM_ACT_I64, seed, call, env_offset);
    if (rc) return rc;
    if (size <= 8) return WURM_ERR_UNSUPPORTED; // single_snake.py:346-347
    if (num_envs > 0 && !done) return WURM_ERR_INVALID_ARG;
    p.done_in = done; p.inject_reset = inject_reset;
    return launch<true>(K_RESET, p, stream);
}

int wurm_single_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                        void *stream)
{
    if (obs_mode == WURM_OBS_NONE) return WURM_ERR_INVALID_ARG;
    StepArgs p;
    int rc = checked_args(true, p, const_cast<float *>(envs), obs, obs_mode, obs_n, num_envs, size, WURM_ACT_I64, 0, 0, 0);
    return rc ? rc : launch<true>(K_OBSERVE, p, stream);
}

int wurm_single_rollout(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                        uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                        int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                        int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream)
{
    StepArgs p;
    int rc = rollout_args(true, p, envs, actions, actions_dtype, reward, done, self_collision, edge_collision, obs, obs_mode,
                          obs_n, num_envs, size, num_steps, 0, 0, seed, call0, env_offset);
    if (rc || num_steps == 0) return rc;
    p.inject_food = inject_food; p.inject_reset = inject_reset;
    return launch<true>(K_ROLLOUT, p, stream);
}

// *mirror_state (nullable): 1 = c->resident describes the state once this call has run, 0 = another path wrote envs (the
// mirror is stale), -1 = nothing was launched
static int fused_entry(bool snake, const wurm_single_call *c, void *stream, int *mirror_state = nullptr)
{
    int unused;
    int &mirror = mirror_state ? *mirror_state : unused;
    mirror = -1;
    if (!c) return WURM_ERR_INVALID_ARG;
    StepArgs p;
    int rc = checked_args(snake, p, c->envs, c->obs, c->obs_mode, c->obs_n, c->num_envs, c->size, c->actions_dtype, c->seed,
                          c->call, c->env_offset);
    if (rc) return rc;
    const int64_t N = c->num_envs;
    if (N > 0 && (!c->actions || !c->reward || !c->done || !c->edge_collision || (snake && !c->self_collision)))
        return WURM_ERR_INVALID_ARG;
    const bool resets = c->pre_done || c->post_reset || c->obs_after;
    if (resets) { // the same limits as wurm_single_reset / wurm_grid_reset
        if (snake && c->size <= 8) return WURM_ERR_UNSUPPORTED;
        if (!snake && (c->size <= 4 || !start_ok(c->size, c->start_y, c->start_x))) return WURM_ERR_UNSUPPORTED;
    }
    // nothing to rebuild and no second observation: the plain step kernel (lighter on registers for large grids)
    const Kind kind = resets ? K_FUSED : K_STEP;
    step_outputs(p, c->actions, c->actions_dtype, c->reward, c->done, c->self_collision, c->edge_collision);
    // check_mask: only the resident 9 x 9 step computes it (below); any other kernel leaves "not computed" for every env
    auto no_mask = [&]() -> int {
        if (c->check_mask == nullptr || N == 0) return WURM_OK;
        return hipMemsetAsync(c->check_mask, 0xFF, (size_t)N * 4, (hipStream_t)stream) == hipSuccess ? WURM_OK : WURM_ERR_HIP;
    };
    p.start_y = c->start_y; p.start_x = c->start_x;
    p.inject_food = c->inject_food; p.inject_reset = c->inject_reset; p.done_in = c->pre_done;
    p.obs_after = c->obs_after; p.done_copy = c->done_copy; p.inject_pre_reset = c->inject_pre_reset;
    p.pre_call = c->pre_call; p.post_reset = c->post_reset;
    const bool mirrored = c->resident != nullptr && N > 0;
    if (snake && mirrored) {
        p.lds_per_wave = ((p.S * p.S + 15) / 16) * 16;
        if (lane_resident_eligible(p)) {
            // the caller keeps a compact mirror of the state: the step reads that instead of envs (lane_resident.hpp)
            if (launch_lane_resident(p, c->resident, c->resident_valid != 0, c->resident_lazy != 0, c->check_mask,
                                     (hipStream_t)stream) != hipSuccess)
                return WURM_ERR_HIP;
            last_route = R_LANE_RESIDENT;
            mirror = 1;
            return WURM_OK;
        }
        if (lane_wide_resident_eligible(p) && c->resident_lazy) {
            // 10 x 10 / 11 x 11: the same on lane_wide.hpp's state (lane_wide_resident.hpp), lazy form only — a caller that
            // wants envs written every call gets the kernels without a mirror below, and the mirror reported stale
            if (launch_lane_wide_resident(p, c->resident, c->resident_valid != 0, c->check_mask, (hipStream_t)stream) != hipSuccess)
                return WURM_ERR_HIP;
            last_route = R_LANE_WIDE_RESIDENT;
            mirror = 1;
            return WURM_OK;
        }
        if (no_mask() != WURM_OK) return WURM_ERR_HIP;
        if (grid_resident_eligible(p)) {
            // 12 x 12 and larger: the LDS clock-grid step keeps its grids in the mirror (grid_rollout.hip)
            p.resident = c->resident;
            p.resident_valid = c->resident_valid != 0;
            p.resident_lazy = c->resident_lazy != 0;
            rc = launch<true>(kind, p, stream);
            mirror = rc == WURM_OK ? 1 : 0;
            return rc;
        }
        // this call cannot use the mirror: a lazy one is written out to envs before the ordinary kernels read them
        if (c->resident_lazy && c->resident_valid && write_out_lazy_mirror(true, p, c->resident, stream) == WURM_ERR_HIP)
            return WURM_ERR_HIP;
    }
    if (!snake && mirrored) {
        // SimpleGridworld's mirror (gridworld_lane.hip): one record per env.  resident_valid: 0 = build it in this launch,
        // 1 = current, 2 = refused (the launch that built it found envs outside the lane kernel's domain: the planes stay
        // the state until the caller clears resident_valid again).
        if (no_mask() != WURM_OK) return WURM_ERR_HIP;
        if (c->resident_valid != 2 && gridworld_lane_step_eligible(p))
            return launch_gridworld_on_mirror(kind, p, c->resident, c->resident_valid, c->resident_lazy, stream, &mirror);
        // this call cannot use the mirror: a lazy one is written out to envs before the ordinary kernels read them
        if (c->resident_lazy && c->resident_valid == 1 && write_out_lazy_mirror(false, p, c->resident, stream) != WURM_OK)
            return WURM_ERR_HIP;
        mirror = c->resident_valid == 2 ? 2 : 0;
        return launch<false>(kind, p, stream);
    }
    if (!mirrored && no_mask() != WURM_OK) return WURM_ERR_HIP;
    mirror = 0;
    return launch_kind(snake, kind, p, stream);
}

int wurm_single_resident_flush(const wurm_single_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (!c->resident || !c->resident_lazy || !c->resident_valid || c->num_envs <= 0) return WURM_OK;
    if (!c->envs) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = c->envs; p.N = c->num_envs; p.S = c->size;
    return write_out_lazy_mirror(true, p, c->resident, stream);
}

int64_t wurm_single_resident_size(int64_t num_envs, int size, int obs_mode, int obs_n)
{
    if (num_envs <= 0) return 0;
    if (lane_resident_shape(size, obs_mode, obs_n)) return num_envs * 32; // 9 x 9: 32 bytes per env (lane_resident.hpp)
    if (lane_wide_resident_shape(size, obs_mode, obs_n)) return num_envs * 48; // 10 x 10 / 11 x 11: 48 (lane_wide_resident.hpp)
    StepArgs p = {};
    p.S = size;
    if (grid_step_eligible(p) && obs_elems(true, obs_mode, obs_n, size) >= 0) // 12 x 12 and larger: grid + record per env
        return grid_resident_bytes(num_envs, size);
    return 0;
}

int64_t wurm_single_resident_bytes(int64_t num_envs, int size, int obs_mode, int obs_n)
{
    if (num_envs <= 0) return 0;
    const long long e = opt.resident_min_envs; // -1: by shape
    const bool big = e >= 0 ? num_envs >= e
                            : ((lane_resident_shape(size, obs_mode, obs_n) || lane_wide_resident_shape(size, obs_mode, obs_n)) ? num_envs >= 4096
                                                                          : num_envs * (long long)size * size >= (1ll << 20));
    return big ? wurm_single_resident_size(num_envs, size, obs_mode, obs_n) : 0;
}

int64_t wurm_grid_resident_size(int64_t num_envs, int size, int obs_mode)
{
    if (num_envs <= 0 || size < 5 || size > 64) return 0;
    if (!(obs_mode == WURM_OBS_DEFAULT || obs_mode == WURM_OBS_RAW || obs_mode == WURM_OBS_POSITIONS || obs_mode == WURM_OBS_NONE)) return 0;
    return gridworld_resident_bytes(num_envs, size, obs_mode, obs_elems(false, obs_mode, 0, size));
}

int64_t wurm_grid_resident_bytes(int64_t num_envs, int size, int obs_mode)
{
    const long long e = opt.resident_min_envs; // -1: where the per-call lane kernel takes over
    return num_envs >= (e >= 0 ? e : opt.lane_step_min_envs) ? wurm_grid_resident_size(num_envs, size, obs_mode) : 0;
}

int wurm_grid_resident_flush(const wurm_single_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (!c->resident || !c->resident_lazy || c->resident_valid != 1 || c->num_envs <= 0) return WURM_OK;
    if (!c->envs) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = c->envs; p.N = c->num_envs; p.S = c->size;
    return write_out_lazy_mirror(false, p, c->resident, stream);
}

int wurm_single_step_reset(const wurm_single_call *c, void *stream) { return fused_entry(true, c, stream); }

int wurm_grid_step_reset(const wurm_single_call *c, void *stream)
{
    int mirror = -1;
    const int rc = fused_entry(false, c, stream, &mirror);
    // (the block is const here: a caller that keeps the mirror learns of a refusal from the return value)
    return (rc == WURM_OK && c && c->resident && c->resident_valid == 0 && mirror == 2) ? WURM_MIRROR_REFUSED : rc;
}

static int step_slot(bool snake, wurm_single_call *c, const wurm_single_slabs *s, int64_t slot, void *actions,
                     int actions_dtype, uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after,
                     void *stream)
{
    if (!c || !s || slot < 0 || slot >= s->steps) return WURM_ERR_INVALID_ARG;
    const int64_t N = c->num_envs, elems = obs_elems(snake, c->obs_mode, c->obs_n, c->size);
    c->actions = actions;
    c->actions_dtype = actions_dtype;
    c->call = call;
    c->obs = s->obs ? s->obs + slot * N * elems : nullptr;
    c->obs_after = (want_obs_after && s->obs_after) ? s->obs_after + slot * N * elems : nullptr;
    c->reward = s->reward + slot * N;
    c->done = s->flags + slot * N;
    c->self_collision = s->flags + (s->steps + slot) * N;
    c->edge_collision = s->flags + (2 * s->steps + slot) * N;
    if (apply_pending) {
        if (!c->done_copy) return WURM_ERR_INVALID_ARG;
        c->pre_done = c->done_copy;
        c->pre_call = pre_call;
    } else {
        c->pre_done = nullptr;
    }
    int mirror = -1;
    const int rc = fused_entry(snake, c, stream, &mirror);
    if (c->resident && mirror >= 0) c->resident_valid = rc != WURM_OK ? 0 : mirror; // (2: SimpleGridworld's mirror refused)
    return rc;
}

int wurm_single_step_slot(wurm_single_call *c, const wurm_single_slabs *s, int64_t slot, void *actions,
                          int actions_dtype, uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after,
                          void *stream)
{
    return step_slot(true, c, s, slot, actions, actions_dtype, call, apply_pending, pre_call, want_obs_after, stream);
}

int wurm_grid_step_slot(wurm_single_call *c, const wurm_single_slabs *s, int64_t slot, void *actions,
                        int actions_dtype, uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after,
                        void *stream)
{
    return step_slot(false, c, s, slot, actions, actions_dtype, call, apply_pending, pre_call, want_obs_after, stream);
}

int wurm_single_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                               float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                               uint8_t *edge_collision, float *obs, uint8_t *status, int obs_n, int64_t num_envs,
                               int size, int64_t num_steps, uint64_t seed, uint64_t call0, int64_t env_offset,
                               void *stream)
{
    return single_policy_rollout(envs, obs0, params, actions, probs, values, reward, done, self_collision, edge_collision,
                                 obs, status, obs_n, num_envs, size, num_steps, seed, call0, env_offset, stream, 0);
}

int wurm_single_check(const float *envs, uint32_t *err, int64_t num_envs, int size, void *stream)
{
    if (num_envs < 0 || size < 3) return WURM_ERR_INVALID_ARG;
    if (num_envs == 0) return WURM_OK;
    if (!envs || !err) return WURM_ERR_INVALID_ARG;
    const int cpl = pick_cpl(size);
    if (cpl < 0) return WURM_ERR_UNSUPPORTED;
    const int wpb = 4;
    dim3 block(64 * wpb), grid((unsigned)((num_envs + wpb - 1) / wpb));
    hipStream_t st = (hipStream_t)stream;
    long long N = num_envs;
    (void)hipGetLastError();
    auto go = [&](auto kernel) { WURM_LAUNCH(kernel, grid, block, 0, st, envs, err, N, size); };
    WURM_CPL_LADDER(cpl, go, check_kernel);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_orientations(const float *envs, int64_t *out, int64_t n, int size, void *stream)
{
    if (n < 0 || size < 3) return WURM_ERR_INVALID_ARG;
    if (n == 0) return WURM_OK;
    if (!envs || !out) return WURM_ERR_INVALID_ARG;
    const int cpl = pick_cpl(size);
    if (cpl < 0) return WURM_ERR_UNSUPPORTED;
    const int wpb = 4, lpw = ((size * size + 15) / 16) * 16;
    dim3 block(64 * wpb), grid((unsigned)((n + wpb - 1) / wpb));
    hipStream_t st = (hipStream_t)stream;
    long long N = n;
    long long *o = (long long *)out;
    size_t lds = (size_t)lpw * wpb;
    (void)hipGetLastError();
    auto go = [&](auto kernel) { WURM_LAUNCH(kernel, grid, block, lds, st, envs, o, N, size, lpw); };
    WURM_CPL_LADDER(cpl, go, orientations_kernel);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

/* ---------------------------------------------------------------------------------------- SimpleGridworld */

int wurm_grid_step(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                   uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                   uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_food, void *stream)
{
    StepArgs p;
    int rc = checked_args(false, p, envs, obs, obs_mode, obs_n, num_envs, size, actions_dtype, seed, call, env_offset);
    if (rc) return rc;
    if (num_envs > 0 && (!actions || !reward || !done || !edge_collision)) return WURM_ERR_INVALID_ARG;
    step_outputs(p, actions, actions_dtype, reward, done, nullptr, edge_collision);
    p.inject_food = inject_food;
    return launch<false>(K_STEP, p, stream);
}

int wurm_grid_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                    int size, int start_y, int start_x, uint64_t seed, uint64_t call, int64_t env_offset,
                    const int32_t *inject_reset, void *stream)
{
    StepArgs p;
    int rc = checked_args(false, p, envs, obs, obs_mode, obs_n, num_envs, size, WURM_ACT_I64, seed, call, env_offset);
    if (rc) return rc;
    if (size <= 4) return WURM_ERR_UNSUPPORTED; // simple_gridworld.py:249-250
    if (!start_ok(size, start_y, start_x)) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && !done) return WURM_ERR_INVALID_ARG;
    p.done_in = done; p.start_y = start_y; p.start_x = start_x; p.inject_reset = inject_reset;
    return launch<false>(K_RESET, p, stream);
}

int wurm_grid_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      void *stream)
{
    if (obs_mode == WURM_OBS_NONE) return WURM_ERR_INVALID_ARG;
    StepArgs p;
    int rc = checked_args(false, p, const_cast<float *>(envs), obs, obs_mode, obs_n, num_envs, size, WURM_ACT_I64, 0, 0, 0);
    return rc ? rc : launch<false>(K_OBSERVE, p, stream);
}

int wurm_grid_rollout(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                      uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0,
                      int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream)
{
    StepArgs p;
    int rc = rollout_args(false, p, envs, actions, actions_dtype, reward, done, nullptr, edge_collision, obs, obs_mode, obs_n,
                          num_envs, size, num_steps, start_y, start_x, seed, call0, env_offset);
    if (rc || num_steps == 0) return rc;
    p.inject_food = inject_food; p.inject_reset = inject_reset;
    return launch<false>(K_ROLLOUT, p, stream);
}

/* wurm_single_rollout (RNG mode) for a caller that keeps the mirror of wurm_single_call.resident: grids of 12 x 12 and larger
 * roll out on the clock grids and records of the per-call step (grid_rollout.hip) — an env its record describes is read from
 * the mirror (2 bytes per cell instead of 12) and written back there, the planes only while the mirror is not lazy; the
 * mirror describes the final state afterwards (*resident_valid = 1).  9 x 9 (another mirror format, a launch that costs 11 us
 * besides its steps) and every other case run wurm_single_rollout on the planes after writing a lazy valid mirror out;
 * *resident_valid is then 0. */
int wurm_single_rollout_resident(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                                 uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                                 int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                 int64_t env_offset, void *resident, int *resident_valid, int resident_lazy, void *stream)
{
    if (!resident || !resident_valid)
        return wurm_single_rollout(envs, actions, actions_dtype, reward, done, self_collision, edge_collision, obs, obs_mode, obs_n,
                                   num_envs, size, num_steps, seed, call0, env_offset, nullptr, nullptr, stream);
    StepArgs p;
    int rc = rollout_args(true, p, envs, actions, actions_dtype, reward, done, self_collision, edge_collision, obs, obs_mode,
                          obs_n, num_envs, size, num_steps, 0, 0, seed, call0, env_offset);
    if (rc || num_steps == 0 || num_envs == 0) return rc;
    if (grid_rollout_eligible(p) && grid_resident_eligible(p)) {
        p.resident = resident;
        p.resident_valid = *resident_valid != 0;
        p.resident_lazy = resident_lazy != 0;
        rc = launch<true>(K_ROLLOUT, p, stream);
        *resident_valid = rc == WURM_OK ? 1 : 0;
        return rc;
    }
    if (resident_lazy && *resident_valid && write_out_lazy_mirror(true, p, resident, stream) == WURM_ERR_HIP) return WURM_ERR_HIP;
    *resident_valid = 0;
    return launch<true>(K_ROLLOUT, p, stream);
}

/* wurm_grid_rollout (RNG mode) for a caller that keeps SimpleGridworld's mirror (wurm_grid_resident_bytes; meaning of
 * *resident_valid / resident_lazy as in wurm_single_call): where the lane kernel serves the launch the state is read from the
 * records when *resident_valid == 1 — no scan of the planes, no flag pass behind the launch — and the records describe the final
 * state afterwards; the planes are written unless the mirror is lazy and was current.  A launch that builds the mirror reads
 * its verdict back (one stream synchronisation): *resident_valid = 1, or 2 = refused.  Any other launch (a batch or
 * observation the lane kernel does not serve, a refused mirror) runs wurm_grid_rollout on the planes, after writing a lazy
 * valid mirror out; *resident_valid is then 0 (2 stays 2). */
int wurm_grid_rollout_resident(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                               uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                               int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0, int64_t env_offset,
                               void *resident, int *resident_valid, int resident_lazy, void *stream)
{
    if (!resident || !resident_valid)
        return wurm_grid_rollout(envs, actions, actions_dtype, reward, done, edge_collision, obs, obs_mode, obs_n, num_envs, size,
                                 num_steps, start_y, start_x, seed, call0, env_offset, nullptr, nullptr, stream);
    StepArgs p;
    int rc = rollout_args(false, p, envs, actions, actions_dtype, reward, done, nullptr, edge_collision, obs, obs_mode, obs_n,
                          num_envs, size, num_steps, start_y, start_x, seed, call0, env_offset);
    if (rc || num_steps == 0 || num_envs == 0) return rc;
    if (*resident_valid != 2 && gridworld_lane_eligible(p)) // (a launch that builds the mirror reads its verdict: see fused_entry)
        return launch_gridworld_on_mirror(K_ROLLOUT, p, resident, *resident_valid, resident_lazy, stream, resident_valid);
    if (resident_lazy && *resident_valid == 1 && write_out_lazy_mirror(false, p, resident, stream) != WURM_OK) return WURM_ERR_HIP;
    if (*resident_valid != 2) *resident_valid = 0;
    return launch<false>(K_ROLLOUT, p, stream);
}

} // extern "C"
