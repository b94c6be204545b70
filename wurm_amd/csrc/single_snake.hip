// single_snake.hip — the C-ABI entry points of SingleSnake and SimpleGridworld, and the SingleSnake half of the kernels
// (launch<true>; single_grid.hip holds launch<false>).
#include "single_launch.hpp"
#include "policy_rollout.hpp"

namespace wurm {

thread_local Route last_route = R_GENERIC;

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

// policy_wide.hip: the fused actor beyond policy_rollout.hpp's domain, and the route of the last policy launch
int launch_policy_wide(const PolicyArgs &p, int obs_mode, int obs_n, void *stream);
extern thread_local int policy_route;

// the fused actor on policy_rollout.hpp's domain (S <= 11, partial_n with n <= 3); arguments already validated
static int launch_policy_rollout(const PolicyArgs &p, int obs_n, void *stream)
{
    const int W2 = (2 * obs_n + 1) * (2 * obs_n + 1), EP = (3 * W2 + 3) & ~3;
    const size_t lds = (size_t)(EP + 64) * sizeof(float);
    dim3 grid((unsigned)p.N), block(64);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    const bool s9 = p.S == 9 && !opt.policy_generic; // (debug switch: time / test the generic loop on 9x9 grids)
    switch (obs_n) {
    case 0:
        if (s9) WURM_LAUNCH(policy_rollout_s9_kernel<0>, grid, block, lds, st, p);
        else WURM_LAUNCH(policy_rollout_kernel<0>, grid, block, lds, st, p);
        break;
    case 1:
        if (s9) WURM_LAUNCH(policy_rollout_s9_kernel<1>, grid, block, lds, st, p);
        else WURM_LAUNCH(policy_rollout_kernel<1>, grid, block, lds, st, p);
        break;
    case 2:
        if (s9) WURM_LAUNCH(policy_rollout_s9_kernel<2>, grid, block, lds, st, p);
        else WURM_LAUNCH(policy_rollout_kernel<2>, grid, block, lds, st, p);
        break;
    case 3:
        if (s9) WURM_LAUNCH(policy_rollout_s9_kernel<3>, grid, block, lds, st, p);
        else WURM_LAUNCH(policy_rollout_kernel<3>, grid, block, lds, st, p);
        break;
    default: return WURM_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace wurm

using namespace wurm;

extern "C" {

const char *wurm_version(void) { return "wurm_hip 0.1 gfx950"; }
const char *wurm_single_last_route(void) { return route_name(last_route); }

int64_t wurm_single_obs_elems(int obs_mode, int obs_n, int size) { return obs_elems(true, obs_mode, obs_n, size); }
int64_t wurm_grid_obs_elems(int obs_mode, int obs_n, int size) { return obs_elems(false, obs_mode, obs_n, size); }

int wurm_single_step(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                     uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                     int64_t num_envs, int size, uint64_t seed, uint64_t call, int64_t env_offset,
                     const int32_t *inject_food, void *stream)
{
    int rc = check_common(true, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_envs > 0 && (!actions || !reward || !done || !self_collision || !edge_collision)) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = envs; p.actions = actions; p.act_dtype = actions_dtype; p.reward = reward; p.done = done;
    p.selfc = self_collision; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(true, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.seed = seed; p.call = call;
    p.env_offset = env_offset; p.inject_food = inject_food;
    return launch<true>(K_STEP, p, stream);
}

int wurm_single_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                      int size, uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_reset,
                      void *stream)
{
    int rc = check_common(true, envs, num_envs, size, obs, obs_mode, obs_n, WURM_ACT_I64);
    if (rc) return rc;
    if (size <= 8) return WURM_ERR_UNSUPPORTED; // single_snake.py:346-347
    if (num_envs > 0 && !done) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = envs; p.done_in = done; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(true, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.seed = seed; p.call = call;
    p.env_offset = env_offset; p.inject_reset = inject_reset;
    return launch<true>(K_RESET, p, stream);
}

int wurm_single_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                        void *stream)
{
    if (obs_mode == WURM_OBS_NONE) return WURM_ERR_INVALID_ARG;
    int rc = check_common(true, envs, num_envs, size, obs, obs_mode, obs_n, WURM_ACT_I64);
    if (rc) return rc;
    StepArgs p = {};
    p.envs = const_cast<float *>(envs); p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(true, obs_mode, obs_n, size); p.N = num_envs; p.S = size;
    return launch<true>(K_OBSERVE, p, stream);
}

int wurm_single_rollout(float *envs, void *actions, int actions_dtype, float *reward, uint8_t *done,
                        uint8_t *self_collision, uint8_t *edge_collision, float *obs, int obs_mode, int obs_n,
                        int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                        int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream)
{
    int rc = check_common(true, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_steps < 0) return WURM_ERR_INVALID_ARG;
    if (size <= 8) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && num_steps > 0 && (!actions || !reward || !done || !self_collision || !edge_collision))
        return WURM_ERR_INVALID_ARG;
    if (num_steps == 0) return WURM_OK;
    StepArgs p = {};
    p.envs = envs; p.actions = actions; p.act_dtype = actions_dtype; p.reward = reward; p.done = done;
    p.selfc = self_collision; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(true, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.T = num_steps; p.seed = seed;
    p.call = call0; p.env_offset = env_offset; p.inject_food = inject_food; p.inject_reset = inject_reset;
    return launch<true>(K_ROLLOUT, p, stream);
}

// *mirror_state (nullable): 1 = c->resident describes the state once this call has run, 0 = another path wrote envs (the
// mirror is stale), -1 = nothing was launched
static int fused_entry(bool snake, const wurm_single_call *c, void *stream, int *mirror_state = nullptr)
{
    if (mirror_state) *mirror_state = -1;
    if (!c) return WURM_ERR_INVALID_ARG;
    int rc = check_common(snake, c->envs, c->num_envs, c->size, c->obs, c->obs_mode, c->obs_n, c->actions_dtype);
    if (rc) return rc;
    const int64_t N = c->num_envs;
    if (N > 0 && (!c->actions || !c->reward || !c->done || !c->edge_collision || (snake && !c->self_collision)))
        return WURM_ERR_INVALID_ARG;
    const bool resets = c->pre_done || c->post_reset || c->obs_after;
    if (resets) { // the same limits as wurm_single_reset / wurm_grid_reset
        if (snake && c->size <= 8) return WURM_ERR_UNSUPPORTED;
        if (!snake && (c->size <= 4 || c->start_y < 0 || c->start_x < 0 || c->start_y >= c->size || c->start_x >= c->size))
            return WURM_ERR_UNSUPPORTED;
    }
    StepArgs p = {};
    p.envs = c->envs; p.actions = c->actions; p.act_dtype = c->actions_dtype; p.reward = c->reward; p.done = c->done;
    p.selfc = c->self_collision; p.edgec = c->edge_collision; p.obs = c->obs; p.obs_mode = c->obs_mode;
    p.obs_n = c->obs_n; p.obs_elems = obs_elems(snake, c->obs_mode, c->obs_n, c->size); p.N = N; p.S = c->size;
    // check_mask: only the resident 9 x 9 step computes it (below); any other kernel leaves "not computed" for every env
    auto no_mask = [&]() -> int {
        if (c->check_mask == nullptr || N == 0) return WURM_OK;
        return hipMemsetAsync(c->check_mask, 0xFF, (size_t)N * 4, (hipStream_t)stream) == hipSuccess ? WURM_OK : WURM_ERR_HIP;
    };
    p.start_y = c->start_y; p.start_x = c->start_x; p.seed = c->seed; p.call = c->call; p.env_offset = c->env_offset;
    p.inject_food = c->inject_food; p.inject_reset = c->inject_reset; p.done_in = c->pre_done;
    p.obs_after = c->obs_after; p.done_copy = c->done_copy; p.inject_pre_reset = c->inject_pre_reset;
    p.pre_call = c->pre_call; p.post_reset = c->post_reset;
    if (snake && c->resident != nullptr && N > 0) {
        p.lds_per_wave = ((p.S * p.S + 15) / 16) * 16;
        if (lane_resident_eligible(p)) {
            // the caller keeps a compact mirror of the state: the step reads that instead of envs (lane_resident.hpp)
            if (launch_lane_resident(p, c->resident, c->resident_valid != 0, c->resident_lazy != 0, c->check_mask,
                                     (hipStream_t)stream) != hipSuccess)
                return WURM_ERR_HIP;
            last_route = R_LANE_RESIDENT;
            if (mirror_state) *mirror_state = 1;
            return WURM_OK;
        }
        if (lane_wide_resident_eligible(p) && c->resident_lazy) {
            // 10 x 10 / 11 x 11: the same on lane_wide.hpp's state (lane_wide_resident.hpp), lazy form only — a caller that
            // wants envs written every call gets the kernels without a mirror below, and the mirror reported stale
            if (launch_lane_wide_resident(p, c->resident, c->resident_valid != 0, c->check_mask, (hipStream_t)stream) != hipSuccess)
                return WURM_ERR_HIP;
            last_route = R_LANE_WIDE_RESIDENT;
            if (mirror_state) *mirror_state = 1;
            return WURM_OK;
        }
        if (no_mask() != WURM_OK) return WURM_ERR_HIP;
        if (grid_resident_eligible(p)) {
            // 12 x 12 and larger: the LDS clock-grid step keeps its grids in the mirror (grid_rollout.hip)
            p.resident = c->resident;
            p.resident_valid = c->resident_valid != 0;
            p.resident_lazy = c->resident_lazy != 0;
            rc = launch<true>(resets ? K_FUSED : K_STEP, p, stream);
            if (mirror_state) *mirror_state = rc == WURM_OK ? 1 : 0;
            return rc;
        }
        // this call cannot use the mirror: a lazy one is written out to envs before the ordinary kernels read them
        if (c->resident_lazy && c->resident_valid) {
            hipError_t err = hipSuccess;
            if (p.S == 9) err = launch_lane_resident_flush(p, c->resident, (hipStream_t)stream);
            else if (p.S == 10 || p.S == 11) err = launch_lane_wide_resident_flush(p, c->resident, (hipStream_t)stream);
            else if (grid_step_eligible(p)) { StepArgs q = p; q.resident = c->resident; err = launch_grid_resident_flush(q, (hipStream_t)stream); }
            if (err != hipSuccess) return WURM_ERR_HIP;
        }
    }
    if (!snake && c->resident != nullptr && N > 0) {
        // SimpleGridworld's mirror (gridworld_lane.hip): one record per env.  resident_valid: 0 = build it in this launch,
        // 1 = current, 2 = refused (the launch that built it found envs outside the lane kernel's domain: the planes stay
        // the state until the caller clears resident_valid again).
        if (no_mask() != WURM_OK) return WURM_ERR_HIP;
        if (c->resident_valid != 2 && gridworld_lane_step_eligible(p)) {
            p.resident = c->resident;
            p.resident_valid = c->resident_valid == 1;
            p.resident_lazy = c->resident_lazy != 0;
            if (!p.resident_valid && hipMemsetAsync(c->resident, 0, 16, (hipStream_t)stream) != hipSuccess) return WURM_ERR_HIP;
            rc = launch<false>(resets ? K_FUSED : K_STEP, p, stream);
            if (rc != WURM_OK) { if (mirror_state) *mirror_state = 0; return rc; }
            int state = 1;
            if (!p.resident_valid) {
                // the launch built the mirror (and wrote the planes whatever `lazy` says): valid only if it could describe every
                // env.  One synchronous 4-byte read per BUILD — the first step of an env object, and the step after something
                // else wrote the state — is what lets every other call be a single launch
                int odd = 0;
                if (hipMemcpyAsync(&odd, c->resident, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
                    hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
                    return WURM_ERR_HIP;
                if (odd != 0) state = 2;
            }
            if (mirror_state) *mirror_state = state;
            return WURM_OK;
        }
        // this call cannot use the mirror: a lazy one is written out to envs before the ordinary kernels read them
        if (c->resident_lazy && c->resident_valid == 1) {
            StepArgs q = p;
            q.resident = c->resident;
            if (launch_gridworld_lane_flush(q, (hipStream_t)stream) != hipSuccess) return WURM_ERR_HIP;
        }
        if (mirror_state) *mirror_state = c->resident_valid == 2 ? 2 : 0;
        const Kind kind_g = resets ? K_FUSED : K_STEP;
        return launch<false>(kind_g, p, stream);
    }
    if (!(snake && c->resident != nullptr && N > 0) && no_mask() != WURM_OK) return WURM_ERR_HIP;
    if (mirror_state) *mirror_state = 0;
    // nothing to rebuild and no second observation: the plain step kernel (lighter on registers for large grids)
    const Kind kind = resets ? K_FUSED : K_STEP;
    return snake ? launch<true>(kind, p, stream) : launch<false>(kind, p, stream);
}

int wurm_single_resident_flush(const wurm_single_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (!c->resident || !c->resident_lazy || !c->resident_valid || c->num_envs <= 0) return WURM_OK;
    if (!c->envs) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = c->envs; p.N = c->num_envs; p.S = c->size; p.resident = c->resident;
    hipError_t err;
    if (c->size == 9) err = launch_lane_resident_flush(p, c->resident, (hipStream_t)stream);
    else if (c->size == 10 || c->size == 11) err = launch_lane_wide_resident_flush(p, c->resident, (hipStream_t)stream);
    else if (grid_step_eligible(p)) err = launch_grid_resident_flush(p, (hipStream_t)stream);
    else return WURM_ERR_INVALID_ARG;
    return err == hipSuccess ? WURM_OK : WURM_ERR_HIP;
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
    p.envs = c->envs; p.N = c->num_envs; p.S = c->size; p.resident = c->resident;
    return launch_gridworld_lane_flush(p, (hipStream_t)stream) == hipSuccess ? WURM_OK : WURM_ERR_HIP;
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
    if (size > 11 || obs_n > 3 || opt.policy_wide) return launch_policy_wide(p, WURM_OBS_PARTIAL, obs_n, stream);
    policy_route = size == 9 && !opt.policy_generic ? 1 : 2;
    return launch_policy_rollout(p, obs_n, stream);
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
    switch (cpl) {
    case 2: WURM_LAUNCH(check_kernel<2>, grid, block, 0, st, envs, err, N, size); break;
    case 4: WURM_LAUNCH(check_kernel<4>, grid, block, 0, st, envs, err, N, size); break;
    case 8: WURM_LAUNCH(check_kernel<8>, grid, block, 0, st, envs, err, N, size); break;
    case 16: WURM_LAUNCH(check_kernel<16>, grid, block, 0, st, envs, err, N, size); break;
    case 24: WURM_LAUNCH(check_kernel<24>, grid, block, 0, st, envs, err, N, size); break;
    case 32: WURM_LAUNCH(check_kernel<32>, grid, block, 0, st, envs, err, N, size); break;
    case 48: WURM_LAUNCH(check_kernel<48>, grid, block, 0, st, envs, err, N, size); break;
    default: WURM_LAUNCH(check_kernel<64>, grid, block, 0, st, envs, err, N, size); break;
    }
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
    switch (cpl) {
    case 2: WURM_LAUNCH(orientations_kernel<2>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 4: WURM_LAUNCH(orientations_kernel<4>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 8: WURM_LAUNCH(orientations_kernel<8>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 16: WURM_LAUNCH(orientations_kernel<16>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 24: WURM_LAUNCH(orientations_kernel<24>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 32: WURM_LAUNCH(orientations_kernel<32>, grid, block, lds, st, envs, o, N, size, lpw); break;
    case 48: WURM_LAUNCH(orientations_kernel<48>, grid, block, lds, st, envs, o, N, size, lpw); break;
    default: WURM_LAUNCH(orientations_kernel<64>, grid, block, lds, st, envs, o, N, size, lpw); break;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

/* ---------------------------------------------------------------------------------------- SimpleGridworld */

int wurm_grid_step(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                   uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                   uint64_t seed, uint64_t call, int64_t env_offset, const int32_t *inject_food, void *stream)
{
    int rc = check_common(false, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_envs > 0 && (!actions || !reward || !done || !edge_collision)) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = envs; p.actions = const_cast<void *>(actions); p.act_dtype = actions_dtype; p.reward = reward;
    p.done = done; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(false, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.seed = seed; p.call = call;
    p.env_offset = env_offset; p.inject_food = inject_food;
    return launch<false>(K_STEP, p, stream);
}

int wurm_grid_reset(float *envs, const uint8_t *done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                    int size, int start_y, int start_x, uint64_t seed, uint64_t call, int64_t env_offset,
                    const int32_t *inject_reset, void *stream)
{
    int rc = check_common(false, envs, num_envs, size, obs, obs_mode, obs_n, WURM_ACT_I64);
    if (rc) return rc;
    if (size <= 4) return WURM_ERR_UNSUPPORTED;                                                  // simple_gridworld.py:249-250
    if (start_y < 0 || start_x < 0 || start_y >= size || start_x >= size) return WURM_ERR_UNSUPPORTED; // :254-260
    if (num_envs > 0 && !done) return WURM_ERR_INVALID_ARG;
    StepArgs p = {};
    p.envs = envs; p.done_in = done; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(false, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.start_y = start_y;
    p.start_x = start_x; p.seed = seed; p.call = call; p.env_offset = env_offset; p.inject_reset = inject_reset;
    return launch<false>(K_RESET, p, stream);
}

int wurm_grid_observe(const float *envs, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      void *stream)
{
    if (obs_mode == WURM_OBS_NONE) return WURM_ERR_INVALID_ARG;
    int rc = check_common(false, envs, num_envs, size, obs, obs_mode, obs_n, WURM_ACT_I64);
    if (rc) return rc;
    StepArgs p = {};
    p.envs = const_cast<float *>(envs); p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(false, obs_mode, obs_n, size); p.N = num_envs; p.S = size;
    return launch<false>(K_OBSERVE, p, stream);
}

int wurm_grid_rollout(float *envs, const void *actions, int actions_dtype, float *reward, uint8_t *done,
                      uint8_t *edge_collision, float *obs, int obs_mode, int obs_n, int64_t num_envs, int size,
                      int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0,
                      int64_t env_offset, const int32_t *inject_food, const int32_t *inject_reset, void *stream)
{
    int rc = check_common(false, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_steps < 0) return WURM_ERR_INVALID_ARG;
    if (size <= 4) return WURM_ERR_UNSUPPORTED;
    if (start_y < 0 || start_x < 0 || start_y >= size || start_x >= size) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && num_steps > 0 && (!actions || !reward || !done || !edge_collision)) return WURM_ERR_INVALID_ARG;
    if (num_steps == 0) return WURM_OK;
    StepArgs p = {};
    p.envs = envs; p.actions = const_cast<void *>(actions); p.act_dtype = actions_dtype; p.reward = reward;
    p.done = done; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(false, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.T = num_steps;
    p.start_y = start_y; p.start_x = start_x; p.seed = seed; p.call = call0; p.env_offset = env_offset;
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
    int rc = check_common(true, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_steps < 0) return WURM_ERR_INVALID_ARG;
    if (size <= 8) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && num_steps > 0 && (!actions || !reward || !done || !self_collision || !edge_collision))
        return WURM_ERR_INVALID_ARG;
    if (num_steps == 0 || num_envs == 0) return WURM_OK;
    StepArgs p = {};
    p.envs = envs; p.actions = actions; p.act_dtype = actions_dtype; p.reward = reward; p.done = done;
    p.selfc = self_collision; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(true, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.T = num_steps; p.seed = seed;
    p.call = call0; p.env_offset = env_offset;
    if (grid_rollout_eligible(p) && grid_resident_eligible(p)) {
        p.resident = resident;
        p.resident_valid = *resident_valid != 0;
        p.resident_lazy = resident_lazy != 0;
        rc = launch<true>(K_ROLLOUT, p, stream);
        *resident_valid = rc == WURM_OK ? 1 : 0;
        return rc;
    }
    if (resident_lazy && *resident_valid) {
        hipError_t err = hipSuccess;
        if (size == 9) err = launch_lane_resident_flush(p, resident, (hipStream_t)stream);
        else if (size == 10 || size == 11) err = launch_lane_wide_resident_flush(p, resident, (hipStream_t)stream);
        else if (grid_step_eligible(p)) { StepArgs q = p; q.resident = resident; err = launch_grid_resident_flush(q, (hipStream_t)stream); }
        if (err != hipSuccess) return WURM_ERR_HIP;
    }
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
    int rc = check_common(false, envs, num_envs, size, obs, obs_mode, obs_n, actions_dtype);
    if (rc) return rc;
    if (num_steps < 0) return WURM_ERR_INVALID_ARG;
    if (size <= 4) return WURM_ERR_UNSUPPORTED;
    if (start_y < 0 || start_x < 0 || start_y >= size || start_x >= size) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && num_steps > 0 && (!actions || !reward || !done || !edge_collision)) return WURM_ERR_INVALID_ARG;
    if (num_steps == 0 || num_envs == 0) return WURM_OK;
    StepArgs p = {};
    p.envs = envs; p.actions = const_cast<void *>(actions); p.act_dtype = actions_dtype; p.reward = reward;
    p.done = done; p.edgec = edge_collision; p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n;
    p.obs_elems = obs_elems(false, obs_mode, obs_n, size); p.N = num_envs; p.S = size; p.T = num_steps;
    p.start_y = start_y; p.start_x = start_x; p.seed = seed; p.call = call0; p.env_offset = env_offset;
    if (*resident_valid != 2 && gridworld_lane_eligible(p)) {
        p.resident = resident;
        p.resident_valid = *resident_valid == 1;
        p.resident_lazy = resident_lazy != 0;
        if (!p.resident_valid && hipMemsetAsync(resident, 0, 16, (hipStream_t)stream) != hipSuccess) return WURM_ERR_HIP;
        rc = launch<false>(K_ROLLOUT, p, stream);
        if (rc != WURM_OK) { *resident_valid = 0; return rc; }
        if (!p.resident_valid) { // the launch built the mirror: valid only if it could describe every env (see fused_entry)
            int odd = 0;
            if (hipMemcpyAsync(&odd, resident, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
                hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
                return WURM_ERR_HIP;
            *resident_valid = odd != 0 ? 2 : 1;
        }
        return WURM_OK;
    }
    if (resident_lazy && *resident_valid == 1) {
        StepArgs q = p;
        q.resident = resident;
        if (launch_gridworld_lane_flush(q, (hipStream_t)stream) != hipSuccess) return WURM_ERR_HIP;
    }
    if (*resident_valid != 2) *resident_valid = 0;
    return launch<false>(K_ROLLOUT, p, stream);
}

} // extern "C"
