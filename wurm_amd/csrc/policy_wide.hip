// policy_wide.hip — translation unit of the fused acting loop for every configuration the reference's feed-forward
// experiment accepts (policy_wide.hpp) and of its entry points: the observation-mode entry of SingleSnake, the
// SimpleGridworld one, and the route query of the policy entry points.  wurm_single_policy_rollout (single_snake.hip) calls
// launch_policy_wide for the shapes outside policy_rollout.hpp's domain.
#include "policy_wide.hpp"

namespace wurm {

// which kernel served the CALLING THREAD's last policy launch (wurm_policy_last_route): 0 none yet, 1 policy_rollout_s9_kernel,
// 2 policy_rollout_kernel, 3 policy_wide_kernel.  Set by both translation units of the policy entry points.
thread_local int policy_route = 0;

// the SingleSnake launch (obs_mode WURM_OBS_PARTIAL or WURM_OBS_POSITIONS); arguments already validated
int launch_policy_wide(const PolicyArgs &p, int obs_mode, int obs_n, void *stream, long long members)
{
    PolicyWideArgs a = {};
    a.p = p;
    a.obs_mode = obs_mode;
    a.obs_n = obs_mode == WURM_OBS_PARTIAL ? obs_n : 0;
    a.E = obs_mode == WURM_OBS_PARTIAL ? 3 * (2 * obs_n + 1) * (2 * obs_n + 1) : 4;
    policy_route = 3;
    return launch_policy_wide_cpl<true>(a, pick_cpl(p.S), (hipStream_t)stream, members);
}

// single_snake.hip
int single_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                          float *values, float *reward, uint8_t *done, uint8_t *self_collision, uint8_t *edge_collision,
                          float *obs, uint8_t *status, int obs_n, int64_t num_envs, int size, int64_t num_steps,
                          uint64_t seed, uint64_t call0, int64_t env_offset, void *stream, long long members);

// wurm_single_policy_rollout_mode (members == 0) and wurm_single_policy_rollout_pop
static int single_policy_rollout_mode(float *envs, const float *obs0, const float *params, int64_t *actions,
                                      float *probs, float *values, float *reward, uint8_t *done,
                                      uint8_t *self_collision, uint8_t *edge_collision, float *obs, uint8_t *status,
                                      int obs_mode, int obs_n, int64_t num_envs, int size, int64_t num_steps,
                                      uint64_t seed, uint64_t call0, int64_t env_offset, void *stream, long long members)
{
    if (obs_mode == WURM_OBS_PARTIAL)
        return single_policy_rollout(envs, obs0, params, actions, probs, values, reward, done, self_collision,
                                     edge_collision, obs, status, obs_n, num_envs, size, num_steps, seed, call0,
                                     env_offset, stream, members);
    if (num_envs < 0 || num_steps < 0 || size < 3) return WURM_ERR_INVALID_ARG;
    // the image modes: the reference's FeedforwardAgent takes a flat vector (experiments/main.py:129-137 builds it for
    // 'positions' and 'partial_n' only); WURM_OBS_NONE leaves the policy nothing to act on
    if (obs_mode != WURM_OBS_POSITIONS) return WURM_ERR_UNSUPPORTED;
    if (size <= 8 || size > 64) return WURM_ERR_UNSUPPORTED; // the reset draw needs 9 x 9; 64 x 64 is the largest grid
    if (num_envs == 0 || num_steps == 0) return WURM_OK;
    if (!envs || !obs0 || !params || !actions || !probs || !values || !reward || !done || !self_collision ||
        !edge_collision || !obs || !status)
        return WURM_ERR_INVALID_ARG;
    const PolicyArgs p = make_policy_args(envs, obs0, params, actions, probs, values, reward, done, self_collision,
                                          edge_collision, obs, status, num_envs, size, num_steps, seed, call0, env_offset);
    return launch_policy_wide(p, WURM_OBS_POSITIONS, 0, stream, members);
}

// wurm_grid_policy_rollout (members == 0) and wurm_grid_policy_rollout_pop
static int grid_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                               float *values, float *reward, uint8_t *done, uint8_t *edge_collision, float *obs,
                               uint8_t *status, int64_t num_envs, int size, int64_t num_steps, int start_y, int start_x,
                               uint64_t seed, uint64_t call0, int64_t env_offset, void *stream, long long members)
{
    if (num_envs < 0 || num_steps < 0 || size < 3) return WURM_ERR_INVALID_ARG;
    if (size <= 4 || size > 64) return WURM_ERR_UNSUPPORTED; // simple_gridworld.py:249-250; 64 x 64 is the largest grid
    if (start_y < 0 || start_x < 0 || start_y >= size || start_x >= size) return WURM_ERR_UNSUPPORTED;
    if (num_envs == 0 || num_steps == 0) return WURM_OK;
    if (!envs || !obs0 || !params || !actions || !probs || !values || !reward || !done || !edge_collision || !obs ||
        !status)
        return WURM_ERR_INVALID_ARG;
    PolicyWideArgs a = {};
    a.p = make_policy_args(envs, obs0, params, actions, probs, values, reward, done, nullptr, edge_collision, obs, status,
                           num_envs, size, num_steps, seed, call0, env_offset);
    a.obs_mode = WURM_OBS_POSITIONS;
    a.E = 4;
    a.start_y = start_y;
    a.start_x = start_x;
    policy_route = 3;
    return launch_policy_wide_cpl<false>(a, pick_cpl(size), (hipStream_t)stream, members);
}

} // namespace wurm

using namespace wurm;

extern "C" {

const char *wurm_policy_last_route(void)
{
    switch (policy_route) {
    case 1: return "policy_s9";
    case 2: return "policy_generic";
    case 3: return "policy_wide";
    default: return "none";
    }
}

int wurm_single_policy_rollout_mode(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                    float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                                    uint8_t *edge_collision, float *obs, uint8_t *status, int obs_mode, int obs_n,
                                    int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                    int64_t env_offset, void *stream)
{
    return single_policy_rollout_mode(envs, obs0, params, actions, probs, values, reward, done, self_collision,
                                      edge_collision, obs, status, obs_mode, obs_n, num_envs, size, num_steps, seed,
                                      call0, env_offset, stream, 0);
}

int wurm_single_policy_rollout_pop(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                   float *values, float *reward, uint8_t *done, uint8_t *self_collision,
                                   uint8_t *edge_collision, float *obs, uint8_t *status, int obs_mode, int obs_n,
                                   int64_t num_envs, int size, int64_t num_steps, uint64_t seed, uint64_t call0,
                                   int64_t env_offset, void *stream, int64_t num_members)
{
    if (num_members <= 0 || num_envs % num_members != 0) return WURM_ERR_INVALID_ARG;
    return single_policy_rollout_mode(envs, obs0, params, actions, probs, values, reward, done, self_collision,
                                      edge_collision, obs, status, obs_mode, obs_n, num_envs, size, num_steps, seed,
                                      call0, env_offset, stream, num_members);
}

int wurm_grid_policy_rollout(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                             float *values, float *reward, uint8_t *done, uint8_t *edge_collision, float *obs,
                             uint8_t *status, int64_t num_envs, int size, int64_t num_steps, int start_y, int start_x,
                             uint64_t seed, uint64_t call0, int64_t env_offset, void *stream)
{
    return grid_policy_rollout(envs, obs0, params, actions, probs, values, reward, done, edge_collision, obs, status,
                               num_envs, size, num_steps, start_y, start_x, seed, call0, env_offset, stream, 0);
}

int wurm_grid_policy_rollout_pop(float *envs, const float *obs0, const float *params, int64_t *actions, float *probs,
                                 float *values, float *reward, uint8_t *done, uint8_t *edge_collision, float *obs,
                                 uint8_t *status, int64_t num_envs, int size, int64_t num_steps, int start_y,
                                 int start_x, uint64_t seed, uint64_t call0, int64_t env_offset, void *stream,
                                 int64_t num_members)
{
    if (num_members <= 0 || num_envs % num_members != 0) return WURM_ERR_INVALID_ARG;
    return grid_policy_rollout(envs, obs0, params, actions, probs, values, reward, done, edge_collision, obs, status,
                               num_envs, size, num_steps, start_y, start_x, seed, call0, env_offset, stream, num_members);
}

} // extern "C"
