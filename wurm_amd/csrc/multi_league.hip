// multi_league.hip — translation unit and C ABI of the MultiSnake league kernels (multi_league.hpp; include/wurm_hip.h:
// wurm_multi_act_league, wurm_multi_league_scores).  Arguments are validated before the first HIP call, so refusals work
// with no device present.
#include "multi_league.hpp"

using namespace wurm;

extern "C" {

int wurm_multi_act_league(const float *params, const float *obs, const int32_t *order, const int64_t *offsets,
                          int64_t *actions, float *probs, float *values, int64_t num_envs, int num_snakes,
                          int num_policies, int num_inputs, uint64_t seed, uint64_t call, int64_t env_offset, void *stream)
{
    if (num_envs < 0 || num_snakes < 0 || num_inputs < 0 || num_policies < 1) return WURM_ERR_INVALID_ARG;
    const int obs_n = multi_act_obs_n(num_inputs);
    if (obs_n < 0) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && (long long)num_snakes > (long long)INT32_MAX / num_envs) return WURM_ERR_UNSUPPORTED; // (`order` is int32)
    if (num_envs == 0 || num_snakes == 0) return WURM_OK;
    if (!params || !obs || !order || !offsets || !actions) return WURM_ERR_INVALID_ARG;
    MultiLeagueArgs a = {};
    a.params = params; a.obs = obs; a.actions = (long long *)actions; a.probs = probs; a.values = values;
    a.N = num_envs; a.K = num_snakes; a.P = num_policies; a.seed = seed; a.call = call; a.env_offset = env_offset;
    a.order = order; a.offsets = (const long long *)offsets;
    return launch_multi_act_league(a, obs_n, (hipStream_t)stream);
}

int wurm_multi_league_scores(const float *rewards, const uint8_t *dones, const float *food, const float *size,
                             const uint8_t *boost, const uint8_t *snake_collision, const uint8_t *edge_collision,
                             const int32_t *order, const int64_t *offsets, double *table, int64_t num_rows,
                             int64_t num_steps, int num_policies, void *stream)
{
    if (num_rows < 0 || num_steps < 0 || num_policies < 1) return WURM_ERR_INVALID_ARG;
    if (num_rows > INT32_MAX) return WURM_ERR_UNSUPPORTED; // (`order` is int32)
    if (num_rows == 0 || num_steps == 0) return WURM_OK;
    if (!rewards || !dones || !order || !offsets || !table) return WURM_ERR_INVALID_ARG;
    league::scores_args g = {};
    g.rewards = rewards; g.dones = dones; g.food = food; g.size = size; g.boost = boost; g.snake = snake_collision;
    g.edge = edge_collision; g.order = order; g.offsets = (const long long *)offsets; g.table = table;
    g.R = num_rows; g.T = num_steps;
    (void)hipGetLastError();
    WURM_LAUNCH(league_scores_kernel, dim3((unsigned)num_policies), dim3(league::THREADS), 0, (hipStream_t)stream, g);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
