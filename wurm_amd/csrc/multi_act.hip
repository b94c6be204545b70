// multi_act.hip — translation unit and C ABI of the MultiSnake acting kernel (multi_act.hpp; include/wurm_hip.h:
// wurm_multi_act).  Arguments are validated before the first HIP call, so refusals work with no device present.
#include "multi_act.hpp"

using namespace wurm;

extern "C" {

int wurm_multi_act(const float *params, const float *obs, int64_t *actions, float *probs, float *values,
                   int64_t num_envs, int num_snakes, int num_species, int num_inputs, uint64_t seed, uint64_t call,
                   int64_t env_offset, void *stream)
{
    if (num_envs < 0 || num_snakes < 0 || num_inputs < 0) return WURM_ERR_INVALID_ARG;
    if (num_species < 1 || num_species > num_snakes) return WURM_ERR_INVALID_ARG;
    const int obs_n = multi_act_obs_n(num_inputs);
    if (obs_n < 0) return WURM_ERR_UNSUPPORTED;
    if (num_envs == 0) return WURM_OK;
    if (!params || !obs || !actions) return WURM_ERR_INVALID_ARG;
    MultiActArgs a = {};
    a.params = params; a.obs = obs; a.actions = (long long *)actions; a.probs = probs; a.values = values;
    a.N = num_envs; a.K = num_snakes; a.P = num_species; a.seed = seed; a.call = call; a.env_offset = env_offset;
    return launch_multi_act(a, obs_n, (hipStream_t)stream);
}

} // extern "C"
