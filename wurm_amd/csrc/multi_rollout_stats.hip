// multi_rollout_stats.hip — C ABI of the per-agent training statistics of a MultiSnake window (kernels:
// multi_rollout_stats.hpp; include/wurm_hip.h: wurm_multi_rollout_stats*).  Arguments are validated before the first HIP
// call, so refusals work with no device present.
#include "multi_rollout_stats.hpp"
#include "../../include/wurm_hip.h"

using namespace wurm;
using namespace wurm::mstats;

namespace {

constexpr int64_t MAX_SNAKES = 65535; // the agent is the grid's y

long long num_groups(int64_t N) { return (N + THREADS - 1) / THREADS; }

bool valid_shape(int64_t N, int64_t K, int64_t T) { return N > 0 && K > 0 && T > 0; }

// every wave's partials (agent-major), then every agent's per-step sums (used when the caller gives no table)
int64_t workspace_bytes(int64_t N, int64_t K, int64_t T)
{
    return 8 * K * (num_groups(N) * WAVES * partial_stride(T) + SUMS * T);
}

} // namespace

extern "C" {

int64_t wurm_multi_rollout_stats_workspace_bytes(int64_t num_envs, int64_t num_snakes, int64_t num_steps)
{
    if (!valid_shape(num_envs, num_snakes, num_steps) || num_snakes > MAX_SNAKES) return 0;
    return workspace_bytes(num_envs, num_snakes, num_steps);
}

int wurm_multi_rollout_stats(const float *rewards, const float *food, const float *size, const uint8_t *dones,
                             const uint8_t *boost, const uint8_t *snake_collision, const uint8_t *edge_collision,
                             const float *probs, const uint8_t *all_done, void *carry, double *accum, double *smooth,
                             double *table, void *workspace, int64_t workspace_bytes_given, int64_t num_envs,
                             int64_t num_snakes, int64_t num_steps, double alpha, void *stream)
{
    if (!rewards || !food || !size || !dones || !boost || !snake_collision || !edge_collision) return WURM_ERR_INVALID_ARG;
    if (!carry || !accum || !smooth || !workspace) return WURM_ERR_INVALID_ARG;
    if (!valid_shape(num_envs, num_snakes, num_steps)) return WURM_ERR_INVALID_ARG;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return WURM_ERR_INVALID_ARG; // (a NaN fails both)
    if (num_snakes > MAX_SNAKES) return WURM_ERR_UNSUPPORTED;
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)probs % 16 != 0) return WURM_ERR_INVALID_ARG; // 16-byte loads
    if (workspace_bytes_given < workspace_bytes(num_envs, num_snakes, num_steps)) return WURM_ERR_INVALID_ARG;
    const long long G = num_groups(num_envs);
    if (G > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED;

    scan_args a;
    a.rewards = rewards;
    a.food = food;
    a.size = size;
    a.dones = dones;
    a.boost = boost;
    a.snake = snake_collision;
    a.edge = edge_collision;
    a.probs = probs;
    a.all_done = all_done;
    a.carry_return = (float *)carry;
    a.carry_length = (int *)carry + num_snakes * num_envs;
    a.partials = (double *)workspace;
    a.N = num_envs;
    a.T = num_steps;
    const long long W = G * WAVES;
    double *steps = table ? table : a.partials + num_snakes * W * partial_stride(num_steps);
    (void)hipGetLastError();
    WURM_LAUNCH(multi_rollout_stats_scan_kernel, dim3((unsigned)G, (unsigned)num_snakes), dim3(THREADS), 0,
                (hipStream_t)stream, a);
    WURM_LAUNCH(multi_rollout_stats_reduce_kernel, dim3(1, (unsigned)num_snakes), dim3(THREADS), 0, (hipStream_t)stream,
                a.partials, W, (long long)num_envs, (long long)num_steps, alpha, steps, accum, smooth);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
