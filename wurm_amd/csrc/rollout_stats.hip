// rollout_stats.hip — C ABI of the training statistics of a policy rollout (kernels: rollout_stats.hpp;
// include/wurm_hip.h: wurm_rollout_stats*).  Arguments are validated before the first HIP call, so refusals work with no
// device present.
#include "rollout_stats.hpp"
#include "../../include/wurm_hip.h"

using namespace wurm;
using namespace wurm::stats;

namespace {

long long num_groups(int64_t M) { return (M + THREADS - 1) / THREADS; }

// every member's partials (member-major), then every member's per-step sums (used when the caller gives no table)
int64_t workspace_bytes(int64_t N, int64_t T, int64_t members)
{
    return 8 * members * (num_groups(N / members) * partial_stride(T) + COLS * T);
}

bool valid_shape(int64_t N, int64_t T, int64_t members)
{
    return N > 0 && T > 0 && members > 0 && N % members == 0;
}

} // namespace

extern "C" {

int64_t wurm_rollout_stats_workspace_bytes(int64_t num_envs, int64_t num_steps, int64_t num_members)
{
    if (!valid_shape(num_envs, num_steps, num_members) || num_members > 65535) return 0;
    return workspace_bytes(num_envs, num_steps, num_members);
}

int wurm_rollout_stats(const float *rewards, const uint8_t *dones, const uint8_t *edge_collision,
                       const uint8_t *self_collision, const float *probs, void *carry, double *accum, double *smooth,
                       double *table, void *workspace, int64_t workspace_bytes_given, int64_t num_envs,
                       int64_t num_steps, int64_t num_members, int initial_size, double alpha, void *stream)
{
    if (!rewards || !dones || !edge_collision || !carry || !accum || !smooth || !workspace) return WURM_ERR_INVALID_ARG;
    if (!valid_shape(num_envs, num_steps, num_members)) return WURM_ERR_INVALID_ARG;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return WURM_ERR_INVALID_ARG; // (a NaN fails both)
    if (num_members > 65535) return WURM_ERR_UNSUPPORTED; // the member is the grid's y
    if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)probs % 16 != 0) return WURM_ERR_INVALID_ARG; // 16-byte loads
    if (workspace_bytes_given < workspace_bytes(num_envs, num_steps, num_members)) return WURM_ERR_INVALID_ARG;
    const int64_t M = num_envs / num_members;
    const long long G = num_groups(M);
    if (G > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED;

    scan_args a;
    a.rewards = rewards;
    a.dones = dones;
    a.edge = edge_collision;
    a.self = self_collision;
    a.probs = probs;
    a.carry_return = (float *)carry;
    a.carry_length = (int *)carry + num_envs;
    a.carry_size = (int *)carry + 2 * num_envs;
    a.partials = (double *)workspace;
    a.N = num_envs;
    a.M = M;
    a.T = num_steps;
    a.initial_size = initial_size;
    double *steps = table ? table : a.partials + num_members * G * partial_stride(num_steps);
    (void)hipGetLastError();
    WURM_LAUNCH(rollout_stats_scan_kernel, dim3((unsigned)G, (unsigned)num_members), dim3(THREADS), 0,
                (hipStream_t)stream, a);
    WURM_LAUNCH(rollout_stats_reduce_kernel, dim3(1, (unsigned)num_members), dim3(THREADS), 0, (hipStream_t)stream,
                a.partials, (int)G, (long long)M, (long long)num_steps, alpha, steps, accum, smooth);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
