// multi_policy_window.hip — C ABI of MultiSnake.policy_window (kernel: multi_policy_window.hpp; include/wurm_hip.h:
// wurm_multi_policy_window).  Arguments are validated before the first HIP call, so refusals work with no device present.
#include <algorithm>
#include <cstdint>

#include "multi_policy_window.hpp"
#include "options.hpp"

using namespace wurm;

namespace {

bool aligned(const void *ptr, uintptr_t to) { return ((uintptr_t)ptr & (to - 1)) == 0; }

// what the kernel serves of (K, S, n, P): WURM_OK, or the refusal
int shape_check(int K, int S, int n, int P)
{
    if (K < 1 || S < 3 || P < 1 || P > K) return WURM_ERR_INVALID_ARG;
    if (K > 64 || S > 64 || S < 5) return WURM_ERR_UNSUPPORTED; // what wurm_multi_rollout serves
    if (n < 0 || n > MPW_MAX_OBS_N) return WURM_ERR_UNSUPPORTED;
    return WURM_OK;
}

} // namespace

extern "C" {

int wurm_multi_policy_window_plan(int num_snakes, int size, int obs_n, int num_species, int64_t num_envs)
{
    if (shape_check(num_snakes, size, obs_n, num_species) != WURM_OK || num_envs < 0) return 0;
    MultiArgs m = {};
    m.K = num_snakes; m.S = size; m.N = num_envs;
    const MultiPolicyWindowPlan pl = multi_policy_window_plan(m, num_species, obs_n, 0);
    return pl.ns == 0 ? 0 : pl.reload ? 2 : 1;
}

int wurm_multi_policy_window(const wurm_multi_policy_window_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (!c->foods || !c->heads || !c->bodies || !c->dones || !c->orientations || !c->colours || !c->boost_this_step ||
        !c->params || !c->obs0)
        return WURM_ERR_INVALID_ARG;
    if (c->num_envs < 0 || c->num_steps < 0) return WURM_ERR_INVALID_ARG;
    const int K = c->num_snakes, S = c->size, n = c->obs_n, P = c->num_species;
    const int rc = shape_check(K, S, n, P);
    if (rc != WURM_OK) return rc;
    const int W = 2 * n + 1, E = 3 * W * W;
    if (c->num_params != policy_num_params(E)) return WURM_ERR_INVALID_ARG;
    if (c->waves_per_group < 0 || c->waves_per_group > MPW_MAX_WAVES) return WURM_ERR_INVALID_ARG;
    if (c->num_steps > 0 && (!c->actions || !c->probs || !c->values || !c->observations || !c->rewards || !c->dones_out ||
                             !c->all_done || !c->food || !c->sizes || !c->boost || !c->snake_collision || !c->edge_collision))
        return WURM_ERR_INVALID_ARG;
    if (!aligned(c->foods, 4) || !aligned(c->heads, 4) || !aligned(c->bodies, 4) || !aligned(c->orientations, 8) ||
        !aligned(c->colours, 2) || !aligned(c->params, 4) || !aligned(c->obs0, 4) || !aligned(c->actions, 8) ||
        !aligned(c->probs, 4) || !aligned(c->values, 4) || !aligned(c->observations, 4) || !aligned(c->rewards, 4) ||
        !aligned(c->food, 4) || !aligned(c->sizes, 4))
        return WURM_ERR_INVALID_ARG;
    MultiPolicyWindowArgs a = {};
    MultiArgs &p = a.m;
    p.foods = c->foods; p.heads = c->heads; p.bodies = c->bodies; p.dones = c->dones;
    p.orientations = (long long *)c->orientations; p.colours = (short *)c->colours; p.boost_state = c->boost_this_step;
    p.obs_mode = WURM_OBS_PARTIAL; p.obs_n = n; p.obs_elems = E;
    p.N = c->num_envs; p.K = K; p.S = S; p.T = c->num_steps;
    p.cfg = c->cfg; p.seed = c->seed; p.call = c->call0; p.env_offset = c->env_offset;
    p.done_env = c->pre_done; p.pre_call = c->pre_call;
    const MultiPolicyWindowPlan pl = multi_policy_window_plan(p, P, n, c->waves_per_group);
    if (pl.ns == 0) return WURM_ERR_UNSUPPORTED; // an env whose grids do not fit beside one W1 block
    const long long groups = (c->num_envs + pl.wpb - 1) / pl.wpb;
    if (groups > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED;
    if (c->num_envs == 0 || c->num_steps == 0) return WURM_OK; // nothing to launch (a postponed reset stays the caller's)
    a.params = c->params; a.obs0 = c->obs0; a.actions = (long long *)c->actions; a.probs = c->probs; a.values = c->values;
    a.obs = c->observations; a.rewards = c->rewards; a.food = c->food; a.sizes = c->sizes; a.dones = c->dones_out;
    a.boost = c->boost; a.snakecol = c->snake_collision; a.edgecol = c->edge_collision; a.all_done = c->all_done;
    a.pcall = c->policy_call0; a.P = P; a.E = E; a.EP = (E + 15) & ~15;
    a.wpb = pl.wpb; a.reload = pl.reload; a.w1_bytes = pl.w1_bytes; a.env_bytes = pl.env_bytes;
    const dim3 grid((unsigned)groups), block(64 * pl.wpb);
    (void)hipGetLastError();
    auto go = [&](auto kernel) {
        // dynamic LDS beyond the default 64 KB of a launch needs the kernel's opt-in
        if (pl.lds > 65536 && hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds) != hipSuccess)
            return WURM_ERR_HIP;
        WURM_LAUNCH(kernel, grid, block, (size_t)pl.lds, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
    };
    switch (pl.ns) {
    case 1: return go(multi_policy_window_kernel<1>);
    case 2: return go(multi_policy_window_kernel<2>);
    default: return go(multi_policy_window_kernel<4>);
    }
}

} // extern "C"
