// a2c_learner.hip — C ABI of the fused A2C learner (kernels: a2c_learner.hpp; include/wurm_hip.h: wurm_a2c_ff_*).
// Every entry point validates its arguments before the first HIP call, so refusals work with no device present.
#include "a2c_learner.hpp"
#include "../../include/wurm_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace wurm;
using namespace wurm::a2c;

namespace {

bool supported_inputs(int E)
{
    if (E == 4) return true; // 'positions'
    for (int n = 0; n <= 6; ++n)
        if (E == 3 * (2 * n + 1) * (2 * n + 1)) return true; // 'partial_n'
    return false;
}

int num_groups(int64_t N) { return (int)(N < MAX_GROUPS ? N : MAX_GROUPS); }

int64_t workspace_bytes(int64_t N, int64_t T, int E)
{
    return 4 * (num_groups(N) * partial_stride(E) + N * (T + 1) * ROW_FLOATS);
}

// A league's members have min(M_a, 256) partials each, and their M_a sum to at most N: min(N, 256 A) partials serve any
// line-up (the host knows no more), then the parked rows of all N columns
int64_t league_groups(int64_t N, int64_t A) { return N < MAX_GROUPS * A ? N : MAX_GROUPS * A; }

int64_t league_workspace_bytes(int64_t N, int64_t T, int E, int64_t A)
{
    return 4 * (league_groups(N, A) * partial_stride(E) + N * (T + 1) * ROW_FLOATS);
}

// The hyper-parameters cross the ABI as floats, torch.optim.Adam keeps them as doubles: 0.999f is 0.99900001287, and
// 1 - beta2 taken from it is off by 1.3e-5 of itself.  The shortest decimal that rounds to the float is the number the
// caller wrote (0.999, 1e-3, 1e-8, ...), so the host arithmetic below runs on that.
double as_written(float x)
{
    if (!std::isfinite(x) || x == 0.0f) return (double)x;
    char buf[40];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof buf, "%.*g", digits, (double)x);
        const double d = strtod(buf, nullptr);
        if ((float)d == x) return d;
    }
    return (double)x;
}

// gamma * lambda as the caller rounded it: finite and not negative (refused like the other arguments, before any launch)
bool valid_gamma_lambda(float gamma_lambda) { return std::isfinite(gamma_lambda) && gamma_lambda >= 0.0f; }

// What an entry point asks for, as its caller handed it over.  pop: the population kernels, `members` sets of weights of
// N / members consecutive envs each, gamma, entropy_coef and gamma_lambda out of `hyper`; else the stand-alone kernels,
// which take the three by value.  league: the league kernels, `members` sets of weights, each with the columns its piece
// of `order` names (`offsets`; `learn` nullable), the rest as for pop.
struct GradRequest {
    const float *params, *obs0, *obs;
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    int value_loss_kind;
    float *grad, *losses, *values_out; // values_out: nullable
    void *workspace;
    int64_t workspace_bytes, N, T;
    int E;
    bool pop;
    int64_t members;
    const double *hyper;
    float gamma, entropy_coef;
    bool gae;
    float gamma_lambda;
    float *returns_out; // nullable
    bool league;
    const int32_t *order;
    const int64_t *offsets;
    const uint8_t *learn; // nullable
};

struct ApplyRequest {
    float *params;
    const float *grad;
    float *exp_avg, *exp_avg_sq, *grad_norm; // grad_norm: nullable
    int64_t step;
    float beta1, beta2, eps, max_grad_norm;
    int64_t num_params;
    bool pop;
    int64_t members;
    const double *hyper;
    float lr; // stand-alone only: a member's is in its row of `hyper`
    bool league;
    const int64_t *offsets;
    const uint8_t *learn; // nullable
    int64_t rows;         // the N of the lists
};

int check_grad(const GradRequest &r)
{
    if (r.gae && !r.pop && !valid_gamma_lambda(r.gamma_lambda)) return WURM_ERR_INVALID_ARG; // (a member's: wurm_a2c_ff_pop_hyper)
    if (r.pop && (!r.hyper || r.members <= 0 || r.N <= 0 || r.N % r.members != 0)) return WURM_ERR_INVALID_ARG;
    if (r.league && (!r.hyper || !r.order || !r.offsets || r.members <= 0 || r.N <= 0)) return WURM_ERR_INVALID_ARG;
    const int64_t M = r.pop ? r.N / r.members : r.N; // the envs of one set of weights
    if (!r.params || !r.obs0 || !r.obs || !r.actions || !r.rewards || !r.dones || !r.grad || !r.losses || !r.workspace)
        return WURM_ERR_INVALID_ARG;
    if (M <= 0 || r.T <= 0 || r.E <= 0 || r.workspace_bytes < 0) return WURM_ERR_INVALID_ARG;
    if ((uintptr_t)r.workspace % 16 != 0) return WURM_ERR_INVALID_ARG; // 16-byte accesses
    if (!supported_inputs(r.E)) return WURM_ERR_UNSUPPORTED;
    if (r.value_loss_kind != WURM_A2C_SMOOTH_L1 && r.value_loss_kind != WURM_A2C_MSE) return WURM_ERR_UNSUPPORTED;
    if (r.league) { // (M = N above: a member's columns are known on the device only)
        if (r.members > 65535 || r.N >= (1LL << 31)) return WURM_ERR_UNSUPPORTED; // the grid's y; `order` is int32
        return r.workspace_bytes < league_workspace_bytes(r.N, r.T, r.E, r.members) ? WURM_ERR_INVALID_ARG : WURM_OK;
    }
    if (r.workspace_bytes < workspace_bytes(M, r.T, r.E)) return WURM_ERR_INVALID_ARG;
    if (!r.pop) return WURM_OK;
    if (r.members > 65535) return WURM_ERR_UNSUPPORTED; // the member is the grid's y
    return r.workspace_bytes < r.members * workspace_bytes(M, r.T, r.E) ? WURM_ERR_INVALID_ARG : WURM_OK;
}

int check_apply(const ApplyRequest &r)
{
    if ((r.pop || r.league) && (!r.hyper || r.members <= 0)) return WURM_ERR_INVALID_ARG;
    if (r.league && (!r.offsets || r.rows <= 0)) return WURM_ERR_INVALID_ARG;
    if (!r.params || !r.grad || !r.exp_avg || !r.exp_avg_sq) return WURM_ERR_INVALID_ARG;
    if (r.step < 1 || r.num_params <= 0) return WURM_ERR_INVALID_ARG;
    if ((!r.pop && !r.league && !(r.lr >= 0.0f)) || !(r.beta1 >= 0.0f && r.beta1 < 1.0f) || !(r.beta2 >= 0.0f && r.beta2 < 1.0f) ||
        !(r.eps >= 0.0f))
        return WURM_ERR_INVALID_ARG; // (a member's lr: wurm_a2c_ff_pop_hyper)
    if (r.league && r.rows >= (1LL << 31)) return WURM_ERR_UNSUPPORTED;
    return (r.pop || r.league) && r.members > 65535 ? WURM_ERR_UNSUPPORTED : WURM_OK;
}

// The population's workspace holds every member's partials (member-major), then every member's parked rows: each part is
// what a stand-alone update of M envs has, `members` times over.
// The league's holds league_groups partials, each member's behind those of the members before it, then the parked rows of
// all N columns by list position; its grid is (min(N, 256), members), whatever the lists hold.
template <bool GAE, bool POP, bool LEAGUE = false> void launch_grad(const GradRequest &r, hipStream_t stream)
{
    const int64_t sets = POP || LEAGUE ? r.members : 1, M = LEAGUE ? r.N : r.N / sets;
    typename kernel_args<GAE, POP, LEAGUE>::type a = {};
    a.params = r.params;
    a.obs0 = r.obs0;
    a.obs = r.obs;
    a.actions = (const long long *)r.actions;
    a.rewards = r.rewards;
    a.dones = r.dones;
    a.values_out = r.values_out;
    a.partials = (float *)r.workspace;
    a.G = num_groups(M);
    a.rows = a.partials + (LEAGUE ? league_groups(r.N, sets) : sets * a.G) * partial_stride(r.E);
    a.N = r.N;
    a.T = r.T;
    a.E = r.E;
    a.loss_kind = r.value_loss_kind;
    a.inv_B = 1.0f / (float)(M * r.T); // (LEAGUE: every member's own, formed on the device)
    if constexpr (GAE) a.returns_out = r.returns_out;
    if constexpr (POP) {
        a.M = M;
        a.hyper = r.hyper;
    } else if constexpr (LEAGUE) {
        a.hyper = r.hyper;
        a.order = r.order;
        a.offsets = (const long long *)r.offsets;
        a.learn = r.learn;
    } else {
        a.gamma = r.gamma;
        a.entropy_coef = r.entropy_coef;
        if constexpr (GAE) a.gamma_lambda = r.gamma_lambda;
    }
    WURM_LAUNCH((a2c_ff_main_kernel<GAE, POP, LEAGUE>), dim3((unsigned)a.G, (unsigned)sets), dim3(THREADS), 0, stream, a);
    const long long P = num_params(r.E);
    if constexpr (LEAGUE) {
        WURM_LAUNCH(a2c_ff_reduce_league_kernel, dim3((unsigned)((P + 3 + THREADS - 1) / THREADS), (unsigned)sets),
                    dim3(THREADS), 0, stream, a.partials, a.offsets, a.learn, a.N, a.T, r.E, r.grad, r.losses);
        return;
    }
    WURM_LAUNCH(POP ? a2c_ff_reduce_pop_kernel : a2c_ff_reduce_kernel,
                dim3((unsigned)((P + 3 + THREADS - 1) / THREADS), (unsigned)sets), dim3(THREADS), 0, stream, a.partials, a.G,
                r.E, a.inv_B, r.grad, r.losses);
}

// step_size = lr / (1 - beta1^step), divided in double and rounded once: here for the stand-alone kernel, by the
// population kernel itself from bc1 and the member's lr
void launch_apply(const ApplyRequest &r, hipStream_t stream)
{
    const double b1 = as_written(r.beta1), b2 = as_written(r.beta2);
    const double bc1 = 1.0 - std::pow(b1, (double)r.step);
    const float bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)r.step));
    const float w1 = (float)(1.0 - b1), w2 = (float)(1.0 - b2), eps = (float)as_written(r.eps);
    const dim3 grid((unsigned)((r.num_params + APPLY_PER_BLOCK - 1) / APPLY_PER_BLOCK),
                    r.pop || r.league ? (unsigned)r.members : 1u);
    if (r.league)
        WURM_LAUNCH(a2c_ff_apply_league_kernel, grid, dim3(THREADS), 0, stream, r.params, r.grad, r.exp_avg, r.exp_avg_sq,
                    r.grad_norm, r.hyper, (const long long *)r.offsets, r.learn, (long long)r.rows, bc1, bc2_sqrt,
                    (float)b2, w1, w2, eps, r.max_grad_norm, (long long)r.num_params);
    else if (r.pop)
        WURM_LAUNCH(a2c_ff_apply_pop_kernel, grid, dim3(THREADS), 0, stream, r.params, r.grad, r.exp_avg, r.exp_avg_sq,
                    r.grad_norm, r.hyper, bc1, bc2_sqrt, (float)b2, w1, w2, eps, r.max_grad_norm, (long long)r.num_params);
    else
        WURM_LAUNCH(a2c_ff_apply_kernel, grid, dim3(THREADS), 0, stream, r.params, r.grad, r.exp_avg, r.exp_avg_sq,
                    r.grad_norm, (float)(as_written(r.lr) / bc1), bc2_sqrt, (float)b2, w1, w2, eps, r.max_grad_norm,
                    (long long)r.num_params);
}

// grad (g), apply (a) or update (both): every check of the grad half, then every check of the apply half, then the launches
int run(const GradRequest *g, const ApplyRequest *a, void *stream)
{
    int rc = g ? check_grad(*g) : WURM_OK;
    if (rc == WURM_OK && a) rc = check_apply(*a);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    if (g) {
        auto *launch = g->league ? (g->gae ? launch_grad<true, false, true> : launch_grad<false, false, true>)
                       : g->pop  ? (g->gae ? launch_grad<true, true> : launch_grad<false, true>)
                                 : (g->gae ? launch_grad<true, false> : launch_grad<false, false>);
        launch(*g, (hipStream_t)stream);
    }
    if (a) launch_apply(*a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace

extern "C" {

int64_t wurm_a2c_ff_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs)
{
    if (num_envs <= 0 || num_steps <= 0 || !supported_inputs(num_inputs)) return 0;
    return workspace_bytes(num_envs, num_steps, num_inputs);
}

int wurm_a2c_ff_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                     const float *rewards, const uint8_t *dones, float gamma, float entropy_coef, int value_loss_kind,
                     float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                     int64_t num_envs, int64_t num_steps, int num_inputs, void *stream)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, false, 0, nullptr, gamma, entropy_coef};
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                         int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                         int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, void *stream,
                         float gamma_lambda, float *returns_out)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, false, 0, nullptr, gamma, entropy_coef,
                           true, gamma_lambda, returns_out};
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                      int64_t step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                      int64_t num_params, void *stream)
{
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            num_params, false, 0, nullptr, lr};
    return run(nullptr, &a, stream);
}

int wurm_a2c_ff_hyper_parameter(float x, double *value)
{
    if (!value) return WURM_ERR_INVALID_ARG;
    *value = as_written(x);
    return WURM_OK;
}

int wurm_a2c_ff_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                       const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                       int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                       int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, float *exp_avg,
                       float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1, float beta2, float eps,
                       float max_grad_norm, void *stream)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, false, 0, nullptr, gamma, entropy_coef};
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            a2c::num_params(num_inputs), false, 0, nullptr, lr};
    return run(&g, &a, stream);
}

int wurm_a2c_ff_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                           int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                           int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs,
                           float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1,
                           float beta2, float eps, float max_grad_norm, void *stream, float gamma_lambda,
                           float *returns_out)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, false, 0, nullptr, gamma, entropy_coef,
                           true, gamma_lambda, returns_out};
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            a2c::num_params(num_inputs), false, 0, nullptr, lr};
    return run(&g, &a, stream);
}

int64_t wurm_a2c_ff_pop_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members)
{
    if (num_members <= 0 || num_envs <= 0 || num_envs % num_members != 0 || num_steps <= 0 ||
        !supported_inputs(num_inputs))
        return 0;
    return num_members * workspace_bytes(num_envs / num_members, num_steps, num_inputs);
}

int wurm_a2c_ff_pop_hyper(const float *lr, const float *gamma, const float *entropy_coef, const float *gamma_lambda,
                          int64_t num_members, double *table)
{
    if (!lr || !gamma || !entropy_coef || !table || num_members <= 0) return WURM_ERR_INVALID_ARG;
    for (int64_t m = 0; m < num_members; ++m) {
        if (!(lr[m] >= 0.0f)) return WURM_ERR_INVALID_ARG; // (what check_apply asks of a stand-alone lr)
        if (gamma_lambda && !valid_gamma_lambda(gamma_lambda[m])) return WURM_ERR_INVALID_ARG;
    }
    for (int64_t m = 0; m < num_members; ++m) {
        double *row = table + m * HYPER_DOUBLES;
        row[0] = as_written(lr[m]);
        row[1] = (double)gamma[m];
        row[2] = (double)entropy_coef[m];
        row[3] = gamma_lambda ? (double)gamma_lambda[m] : 0.0;
    }
    return WURM_OK;
}

int wurm_a2c_ff_pop_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                         float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                         int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, true, num_members, hyper};
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_pop_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                             const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                             float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                             int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                             float *returns_out)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, true, num_members, hyper, 0.0f, 0.0f,
                           true, 0.0f, returns_out};
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_pop_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                          const double *hyper, int64_t step, float beta1, float beta2, float eps, float max_grad_norm,
                          int64_t num_params, int64_t num_members, void *stream)
{
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            num_params, true, num_members, hyper};
    return run(nullptr, &a, stream);
}

int wurm_a2c_ff_pop_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                           float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                           int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                           float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                           float max_grad_norm, void *stream)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, true, num_members, hyper};
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            a2c::num_params(num_inputs), true, num_members, hyper};
    return run(&g, &a, stream);
}

int wurm_a2c_ff_pop_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                               const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                               float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                               int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members,
                               float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                               float beta2, float eps, float max_grad_norm, void *stream, float *returns_out)
{
    const GradRequest g = {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
                           workspace_bytes, num_envs, num_steps, num_inputs, true, num_members, hyper, 0.0f, 0.0f,
                           true, 0.0f, returns_out};
    const ApplyRequest a = {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm,
                            a2c::num_params(num_inputs), true, num_members, hyper};
    return run(&g, &a, stream);
}

int64_t wurm_a2c_ff_league_workspace_bytes(int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members)
{
    if (num_members <= 0 || num_members > 65535 || num_rows <= 0 || num_rows >= (1LL << 31) || num_steps <= 0 ||
        !supported_inputs(num_inputs))
        return 0;
    return league_workspace_bytes(num_rows, num_steps, num_inputs, num_members);
}

namespace {

GradRequest league_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                        const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                        const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad, float *losses,
                        float *values_out, void *workspace, int64_t workspace_bytes, int64_t num_rows, int64_t num_steps,
                        int num_inputs, int64_t num_members, bool gae, float *returns_out)
{
    return {params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,
            workspace_bytes, num_rows, num_steps, num_inputs, false, num_members, hyper, 0.0f, 0.0f, gae, 0.0f,
            returns_out, true, order, offsets, learn};
}

ApplyRequest league_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                          const double *hyper, const int64_t *offsets, const uint8_t *learn, int64_t step, float beta1,
                          float beta2, float eps, float max_grad_norm, int64_t num_params, int64_t num_rows,
                          int64_t num_members)
{
    return {params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm, num_params, false,
            num_members, hyper, 0.0f, true, offsets, learn, num_rows};
}

} // namespace

int wurm_a2c_ff_league_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                            const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                            const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                            float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                            int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream)
{
    const GradRequest g = league_grad(params, obs0, obs, actions, rewards, dones, hyper, order, offsets, learn,
                                      value_loss_kind, grad, losses, values_out, workspace, workspace_bytes, num_rows,
                                      num_steps, num_inputs, num_members, false, nullptr);
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_league_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                                const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                                float *returns_out)
{
    const GradRequest g = league_grad(params, obs0, obs, actions, rewards, dones, hyper, order, offsets, learn,
                                      value_loss_kind, grad, losses, values_out, workspace, workspace_bytes, num_rows,
                                      num_steps, num_inputs, num_members, true, returns_out);
    return run(&g, nullptr, stream);
}

int wurm_a2c_ff_league_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                             const double *hyper, const int64_t *offsets, const uint8_t *learn, int64_t step,
                             float beta1, float beta2, float eps, float max_grad_norm, int64_t num_params,
                             int64_t num_rows, int64_t num_members, void *stream)
{
    const ApplyRequest a = league_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, offsets, learn, step, beta1,
                                        beta2, eps, max_grad_norm, num_params, num_rows, num_members);
    return run(nullptr, &a, stream);
}

int wurm_a2c_ff_league_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                              const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                              const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                              float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                              int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                              float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                              float max_grad_norm, void *stream)
{
    const GradRequest g = league_grad(params, obs0, obs, actions, rewards, dones, hyper, order, offsets, learn,
                                      value_loss_kind, grad, losses, values_out, workspace, workspace_bytes, num_rows,
                                      num_steps, num_inputs, num_members, false, nullptr);
    const ApplyRequest a = league_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, offsets, learn, step, beta1,
                                        beta2, eps, max_grad_norm, a2c::num_params(num_inputs), num_rows, num_members);
    return run(&g, &a, stream);
}

int wurm_a2c_ff_league_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                                  const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                  const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                  float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                  int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members,
                                  float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                                  float beta2, float eps, float max_grad_norm, void *stream, float *returns_out)
{
    const GradRequest g = league_grad(params, obs0, obs, actions, rewards, dones, hyper, order, offsets, learn,
                                      value_loss_kind, grad, losses, values_out, workspace, workspace_bytes, num_rows,
                                      num_steps, num_inputs, num_members, true, returns_out);
    const ApplyRequest a = league_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, offsets, learn, step, beta1,
                                        beta2, eps, max_grad_norm, a2c::num_params(num_inputs), num_rows, num_members);
    return run(&g, &a, stream);
}

} // extern "C"
