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

int check_grad_args(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                    const float *rewards, const uint8_t *dones, int value_loss_kind, float *grad, float *losses,
                    void *workspace, int64_t workspace_bytes_given, int64_t N, int64_t T, int E)
{
    if (!params || !obs0 || !obs || !actions || !rewards || !dones || !grad || !losses || !workspace)
        return WURM_ERR_INVALID_ARG;
    if (N <= 0 || T <= 0 || E <= 0 || workspace_bytes_given < 0) return WURM_ERR_INVALID_ARG;
    if ((uintptr_t)workspace % 16 != 0) return WURM_ERR_INVALID_ARG; // 16-byte accesses
    if (!supported_inputs(E)) return WURM_ERR_UNSUPPORTED;
    if (value_loss_kind != WURM_A2C_SMOOTH_L1 && value_loss_kind != WURM_A2C_MSE) return WURM_ERR_UNSUPPORTED;
    if (workspace_bytes_given < workspace_bytes(N, T, E)) return WURM_ERR_INVALID_ARG;
    return WURM_OK;
}

int check_apply_args(const float *params, const float *grad, const float *exp_avg, const float *exp_avg_sq,
                     int64_t step, float lr, float beta1, float beta2, float eps, int64_t P)
{
    if (!params || !grad || !exp_avg || !exp_avg_sq) return WURM_ERR_INVALID_ARG;
    if (step < 1 || P <= 0) return WURM_ERR_INVALID_ARG;
    if (!(lr >= 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f))
        return WURM_ERR_INVALID_ARG;
    return WURM_OK;
}

// gamma * lambda as the caller rounded it: finite and not negative (refused like the other arguments, before any launch)
bool valid_gamma_lambda(float gamma_lambda) { return std::isfinite(gamma_lambda) && gamma_lambda >= 0.0f; }

template <bool GAE>
void launch_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                 const float *rewards, const uint8_t *dones, float gamma, float entropy_coef, int value_loss_kind,
                 float *grad, float *losses, float *values_out, void *workspace, int64_t N, int64_t T, int E,
                 hipStream_t stream, float gamma_lambda = 0.0f, float *returns_out = nullptr)
{
    typename main_args<GAE>::type a;
    a.params = params;
    a.obs0 = obs0;
    a.obs = obs;
    a.actions = (const long long *)actions;
    a.rewards = rewards;
    a.dones = dones;
    a.values_out = values_out;
    a.partials = (float *)workspace;
    a.G = num_groups(N);
    a.rows = a.partials + a.G * partial_stride(E);
    a.N = N;
    a.T = T;
    a.E = E;
    a.loss_kind = value_loss_kind;
    a.gamma = gamma;
    a.entropy_coef = entropy_coef;
    a.inv_B = 1.0f / (float)(N * T);
    if constexpr (GAE) {
        a.gamma_lambda = gamma_lambda;
        a.returns_out = returns_out;
    }
    WURM_LAUNCH(a2c_ff_main_kernel<GAE>, dim3((unsigned)a.G), dim3(THREADS), 0, stream, a);
    const long long P = num_params(E);
    WURM_LAUNCH(a2c_ff_reduce_kernel, dim3((unsigned)((P + 3 + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                a.partials, a.G, E, a.inv_B, grad, losses);
}

void launch_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step,
                  float lr, float beta1, float beta2, float eps, float max_grad_norm, int64_t P, hipStream_t stream)
{
    const double b1 = as_written(beta1), b2 = as_written(beta2);
    const float step_size = (float)(as_written(lr) / (1.0 - std::pow(b1, (double)step)));
    const float bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)step));
    WURM_LAUNCH(a2c_ff_apply_kernel, dim3((unsigned)((P + APPLY_PER_BLOCK - 1) / APPLY_PER_BLOCK)), dim3(THREADS), 0,
                stream, params, grad, exp_avg, exp_avg_sq, grad_norm, step_size, bc2_sqrt, (float)b2,
                (float)(1.0 - b1), (float)(1.0 - b2), (float)as_written(eps), max_grad_norm, (long long)P);
}

// ---- population: P members of M = N / P consecutive envs each (a2c_learner.hpp: a2c_ff_*_pop_kernel)

int check_pop_grad_args(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                        const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                        float *grad, float *losses, void *workspace, int64_t workspace_bytes_given, int64_t N, int64_t T,
                        int E, int64_t members)
{
    if (!hyper || members <= 0 || N <= 0 || N % members != 0) return WURM_ERR_INVALID_ARG;
    const int rc = check_grad_args(params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, workspace,
                                   workspace_bytes_given, N / members, T, E);
    if (rc != WURM_OK) return rc;
    if (members > 65535) return WURM_ERR_UNSUPPORTED; // the member is the grid's y
    if (workspace_bytes_given < members * workspace_bytes(N / members, T, E)) return WURM_ERR_INVALID_ARG;
    return WURM_OK;
}

int check_pop_apply_args(const float *params, const float *grad, const float *exp_avg, const float *exp_avg_sq,
                         const double *hyper, int64_t step, float beta1, float beta2, float eps, int64_t P,
                         int64_t members)
{
    if (!hyper || members <= 0) return WURM_ERR_INVALID_ARG;
    const int rc = check_apply_args(params, grad, exp_avg, exp_avg_sq, step, 0.0f, beta1, beta2, eps, P);
    if (rc != WURM_OK) return rc;
    return members > 65535 ? WURM_ERR_UNSUPPORTED : WURM_OK;
}

// the workspace holds every member's partials (member-major), then every member's parked rows: each part is what a
// stand-alone update of M envs has, P times over
template <bool GAE>
void launch_pop_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                     const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind, float *grad,
                     float *losses, float *values_out, void *workspace, int64_t N, int64_t T, int E, int64_t members,
                     hipStream_t stream, float *returns_out = nullptr)
{
    const int64_t M = N / members;
    typename kernel_args<GAE, true>::type a = {};
    a.params = params;
    a.obs0 = obs0;
    a.obs = obs;
    a.actions = (const long long *)actions;
    a.rewards = rewards;
    a.dones = dones;
    a.values_out = values_out;
    a.partials = (float *)workspace;
    a.G = num_groups(M);
    a.rows = a.partials + members * a.G * partial_stride(E);
    a.N = N;
    a.M = M;
    a.T = T;
    a.E = E;
    a.loss_kind = value_loss_kind;
    a.inv_B = 1.0f / (float)(M * T);
    if constexpr (GAE) a.returns_out = returns_out;
    a.hyper = hyper;
    WURM_LAUNCH((a2c_ff_main_kernel<GAE, true>), dim3((unsigned)a.G, (unsigned)members), dim3(THREADS), 0, stream, a);
    const long long P = num_params(E);
    WURM_LAUNCH(a2c_ff_reduce_pop_kernel, dim3((unsigned)((P + 3 + THREADS - 1) / THREADS), (unsigned)members),
                dim3(THREADS), 0, stream, a.partials, a.G, E, a.inv_B, grad, losses);
}

void launch_pop_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                      const double *hyper, int64_t step, float beta1, float beta2, float eps, float max_grad_norm,
                      int64_t P, int64_t members, hipStream_t stream)
{
    const double b1 = as_written(beta1), b2 = as_written(beta2);
    const double bc1 = 1.0 - std::pow(b1, (double)step); // (launch_apply divides lr by this; here the kernel does)
    const float bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)step));
    WURM_LAUNCH(a2c_ff_apply_pop_kernel,
                dim3((unsigned)((P + APPLY_PER_BLOCK - 1) / APPLY_PER_BLOCK), (unsigned)members), dim3(THREADS), 0,
                stream, params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, bc1, bc2_sqrt, (float)b2,
                (float)(1.0 - b1), (float)(1.0 - b2), (float)as_written(eps), max_grad_norm, (long long)P);
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
    const int rc = check_grad_args(params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, workspace,
                                   workspace_bytes, num_envs, num_steps, num_inputs);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_grad<false>(params, obs0, obs, actions, rewards, dones, gamma, entropy_coef, value_loss_kind, grad, losses,
                       values_out, workspace, num_envs, num_steps, num_inputs, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                         int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                         int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, void *stream,
                         float gamma_lambda, float *returns_out)
{
    if (!valid_gamma_lambda(gamma_lambda)) return WURM_ERR_INVALID_ARG;
    const int rc = check_grad_args(params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, workspace,
                                   workspace_bytes, num_envs, num_steps, num_inputs);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_grad<true>(params, obs0, obs, actions, rewards, dones, gamma, entropy_coef, value_loss_kind, grad, losses,
                      values_out, workspace, num_envs, num_steps, num_inputs, (hipStream_t)stream, gamma_lambda,
                      returns_out);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                      int64_t step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                      int64_t num_params, void *stream)
{
    const int rc = check_apply_args(params, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, num_params);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, step, lr, beta1, beta2, eps, max_grad_norm, num_params,
                 (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
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
    int rc = check_grad_args(params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, workspace,
                             workspace_bytes, num_envs, num_steps, num_inputs);
    if (rc != WURM_OK) return rc;
    const int64_t P = a2c::num_params(num_inputs);
    rc = check_apply_args(params, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, P);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_grad<false>(params, obs0, obs, actions, rewards, dones, gamma, entropy_coef, value_loss_kind, grad, losses,
                       values_out, workspace, num_envs, num_steps, num_inputs, (hipStream_t)stream);
    launch_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, step, lr, beta1, beta2, eps, max_grad_norm, P,
                 (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                           int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                           int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs,
                           float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1,
                           float beta2, float eps, float max_grad_norm, void *stream, float gamma_lambda,
                           float *returns_out)
{
    if (!valid_gamma_lambda(gamma_lambda)) return WURM_ERR_INVALID_ARG;
    int rc = check_grad_args(params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, workspace,
                             workspace_bytes, num_envs, num_steps, num_inputs);
    if (rc != WURM_OK) return rc;
    const int64_t P = a2c::num_params(num_inputs);
    rc = check_apply_args(params, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, P);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_grad<true>(params, obs0, obs, actions, rewards, dones, gamma, entropy_coef, value_loss_kind, grad, losses,
                      values_out, workspace, num_envs, num_steps, num_inputs, (hipStream_t)stream, gamma_lambda,
                      returns_out);
    launch_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, step, lr, beta1, beta2, eps, max_grad_norm, P,
                 (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
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
        if (!(lr[m] >= 0.0f)) return WURM_ERR_INVALID_ARG; // (what check_apply_args asks of a stand-alone lr)
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
    const int rc = check_pop_grad_args(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses,
                                       workspace, workspace_bytes, num_envs, num_steps, num_inputs, num_members);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_pop_grad<false>(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses, values_out,
                           workspace, num_envs, num_steps, num_inputs, num_members, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_pop_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                             const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                             float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                             int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                             float *returns_out)
{
    const int rc = check_pop_grad_args(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses,
                                       workspace, workspace_bytes, num_envs, num_steps, num_inputs, num_members);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_pop_grad<true>(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses, values_out,
                          workspace, num_envs, num_steps, num_inputs, num_members, (hipStream_t)stream, returns_out);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_pop_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                          const double *hyper, int64_t step, float beta1, float beta2, float eps, float max_grad_norm,
                          int64_t num_params, int64_t num_members, void *stream)
{
    const int rc = check_pop_apply_args(params, grad, exp_avg, exp_avg_sq, hyper, step, beta1, beta2, eps, num_params,
                                        num_members);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_pop_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, step, beta1, beta2, eps, max_grad_norm,
                     num_params, num_members, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_pop_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                           float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                           int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                           float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                           float max_grad_norm, void *stream)
{
    int rc = check_pop_grad_args(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses,
                                 workspace, workspace_bytes, num_envs, num_steps, num_inputs, num_members);
    if (rc != WURM_OK) return rc;
    const int64_t P = a2c::num_params(num_inputs);
    rc = check_pop_apply_args(params, grad, exp_avg, exp_avg_sq, hyper, step, beta1, beta2, eps, P, num_members);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_pop_grad<false>(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses, values_out,
                           workspace, num_envs, num_steps, num_inputs, num_members, (hipStream_t)stream);
    launch_pop_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, step, beta1, beta2, eps, max_grad_norm, P,
                     num_members, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_a2c_ff_pop_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                               const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                               float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                               int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members,
                               float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                               float beta2, float eps, float max_grad_norm, void *stream, float *returns_out)
{
    int rc = check_pop_grad_args(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses,
                                 workspace, workspace_bytes, num_envs, num_steps, num_inputs, num_members);
    if (rc != WURM_OK) return rc;
    const int64_t P = a2c::num_params(num_inputs);
    rc = check_pop_apply_args(params, grad, exp_avg, exp_avg_sq, hyper, step, beta1, beta2, eps, P, num_members);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    launch_pop_grad<true>(params, obs0, obs, actions, rewards, dones, hyper, value_loss_kind, grad, losses, values_out,
                          workspace, num_envs, num_steps, num_inputs, num_members, (hipStream_t)stream, returns_out);
    launch_pop_apply(params, grad, exp_avg, exp_avg_sq, grad_norm, hyper, step, beta1, beta2, eps, max_grad_norm, P,
                     num_members, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
