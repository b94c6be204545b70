// a2c_learner.hip — C ABI of the fused A2C learner (kernels: a2c_learner.hpp; include/wurm_hip.h: wurm_a2c_ff_*).
// Every entry point validates its arguments before the first HIP call, so refusals work with no device present.
#include "a2c_learner.hpp"
#include "../../include/wurm_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <optional>

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

// What a member dimension can hold: the member is the grid's y, and a League's `order` is int32
bool within_limits(Kind kind, int64_t N, int64_t members)
{
    return members <= 65535 && (kind != Kind::League || N < (1LL << 31));
}

// The workspace: the partials of every workgroup, then the parked rows of all N columns.
// Alone: min(N, 256) partials.  Pop: every member's min(M, 256), member-major, and the parked rows member by member: each
// part is what a stand-alone update of M = N / members envs has, `members` times over.  League: a member has min(M_a, 256)
// partials behind those of the members before it, and the M_a sum to at most N: min(N, 256 members) serve any line-up (the
// host knows no more); the parked rows go by list position, and the grid is (min(N, 256), members) whatever the lists hold.
struct Layout {
    int64_t M;      // the envs the grid's x shares out: N, a member's N / members, or (League) at most N
    int G;          // the grid's x: min(M, 256)
    int64_t groups; // partials in all: the parked rows start behind them
    int64_t bytes;
};

// false: no such workspace (a size <= 0, or a population whose members do not divide N)
bool layout(Kind kind, int64_t N, int64_t T, int E, int64_t members, Layout *l)
{
    if (N <= 0 || T <= 0 || members <= 0 || (kind == Kind::Pop && N % members != 0)) return false;
    l->M = kind == Kind::Pop ? N / members : N;
    l->G = (int)(l->M < MAX_GROUPS ? l->M : MAX_GROUPS);
    l->groups = kind != Kind::League ? members * l->G : (N < MAX_GROUPS * members ? N : MAX_GROUPS * members);
    l->bytes = 4 * (l->groups * partial_stride(E) + N * (T + 1) * ROW_FLOATS);
    return true;
}

int64_t workspace_query(Kind kind, int64_t N, int64_t T, int E, int64_t members)
{
    Layout l;
    if (!supported_inputs(E) || !layout(kind, N, T, E, members, &l)) return 0;
    return kind == Kind::League && !within_limits(kind, N, members) ? 0 : l.bytes; // (Pop: the query has no limit)
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

// What every grad / update entry point takes, whatever its kind: the rollout window, the outputs and the workspace
struct Window {
    const float *params, *obs0, *obs;
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    int value_loss_kind;
    float *grad, *losses, *values_out; // values_out: nullable
    void *workspace;
    int64_t workspace_bytes, N, T;
    int E;
};
// ... taken from the entry point it expands in, under the names include/wurm_hip.h gives its parameters (the 14 listed,
// in the struct's order, and N: num_envs, or the League's num_rows): rename one in the header and this stops compiling
#define WINDOW(N)                                                                                                     \
    Window { params, obs0, obs, actions, rewards, dones, value_loss_kind, grad, losses, values_out, workspace,         \
             workspace_bytes, N, num_steps, num_inputs }

// What an entry point asks for, as its caller handed it over: kind, window and sets of weights, then what the kind adds,
// which the builders below assign by name (the rest stays zero)
struct GradRequest {
    Kind kind;
    Window w;
    int64_t members;     // sets of weights.  Pop: of N / members consecutive envs each
    bool gae;
    float *returns_out;  // GAE; nullable
    float gamma, entropy_coef, gamma_lambda; // Alone (gamma_lambda: GAE): Pop and League read a member's from `hyper`
    const double *hyper;                     // Pop, League
    const int32_t *order;                    // League: a member learns from the columns its piece of `order` names
    const int64_t *offsets;
    const uint8_t *learn; // nullable
};

GradRequest alone_grad(const Window &w, float gamma, float entropy_coef)
{
    GradRequest r = {Kind::Alone, w, 1};
    r.gamma = gamma;
    r.entropy_coef = entropy_coef;
    return r;
}

GradRequest pop_grad(const Window &w, const double *hyper, int64_t members)
{
    GradRequest r = {Kind::Pop, w, members};
    r.hyper = hyper;
    return r;
}

GradRequest league_grad(const Window &w, const double *hyper, const int32_t *order, const int64_t *offsets,
                        const uint8_t *learn, int64_t members)
{
    GradRequest r = pop_grad(w, hyper, members);
    r.kind = Kind::League;
    r.order = order;
    r.offsets = offsets;
    r.learn = learn;
    return r;
}

// the same request with generalised advantage estimation; gamma_lambda: Alone (a member's: wurm_a2c_ff_pop_hyper)
GradRequest with_gae(GradRequest r, float *returns_out, float gamma_lambda = 0.0f)
{
    r.gae = true;
    r.returns_out = returns_out;
    r.gamma_lambda = gamma_lambda;
    return r;
}

// What every apply / update entry point takes: the optimiser's state and constants
struct Adam {
    float *params;
    const float *grad;
    float *exp_avg, *exp_avg_sq, *grad_norm; // grad_norm: nullable
    int64_t step;
    float beta1, beta2, eps, max_grad_norm;
    int64_t num_params;
};
// ... likewise from the entry point's own parameters, in the struct's order; num_params: given, or that of num_inputs
#define ADAM(num_params) Adam{params, grad, exp_avg, exp_avg_sq, grad_norm, step, beta1, beta2, eps, max_grad_norm, num_params}

struct ApplyRequest {
    Kind kind;
    Adam s;
    int64_t members;
    float lr;               // Alone: a member's is in its row of `hyper`
    const double *hyper;    // Pop, League
    const int64_t *offsets; // League: who steps
    const uint8_t *learn;   // nullable
    int64_t rows;           // the N of the lists
};

ApplyRequest alone_apply(const Adam &s, float lr)
{
    ApplyRequest r = {Kind::Alone, s, 1};
    r.lr = lr;
    return r;
}

ApplyRequest pop_apply(const Adam &s, const double *hyper, int64_t members)
{
    ApplyRequest r = {Kind::Pop, s, members};
    r.hyper = hyper;
    return r;
}

ApplyRequest league_apply(const Adam &s, const double *hyper, const int64_t *offsets, const uint8_t *learn, int64_t rows,
                          int64_t members)
{
    ApplyRequest r = pop_apply(s, hyper, members);
    r.kind = Kind::League;
    r.offsets = offsets;
    r.learn = learn;
    r.rows = rows;
    return r;
}

// WURM_ERR_INVALID_ARG for an argument that is missing or out of range, then WURM_ERR_UNSUPPORTED for a shape the kernels
// do not have, then the size of the workspace: first what every kind asks, then what the request's own kind adds.
int check_grad(const GradRequest &r)
{
    const Window &w = r.w;
    if (!w.params || !w.obs0 || !w.obs || !w.actions || !w.rewards || !w.dones || !w.grad || !w.losses || !w.workspace)
        return WURM_ERR_INVALID_ARG;
    if (w.E <= 0 || w.workspace_bytes < 0) return WURM_ERR_INVALID_ARG;
    if ((uintptr_t)w.workspace % 16 != 0) return WURM_ERR_INVALID_ARG; // 16-byte accesses
    Layout l;
    if (!layout(r.kind, w.N, w.T, w.E, r.members, &l)) return WURM_ERR_INVALID_ARG;
    const bool supported =
        supported_inputs(w.E) && (w.value_loss_kind == WURM_A2C_SMOOTH_L1 || w.value_loss_kind == WURM_A2C_MSE);
    switch (r.kind) {
    case Kind::Alone:
        if (r.gae && !valid_gamma_lambda(r.gamma_lambda)) return WURM_ERR_INVALID_ARG;
        if (!supported) return WURM_ERR_UNSUPPORTED;
        break;
    case Kind::Pop:
        if (!r.hyper) return WURM_ERR_INVALID_ARG;
        if (!supported) return WURM_ERR_UNSUPPORTED;
        // what the stand-alone call refuses for a member's envs comes before the limit on the members
        if (w.workspace_bytes < l.bytes / r.members) return WURM_ERR_INVALID_ARG;
        if (!within_limits(r.kind, w.N, r.members)) return WURM_ERR_UNSUPPORTED;
        break;
    case Kind::League:
        if (!r.hyper || !r.order || !r.offsets) return WURM_ERR_INVALID_ARG;
        if (!supported || !within_limits(r.kind, w.N, r.members)) return WURM_ERR_UNSUPPORTED;
        break;
    }
    return w.workspace_bytes < l.bytes ? WURM_ERR_INVALID_ARG : WURM_OK;
}

int check_apply(const ApplyRequest &r)
{
    const Adam &s = r.s;
    if (!s.params || !s.grad || !s.exp_avg || !s.exp_avg_sq) return WURM_ERR_INVALID_ARG;
    if (s.step < 1 || s.num_params <= 0) return WURM_ERR_INVALID_ARG;
    if (!(s.beta1 >= 0.0f && s.beta1 < 1.0f) || !(s.beta2 >= 0.0f && s.beta2 < 1.0f) || !(s.eps >= 0.0f))
        return WURM_ERR_INVALID_ARG;
    if (r.kind == Kind::Alone) return r.lr >= 0.0f ? WURM_OK : WURM_ERR_INVALID_ARG; // (a member's lr: wurm_a2c_ff_pop_hyper)
    if (!r.hyper || r.members <= 0) return WURM_ERR_INVALID_ARG;                        // Pop, League
    if (r.kind == Kind::League && (!r.offsets || r.rows <= 0)) return WURM_ERR_INVALID_ARG;
    return within_limits(r.kind, r.rows, r.members) ? WURM_OK : WURM_ERR_UNSUPPORTED;
}

template <bool GAE, Kind K> void launch_grad(const GradRequest &r, hipStream_t stream)
{
    const Window &w = r.w;
    Layout l;
    layout(K, w.N, w.T, w.E, r.members, &l); // (check_grad has seen it exist)
    typename kernel_args<GAE, K>::type a = {};
    a.params = w.params;
    a.obs0 = w.obs0;
    a.obs = w.obs;
    a.actions = (const long long *)w.actions;
    a.rewards = w.rewards;
    a.dones = w.dones;
    a.values_out = w.values_out;
    a.partials = (float *)w.workspace;
    a.G = l.G;
    a.rows = a.partials + l.groups * partial_stride(w.E);
    a.N = w.N;
    a.T = w.T;
    a.E = w.E;
    a.loss_kind = w.value_loss_kind;
    a.inv_B = 1.0f / (float)(l.M * w.T); // (League: every member's own, formed on the device)
    if constexpr (GAE) a.returns_out = r.returns_out;
    if constexpr (K == Kind::Pop) {
        a.M = l.M;
        a.hyper = r.hyper;
    } else if constexpr (K == Kind::League) {
        a.hyper = r.hyper;
        a.order = r.order;
        a.offsets = (const long long *)r.offsets;
        a.learn = r.learn;
    } else {
        a.gamma = r.gamma;
        a.entropy_coef = r.entropy_coef;
        if constexpr (GAE) a.gamma_lambda = r.gamma_lambda;
    }
    const dim3 main_grid((unsigned)a.G, (unsigned)r.members);
    WURM_LAUNCH((a2c_ff_main_kernel<GAE, K>), main_grid, dim3(THREADS), 0, stream, a);
    const long long P = num_params(w.E);
    const dim3 grid((unsigned)((P + 3 + THREADS - 1) / THREADS), (unsigned)r.members);
    if constexpr (K == Kind::League)
        WURM_LAUNCH(a2c_ff_reduce_league_kernel, grid, dim3(THREADS), 0, stream, a.partials, a.offsets, a.learn, a.N, a.T,
                    w.E, w.grad, w.losses);
    else
        WURM_LAUNCH(K == Kind::Pop ? a2c_ff_reduce_pop_kernel : a2c_ff_reduce_kernel, grid, dim3(THREADS), 0, stream,
                    a.partials, a.G, w.E, a.inv_B, w.grad, w.losses);
}

// step_size = lr / (1 - beta1^step), divided in double and rounded once: here for the stand-alone kernel, by the
// population and League kernels themselves from bc1 and the member's lr
void launch_apply(const ApplyRequest &r, hipStream_t stream)
{
    const Adam &s = r.s;
    const double b1 = as_written(s.beta1), b2 = as_written(s.beta2);
    const double bc1 = 1.0 - std::pow(b1, (double)s.step);
    const float bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)s.step));
    const float w1 = (float)(1.0 - b1), w2 = (float)(1.0 - b2), eps = (float)as_written(s.eps);
    const dim3 grid((unsigned)((s.num_params + APPLY_PER_BLOCK - 1) / APPLY_PER_BLOCK), (unsigned)r.members);
    if (r.kind == Kind::League)
        WURM_LAUNCH(a2c_ff_apply_league_kernel, grid, dim3(THREADS), 0, stream, s.params, s.grad, s.exp_avg, s.exp_avg_sq,
                    s.grad_norm, r.hyper, (const long long *)r.offsets, r.learn, (long long)r.rows, bc1, bc2_sqrt,
                    (float)b2, w1, w2, eps, s.max_grad_norm, (long long)s.num_params);
    else if (r.kind == Kind::Pop)
        WURM_LAUNCH(a2c_ff_apply_pop_kernel, grid, dim3(THREADS), 0, stream, s.params, s.grad, s.exp_avg, s.exp_avg_sq,
                    s.grad_norm, r.hyper, bc1, bc2_sqrt, (float)b2, w1, w2, eps, s.max_grad_norm, (long long)s.num_params);
    else
        WURM_LAUNCH(a2c_ff_apply_kernel, grid, dim3(THREADS), 0, stream, s.params, s.grad, s.exp_avg, s.exp_avg_sq,
                    s.grad_norm, (float)(as_written(r.lr) / bc1), bc2_sqrt, (float)b2, w1, w2, eps, s.max_grad_norm,
                    (long long)s.num_params);
}

// grad (g), apply (a) or update (both): every check of the grad half, then every check of the apply half, then the launches
int run(std::optional<GradRequest> g, std::optional<ApplyRequest> a, void *stream)
{
    int rc = g ? check_grad(*g) : WURM_OK;
    if (rc == WURM_OK && a) rc = check_apply(*a);
    if (rc != WURM_OK) return rc;
    (void)hipGetLastError();
    if (g) {
        constexpr Kind A = Kind::Alone, P = Kind::Pop, L = Kind::League;
        auto *launch = g->kind == L   ? (g->gae ? launch_grad<true, L> : launch_grad<false, L>)
                       : g->kind == P ? (g->gae ? launch_grad<true, P> : launch_grad<false, P>)
                                      : (g->gae ? launch_grad<true, A> : launch_grad<false, A>);
        launch(*g, (hipStream_t)stream);
    }
    if (a) launch_apply(*a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace

extern "C" {

int64_t wurm_a2c_ff_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs)
{
    return workspace_query(Kind::Alone, num_envs, num_steps, num_inputs, 1);
}

int wurm_a2c_ff_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                     const float *rewards, const uint8_t *dones, float gamma, float entropy_coef, int value_loss_kind,
                     float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                     int64_t num_envs, int64_t num_steps, int num_inputs, void *stream)
{
    return run(alone_grad(WINDOW(num_envs), gamma, entropy_coef), {}, stream);
}

int wurm_a2c_ff_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                         const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                         int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                         int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs, void *stream,
                         float gamma_lambda, float *returns_out)
{
    return run(with_gae(alone_grad(WINDOW(num_envs), gamma, entropy_coef), returns_out, gamma_lambda), {}, stream);
}

int wurm_a2c_ff_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                      int64_t step, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                      int64_t num_params, void *stream)
{
    return run({}, alone_apply(ADAM(num_params), lr), stream);
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
    return run(alone_grad(WINDOW(num_envs), gamma, entropy_coef), alone_apply(ADAM(a2c::num_params(num_inputs)), lr),
               stream);
}

int wurm_a2c_ff_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, float gamma, float entropy_coef,
                           int value_loss_kind, float *grad, float *losses, float *values_out, void *workspace,
                           int64_t workspace_bytes, int64_t num_envs, int64_t num_steps, int num_inputs,
                           float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float lr, float beta1,
                           float beta2, float eps, float max_grad_norm, void *stream, float gamma_lambda,
                           float *returns_out)
{
    return run(with_gae(alone_grad(WINDOW(num_envs), gamma, entropy_coef), returns_out, gamma_lambda),
               alone_apply(ADAM(a2c::num_params(num_inputs)), lr), stream);
}

int64_t wurm_a2c_ff_pop_workspace_bytes(int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members)
{
    return workspace_query(Kind::Pop, num_envs, num_steps, num_inputs, num_members);
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
    return run(pop_grad(WINDOW(num_envs), hyper, num_members), {}, stream);
}

int wurm_a2c_ff_pop_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                             const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                             float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                             int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                             float *returns_out)
{
    return run(with_gae(pop_grad(WINDOW(num_envs), hyper, num_members), returns_out), {}, stream);
}

int wurm_a2c_ff_pop_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                          const double *hyper, int64_t step, float beta1, float beta2, float eps, float max_grad_norm,
                          int64_t num_params, int64_t num_members, void *stream)
{
    return run({}, pop_apply(ADAM(num_params), hyper, num_members), stream);
}

int wurm_a2c_ff_pop_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                           const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                           float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                           int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                           float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                           float max_grad_norm, void *stream)
{
    return run(pop_grad(WINDOW(num_envs), hyper, num_members),
               pop_apply(ADAM(a2c::num_params(num_inputs)), hyper, num_members), stream);
}

int wurm_a2c_ff_pop_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                               const float *rewards, const uint8_t *dones, const double *hyper, int value_loss_kind,
                               float *grad, float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                               int64_t num_envs, int64_t num_steps, int num_inputs, int64_t num_members,
                               float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                               float beta2, float eps, float max_grad_norm, void *stream, float *returns_out)
{
    return run(with_gae(pop_grad(WINDOW(num_envs), hyper, num_members), returns_out),
               pop_apply(ADAM(a2c::num_params(num_inputs)), hyper, num_members), stream);
}

int64_t wurm_a2c_ff_league_workspace_bytes(int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members)
{
    return workspace_query(Kind::League, num_rows, num_steps, num_inputs, num_members);
}

int wurm_a2c_ff_league_grad(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                            const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                            const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                            float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                            int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream)
{
    return run(league_grad(WINDOW(num_rows), hyper, order, offsets, learn, num_members), {}, stream);
}

int wurm_a2c_ff_league_grad_gae(const float *params, const float *obs0, const float *obs, const int64_t *actions,
                                const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, void *stream,
                                float *returns_out)
{
    return run(with_gae(league_grad(WINDOW(num_rows), hyper, order, offsets, learn, num_members), returns_out), {}, stream);
}

int wurm_a2c_ff_league_apply(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float *grad_norm,
                             const double *hyper, const int64_t *offsets, const uint8_t *learn, int64_t step,
                             float beta1, float beta2, float eps, float max_grad_norm, int64_t num_params,
                             int64_t num_rows, int64_t num_members, void *stream)
{
    return run({}, league_apply(ADAM(num_params), hyper, offsets, learn, num_rows, num_members), stream);
}

int wurm_a2c_ff_league_update(float *params, const float *obs0, const float *obs, const int64_t *actions,
                              const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                              const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                              float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                              int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members, float *exp_avg,
                              float *exp_avg_sq, float *grad_norm, int64_t step, float beta1, float beta2, float eps,
                              float max_grad_norm, void *stream)
{
    return run(league_grad(WINDOW(num_rows), hyper, order, offsets, learn, num_members),
               league_apply(ADAM(a2c::num_params(num_inputs)), hyper, offsets, learn, num_rows, num_members), stream);
}

int wurm_a2c_ff_league_update_gae(float *params, const float *obs0, const float *obs, const int64_t *actions,
                                  const float *rewards, const uint8_t *dones, const double *hyper, const int32_t *order,
                                  const int64_t *offsets, const uint8_t *learn, int value_loss_kind, float *grad,
                                  float *losses, float *values_out, void *workspace, int64_t workspace_bytes,
                                  int64_t num_rows, int64_t num_steps, int num_inputs, int64_t num_members,
                                  float *exp_avg, float *exp_avg_sq, float *grad_norm, int64_t step, float beta1,
                                  float beta2, float eps, float max_grad_norm, void *stream, float *returns_out)
{
    return run(with_gae(league_grad(WINDOW(num_rows), hyper, order, offsets, learn, num_members), returns_out),
               league_apply(ADAM(a2c::num_params(num_inputs)), hyper, offsets, learn, num_rows, num_members), stream);
}

} // extern "C"
