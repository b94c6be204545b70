// multi_policy_window.hpp — MultiSnake.policy_window: the reference's multi-agent acting loop (experiments/multiagent.py:
// 350-378; here MultiSnake.act_window, two launches per step) as ONE launch (include/wurm_hip.h: wurm_multi_policy_window).
//
// Per env (= per wave) and per step t, with the env resident in LDS as in multi_rollout_kernel:
//   1. probs, value, action of the env's K snakes from the K crops in the wave's LDS input buffers: PolicyWide's first
//      layer over the (input pair, unit) float2s of the snake's species, PolicyHead for the rest (the shared policy spec:
//      oracle/policy.c), the draw u01(Philox(seed; (env_offset + env) K + k, policy_call0 + t, RNG_POLICY).w0);
//   2. multi_step_body with the actions AS SAMPLED (it sanitises them itself), counter call0 + 2 t;
//   3. observe_partial — the crops of the stepped, not yet reset env — INTO the input buffers (its `obs` argument is the
//      generic address of that LDS: an argument block of its own with N = 1 and EP floats per agent), from where they are
//      copied to the window's `observations` and read by step t + 1;
//   4. rebase_clocks / reroll_colour / multi_reset_grid with counter call0 + 2 t + 1: reset(dones['__all__']).
// Every piece but the loop itself is the code the other kernels run: nothing of the transition, the reset, the crop or the
// policy arithmetic is written here.  A reset(done) the caller postponed in front of the window is applied before step 0 as
// multi_step_kernel's step_middle applies it (pre_done / pre_call); the reset of the last step is applied in the launch, so
// the env's tensors are the state after the window.
//
// Weights.  Snake k acts with species k P / K.  W1 of a species is 256 EP bytes (EP = E rounded up to 16: 8 / 20 / 40 KB for
// partial_0..1 / 2 / 3); everything else of a species, PolicyHead, is 76 registers of a lane.
//   * RESIDENT (P <= 4 and the P W1 blocks fit beside at least one env): the workgroup copies the P blocks into LDS once,
//     every wave loads the P heads into registers once — NS = 1, 2 or 4 PolicyWide objects picked by a wave-uniform
//     branch, never indexed — and a step reads no weight from memory.  __launch_bounds__(256): a wave may take the 512
//     registers of a SIMD it has to itself (4 heads: 304).
//   * RELOAD (anything else the domain allows: P > 4, or partial_3 with P = 4): one env per workgroup, ONE W1 slot and one
//     head; the wave copies a species' block and loads its head whenever the species changes from one snake to the next
//     (P times per step).  Correct for any K and P <= K; slow, and said so in DESIGN.md §4.2.
// LDS per workgroup: slots * 256 EP + wpb * (multi_layout + 4 (K EP + 64)) bytes.
// No atomics, no grid-wide barrier; the only workgroup barrier is the one behind the W1 copy.
#pragma once

#include "multi_step.hpp"
#include "policy_wide.hpp"

namespace wurm {

constexpr int MPW_MAX_OBS_N = 3;     // E = 3 (2n+1)^2 <= 147
constexpr int MPW_MAX_HEADS = 4;     // species whose heads a wave keeps in registers
constexpr int MPW_MAX_WAVES = 4;     // envs per workgroup
constexpr int MPW_LDS_MAX_BYTES = 160 * 1024;

struct MultiPolicyWindowArgs {
    // the launch as multi_rollout_kernel would see it: the state tensors, N, K, S, T, cfg, seed, call, env_offset, obs_mode
    // = partial, obs_n, the offsets of multi_layout with lds_per_wave = wave_bytes; done_env / pre_call: the postponed reset
    MultiArgs m;
    const float *params;  // (P, policy_num_params(E))
    const float *obs0;    // (K, N, E): what the policy acts on at step 0
    long long *actions;   // (T, K N) as sampled
    float *probs, *values; // (T, K N, 4), (T, K N)
    float *obs;           // (T, K N, E)
    float *rewards, *food, *sizes;                      // (T, K N)
    uint8_t *dones, *boost, *snakecol, *edgecol;        // (T, K N)
    uint8_t *all_done;    // (T, N)
    u64 pcall;            // the policy call counter of step 0
    int P, E, EP;
    int wpb, reload;      // envs per workgroup; RELOAD form (wpb == 1)
    int w1_bytes, env_bytes; // LDS in front of the waves' blocks; an env's own part of its wave's block
};

struct MultiPolicyWindowPlan {
    int ns;       // heads in registers (1, 2, 4); 0: not served
    int reload, wpb, w1_bytes, env_bytes, wave_bytes, lds;
};

// (fills in m's LDS offsets) waves_per_group: 0 = by batch size
inline MultiPolicyWindowPlan multi_policy_window_plan(MultiArgs &m, int P, int obs_n, int waves_per_group)
{
    MultiPolicyWindowPlan pl = {};
    const int W = 2 * obs_n + 1, E = 3 * W * W, EP = (E + 15) & ~15;
    pl.env_bytes = multi_layout(m, true, 0);
    pl.wave_bytes = pl.env_bytes + 4 * (m.K * EP + 64);
    const int w1 = 256 * EP;
    const bool resident = P <= MPW_MAX_HEADS && (long long)P * w1 + pl.wave_bytes <= MPW_LDS_MAX_BYTES;
    pl.reload = !resident;
    pl.w1_bytes = resident ? P * w1 : w1;
    if (pl.w1_bytes + pl.wave_bytes > MPW_LDS_MAX_BYTES) return pl; // (ns == 0)
    pl.ns = resident ? (P <= 1 ? 1 : P <= 2 ? 2 : 4) : 1;
    const int fit = (MPW_LDS_MAX_BYTES - pl.w1_bytes) / pl.wave_bytes;
    // as many envs per workgroup as fit (each workgroup copies the W1 blocks once), but no fewer workgroups than CUs
    const long long per_cu = (m.N + 255) / 256;
    long long wpb = waves_per_group > 0 ? waves_per_group : per_cu;
    wpb = std::max(1ll, std::min({wpb, (long long)fit, (long long)MPW_MAX_WAVES}));
    pl.wpb = resident ? (int)wpb : 1;
    pl.lds = pl.w1_bytes + pl.wpb * pl.wave_bytes;
    m.lds_per_wave = pl.wave_bytes;
    return pl;
}

// W1 (64, E) of one species -> LDS as policy_wide.hpp lays it out: (EP / 2, 64) pairs, zero padded, input k of unit j at
// float 128 (k / 2) + 2 j + (k & 1).  By the nth threads tid, tid + nth, ...
__device__ __forceinline__ void mpw_copy_w1(float *w1f, const float *__restrict__ W1, int E, int EP, int tid, int nth)
{
    const int n = 64 * E, pad = EP - E;
#pragma unroll 4
    for (int i = tid; i < n; i += nth) {
        const int j = i / E, k = i - j * E;
        w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = W1[i];
    }
    for (int i = tid; i < 64 * pad; i += nth) {
        const int j = i / pad, k = E + (i - j * pad);
        w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = 0.0f;
    }
}

template <int NS>
__global__ __launch_bounds__(64 * MPW_MAX_WAVES) void multi_policy_window_kernel(MultiPolicyWindowArgs a)
{
    typedef PolicyHead::f2 f2;
    const MultiArgs p = kernel_args<false, WURM_OBS_PARTIAL, 0, 0, -1>(a.m, false);
    const int E = a.E, EP = a.EP, P = a.P;
    const long long nparams = policy_num_params(E);
    float *const w1f = (float *)wurm_multi_lds;
    const bool reload = NS == 1 && a.reload != 0;
    if (!reload) {
        for (int s = 0; s < P; ++s)
            mpw_copy_w1(w1f + (size_t)s * 64 * EP, a.params + s * nparams, E, EP, (int)threadIdx.x, (int)blockDim.x);
        __syncthreads();
    }
    const int wave = uniform((int)(threadIdx.x >> 6));
    const long long env = xcd_block(blockIdx.x, gridDim.x) * a.wpb + wave;
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, wave, a.w1_bytes, true);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    float *const x = (float *)(wurm_multi_lds + a.w1_bytes + (size_t)wave * p.lds_per_wave + a.env_bytes), *const h1 = x + K * EP;
    const bool snake = lane < K;
    const u64 env_id = (u64)(p.env_offset + env);
    const long long agent = env * K + lane, KN = (long long)K * p.N;
    float *foodp = p.foods + env * C, *headp = p.heads + env * K * C, *bodyp = p.bodies + env * K * C;

    // the policy input of step 0, zero padded (the padding is never written again)
    for (int k = 0; k < K; ++k)
        for (int i = lane; i < EP; i += 64) x[k * EP + i] = i < E ? a.obs0[((long long)k * p.N + env) * E + i] : 0.0f;

    PolicyWide pol[NS];
    if (!reload) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sp = min(s, P - 1);
            pol[s].load(a.params + sp * nparams, E, EP, lane, (const f2 *)(w1f + (size_t)sp * 64 * EP), x);
        }
    }
    int cur = -1; // RELOAD: the species in the slot
    for (int s = 0; s < NS; ++s) pol[s].h1 = h1;

    // the env, and in front of it the reset(done) the caller postponed (multi_step_kernel / step_middle)
    const bool rebuild0 = p.done_env != nullptr && uniform((int)p.done_env[env]) != 0;
    u64 fbits0 = 0;
    if (!rebuild0) fbits0 = load_env(cx, foodp, headp, bodyp);
    else {
        clear_snake_slots(cx, lane);
        wave_lds_sync();
    }
    Snake sn;
    sn.hc = snake ? cx.hcell[lane] : -1;
    sn.L = snake ? cx.lmax[lane] : 0;
    sn.done = snake ? p.dones[agent] != 0 : true;
    sn.orient = snake ? p.orientations[agent] : 0;
    sn.boosted = false;
    load_colour(p, agent, snake, sn);
    bool col_dirty = false;
    const int hc0 = sn.hc; // what HBM holds: for the sparse write-back at the end
    if (p.done_env != nullptr) {
        if (rebuild0) sn.done = false; // :798
        if (snake) col_dirty |= reroll_colour(p, agent, sn.done, env_id, p.pre_call, 0, sn);
        const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
        if (rebuild0 || respawn) {
            bool orient_dirty = false;
            multi_reset_grid(cx, p, env, env_id, p.pre_call, rebuild0, respawn, sn, orient_dirty, 0, 0);
        }
    }
    WURM_TLS_INIT(cx);

    // observe_partial's view of the input buffers: "env 0" of a batch of one, EP floats from one agent to the next
    MultiArgs po = p;
    po.N = 1;
    po.obs_elems = EP;

    for (long long t = 0; t < p.T; ++t) {
        const u64 call = p.call + 2ull * (u64)t;
        const long long row0 = t * KN + env; // row of snake 0: column k N + env of step t
        const float my_u = snake ? u01(rng_words(p.seed, a.pcall + (u64)t, env_id * (u64)K + (u64)lane, RNG_POLICY, 0).w[0]) : 0.0f;
        long long act_mine = 0;
        for (int k = 0; k < K; ++k) {
            const int s = k * P / K;
            const float u = __int_as_float(lane_value(__float_as_int(my_u), k));
            float *const xk = x + k * EP;
            float p0, p1, p2, p3, value;
            int act;
            if (reload) {
                if (s != cur) { // (one env per workgroup: the slot is this wave's own)
                    wave_lds_sync();
                    mpw_copy_w1(w1f, a.params + s * nparams, E, EP, lane, 64);
                    pol[0].load(a.params + s * nparams, E, EP, lane, (const f2 *)w1f, xk);
                    pol[0].h1 = h1;
                    cur = s;
                }
                pol[0].x = xk;
                act = pol[0].act(lane, u, p0, p1, p2, p3, value);
            } else if (NS > 3 && s == 3) {
                pol[NS > 3 ? 3 : 0].x = xk;
                act = pol[NS > 3 ? 3 : 0].act(lane, u, p0, p1, p2, p3, value);
            } else if (NS > 2 && s == 2) {
                pol[NS > 2 ? 2 : 0].x = xk;
                act = pol[NS > 2 ? 2 : 0].act(lane, u, p0, p1, p2, p3, value);
            } else if (NS > 1 && s == 1) {
                pol[NS > 1 ? 1 : 0].x = xk;
                act = pol[NS > 1 ? 1 : 0].act(lane, u, p0, p1, p2, p3, value);
            } else {
                pol[0].x = xk;
                act = pol[0].act(lane, u, p0, p1, p2, p3, value);
            }
            if (lane == k) act_mine = (long long)act;
            const long long row = row0 + (long long)k * p.N;
            if (lane == 0) {
                a.actions[row] = (long long)act;
                a.values[row] = value;
            }
            if (lane < 4) a.probs[4 * row + lane] = lane == 0 ? p0 : lane == 1 ? p1 : lane == 2 ? p2 : p3;
        }

        StepRes r;
        multi_step_body(cx, p, env, env_id, call, act_mine, sn, r, 0, 0, 0);
        // the crops of the stepped env: into LDS (generic stores; the wait makes them LDS's before the DS reads below — the
        // step's own outputs are stored behind it, so that it waits for nothing else), then out to the window's observations
        observe_partial(cx, po, x, 0, sn);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        wave_lds_sync();
        if (snake) {
            const long long row = row0 + (long long)lane * p.N;
            a.rewards[row] = r.reward;
            a.food[row] = r.foodcons;
            a.sizes[row] = (float)sn.L;
            a.dones[row] = (uint8_t)sn.done;
            a.boost[row] = (uint8_t)sn.boosted;
            a.snakecol[row] = (uint8_t)r.snakecol;
            a.edgecol[row] = (uint8_t)r.edgecol;
        }
        if (lane == 0) a.all_done[t * p.N + env] = (uint8_t)r.all_done;

        for (int k = 0; k < K; ++k) {
            float *const o = a.obs + (row0 + (long long)k * p.N) * E;
            for (int i = lane; i < E; i += 64) o[i] = x[k * EP + i];
        }
        rebase_clocks(cx);

        // reset(dones['__all__']) (:771-836), as multi_rollout_kernel applies it
        if (snake && sn.done) sn.L = 0;           // deleted snakes have an all-zero body
        const bool rebuild = r.all_done;
        if (rebuild) sn.done = false;             // :798
        if (snake) col_dirty |= reroll_colour(p, agent, sn.done, env_id, call + 1ull, 0, sn);
        const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
        if (rebuild || respawn) {
            bool orient_dirty = false;
            multi_reset_grid(cx, p, env, env_id, call + 1ull, rebuild, respawn, sn, orient_dirty, 0, 0);
        }
    }

    if (snake) {
        p.dones[agent] = (uint8_t)sn.done;
        p.orientations[agent] = sn.orient;
        if (p.boost_state) p.boost_state[agent] = (uint8_t)sn.boosted;
        if (col_dirty) store_colour(p, agent, sn);
        cx.hcell[lane] = sn.hc;
    }
    wave_lds_sync();
    // only what may differ from HBM (multi_rollout_kernel); an env the postponed reset rebuilt was not read: stored whole
    store_env(cx, foodp, headp, bodyp, fbits0, hc0, sn.hc, rebuild0);
}

} // namespace wurm
