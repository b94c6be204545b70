// policy_wide.hpp — the fused acting loop of policy_rollout.hpp for every configuration the reference's feed-forward
// experiment accepts (experiments/main.py:129-137: FeedforwardAgent(num_inputs = 4) for 'positions', 3 (2n+1)^2 for
// 'partial_n'):
//   SingleSnake      9 <= S <= 64, partial_n with 0 <= n <= 6 (E = 3 (2n+1)^2 <= 507) or positions (E = 4);
//   SimpleGridworld  5 <= S <= 64, positions (E = 4), the fixed start location.
//
// The loop is rollout_generic's (one env per wave, Env<CPL> at every cells-per-lane bucket, the scalar carry of `Fast`
// for snakes) with the action tape replaced by the policy: per step, probs / value / sampled action from the observation
// in the wave's LDS input buffer, then step, observation to HBM and to that buffer, reset on done.  The arithmetic is
// policy_rollout.hpp's spec (two interleaved fmaf chains per hidden unit, tree_sum5 heads, exp_spec softmax, inverse-CDF
// sampling with the RNG_POLICY draw of call0 + 2t), so the results are bit-identical to oracle/policy.c and, on the
// shapes both kernels serve, to policy_rollout_kernel / policy_rollout_s9_kernel.
//
// First-layer weights: W1 is 64 E floats (130 KB at E = 507), too many for registers beyond n = 3.  The workgroup
// copies it ONCE into LDS, shared by its waves, as (input pair, unit) float2s: lane j reads the pair of inputs
// (2i, 2i+1) of unit j at float2 index 64 i + j, so one ds_read_b64 per wave moves 32 consecutive lanes x 8 bytes =
// all 64 banks, conflict-free.  The input vector is read as broadcast ds_read_b128s.  Inputs are zero-padded to a
// multiple of 16 (weights and inputs both 0): fmaf(0, 0, acc) == acc except that -0 becomes +0, which the ReLU after
// the layer maps to the same +0.  W2 (64 x 64) stays in registers as in policy_rollout.hpp.
// LDS per workgroup = 256 EP + wpb (4 EP + 256 + S^2 rounded to 16) bytes (EP = E rounded up to 16; the S^2 bytes are
// write_obs's class map for crops on grids of more than 128 cells); wpb = waves per workgroup, as many as fit in 160 KiB
// (at most 8), fewer for small batches so that the workgroups still spread over the CUs.
#pragma once

#include <algorithm>

#include "policy_rollout.hpp"

namespace wurm {

struct PolicyWideArgs {
    PolicyArgs p;        // selfc == nullptr for SimpleGridworld
    int E, EP;           // observation size, and rounded up to 16
    int obs_mode, obs_n; // WURM_OBS_PARTIAL (SingleSnake) or WURM_OBS_POSITIONS
    int start_y, start_x;
    int wpb, wave_bytes; // waves per workgroup, LDS bytes per wave
};

// What the POP instantiations take (policy_rollout.hpp: PolicyPopArgs).  A workgroup copies W1 into LDS once for all its
// waves, so it must not hold envs of two members: the grid is wgpm = ceil(M / wpb) workgroups PER MEMBER, member-major,
// workgroup i of a member holds its envs [i wpb, (i + 1) wpb) and the waves past the member's last env leave — for any M,
// M = 1 and M prime included.
struct PolicyWidePopArgs : PolicyWideArgs {
    long long M;
    unsigned wgpm;
};

template <bool POP> struct policy_wide_args { using type = PolicyWideArgs; };
template <> struct policy_wide_args<true> { using type = PolicyWidePopArgs; };

// the policy of one wave with the first layer in LDS
struct PolicyWide : PolicyHead {
    const f2 *w1;   // LDS: (EP / 2, 64) pairs, shared by the workgroup
    float *x, *h1;  // LDS of this wave: x[EP] (input, zero padded), h1[64]
    int EP;

    __device__ __forceinline__ void load(const float *params, int E, int ep, int lane, const f2 *w1_lds, float *x_lds)
    {
        PolicyHead::load(params, E, lane);
        w1 = w1_lds;
        x = x_lds;
        h1 = x_lds + ep;
        EP = ep;
    }

    // the action of PolicyHead::act for the observation in x
    __device__ __forceinline__ int act(int lane, float u, float &p0, float &p1, float &p2, float &p3, float &value) const
    {
        wave_lds_sync();
        f2 acc2 = {bias1, 0.0f};
        const f2 *wl = w1 + lane;
        // 16 inputs per batch: 4 broadcast ds_read_b128 of x and 8 ds_read_b64 of weights in flight, then 8 v_pk_fma
#pragma unroll 2
        for (int k0 = 0; k0 < EP; k0 += 16) {
            float4 xs[4];
            f2 ws[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) xs[i] = *(const float4 *)(x + k0 + 4 * i);
#pragma unroll
            for (int i = 0; i < 8; ++i) ws[i] = wl[(k0 / 2 + i) * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f2 lo = {xs[i].x, xs[i].y}, hi = {xs[i].z, xs[i].w};
                acc2 = __builtin_elementwise_fma(ws[2 * i], lo, acc2);
                acc2 = __builtin_elementwise_fma(ws[2 * i + 1], hi, acc2);
            }
        }
        return PolicyHead::act(acc2, h1, lane, u, p0, p1, p2, p3, value);
    }
};

// 'positions' of a snake from the carried scalars: (head row, head column, food row, food column), 0 for a missing
// head / food — write_obs's argmax of the two channels, which for fast_init's at most one food is the food cell itself
__device__ __forceinline__ void fast_positions(const Geo &g, const Fast &f, float *__restrict__ o, float *lds_copy)
{
    const int h = f.hc < 0 ? 0 : f.hc, fc = f.food < 0 ? 0 : f.food;
    const int hy = div_size(h, g.rcpS), fy = div_size(fc, g.rcpS), lane = g.lane;
    const float v = (float)(lane == 0 ? hy : lane == 1 ? h - hy * g.S : lane == 2 ? fy : fc - fy * g.S);
    if (lane < 4) {
        o[lane] = v;
        lds_copy[lane] = v;
    }
}

// at most 8 waves per workgroup; 4 from 48 cells per lane on, where the snake's body registers and W2 need more than the
// 256 VGPRs an 8-wave workgroup leaves a lane (scratch otherwise)
template <int CPL>
constexpr int policy_wide_max_wpb() { return CPL >= 48 ? 4 : 8; }

template <int CPL, bool SNAKE, bool POP = false>
__global__ __launch_bounds__(64 * policy_wide_max_wpb<CPL>())
void policy_wide_kernel(typename policy_wide_args<POP>::type a)
{
    typedef PolicyWide::f2 f2;
    long long pop_first = 0, pop_wg = 0; // POP: the member's first env, the workgroup's place among the member's
    if constexpr (POP) {
        const long long wg = xcd_block(blockIdx.x, gridDim.x), member = wg / a.wgpm;
        pop_wg = wg - member * a.wgpm;
        pop_first = member * a.M;
        a.p.params += member * policy_num_params(a.E);
    }
    const PolicyArgs &p = a.p;
    const int E = a.E, EP = a.EP;
    {   // W1 (64, E) -> LDS as (EP / 2, 64) pairs, zero padded: input k of unit j at float 128 (k / 2) + 2 j + (k & 1).
        // Coalesced reads of W1 in its own order, scattered LDS writes.
        float *w1f = (float *)wurm_lds;
        const int n = 64 * E, pad = EP - E;
#pragma unroll 4
        for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
            const int j = i / E, k = i - j * E;
            w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = p.params[i];
        }
        for (int i = (int)threadIdx.x; i < 64 * pad; i += (int)blockDim.x) {
            const int j = i / pad, k = E + (i - j * pad);
            w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = 0.0f;
        }
    }
    __syncthreads();
    const int wave = uniform((int)(threadIdx.x >> 6));
    long long env;
    if constexpr (POP) {
        const long long i = pop_wg * a.wpb + wave;
        if (i >= a.M) return;
        env = pop_first + i;
    } else {
        env = xcd_block(blockIdx.x, gridDim.x) * a.wpb + wave;
        if (env >= p.N) return;
    }
    signed char *wl = wurm_lds + (size_t)EP * 256 + (size_t)wave * a.wave_bytes;
    float *x = (float *)wl;
    signed char *cls = wl + (size_t)EP * 4 + 256; // write_obs's class map (crops of grids > 128 cells)
    const Geo g = make_geo<CPL>(p.S);
    const int lane = g.lane;
    float *envp = p.envs + env * (SNAKE ? 3 : 2) * g.C;
    Env<CPL> e;
    load_state<CPL, SNAKE>(envp, g, e);
    Fast f = {-1, 0, 0, 0, 0, -1};
    bool ok;
    if constexpr (SNAKE) {
        ok = fast_init<CPL>(e, g, f);
    } else { // exactly one agent and one food
        const int counts = wave_sum_i32(__popcll(e.head) | (__popcll(e.food) << 16));
        ok = counts == (1 | (1 << 16));
    }
    if (!uniform((int)ok)) {
        if (lane == 0) p.status[env] = 1;
        return;
    }
    if (lane == 0) p.status[env] = 0;
    PolicyWide pol;
    pol.load(p.params, E, EP, lane, (const f2 *)wurm_lds, x);
    for (int k = lane; k < EP; k += 64) x[k] = k < E ? p.obs0[env * E + k] : 0.0f;

    const u64 env_id = (u64)(p.env_offset + env);
    const bool positions = a.obs_mode == WURM_OBS_POSITIONS;
    const bool small_crop = SNAKE && CPL <= 2 && !positions;
    const Crop cg = make_crop(lane, small_crop ? a.obs_n : 0);
    const long long obs_stride = p.N * E;
    float *obs_t = p.obs + env * E;
    u64 call = p.call;
    for (long long t0 = 0; t0 < p.T; t0 += 64) {
        const int nt = (int)min((long long)64, p.T - t0);
        const long long my_t = t0 + lane;
        const float my_u = u01(rng_words(p.seed, p.call + 2ull * (u64)my_t, env_id, RNG_POLICY, 0).w[0]);
        PolicyRecord rec = {0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < nt; ++j, obs_t += obs_stride, call += 2) {
            float p0, p1, p2, p3, value;
            const int act = pol.act(lane, __int_as_float(lane_value(__float_as_int(my_u), j)), p0, p1, p2, p3, value);
            StepOut out;
            if constexpr (SNAKE) { // env.step(action) (single_snake.py:197-304), observation to HBM and LDS, env.reset(done)
                fast_step<CPL>(e, g, f, act, act, out, p.seed, call, env_id, false, -1);
                if (positions) {
                    fast_positions(g, f, obs_t, x);
                } else if (small_crop) {
                    if constexpr (CPL <= 2) fast_partial_small<CPL>(e, g, f, obs_t, cg, x);
                } else {
                    fast_sync_bits<CPL>(e, g, f);
                    write_obs<CPL, true>(e, g, f.hc, obs_t, WURM_OBS_PARTIAL, a.obs_n, cls, x);
                }
                if (out.done) fast_reset<CPL>(e, g, f, p.seed, call + 1ull, env_id, nullptr);
            } else {               // simple_gridworld.py:135-202, :111-133, :225-268
                step_core<CPL, false, false>(e, g, nullptr, (long long)act, out, p.seed, call, env_id, false, -1, cls);
                write_obs<CPL, false>(e, g, out.headcell, obs_t, WURM_OBS_POSITIONS, 0, cls, x);
                if (out.done) reset_core<CPL, false>(e, g, p.seed, call + 1ull, env_id, nullptr, a.start_y, a.start_x);
            }
            if (lane == j) {
                rec.act = (int)out.action;
                rec.flags = out.done | (out.selfc << 1) | (out.edgec << 2) | (out.reward != 0.0f ? 8 : 0);
                rec.val = value; rec.p0 = p0; rec.p1 = p1; rec.p2 = p2; rec.p3 = p3;
            }
        }
        if (lane < nt) rec.template flush<SNAKE>(p, my_t * p.N + env);
    }
    if constexpr (SNAKE) fast_sync_bits<CPL>(e, g, f);
    store_state<CPL, SNAKE>(envp, g, e);
}

// members == 0: the N envs act with one set of weights; members >= 1: a population of that many members (N % members == 0)
template <bool SNAKE>
static int launch_policy_wide_cpl(PolicyWideArgs a, int cpl, hipStream_t st, long long members = 0)
{
    constexpr int LDS_MAX = 160 * 1024, W1_LDS_PER_INPUT = 64 * 4;
    const int S = a.p.S;
    a.EP = (a.E + 15) & ~15;
    a.wave_bytes = a.EP * 4 + 64 * 4 + ((S * S + 15) & ~15);
    const int fit = (LDS_MAX - a.EP * W1_LDS_PER_INPUT) / a.wave_bytes;
    // as many waves per workgroup as fit (each workgroup copies W1 once), but no fewer workgroups than CUs
    const long long per_cu = (a.p.N + 255) / 256, most = cpl >= 48 ? 4 : 8;
    a.wpb = (int)std::max(1ll, std::min({(long long)fit, most, per_cu}));
    const size_t lds = (size_t)a.EP * W1_LDS_PER_INPUT + (size_t)a.wpb * a.wave_bytes;
    dim3 block(64 * a.wpb), grid((unsigned)((a.p.N + a.wpb - 1) / a.wpb));
    auto go = [&](auto kernel) {
        if (lds > 65536) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        WURM_LAUNCH(kernel, grid, block, lds, st, a);
    };
    (void)hipGetLastError();
    if (members > 0) {
        PolicyWidePopArgs b = {};
        static_cast<PolicyWideArgs &>(b) = a;
        b.M = a.p.N / members;
        b.wpb = (int)std::min((long long)a.wpb, b.M); // (no workgroup of idle waves only)
        b.wgpm = (unsigned)((b.M + b.wpb - 1) / b.wpb);
        const size_t lds_pop = (size_t)a.EP * W1_LDS_PER_INPUT + (size_t)b.wpb * a.wave_bytes;
        block = dim3(64 * b.wpb);
        grid = dim3((unsigned)(members * b.wgpm));
        auto go_pop = [&](auto kernel) {
            if (lds_pop > 65536)
                (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pop);
            WURM_LAUNCH(kernel, grid, block, lds_pop, st, b);
        };
        switch (cpl) {
        case 2: go_pop(policy_wide_kernel<2, SNAKE, true>); break;
        case 4: go_pop(policy_wide_kernel<4, SNAKE, true>); break;
        case 8: go_pop(policy_wide_kernel<8, SNAKE, true>); break;
        case 16: go_pop(policy_wide_kernel<16, SNAKE, true>); break;
        case 24: go_pop(policy_wide_kernel<24, SNAKE, true>); break;
        case 32: go_pop(policy_wide_kernel<32, SNAKE, true>); break;
        case 48: go_pop(policy_wide_kernel<48, SNAKE, true>); break;
        case 64: go_pop(policy_wide_kernel<64, SNAKE, true>); break;
        default: return WURM_ERR_UNSUPPORTED;
        }
        return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
    }
    switch (cpl) {
    case 2: go(policy_wide_kernel<2, SNAKE>); break;
    case 4: go(policy_wide_kernel<4, SNAKE>); break;
    case 8: go(policy_wide_kernel<8, SNAKE>); break;
    case 16: go(policy_wide_kernel<16, SNAKE>); break;
    case 24: go(policy_wide_kernel<24, SNAKE>); break;
    case 32: go(policy_wide_kernel<32, SNAKE>); break;
    case 48: go(policy_wide_kernel<48, SNAKE>); break;
    case 64: go(policy_wide_kernel<64, SNAKE>); break;
    default: return WURM_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace wurm
