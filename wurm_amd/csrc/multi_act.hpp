// multi_act.hpp — the acting half of the reference's multi-agent loop (experiments/multiagent.py:354-364) for EVERY snake
// and EVERY species in one launch: observations (K, N, E) -> probs (K, N, 4), value (K, N), sampled action (K, N).
//
// Per agent k the reference runs  probs, value = models[k * num_species // K](obs_k);  action = Categorical(probs).sample()
// — K torch forwards, K Categoricals and a few clones around an env step of some tens of microseconds.  Here a ROW is one
// (snake k, env i) pair, r = k N + i; the rows of species s are the consecutive range [k0 N, k1 N) with
// k0 = ceil(s K / P), k1 = ceil((s + 1) K / P)  (exactly the k with k P / K == s in integer division), so a species is a
// block of rows and a block of the grid.
//
// Arithmetic: policy_rollout.hpp's spec, bit for bit (oracle/policy.c: oracle_policy_forward / oracle_policy_sample).
// PolicyHead (second layer, heads, softmax, sampler) is used as it is; only the first layer and the row loop are here.
// The draw of row (k, i) is u01(Philox(seed; env_id = (env_offset + i) K + k, call, RNG_POLICY).w0): every agent of
// every env has a stream of its own, and `call` is the env object's POLICY call counter, not the env's RNG counter.
//
// Mapping: one wave = one row at a time, lane = hidden unit (as in the single-agent actors).  A workgroup of
// MULTI_ACT_WAVES waves serves ONE species: it copies that species' W1 into LDS once, laid out as policy_wide.hpp's
// (input pair, unit) float2s — lane j reads float2 64 i + j, one conflict-free ds_read_b64 per pair of inputs — and each
// wave keeps the species' W2 and heads in registers across all its rows.  W1 is streamed from LDS for every E: at
// E = 507 it is 130 KB, beyond the register file, and at E <= 147, where Policy<NOBS> keeps it in registers, a second
// copy of this kernel would buy one LDS read per fma pair on a kernel whose launch the host already dominates at those
// sizes.  One row per pass over the weights.  A wave walks the rows r = first + wave, + stride, ...; the next row's
// observation is loaded from HBM into registers while the current one is multiplied.
// Inputs are zero padded to a multiple of 16 in LDS (weights AND inputs 0): fmaf(0, 0, acc) == acc except that -0
// becomes +0, which the ReLU after the layer maps to the same +0 (policy_wide.hpp) — both chains stay exact for the odd
// E = 27, 75, 147, 243, 363, 507 of 'partial_n'.
// LDS per workgroup: 256 EP + MULTI_ACT_WAVES (4 EP + 256) bytes (EP = E rounded up to 16): 149 504 at E = 507.
// No atomics, no grid-wide barrier; the only workgroup barrier is the one behind the W1 copy.
#pragma once

#include <algorithm>

#include "policy_rollout.hpp"

namespace wurm {

constexpr int MULTI_ACT_WAVES = 8; // rows a workgroup takes per pass

struct MultiActArgs {
    const float *params; // (P, policy_num_params(E))
    const float *obs;    // (K, N, E)
    long long *actions;  // (K, N)
    float *probs;        // (K, N, 4), nullable
    float *values;       // (K, N), nullable
    long long N;
    int K, P;            // snakes per env, species
    unsigned wgps;       // workgroups per species
    u64 seed, call;
    long long env_offset;
};

// snakes [k0, k1) of species s: the k with k * P / K == s
__host__ __device__ inline int multi_act_first_snake(int s, int K, int P) { return (int)(((long long)s * K + P - 1) / P); }

// The three pieces of the kernel that do not depend on how a workgroup finds its rows, written once: multi_act_kernel below
// walks a consecutive range, multi_act_league_kernel (multi_league.hpp) an index list.

// W1 (64, E) of `params` -> LDS as (EP / 2, 64) pairs, zero padded: input k of unit j at float 128 (k / 2) + 2 j + (k & 1).
// The whole workgroup; its barrier follows at the caller.
template <int E>
__device__ __forceinline__ void multi_act_copy_w1(const float *params)
{
    constexpr int EP = (E + 15) & ~15;
    float *w1f = (float *)wurm_lds;
    constexpr int n = 64 * E, pad = EP - E;
#pragma unroll 4
    for (int i = (int)threadIdx.x; i < n; i += 64 * MULTI_ACT_WAVES) {
        const int j = i / E, k = i - j * E;
        w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = params[i];
    }
    for (int i = (int)threadIdx.x; i < 64 * pad; i += 64 * MULTI_ACT_WAVES) {
        const int j = i / pad, k = E + (i - j * pad);
        w1f[(k >> 1) * 128 + 2 * j + (k & 1)] = 0.0f;
    }
}

// the observation of row r from HBM into registers: input lane + 64 i in slot i
template <int E, int NX>
__device__ __forceinline__ void multi_act_load_row(float (&xs)[NX], const float *obs, long long r, int lane)
{
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = lane + 64 * i < E ? obs[r * E + lane + 64 * i] : 0.0f;
}

// ... and from the registers into the wave's LDS row x (EP floats)
template <int EP, int NX>
__device__ __forceinline__ void multi_act_stage_row(float *x, const float (&xs)[NX], int lane)
{
#pragma unroll
    for (int i = 0; i < NX; ++i)
        if (lane + 64 * i < EP) x[lane + 64 * i] = xs[i];
}

// Row r = k N + i with its observation staged in x: the draw, the first layer against the workgroup's W1 (wl: the lane's
// column of pairs), the head, and the row's three outputs.  Ends with the wave's LDS fence: x and h1 may be rewritten.
template <int EP>
__device__ __forceinline__ void multi_act_row(const MultiActArgs &a, long long r, const float *x, float *h1,
                                              const PolicyHead::f2 *wl, const PolicyHead &head, int lane)
{
    typedef PolicyHead::f2 f2;
    const long long k = r / a.N, env = r - k * a.N;
    const u64 env_id = (u64)(a.env_offset + env) * (u64)a.K + (u64)k;
    const float u = u01(rng_words(a.seed, a.call, env_id, RNG_POLICY, 0).w[0]);
    wave_lds_sync();
    // first layer: 16 inputs per batch — 4 broadcast ds_read_b128 of x and 8 ds_read_b64 of weights, then 8 v_pk_fma
    f2 acc2 = {head.bias1, 0.0f};
#pragma unroll 2
    for (int k0 = 0; k0 < EP; k0 += 16) {
        float4 xv[4];
        f2 ws[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *(const float4 *)(x + k0 + 4 * i);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[i] = wl[(k0 / 2 + i) * 64];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f2 lo = {xv[i].x, xv[i].y}, hi = {xv[i].z, xv[i].w};
            acc2 = __builtin_elementwise_fma(ws[2 * i], lo, acc2);
            acc2 = __builtin_elementwise_fma(ws[2 * i + 1], hi, acc2);
        }
    }
    float p0, p1, p2, p3, value;
    const int act = head.act(acc2, h1, lane, u, p0, p1, p2, p3, value);
    if (lane == 0) {
        a.actions[r] = (long long)act;
        if (a.values) a.values[r] = value;
    }
    if (a.probs && lane < 4) a.probs[4 * r + lane] = lane == 0 ? p0 : lane == 1 ? p1 : lane == 2 ? p2 : p3;
    wave_lds_sync(); // (x and h1 are rewritten for the next row)
}

template <int NOBS>
__global__ __launch_bounds__(64 * MULTI_ACT_WAVES)
void multi_act_kernel(MultiActArgs a)
{
    typedef PolicyHead::f2 f2;
    constexpr int W = 2 * NOBS + 1, E = 3 * W * W, EP = (E + 15) & ~15, NX = (EP + 63) / 64;
    const unsigned species = blockIdx.x / a.wgps, part = blockIdx.x - species * a.wgps;
    const long long row_end = (long long)multi_act_first_snake((int)species + 1, a.K, a.P) * a.N;
    const long long wg_first = (long long)multi_act_first_snake((int)species, a.K, a.P) * a.N + (long long)part * MULTI_ACT_WAVES;
    const long long stride = (long long)a.wgps * MULTI_ACT_WAVES;
    if (wg_first >= row_end) return; // (the whole workgroup: a species with fewer rows than the largest one)
    const float *params = a.params + (long long)species * policy_num_params(E);
    multi_act_copy_w1<E>(params);
    __syncthreads();
    const int wave = uniform((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    long long r = wg_first + wave;
    if (r >= row_end) return;
    float *x = (float *)(wurm_lds + (size_t)EP * 256 + (size_t)wave * (EP * 4 + 256)), *h1 = x + EP;
    const f2 *wl = (const f2 *)wurm_lds + lane;
    PolicyHead head;
    head.load(params, E, lane);

    float xs[NX]; // the row's observation, input lane + 64 i in slot i
    multi_act_load_row<E>(xs, a.obs, r, lane);
    for (; r < row_end; r += stride) {
        multi_act_stage_row<EP>(x, xs, lane);
        const long long next = r + stride;
        if (next < row_end) multi_act_load_row<E>(xs, a.obs, next, lane);
        multi_act_row<EP>(a, r, x, h1, wl, head, lane);
    }
}

// n of 'partial_n' for num_inputs = 3 (2n+1)^2, n <= 6; -1 for anything else
inline int multi_act_obs_n(int num_inputs)
{
    for (int n = 0; n <= 6; ++n)
        if (num_inputs == 3 * (2 * n + 1) * (2 * n + 1)) return n;
    return -1;
}

// arguments already validated, K N > 0
static int launch_multi_act(MultiActArgs a, int obs_n, hipStream_t st)
{
    const int E = 3 * (2 * obs_n + 1) * (2 * obs_n + 1), EP = (E + 15) & ~15;
    // a species' workgroups: one per MULTI_ACT_WAVES rows of the largest species, but about one workgroup per CU in all
    // (each copies W1 once; at E = 507 one fits a CU), the waves looping over the rest
    const long long most_rows = (long long)((a.K + a.P - 1) / a.P) * a.N;
    const long long want = (most_rows + MULTI_ACT_WAVES - 1) / MULTI_ACT_WAVES, cap = std::max(1, 256 / a.P);
    a.wgps = (unsigned)std::min(want, cap);
    const size_t lds = (size_t)EP * 256 + (size_t)MULTI_ACT_WAVES * (EP * 4 + 256);
    const dim3 grid((unsigned)a.P * a.wgps), block(64 * MULTI_ACT_WAVES);
    auto go = [&](auto kernel) {
        if (lds > 65536) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        WURM_LAUNCH(kernel, grid, block, lds, st, a);
    };
    (void)hipGetLastError();
    switch (obs_n) {
    case 0: go(multi_act_kernel<0>); break;
    case 1: go(multi_act_kernel<1>); break;
    case 2: go(multi_act_kernel<2>); break;
    case 3: go(multi_act_kernel<3>); break;
    case 4: go(multi_act_kernel<4>); break;
    case 5: go(multi_act_kernel<5>); break;
    case 6: go(multi_act_kernel<6>); break;
    default: return WURM_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace wurm
