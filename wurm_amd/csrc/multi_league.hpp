// multi_league.hpp — a league of policies in one MultiSnake batch: every (snake k, env i) row names the policy that plays
// it (include/wurm_hip.h: wurm_multi_act_league, wurm_multi_league_scores; host side: multi_league.hip; Python:
// wurm_amd/envs/_multi_league.py, wurm_amd/rl/league_table.py).
//
// multi_act_league_kernel<NOBS> is multi_act_kernel (multi_act.hpp) with an INDEX LIST where that kernel has a consecutive
// range.  The caller sorts the K N rows by policy once per draw of matchups:
//   order   (K N) int32: the rows r = k N + i, those of policy 0 first, ascending within a policy
//   offsets (A + 1) int64: policy a owns order[offsets[a] .. offsets[a + 1])
// Both live on the device and are read on the device only.  A workgroup serves policy a = blockIdx.x / wgps: W1 of row a
// of `params` in LDS, the heads in registers, its waves walking j = offsets[a] + part * 8 + wave, + wgps * 8, ... and
// acting for row order[j]; the next row's observation is prefetched through `order` as well.  The W1 copy, the staging
// of a row and the row's body (draw, first layer, head, stores) are the device functions of multi_act.hpp: the arithmetic
// and the Philox stream of a row — env_id = (env_offset + i) K + k at the POLICY call counter — do not depend on who
// plays it, nor on where in a list the row stands.
// The grid is sized from K, N and A alone (launch_multi_act_league), never from the list: a policy without rows costs
// workgroups that read two offsets and return BEFORE the W1 copy.
// Bounds: the two offsets are clamped to [0, K N] and an entry of `order` outside [0, K N) is skipped, so the kernel
// reads `order` only inside its K N entries and touches no row outside the outputs, whatever the two arrays hold.  (A
// row listed twice is written twice: a plan's business, not a fault.)
// No atomics, no grid-wide barrier, no scratch; the only workgroup barrier is the one behind the W1 copy.
//
// league_scores_kernel: the per-policy sums of a window's (T, K N) tensors over the same lists.  One workgroup per
// policy; thread t of it takes the list entries offsets[a] + t, + 256, ... and walks each one's column down the T steps,
// adding into eight doubles of its own.  Then the fixed butterfly of rollout_stats.hpp in every wave, the waves' values
// through LDS in wave order, and threads 0 .. 7 add the workgroup's sums to row a of the persistent (A, 8) table: no
// atomics, the same association every run, so the same bits every run.
#pragma once

#include "multi_act.hpp"

#define WURM_STATS_HELPERS_ONLY // wave_sum_f64: not the kernels
#include "rollout_stats.hpp"
#undef WURM_STATS_HELPERS_ONLY

namespace wurm {

struct MultiLeagueArgs : MultiActArgs { // P: the number of policies A; wgps: workgroups per policy
    const int *order;          // (K N)
    const long long *offsets;  // (A + 1)
};

__device__ __forceinline__ long long league_clamp(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

template <int NOBS>
__global__ __launch_bounds__(64 * MULTI_ACT_WAVES)
void multi_act_league_kernel(MultiLeagueArgs a)
{
    typedef PolicyHead::f2 f2;
    constexpr int W = 2 * NOBS + 1, E = 3 * W * W, EP = (E + 15) & ~15, NX = (EP + 63) / 64;
    const unsigned policy = blockIdx.x / a.wgps, part = blockIdx.x - policy * a.wgps;
    const long long rows = (long long)a.K * a.N;
    const long long list_end = league_clamp(a.offsets[policy + 1], rows);
    const long long wg_first = league_clamp(a.offsets[policy], rows) + (long long)part * MULTI_ACT_WAVES;
    const long long stride = (long long)a.wgps * MULTI_ACT_WAVES;
    if (wg_first >= list_end) return; // (the whole workgroup: a policy nobody plays, or one with fewer rows than a pass)
    const float *params = a.params + (long long)policy * policy_num_params(E);
    multi_act_copy_w1<E>(params);
    __syncthreads();
    const int wave = uniform((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    long long j = wg_first + wave;
    if (j >= list_end) return;
    float *x = (float *)(wurm_lds + (size_t)EP * 256 + (size_t)wave * (EP * 4 + 256)), *h1 = x + EP;
    const f2 *wl = (const f2 *)wurm_lds + lane;
    PolicyHead head;
    head.load(params, E, lane);

    float xs[NX]; // the row's observation, input lane + 64 i in slot i
    long long r = a.order[j]; // (0 <= j < list_end <= K N)
    bool ok = r >= 0 && r < rows;
    if (ok) multi_act_load_row<E>(xs, a.obs, r, lane);
    for (; j < list_end; j += stride) {
        if (ok) multi_act_stage_row<EP>(x, xs, lane);
        const long long next = j + stride;
        const long long rn = next < list_end ? (long long)a.order[next] : -1;
        const bool okn = rn >= 0 && rn < rows;
        if (okn) multi_act_load_row<E>(xs, a.obs, rn, lane);
        if (ok) multi_act_row<EP>(a, r, x, h1, wl, head, lane);
        r = rn;
        ok = okn;
    }
}

// workgroups per policy: one per MULTI_ACT_WAVES rows if every row were one policy's, but about 256 workgroups in all
inline unsigned multi_league_wgps(long long rows, int A)
{
    const long long want = (rows + MULTI_ACT_WAVES - 1) / MULTI_ACT_WAVES, cap = std::max(1, 256 / A);
    return (unsigned)std::min(want, cap);
}

// arguments already validated, 0 < K N < 2^31, A >= 1
static int launch_multi_act_league(MultiLeagueArgs a, int obs_n, hipStream_t st)
{
    const int E = 3 * (2 * obs_n + 1) * (2 * obs_n + 1), EP = (E + 15) & ~15;
    a.wgps = multi_league_wgps((long long)a.K * a.N, a.P);
    const size_t lds = (size_t)EP * 256 + (size_t)MULTI_ACT_WAVES * (EP * 4 + 256);
    const dim3 grid((unsigned)a.P * a.wgps), block(64 * MULTI_ACT_WAVES);
    auto go = [&](auto kernel) {
        if (lds > 65536) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        WURM_LAUNCH(kernel, grid, block, lds, st, a);
    };
    (void)hipGetLastError();
    switch (obs_n) {
    case 0: go(multi_act_league_kernel<0>); break;
    case 1: go(multi_act_league_kernel<1>); break;
    case 2: go(multi_act_league_kernel<2>); break;
    case 3: go(multi_act_league_kernel<3>); break;
    case 4: go(multi_act_league_kernel<4>); break;
    case 5: go(multi_act_league_kernel<5>); break;
    case 6: go(multi_act_league_kernel<6>); break;
    default: return WURM_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

// ---- scores ---------------------------------------------------------------------------------------------------------

namespace league {

constexpr int THREADS = 256, WAVES = THREADS / 64;
// steps, reward, deaths, food, snake_collisions, edge_collisions, boost, size_sum
constexpr int COLS = 8;

struct scores_args {
    const float *rewards;                  // (T, R)
    const uint8_t *dones;                  // (T, R)
    const float *food, *size;              // (T, R), nullable
    const uint8_t *snake, *edge, *boost;   // (T, R), nullable
    const int *order;                      // (R)
    const long long *offsets;              // (A + 1)
    double *table;                         // (A, COLS), added to
    long long R, T;                        // rows K N, steps
};

} // namespace league

__global__ __launch_bounds__(league::THREADS) void league_scores_kernel(league::scores_args g)
{
    using namespace league;
    __shared__ double buf[WAVES][COLS];
    const unsigned policy = blockIdx.x;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long first = league_clamp(g.offsets[policy], g.R), end = league_clamp(g.offsets[policy + 1], g.R);
    if (first >= end) return; // (the whole workgroup: nothing to add)
    double c[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) c[k] = 0.0;
    for (long long j = first + tid; j < end; j += THREADS) {
        const long long r = g.order[j]; // (0 <= j < end <= R)
        if (r < 0 || r >= g.R) continue;
        for (long long t = 0; t < g.T; ++t) {
            const long long i = t * g.R + r;
            c[0] += 1.0;
            c[1] += (double)g.rewards[i];
            c[2] += g.dones[i] != 0 ? 1.0 : 0.0;
            if (g.food) c[3] += (double)g.food[i];
            if (g.snake) c[4] += g.snake[i] != 0 ? 1.0 : 0.0;
            if (g.edge) c[5] += g.edge[i] != 0 ? 1.0 : 0.0;
            if (g.boost) c[6] += g.boost[i] != 0 ? 1.0 : 0.0;
            if (g.size) c[7] += (double)g.size[i];
        }
    }
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
        const double s = stats::wave_sum_f64(c[k]);
        if (lane == 0) buf[wave][k] = s;
    }
    __syncthreads();
    if (tid < COLS) {
        double s = buf[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += buf[w][tid];
        g.table[(long long)policy * COLS + tid] += s; // (row `policy` is this workgroup's alone)
    }
}

} // namespace wurm
