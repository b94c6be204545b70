// multi_rollout_stats.hpp — the per-agent log columns of experiments/multiagent.py:486-505 from the (T, K N) outputs of a
// MultiSnake window, in two launches with no host synchronisation (include/wurm_hip.h: wurm_multi_rollout_stats; host
// side: multi_rollout_stats.hip).  A row is one (snake k, env i) pair, column k N + i.
//
// multi_rollout_stats_scan_kernel: one lane per row walks the window forwards and carries the life's return and length
// from window to window.  The carried state is private to the lane, so the step loop has NO workgroup barrier and no
// LDS: every WAVE forms its own ten per-step sums and writes them to its own rows of the workspace.  Five of the ten
// are counts of flags (a ballot and a popcount), two are sizes under a flag (an integer butterfly); only reward, food
// and entropy go through the double butterfly of rollout_stats.hpp.  The next step's row is loaded before this step's
// cross-lane work, so a step costs its butterflies, not a trip to memory.
// multi_rollout_stats_reduce_kernel: one workgroup per agent sums the waves' partials in (workgroup, wave) order, adds
// them to the persistent accumulator and runs the reference's exponential smoother over the window's per-step masked
// means, in step order.  A step whose mask is empty leaves that column's smoother as it was.
//
// No atomics, no grid-wide barrier, no scratch: the same bits every run; agent k's waves and lanes are those of a
// stand-alone call on its N columns.
#pragma once

#define WURM_STATS_HELPERS_ONLY // wave_sum_f64, wave_max_f64, entropy_f32 and the workgroup shape: not the kernels
#include "rollout_stats.hpp"
#undef WURM_STATS_HELPERS_ONLY

namespace wurm {
namespace mstats {

using stats::THREADS;
using stats::WAVES;
constexpr int SUMS = 10;   // per step: alive, done, reward alive, H alive, food alive, boost alive, size alive, edge, snake, size done
constexpr int WINDOW = 5;  // per window: sum of life return, of life length; max size at death, max life return; episodes
constexpr int ACC = 16;    // accumulator: env steps, the ten sums, the five window values
constexpr int COLS = 9;    // smoother: reward, policy_entropy, food, edge_collisions, snake_collisions, boost, size, done, return

__host__ __device__ inline long long partial_stride(long long T) { return SUMS * T + WINDOW; } // of one wave

struct scan_args {
    const float *rewards, *food, *size;             // (T, K N)
    const uint8_t *dones, *boost, *snake, *edge;    // (T, K N)
    const float *probs;                             // (T, K N, 4), nullable
    const uint8_t *all_done;                        // (T, N), nullable
    float *carry_return;                            // (K N)
    int *carry_length;                              // (K N)
    double *partials;                               // (K, G, WAVES, partial_stride(T))
    long long N, T;                                 // envs, steps (K is the grid's y)
};

// what a lane reads of one step
struct step_row {
    float r, food, h;
    int size;
    bool done, boost, snake, edge, all;
};

__device__ __forceinline__ step_row load_row(const scan_args &g, long long t, long long KN, long long col, long long env)
{
    step_row x;
    const long long i = t * KN + col;
    x.r = g.rewards[i];
    x.food = g.food[i];
    x.size = (int)g.size[i]; // a snake's length: an integer held in a float
    x.done = g.dones[i] != 0;
    x.boost = g.boost[i] != 0;
    x.snake = g.snake[i] != 0;
    x.edge = g.edge[i] != 0;
    x.h = g.probs ? stats::entropy_f32(*reinterpret_cast<const float4 *>(g.probs + 4 * i)) : 0.0f;
    x.all = g.all_done && g.all_done[t * g.N + env] != 0;
    return x;
}

__device__ __forceinline__ int wave_sum_i32(int v) // integers: exact in any order
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double count(bool flag) { return (double)__popcll(__ballot(flag)); }

// agent blockIdx.y: workgroup blockIdx.x has its envs [256 x, 256 x + 256)
__global__ __launch_bounds__(THREADS) void multi_rollout_stats_scan_kernel(scan_args g)
{
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long KN = (long long)gridDim.y * g.N, env = (long long)blockIdx.x * THREADS + tid;
    const long long col = (long long)blockIdx.y * g.N + env;
    const bool live = env < g.N; // the others add zeros: every lane takes part in the ballots and the butterflies
    double *out = g.partials + (((long long)blockIdx.y * gridDim.x + blockIdx.x) * WAVES + wave) * partial_stride(g.T);

    const step_row none = {0.0f, 0.0f, 0.0f, 0, false, false, false, false, false};
    float ret = 0.0f;
    int len = 0;
    step_row next = none;
    if (live) {
        ret = g.carry_return[col];
        len = g.carry_length[col];
        next = load_row(g, 0, KN, col, env);
    }
    double ep_ret = 0.0, ep_len = 0.0, max_size = -INFINITY, max_ret = -INFINITY, episodes = 0.0; // no death yet

    for (long long t = 0; t < g.T; ++t) {
        const step_row x = next;
        if (live && t + 1 < g.T) next = load_row(g, t + 1, KN, col, env);
        const bool alive = live && !x.done;
        if (live) {
            ret += x.r;
            len += 1;
            if (x.done) { // (a snake that stays dead counts on every step, as size_i[done_i] does)
                ep_ret += (double)ret;
                ep_len += (double)len;
                max_size = fmax(max_size, (double)x.size);
                max_ret = fmax(max_ret, (double)ret);
                ret = 0.0f;
                len = 0;
            }
        }
        const double s_reward = stats::wave_sum_f64(alive ? (double)x.r : 0.0);
        const double s_h = stats::wave_sum_f64(alive ? (double)x.h : 0.0);
        const double s_food = stats::wave_sum_f64(alive ? (double)x.food : 0.0);
        const double s_size = (double)wave_sum_i32(alive ? x.size : 0);
        const double s_size_done = (double)wave_sum_i32(x.done ? x.size : 0);
        const double n_alive = count(alive), n_done = count(x.done), n_boost = count(alive && x.boost);
        const double n_edge = count(x.edge), n_snake = count(x.snake);
        episodes += count(x.all);
        // every lane holds every sum: lane j stores sum j
        double v = n_alive;
        v = lane == 1 ? n_done : v;
        v = lane == 2 ? s_reward : v;
        v = lane == 3 ? s_h : v;
        v = lane == 4 ? s_food : v;
        v = lane == 5 ? n_boost : v;
        v = lane == 6 ? s_size : v;
        v = lane == 7 ? n_edge : v;
        v = lane == 8 ? n_snake : v;
        v = lane == 9 ? s_size_done : v;
        if (lane < SUMS) out[SUMS * t + lane] = v;
    }

    if (live) {
        g.carry_return[col] = ret;
        g.carry_length[col] = len;
    }
    const double w_ret = stats::wave_sum_f64(ep_ret), w_len = stats::wave_sum_f64(ep_len);
    const double w_size = stats::wave_max_f64(max_size), w_max = stats::wave_max_f64(max_ret);
    double v = w_ret;
    v = lane == 1 ? w_len : v;
    v = lane == 2 ? w_size : v;
    v = lane == 3 ? w_max : v;
    v = lane == 4 ? episodes : v;
    if (lane < WINDOW) out[SUMS * g.T + lane] = v;
}

// agent blockIdx.y: its W = G WAVES partials -> its rows of steps (T, SUMS), accum (ACC) and smooth (COLS)
__global__ __launch_bounds__(THREADS) void multi_rollout_stats_reduce_kernel(const double *__restrict__ partials,
                                                                             long long W, long long N, long long T,
                                                                             double alpha, double *steps,
                                                                             double *__restrict__ accum,
                                                                             double *__restrict__ smooth)
{
    __shared__ double window[WINDOW];
    const long long k = blockIdx.y, stride = partial_stride(T);
    const int tid = (int)threadIdx.x;
    partials += k * W * stride;
    steps += k * T * SUMS;
    accum += k * ACC;
    smooth += k * COLS;
    for (long long i = tid; i < stride; i += THREADS) {
        const long long j = i - SUMS * T;
        double s = partials[i];
        if (j == 2 || j == 3) {
#pragma unroll 8
            for (long long w = 1; w < W; ++w) s = fmax(s, partials[w * stride + i]);
        } else {
#pragma unroll 8
            for (long long w = 1; w < W; ++w) s += partials[w * stride + i];
        }
        if (j < 0)
            steps[i] = s;
        else
            window[j] = s;
    }
    __syncthreads(); // (the workgroup's own stores to steps are visible to it from here on)
    if (tid < SUMS) {
        double sum = 0.0;
        for (long long t = 0; t < T; ++t) sum += steps[SUMS * t + tid];
        accum[1 + tid] += sum;
    } else if (tid < SUMS + COLS) {
        // the reference's columns, multiagent.py:493-502: numerator and mask (-1: all N envs) among the ten sums
        const int c = tid - SUMS;
        const int num = c == 0 ? 2 : c == 1 ? 3 : c == 2 ? 4 : c == 3 ? 7 : c == 4 ? 8 : c == 5 ? 5 : c == 6 ? 6 : c == 7 ? 1 : 9;
        const int den = c == 3 || c == 4 || c == 7 ? -1 : c == 8 ? 1 : 0;
        // wurm/utils.py:329-335: the first value ever seen initialises the state, which is NaN until then.  A step with
        // an empty mask (a NaN mean in the reference, which its tracker never recovers from) is skipped.
        double s = smooth[c];
        for (long long t = 0; t < T; ++t) {
            const double d = den < 0 ? (double)N : steps[SUMS * t + den];
            if (d > 0.0) {
                const double mean = steps[SUMS * t + num] / d;
                s = s != s ? mean : alpha * mean + (1.0 - alpha) * s;
            }
        }
        smooth[c] = s;
    } else if (tid == SUMS + COLS) {
        accum[0] += (double)(T * N);
    } else if (tid <= SUMS + COLS + WINDOW) {
        const int j = tid - (SUMS + COLS + 1);
        accum[1 + SUMS + j] = j == 2 || j == 3 ? fmax(accum[1 + SUMS + j], window[j])  // (-inf: no death yet)
                                               : accum[1 + SUMS + j] + window[j];
    }
}

} // namespace mstats
} // namespace wurm
