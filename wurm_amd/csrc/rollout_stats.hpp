// rollout_stats.hpp — the log columns of experiments/main.py:252-316 from the (T, N) outputs of a policy rollout, in two
// launches with no host synchronisation (include/wurm_hip.h: wurm_rollout_stats; host side: rollout_stats.hip).
//
// rollout_stats_scan_kernel: one thread per env walks the window forwards and carries the env's episode state (return,
// length, snake size) from window to window.  Per step the workgroup forms the batch sums of done, reward, edge collision,
// self collision, snake size after the reset and policy entropy: a fixed wave butterfly in double, then the waves' values
// through LDS in wave order.  Per window it forms the sums and maxima over the episodes that ended.  Every workgroup writes
// its partials to its own rows of the workspace: no atomics, no grid-wide barrier.
// rollout_stats_reduce_kernel: one workgroup per member sums the partials in workgroup order, adds them to the persistent
// accumulator and runs the reference's exponential smoother over the window's per-step batch means, in step order.
//
// Every sum but the entropy's is a sum of small integers held in doubles: exact, whatever the grid and the order.
#pragma once

#include "wurm_device.hpp"

namespace wurm {
namespace stats {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int COLS = 6;     // per step: done, reward, edge collision, self collision, size, entropy
constexpr int EPISODE = 5;  // per window: sum of return, of length, of final size; max return, max final size
constexpr int ACC = 12;     // accumulator: env steps, the six columns, the three episode sums, the two maxima

__host__ __device__ inline long long partial_stride(long long T) { return COLS * T + EPISODE; }

struct scan_args {
    const float *rewards;        // (T, N)
    const uint8_t *dones;        // (T, N)
    const uint8_t *edge;         // (T, N)
    const uint8_t *self;         // (T, N), nullable
    const float *probs;          // (T, N, 4), nullable
    float *carry_return;         // (N)
    int *carry_length;           // (N)
    int *carry_size;             // (N)
    double *partials;            // (members, G, partial_stride(T))
    long long N, M, T;           // envs, envs per member, steps
    int initial_size;
};

__device__ __forceinline__ double wave_sum_f64(double v) // fixed butterfly order: the same bits every run
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// H = - sum_k p_k log(clamp(p_k, eps32, 1 - eps32)) in fp32: the learner's expression (a2c_learner.hpp)
__device__ __forceinline__ float entropy_f32(const float4 p4)
{
    const float eps32 = 1.1920928955078125e-07f, hi32 = 1.0f - eps32;
    const float p[4] = {p4.x, p4.y, p4.z, p4.w};
    float h = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) h -= p[k] * logf(fminf(fmaxf(p[k], eps32), hi32));
    return h;
}

#ifndef WURM_STATS_HELPERS_ONLY // (multi_rollout_stats.hpp includes this header for what is above, not for the kernels)

// member blockIdx.y, envs [m M, (m + 1) M): workgroup blockIdx.x of the member has its envs [256 x, 256 x + 256), the
// waves and lanes of a stand-alone call on the member's M columns
__global__ __launch_bounds__(THREADS) void rollout_stats_scan_kernel(scan_args g)
{
    __shared__ double sums[2][WAVES][COLS];
    __shared__ double ends[WAVES][EPISODE];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long local = (long long)blockIdx.x * THREADS + tid, env = (long long)blockIdx.y * g.M + local;
    const bool live = local < g.M; // the others add zeros: every lane takes part in the butterflies and the barriers
    double *out = g.partials + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * partial_stride(g.T);

    float ret = 0.0f;
    int len = 0, size = 0;
    if (live) {
        ret = g.carry_return[env];
        len = g.carry_length[env];
        size = g.carry_size[env];
    }
    double ep_ret = 0.0, ep_len = 0.0, ep_size = 0.0, max_ret = -INFINITY, max_size = -INFINITY; // no episode yet

    for (long long t = 0; t < g.T; ++t) {
        double c[COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (live) {
            const long long i = t * g.N + env;
            const float r = g.rewards[i];
            const bool done = g.dones[i] != 0;
            // single_snake.py:268-271: +1 exactly when the snake ate (initial_size 0: an env without a snake, all sizes 0)
            const int grown = size + (g.initial_size > 0 && r == 1.0f ? 1 : 0);
            ret += r;
            len += 1;
            if (done) {
                ep_ret += (double)ret;
                ep_len += (double)len;
                ep_size += (double)grown;
                max_ret = fmax(max_ret, (double)ret);
                max_size = fmax(max_size, (double)grown);
                ret = 0.0f;
                len = 0;
            }
            size = done ? g.initial_size : grown; // what main.py:273 reads after env.reset(done)
            c[0] = done ? 1.0 : 0.0;
            c[1] = (double)r;
            c[2] = g.edge[i] ? 1.0 : 0.0;
            c[3] = g.self && g.self[i] ? 1.0 : 0.0;
            c[4] = (double)size;
            if (g.probs) c[5] = (double)entropy_f32(*reinterpret_cast<const float4 *>(g.probs + 4 * i));
        }
        double (*buf)[COLS] = sums[t & 1]; // two buffers: one barrier per step
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const double s = wave_sum_f64(c[k]);
            if (lane == 0) buf[wave][k] = s;
        }
        __syncthreads();
        if (tid < COLS) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += buf[w][tid];
            out[COLS * t + tid] = s;
        }
    }

    if (live) {
        g.carry_return[env] = ret;
        g.carry_length[env] = len;
        g.carry_size[env] = size;
    }
    const double e[EPISODE] = {wave_sum_f64(ep_ret), wave_sum_f64(ep_len), wave_sum_f64(ep_size), wave_max_f64(max_ret),
                               wave_max_f64(max_size)};
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < EPISODE; ++k) ends[wave][k] = e[k];
    }
    __syncthreads();
    if (tid < EPISODE) {
        double s = ends[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s = tid < 3 ? s + ends[w][tid] : fmax(s, ends[w][tid]);
        out[COLS * g.T + tid] = s;
    }
}

// member blockIdx.y: its G partials -> its row of steps (T, COLS), accum (ACC) and smooth (COLS)
__global__ __launch_bounds__(THREADS) void rollout_stats_reduce_kernel(const double *__restrict__ partials, int G,
                                                                       long long M, long long T, double alpha,
                                                                       double *steps,
                                                                       double *__restrict__ accum,
                                                                       double *__restrict__ smooth)
{
    __shared__ double window[EPISODE];
    const long long m = blockIdx.y, stride = partial_stride(T);
    const int tid = (int)threadIdx.x;
    partials += m * G * stride;
    steps += m * T * COLS;
    accum += m * ACC;
    smooth += m * COLS;
    for (long long i = tid; i < stride; i += THREADS) {
        double s = partials[i];
        if (i < COLS * T + 3) {
#pragma unroll 8
            for (int w = 1; w < G; ++w) s += partials[w * stride + i];
        } else {
#pragma unroll 8
            for (int w = 1; w < G; ++w) s = fmax(s, partials[w * stride + i]);
        }
        if (i < COLS * T)
            steps[i] = s;
        else
            window[i - COLS * T] = s;
    }
    __syncthreads(); // (the workgroup's own stores to steps are visible to it from here on)
    if (tid < COLS) {
        // the column's window sum, then the smoother over its per-step batch means (wurm/utils.py:329-335): the first
        // value ever seen initialises the state, which is NaN until then
        double sum = 0.0, s = smooth[tid];
        for (long long t = 0; t < T; ++t) {
            const double x = steps[COLS * t + tid];
            sum += x;
            const double mean = x / (double)M;
            s = s != s ? mean : alpha * mean + (1.0 - alpha) * s;
        }
        accum[1 + tid] += sum;
        smooth[tid] = s;
    } else if (tid == COLS) {
        accum[0] += (double)(T * M);
    } else if (tid < COLS + 1 + 3) {
        accum[tid] += window[tid - (COLS + 1)];
    } else if (tid < ACC) {
        accum[tid] = fmax(accum[tid], window[tid - (COLS + 1)]); // (-inf: no episode has ended yet)
    }
}

#endif // WURM_STATS_HELPERS_ONLY

} // namespace stats
} // namespace wurm
