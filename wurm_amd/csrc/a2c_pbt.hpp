// a2c_pbt.hpp — the exploit / explore step of population-based training for FusedA2CPopulation as two kernels
// (include/wurm_hip.h: wurm_a2c_ff_pop_exploit):
//   pbt_rank_kernel  order[rank(p)] = p: the members best to worst by score
//   pbt_copy_kernel  the worst k members take the rows (params, exp_avg, exp_avg_sq) and the hyper-parameters of a member
//                    drawn from the best k; the copied lr and entropy_coef are multiplied by one of two factors and clamped
// No atomics, no grid-wide barrier, nothing read back: the second launch follows the first on the same stream, which is
// all the ordering there is.
//
// Rank.  key(p) = scores[p], a NaN counting as -infinity;  rank(p) = #{q : key(q) > key(p) or (key(q) == key(p) and
// q < p)}: a total order (ties go to the lower index), so the ranks are a permutation of 0 .. P - 1 and every slot of
// `order` is written exactly once.  The rank kernel has one member per thread and reads the scores through LDS in tiles
// of 256.  A workgroup of the copy kernel counts the rank of ITS member again, 256 threads over the P scores, rather than
// reading it from an array the first launch wrote (one coalesced pass over P doubles per workgroup, which the L2 serves;
// one array less in the ABI).  The count is an integer: the two kernels agree whatever the order of summation.
#pragma once
#include "wurm_device.hpp"

namespace wurm {
namespace pbt {

constexpr int THREADS = 256;
constexpr int SLICE = 1024;     // floats of a row per workgroup of the copy kernel: four coalesced dwords per thread
constexpr int HYPER_DOUBLES = 4; // a2c_learner.hpp: lr (as written), gamma, entropy_coef, gamma_lambda

// the factors and bounds of the explore step, by value in the argument block
struct Perturb {
    double lr_down, lr_up, lr_lo, lr_hi, e_down, e_up, e_lo, e_hi;
};

__device__ __forceinline__ double key_of(double score) { return score != score ? -INFINITY : score; }

// does q come before p?
__device__ __forceinline__ bool before(double key_q, long long q, double key_p, long long p)
{
    return key_q > key_p || (key_q == key_p && q < p);
}

// One member per thread.  Every thread of the workgroup walks all tiles (the barriers), also one past the last member.
__global__ void __launch_bounds__(THREADS) pbt_rank_kernel(const double *__restrict__ scores, int *__restrict__ order,
                                                           long long P)
{
    __shared__ double tile[THREADS];
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    const double mine = p < P ? key_of(scores[p]) : 0.0;
    int rank = 0;
    for (long long base = 0; base < P; base += THREADS) {
        const long long q = base + threadIdx.x;
        tile[threadIdx.x] = q < P ? key_of(scores[q]) : 0.0;
        __syncthreads();
        const int n = (int)(P - base < THREADS ? P - base : THREADS);
        for (int i = 0; i < n; ++i) rank += before(tile[i], base + i, mine, p) ? 1 : 0; // (tile[i]: a broadcast read)
        __syncthreads();
    }
    if (p < P) order[rank] = (int)p;
}

// Workgroup (x, p): the floats [x SLICE, (x + 1) SLICE) of member p's three rows.
// NO RACE: a row (of params, exp_avg, exp_avg_sq or hyper) is written only by the workgroups of a member of rank >= P - k,
// and only that member's own row; it is read only where it is a source, and a source is order[j] with j < k, a member of
// rank < k.  The entry point refuses 2 k > P, so k <= P - k: no member is both, no source row is written during the launch,
// and the workgroups need no order among themselves.  scores and order are only read.
// The rows are num_params = 64 E + 4549 floats, always odd: every other row is only 4-byte aligned, hence dword accesses.
__global__ void __launch_bounds__(THREADS) pbt_copy_kernel(float *params, float *exp_avg, float *exp_avg_sq, double *hyper,
                                                           const double *__restrict__ scores,
                                                           const int *__restrict__ order, int *__restrict__ parent,
                                                           long long num_params, long long P, unsigned k, Perturb f,
                                                           u64 seed, u64 generation)
{
    __shared__ int wave_count[THREADS / WAVE];
    const long long p = blockIdx.y;
    const double mine = key_of(scores[p]);
    // rank(p): every wave counts the members of its 64 slots of each tile that come before p
    int count = 0;
    for (long long base = 0; base < P; base += THREADS) {
        const long long q = base + threadIdx.x;
        count += popc64(ballot(q < P && before(key_of(q < P ? scores[q] : 0.0), q, mine, p)));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_count[threadIdx.x / WAVE] = count;
    __syncthreads();
    int rank = 0;
    for (int w = 0; w < THREADS / WAVE; ++w) rank += wave_count[w];

    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if ((long long)rank < P - (long long)k) { // (workgroup-uniform) the member keeps everything
        if (first) parent[p] = (int)p;
        return;
    }
    const Words w = rng_words(seed, generation, (u64)p, RNG_PBT, 0);
    const long long src = order[mulhi_range(w.w[0], k)];
    const long long lo = (long long)blockIdx.x * SLICE;
    const long long n = num_params - lo < SLICE ? num_params - lo : SLICE;
    const long long to = p * num_params + lo, from = src * num_params + lo;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        params[to + i] = params[from + i];
        exp_avg[to + i] = exp_avg[from + i];
        exp_avg_sq[to + i] = exp_avg_sq[from + i];
    }
    if (first) {
        parent[p] = (int)src;
        const double *h = hyper + src * HYPER_DOUBLES;
        double *mine_h = hyper + p * HYPER_DOUBLES;
        // lr is a double; columns 1-3 are floats held exactly, so the perturbed entropy_coef is rounded to float
        mine_h[0] = fmin(fmax(h[0] * ((w.w[1] >> 31) ? f.lr_up : f.lr_down), f.lr_lo), f.lr_hi);
        mine_h[1] = h[1];
        mine_h[2] = (double)(float)fmin(fmax(h[2] * ((w.w[2] >> 31) ? f.e_up : f.e_down), f.e_lo), f.e_hi);
        mine_h[3] = h[3];
    }
}

} // namespace pbt
} // namespace wurm
