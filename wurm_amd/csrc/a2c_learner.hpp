// a2c_learner.hpp — one A2C update of the 2 x 64 feed-forward actor-critic as three kernels:
//   a2c_ff_main_kernel    forward, return scan, loss derivatives and backward pass of a block of envs per workgroup;
//                         every workgroup writes ITS gradient (P floats) and loss sums to the caller's workspace
//   a2c_ff_reduce_kernel  sums the workgroups' partials in workgroup order into grad / losses
//   a2c_ff_apply_kernel   ||g|| in a fixed order (every workgroup computes the same bits), clip, Adam
// and the three with a member dimension in the grid (a2c_ff_main_kernel<GAE, Kind::Pop>, a2c_ff_*_pop_kernel): P updates at once
// and with an index list of columns per member (a2c_ff_main_kernel<GAE, Kind::League>, a2c_ff_*_league_kernel): a league
// No float atomics anywhere: two runs on the same inputs give the same bits.
//
// Main kernel.  A workgroup (256 threads) owns the envs [wg N / G, (wg + 1) N / G) with all T + 1 rows of each (the T
// policy inputs and the bootstrap input), in the local order row = t * nenv + i, cut into tiles of 64 rows.  All
// products are 64-row tiles against 64-wide weights out of LDS: a thread owns a 4 x 4 block of the 64 x 64 result and
// feeds it with 16-byte LDS reads (8 reads per 64 fmaf).  Rows of LDS images are 68 floats apart, which keeps the 16
// rows a 16-lane group reads on 16 different bank quartets.  W1 and the inputs go through LDS in chunks of 64 inputs,
// zero-padded to a multiple of 16 on both sides, so a padded product is an exact zero.
//   pass 1: forward of every tile -> softmax probabilities and value of every row, parked in the workspace
//           (6 floats per row; written and read by this workgroup only)
//   scan:   one thread per env walks its T rows backwards (the fp32 expression of rl.hip: a2c_returns_kernel).  The GAE
//           instantiation (a2c_ff_main_kernel<true>) builds R from the parked values instead and then walks forwards once:
//           the scan's adjoint (rl.hip: a2c_returns_backward_kernel) turns G = dL/dR into the term `extra` that R's
//           dependence on v adds to dL/dv, parked beside R
//   pass 2: forward of the tile again (skipped when the workgroup has a single tile: H1 / H2 are still in LDS), the loss
//           derivatives per row (GAE: dv = l'(v - R) + extra), then dZ2 = (dz Wp + dv Wv) [H2 > 0], dW2 += dZ2^T H1, dZ1 = (dZ2 W2) [H1 > 0],
//           dW1 += dZ1^T X.  dW2, the head and bias gradients accumulate in registers over the tiles; dW1 (up to 128 floats
//           per thread at E = 507) accumulates in the workgroup's own partial, read and written by the same thread.
// Rows past the workgroup's last row and the bootstrap rows get dz = dv = 0, so they add exact zeros everywhere.
// The products are fp32 fmaf chains in a fixed order (the build has -ffp-contract=off: every fmaf here is explicit); the
// bias and loss sums and the sum over the workgroups run in double.
#pragma once
#include "wurm_device.hpp"

namespace wurm {
namespace a2c {

constexpr int HID = 64;      // hidden units of both layers
constexpr int TILE = 64;     // rows per tile
constexpr int LD = 68;       // floats between rows of an LDS image
constexpr int CHUNK = 64;    // inputs per pass through LDS
constexpr int THREADS = 256;
constexpr int ROW_FLOATS = 8; // parked per row: p0..p3, v, R, extra (GAE only) (+ 1 unused: 32-byte rows)
constexpr int MAX_GROUPS = 256;

__host__ __device__ inline long long num_params(int E) { return 64LL * E + 64 + 4096 + 64 + 256 + 4 + 64 + 1; }
__host__ __device__ inline int padded_inputs(int E) { return (E + 15) & ~15; }
// floats per workgroup partial: dW1 with its rows padded to padded_inputs(E) (16-byte stores), the other seven blocks
// as they are packed, then the three loss sums; rounded up to 16 bytes
__host__ __device__ inline long long partial_stride(int E)
{
    return (64LL * padded_inputs(E) + (num_params(E) - 64LL * E) + 3 + 3) & ~3LL;
}

struct MainArgs {
    const float *params, *obs0, *obs;
    const long long *actions;
    const float *rewards;
    const uint8_t *dones;
    float *values_out; // nullable
    float *partials;   // (G, partial_stride)
    float *rows;       // (N (T + 1), ROW_FLOATS)
    long long N, T;
    int E, G, loss_kind;
    float gamma, entropy_coef, inv_B;
};

// what the GAE instantiation takes on top (the n-step kernel keeps its argument block as it is)
struct GaeArgs : MainArgs {
    float *returns_out; // nullable, (T, N)
    float gamma_lambda; // (float)(gamma * lambda), rounded by the caller
};

template <bool GAE> struct main_args { using type = MainArgs; };
template <> struct main_args<true> { using type = GaeArgs; };

// ---- population: P members of M envs each in one grid, blockIdx.y = member.  A member's part of the
// grid is the grid of a stand-alone update of its M envs — the same G, env ranges, tile and summation order — on pointers
// moved to its columns and rows, so its bits are those of the stand-alone update.
constexpr int HYPER_DOUBLES = 4; // a member's row of the hyper-parameter table: lr (as written), gamma, entropy_coef, gamma_lambda

// What the population instantiations take: member 0's pointers; N stays the envs per row of the (T, N, .) tensors, M of
// them belong to a member; gamma, entropy_coef and gamma_lambda come from the member's row of `hyper`.
template <class Base> struct PopArgs : Base {
    const double *hyper; // (P, HYPER_DOUBLES) on the device: floats held exactly, but for lr
    long long M;
};

// ---- league: the population with an INDEX LIST where it has a consecutive block.  Member a learns from
// the columns order[offsets[a] .. offsets[a + 1]) of the (T, N, .) tensors, N = K N_envs rows of a MultiSnake window, as
// MultiSnake.league_plan lays the two out (multi_league.hpp).  Nothing about the lists is known on the host: the grid is
// (min(N, 256), A) and member a's workgroups size themselves — M_a, G_a = min(M_a, 256), inv_B — from `offsets`, so
// that its part of the grid is again the grid of a stand-alone update of its M_a columns in list order.  Everything
// indexed by env goes through the list; the parked rows and the partials are indexed by list position.
template <class Base> struct LeagueArgs : Base { // N: all rows; G: the grid's x (an upper bound of every G_a)
    const double *hyper;        // (A, HYPER_DOUBLES)
    const int *order;           // (N)
    const long long *offsets;   // (A + 1)
    const uint8_t *learn;       // (A), nullable: 0 = this member sits the update out
};

// What member a of a league owns.  The offsets are clamped to [0, N] and made non-decreasing (a running maximum), so the
// members' lists are disjoint pieces of `order` whatever `offsets` holds: first + M <= N, and the M of all members sum
// to at most N.  `base` is the group index of the member's first partial, sum over b < a of min(M_b, 256): sums of
// integers, the same in every workgroup and kernel.  (A serial walk over a + 1 offsets per workgroup, all of it scalar.)
struct LeagueMember {
    long long first, M, base;
    int G;       // min(M, 256)
    float inv_B; // 1 / (M T), rounded as the host rounds 1.0f / (float)(M T)
};

__device__ __forceinline__ LeagueMember league_member(const long long *__restrict__ offsets, long long a, long long N,
                                                      long long T)
{
    LeagueMember m;
    long long lo = offsets[0];
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    m.base = 0;
    for (long long b = 0; b < a; ++b) {
        long long hi = offsets[b + 1];
        hi = hi < lo ? lo : (hi > N ? N : hi);
        m.base += hi - lo < MAX_GROUPS ? hi - lo : MAX_GROUPS;
        lo = hi;
    }
    long long hi = offsets[a + 1];
    hi = hi < lo ? lo : (hi > N ? N : hi);
    m.first = lo;
    m.M = hi - lo;
    m.G = (int)(m.M < MAX_GROUPS ? m.M : MAX_GROUPS);
    // The host forms 1.0f / (float)(M T), one correctly rounded fp32 division.  Here the quotient is taken in double and
    // rounded to float: the reciprocal of a 24-bit number is either exact (a power of two) or at least 2^-49 of itself
    // away from every 25-bit number, so the double quotient never sits on a float rounding boundary and the second
    // rounding gives the correctly rounded fp32 quotient — whatever the fp32 division of the build expands to.
    m.inv_B = (float)(1.0 / (double)(float)(m.M * T));
    return m;
}

// the three kinds of update: one agent, a population (PopArgs), a league (LeagueArgs)
enum class Kind { Alone, Pop, League };

template <bool GAE, Kind K> struct kernel_args { using type = typename main_args<GAE>::type; };
template <bool GAE> struct kernel_args<GAE, Kind::Pop> { using type = PopArgs<typename main_args<GAE>::type>; };
template <bool GAE> struct kernel_args<GAE, Kind::League> { using type = LeagueArgs<typename main_args<GAE>::type>; };

// acc[i][j] += sum_k A[4 tr + i][k] * B[tj + 16 j][k], k < K (a multiple of 4)
__device__ __forceinline__ void gemm_nt(const float *A, const float *B, int K, int tr, int tj, float (&acc)[4][4])
{
    const float *pa = A + 4 * tr * LD, *pb = B + tj * LD;
    for (int k = 0; k < K; k += 4) {
        float4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = *reinterpret_cast<const float4 *>(pa + i * LD + k);
            b[i] = *reinterpret_cast<const float4 *>(pb + 16 * i * LD + k);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = acc[i][j];
                s = fmaf(a[i].x, b[j].x, s);
                s = fmaf(a[i].y, b[j].y, s);
                s = fmaf(a[i].z, b[j].z, s);
                acc[i][j] = fmaf(a[i].w, b[j].w, s);
            }
    }
}

// acc[i][j] += sum_r A[r][4 tr + i] * B[r][4 tj + j], r < 64
__device__ __forceinline__ void gemm_tn(const float *A, const float *B, int tr, int tj, float (&acc)[4][4])
{
    const float *pa = A + 4 * tr, *pb = B + 4 * tj;
#pragma unroll 4
    for (int r = 0; r < TILE; ++r) {
        const float4 a = *reinterpret_cast<const float4 *>(pa + r * LD);
        const float4 b = *reinterpret_cast<const float4 *>(pb + r * LD);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
}

__device__ __forceinline__ float wave_sum_f32(float v) // fixed butterfly order: the same bits every run
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// d l(x) / dx of the value loss at x = v - R
__device__ __forceinline__ float value_loss_derivative(int loss_kind, float dl)
{
    if (loss_kind == 0) { // smooth_l1, beta = 1
        const float ad = fabsf(dl);
        return ad < 1.0f ? dl : (dl > 0.0f ? 1.0f : -1.0f);
    }
    return 2.0f * dl; // squared error
}

template <bool GAE, Kind K = Kind::Alone>
__global__ __launch_bounds__(THREADS) void a2c_ff_main_kernel(typename kernel_args<GAE, K>::type g)
{
    constexpr bool POP = K == Kind::Pop, LEAGUE = K == Kind::League;
    __shared__ __attribute__((aligned(16))) float Xs[TILE * LD], W1s[HID * LD], W2s[HID * LD], W2Ts[HID * LD];
    __shared__ __attribute__((aligned(16))) float H1s[TILE * LD], H2s[TILE * LD], dZ2s[TILE * LD], dZ1s[TILE * LD];
    __shared__ __attribute__((aligned(16))) float Wps[4 * HID], Wvs[HID], b1s[HID], b2s[HID], zs[TILE * 8];
    __shared__ float bhs[8];
    __shared__ const float *row_x[TILE]; // the row's input, nullptr past the workgroup's last row
    __shared__ long long row_env[TILE];
    __shared__ long long row_t[TILE];

    const int tid = (int)threadIdx.x, tr = tid >> 4, tj = tid & 15, lane = tid & 63, part = tid >> 6;
    if constexpr (POP) { // this member's columns, weights, workspace and hyper-parameters; from here on a stand-alone update
        const long long m = blockIdx.y, first = m * g.M;
        g.params += m * num_params(g.E);
        g.obs0 += first * g.E;
        g.obs += first * g.E;
        g.actions += first;
        g.rewards += first;
        g.dones += first;
        if (g.values_out != nullptr) g.values_out += first;
        g.partials += m * g.G * partial_stride(g.E);
        g.rows += first * (g.T + 1) * ROW_FLOATS;
        const double *h = g.hyper + m * HYPER_DOUBLES;
        g.gamma = (float)h[1];
        g.entropy_coef = (float)h[2];
        if constexpr (GAE) {
            g.gamma_lambda = (float)h[3];
            if (g.returns_out != nullptr) g.returns_out += first;
        }
    }
    const int *order = nullptr; // LEAGUE: the member's list; list position i is column order[i] of the inputs
    long long listed = 0;       // LEAGUE: M_a
    if constexpr (LEAGUE) { // this member's list, weights, workspace and hyper-parameters, sized here from `offsets`
        const long long m = blockIdx.y;
        const LeagueMember mem = league_member(g.offsets, m, g.N, g.T);
        // nothing to learn from, told to sit out, or a workgroup past this member's G_a: gone before LDS is touched
        if (mem.M == 0 || (g.learn != nullptr && g.learn[m] == 0) || (long long)blockIdx.x >= mem.G) return;
        g.params += m * num_params(g.E);
        g.partials += mem.base * partial_stride(g.E);
        g.rows += mem.first * (g.T + 1) * ROW_FLOATS;
        g.G = mem.G;
        g.inv_B = mem.inv_B;
        order = g.order + mem.first; // (first + M <= N: every read of it stays inside the N entries)
        listed = mem.M;
        const double *h = g.hyper + m * HYPER_DOUBLES;
        g.gamma = (float)h[1];
        g.entropy_coef = (float)h[2];
        if constexpr (GAE) g.gamma_lambda = (float)h[3];
    }
    const long long N = g.N, T = g.T; // N: envs per row of the inputs
    const int E = g.E, Epad = padded_inputs(E);
    long long owned; // the envs the grid's x shares out: all N, or the member's M
    if constexpr (POP) owned = g.M;
    else if constexpr (LEAGUE) owned = listed;
    else owned = N;
    const long long e0 = (long long)blockIdx.x * owned / g.G, e1 = ((long long)blockIdx.x + 1) * owned / g.G;
    const long long nenv = e1 - e0, rows = nenv * (T + 1), ntiles = (rows + TILE - 1) / TILE;
    const float *W1 = g.params, *b1 = W1 + 64LL * E, *W2 = b1 + 64, *b2 = W2 + 4096, *Wp = b2 + 64, *bp = Wp + 256,
                *Wv = bp + 4, *bv = Wv + 64;
    float *parked = g.rows + e0 * (T + 1) * ROW_FLOATS;
    float *partial = g.partials + (long long)blockIdx.x * partial_stride(E);

    for (int idx = tid; idx < HID * HID; idx += THREADS) {
        const int j = idx >> 6, k = idx & 63;
        const float w = W2[idx];
        W2s[j * LD + k] = w;
        W2Ts[k * LD + j] = w;
    }
    Wps[tid] = Wp[tid];
    if (tid < HID) {
        b1s[tid] = b1[tid];
        b2s[tid] = b2[tid];
        Wvs[tid] = Wv[tid];
    }
    if (tid < 4) bhs[tid] = bp[tid];
    if (tid == 4) bhs[4] = bv[0];

    int xs_c0 = -1; // the chunk of the current tile that Xs holds

    // all CHUNK columns of Xs are written: the columns past the last chunk's end are zeros, as the padded ones are
    // (gemm_tn reads all 64)
    auto load_x = [&](int c0) {
        for (int idx = tid; idx < TILE * CHUNK; idx += THREADS) {
            const int r = idx / CHUNK, k = idx % CHUNK, e = c0 + k;
            const float *x = row_x[r];
            Xs[r * LD + k] = (x != nullptr && e < E) ? x[e] : 0.0f;
        }
        xs_c0 = c0;
    };

    // rows of tile -> H1s, H2s (post-ReLU; a unit is live where its entry is > 0)
    auto forward = [&](long long tile) {
        __syncthreads(); // everybody is done with the previous tile's row table and images
        if (tid < TILE) {
            const long long lr = tile * TILE + tid;
            const float *x = nullptr;
            long long t = -1, env = 0;
            if (lr < rows) {
                t = lr / nenv;
                env = e0 + (lr - t * nenv);
                if constexpr (LEAGUE) {
                    env = order[env];
                    if (env < 0 || env >= N) env = -1; // not a column: zero input, no loss term, nothing read or written
                }
                if (!LEAGUE || env >= 0) x = t == 0 ? g.obs0 + env * E : g.obs + ((t - 1) * N + env) * E;
            }
            row_x[tid] = x;
            row_env[tid] = env;
            row_t[tid] = t;
        }
        float acc[4][4] = {};
        for (int c0 = 0; c0 < Epad; c0 += CHUNK) {
            const int kc = min(CHUNK, Epad - c0);
            __syncthreads();
            load_x(c0);
            for (int idx = tid; idx < HID * kc; idx += THREADS) {
                const int j = idx / kc, k = idx - j * kc, e = c0 + k;
                W1s[j * LD + k] = e < E ? W1[(long long)j * E + e] : 0.0f;
            }
            __syncthreads();
            gemm_nt(Xs, W1s, kc, tr, tj, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = acc[i][j] + b1s[tj + 16 * j];
                H1s[(4 * tr + i) * LD + tj + 16 * j] = z > 0.0f ? z : 0.0f;
                acc[i][j] = 0.0f;
            }
        __syncthreads();
        gemm_nt(H1s, W2s, HID, tr, tj, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = acc[i][j] + b2s[tj + 16 * j];
                H2s[(4 * tr + i) * LD + tj + 16 * j] = z > 0.0f ? z : 0.0f;
            }
        __syncthreads();
    };

    // ---------------------------------------------------------------- pass 1: probabilities and values of every row
    for (long long tile = 0; tile < ntiles; ++tile) {
        forward(tile);
        {
            const float *h = H2s + lane * LD;
            float s = 0.0f, sv = 0.0f;
#pragma unroll
            for (int q = 0; q < HID; q += 4) {
                const float4 x = *reinterpret_cast<const float4 *>(h + q);
                const float4 w = *reinterpret_cast<const float4 *>(Wps + part * HID + q);
                s = fmaf(x.x, w.x, s);
                s = fmaf(x.y, w.y, s);
                s = fmaf(x.z, w.z, s);
                s = fmaf(x.w, w.w, s);
                if (part == 0) {
                    const float4 u = *reinterpret_cast<const float4 *>(Wvs + q);
                    sv = fmaf(x.x, u.x, sv);
                    sv = fmaf(x.y, u.y, sv);
                    sv = fmaf(x.z, u.z, sv);
                    sv = fmaf(x.w, u.w, sv);
                }
            }
            zs[lane * 8 + part] = s + bhs[part];
            if (part == 0) zs[lane * 8 + 4] = sv + bhs[4];
        }
        __syncthreads();
        if (tid < TILE && row_t[tid] >= 0) {
            const float z0 = zs[tid * 8], z1 = zs[tid * 8 + 1], z2 = zs[tid * 8 + 2], z3 = zs[tid * 8 + 3];
            const float v = zs[tid * 8 + 4];
            const float m = fmaxf(fmaxf(z0, z1), fmaxf(z2, z3));
            const float x0 = expf(z0 - m), x1 = expf(z1 - m), x2 = expf(z2 - m), x3 = expf(z3 - m);
            const float sum = ((x0 + x1) + x2) + x3;
            float *o = parked + (tile * TILE + tid) * ROW_FLOATS;
            *reinterpret_cast<float4 *>(o) = make_float4(x0 / sum, x1 / sum, x2 / sum, x3 / sum);
            o[4] = v;
            if (g.values_out != nullptr && row_t[tid] < T && (!LEAGUE || row_env[tid] >= 0))
                g.values_out[row_t[tid] * N + row_env[tid]] = v;
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---------------------------------------------------------------- return scan (rl.hip: a2c_returns_kernel)
    for (long long i = tid; i < nenv; i += THREADS) {
        long long env = e0 + i;
        if constexpr (LEAGUE) {
            env = order[env];
            if (env < 0 || env >= N) continue; // (pass 2 does not read what this would have parked)
        }
        if constexpr (GAE) {
            // backwards: delta_t = r_t + gamma v_{t+1} nd_t - v_t, gae_t = delta_t + gamma_lambda nd_t gae_{t+1}, R = gae + v
            float gae = 0.0f, next = parked[(T * nenv + i) * ROW_FLOATS + 4];
            for (long long t = T - 1; t >= 0; --t) {
                float *o = parked + (t * nenv + i) * ROW_FLOATS;
                const float nd = g.dones[t * N + env] ? 0.0f : 1.0f, v = o[4];
                const float delta = g.rewards[t * N + env] + g.gamma * next * nd - v;
                gae = delta + g.gamma_lambda * nd * gae;
                const float R = gae + v;
                o[5] = R;
                if (g.returns_out != nullptr) g.returns_out[t * N + env] = R;
                next = v;
            }
            // forwards, the adjoint (rl.hip: a2c_returns_backward_kernel) with G_t = dL/dR_t = -l'(v_t - R_t) before the
            // 1 / B that pass 2 applies: A_t = G_t + gamma_lambda nd_{t-1} A_{t-1} is dL/dgae_t, and v_t enters R_t, delta_t
            // and delta_{t-1}: extra_t = G_t - A_t + gamma nd_{t-1} A_{t-1}.  The bootstrap value gets no gradient.
            float A_prev = 0.0f, nd_prev = 0.0f;
            for (long long t = 0; t < T; ++t) {
                float *o = parked + (t * nenv + i) * ROW_FLOATS;
                const float G = -value_loss_derivative(g.loss_kind, o[4] - o[5]);
                const float A = G + g.gamma_lambda * nd_prev * A_prev;
                o[6] = G - A + g.gamma * nd_prev * A_prev;
                A_prev = A;
                nd_prev = g.dones[t * N + env] ? 0.0f : 1.0f;
            }
        } else {
            float R = parked[(T * nenv + i) * ROW_FLOATS + 4] * (g.dones[(T - 1) * N + env] ? 0.0f : 1.0f);
            for (long long t = T - 1; t >= 0; --t) {
                const float nd = g.dones[t * N + env] ? 0.0f : 1.0f;
                R = g.rewards[t * N + env] + g.gamma * R * nd;
                parked[(t * nenv + i) * ROW_FLOATS + 5] = R;
            }
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---------------------------------------------------------------- pass 2: derivatives and weight gradients
    float gW2[4][4] = {};            // dW2[4 tr + i][4 tj + j]
    float gWp = 0.0f, gWv = 0.0f;    // dWp[part][lane]; dWv[lane] (part 0)
    // The bias gradients and the loss sums are plain sums of signed per-row terms that largely cancel (dbv is one number:
    // sum of (v - R) / B), so a sequential fp32 sum loses what torch's pairwise reductions keep: they run in double.
    double gb = 0.0;                 // part 1: db2[lane]; part 2: db1[lane]; part 3, lane < 5: dbp / dbv
    double lv = 0.0, lp = 0.0, le = 0.0; // loss sums (thread 0)
    const float eps32 = 1.1920928955078125e-07f, hi32 = 1.0f - eps32;

    for (long long tile = 0; tile < ntiles; ++tile) {
        if (ntiles > 1) forward(tile);
        if (tid < TILE) {
            float d[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            float rv = 0.0f, rp = 0.0f, re = 0.0f;
            const long long t = row_t[tid];
            if (t >= 0 && t < T && (!LEAGUE || row_env[tid] >= 0)) {
                const float *o = parked + (tile * TILE + tid) * ROW_FLOATS;
                const float p[4] = {o[0], o[1], o[2], o[3]};
                const float v = o[4], R = o[5];
                long long a = g.actions[t * N + row_env[tid]];
                a = a < 0 ? 0 : (a > 3 ? 3 : a);
                const float dl = v - R, adv = R - v;
                float dv;
                if (g.loss_kind == 0) { // smooth_l1, beta = 1
                    const float ad = fabsf(dl);
                    rv = ad < 1.0f ? 0.5f * dl * dl : ad - 0.5f;
                    dv = ad < 1.0f ? dl : (dl > 0.0f ? 1.0f : -1.0f);
                } else { // squared error
                    rv = dl * dl;
                    dv = 2.0f * dl;
                }
                if constexpr (GAE) dv += o[6]; // R is a function of the values: what comes back through it
                float gk[4], dot = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool inside = p[k] > eps32 && p[k] < hi32; // the clamp passes gradient strictly inside only
                    const float lg = logf(fminf(fmaxf(p[k], eps32), hi32));
                    re -= p[k] * lg;
                    gk[k] = g.entropy_coef * (lg + (inside ? 1.0f : 0.0f));
                    if (k == (int)a) {
                        rp = -(adv * lg);
                        if (inside) gk[k] -= adv / p[k];
                    }
                    dot = fmaf(gk[k], p[k], dot);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = p[k] * (gk[k] - dot) * g.inv_B;
                d[4] = dv * g.inv_B;
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) zs[tid * 8 + k] = d[k];
            lv += (double)wave_sum_f32(rv);
            lp += (double)wave_sum_f32(rp);
            le += (double)wave_sum_f32(re);
        }
        __syncthreads();
        // head gradients: sums over the tile's rows, in row order
        for (int r = 0; r < TILE; ++r) {
            const float h = H2s[r * LD + lane];
            gWp = fmaf(zs[r * 8 + part], h, gWp);
            if (part == 0) gWv = fmaf(zs[r * 8 + 4], h, gWv);
            if (part == 3 && lane < 5) gb += (double)zs[r * 8 + lane];
        }
        // dZ2[r][k] = (sum_a dz[r][a] Wp[a][k] + dv[r] Wv[k]) where unit k of layer 2 is live
        {
            const float w0 = Wps[lane], w1 = Wps[HID + lane], w2 = Wps[2 * HID + lane], w3 = Wps[3 * HID + lane];
            const float wv = Wvs[lane];
#pragma unroll 4
            for (int r = part; r < TILE; r += 4) {
                float s = zs[r * 8] * w0;
                s = fmaf(zs[r * 8 + 1], w1, s);
                s = fmaf(zs[r * 8 + 2], w2, s);
                s = fmaf(zs[r * 8 + 3], w3, s);
                s = fmaf(zs[r * 8 + 4], wv, s);
                dZ2s[r * LD + lane] = H2s[r * LD + lane] > 0.0f ? s : 0.0f;
            }
        }
        __syncthreads();
        if (part == 1)
            for (int r = 0; r < TILE; ++r) gb += (double)dZ2s[r * LD + lane];
        gemm_tn(dZ2s, H1s, tr, tj, gW2);
        {
            float acc[4][4] = {};
            gemm_nt(dZ2s, W2Ts, HID, tr, tj, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int o = (4 * tr + i) * LD + tj + 16 * j;
                    dZ1s[o] = H1s[o] > 0.0f ? acc[i][j] : 0.0f;
                }
        }
        __syncthreads();
        if (part == 2)
            for (int r = 0; r < TILE; ++r) gb += (double)dZ1s[r * LD + lane];
        for (int c0 = 0; c0 < Epad; c0 += CHUNK) {
            if (xs_c0 != c0) { // (the forward pass of this tile left its last chunk behind)
                __syncthreads();
                load_x(c0);
                __syncthreads();
            }
            float acc[4][4] = {};
            gemm_tn(dZ1s, Xs, tr, tj, acc);
            if (c0 + 4 * tj < Epad) // (the partial has Epad columns; up to there padded columns hold exact zeros)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float4 *o = reinterpret_cast<float4 *>(partial + (4 * tr + i) * Epad + c0 + 4 * tj);
                    float4 v = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                    if (tile != 0) {
                        const float4 old = *o;
                        v = make_float4(old.x + v.x, old.y + v.y, old.z + v.z, old.w + v.w);
                    }
                    *o = v;
                }
        }
        if (ntiles > 1) xs_c0 = -1; // the next tile has other rows
    }

    float *o = partial + 64 * Epad;
    if (part == 2) o[lane] = (float)gb; // b1
    o += 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(o + (4 * tr + i) * HID + 4 * tj) =
            make_float4(gW2[i][0], gW2[i][1], gW2[i][2], gW2[i][3]);
    o += 4096;
    if (part == 1) o[lane] = (float)gb; // b2
    o += 64;
    o[part * HID + lane] = gWp;
    o += 256;
    if (part == 3 && lane < 4) o[lane] = (float)gb; // bp
    o += 4;
    if (part == 0) o[lane] = gWv;
    o += 64;
    if (part == 3 && lane == 4) o[0] = (float)gb; // bv
    o += 1;
    if (tid == 0) {
        o[0] = (float)lv;
        o[1] = (float)lp;
        o[2] = (float)le;
    }
}

// grad[i] = sum over the workgroups, in workgroup order; the three loss sums behind it become means
__device__ __forceinline__ void a2c_ff_reduce_body(const float *__restrict__ partials, int G, int E, float inv_B,
                                                   float *__restrict__ grad, float *__restrict__ losses)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x, P = num_params(E), stride = partial_stride(E);
    if (i >= P + 3) return;
    const int Epad = padded_inputs(E);
    const long long src = i < 64LL * E ? (i / E) * Epad + i % E : i - 64LL * E + 64LL * Epad; // dW1 rows are padded
    double s = 0.0; // (up to 256 signed terms per element: summed in double, rounded once)
#pragma unroll 8
    for (int w = 0; w < G; ++w) s += (double)partials[w * stride + src];
    if (i < P)
        grad[i] = (float)s;
    else
        losses[i - P] = (float)(s * (double)inv_B);
}

__global__ __launch_bounds__(THREADS) void a2c_ff_reduce_kernel(const float *__restrict__ partials, int G, int E,
                                                                float inv_B, float *__restrict__ grad,
                                                                float *__restrict__ losses)
{
    a2c_ff_reduce_body(partials, G, E, inv_B, grad, losses);
}

// member blockIdx.y: its G partials -> its row of grad (P, num_params) and of losses (P, 3)
__global__ __launch_bounds__(THREADS) void a2c_ff_reduce_pop_kernel(const float *__restrict__ partials, int G, int E,
                                                                    float inv_B, float *__restrict__ grad,
                                                                    float *__restrict__ losses)
{
    const long long m = blockIdx.y;
    a2c_ff_reduce_body(partials + m * G * partial_stride(E), G, E, inv_B, grad + m * num_params(E), losses + 3 * m);
}

// league member blockIdx.y: its G_a partials, found and sized by league_member as the main kernel found them -> its row of
// grad and of losses.  A member that did not learn (no columns, or learn[a] == 0) wrote no partials: its rows are zeros.
__global__ __launch_bounds__(THREADS) void a2c_ff_reduce_league_kernel(const float *__restrict__ partials,
                                                                       const long long *__restrict__ offsets,
                                                                       const uint8_t *__restrict__ learn, long long N,
                                                                       long long T, int E, float *__restrict__ grad,
                                                                       float *__restrict__ losses)
{
    const long long m = blockIdx.y, P = num_params(E);
    const LeagueMember mem = league_member(offsets, m, N, T);
    if (mem.M == 0 || (learn != nullptr && learn[m] == 0)) {
        const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
        if (i < P) grad[m * P + i] = 0.0f;
        else if (i < P + 3) losses[3 * m + (i - P)] = 0.0f;
        return;
    }
    a2c_ff_reduce_body(partials + mem.base * partial_stride(E), mem.G, E, mem.inv_B, grad + m * P, losses + 3 * m);
}

constexpr int APPLY_PER_BLOCK = 4 * THREADS;

// Every workgroup forms sum g^2 over ALL of grad in the same order (so they all hold the same bits), then clips and
// steps its own 1024 parameters.  step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), w1 = 1 - beta1 and
// w2 = 1 - beta2 come from the host, computed in double as torch.optim.Adam does.
__device__ __forceinline__ void a2c_ff_apply_body(float *__restrict__ params, const float *__restrict__ grad,
                                                  float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                  float *__restrict__ grad_norm, float step_size, float bc2_sqrt,
                                                  float beta2, float w1, float w2, float eps, float max_norm,
                                                  long long P)
{
    __shared__ float red[THREADS];
    const int tid = (int)threadIdx.x;
    float s = 0.0f;
    for (long long i = tid; i < P; i += THREADS) s = fmaf(grad[i], grad[i], s);
    red[tid] = s;
    __syncthreads();
    for (int w = THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const float norm = sqrtf(red[0]);
    if (blockIdx.x == 0 && tid == 0 && grad_norm != nullptr) grad_norm[0] = norm;
    float scale = 1.0f;
    if (max_norm > 0.0f) scale = fminf(max_norm / (norm + 1e-6f), 1.0f);
    const long long base = (long long)blockIdx.x * APPLY_PER_BLOCK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long i = base + q * THREADS + tid;
        if (i < P) {
            const float gi = grad[i] * scale;
            const float m = exp_avg[i] + w1 * (gi - exp_avg[i]);
            const float u = beta2 * exp_avg_sq[i] + w2 * gi * gi;
            exp_avg[i] = m;
            exp_avg_sq[i] = u;
            params[i] = params[i] - step_size * (m / (sqrtf(u) / bc2_sqrt + eps));
        }
    }
}

__global__ __launch_bounds__(THREADS) void a2c_ff_apply_kernel(float *__restrict__ params,
                                                               const float *__restrict__ grad,
                                                               float *__restrict__ exp_avg,
                                                               float *__restrict__ exp_avg_sq,
                                                               float *__restrict__ grad_norm, float step_size,
                                                               float bc2_sqrt, float beta2, float w1, float w2,
                                                               float eps, float max_norm, long long P)
{
    a2c_ff_apply_body(params, grad, exp_avg, exp_avg_sq, grad_norm, step_size, bc2_sqrt, beta2, w1, w2, eps, max_norm, P);
}

// member blockIdx.y steps its row of the four (P, num_params) buffers with its own learning rate.  step_size is what the
// host forms for a stand-alone apply, lr / (1 - beta1^step) divided in double and rounded to float once: the table holds
// lr as the double the host would divide, bc1 is the host's 1 - beta1^step, and the double division and the conversion
// round to nearest here as they do there.
__global__ __launch_bounds__(THREADS) void a2c_ff_apply_pop_kernel(float *__restrict__ params,
                                                                   const float *__restrict__ grad,
                                                                   float *__restrict__ exp_avg,
                                                                   float *__restrict__ exp_avg_sq,
                                                                   float *__restrict__ grad_norm,
                                                                   const double *__restrict__ hyper, double bc1,
                                                                   float bc2_sqrt, float beta2, float w1, float w2,
                                                                   float eps, float max_norm, long long P)
{
    const long long m = blockIdx.y, o = m * P;
    const float step_size = (float)(hyper[m * HYPER_DOUBLES] / bc1);
    a2c_ff_apply_body(params + o, grad + o, exp_avg + o, exp_avg_sq + o, grad_norm != nullptr ? grad_norm + m : nullptr,
                      step_size, bc2_sqrt, beta2, w1, w2, eps, max_norm, P);
}

// the same for a league: a member that did not learn (as the reduce kernel decides it) keeps its rows of params, exp_avg
// and exp_avg_sq bit for bit — an Adam step on a zero gradient would still move them — and gets grad_norm = 0
__global__ __launch_bounds__(THREADS) void a2c_ff_apply_league_kernel(float *__restrict__ params,
                                                                      const float *__restrict__ grad,
                                                                      float *__restrict__ exp_avg,
                                                                      float *__restrict__ exp_avg_sq,
                                                                      float *__restrict__ grad_norm,
                                                                      const double *__restrict__ hyper,
                                                                      const long long *__restrict__ offsets,
                                                                      const uint8_t *__restrict__ learn, long long N,
                                                                      double bc1, float bc2_sqrt, float beta2, float w1,
                                                                      float w2, float eps, float max_norm, long long P)
{
    const long long m = blockIdx.y, o = m * P;
    if (league_member(offsets, m, N, 1).M == 0 || (learn != nullptr && learn[m] == 0)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm != nullptr) grad_norm[m] = 0.0f;
        return;
    }
    const float step_size = (float)(hyper[m * HYPER_DOUBLES] / bc1);
    a2c_ff_apply_body(params + o, grad + o, exp_avg + o, exp_avg_sq + o, grad_norm != nullptr ? grad_norm + m : nullptr,
                      step_size, bc2_sqrt, beta2, w1, w2, eps, max_norm, P);
}

} // namespace a2c
} // namespace wurm
