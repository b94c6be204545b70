// single_device.hpp — the device code of the one-env-per-wavefront SingleSnake / SimpleGridworld kernels: the state of an
// env in registers (Env, Geo), step / reset / observation on it, the scalar carry of the rollouts (Fast) and the helpers of
// the lean and 9 x 9 rollout loops.  Shared by every translation unit that steps an env this way (the kernels of
// single_kernels.hpp, the fall-back paths of the lane kernels, the fused actors of policy_rollout.hpp / policy_wide.hpp).
//
// Replaces the reference's op sequences (cited against oscarknagg/wurm):
//   SingleSnake.step      wurm/envs/single_snake.py:197-304   (~60 torch op dispatches + 2-3 host syncs)
//   SingleSnake._observe  wurm/envs/single_snake.py:104-195
//   SingleSnake.reset     wurm/envs/single_snake.py:322-387
//   determine_orientations wurm/utils.py:36-65, food respawn wurm/utils.py:181-232
//   SimpleGridworld.*     wurm/envs/simple_gridworld.py:88-268
// One env per wavefront, the env's cells spread over the lanes (cell c = lane + 64*k), food/head channels held as per-lane
// bit sets, the body channel as per-lane ints, per-env scalars wave-uniform via ballots and DPP wave reductions (per-lane
// partials + one reduction, never one ballot per k), no host sync, no MFMA (integer/index work, HBM-bound).
// The only LDS use is a one-byte-per-cell class map for the cropped `partial_n` observation on grids > 128 cells and
// for the general (irregular-state) orientation stencil.
#pragma once

#include "step_args.hpp"
#include <cstdlib>

namespace wurm {

// cells per lane: the bucket of Env<CPL> that holds an S x S grid (host side: which instantiation a launch takes)
static int pick_cpl(int S)
{
    int need = (S * S + 63) / 64;
    const int opts[] = {2, 4, 8, 16, 24, 32, 48, 64};
    for (int o : opts)
        if (need <= o) return o;
    return -1;
}

// ------------------------------------------------------------------------------------------------ state

template <int CPL>
struct Env {
    int body[CPL]; // body channel (SingleSnake only), cell lane + 64k
    u64 food;      // bit k: food at cell lane + 64k
    u64 head;      // bit k: head / agent at cell lane + 64k
};

struct Geo {
    int S, C, lane;
    float rcpS;
    u64 valid;    // bit k: lane + 64k < C
    u64 interior; // bit k: cell is not on the border ring
};

template <int CPL>
__device__ __forceinline__ Geo make_geo(int S)
{
    Geo g;
    g.S = S;
    g.C = S * S;
    g.lane = (int)(threadIdx.x & 63u);
    g.rcpS = 1.0f / (float)S;
    g.valid = 0;
    g.interior = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if (c < g.C) {
            g.valid |= 1ull << k;
            int y = div_size(c, g.rcpS), x = c - y * S;
            if (y >= 1 && y <= S - 2 && x >= 1 && x <= S - 2) g.interior |= 1ull << k;
        }
    }
    return g;
}

template <int CPL, bool SNAKE>
__device__ __forceinline__ void load_state(const float *__restrict__ envp, const Geo &g, Env<CPL> &e)
{
    float f[CPL], h[CPL], b[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        bool v = (g.valid >> k) & 1;
        f[k] = v ? envp[c] : 0.0f;
        h[k] = v ? envp[g.C + c] : 0.0f;
        b[k] = (SNAKE && v) ? envp[2 * g.C + c] : 0.0f;
    }
    e.food = 0;
    e.head = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        if (f[k] > 0.5f) e.food |= 1ull << k;
        if (h[k] > 0.5f) e.head |= 1ull << k;
        e.body[k] = SNAKE ? __float2int_rn(b[k]) : 0;
    }
}

template <int CPL, bool SNAKE>
__device__ __forceinline__ void store_state(float *__restrict__ envp, const Geo &g, const Env<CPL> &e)
{
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if ((g.valid >> k) & 1) {
            envp[c] = ((e.food >> k) & 1) ? 1.0f : 0.0f;
            envp[g.C + c] = ((e.head >> k) & 1) ? 1.0f : 0.0f;
            if (SNAKE) envp[2 * g.C + c] = (float)e.body[k];
        }
    }
}

constexpr int NO_CELL = 1 << 20;

// lowest cell (row-major) whose bit is set in the per-lane bit set `bits` (bit k <=> cell lane + 64k), or -1.
// One per-lane ctz + one DPP min reduction — no per-k ballots (they cost two SGPRs each and, fully unrolled for
// large grids, drown the kernel in SGPR spills).
__device__ __forceinline__ int first_cell(u64 bits, int lane)
{
    int mine = bits ? lane + 64 * (__ffsll((long long)bits) - 1) : NO_CELL;
    int c = wave_min_i32(mine);
    return c >= NO_CELL ? -1 : c;
}

template <int CPL>
__device__ __forceinline__ int find_head(const Env<CPL> &e)
{
    return first_cell(e.head, (int)(threadIdx.x & 63u));
}

// ------------------------------------------------------------------------------------------------ orientation

// General form of determine_orientations (wurm/utils.py:36-65) for states that are not a well-formed snake
// (e.g. a done env stepped again before reset): neck map in LDS, 4-tap stencil, wave max, first argmax.
template <int CPL>
__device__ __forceinline__ int slow_orientation(const Env<CPL> &e, const Geo &g, int L, signed char *lds)
{
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if ((g.valid >> k) & 1) {
            int r = e.body[k] - (L - 2);                   // utils.py:51-53 relu(body - (L-2))
            lds[c] = (signed char)(r <= 0 ? 0 : 2 * r - 3); // utils.py:54-55: r=1 -> -1 (neck), r=2 -> +1 (head)
        }
    }
    wave_lds_sync();
    int best0 = -128, best1 = -128, best2 = -128, best3 = -128;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if ((g.valid >> k) & 1) {
            int y = div_size(c, g.rcpS), x = c - y * g.S;
            int own = lds[c];
            int n0 = y >= 1 ? lds[c - g.S] : 0;       // tap (-1, 0)
            int n1 = x <= g.S - 2 ? lds[c + 1] : 0;   // tap ( 0,+1)
            int n2 = y <= g.S - 2 ? lds[c + g.S] : 0; // tap (+1, 0)
            int n3 = x >= 1 ? lds[c - 1] : 0;         // tap ( 0,-1)
            best0 = max(best0, n0 - own);
            best1 = max(best1, n1 - own);
            best2 = max(best2, n2 - own);
            best3 = max(best3, n3 - own);
        }
    }
    best0 = wave_max_i32(best0);
    best1 = wave_max_i32(best1);
    best2 = wave_max_i32(best2);
    best3 = wave_max_i32(best3);
    int o = 0, bv = best0; // utils.py:63 argmax, first maximum wins
    if (best1 > bv) { bv = best1; o = 1; }
    if (best2 > bv) { bv = best2; o = 2; }
    if (best3 > bv) { bv = best3; o = 3; }
    wave_lds_sync();
    return uniform(o);
}

// determine_orientations (wurm/utils.py:36-65) of the env in registers.  Well-formed snake (exactly one cell == L
// and one == L-1, L >= 2): the filter response is 2 only for the tap pointing from the neck to the head, so the
// orientation follows from the two cells; anything else takes the exact stencil path.
// determine_orientations (wurm/utils.py:36-65) of the env in registers.  Well-formed snake (exactly one cell == L
// and one == L-1, L >= 2): the filter response is 2 only for the tap pointing from the neck to the head, so the
// orientation follows from the two cells; anything else takes the exact stencil path.
// top_two: count of cells equal to L and to L-1 and the lowest such cells (per-lane partials + 3 wave reductions).
template <int CPL>
__device__ __forceinline__ void top_two(const Env<CPL> &e, const Geo &g, int L, int &cntL, int &cntN, int &cellL,
                                        int &cellN)
{
    int packed = 0, cL = NO_CELL, cN = NO_CELL;
#pragma unroll
    for (int k = CPL - 1; k >= 0; --k) {
        const bool v = (g.valid >> k) & 1;
        if (v && e.body[k] == L) { packed += 1; cL = g.lane + 64 * k; }
        if (v && e.body[k] == L - 1) { packed += 1 << 16; cN = g.lane + 64 * k; }
    }
    packed = wave_sum_i32(packed);
    cntL = packed & 0xffff;
    cntN = packed >> 16;
    cellL = wave_min_i32(cL);
    cellN = wave_min_i32(cN);
}

template <int CPL>
__device__ __forceinline__ int orientation_of(const Env<CPL> &e, const Geo &g, int L, signed char *lds)
{
    int cntL, cntN, cellL, cellN;
    top_two<CPL>(e, g, L, cntL, cntN, cellL, cellN);
    if (cntL == 1 && cntN == 1 && L >= 2) {
        int yL = div_size(cellL, g.rcpS), xL = cellL - yL * g.S;
        int yN = div_size(cellN, g.rcpS), xN = cellN - yN * g.S;
        int dy = yL - yN, dx = xL - xN;
        return (dy == 0 && dx == 1) ? 1 : (dy == 1 && dx == 0) ? 2 : (dy == 0 && dx == -1) ? 3 : 0;
    }
    return slow_orientation<CPL>(e, g, L, lds);
}

// ------------------------------------------------------------------------------------------------ food respawn

// _get_food_addition (single_snake.py:306-320, simple_gridworld.py:209-223): +1 food on one uniformly random
// interior cell with nothing on it.  RNG form: the K-th free cell in row-major order, K = mulhi(word, n_free).
template <int CPL, bool SNAKE, bool WRITE>
__device__ __forceinline__ void add_food(Env<CPL> &e, const Geo &g, float *__restrict__ envp, bool use_inject,
                                         int inject_cell, u32 word)
{
    if (use_inject) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            int c = g.lane + 64 * k;
            if (c == inject_cell && ((g.valid >> k) & 1)) {
                e.food |= 1ull << k;
                if (WRITE) envp[c] = 1.0f;
            }
        }
        return;
    }
    const u64 occupied = e.food | e.head;
    u64 fr = 0; // bit k: cell lane + 64k is free
#pragma unroll
    for (int k = 0; k < CPL; ++k)
        if (((g.interior >> k) & 1) && !((occupied >> k) & 1) && (!SNAKE || e.body[k] == 0)) fr |= 1ull << k;
    const int n_free = wave_sum_i32(__popcll(fr));
    if (n_free == 0) return;
    const int K = (int)mulhi_range(word, (u32)n_free);
    // row-major order = k-major, lane-minor: walk the k planes (NOT unrolled: one live ballot at a time)
    int base = 0;
#pragma unroll 1
    for (int k = 0; k < CPL; ++k) {
        const bool b = (fr >> k) & 1;
        const u64 m = ballot(b);
        const int cnt = popc64(m);
        if (K < base + cnt) {
            if (b && base + rank_below(m) == K) {
                e.food |= 1ull << k;
                if (WRITE) envp[g.lane + 64 * k] = 1.0f;
            }
            break;
        }
        base += cnt;
    }
}

// ------------------------------------------------------------------------------------------------ step

struct StepOut {
    long long action; // sanitised action (SingleSnake)
    int headcell;     // head cell after the move, -1 if it left the grid
    float reward;
    int done, selfc, edgec;
    int foodcell;     // small_step only: the food cell after the step (-1: none); -2: the generic path ran
};

// step_core for grids of at most 128 cells whose state is a well-formed snake (exactly one head, on the unique maximum
// L >= 2 of the body channel; exactly one cell L - 1; at most one food cell; no negative values) — the state every
// per-call step of a reset-after-done loop sees.  Same transition, but every wave-level quantity comes from BALLOTS of
// per-lane compares (a v_cmp into an SGPR pair + s_bcnt1 / s_ff1) instead of DPP butterfly reductions: head and food
// cells are the set bits of two masks, L is the body value under the head (one v_readlane), "unique maximum" is
// popc(body == L) == 1 && no lane has body > L, the neck is the set bit of (body == L - 1).  PMC on round 1's
// step_kernel<2> at 65 536 envs: 404 VALU + 237 SALU per env, six compiler-emitted DPP reductions (~20 instructions
// each) among them, and the kernel was issue-bound at 2.1x the time its HBM traffic needs.  Returns false (nothing
// touched) if the state is anything else; step_core then runs its general path.
template <bool WRITE>
__device__ __forceinline__ bool small_step(Env<2> &e, const Geo &g, float *__restrict__ envp, long long a_in, StepOut &out,
                                           u64 seed, u64 call, u64 env_id, bool use_inject, int inject_cell)
{
    const int S = g.S, C = g.C, lane = g.lane;
    const u64 H0 = ballot((e.head & 1) != 0), H1 = ballot((e.head & 2) != 0);
    const u64 F0 = ballot((e.food & 1) != 0), F1 = ballot((e.food & 2) != 0);
    if (popc64(H0) + popc64(H1) != 1 || popc64(F0) + popc64(F1) > 1) return false;
    const int hc = H0 ? first_bit(H0) : 64 + first_bit(H1);
    const int fc = F0 ? first_bit(F0) : (F1 ? 64 + first_bit(F1) : -1);
    const int L = lane_value(hc < 64 ? e.body[0] : e.body[1], hc & 63);           // single_snake.py:210 snake_sizes
    if (L < 2) return false;
    const u64 above = ballot(e.body[0] > L || e.body[1] > L || e.body[0] < 0 || e.body[1] < 0);
    const u64 M0 = ballot(e.body[0] == L), M1 = ballot(e.body[1] == L);
    const u64 N0 = ballot(e.body[0] == L - 1), N1 = ballot(e.body[1] == L - 1);
    if (above != 0 || popc64(M0) + popc64(M1) != 1 || popc64(N0) + popc64(N1) != 1) return false;
    const int neck = N0 ? first_bit(N0) : 64 + first_bit(N1);
    // orientation (wurm/utils.py:36-65) from the two newest cells, as orientation_of
    const int hy = div_size(hc, g.rcpS), hx = hc - hy * S;
    const int yN = div_size(neck, g.rcpS), xN = neck - yN * S;
    const int dy = hy - yN, dx = hx - xN;
    const int o = (dy == 0 && dx == 1) ? 1 : (dy == 1 && dx == 0) ? 2 : (dy == 0 && dx == -1) ? 3 : 0;
    long long a = a_in;
    if ((long long)o == a) a += 2;                                                  // :221-222
    a = a % 4;
    const int ai = (int)(((a % 4) + 4) % 4);
    const int ny = hy - tap_y(ai), nx = hx - tap_x(ai);                            // :225-233
    const bool inside = ny >= 0 && ny < S && nx >= 0 && nx < S;
    const int nh = inside ? ny * S + nx : -1;
    const bool EAT = inside && nh == fc;                                           // :242
    const int under = inside ? lane_value(nh < 64 ? e.body[0] : e.body[1], nh & 63) : 0;
    const bool SELFC = inside && (EAT ? under : max(under - 1, 0)) > 0;            // :252 (after the decay)
    const int grow = L + (EAT ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = lane + 64 * k;
        const int b0 = e.body[k];
        int b = EAT ? b0 : max(b0 - 1, 0);                                         // :246-249
        if (c == nh) b += grow;                                                    // :258-262
        if (WRITE && b != b0) envp[2 * C + c] = (float)b;
        e.body[k] = b;
    }
    if (WRITE && lane == 0) {
        envp[C + hc] = 0.0f;
        if (inside) envp[C + nh] = 1.0f;
        if (EAT) envp[nh] = 0.0f;                                                  // :270-272
    }
    e.head = (inside && lane == (nh & 63)) ? (nh < 64 ? 1ull : 2ull) : 0ull;
    if (EAT) {                                                                     // :277-282
        e.food = 0;
        u32 word = 0;
        if (!use_inject) word = rng_words(seed, call, env_id, RNG_FOOD, 0).w[0];
        add_food<2, true, WRITE>(e, g, envp, use_inject, inject_cell, word);
    }
    const bool EDGEC = !(inside && ny >= 1 && ny <= S - 2 && nx >= 1 && nx <= S - 2); // :290-295
    out.action = a;
    out.headcell = nh;
    out.reward = EAT ? 1.0f : 0.0f;
    out.selfc = SELFC;
    out.edgec = EDGEC;
    out.done = SELFC | EDGEC;
    if (EAT) {
        const u64 G0 = ballot((e.food & 1) != 0), G1 = ballot((e.food & 2) != 0);
        out.foodcell = G0 ? first_bit(G0) : (G1 ? 64 + first_bit(G1) : -1);
    } else {
        out.foodcell = fc;
    }
    return true;
}

// One transition of one env held in registers.  WRITE: changed cells are written through to HBM as they are
// produced (per-call kernels); !WRITE: registers only (rollout kernel).
// HEADS (grids of at most 128 cells; rollout_s9_kernel's generic path sets it): a 0 / 1 head plane with SEVERAL heads moves as
// the reference's does, every head of it.
template <int CPL, bool SNAKE, bool WRITE, bool HEADS = false>
__device__ __forceinline__ void step_core(Env<CPL> &e, const Geo &g, float *__restrict__ envp, long long a_in,
                                          StepOut &out, u64 seed, u64 call, u64 env_id, bool use_inject,
                                          int inject_cell, signed char *lds)
{
    out.foodcell = -2;
    if constexpr (SNAKE && CPL == 2 && WRITE) {
        if (small_step<WRITE>(e, g, envp, a_in, out, seed, call, env_id, use_inject, inject_cell)) return;
        out.foodcell = -2;
    }
    const int S = g.S, C = g.C, lane = g.lane;
    long long a = a_in;
    int L = 0;
    if (SNAKE) {
        int lm = 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) lm = max(lm, e.body[k]);
        L = uniform(wave_max_i32(lm)); // single_snake.py:210 snake_sizes

        const int o = orientation_of<CPL>(e, g, L, lds); // utils.py:36-65
        if ((long long)o == a) a += 2; // single_snake.py:221-222 (written back in place by the caller)
        a = a % 4;                     // fmod_: sign follows the dividend
    }
    const int ai = (int)(((a % 4) + 4) % 4);

    // Two spellings of the same transition.  HEADS: EVERY head of the head plane moves, as in the reference (a state edited
    // by hand: the library itself produces at most one head).  Otherwise the one-head form; several heads are outside its
    // domain (deviations).
    if constexpr (HEADS && CPL <= 2) {
        // head shift (single_snake.py:225-233 / simple_gridworld.py:149-157): the whole channel moves by -TAP[a]; what leaves
        // the grid vanishes.  newbits: bit k = cell lane + 64 k holds a head after the move.  The states the library itself
        // produces have at most one head, and that one is moved as a scalar; several heads (a state edited by hand) move
        // through LDS, one byte per cell, each cell looking at the cell its head would come from.
        const bool many = popc64(ballot(e.head != 0)) > 1 || ballot((e.head & (e.head - 1)) != 0) != 0;
        int newhead = -1, ny = -1, nx = -1;
        u64 newbits = 0;
        if (!many) {
            const int headcell = find_head<CPL>(e);
            if (headcell >= 0) {
                int hy = div_size(headcell, g.rcpS), hx = headcell - hy * S;
                ny = hy - tap_y(ai);
                nx = hx - tap_x(ai);
                if (ny >= 0 && ny < S && nx >= 0 && nx < S) newhead = ny * S + nx;
            }
    #pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (lane + 64 * k == newhead) newbits |= 1ull << k;
        } else {
            wave_lds_sync();
    #pragma unroll 1
            for (int k = 0; k < CPL; ++k)
                if ((g.valid >> k) & 1) lds[lane + 64 * k] = (signed char)((e.head >> k) & 1);
            wave_lds_sync();
    #pragma unroll 1
            for (int k = 0; k < CPL; ++k) {
                if (!((g.valid >> k) & 1)) continue;
                const int c = lane + 64 * k, y = div_size(c, g.rcpS), x = c - y * S;
                const int fy = y + tap_y(ai), fx = x + tap_x(ai);
                if (fy >= 0 && fy < S && fx >= 0 && fx < S && lds[fy * S + fx] != 0) newbits |= 1ull << k;
            }
            wave_lds_sync();
            newhead = first_cell(newbits, lane); // the first head in row-major order: what a crop is centred on
        }

        // single_snake.py:242 head_food_overlap: the number of heads that moved onto food
        const int overlap = many ? wave_sum_i32(__popcll(newbits & e.food)) : (int)(ballot((newbits & e.food) != 0) != 0);
        const bool EAT = overlap != 0;

        bool selfc_l = false;
    #pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lane + 64 * k;
            const bool is_new = (newbits >> k) & 1;
            if (SNAKE) {
                const int b0 = e.body[k];
                int b = b0;
                if (!EAT) b = max(b - 1, 0); // :246-249 decay unless food was eaten
                if (is_new) {
                    selfc_l |= b > 0;        // :252 self collision (after the decay)
                    b += L + overlap;        // :258-262 new head segment
                }
                if (WRITE && b != b0) envp[2 * C + c] = (float)b;
                e.body[k] = b;
            }
            if (is_new) {
                if ((e.food >> k) & 1) {     // :270-272 food removal
                    e.food &= ~(1ull << k);
                    if (WRITE) envp[c] = 0.0f;
                }
            }
            if (WRITE && (((e.head >> k) & 1) != (u64)is_new)) envp[C + c] = is_new ? 1.0f : 0.0f;
        }
        e.head = newbits;
        const bool SELFC = SNAKE && (ballot(selfc_l) != 0);

        if (EAT) { // :277-282
            u32 word = 0;
            if (!use_inject) word = rng_words(seed, call, env_id, RNG_FOOD, 0).w[0];
            add_food<CPL, SNAKE, WRITE>(e, g, envp, use_inject, inject_cell, word);
        }

        // :290-295 edge collision: head not in the interior (on the border ring or gone)
        const bool EDGEC = many ? ballot((newbits & g.interior) != 0) == 0
                                : !(newhead >= 0 && ny >= 1 && ny <= S - 2 && nx >= 1 && nx <= S - 2);

        out.action = a;
        out.headcell = newhead;
        out.reward = (float)overlap;
        out.selfc = SELFC;
        out.edgec = EDGEC;
        out.done = SELFC | EDGEC;
    } else {
        // head shift (single_snake.py:225-233 / simple_gridworld.py:149-157): by -TAP[a]; off-grid => vanishes
        const int headcell = find_head<CPL>(e);
        int newhead = -1, ny = -1, nx = -1;
        if (headcell >= 0) {
            int hy = div_size(headcell, g.rcpS), hx = headcell - hy * S;
            ny = hy - tap_y(ai);
            nx = hx - tap_x(ai);
            if (ny >= 0 && ny < S && nx >= 0 && nx < S) newhead = ny * S + nx;
        }

        bool eat_l = false;
    #pragma unroll
        for (int k = 0; k < CPL; ++k) eat_l |= (lane + 64 * k == newhead) && ((e.food >> k) & 1);
        const bool EAT = ballot(eat_l) != 0; // single_snake.py:242 head_food_overlap

        bool selfc_l = false;
        u64 newbits = 0;
    #pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lane + 64 * k;
            const bool is_new = (c == newhead);
            if (SNAKE) {
                const int b0 = e.body[k];
                int b = b0;
                if (!EAT) b = max(b - 1, 0); // :246-249 decay unless food was eaten
                if (is_new) {
                    selfc_l |= b > 0;        // :252 self collision (after the decay)
                    b += L + (EAT ? 1 : 0);  // :258-262 new head segment
                }
                if (WRITE && b != b0) envp[2 * C + c] = (float)b;
                e.body[k] = b;
            }
            if (is_new) {
                newbits |= 1ull << k;
                if ((e.food >> k) & 1) {     // :270-272 food removal
                    e.food &= ~(1ull << k);
                    if (WRITE) envp[c] = 0.0f;
                }
            }
            if (WRITE && (((e.head >> k) & 1) != (u64)is_new)) envp[C + c] = is_new ? 1.0f : 0.0f;
        }
        e.head = newbits;
        const bool SELFC = SNAKE && (ballot(selfc_l) != 0);

        if (EAT) { // :277-282
            u32 word = 0;
            if (!use_inject) word = rng_words(seed, call, env_id, RNG_FOOD, 0).w[0];
            add_food<CPL, SNAKE, WRITE>(e, g, envp, use_inject, inject_cell, word);
        }

        // :290-295 edge collision: head not in the interior (on the border ring or gone)
        const bool EDGEC = !(newhead >= 0 && ny >= 1 && ny <= S - 2 && nx >= 1 && nx <= S - 2);

        out.action = a;
        out.headcell = newhead;
        out.reward = EAT ? 1.0f : 0.0f;
        out.selfc = SELFC;
        out.edgec = EDGEC;
        out.done = SELFC | EDGEC;
    }
}

// ------------------------------------------------------------------------------------------------ reset

// _create_envs for one env (single_snake.py:344-387 / simple_gridworld.py:247-268).  inj: SNAKE {seed_y,
// seed_x, direction, food_cell}; GRID {food_cell}.
template <int CPL, bool SNAKE>
__device__ __forceinline__ void reset_core(Env<CPL> &e, const Geo &g, u64 seed, u64 call, u64 env_id,
                                           const int *__restrict__ inj, int start_y, int start_x)
{
    const int S = g.S, lane = g.lane;
    const bool use_inject = inj != nullptr;
    Words w;
    w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
    if (!use_inject) w = rng_words(seed, call, env_id, RNG_RESET, 0);
    int hc, sc = -1, tc = -1, foodcell = -1;
    if (SNAKE) {
        int sy, sx, d;
        if (use_inject) {
            sy = inj[0]; sx = inj[1]; d = inj[2]; foodcell = inj[3];
        } else { // randint(4, S-4) twice, randint(4) (:358-359,366)
            sy = 4 + (int)mulhi_range(w.w[0], (u32)(S - 8));
            sx = 4 + (int)mulhi_range(w.w[1], (u32)(S - 8));
            d = (int)(w.w[2] >> 30);
        }
        // conv2d(seed, LENGTH_3_SNAKES[d]) (:372-376): 3 at seed + TAP[d], 2 at the seed, 1 at seed - TAP[d]
        hc = (sy + tap_y(d)) * S + sx + tap_x(d);
        sc = sy * S + sx;
        tc = (sy - tap_y(d)) * S + sx - tap_x(d);
    } else {
        hc = start_y * S + start_x; // simple_gridworld.py:262
        if (use_inject) foodcell = inj[0];
    }
    e.food = 0;
    e.head = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = lane + 64 * k;
        e.body[k] = SNAKE ? (c == hc ? 3 : c == sc ? 2 : c == tc ? 1 : 0) : 0;
        if (c == hc) e.head |= 1ull << k;
    }
    add_food<CPL, SNAKE, false>(e, g, nullptr, use_inject, foodcell, w.w[3]); // :384-385
}

// ------------------------------------------------------------------------------------------------ observations

__device__ __forceinline__ float class_rgb(int cls, int ch, bool snake)
{
    // classes: 0 background, 1 body, 2 head, 3 food, 4 border ring.  single_snake.py:99-128 paints body
    // (0,127,0), head (0,255,0), food (255,0,0) on white, ring black; simple_gridworld.py:84-109 on black.
    switch (cls) {
    case 0: return snake ? 1.0f : 0.0f;
    case 1: return ch == 1 ? 127.0f / 255.0f : 0.0f;
    case 2: return ch == 1 ? 1.0f : 0.0f;
    case 3: return ch == 0 ? 1.0f : 0.0f;
    default: return 0.0f;
    }
}

template <int CPL, bool SNAKE>
__device__ __forceinline__ int cell_class(const Env<CPL> &e, const Geo &g, int k)
{
    if (!((g.interior >> k) & 1)) return 4;
    if ((e.food >> k) & 1) return 3;
    if ((e.head >> k) & 1) return 2;
    if (SNAKE && e.body[k] > 0) return 1;
    return 0;
}

// _observe of one env (single_snake.py:130-195, simple_gridworld.py:111-133) from registers.
// headcell: the env's head cell (-1 = none).  lds_copy (partial_n and positions only): a second target for the same
// observation, for a consumer inside the kernel (policy_wide.hpp); off by default.
template <int CPL, bool SNAKE>
__device__ __forceinline__ void write_obs(const Env<CPL> &e, const Geo &g, int headcell, float *__restrict__ o,
                                          int mode, int n, signed char *lds, float *lds_copy = nullptr)
{
    const int S = g.S, C = g.C, lane = g.lane;
    if (mode == WURM_OBS_DEFAULT) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            int c = lane + 64 * k;
            if ((g.valid >> k) & 1) {
                int cls = cell_class<CPL, SNAKE>(e, g, k);
                o[c] = class_rgb(cls, 0, SNAKE);
                o[C + c] = class_rgb(cls, 1, SNAKE);
                o[2 * C + c] = class_rgb(cls, 2, SNAKE);
            }
        }
    } else if (mode == WURM_OBS_PARTIAL) {
        // (2n+1)^2 crop of the zero-padded RGB image around the head, channel-major (single_snake.py:166-193).
        // Each window cell is classified once and written to its three channel planes.
        const int W = 2 * n + 1, W2 = W * W;
        wave_lds_sync();
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if ((g.valid >> k) & 1) lds[lane + 64 * k] = (signed char)cell_class<CPL, SNAKE>(e, g, k);
        wave_lds_sync();
        const int hy = headcell >= 0 ? div_size(headcell, g.rcpS) : 0;
        const int hx = headcell - hy * S;
        const float rcpW = 1.0f / (float)W;
        for (int w = lane; w < W2; w += 64) {
            int wy = div_size(w, rcpW), wx = w - wy * W;
            int y = hy - n + wy, x = hx - n + wx;
            // F.pad zeros (single_snake.py:179); no head: zeros (the reference raises at :191)
            int cls = 4;
            if (headcell >= 0 && y >= 0 && y < S && x >= 0 && x < S) cls = lds[y * S + x];
            o[w] = class_rgb(cls, 0, SNAKE);
            o[W2 + w] = class_rgb(cls, 1, SNAKE);
            o[2 * W2 + w] = class_rgb(cls, 2, SNAKE);
            if (lds_copy) {
                lds_copy[w] = class_rgb(cls, 0, SNAKE);
                lds_copy[W2 + w] = class_rgb(cls, 1, SNAKE);
                lds_copy[2 * W2 + w] = class_rgb(cls, 2, SNAKE);
            }
        }
        wave_lds_sync();
    } else if (mode == WURM_OBS_ONE_CHANNEL) { // single_snake.py:142-151
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            int c = lane + 64 * k;
            if ((g.valid >> k) & 1) {
                float v = (e.body[k] > 0 ? 0.5f : 0.0f) + (((e.head >> k) & 1) ? 0.5f : 0.0f) +
                          (((e.food >> k) & 1) ? 1.5f : 0.0f);
                if (!((g.interior >> k) & 1)) v = -1.0f;
                o[c] = v;
            }
        }
    } else if (mode == WURM_OBS_RAW) { // clone of the state
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            int c = lane + 64 * k;
            if ((g.valid >> k) & 1) {
                o[c] = ((e.food >> k) & 1) ? 1.0f : 0.0f;
                o[C + c] = ((e.head >> k) & 1) ? 1.0f : 0.0f;
                if (SNAKE) o[2 * C + c] = (float)e.body[k];
            }
        }
    } else if (mode == WURM_OBS_POSITIONS) { // argmax of the head and food channels (first maximum; 0 if empty)
        const int fcell = first_cell(e.food, lane);
        int h = headcell < 0 ? 0 : headcell, f = fcell < 0 ? 0 : fcell;
        int hy = div_size(h, g.rcpS), fy = div_size(f, g.rcpS);
        if (lane < 4) o[lane] = (float)(lane == 0 ? hy : lane == 1 ? h - hy * S : lane == 2 ? fy : f - fy * S);
        if (lds_copy && lane < 4) lds_copy[lane] = (float)(lane == 0 ? hy : lane == 1 ? h - hy * S : lane == 2 ? fy : f - fy * S);
    }
}

// per-wave scratch of the kernels built on this header (dynamic LDS, lds_per_wave bytes each unless a kernel says otherwise)
extern __shared__ __attribute__((aligned(16))) signed char wurm_lds[];

// One launch for the caller loop `obs, r, d, info = env.step(a); env.reset(d)` (tests/test_single_snake_env.py:24-31,
// experiments/main.py:212-227), in either of two groupings:
//   * deferred reset: envs flagged in p.done_in (the `done` of the PREVIOUS step, whose reset(done) call the host
//     side postponed) are rebuilt first — exactly reset_kernel with call = p.pre_call — then every env is stepped
//     (call = p.call) and observed;
//   * immediate reset (p.post_reset): after the observation of the post-step state (:304) done envs are rebuilt
//     (call = p.call + 1) and stored, as rollout_kernel does per iteration.
// p.obs_after (nullable): what reset(done) returns — the observation of every env after done envs are rebuilt —
// written whether or not the rebuilt state is stored (the deferred reset of the next launch recreates it from the
// same counters).  p.done_copy (nullable): second copy of `done` in a buffer the caller cannot modify.
template <int CPL, bool SNAKE>
__device__ __forceinline__ void fused_step_env(const StepArgs &p, long long env, signed char *lds)
{
    const int NCH = SNAKE ? 3 : 2;
    const Geo g = make_geo<CPL>(p.S);
    float *envp = p.envs + env * NCH * g.C;
    const u64 env_id = (u64)(p.env_offset + env);
    Env<CPL> e;
    const bool pre = p.done_in != nullptr && uniform((int)p.done_in[env]) != 0;
    if (pre) {
        const int *inj = p.inject_pre_reset ? p.inject_pre_reset + env * (SNAKE ? 4 : 1) : nullptr;
        reset_core<CPL, SNAKE>(e, g, p.seed, p.pre_call, env_id, inj, p.start_y, p.start_x);
        store_state<CPL, SNAKE>(envp, g, e); // step_core then writes the cells it changes on top (same wave: in order)
    } else {
        load_state<CPL, SNAKE>(envp, g, e);
    }
    const long long a_in = uniform64(load_action(p.actions, p.act_dtype, env));
    const bool inj = p.inject_food != nullptr;
    const int inj_cell = inj ? uniform(p.inject_food[env]) : -1;
    StepOut out;
    step_core<CPL, SNAKE, true>(e, g, envp, a_in, out, p.seed, p.call, env_id, inj, inj_cell, lds);
    if (g.lane == 0) {
        if (SNAKE) {
            store_action(p.actions, p.act_dtype, env, out.action);
            p.selfc[env] = (uint8_t)out.selfc;
        }
        p.reward[env] = out.reward;
        p.done[env] = (uint8_t)out.done;
        p.edgec[env] = (uint8_t)out.edgec;
        if (p.done_copy) p.done_copy[env] = (uint8_t)out.done;
    }
    if (p.obs_mode != WURM_OBS_NONE)
        write_obs<CPL, SNAKE>(e, g, out.headcell, p.obs + env * p.obs_elems, p.obs_mode, p.obs_n, lds);
    if (!p.post_reset && p.obs_after == nullptr) return;
    int headcell = out.headcell;
    if (out.done) {
        const int *inj_r = p.inject_reset ? p.inject_reset + env * (SNAKE ? 4 : 1) : nullptr;
        reset_core<CPL, SNAKE>(e, g, p.seed, p.call + 1ull, env_id, inj_r, p.start_y, p.start_x);
        if (p.post_reset) store_state<CPL, SNAKE>(envp, g, e);
        headcell = find_head<CPL>(e);
    }
    if (p.obs_after != nullptr && p.obs_mode != WURM_OBS_NONE)
        write_obs<CPL, SNAKE>(e, g, headcell, p.obs_after + env * p.obs_elems, p.obs_mode, p.obs_n, lds);
}

// ------------------------------------------------------------------------------------------------ rollout fast path
//
// Inside a rollout nothing but this wave touches the env, so the quantities step_core re-derives from the grid on
// every call — head cell, snake length, orientation, food cell — are known wave-uniform scalars that can simply be
// carried from step to step.  Exactness (same results as step_core on the same state) needs the state to be a
// well-formed snake when the carry starts: at most one head cell, at most one food cell, exactly one body cell == L
// (under the head, if there is a head) and exactly one == L-1, L >= 2.  Then, for an env that is not done:
//   * the new head cell holds L + eat and is the unique maximum, the old head cell holds the unique maximum - 1
//     => next length = L + eat, next orientation = (action + 2) % 4 (head = neck + TAP[o] with the move being -TAP[a]);
//   * a done env (self collision / edge) is rebuilt by the reset that follows every step of a rollout.
// Any other start state runs the generic loop (step_core), which makes no assumption.
struct Fast {
    int hc, hy, hx; // head cell (-1: none) and its row / column
    int L;          // snake length = max body value
    int o;          // orientation
    int food;       // food cell (-1: none)
};

template <int CPL>
__device__ __forceinline__ bool fast_init(const Env<CPL> &e, const Geo &g, Fast &f)
{
    int lm = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) lm = max(lm, e.body[k]);
    const int counts = wave_sum_i32(__popcll(e.head) | (__popcll(e.food) << 16));
    const int nhead = counts & 0xffff, nfood = counts >> 16;
    const int hc = first_cell(e.head, g.lane), fc = first_cell(e.food, g.lane);
    const int L = wave_max_i32(lm);
    int cntL, cntN, cellL, cellN;
    top_two<CPL>(e, g, L, cntL, cntN, cellL, cellN);
    if (nhead > 1 || nfood > 1 || cntL != 1 || cntN != 1 || L < 2 || (hc >= 0 && hc != cellL)) return false;
    int yL = div_size(cellL, g.rcpS), xL = cellL - yL * g.S;
    int yN = div_size(cellN, g.rcpS), xN = cellN - yN * g.S;
    int dy = yL - yN, dx = xL - xN;
    f.o = (dy == 0 && dx == 1) ? 1 : (dy == 1 && dx == 0) ? 2 : (dy == 0 && dx == -1) ? 3 : 0; // as orientation_of
    f.hc = hc;
    f.hy = hc >= 0 ? div_size(hc, g.rcpS) : 0;
    f.hx = hc - f.hy * g.S;
    f.L = L;
    f.food = fc;
    return true;
}

// K-th free interior cell (body == 0; the head cell has body > 0 and the only food was just eaten / the grid was
// just rebuilt) in row-major order — the same choice add_food makes.  Returns the cell or -1.
template <int CPL>
__device__ __forceinline__ int fast_food_cell(const Env<CPL> &e, const Geo &g, u32 word)
{
    u64 fr = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
        if (((g.interior >> k) & 1) && e.body[k] == 0) fr |= 1ull << k;
    const int n_free = wave_sum_i32(__popcll(fr));
    if (n_free == 0) return -1;
    const int K = (int)mulhi_range(word, (u32)n_free);
    int base = 0;
#pragma unroll 1
    for (int k = 0; k < CPL; ++k) {
        const u64 m = ballot((fr >> k) & 1);
        const int cnt = popc64(m);
        if (K < base + cnt) { // the (K - base)-th set bit of m
            const u64 hit = ballot(((m >> g.lane) & 1) && rank_below(m) == K - base);
            return 64 * k + first_bit(hit);
        }
        base += cnt;
    }
    return -1;
}

// step_core with carried scalars (single_snake.py:197-304; same line references as step_core)
// a_small = the action if it is one of 0..3, else -1;  a_mod = action % 4 (C semantics: -3..3).  Both are computed
// once per 64-step tape chunk so that the per-step sanitisation is 32-bit scalar work.
template <int CPL>
__device__ __forceinline__ void fast_step(Env<CPL> &e, const Geo &g, Fast &f, int a_small, int a_mod, StepOut &out,
                                          u64 seed, u64 call, u64 env_id, bool use_inject, int inject_cell)
{
    const int S = g.S;
    const bool rev = f.o == a_small;                                      // :221-222
    const int a_out = rev ? ((f.o + 2) & 3) : a_mod;
    const int ai = a_out & 3;                                             // == ((a_out % 4) + 4) % 4 for -3..3
    int newhead = -1, ny = -1, nx = -1;
    if (f.hc >= 0) {                                                      // :225-233
        ny = f.hy - tap_y(ai);
        nx = f.hx - tap_x(ai);
        if (ny >= 0 && ny < S && nx >= 0 && nx < S) newhead = ny * S + nx;
    }
    const bool inside = newhead >= 0;
    const bool EAT = inside && newhead == f.food;                         // :242
    int sel = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) sel = (newhead >> 6) == k ? e.body[k] : sel;
    const int bnew = inside ? lane_value(sel, newhead & 63) : 0;
    const int bdec = EAT ? bnew : max(bnew - 1, 0);
    const bool SELFC = inside && bdec > 0;                                // :252
    const int grow = f.L + (EAT ? 1 : 0);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int b = e.body[k];
        if (!EAT) b = max(b - 1, 0);                                      // :246-249
        if (g.lane + 64 * k == newhead) b += grow;                        // :258-262
        e.body[k] = b;
    }
    const bool EDGEC = !(inside && ny >= 1 && ny <= S - 2 && nx >= 1 && nx <= S - 2); // :290-295
    f.hc = newhead; f.hy = ny; f.hx = nx;
    f.L = grow;
    f.o = (ai + 2) & 3;
    if (EAT) {                                                            // :270-282
        if (use_inject) f.food = (inject_cell >= 0 && inject_cell < g.C) ? inject_cell : -1;
        else f.food = fast_food_cell<CPL>(e, g, rng_words(seed, call, env_id, RNG_FOOD, 0).w[0]);
    }
    out.action = a_out;
    out.headcell = newhead;
    out.reward = EAT ? 1.0f : 0.0f;
    out.selfc = SELFC;
    out.edgec = EDGEC;
    out.done = SELFC | EDGEC;
}

// reset_core with carried scalars (single_snake.py:344-387)
template <int CPL>
__device__ __forceinline__ void fast_reset(Env<CPL> &e, const Geo &g, Fast &f, u64 seed, u64 call, u64 env_id,
                                           const int *__restrict__ inj)
{
    const int S = g.S;
    Words w;
    w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0;
    int sy, sx, d, fc = -1;
    if (inj) {
        sy = inj[0]; sx = inj[1]; d = inj[2]; fc = inj[3];
        if (fc >= g.C) fc = -1;
    } else {
        w = rng_words(seed, call, env_id, RNG_RESET, 0);
        sy = 4 + (int)mulhi_range(w.w[0], (u32)(S - 8));
        sx = 4 + (int)mulhi_range(w.w[1], (u32)(S - 8));
        d = (int)(w.w[2] >> 30);
    }
    const int hy = sy + tap_y(d), hx = sx + tap_x(d);
    const int hc = hy * S + hx, sc = sy * S + sx, tc = (sy - tap_y(d)) * S + sx - tap_x(d);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        e.body[k] = c == hc ? 3 : c == sc ? 2 : c == tc ? 1 : 0;
    }
    f.hc = hc; f.hy = hy; f.hx = hx;
    f.L = 3;
    f.o = d;
    f.food = inj ? fc : fast_food_cell<CPL>(e, g, w.w[3]);
}

// food / head bit sets of the Env from the carried scalars (for the generic observation writer and store_state)
template <int CPL>
__device__ __forceinline__ void fast_sync_bits(Env<CPL> &e, const Geo &g, const Fast &f)
{
    e.food = 0;
    e.head = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if (c == f.food) e.food |= 1ull << k;
        if (c == f.hc) e.head |= 1ull << k;
    }
}

// Per-lane geometry of the partial_n crop, computed once per kernel: lane owns window cells w = lane + 64*i.
constexpr int CROP_NI = 3; // (2n+1)^2 <= 192, i.e. n <= 6
struct Crop {
    int W2;
    int dy[CROP_NI], dx[CROP_NI]; // window cell offset from the head; dy = INT_MIN/2 marks "no such cell"
};

__device__ __forceinline__ Crop make_crop(int lane, int n)
{
    Crop c;
    const int W = 2 * n + 1;
    c.W2 = W * W;
    const float rcpW = 1.0f / (float)W;
#pragma unroll
    for (int i = 0; i < CROP_NI; ++i) {
        int w = lane + 64 * i;
        int wy = div_size(w, rcpW), wx = w - wy * W;
        c.dy[i] = w < c.W2 ? wy - n : -(1 << 20);
        c.dx[i] = wx - n;
    }
    return c;
}

// partial_n crop for grids of at most 128 cells (single_snake.py:166-193): body occupancy as two ballot masks, the
// head and food cells as scalars — no LDS.  A window cell that is off the grid, on the border ring, or seen from
// an env without a head is (0,0,0); otherwise food (1,0,0), head (0,1,0), body (0,127/255,0), background (1,1,1).
template <int CPL>
__device__ __forceinline__ void fast_partial_small(const Env<CPL> &e, const Geo &g, const Fast &f,
                                                   float *__restrict__ o, const Crop &cg, float *lds_copy = nullptr)
{
    static_assert(CPL <= 2, "ballot-mask crop needs <= 128 cells");
    const int S = g.S, W2 = cg.W2;
    const u64 m0 = ballot(e.body[0] > 0), m1 = CPL > 1 ? ballot(e.body[CPL - 1] > 0) : 0;
    const bool has_head = f.hc >= 0;
#pragma unroll
    for (int i = 0; i < CROP_NI; ++i) {
        if (64 * i >= W2) break;
        const int y = f.hy + cg.dy[i], x = f.hx + cg.dx[i];
        if (cg.dy[i] <= -(1 << 19)) continue;
        const bool live = has_head && (unsigned)(y - 1) < (unsigned)(S - 2) && (unsigned)(x - 1) < (unsigned)(S - 2);
        const int cell = y * S + x;
        const bool fd = cell == f.food, hd = cell == f.hc;
        const bool bd = (((cell < 64 ? m0 : m1) >> (cell & 63)) & 1) != 0;
        const float bg = (live && !fd && !hd && !bd) ? 1.0f : 0.0f;
        const float r = (live && fd) ? 1.0f : bg;
        const float gr = (live && !fd) ? (hd ? 1.0f : (bd ? 127.0f / 255.0f : bg)) : 0.0f;
        const int w = g.lane + 64 * i;
        o[w] = r;
        o[W2 + w] = gr;
        o[2 * W2 + w] = bg;
        if (lds_copy) { // the same observation for a consumer inside the kernel (policy_rollout.hpp)
            lds_copy[w] = r;
            lds_copy[W2 + w] = gr;
            lds_copy[2 * W2 + w] = bg;
        }
    }
}

// T fused step+reset iterations with the env resident in registers.  Lane j of the wave buffers the
// per-step scalars of step t0+j; they are flushed every 64 steps.
// OBSK >= 0 fixes the observation mode at compile time and INJ = false compiles the injection plumbing out: the
// flagship configuration (9x9, partial_n / no observation, RNG mode) gets a lean instantiation, everything else the
// fully general one (OBSK = -1, INJ = true).
template <int CPL, bool SNAKE, int OBSK, bool INJ, bool HEADS = false>
__device__ __forceinline__ void rollout_generic(const StepArgs &p, long long env, float *__restrict__ envp, const Geo &g,
                                                Env<CPL> &e, signed char *lds)
{
    const u64 env_id = (u64)(p.env_offset + env);
    const bool inj_f = INJ && p.inject_food != nullptr, inj_r = INJ && p.inject_reset != nullptr;
    const int obs_mode = OBSK >= 0 ? OBSK : p.obs_mode;
    Fast f = {-1, 0, 0, 0, 0, -1};
    bool fast = false;
    if (SNAKE) fast = fast_init<CPL>(e, g, f);
    const bool small_crop = SNAKE && CPL <= 2 && obs_mode == WURM_OBS_PARTIAL && p.obs_n <= 6;
    const Crop cg = make_crop(g.lane, small_crop ? p.obs_n : 0);
    const long long obs_stride = p.N * p.obs_elems;
    float *obs_t = p.obs + env * p.obs_elems; // observation of step t; advanced by obs_stride per step
    u64 call = p.call;                        // step t uses call0 + 2t, its reset call0 + 2t + 1

    for (long long t0 = 0; t0 < p.T; t0 += 64) {
        const int nt = (int)min((long long)64, p.T - t0);
        const long long my_t = t0 + g.lane;
        long long my_a = g.lane < nt ? load_action(p.actions, p.act_dtype, my_t * p.N + env) : 0;
        int my_inj = (inj_f && g.lane < nt) ? p.inject_food[my_t * p.N + env] : -1;
        int my_flags = 0; // bit 0 done, 1 self collision, 2 edge collision, 3 reward
        // Retire the two prefetch loads HERE.  Otherwise the compiler, seeing a register that may still be in flight
        // on loop entry, puts `s_waitcnt vmcnt(0)` in front of the per-step readlane, and every step then also waits
        // for the previous step's observation stores to be acknowledged by HBM (vmcnt counts loads and stores).
        asm volatile("" : "+v"(my_a), "+v"(my_inj));
        const int my_small = (my_a >= 0 && my_a < 4) ? (int)my_a : -1, my_mod = (int)(my_a % 4);
        int my_out = 0; // sanitised action of step t0 + lane (always in -3..3)
        for (int j = 0; j < nt; ++j, obs_t += obs_stride, call += 2) {
            const int inj_cell = INJ ? lane_value(my_inj, j) : -1;
            StepOut out;
            if (SNAKE && fast) {
                fast_step<CPL>(e, g, f, lane_value(my_small, j), lane_value(my_mod, j), out, p.seed, call, env_id, inj_f,
                               inj_cell);
                if (small_crop) {
                    if constexpr (CPL <= 2) fast_partial_small<CPL>(e, g, f, obs_t, cg);
                } else if (obs_mode != WURM_OBS_NONE) {
                    fast_sync_bits<CPL>(e, g, f);
                    write_obs<CPL, SNAKE>(e, g, f.hc, obs_t, obs_mode, p.obs_n, lds);
                }
                if (out.done)
                    fast_reset<CPL>(e, g, f, p.seed, call + 1ull, env_id,
                                    inj_r ? p.inject_reset + ((t0 + j) * p.N + env) * 4 : nullptr);
            } else {
                const long long a_in = lane_value64(my_a, j);
                step_core<CPL, SNAKE, false, HEADS>(e, g, nullptr, a_in, out, p.seed, call, env_id, inj_f, inj_cell, lds);
                if (obs_mode != WURM_OBS_NONE)
                    write_obs<CPL, SNAKE>(e, g, out.headcell, obs_t, obs_mode, p.obs_n, lds);
                if (out.done) {
                    const int *inj = inj_r ? p.inject_reset + ((t0 + j) * p.N + env) * (SNAKE ? 4 : 1) : nullptr;
                    reset_core<CPL, SNAKE>(e, g, p.seed, call + 1ull, env_id, inj, p.start_y, p.start_x);
                }
            }
            if (g.lane == j) {
                my_out = (int)out.action;
                my_flags = out.done | (out.selfc << 1) | (out.edgec << 2) | (out.reward != 0.0f ? 8 : 0);
            }
        }
        if (g.lane < nt) {
            const long long i = my_t * p.N + env;
            if (SNAKE) {
                store_action(p.actions, p.act_dtype, i, (long long)my_out);
                p.selfc[i] = (uint8_t)((my_flags >> 1) & 1);
            }
            p.reward[i] = (my_flags & 8) ? 1.0f : 0.0f;
            p.done[i] = (uint8_t)(my_flags & 1);
            p.edgec[i] = (uint8_t)((my_flags >> 2) & 1);
        }
    }
    if (SNAKE && fast) fast_sync_bits<CPL>(e, g, f);
    store_state<CPL, SNAKE>(envp, g, e);
}

// ------------------------------------------------------------------------------- lean rollout helpers
// (rollout_lean_kernel, single_kernels.hpp)

struct LeanReset {
    int a; // hy | hx << 4 | d << 8 | food cell << 10
    int b; // head cell | seed cell << 7 | tail cell << 14
};

// would-be reset of (env, call): reset_core / fast_reset in closed form.  After a rebuild the free interior cells
// are the (S-2)^2 interior cells minus the three collinear snake cells, so the K-th free cell in row-major order is
// the K-th interior cell pushed past the snake cells' interior ranks in ascending order.
__device__ __forceinline__ LeanReset lean_reset_draw(u64 seed, u64 call, u64 env_id, int S, float rcpSm2)
{
    const Words w = rng_words(seed, call, env_id, RNG_RESET, 0);
    const int Sm2 = S - 2;
    const int sy = 4 + (int)mulhi_range(w.w[0], (u32)(S - 8));
    const int sx = 4 + (int)mulhi_range(w.w[1], (u32)(S - 8));
    const int d = (int)(w.w[2] >> 30);
    const int ty = tap_y(d), tx = tap_x(d);
    const int hy = sy + ty, hx = sx + tx;
    const int rs = (sy - 1) * Sm2 + sx - 1, dr = ty * Sm2 + tx; // interior rank of the seed cell; head = rs + dr
    const int lo = rs - abs(dr), hi = rs + abs(dr);
    int K = (int)mulhi_range(w.w[3], (u32)(Sm2 * Sm2 - 3));
    K += K >= lo;
    K += K >= rs;
    K += K >= hi;
    const int qy = div_size(K, rcpSm2), qx = K - qy * Sm2;
    const int food = (qy + 1) * S + qx + 1;
    const int sc = sy * S + sx, dc = ty * S + tx;
    LeanReset r;
    r.a = hy | (hx << 4) | (d << 8) | (food << 10);
    r.b = (sc + dc) | (sc << 7) | ((sc - dc) << 14);
    return r;
}

// K-th free interior cell (K = mulhi(word, n_free)) given the occupancy masks of cells 0..63 / 64..127; -1 if none
__device__ __forceinline__ int lean_food_cell(u64 m0, u64 m1, u64 int0, u64 int1, u32 word, int lane)
{
    const u64 F0 = int0 & ~m0, F1 = int1 & ~m1;
    const int n0 = popc64(F0), n_free = n0 + popc64(F1);
    if (n_free == 0) return -1;
    const int K = (int)mulhi_range(word, (u32)n_free);
    const bool second = K >= n0;
    const u64 F = second ? F1 : F0;
    const int K2 = second ? K - n0 : K;
    const u64 hit = ballot((int)((F >> lane) & 1) & (int)(rank_below(F) == K2));
    return (second ? 64 : 0) + first_bit(hit);
}

// lane mask of a per-lane predicate (folds with the compares / logic that produce it; __ballot goes through an int)
__device__ __forceinline__ u64 lane_mask(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// ----------------------------------------------------------------------------- 9 x 9 rollout helpers
// (rollout_s9_kernel, single_kernels.hpp; policy_rollout_s9_kernel, policy_rollout.hpp)

struct S9Reset {
    int a; // orientation | food code << 2
    int b; // head code | seed code << 7 | tail code << 14
};

// lean_reset_draw in code numbering (single_snake.py:344-387)
__device__ __forceinline__ S9Reset s9_reset_draw(u64 seed, u64 call, u64 env_id)
{
    const Words w = rng_words(seed, call, env_id, RNG_RESET, 0);
    const int sy = 4 + (int)mulhi_range(w.w[0], 1u), sx = 4 + (int)mulhi_range(w.w[1], 1u); // S - 8 = 1
    const int d = (int)(w.w[2] >> 30);
    const int ty = tap_y(d), tx = tap_x(d);
    const int rs = (sy - 1) * 7 + sx - 1, dr = ty * 7 + tx; // interior rank of the seed cell; head = rs + dr
    const int lo = rs - abs(dr), hi = rs + abs(dr);
    int K = (int)mulhi_range(w.w[3], 46u); // 49 interior cells - 3 snake cells
    K += K >= lo;
    K += K >= rs;
    K += K >= hi;
    const int qy = div_size(K, 1.0f / 7.0f), qx = K - qy * 7;
    const int sc = sy * 8 + sx, dc = ty * 8 + tx;
    S9Reset r;
    r.a = d | (((qy + 1) * 8 + qx + 1) << 2);
    r.b = (sc + dc) | (sc << 7) | ((sc - dc) << 14);
    return r;
}

// what the 64 steps of a chunk need that does not depend on the state, lane j holding step t0 + j's (rollout_s9_kernel)
struct S9Chunk {
    int mov01, mov23; // the move entries for the orientations 0, 1 and 2, 3
    S9Reset reset;    // the would-be reset
    int food;         // RNG: the word the food cell of an eating step is drawn with; injected: its code (-1: none)
};

// Barrier between the two waves of rollout_s9_kernel's pair form.  It orders LDS only: the waves' global stores stay in
// flight across it (__syncthreads() would wait for vmcnt(0), that is for every observation store of the chunk).
__device__ __forceinline__ void pair_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// v = value in the lanes of `lanes`, unchanged elsewhere — with the lane mask taken from an SGPR pair as it is (the
// compiler has no way to say that; `lane == j` costs a VALU compare and drags the scalar j into a VGPR)
__device__ __forceinline__ int keep_in_lane(int v, int value, u64 lanes)
{
    asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(v) : "v"(value), "s"(lanes));
    return v;
}

// v = value in lane `dst`, unchanged elsewhere; value and dst wave-uniform.  v_writelane_b32 with the lane select in m0:
// two ordinary SGPR operands break the constant-bus limit.  (m0 written by the SALU needs no wait state before a lane
// select; only an SGPR written by the VALU does.)
__device__ __forceinline__ int set_lane(int v, int value, int dst)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm" // m0 is reserved, and is named as clobbered on purpose
    asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(value), "s"(dst) : "m0");
#pragma clang diagnostic pop
    return v;
}

// What the helper wave needs of step t0 + j to render its crop (rollout_s9_kernel, CROPH), each in lane j of its register: the
// move entry, the head code, the food code the crop shows and the body mask without the head.  set_lane five times over
// with ONE lane select in m0.
struct S9CropRec {
    int ent, c, food, body_lo, body_hi;
};
__device__ __forceinline__ void set_lane(S9CropRec &r, int ent, int c, int food, u64 body, int dst)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm" // (m0: as above)
    asm("s_mov_b32 m0, %10\n\t"
        "v_writelane_b32 %0, %5, m0\n\t"
        "v_writelane_b32 %1, %6, m0\n\t"
        "v_writelane_b32 %2, %7, m0\n\t"
        "v_writelane_b32 %3, %8, m0\n\t"
        "v_writelane_b32 %4, %9, m0"
        : "+v"(r.ent), "+v"(r.c), "+v"(r.food), "+v"(r.body_lo), "+v"(r.body_hi)
        : "s"(ent), "s"(c), "s"(food), "s"((int)(u32)body), "s"((int)(u32)(body >> 32)), "s"(dst)
        : "m0");
#pragma clang diagnostic pop
}
// (The trio form's record of a plain move is the move entry alone, one set_lane into r.ent: r.c and the body halves stay unused,
// r.food is written by eating steps alone; the render waves rebuild the head codes, the food codes and the body masks of a whole
// chunk from that: s9_rebuild_crop_words, s9_rebuild_body.)

// The crop words of a chunk's 64 steps, step j in lane j, from what the stepper of the trio form hands over (rollout_s9_kernel):
//   rec   action & 7 | ate << 3 | collisions << 4 of step j
//   pw    the crop word of step j without its head code, and with a food field (bits 7-13: food code + 1) that only an eating
//         step defines: the cell drawn on that step
//   ra/rb the would-be reset of step j (S9Reset)
//   c0/f0 head code and food code the stepper entered the chunk with
// Head code of step j: c0, or the head code of the last reset before j, plus the code steps since — integer sums, so the same
// integer as the stepper's chain of s_add_i32 whatever the order (the caller masks it like the stepper did).  Shown food of
// step j: what the last of these left: an eating step at or before j, a reset before j, the chunk start.  An eating step does
// not collide (no food on the ring or under the body), so "the last" is decided by the step indices alone.
__device__ __forceinline__ int s9_rebuild_crop_words(int rec, int pw, int ra, int rb, int c0, int f0, int lane)
{
    int P = (pw << 10) >> 26; // the code step of the move entry, then its inclusive prefix sum over the lanes
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int below = __shfl_up(P, s, 64);
        P += lane >= s ? below : 0;
    }
    const u64 resets = lane_mask((rec >> 4) != 0), eats = lane_mask(((rec >> 3) & 1) != 0);
    const u64 before = (1ull << lane) - 1ull, upto = before | (1ull << lane);
    const u64 rbef = resets & before, eupto = eats & upto;
    const int r = rbef ? 63 - __clzll((long long)rbef) : -1;   // the last reset before this step
    const int e = eupto ? 63 - __clzll((long long)eupto) : -1; // the last eating step up to this one
    // from lane r: head code of the new snake less the steps up to there, and its food; from lane e: the food drawn there
    const int base_r = __shfl((rb & 127) - P, r & 63, 64);
    const int food_r = __shfl(((ra >> 2) + 1) & 127, r & 63, 64);
    const int food_e = __shfl((pw >> 7) & 127, e & 63, 64);
    const int c = (r >= 0 ? base_r : c0) + P;
    const int food1 = e > r ? food_e : r >= 0 ? food_r : (f0 + 1) & 127;
    return (c & 127) | (food1 << 7) | (pw & ~0x3FFF);
}

// The body mask without the head of a chunk's 64 steps, step j in lane j (bit x: the cell of code x), from what the stepper of
// the trio form hands over (rollout_s9_kernel) — the integer its compare `ex > T` gave on step j:
//   rec    action & 7 | ate << 3 | collisions << 4 of step j
//   word   the rebuilt crop word of step j (s9_rebuild_crop_words): bits 0-6 the head code after the move
//   rb     the would-be reset of step j (S9Reset::b: head | seed << 7 | tail << 14 of the new snake)
//   ex0    the clock of the cell whose code is `lane`, on entering the chunk, re-based to the clock 0 (0: free)
//   len0   the length on entering the chunk
// With r the last reset before step j (none: the chunk start) and len_j the length after step j's move — 3, or len0 in the
// chunk's first segment, plus the eating steps behind r up to j, for the clock stands still on a step that eats —, a cell is
// body on step j if the head stood there on a step i with 0 < j - i < len_j: the head wrote the clock G_i there, G_j - G_i =
// j - i and len_j = G_j - T_j, so that is G_i > T_j.  The head of step i is
//   * the head code of step i's crop word for r < i (no reset in between: the head is inside the ring, one lane, one bit);
//   * the head, seed and tail cell of reset r's new snake for i = r, r - 1, r - 2: the reset gave them the clocks the head
//     would have written there (T + 3, T + 2, T + 1), and nothing else survived it.  The window never reaches behind r - 2:
//     len_j - 3 eating steps lie between r and j;
//   * before the chunk's first reset, for i < 0, whatever the chunk-start clocks say: the cell of code x is body while
//     ex0[x] > T_j, and T_j is the number of steps up to j that did not eat.  No assumption on the clocks being consecutive.
// A cell the head visited twice is body if either visit says so (the later clock is the larger one).  A code that is no
// lane's (a hand-made reset word) sets no bit, as in the stepper, which compares lanes with codes.
__device__ __forceinline__ u64 s9_rebuild_body(int rec, int word, int rb, int ex0, int len0, int lane)
{
    const u64 resets = lane_mask((rec >> 4) != 0), eats = lane_mask(((rec >> 3) & 1) != 0);
    const u64 before = (1ull << lane) - 1ull, upto = before | (1ull << lane);
    const u64 rbef = resets & before;
    const int r = rbef ? 63 - __clzll((long long)rbef) : -1;             // the last reset before this step (r <= 62)
    const u64 behind_r = r >= 0 ? ~((2ull << r) - 1ull) : ~0ull;
    const int grown = popc64(eats & upto & behind_r);                    // eating steps behind r up to this step
    const int len = (r >= 0 ? 3 : len0) + grown;
    const int nb = __shfl(rb, r & 63, 64);
    const int new_head = nb & 127, new_seed = (nb >> 7) & 127, new_tail = nb >> 14;
    u64 body = 0;
    // the chunk-start clocks: one ballot over the cells per clock value, taken by the steps at which the clock has that value
    const int clock = r >= 0 ? -1 : lane + 1 - grown;
    for (int t = 0; t <= 64; ++t) {
        const u64 later = lane_mask(ex0 > t);
        if (later == 0) break;
        body = clock == t ? later : body;
    }
    // the trail: the head of d steps ago, for every d below the longest length among the 64 steps
    const int hc = word & 63;
    const int longest = min(wave_max_i32(len), 64);
    for (int d = 1; d < longest; ++d) {
        const int i = lane - d;
        const int moved = __shfl_up(hc, (unsigned)d, 64);                // (lanes below d get their own: i < 0, not used)
        const int code = i > r ? moved : i == r ? new_head : i == r - 1 ? new_seed : new_tail;
        const bool in_window = d < len && (i > r || r >= 0) && (unsigned)code < 64u;
        body |= in_window ? 1ull << (code & 63) : 0ull;
    }
    return body;
}

// The partial_n window cell a lane of the 9 x 9 rollout renders, for window-cell index wl (lanes past the window repeat
// its last cell: same address, same value): its offset from the head in rows, columns and codes, what an occupied cell
// shows in channel 1 there, and which head codes put it inside the ring.
struct S9Window {
    int w, dy0, dx0, code_d;
    float green;
    u64 live_tab; // bit (8 * row + column): with the head there, this window cell is inside the ring
};
__device__ __forceinline__ S9Window s9_window(int wl, int n)
{
    S9Window r;
    const int W = 2 * n + 1, W2 = W * W;
    r.w = min(wl, W2 - 1);
    const int wy = div_size(r.w, 1.0f / (float)W), wx = r.w - wy * W;
    r.dy0 = wy - n; r.dx0 = wx - n;            // window row / column offset from the head
    r.code_d = r.dy0 * 8 + r.dx0;              // code of the window cell = head code + code_d
    r.green = (r.w == n * W + n) ? 1.0f : 127.0f / 255.0f;
    r.live_tab = 0;
#pragma unroll
    for (int y = 1; y <= 7; ++y) {
        u32 cols = 0;
#pragma unroll
        for (int x = 1; x <= 7; ++x)
            if ((unsigned)(x + r.dx0 - 1) < 7u) cols |= 1u << x;
        if ((unsigned)(y + r.dy0 - 1) < 7u) r.live_tab |= (u64)cols << (8 * y);
    }
    return r;
}

// bit (i & 63) of m, for a branch: s_bitcmp1_b64 reads bits [5:0] of its index operand
__device__ __forceinline__ bool bit_set(u64 m, int i) { return ((m >> (i & 63)) & 1) != 0; }

} // namespace wurm
