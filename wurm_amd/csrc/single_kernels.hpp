// single_kernels.hpp — the __global__ kernels of SingleSnake and SimpleGridworld on the one-env-per-wavefront device code
// of single_device.hpp: ONE fused launch per call (step, reset, observe, step + reset, T-step rollout), the rollout
// specialisations for the small grids (lean, 9 x 9), and the consistency / orientation queries.
// rollout_kernel fuses T step+reset iterations with the env resident in registers; for well-formed start states it
// carries head cell / length / orientation / food cell as scalars (fast_step) instead of re-deriving them.
#pragma once

#include "single_device.hpp"

namespace wurm {

template <int CPL, bool SNAKE>
__global__ __launch_bounds__(256) void step_kernel(StepArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    if (p.only_flagged && uniform((int)p.done[env]) != (int)GRID_SKIPPED) return; // grid_step_kernel stepped this env
    signed char *lds = wurm_lds + wave * p.lds_per_wave;
    const int NCH = SNAKE ? 3 : 2;
    const Geo g = make_geo<CPL>(p.S);
    float *envp = p.envs + env * NCH * g.C;
    Env<CPL> e;
    load_state<CPL, SNAKE>(envp, g, e);
    const long long a_in = uniform64(load_action(p.actions, p.act_dtype, env));
    const bool inj = p.inject_food != nullptr;
    const int inj_cell = inj ? uniform(p.inject_food[env]) : -1;
    StepOut out;
    step_core<CPL, SNAKE, true>(e, g, envp, a_in, out, p.seed, p.call, (u64)(p.env_offset + env), inj, inj_cell, lds);
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
}

template <int CPL, bool SNAKE>
__global__ __launch_bounds__(256) void fused_step_kernel(StepArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    if (p.only_flagged && uniform((int)p.done[env]) != (int)GRID_SKIPPED) return; // grid_step_kernel stepped this env
    fused_step_env<CPL, SNAKE>(p, env, wurm_lds + wave * p.lds_per_wave);
}

template <int CPL, bool SNAKE>
__global__ __launch_bounds__(256) void reset_kernel(StepArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    signed char *lds = wurm_lds + wave * p.lds_per_wave;
    const int NCH = SNAKE ? 3 : 2;
    const Geo g = make_geo<CPL>(p.S);
    float *envp = p.envs + env * NCH * g.C;
    Env<CPL> e;
    const bool d = uniform((int)p.done_in[env]) != 0;
    if (d) {
        const int *inj = p.inject_reset ? p.inject_reset + env * (SNAKE ? 4 : 1) : nullptr;
        reset_core<CPL, SNAKE>(e, g, p.seed, p.call, (u64)(p.env_offset + env), inj, p.start_y, p.start_x);
        store_state<CPL, SNAKE>(envp, g, e);
    } else {
        if (p.obs_mode == WURM_OBS_NONE) return;
        load_state<CPL, SNAKE>(envp, g, e);
    }
    if (p.obs_mode != WURM_OBS_NONE)
        write_obs<CPL, SNAKE>(e, g, find_head<CPL>(e), p.obs + env * p.obs_elems, p.obs_mode, p.obs_n, lds);
}

template <int CPL, bool SNAKE>
__global__ __launch_bounds__(256) void observe_kernel(StepArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    signed char *lds = wurm_lds + wave * p.lds_per_wave;
    const int NCH = SNAKE ? 3 : 2;
    const Geo g = make_geo<CPL>(p.S);
    Env<CPL> e;
    load_state<CPL, SNAKE>(p.envs + env * NCH * g.C, g, e);
    write_obs<CPL, SNAKE>(e, g, find_head<CPL>(e), p.obs + env * p.obs_elems, p.obs_mode, p.obs_n, lds);
}

template <int CPL, bool SNAKE, int OBSK = -1, bool INJ = true>
__global__ __launch_bounds__(256) void rollout_kernel(StepArgs p)
{
    const int wave = uniform((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    if (p.only_flagged && uniform((int)p.done[env]) != (int)GRID_SKIPPED) return; // the grid kernel rolled this env out
    signed char *lds = wurm_lds + wave * p.lds_per_wave;
    const Geo g = make_geo<CPL>(p.S);
    float *envp = p.envs + env * (SNAKE ? 3 : 2) * g.C;
    Env<CPL> e;
    load_state<CPL, SNAKE>(envp, g, e);
    rollout_generic<CPL, SNAKE, OBSK, INJ>(p, env, envp, g, e, lds);
}

// ---- the envs a grid / lane kernel left to the one-env-per-wave code (done[env] == GRID_SKIPPED; for a rollout the flag is in
// done[0][env]): ONE WAVE PER 64 ENVS reads their flags — one coalesced load, one ballot — and serves the flagged ones in
// turn.  Launching the one-env-per-wave kernels for EVERY env just to read its flag (only_flagged, rounds 3-5) cost 3.9 us at
// 8 192 envs and 6.8-9 us at 65 536: a fifth of the per-call step of 8 192 x 36 x 36 that it stood behind.
// ROLL: rollout_kernel's body; else fused_step_env (which is step_kernel's body when the call carries no reset).
template <int CPL, bool SNAKE, bool ROLL>
__global__ __launch_bounds__(256) void flagged_kernel(StepArgs p)
{
    const int wave = uniform((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6), lane = (int)(threadIdx.x & 63u);
    const long long base = ((long long)blockIdx.x * wpb + wave) * 64;
    if (base >= p.N) return;
    const bool flag = base + lane < p.N && p.done[base + lane] == GRID_SKIPPED;
    signed char *lds = wurm_lds + wave * p.lds_per_wave;
    for (u64 m = ballot(flag); m != 0; m &= m - 1) {
        const long long env = base + first_bit(m);
        if constexpr (ROLL) {
            const Geo g = make_geo<CPL>(p.S);
            float *envp = p.envs + env * (SNAKE ? 3 : 2) * g.C;
            Env<CPL> e;
            load_state<CPL, SNAKE>(envp, g, e);
            rollout_generic<CPL, SNAKE, -1, true>(p, env, envp, g, e, lds);
        } else {
            fused_step_env<CPL, SNAKE>(p, env, lds);
        }
        wave_lds_sync(); // (the next env reuses the wave's LDS)
    }
}

// ---------------------------------------------------------------------------------------------- lean rollout
// The headline shape — SingleSnake on a grid of at most 128 cells (S <= 11), partial_n crop of at most 64 window
// cells (n <= 3) or no observation, RNG mode — runs 512 envs as 512 lone waves on 1024 SIMDs: nothing hides
// latency, every instruction costs its full issue slot and every taken branch an instruction-fetch bubble, so the
// loop below is written for instruction count (PMC: 205 -> ~95 instructions per env-step).  On top of the scalar
// carry of `Fast` it uses
//   * a virtual clock for the body channel: cell value = max(expire - T, 0).  A step that does not eat advances T
//     (= "every body cell decays by one", single_snake.py:246-249) and a step that eats leaves it alone; only the new
//     head cell is written (expire = T + L), so the decay costs no per-cell work;
//   * everything a reset needs (single_snake.py:344-387: seed cell, direction, the three body cells, the food cell)
//     depends only on (seed, env, call), never on the state: lane j of the wave computes the would-be reset of step
//     t0+j — both Philox blocks included — once per 64-step chunk, in parallel, and a reset is two readlanes;
//   * the food draw of an eating step (purpose RNG_FOOD) is precomputed the same way; only the rank select over the
//     free cells, which does depend on the state, runs when food is eaten;
//   * observation masks combined as 64-bit scalar lane masks; lanes past the window duplicate its last cell
//     instead of being masked off.
// Preconditions (else the kernel runs rollout_generic): fast_init's well-formed snake, a head strictly inside the
// border ring, and no food on a body cell.  They are preserved by step + reset, so they are checked once.
// A state that self-collided is rebuilt by the reset of the same iteration, so the value under the new head is not
// accumulated (only its occupancy is observable, through the crop).

template <int OBSK, bool COMPACT>
__global__ __launch_bounds__(256) void rollout_lean_kernel(StepArgs p)
{
    constexpr int CPL = 2;
    static_assert(OBSK == WURM_OBS_PARTIAL || OBSK == WURM_OBS_NONE, "lean rollout: partial_n or no observation");
    const int wave = uniform((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    const Geo g = make_geo<CPL>(p.S);
    const int S = g.S, Sm2 = S - 2, lane = g.lane;
    float *envp = p.envs + env * 3 * g.C;
    Env<CPL> e;
    load_state<CPL, true>(envp, g, e);

    Fast f = {-1, 0, 0, 0, 0, -1};
    bool lean = fast_init<CPL>(e, g, f);
    if (lean) {
        const bool head_in = f.hc >= 0 && (unsigned)(f.hy - 1) < (unsigned)Sm2 && (unsigned)(f.hx - 1) < (unsigned)Sm2;
        int under_food = 0;
        if (f.food >= 0) under_food = lane_value(f.food >= 64 ? e.body[1] : e.body[0], f.food & 63);
        lean = head_in && under_food == 0;
    }
    if (!uniform((int)lean)) {
        rollout_generic<CPL, true, OBSK, false>(p, env, envp, g, e, wurm_lds + wave * p.lds_per_wave);
        return;
    }

    const u64 env_id = (u64)(p.env_offset + env);
    const u64 int0 = ballot((g.interior & 1) != 0), int1 = ballot((g.interior & 2) != 0);
    const float rcpSm2 = 1.0f / (float)Sm2;
    // carried scalars: head row - 1, head column - 1, head cell, length, orientation * 16, food cell
    int hy1 = uniform(f.hy) - 1, hx1 = uniform(f.hx) - 1, hc = uniform(f.hc), L = uniform(f.L), o16 = uniform(f.o) << 4;
    int food = uniform(f.food);
    int foodc = food - (COMPACT ? S + 1 : 0); // the food cell in the crop's cell numbering
    int G = L;                                // G = T + L: the expiry clock a new head cell gets; +1 every step
    int ex0 = e.body[0], ex1 = e.body[1];     // expiry clock of cells lane, lane + 64
    // cells whose entry makes a step "eventful" besides body cells: the border ring (edge collision) and the food cell
    const u64 ring0 = lane_mask((g.valid & 1) != 0) & ~int0, ring1 = lane_mask((g.valid & 2) != 0) & ~int1;
    u64 X0 = ring0 | ((unsigned)food < 64u ? 1ull << food : 0), X1 = ring1 | (food >= 64 ? 1ull << (food - 64) : 0);

    // partial_n crop: lane owns window cell w (lanes past the window repeat its last cell: same address, same value).
    // COMPACT (S <= 9): the interior cells S+1 .. S*S-S-2 fit one 64-bit occupancy mask M with bit 63 to spare;
    // bit 63 is kept set and the centre lane (the head cell itself) looks at it, the others at head cell + offset.
    const int n = OBSK == WURM_OBS_PARTIAL ? p.obs_n : 0, W = 2 * n + 1, W2 = W * W;
    const int w = min(lane, W2 - 1), wy = div_size(w, 1.0f / (float)W), wx = w - wy * W;
    const int dy0 = wy - n, dx0 = wx - n;                                // window row / column offset from the head
    const bool centre = w == n * W + n;
    const int cell_d = dy0 * S + dx0 - (COMPACT ? S + 1 : 0);           // crop cell = head cell + cell_d
    const float green = centre ? 1.0f : 127.0f / 255.0f;                 // what an occupied cell shows in channel 1
    const u32 off_r = (u32)w * 4u, off_g = (u32)(W2 + w) * 4u, off_b = (u32)(2 * W2 + w) * 4u;
    const long long obs_stride = p.N * p.obs_elems;
    float *obs_t = p.obs + env * p.obs_elems;

    for (long long t0 = 0; t0 < p.T; t0 += 64) {
        const int nt = (int)min((long long)64, p.T - t0);
        const long long my_t = t0 + lane;
        long long my_a = lane < nt ? load_action(p.actions, p.act_dtype, my_t * p.N + env) : 0;
        asm volatile("" : "+v"(my_a)); // retire the load here, not in front of the first readlane of the step loop
        // Moves of step t0 + lane for each of the four orientations the snake may have by then, 16 bits each:
        // sanitised action (single_snake.py:221-222) & 7 | next orientation << 4 | (row step & 3) << 6
        // | (column step & 3) << 8 | (cell step & 63) << 10, the step being -TAP[action] (:225-233).  The step loop
        // reads both words with readlanes that do not depend on the state (so they are off its critical path) and
        // picks one with the carried orientation.
        int my_mov01, my_mov23;
        {
            const bool in_range = my_a >= 0 && my_a < 4;
            const int a_small = in_range ? (int)my_a : 7, a_mod = (int)(my_a % 4);
            int ent[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int a_out = o == a_small ? (o ^ 2) : a_mod;
                const int ai = a_out & 3, dy = -tap_y(ai), dx = -tap_x(ai);
                ent[o] = (a_out & 7) | ((ai ^ 2) << 4) | ((dy & 3) << 6) | ((dx & 3) << 8) | (((dy * S + dx) & 63) << 10);
            }
            my_mov01 = ent[0] | (ent[1] << 16);
            my_mov23 = ent[2] | (ent[3] << 16);
        }
        const u64 my_call = p.call + 2ull * (u64)my_t; // step t uses call0 + 2t, its reset call0 + 2t + 1
        const LeanReset my_reset = lean_reset_draw(p.seed, my_call + 1ull, env_id, S, rcpSm2);
        const int my_food = (int)rng_words(p.seed, my_call, env_id, RNG_FOOD, 0).w[0];
        // what lane j keeps of step t0 + j: its move entry, whether it ate, self collision | edge collision << 1
        int my_rec = 0, my_ate = 0, my_fl = 0;
        {   // re-base the clocks so that they cannot overflow however long the tape is
            const int T = G - L;
            ex0 = max(ex0 - T, 0);
            ex1 = max(ex1 - T, 0);
            G = L;
        }

        for (int j = 0; j < nt; ++j) {
            // ---- step (single_snake.py:197-304; same line references as step_core / fast_step)
            // the two words are the halves of one 64-bit table: entry o is bits [16 o, 16 o + 16)
            const u64 mov = (u64)(u32)lane_value(my_mov01, j) | ((u64)(u32)lane_value(my_mov23, j) << 32);
            const int ent = (int)(u32)(mov >> o16);
            o16 = ent & 48;
            hy1 += (ent << 24) >> 30;                // the head is off the border ring: the move stays on the grid
            hx1 += (ent << 22) >> 30;
            hc += (ent << 16) >> 26;
            G += 1;
            // L += (head cell == food cell)  (:242; spelled out: the compiler detours through a 64-bit lane mask)
            asm("s_cmp_eq_u32 %1, %2\n\ts_addc_u32 %0, %0, 0" : "+s"(L) : "s"(hc), "s"(food) : "scc");
            const int T = G - L;                     // :246-249: the clock stands still on the step that eats
            const u64 p0 = lane_mask(ex0 > T), p1 = lane_mask(ex1 > T); // body after the decay, before the head is written
            ex0 = lane == hc ? G : ex0;              // :258-262
            ex1 = lane + 64 == hc ? G : ex1;
            // One test for everything that is not a plain move: the head entered a body cell (:252), the border ring
            // (:290-295) or the food cell (:242).
            const u64 special = hc >= 64 ? (p1 | X1) : (p0 | X0);
            bool finished = false, selfc = false, edgec = false;
            if (__builtin_expect(((special >> (hc & 63)) & 1) != 0, 0)) {
                if (hc == food) {                    // :270-282
                    my_ate = lane == j ? 1 : my_ate;
                    const u64 head0 = (unsigned)hc < 64u ? 1ull << hc : 0, head1 = hc >= 64 ? 1ull << (hc - 64) : 0;
                    food = lean_food_cell(p0 | head0, p1 | head1, int0, int1, (u32)lane_value(my_food, j), lane);
                    foodc = food - (COMPACT ? S + 1 : 0);
                    X0 = ring0 | ((unsigned)food < 64u ? 1ull << food : 0);
                    X1 = ring1 | (food >= 64 ? 1ull << (food - 64) : 0);
                }
                selfc = (((hc >= 64 ? p1 : p0) >> (hc & 63)) & 1) != 0;
                edgec = max((unsigned)hy1, (unsigned)hx1) >= (unsigned)Sm2;
                finished = selfc | edgec;
            }

            // ---- observation of the stepped state (single_snake.py:166-193): a window cell that is off the grid or
            // on the border ring is (0,0,0); food (1,0,0), head (0,1,0), body (0,127/255,0), background (1,1,1).
            // The class logic stays in the VALU (compare -> select through vcc): every detour of a lane mask through
            // scalar logic and back costs a lone wave about two extra issue slots.
            if (OBSK == WURM_OBS_PARTIAL) {
                const unsigned off_grid = max((unsigned)(hy1 + dy0), (unsigned)(hx1 + dx0)); // < S-2: a live cell
                const int cell = (COMPACT && centre) ? 63 : hc + cell_d;
                unsigned occ;
                if (COMPACT) {
                    const u64 M = (p0 >> (S + 1)) | (p1 << (63 - S)) | (1ull << 63);
                    u64 sh; // M >> cell; spelled out: the compiler prefers (1 << cell) & M, two 64-bit VALU ops more
                    asm("v_lshrrev_b64 %0, %1, %2" : "=v"(sh) : "v"(cell), "s"(M));
                    occ = (u32)sh & 1u;
                } else {
                    occ = ((u32)((cell < 64 ? p0 : p1) >> (cell & 63)) & 1u) | (centre ? 1u : 0u);
                }
                const float vr = (off_grid | (occ << 30)) < (unsigned)Sm2 ? 1.0f : 0.0f;          // live and free
                const float vb = cell == foodc ? 0.0f : vr;                                       // ... and not food
                const float vg = (off_grid | ((occ ^ 1u) << 30)) < (unsigned)Sm2 ? green : vb;    // live and occupied
                // scalar base + 32-bit lane offset form, spelled out: the compiler hoists the zero-extension of the
                // lane offsets out of the loop and then pays a 64-bit VALU add per store.  (Untracked stores are
                // harmless for its vmcnt bookkeeping: nothing is read back and waits only become conservative.)
                asm volatile("global_store_dword %0, %1, %2" : : "v"(off_r), "v"(vr), "s"(obs_t) : "memory");
                asm volatile("global_store_dword %0, %1, %2" : : "v"(off_g), "v"(vg), "s"(obs_t) : "memory");
                asm volatile("global_store_dword %0, %1, %2" : : "v"(off_b), "v"(vb), "s"(obs_t) : "memory");
                obs_t += obs_stride;
            }
            my_rec = set_lane(my_rec, ent, j);

            // ---- reset of a finished env (single_snake.py:322-387)
            if (__builtin_expect(finished, 0)) {
                my_fl = lane == j ? (selfc ? 1 : 0) | (edgec ? 2 : 0) : my_fl;
                const int ra = lane_value(my_reset.a, j), rb = lane_value(my_reset.b, j);
                hy1 = (ra & 15) - 1; hx1 = ((ra >> 4) & 15) - 1; o16 = ((ra >> 8) & 3) << 4; food = ra >> 10;
                foodc = food - (COMPACT ? S + 1 : 0);
                X0 = ring0 | ((unsigned)food < 64u ? 1ull << food : 0);
                X1 = ring1 | (food >= 64 ? 1ull << (food - 64) : 0);
                hc = rb & 127;
                const int sc = (rb >> 7) & 127, tc = rb >> 14;
                const int c1 = lane + 64;
                ex0 = lane == tc ? T + 1 : 0; ex0 = lane == sc ? T + 2 : ex0; ex0 = lane == hc ? T + 3 : ex0;
                ex1 = c1 == tc ? T + 1 : 0;   ex1 = c1 == sc ? T + 2 : ex1;   ex1 = c1 == hc ? T + 3 : ex1;
                L = 3;
                G = T + 3;
            }
        }
        if (lane < nt) {
            const long long i = my_t * p.N + env;
            store_action(p.actions, p.act_dtype, i, (long long)((my_rec << 29) >> 29));
            p.reward[i] = my_ate ? 1.0f : 0.0f;
            p.done[i] = (uint8_t)(my_fl != 0);
            p.selfc[i] = (uint8_t)(my_fl & 1);
            p.edgec[i] = (uint8_t)(my_fl >> 1);
        }
    }
    const int T = G - L;
    e.body[0] = max(ex0 - T, 0);
    e.body[1] = max(ex1 - T, 0);
    f.hc = hc; f.hy = hy1 + 1; f.hx = hx1 + 1; f.L = L; f.o = o16 >> 4; f.food = food;
    fast_sync_bits<CPL>(e, g, f);
    store_state<CPL, true>(envp, g, e);
}

// ------------------------------------------------------------------------------------------- 9 x 9 rollout
// The reference's default grid (size 9: 7 x 7 interior cells) gets one more specialisation of the lean loop.
// Cells are numbered code = 8 * row + column.  The 49 interior cells have distinct codes in 9..63, so ONE lane per
// interior cell holds the whole body channel (one expiry clock per lane, one 64-bit occupancy mask); the border
// ring's codes alias only each other, also modulo 64 (column 8 of a row = column 0 of the next, row 8 = row 0), so
//   * "the head entered the ring, a body cell or the food cell" is one bit test on (occupancy | RING | food bit);
//   * which window cells of the crop are inside the ring is a per-lane constant 64-bit table indexed by the head
//     code (valid while the head is inside the ring; the final observation of an env whose head is on the ring is
//     computed from row / column arithmetic on the rare path).
// Extra preconditions (else rollout_generic): no body and no food on the ring.

// INJ: the random outcomes (food cell of an eating step, seed cell / direction / food cell of a reset) come from
// p.inject_food / p.inject_reset instead of Philox, so that the tapes recorded from the reference (tests/golden) run
// through THIS kernel; the RNG instantiation is compiled without any of it.
// PAIR: a workgroup of two waves per env (single_launch.hpp: batches of at most WURM_S9_PAIR_MAX_ENVS envs).  Wave 1 does
// what a chunk needs around its step loop — tape load, move entries, Philox blocks or recorded outcomes one chunk ahead,
// the record stores one chunk behind — and wave 0 only steps (DESIGN.md section 4 has the protocol and the measurements).
// CROPH (with PAIR and partial_n only; single_launch.hpp: launches of at least WURM_S9_CROP_HELPER_MIN_STEPS steps): wave 1
// also renders the crops, one chunk behind, from what wave 0 records of each step; wave 0's loop holds the transition alone.
// RW (with CROPH; single_launch.hpp: batches of at most WURM_S9_TRIO_MAX_ENVS envs, launches of at least WURM_S9_TRIO_MIN_STEPS
// steps): the number of waves that render.  RW = 2 is the trio form, a workgroup of three waves per env: wave 1 renders the
// first steps of each chunk only, wave 2 renders the others and does nothing else, on wave 1's barrier schedule.
template <int OBSK, bool INJ = false, bool PAIR = false, bool CROPH = false, int RW = 1>
__global__ __launch_bounds__(256) void rollout_s9_kernel(StepArgs p)
{
    constexpr int CPL = 2, S = 9;
    // RW = 2: of a chunk's 64 steps the helper renders the first 24 — its other work takes the time of about 9 passes of the
    // 32 (tools/kernel_timeline.py --render-waves 2) —, of the last chunk's the first half
    constexpr int S9_TRIO_SHARE = 24, S9_TRIO_LAST_SHARE = 32;
    static_assert(OBSK == WURM_OBS_PARTIAL || OBSK == WURM_OBS_NONE, "9x9 rollout: partial_n or no observation");
    static_assert(!CROPH || (PAIR && OBSK == WURM_OBS_PARTIAL), "9x9 rollout: the helper renders the crops of the pair form");
    static_assert(RW == 1 || (RW == 2 && CROPH), "9x9 rollout: a second render wave beside a helper that renders");
    constexpr bool REBUILD = CROPH && RW == 2; // the trio form: the render waves rebuild the head and food codes of a chunk
    const int wave = uniform((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
    // PAIR: one workgroup of two (RW = 2: three) waves per env; all take the next line's exit, or none
    const long long env = PAIR ? xcd_block(blockIdx.x, gridDim.x) : xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    const Geo g = make_geo<CPL>(S);
    const int lane = g.lane;
    const u64 env_id = (u64)(p.env_offset + env);
    WURM_TL_DECL;
    WURM_TL(0);
    WURM_TL(6);

    // What the 64 steps of the chunk at t0 need that does not depend on the state, step t0 + lane in lane `lane`.
    const auto chunk_draw = [&](const long long t0, const int nt) __attribute__((always_inline)) {
        S9Chunk ch;
        const long long my_t = t0 + lane;
        long long my_a = lane < nt ? load_action(p.actions, p.act_dtype, my_t * p.N + env) : 0;
        asm volatile("" : "+v"(my_a)); // retire the load here, not in front of the first readlane of the step loop
        if constexpr (!PAIR) WURM_TL_LAP(1);
        // Moves of step t0 + lane for each of the four orientations the snake may have by then, 16 bits each:
        // next orientation << 4 | (code step & 63) << 6 | (sanitised action (single_snake.py:221-222) & 7) << 12, the
        // step being -TAP[action] (:225-233); bits 0-3 are zero, so the low 6 bits of an entry are the shift that picks
        // the NEXT step's entry.  The step loop reads both words with readlanes that do not depend on the state.
        {
            const auto entry = [](int a_out) {
                const int ai = a_out & 3;
                return ((ai ^ 2) << 4) | (((-tap_y(ai) * 8 - tap_x(ai)) & 63) << 6) | ((a_out & 7) << 12);
            };
            const bool in_range = my_a >= 0 && my_a < 4;
            const int a_small = in_range ? (int)my_a : 7, a_mod = (int)(my_a % 4);
            int me[4];
#pragma unroll
            for (int o = 0; o < 4; ++o)
                me[o] = entry(o == a_small ? (o ^ 2) : a_mod);
            ch.mov01 = me[0] | (me[1] << 16);
            ch.mov23 = me[2] | (me[3] << 16);
        }
        const u64 my_call = p.call + 2ull * (u64)my_t; // step t uses call0 + 2t, its reset call0 + 2t + 1
        if constexpr (INJ) {
            // recorded outcomes of step t0 + lane, converted to cell codes 8 * row + column (reset_core's layout of inj[])
            int sy = 4, sx = 4, d = 0, fc = -1, fe = -1;
            if (lane < nt) {
                const int *ir = p.inject_reset + (my_t * p.N + env) * 4;
                sy = ir[0]; sx = ir[1]; d = ir[2]; fc = ir[3];
                fe = p.inject_food[my_t * p.N + env];
            }
            asm volatile("" : "+v"(sy), "+v"(sx), "+v"(d), "+v"(fc), "+v"(fe)); // retire the loads before the step loop
            d &= 3;
            const int sc = sy * 8 + sx, dc = tap_y(d) * 8 + tap_x(d);
            const int fcy = div_size(max(fc, 0), g.rcpS), fey = div_size(max(fe, 0), g.rcpS);
            const int fcode = (fc >= 0 && fc < S * S) ? fcy * 8 + (fc - fcy * S) : -1;
            ch.reset.a = d | (fcode << 2);
            ch.reset.b = (sc + dc) | (sc << 7) | ((sc - dc) << 14);
            ch.food = (fe >= 0 && fe < S * S) ? fey * 8 + (fe - fey * S) : -1;
        } else {
            ch.reset = s9_reset_draw(p.seed, my_call + 1ull, env_id);
            ch.food = (int)rng_words(p.seed, my_call, env_id, RNG_FOOD, 0).w[0];
        }
        return ch;
    };
    // The step records of the chunk at t0, lane j's being step t0 + j's: sanitised action, ate, self collision | edge collision << 1
    const auto flush = [&](const long long t0, const int nt, const int act, const int ate, const int fl) __attribute__((always_inline)) {
        if (lane < nt) {
            const long long i = (t0 + lane) * p.N + env;
            store_action(p.actions, p.act_dtype, i, (long long)act);
            p.reward[i] = ate ? 1.0f : 0.0f;
            p.done[i] = (uint8_t)(fl != 0);
            p.selfc[i] = (uint8_t)(fl & 1);
            p.edgec[i] = (uint8_t)(fl >> 1);
        }
    };

    // PAIR: the helper wave (wave 1) works one chunk ahead of the stepper (wave 0) and one behind it, through LDS behind
    // rollout_generic's region: chunk buffers k & 1 (S9Chunk, 5 dwords x 64 lanes), record buffers k & 1 (64 dwords: action
    // & 7 | ate << 3 | collisions << 4), and the stepper's verdict on the state.  Both waves pass 1 + ceil(T / 64) barriers:
    // B0 once chunk 0 and the verdict are written, B(k+1) at the end of chunk k.  Between B(k) and B(k+1) the helper writes
    // chunk buffer (k+1) & 1 and reads record buffer (k-1) & 1, the stepper reads chunk buffer k & 1 (at once, into
    // registers) and writes record buffer k & 1 (last).
    // CROPH: a record buffer is four planes of 64 dwords, the word above and what the crop of step t0 + j is a function of:
    // head code | (food code + 1) << 7 | move entry bits 4-14 << 14 | collisions << 25, and the two halves of the body mask
    // without the head.  Between B(k) and B(k+1) the helper also renders chunk k - 1 from record buffer (k-1) & 1 (last, after
    // the tape load and the record stores); after the last barrier it renders the last chunk.  Same barriers, same parities.
    // RW = 2: wave 2 passes the helper's barriers — B0, then the verdict, then one per chunk — and between them renders the
    // steps from S9_TRIO_SHARE / 64 of the chunk on (of the last chunk, which the helper renders with no tape left to load:
    // from S9_TRIO_LAST_SHARE / 64 on) from the same record buffer, which both renderers only read; the helper renders the
    // steps before.  No parity or barrier more.  (The split is even, so that a pass of two steps never straddles it.)
    // REBUILD (RW = 2): the stepper records per step only the move entry, and on an eating step the food it drew; plane 1 of
    // a record buffer holds the crop word without the head code, its food field defined on eating steps alone, and there
    // are no body planes.  The record buffer is five planes and three dwords: at the START of chunk k the stepper copies the
    // re-based clocks `ex` it enters the chunk with (plane 2, one clock per cell), the chunk's would-be reset words (planes
    // 3, 4) and the head code, food code and length it enters the chunk with (dwords 320-322) into record buffer k & 1,
    // whose last readers passed B(k); so they live as long as the record — the chunk buffer the reset words come from is
    // overwritten by the helper (chunk k + 2) just while chunk k is rendered.  Each render wave rebuilds the crop words
    // (s9_rebuild_crop_words) and the body masks (s9_rebuild_body) of all 64 steps, step j in lane j, into three planes of
    // its own behind the verdict, which no other wave touches, and renders its share from there: both rebuild, neither
    // waits for the other.
    int *const pair_lds = (int *)(wurm_lds + p.lds_per_wave);
    constexpr int PAIR_CHUNK = 5 * 64, PAIR_REC = 2 * PAIR_CHUNK, PAIR_RECSZ = REBUILD ? 5 * 64 + 4 : CROPH ? 4 * 64 : 64;
    constexpr int PAIR_LEAN = PAIR_REC + 2 * PAIR_RECSZ, PAIR_OWN = PAIR_LEAN + 4;
    const long long n_chunks = (p.T + 63) >> 6;
    if constexpr (PAIR) {
        if (wave != 0) {
            const bool renders_only = RW == 2 && wave == 2; // wave-uniform: wave 2 of the trio form
            const auto draw_into = [&](const long long k) __attribute__((always_inline)) {
                const long long t0 = k << 6;
                const S9Chunk ch = chunk_draw(t0, (int)min((long long)64, p.T - t0));
                int *cb = pair_lds + (int)(k & 1) * PAIR_CHUNK + lane;
                cb[0] = ch.mov01; cb[64] = ch.mov23; cb[128] = ch.reset.a; cb[192] = ch.reset.b; cb[256] = ch.food;
            };
            const auto flush_from = [&](const long long k) __attribute__((always_inline)) {
                const long long t0 = k << 6;
                const int rec = pair_lds[PAIR_REC + (int)(k & 1) * PAIR_RECSZ + lane];
                flush(t0, (int)min((long long)64, p.T - t0), (rec << 29) >> 29, (rec >> 3) & 1, rec >> 4);
            };
            // CROPH: the crops of chunk k from record buffer k & 1.  The steps are independent: every lane reads its own
            // step's record, so a window of at most 32 cells renders two steps per pass (lanes 0-31 step j, lanes 32-63
            // step j + 1; an odd tail renders its last step in both halves: same address, same value).  The head is the
            // window's centre cell, so `taken` is the body bit or "this lane is the centre"; on an edge collision the head is on
            // the ring, the centre is outside (shows nothing) and the bit the head would have set aliases ring cells only.
            // (WURM_S9_CROP_SPP1: a build for tools/kernel_timeline.py that renders one step per pass whatever the window)
            int spp = 1, sub = 0;
            S9Window win = {};
            if constexpr (CROPH) {
#ifndef WURM_S9_CROP_SPP1
                spp = (2 * p.obs_n + 1) * (2 * p.obs_n + 1) <= 32 ? 2 : 1;
#endif
                sub = spp == 2 ? lane >> 5 : 0;
                win = s9_window(spp == 2 ? lane & 31 : lane, p.obs_n);
            }
            const auto render = [&](const long long k, const int share) __attribute__((always_inline)) {
                const int W2 = (2 * p.obs_n + 1) * (2 * p.obs_n + 1);
                const long long t0 = k << 6, obs_stride = p.N * p.obs_elems;
                const int nt = (int)min((long long)64, p.T - t0);
                // this wave's steps of the chunk: [j0, j1)
                const int split = RW == 2 ? ((nt * share) >> 6) & ~1 : nt;
                const int j0 = renders_only ? split : 0, j1 = renders_only ? nt : split;
                const int *rb = pair_lds + PAIR_REC + (int)(k & 1) * PAIR_RECSZ;
                // the crop word of step j at words[j], the halves of its body mask without the head at body_lo[j], body_hi[j]
                const int *words = rb + 64, *body_lo = rb + 128, *body_hi = rb + 192;
                if constexpr (REBUILD) {
                    int *own = pair_lds + PAIR_OWN + (wave - 1) * 3 * 64;
                    const int rec = rb[lane], reset_b = rb[256 + lane];
                    const int w1 = s9_rebuild_crop_words(rec, rb[64 + lane], rb[192 + lane], reset_b, uniform(rb[320]), uniform(rb[321]), lane);
                    const u64 body = s9_rebuild_body(rec, w1, reset_b, rb[128 + lane], uniform(rb[322]), lane);
                    own[lane] = w1;
                    own[64 + lane] = (int)(u32)body;
                    own[128 + lane] = (int)(u32)(body >> 32);
                    words = own; body_lo = own + 64; body_hi = own + 128;
                    WURM_TL_LAP(5); // (the render waves' slot 5: both rebuilds, LDS reads and writes included)
                }
                const int centre = win.code_d == 0 ? 1 : 0, code_d1 = win.code_d + 1;
                float *obs_t = p.obs + ((t0 + j0) * p.N + env) * p.obs_elems;
                const auto pass = [&](const int j, const int my_sub) __attribute__((always_inline)) {
                    const int sj = j + my_sub;
                    const int w1 = words[sj];
                    const u64 body = (u64)(u32)body_lo[sj] | ((u64)(u32)body_hi[sj] << 32);
                    const int c = w1 & 127;
                    // (both shifts read the low 6 bits of their amount, which are those of the head code in w1)
                    unsigned inside = (u32)(win.live_tab >> (w1 & 63)) & 1u;
                    const bool edge = ((w1 >> 26) & 1) != 0;
                    if (lane_mask(edge) != 0) {
                        // the head is on the ring and its code may have wrapped: row / column arithmetic from the cell it left
                        const int ai = (w1 >> 22) & 3, pc = c - ((w1 << 10) >> 26);
                        const int hy = (pc >> 3) - tap_y(ai), hx = (pc & 7) - tap_x(ai);
                        const unsigned e_inside = max((unsigned)(hy + win.dy0 - 1), (unsigned)(hx + win.dx0 - 1)) < 7u ? 1u : 0u;
                        inside = edge ? e_inside : inside;
                    }
                    const unsigned taken = ((u32)(body >> ((w1 + win.code_d) & 63)) & 1u) | (u32)centre;
                    const unsigned both = inside & taken;
                    const int code1 = c + code_d1, food1 = (w1 >> 7) & 127; // window cell code + 1, food code + 1 (0: no food)
                    // as the stepper's crop: vr = inside > taken, vb = code == food ? 0 : vr, vg = inside & taken ? green : vb
                    const float vr = inside > taken ? 1.0f : 0.0f;
                    const float vb = code1 != food1 ? vr : 0.0f;
                    const float vg = both != 0 ? win.green : vb;
                    const u32 o = (u32)((long long)my_sub * obs_stride * 4) + (u32)win.w * 4u;
                    // (said outright: the instrumented build loses track of the base being wave-uniform and offers a VGPR pair)
                    float *const obs_s = (float *)uniform64((long long)obs_t);
                    asm volatile("global_store_dword %0, %1, %6\n\tglobal_store_dword %2, %3, %6\n\tglobal_store_dword %4, %5, %6"
                                 : : "v"(o), "v"(vr), "v"(o + (u32)W2 * 4u), "v"(vg), "v"(o + (u32)W2 * 8u), "v"(vb), "s"(obs_s) : "memory");
                };
                int j = j0;
                for (; j + spp <= j1; j += spp) {
                    pass(j, sub);
                    obs_t += spp * obs_stride;
                }
                if (j < j1) pass(j, 0);
            };
            if (n_chunks > 0 && !renders_only) draw_into(0);
            pair_barrier(); // B0
            if (uniform(pair_lds[PAIR_LEAN]) == 0) return; // the stepper runs rollout_generic, which has no barrier
            for (long long k = 0; k < n_chunks; ++k) {
                if (!renders_only) {
                    if (k + 1 < n_chunks) draw_into(k + 1); // (reads the tape of chunk k + 1 before chunk k - 1 is written back)
                    if (k > 0) flush_from(k - 1);
                }
                if constexpr (CROPH) {
                    WURM_TL_LAP(1);
                    if (k > 0) render(k - 1, S9_TRIO_SHARE);
                    WURM_TL_LAP(2);
                }
                pair_barrier(); // B(k+1)
                if constexpr (CROPH) WURM_TL_LAP(3);
            }
            if (n_chunks > 0 && !renders_only) flush_from(n_chunks - 1);
            if constexpr (CROPH) {
                WURM_TL_LAP(1);
                if (n_chunks > 0) render(n_chunks - 1, S9_TRIO_LAST_SHARE);
                WURM_TL_LAP(4);
                // (the helper's laps go over the crop of step 1, wave 2's over that of step 2, the stepper's over that of step 0)
                if (p.T > wave) WURM_TL_STORE(p.obs + (wave * p.N + env) * p.obs_elems, lane);
            }
            return;
        }
    }

    float *envp = p.envs + env * 3 * (S * S);
    Env<CPL> e;
    load_state<CPL, true>(envp, g, e);

    Fast f = {-1, 0, 0, 0, 0, -1};
    bool lean = fast_init<CPL>(e, g, f);
    if (lean) {
        const bool head_in = f.hc >= 0 && (unsigned)(f.hy - 1) < 7u && (unsigned)(f.hx - 1) < 7u;
        const int fy = f.food >= 0 ? div_size(f.food, g.rcpS) : 1, fx = f.food >= 0 ? f.food - fy * S : 1;
        const bool food_in = (unsigned)(fy - 1) < 7u && (unsigned)(fx - 1) < 7u;
        int under_food = 0;
        if (f.food >= 0) under_food = lane_value(f.food >= 64 ? e.body[1] : e.body[0], f.food & 63);
        const bool ring_body = lane_mask((e.body[0] > 0 && !(g.interior & 1)) || (e.body[1] > 0 && !(g.interior & 2))) != 0;
        lean = head_in && food_in && under_food == 0 && !ring_body;
    }
    if constexpr (PAIR) {
        if (lane == 0) pair_lds[PAIR_LEAN] = lean ? 1 : 0;
        pair_barrier(); // B0
    }
    if (!uniform((int)lean)) {
        rollout_generic<CPL, true, OBSK, INJ, true>(p, env, envp, g, e, wurm_lds + wave * p.lds_per_wave); // (several heads: as the reference)
        return;
    }

    // code layout: lane = 8 * row + column holds that cell if it is inside the ring
    const int ly = lane >> 3, lx = lane & 7;
    const bool lane_in = ly >= 1 && lx >= 1;
    const int my_cell = ly * S + lx;
    const u64 RING = ~lane_mask(lane_in);
    int ex = lane_in ? __float2int_rn(envp[2 * S * S + my_cell]) : 0; // expiry clock of the lane's cell (body, re-read)
    // carried scalars: head code, the last move entry (its low 6 bits are orientation * 16), food code (-1: none), the
    // clock as T1 = T + 1 and G = T + length (the length itself is only ever needed as G - T)
    int c = uniform(f.hy) * 8 + uniform(f.hx), ent = uniform(f.o) << 4;
    int foodc = -1;
    if (f.food >= 0) {
        const int fy = uniform(div_size(f.food, g.rcpS)); // (float arithmetic: a VALU result, back to an SGPR)
        foodc = fy * 8 + (uniform(f.food) - fy * S);
    }
    u64 XF = RING | (foodc >= 0 ? 1ull << foodc : 0); // ring + food: the non-body cells that make a step eventful
    int G = uniform(f.L), T1 = 1;

    // partial_n crop: lane owns window cell w (lanes past the window repeat its last cell: same address, same value)
    const int n = OBSK == WURM_OBS_PARTIAL ? p.obs_n : 0, W = 2 * n + 1, W2 = W * W;
    const int w = min(lane, W2 - 1), wy = div_size(w, 1.0f / (float)W), wx = w - wy * W;
    const int dy0 = wy - n, dx0 = wx - n;      // window row / column offset from the head
    const int code_d = dy0 * 8 + dx0;          // code of the window cell = head code + code_d
    const float green = (w == n * W + n) ? 1.0f : 127.0f / 255.0f; // what an occupied cell shows in channel 1
    u64 live_tab = 0;                          // bit (8 * row + column): with the head there, this window cell is inside the ring
#pragma unroll
    for (int y = 1; y <= 7; ++y) {
        u32 cols = 0;
#pragma unroll
        for (int x = 1; x <= 7; ++x)
            if ((unsigned)(x + dx0 - 1) < 7u) cols |= 1u << x;
        if ((unsigned)(y + dy0 - 1) < 7u) live_tab |= (u64)cols << (8 * y);
    }
    const u32 off_r = (u32)w * 4u, off_g = (u32)(W2 + w) * 4u, off_b = (u32)(2 * W2 + w) * 4u;
    const long long obs_stride = p.N * p.obs_elems;
    float *obs_t = p.obs + env * p.obs_elems;

    WURM_TL_LAP(5);
    for (long long t0 = 0; t0 < p.T; t0 += 64) {
        const int nt = (int)min((long long)64, p.T - t0);
        int my_mov01, my_mov23, my_food; // my_food, RNG: the word the food cell is drawn with; INJ: the food code itself (-1: none)
        S9Reset my_reset;
        if constexpr (PAIR) {
            const int *cb = pair_lds + (int)((t0 >> 6) & 1) * PAIR_CHUNK + lane;
            my_mov01 = cb[0]; my_mov23 = cb[64]; my_reset.a = cb[128]; my_reset.b = cb[192]; my_food = cb[256];
            // retire the reads here, not in front of the first readlane of the step loop
            asm volatile("" : "+v"(my_mov01), "+v"(my_mov23), "+v"(my_reset.a), "+v"(my_reset.b), "+v"(my_food));
            WURM_TL_LAP(1);
        } else {
            const S9Chunk ch = chunk_draw(t0, nt);
            my_mov01 = ch.mov01; my_mov23 = ch.mov23; my_reset = ch.reset; my_food = ch.food;
#ifdef WURM_TIMELINE
            asm volatile("" : "+v"(my_mov01), "+v"(my_mov23), "+v"(my_reset.a), "+v"(my_reset.b), "+v"(my_food));
#endif
            WURM_TL_LAP(2);
        }
        // what lane j keeps of step t0 + j: its move entry, whether it ate, self collision | edge collision << 1
        int my_rec = 0, my_ate = 0, my_fl = 0;
        S9CropRec crop_rec = {0, 0, 0, 0, 0};        // CROPH: what the helper renders step t0 + j's crop from, in lane j
        {   // re-base the clocks so that they cannot overflow however long the tape is
            const int T = T1 - 1;
            ex = max(ex - T, 0);
            G -= T;
            T1 = 1;
        }
        if constexpr (REBUILD) { // what the render waves rebuild the chunk's head codes, food codes and body masks from (protocol: above)
            int *rb = pair_lds + PAIR_REC + (int)((t0 >> 6) & 1) * PAIR_RECSZ;
            rb[128 + lane] = ex;
            rb[192 + lane] = my_reset.a;
            rb[256 + lane] = my_reset.b;
            if (lane == 0) { rb[320] = c; rb[321] = foodc; rb[322] = G; } // (the clock is 0 here: G is the length)
        }

        // one step: step t0 + j of this env.  Inlined U + 1 times below (U copies in the unrolled body, one in the tail
        // loop), each with its own out-of-line event and reset block: the listing holds five of everything in here.
        const auto step = [&](const int j) __attribute__((always_inline)) {
            // ---- step (single_snake.py:197-304; same line references as step_core / fast_step)
            // The body after the decay of a step that does not eat, before the head is written and before the move is
            // known: such a step advances the clock to T1.  A step that eats leaves the clock alone; it takes the
            // event branch (XF holds the food bit) and looks again there.  (Up here the compare's way to the scalar
            // unit is covered by the move's scalar instructions.)
            const u64 body_moved = lane_mask(ex > T1);
            // the two words are the halves of one 64-bit table: entry o is bits [16 o, 16 o + 16)
            const u64 mov = (u64)(u32)lane_value(my_mov01, j) | ((u64)(u32)lane_value(my_mov23, j) << 32);
            ent = (int)(u32)(mov >> (ent & 63));     // (the shift reads the low 6 bits of its amount: no instruction)
            if constexpr (!CROPH) my_rec = set_lane(my_rec, ent, j); // lane j keeps the record of step t0 + j
            // c += code step: the head is inside the ring, so the move stays on the grid (in place: left to the compiler, the
            // sum lands in a new register and the plain move pays a copy on the back edge)
            asm("s_add_i32 %0, %0, %1" : "+s"(c) : "s"((ent << 20) >> 26) : "scc");
            G += 1;
            // T1 += head != food, through the carry: the clock stands still on the step that eats (:242, :246-249), which
            // is the length growing by one
            asm("s_cmp_lg_u32 %1, %2\n\ts_addc_u32 %0, %0, 0" : "+s"(T1) : "s"(c), "s"(foodc) : "scc");
            // CROPH: the record of a plain move, of a collision and of the reset behind it; a step that eats rewrites its lane below
            // (REBUILD: the move entry alone)
            if constexpr (REBUILD) crop_rec.ent = set_lane(crop_rec.ent, ent, j);
            else if constexpr (CROPH) set_lane(crop_rec, ent, c, foodc, body_moved, j);
            u64 body = body_moved;
            const u64 head = 1ull << (c & 63);
            ex = keep_in_lane(ex, G, head);          // :258-262 (a head on the ring may land in a wrong lane: it is reset below)
            u64 occ = body | head;

            // what the crop shows: per lane, is the window cell inside the ring (0 / 1), its code, the occupancy mask
            unsigned inside = 0;
            int code = c + code_d;
            u64 mask = occ;
            if (OBSK == WURM_OBS_PARTIAL && !CROPH) {
                u64 lv; // live_tab >> head code
                asm("v_lshrrev_b64 %0, %1, %2" : "=v"(lv) : "s"(c), "v"(live_tab));
                inside = (u32)lv & 1u;
            }

            // One test for everything that is not a plain move: the head entered a body cell (:252), the border ring
            // (:290-295) or the food cell (:242).  All of it — the reset too — sits behind this one branch, so the plain
            // move carries no event flag and no second test; the crop below is of the state BEFORE the reset and takes
            // what it shows (inside, code, mask, shown_food) from there.
            int shown_food = foodc;
            if (__builtin_expect((((body | XF) >> (c & 63)) & 1) != 0, 0)) {
                const u64 lane_j = 1ull << (j & 63);
                if (c == foodc) {                    // :270-282: K-th free interior cell in row-major order
                    my_ate = keep_in_lane(my_ate, 1, lane_j);
                    // The clock stood still (T = T1 - 1): the cell the tail would have left is still body.  `ex` holds
                    // the head by now, in its own lane (the food cell is inside the ring) and on a cell that was free
                    // (no food lies on a body cell), so the compare gives the occupancy and the body is that less the head.
                    occ = lane_mask(ex > T1 - 1);
                    body = occ & ~head;
                    mask = occ;
                    if constexpr (INJ) {
                        foodc = lane_value(my_food, j);
                    } else {
                        const u64 fr = ~(occ | RING);
                        const int n_free = popc64(fr);
                        foodc = -1;
                        if (n_free > 0) {
                            const int K = (int)mulhi_range((u32)lane_value(my_food, j), (u32)n_free);
                            foodc = first_bit(lane_mask((int)((fr >> lane) & 1) & (int)(rank_below(fr) == K)));
                        }
                    }
                    XF = RING | (foodc >= 0 ? 1ull << foodc : 0);
                    if constexpr (CROPH) // the crop shows the food drawn just now and the body that kept its tail
                        crop_rec.food = set_lane(crop_rec.food, foodc, j);
                    if constexpr (CROPH && !REBUILD) { // (REBUILD: the render waves know that the clock stood still)
                        crop_rec.body_lo = set_lane(crop_rec.body_lo, (int)(u32)body, j);
                        crop_rec.body_hi = set_lane(crop_rec.body_hi, (int)(u32)(body >> 32), j);
                    }
                }
                shown_food = foodc;
                const int event = ((RING >> (c & 63)) & 1) ? 2 : ((body >> (c & 63)) & 1) ? 1 : 0; // self / edge collision
                if (OBSK == WURM_OBS_PARTIAL && !CROPH && event == 2) {
                    // the head is on the ring and its code may have wrapped: row / column arithmetic from the cell it left
                    const int ai = (ent >> 12) & 3, pc = c - ((ent << 20) >> 26);
                    const int hy = (pc >> 3) - tap_y(ai), hx = (pc & 7) - tap_x(ai);
                    inside = max((unsigned)(hy + dy0 - 1), (unsigned)(hx + dx0 - 1)) < 7u ? 1u : 0u;
                    code = (hy + dy0) * 8 + hx + dx0;
                    mask = body;
                }
                // ---- reset of a finished env (single_snake.py:322-387)
                if (event != 0) {
                    my_fl = keep_in_lane(my_fl, event, lane_j);
                    const int ra = lane_value(my_reset.a, j), rb = lane_value(my_reset.b, j);
                    ent = (ra & 3) << 4;             // what is left of the entry: the orientation of the new snake
                    foodc = ra >> 2;
                    XF = INJ ? (RING | (foodc >= 0 ? 1ull << foodc : 0)) : (RING | (1ull << foodc));
                    c = rb & 127;
                    const int sc = (rb >> 7) & 127, tc = rb >> 14;
                    ex = lane == tc ? T1 : 0; ex = lane == sc ? T1 + 1 : ex; ex = lane == c ? T1 + 2 : ex;
                    G = T1 + 2;                      // T + length 3
                }
            }

            // ---- crop of the stepped state (single_snake.py:166-193): a window cell that is off the grid or on the
            // ring is (0,0,0); food (1,0,0), head (0,1,0), body (0,127/255,0), background (1,1,1).  `inside` / `taken`
            // are 0 / 1 per lane; the class logic stays in the VALU (compare -> select through vcc).  (CROPH: the helper's.)
            if (OBSK == WURM_OBS_PARTIAL && !CROPH) {
                u64 sh; // mask >> code; spelled out: the compiler prefers (1 << code) & mask, two 64-bit VALU ops more
                asm("v_lshrrev_b64 %0, %1, %2" : "=v"(sh) : "v"(code), "s"(mask));
                const unsigned taken = (u32)sh & 1u;
                // vr = inside > taken ? 1 : 0        (inside the ring and free)
                // vb = code == food ? 0 : vr         (... and not the food)
                // vg = inside & taken ? green : vb   (inside the ring and occupied)
                // Spelled out: three compares into three SGPR pairs, then three selects.  The compiler funnels all of
                // them through vcc and pads each compare -> select pair with s_nop (gfx950 needs two wait states there).
                const unsigned both = inside & taken;
                float vr, vb, vg;
                u64 m_free, m_not_food, m_taken;
                asm("v_cmp_gt_u32_e64 %3, %6, %7\n\t"
                    "v_cmp_ne_u32_e64 %4, %8, %9\n\t"
                    "v_cmp_ne_u32_e64 %5, 0, %10\n\t"
                    "v_cndmask_b32_e64 %0, 0, 1.0, %3\n\t"
                    "v_cndmask_b32_e64 %1, 0, %0, %4\n\t"
                    "v_cndmask_b32_e64 %2, %1, %11, %5"
                    : "=&v"(vr), "=&v"(vb), "=&v"(vg), "=&s"(m_free), "=&s"(m_not_food), "=&s"(m_taken)
                    : "v"(inside), "v"(taken), "s"(shown_food), "v"(code), "v"(both), "v"(green));
                // scalar base + 32-bit lane offset form, spelled out: the compiler hoists the zero-extension of the
                // lane offsets out of the loop and then pays a 64-bit VALU add per store.  (Untracked stores are
                // harmless for its vmcnt bookkeeping: nothing is read back and waits only become conservative.)
                asm volatile("global_store_dword %0, %1, %6\n\tglobal_store_dword %2, %3, %6\n\tglobal_store_dword %4, %5, %6"
                             : : "v"(off_r), "v"(vr), "v"(off_g), "v"(vg), "v"(off_b), "v"(vb), "s"(obs_t) : "memory");
                obs_t += obs_stride;
            }
        };
        // U steps per back edge while the chunk has that many left, then one by one.  The step index stays a scalar that
        // is advanced per step: the lane selects of the readlanes and of the record take it from a register.
        constexpr int U = 4; // measured against 2 (1.4 % slower) and 8 (0.5-0.9 % slower): DESIGN.md section 13
        const int nu = nt & -U;
        int j = 0;
        for (; j != nu; j += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) step(j + u);
        }
        for (; j < nt; ++j) step(j);
        WURM_TL_LAP(3);
        if constexpr (PAIR) {
            if constexpr (CROPH) {
                // bit fields of the crop word: head code 0-6 (a code is 0 .. 72), food code + 1 7-13 (0 .. 73), move entry
                // bits 4-14 at 14-24, self / edge collision 25 / 26 (the helper tests bit 26); masked, so that a wider event
                // code or a negative head code could not spill into a neighbour
                int *rb = pair_lds + PAIR_REC + (int)((t0 >> 6) & 1) * PAIR_RECSZ + lane;
                my_rec = crop_rec.ent;
                // (REBUILD: crop_rec.c stays 0, the food field holds what an eating step drew; the render waves fill both in)
                rb[64] = (crop_rec.c & 127) | (((crop_rec.food + 1) & 127) << 7) | (((my_rec >> 4) & 0x7FF) << 14) | ((my_fl & 3) << 25);
                if constexpr (!REBUILD) {
                    rb[128] = crop_rec.body_lo;
                    rb[192] = crop_rec.body_hi;
                }
                rb[0] = ((my_rec >> 12) & 7) | (my_ate << 3) | (my_fl << 4);
            } else {
                pair_lds[PAIR_REC + (int)((t0 >> 6) & 1) * 64 + lane] = ((my_rec >> 12) & 7) | (my_ate << 3) | (my_fl << 4);
            }
            pair_barrier(); // B(k+1)
        } else {
            flush(t0, nt, (my_rec << 17) >> 29, my_ate, my_fl);
        }
        WURM_TL_LAP(4);
    }
    // (CROPH: the helper renders step 0's crop behind the stepper's back while there is one chunk only: no stamps then)
    if (OBSK == WURM_OBS_PARTIAL && (!CROPH || p.T > 64)) WURM_TL_STORE(p.obs + env * p.obs_elems, lane);
    if (lane_in) { // the ring was empty and still is
        envp[my_cell] = lane == foodc ? 1.0f : 0.0f;
        envp[S * S + my_cell] = lane == c ? 1.0f : 0.0f;
        envp[2 * S * S + my_cell] = (float)max(ex - (T1 - 1), 0);
    }
}

// wurm.utils.env_consistency (wurm/utils.py:113-178) per env, as an error bitmask
template <int CPL>
__global__ __launch_bounds__(256) void check_kernel(const float *__restrict__ envs, uint32_t *__restrict__ err,
                                                    long long N, int S)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= N) return;
    const Geo g = make_geo<CPL>(S);
    const float *envp = envs + env * 3 * g.C;
    // in fp32 like the reference's sums (wurm/utils.py:113-178) — a state that holds non-integers (food 0.5, only ever by
    // hand) gets the reference's verdict on every check, not only on the first one (tests/test_checker_failing_states.py).
    // Sums of integer-valued floats are exact in any order WHILE THEY STAY BELOW 2^24 (so are sums of a few halves and
    // quarters): a body sum reaches 2^24 only for a snake of more than 5 792 cells (S = 64 has 4 096), so for every snake a
    // grid of the supported sizes can hold the lane-then-butterfly order here and torch's .sum() agree bit for bit; with
    // hand-made non-dyadic values the two orders may round differently, and so may the verdict.
    int bad_food = 0;
    float hs = 0.0f, bs = 0.0f, bm = -INFINITY, hb = 0.0f, hf = 0.0f, fs = 0.0f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        int c = g.lane + 64 * k;
        if ((g.valid >> k) & 1) {
            float f = envp[c], h = envp[g.C + c], b = envp[2 * g.C + c];
            bad_food |= !(f == 0.0f || f == 1.0f);
            hs += h; bs += b; hb += h * b; hf += h * f; fs += f;
            bm = fmaxf(bm, b);
        }
    }
    bad_food = ballot(bad_food != 0) != 0;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        hs += __shfl_xor(hs, sh); bs += __shfl_xor(bs, sh); hb += __shfl_xor(hb, sh); hf += __shfl_xor(hf, sh);
        fs += __shfl_xor(fs, sh); bm = fmaxf(bm, __shfl_xor(bm, sh));
    }
    uint32_t m = 0;
    if (bad_food) m |= WURM_CHK_FOOD_VALUE;
    if (hs != 1.0f) m |= WURM_CHK_ONE_HEAD;
    if (!(bs > 0.0f)) m |= WURM_CHK_HAS_SNAKE;
    if (bm != hb) m |= WURM_CHK_HEAD_AT_END;
    if ((__fsqrt_rn(8.0f * bs + 1.0f) - 1.0f) / 2.0f != bm) m |= WURM_CHK_BODY_RANGE; // bs is the bm-th triangular number
    if (!(bs >= 6.0f)) m |= WURM_CHK_MIN_LENGTH;
    if (hf != 0.0f) m |= WURM_CHK_HEAD_ON_FOOD;
    if (fs != 1.0f) m |= WURM_CHK_ONE_FOOD;
    if (g.lane == 0) err[env] = m;
}

// wurm.utils.determine_orientations over a (n,3,S,S) batch
template <int CPL>
__global__ __launch_bounds__(256) void orientations_kernel(const float *__restrict__ envs, long long *__restrict__ out,
                                                           long long N, int S, int lds_per_wave)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= N) return;
    signed char *lds = wurm_lds + wave * lds_per_wave;
    const Geo g = make_geo<CPL>(S);
    Env<CPL> e;
    load_state<CPL, true>(envs + env * 3 * g.C, g, e);
    int lm = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) lm = max(lm, e.body[k]);
    const int L = uniform(wave_max_i32(lm));
    const int o = orientation_of<CPL>(e, g, L, lds);
    if (g.lane == 0) out[env] = o;
}

} // namespace wurm
