// single_launch.hpp — the host side of the SingleSnake / SimpleGridworld dispatch: which kernel serves a call (route_of)
// and its launch.  launch<SNAKE> is instantiated once per environment, each in a translation unit of its own
// (single_snake.hip: launch<true>, single_grid.hip: launch<false>).
#pragma once

#include "single_kernels.hpp"
#include "lane_step.hpp"

namespace wurm {

enum Kind { K_STEP, K_RESET, K_OBSERVE, K_ROLLOUT, K_FUSED };

// ---- which kernel serves a call.  ONE table (route_of), read top to bottom: the first row whose condition holds wins.
//   kind             | condition                                                                    | route
//   step / fused     | snake, S >= 12, grid_step_eligible, (N S^2 >= grid_step_min_cells or a mirror) | R_GRID_STEP   grid_rollout.hip (+ generic for the rest)
//   step / fused     | snake, S <= 11, N >= lane_step_min_envs, lane_step_eligible                    | R_LANE_STEP   lane_step.hpp
//   step/reset/observe/fused | otherwise                                                              | R_GENERIC     one env per wave
//   rollout          | snake, S >= 12, grid_rollout_eligible                                          | R_GRID_ROLLOUT
//   rollout          | snake, S <= 11, N >= lane_rollout_min_envs, lane_rollout_eligible              | R_LANE_ROLLOUT lane_rollout.hpp (9 x 9)
//   rollout          | snake, S = 10 / 11, N >= lane_rollout_min_envs, lane_wide_eligible              | R_LANE_WIDE   lane_wide.hpp (default, one_channel, partial_2 / 3, positions, none)
//   rollout          | snake, S == 9, both inject arrays, partial_n (n <= 3) or none                  | R_S9_INJ      rollout_s9_kernel<., true>
//   rollout          | snake, S == 9, RNG mode, partial_n (n <= 3) or none                            | R_S9          rollout_s9_kernel
//                    |   (both rows: N <= s9_pair_max_envs launches the kernel's pair form, two waves per env; with partial_n
//                    |    and T >= s9_crop_helper_min_steps the form of it whose helper wave renders the crops)
//   rollout          | snake, S = 10 / 11, RNG mode, partial_n (n <= 3) or none                       | R_LEAN        rollout_lean_kernel
//   rollout          | snake, S <= 11, RNG mode, partial_n (n <= 6) / none                            | R_GENERIC_PARTIAL / R_GENERIC_NONE (mode as template argument)
//   rollout          | gridworld, RNG mode, N >= lane_rollout_min_envs, gridworld_lane_eligible        | R_GRIDWORLD_LANE gridworld_lane.hip (+ generic for the rest)
//   step / fused     | gridworld, RNG mode, no immediate reset, N >= lane_step_min_envs                | R_GRIDWORLD_LANE_STEP gridworld_lane.hip (+ generic for the rest)
//   rollout          | otherwise                                                                      | R_GENERIC
// (the resident 9 x 9 step, lane_resident.hpp, is chosen by fused_entry: it needs the caller's mirror)
enum Route { R_GENERIC, R_GRID_STEP, R_LANE_STEP, R_GRID_ROLLOUT, R_LANE_ROLLOUT, R_LANE_WIDE, R_S9_INJ, R_S9, R_LEAN, R_GENERIC_PARTIAL, R_GENERIC_NONE, R_LANE_RESIDENT, R_LANE_WIDE_RESIDENT, R_GRIDWORLD_LANE, R_GRIDWORLD_LANE_STEP };
// (wurm_single_last_route: the route of the CALLING THREAD's last launch — a diagnostic the tests and bench.py name a launch by; no
// state that a later call depends on.  Defined in single_snake.hip.)
extern thread_local Route last_route;
// (wurm_single_last_waves_per_env: 2 if that launch was rollout_s9_kernel's pair form, 3 if its trio form, else 1)
extern thread_local int last_waves_per_env;
// (wurm_single_last_crop_wave: 1 if that launch was the pair form whose helper wave renders the crops, else 0)
extern thread_local int last_crop_wave;

static const char *route_name(Route r)
{
    switch (r) {
    case R_GRID_STEP: return "grid_step";
    case R_LANE_STEP: return "lane_step";
    case R_GRID_ROLLOUT: return "grid_rollout";
    case R_LANE_ROLLOUT: return "lane_rollout";
    case R_LANE_WIDE: return "lane_wide";
    case R_S9_INJ: return "rollout_s9_injected";
    case R_S9: return "rollout_s9";
    case R_LEAN: return "rollout_lean";
    case R_GENERIC_PARTIAL: return "rollout_generic_partial";
    case R_GENERIC_NONE: return "rollout_generic_none";
    case R_LANE_RESIDENT: return "lane_resident";
    case R_LANE_WIDE_RESIDENT: return "lane_wide_resident";
    case R_GRIDWORLD_LANE: return "gridworld_lane";
    case R_GRIDWORLD_LANE_STEP: return "gridworld_lane_step";
    default: return "generic";
    }
}

static Route route_of(Kind kind, bool snake, int cpl, const StepArgs &p)
{
    const bool stepish = kind == K_STEP || kind == K_FUSED;
    if (snake && cpl >= 4 && stepish && grid_step_eligible(p) &&
        (p.N * (long long)p.S * p.S >= opt.grid_step_min_cells || p.resident != nullptr)) return R_GRID_STEP;
    if (snake && cpl == 2 && stepish && p.N >= opt.lane_step_min_envs && lane_step_eligible(p)) return R_LANE_STEP;
    if (kind == K_ROLLOUT && !snake && gridworld_lane_eligible(p)) return R_GRIDWORLD_LANE;
    if (stepish && !snake && gridworld_lane_step_eligible(p)) return R_GRIDWORLD_LANE_STEP;
    if (kind != K_ROLLOUT || !snake) return R_GENERIC;
    if (cpl >= 4) return grid_rollout_eligible(p) ? R_GRID_ROLLOUT : R_GENERIC;
    if (p.N >= opt.lane_rollout_min_envs && lane_rollout_eligible(p)) return R_LANE_ROLLOUT;
    if (p.N >= opt.lane_rollout_min_envs && lane_wide_eligible(p)) return R_LANE_WIDE;
    const bool rng_mode = p.inject_food == nullptr && p.inject_reset == nullptr;
    const bool injected = p.inject_food != nullptr && p.inject_reset != nullptr;
    const bool small_crop_or_none = (p.obs_mode == WURM_OBS_PARTIAL && p.obs_n <= 3) || p.obs_mode == WURM_OBS_NONE;
    if (injected && p.S == 9 && small_crop_or_none) return R_S9_INJ;
    if (rng_mode && p.S == 9 && small_crop_or_none) return R_S9;
    if (rng_mode && p.S > 9 && small_crop_or_none) return R_LEAN;
    if (rng_mode && p.obs_mode == WURM_OBS_PARTIAL && p.obs_n <= 6) return R_GENERIC_PARTIAL;
    if (rng_mode && p.obs_mode == WURM_OBS_NONE) return R_GENERIC_NONE;
    return R_GENERIC;
}

template <int CPL, bool SNAKE>
static hipError_t launch_one(Kind kind, const StepArgs &p, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    (void)hipGetLastError(); // drop any stale error left by earlier runtime calls of this thread
    const Route route = route_of(kind, SNAKE, CPL, p);
    last_route = route;
    last_waves_per_env = 1;
    last_crop_wave = 0;
    // (the one-env-per-wave code behind a grid / lane kernel, for the envs that one could not take: flagged_kernel, a wave per 64 envs)
    const unsigned wpb_f = block.x / 64u;
    const dim3 fgrid((unsigned)((p.N + 64ll * wpb_f - 1) / (64ll * wpb_f)));
    switch (route) {
    case R_GRID_STEP:
        if constexpr (SNAKE && CPL >= 4) {
            hipError_t err = launch_grid_step(p, st);
            if (err != hipSuccess) return err;
            WURM_LAUNCH((flagged_kernel<CPL, SNAKE, false>), fgrid, block, lds, st, p);
        }
        break;
    case R_LANE_STEP:
        if constexpr (SNAKE && CPL == 2) return launch_lane_step(p, st);
        break;
    case R_GRID_ROLLOUT:
        if constexpr (SNAKE && CPL >= 4) {
            hipError_t err = launch_grid_rollout(p, st);
            if (err != hipSuccess) return err;
            WURM_LAUNCH((flagged_kernel<CPL, SNAKE, true>), fgrid, block, lds, st, p);
        }
        break;
    case R_LANE_ROLLOUT:
        if constexpr (SNAKE && CPL == 2) return launch_lane_rollout(p, st);
        break;
    case R_LANE_WIDE:
        if constexpr (SNAKE && CPL == 2) return launch_lane_wide(p, st);
        break;
    case R_GRIDWORLD_LANE:
        if constexpr (!SNAKE) {
            hipError_t err = launch_gridworld_lane_rollout(p, st);
            if (err != hipSuccess) return err;
            if (!(p.resident != nullptr && p.resident_valid)) // (a mirror that was current describes every env: see R_GRIDWORLD_LANE_STEP)
                WURM_LAUNCH((flagged_kernel<CPL, SNAKE, true>), fgrid, block, lds, st, p); // (the envs outside the lane kernel's domain)
        }
        break;
    case R_GRIDWORLD_LANE_STEP:
        if constexpr (!SNAKE) {
            hipError_t err = launch_gridworld_lane_step(p, st);
            if (err != hipSuccess) return err;
            // (a mirror that was current describes every env — the library reports a mirror valid only if the launch that
            // built it found nothing outside the lane kernel's domain, and that domain is closed under the library's own
            // launches — so nothing can be flagged: ONE launch per call)
            if (!(p.resident != nullptr && p.resident_valid))
                WURM_LAUNCH((flagged_kernel<CPL, SNAKE, false>), fgrid, block, lds, st, p);
        }
        break;
    case R_S9_INJ:
    case R_S9:
        if constexpr (SNAKE && CPL == 2) {
            const bool inj = route == R_S9_INJ, none = p.obs_mode == WURM_OBS_NONE;
            if (p.N <= opt.s9_pair_max_envs) {
                // the pair form: a workgroup of two waves per env, stepper and helper, and the helper's buffers behind
                // the stepper's lds_per_wave bytes (single_kernels.hpp: 2 chunk buffers of 5 x 64 dwords, 2 record
                // buffers of 64, the verdict)
                const dim3 pgrid((unsigned)p.N), pblock(128);
                const size_t plds = (size_t)p.lds_per_wave + (2 * 5 * 64 + 2 * 64 + 4) * sizeof(int);
                last_waves_per_env = 2;
                // The helper renders the crops too where the launch is long enough for that to pay (the last chunk is
                // rendered after the stepper has finished): record buffers of 4 x 64 dwords.  (Its lanes address the second
                // step of a pass by a 32-bit byte offset of one step's observations.)
                if (!none && opt.s9_crop_helper_min_steps >= 0 && p.T >= opt.s9_crop_helper_min_steps &&
                    p.N * p.obs_elems * 4 < (1ll << 31)) {
                    const size_t clds = (size_t)p.lds_per_wave + (2 * 5 * 64 + 2 * 4 * 64 + 4) * sizeof(int);
                    last_crop_wave = 1;
                    // The trio form: a second render wave (wave 2) takes most of each chunk's crops off the helper, in small
                    // batches — the machine has room for a third wave per env there — and launches of several chunks.  Same
                    // barriers, three waves at each: 192 threads per env.  Its render waves rebuild the head codes, food codes
                    // and body masks the stepper no longer records: record buffers of 5 x 64 + 4 dwords (the chunk-start
                    // clocks, two planes of reset words, the chunk-start codes and length) and three planes for each render
                    // wave (rebuilt crop words, the two halves of the rebuilt body masks), behind the verdict.
                    if (p.N <= opt.s9_trio_max_envs && opt.s9_trio_min_steps >= 0 && p.T >= opt.s9_trio_min_steps) {
                        const dim3 tblock(192);
                        const size_t tlds = (size_t)p.lds_per_wave + (2 * 5 * 64 + 2 * (5 * 64 + 4) + 4 + 2 * 3 * 64) * sizeof(int);
                        last_waves_per_env = 3;
                        if (inj) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, true, true, true, 2>), pgrid, tblock, tlds, st, p);
                        else WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, false, true, true, 2>), pgrid, tblock, tlds, st, p);
                    } else
                    if (inj) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, true, true, true>), pgrid, pblock, clds, st, p);
                    else WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, false, true, true>), pgrid, pblock, clds, st, p);
                } else
                if (inj && none) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_NONE, true, true>), pgrid, pblock, plds, st, p);
                else if (inj) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, true, true>), pgrid, pblock, plds, st, p);
                else if (none) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_NONE, false, true>), pgrid, pblock, plds, st, p);
                else WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, false, true>), pgrid, pblock, plds, st, p);
            } else if (inj) {
                if (none) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_NONE, true>), grid, block, lds, st, p);
                else WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL, true>), grid, block, lds, st, p);
            } else {
                if (none) WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_NONE>), grid, block, lds, st, p);
                else WURM_LAUNCH((rollout_s9_kernel<WURM_OBS_PARTIAL>), grid, block, lds, st, p);
            }
        }
        break;
    case R_LEAN:
        if constexpr (SNAKE && CPL == 2) {
            if (p.obs_mode == WURM_OBS_NONE) WURM_LAUNCH((rollout_lean_kernel<WURM_OBS_NONE, false>), grid, block, lds, st, p);
            else WURM_LAUNCH((rollout_lean_kernel<WURM_OBS_PARTIAL, false>), grid, block, lds, st, p);
        }
        break;
    case R_GENERIC_PARTIAL:
        if constexpr (SNAKE && CPL == 2) WURM_LAUNCH((rollout_kernel<CPL, SNAKE, WURM_OBS_PARTIAL, false>), grid, block, lds, st, p);
        break;
    case R_GENERIC_NONE:
        if constexpr (SNAKE && CPL == 2) WURM_LAUNCH((rollout_kernel<CPL, SNAKE, WURM_OBS_NONE, false>), grid, block, lds, st, p);
        break;
    case R_LANE_RESIDENT: // (chosen by fused_entry, which launches it itself)
    case R_LANE_WIDE_RESIDENT:
    case R_GENERIC:
        switch (kind) {
        case K_STEP: WURM_LAUNCH((step_kernel<CPL, SNAKE>), grid, block, lds, st, p); break;
        case K_RESET: WURM_LAUNCH((reset_kernel<CPL, SNAKE>), grid, block, lds, st, p); break;
        case K_OBSERVE: WURM_LAUNCH((observe_kernel<CPL, SNAKE>), grid, block, lds, st, p); break;
        case K_FUSED: WURM_LAUNCH((fused_step_kernel<CPL, SNAKE>), grid, block, lds, st, p); break;
        case K_ROLLOUT: WURM_LAUNCH((rollout_kernel<CPL, SNAKE>), grid, block, lds, st, p); break;
        }
        break;
    }
    return hipGetLastError();
}

// Instantiated in TWO translation units, one per environment, so that the build compiles the two halves of the kernels
// side by side (as one unit this was the build's longest, 4.7 of its 6 minutes).
template <bool SNAKE>
int launch(Kind kind, StepArgs p, void *stream)
{
    if (p.N == 0) return WURM_OK;
    const int cpl = pick_cpl(p.S);
    if (cpl < 0) return WURM_ERR_UNSUPPORTED;
    // small batches: one wave per workgroup so the envs spread over all 256 CUs; large: 4 waves per workgroup
    const int wpb = p.N <= 4096 ? 1 : 4;
    p.lds_per_wave = ((p.S * p.S + 15) / 16) * 16;
    dim3 block(64 * wpb), grid((unsigned)((p.N + wpb - 1) / wpb));
    size_t lds = (size_t)p.lds_per_wave * wpb;
    hipStream_t st = (hipStream_t)stream;
    hipError_t err;
    switch (cpl) {
    case 2: err = launch_one<2, SNAKE>(kind, p, grid, block, lds, st); break;
    case 4: err = launch_one<4, SNAKE>(kind, p, grid, block, lds, st); break;
    case 8: err = launch_one<8, SNAKE>(kind, p, grid, block, lds, st); break;
    case 16: err = launch_one<16, SNAKE>(kind, p, grid, block, lds, st); break;
    case 24: err = launch_one<24, SNAKE>(kind, p, grid, block, lds, st); break;
    case 32: err = launch_one<32, SNAKE>(kind, p, grid, block, lds, st); break;
    case 48: err = launch_one<48, SNAKE>(kind, p, grid, block, lds, st); break;
    default: err = launch_one<64, SNAKE>(kind, p, grid, block, lds, st); break;
    }
    return err == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // namespace wurm
