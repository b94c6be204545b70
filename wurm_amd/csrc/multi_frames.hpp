// multi_frames.hpp — replay of a MultiSnake window for the few envs somebody wants to watch (include/wurm_hip.h:
// wurm_multi_rollout_frames).  The multi-agent twin of rollout_frames.hpp.
//
// `MultiSnake.act_window` runs its T iterations of act / step / reset inside the library, `MultiSnake.rollout` keeps the envs
// in LDS for a whole launch: neither shows the states in between, and neither is touched for the sake of a video.  But the
// window of one env is a pure function of its start state, its global id (env_offset + index), the seed, the configuration
// block, the call counter the window consumed (step t uses c + 2 t, its reset c + 2 t + 1) and the actions AS SAMPLED — `act`
// draws from another counter, and the step sanitises its actions itself.  So ONE WAVE PER SELECTED ENV re-runs the loop body
// of multi_rollout_kernel — multi_step_body, reroll_colour, multi_reset_grid, unchanged — on a gathered copy of the start
// state, and writes the image `_get_env_images()` would have shown in front of every step.  Where the DATA of env j lies
// (index j of the gathered tensors) and what keys its Philox draws (env_offset + select[j]) are two arguments of those
// functions already.  Nothing here is on a training path: the cost is paid only by the caller who asks for frames.
#pragma once

#include "multi_step.hpp"

namespace wurm {

struct MultiFrameArgs {
    // The replayed launch as multi_rollout_kernel would see it: foods / heads / bodies / dones / orientations / colours /
    // boost_state = the GATHERED start state (k envs, read only), actions = the window's (T, K, N) tape, N = the object's
    // envs, K, S, T, cfg, seed, call, env_offset; no observation, no tapes of injected outcomes, no status counter.
    MultiArgs m;
    const long long *select;  // (k) env indices within the object
    long long k;              // number of selected envs
    short *frames;            // (T + 1, k, 3, S, S)
    float *fin_foods, *fin_heads, *fin_bodies; // (k, 1, S, S), (k K, 1, S, S) twice
    uint8_t *fin_dones;       // (k K)
    long long *fin_orient;    // (k K)
    short *fin_colours;       // (k K, 3)
    uint8_t *fin_boost;       // (k K)
    uint8_t *status;          // (k) 0 = replayed, 1 = select[j] outside [0, N): frames and final state are zeros
};

// `_get_env_images()` of the env in LDS (multi_snake.py:617-628 here, :194-227 in the reference), the very operations in the
// very order, so that the bits agree and not just the picture:
//   inten = body.gt(EPS) * 1 / 3 + head.gt(EPS) * 1 / 3     torch divides by a scalar as a product with its fp32 reciprocal:
//                                                            1 * (1.0f / 3.0f) either way
//   inten *= 1 + 0.5 * boost;   img = sum over snakes, k = 0 .. K - 1, of inten * colour, in fp32;   .short() truncates
//   img[0] += 255 * food (int16);   a pixel that is 0 in all three channels becomes 255;   the border ring is 0
// Each product and sum is a rounding of its own (__fmul_rn / __fadd_rn: never contracted into an fma).  A snake that is not on
// the cell adds +0, which changes no bit, so the order of the sum only shows where two snakes share a cell — in a state the
// dynamics do not produce; there it is this one.  o: the frame's three (S, S) planes.  Reads cx.hcell (the step and the reset
// leave the head cells there), writes cx.colf.
__device__ __forceinline__ void write_env_image(const Ctx &cx, const Snake &sn, short *__restrict__ o)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    if (lane < K) {
        cx.colf[lane * 4 + 0] = (float)sn.col[0];
        cx.colf[lane * 4 + 1] = (float)sn.col[1];
        cx.colf[lane * 4 + 2] = (float)sn.col[2];
        cx.colf[lane * 4 + 3] = __fadd_rn(1.0f, __fmul_rn(0.5f, sn.boosted ? 1.0f : 0.0f));
    }
    wave_lds_sync();
    const float third = 1.0f / 3.0f;
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = lane + 64 * k;
        if (c >= C) continue;
        const int y = div_size(c, cx.rcpS), x = c - y * S;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int s = 0; s < K; ++s) {
            const bool isb = (int)(cx.body[s * C + c] & VMASK) > cx.tclk[s], ish = cx.hcell[s] == c;
            if (isb || ish) {
                const float *cf = cx.colf + 4 * s; // (12 K bytes into the env's LDS: 16-byte aligned only for some K)
                const float inten = __fmul_rn(__fadd_rn(isb ? third : 0.0f, ish ? third : 0.0f), cf[3]);
                a0 = __fadd_rn(a0, __fmul_rn(inten, cf[0]));
                a1 = __fadd_rn(a1, __fmul_rn(inten, cf[1]));
                a2 = __fadd_rn(a2, __fmul_rn(inten, cf[2]));
            }
        }
        short r = (short)(int)a0, g = (short)(int)a1, b = (short)(int)a2;
        if (cx.food[c] != 0) r = (short)(r + 255);
        if (r == 0 && g == 0 && b == 0) r = g = b = 255;
        if (y == 0 || x == 0 || y == S - 1 || x == S - 1) r = g = b = 0;
        o[c] = r;
        o[C + c] = g;
        o[2 * C + c] = b;
    }
    wave_lds_sync();
}

// One wave per workgroup, one workgroup per selected env: a handful of envs, spread over the CUs, each with the LDS of an env
// to itself (10 snakes on 36 x 36: 33 KB; the launch opts into more than 64 KB where an env needs it, as multi_launch does).
__global__ __launch_bounds__(64) void multi_rollout_frames_kernel(MultiFrameArgs f)
{
    const long long j = (long long)blockIdx.x;
    if (j >= f.k) return;
    // (the instantiation multi_rollout_kernel<false, false, WURM_OBS_NONE> starts from: the launch draws its own outcomes)
    const MultiArgs p = kernel_args<false, WURM_OBS_NONE, 0, 0, -1>(f.m, false);
    const Ctx cx = make_ctx(p, 0, 0, true);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const long long KC = (long long)K * C, frame_stride = f.k * 3 * C;
    short *fr = f.frames + j * 3 * C;
    float *fin_food = f.fin_foods + j * C, *fin_head = f.fin_heads + j * KC, *fin_body = f.fin_bodies + j * KC;
    const long long agent = j * K + lane; // in the gathered tensors and in the final state
    const bool snake = lane < K;
    const long long sel = uniform64(f.select[j]);
    if (sel < 0 || sel >= p.N) { // nothing of this env is read: no start state, no action column, no RNG stream
        if (lane == 0) f.status[j] = 1;
        for (long long t = 0; t <= p.T; ++t, fr += frame_stride)
            for (int c = lane; c < 3 * C; c += 64) fr[c] = 0;
        for (int c = lane; c < C; c += 64) fin_food[c] = 0.0f;
        for (long long i = lane; i < KC; i += 64) {
            fin_head[i] = 0.0f;
            fin_body[i] = 0.0f;
        }
        if (snake) {
            f.fin_dones[agent] = 0;
            f.fin_orient[agent] = 0;
            f.fin_boost[agent] = 0;
            f.fin_colours[agent * 3] = f.fin_colours[agent * 3 + 1] = f.fin_colours[agent * 3 + 2] = 0;
        }
        return;
    }
    if (lane == 0) f.status[j] = 0;
    const u64 env_id = (u64)(p.env_offset + sel);
    const long long KN = (long long)K * p.N;

    (void)load_env(cx, p.foods + j * C, p.heads + j * KC, p.bodies + j * KC);
    Snake sn;
    sn.hc = snake ? cx.hcell[lane] : -1;
    sn.L = snake ? cx.lmax[lane] : 0;
    sn.done = snake ? p.dones[agent] != 0 : true;
    sn.orient = snake ? p.orientations[agent] : 0;
    sn.boosted = snake ? p.boost_state[agent] != 0 : false;
    load_colour(p, agent, snake, sn);
    WURM_TLS_INIT(cx);

    for (long long t = 0; t < p.T; ++t, fr += frame_stride) {
        const u64 call = p.call + 2ull * (u64)t;
        // the tape in 64-step chunks through LDS, kept per action as multi_rollout_kernel keeps it: a % 4 (C semantics) and a > 3
        if ((t & 63) == 0) {
            const int nt = (int)min((long long)64, p.T - t);
            wave_lds_sync();
            for (int i = lane; i < nt * K; i += 64) {
                const int q = i / K, sidx = i - q * K;
                const long long av = p.actions[(t + q) * KN + (long long)sidx * p.N + sel];
                cx.acts[i] = (unsigned char)(((int)(av % 4) + 4) | (av > 3 ? 8 : 0));
            }
            wave_lds_sync();
        }
        long long a = 0;
        if (snake) {
            const int b = cx.acts[(int)(t & 63) * K + lane];
            const int d4 = (b & 7) - 4;
            a = (b & 8) ? 4 + d4 : d4;
        }
        write_env_image(cx, sn, fr); // the env as step t finds it
        StepRes r;
        multi_step_body(cx, p, j, env_id, call, a, sn, r, 0, 0, 0);
        rebase_clocks(cx);

        // reset(dones['__all__']) (:771-836), as multi_rollout_kernel applies it
        if (snake && sn.done) sn.L = 0;
        const bool rebuild = r.all_done;
        if (rebuild) sn.done = false;
        if (snake) (void)reroll_colour(p, agent, sn.done, env_id, call + 1ull, 0, sn);
        const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
        if (rebuild || respawn) {
            bool orient_dirty = false;
            multi_reset_grid(cx, p, j, env_id, call + 1ull, rebuild, respawn, sn, orient_dirty, 0, 0);
        }
    }
    write_env_image(cx, sn, fr); // frame T: what the window leaves behind

    if (snake) {
        f.fin_dones[agent] = (uint8_t)sn.done;
        f.fin_orient[agent] = sn.orient;
        f.fin_boost[agent] = (uint8_t)sn.boosted;
        f.fin_colours[agent * 3] = sn.col[0];
        f.fin_colours[agent * 3 + 1] = sn.col[1];
        f.fin_colours[agent * 3 + 2] = sn.col[2];
        cx.hcell[lane] = sn.hc;
    }
    wave_lds_sync();
    store_env(cx, fin_food, fin_head, fin_body, 0, -1, sn.hc, true); // every cell: the final tensors are this kernel's own
}

} // namespace wurm
