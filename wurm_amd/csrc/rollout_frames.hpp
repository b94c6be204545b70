// rollout_frames.hpp — replay of a fused window for the few envs somebody wants to watch (include/wurm_hip.h:
// wurm_single_rollout_frames, wurm_grid_rollout_frames).
//
// A fused window (rollout, policy_rollout) never materialises the states between its T steps, and its kernels are not
// touched for the sake of a video.  But the window of one env is a pure function of its start state, its global id
// (env_offset + index), the seed and call counter the launch consumed and the sanitised actions the launch returned —
// so ONE WAVE PER SELECTED ENV re-runs it after the fact from a saved copy of the start planes, with the very transition,
// reset and colour code of single_device.hpp (step_core, reset_core, cell_class / class_rgb), and writes what
// `_get_rgb()` would have shown in front of every step.  Nothing here is on a training path: the cost is paid only by
// the caller who asks for frames.
#pragma once

#include "single_device.hpp"

namespace wurm {

struct FrameArgs {
    const float *start;       // (K, NCH, S, S) planes of the selected envs before the window
    const long long *select;  // (K) env indices within the object
    const long long *actions; // (T, N) sanitised actions as the window returned them
    uint8_t *frames;          // (T + 1, K, 3, S, S)
    float *final_state;       // (K, NCH, S, S)
    uint8_t *status;          // (K) 0 = replayed, 1 = select[j] outside [0, N): frames and final state are zeros
    long long K, N, T;
    int S, start_y, start_x;
    u64 seed, call;           // call: the window's first counter (step t uses call + 2t, its reset call + 2t + 1)
    long long env_offset;
    int lds_per_wave;
};

// `(_observe('default') * 255).round()` of one env from registers (single_snake.py:104-128, simple_gridworld.py:88-109)
template <int CPL, bool SNAKE>
__device__ __forceinline__ void write_frame(const Env<CPL> &e, const Geo &g, uint8_t *__restrict__ o)
{
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = g.lane + 64 * k;
        if ((g.valid >> k) & 1) {
            const int cls = cell_class<CPL, SNAKE>(e, g, k);
            o[c] = (uint8_t)__float2int_rn(class_rgb(cls, 0, SNAKE) * 255.0f);
            o[g.C + c] = (uint8_t)__float2int_rn(class_rgb(cls, 1, SNAKE) * 255.0f);
            o[2 * g.C + c] = (uint8_t)__float2int_rn(class_rgb(cls, 2, SNAKE) * 255.0f);
        }
    }
}

template <int CPL, bool SNAKE>
__global__ __launch_bounds__(64) void rollout_frames_kernel(FrameArgs p)
{
    const long long j = (long long)blockIdx.x; // one wave per workgroup: a handful of envs, spread over the CUs
    if (j >= p.K) return;
    constexpr int NCH = SNAKE ? 3 : 2;
    const Geo g = make_geo<CPL>(p.S);
    const long long frame_stride = p.K * 3 * g.C;
    uint8_t *fr = p.frames + j * 3 * g.C;
    float *fin = p.final_state + j * NCH * g.C;
    const long long sel = uniform64(p.select[j]);
    if (sel < 0 || sel >= p.N) { // nothing of this env is read: no action column, no RNG stream
        if (g.lane == 0) p.status[j] = 1;
        for (long long t = 0; t <= p.T; ++t, fr += frame_stride)
            for (int c = g.lane; c < 3 * g.C; c += 64) fr[c] = 0;
        for (int c = g.lane; c < NCH * g.C; c += 64) fin[c] = 0.0f;
        return;
    }
    if (g.lane == 0) p.status[j] = 0;
    signed char *lds = wurm_lds;
    const u64 env_id = (u64)(p.env_offset + sel);
    Env<CPL> e;
    load_state<CPL, SNAKE>(p.start + j * NCH * g.C, g, e);
    u64 call = p.call;
    for (long long t0 = 0; t0 < p.T; t0 += 64) {
        const int nt = (int)min((long long)64, p.T - t0);
        // lane i holds the action of step t0 + i (as rollout_generic prefetches its tape)
        long long my_a = g.lane < nt ? p.actions[(t0 + g.lane) * p.N + sel] : 0;
        // The tape holds SANITISED actions: the move the env made.  step_core would sanitise again, and for an action that
        // left the sanitiser as the orientation itself (4 + o on the way in) that is another move — so the replay hands it
        // the same move as an action no orientation equals: (a mod 4) + 4.
        my_a = (((my_a % 4) + 4) % 4) + 4;
        for (int i = 0; i < nt; ++i, fr += frame_stride, call += 2) {
            write_frame<CPL, SNAKE>(e, g, fr); // the env as step t0 + i finds it
            StepOut out;
            step_core<CPL, SNAKE, false>(e, g, nullptr, lane_value64(my_a, i), out, p.seed, call, env_id, false, -1, lds);
            if (out.done) reset_core<CPL, SNAKE>(e, g, p.seed, call + 1ull, env_id, nullptr, p.start_y, p.start_x);
        }
    }
    write_frame<CPL, SNAKE>(e, g, fr); // frame T: what the window leaves behind
    store_state<CPL, SNAKE>(fin, g, e);
}

} // namespace wurm
