// rollout_frames.hip — C ABI of the frame replay of a fused window (kernel: rollout_frames.hpp; include/wurm_hip.h:
// wurm_single_rollout_frames, wurm_grid_rollout_frames).  Arguments are validated before the first HIP call, so refusals
// work with no device present.
#include "rollout_frames.hpp"

using namespace wurm;

namespace {

template <bool SNAKE>
int launch_frames(FrameArgs p, void *stream)
{
    const int cpl = pick_cpl(p.S);
    if (cpl < 0) return WURM_ERR_UNSUPPORTED;
    p.lds_per_wave = ((p.S * p.S + 15) / 16) * 16; // the class / neck map of single_device.hpp: one byte per cell
    const dim3 grid((unsigned)p.K), block(64);
    const size_t lds = (size_t)p.lds_per_wave;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    switch (cpl) {
    case 2: WURM_LAUNCH((rollout_frames_kernel<2, SNAKE>), grid, block, lds, st, p); break;
    case 4: WURM_LAUNCH((rollout_frames_kernel<4, SNAKE>), grid, block, lds, st, p); break;
    case 8: WURM_LAUNCH((rollout_frames_kernel<8, SNAKE>), grid, block, lds, st, p); break;
    case 16: WURM_LAUNCH((rollout_frames_kernel<16, SNAKE>), grid, block, lds, st, p); break;
    case 24: WURM_LAUNCH((rollout_frames_kernel<24, SNAKE>), grid, block, lds, st, p); break;
    case 32: WURM_LAUNCH((rollout_frames_kernel<32, SNAKE>), grid, block, lds, st, p); break;
    case 48: WURM_LAUNCH((rollout_frames_kernel<48, SNAKE>), grid, block, lds, st, p); break;
    default: WURM_LAUNCH((rollout_frames_kernel<64, SNAKE>), grid, block, lds, st, p); break;
    }
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int frames_entry(bool snake, const float *start, const int64_t *select, const int64_t *actions, uint8_t *frames,
                 float *final_state, uint8_t *status, int64_t num_select, int64_t num_envs, int size, int64_t num_steps,
                 int start_y, int start_x, uint64_t seed, uint64_t call0, int64_t env_offset, void *stream)
{
    if (!start || !select || !frames || !final_state || !status) return WURM_ERR_INVALID_ARG;
    if (num_select <= 0 || num_steps < 0 || num_envs <= 0 || size < 3) return WURM_ERR_INVALID_ARG;
    if (num_steps > 0 && !actions) return WURM_ERR_INVALID_ARG;
    if (size > 64 || size <= (snake ? 8 : 4)) return WURM_ERR_UNSUPPORTED; // single_snake.py:346-347, simple_gridworld.py:249-250
    if (!snake && (start_y < 0 || start_x < 0 || start_y >= size || start_x >= size)) return WURM_ERR_UNSUPPORTED;
    if (num_select > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED; // the selected env is the workgroup
    FrameArgs p = {};
    p.start = start; p.select = (const long long *)select; p.actions = (const long long *)actions;
    p.frames = frames; p.final_state = final_state; p.status = status;
    p.K = num_select; p.N = num_envs; p.T = num_steps; p.S = size; p.start_y = start_y; p.start_x = start_x;
    p.seed = seed; p.call = call0; p.env_offset = env_offset;
    return snake ? launch_frames<true>(p, stream) : launch_frames<false>(p, stream);
}

} // namespace

extern "C" {

int wurm_single_rollout_frames(const float *start, const int64_t *select, const int64_t *actions, uint8_t *frames,
                               float *final_state, uint8_t *status, int64_t num_select, int64_t num_envs, int size,
                               int64_t num_steps, uint64_t seed, uint64_t call0, int64_t env_offset, void *stream)
{
    return frames_entry(true, start, select, actions, frames, final_state, status, num_select, num_envs, size, num_steps, 0, 0,
                        seed, call0, env_offset, stream);
}

int wurm_grid_rollout_frames(const float *start, const int64_t *select, const int64_t *actions, uint8_t *frames,
                             float *final_state, uint8_t *status, int64_t num_select, int64_t num_envs, int size,
                             int64_t num_steps, int start_y, int start_x, uint64_t seed, uint64_t call0,
                             int64_t env_offset, void *stream)
{
    return frames_entry(false, start, select, actions, frames, final_state, status, num_select, num_envs, size, num_steps,
                        start_y, start_x, seed, call0, env_offset, stream);
}

} // extern "C"
