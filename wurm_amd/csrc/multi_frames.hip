// multi_frames.hip — C ABI of the frame replay of a MultiSnake window (kernel: multi_frames.hpp; include/wurm_hip.h:
// wurm_multi_rollout_frames).  Arguments are validated before the first HIP call, so refusals work with no device present.
#include <cstdint>

#include "multi_frames.hpp"
#include "options.hpp"

using namespace wurm;

namespace {

constexpr int FRAMES_LDS_MAX_BYTES = 160 * 1024; // per workgroup on CDNA4: what multi_launch allows an env too

bool aligned(const void *ptr, uintptr_t to) { return ((uintptr_t)ptr & (to - 1)) == 0; }

} // namespace

extern "C" {

int wurm_multi_rollout_frames(const float *foods, const float *heads, const float *bodies, const uint8_t *dones,
                              const int64_t *orientations, const int16_t *colours, const uint8_t *boost_this_step,
                              const int64_t *select, const int64_t *actions, int16_t *frames, float *final_foods,
                              float *final_heads, float *final_bodies, uint8_t *final_dones, int64_t *final_orientations,
                              int16_t *final_colours, uint8_t *final_boost, uint8_t *status, int64_t num_select,
                              int64_t num_envs, int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg,
                              uint64_t seed, uint64_t call0, int64_t env_offset, void *stream)
{
    if (!foods || !heads || !bodies || !dones || !orientations || !colours || !boost_this_step || !select || !frames ||
        !final_foods || !final_heads || !final_bodies || !final_dones || !final_orientations || !final_colours ||
        !final_boost || !status || !cfg)
        return WURM_ERR_INVALID_ARG;
    if (num_select <= 0 || num_steps < 0 || num_envs <= 0 || num_snakes < 1 || size < 3) return WURM_ERR_INVALID_ARG;
    if (num_steps > 0 && !actions) return WURM_ERR_INVALID_ARG;
    if (!aligned(foods, 4) || !aligned(heads, 4) || !aligned(bodies, 4) || !aligned(final_foods, 4) ||
        !aligned(final_heads, 4) || !aligned(final_bodies, 4) || !aligned(orientations, 8) ||
        !aligned(final_orientations, 8) || !aligned(select, 8) || !aligned(actions, 8) || !aligned(colours, 2) ||
        !aligned(final_colours, 2) || !aligned(frames, 2))
        return WURM_ERR_INVALID_ARG;
    // what wurm_multi_rollout serves: at most 64 snakes on 5 x 5 .. 64 x 64, an env whose grids fit the LDS of a CU
    if (num_snakes > 64 || size > 64 || size < 5) return WURM_ERR_UNSUPPORTED;
    if (num_select > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED; // the selected env is the workgroup
    MultiFrameArgs f = {};
    MultiArgs &p = f.m;
    p.foods = const_cast<float *>(foods); p.heads = const_cast<float *>(heads); p.bodies = const_cast<float *>(bodies);
    p.dones = const_cast<uint8_t *>(dones); p.orientations = (long long *)orientations; p.colours = (short *)colours;
    p.boost_state = const_cast<uint8_t *>(boost_this_step);
    p.actions = (const long long *)actions;
    p.obs_mode = WURM_OBS_NONE;
    p.N = num_envs; p.K = num_snakes; p.S = size; p.T = num_steps;
    p.cfg = *cfg; p.seed = seed; p.call = call0; p.env_offset = env_offset;
    const int lds = multi_layout(p, false, 0);
    if (lds > FRAMES_LDS_MAX_BYTES) return WURM_ERR_UNSUPPORTED;
    f.select = (const long long *)select; f.k = num_select; f.frames = frames;
    f.fin_foods = final_foods; f.fin_heads = final_heads; f.fin_bodies = final_bodies; f.fin_dones = final_dones;
    f.fin_orient = (long long *)final_orientations; f.fin_colours = final_colours; f.fin_boost = final_boost;
    f.status = status;
    (void)hipGetLastError();
    // dynamic LDS beyond the default 64 KB of a launch needs the kernel's opt-in
    if (lds > 65536 && hipFuncSetAttribute((const void *)multi_rollout_frames_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return WURM_ERR_HIP;
    WURM_LAUNCH(multi_rollout_frames_kernel, dim3((unsigned)num_select), dim3(64), (size_t)lds, (hipStream_t)stream, f);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
