// lane_launch.hpp — the one launch of the one-env-per-LANE kernels (host side; lane_step.hpp, lane_rollout.hpp, lane_resident.hpp,
// lane_wide.hpp, lane_wide_resident.hpp, gridworld_lane.hip): a wave owns epw consecutive envs, a workgroup one wave or — from
// wide_from_waves waves on — four, and its dynamic LDS is the workgroup's tables plus wave_bytes per wave.
#pragma once

#include <hip/hip_runtime.h>

#include "options.hpp"

namespace wurm {

// wide_from_waves: 2048 for the rollouts, 1024 for the per-call kernels; 0: always four waves.  static_bytes: the kernel's
// static LDS.  Past the 64 KB a launch gets by default the kernel is opted into the larger budget ('raw' at four waves per
// workgroup: 80 KB).  Errors are the caller's to collect (hipGetLastError).
template <typename Kernel, typename Args>
static void lane_launch(Kernel kernel, const Args &args, long long N, int epw, long long wide_from_waves, size_t table_bytes,
                        size_t wave_bytes, hipStream_t stream, size_t static_bytes = 0)
{
    const long long waves = (N + epw - 1) / epw;
    const int wpb = waves >= wide_from_waves ? 4 : 1;
    const dim3 block(64 * wpb), grid((unsigned)((waves + wpb - 1) / wpb));
    const size_t lds_bytes = table_bytes + wave_bytes * wpb;
    if (lds_bytes + static_bytes > 65536)
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    WURM_LAUNCH(kernel, grid, block, lds_bytes, stream, args);
}

} // namespace wurm
