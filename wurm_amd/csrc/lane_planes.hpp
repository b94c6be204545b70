// lane_planes.hpp — bit planes to floats, the observation writer shared by the one-env-per-LANE kernels of every grid size
// (lane_rollout.hpp / lane_resident.hpp: 9 x 9; lane_wide.hpp / lane_wide_resident.hpp: 10 x 10 and 11 x 11).
//
// A (step, env) pair lane ORs the planes of its observation into NPL interleaved flat bit strings in LDS (word w of plane k:
// bits[NPL w + k]; bit i of a string = float i of the wave's contiguous run of observations); every lane then turns aligned
// nibbles of the strings into four floats through a 256-entry table of float4 and stores 16 bytes.
//   two planes ('default', the crops): "value is 1", "value is 127/255";
//   four planes ('one_channel', single_snake.py:142-151): body without the head (0.5), head (1.0), food (1.5), ring (-1) — two
//       tables whose results are ADDED: the planes exclude each other, so one addend is always +0 and the sum is exact.
// What depends on the grid — how a state becomes planes (lr_grid_planes, lr_crop3_planes, lw_planes_of), and the wide ORs
// lr_or81 / lw_or128 — stays with the kernels.
#pragma once

#include "wurm_device.hpp"

namespace wurm {

constexpr int LANE_OBS_GRID1 = -2, LANE_OBS_GRID3 = -3; // OBSK of the lane kernels: 'one_channel' / 'default' through bit planes

template <int OBSK>
constexpr int lane_plane_count() { return OBSK == LANE_OBS_GRID1 ? 4 : 2; }

// tabA[low nibble: "value is 1", high nibble: "value is 127/255"]; for 'one_channel' tabA[low nibble: 0.5, high: 1.0],
// tabB[low nibble: 1.5, high: -1.0]
template <int OBSK>
__device__ __forceinline__ void lane_build_tables(float4 *tabA, float4 *tabB)
{
    for (int i = (int)threadIdx.x; i < 256; i += (int)blockDim.x) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool lo = ((i >> j) & 1) != 0, hi = ((i >> (4 + j)) & 1) != 0;
            if (OBSK == LANE_OBS_GRID1) { a[j] = lo ? 0.5f : hi ? 1.0f : 0.0f; b[j] = lo ? 1.5f : hi ? -1.0f : 0.0f; }
            else { a[j] = lo ? 1.0f : hi ? 127.0f / 255.0f : 0.0f; b[j] = 0.0f; }
        }
        tabA[i] = make_float4(a[0], a[1], a[2], a[3]);
        if (OBSK == LANE_OBS_GRID1) tabB[i] = make_float4(b[0], b[1], b[2], b[3]);
    }
}

// 16-byte group j of the flat run of floats whose bits start at bit 0 of the strings -> four floats
template <int OBSK>
__device__ __forceinline__ float4 lane_group(const u32 *bits, const float4 *tabA, const float4 *tabB, int j)
{
    const int w = j >> 3, sh = (j & 7) * 4;
    if (OBSK == LANE_OBS_GRID1) {
        const uint4 q = ((const uint4 *)bits)[w];
        const float4 a = tabA[((q.x >> sh) & 15u) | (((q.y >> sh) & 15u) << 4)];
        const float4 b = tabB[((q.z >> sh) & 15u) | (((q.w >> sh) & 15u) << 4)];
        return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    const uint2 q = ((const uint2 *)bits)[w];
    return tabA[((q.x >> sh) & 15u) | (((q.y >> sh) & 15u) << 4)];
}

// float f of the flat run, bit by bit (the ragged last wave, the last chunk of a tape that is not a multiple of TC)
template <int OBSK>
__device__ __forceinline__ float lane_float(const u32 *bits, int f)
{
    constexpr int NPL = lane_plane_count<OBSK>();
    const u32 *P = bits + NPL * (f >> 5);
    const int b = f & 31;
    if (OBSK == LANE_OBS_GRID1)
        return ((P[0] >> b) & 1u) ? 0.5f : ((P[1] >> b) & 1u) ? 1.0f : ((P[2] >> b) & 1u) ? 1.5f : ((P[3] >> b) & 1u) ? -1.0f : 0.0f;
    return ((P[0] >> b) & 1u) ? 1.0f : ((P[1] >> b) & 1u) ? 127.0f / 255.0f : 0.0f;
}

// ORs a value of at most 64 bits (the crops: 25 / 49 bits per channel) into plane k at bit offset off
template <int NPL>
__device__ __forceinline__ void lane_or64(u32 *bits, int k, int off, u64 v)
{
    const int w = off >> 5, sb = off & 31;
    const u64 a = (u64)(u32)v << sb, b = (u64)(u32)(v >> 32) << sb;
    u32 *P = bits + NPL * w + k;
    atomicOr(&P[0], (u32)a);
    atomicOr(&P[NPL], (u32)(a >> 32) | (u32)b);
    if ((u32)(b >> 32)) atomicOr(&P[2 * NPL], (u32)(b >> 32));
}

// The colours of a crop (single_snake.py:166-193) as window planes: a window cell that is off the grid or on the ring is
// (0,0,0); food (1,0,0), head (0,1,0), body (0,127/255,0), background (1,1,1).  V = occupancy of the window, W = its cells
// inside the ring, F = the food's bit (inside W, or 0), CENTRE = the head's bit.
struct LaneCrop {
    u64 R, G1, B, GH; // red 1, green 1, blue 1, green 127/255
};
__device__ __forceinline__ LaneCrop lane_crop_colours(u64 V, u64 W, u64 F, u64 CENTRE)
{
    LaneCrop k;
    k.R = W & ~V;                  // free or food
    k.B = k.R & ~F;                // free
    k.G1 = k.B | (W & CENTRE);     // free, or the head inside the ring
    k.GH = V & W & ~CENTRE;        // body
    return k;
}

} // namespace wurm
