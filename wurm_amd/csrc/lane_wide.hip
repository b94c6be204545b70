// lane_wide.hip — translation unit of the one-env-per-LANE rollout of 10 x 10 and 11 x 11 SingleSnake grids (lane_wide.hpp) and of
// the per-call step of those sizes on a resident compact state (lane_wide_resident.hpp).
// Like lane_rollout.hip it needs the one-env-per-wave device code (single_device.hpp: state load / store, rollout_generic for
// envs outside its domain, the reset draw) and none of the kernels or entry points built on it.
#include "single_device.hpp"
#include "lane_wide.hpp"
#include "lane_wide_resident.hpp"
