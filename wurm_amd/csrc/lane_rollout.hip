// lane_rollout.hip — translation unit of the one-env-per-LANE rollout (lane_rollout.hpp) and of the per-call step on a
// resident compact state built from the same pieces (lane_resident.hpp).  It needs the one-env-per-wave device code
// (single_device.hpp: state load / store, rollout_generic for envs outside its domain, the 9 x 9 reset draw) and none of the
// kernels or entry points built on it; compiled on its own it builds in a fraction of the time of single_snake.hip.
#include "single_device.hpp"
#include "lane_rollout.hpp"
#include "lane_resident.hpp"
