// single_grid.hip — the SimpleGridworld half of the one-env-per-wave kernels: launch<false> and every kernel it instantiates
// (single_snake.hip holds launch<true> and the entry points), so that the two halves compile side by side.
#include "single_launch.hpp"

namespace wurm {

template int launch<false>(Kind, StepArgs, void *);

} // namespace wurm
