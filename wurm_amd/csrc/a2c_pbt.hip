// a2c_pbt.hip — C ABI of the exploit / explore step of population-based training (kernels: a2c_pbt.hpp;
// include/wurm_hip.h: wurm_a2c_ff_pop_exploit).  Arguments are validated before the first HIP call, so refusals work with
// no device present.
#include "a2c_pbt.hpp"
#include "../../include/wurm_hip.h"

#include <cmath>

using namespace wurm;
using namespace wurm::pbt;

namespace {

bool valid_factor(double f) { return std::isfinite(f) && f > 0.0; }

// 0 <= lo <= hi, hi = +infinity allowed (a NaN fails the comparisons)
bool valid_bounds(double lo, double hi) { return lo >= 0.0 && lo <= hi; }

} // namespace

extern "C" {

int wurm_a2c_ff_pop_exploit(float *params, float *exp_avg, float *exp_avg_sq, double *hyper, const double *scores,
                            int32_t *order, int32_t *parent, int64_t num_params, int64_t num_members,
                            int64_t num_replace, const double *perturb, uint64_t seed, int64_t generation, void *stream)
{
    if (!params || !exp_avg || !exp_avg_sq || !hyper || !scores || !order || !parent || !perturb)
        return WURM_ERR_INVALID_ARG;
    if (num_params <= 0 || num_members <= 0 || num_replace < 0 || generation < 0) return WURM_ERR_INVALID_ARG;
    if (num_replace > num_members / 2) return WURM_ERR_INVALID_ARG; // 2 k > P: a source would also be a destination
    const Perturb f = {perturb[0], perturb[1], perturb[2], perturb[3], perturb[4], perturb[5], perturb[6], perturb[7]};
    if (!valid_factor(f.lr_down) || !valid_factor(f.lr_up) || !valid_factor(f.e_down) || !valid_factor(f.e_up))
        return WURM_ERR_INVALID_ARG;
    if (!valid_bounds(f.lr_lo, f.lr_hi) || !valid_bounds(f.e_lo, f.e_hi)) return WURM_ERR_INVALID_ARG;
    if (num_members > 65535) return WURM_ERR_UNSUPPORTED; // the member is the copy kernel's grid y
    const int64_t slices = (num_params + SLICE - 1) / SLICE;
    if (slices > 0x7fffffffLL) return WURM_ERR_UNSUPPORTED;

    (void)hipGetLastError();
    WURM_LAUNCH(pbt_rank_kernel, dim3((unsigned)((num_members + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                (hipStream_t)stream, scores, (int *)order, (long long)num_members);
    WURM_LAUNCH(pbt_copy_kernel, dim3((unsigned)slices, (unsigned)num_members), dim3(THREADS), 0, (hipStream_t)stream,
                params, exp_avg, exp_avg_sq, hyper, scores, (const int *)order, (int *)parent, (long long)num_params,
                (long long)num_members, (unsigned)num_replace, f, (u64)seed, (u64)generation);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
