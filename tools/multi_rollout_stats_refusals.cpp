// multi_rollout_stats_refusals.cpp — the argument checks of wurm_multi_rollout_stats (wurm_amd/csrc/multi_rollout_stats.hip)
// from a stand-alone host program, for a sanitizer pass on the CPU: every call below is refused before any HIP call, so no
// device is needed (and none is touched).  Build the entry point's translation unit and this file with the host
// sanitizers and run the result:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined wurm_amd/csrc/multi_rollout_stats.hip wurm_amd/csrc/options.hip \
//       tools/multi_rollout_stats_refusals.cpp -o /tmp/multi_rollout_stats_refusals && /tmp/multi_rollout_stats_refusals
//
// Prints the number of refusals checked and exits 0; a wrong code, or a sanitizer report, ends it with a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/wurm_hip.h"

namespace {

int checked = 0;

void expect(int got, int want, const char *what)
{
    ++checked;
    if (got != want) {
        std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
        std::exit(1);
    }
}

struct Args {
    const float *rewards, *food, *size;
    const uint8_t *dones, *boost, *snake, *edge;
    const float *probs;
    const uint8_t *all_done;
    void *carry;
    double *accum, *smooth, *table;
    void *workspace;
    int64_t bytes, N, K, T;
    double alpha;
};

int call(const Args &a)
{
    return wurm_multi_rollout_stats(a.rewards, a.food, a.size, a.dones, a.boost, a.snake, a.edge, a.probs, a.all_done,
                                    a.carry, a.accum, a.smooth, a.table, a.workspace, a.bytes, a.N, a.K, a.T, a.alpha,
                                    nullptr);
}

} // namespace

int main()
{
    alignas(16) static float f[64];
    alignas(16) static uint8_t b[64];
    alignas(16) static double d[64];
    const int64_t N = 12, K = 2, T = 3;
    const int64_t bytes = wurm_multi_rollout_stats_workspace_bytes(N, K, T);
    if (bytes != 8 * K * (4 * (10 * T + 5) + 10 * T)) {
        std::fprintf(stderr, "workspace_bytes(%lld, %lld, %lld) = %lld\n", (long long)N, (long long)K, (long long)T,
                     (long long)bytes);
        return 1;
    }
    const Args ok = {f, f, f, b, b, b, b, f, b, d, d, d, d, d, bytes, N, K, T, 0.025};
    Args a;

#define REFUSED(field, value, code) a = ok; a.field = value; expect(call(a), code, #field " = " #value)
    REFUSED(rewards, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(food, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(size, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(dones, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(boost, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(snake, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(edge, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(carry, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(accum, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(smooth, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(workspace, nullptr, WURM_ERR_INVALID_ARG);
    REFUSED(N, 0, WURM_ERR_INVALID_ARG);
    REFUSED(N, -12, WURM_ERR_INVALID_ARG);
    REFUSED(N, INT64_MIN, WURM_ERR_INVALID_ARG);
    REFUSED(K, 0, WURM_ERR_INVALID_ARG);
    REFUSED(K, -1, WURM_ERR_INVALID_ARG);
    REFUSED(K, 65536, WURM_ERR_UNSUPPORTED);
    REFUSED(T, 0, WURM_ERR_INVALID_ARG);
    REFUSED(T, -3, WURM_ERR_INVALID_ARG);
    REFUSED(alpha, -0.1, WURM_ERR_INVALID_ARG);
    REFUSED(alpha, 1.5, WURM_ERR_INVALID_ARG);
    REFUSED(alpha, std::nan(""), WURM_ERR_INVALID_ARG);
    REFUSED(alpha, INFINITY, WURM_ERR_INVALID_ARG);
    REFUSED(bytes, bytes - 1, WURM_ERR_INVALID_ARG);
    REFUSED(bytes, 0, WURM_ERR_INVALID_ARG);
    REFUSED(bytes, -1, WURM_ERR_INVALID_ARG);
    REFUSED(workspace, (char *)d + 8, WURM_ERR_INVALID_ARG);
    REFUSED(probs, f + 1, WURM_ERR_INVALID_ARG);
#undef REFUSED
    // the workspace query at refused and at large sizes: 0, or a positive count without a signed overflow on the way
    const int64_t zero[][3] = {{0, 2, 5}, {-3, 2, 5}, {8, 0, 5}, {8, -1, 5}, {8, 2, 0}, {8, 2, -1}, {8, 65536, 5}};
    for (const auto &z : zero) expect((int)(wurm_multi_rollout_stats_workspace_bytes(z[0], z[1], z[2]) != 0), 0, "query");
    expect((int)(wurm_multi_rollout_stats_workspace_bytes(1 << 20, 8, 1000) > 0), 1, "large query");
    std::printf("%d refusals checked\n", checked);
    return 0;
}
