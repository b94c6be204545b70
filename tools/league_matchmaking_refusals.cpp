// league_matchmaking_refusals.cpp — the argument checks of wurm_multi_league_draw and wurm_multi_league_plan
// (wurm_amd/csrc/multi_matchmaking.hip) from a stand-alone host program, for a sanitizer pass on the CPU: every call below
// is refused, or is a no-op, before any HIP call, so no device is needed (and none is touched).  Build the entry points'
// translation unit and this file with the host sanitizers and run the result:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined wurm_amd/csrc/multi_matchmaking.hip wurm_amd/csrc/options.hip \
//       tools/league_matchmaking_refusals.cpp -o /tmp/league_matchmaking_refusals && /tmp/league_matchmaking_refusals
//
// Prints the number of calls checked and exits 0; a wrong code, or a sanitizer report, ends it with a failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/wurm_hip.h"

namespace {

int checked = 0;

void expect(long long got, long long want, const char *what)
{
    ++checked;
    if (got != want) {
        std::fprintf(stderr, "%s: returned %lld, expected %lld\n", what, got, want);
        std::exit(1);
    }
}

} // namespace

int main()
{
    alignas(16) static int64_t words[64];
    static int32_t ints[64];
    int32_t pins[2] = {-1, -1};
    const wurm_league_draw draw = {ints, words, pins, 8, 0, 1, 0, 2, 4, 0, nullptr};
    wurm_league_draw d;

#define DRAW(field, value, code) d = draw; d.field = value; expect(wurm_multi_league_draw(&d), code, "draw " #field " = " #value)
    expect(wurm_multi_league_draw(nullptr), WURM_ERR_INVALID_ARG, "draw null block");
    DRAW(num_envs, -1, WURM_ERR_INVALID_ARG);
    DRAW(num_envs, INT64_MIN, WURM_ERR_INVALID_ARG);
    DRAW(env_offset, -1, WURM_ERR_INVALID_ARG);
    DRAW(num_snakes, 0, WURM_ERR_INVALID_ARG);
    DRAW(num_snakes, -1, WURM_ERR_INVALID_ARG);
    DRAW(num_snakes, 5, WURM_ERR_INVALID_ARG);      // (more seats than policies, before `pinned` is read)
    DRAW(num_policies, 0, WURM_ERR_INVALID_ARG);
    DRAW(num_policies, 1, WURM_ERR_INVALID_ARG);
    DRAW(lineup, nullptr, WURM_ERR_INVALID_ARG);
    DRAW(num_snakes, 65, WURM_ERR_UNSUPPORTED);
    DRAW(num_envs, INT64_MAX, WURM_ERR_UNSUPPORTED);
    DRAW(num_envs, 1LL << 30, WURM_ERR_UNSUPPORTED);
    DRAW(env_offset, (1LL << 32) - 7, WURM_ERR_UNSUPPORTED);
    DRAW(env_offset, INT64_MAX, WURM_ERR_UNSUPPORTED);
    DRAW(num_envs, 0, WURM_OK);
    pins[0] = 4;
    DRAW(seed, 1, WURM_ERR_INVALID_ARG);
    pins[0] = -2;
    DRAW(seed, 1, WURM_ERR_INVALID_ARG);
    pins[0] = pins[1] = 3;
    DRAW(seed, 1, WURM_ERR_INVALID_ARG);
    d = draw; d.replacement = 1; d.num_envs = 0;
    expect(wurm_multi_league_draw(&d), WURM_OK, "draw: pinned twice with replacement, no envs");
#undef DRAW

    const int64_t need = wurm_multi_league_plan_workspace_bytes(24, 4);
    expect(need, 24, "workspace_bytes(24, 4)");
    const wurm_league_plan plan = {words, ints, words, ints, words, need, 24, 4, WURM_LINEUP_I64, nullptr};
    wurm_league_plan p;
#define PLAN(field, value, code) p = plan; p.field = value; expect(wurm_multi_league_plan(&p), code, "plan " #field " = " #value)
    expect(wurm_multi_league_plan(nullptr), WURM_ERR_INVALID_ARG, "plan null block");
    PLAN(num_rows, -1, WURM_ERR_INVALID_ARG);
    PLAN(num_rows, INT64_MIN, WURM_ERR_INVALID_ARG);
    PLAN(num_policies, 0, WURM_ERR_INVALID_ARG);
    PLAN(num_policies, -7, WURM_ERR_INVALID_ARG);
    PLAN(lineup_dtype, -1, WURM_ERR_INVALID_ARG);
    PLAN(lineup_dtype, 5, WURM_ERR_INVALID_ARG);
    PLAN(lineup, nullptr, WURM_ERR_INVALID_ARG);
    PLAN(order, nullptr, WURM_ERR_INVALID_ARG);
    PLAN(offsets, nullptr, WURM_ERR_INVALID_ARG);
    PLAN(dropped, nullptr, WURM_ERR_INVALID_ARG);
    PLAN(workspace, nullptr, WURM_ERR_INVALID_ARG);
    PLAN(workspace, (char *)words + 4, WURM_ERR_INVALID_ARG);
    PLAN(workspace_bytes, need - 1, WURM_ERR_INVALID_ARG);
    PLAN(workspace_bytes, 0, WURM_ERR_INVALID_ARG);
    PLAN(workspace_bytes, -8, WURM_ERR_INVALID_ARG);
    PLAN(num_rows, 1LL << 31, WURM_ERR_UNSUPPORTED);
    PLAN(num_rows, INT64_MAX, WURM_ERR_UNSUPPORTED);
    PLAN(num_rows, 0, WURM_OK);
#undef PLAN
    // the query at refused and at large sizes: 0, or a positive count without a signed overflow on the way
    const int64_t zero[][2] = {{-1, 4}, {1LL << 31, 4}, {INT64_MAX, 4}, {24, 0}, {24, -1}};
    for (const auto &z : zero) expect(wurm_multi_league_plan_workspace_bytes(z[0], (int)z[1]), 0, "query");
    expect(wurm_multi_league_plan_workspace_bytes(0, 4), 8, "query without rows");
    expect(wurm_multi_league_plan_workspace_bytes(INT32_MAX, INT32_MAX) > (1LL << 40), 1, "large query");
    std::printf("%d calls checked\n", checked);
    return 0;
}
