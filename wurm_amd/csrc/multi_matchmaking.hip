// multi_matchmaking.hip — translation unit and C ABI of the league's matchmaking kernels (multi_matchmaking.hpp;
// include/wurm_hip.h: wurm_multi_league_draw, wurm_multi_league_plan, wurm_multi_league_plan_workspace_bytes).  Arguments
// are validated before the first HIP call, so refusals work with no device present.
#include "multi_matchmaking.hpp"
#include "../../include/wurm_hip.h"

using namespace wurm;

static_assert(plan::LAUNCHES == WURM_LEAGUE_PLAN_LAUNCHES, "the header states the number of launches");

extern "C" {

int wurm_multi_league_draw(const wurm_league_draw *c)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    const int K = c->num_snakes, A = c->num_policies;
    if (c->num_envs < 0 || c->env_offset < 0 || K < 1 || A < 1) return WURM_ERR_INVALID_ARG;
    if (K > draw::MAX_SEATS) return WURM_ERR_UNSUPPORTED;
    const bool distinct = c->replacement == 0;
    if (distinct && A < K) return WURM_ERR_INVALID_ARG;
    draw::args g = {};
    for (int k = 0; k < draw::MAX_SEATS; ++k) g.pinned[k] = -1;
    if (c->pinned) {
        for (int k = 0; k < K; ++k) {
            const int p = c->pinned[k];
            if (p < -1 || p >= A) return WURM_ERR_INVALID_ARG;
            if (distinct && p >= 0)
                for (int j = 0; j < k; ++j)
                    if (g.pinned[j] == p) return WURM_ERR_INVALID_ARG;
            g.pinned[k] = p;
        }
    }
    if (c->num_envs > INT32_MAX / K) return WURM_ERR_UNSUPPORTED;                      // (the row list is int32)
    if (c->env_offset > (1LL << 32) - c->num_envs) return WURM_ERR_UNSUPPORTED;        // (env ids are 32 bits)
    if (c->num_envs == 0) return WURM_OK;
    if (!c->lineup) return WURM_ERR_INVALID_ARG;
    g.tickets = c->tickets; g.lineup = (long long *)c->lineup; g.N = c->num_envs; g.env_offset = c->env_offset;
    g.seed = c->seed; g.call = c->call; g.K = K; g.A = A; g.replacement = distinct ? 0 : 1;
    const dim3 grid((unsigned)((g.N + draw::THREADS - 1) / draw::THREADS)), block(draw::THREADS);
    (void)hipGetLastError();
    if (K <= 4) WURM_LAUNCH(league_draw_kernel<4>, grid, block, 0, (hipStream_t)c->stream, g);
    else if (K <= 16) WURM_LAUNCH(league_draw_kernel<16>, grid, block, 0, (hipStream_t)c->stream, g);
    else WURM_LAUNCH(league_draw_kernel<64>, grid, block, 0, (hipStream_t)c->stream, g);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int64_t wurm_multi_league_plan_workspace_bytes(int64_t num_rows, int num_policies)
{
    if (num_rows < 0 || num_rows > INT32_MAX || num_policies < 1) return 0;
    if (num_rows == 0) return 8;
    const long long words = plan::num_chunks(num_rows) * num_policies + plan::num_tiles(num_policies);
    return (int64_t)((words * 4 + 7) / 8 * 8);
}

int wurm_multi_league_plan(const wurm_league_plan *c)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (c->num_rows < 0 || c->num_policies < 1) return WURM_ERR_INVALID_ARG;
    if (c->lineup_dtype < WURM_LINEUP_I64 || c->lineup_dtype > WURM_LINEUP_U8) return WURM_ERR_INVALID_ARG;
    if (c->num_rows > INT32_MAX) return WURM_ERR_UNSUPPORTED; // (`order` is int32)
    if (c->num_rows == 0) return WURM_OK;
    if (!c->lineup || !c->order || !c->offsets || !c->dropped || !c->workspace) return WURM_ERR_INVALID_ARG;
    if (((uintptr_t)c->workspace & 7) != 0) return WURM_ERR_INVALID_ARG;
    if (c->workspace_bytes < wurm_multi_league_plan_workspace_bytes(c->num_rows, c->num_policies)) return WURM_ERR_INVALID_ARG;
    plan::args g = {};
    g.lineup = c->lineup; g.order = c->order; g.offsets = (long long *)c->offsets; g.dropped = c->dropped;
    g.R = c->num_rows; g.A = c->num_policies; g.L = plan::chunk_rows(g.R); g.C = plan::num_chunks(g.R);
    g.table = (int *)c->workspace; g.tile_sum = g.table + g.C * g.A; g.dtype = c->lineup_dtype;
    const dim3 block(plan::THREADS), chunks((unsigned)((g.C + plan::WAVES - 1) / plan::WAVES)),
        tiles((unsigned)plan::num_tiles(g.A));
    hipStream_t st = (hipStream_t)c->stream;
    (void)hipGetLastError();
    WURM_LAUNCH(league_plan_count_kernel, chunks, block, 0, st, g);
    WURM_LAUNCH(league_plan_chunks_kernel, tiles, block, 0, st, g);
    WURM_LAUNCH(league_plan_offsets_kernel, tiles, block, 0, st, g);
    WURM_LAUNCH(league_plan_place_kernel, chunks, block, 0, st, g);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
