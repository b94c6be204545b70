// multi_observe.hpp — MultiSnake's observation writers from the env in LDS: 'full', 'partial_n', the grouped 'full' writer.
#pragma once
#include "multi_device.hpp"

namespace wurm {

// ------------------------------------------------------------------------------------------------ observations

// 'full' observation (_observe_agent :268-281 + _make_generic_rgb :175-192) of every agent from LDS.
// Per row of 64 cells the class of each cell is worked out ONCE (K clock compares, head owner, food); what an agent
// sees that has neither its head nor its body on the cell — border (0,0,0), somebody's head (0,0,192), somebody's body
// (0,0,96), food (255,0,0), background (255,255,255) — is the same for every agent, so rows without any snake cell (most
// of them) store the same three registers K times, and the per-agent priority chain runs only in rows that hold a
// snake.  Stores take the scalar base of (agent, env) plus a 32-bit lane offset.
__device__ __forceinline__ void store_rgb(float *base, u32 off0, u32 off1, u32 off2, float r, float g, float b)
{
    asm volatile("global_store_dword %0, %1, %6\n\tglobal_store_dword %2, %3, %6\n\tglobal_store_dword %4, %5, %6"
                 : : "v"(off0), "v"(r), "v"(off1), "v"(g), "v"(off2), "v"(b), "s"(base) : "memory");
}

__device__ __forceinline__ void observe_full(const Ctx &cx, const MultiArgs &p, float *__restrict__ obs,
                                             long long env, int hc)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    // head owner per cell: hmap[c] = 1 + snake index (consistent states have at most one head per cell)
    if (lane < K && hc >= 0) cx.hmap[hc] = (unsigned char)(lane + 1);
    wave_lds_sync();
    const float G1 = 192.0f / 255.0f, G2 = 96.0f / 255.0f;
    // agent 0's observation of this env (wave-uniform: told to the compiler so that it lives in SGPRs)
    float *const obs_env = (float *)uniform64((long long)(obs + env * p.obs_elems));
    const long long agent_stride = p.N * p.obs_elems;    // to the next agent's
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = lane + 64 * k;
        const bool valid = c < C;
        const int cc = valid ? c : 0;
        const int y = div_size(cc, cx.rcpS), x = cc - y * S;
        const bool edge = y == 0 || x == 0 || y == S - 1 || x == S - 1;
        u64 bm = 0; // bit s: snake s has body on this cell
        for (int s = 0; s < K; ++s) bm |= (u64)((int)(cx.body[s * C + cc] & VMASK) > cx.tclk[s]) << s;
        const int ho = (int)cx.hmap[cc] - 1;
        const bool fd = cx.food[cc] != 0;
        const bool snake_here = valid && !edge && (ho >= 0 || bm != 0);
        const float ro = (edge || snake_here) ? 0.0f : 1.0f;
        const float go = (edge || snake_here || fd) ? 0.0f : 1.0f;
        const float bo = edge ? 0.0f : (ho >= 0 ? G1 : (bm != 0 ? G2 : (fd ? 0.0f : 1.0f)));
        const u32 o0 = (u32)cc * 4u, o1 = (u32)(C + cc) * 4u, o2 = (u32)(2 * C + cc) * 4u;
        const bool row_has_snake = ballot(snake_here) != 0;
        float *base = obs_env;
        if (valid) {
            if (!row_has_snake) {
                for (int a = 0; a < K; ++a, base += agent_stride) store_rgb(base, o0, o1, o2, ro, go, bo);
            } else {
                for (int a = 0; a < K; ++a, base += agent_stride) {
                    float r = ro, g = go, b = bo;
                    if (snake_here && (ho == a || ((bm >> a) & 1))) {
                        // an agent with its own head or body on the cell: the reference's paint order
                        if (ho >= 0 && ho != a) { r = 0.0f; g = 0.0f; b = G1; }             // other head (0,0,192)
                        else if (bm & ~(1ull << a)) { r = 0.0f; g = 0.0f; b = G2; }         // other body (0,0,96)
                        else if (ho == a) { r = 0.0f; g = G1; b = 0.0f; }                   // own head (0,192,0)
                        else { r = 0.0f; g = G2; b = 0.0f; }                                // own body (0,96,0)
                    }
                    store_rgb(base, o0, o1, o2, r, g, b);
                }
            }
        }
    }
    wave_lds_sync();
    if (lane < K && hc >= 0) cx.hmap[hc] = 0;
    wave_lds_sync();
}

// 'full' observation of at most 10 snakes (experiments/speeds.py runs 10), agent-major.  With 4096 envs in flight the row-major order of observe_full
// means ~49 000 concurrent 256-byte write streams (every row of 64 cells touches all K agents' regions, megabytes
// apart); a pure store kernel in that order reaches 3.6 TB/s, agent by agent — one contiguous 3 * S * S float region
// at a time per wave — 4.8 TB/s (tools/microbench/store_pattern.hip).  So the class of every cell is first written to
// LDS as a 16-bit code (K clock compares, head owner, food, border: once per cell), then each agent's three planes are
// produced from the codes (layout: SNAP_OWNER_SHIFT below).
// (Also tried, measured, dropped: issuing these stores in four parts between the phases of the NEXT step, so that the
// store queue would drain while the wave computes — no gain: the waves of a launch stall on the store path together.)
// 16-bit class code of a cell: body mask of snakes 0..9 | (head owner + 1) << 10 | food << 14 | border << 15
constexpr int SNAP_OWNER_SHIFT = 10;

// class code of every cell of the env in LDS -> snap[] (executed by the wave that owns the env's state)
__device__ __forceinline__ void snap_write(const Ctx &cx, int hc, unsigned short *snap)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    if (lane < K && hc >= 0) cx.hmap[hc] = (unsigned char)(lane + 1);
    wave_lds_sync();
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = lane + 64 * k;
        if (c < C) {
            const int y = div_size(c, cx.rcpS), x = c - y * S;
            const bool edge = y == 0 || x == 0 || y == S - 1 || x == S - 1;
            u32 v = 0;
            for (int s = 0; s < K; ++s) v |= (u32)((int)(cx.body[s * C + c] & VMASK) > cx.tclk[s]) << s;
            v |= (u32)cx.hmap[c] << SNAP_OWNER_SHIFT;
            v |= (u32)(cx.food[c] != 0) << 14;
            v |= (u32)edge << 15;
            snap[c] = (unsigned short)v;
        }
    }
    wave_lds_sync();
    if (lane < K && hc >= 0) cx.hmap[hc] = 0;
    wave_lds_sync();
}

// the K agents' observations of one env from its class codes, agent by agent (any wave of the workgroup may run this)
// (k0 .. k1: the rows of 64 cells to write — a workgroup hands out parts of an agent's view: wg_observe_snap)
__device__ __forceinline__ void snap_emit_agent(const Ctx &cx, const MultiArgs &p, float *obs_env,
                                                const unsigned short *snap, int a, int k0 = 0, int k1 = 1 << 30)
{
    const int C = cx.C, lane = cx.lane;
    const float G1 = 192.0f / 255.0f, G2 = 96.0f / 255.0f;
    {
        float *const base = obs_env + a * (p.N * p.obs_elems);
        for (int k = k0; k < min(k1, cx.cpl); ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                const u32 v = (u32)snap[c];
                const bool edge = (v >> 15) != 0, fd = ((v >> 14) & 1u) != 0;
                const int ho = (int)((v >> SNAP_OWNER_SHIFT) & 15u) - 1;
                const u32 bm = v & ((1u << SNAP_OWNER_SHIFT) - 1u);
                const bool snake_here = !edge && (ho >= 0 || bm != 0);
                // border (0,0,0), somebody's head (0,0,192), somebody's body (0,0,96), food (255,0,0), background white
                float r = (edge || snake_here) ? 0.0f : 1.0f;
                float g = (edge || snake_here || fd) ? 0.0f : 1.0f;
                float b = edge ? 0.0f : (ho >= 0 ? G1 : (bm != 0 ? G2 : (fd ? 0.0f : 1.0f)));
                if (snake_here && (ho == a || ((bm >> a) & 1u))) { // own head or body here: the reference's paint order
                    if (ho >= 0 && ho != a) { r = 0.0f; g = 0.0f; b = G1; }          // other head (0,0,192)
                    else if (bm & ~(1u << a)) { r = 0.0f; g = 0.0f; b = G2; }         // other body (0,0,96)
                    else if (ho == a) { r = 0.0f; g = G1; b = 0.0f; }                // own head (0,192,0)
                    else { r = 0.0f; g = G2; b = 0.0f; }                             // own body (0,96,0)
                }
                store_rgb(base, (u32)c * 4u, (u32)(C + c) * 4u, (u32)(2 * C + c) * 4u, r, g, b);
            }
        }
    }
}

__device__ __forceinline__ void snap_emit(const Ctx &cx, const MultiArgs &p, float *obs_env, const unsigned short *snap)
{
    for (int a = 0; a < cx.K; ++a) snap_emit_agent(cx, p, obs_env, snap, a);
}

__device__ __forceinline__ void observe_full_snap(const Ctx &cx, const MultiArgs &p, float *__restrict__ obs,
                                                  long long env, int hc)
{
    snap_write(cx, hc, cx.snap);
    snap_emit(cx, p, (float *)uniform64((long long)(obs + env * p.obs_elems)), cx.snap);
    wave_lds_sync();
}

// 'partial_n' observation (:289-332): the crop of the env image (_get_env_images :194-227) around each living head.
// The image is the same for every observer, and a cell of it can only show a handful of different pixels: background,
// border, food, and per snake its body and its head (brightened while it boosts, :198).  So (round 5):
//   * one pass over the grid gives every cell a one-byte CODE (cell_codes):
//     0 background, 1 border ring, 2 food, 3 + 2s body of snake s, 4 + 2s head of snake s, 255 anything else (several
//     snakes on the cell, food under a snake, a head without its body: hand-made states, heads that have just collided);
//   * lanes 0 .. 2K+2 compute the 2K + 3 pixels once per step with the reference's own arithmetic (pixel_table: the
//     float products, `.short()`, black -> white, `/ 255`) into an LDS table of 16-byte entries;
//   * a window cell is then a byte read, one 16-byte table read and three stores (crop_emit); a cell with code 255 is
//     rendered on the spot (pixel_slow: the sum over the snakes found there, ascending, as :201-205 sums).
// History: round 2 rendered the whole image into LDS (8 bytes per cell) and cropped it; rounds 3-4 computed every (agent,
// window cell) pixel directly — 16 000 of a step's 40 400 cycles at cfg4' (profiles/r04_kernel_timeline.txt), VALU-bound.
constexpr int PC_BG = 0, PC_RING = 1, PC_FOOD = 2, PC_SNAKE0 = 3, PC_COMPLEX = 255;

// bit k <=> cell lane + 64 k is a free interior cell (:439-445, :393-399): code 0 of cell_codes
__device__ __forceinline__ u64 free_from_codes(const Ctx &cx, const unsigned char *codes)
{
    u64 fr = 0;
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = cx.lane + 64 * k;
        if (c < cx.C && codes[c] == PC_BG) fr |= 1ull << k;
    }
    return fr;
}

// One pass over the grid.  Bodies only in the scan — five 64-cell rows at a time so that the five reads of a snake are in
// flight together, and per (cell, snake) just a mask, a compare, a select and a carry-add (the compiler must keep this loop
// free of branches: check the ISA after touching it) — the K head cells are raised afterwards by the K lanes that own them:
// a head sits on its own body in every state the dynamics produce; anywhere else the cell is marked complex.
// The same map answers _add_food's "free interior cell" (code 0: free_from_codes), so a step with random_rate food and
// crops scans the grids once, not twice (multi_step_body builds it, observe_partial reuses it: Snake::cmap_ok).
struct CellCounts {
    u64 free;   // bit k <=> cell lane + 64 k is a free interior cell (code 0), as free_cells(cx, hc, 1) / free_from_codes
    int nfree;  // their number over the wave (count_bits)
    int nfood;  // cells that hold food, whatever else is on them (food_count)
};

__device__ __forceinline__ CellCounts cell_codes(const Ctx &cx, int hc, unsigned char *codes, u64 ring)
{
    const int C = cx.C, K = cx.K, lane = cx.lane;
    constexpr int U = 5;
    const int myT = lane < K ? cx.tclk[lane] : 0;
    CellCounts cc_out;
    cc_out.free = 0;
    cc_out.nfree = cc_out.nfood = 0;
    for (int k0 = 0; k0 < cx.cpl; k0 += U) {
        int cc[U];
        u32 fd[U], code[U], cnt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cc[u] = min(lane + 64 * (k0 + u), C - 1); // (rows past the grid: the last cell again, not stored)
            fd[u] = cx.food[cc[u]];
            code[u] = PC_BG;
            cnt[u] = 0;
        }
        for (int s = 0; s < K; ++s) {
            const int T = lane_value(myT, s);
            const u32 mine = (u32)(PC_SNAKE0 + 2 * s);
            const unsigned short *b = cx.body + s * C;
            u32 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = b[cc[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = (int)(v[u] & VMASK) > T;
                code[u] = live ? mine : code[u];
                cnt[u] += (u32)live;
            }
        }
        const u32 rb = (u32)(ring >> k0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32 c1 = cnt[u] > 1u ? (u32)PC_COMPLEX : code[u];             // two bodies on the cell
            c1 = fd[u] != 0 ? (c1 == PC_BG ? (u32)PC_FOOD : (u32)PC_COMPLEX) : c1; // food; food under a body
            c1 = ((rb >> u) & 1u) ? (u32)PC_RING : c1;                    // :225 the border wins over everything
            const bool valid = lane + 64 * (k0 + u) < C;
            if (valid) codes[cc[u]] = (unsigned char)c1;
            // the counts _add_food needs come out of the same pass (the compares' own wave masks, counted on the scalar unit)
            const bool fr = valid && c1 == PC_BG;
            cc_out.free |= (u64)fr << (k0 + u);
            cc_out.nfree += popc64(ballot(fr));
            cc_out.nfood += popc64(ballot(valid && fd[u] != 0));
        }
    }
    wave_lds_sync();
    // heads: the cell must hold its own snake's body (code 3 + 2s) and becomes 4 + 2s; anything else under a head — no
    // body, food, another snake's body, the ring is fine (it wins anyway) — is complex.  Two heads on one cell: at most one of
    // them finds its own code there; the other lanes all write the same value.
    int want = -1;
    if (lane < K && hc >= 0) {
        const int code = codes[hc];
        want = code == PC_RING ? -1 : code == PC_SNAKE0 + 2 * lane ? PC_SNAKE0 + 2 * lane + 1 : PC_COMPLEX;
    }
    wave_lds_sync();
    if (want == PC_COMPLEX) codes[hc] = (unsigned char)PC_COMPLEX;
    wave_lds_sync();
    if (want >= 0 && want != PC_COMPLEX && codes[hc] != PC_COMPLEX) codes[hc] = (unsigned char)want;
    wave_lds_sync();
    if (ballot(want == PC_COMPLEX) != 0) { // (a head on a cell without its own body may have stood on a "free" cell: hand-made states)
        cc_out.free = free_from_codes(cx, codes);
        cc_out.nfree = count_bits(cx, cc_out.free);
    }
    return cc_out;
}

// food on a cell (wave-uniform or per-lane `cell`; the caller fences), and its code with it where the map is current
__device__ __forceinline__ void put_food(const Ctx &cx, int cell, bool cmap_ok)
{
    cx.food[cell] = 1;
    if (cmap_ok) {
        const int code = cx.hmap[cell];
        cx.hmap[cell] = (unsigned char)(code == PC_BG || code == PC_FOOD ? PC_FOOD : code == PC_RING ? PC_RING : PC_COMPLEX);
    }
}

// the reference's pixel of a cell from the float sums of :201-205: .short() truncation, food, black -> white (:206-219)
__device__ __forceinline__ void pixel_finish(float a0, float a1, float a2, bool food, float &r, float &g, float &b)
{
    int ri = (int)a0, gi = (int)a1, bi = (int)a2;         // :206 .short() truncates
    if (food) ri += 255;                                  // :208-209
    if (ri == 0 && gi == 0 && bi == 0) ri = gi = bi = 255; // :214-219
    r = div255(ri);
    g = div255(gi);
    b = div255(bi);
}

// the 2K + 3 pixels a cell with a simple code can show -> tab[code] = (r, g, b, -); colf[s] = (colour, 1 + 0.5 boost) is
// in LDS already.  Lane j computes entry j (K <= 64: two rounds at most).
__device__ __forceinline__ void pixel_table(const Ctx &cx, float *tab)
{
    const int K = cx.K;
    for (int j = cx.lane; j < 2 * K + PC_SNAKE0; j += 64) {
        float r = 0.0f, g = 0.0f, b = 0.0f;                // PC_RING (:225)
        if (j != PC_RING) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            if (j >= PC_SNAKE0) {
                const int s = (j - PC_SNAKE0) >> 1;
                // :197 `body.float() * 1/3 + head.float() * 1/3`: 1.0f / 3.0f is the correctly rounded quotient the two
                // IEEE divisions gave; then the boost factor, then the colour (:198-205), summed from 0 as torch's sum does
                const float third = 1.0f / 3.0f;
                float inten = third + (((j - PC_SNAKE0) & 1) ? third : 0.0f);
                inten *= cx.colf[s * 4 + 3];
                a0 += inten * cx.colf[s * 4 + 0];
                a1 += inten * cx.colf[s * 4 + 1];
                a2 += inten * cx.colf[s * 4 + 2];
            }
            pixel_finish(a0, a1, a2, j == PC_FOOD, r, g, b);
        }
        tab[4 * j + 0] = r;
        tab[4 * j + 1] = g;
        tab[4 * j + 2] = b;
    }
}

// a cell whose code is PC_COMPLEX, rendered from the grids (interior cells only: the ring has its own code)
__device__ __forceinline__ void pixel_slow(const Ctx &cx, int c, float &r, float &g, float &b)
{
    const int C = cx.C, K = cx.K;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int s = 0; s < K; ++s) {
        const bool isb = (int)(cx.body[s * C + c] & VMASK) > cx.tclk[s], ish = cx.hcell[s] == c;
        if (isb || ish) { // a snake that is not on the cell adds inten = 0, i.e. nothing
            const float third = 1.0f / 3.0f;
            float inten = (isb ? third : 0.0f) + (ish ? third : 0.0f);
            inten *= cx.colf[s * 4 + 3];
            a0 += inten * cx.colf[s * 4 + 0];
            a1 += inten * cx.colf[s * 4 + 1];
            a2 += inten * cx.colf[s * 4 + 2];
        }
    }
    pixel_finish(a0, a1, a2, cx.food[c] != 0, r, g, b);
}

__device__ __forceinline__ void observe_partial(const Ctx &cx, const MultiArgs &p, float *__restrict__ obs,
                                                long long env, const Snake &sn)
{
    const int S = cx.S, K = cx.K, lane = cx.lane, n = p.obs_n;
    unsigned char *const codes = cx.hmap;      // (the head map of observe_full: free in a launch that writes crops)
    float *const tab = (float *)cx.img;        // 16 bytes per code (multi_layout: need_img)
    if (lane < K) {
        cx.colf[lane * 4 + 0] = (float)sn.col[0];
        cx.colf[lane * 4 + 1] = (float)sn.col[1];
        cx.colf[lane * 4 + 2] = (float)sn.col[2];
        // :198 the brightening of a boosting snake
        cx.colf[lane * 4 + 3] = 1.0f + 0.5f * (sn.boosted ? 1.0f : 0.0f);
        cx.hcell[lane] = sn.hc;
    }
    wave_lds_sync();
    pixel_table(cx, tab);
    if (!sn.cmap_ok) cell_codes(cx, sn.hc, codes, cx.has_ring ? cx.ring : border_bits(cx));
    wave_lds_sync(); // (the table)
    WURM_TLS(cx, 13);
    const int W = 2 * n + 1, W2 = W * W;
    const float rcpW = 1.0f / (float)W;
    const long long agent_stride = p.N * p.obs_elems;
    float *const o_env = obs + env * p.obs_elems;
    const u64 dead = ballot(lane < K && sn.done); // a dead observer sees zeros (:320-323)
    for (int w = lane; w < W2; w += 64) {
        // the lane's window cell relative to the observer's head: the same for every agent
        const int wy = div_size(w, rcpW), wx = w - wy * W, dy = wy - n, dx = wx - n;
        for (int a = 0; a < K; ++a) {
            float *const o = (float *)uniform64((long long)(o_env + (long long)a * agent_stride));
            const int h = ((dead >> a) & 1ull) ? -1 : lane_value(sn.hc, a);
            float r = 0.0f, g = 0.0f, b = 0.0f; // a dead observer; the zero padding (:302)
            if (h >= 0) {
                const int hy = div_size(h, cx.rcpS), hx = h - hy * S; // (uniform)
                const int y = hy + dy, x = hx + dx;
                if (y >= 0 && y < S && x >= 0 && x < S) {
                    const int c = y * S + x;
                    const int code = codes[c];
                    if (code == PC_COMPLEX) pixel_slow(cx, c, r, g, b);
                    else {
                        const float4 t = *(const float4 *)(tab + 4 * code);
                        r = t.x; g = t.y; b = t.z;
                    }
                }
            }
            o[w] = r;
            o[W2 + w] = g;
            o[2 * W2 + w] = b;
        }
    }
    wave_lds_sync();
}

__device__ __forceinline__ void observe(const Ctx &cx, const MultiArgs &p, float *__restrict__ obs, long long env,
                                        const Snake &sn)
{
    if (p.obs_mode == WURM_OBS_DEFAULT) {
        if (p.off_snap >= 0) observe_full_snap(cx, p, obs, env, sn.hc);
        else observe_full(cx, p, obs, env, sn.hc);
    }
    else if (p.obs_mode == WURM_OBS_PARTIAL) observe_partial(cx, p, obs, env, sn);
}

__device__ __forceinline__ void load_colour(const MultiArgs &p, long long agent, bool active, Snake &sn)
{
    sn.col[0] = sn.col[1] = sn.col[2] = 0;
    if (active && p.colours) {
        sn.col[0] = p.colours[agent * 3];
        sn.col[1] = p.colours[agent * 3 + 1];
        sn.col[2] = p.colours[agent * 3 + 2];
    }
}

// ---- 'full' observations of at most 5 snakes, large batches: G consecutive envs per WORKGROUP (round 4).
// G stepper waves (one env each, as above) + W writer waves.  What changed against multi_rollout_kernel<true>, and why
// (tools/microbench/store_runs.hip, profiles/r04_store_runs_microbench.txt):
//   * the stream shape: writer wave w owns agent w (w + W, ...) and writes that agent's observations of the G envs of the
//     group as ONE linear run of G * 3 S^2 floats per step (the layout is (T, K, N, 3 S^2): for a fixed agent consecutive
//     envs are adjacent) — 60 KB at cfg4 with G = 8, 16-byte stores on 16-byte boundaries.  A pure store kernel of this
//     shape runs at 5.5 TB/s (0.358 ms per 16 steps at cfg4) against 4.3 TB/s for one 7.5 KB run per wave; waves of one
//     workgroup INTERLEAVING 1 KB pieces of the same run is the slow shape (3.3 - 3.9 TB/s);
//   * the writer's arithmetic: the stepper leaves a 16-bit word per cell holding each agent's 3-bit CLASS of the cell
//     (numbered in paint order: 0 background, 1 food, 2 own body, 3 own head, 4 other body, 5 other head, 6 border), the
//     writer extracts its agent's field and reads the plane's value from a 3 x 8 float table in LDS: two VALU instructions
//     and two LDS reads per float instead of ~14 VALU per 64-cell store group for the colour logic;
//   * the steppers issue NO global memory instruction in the steady state: rewards / flags go to LDS and are written by a
//     writer wave (the CU's vector memory pipeline is in order: a stepper's small stores queued behind the observation
//     stream of the whole CU stall the stepper at issue).
constexpr int GRP_MAX_SNAKES = 5;   // 3 bits per agent in a 16-bit word (double-buffered)
constexpr int GRP_MAX_SNAKES32 = 10; // ... in a 32-bit word (single-buffered: 4 bytes per cell is what the LDS has room for once)
constexpr int GRP_TAB_BYTES = 128;  // float tab[3][8] at the start of the workgroup's LDS
constexpr int GRP_CODE_SLACK = 640;  // bytes the writers may READ behind the last code array (grp_emit_cells: 5 x 64 codes)

// LDS of multi_rollout_group_kernel with G envs per workgroup: the colour table, the envs' blocks (multi_layout), the class
// code buffers (two of 16-bit words, WIDE: one of 32-bit words), the per-step output rows and the snakes' saved scalars.
// Fills in p's offsets; returns the total (the writers read up to GRP_CODE_SLACK bytes past a code array: what lies behind
// the last one must be this LDS).
__host__ __device__ inline int group_layout(MultiArgs &p, int G, bool wide)
{
    const int lds_env = multi_layout(p, false, 0), C = p.S * p.S;
    p.grp_code_bytes = ((wide ? 4 : 2) * C + 15) & ~15;
    const int nbuf = wide ? 1 : 2;
    p.grp_out_bytes = (16 * p.K + 1 + 15) & ~15;
    const int save_bytes = 32 * p.K; // grp_save: 8 ints per snake
    const int slack0 = (wide ? 2 : 1) * GRP_CODE_SLACK - G * (nbuf * p.grp_out_bytes + save_bytes), slack = slack0 > 0 ? slack0 : 0;
    p.grp_env0 = GRP_TAB_BYTES;
    p.grp_codes = p.grp_env0 + G * lds_env;
    p.grp_outs = p.grp_codes + nbuf * G * p.grp_code_bytes;
    p.grp_save = p.grp_outs + nbuf * G * p.grp_out_bytes;
    return GRP_TAB_BYTES + G * (lds_env + nbuf * p.grp_code_bytes + nbuf * p.grp_out_bytes + save_bytes) + slack;
}

// (sum over a < K of 8^a): a 3-bit value replicated into the K agents' fields
__device__ __forceinline__ u32 grp_rep(int K) { return (u32)(((1ull << (3 * K)) - 1ull) / 7ull); }

// per-agent classes of every cell of the env in LDS -> codes[] (the wave that owns the env's state).  _observe_agent
// :268-281 paints food, own body, own head, other bodies, other heads, then the border (:183-186): a later layer wins, so
// the class of a cell for an agent is the LAST layer that covers it — with the classes numbered in paint order, the
// maximum over the layers.  Bodies first (every cell), then the K head cells are raised.
template <typename CT>
__device__ __forceinline__ void class_write(const Ctx &cx, int hc, CT *codes, u64 border)
{
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const u32 REP = grp_rep(K), REP4 = 4u * REP, REP5 = 5u * REP, REP6 = 6u * REP;
    // Five 64-cell rows at a time: for each snake its clock and head cell come out of lanes 0 .. K-1 (readlane), its five
    // body cells are read TOGETHER (one LDS round trip per snake and block, not per cell), "head on this cell" is a compare
    // with the K head cells — no head map, no pass over the border afterwards, one fence at the end — and the code of a cell
    // is a few selects; only a cell with several snakes on it branches.  (The first form read cell by cell, kept a
    // head-owner map in LDS and painted the border in a second pass: 11 000 cycles of a stepper's 67 000 per call at cfg4,
    // tools/multi_timeline.py.)
    constexpr int U = 5;
    const int myT = lane < K ? cx.tclk[lane] : 0, myH = lane < K ? hc : -1;
    for (int k0 = 0; k0 < cx.cpl; k0 += U) {
        int cc[U];
        u32 bm[U], hm[U], fd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cc[u] = min(lane + 64 * (k0 + u), C - 1); // (rows past the grid: the last cell again, not stored)
            bm[u] = hm[u] = 0;
            fd[u] = cx.food[cc[u]];
        }
        for (int s = 0; s < K; ++s) {
            const int T = lane_value(myT, s), H = lane_value(myH, s);
            const unsigned short *b = cx.body + s * C;
            u32 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = b[cc[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bm[u] |= (u32)((int)(v[u] & VMASK) > T) << s;
                hm[u] |= (u32)(cc[u] == H) << s;
            }
        }
        const u32 bb = (u32)(border >> k0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = lane + 64 * (k0 + u);
            const u32 occ = bm[u] | hm[u];
            const int first = max(__ffs((int)occ) - 1, 0);
            // one snake: the others see 4 (body) / 5 (head), the snake itself 2 / 3
            u32 code = occ == 0 ? (fd[u] != 0 ? REP : 0u) : ((hm[u] ? REP5 : REP4) ^ (6u << (3 * first)));
            const bool ring = ((bb >> u) & 1u) != 0;
            if ((occ & (occ - 1u)) != 0 && !ring) { // several snakes on the cell (hand-made states, heads that have just run into something)
                code = 0;
                for (int a = 0; a < K; ++a) {
                    const u32 others = ~(1u << a);
                    code |= ((hm[u] & others) ? 5u : (bm[u] & others) ? 4u : ((hm[u] >> a) & 1u) ? 3u : 2u) << (3 * a);
                }
            }
            if (ring) code = REP6;
            if (c < C) codes[c] = (CT)code;
        }
    }
    wave_lds_sync();
}

typedef __attribute__((address_space(1))) float grp_gfloat;     // a pointer KNOWN to be global memory: global_store, not flat_store
// Probe build (make -C wurm_amd/csrc probe -> libwurm_hip_probe.so; tools/multi_group_probe.py): WURM_MULTI_GROUP_VARIANT
// bit 2 drops the writers' stores, bit 3 the steppers' transition — which half bounds the launch.  Results are wrong by
// construction with either bit; the shipped library compiles the switches out.
#ifdef WURM_GROUP_PROBE
#define WURM_PROBE(probe, shipped) (probe)
#else
#define WURM_PROBE(probe, shipped) (shipped)
#endif

__device__ __forceinline__ float grp_tab(const float *tabp, u32 off) { return *(const float *)((const unsigned char *)tabp + off); }

// The writer: one CELL per lane — its class is extracted ONCE and looked up in the three planes' rows of the table (three
// LDS reads off one address register), three 4-byte stores per 64 cells (256 contiguous bytes each: the same stream rate as
// 16-byte stores in tools/microbench/store_runs.hip, and nothing to align or peel).  Per 64 cells: 1 + 3 LDS reads, 2 VALU,
// 3 stores.  (Round 4 first built the 16-byte-store form VERDICT r03 asked for — lane = 4 consecutive floats of a plane,
// planes peeled to 16-byte boundaries: it extracts every class three times, once per plane, and pays ~60 instructions of
// alignment / predication per plane; its writer waves alone took 17.6 us per step against 10.2 us for this form, the
// launch 26.0 against 24.0 us per step on the same box: profiles/r04_multi_group_probe.txt.)
template <int U, typename CT>
__device__ __forceinline__ void grp_emit_cells_chunk(grp_gfloat *blk, const CT *cg, const float *tab, u32 sh, int C,
                                                     int c0, bool stores)
{
    u32 off[U];
#pragma unroll
    for (int u = 0; u < U; ++u) off[u] = __builtin_amdgcn_ubfe((u32)cg[c0 + 64 * u], sh, 3u) << 2; // (reads past C: see GRP_CODE_SLACK)
    float r[U], g[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        r[u] = grp_tab(tab, off[u]);
        g[u] = grp_tab(tab + 8, off[u]);
        b[u] = grp_tab(tab + 16, off[u]);
    }
    typedef __attribute__((address_space(1))) char gchar;
#pragma unroll
    for (int u = 0; u < U; ++u) { // (unsigned 32-bit BYTE offsets off the uniform block pointer: global_store with an SGPR base)
        const u32 c = (u32)(c0 + 64 * u), o = 4u * c, pl = 4u * (u32)C;
        if (c < (u32)C && stores) {
            *(grp_gfloat *)((gchar *)blk + o) = r[u];
            *(grp_gfloat *)((gchar *)blk + (o + pl)) = g[u];
            *(grp_gfloat *)((gchar *)blk + (o + 2u * pl)) = b[u];
        }
    }
}

template <typename CT>
__device__ __forceinline__ void grp_emit_cells(grp_gfloat *blk, const CT *cg, const float *tab, u32 sh, int C, int lane,
                                               bool stores)
{
    const int cpl = (C + 63) >> 6;
    int k = 0;
    for (; k + 5 <= cpl; k += 5) grp_emit_cells_chunk<5, CT>(blk, cg, tab, sh, C, lane + 64 * k, stores);
    for (; k < cpl; ++k) grp_emit_cells_chunk<1, CT>(blk, cg, tab, sh, C, lane + 64 * k, stores);
}

// tab[plane][class]: the reference's colours / 255 (true divisions, as `.to(dtype) / 255` :281); the caller synchronises
__device__ __forceinline__ void grp_table_init(float *tab, int tid)
{
    if (tid < 24) {
        const int pl = tid >> 3, cls = tid & 7;
        const float G1 = 192.0f / 255.0f, G2 = 96.0f / 255.0f;
        float v = 0.0f;
        if (cls == 0) v = 1.0f;                              // background (255, 255, 255)
        else if (cls == 1) v = pl == 0 ? 1.0f : 0.0f;        // food (255, 0, 0)
        else if (cls == 2) v = pl == 1 ? G2 : 0.0f;          // own body (0, 96, 0)
        else if (cls == 3) v = pl == 1 ? G1 : 0.0f;          // own head (0, 192, 0)
        else if (cls == 4) v = pl == 2 ? G2 : 0.0f;          // other body (0, 0, 96)
        else if (cls == 5) v = pl == 2 ? G1 : 0.0f;          // other head (0, 0, 192)
        tab[pl * 8 + cls] = v;                               // 6: border (0, 0, 0)
    }
}

// per-call kernels: the nwaves waves of a workgroup write the observations of its nG consecutive envs (first env0), wave w
// the whole run of agent w (w + nwaves, ...); obs: this call's (K, N, 3 S^2) block
__device__ __forceinline__ void grp_emit_group(const MultiArgs &p, float *obs, long long env0, int nG, int wave, int nwaves,
                                               const unsigned char *codes0, int code_stride, const float *tab, int lane)
{
    const int C = p.S * p.S, K = p.K;
    // wave -> (agent, part of the envs): one agent after the other while there are at most as many waves as agents, else
    // nwaves / K waves per agent, each with its own contiguous part of the agent's run
    const int parts = nwaves > K ? nwaves / K : 1, part = nwaves > K ? wave / K : 0;
    const int g0 = part * nG / parts, g1 = (part + 1) * nG / parts;
    for (int a = nwaves > K ? wave % K : wave; a < K && part < parts; a += nwaves > K ? K : nwaves) {
        grp_gfloat *const run = (grp_gfloat *)uniform64((long long)(obs + ((long long)a * p.N + env0) * p.obs_elems));
        const u32 sh = 3u * (u32)a;
        for (int g = g0; g < g1; ++g) {
            const unsigned short *cg = (const unsigned short *)(codes0 + (size_t)g * code_stride);
            grp_emit_cells<unsigned short>(run + g * 3 * C, cg, tab, sh, C, lane, true);
        }
    }
}

// Work sharing between the waves of a group: the K * nG (agent, env) observation blocks of a step are ITEMS handed out by
// an LDS counter, in address order (agent-major: consecutive items are consecutive envs of one agent's run).  The writer
// waves take items from the barrier of step t on; a stepper wave joins in once it has finished its own step t + 1 — what
// the store path takes grows with the number of waves that have stores in flight (tools/microbench/store_window.hip: the
// same bytes at 4.7 / 5.2 / 5.7 / 6.3 TB/s from 4 / 8 / 16 / 32 storing waves per CU), and the steppers are idle for half
// of a step's period otherwise.
template <typename CT>
__device__ __forceinline__ void grp_take_items(const MultiArgs &p, int *ctr, const unsigned char *cbuf, long long t, long long env0,
                                               int nG, const float *tab, int lane, bool stores)
{
    const int C = p.S * p.S, K = p.K, items = K * nG;
    for (;;) {
        int i = 0;
        if (lane == 0) i = atomicAdd(ctr, 1);
        i = uniform(i);
        if (i >= items) break;
        const int a = i / nG, g = i - a * nG;
        grp_gfloat *const blk = (grp_gfloat *)uniform64((long long)(p.obs + ((t * K + a) * p.N + env0 + g) * p.obs_elems));
        grp_emit_cells<CT>(blk, (const CT *)(cbuf + (size_t)g * p.grp_code_bytes), tab, 3u * (u32)a, C, lane, stores);
    }
}

// Per-snake scalars of an env while its stepper wave works on another one (EPS > 1): 8 ints per snake in LDS
__device__ __forceinline__ void grp_save(int *sv, int lane, int K, const Snake &sn, bool col_dirty, int hc0)
{
    if (lane < K) {
        int *q = sv + 8 * lane;
        q[0] = sn.hc; q[1] = sn.L; q[2] = (int)sn.done | ((int)sn.boosted << 1) | ((int)col_dirty << 2); q[3] = (int)sn.orient;
        q[4] = (int)(unsigned short)sn.col[0] | ((int)(unsigned short)sn.col[1] << 16); q[5] = (int)sn.col[2]; q[6] = hc0;
    }
}

__device__ __forceinline__ void grp_restore(const int *sv, int lane, int K, Snake &sn, bool &col_dirty, int &hc0)
{
    sn.hc = -1; sn.L = 0; sn.done = true; sn.orient = 0; sn.boosted = false; sn.col[0] = sn.col[1] = sn.col[2] = 0;
    col_dirty = false; hc0 = -1;
    if (lane < K) {
        const int *q = sv + 8 * lane;
        sn.hc = q[0]; sn.L = q[1]; sn.done = (q[2] & 1) != 0; sn.boosted = (q[2] & 2) != 0; col_dirty = (q[2] & 4) != 0;
        sn.orient = q[3]; sn.col[0] = (short)(q[4] & 0xffff); sn.col[1] = (short)(q[4] >> 16); sn.col[2] = (short)q[5]; hc0 = q[6];
    }
}

} // namespace wurm
