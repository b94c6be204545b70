// multi_reset.hpp — MultiSnake.reset on the env in LDS (the per-call step applies a postponed one before its transition).
#pragma once
#include "multi_observe.hpp"

namespace wurm {

// ------------------------------------------------------------------------------------------------ reset

// availability of _add_snake (:927-941) / _get_snake_addition (:848-858): the 3x3 neighbourhood is empty and the
// cell is at least 2 from the border.  occ[] holds the occupancy (food, heads, bodies).
__device__ __forceinline__ u64 spawn_cells(const Ctx &cx)
{
    const int S = cx.S, C = cx.C, lane = cx.lane;
    u64 av = 0;
    for (int k = 0; k < cx.cpl; ++k) {
        int c = lane + 64 * k;
        if (c >= C) continue;
        int y = div_size(c, cx.rcpS), x = c - y * S;
        if (y < 2 || x < 2 || y > S - 3 || x > S - 3) continue;
        int any = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) any |= cx.occ[c + dy * S + dx];
        if (!any) av |= 1ull << k;
    }
    return av;
}

// occupancy of the env currently in LDS
__device__ __forceinline__ void build_occ(const Ctx &cx, int hc)
{
    const int C = cx.C, lane = cx.lane;
    for (int k = 0; k < cx.cpl; ++k) {
        int c = lane + 64 * k;
        if (c >= C) continue;
        bool o = cx.food[c] != 0;
#pragma unroll 4
        for (int s = 0; s < cx.K; ++s) o |= BV(cx, s, c) > 0;
        cx.occ[c] = (unsigned char)o;
    }
    wave_lds_sync();
    if (lane < cx.K && hc >= 0) cx.occ[hc] = 1;
    wave_lds_sync();
}

// The respawn search of respawn_mode = 'any' (:805-831 -> _get_snake_addition :848-858) on row masks: the K-th cell, in
// row-major order, that is at least 2 from the border with nothing (food, body, head) in its 3 x 3 neighbourhood, K =
// mulhi(word, number of such cells); -1 if there is none.  Same cells in the same order as build_occ + spawn_cells +
// rank_select — which read every (cell, snake) pair one by one: 420 LDS reads per lane at 10 snakes on 36 x 36, run in
// nearly every step of such an env (some snake is almost always dead), half of the transition's time there.  Here lane l
// reads cells 8 l .. 8 l + 7 of every run of 512 with one 16-byte read per snake, leaves one occupancy BIT per cell in the
// scratch byte map, and lane r assembles row r's 64-bit mask from it; the rest is the dilation / popcount walk that the
// rebuild of an env uses.  Needs S * S to be a multiple of 8 (16-byte aligned snake grids).
__device__ __forceinline__ int respawn_cell_rows(const Ctx &cx, int hc, u32 word)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    unsigned char *bm = cx.occ; // C bytes of scratch: C / 8 of bitmap, the rest zero padding for the row reads
    const int myT = lane < K ? cx.tclk[lane] : 0;
    for (int i = lane; i < (C >> 3) + 16 && i < C; i += 64) bm[i] = 0;
    wave_lds_sync();
    const int runs = (C + 511) >> 9;
    for (int r = 0; r < runs; ++r) {
        const int c0 = 512 * r + 8 * lane;
        if (c0 >= C) continue;
        const u64 f8 = *(const u64 *)(cx.food + c0);
        u32 o8 = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) o8 |= (u32)(((f8 >> (8 * j)) & 0xffull) != 0) << j;
        for (int s = 0; s < K; ++s) {
            const int T = lane_value(myT, s);
            const uint4 q = *(const uint4 *)(cx.body + s * C + c0);
            o8 |= (u32)((int)(q.x & VMASK) > T) | ((u32)((int)((q.x >> 16) & VMASK) > T) << 1) |
                  ((u32)((int)(q.y & VMASK) > T) << 2) | ((u32)((int)((q.y >> 16) & VMASK) > T) << 3) |
                  ((u32)((int)(q.z & VMASK) > T) << 4) | ((u32)((int)((q.z >> 16) & VMASK) > T) << 5) |
                  ((u32)((int)(q.w & VMASK) > T) << 6) | ((u32)((int)((q.w >> 16) & VMASK) > T) << 7);
        }
        bm[c0 >> 3] = (unsigned char)o8;
    }
    wave_lds_sync();
    if (lane < K && hc >= 0) atomicOr((u32 *)bm + (hc >> 5), 1u << (hc & 31)); // head cells (the map is 16-byte aligned)
    wave_lds_sync();
    u64 occ_row = 0;
    if (lane < S) { // bits lane * S .. lane * S + S - 1 of the map
        const int bit0 = lane * S, byte0 = bit0 >> 3, sh = bit0 & 7;
        u64 lo = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) lo |= (u64)bm[byte0 + i] << (8 * i);
        const u64 hi = bm[byte0 + 8];
        const u64 v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        occ_row = S == 64 ? v : v & ((1ull << S) - 1ull);
    }
    // available (:848-858): at least 2 from the border, nothing in the 3 x 3 neighbourhood
    const u64 h = occ_row | (occ_row << 1) | (occ_row >> 1);
    const u64 up = lane == 0 ? 0ull : (u64)__shfl_up((long long)h, 1);
    const u64 dn = lane == 63 ? 0ull : (u64)__shfl_down((long long)h, 1);
    const u64 cols = S >= 5 ? (((1ull << (S - 4)) - 1ull) << 2) : 0ull;
    const u64 av = (lane >= 2 && lane <= S - 3) ? (~(h | up | dn) & cols) : 0ull;
    const int cnt = popc64(av), n = wave_sum_i32(cnt);
    if (n == 0) return -1;
    int kth = (int)mulhi_range(word, (u32)n), r = 0;
    for (; r < S - 1; ++r) {
        const int c = lane_value(cnt, r);
        if (kth < c) break;
        kth -= c;
    }
    return r * S + nth_bit64((u64)lane_value64((long long)av, r), kth);
}

// writes a 3-segment snake `s` at `cell` heading `d` into LDS (body, occ); cell < 0: nothing
__device__ __forceinline__ int place_snake(const Ctx &cx, int s, int cell, int d)
{
    const int S = cx.S, C = cx.C;
    if (cell < 0) return -1;
    int sy = div_size(cell, cx.rcpS), sx = cell - sy * S;
    int hcell = (sy + tap_y(d)) * S + sx + tap_x(d), tcell = (sy - tap_y(d)) * S + sx - tap_x(d);
    if (cx.lane == 0) { // LENGTH_3_SNAKES (:965-973): 3 at seed + TAP[d], 2 at the seed, 1 at seed - TAP[d]
        cx.body[s * C + hcell] = (unsigned short)(3 | DIRTY);
        cx.body[s * C + cell] = (unsigned short)(2 | DIRTY);
        cx.body[s * C + tcell] = (unsigned short)(1 | DIRTY);
        cx.occ[hcell] = 1;
        cx.occ[cell] = 1;
        cx.occ[tcell] = 1;
    }
    wave_lds_sync();
    return hcell;
}

__device__ __forceinline__ void colour_from_words(const Words &w, short out[3])
{
    // get_n_colours (:163-169): rand(3); red / 1.5; normalise; * 192; .short()
    // plain `/` and sqrtf are the correctly rounded IEEE operations here (hipcc's default
    // -fhip-fp32-correctly-rounded-divide-sqrt); the __fdiv_rn / __fsqrt_rn intrinsics are NOT (found by
    // tools/fuzz_parity.py: one colour component in thousands came out one lower than on the CPU)
    float c0 = u01(w.w[0]) / 1.5f, c1 = u01(w.w[1]), c2 = u01(w.w[2]);
    float norm = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
    out[0] = (short)(c0 / norm * 192.0f);
    out[1] = (short)(c1 / norm * 192.0f);
    out[2] = (short)(c2 / norm * 192.0f);
}

// colours of snakes that are still dead are re-rolled on every reset (:800-803).  Returns true if sn.col changed.
__device__ __forceinline__ bool reroll_colour(const MultiArgs &p, long long agent, bool dead, u64 env_id, u64 call,
                                              long long offA, Snake &sn)
{
    if (!(p.cfg.colour_random && dead)) return false;
    if (p.has_rinj) {
        sn.col[0] = p.rinj.colours[(offA + agent) * 3];
        sn.col[1] = p.rinj.colours[(offA + agent) * 3 + 1];
        sn.col[2] = p.rinj.colours[(offA + agent) * 3 + 2];
    } else {
        colour_from_words(rng_words(p.seed, call, env_id, RNG_COLOUR, (u32)(threadIdx.x & 63u)), sn.col);
    }
    return true;
}

// a re-rolled colour to HBM (load_colour reads it back)
__device__ __forceinline__ void store_colour(const MultiArgs &p, long long agent, const Snake &sn)
{
    p.colours[agent * 3] = sn.col[0];
    p.colours[agent * 3 + 1] = sn.col[1];
    p.colours[agent * 3 + 2] = sn.col[2];
}

// The respawn search from the map of cell codes the step left (cell_codes + put_food: Snake::cmap_ok) — any state, any
// size: a cell is occupied iff its code is neither 0 nor the ring's (what sits ON the ring never matters: a spawn cell is
// at least 2 from the border, so its 3 x 3 neighbourhood stops at row / column 1).  Ten ballots give the occupancy of the
// 64-cell chunks, lane r cuts grid row r out of at most two of them, and the rest is the dilation / popcount walk of the
// rebuild: ~100 instructions for what build_occ + spawn_cells + rank_select read cell by cell — K clock compares and nine
// byte reads per cell, 5 100 of a step's 30 000 cycles with respawn_mode = 'any' (profiles/r05_kernel_timeline.txt: 2 850 now).
__device__ __forceinline__ int respawn_cell_codes(const Ctx &cx, const unsigned char *codes, u32 word)
{
    const int S = cx.S, C = cx.C, lane = cx.lane;
    u64 *chunks = (u64 *)cx.occ;   // scratch: cpl <= 64 masks of 64 cells (C bytes, 16-byte aligned; 8 cpl <= C for S >= 5)
    u64 mine = 0;
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = lane + 64 * k;
        const int code = c < C ? (int)codes[c] : PC_BG;
        const u64 m = ballot(code != PC_BG && code != PC_RING);
        if (lane == k) mine = m;
    }
    if (lane < cx.cpl) chunks[lane] = mine;
    wave_lds_sync();
    u64 occ_row = 0;
    if (lane < S) { // grid row `lane`: bits lane * S .. lane * S + S - 1 of the linear occupancy
        const int b = lane * S, q = b >> 6, off = b & 63;
        const u64 lo = chunks[q], hi = (q + 1 < cx.cpl) ? chunks[q + 1] : 0ull;
        occ_row = (lo >> off) | (off ? hi << (64 - off) : 0ull);
        if (S < 64) occ_row &= (1ull << S) - 1ull;
    }
    wave_lds_sync();
    // available (:848-858): at least 2 from the border, nothing in the 3 x 3 neighbourhood
    const u64 h = occ_row | (occ_row << 1) | (occ_row >> 1);
    const u64 up = lane == 0 ? 0ull : (u64)__shfl_up((long long)h, 1);
    const u64 dn = lane == 63 ? 0ull : (u64)__shfl_down((long long)h, 1);
    const u64 cols = S >= 5 ? (((1ull << (S - 4)) - 1ull) << 2) : 0ull;
    const u64 av = (lane >= 2 && lane <= S - 3) ? (~(h | up | dn) & cols) : 0ull;
    const int cnt = popc64(av), n = wave_sum_i32(cnt);
    if (n == 0) return -1;
    int kth = (int)mulhi_range(word, (u32)n), r = 0;
    for (; r < S - 1; ++r) { // the K-th available cell in row-major order
        const int c = lane_value(cnt, r);
        if (kth < c) break;
        kth -= c;
    }
    return r * S + nth_bit64((u64)lane_value64((long long)av, r), kth);
}

// the grid part of MultiSnake.reset on the env held in LDS: _create_envs (:996-1019) when `rebuild`, then the
// respawn of the first dead snake (:805-831) when `respawn`.  sn.done must already be false for rebuilt envs (:798).
__device__ __forceinline__ void multi_reset_grid(const Ctx &cx, const MultiArgs &p, long long env, u64 env_id, u64 call,
                                                 bool rebuild, bool respawn, Snake &sn, bool &orient_dirty,
                                                 long long offA, long long offE)
{
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    const bool had_map = sn.cmap_ok && !rebuild; // the step's map of cell codes still describes the grids the respawn looks at
    sn.cmap_ok = false; // (... but not the state this reset leaves)
    if (rebuild) { // _create_envs (:996-1019)
        { // value 0; a cell that ever held one stays marked.  Four cells per access: the grids start on a 16-byte
          // boundary and are followed by padding up to the next one, so the last access may run into the padding.
            u64 *b8 = (u64 *)cx.body;
            const u64 keep = (u64)DIRTY * 0x0001000100010001ull;
            for (int i = lane; i < (K * C + 3) >> 2; i += 64) b8[i] &= keep;
        }
        for (int k = 0; k < cx.cpl; ++k) {
            int c = lane + 64 * k;
            if (c < C) { cx.food[c] = 0; cx.occ[c] = 0; cx.hmap[c] = 0; }
        }
        if (snake) cx.tclk[lane] = 0;
        wave_lds_sync();
        sn.hc = -1;
        // RNG mode: the env is empty, so the occupancy is just the cells of the snakes placed so far — one 64-bit row
        // mask per lane (lane r = row r) instead of the byte map: "3x3 neighbourhood empty" is a dilation (two shifts
        // and the rows above / below), the count a popcount, the K-th free cell in row-major order a walk over the
        // rows' counts.  Same cells as spawn_cells / count_bits / rank_select (measured: a rebuilt env took 52 000
        // cycles of a 35 000-cycle step launch, and the launch waits for its slowest env).
        const int S = cx.S;
        u64 occ_row = 0;
        auto pick = [&](u64 av, u32 word) -> int { // K-th set bit over the rows, K = mulhi(word, total)
            const int cnt = popc64(av), n = wave_sum_i32(cnt);
            if (n == 0) return -1;
            int kth = (int)mulhi_range(word, (u32)n), r = 0;
            for (; r < S - 1; ++r) {
                const int c = lane_value(cnt, r);
                if (kth < c) break;
                kth -= c;
            }
            return r * S + nth_bit64((u64)lane_value64((long long)av, r), kth);
        };
        auto mark = [&](int cell) {
            const int y = div_size(cell, cx.rcpS), x = cell - y * S;
            if (lane == y) occ_row |= 1ull << x;
        };
        // all the draws of the rebuild in one Philox evaluation: lane s < K takes the spawn block of snake s, lane K
        // the block the food cell comes from (K = 64: there is no such lane, the food block is drawn on its own)
        Words draws;
        draws.w[0] = draws.w[1] = draws.w[2] = draws.w[3] = 0;
        if (!p.has_rinj)
            draws = rng_words(p.seed, call, env_id, lane < K ? RNG_SPAWN : RNG_RESET, lane < K ? (u32)lane : 0u);
        for (int s = 0; s < K; ++s) { // _add_snake (:911-994), one snake after another
            int cell = -1, dnew = 0;
            if (p.has_rinj) {
                cell = p.rinj.create[(offA + env * K + s) * 2];
                dnew = p.rinj.create[(offA + env * K + s) * 2 + 1];
            } else {
                Words w;
                w.w[0] = (u32)lane_value((int)draws.w[0], s);
                w.w[1] = (u32)lane_value((int)draws.w[1], s);
                dnew = (int)(w.w[1] >> 30);
                // available (:927-941): at least 2 from the border, nothing in the 3x3 neighbourhood
                const u64 h = occ_row | (occ_row << 1) | (occ_row >> 1);
                const u64 up = lane == 0 ? 0ull : (u64)__shfl_up((long long)h, 1);
                const u64 dn = lane == 63 ? 0ull : (u64)__shfl_down((long long)h, 1);
                const u64 cols = S >= 5 ? (((1ull << (S - 4)) - 1ull) << 2) : 0ull;
                const u64 av = (lane >= 2 && lane <= S - 3) ? (~(h | up | dn) & cols) : 0ull;
                cell = pick(av, w.w[0]);
            }
            cell = uniform(cell);
            if (cell < 0 && p.status && lane == 0) atomicAdd(p.status, 1); // the reference raises (:946-947)
            int h = place_snake(cx, s, cell, dnew);
            if (cell >= 0 && !p.has_rinj) {
                const int sy = div_size(cell, cx.rcpS), sx = cell - sy * S;
                mark(cell);
                mark((sy + tap_y(dnew)) * S + sx + tap_x(dnew));
                mark((sy - tap_y(dnew)) * S + sx - tap_x(dnew));
            }
            if (lane == s) {
                sn.hc = h;
                sn.L = h >= 0 ? 3 : 0;
                sn.orient = dnew;
                orient_dirty = true;
            }
        }
        { // food (:1016-1017)
            if (p.has_rinj) {
                int cell = p.rinj.create_food[offE + env];
                if (cell >= 0 && cell < C && lane == 0) cx.food[cell] = 1;
            } else { // free (:439-445): not on the border ring, nothing on it
                const u64 cols = ((1ull << (S - 2)) - 1ull) << 1;
                const u64 fr = (lane >= 1 && lane <= S - 2) ? (~occ_row & cols) : 0ull;
                const u32 word = K < 64 ? (u32)lane_value((int)draws.w[3], K)
                                        : rng_words(p.seed, call, env_id, RNG_RESET, 0).w[3];
                const int cell = pick(fr, word);
                if (cell >= 0 && lane == 0) cx.food[cell] = 1;
            }
            wave_lds_sync();
        }
    }
    if (respawn) { // :805-831 the first dead snake of the env respawns if there is room
        const int f = first_bit(ballot(snake && sn.done));
        int cell = -1, dnew = 0;
        if (p.has_rinj) {
            build_occ(cx, sn.hc);
            cell = p.rinj.respawn[(offE + env) * 2];
            dnew = p.rinj.respawn[(offE + env) * 2 + 1];
        } else {
            Words w = rng_words(p.seed, call, env_id, RNG_SPAWN, (u32)K);
            dnew = (int)(w.w[1] >> 30);
            if (had_map) {
                cell = respawn_cell_codes(cx, cx.hmap, w.w[0]);
            } else if (p.obs_mode == WURM_OBS_PARTIAL) {
                // no map of this state yet (the postponed reset in front of a per-call step: the launch has just loaded the
                // env): one scan builds it — 4 100 cycles + 2 500 for the search, where build_occ + spawn_cells + rank_select
                // below took 23 000 in every env with a dead snake, and the launch ends with its slowest wave
                // (profiles/r06_kernel_timeline_multi.txt).  hmap is the crops' map of cell codes in such a launch anyway (the one-env-per-
                // workgroup kernels, which keep flags in it, never write crops).
                (void)cell_codes(cx, sn.hc, cx.hmap, cx.has_ring ? cx.ring : border_bits(cx));
                cell = respawn_cell_codes(cx, cx.hmap, w.w[0]);
            } else if ((C & 7) == 0) {
                cell = respawn_cell_rows(cx, sn.hc, w.w[0]);
            } else {
                build_occ(cx, sn.hc);
                u64 av = spawn_cells(cx);
                int n = count_bits(cx, av);
                if (n > 0) cell = selected_cell(rank_select(cx, av, (int)mulhi_range(w.w[0], (u32)n)));
            }
        }
        cell = uniform(cell);
        // bodies[first] = new_bodies (:826): the dead snake's grid is replaced (it reads all-zero in consistent
        // states: its clock is CLOCK_DEAD) and its clock restarts
        for (int k = 0; k < cx.cpl; ++k) {
            int c = lane + 64 * k;
            if (c < C && (cx.body[f * C + c] & VMASK)) cx.body[f * C + c] = DIRTY;
        }
        if (lane == f) cx.tclk[lane] = 0;
        wave_lds_sync();
        int h = place_snake(cx, f, cell, dnew);
        if (lane == f) {
            sn.hc = h;
            sn.L = h >= 0 ? 3 : 0;
            sn.orient = dnew;     // :828 assigned whether or not the snake found room
            orient_dirty = true;
            sn.done = cell < 0;   // :829
        }
    }
    if (snake) cx.hcell[lane] = sn.hc;
    wave_lds_sync();
}

} // namespace wurm
