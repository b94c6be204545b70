// multi_step.hpp — MultiSnake.step on the env in LDS: the transition every kernel that steps an env runs (multi_snake.hip:
// the per-call step and the rollouts; multi_frames.hpp: the replay of a window for its frames).
#pragma once
#include "multi_reset.hpp"

namespace wurm {

// ------------------------------------------------------------------------------------------------ step

// MultiSnake.step (:462-731) of the env held in LDS.  `a` is this lane's (snake's) action.  offC / offA / offE are the
// offsets of this step's slice in the injected-outcome arrays (0 for a single step; t*N*C, t*N*K, t*N in a rollout).
__device__ __forceinline__ void multi_step_body(const Ctx &cx, const MultiArgs &p, long long env, u64 env_id, u64 call,
                                                long long a, Snake &sn, StepRes &res, long long offC, long long offA,
                                                long long offE)
{
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    int hc = sn.hc, L = sn.L;
    bool done = sn.done;
    bool has_body = L > 0;
    const long long agent = env * K + lane;

    // prologue (:475-502)
    const bool done0 = done;
    long long orient = sn.orient;
    long long d = a % 4;                        // :483
    const bool boost_act = a > 3;               // :484
    if (orient == d) d = (d + 2) % 4;           // :493 sanitize_movements
    orient = (d + 2) % 4;                       // :494
    const int dir = (int)(((d % 4) + 4) % 4);
    const bool boosted = snake && boost_act && L >= 4; // :497-499
    float reward = 0.0f, foodcons = 0.0f;
    bool snakecol = false, edgecol = false;

    if (p.cfg.boost && ballot(boosted) != 0) {  // :503 (per env; the batch-global gate has no per-env effect)
        run_phase(cx, boosted, dir, hc, L, done, reward, foodcons, snakecol, edgecol);
        if (p.cfg.food_on_death)                // :565-576
            food_from_death(cx, done, has_body, p.has_inj ? p.inj.death_a + offC + env * C : nullptr,
                            p.cfg.death_threshold, p.seed, call, env_id, RNG_DEATH_FOOD_A);
        // boost cost (:579-592): tail cell becomes food, body decays, reward -1
        bool pay = false;
        if (boosted) {
            if (p.has_inj) pay = p.inj.cost[offA + agent] != 0;
            else pay = u01(rng_words(p.seed, call, env_id, RNG_BOOST_COST, (u32)lane).w[0]) < p.cfg.boost_cost_prob;
        }
        u64 m = ballot(pay);
        while (m) { // the tail cell (value 1) becomes food; the decay itself is the clock
            int s = first_bit(m);
            m &= m - 1;
            const unsigned short *b = cx.body + s * C;
            const int tail = cx.tclk[s] + 1;
            for (int k = 0; k < cx.cpl; ++k) {
                int c = lane + 64 * k;
                if (c < C && (int)(b[c] & VMASK) == tail) cx.food[c] = 1;
            }
        }
        if (pay) {
            cx.tclk[lane] += 1;
            reward -= 1.0f;
            L -= 1;
        }
        wave_lds_sync();
        delete_done(cx, done, has_body, hc);    // :595-596
    }

    WURM_TLS(cx, 3);
    run_phase(cx, snake, dir, hc, L, done, reward, foodcons, snakecol, edgecol); // :613-660
    WURM_TLS(cx, 4);
    int doubled_b = 0;                          // (food cells the sum of :382 sees twice: food_from_death)
    if (p.cfg.food_on_death)                    // :662-673
        doubled_b = food_from_death(cx, done, has_body, p.has_inj ? p.inj.death_b + offC + env * C : nullptr,
                                    p.cfg.death_threshold, p.seed, call, env_id, RNG_DEATH_FOOD_B);
    delete_done(cx, done, has_body, hc);        // :676-677
    WURM_TLS(cx, 5);

    // _add_food (:368-410)
    bool cmap_ok = false;
    {
        // The map of cell codes (cell_codes: one scan of the K grids) serves both "which interior cells are free" here and the
        // crops of observe_partial, and counts the food and the free cells on the way; it lives where observe_full keeps its
        // head map, so only launches without 'full' observations build it — a launch that writes crops every step, one
        // without observations when food has to be placed.
        CellCounts cc;
        cc.free = 0;
        cc.nfree = -1;
        int nfood;
        if (p.obs_mode == WURM_OBS_PARTIAL && cx.has_ring) {
            cc = cell_codes(cx, hc, cx.hmap, cx.ring);
            cmap_ok = true;
            nfood = cc.nfood + doubled_b;
        } else {
            nfood = food_count(cx) + doubled_b;
            const bool want_free = p.cfg.food_mode == 0 ? (nfood == 0 && !p.has_inj) : nfood < p.cfg.max_food;
            if (p.obs_mode == WURM_OBS_NONE && cx.has_ring && want_free) {
                cc = cell_codes(cx, hc, cx.hmap, cx.ring);
                cmap_ok = true;
            }
        }
        WURM_TLS(cx, 10);
        if (p.cfg.food_mode == 0) {
            if (nfood == 0) {                   // :371-379
                if (p.has_inj) {
                    int cell = p.inj.food_cell[offE + env];
                    if (cell >= 0 && cell < C && lane == 0) put_food(cx, cell, cmap_ok);
                } else {
                    u64 fr = cmap_ok ? cc.free : free_cells(cx, hc, 1);
                    int nf = cmap_ok ? cc.nfree : count_bits(cx, fr);
                    if (nf > 0) {
                        int Kr = (int)mulhi_range(rng_words(p.seed, call, env_id, RNG_FOOD, 0).w[0], (u32)nf);
                        int k = rank_select(cx, fr, Kr);
                        if (k >= 0) put_food(cx, lane + 64 * k, cmap_ok);
                    }
                }
            }
        } else if (nfood < p.cfg.max_food) {    // :382-408
            u64 fr = cmap_ok ? cc.free : free_cells(cx, hc, 1);
            WURM_TLS(cx, 11);
            if (p.has_inj) {
                for (int k = 0; k < cx.cpl; ++k)
                    if (((fr >> k) & 1) && p.inj.rate[offC + env * C + lane + 64 * k] != 0) put_food(cx, lane + 64 * k, cmap_ok);
            } else {
                // Every free cell spawns food independently with probability food_rate (:401-408).  RNG mode draws the NUMBER
                // of cells — Binomial(n free, food_rate) by inversion from ONE uniform — and then that many distinct cells,
                // the j-th as the mulhi(word, n - j)-th remaining free cell in row-major order: the same distribution as n
                // independent draws (this build's own RNG specification, oracle/multi_snake.c step_env), for one Philox block
                // per env-step instead of one per four cells and lane (625 draws to place 0.13 foods on average at cfg4').
                const int nf = cmap_ok ? cc.nfree : count_bits(cx, fr);
                const float pw = pow_n(1.0f - p.cfg.food_rate, nf);
                if (!(p.cfg.food_rate > 0.0f) || pw < BINOMIAL_MIN_P0) {
                    // P(no food) too small for the recurrence (rates far above the reference's): cell by cell — the cells
                    // lane + 64k, k = 4j .. 4j+3, share Philox block j of this lane (word k & 3)
                    for (int j = 0; 4 * j < cx.cpl; ++j) {
                        const u32 four = (u32)(fr >> (4 * j)) & 15u;
                        if (!four) continue;
                        const Words w = rng_words(p.seed, call, env_id, RNG_RATE_FOOD, ((u32)j << 6) | (u32)lane);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (((four >> q) & 1u) && u01(w.w[q]) < p.cfg.food_rate) put_food(cx, lane + 64 * (4 * j + q), cmap_ok);
                    }
                } else {
                    Words w = rng_words(p.seed, call, env_id, RNG_RATE_FOOD, 0);
                    const int kf = uniform(binomial_inverse(nf, p.cfg.food_rate, pw, u01(w.w[0])));
                    WURM_TLS(cx, 12);
                    for (int j = 0; j < kf; ++j) {
                        const int wi = j + 1;
                        if ((wi & 3) == 0) w = rng_words(p.seed, call, env_id, RNG_RATE_FOOD, (u32)(wi >> 2));
                        const u32 wj = (wi & 3) == 0 ? w.w[0] : (wi & 3) == 1 ? w.w[1] : (wi & 3) == 2 ? w.w[2] : w.w[3];
                        const int Kr = (int)mulhi_range(wj, (u32)(nf - j));
                        const int k = rank_select(cx, fr, Kr);
                        if (k >= 0) {
                            put_food(cx, lane + 64 * k, cmap_ok);
                            fr &= ~(1ull << k);
                        }
                    }
                }
            }
        }
        wave_lds_sync();
    }

    WURM_TLS(cx, 6);
    if (snake && done && !done0) reward += p.cfg.reward_on_death; // :683-685

    sn.hc = hc;
    sn.L = L;
    sn.done = done;
    sn.orient = orient;
    sn.boosted = boosted;
    sn.cmap_ok = cmap_ok;
    res.reward = reward;
    res.foodcons = foodcons;
    res.snakecol = snakecol;
    res.edgecol = edgecol;
    res.all_done = ballot(snake && !done) == 0; // :703
    if (snake) cx.hcell[lane] = hc;
    wave_lds_sync();
}

} // namespace wurm
