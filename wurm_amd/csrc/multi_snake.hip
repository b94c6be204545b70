// multi_snake.hip — gfx950 kernels and C-ABI entry points for MultiSnake.
//
// Replaces (citations into oscarknagg/wurm):
//   MultiSnake.step     wurm/envs/multi_snake.py:462-731   two phases (boost, regular) of move / eat / decay /
//                       collide / grow / edge, food-on-death, boost cost, food respawn, death reward
//   MultiSnake._observe wurm/envs/multi_snake.py:175-227,268-334   'full' (per-agent RGB) and 'partial_n'
//   MultiSnake.reset    wurm/envs/multi_snake.py:771-1019  env re-creation, colour re-roll, respawn 'any'
//   check_consistency   wurm/envs/multi_snake.py:733-769
// The reference runs these as conv2d / einsum / repeat_interleave(xK) / masked scatter sequences with many host
// syncs; here each call is ONE launch, one env per wavefront, runtime K and S:
//   * the env's K body grids live in LDS as 16-bit cells [K][S*S] (bit 15 = "must be written back"), the food grid
//     as bytes; lane l owns cells l + 64k of every grid, so HBM traffic is coalesced dword runs and every grid
//     update is a conflict-free LDS access;
//   * a body cell holds an EXPIRY CLOCK, not a value: value = max(ex - T_s, 0) with one clock T_s per snake.  "Every
//     body cell of a mover decays by one" (:523-526 / :627-628) is T_s += 1, deleting a dead snake (:595-596 /
//     :676-677) is T_s = CLOCK_DEAD — no pass over the grid; only the new head segment is written;
//   * per-SNAKE scalars (head cell, length, done, orientation, reward ...) live one per lane in lanes 0..K-1, so
//     the snake-level logic of all K snakes runs in parallel and exchanges values with shuffles / ballots;
//   * cross-cell lookups (food under a head, bodies under a head) are single LDS reads at the head cell.
// Integer/index work: no MFMA.  Bound: HBM ((1+2K)*S*S*4 B read + observation written per env-step).
// The device functions are in headers by role, each in front of what calls it (no declaration ahead of a definition):
// multi_device.hpp, multi_observe.hpp (the observation writers), multi_reset.hpp, multi_step.hpp (the transition, which the
// frame replay of multi_frames.hpp runs too).  Here: the glue of a
// step, every __global__ kernel, which kernel serves a call (multi_plan), its launch, and the extern "C" entry points.
// Phases that several kernels run the same way are written once: kernel_args (a kernel's prologue), clear_snake_slots (an
// env about to be rebuilt) and store_moved_head in multi_device.hpp, store_colour in multi_reset.hpp.
// The entry, the action staging, the reset after a step and the exit of the two rollouts, the check mask behind obs_after
// and the Snake initialisation of the reset kernels are still written per kernel: DESIGN.md section 4 says why.
#include <cstdio>

#include "multi_step.hpp"

namespace wurm {

// foods / heads / bodies from the mirror (lazy form), no LDS: one workgroup per env
__global__ __launch_bounds__(256) void multi_flush_kernel(MultiArgs p)
{
    const long long env = blockIdx.x;
    const int C = p.S * p.S, K = p.K, KC = K * C, tid = (int)threadIdx.x, nth = (int)blockDim.x;
    const unsigned char *m = p.resident + env * mirror_env_bytes(K, C);
    const unsigned short *mb = (const unsigned short *)m;
    const unsigned char *mf = m + mirror_body_bytes(K, C);
    const int *ms = (const int *)(m + mirror_body_bytes(K, C) + mirror_food_bytes(C));
    float *foodp = p.foods + env * C, *headp = p.heads + env * KC, *bodyp = p.bodies + env * KC;
    const float rcpC = 1.0f / (float)C;
    for (int i = tid; i < KC; i += nth) {
        const int s = div_size(i, rcpC);
        bodyp[i] = (float)max((int)(mb[i] & VMASK) - ms[s], 0);
        headp[i] = (i - s * C == ms[K + s]) ? 1.0f : 0.0f;
    }
    for (int c = tid; c < C; c += nth) foodp[c] = mf[c] ? 1.0f : 0.0f;
}

// check_consistency (:733-769) of the env as it sits in LDS — the masks of multi_check_kernel, for an image that came from
// the mirror or from a rebuild (16-bit clocks, one head cell per snake, food bytes 0 / 1: what the fp32 planes could
// additionally hold — several heads, fractional values — cannot occur there).  ONE wave; sn = the snakes' scalars.
// one snake's share: its verdict bits; occ / over collect the overlap test (bit 8 r + j of a lane's occ: cell
// 512 r + 8 lane + j holds a body value of a snake seen so far; at most 8 runs: C <= 4096)
__device__ __forceinline__ uint32_t lds_check_snake(const Ctx &cx, int s, int hc, bool dead, u64 &occ, int &over)
{
    const int C = cx.C, lane = cx.lane;
    // lane l owns cells 8 l .. 8 l + 7 of every run of 512: one 16-byte LDS read per run and snake.  The body grids start
    // on a 16-byte boundary (multi_layout) and snake s's at 2 s C bytes behind it: aligned for every s only if C is a
    // multiple of 8 — else the cells are read one by one
    const int runs = (C + 511) >> 9;
    const bool wide = (C & 7) == 0;
    const int T = cx.tclk[s];
    const unsigned short *b = cx.body + s * C;
    uint32_t m = 0;
    int bs = 0, bm = 0;
    for (int r = 0; r < runs; ++r) {
        const int c0 = 512 * r + 8 * lane;
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0; // (scalars, not an array: an indexed local array ends up in scratch)
        if (wide) {
            if (c0 < C) {
                const uint4 q = *(const uint4 *)(b + c0);
                w0 = q.x; w1 = q.y; w2 = q.z; w3 = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < C) {
                    const u32 v16 = (u32)b[c0 + j] << (16 * (j & 1));
                    if ((j >> 1) == 0) w0 |= v16;
                    else if ((j >> 1) == 1) w1 |= v16;
                    else if ((j >> 1) == 2) w2 |= v16;
                    else w3 |= v16;
                }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u32 word = (j >> 1) == 0 ? w0 : (j >> 1) == 1 ? w1 : (j >> 1) == 2 ? w2 : w3;
            const int v = max((int)((word >> (16 * (j & 1))) & VMASK) - T, 0);
            bs += v;
            bm = max(bm, v);
            const u64 bit = 1ull << (8 * r + j);
            if (v > 0) {
                over |= (int)((occ & bit) != 0);
                occ |= bit;
            }
        }
    }
    const int t_bs = wave_sum_i32(bs), t_bm = wave_max_i32(bm);
    if (dead) {
        if (t_bs > 0 || hc >= 0) m |= WURM_MCHK_DEAD_NONZERO;
    } else {
        const int t_hb = hc >= 0 ? BV(cx, s, hc) : 0, t_hf = hc >= 0 ? (int)cx.food[hc] : 0;
        if (hc < 0) m |= WURM_CHK_ONE_HEAD;
        if (!(t_bs > 0)) m |= WURM_CHK_HAS_SNAKE;
        if (t_bm != t_hb) m |= WURM_CHK_HEAD_AT_END;
        if (2 * t_bs != t_bm * (t_bm + 1)) m |= WURM_CHK_BODY_RANGE;
        if (!(t_bs >= 6)) m |= WURM_CHK_MIN_LENGTH;
        if (t_hf != 0) m |= WURM_CHK_HEAD_ON_FOOD;
    }
    return m;
}

__device__ __forceinline__ uint32_t lds_check(const Ctx &cx, const Snake &sn)
{
    uint32_t m = 0;
    u64 occ = 0;
    int over = 0;
    for (int s = 0; s < cx.K; ++s)
        m |= lds_check_snake(cx, s, lane_value(sn.hc, s), lane_value((int)sn.done, s) != 0, occ, over);
    if (ballot(over != 0)) m |= WURM_MCHK_OVERLAP;
    return m;
}

// The same by the `nw` waves of a workgroup (multi_step_wg_kernel): wave w takes snakes w, w + nw, ...; head cells from
// cx.hcell, the done flags from cx.lmax (the caller parks them there); `scratch`: 8 * 64 * nw + 8 * nw bytes of LDS that
// nobody else uses right now.  Every thread of the workgroup calls it; the same value comes back in all of them.
__device__ __forceinline__ uint32_t wg_lds_check(const Ctx &cx, int wave, int nw, unsigned char *scratch)
{
    const int lane = cx.lane;
    u64 *occs = (u64 *)scratch;                  // [nw][64]
    u32 *flags = (u32 *)(scratch + 512 * nw);    // [nw][2]: verdict bits, overlap inside the wave's own snakes
    uint32_t m = 0;
    u64 occ = 0;
    int over = 0;
    for (int s = wave; s < cx.K; s += nw) m |= lds_check_snake(cx, s, cx.hcell[s], cx.lmax[s] != 0, occ, over);
    occs[wave * 64 + lane] = occ;
    if (lane == 0) { flags[2 * wave] = m; flags[2 * wave + 1] = 0; }
    if (ballot(over != 0) && lane == 0) flags[2 * wave + 1] = 1;
    __syncthreads();
    uint32_t total = 0;
    u64 seen = 0;
    int cross = 0;
    for (int w = 0; w < nw; ++w) {
        total |= flags[2 * w] | (flags[2 * w + 1] ? WURM_MCHK_OVERLAP : 0u);
        const u64 o = occs[w * 64 + lane];
        cross |= (int)((seen & o) != 0);
        seen |= o;
    }
    if (ballot(cross != 0)) total |= WURM_MCHK_OVERLAP;
    __syncthreads();
    return total;
}

constexpr uint32_t MCHK_NOT_COMPUTED = 0xffffffffu; // read from fp32 planes that hold what the image cannot: run multi_check_kernel

// The part of the per-call step between the load and the store of the env (LDS state ready, hcell / lmax / tclk set):
// [the reset(done) the caller postponed, exactly multi_reset_kernel without observation, with its own counter,] the
// transition, and the per-agent outputs.  Runs on ONE wave.  hc0: the head cells HBM holds (sparse write-back).
// what step_middle reads from global memory before anything else: a kernel requests it at its entry, together with the
// env's image, so that the transition does not start with a memory round trip of its own (2 400 of a stepper's 67 000 cycles
// per call at cfg4: tools/multi_timeline.py)
struct StepIn {
    bool done;
    long long orient, a;
    short col[3];
};

__device__ __forceinline__ void step_inputs(const MultiArgs &p, long long env, int lane, StepIn &in)
{
    const bool snake = lane < p.K;
    const long long agent = env * p.K + lane;
    in.done = snake ? p.dones[agent] != 0 : true;
    in.orient = snake ? p.orientations[agent] : 0;
    in.a = snake ? p.actions[(long long)lane * p.N + env] : 0;
    Snake c;
    load_colour(p, agent, snake && (p.done_env != nullptr || p.obs_mode == WURM_OBS_PARTIAL), c);
    in.col[0] = c.col[0]; in.col[1] = c.col[1]; in.col[2] = c.col[2];
}

__device__ __forceinline__ void step_middle(const Ctx &cx, const MultiArgs &p, long long env, bool rebuild, Snake &sn,
                                            StepRes &r, int &hc0, const StepIn *in = nullptr)
{
    const int K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    const u64 env_id = (u64)(p.env_offset + env);
    const long long agent = env * K + lane;
    sn.hc = snake ? cx.hcell[lane] : -1;
    sn.L = snake ? cx.lmax[lane] : 0;
    sn.done = in ? in->done : snake ? p.dones[agent] != 0 : true;
    sn.orient = in ? in->orient : snake ? p.orientations[agent] : 0;
    sn.boosted = false;
    hc0 = sn.hc;
    if (p.done_env != nullptr) {
        if (rebuild) sn.done = false; // :798
        if (in) { sn.col[0] = in->col[0]; sn.col[1] = in->col[1]; sn.col[2] = in->col[2]; }
        else load_colour(p, agent, snake, sn);
        if (snake && reroll_colour(p, agent, sn.done, env_id, p.pre_call, 0, sn)) store_colour(p, agent, sn);
        const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
        if (rebuild || respawn) {
            bool orient_dirty = false;
            multi_reset_grid(cx, p, env, env_id, p.pre_call, rebuild, respawn, sn, orient_dirty, 0, 0);
        }
    } else {
        if (in) { sn.col[0] = in->col[0]; sn.col[1] = in->col[1]; sn.col[2] = in->col[2]; }
        else load_colour(p, agent, snake && p.obs_mode == WURM_OBS_PARTIAL, sn);
    }
    const long long a = in ? in->a : snake ? p.actions[(long long)lane * p.N + env] : 0;
    WURM_TLS(cx, 2);
    multi_step_body(cx, p, env, env_id, p.call, a, sn, r, 0, 0, 0);
    WURM_TLS(cx, 7);

    // outputs (:701-729)
    if (snake) {
        p.dones[agent] = (uint8_t)sn.done;
        p.orientations[agent] = sn.orient;
        p.boost[agent] = (uint8_t)sn.boosted;
        p.rewards[agent] = r.reward;
        p.snakecol[agent] = (uint8_t)r.snakecol;
        p.edgecol[agent] = (uint8_t)r.edgecol;
        p.foodcons[agent] = r.foodcons;
        p.sizes[agent] = (float)sn.L;
        if (p.am_f32) { // agent-major copies: row i = agent_i over all envs
            const long long KN = (long long)K * p.N, am = (long long)lane * p.N + env;
            p.am_f32[am] = r.reward;
            p.am_f32[KN + am] = r.foodcons;
            p.am_f32[2 * KN + am] = (float)sn.L;
            p.am_u8[am] = (uint8_t)sn.done;
            p.am_u8[KN + am] = (uint8_t)sn.boosted;
            p.am_u8[2 * KN + am] = (uint8_t)r.snakecol;
            p.am_u8[3 * KN + am] = (uint8_t)r.edgecol;
        }
    }
    if (lane == 0) {
        p.all_done[env] = (uint8_t)r.all_done;
        if (p.all_done_copy) p.all_done_copy[env] = (uint8_t)r.all_done;
    }
}

// What reset(dones['__all__']) will do (multi_reset_kernel with done_env = all_done, call + 1), applied to the LDS copy
// only: the caller postpones that reset into the next launch, which recreates it from the same counters.  ONE wave.
// Returns whether the env was rebuilt or a snake respawned (else the grids are as the step left them).
__device__ __forceinline__ bool reset_for_obs_after(const Ctx &cx, const MultiArgs &p, long long env, Snake &sn,
                                                    const StepRes &r)
{
    const bool snake = cx.lane < cx.K;
    const u64 env_id = (u64)(p.env_offset + env);
    const bool rebuild_after = r.all_done;
    if (rebuild_after) sn.done = false; // :798
    // :800-803 the colours of snakes that are still dead are re-rolled (registers only; they matter to 'partial_n')
    if (p.obs_mode == WURM_OBS_PARTIAL)
        reroll_colour(p, env * cx.K + cx.lane, snake && sn.done, env_id, p.call + 1ull, 0, sn);
    const bool respawn_after = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
    if (rebuild_after || respawn_after) {
        bool orient_dirty = false;
        multi_reset_grid(cx, p, env, env_id, p.call + 1ull, rebuild_after, respawn_after, sn, orient_dirty, 0, 0);
    }
    return rebuild_after || respawn_after;
}

// (LDS written by some waves of a workgroup and read by others)
__device__ __forceinline__ void workgroup_handoff()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// `p.grp_emit` (large batches, 'full' observations of at most 5 snakes, several envs per workgroup): the waves of the
// workgroup first step their envs, then write the observations TOGETHER — wave w writes agent w's view of all the
// workgroup's envs, one linear run (class codes + colour table: see multi_rollout_group_kernel).
// INJ / OBS: as multi_rollout_kernel — a launch that draws its own random outcomes, with the observation mode a constant.
// (a shape-specialised instantiation keeps to 128 VGPRs: 4 096 envs are one round of waves at 4 per SIMD, not two at 3)
template <bool INJ = true, int OBS = -1, int KT = 0, int ST = 0, int NT = -1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(KT > 0 ? 4 : 1))) void multi_step_kernel(MultiArgs p_in)
{
    const MultiArgs p = kernel_args<INJ, OBS, KT, ST, NT>(p_in, true);
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env0 = xcd_block(blockIdx.x, gridDim.x) * wpb, env = env0 + wave;
    const bool grouped = p.grp_emit != 0;
    float *const tab = (float *)(wurm_multi_lds + p.grp_env0); // (grouped: the colour table behind the envs' blocks)
    const bool solo = p.grp_emit == 2; // every wave writes its own env's views
    if (grouped) {
        if (env0 >= p.N) return;
        grp_table_init(tab, (int)threadIdx.x);
        // (solo: the table is handed over HERE, where the workgroup's waves still run together — a barrier behind the step
        // would wait for the slowest of its envs)
        if (solo) workgroup_handoff();
    } else if (env >= p.N) return;
    const bool active = env < p.N;
    if (solo && !active) return;
    const Ctx cx = make_ctx(p, wave, 0, p.obs_mode != WURM_OBS_DEFAULT); // (the ring bits: multi_step_body's map of cell codes)
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    const int nG = (int)min((long long)wpb, p.N - env0);
    WURM_TLS_INIT(cx);
    WURM_TLS(cx, 0);
    const u64 ring = grouped ? border_bits(cx) : 0ull;
    Snake sn;
    StepRes r;
    bool clean = false;
    uint32_t m_step = MCHK_NOT_COMPUTED;
    float *foodp = nullptr, *headp = nullptr, *bodyp = nullptr;
    const bool mirrored = p.resident != nullptr, lazy = mirrored && p.resident_lazy != 0;
    const bool from_mirror = mirrored && p.resident_valid != 0;
    unsigned char *mp = nullptr;
    auto fence = [] { wave_lds_sync(); };
    u64 fbits0 = 0;
    bool rebuild = false;
    int t0 = 0, hc0 = -1;
    // the stepped state back to memory: the check mask, the fp32 planes (unless the mirror is lazy), the mirror.  In front of
    // the observation everywhere but in the solo form, where it follows it: nothing the observation needs depends on it, and
    // in a launch that is a chain of latencies (section 4.11 item 7 of DESIGN.md) it was 5 900 cycles in front of the first
    // observation store.
    auto store_state = [&]() {
        if (p.err != nullptr) {
            if (clean) m_step = lds_check(cx, sn);
            if (lane == 0) p.err[env] = m_step;
        }
        if (!lazy) {
            if (from_mirror) { // (step_middle has read the lengths out of lmax)
                if (snake) cx.lmax[lane] = t0;
                wave_lds_sync();
            }
            store_env(cx, foodp, headp, bodyp, fbits0, hc0, sn.hc, rebuild, from_mirror); // a rebuilt env is stored whole
        }
        if (mirrored) {
            const bool rebased = rebase_clocks(cx); // the clocks stay with the mirror from call to call
            mirror_store(cx, mp, lane, 64, sn.hc, (snake && !sn.done) ? sn.L : 0, fence, // (a deleted snake's body reads all-zero)
                         from_mirror && !rebuild && !rebased, fbits0);
            wave_lds_sync();
        }
    };
    if (active) {
    foodp = p.foods + env * C; headp = p.heads + env * K * C; bodyp = p.bodies + env * K * C;

    // An env the postponed reset rebuilds is not read from the fp32 planes (as in multi_reset_kernel): the launch is one
    // round of waves and ends with its slowest env, and a rebuilt env — rebuild + whole-env store — is the slowest already.
    // The compact image is requested whether or not the env is rebuilt: "is it rebuilt" is itself a load, and waiting for
    // it first made two memory round trips of one.
    StepIn in;
    step_inputs(p, env, lane, in); // (requested here, used after the env's image has arrived)
    const int rebuild_byte = p.done_env != nullptr ? (int)p.done_env[env] : 0;
    mp = mirrored ? p.resident + env * mirror_env_bytes(K, C) : nullptr;
    bool plain = false; // read from the fp32 planes, which held nothing the image cannot represent
    if (from_mirror) fbits0 = mirror_load(cx, mp, lane, 64, fence, !lazy);
    rebuild = uniform(rebuild_byte) != 0;
    if (!rebuild) {
        if (!from_mirror) fbits0 = load_env(cx, foodp, headp, bodyp, p.err != nullptr, plain);
    } else {
        fbits0 = 0;
        clear_snake_slots(cx, lane);
        wave_lds_sync();
    }
    t0 = snake ? cx.tclk[lane] : 0; // the clocks as loaded (0 unless the state came from the mirror)
    WURM_TLS(cx, 1);
    step_middle(cx, p, env, rebuild, sn, r, hc0, &in);
    WURM_TLS(cx, 8);
    clean = from_mirror || rebuild || plain; // lds_check sees everything there is to check
    if (!solo) store_state();
    WURM_TLS(cx, 9);
    }
    if (solo) { // every wave for itself: its env's class codes -> its K agents' views (no barrier)
        WURM_TLS(cx, 9);
        class_write<unsigned short>(cx, sn.hc, cx.snap, ring);
        WURM_TLS(cx, 10);
        WURM_TLS(cx, 11); // (no barrier in this form)
        grp_emit_group(p, p.obs + env * p.obs_elems - env0 * p.obs_elems, env0, 1, 0, 1, (const unsigned char *)cx.snap, 0, tab, lane);
        WURM_TLS(cx, 12);
        store_state();
#ifdef WURM_TIMELINE
        if (p.obs_after == nullptr) WURM_TLS_STORE(cx, p.obs + env * p.obs_elems);
#endif
        if (p.obs_after == nullptr) return;
        const bool touched = reset_for_obs_after(cx, p, env, sn, r);
        if (p.err_after != nullptr) {
            if (touched) m_step = clean ? lds_check(cx, sn) : MCHK_NOT_COMPUTED;
            if (lane == 0) p.err_after[env] = m_step;
        }
        if (touched) class_write<unsigned short>(cx, sn.hc, cx.snap, ring); // (else: the codes of the stepped state are still there)
        grp_emit_group(p, p.obs_after + env * p.obs_elems - env0 * p.obs_elems, env0, 1, 0, 1, (const unsigned char *)cx.snap, 0, tab, lane);
        return;
    }
    if (grouped) {
        const unsigned char *codes0 = (const unsigned char *)make_ctx(p, 0).snap;
        WURM_TLS(cx, 9);
        if (active) class_write<unsigned short>(cx, sn.hc, cx.snap, ring);
        WURM_TLS(cx, 10);
        workgroup_handoff();
        WURM_TLS(cx, 11);
        grp_emit_group(p, p.obs, env0, nG, wave, wpb, codes0, p.lds_per_wave, tab, lane);
        WURM_TLS(cx, 12);
#ifdef WURM_TIMELINE
        if (p.obs_after == nullptr) {
            workgroup_handoff(); // (the stamps go over what another wave has written)
            if (active) WURM_TLS_STORE(cx, p.obs + env * p.obs_elems);
        }
#endif
        if (p.obs_after == nullptr) return;
        workgroup_handoff(); // every wave has read the codes of the stepped state
        if (active) {
            const bool touched = reset_for_obs_after(cx, p, env, sn, r);
            if (p.err_after != nullptr) {
                if (touched) m_step = clean ? lds_check(cx, sn) : MCHK_NOT_COMPUTED; // (else: the state the first mask describes)
                if (lane == 0) p.err_after[env] = m_step;
            }
            class_write<unsigned short>(cx, sn.hc, cx.snap, ring);
        }
        workgroup_handoff();
        grp_emit_group(p, p.obs_after, env0, nG, wave, wpb, codes0, p.lds_per_wave, tab, lane);
        return;
    }
    if (p.obs_mode != WURM_OBS_NONE) observe(cx, p, p.obs, env, sn);
#ifdef WURM_TIMELINE
    WURM_TLS(cx, 12);
    if (p.obs_after == nullptr && p.obs_mode != WURM_OBS_NONE) WURM_TLS_STORE(cx, p.obs + env * p.obs_elems);
#endif
    if (p.obs_after == nullptr || p.obs_mode == WURM_OBS_NONE) return;
    const bool touched = reset_for_obs_after(cx, p, env, sn, r);
    if (p.err_after != nullptr) {
        if (touched) m_step = clean ? lds_check(cx, sn) : MCHK_NOT_COMPUTED; // (else: the state the first mask describes)
        if (lane == 0) p.err_after[env] = m_step;
    }
    observe(cx, p, p.obs_after, env, sn);
}

// ---- one env per WORKGROUP.  With 10 snakes on 36 x 36 (experiments/speeds.py) an env's grids take 33 KB of LDS: one
// wave per SIMD, and multi_step_kernel spends 445 us on 1.1 GB with nothing to overlap the load, the transition and the
// stores.  Here the four waves of a workgroup share ONE env: all of them copy it in, turn it into class codes and write
// it back (flat over the K * S * S cells; the K agents' observations go out one agent per wave), wave 0 alone runs the
// transition in between.  Same LDS layout, same device functions for everything that is not a plain copy.
// plain: as load_env's (the same in every thread)
__device__ __forceinline__ u64 wg_load_env(const Ctx &cx, const float *__restrict__ foodp, const float *__restrict__ headp,
                                           const float *__restrict__ bodyp, int tid, int nth, bool want_plain, bool &plain)
{
    const int C = cx.C, KC = cx.K * C;
    int odd = 0, nheads = 0;
    clear_snake_slots(cx, tid);
    for (int c = tid; c < C; c += nth) cx.hmap[c] = 0;
    __syncthreads();
    const float rcpC = 1.0f / (float)C;
    constexpr int CH = 8;
    for (int base = 0; base < KC; base += nth * CH) {
        float hv[CH], bv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { // unconditional loads (index clamped into the env), all in flight together
            const int i = min(base + tid + nth * j, KC - 1);
            hv[j] = headp[i];
            bv[j] = bodyp[i];
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = base + tid + nth * j;
            if (i < KC) {
                const int bi = __float2int_rn(bv[j]);
                cx.body[i] = (unsigned short)(bi != 0 ? ((bi & VMASK) | DIRTY) : 0);
                odd |= (int)((hv[j] != 0.0f && hv[j] != 1.0f) || bv[j] != (float)bi || bi < 0 || bi > (int)VMASK);
                nheads += (int)(hv[j] > 0.5f);
                if (hv[j] > 0.5f || bi > 0) { // rare: a head cell or a body cell
                    const int s = div_size(i, rcpC);
                    if (hv[j] > 0.5f) cx.hcell[s] = i - s * C;
                    if (bi > 0) atomicMax(&cx.lmax[s], bi);
                }
            }
        }
    }
    u64 fbits = 0; // bit k: food at cell tid + nth * k
    for (int k = 0, c = tid; c < C; ++k, c += nth) {
        const float fv = foodp[c];
        const int f = fv > 0.5f;
        cx.food[c] = (unsigned char)f;
        fbits |= (u64)f << k;
        odd |= (int)(fv != 0.0f && fv != 1.0f);
    }
    if (want_plain) { // (the colour slots are free until step_middle loads them: a counter for the heads seen by all threads)
        int *cnt = (int *)cx.colf;
        if (tid == 0) *cnt = 0;
        __syncthreads();
        if (nheads) atomicAdd(cnt, nheads);
        const int any_odd = __syncthreads_or(odd);
        int with_head = 0;
        for (int s2 = 0; s2 < cx.K; ++s2) with_head += (int)(cx.hcell[s2] >= 0);
        plain = !any_odd && *cnt == with_head;
        __syncthreads();
    }
    return fbits;
}

__device__ __forceinline__ u64 wg_load_env(const Ctx &cx, const float *__restrict__ foodp, const float *__restrict__ headp,
                                           const float *__restrict__ bodyp, int tid, int nth)
{
    bool unused = false;
    return wg_load_env(cx, foodp, headp, bodyp, tid, nth, false, unused);
}

__device__ __forceinline__ void wg_store_env(const Ctx &cx, float *__restrict__ foodp, float *__restrict__ headp,
                                             float *__restrict__ bodyp, u64 fbits0, bool full, int tid, int nth,
                                             bool t0_in_lmax = false)
{
    const int C = cx.C, KC = cx.K * C;
    const float rcpC = 1.0f / (float)C;
    for (int i = tid; i < KC; i += nth) {
        const unsigned short v = cx.body[i];
        const int s = div_size(i, rcpC), T = cx.tclk[s], T0 = t0_in_lmax ? cx.lmax[s] : 0;
        // changed since the load: written cells, and — once the clock has moved — every cell that held a value
        if (full || (v & DIRTY) || (T != T0 && (int)(v & VMASK) > T0)) bodyp[i] = (float)max((int)(v & VMASK) - T, 0);
        if (full) headp[i] = (i - s * C == cx.hcell[s]) ? 1.0f : 0.0f;
    }
    for (int k = 0, c = tid; c < C; ++k, c += nth) {
        const int f = cx.food[c] != 0;
        if (full || f != (int)((fbits0 >> k) & 1)) foodp[c] = f ? 1.0f : 0.0f;
    }
}

// 'full' observation of the env in LDS by the whole workgroup: class codes (cells over all threads), then one agent
// per wave.  cx.hcell holds the head cells.  Ends with a barrier (the codes and the head map may be rewritten after it).
__device__ __forceinline__ void wg_observe_snap(const Ctx &cx, const MultiArgs &p, float *obs, long long env, int tid,
                                                int nth, int wave)
{
    const int S = cx.S, C = cx.C, K = cx.K;
    int hc = -1;
    if (tid < K) {
        hc = cx.hcell[tid];
        if (hc >= 0) cx.hmap[hc] = (unsigned char)(tid + 1);
    }
    __syncthreads();
    for (int c = tid; c < C; c += nth) {
        const int y = div_size(c, cx.rcpS), x = c - y * S;
        const bool edge = y == 0 || x == 0 || y == S - 1 || x == S - 1;
        u32 v = 0;
        for (int s = 0; s < K; ++s) v |= (u32)((int)(cx.body[s * C + c] & VMASK) > cx.tclk[s]) << s;
        v |= (u32)cx.hmap[c] << SNAP_OWNER_SHIFT;
        v |= (u32)(cx.food[c] != 0) << 14;
        v |= (u32)edge << 15;
        cx.snap[c] = (unsigned short)v;
    }
    __syncthreads();
    if (tid < K && hc >= 0) cx.hmap[hc] = 0;
    float *obs_env = (float *)uniform64((long long)(obs + env * p.obs_elems));
    // (agent, half of its rows) items, dealt round robin: 10 agents over 4 waves were 3 + 3 + 2 + 2 whole views — the
    // workgroup waited for the waves with three
    const int nw = nth >> 6, half = (cx.cpl + 1) >> 1;
    if (p.grp_variant & 1) { // (A/B switch, WURM_MULTI_GROUP_VARIANT bit 0: whole views, round robin)
        for (int a = wave; a < K; a += nw) snap_emit_agent(cx, p, obs_env, cx.snap, a);
    } else {
        for (int i = wave; i < 2 * K; i += nw) snap_emit_agent(cx, p, obs_env, cx.snap, i >> 1, (i & 1) * half, (i & 1) ? cx.cpl : half);
    }
    __syncthreads();
}

template <bool INJ = true, int OBS = -1, int KT = 0, int ST = 0>   // (INJ = false: as multi_rollout_kernel — the launch draws its own random outcomes)
__global__ __launch_bounds__(256) void multi_step_wg_kernel(MultiArgs p_in)
{
    const MultiArgs p = kernel_args<INJ, OBS, KT, ST, -1>(p_in, true);
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x, wave = uniform(tid >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x);
    if (env >= p.N) return; // the whole workgroup: the barriers below see every wave or none
    const Ctx cx = make_ctx(p, 0);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    if (wave == 0) { WURM_TLS_INIT(cx); WURM_TLS(cx, 0); }
    float *foodp = p.foods + env * C, *headp = p.heads + env * K * C, *bodyp = p.bodies + env * K * C;
    // (the rebuild flag, wave 0's step inputs and the compact image are requested together: see multi_step_kernel)
    const int rebuild_byte = p.done_env != nullptr ? (int)p.done_env[env] : 0;
    StepIn in = {};
    if (wave == 0) step_inputs(p, env, lane, in);
    const bool mirrored = p.resident != nullptr, lazy = mirrored && p.resident_lazy != 0;
    const bool from_mirror = mirrored && p.resident_valid != 0;
    unsigned char *mp = mirrored ? p.resident + env * mirror_env_bytes(K, C) : nullptr;
    auto barrier = [] { __syncthreads(); };
    u64 fbits0 = 0;
    bool plain = false;
    if (from_mirror) fbits0 = mirror_load(cx, mp, tid, nth, barrier, !lazy);
    const bool rebuild = rebuild_byte != 0;
    if (!rebuild) {
        if (!from_mirror) fbits0 = wg_load_env(cx, foodp, headp, bodyp, tid, nth, p.err != nullptr, plain);
    } else {
        fbits0 = 0;
        clear_snake_slots(cx, tid);
    }
    __syncthreads();
    const int t0 = tid < K ? cx.tclk[tid] : 0;
    Snake sn;
    StepRes r;
    int hc0 = -1;
    if (wave == 0) {
        WURM_TLS(cx, 1);
        step_middle(cx, p, env, rebuild, sn, r, hc0, &in);
        WURM_TLS(cx, 8);
    }
    const bool clean = from_mirror || rebuild || plain;
    // check_consistency's mask by all four waves when the class-code buffer is there to lend them 2 KB (a snake per wave at
    // a time), else by wave 0 alone
    const int nwv = nth >> 6;
    const bool spread = p.off_snap >= 0 && 2 * C >= 520 * nwv;
    uint32_t m_step = MCHK_NOT_COMPUTED;
    if (p.err != nullptr) {
        if (clean && spread) {
            if (wave == 0 && lane < K) cx.lmax[lane] = (int)sn.done; // (step_middle has read the lengths out of lmax)
            __syncthreads();
            m_step = wg_lds_check(cx, wave, nwv, (unsigned char *)cx.snap);
        } else if (clean && wave == 0) {
            m_step = lds_check(cx, sn);
        }
        if (tid == 0) p.err[env] = m_step;
    }
    __syncthreads();
    if (!lazy) {
        if (from_mirror) {
            if (tid < K) cx.lmax[tid] = t0;
            __syncthreads();
        }
        wg_store_env(cx, foodp, headp, bodyp, fbits0, rebuild, tid, nth, from_mirror);
        if (wave == 0 && !rebuild && lane < K && sn.hc != hc0) store_moved_head(headp, C, lane, hc0, sn.hc);
    }
    if (mirrored) {
        if (wave == 0 && rebase_clocks(cx) && lane == 0) cx.hmap[0] = 1; // (the head map is all-zero here: a flag for the others)
        __syncthreads();
        const bool rebased = cx.hmap[0] != 0;
        __syncthreads();
        if (tid == 0) cx.hmap[0] = 0;
        // (threads 0..K-1 are lanes of wave 0: they hold the snakes' head cells and lengths)
        mirror_store(cx, mp, tid, nth, sn.hc, (tid < K && !sn.done) ? sn.L : 0, barrier, from_mirror && !rebuild && !rebased,
                     fbits0);
        __syncthreads();
    }
    if (p.obs_mode == WURM_OBS_NONE) return;
    if (wave == 0) WURM_TLS(cx, 9);
    wg_observe_snap(cx, p, p.obs, env, tid, nth, wave);
#ifdef WURM_TIMELINE
    if (p.obs_after == nullptr && wave == 0) {
        WURM_TLS(cx, 12);
        WURM_TLS_STORE(cx, p.obs + env * p.obs_elems);
    }
#endif
    if (p.obs_after == nullptr) return;
    if (wave == 0) {
        const bool touched = reset_for_obs_after(cx, p, env, sn, r);
        if (lane == 0) cx.hmap[0] = (unsigned char)touched; // (the head map is all-zero between observations: a flag)
        if (lane < K) cx.lmax[lane] = (int)sn.done;
    }
    __syncthreads();
    if (p.err_after != nullptr) {
        const bool touched = cx.hmap[0] != 0;
        if (touched) {
            if (clean && spread) m_step = wg_lds_check(cx, wave, nwv, (unsigned char *)cx.snap);
            else if (clean && wave == 0) m_step = lds_check(cx, sn);
            else if (!clean) m_step = MCHK_NOT_COMPUTED;
        }
        if (tid == 0) p.err_after[env] = m_step;
    }
    __syncthreads();
    if (tid == 0) cx.hmap[0] = 0;
    __syncthreads();
    wg_observe_snap(cx, p, p.obs_after, env, tid, nth, wave);
}

__global__ __launch_bounds__(256) void multi_reset_kernel(MultiArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, wave);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    const u64 env_id = (u64)(p.env_offset + env);
    const long long agent = env * K + lane;
    float *foodp = p.foods + env * C, *headp = p.heads + env * K * C, *bodyp = p.bodies + env * K * C;

    const bool rebuild = uniform((int)p.done_env[env]) != 0;
    Snake sn;
    sn.hc = -1;
    sn.L = 0;
    sn.done = snake ? p.dones[agent] != 0 : false;
    if (rebuild) sn.done = false; // :798
    sn.orient = 0;
    sn.boosted = false;
    const bool any_dead = ballot(snake && sn.done) != 0;
    const bool respawn = p.cfg.respawn_any && any_dead;
    const bool want_obs = p.obs_mode != WURM_OBS_NONE;

    load_colour(p, agent, snake && (want_obs || p.cfg.colour_random), sn);
    if (snake && reroll_colour(p, agent, sn.done, env_id, p.call, 0, sn)) store_colour(p, agent, sn);
    if (!rebuild && !respawn && !want_obs) return;

    int hc0 = -1;
    u64 fbits0 = 0;
    if (!rebuild) {
        fbits0 = load_env(cx, foodp, headp, bodyp);
        sn.hc = snake ? cx.hcell[lane] : -1;
        sn.L = snake ? cx.lmax[lane] : 0;
        hc0 = sn.hc;
    }
    bool orient_dirty = false;
    multi_reset_grid(cx, p, env, env_id, p.call, rebuild, respawn, sn, orient_dirty, 0, 0);

    if (snake) {
        if (rebuild || respawn) p.dones[agent] = (uint8_t)sn.done;
        if (orient_dirty) p.orientations[agent] = sn.orient;
    }
    if (rebuild) store_env(cx, foodp, headp, bodyp, 0, -1, sn.hc, true);
    else if (respawn) store_env(cx, foodp, headp, bodyp, fbits0, hc0, sn.hc, false);
    if (want_obs) {
        sn.boosted = snake ? p.boost[agent] != 0 : false;
        observe(cx, p, p.obs, env, sn);
    }
}

__global__ __launch_bounds__(256) void multi_observe_kernel(MultiArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, wave);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    load_env(cx, p.foods + env * C, p.heads + env * K * C, p.bodies + env * K * C);
    const bool snake = lane < K;
    Snake sn;
    sn.hc = snake ? cx.hcell[lane] : -1;
    sn.L = 0;
    sn.orient = 0;
    sn.done = snake ? p.dones[env * K + lane] != 0 : false;
    sn.boosted = snake ? p.boost[env * K + lane] != 0 : false;
    load_colour(p, env * K + lane, snake && p.obs_mode == WURM_OBS_PARTIAL, sn);
    observe(cx, p, p.obs, env, sn);
}

// ---- reset and _observe of large envs, one env per workgroup (see multi_step_wg_kernel)
__global__ __launch_bounds__(256) void multi_reset_wg_kernel(MultiArgs p)
{
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x, wave = uniform(tid >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x);
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, 0);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = wave == 0 && lane < K;
    const u64 env_id = (u64)(p.env_offset + env);
    const long long agent = env * K + lane;
    float *foodp = p.foods + env * C, *headp = p.heads + env * K * C, *bodyp = p.bodies + env * K * C;
    const bool rebuild = p.done_env[env] != 0;
    const bool want_obs = p.obs_mode != WURM_OBS_NONE;
    // every thread works out whether a snake is (still) dead: the workgroup decides together whether there is work
    bool any_dead = false;
    if (!rebuild)
        for (int sidx = 0; sidx < K; ++sidx) any_dead |= p.dones[env * K + sidx] != 0;
    const bool respawn = p.cfg.respawn_any && any_dead;
    Snake sn;
    sn.hc = -1;
    sn.L = 0;
    sn.done = snake ? p.dones[agent] != 0 : false;
    if (rebuild) sn.done = false; // :798
    sn.orient = 0;
    sn.boosted = false;
    if (wave == 0) {
        load_colour(p, agent, snake && (want_obs || p.cfg.colour_random), sn);
        if (snake && reroll_colour(p, agent, sn.done, env_id, p.call, 0, sn)) store_colour(p, agent, sn);
    }
    if (!rebuild && !respawn && !want_obs) return;
    u64 fbits0 = 0;
    if (!rebuild) fbits0 = wg_load_env(cx, foodp, headp, bodyp, tid, nth);
    else clear_snake_slots(cx, tid);
    __syncthreads();
    int hc0 = -1;
    if (wave == 0) {
        if (!rebuild) {
            sn.hc = snake ? cx.hcell[lane] : -1;
            sn.L = snake ? cx.lmax[lane] : 0;
            hc0 = sn.hc;
        }
        bool orient_dirty = false;
        multi_reset_grid(cx, p, env, env_id, p.call, rebuild, respawn, sn, orient_dirty, 0, 0);
        if (snake) {
            if (rebuild || respawn) p.dones[agent] = (uint8_t)sn.done;
            if (orient_dirty) p.orientations[agent] = sn.orient;
        }
    }
    __syncthreads();
    if (rebuild || respawn) {
        wg_store_env(cx, foodp, headp, bodyp, fbits0, rebuild, tid, nth);
        if (snake && !rebuild && sn.hc != hc0) store_moved_head(headp, C, lane, hc0, sn.hc);
    }
    if (want_obs) wg_observe_snap(cx, p, p.obs, env, tid, nth, wave);
}

__global__ __launch_bounds__(256) void multi_observe_wg_kernel(MultiArgs p)
{
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x, wave = uniform(tid >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x);
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, 0);
    wg_load_env(cx, p.foods + env * cx.C, p.heads + env * cx.K * cx.C, p.bodies + env * cx.K * cx.C, tid, nth);
    __syncthreads();
    wg_observe_snap(cx, p, p.obs, env, tid, nth, wave);
}

// ------------------------------------------------------------------------------------------------ rollout

// T fused iterations of the caller loop of experiments/speeds.py:30-37 / tests/test_multi_snake_env.py:78-89:
//   step(actions[t]) with call = call0 + 2t  ->  outputs[t], observation[t];   reset(dones['__all__']) with call0 + 2t + 1
// with the env resident in LDS and the per-snake scalars in lanes for the whole launch: the state crosses HBM twice
// per launch instead of four times per iteration; per iteration only the actions are read and the outputs written.
//   actions (T,K,N);  out_f32 (T,3,K,N) = rewards, food, sizes;  out_u8 (T,4,K,N) = dones, boost, snake_collision,
//   edge_collision;  all_done (T,N);  obs (T,K,N,elems).
// TWO ('full' observations of at most 10 snakes): a workgroup is TWO waves for ONE env.  Wave 0 steps the env and leaves
// the class codes of the stepped state in one of two LDS buffers; wave 1 turns the codes of step t into the ~120 stores
// of its observation while wave 0 is already computing step t + 1; one s_barrier per step hands a buffer over.  The
// transition (latency-bound LDS work) and the observation (store-bound) of a launch otherwise ADD UP — every wave is in
// the same phase — and interleaving them inside one wave does not help (measured); two waves with their own
// instruction streams do overlap.

// INJ = false: the launch draws its random outcomes itself (every launch but the replays of recorded fixtures) — the
// injected-outcome branches of the step and of the reset, their nine pointers and three running offsets fold away, which
// matters in a kernel whose uniform state does not fit the scalar registers (profiles/r05_kernel_resources.txt).
// OBS >= 0: the observation mode is a compile-time constant too (the other modes' writers and their loop invariants go).
template <bool TWO, bool INJ, int OBS = -1, int KT = 0, int ST = 0, int NT = -1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void multi_rollout_kernel(MultiArgs p_in)
{
    const MultiArgs p = kernel_args<INJ, OBS, KT, ST, NT>(p_in, !TWO && (OBS == WURM_OBS_PARTIAL || OBS == WURM_OBS_NONE), 0);
    const int wave = uniform((int)(threadIdx.x >> 6)), wpb = TWO ? 1 : (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + (TWO ? 0 : wave);
    if (env >= p.N) return;
    const Ctx cx = make_ctx(p, TWO ? 0 : wave, 0, !TWO && p.obs_mode != WURM_OBS_DEFAULT);
    const int C = cx.C, K = cx.K, lane = cx.lane;
    if (TWO && wave == 1) { // the writer: observation of step t from buffer t & 1, handed over by the barrier of step t
        const long long KNw = (long long)K * p.N;
        for (long long t = 0; t < p.T; ++t) {
            workgroup_handoff();
            snap_emit(cx, p, (float *)uniform64((long long)(p.obs + t * KNw * p.obs_elems + env * p.obs_elems)),
                      cx.snap + (t & 1) * C);
        }
        return;
    }
    const bool snake = lane < K;
    const u64 env_id = (u64)(p.env_offset + env);
    const long long agent = env * K + lane, KN = (long long)K * p.N;
    float *foodp = p.foods + env * C, *headp = p.heads + env * K * C, *bodyp = p.bodies + env * K * C;

    // (the caller's compact mirror when it describes the state — wurm_multi_rollout_resident — else the fp32 planes; the writer
    // wave of the TWO form never gets here with a mirror: that form works on the planes)
    const bool mirrored = !TWO && p.resident != nullptr, from_mirror = mirrored && p.resident_valid != 0;
    unsigned char *const mp = mirrored ? p.resident + env * mirror_env_bytes(K, C) : nullptr;
    const u64 fbits0 = from_mirror ? mirror_load(cx, mp, lane, 64, [] { wave_lds_sync(); }, false) : load_env(cx, foodp, headp, bodyp);
    Snake sn;
    sn.hc = snake ? cx.hcell[lane] : -1;
    sn.L = snake ? cx.lmax[lane] : 0;
    sn.done = snake ? p.dones[agent] != 0 : true;
    sn.orient = snake ? p.orientations[agent] : 0;
    sn.boosted = false;
    load_colour(p, agent, snake, sn);
    bool col_dirty = false;
    const int hc0 = sn.hc; // what HBM holds: for the sparse write-back at the end
    WURM_TLS_INIT(cx);

    for (long long t = 0; t < p.T; ++t) {
        const u64 call = p.call + 2ull * (u64)t;
        WURM_TLS(cx, 0); // (timeline: the segment that ends here is the previous step's reset)
        // Actions come from LDS, 64 steps at a time.  A global LOAD inside the step loop would queue behind the
        // observation stores of the whole CU — the vector memory pipeline is in order — and every step would wait for
        // the store backlog to drain: that, not the arithmetic, is why transition and observation time used to add up.
        // Kept per action: a % 4 (C semantics, -3..3) and a > 3, which is all the step reads of it (:483-484).
        if ((t & 63) == 0) {
            const int nt = (int)min((long long)64, p.T - t);
            wave_lds_sync();
            for (int i = lane; i < nt * K; i += 64) {
                const int j = i / K, sidx = i - j * K;
                const long long av = p.actions[(t + j) * KN + (long long)sidx * p.N + env];
                cx.acts[i] = (unsigned char)(((int)(av % 4) + 4) | (av > 3 ? 8 : 0));
            }
            wave_lds_sync();
        }
        long long a = 0;
        if (snake) {
            const int b = cx.acts[(int)(t & 63) * K + lane];
            const int d4 = (b & 7) - 4;
            a = (b & 8) ? 4 + d4 : d4; // same a % 4 and a > 3 as the caller's value (a > 3 implies a % 4 >= 0)
        }
        StepRes r;
        WURM_TLS(cx, 2); // actions decoded
        multi_step_body(cx, p, env, env_id, call, a, sn, r, t * p.N * C, t * KN, t * p.N);
        WURM_TLS(cx, 7);
        if (snake) {
            const long long am = (long long)lane * p.N + env;
            float *of = p.am_f32 + t * 3 * KN;
            uint8_t *ob = p.am_u8 + t * 4 * KN;
            of[am] = r.reward;
            of[KN + am] = r.foodcons;
            of[2 * KN + am] = (float)sn.L;
            ob[am] = (uint8_t)sn.done;
            ob[KN + am] = (uint8_t)sn.boosted;
            ob[2 * KN + am] = (uint8_t)r.snakecol;
            ob[3 * KN + am] = (uint8_t)r.edgecol;
        }
        if (lane == 0) p.all_done[t * p.N + env] = (uint8_t)r.all_done;
        if (TWO) {
            // buffer t & 1 is free: the writer finished with it before it arrived at the barrier of step t - 1
            snap_write(cx, sn.hc, cx.snap + (t & 1) * C);
            workgroup_handoff();
        } else if (p.obs_mode != WURM_OBS_NONE) {
            WURM_TLS(cx, 8); // outputs stored
            observe(cx, p, p.obs + t * KN * p.obs_elems, env, sn);
            WURM_TLS(cx, 9); // observation issued
        }
        rebase_clocks(cx);

        // reset(dones['__all__']) (:771-836)
        if (snake && sn.done) sn.L = 0;           // deleted snakes have an all-zero body
        const bool rebuild = r.all_done;
        if (rebuild) sn.done = false;             // :798
        if (snake) col_dirty |= reroll_colour(p, agent, sn.done, env_id, call + 1ull, t * KN, sn);
        const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
        if (rebuild || respawn) {
            bool orient_dirty = false;
            multi_reset_grid(cx, p, env, env_id, call + 1ull, rebuild, respawn, sn, orient_dirty, t * KN, t * p.N);
        }
    }

    if (snake) {
        p.dones[agent] = (uint8_t)sn.done;
        p.orientations[agent] = sn.orient;
        if (p.boost_state) p.boost_state[agent] = (uint8_t)sn.boosted;
        if (col_dirty) store_colour(p, agent, sn);
        cx.hcell[lane] = sn.hc;
    }
    wave_lds_sync();
    // only what may differ from HBM: body cells that have held a value since the load (DIRTY survives deletions, rebuilds
    // and re-bases), the head cell of each snake, food cells that changed — everything when the state came from the mirror,
    // nothing while the mirror is lazy
    if (!(mirrored && p.resident_lazy)) store_env(cx, foodp, headp, bodyp, fbits0, hc0, sn.hc, from_mirror);
    if (mirrored) {
        (void)rebase_clocks(cx);
        mirror_store(cx, mp, lane, 64, sn.hc, (snake && !sn.done) ? sn.L : 0, [] { wave_lds_sync(); });
        wave_lds_sync();
    }
#ifdef WURM_TIMELINE
    if (!TWO && p.obs_mode != WURM_OBS_NONE) WURM_TLA_STORE(cx, p.obs + env * p.obs_elems); // (step 0, agent 0: garbage by construction)
#endif
}

// G envs, G / EPS stepper waves (EPS envs each, one after the other within a step: the transition of one env is a chain of
// dependent LDS operations that takes a wave ~5 us of the ~22 us the step's observations need on the store path, and a
// stepper's register budget is what limits the waves per SIMD — so fewer, fuller stepper waves), W writer waves.
// WIDE (6 .. 10 snakes): 32-bit class words and ONE code / output buffer — the steppers wait for the writers to be done with
// step t - 1 before they write the codes of step t (a second barrier per step; the transition itself still runs beside the
// writers: the speeds.py shape, 10 snakes on 36 x 36, has 41 KB of LDS per env with one 32-bit buffer and four envs per CU).
// INJ = false: as multi_rollout_kernel — the launch draws its own random outcomes, the injected-outcome branches fold away.
template <int G, int W, int EPS, int OCC, bool WIDE = false, bool INJ = true, int KT = 0, int ST = 0>
__global__ __launch_bounds__(64 * (G / EPS + W)) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void multi_rollout_group_kernel(MultiArgs p_in)
{
    MultiArgs p = p_in;
    if (!INJ) p.has_inj = p.has_rinj = 0;
    p.obs_mode = WURM_OBS_DEFAULT; // (what multi_group_shape requires: a constant here)
    if (KT > 0 && ST > 0) { // (shape_constants: K, S and with them the whole LDS layout of the group as constants)
        p.K = KT;
        p.S = ST;
        p.obs_elems = 3ll * ST * ST;
        (void)group_layout(p, G, WIDE);
    }
    typedef typename std::conditional<WIDE, u32, unsigned short>::type CT;
    constexpr int NSW = G / EPS; // stepper waves
    // SHARE: the (agent, env) blocks of a step are handed out by an LDS counter and the steppers take some too
    // (grp_take_items) — measured to pay only where the writer waves alone cannot keep up (fewer writers than agents:
    // 8 / 2 / 1 / 5 went from 1.93 to 1.64 ms per 64 steps at cfg4); with one writer per agent the steppers queueing on the
    // store path lengthen the step (8 / 4 / 1 / 6: 1.61 -> 1.96 ms), so each writer keeps its own agent's run there
    constexpr bool SHARE = W < 4 && !WIDE;
    const int wave = uniform((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const long long env0 = xcd_block(blockIdx.x, gridDim.x) * G;
    if (env0 >= p.N) return;
    const int nG = (int)min((long long)G, p.N - env0);
    const int C = p.S * p.S, K = p.K;
    const long long KN = (long long)K * p.N;
    float *const tab = (float *)wurm_multi_lds;
    unsigned char *const codes0 = wurm_multi_lds + p.grp_codes, *const outs0 = wurm_multi_lds + p.grp_outs;
    int *const ctr = (int *)(wurm_multi_lds + 96); // two item counters (one per buffer) behind the 24 floats of the table
    grp_table_init(tab, (int)threadIdx.x);
    if (SHARE && threadIdx.x < 2) ctr[threadIdx.x] = 0;
    __syncthreads();
#ifdef WURM_GROUP_PROBE
    const bool stores = !(p.grp_variant & 4);
#else
    constexpr bool stores = true;
#endif

    if (wave >= NSW) { // ---- a writer: the observations of step t from buffer t & 1, handed over by the barrier of step t
        const int w = wave - NSW;
        for (long long t = 0; t < p.T; ++t) {
            if (WIDE) workgroup_handoff();   // (the steppers may now overwrite the single buffer: the writers are done with t - 1)
            workgroup_handoff();
            const int buf = WIDE ? 0 : (int)(t & 1);
            const unsigned char *cbuf = codes0 + (size_t)buf * G * p.grp_code_bytes;
            if (w == 0) { // the steppers' per-step outputs: rows (j K + s) of G consecutive envs each
                const unsigned char *obuf = outs0 + (size_t)buf * G * p.grp_out_bytes;
                float *of = p.am_f32 + t * 3 * KN;
                uint8_t *ob = p.am_u8 + t * 4 * KN;
                for (int i = lane; i < 3 * K * G; i += 64) {
                    const int g = i % G, js = i / G;
                    if (g < nG) of[(long long)js * p.N + env0 + g] = ((const float *)(obuf + (size_t)g * p.grp_out_bytes))[js];
                }
                for (int i = lane; i < 4 * K * G; i += 64) {
                    const int g = i % G, js = i / G;
                    if (g < nG) ob[(long long)js * p.N + env0 + g] = (obuf + (size_t)g * p.grp_out_bytes)[12 * K + js];
                }
                if (lane < nG) p.all_done[t * p.N + env0 + lane] = (obuf + (size_t)lane * p.grp_out_bytes)[16 * K];
            }
            if (SHARE) {
                grp_take_items<CT>(p, ctr + buf, cbuf, t, env0, nG, tab, lane, stores);
            } else {
                // writer wave -> (agent, part of the group's envs): one agent after the other while there are at most as many
                // waves as agents, else W / K waves per agent, each with its own contiguous part of the run
                const int parts = W > K ? W / K : 1, part = W > K ? w / K : 0;
                const int g0 = part * G / parts, g1 = min((part + 1) * G / parts, nG);
                for (int a = W > K ? w % K : w; a < K && part < parts; a += W > K ? K : W) {
                    grp_gfloat *const run = (grp_gfloat *)uniform64((long long)(p.obs + ((t * K + a) * p.N + env0) * p.obs_elems));
                    for (int g = g0; g < g1; ++g)
                        grp_emit_cells<CT>(run + g * 3 * C, (const CT *)(cbuf + (size_t)g * p.grp_code_bytes), tab, 3u * (u32)a, C, lane,
                                           stores);
                }
            }
        }
        return;
    }

    // ---- a stepper: envs env0 + wave * EPS + e, e < EPS; the scalars of the envs it is not working on wait in LDS
    if (env0 + wave * EPS >= p.N) { // a ragged last group: nothing to step — the barriers are the workgroup's, and it writes
        for (long long t = 0; t < p.T; ++t) {
            if (WIDE) workgroup_handoff();
            workgroup_handoff();
            const int buf = WIDE ? 0 : (int)(t & 1);
            if (SHARE) grp_take_items<CT>(p, ctr + buf, codes0 + (size_t)buf * G * p.grp_code_bytes, t, env0, nG, tab, lane, stores);
        }
        return;
    }
    const bool snake = lane < K;
    const u64 ring = border_bits(make_ctx(p, 0, p.grp_env0));
    int *const save0 = (int *)(wurm_multi_lds + p.grp_save);
    for (int e = 0; e < EPS; ++e) {
        const int g = wave * EPS + e;
        const long long env = env0 + g;
        if (env >= p.N) break;
        const Ctx cx = make_ctx(p, g, p.grp_env0);
        const long long agent = env * K + lane;
        // the caller's compact mirror (wurm_multi_rollout_resident), when it describes the state: 2 K + 1 bytes per cell
        // instead of (1 + 2 K) fp32 planes — 23 MB against 92 at cfg4, 110 against 446 at the speeds.py shape, which is a
        // tenth of a 4-step launch there
        if (p.resident != nullptr && p.resident_valid)
            (void)mirror_load(cx, p.resident + env * mirror_env_bytes(K, C), lane, 64, [] { wave_lds_sync(); }, false);
        else
            (void)load_env(cx, p.foods + env * C, p.heads + env * K * C, p.bodies + env * K * C);
        Snake sn;
        sn.hc = snake ? cx.hcell[lane] : -1;
        sn.L = snake ? cx.lmax[lane] : 0;
        sn.done = snake ? p.dones[agent] != 0 : true;
        sn.orient = snake ? p.orientations[agent] : 0;
        sn.boosted = false;
        load_colour(p, agent, snake, sn);
        grp_save(save0 + g * 8 * K, lane, K, sn, false, sn.hc);
    }
    wave_lds_sync();

    for (long long t = 0; t < p.T; ++t) {
        const u64 call = p.call + 2ull * (u64)t;
        for (int e = 0; e < EPS; ++e) {
            const int g = wave * EPS + e;
            const long long env = env0 + g;
            if (env >= p.N) break; // (a ragged last group: the barrier below is still the workgroup's)
            const Ctx cx = make_ctx(p, g, p.grp_env0);
            const u64 env_id = (u64)(p.env_offset + env);
            Snake sn;
            bool col_dirty;
            int hc0;
            grp_restore(save0 + g * 8 * K, lane, K, sn, col_dirty, hc0);
            if ((t & 63) == 0) { // actions: 64 steps at a time into LDS (see multi_rollout_kernel)
                const int nt = (int)min((long long)64, p.T - t);
                wave_lds_sync();
                for (int i = lane; i < nt * K; i += 64) {
                    const int j = i / K, sidx = i - j * K;
                    const long long av = p.actions[(t + j) * KN + (long long)sidx * p.N + env];
                    cx.acts[i] = (unsigned char)(((int)(av % 4) + 4) | (av > 3 ? 8 : 0));
                }
                wave_lds_sync();
            }
            long long a = 0;
            if (snake) {
                const int b = cx.acts[(int)(t & 63) * K + lane];
                const int d4 = (b & 7) - 4;
                a = (b & 8) ? 4 + d4 : d4;
            }
            StepRes r = {};
            if (WURM_PROBE(!(p.grp_variant & 8), true)) multi_step_body(cx, p, env, env_id, call, a, sn, r, t * p.N * C, t * KN, t * p.N);
            // buffer t & 1 is free: the writers finished with it before they arrived at the barrier of step t - 1
            // (WIDE: the one buffer is free once the writers have passed the extra barrier of this step)
            if (WIDE && e == 0) {
                // this wave's transition is done: the rest of step t - 1's observations, with the writers — then the one
                // buffer is free for this step's codes
                if (SHARE && t > 0) grp_take_items<CT>(p, ctr, codes0, t - 1, env0, nG, tab, lane, stores);
                workgroup_handoff();
            }
            const int buf = WIDE ? 0 : (int)(t & 1);
            if (SHARE && e == 0 && wave == 0 && lane == 0) ctr[buf] = 0; // (everybody is done with the items this counter handed out last)
            unsigned char *obuf = outs0 + ((size_t)buf * G + g) * p.grp_out_bytes;
            if (snake) {
                float *f = (float *)obuf;
                f[lane] = r.reward;
                f[K + lane] = r.foodcons;
                f[2 * K + lane] = (float)sn.L;
                unsigned char *b = obuf + 12 * K;
                b[lane] = (unsigned char)sn.done;
                b[K + lane] = (unsigned char)sn.boosted;
                b[2 * K + lane] = (unsigned char)r.snakecol;
                b[3 * K + lane] = (unsigned char)r.edgecol;
            }
            if (lane == 0) obuf[16 * K] = (unsigned char)r.all_done;
            class_write<CT>(cx, sn.hc, (CT *)(codes0 + ((size_t)buf * G + g) * p.grp_code_bytes), ring);
            if (lane == 0) ((int *)(save0 + g * 8 * K))[7] = (int)r.all_done;   // (slot 7 of snake 0: for the reset below)
            grp_save(save0 + g * 8 * K, lane, K, sn, col_dirty, hc0);
            wave_lds_sync();
        }
        // (two buffers: the codes of step t are in place — the rest of step t - 1's observations, with the writers)
        if (SHARE && !WIDE && t > 0) {
            const int pb = (int)((t - 1) & 1);
            grp_take_items<CT>(p, ctr + pb, codes0 + (size_t)pb * G * p.grp_code_bytes, t - 1, env0, nG, tab, lane, stores);
        }
        // the writers start on step t NOW: the reset that follows the step (a rebuilt env costs as much as a whole
        // transition) runs beside them, not in front of them
        workgroup_handoff();
        for (int e = 0; e < EPS; ++e) {
            const int g = wave * EPS + e;
            const long long env = env0 + g;
            if (env >= p.N) break;
            const Ctx cx = make_ctx(p, g, p.grp_env0);
            const u64 env_id = (u64)(p.env_offset + env);
            const long long agent = env * K + lane;
            Snake sn;
            bool col_dirty;
            int hc0;
            grp_restore(save0 + g * 8 * K, lane, K, sn, col_dirty, hc0);
            const bool rebuild = uniform(((const int *)(save0 + g * 8 * K))[7]) != 0;
            rebase_clocks(cx);

            // reset(dones['__all__']) (:771-836)
            if (snake && sn.done) sn.L = 0;
            if (rebuild) sn.done = false;             // :798
            if (snake) col_dirty |= reroll_colour(p, agent, sn.done, env_id, call + 1ull, t * KN, sn);
            const bool respawn = p.cfg.respawn_any && ballot(snake && sn.done) != 0;
            if (rebuild || respawn) {
                bool orient_dirty = false;
                multi_reset_grid(cx, p, env, env_id, call + 1ull, rebuild, respawn, sn, orient_dirty, t * KN, t * p.N);
            }
            grp_save(save0 + g * 8 * K, lane, K, sn, col_dirty, hc0);
            wave_lds_sync();
        }
    }

    for (int e = 0; e < EPS; ++e) {
        const int g = wave * EPS + e;
        const long long env = env0 + g;
        if (env >= p.N) break;
        const Ctx cx = make_ctx(p, g, p.grp_env0);
        const long long agent = env * K + lane;
        Snake sn;
        bool col_dirty;
        int hc0;
        grp_restore(save0 + g * 8 * K, lane, K, sn, col_dirty, hc0);
        if (snake) {
            p.dones[agent] = (uint8_t)sn.done;
            p.orientations[agent] = sn.orient;
            if (p.boost_state) p.boost_state[agent] = (uint8_t)sn.boosted;
            if (col_dirty) store_colour(p, agent, sn);
            cx.hcell[lane] = sn.hc;
        }
        wave_lds_sync();
        // the food plane is written whole (the original bits are not kept across the launch: ~cur marks every cell changed)
        u64 cur = 0;
        for (int k = 0; k < cx.cpl; ++k) {
            const int c = lane + 64 * k;
            if (c < C && cx.food[c]) cur |= 1ull << k;
        }
        // the fp32 planes: not at all while the mirror is lazy; whole when the state came from the mirror (the DIRTY marks
        // only cover what was written since a load from the planes); else what changed
        const bool from_mirror = p.resident != nullptr && p.resident_valid;
        if (!(p.resident != nullptr && p.resident_lazy))
            store_env(cx, p.foods + env * C, p.heads + env * K * C, p.bodies + env * K * C, ~cur, hc0, sn.hc, from_mirror);
        if (p.resident != nullptr) {
            (void)rebase_clocks(cx);
            mirror_store(cx, p.resident + env * mirror_env_bytes(K, C), lane, 64, sn.hc, (snake && !sn.done) ? sn.L : 0,
                         [] { wave_lds_sync(); });
            wave_lds_sync();
        }
    }
}

// check_consistency (:733-769) -> per-env bitmask.  Every plane is read once: the per-cell count of snakes (overlap test)
// is kept in LDS, one byte per cell; a cell belongs to one lane, so plain read-modify-writes.
// The env's planes are walked as ITEMS of (snake, 11 rows of 64 cells), double-buffered in registers: the 16 loads of item
// i + 1 are in flight while item i is reduced (round 2 issued a snake's loads, waited, reduced, and only then touched the
// next snake: five dependent memory round trips per env at K = 4, 2.6 TB/s).
constexpr int MCHK_U = 11; // 25 x 25: a snake is one item, 36 x 36: two (11 + 10 rows)

__device__ __forceinline__ void mchk_load(const float *__restrict__ hp, const float *__restrict__ bp, int k0, int lane, int C,
                                          float (&h)[MCHK_U], float (&b)[MCHK_U])
{
#pragma unroll
    for (int j = 0; j < MCHK_U; ++j) {
        const int c = lane + 64 * (k0 + j);
        const bool in = c < C;
        h[j] = in ? hp[c] : 0.0f;
        b[j] = in ? bp[c] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void multi_check_kernel(MultiArgs p)
{
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const long long env = xcd_block(blockIdx.x, gridDim.x) * wpb + wave;
    if (env >= p.N) return;
    const int S = p.S, C = S * S, K = p.K, lane = (int)(threadIdx.x & 63u), cpl = (C + 63) >> 6;
    unsigned char *cnt = wurm_multi_lds + (size_t)wave * p.lds_per_wave;
    const float *foodp = p.foods + env * C;
    const float *heads = p.heads + env * K * C, *bodies = p.bodies + env * K * C;
    const int nchunk = (cpl + MCHK_U - 1) / MCHK_U, nitems = K * nchunk;
    float hA[MCHK_U], bA[MCHK_U], hB[MCHK_U], bB[MCHK_U];
    mchk_load(heads, bodies, 0, lane, C, hA, bA); // item 0 is in flight while the food plane is checked
    uint32_t m = 0;
    int badf = 0;
    for (int k = 0; k < cpl; ++k) {
        int c = lane + 64 * k;
        if (c < C) {
            const float f = rintf(foodp[c]); // the reference checks living_envs.round() (:742): 0.5 is a 0, 1.5 a 2
            badf |= !(f == 0.0f || f == 1.0f);
            cnt[c] = 0;
        }
    }
    const bool bad_food = ballot(badf != 0) != 0;
    bool any_alive = false;
    int hs = 0, bs = 0, bm = 0, hb = 0, hf = 0, nz = 0; // per-lane partials of the current snake
    auto reduce_item = [&](int item, const float (&h)[MCHK_U], const float (&b)[MCHK_U]) {
        const int s = item / nchunk, k0 = (item - s * nchunk) * MCHK_U;
#pragma unroll
        for (int j = 0; j < MCHK_U; ++j) {
            const int c = lane + 64 * (k0 + j);
            if (c < C) {
                const int hi = __float2int_rn(h[j]), bi = __float2int_rn(b[j]);
                hs += hi; bs += bi; hb += hi * bi;
                if (hi != 0) hf += hi * __float2int_rn(foodp[c]); // at the head cells only (one per snake)
                bm = max(bm, bi);
                nz |= (h[j] != 0.0f) || (b[j] != 0.0f);
                if (b[j] > 1e-6f) cnt[c] += 1;
            }
        }
        if (k0 + MCHK_U >= cpl) { // the snake's last item: its verdict
            const bool dead = p.dones[env * K + s] != 0;
            if (dead) {
                if (ballot(nz != 0)) m |= WURM_MCHK_DEAD_NONZERO;
            } else {
                any_alive = true;
                const int t_hs = wave_sum_i32(hs), t_bs = wave_sum_i32(bs), t_hb = wave_sum_i32(hb), t_hf = wave_sum_i32(hf);
                const int t_bm = wave_max_i32(bm);
                if (t_hs != 1) m |= WURM_CHK_ONE_HEAD;
                if (!(t_bs > 0)) m |= WURM_CHK_HAS_SNAKE;
                if (t_bm != t_hb) m |= WURM_CHK_HEAD_AT_END;
                if (2 * t_bs != t_bm * (t_bm + 1)) m |= WURM_CHK_BODY_RANGE;
                if (!(t_bs >= 6)) m |= WURM_CHK_MIN_LENGTH;
                if (t_hf != 0) m |= WURM_CHK_HEAD_ON_FOOD;
            }
            hs = bs = bm = hb = hf = nz = 0;
        }
    };
    auto issue = [&](int item, float (&h)[MCHK_U], float (&b)[MCHK_U]) {
        const int s = item / nchunk, k0 = (item - s * nchunk) * MCHK_U;
        mchk_load(heads + s * C, bodies + s * C, k0, lane, C, h, b);
    };
    for (int it = 0; it < nitems; it += 2) {
        if (it + 1 < nitems) issue(it + 1, hB, bB);
        reduce_item(it, hA, bA);
        if (it + 2 < nitems) issue(it + 2, hA, bA);
        if (it + 1 < nitems) reduce_item(it + 1, hB, bB);
    }
    if (any_alive && bad_food) m |= WURM_CHK_FOOD_VALUE; // reported per living snake by the loop this replaces
    int over = 0;
    for (int k = 0; k < cpl; ++k) {
        int c = lane + 64 * k;
        if (c < C) over |= cnt[c] > 1;
    }
    if (ballot(over != 0)) m |= WURM_MCHK_OVERLAP;
    if (lane == 0) p.err[env] = m;
}

__global__ void multi_colours_kernel(short *colours, long long N, int K, int fixed, u64 seed, u64 call, long long env_offset)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    long long env = i / K;
    int s = (int)(i - env * K);
    u64 env_id = fixed ? 0xffffffffull : (u64)(env_offset + env);
    short col[3];
    colour_from_words(rng_words(seed, call, env_id, RNG_COLOUR, (u32)s), col);
    colours[i * 3] = col[0];
    colours[i * 3 + 1] = col[1];
    colours[i * 3 + 2] = col[2];
}

// ------------------------------------------------------------------------------------------------ host side

enum MKind { MK_STEP, MK_RESET, MK_OBSERVE, MK_CHECK, MK_ROLLOUT };
constexpr int LDS_MAX_BYTES = 160 * 1024; // per workgroup on CDNA4 (MI355X_MICROARCH.md)

// ---- every kernel instantiation multi_launch can start: ONE list; a route is a row of it, its name what wurm_multi_last_route
// reports.  A grouped rollout is named by the code of its shape (1000 G + 100 W + 10 EPS + OCC, as WURM_MULTI_GROUP_SHAPE takes
// it).  No suffix: the instantiation that reads tapes or draws, as the call asks; _rng: the one that only draws (INJ = false);
// _full / _partial / _none: the observation mode compiled in; _kK_sS[_nN]: the shape compiled in (shape_constants).
struct MultiKernel { const char *name; void (*fn)(MultiArgs); };
typedef const MultiKernel *MRoute; // nullptr: no kernel takes the call
static const MultiKernel
    MR_STEP{"step", multi_step_kernel<true, -1>}, MR_STEP_RNG_FULL{"step_rng_full", multi_step_kernel<false, WURM_OBS_DEFAULT>},
    MR_STEP_RNG_PARTIAL{"step_rng_partial", multi_step_kernel<false, WURM_OBS_PARTIAL>}, MR_STEP_RNG_NONE{"step_rng_none", multi_step_kernel<false, WURM_OBS_NONE>},
    // the shape of the reference's multi-agent experiments (experiments/multiagent.py:79-86: 4 snakes on 25 x 25, partial_5)
    // has kernels with K, S and the crop radius as constants (WURM_MULTI_SHAPE_KERNELS = 0: the generic ones)
    MR_STEP_RNG_PARTIAL_K4_S25_N5{"step_rng_partial_k4_s25_n5", multi_step_kernel<false, WURM_OBS_PARTIAL, 4, 25, 5>},
    MR_STEP_RNG_FULL_K4_S25{"step_rng_full_k4_s25", multi_step_kernel<false, WURM_OBS_DEFAULT, 4, 25>},
    // (the reference's own test shape, tests/test_multi_snake_env.py:340: 512 envs of 2 snakes on 12 x 12)
    MR_STEP_RNG_FULL_K2_S12{"step_rng_full_k2_s12", multi_step_kernel<false, WURM_OBS_DEFAULT, 2, 12>},
    MR_RESET{"reset", multi_reset_kernel}, MR_OBSERVE{"observe", multi_observe_kernel}, MR_CHECK{"check", multi_check_kernel},
    MR_ROLLOUT{"rollout", multi_rollout_kernel<false, true>}, MR_ROLLOUT_RNG{"rollout_rng", multi_rollout_kernel<false, false>},
    MR_ROLLOUT_RNG_PARTIAL{"rollout_rng_partial", multi_rollout_kernel<false, false, WURM_OBS_PARTIAL>}, MR_ROLLOUT_RNG_NONE{"rollout_rng_none", multi_rollout_kernel<false, false, WURM_OBS_NONE>},
    MR_ROLLOUT_RNG_PARTIAL_K4_S25_N5{"rollout_rng_partial_k4_s25_n5", multi_rollout_kernel<false, false, WURM_OBS_PARTIAL, 4, 25, 5>},
    MR_ROLLOUT_TWO{"rollout_two", multi_rollout_kernel<true, true>}, MR_ROLLOUT_TWO_RNG{"rollout_two_rng", multi_rollout_kernel<true, false>},
    MR_STEP_WG{"step_wg", multi_step_wg_kernel<true>}, MR_STEP_WG_RNG{"step_wg_rng", multi_step_wg_kernel<false>},
    MR_STEP_WG_RNG_FULL_K10_S36{"step_wg_rng_full_k10_s36", multi_step_wg_kernel<false, WURM_OBS_DEFAULT, 10, 36>}, // experiments/speeds.py
    MR_RESET_WG{"reset_wg", multi_reset_wg_kernel}, MR_OBSERVE_WG{"observe_wg", multi_observe_wg_kernel},
    MR_GROUP_8215{"rollout_group_8215", multi_rollout_group_kernel<8, 2, 1, 5>}, MR_GROUP_8215_RNG{"rollout_group_8215_rng", multi_rollout_group_kernel<8, 2, 1, 5, false, false>},
    MR_GROUP_8416{"rollout_group_8416", multi_rollout_group_kernel<8, 4, 1, 6>}, MR_GROUP_8416_RNG{"rollout_group_8416_rng", multi_rollout_group_kernel<8, 4, 1, 6, false, false>},
    MR_GROUP_4414{"rollout_group_4414", multi_rollout_group_kernel<4, 4, 1, 4>}, MR_GROUP_4414_RNG{"rollout_group_4414_rng", multi_rollout_group_kernel<4, 4, 1, 4, false, false>},
    MR_GROUP_4414_RNG_K4_S25{"rollout_group_4414_rng_k4_s25", multi_rollout_group_kernel<4, 4, 1, 4, false, false, 4, 25>}, MR_GROUP_8424{"rollout_group_8424", multi_rollout_group_kernel<8, 4, 2, 4>},
    MR_GROUP_5014{"rollout_group_5014", multi_rollout_group_kernel<4, 10, 1, 4, true>}, MR_GROUP_5014_RNG{"rollout_group_5014_rng", multi_rollout_group_kernel<4, 10, 1, 4, true, false>},
    MR_GROUP_4514{"rollout_group_4514", multi_rollout_group_kernel<4, 5, 1, 4, true>}, MR_GROUP_3014{"rollout_group_3014", multi_rollout_group_kernel<2, 10, 1, 4, true>};

// A shape of multi_rollout_group_kernel: G envs, W writer waves, EPS envs per stepper wave, OCC waves per SIMD (option
// WURM_MULTI_GROUP_SHAPE = 1000 G + 100 W + 10 EPS + OCC picks one of the compiled shapes; 0 = automatic: the first that fits).
// any / rng / shaped: its routes (nullptr: not compiled); shaped has K = sk and S = ss compiled in.
struct GroupShape { int G, W, eps, occ; MRoute any, rng, shaped; int sk, ss; };
static const GroupShape wide_shapes[] = { // 6 .. 10 snakes (the first that fits)
    // (no shape-specialised form: with 10 snakes' loops unrolled the kernel spills 89 VGPRs at its 128 and measured 0.657 ms
    // per 4 steps of the speeds.py shape against 0.616 — profiles/r06_shape_kernels_ab.txt)
    {4, 10, 1, 4, &MR_GROUP_5014, &MR_GROUP_5014_RNG, nullptr, 0, 0},
    {4, 5, 1, 4, &MR_GROUP_4514, nullptr, nullptr, 0, 0},
    {2, 10, 1, 4, &MR_GROUP_3014, nullptr, nullptr, 0, 0},
};
static const GroupShape shapes[] = {
    // (automatic: the first that fits.  Measured at cfg4 on four boxes, ms per 16- / 64-step launch: 8 / 2 / 1 / 5 — two
    // writers, the steppers sharing their work, 5 waves per SIMD at 96 VGPRs — 0.484-0.486 / 1.62-1.65 on every box;
    // 8 / 4 / 1 / 6 — a writer per agent, 6 waves per SIMD at 80 VGPRs with 130 bytes of scratch — 0.44-0.51 / 1.57-1.81
    // depending on the box and on how the allocator spills; 4 / 4 / 1 / 4: 0.51 / 1.66; 8 / 4 / 2 / 4: 1.79 per 64;
    // the two-wave kernel of round 3: 0.55 / 1.73-2.15 — profiles/r04_multi_group_probe.txt)
    {8, 2, 1, 5, &MR_GROUP_8215, &MR_GROUP_8215_RNG, nullptr, 0, 0},
    {8, 4, 1, 6, &MR_GROUP_8416, &MR_GROUP_8416_RNG, nullptr, 0, 0},
    // (round 6) BASELINE configs[3] — 4 snakes on 25 x 25 — takes THIS shape with K and S compiled in: 121 VGPRs, no
    // spilled VGPR, no scratch, and per 16- / 64-step launch on two boxes 0.4035 / 0.4278 and - / 1.5335 ms, against
    // 0.4135 / 0.4316 and - / 1.5306 for 8 / 2 / 1 / 5 specialised (34 spilled VGPRs, 140 bytes of scratch) and
    // 0.4305 / 0.4386 and - / 1.5724 for the generic 8 / 2 / 1 / 5 that shipped in round 5 (profiles/r06_group_shapes.txt)
    {4, 4, 1, 4, &MR_GROUP_4414, &MR_GROUP_4414_RNG, &MR_GROUP_4414_RNG_K4_S25, 4, 25},
    {8, 4, 2, 4, &MR_GROUP_8424, nullptr, nullptr, 0, 0},
};

// What multi_launch does for a call: worked out by multi_plan without a HIP call.
struct MultiPlan {
    MRoute route = nullptr;    // nullptr: no kernel takes an env of this size; else route->fn is the kernel
    dim3 grid, block;
    size_t lds = 0;            // dynamic LDS, bytes
    MultiArgs args;            // the kernel's argument: the caller's with the LDS layout, grp_emit, grp_env0 and grp_variant filled in
    bool keeps_mirror = false; // the kernel works from and maintains args.resident (the others know the fp32 planes only)
    bool grouped = false;      // multi_rollout_group_kernel
};

static MultiPlan &plan_kernel(MultiPlan &pl, const MultiKernel &k, long long grid, int block, size_t lds)
{
    pl.route = &k; pl.grid = dim3((unsigned)grid); pl.block = dim3(block); pl.lds = lds;
    return pl;
}

// the grouped rows of multi_plan: the GroupShape that serves this rollout, if any
static bool plan_group(const MultiArgs &p, const Options &o, bool rng, bool shaped, MultiPlan &pl)
{
    const bool wide = p.K > GRP_MAX_SNAKES; // 32-bit class words, one buffer
    auto total = [&](int G) { MultiArgs t = p; return group_layout(t, G, wide); };
    auto fits = [&](const GroupShape &c) { return total(c.G) <= LDS_MAX_BYTES; };
    auto asked = [&](const GroupShape &c) { return 1000 * c.G + 100 * c.W + 10 * c.eps + c.occ == o.multi_group_shape; };
    auto own = [&](const GroupShape &c) { return shaped && c.shaped && c.sk == p.K && c.ss == p.S; };
    const GroupShape *sh = nullptr;
    for (const GroupShape &c : wide_shapes) {
        if (!wide) break;
        if (fits(c) && (o.multi_group_shape == 0 || asked(c))) { sh = &c; break; }
    }
    // a shape whose specialised form serves this launch comes first
    if (!wide && o.multi_group_shape == 0)
        for (const GroupShape &c : shapes)
            if (own(c) && fits(c)) { sh = &c; break; }
    for (const GroupShape &c : shapes) {
        if (wide || sh) break;
        if (o.multi_group_shape ? (asked(c) && fits(c)) : (fits(c) && (c.G == 4 || 2 * total(8) <= LDS_MAX_BYTES))) { sh = &c; break; }
    }
    if (!sh) return false;
    const size_t bytes = (size_t)group_layout(pl.args, sh->G, wide);
    pl.args.grp_variant = (int)o.multi_group_variant;
    pl.keeps_mirror = pl.grouped = true;
    plan_kernel(pl, *(own(*sh) ? sh->shaped : (rng && sh->rng) ? sh->rng : sh->any), (p.N + sh->G - 1) / sh->G, 64 * (sh->G / sh->eps + sh->W), bytes);
    return true;
}

// ---- which kernel serves a call.  ONE table (multi_plan), read top to bottom: the first row whose condition holds wins.
// snap: 'full' observations of at most 10 snakes (SNAP_MAX_SNAKES: class codes in LDS, observe_full_snap); tapes: recorded
// outcomes (inject / reset inject), rng: none; shaped: rng and WURM_MULTI_SHAPE_KERNELS != 0; big: N >= WURM_MULTI_GROUP_MIN_ENVS;
// lds: one env's bytes (multi_layout; the checker: a byte per cell); wpb: envs (waves) per workgroup, 1 below 2048 envs, else 4
// (a big snap step of K <= 5: 4, and there its waves write the observations through class codes: grp_emit), while wpb lds <= 64 KB
//   kind                  | condition                                     | route                                           | workgroup
//   rollout               | snap, T > 1, big, a GroupShape fits 160 KB    | rollout_group_<code>[_rng[_k4_s25]] (plan_group) | G envs, G / EPS + W waves
//   any                   | lds > 160 KB                                  | none: WURM_ERR_UNSUPPORTED
//   rollout               | snap, T > 1                                   | rollout_two[_rng]                               | one env, 2 waves
//   step, reset, observe  | 4 lds > 64 KB, snap or no observation written | step_wg[_rng[_full_k10_s36]], reset_wg, observe_wg | one env, 4 waves
//   step                  | tapes                                         | step                                            | wpb envs
//   step                  | shaped, K = 4, S = 25, partial_5 / 'full'; K = 2, S = 12, 'full' | step_rng_partial_k4_s25_n5 / step_rng_full_k4_s25; step_rng_full_k2_s12
//   step                  | 'full' / partial_n / none                     | step_rng_full / step_rng_partial / step_rng_none
//   reset, observe, check | -                                             | reset, observe, check
//   rollout               | tapes                                         | rollout
//   rollout               | shaped, K = 4, S = 25, partial_5              | rollout_rng_partial_k4_s25_n5
//   rollout               | partial_n / none / 'full' (T = 1 or K > 10)   | rollout_rng_partial / rollout_rng_none / rollout_rng
static MultiPlan multi_plan(MKind kind, const MultiArgs &p, const Options &o)
{
    MultiPlan pl;
    pl.args = p;
    MultiArgs &q = pl.args;
    const bool snap = p.obs_mode == WURM_OBS_DEFAULT && p.K <= SNAP_MAX_SNAKES;
    // rollouts double-buffer the class codes between a stepping and a writing wave (multi_rollout_kernel<true>)
    const bool two = kind == MK_ROLLOUT && snap && p.T > 1;
    const bool rng = !p.has_inj && !p.has_rinj, shaped = rng && o.multi_shape_kernels != 0, big = p.N >= o.multi_group_min_envs;
    pl.keeps_mirror = kind == MK_STEP || (kind == MK_ROLLOUT && !two);
    // large batches: G consecutive envs per workgroup, one linear observation run per agent (multi_rollout_group_kernel)
    if (two && p.K <= GRP_MAX_SNAKES32 && big && plan_group(p, o, rng, shaped, pl)) return pl;
    int lds = multi_layout(q, p.obs_mode == WURM_OBS_PARTIAL, snap ? (two ? 2 : 1) : 0);
    if (kind == MK_CHECK) lds = q.lds_per_wave = (p.S * p.S + 15) & ~15; // the checker keeps one byte per cell
    // One env's grids must fit the LDS of a CU.  Up to 64 KB is the default limit of a launch; beyond it the kernel is
    // opted into CDNA4's 160 KB per workgroup (one env per CU at a time, e.g. 32 snakes on 36 x 36: 90 KB).  Larger envs
    // (2 K S^2 + 3 S^2 bytes and change > 160 KB, e.g. S = 64 with K > 18) are UNSUPPORTED (DESIGN.md §5 deviation 10).
    if (lds > LDS_MAX_BYTES) return pl;
    if (two) return plan_kernel(pl, rng ? MR_ROLLOUT_TWO_RNG : MR_ROLLOUT_TWO, p.N, 128, (size_t)lds);
    if ((kind == MK_STEP || kind == MK_RESET || (kind == MK_OBSERVE && snap)) && lds * 4 > 65536 &&
        (snap || p.obs_mode == WURM_OBS_NONE)) {
        // an env too large for four per workgroup: one env per workgroup of four waves (multi_step_wg_kernel)
        q.grp_variant = (int)o.multi_group_variant;
        return plan_kernel(pl, kind == MK_RESET ? MR_RESET_WG : kind == MK_OBSERVE ? MR_OBSERVE_WG : !rng ? MR_STEP_WG
                               : (shaped && snap && p.K == 10 && p.S == 36) ? MR_STEP_WG_RNG_FULL_K10_S36 : MR_STEP_WG_RNG, p.N, 256, (size_t)lds);
    }
    // few envs: one wave per workgroup so that they spread over all 256 CUs; from 2048 envs on 4 waves per workgroup
    // (8 workgroups per CU either way; the observation stream of 4096 envs measured ~5 % faster this way)
    const bool want_group = kind == MK_STEP && snap && p.K <= GRP_MAX_SNAKES && big;
    int wpb = (p.N < 2048 && !want_group) ? 1 : 4;
    while (wpb > 1 && lds * wpb > 65536) wpb >>= 1;
    size_t extra = 0;
    if (want_group && wpb == 4 && o.multi_group_step_wpb != 0) {
        // large batches: 'full' observations through per-agent class codes and the colour table (class_write, grp_emit_cells).
        // Option WURM_MULTI_GROUP_STEP_WPB: 0 = off; 1 (and -1, automatic) = every wave writes its own env's K views, no
        // barrier; 4 / 8 = the workgroup's waves write one linear run per agent together, that many envs per workgroup.
        // One call's observations (123 MB at cfg4) are absorbed by the 256 MB Infinity Cache — the per-call launch is a chain
        // of latencies (tools/multi_timeline.py), not a stream, so the barrier of the shared form costs more than its
        // longer runs gain: 36.8 against 37.8 us per iteration at cfg4 (profiles/r04_multi_percall_timeline.txt).
        const long long mode = o.multi_group_step_wpb < 0 ? 1 : o.multi_group_step_wpb;
        extra = GRP_TAB_BYTES + GRP_CODE_SLACK;
        if (2 * (8 * (size_t)lds + extra) <= (size_t)LDS_MAX_BYTES && mode != 4 && mode != 1) wpb = 8;
        q.grp_emit = mode == 1 ? 2 : 1;
        q.grp_env0 = lds * wpb; // the table, behind the envs' blocks
    }
    const bool k4_s25 = shaped && p.K == 4 && p.S == 25, k4_s25_n5 = k4_s25 && p.obs_mode == WURM_OBS_PARTIAL && p.obs_n == 5;
    const bool full = p.obs_mode == WURM_OBS_DEFAULT, partial = p.obs_mode == WURM_OBS_PARTIAL;
    MRoute r = kind == MK_RESET ? &MR_RESET : kind == MK_OBSERVE ? &MR_OBSERVE : &MR_CHECK;
    if (kind == MK_STEP)
        r = &(!rng ? MR_STEP : k4_s25_n5 ? MR_STEP_RNG_PARTIAL_K4_S25_N5 : (k4_s25 && full) ? MR_STEP_RNG_FULL_K4_S25
          : (shaped && p.K == 2 && p.S == 12 && full) ? MR_STEP_RNG_FULL_K2_S12
          : full ? MR_STEP_RNG_FULL : partial ? MR_STEP_RNG_PARTIAL : MR_STEP_RNG_NONE);
    if (kind == MK_ROLLOUT)
        r = &(!rng ? MR_ROLLOUT : k4_s25_n5 ? MR_ROLLOUT_RNG_PARTIAL_K4_S25_N5 : partial ? MR_ROLLOUT_RNG_PARTIAL
          : p.obs_mode == WURM_OBS_NONE ? MR_ROLLOUT_RNG_NONE : MR_ROLLOUT_RNG);
    return plan_kernel(pl, *r, (p.N + wpb - 1) / wpb, 64 * wpb, (size_t)lds * wpb + extra);
}

// (wurm_multi_last_route: the kernel of the CALLING THREAD's last launch and how it was driven — a diagnostic the tests name a
// launch by; no state that a later call depends on)
struct MultiLast { MRoute route; int grp_emit; bool tapes; };
static thread_local MultiLast multi_last = {nullptr, 0, false};

static int multi_launch(MKind kind, MultiArgs &p, void *stream)
{
    if (p.N == 0) return WURM_OK;
    MultiPlan pl = multi_plan(kind, p, opt);
    if (pl.route == nullptr) return WURM_ERR_UNSUPPORTED;
    multi_last = {pl.route, pl.args.grp_emit, p.has_inj || p.has_rinj};
    const void *fn = (const void *)pl.route->fn;
    (void)hipGetLastError();
    // dynamic LDS beyond the default 64 KB of a launch needs the kernel's opt-in (allow_lds)
    if (pl.lds > 65536 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds) != hipSuccess) return WURM_ERR_HIP;
    void *args[] = {&pl.args};
    launch_count.fetch_add(1, std::memory_order_relaxed);
    if (hipLaunchKernel(fn, pl.grid, pl.block, args, pl.lds, (hipStream_t)stream) != hipSuccess) return WURM_ERR_HIP;
    if (pl.grouped) p.resident_used = 1; // (the kernel keeps the caller's mirror, if one was given)
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

static long long multi_obs_elems(int mode, int n, int S)
{
    if (mode == WURM_OBS_DEFAULT) return 3ll * S * S;
    if (mode == WURM_OBS_PARTIAL && n >= 0) return 3ll * (2 * n + 1) * (2 * n + 1);
    return 0;
}

static int multi_check_args(long long N, int K, int S, int mode, int n, const void *obs)
{
    if (N < 0 || K < 1 || S < 3) return WURM_ERR_INVALID_ARG;
    if (K > 64 || S > 64) return WURM_ERR_UNSUPPORTED;
    if (mode != WURM_OBS_NONE) {
        if (multi_obs_elems(mode, n, S) == 0) return WURM_ERR_INVALID_ARG;
        if (N > 0 && obs == nullptr) return WURM_ERR_INVALID_ARG;
    }
    return WURM_OK;
}


// the state pointers and the shape, as every entry point hands them to a kernel
static MultiArgs multi_args(const float *foods, const float *heads, const float *bodies, const uint8_t *dones,
                            const int64_t *orientations, const int16_t *colours, float *obs, int obs_mode, int obs_n,
                            int64_t num_envs, int num_snakes, int size)
{
    MultiArgs p = {};
    p.foods = const_cast<float *>(foods); p.heads = const_cast<float *>(heads); p.bodies = const_cast<float *>(bodies);
    p.dones = const_cast<uint8_t *>(dones); p.orientations = (long long *)orientations; p.colours = const_cast<short *>(colours);
    p.obs = obs; p.obs_mode = obs_mode; p.obs_n = obs_n; p.obs_elems = multi_obs_elems(obs_mode, obs_n, size);
    p.N = num_envs; p.K = num_snakes; p.S = size;
    return p;
}

// what the two rollout entries check and fill alike (the tapes and the mirror are theirs)
static int multi_rollout_args(MultiArgs &p, float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                              int16_t *colours, uint8_t *boost_this_step, const int64_t *actions, float *out_f32, uint8_t *out_u8,
                              uint8_t *all_done, float *obs, int obs_mode, int obs_n, int64_t num_envs, int num_snakes, int size,
                              int64_t num_steps, const wurm_multi_config *cfg, uint64_t seed, uint64_t call0, int64_t env_offset)
{
    if (int rc = multi_check_args(num_envs, num_snakes, size, obs_mode, obs_n, obs)) return rc;
    if (!cfg || num_steps < 0) return WURM_ERR_INVALID_ARG;
    if (size < 5) return WURM_ERR_UNSUPPORTED;
    if (num_envs > 0 && (!foods || !heads || !bodies || !dones || !orientations || !colours)) return WURM_ERR_INVALID_ARG;
    if (num_envs > 0 && num_steps > 0 && (!actions || !out_f32 || !out_u8 || !all_done)) return WURM_ERR_INVALID_ARG;
    p = multi_args(foods, heads, bodies, dones, orientations, colours, obs, obs_mode, obs_n, num_envs, num_snakes, size);
    p.boost_state = boost_this_step; p.actions = (const long long *)actions; p.am_f32 = out_f32; p.am_u8 = out_u8;
    p.all_done = all_done; p.T = num_steps;
    p.cfg = *cfg; p.seed = seed; p.call = call0; p.env_offset = env_offset;
    return WURM_OK;
}

} // namespace wurm

using namespace wurm;

extern "C" {

int64_t wurm_multi_obs_elems(int obs_mode, int obs_n, int size) { return multi_obs_elems(obs_mode, obs_n, size); }

const char *wurm_multi_last_route(void)
{
    static thread_local char name[64];
    snprintf(name, sizeof name, "%s%s%s", multi_last.route ? multi_last.route->name : "none",
             multi_last.grp_emit == 1 ? "+emit_group" : multi_last.grp_emit == 2 ? "+emit_wave" : "", multi_last.tapes ? "/tapes" : "");
    return name;
}

int wurm_multi_step(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                    const int64_t *actions, uint8_t *boost_this_step, float *rewards, uint8_t *snake_collision,
                    uint8_t *edge_collision, float *food_consumed, float *sizes, uint8_t *all_done,
                    const int16_t *colours, float *obs, int obs_mode, int obs_n, int64_t num_envs, int num_snakes,
                    int size, const wurm_multi_config *cfg, uint64_t seed, uint64_t call, int64_t env_offset,
                    const wurm_multi_inject *inject, float *agent_major_f32, uint8_t *agent_major_u8, void *stream)
{
    if (int rc = multi_check_args(num_envs, num_snakes, size, obs_mode, obs_n, obs)) return rc;
    if (!cfg) return WURM_ERR_INVALID_ARG;
    wurm_multi_call c = {}; // (the same checks, the same argument block: one path for the per-call step)
    c.foods = foods; c.heads = heads; c.bodies = bodies; c.dones = dones; c.orientations = orientations; c.actions = actions;
    c.boost_this_step = boost_this_step; c.rewards = rewards; c.snake_collision = snake_collision; c.edge_collision = edge_collision;
    c.food_consumed = food_consumed; c.sizes = sizes; c.all_done = all_done; c.colours = const_cast<int16_t *>(colours); c.obs = obs;
    c.obs_mode = obs_mode; c.obs_n = obs_n; c.num_envs = num_envs; c.num_snakes = num_snakes; c.size = size; c.cfg = *cfg;
    c.seed = seed; c.call = call; c.env_offset = env_offset; c.inject = inject; c.agent_major_f32 = agent_major_f32;
    c.agent_major_u8 = agent_major_u8;
    return wurm_multi_step_reset(&c, stream);
}

int wurm_multi_step_reset(const wurm_multi_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    int rc = multi_check_args(c->num_envs, c->num_snakes, c->size, c->obs_mode, c->obs_n, c->obs);
    if (rc) return rc;
    if (c->num_envs > 0 && (!c->foods || !c->heads || !c->bodies || !c->dones || !c->orientations || !c->actions ||
                            !c->boost_this_step || !c->rewards || !c->snake_collision || !c->edge_collision ||
                            !c->food_consumed || !c->sizes || !c->all_done))
        return WURM_ERR_INVALID_ARG;
    if ((c->obs_mode == WURM_OBS_PARTIAL || c->pre_done) && c->num_envs > 0 && !c->colours) return WURM_ERR_INVALID_ARG;
    if ((c->pre_done || c->obs_after) && c->size < 5) return WURM_ERR_UNSUPPORTED;
    if (c->obs_after && c->pre_inject) return WURM_ERR_UNSUPPORTED; // the reset behind obs_after draws from the RNG
    MultiArgs p = multi_args(c->foods, c->heads, c->bodies, c->dones, c->orientations, c->colours, c->obs, c->obs_mode, c->obs_n,
                             c->num_envs, c->num_snakes, c->size);
    p.actions = (const long long *)c->actions; p.boost = c->boost_this_step; p.rewards = c->rewards;
    p.snakecol = c->snake_collision; p.edgecol = c->edge_collision; p.foodcons = c->food_consumed; p.sizes = c->sizes;
    p.all_done = c->all_done; p.all_done_copy = c->all_done_copy; p.obs_after = c->obs_after;
    p.cfg = c->cfg; p.seed = c->seed; p.call = c->call; p.env_offset = c->env_offset;
    p.done_env = c->pre_done; p.pre_call = c->pre_call;
    if (c->inject) { p.inj = *c->inject; p.has_inj = 1; }
    if (c->pre_inject) { p.rinj = *c->pre_inject; p.has_rinj = 1; }
    if (c->agent_major_f32 && c->agent_major_u8) { p.am_f32 = c->agent_major_f32; p.am_u8 = c->agent_major_u8; }
    p.err = c->check_mask; p.err_after = c->check_mask_after;
    if (c->resident && c->num_envs > 0) {
        if (!c->inject && !c->pre_inject) {
            p.resident = (unsigned char *)c->resident; p.resident_valid = c->resident_valid != 0; p.resident_lazy = c->resident_lazy != 0;
        } else if (c->resident_lazy && c->resident_valid) { // recorded outcomes step the fp32 state: write the mirror out first
            rc = wurm_multi_resident_flush(c, stream);
            if (rc) return rc;
        }
    }
    return multi_launch(MK_STEP, p, stream);
}

int64_t wurm_multi_resident_size(int64_t num_envs, int num_snakes, int size)
{
    if (num_envs <= 0 || num_snakes < 1 || num_snakes > 64 || size < 5 || size > 64) return 0;
    return num_envs * mirror_env_bytes(num_snakes, size * size);
}

int64_t wurm_multi_resident_bytes(int64_t num_envs, int num_snakes, int size)
{
    const long long e = opt.resident_min_envs; // -1: by shape
    const bool big = e >= 0 ? num_envs >= e : num_envs * (long long)num_snakes * size * size >= (1ll << 20);
    return big ? wurm_multi_resident_size(num_envs, num_snakes, size) : 0;
}

int wurm_multi_resident_flush(const wurm_multi_call *c, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (!c->resident || !c->resident_lazy || !c->resident_valid || c->num_envs <= 0) return WURM_OK;
    if (!c->foods || !c->heads || !c->bodies) return WURM_ERR_INVALID_ARG;
    MultiArgs p = multi_args(c->foods, c->heads, c->bodies, nullptr, nullptr, nullptr, nullptr, WURM_OBS_NONE, 0, c->num_envs,
                             c->num_snakes, c->size);
    p.resident = (unsigned char *)c->resident;
    (void)hipGetLastError();
    WURM_LAUNCH(multi_flush_kernel, dim3((unsigned)p.N), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

int wurm_multi_step_packed(wurm_multi_call *c, float *out_f32, uint8_t *out_u8, float *obs, float *obs_after,
                           const int64_t *actions, uint64_t call, int apply_pending, uint64_t pre_call, void *stream)
{
    if (!c) return WURM_ERR_INVALID_ARG;
    if (c->num_envs > 0 && (!out_f32 || !out_u8)) return WURM_ERR_INVALID_ARG;
    if (apply_pending && !c->all_done_copy) return WURM_ERR_INVALID_ARG;
    const long long KN = (long long)c->num_snakes * c->num_envs;
    c->rewards = out_f32; c->food_consumed = out_f32 + KN; c->sizes = out_f32 + 2 * KN; c->agent_major_f32 = out_f32 + 3 * KN;
    c->boost_this_step = out_u8; c->snake_collision = out_u8 + KN; c->edge_collision = out_u8 + 2 * KN;
    c->agent_major_u8 = out_u8 + 3 * KN; c->all_done = out_u8 + 7 * KN;
    c->obs = obs; c->obs_after = obs_after; c->actions = actions; c->call = call;
    c->pre_done = apply_pending ? c->all_done_copy : nullptr; c->pre_call = pre_call;
    const int rc = wurm_multi_step_reset(c, stream);
    if (c->resident) c->resident_valid = (rc == WURM_OK && !c->inject && !c->pre_inject) ? 1 : 0;
    return rc;
}

int wurm_multi_step_slot(wurm_multi_call *c, const wurm_multi_slabs *slabs, int64_t slot, const int64_t *actions,
                         uint64_t call, int apply_pending, uint64_t pre_call, int want_obs_after, void *stream)
{
    if (!c || !slabs || slot < 0 || slot >= slabs->steps) return WURM_ERR_INVALID_ARG;
    if (want_obs_after && !slabs->obs_after) return WURM_ERR_INVALID_ARG;
    const long long KN = (long long)c->num_snakes * c->num_envs, per_obs = KN * slabs->obs_elems;
    return wurm_multi_step_packed(c, slabs->out_f32 ? slabs->out_f32 + slot * 6 * KN : nullptr,
                                  slabs->out_u8 ? slabs->out_u8 + slot * (7 * KN + c->num_envs) : nullptr,
                                  slabs->obs ? slabs->obs + slot * per_obs : nullptr,
                                  want_obs_after ? slabs->obs_after + slot * per_obs : nullptr, actions, call, apply_pending,
                                  pre_call, stream);
}

int wurm_multi_reset(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                     int16_t *colours, const uint8_t *done_env, int32_t *status, const uint8_t *boost_this_step,
                     float *obs, int obs_mode, int obs_n, int64_t num_envs, int num_snakes, int size,
                     const wurm_multi_config *cfg, uint64_t seed, uint64_t call, int64_t env_offset,
                     const wurm_multi_reset_inject *inject, void *stream)
{
    if (int rc = multi_check_args(num_envs, num_snakes, size, obs_mode, obs_n, obs)) return rc;
    if (!cfg) return WURM_ERR_INVALID_ARG;
    if (size < 5) return WURM_ERR_UNSUPPORTED; // no cell is >= 2 from the border (multi_snake.py:938-941)
    if (num_envs > 0 && (!foods || !heads || !bodies || !dones || !orientations || !done_env || !colours))
        return WURM_ERR_INVALID_ARG;
    if (obs_mode != WURM_OBS_NONE && num_envs > 0 && !boost_this_step) return WURM_ERR_INVALID_ARG;
    MultiArgs p = multi_args(foods, heads, bodies, dones, orientations, colours, obs, obs_mode, obs_n, num_envs, num_snakes, size);
    p.done_env = done_env; p.status = status; p.boost = const_cast<uint8_t *>(boost_this_step);
    p.cfg = *cfg; p.seed = seed; p.call = call; p.env_offset = env_offset;
    if (inject) { p.rinj = *inject; p.has_rinj = 1; }
    return multi_launch(MK_RESET, p, stream);
}

int wurm_multi_rollout(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                       int16_t *colours, uint8_t *boost_this_step, const int64_t *actions, float *out_f32,
                       uint8_t *out_u8, uint8_t *all_done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                       int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg, uint64_t seed,
                       uint64_t call0, int64_t env_offset, const wurm_multi_inject *inject,
                       const wurm_multi_reset_inject *reset_inject, void *stream)
{
    MultiArgs p;
    const int rc = multi_rollout_args(p, foods, heads, bodies, dones, orientations, colours, boost_this_step, actions, out_f32,
                                      out_u8, all_done, obs, obs_mode, obs_n, num_envs, num_snakes, size, num_steps, cfg, seed,
                                      call0, env_offset);
    if (rc || num_steps == 0) return rc;
    if (inject) { p.inj = *inject; p.has_inj = 1; }
    if (reset_inject) { p.rinj = *reset_inject; p.has_rinj = 1; }
    if ((inject == nullptr) != (reset_inject == nullptr)) return WURM_ERR_INVALID_ARG; // replay needs both tapes
    return multi_launch(MK_ROLLOUT, p, stream);
}

int wurm_multi_rollout_resident(float *foods, float *heads, float *bodies, uint8_t *dones, int64_t *orientations,
                                int16_t *colours, uint8_t *boost_this_step, const int64_t *actions, float *out_f32,
                                uint8_t *out_u8, uint8_t *all_done, float *obs, int obs_mode, int obs_n, int64_t num_envs,
                                int num_snakes, int size, int64_t num_steps, const wurm_multi_config *cfg, uint64_t seed,
                                uint64_t call0, int64_t env_offset, void *resident, int *resident_valid, int resident_lazy,
                                void *stream)
{
    if (resident == nullptr)
        return wurm_multi_rollout(foods, heads, bodies, dones, orientations, colours, boost_this_step, actions, out_f32, out_u8,
                                  all_done, obs, obs_mode, obs_n, num_envs, num_snakes, size, num_steps, cfg, seed, call0,
                                  env_offset, nullptr, nullptr, stream);
    if (resident_valid == nullptr) return WURM_ERR_INVALID_ARG;
    MultiArgs p;
    int rc = multi_rollout_args(p, foods, heads, bodies, dones, orientations, colours, boost_this_step, actions, out_f32, out_u8,
                                all_done, obs, obs_mode, obs_n, num_envs, num_snakes, size, num_steps, cfg, seed, call0, env_offset);
    if (rc || num_steps == 0 || num_envs == 0) return rc;
    // the kernels that keep a mirror: the grouped writer, and the one-wave-per-env rollout (everything but 'full'
    // observations of at most 10 snakes over several steps in a small batch, which goes to the two-wave form)
    if (multi_plan(MK_ROLLOUT, p, opt).keeps_mirror) {
        p.resident = (unsigned char *)resident; p.resident_valid = *resident_valid != 0; p.resident_lazy = resident_lazy != 0;
        rc = multi_launch(MK_ROLLOUT, p, stream);
        if (rc == WURM_OK) *resident_valid = 1;
        return rc;
    }
    // any other rollout kernel works on the fp32 planes: a lazy mirror is written out to them first, and it is stale afterwards
    wurm_multi_call c = {};
    c.foods = foods; c.heads = heads; c.bodies = bodies; c.num_envs = num_envs; c.num_snakes = num_snakes; c.size = size;
    c.resident = resident; c.resident_valid = *resident_valid; c.resident_lazy = resident_lazy;
    if ((rc = wurm_multi_resident_flush(&c, stream)) != WURM_OK) return rc;
    *resident_valid = 0;
    return multi_launch(MK_ROLLOUT, p, stream);
}

int wurm_multi_observe(const float *foods, const float *heads, const float *bodies, const uint8_t *dones,
                       const uint8_t *boost_this_step, const int16_t *colours, float *obs, int obs_mode, int obs_n,
                       int64_t num_envs, int num_snakes, int size, void *stream)
{
    if (obs_mode == WURM_OBS_NONE) return WURM_ERR_INVALID_ARG;
    if (int rc = multi_check_args(num_envs, num_snakes, size, obs_mode, obs_n, obs)) return rc;
    if (num_envs > 0 && (!foods || !heads || !bodies || !dones || !boost_this_step)) return WURM_ERR_INVALID_ARG;
    if (obs_mode == WURM_OBS_PARTIAL && num_envs > 0 && !colours) return WURM_ERR_INVALID_ARG;
    MultiArgs p = multi_args(foods, heads, bodies, dones, nullptr, colours, obs, obs_mode, obs_n, num_envs, num_snakes, size);
    p.boost = const_cast<uint8_t *>(boost_this_step);
    return multi_launch(MK_OBSERVE, p, stream);
}

int wurm_multi_check(const float *foods, const float *heads, const float *bodies, const uint8_t *dones, uint32_t *err,
                     int64_t num_envs, int num_snakes, int size, void *stream)
{
    if (int rc = multi_check_args(num_envs, num_snakes, size, WURM_OBS_NONE, 0, nullptr)) return rc;
    if (num_envs > 0 && (!foods || !heads || !bodies || !dones || !err)) return WURM_ERR_INVALID_ARG;
    MultiArgs p = multi_args(foods, heads, bodies, dones, nullptr, nullptr, nullptr, WURM_OBS_NONE, 0, num_envs, num_snakes, size);
    p.err = err;
    return multi_launch(MK_CHECK, p, stream);
}

int wurm_multi_colours(int16_t *colours, int64_t num_envs, int num_snakes, int fixed, uint64_t seed, uint64_t call,
                       int64_t env_offset, void *stream)
{
    if (num_envs < 0 || num_snakes < 1) return WURM_ERR_INVALID_ARG;
    if (num_envs == 0) return WURM_OK;
    if (!colours) return WURM_ERR_INVALID_ARG;
    long long n = (long long)num_envs * num_snakes;
    (void)hipGetLastError();
    WURM_LAUNCH(multi_colours_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       colours, (long long)num_envs, num_snakes, fixed, seed, call, (long long)env_offset);
    return hipGetLastError() == hipSuccess ? WURM_OK : WURM_ERR_HIP;
}

} // extern "C"
