// multi_device.hpp — MultiSnake (multi_snake.hip): the argument block, the LDS image of an env, the device functions of a step.
#pragma once
#include <type_traits>

#include "wurm_device.hpp"
#include "../../include/wurm_hip.h"

namespace wurm {

constexpr unsigned short DIRTY = 0x8000u;
constexpr unsigned short VMASK = 0x7fffu;
constexpr int CLOCK_DEAD = 0x7fff;   // clock of a deleted snake: every cell of its grid reads 0
#ifndef WURM_MULTI_CLOCK_REBASE
#define WURM_MULTI_CLOCK_REBASE 0x3000
#endif
constexpr int CLOCK_REBASE = WURM_MULTI_CLOCK_REBASE; // rollout: re-base a snake's grid (ex -= T) past this clock

struct MultiArgs {
    float *foods, *heads, *bodies;
    uint8_t *dones;
    long long *orientations;
    const long long *actions;
    uint8_t *boost;
    float *rewards;
    uint8_t *snakecol, *edgecol;
    float *foodcons, *sizes;
    uint8_t *all_done;
    short *colours;
    float *obs;
    float *obs_after;     // multi_step_kernel, nullable: the observation the caller's reset(all_done) will return
    int obs_mode, obs_n;
    long long obs_elems;
    long long N;
    int K, S;
    wurm_multi_config cfg;
    u64 seed, call;
    long long env_offset;
    wurm_multi_inject inj;
    int has_inj;
    const uint8_t *done_env;
    int *status;
    u64 pre_call;            // multi_step_kernel: counter of the postponed reset applied in front of the step
    uint8_t *all_done_copy;  // nullable: second copy of all_done (a buffer the caller cannot modify)
    wurm_multi_reset_inject rinj;
    int has_rinj;
    uint32_t *err;
    uint32_t *err_after;  // step kernels: the mask of the state reset_for_obs_after leaves (with obs_after), nullable
    float *am_f32;
    uint8_t *am_u8;
    long long T;          // rollout: number of fused step+reset iterations
    uint8_t *boost_state; // rollout: boost_this_step (N*K) written back at the end
    int lds_per_wave, off_body, off_food, off_occ, off_hmap, off_img, off_col, off_snap, off_acts;
    int off_tl; // timeline build only: 32 stamp slots per env (WURM_TLS)
    // per-call step: the caller's compact mirror of foods / heads / bodies (wurm_multi_call.resident), nullable; valid: it
    // describes them; lazy: the step does not write them
    unsigned char *resident;
    int resident_valid, resident_lazy;
    // multi_rollout_group_kernel: offsets (bytes, from the start of the workgroup's LDS) of the env blocks, the two class
    // code buffers and the two output buffers, and the size of one env's share of each
    int grp_env0, grp_codes, grp_outs, grp_save, grp_code_bytes, grp_out_bytes;
    int grp_variant; // WURM_MULTI_GROUP_VARIANT.  bit 0 (every build): multi_step_wg_kernel writes whole agent views per wave (A/B switch,
                     // same bytes); multi_rollout_group_kernel, probe build only: bit 2 no observation stores, bit 3 no transition
    int resident_used; // out (host side): the rollout launch kept the mirror (multi_rollout_group_kernel)
    int grp_emit; // multi_step_kernel: the workgroup's waves write the 'full' observations together (grp_env0: the table)
};

struct Ctx {
    int S, C, K, lane, cpl;
    float rcpS;
    int *hcell;            // [K] head cell per snake (-1 = none)
    int *lmax;             // [K] max body value per snake
    int *tclk;             // [K] clock per snake: body value = max(ex - tclk, 0)
    unsigned short *body;  // [K][C] expiry clocks (low 15 bits) | DIRTY
    unsigned char *food;   // [C]
    unsigned char *occ;    // [C] scratch (reset: occupancy)
    unsigned char *hmap;   // [C] head owner + 1 per cell, all-zero outside observe_full
    unsigned short *snap;  // [C] observe_full_snap: class code per cell
    unsigned char *acts;   // [64][K] rollout: the actions of the current 64-step chunk (see multi_rollout_kernel)
    short *img;            // [C][4] env image (partial_n): r, g, b, 0
    float *colf;           // [K][4]: r, g, b, 1 + 0.5*boost
    unsigned long long *tl; // timeline build: stamp slots (WURM_TLS)
    u64 ring;              // bit k <=> cell lane + 64 k lies on the border ring (border_bits), where make_ctx was asked for it
    bool has_ring;
};

extern __shared__ __attribute__((aligned(16))) unsigned char wurm_multi_lds[];

// The LDS of one env (one wave): fills in p's offsets, returns the bytes (host: multi_plan; device: shape_constants)
__host__ __device__ inline int multi_layout(MultiArgs &p, bool need_img, int need_snap)
{
    const int C = p.S * p.S, K = p.K;
    int off = 12 * K;                      // hcell, lmax, tclk
    p.off_col = off; off += 16 * K;        // colf
    off = (off + 15) & ~15;
    p.off_body = off; off += 2 * K * C;
    off = (off + 15) & ~15;
    p.off_food = off; off += C;
    off = (off + 15) & ~15;
    p.off_occ = off; off += C;
    off = (off + 15) & ~15;
    p.off_hmap = off; off += C;
    off = (off + 15) & ~15;
    p.off_img = off; if (need_img) off += 16 * (2 * K + 3); // partial_n: the pixel table (pixel_table), 16 bytes per cell code
    off = (off + 15) & ~15;
    p.off_snap = -1;
    if (need_snap) { p.off_snap = off; off += need_snap * ((2 * C + 15) & ~15); }
    p.off_acts = off; off += 64 * K;
    off = (off + 15) & ~15;
    p.off_tl = p.off_acts;
#ifdef WURM_TIMELINE
    p.off_tl = off; off += 256;
#endif
    p.lds_per_wave = (off + 15) & ~15;
    return p.lds_per_wave;
}

// Shape-specialised kernels (round 6).  KT / ST / NT > 0: the number of snakes, the grid size and the crop radius are
// compile-time constants — the shapes of the reference's own experiments (4 snakes on 25 x 25 with partial_5 crops:
// experiments/multiagent.py:79-86, tests/test_multi_snake_env.py:100-104; 10 snakes on 36 x 36: experiments/speeds.py) — so
// every loop over snakes, rows of 64 cells and window cells has a known trip count, the divisions by S are by a constant and
// the LDS offsets multi_launch worked out are immediates.  Same source, same results (tests/test_multi_shape_kernels.py
// compares the two bit for bit); the generic kernels serve every other shape.  WURM_MULTI_SHAPE_KERNELS = 0 switches them off.
constexpr int SNAP_MAX_SNAKES = 10; // observe_full_snap: 10 mask bits, and owner + 1 <= 11 fits the 4 owner bits
template <int OBS, int KT, int ST, int NT>
__device__ __forceinline__ void shape_constants(MultiArgs &p, bool layout, int snap_buffers = -1)
{
    if (KT > 0) p.K = KT;
    if (ST > 0) p.S = ST;
    if (NT >= 0) p.obs_n = NT;
    if (OBS == WURM_OBS_PARTIAL && NT >= 0) p.obs_elems = 3ll * (2 * NT + 1) * (2 * NT + 1);
    if (OBS == WURM_OBS_DEFAULT && ST > 0) p.obs_elems = 3ll * ST * ST;
    if (layout && KT > 0 && ST > 0 && OBS >= 0) {
        const int snap = snap_buffers >= 0 ? snap_buffers : (OBS == WURM_OBS_DEFAULT && KT <= SNAP_MAX_SNAKES) ? 1 : 0;
        (void)multi_layout(p, OBS == WURM_OBS_PARTIAL, snap);
    }
}

// The prologue of a kernel: its own copy of the argument block with what the instantiation fixes written into it.
// INJ = false: the launch draws its random outcomes itself, the injected-outcome branches fold away; OBS >= 0: the
// observation mode is a constant; KT / ST / NT, layout, snap_buffers: shape_constants.
template <bool INJ, int OBS, int KT, int ST, int NT>
__device__ __forceinline__ MultiArgs kernel_args(const MultiArgs &p_in, bool layout, int snap_buffers = -1)
{
    MultiArgs p = p_in;
    if (!INJ) p.has_inj = p.has_rinj = 0;
    if (OBS >= 0) p.obs_mode = OBS;
    shape_constants<OBS, KT, ST, NT>(p, layout, snap_buffers);
    return p;
}

// bit k of the lane's mask <=> cell lane + 64 k lies on the border ring (:183-186): a property of the grid, worked out once
// per kernel (class_write paints the ring last, over whatever sits there)
__device__ __forceinline__ u64 border_bits(const Ctx &cx)
{
    const int S = cx.S, C = cx.C;
    u64 m = 0;
    for (int k = 0; k < cx.cpl; ++k) {
        const int c = cx.lane + 64 * k, y = div_size(c, cx.rcpS), x = c - y * S;
        if (c < C && (y == 0 || x == 0 || y == S - 1 || x == S - 1)) m |= 1ull << k;
    }
    return m;
}

__device__ __forceinline__ Ctx make_ctx(const MultiArgs &p, int wave, int base_off = 0, bool want_ring = false)
{
    Ctx cx;
    unsigned char *base = wurm_multi_lds + base_off + (size_t)wave * p.lds_per_wave;
    cx.S = p.S;
    cx.C = p.S * p.S;
    cx.K = p.K;
    cx.lane = (int)(threadIdx.x & 63u);
    cx.cpl = (cx.C + 63) >> 6;
    cx.rcpS = 1.0f / (float)p.S;
    cx.hcell = (int *)base;
    cx.lmax = (int *)(base + 4 * p.K);
    cx.tclk = (int *)(base + 8 * p.K);
    cx.body = (unsigned short *)(base + p.off_body);
    cx.food = base + p.off_food;
    cx.occ = base + p.off_occ;
    cx.hmap = base + p.off_hmap;
    cx.snap = (unsigned short *)(base + (p.off_snap >= 0 ? p.off_snap : 0));
    cx.acts = base + p.off_acts;
    cx.img = (short *)(base + p.off_img);
    cx.colf = (float *)(base + p.off_col);
    cx.tl = (unsigned long long *)(base + p.off_tl);
    cx.has_ring = want_ring;
    cx.ring = want_ring ? border_bits(cx) : 0ull;
    return cx;
}

// body value of snake s at cell c
__device__ __forceinline__ int BV(const Ctx &cx, int s, int c)
{
    return max((int)(cx.body[s * cx.C + c] & VMASK) - cx.tclk[s], 0);
}

// ------------------------------------------------------------------------------------------------ load / store

// HBM -> LDS.  Returns the lane's original food bits (bit k = food at cell lane + 64k).
// heads and bodies of one env are each one contiguous run of K*C floats with the same [K][C] layout as the LDS body
// grid, so they are copied as flat lane-strided streams, LOAD_CHUNK dwords per lane in flight at a time (the wave is
// alone with its latency at 16 waves/CU: few large batches of loads, not many small ones).
constexpr int LOAD_CHUNK = 16;

// The per-snake slots of an env with nothing in it yet, by threads 0 .. K - 1: where a load starts, and all that is done for
// an env that is about to be rebuilt — it is not read, the rest is multi_reset_grid(rebuild).  No sync: the caller's.
__device__ __forceinline__ void clear_snake_slots(const Ctx &cx, int tid)
{
    if (tid < cx.K) {
        cx.hcell[tid] = -1;
        cx.lmax[tid] = 0;
        cx.tclk[tid] = 0;
    }
}

// plain (out if want_plain, wave-uniform; a reference, not a pointer: a conditional pointer to a local puts it in scratch):
// the planes held nothing the LDS image cannot represent — food and head values 0 / 1,
// at most one head per snake, body values integers in 0 .. 0x7fff — so lds_check sees all there is to check.
__device__ __forceinline__ u64 load_env(const Ctx &cx, const float *__restrict__ foodp,
                                        const float *__restrict__ headp, const float *__restrict__ bodyp,
                                        bool want_plain, bool &plain)
{
    const int C = cx.C, lane = cx.lane, KC = cx.K * C;
    int odd = 0, nheads = 0;
    clear_snake_slots(cx, lane); // (clocks 0: values are loaded as they are, ex = value)
    for (int c = lane; c < C; c += 64) cx.hmap[c] = 0;
    wave_lds_sync();
    const float rcpC = 1.0f / (float)C;
    for (int base = 0; base < KC; base += 64 * LOAD_CHUNK) {
        float hv[LOAD_CHUNK], bv[LOAD_CHUNK];
#pragma unroll
        for (int j = 0; j < LOAD_CHUNK; ++j) {
            // unconditional loads (index clamped into the env): a `cond ? load : 0` would make the compiler wait
            // for every load at its own join point and serialise the batch
            const int i = min(base + lane + 64 * j, KC - 1);
            hv[j] = headp[i];
            bv[j] = bodyp[i];
        }
#pragma unroll
        for (int j = 0; j < LOAD_CHUNK; ++j) {
            const int i = base + lane + 64 * j;
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
    u64 fbits = 0;
    for (int k0 = 0; k0 < cx.cpl; k0 += LOAD_CHUNK) {
        float fv[LOAD_CHUNK];
#pragma unroll
        for (int j = 0; j < LOAD_CHUNK; ++j) {
            fv[j] = foodp[min(lane + 64 * (k0 + j), C - 1)];
        }
#pragma unroll
        for (int j = 0; j < LOAD_CHUNK; ++j) {
            const int c = lane + 64 * (k0 + j);
            if (k0 + j < cx.cpl && c < C) {
                const int f = fv[j] > 0.5f;
                cx.food[c] = (unsigned char)f;
                fbits |= (u64)f << (k0 + j);
                odd |= (int)(fv[j] != 0.0f && fv[j] != 1.0f);
            }
        }
    }
    wave_lds_sync();
    if (want_plain) // as many heads as snakes that have one <=> nobody has two
        plain = ballot(odd != 0) == 0 && wave_sum_i32(nheads) == popc64(ballot(lane < cx.K && cx.hcell[lane] >= 0));
    return fbits;
}

__device__ __forceinline__ u64 load_env(const Ctx &cx, const float *__restrict__ foodp, const float *__restrict__ headp,
                                        const float *__restrict__ bodyp)
{
    bool unused = false;
    return load_env(cx, foodp, headp, bodyp, false, unused);
}

// A head cell that moved, in a sparse write-back: snake s's head plane has it at hc0 (-1: nowhere), it is at hc now.
__device__ __forceinline__ void store_moved_head(float *__restrict__ headp, int C, int s, int hc0, int hc)
{
    float *hp = headp + (size_t)s * C;
    if (hc0 >= 0) hp[hc0] = 0.0f;
    if (hc >= 0) hp[hc] = 1.0f;
}

// LDS -> HBM: body cells flagged DIRTY, the two head cells that changed, food cells that changed.
// t0_in_lmax: the clocks the snakes had when the env was loaded are in cx.lmax (a state that came from the mirror keeps
// its clocks between calls); else they were 0 (load_env).
__device__ __forceinline__ void store_env(const Ctx &cx, float *__restrict__ foodp, float *__restrict__ headp,
                                          float *__restrict__ bodyp, u64 fbits0, int hc0, int hc, bool full,
                                          bool t0_in_lmax = false)
{
    const int C = cx.C, lane = cx.lane;
    for (int s = 0; s < cx.K; ++s) {
        float *bp = bodyp + (size_t)s * C, *hp = headp + (size_t)s * C;
        const int hs = cx.hcell[s], T = cx.tclk[s], T0 = t0_in_lmax ? cx.lmax[s] : 0;
#pragma unroll 4
        for (int k = 0; k < cx.cpl; ++k) {
            int c = lane + 64 * k;
            if (c < C) {
                const unsigned short v = cx.body[s * C + c];
                // changed since the load: written cells, and — once the clock has moved — every cell that held a value
                if (full || (v & DIRTY) || (T != T0 && (int)(v & VMASK) > T0)) bp[c] = (float)max((int)(v & VMASK) - T, 0);
                if (full) hp[c] = (c == hs) ? 1.0f : 0.0f;
            }
        }
    }
    if (!full && lane < cx.K && hc != hc0) store_moved_head(headp, C, lane, hc0, hc);
    for (int k = 0; k < cx.cpl; ++k) {
        int c = lane + 64 * k;
        if (c < C) {
            int f = cx.food[c] != 0;
            if (full || f != (int)((fbits0 >> k) & 1)) foodp[c] = f ? 1.0f : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the mirror
// wurm_multi_call.resident: per env the LDS image of its grids — the K body grids as 16-bit expiry clocks (without the
// DIRTY bits), the food grid as bytes, and per snake its clock, head cell and length — kept by the caller between calls,
// so that the per-call step copies (2 K + 1) S^2 bytes into LDS instead of reading and converting (1 + 2 K) S^2 fp32.
// Any state load_env accepts is representable (the image IS what load_env produces), so there is no domain and no fallback.
__host__ __device__ __forceinline__ int mirror_body_bytes(int K, int C) { return (2 * K * C + 15) & ~15; }
__host__ __device__ __forceinline__ int mirror_food_bytes(int C) { return (C + 15) & ~15; }
__host__ __device__ __forceinline__ long long mirror_env_bytes(int K, int C)
{
    return (long long)mirror_body_bytes(K, C) + mirror_food_bytes(C) + ((12 * K + 15) & ~15);
}

// mirror -> LDS by `nth` threads (tid 0..nth-1; nth = 64: one wave, then `sync` is a wave-level LDS fence).  Returns the
// thread's food bits in load_env's layout (bit k = food at cell tid + nth * k).  hcell / lmax / tclk as load_env leaves
// them (lmax = the snake's length).
template <typename Sync>
__device__ __forceinline__ u64 mirror_load(const Ctx &cx, const unsigned char *__restrict__ m, int tid, int nth, Sync sync,
                                           bool want_bits = true)
{
    const int C = cx.C, K = cx.K, nb = mirror_body_bytes(K, C) >> 4, nf = mirror_food_bytes(C) >> 4;
    const uint4 *mb = (const uint4 *)m, *mf = (const uint4 *)(m + mirror_body_bytes(K, C));
    const int *ms = (const int *)(m + mirror_body_bytes(K, C) + mirror_food_bytes(C));
    // (the grids start on 16-byte boundaries in LDS and are followed by padding up to the next one: multi_layout)
    uint4 *lb = (uint4 *)cx.body, *lf = (uint4 *)cx.food;
    if (nb <= 8 * nth && nf <= nth) {
        // the whole image in ONE round of loads (cfg4: 313 + 40 sixteen-byte pieces and 12 ints for one wave): bodies, food and
        // the per-snake words are requested before anything is waited for — three dependent round trips took 13 400 cycles of
        // a stepper's 67 000 per call (tools/multi_timeline.py) — and the head map is cleared while they are under way
        uint4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = mb[min(tid + j * nth, nb - 1)];
        const uint4 f = mf[min(tid, nf - 1)];
        int w0 = 0, w1 = 0, w2 = 0;
        if (tid < K) { w0 = ms[tid]; w1 = ms[K + tid]; w2 = ms[2 * K + tid]; }
        for (int c = tid; c < C; c += nth) cx.hmap[c] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (tid + j * nth < nb) lb[tid + j * nth] = v[j];
        if (tid < nf) lf[tid] = f;
        if (tid < K) { cx.tclk[tid] = w0; cx.hcell[tid] = w1; cx.lmax[tid] = w2; }
        WURM_TLS(cx, 13);
    } else {
        for (int i0 = 0; i0 < nb; i0 += 8 * nth) {
            uint4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = mb[min(i0 + tid + j * nth, nb - 1)];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i0 + tid + j * nth < nb) lb[i0 + tid + j * nth] = v[j];
        }
        for (int i = tid; i < nf; i += nth) lf[i] = mf[i];
        if (tid < K) {
            cx.tclk[tid] = ms[tid];
            cx.hcell[tid] = ms[K + tid];
            cx.lmax[tid] = ms[2 * K + tid];
        }
        for (int c = tid; c < C; c += nth) cx.hmap[c] = 0;
    }
    sync();
    u64 fbits = 0;
    if (want_bits) { // (only store_env — the write-back to the fp32 planes — compares with them)
#pragma unroll 5
        for (int k = 0, c = tid; c < C; ++k, c += nth) fbits |= (u64)(cx.food[c] != 0) << k;
    }
    WURM_TLS(cx, 14);
    return fbits;
}

// LDS -> mirror (the DIRTY bits stay behind: they mean "written since the load from fp32").  hc / L: the snake's head
// cell and length as of now (threads 0..K-1).
// sparse: the grids came from this mirror in this launch — only the body cells written since (DIRTY) are stored, and the
// food grid whole (C bytes).
template <typename Sync>
__device__ __forceinline__ void mirror_store(const Ctx &cx, unsigned char *__restrict__ m, int tid, int nth, int hc, int L,
                                             Sync sync, bool sparse = false, u64 fbits0 = 0)
{
    const int C = cx.C, K = cx.K, nb = mirror_body_bytes(K, C) >> 4, nf = mirror_food_bytes(C) >> 4;
    uint4 *mb = (uint4 *)m, *mf = (uint4 *)(m + mirror_body_bytes(K, C));
    int *ms = (int *)(m + mirror_body_bytes(K, C) + mirror_food_bytes(C));
    const uint4 *lb = (const uint4 *)cx.body, *lf = (const uint4 *)cx.food;
    sync();
    const u32 keep = (u32)VMASK * 0x00010001u, dirty = (u32)DIRTY * 0x00010001u;
    (void)fbits0;
    if (sparse) {
        // (LDS reads in batches, the few stores afterwards: read-test-store cell by cell was a chain of dependent LDS round
        // trips — 5 400 cycles of a stepper's 67 000 per call at cfg4)
        unsigned short *mb16 = (unsigned short *)m;
        for (int i0 = 0; i0 < nb; i0 += 4 * nth) {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lb[min(i0 + tid + j * nth, nb - 1)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + tid + j * nth;
                if (i >= nb || ((v[j].x | v[j].y | v[j].z | v[j].w) & dirty) == 0) continue;
                const u32 w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (w[q] & (u32)DIRTY) mb16[8 * i + 2 * q] = (unsigned short)(w[q] & VMASK);
                    if (w[q] & ((u32)DIRTY << 16)) mb16[8 * i + 2 * q + 1] = (unsigned short)((w[q] >> 16) & VMASK);
                }
            }
        }
        // (the food grid whole: C bytes per env — cheaper than finding the few cells that changed)
        for (int i = tid; i < nf; i += nth) mf[i] = lf[i];
    } else {
        for (int i = tid; i < nb; i += nth) {
            uint4 v = lb[i];
            v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
            mb[i] = v;
        }
        for (int i = tid; i < nf; i += nth) mf[i] = lf[i];
    }
    if (tid < K) {
        ms[tid] = cx.tclk[tid];
        ms[K + tid] = hc;
        ms[2 * K + tid] = L;
    }
}

// ------------------------------------------------------------------------------------------------ step pieces

// One phase of MultiSnake.step (boost phase multi_snake.py:509-563, regular phase :613-660) for the snakes
// (lanes) with who == true.  All per-snake values are per-lane (lane = snake index).
__device__ __forceinline__ void run_phase(const Ctx &cx, bool who, int dir, int &hc, int &L, bool &done,
                                          float &reward, float &foodcons, bool &snakecol, bool &edgecol)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    const bool snake = lane < K;
    // move heads (:509 / :613, _move_heads :341-353): by -TAP[dir]; off the grid => the head vanishes
    if (who && hc >= 0) {
        int y = div_size(hc, cx.rcpS), x = hc - y * S;
        int ny = y - tap_y(dir), nx = x - tap_x(dir);
        hc = (ny >= 0 && ny < S && nx >= 0 && nx < S) ? ny * S + nx : -1;
    }
    // food overlap of ALL snakes (:514 / :618); each eaten cell loses its food once (:517-518 / :622)
    const bool ov = snake && hc >= 0 && cx.food[hc] != 0;
    wave_lds_sync();
    if (ov) cx.food[hc] = 0;
    // decay the movers that did not eat (:523-526 / :627-628): their clock advances
    if (who && !ov) cx.tclk[lane] += 1;
    if (who && ov) { // :527-529 / :629-631
        reward += 1.0f;
        foodcons += 1.0f;
    }
    wave_lds_sync();
    // collisions with any body (after the decay) or another snake's head (:534-547 / :636-644)
    bool coll = false;
    if (who && hc >= 0) {
        int sum = 0;
#pragma unroll 4
        for (int t = 0; t < K; ++t) sum += BV(cx, t, hc);
        coll = sum > 0;
    }
    for (int o = 0; o < K; ++o) {
        int ho = lane_value(hc, o);
        if (who && hc >= 0 && o != lane && ho == hc) coll = true;
    }
    done |= coll;
    snakecol |= coll;
    wave_lds_sync();
    // new head segment (:552-555 / :649-652)
    if (who && hc >= 0) {
        int v = BV(cx, lane, hc);
        cx.body[lane * C + hc] = (unsigned short)(((cx.tclk[lane] + v + L + (ov ? 1 : 0)) & VMASK) | DIRTY);
    }
    if (who && ov) L += 1;
    // edge collisions (:560-562 / :657-659)
    if (who && hc >= 0) {
        int y = div_size(hc, cx.rcpS), x = hc - y * S;
        bool e = y == 0 || x == 0 || y == S - 1 || x == S - 1;
        done |= e;
        edgecol |= e;
    }
    wave_lds_sync();
}

// _food_from_death (:416-428) as applied at :565-576 / :662-673.  Returns the number of cells where the food landed on a cell
// that held food already: `self.foods += food_on_death` makes those 2 until the clamp at the end of the phase (:603 / :692),
// and the second phase's _add_food (:680) sums the food plane BEFORE its clamp — the test against max_food sees them twice
// (a dead body over food only comes from a hand-edited state; round 6's fuzz found the step after one: seed 722).
__device__ __forceinline__ int food_from_death(const Ctx &cx, bool done, bool has_body, const uint8_t *inj,
                                               float thr, u64 seed, u64 call, u64 env_id, u32 purpose)
{
    const int S = cx.S, C = cx.C, lane = cx.lane;
    const bool snake = lane < cx.K;
    const u64 dead = ballot(snake && done && has_body);
    if (!dead) return 0;
    int doubled = 0;
    const u64 live = ballot(snake && !done);
    for (int k = 0; k < cx.cpl; ++k) {
        int c = lane + 64 * k;
        if (c >= C) continue;
        int y = div_size(c, cx.rcpS), x = c - y * S;
        if (y == 1 || x == 0 || y == S - 1 || x == S - 1) continue; // :418-421 (row 1, sic)
        bool d = false;
        for (u64 m = dead; m; m &= m - 1) d |= BV(cx, first_bit(m), c) > 0;
        if (!d) continue;
        bool l = false;
        for (u64 m = live; m; m &= m - 1) l |= BV(cx, first_bit(m), c) > 0;
        if (l) continue; // :426 not under a living body
        bool hit = inj ? inj[c] != 0 : cell_u01(seed, call, env_id, purpose, (u32)c) > thr; // :424
        if (hit) { // += 1 then clamp(0,1) (:575,603 / :672,692)
            doubled += (int)(cx.food[c] != 0);
            cx.food[c] = 1;
        }
    }
    wave_lds_sync();
    return wave_sum_i32(doubled);
}

// delete done snakes (:595-596 / :676-677)
__device__ __forceinline__ void delete_done(const Ctx &cx, bool done, bool &has_body, int &hc)
{
    const int lane = cx.lane;
    if (lane < cx.K && done) {
        if (has_body) cx.tclk[lane] = CLOCK_DEAD; // every cell of the grid now reads 0
        has_body = false;
        hc = -1;
    }
    wave_lds_sync();
}

// keeps the 15-bit clocks of long-lived snakes away from the top of their range: ex -= T, T = 0 (values unchanged)
__device__ __forceinline__ bool rebase_clocks(const Ctx &cx)
{
    const int C = cx.C, lane = cx.lane;
    const int myT = lane < cx.K ? cx.tclk[lane] : 0;
    u64 m = ballot(lane < cx.K && myT > CLOCK_REBASE && myT < CLOCK_DEAD);
    if (!m) return false;
    const u64 mine = m;
    while (m) {
        const int s = first_bit(m);
        m &= m - 1;
        unsigned short *b = cx.body + s * C;
        const int T = cx.tclk[s];
        for (int k = 0; k < cx.cpl; ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                const unsigned short v = b[c];
                if (v & VMASK) b[c] = (unsigned short)((v & DIRTY) | max((int)(v & VMASK) - T, 0));
            }
        }
    }
    wave_lds_sync();
    if ((mine >> lane) & 1) cx.tclk[lane] = 0;
    wave_lds_sync();
    return true;
}

// bit k set <=> cell lane + 64k is interior and has no food, head or body on it (:439-445, :393-399).
// Five rows of 64 cells at a time: each snake's clock and head cell come out of lanes 0 .. K-1 (readlane) and its five body
// cells are read together — one LDS round trip per snake and block.  (Cell by cell — K dependent reads each — this scan was
// most of the 21 000 cycles `_add_food` took of a 51 000-cycle step with random_rate food: tools/multi_timeline.py --rollout.)
__device__ __forceinline__ u64 free_cells(const Ctx &cx, int hc, int margin)
{
    const int S = cx.S, C = cx.C, K = cx.K, lane = cx.lane;
    const int myT = lane < K ? cx.tclk[lane] : 0, myH = lane < K ? hc : -1;
    constexpr int U = 5;
    u64 fr = 0;
    for (int k0 = 0; k0 < cx.cpl; k0 += U) {
        int cc[U];
        u32 taken[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cc[u] = min(lane + 64 * (k0 + u), C - 1); // (rows past the grid: the last cell again, dropped below)
            taken[u] = cx.food[cc[u]];
        }
        for (int s = 0; s < K; ++s) {
            const int T = lane_value(myT, s), H = lane_value(myH, s);
            const unsigned short *b = cx.body + s * C;
            u32 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = b[cc[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) taken[u] |= (u32)((int)(v[u] & VMASK) > T) | (u32)(cc[u] == H);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = lane + 64 * (k0 + u);
            const int y = div_size(cc[u], cx.rcpS), x = cc[u] - y * S;
            const bool inside = c < C && y >= margin && x >= margin && y <= S - 1 - margin && x <= S - 1 - margin;
            if (inside && taken[u] == 0) fr |= 1ull << (k0 + u);
        }
    }
    return fr;
}

// the K-th set bit over all lanes' `bits` in row-major cell order (cell = lane + 64k): returns true in the
// lane/bit that owns it through `hit_k` (>= 0), -1 elsewhere
__device__ __forceinline__ int rank_select(const Ctx &cx, u64 bits, int K_rank)
{
    int base = 0, hit = -1;
    for (int k = 0; k < cx.cpl; ++k) {
        bool b = (bits >> k) & 1;
        u64 m = ballot(b);
        if (b && base + rank_below(m) == K_rank) hit = k;
        base += popc64(m);
    }
    return hit;
}

// wave-uniform cell index of the (single) lane/bit chosen by rank_select, -1 if none
__device__ __forceinline__ int selected_cell(int k)
{
    u64 m = ballot(k >= 0);
    if (!m) return -1;
    int owner = first_bit(m);
    return owner + 64 * lane_value(k, owner);
}

__device__ __forceinline__ int count_bits(const Ctx &cx, u64 bits)
{
    int n = 0;
    for (int k = 0; k < cx.cpl; ++k) n += popc64(ballot((bits >> k) & 1));
    return n;
}

// number of food cells of the env: four cells per lane and LDS read (the byte grid starts on a 16-byte boundary), one DPP
// sum — the per-cell form (a read, a ballot and a popcount per row of 64 cells) was 3 000 cycles of every step at cfg4.
// Wave-uniform call sites only (wave_sum_i32).
__device__ __forceinline__ int food_count(const Ctx &cx)
{
    const int C = cx.C, nd = (C + 3) >> 2;
    const u32 *f = (const u32 *)cx.food;
    const u32 last = (C & 3) ? (1u << (8 * (C & 3))) - 1u : 0xffffffffu; // (the bytes behind the grid are padding)
    int n = 0;
#pragma unroll 4
    for (int i = cx.lane; i < nd; i += 64) {
        u32 w = f[i];
        if (i == nd - 1) w &= last;
        n += __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u); // non-zero bytes
    }
    return wave_sum_i32(n);
}

// Per-snake state, one snake per lane (lanes 0..K-1), carried through a step / reset / rollout.
struct Snake {
    int hc;           // head cell, -1 = none
    int L;            // length (max body value)
    bool done;
    long long orient; // stored orientation (multi_snake.py:108,494)
    bool boosted;     // boost_this_step of the last step (brightens the snake in partial_n observations)
    short col[3];     // agent colour
    bool cmap_ok = false; // wave-uniform: cx.hmap holds cell_codes of the state as it is (multi_step_body leaves it; a reset voids it)
};

struct StepRes {
    float reward, foodcons;
    bool snakecol, edgecol, all_done;
};

// v / 255.0f, correctly rounded, for the integers a pixel can hold: one multiplication by the rounded reciprocal and one
// Newton step in fused arithmetic give the IEEE quotient for every integer in [0, 70 000) (checked exhaustively against the
// division in exact rational arithmetic: tests/test_div255.py); anything else takes the division itself (~11 instructions, three
// per pixel: a tenth of the VALU work of a step with partial_n observations).
__device__ __forceinline__ float div255(int v)
{
    const float x = (float)v;
    if ((unsigned)v < 70000u) {
        const float rc = 1.0f / 255.0f;
        const float q = x * rc;
        return __fmaf_rn(__fmaf_rn(-q, 255.0f, x), rc, q);
    }
    return x / 255.0f;
}

} // namespace wurm
