// multi_matchmaking.hpp — the league schedules itself on the device: the line-up of every env DRAWN from integer tickets
// and the order / offsets lists of a line-up BUILT, without a host read (include/wurm_hip.h: wurm_multi_league_draw,
// wurm_multi_league_plan; host side: multi_matchmaking.hip; Python: wurm_amd/envs/_multi_league.py: league_draw,
// league_plan(sync=False)).
//
// league_draw_kernel<KMAX>: ONE ENV PER LANE, 256 envs per workgroup.  The tickets, clamped at 0, are staged once per
// workgroup in LDS when there are at most draw::STAGE of them (every lane then reads the same address: a broadcast); above
// that they are read from global memory at the same, wave-uniform index.  The seats of an env are KMAX registers of its
// lane: the seats are a recursion over KMAX (4, 16 or 64, the smallest that holds num_snakes), so no array is indexed by a
// run-time value and nothing lives in scratch.  Per free seat: one Philox block keyed by (env_offset + i, the draw
// counter, RNG_LEAGUE, the seat), r = mulhi64(w0 << 32 | w1, total), and a walk up the policies that skips the lane's
// seats (without replacement: the pinned ones are seats from the start) until the running sum exceeds r.  The total of
// the pool is kept, not recounted: the sum over all policies less the tickets of the seats taken.  r < total, so the walk
// always ends inside [0, A).  No atomics, no barrier but the one behind the staging, no scratch.
//
// The plan builder: a stable counting sort of the R = K N rows by policy in plan::LAUNCHES = 4 launches, for any number of
// policies A.  The rows are cut into C <= 256 chunks of L consecutive rows (L a multiple of 64, from R alone); a chunk is
// ONE WAVE's, which walks it 64 rows at a time.  Workspace: table (C, A) int32, tile_sum (ceil(A / 256)) int32.
//   1 league_plan_count_kernel    a wave zeroes row c of `table`, then adds one per row of its chunk at its policy:
//                                 integer atomic adds, whose sum does not depend on their order
//   2 league_plan_chunks_kernel   a thread per policy a: table[., a] becomes its exclusive sum over the chunks, the total
//                                 goes to offsets[a + 1], a workgroup's 256 totals to tile_sum
//   3 league_plan_offsets_kernel  a workgroup per 256 policies: the sums of the tiles in front, then the inclusive scan
//                                 of its totals in place: offsets.  The last one also writes `dropped`
//   4 league_plan_place_kernel    a wave per chunk again, 64 rows at a time: the lanes that share a policy are found by
//                                 ballot, each gets offsets[a] + table[c, a] + its rank among them (mbcnt), the first of
//                                 them moves table[c, a] on by their number.  Rows ascending within a wave step, the
//                                 steps in order, the chunks by the scan: stable.  order[j] = -1 for j >= offsets[A].
// A row whose entry is outside [0, A) is counted nowhere and placed nowhere.  No grid-wide barrier: the launches order
// the passes.  Every index is checked against the array it goes into before the store.
#pragma once

#include <algorithm>

#include "wurm_device.hpp"

namespace wurm {

namespace draw {

constexpr int THREADS = 256, STAGE = 256, MAX_SEATS = 64;

struct args {
    const int *tickets;    // (A), nullable: one ticket each
    long long *lineup;     // (K, N)
    long long N, env_offset;
    u64 seed, call;
    int K, A, replacement;
    int pinned[MAX_SEATS]; // -1: drawn
};

} // namespace draw

namespace draw {

// what a lane carries from seat to seat
template <int KMAX>
struct lane_state {
    int seat[KMAX];  // the policy of seat k; -1: not seated yet (or no such seat)
    u64 pool_total;  // tickets in the pool
    int pool_size;   // members of the pool
};

// Seats K0, K0 + 1, ... of one env.  A recursion over the seat, not a loop: every index into `seat` is a constant
// whatever the optimizer makes of an unroll request, so the array is registers.
template <int K0, int KMAX, typename Ticket>
__device__ __forceinline__ void seats_from(const args &g, lane_state<KMAX> &s, u64 env_id, long long i, const Ticket &ticket)
{
    if constexpr (K0 < KMAX) {
        if (K0 >= g.K) return;
        if (s.seat[K0] < 0) { // (wave-uniform: the pins are the launch's)
            const bool flat = s.pool_total == 0; // nobody in the pool holds a ticket: one each
            const u64 total = flat ? (u64)s.pool_size : s.pool_total;
            const Words w = rng_words(g.seed, g.call, env_id, RNG_LEAGUE, (u32)K0);
            const u64 r = __umul64hi(((u64)w.w[0] << 32) | w.w[1], total);
            u64 run = 0;
            int pick = -1;
            for (int a = 0; a < g.A; ++a) {
                bool out = false;
                if (!g.replacement) {
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) out = out || s.seat[j] == a;
                }
                if (out) continue;
                run += flat ? 1 : ticket(a);
                if (run > r) {
                    pick = a;
                    break;
                }
            }
            s.seat[K0] = pick;
            if (!g.replacement && pick >= 0) {
                s.pool_total -= ticket(pick);
                --s.pool_size;
            }
        }
        g.lineup[(long long)K0 * g.N + i] = s.seat[K0];
        seats_from<K0 + 1, KMAX>(g, s, env_id, i, ticket);
    }
}

} // namespace draw

template <int KMAX>
__global__ __launch_bounds__(draw::THREADS) void league_draw_kernel(draw::args g)
{
    using namespace draw;
    __shared__ int staged[STAGE];
    const bool use_lds = g.A <= STAGE;
    if (use_lds) {
        for (int a = (int)threadIdx.x; a < g.A; a += THREADS) staged[a] = g.tickets ? max(g.tickets[a], 0) : 1;
        __syncthreads();
    }
    auto ticket = [&](int a) -> u64 { // a wave-uniform, 0 <= a < A
        return (u64)(use_lds ? staged[a] : g.tickets ? max(g.tickets[a], 0) : 1);
    };
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= g.N) return;

    // wave-uniform: the sum over every policy, and what the pinned seats take out of the pool
    lane_state<KMAX> s;
    s.pool_total = 0;
    for (int a = 0; a < g.A; ++a) s.pool_total += ticket(a);
    s.pool_size = g.A;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        s.seat[k] = k < g.K ? g.pinned[k] : -1;
        if (!g.replacement && s.seat[k] >= 0) {
            s.pool_total -= ticket(s.seat[k]);
            --s.pool_size;
        }
    }
    seats_from<0, KMAX>(g, s, (u64)(g.env_offset + i), i, ticket);
}

// ---- the plan ---------------------------------------------------------------------------------------------------------

namespace plan {

constexpr int LAUNCHES = 4, THREADS = 256, WAVES = THREADS / 64, MAX_CHUNKS = 256, TILE = 256;

// rows per chunk: a multiple of 64, at most MAX_CHUNKS chunks
inline long long chunk_rows(long long R) { return std::max(1LL, ((R + MAX_CHUNKS - 1) / MAX_CHUNKS + 63) / 64) * 64; }
inline long long num_chunks(long long R) { return (R + chunk_rows(R) - 1) / chunk_rows(R); }
inline long long num_tiles(long long A) { return (A + TILE - 1) / TILE; }

struct args {
    const void *lineup;   // (R) of `dtype`
    int *order;           // (R)
    long long *offsets;   // (A + 1)
    int *dropped;         // scalar
    int *table;           // (C, A)
    int *tile_sum;        // (num_tiles(A))
    long long R, L, C, A;
    int dtype;            // WURM_LINEUP_*
};

__device__ __forceinline__ long long entry(const args &g, long long r)
{
    switch (g.dtype) {
    case 0: return ((const long long *)g.lineup)[r];
    case 1: return ((const int *)g.lineup)[r];
    case 2: return ((const short *)g.lineup)[r];
    case 3: return ((const signed char *)g.lineup)[r];
    default: return ((const unsigned char *)g.lineup)[r];
    }
}

// the sum of v over the workgroup's 256 threads, in every thread (all of them call it)
__device__ __forceinline__ int block_sum(int v, int *buf)
{
    const int s = wave_sum_i32(v);
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = s;
    __syncthreads();
    const int total = buf[0] + buf[1] + buf[2] + buf[3];
    __syncthreads();
    return total;
}

// Global memory written by some lanes of a wave and then read, or added to, by OTHER lanes of the same wave.  By the
// language's rules the lanes are threads of their own, so the hand-off is spelled out as wave_lds_sync (wurm_device.hpp)
// spells it for LDS: a release fence, a barrier of the wave, an acquire fence — here at a scope that makes the compiler
// wait for the stores to be acknowledged (s_waitcnt vmcnt(0)) instead of relying on one wave's accesses staying in order.
// wave_global_sync: later plain loads, served by the CU's own L1 (workgroup scope).  wave_global_sync_atomics: later
// atomic adds, which are served by the L2 (agent scope).
__device__ __forceinline__ void wave_global_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void wave_global_sync_atomics()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

} // namespace plan

__global__ __launch_bounds__(plan::THREADS) void league_plan_count_kernel(plan::args g)
{
    using namespace plan;
    const long long c = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (c >= g.C) return;
    int *row = g.table + c * g.A;
    for (long long a = lane; a < g.A; a += 64) row[a] = 0;
    wave_global_sync_atomics(); // every lane's zeroes are in place before any lane's add arrives
    const long long end = min((c + 1) * g.L, g.R);
    for (long long r = c * g.L + lane; r < end; r += 64) {
        const long long v = entry(g, r);
        if (v >= 0 && v < g.A) atomicAdd(row + v, 1);
    }
}

__global__ __launch_bounds__(plan::THREADS) void league_plan_chunks_kernel(plan::args g)
{
    using namespace plan;
    __shared__ int buf[WAVES];
    const long long a = (long long)blockIdx.x * TILE + threadIdx.x;
    int run = 0;
    if (a < g.A) {
        for (long long c = 0; c < g.C; ++c) {
            int *p = g.table + c * g.A + a;
            const int n = *p;
            *p = run;
            run += n;
        }
        g.offsets[a + 1] = run;
    }
    const int total = block_sum(run, buf);
    if (threadIdx.x == 0) g.tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(plan::THREADS) void league_plan_offsets_kernel(plan::args g)
{
    using namespace plan;
    __shared__ int buf[WAVES];
    __shared__ int wave_total[WAVES];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int part = 0;
    for (long long t = tid; t < (long long)blockIdx.x; t += THREADS) part += g.tile_sum[t];
    const int base = block_sum(part, buf); // rows of the policies in front of this tile
    const long long a = (long long)blockIdx.x * TILE + tid;
    const int n = a < g.A ? (int)g.offsets[a + 1] : 0;
    int incl = n; // inclusive scan over the wave, then the waves in order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int front = base;
    for (int w = 0; w < wave; ++w) front += wave_total[w];
    if (a < g.A) g.offsets[a + 1] = (long long)front + incl;
    if (a == 0) g.offsets[0] = 0;
    if (a == g.A - 1) *g.dropped = (int)(g.R - ((long long)front + incl));
}

__global__ __launch_bounds__(plan::THREADS) void league_plan_place_kernel(plan::args g)
{
    using namespace plan;
    const long long c = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (c >= g.C) return;
    int *row = g.table + c * g.A;
    const long long listed = g.offsets[g.A];
    const long long end = min((c + 1) * g.L, g.R);
    for (long long r0 = c * g.L; r0 < end; r0 += 64) { // (r0 wave-uniform: every lane makes every step)
        const long long r = r0 + lane;
        const bool have = r < end;
        const long long v = have ? entry(g, r) : -1;
        const bool in = v >= 0 && v < g.A;
        const int before = in ? row[v] : 0; // rows of this policy in the chunk's earlier steps (and earlier chunks' none:
        const long long first = in ? g.offsets[v] : 0; // those are in the scan of launch 2)
        long long pos = -1;
        u64 todo = ballot(in);
        while (todo) {
            const int leader = first_bit(todo);
            const long long lv = lane_value64(v, leader);
            const bool mine = in && v == lv;
            const u64 same = ballot(mine);
            if (mine) pos = first + before + rank_below(same);
            if (lane == leader) row[v] = before + popc64(same);
            todo &= ~same;
        }
        if (pos >= 0 && pos < g.R) g.order[pos] = (int)r;
        if (have && r >= listed) g.order[r] = -1;
        wave_global_sync(); // the counts the leaders moved on are in place before the next step's lanes read them
    }
}

} // namespace wurm
