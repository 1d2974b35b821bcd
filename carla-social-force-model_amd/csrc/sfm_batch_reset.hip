// sfm_batch_reset.hip -- restart noise of batched scenes for gfx950 (MI355X): ONE launch behind sfm_batch_restart_kernel, for the
// scenes that kernel has just put back to the snapshot (sfm_batch_set_restart_noise; the rule is specified in include/sfm_hip.h).
//
// What a crowd-navigation environment does on reset: starts drawn from a box around each row's snapshot position and re-drawn until
// nobody is nearer than min_gap to anybody or nearer than point_gap to a point of the scene's geometry, goals drawn from a box around
// the snapshot goal, scripted traffic arriving up to `delay` ticks later.  Every draw is a counter-based word (reset_word,
// sfm_device.h) of the scene's seed, the row's index inside the scene, the scene's restart counter e, the try and the component, so a
// restart is reproducible and a scene's result depends on its own seed, its own rows and e only.
//
// Shape (workgroup b, 4 waves; the same list / mask head as the restart kernel -- a scene that is not chosen leaves at once):
//   0. traffic timing, a wave per vehicle: a tracked vehicle with a delay gets its first tick moved and is placed again by
//      track_vehicle, the one definition sfm_batch_place_tracks_kernel and the tick use;
//   1. a lane owns row tid of each pass of BLOCK rows (1, 2 or 4 passes: a template argument chosen by the scene's size) and keeps
//      that row's snapshot position, proposal and box in registers; LDS holds one position per row, cand[j] -- where row j counts in
//      the current round: a blocker's place, an open row's proposal, +inf for a row that is not live -- and a state byte;
//   2. per try: every open row writes its proposal to LDS (all passes: every proposal of the round is there before anyone is
//      judged); barrier (in round 0 it also orders step 0's ring stores in front of the reads of them); each lane walks all j for
//      its rows -- a blocker counts for everyone, an open row's proposal for the rows j < i; broadcast LDS reads, four in flight --
//      and, while point_gap > 0, the scene's border, static and vehicle points, staged cooperatively in LDS tiles of BLOCK points by
//      per-lane (vector) loads and read as broadcasts; barrier; the accepted rows commit (their state byte: cand already holds the proposal); the round ends with a
//      workgroup-wide "is anyone still open" through LDS, whose barrier is also the one in front of the next round's proposals;
//   3. each lane stores x, y of its placed rows and the goals of its live rows; thread 0 the two counters.
// Barriers: tries, the pass count, the tile counts and the early exit are uniform over the workgroup, so every wave reaches every
// barrier.  A row is rejected against the proposals of ALL open rows of lower index, accepted or not: that is conservative, and
// it makes the outcome a function of the proposals alone, whatever order lanes, waves and passes run in.
// No atomics; plain vector loads and stores; 11 KiB of LDS; no register array is indexed at run time, so nothing goes to scratch.
#include "sfm_device.h"
#include "sfm_interaction.h"

#pragma clang fp contract(off)     // every operation of the rule is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int RESET_PASSES = BATCH_MAX_N / BLOCK;                      // rows a lane owns at most
constexpr uint8_t ROW_OUT = 0, ROW_FIXED = 1, ROW_OPEN = 2, ROW_PLACED = 3;   // bit 0: a blocker

struct ResetShared {
    float2 cand[BATCH_MAX_N];                                          // where row j counts this round: a blocker's position, an open
                                                                       // row's proposal, (+inf, +inf) for a row that is not live
    float2 tile[BLOCK];                                                // geometry points of the current tile
    uint8_t st[BATCH_MAX_N];                                           // ROW_* (4-byte aligned: read four rows at a time)
    int any_open[WAVES_PER_BLOCK];
    int count[WAVES_PER_BLOCK];
};

// Bit s: the lane's proposal of pass s is nearer than gap2 to the point p (`counts`: bit s set where p counts for that row at all).
template <int PASSES>
__device__ __forceinline__ uint32_t reset_near(const float (&px)[PASSES], const float (&py)[PASSES], float2 p, float gap2, uint32_t counts) {
    uint32_t hit = 0;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        const float dx = p.x - px[s], dy = p.y - py[s];
        hit |= (fmaf(dx, dx, dy * dy) < gap2 ? 1u : 0u) << s;
    }
    return hit & counts;
}

// Bit s of the result: the lane's proposal of pass s is nearer than gap2 to a point of scene b's polylines of one kind -- one
// contiguous run of pts, as in sfm_batch_episode.hip.  The points come through LDS by per-lane loads: the vehicle rings may have been
// written by this workgroup in step 0, and only vector loads are coherent with those stores.  Every wave reaches both barriers of
// every tile (the bounds are uniform).  Four LDS reads are in flight before the first is used: a small scene keeps one wave busy,
// and nothing else hides the latency.
template <int PASSES>
__device__ __forceinline__ uint32_t reset_points(const BatchGeo& g, int b, ResetShared& sh, const float (&px)[PASSES],
                                                 const float (&py)[PASSES], bool walk, float gap2) {
    uint32_t rej = 0;
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
    if (k1 <= k0) return rej;                                          // uniform: the scene has no polyline of the kind (g.off may be null)
    const int p1 = g.off[k1];
#pragma unroll 1
    for (int p0 = g.off[k0]; p0 < p1; p0 += BLOCK) {                   // uniform
        const int cnt = min(BLOCK, p1 - p0);
        __syncthreads();                                               // the tile before has been read
        if ((int)threadIdx.x < cnt) sh.tile[threadIdx.x] = g.pts[p0 + (int)threadIdx.x];
        __syncthreads();
        if (!walk) continue;                                           // (no barrier below)
        int q = 0;
#pragma unroll 1
        for (; q + 4 <= cnt; q += 4) {                                 // uniform: the LDS reads are broadcasts
            const float2 c0 = sh.tile[q], c1 = sh.tile[q + 1], c2 = sh.tile[q + 2], c3 = sh.tile[q + 3];
            rej |= reset_near<PASSES>(px, py, c0, gap2, ~0u) | reset_near<PASSES>(px, py, c1, gap2, ~0u) |
                   reset_near<PASSES>(px, py, c2, gap2, ~0u) | reset_near<PASSES>(px, py, c3, gap2, ~0u);
        }
#pragma unroll 1
        for (; q < cnt; ++q) rej |= reset_near<PASSES>(px, py, sh.tile[q], gap2, ~0u);
    }
    return rej;
}

// Row j against the lane's proposals: a blocker counts for every row, an open row's proposal for the rows of higher index.
template <int PASSES>
__device__ __forceinline__ uint32_t reset_row(const float (&px)[PASSES], const float (&py)[PASSES], float2 c, uint32_t st, int j, int tid,
                                              float gap2) {
    uint32_t counts = 0;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) counts |= ((st & 1u) | ((uint32_t)(j - (s * BLOCK + tid)) >> 31)) << s;   // (integer: j < i is the sign bit)
    return reset_near<PASSES>(px, py, c, gap2, counts);
}

// Steps 1 to 3 for a scene of up to PASSES * BLOCK rows: the pass count is a template argument (1, 2 or 4, chosen uniformly by the
// kernel) so that a lane of a small scene -- 64 rows in an RL batch -- does not walk everybody for rows it does not have.
template <int PASSES>
__device__ __forceinline__ void reset_scene(const RestartNoiseArgs& a, ResetShared& sh, int b, int s0, int n, uint32_t seed, uint32_t e,
                                            float2 gap2) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    // 1. classes, from the restored state
    float sx[PASSES], sy[PASSES], px[PASSES], py[PASSES], hx[PASSES], hy[PASSES];   // snapshot position, proposal, box
    uint32_t open = 0;                                                 // bit s: this lane's row of pass s is movable and not yet placed
    uint32_t placed = 0;                                               // bit s: ... has been placed, at (px, py)
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        sx[s] = 0.f; sy[s] = 0.f; px[s] = 0.f; py[s] = 0.f; hx[s] = 0.f; hy[s] = 0.f;
        const int i = s * BLOCK + tid;
        if (i < n) {
            const float4 q = a.pk[s0 + i];
            const float2 hb = a.pos_box[s0 + i];
            sx[s] = q.x; sy[s] = q.y; hx[s] = hb.x; hy[s] = hb.y;
            const bool live = row_live(q.x, q.y);
            const uint8_t st = !live ? ROW_OUT : (hb.x == 0.0f && hb.y == 0.0f) ? ROW_FIXED : ROW_OPEN;
            sh.cand[i] = live ? make_float2(q.x, q.y) : make_float2(__builtin_inff(), __builtin_inff());   // (+inf: d2 = +inf, never < gap2)
            sh.st[i] = st;
            if (st == ROW_OPEN) open |= 1u << s;
        }
    }
    // The ring stores of step 0 are read back below by other waves of this workgroup.  __syncthreads() is a workgroup-scope release
    // and acquire around the barrier: the stores have left the wave (vmcnt 0) before it, and a workgroup's waves share one CU and
    // its vector L1, which is write-through -- so the per-lane loads of reset_points see them.  (Scalar loads would not: hence LDS tiles.)
    // The first round's proposals overwrite cand[i] of open rows only, each by its own lane: no barrier is needed in between.

    // 2. placement rounds
#pragma unroll 1
    for (int t = 0; t < a.tries; ++t) {                                // uniform
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const int i = s * BLOCK + tid;
            if (open & (1u << s)) {
                px[s] = sx[s] + reset_offset(reset_word(seed, (uint32_t)i, e, (uint32_t)t, 0u), hx[s]);
                py[s] = sy[s] + reset_offset(reset_word(seed, (uint32_t)i, e, (uint32_t)t, 1u), hy[s]);
                sh.cand[i] = make_float2(px[s], py[s]);
            }
        }
        __syncthreads();                                               // all proposals of the round are in LDS (and, in round 0, step 0's rings in memory)
        uint32_t rej = 0;
        if (gap2.x > 0.0f && open) {                                   // (a gap of 0 never rejects; no barrier inside)
            int j = 0;
#pragma unroll 1
            for (; j + 4 <= n; j += 4) {                               // uniform: the LDS reads are broadcasts, all in flight together
                const uint32_t s4 = *reinterpret_cast<const uint32_t*>(&sh.st[j]);
                const float2 c0 = sh.cand[j], c1 = sh.cand[j + 1], c2 = sh.cand[j + 2], c3 = sh.cand[j + 3];
                rej |= reset_row<PASSES>(px, py, c0, s4, j, tid, gap2.x) | reset_row<PASSES>(px, py, c1, s4 >> 8, j + 1, tid, gap2.x) |
                       reset_row<PASSES>(px, py, c2, s4 >> 16, j + 2, tid, gap2.x) | reset_row<PASSES>(px, py, c3, s4 >> 24, j + 3, tid, gap2.x);
            }
#pragma unroll 1
            for (; j < n; ++j) rej |= reset_row<PASSES>(px, py, sh.cand[j], sh.st[j], j, tid, gap2.x);
        }
        if (gap2.y > 0.0f) {                                           // uniform
            rej |= reset_points<PASSES>(a.v.geo[0], b, sh, px, py, open != 0, gap2.y);
            rej |= reset_points<PASSES>(a.v.geo[1], b, sh, px, py, open != 0, gap2.y);
            rej |= reset_points<PASSES>(a.v.geo[2], b, sh, px, py, open != 0, gap2.y);
        }
        __syncthreads();                                               // everyone has read this round's cand and st
#pragma unroll
        for (int s = 0; s < PASSES; ++s)
            if ((open & ~rej) & (1u << s)) sh.st[s * BLOCK + tid] = ROW_PLACED;     // (cand[i] already holds the accepted proposal)
        placed |= open & ~rej;
        open &= rej;
        const int mine = __any(open != 0) ? 1 : 0;
        if (lane == 0) sh.any_open[wave] = mine;
        __syncthreads();                                               // the commits; and the flags (rewritten only behind the next round's first barrier)
        int left = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) left |= sh.any_open[w];
        if (!left) break;                                              // uniform: decided on LDS values every wave reads alike
    }

    // 3. the results, from the lane's own registers: positions of the placed rows, goals of the live rows, the counters
    int cnt = __popc(open);                                            // rows no try could place: they stay at the snapshot position
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) sh.count[wave] = cnt;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        const int i = s * BLOCK + tid;
        if (i >= n) continue;
        if (placed & (1u << s)) *reinterpret_cast<float2*>(a.pk + s0 + i) = make_float2(px[s], py[s]);
        if (a.goal_box && row_live(sx[s], sy[s])) {
            float2* w = reinterpret_cast<float2*>(a.own + s0 + i);
            const float2 g = a.goal_box[s0 + i];
            const float2 o = *w;
            *w = make_float2(o.x + reset_offset(reset_word(seed, (uint32_t)i, e, 0u, 2u), g.x),
                             o.y + reset_offset(reset_word(seed, (uint32_t)i, e, 0u, 3u), g.y));
        }
    }
    __syncthreads();
    if (tid == 0) {
        int f = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) f += sh.count[w];
        a.fallbacks[b] = (uint32_t)f;
        a.resets[b] = e + 1u;
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_restart_noise_kernel(const RestartNoiseArgs a) {
    __shared__ ResetShared sh;
    const int b = a.list ? a.list[blockIdx.x] : (int)blockIdx.x;
    if (a.mask && a.mask[b] == 0) return;                              // uniform: the scene is not chosen
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const int s0 = a.v.scene_off[b], n = a.v.scene_off[b + 1] - s0;    // 0 <= n <= BATCH_MAX_N (checked on the host)
    const uint32_t seed = a.seed[b];
    const uint32_t e = a.resets[b];                                    // read before this restart; stored back as e + 1 at the very end
    const float2 gap2 = a.gap2[b];

    // 0. traffic timing: first[k] += floor(h (D + 1) / 2^32), then the vehicle as tick trk.tick sees it.  track_vehicle reads first[k]
    // as it was (nobody has stored to it yet) under a tick counter moved back by the same amount; the new first tick is stored after it.
    if (a.delay) {                                                     // uniform
        const int k0 = a.v.geo[2].item_off[b], k1 = a.v.geo[2].item_off[b + 1];
        for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {        // wave-uniform
            const int D = a.delay[k];
            if (D <= 0 || a.trk.off[k + 1] == a.trk.off[k]) continue;
            if (a.veh_cmd) {                                           // a driven vehicle stays at its snapshot pose
                const float kind = a.veh_cmd[k].w;
                if (kind == 1.0f || kind == 2.0f) continue;
            }
            const uint32_t h = reset_word(seed, (uint32_t)(k - k0), e, 0u, 4u);
            const int add = (int)(((unsigned long long)h * (unsigned long long)((uint32_t)D + 1u)) >> 32);   // 0 .. D
            const int f0 = a.first[k];
            BatchTracks t = a.trk;
            t.tick -= (long long)add;
            track_vehicle(t, k, lane, a.v.geo[2].off, a.veh_local, a.veh_ctr, a.veh_pts);
            if (lane == 0) a.first[k] = f0 + add;                      // (fits int32: checked on the host with the largest delay)
        }
    }
    if (n <= 0) {                                                      // uniform
        if (tid == 0) { a.resets[b] = e + 1u; a.fallbacks[b] = 0u; }
        return;
    }

    if (n <= BLOCK) reset_scene<1>(a, sh, b, s0, n, seed, e, gap2);                    // uniform
    else if (n <= 2 * BLOCK) reset_scene<2>(a, sh, b, s0, n, seed, e, gap2);
    else reset_scene<RESET_PASSES>(a, sh, b, s0, n, seed, e, gap2);
}

hipError_t launch_batch_restart_noise(const RestartNoiseArgs& a, int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_restart_noise_kernel, dim3(scenes), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
