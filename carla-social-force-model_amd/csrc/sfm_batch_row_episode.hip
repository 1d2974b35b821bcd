// sfm_batch_row_episode.hip -- many agents per scene for gfx950 (MI355X): episode ends per ROW (sfm_batch_end_row_step) and respawns
// of single rows from the snapshot (sfm_batch_respawn_rows_device); the records and the rules are specified in include/sfm_hip.h.
//
// Decentralised multi-agent training makes several or all pedestrians of a scene agents, each with its own goal, collision test and
// time limit; an agent that arrives or collides is put back alone while the scene goes on.  sfm_batch_row_episode_kernel is
// sfm_batch_episode_kernel's question asked for every agent row of a scene at once, sfm_batch_row_respawn_kernel the restart (and,
// with restart noise set, its placement rounds) for chosen rows instead of chosen scenes.
//
// sfm_batch_row_episode_kernel (workgroup b, 4 waves, 10 KiB of LDS):
//   1. the scene's agent rows are a list built by sfm_batch_set_row_episodes (settings, not state); a scene without agents returns
//      after reading its count;
//   2. the scene's {x, y} are staged in LDS once, (+inf, +inf) for a row that is not live: d2 to it is +inf and never the minimum;
//   3. a split L, a power of two 1 .. 64 chosen from the scene's agent count (the largest with agents * L <= BLOCK), is uniform over
//      the workgroup: L lanes of one wave share an agent, BLOCK / L agents are served per pass.  Each lane walks the rows j = sub,
//      sub + L, .. (four LDS reads in flight), then its share of the scene's vehicle points and of its border and static points,
//      which come through LDS tiles of BLOCK points as in the restart noise; the L lanes reduce their three minima with __shfl_xor;
//   4. lane 0 of each group takes the decisions and writes its agent's record, mask byte and two state words.
// With one agent per scene L = 64 and a wave strides over the rows; with every row an agent L = 1 .. 4 and a lane owns an agent.
// Determinism: no atomics, and only minima are taken.  A minimum of floats without NaNs does not depend on the order it is taken
// in (the live test keeps NaN rows out, ring points are finite or +inf, fminf drops a NaN operand), so every split gives the same
// bits, and a scene's records are bitwise the same alone or anywhere in any batch.
// Barriers: the agent count, the pass count, L and the tile counts are uniform over the workgroup; every wave reaches every barrier.
//
// sfm_batch_row_respawn_kernel (workgroup b, 4 waves): counts the scene's chosen rows in registers, agrees on "none" through one LDS
// flag per wave behind a barrier and leaves -- such a scene is not written at all.  Without restart noise the chosen rows' entries of
// the per-row arrays are copied from the snapshot by their own lanes.  With it the placement rounds of sfm_batch_reset.hip run for
// the chosen rows: the device functions below are copies of reset_near / reset_points / reset_row / reset_scene with the row classes,
// the random words and the results of a respawn (merging the two files is left to a later change: the restart noise kernel keeps
// its code, registers and LDS as they are).
#include "sfm_device.h"
#include "sfm_interaction.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

struct RowEpisodeShared {
    float2 pos[BATCH_MAX_N];                                           // the scene's rows; (+inf, +inf): not live
    float2 tile[BLOCK];                                                // geometry points of the current tile
};

// This lane's share (q = sub, sub + L, ..) of the minimum of dist2 over all points of scene b's polylines of one kind -- one
// contiguous run of pts -- through LDS tiles.  Every wave reaches both barriers of every tile (the bounds are uniform).
__device__ __forceinline__ float row_episode_points(const BatchGeo& g, int b, RowEpisodeShared& sh, float x, float y, int sub, int L, float m) {
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
    if (k1 <= k0) return m;                                            // uniform: the scene has no polyline of the kind (g.off may be null)
    const int p1 = g.off[k1];
#pragma unroll 1
    for (int p0 = g.off[k0]; p0 < p1; p0 += BLOCK) {                   // uniform
        const int cnt = min(BLOCK, p1 - p0);
        __syncthreads();                                               // the tile before has been read
        if ((int)threadIdx.x < cnt) sh.tile[threadIdx.x] = g.pts[p0 + (int)threadIdx.x];
        __syncthreads();
        int q = sub;
#pragma unroll 1
        for (; q + 3 * L < cnt; q += 4 * L) {
            const float2 c0 = sh.tile[q], c1 = sh.tile[q + L], c2 = sh.tile[q + 2 * L], c3 = sh.tile[q + 3 * L];
            m = fminf(fminf(fminf(m, dist2(x, y, c0.x, c0.y)), dist2(x, y, c1.x, c1.y)),
                      fminf(dist2(x, y, c2.x, c2.y), dist2(x, y, c3.x, c3.y)));
        }
#pragma unroll 1
        for (; q < cnt; q += L) {
            const float2 c = sh.tile[q];
            m = fminf(m, dist2(x, y, c.x, c.y));
        }
    }
    return m;
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_row_episode_kernel(const RowEpisodeArgs a) {
    __shared__ RowEpisodeShared sh;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int a0 = a.agent_off[b], na = a.agent_off[b + 1] - a0;
    if (na <= 0) return;                                               // uniform: the scene has no agent
    const float inf = __builtin_inff();
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 1 <= n <= BATCH_MAX_N (an agent is a row)
    for (int j = tid; j < n; j += BLOCK) {
        const float4 p = a.pk[s0 + j];
        sh.pos[j] = row_live(p.x, p.y) ? make_float2(p.x, p.y) : make_float2(inf, inf);
    }
    int L = 1;                                                         // uniform: the largest power of two <= 64 with na * L <= BLOCK
    while (L < WAVE && na * (L * 2) <= BLOCK) L *= 2;
    const int G = BLOCK / L;                                           // agents per pass
    const int grp = tid / L, sub = tid & (L - 1);
    const BatchEpisodeScene es = a.set[b];
    __syncthreads();                                                   // the rows are in LDS
#pragma unroll 1
    for (int q0 = 0; q0 < na; q0 += G) {                               // uniform
        const int q = q0 + grp;
        const bool mine = q < na;
        const int i = mine ? a.agent_rows[a0 + q] : 0;                 // 0 .. n - 1 (built on the host)
        const float4 s = a.pk[s0 + i];
        const float x = s.x, y = s.y;
        const bool live = row_live(x, y);
        float mp = inf, mv = inf, mw = inf;
        if (mine && live) {                                            // (no barrier inside)
            int j = sub;
#pragma unroll 1
            for (; j + 3 * L < n; j += 4 * L) {
                const float2 c0 = sh.pos[j], c1 = sh.pos[j + L], c2 = sh.pos[j + 2 * L], c3 = sh.pos[j + 3 * L];
                const float dx0 = c0.x - x, dy0 = c0.y - y, dx1 = c1.x - x, dy1 = c1.y - y;
                const float dx2 = c2.x - x, dy2 = c2.y - y, dx3 = c3.x - x, dy3 = c3.y - y;
                const float d0 = fmaf(dx0, dx0, dy0 * dy0), d1 = fmaf(dx1, dx1, dy1 * dy1);
                const float d2 = fmaf(dx2, dx2, dy2 * dy2), d3 = fmaf(dx3, dx3, dy3 * dy3);
                mp = j != i ? fminf(mp, d0) : mp;
                mp = j + L != i ? fminf(mp, d1) : mp;
                mp = j + 2 * L != i ? fminf(mp, d2) : mp;
                mp = j + 3 * L != i ? fminf(mp, d3) : mp;
            }
#pragma unroll 1
            for (; j < n; j += L) {
                const float2 c = sh.pos[j];
                const float dx = c.x - x, dy = c.y - y;
                mp = j != i ? fminf(mp, fmaf(dx, dx, dy * dy)) : mp;
            }
        }
        // (a lane without a live agent walks the tiles with its row's or row 0's position and drops the result: the barriers stay uniform)
        mv = row_episode_points(a.geo[2], b, sh, x, y, sub, L, mv);
        mw = row_episode_points(a.geo[0], b, sh, x, y, sub, L, mw);
        mw = row_episode_points(a.geo[1], b, sh, x, y, sub, L, mw);
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            if (m < L) {                                               // uniform: the group's lanes are neighbours inside one wave
                mp = fminf(mp, __shfl_xor(mp, m)); mv = fminf(mv, __shfl_xor(mv, m)); mw = fminf(mw, __shfl_xor(mw, m));
            }
        }
        if (!mine || sub != 0) continue;                               // (the loop's barriers are inside row_episode_points: bounds uniform)
        const size_t r = (size_t)(s0 + i);
        const int age = a.row_age[r] + 1;
        float goal_d2 = inf, prev = inf;
        int reason = 16;
        if (live) {
            const float4 o = a.own[r];
            const float gx = o.x - x, gy = o.y - y;                    // the goal entry as observe forms it
            goal_d2 = fmaf(gx, gx, gy * gy);
            const float stored = a.row_prev_goal_d2[r];
            prev = stored != stored ? goal_d2 : stored;                // NaN: the first live evaluation since the respawn
            a.row_prev_goal_d2[r] = goal_d2;
            reason = (goal_d2 < es.goal_r2 ? 1 : 0) | (mp < es.ped_r2 ? 4 : 0) | (mv < es.veh_r2 ? 8 : 0);
        } else {
            mp = inf; mv = inf; mw = inf;
        }
        if (es.max_steps > 0 && age >= es.max_steps) reason |= 2;
        const bool done = reason != 0;
        float4* out = reinterpret_cast<float4*>(a.record + r * 8);
        out[0] = make_float4(done ? 1.0f : 0.0f, (float)reason, (float)age, goal_d2);
        out[1] = make_float4(prev, mp, mv, mw);
        a.row_done[r] = done ? 1 : 0;
        a.row_age[r] = age;
    }
}

// The row episodes of the chosen scenes start over: launched behind sfm_batch_restart_kernel with the same choice of scenes (list /
// mask as in BatchRestart); other scenes are not touched.
__global__ __launch_bounds__(BLOCK) void sfm_batch_row_restart_kernel(const int* list, const uint8_t* mask, const int* scene_off, int* row_age,
                                                                      float* row_prev_goal_d2) {
    const int b = list ? list[blockIdx.x] : (int)blockIdx.x;
    if (mask && mask[b] == 0) return;                                  // uniform: the scene is not chosen
    const int s1 = scene_off[b + 1];
    for (int i = scene_off[b] + (int)threadIdx.x; i < s1; i += BLOCK) {
        row_age[i] = 0;
        row_prev_goal_d2[i] = __builtin_nanf("");
    }
}

// ---- respawns ---------------------------------------------------------------------------------------------------------------------

constexpr int RESPAWN_PASSES = BATCH_MAX_N / BLOCK;                    // rows a lane owns at most
constexpr uint8_t RROW_OUT = 0, RROW_FIXED = 1, RROW_OPEN = 2, RROW_PLACED = 3;   // bit 0: a blocker

struct RespawnShared {
    float2 cand[BATCH_MAX_N];                                          // where row j counts this round (as ResetShared::cand)
    float2 tile[BLOCK];
    uint8_t st[BATCH_MAX_N];                                           // RROW_* (4-byte aligned: read four rows at a time)
    int any_open[WAVES_PER_BLOCK];
    int count[WAVES_PER_BLOCK];
};

// The random word of a respawn: reset_word's formula under another constant, with e the ROW's respawn counter -- so the words never
// coincide with a scene restart's and never repeat.
constexpr uint32_t RESPAWN_SALT = 0x2545F491u;
__device__ __forceinline__ uint32_t respawn_word(uint32_t seed, uint32_t i, uint32_t e, uint32_t t, uint32_t c) {
    return mix32(seed ^ mix32(mix32(RESPAWN_SALT ^ (8u * i + c)) + 0x9E3779B9u * (32u * e + t)));
}

// One chosen row's entries of the per-row arrays of BatchRestart back from the snapshot; its row episode starts over.
__device__ __forceinline__ void respawn_copy(const RowRespawnArgs& a, int r) {
    a.pk[r] = a.s_pk[r];
    if (a.zv) a.zv[r] = a.s_zv[r];                                     // (uniform conditions: the batch has the array or not)
    a.own[r] = a.s_own[r];
    a.draws[r] = a.s_draws[r];
    if (a.mode) { a.mode[r] = a.s_mode[r]; a.target[r] = a.s_target[r]; a.cursor[r] = a.s_cursor[r]; }
    if (a.row_age) { a.row_age[r] = 0; a.row_prev_goal_d2[r] = __builtin_nanf(""); }
}

template <int PASSES>
__device__ __forceinline__ uint32_t respawn_near(const float (&px)[PASSES], const float (&py)[PASSES], float2 p, float gap2, uint32_t counts) {
    uint32_t hit = 0;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        const float dx = p.x - px[s], dy = p.y - py[s];
        hit |= (fmaf(dx, dx, dy * dy) < gap2 ? 1u : 0u) << s;
    }
    return hit & counts;
}

template <int PASSES>
__device__ __forceinline__ uint32_t respawn_points(const BatchGeo& g, int b, RespawnShared& sh, const float (&px)[PASSES],
                                                   const float (&py)[PASSES], bool walk, float gap2) {
    uint32_t rej = 0;
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
    if (k1 <= k0) return rej;                                          // uniform
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
            rej |= respawn_near<PASSES>(px, py, c0, gap2, ~0u) | respawn_near<PASSES>(px, py, c1, gap2, ~0u) |
                   respawn_near<PASSES>(px, py, c2, gap2, ~0u) | respawn_near<PASSES>(px, py, c3, gap2, ~0u);
        }
#pragma unroll 1
        for (; q < cnt; ++q) rej |= respawn_near<PASSES>(px, py, sh.tile[q], gap2, ~0u);
    }
    return rej;
}

// Row j against the lane's proposals: a blocker counts for every row, an open row's proposal for the rows of higher index.
template <int PASSES>
__device__ __forceinline__ uint32_t respawn_row(const float (&px)[PASSES], const float (&py)[PASSES], float2 c, uint32_t st, int j, int tid,
                                                float gap2) {
    uint32_t counts = 0;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) counts |= ((st & 1u) | ((uint32_t)(j - (s * BLOCK + tid)) >> 31)) << s;   // (integer: j < i is the sign bit)
    return respawn_near<PASSES>(px, py, c, gap2, counts);
}

// The noisy respawn of scene b's chosen rows (at least one), for a scene of up to PASSES * BLOCK rows.
template <int PASSES>
__device__ __forceinline__ void respawn_scene(const RowRespawnArgs& a, RespawnShared& sh, int b, int s0, int n) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const uint32_t seed = a.seed[b];
    const float2 gap2 = a.gap2[b];
    // 1. copies and classes: a chosen row from the snapshot; every other live row a blocker where it stands now
    float sx[PASSES], sy[PASSES], px[PASSES], py[PASSES], hx[PASSES], hy[PASSES];   // snapshot position, proposal, box
    uint32_t er[PASSES];                                               // the row's respawn counter before this respawn
    uint32_t chosen = 0, open = 0, placed = 0;                         // bit s: this lane's row of pass s
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        sx[s] = 0.f; sy[s] = 0.f; px[s] = 0.f; py[s] = 0.f; hx[s] = 0.f; hy[s] = 0.f; er[s] = 0u;
        const int i = s * BLOCK + tid;
        if (i < n) {
            const int r = s0 + i;
            const bool ch = a.mask[r] != 0;
            const float4 q = ch ? a.s_pk[r] : a.pk[r];
            const bool live = row_live(q.x, q.y);
            uint8_t st = live ? RROW_FIXED : RROW_OUT;
            if (ch) {
                respawn_copy(a, r);
                const float2 hb = a.pos_box[r];
                er[s] = a.row_resets[r];
                a.row_resets[r] = er[s] + 1u;
                sx[s] = q.x; sy[s] = q.y; hx[s] = hb.x; hy[s] = hb.y;
                chosen |= 1u << s;
                if (live && !(hb.x == 0.0f && hb.y == 0.0f)) { st = RROW_OPEN; open |= 1u << s; }
            }
            sh.cand[i] = live ? make_float2(q.x, q.y) : make_float2(__builtin_inff(), __builtin_inff());   // (+inf: d2 = +inf, never < gap2)
            sh.st[i] = st;
        }
    }
    // The first round's proposals overwrite cand[i] of open rows only, each by its own lane: no barrier is needed in between.

    // 2. placement rounds
#pragma unroll 1
    for (int t = 0; t < a.tries; ++t) {                                // uniform
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const int i = s * BLOCK + tid;
            if (open & (1u << s)) {
                px[s] = sx[s] + reset_offset(respawn_word(seed, (uint32_t)i, er[s], (uint32_t)t, 0u), hx[s]);
                py[s] = sy[s] + reset_offset(respawn_word(seed, (uint32_t)i, er[s], (uint32_t)t, 1u), hy[s]);
                sh.cand[i] = make_float2(px[s], py[s]);
            }
        }
        __syncthreads();                                               // all proposals of the round are in LDS
        uint32_t rej = 0;
        if (gap2.x > 0.0f && open) {                                   // (a gap of 0 never rejects; no barrier inside)
            int j = 0;
#pragma unroll 1
            for (; j + 4 <= n; j += 4) {                               // uniform: the LDS reads are broadcasts, all in flight together
                const uint32_t s4 = *reinterpret_cast<const uint32_t*>(&sh.st[j]);
                const float2 c0 = sh.cand[j], c1 = sh.cand[j + 1], c2 = sh.cand[j + 2], c3 = sh.cand[j + 3];
                rej |= respawn_row<PASSES>(px, py, c0, s4, j, tid, gap2.x) | respawn_row<PASSES>(px, py, c1, s4 >> 8, j + 1, tid, gap2.x) |
                       respawn_row<PASSES>(px, py, c2, s4 >> 16, j + 2, tid, gap2.x) | respawn_row<PASSES>(px, py, c3, s4 >> 24, j + 3, tid, gap2.x);
            }
#pragma unroll 1
            for (; j < n; ++j) rej |= respawn_row<PASSES>(px, py, sh.cand[j], sh.st[j], j, tid, gap2.x);
        }
        if (gap2.y > 0.0f) {                                           // uniform
            rej |= respawn_points<PASSES>(a.v.geo[0], b, sh, px, py, open != 0, gap2.y);
            rej |= respawn_points<PASSES>(a.v.geo[1], b, sh, px, py, open != 0, gap2.y);
            rej |= respawn_points<PASSES>(a.v.geo[2], b, sh, px, py, open != 0, gap2.y);
        }
        __syncthreads();                                               // everyone has read this round's cand and st
#pragma unroll
        for (int s = 0; s < PASSES; ++s)
            if ((open & ~rej) & (1u << s)) sh.st[s * BLOCK + tid] = RROW_PLACED;    // (cand[i] already holds the accepted proposal)
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

    // 3. the results, from the lane's own registers: positions of the placed rows, goals of the chosen live rows, the counter
    int cnt = __popc(open);                                            // rows no try could place: they stay at the snapshot position
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) sh.count[wave] = cnt;
#pragma unroll
    for (int s = 0; s < PASSES; ++s) {
        const int i = s * BLOCK + tid;
        if (i >= n || !(chosen & (1u << s))) continue;
        if (placed & (1u << s)) *reinterpret_cast<float2*>(a.pk + s0 + i) = make_float2(px[s], py[s]);   // (behind this lane's own copy)
        if (a.goal_box && row_live(sx[s], sy[s])) {
            float2* w = reinterpret_cast<float2*>(a.own + s0 + i);
            const float2 g = a.goal_box[s0 + i];
            const float4 o = a.s_own[s0 + i];
            *w = make_float2(o.x + reset_offset(respawn_word(seed, (uint32_t)i, er[s], 0u, 2u), g.x),
                             o.y + reset_offset(respawn_word(seed, (uint32_t)i, er[s], 0u, 3u), g.y));
        }
    }
    __syncthreads();
    if (tid == 0) {
        int f = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) f += sh.count[w];
        a.fallbacks[b] = (uint32_t)f;
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_row_respawn_kernel(const RowRespawnArgs a) {
    __shared__ RespawnShared sh;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const int s0 = a.v.scene_off[b], n = a.v.scene_off[b + 1] - s0;    // 0 <= n <= BATCH_MAX_N (checked on the host)
    int c = 0;                                                         // this lane's chosen rows
    for (int i = tid; i < n; i += BLOCK) c += a.mask[s0 + i] != 0 ? 1 : 0;
    const int mine = __any(c != 0) ? 1 : 0;
    if (lane == 0) sh.any_open[wave] = mine;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) any |= sh.any_open[w];
    if (!any) return;                                                  // uniform: no row of the scene is chosen, nothing is written
    if (!a.seed) {                                                     // uniform: no restart noise, plain copies
        for (int i = tid; i < n; i += BLOCK)
            if (a.mask[s0 + i] != 0) respawn_copy(a, s0 + i);
        return;
    }
    __syncthreads();                                                   // any_open has been read: the rounds write it again
    if (n <= BLOCK) respawn_scene<1>(a, sh, b, s0, n);                 // uniform
    else if (n <= 2 * BLOCK) respawn_scene<2>(a, sh, b, s0, n);
    else respawn_scene<RESPAWN_PASSES>(a, sh, b, s0, n);
}

hipError_t launch_batch_row_episode(const RowEpisodeArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_row_episode_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_row_restart(const int* list, const uint8_t* mask, const int* scene_off, int* row_age, float* row_prev_goal_d2,
                                    int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_row_restart_kernel, dim3(scenes), dim3(BLOCK), 0, st, list, mask, scene_off, row_age, row_prev_goal_d2);
    return hipGetLastError();
}

hipError_t launch_batch_row_respawn(const RowRespawnArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_row_respawn_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
