// sfm_batch_episode.hip -- episode ends of batched scenes for gfx950 (MI355X): ONE launch for the whole batch (sfm_batch_end_step,
// ABI 16; the record and its rules are specified in include/sfm_hip.h).
//
// What an RL loop asks after every step: has the scene's agent reached its goal, touched a pedestrian or a vehicle, left the scene, or
// has the episode run out of time -- and what a reward is made of: the squared distances to the goal (now and one evaluation ago), to
// the nearest live pedestrian, to the nearest vehicle ring point and to the nearest border or static-obstacle point.  Computed from the
// buffers the tick reads (state, own, the scene offsets, the three geometry CSRs), into a record [B][8] of floats, a mask done[B] of
// bytes that sfm_batch_restart_device takes as it is, and the per-scene episode state (age, prev_goal_d2).  The kernel writes
// nothing else, so a tick before or after it computes what it computed without it.
//
// Shape (workgroup b, 4 waves):
//   1. every lane reads the agent's {x, y} (one address: a broadcast) and takes the live test, uniform over the workgroup;
//   2. the 256 lanes stride over the scene's rows, then over the points of its vehicles, then of its borders and static obstacles --
//      the points of one kind of one scene are ONE contiguous range of pts, [off[item_off[b]], off[item_off[b + 1]]), so there is no
//      loop over polylines, no lane_nearest and no LDS staging: only the VALUE of each minimum is needed, and each lane keeps three
//      running minima (pedestrians, vehicles, walls);
//   3. the minima are reduced inside the wave with __shfl_xor (DPP / ds_swizzle, no LDS traffic), then across the four waves through
//      48 bytes of LDS and one barrier;
//   4. thread 0 takes the decisions and writes the record with two 16-byte stores, the mask byte and the two state words.
// A scene without an agent, or whose agent is not live, skips step 2 (uniform) and reduces three +inf.
// Determinism: no atomics.  The minimum of floats without NaNs does not depend on the order they are taken in; the live test keeps
// rows with a NaN position out, ring points are finite or +inf (an absent tracked vehicle), and fminf drops a NaN operand whichever
// side it is on.  So a scene's record is bitwise the same alone or anywhere in any batch.
#include "sfm_device.h"
#include "sfm_interaction.h"

namespace sfm {

// The live test of the agent, and of every pedestrian it could touch, is row_live (sfm_device.h), the one the observe and scan
// kernels take: a ghost parked far away fails it, and so does a NaN position.  One definition, so that no sensor
// can count a row as live that another does not.

// this lane's share of the minimum of dist2 over ALL points of ALL polylines of one kind of scene b
__device__ __forceinline__ float episode_points_min(const BatchGeo& g, int b, float x, float y, float m) {
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
    if (k1 <= k0) return m;                                            // uniform: the scene has no polyline of the kind (g.off may be null)
    const int p1 = g.off[k1];
    for (int p = g.off[k0] + (int)threadIdx.x; p < p1; p += BLOCK) {
        const float2 q = g.pts[p];
        m = fminf(m, dist2(x, y, q.x, q.y));
    }
    return m;
}

__device__ __forceinline__ float episode_wave_min(float m) {
#pragma unroll
    for (int s = WAVE / 2; s >= 1; s >>= 1) m = fminf(m, __shfl_xor(m, s));
    return m;
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_episode_kernel(const EpisodeArgs a) {
    __shared__ float red[WAVES_PER_BLOCK][3];                          // 48 bytes
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const float inf = __builtin_inff();
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;
    const BatchEpisodeScene es = a.set[b];
    const int ag = es.agent;                                           // -1 .. n - 1 (checked on the host)
    float x = 0.f, y = 0.f;
    bool live = false;
    if (ag >= 0) {                                                     // uniform
        const float4 s = a.pk[s0 + ag];
        x = s.x; y = s.y;
        live = row_live(x, y);
    }
    float mp = inf, mv = inf, mw = inf;
    if (live) {                                                        // uniform
        for (int j = tid; j < n; j += BLOCK) {
            const float4 pj = a.pk[s0 + j];
            const float dx = pj.x - x, dy = pj.y - y;
            const float d2 = fmaf(dx, dx, dy * dy);
            mp = (j != ag && row_live(pj.x, pj.y)) ? fminf(mp, d2) : mp;
        }
        mv = episode_points_min(a.geo[2], b, x, y, mv);
        mw = episode_points_min(a.geo[0], b, x, y, mw);
        mw = episode_points_min(a.geo[1], b, x, y, mw);
    }
    mp = episode_wave_min(mp);
    mv = episode_wave_min(mv);
    mw = episode_wave_min(mw);
    if (lane == 0) { red[wave][0] = mp; red[wave][1] = mv; red[wave][2] = mw; }
    __syncthreads();                                                   // (every wave of the workgroup reaches it)
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) {
        mp = fminf(mp, red[w][0]); mv = fminf(mv, red[w][1]); mw = fminf(mw, red[w][2]);
    }
    const int age = a.age[b] + 1;
    float goal_d2 = inf, prev = inf;
    int reason = 0;
    if (live) {
        const float4 o = a.own[s0 + ag];
        const float gx = o.x - x, gy = o.y - y;                        // the goal entry as observe forms it
        goal_d2 = fmaf(gx, gx, gy * gy);
        const float stored = a.prev_goal_d2[b];
        prev = stored != stored ? goal_d2 : stored;                    // NaN: the first live evaluation since the restart
        a.prev_goal_d2[b] = goal_d2;
        reason = (goal_d2 < es.goal_r2 ? 1 : 0) | (mp < es.ped_r2 ? 4 : 0) | (mv < es.veh_r2 ? 8 : 0);
    } else if (ag >= 0) {
        reason = 16;
    }
    if (es.max_steps > 0 && age >= es.max_steps) reason |= 2;
    const bool done = reason != 0;
    float4* out = reinterpret_cast<float4*>(a.record + (size_t)b * 8);
    out[0] = make_float4(done ? 1.0f : 0.0f, (float)reason, (float)age, goal_d2);
    out[1] = make_float4(prev, mp, mv, mw);
    a.done[b] = done ? 1 : 0;
    a.age[b] = age;
}

hipError_t launch_batch_episode(const EpisodeArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_episode_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
