// sfm_batch_vehicle_episode.hip -- episode ends per VEHICLE for gfx950 (MI355X) (sfm_batch_end_vehicle_step) and respawns of single
// vehicles from the snapshot (sfm_batch_respawn_vehicles_device); the record and the rules are specified in include/sfm_hip.h.
//
// A driving policy's loop ends an episode when its car arrives, runs out of time or touches something.  "Touches" is asked of the
// car's BODY: the oriented box of half-extents (ex, ey) around the centre, turned by the stored heading.  For a candidate point the
// gap is the distance from the point to that box (0 inside or on it), formed in the heading frame as the vehicle sensors form it;
// the record holds the squared minimum gap to the scene's live pedestrians, to the ring points of the scene's OTHER vehicles and to
// its border and static-obstacle points.
//
// sfm_batch_vehicle_episode_kernel (workgroup b, 4 waves, 8 KiB + 16 bytes of LDS):
//   1. the scene's agent vehicles are a list built by sfm_batch_set_vehicle_episodes (settings, not state); a scene without agents
//      returns after reading its count, before any barrier;
//   2. the scene's {x, y} are staged in LDS once, (+inf, +inf) for a row that is not live; then the one barrier of the loops;
//   3. a wave owns an agent vehicle (wave, wave + 4, .. of the list): centre, heading, extent and goal are wave-uniform loads, the 64
//      lanes stride over the rows, then over the ring points of the other vehicles (the own ring is skipped by its index range), then
//      over the border and static points, each lane keeping three running minima; the wave reduces them with __shfl_xor, after which
//      every lane holds them;
//   4. lane 0 takes the decisions and writes the record (two 16-byte stores), the byte and the two state words;
//   5. the scene's mask byte is the OR of the waves' results through four words of LDS behind a barrier every wave reaches (it sits
//      after the loops, whose trip counts are wave-uniform).
// A candidate counts only if row_live holds for it: an absent tracked vehicle's ring lies at +inf, and inf * 0 under a heading with a
// zero component is NaN, which fmaxf(NaN - ex, 0) would turn into a gap of 0.
// Determinism: no atomics, and only minima are taken.  A minimum of floats without NaNs does not depend on the order it is taken in,
// so a vehicle's record is bitwise the same alone, in any batch and under any split of the work.
//
// sfm_batch_vehicle_respawn_kernel (workgroup b, 4 waves): counts the scene's chosen vehicles in registers, agrees on "none" through
// one LDS flag per wave behind a barrier and leaves -- such a scene is not written at all.  Else a wave takes a chosen vehicle: lane
// 0 copies its centre and velocity, heading and autopilot cursor from the snapshot and starts its episode over, the 64 lanes copy
// its ring.
#include "sfm_device.h"
#include "sfm_interaction.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

struct VehicleEpisodeShared {
    float2 pos[BATCH_MAX_N];                                           // the scene's rows; (+inf, +inf): not live
    int done[WAVES_PER_BLOCK];
};

// The box a wave asks about: centre, stored heading, half-extents -- all wave-uniform.
struct VehicleBox { float cx, cy, hx, hy, ex, ey; };

// gap2 of include/sfm_hip.h: the squared distance from p to the box, 0 inside or on it.
__device__ __forceinline__ float box_gap2(const VehicleBox& o, float px, float py) {
    const float dx = px - o.cx, dy = py - o.cy;
    const float u = fmaf(o.hx, dx, o.hy * dy), v = fmaf(o.hx, dy, -(o.hy * dx));     // the sensors' rotation into the heading frame
    const float ax = fmaxf(fabsf(u) - o.ex, 0.0f), ay = fmaxf(fabsf(v) - o.ey, 0.0f);
    return fmaf(ax, ax, ay * ay);
}

// This lane's share of the minimum gap2 over pts[p0 .. p1) without [lo, hi); only live points count.
__device__ __forceinline__ float box_points(const VehicleBox& o, const float2* pts, int p0, int p1, int lo, int hi, int lane, float m) {
#pragma unroll 2
    for (int p = p0 + lane; p < p1; p += WAVE) {
        if (p >= lo && p < hi) continue;
        const float2 c = pts[p];
        if (row_live(c.x, c.y)) m = fminf(m, box_gap2(o, c.x, c.y));
    }
    return m;
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_episode_kernel(const VehicleEpisodeArgs a) {
    __shared__ VehicleEpisodeShared sh;
    const int b = blockIdx.x;
    const int a0 = a.agent_off[b], na = a.agent_off[b + 1] - a0;
    if (na <= 0) return;                                               // uniform: the scene has no agent vehicle, before any barrier
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const float inf = __builtin_inff();
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    for (int j = tid; j < n; j += BLOCK) {
        const float4 p = a.pk[s0 + j];
        sh.pos[j] = row_live(p.x, p.y) ? make_float2(p.x, p.y) : make_float2(inf, inf);
    }
    const VehicleEpisodeScene es = a.set[b];
    // the scene's points of each kind: one contiguous run of the kind's CSR; an empty kind's arrays are not read
    int r0[3], r1[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int k0 = a.geo[g].item_off[b], k1 = a.geo[g].item_off[b + 1];
        r0[g] = k1 > k0 ? a.geo[g].off[k0] : 0;
        r1[g] = k1 > k0 ? a.geo[g].off[k1] : 0;
    }
    __syncthreads();                                                   // the rows are in LDS
    int any = 0;
#pragma unroll 1
    for (int q = wave; q < na; q += WAVES_PER_BLOCK) {                 // wave-uniform
        const int k = uniform(a.agent_veh[a0 + q]);                    // a vehicle of scene b (built on the host)
        const float4 c = a.geo[2].ctr[k];
        const float2 h = a.rot[k];
        const float4 ge = a.goal_ext[k];
        const VehicleBox o{c.x, c.y, h.x, h.y, ge.z, ge.w};
        const bool live = row_live(c.x, c.y);                          // wave-uniform
        const int age = a.age[k] + 1;
        float mp = inf, mv = inf, mw = inf;
        float goal_d2 = inf, prev = inf;
        int reason = 16;
        if (live) {
#pragma unroll 2
            for (int j = lane; j < n; j += WAVE) {
                const float2 p = sh.pos[j];
                if (row_live(p.x, p.y)) mp = fminf(mp, box_gap2(o, p.x, p.y));
            }
            mv = box_points(o, a.geo[2].pts, r0[2], r1[2], a.geo[2].off[k], a.geo[2].off[k + 1], lane, mv);
            mw = box_points(o, a.geo[0].pts, r0[0], r1[0], 0, 0, lane, mw);
            mw = box_points(o, a.geo[1].pts, r0[1], r1[1], 0, 0, lane, mw);
#pragma unroll
            for (int m = WAVE / 2; m >= 1; m >>= 1) {
                mp = fminf(mp, __shfl_xor(mp, m)); mv = fminf(mv, __shfl_xor(mv, m)); mw = fminf(mw, __shfl_xor(mw, m));
            }
            const float gx = ge.x - c.x, gy = ge.y - c.y;
            goal_d2 = fmaf(gx, gx, gy * gy);
            const float stored = a.prev_goal_d2[k];
            prev = stored != stored ? goal_d2 : stored;                // NaN: the first live evaluation since the respawn
            reason = (goal_d2 < es.goal_r2 ? 1 : 0) | (mp < es.ped_r2 ? 4 : 0) | (mv < es.veh_r2 ? 8 : 0) | (mw < es.wall_r2 ? 32 : 0);
        }
        if (es.max_steps > 0 && age >= es.max_steps) reason |= 2;
        const bool done = reason != 0;                                 // (every lane holds the reduced minima: wave-uniform)
        any |= done ? 1 : 0;
        if (lane == 0) {
            float4* out = reinterpret_cast<float4*>(a.record + (size_t)k * 8);
            out[0] = make_float4(done ? 1.0f : 0.0f, (float)reason, (float)age, goal_d2);
            out[1] = make_float4(prev, mp, mv, mw);
            a.done[k] = done ? 1 : 0;
            a.age[k] = age;
            if (live) a.prev_goal_d2[k] = goal_d2;
        }
    }
    if (lane == 0) sh.done[wave] = any;
    __syncthreads();                                                   // every wave reaches it: the loop above holds no barrier
    if (tid == 0) {
        int f = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) f |= sh.done[w];
        a.scene_done[b] = f ? 1 : 0;
    }
}

// The vehicle episodes of the chosen scenes start over: launched behind sfm_batch_restart_kernel with the same choice of scenes (list
// / mask as in BatchRestart); other scenes are not touched.
__global__ __launch_bounds__(WAVE) void sfm_batch_vehicle_episode_restart_kernel(const int* list, const uint8_t* mask, const int* item_off,
                                                                                int* age, float* prev_goal_d2) {
    const int b = list ? list[blockIdx.x] : (int)blockIdx.x;
    if (mask && mask[b] == 0) return;                                  // uniform: the scene is not chosen
    const int k1 = item_off[b + 1];
    for (int k = item_off[b] + (int)threadIdx.x; k < k1; k += WAVE) {
        age[k] = 0;
        prev_goal_d2[k] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_respawn_kernel(const VehicleRespawnArgs a) {
    __shared__ int chosen[WAVES_PER_BLOCK];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const int k0 = a.item_off[b], k1 = a.item_off[b + 1];
    int c = 0;                                                         // this lane's chosen vehicles
    for (int k = k0 + tid; k < k1; k += BLOCK) c += a.mask[k] != 0 ? 1 : 0;
    const int mine = __any(c != 0) ? 1 : 0;
    if (lane == 0) chosen[wave] = mine;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; ++w) any |= chosen[w];
    if (!any) return;                                                  // uniform: no vehicle of the scene is chosen, nothing is written
#pragma unroll 1
    for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {            // wave-uniform
        if (a.mask[k] == 0) continue;
        if (lane == 0) {
            a.ctr[k] = a.s_ctr[k];
            a.rot[k] = a.s_rot[k];
            if (a.cursor) a.cursor[k] = a.s_cursor[k];
            if (a.age) { a.age[k] = 0; a.prev_goal_d2[k] = __builtin_nanf(""); }
        }
        const int p1 = a.veh_off[k + 1];
        for (int p = a.veh_off[k] + lane; p < p1; p += WAVE) a.pts[p] = a.s_pts[p];     // (pts is null only while no ring has a point)
    }
}

hipError_t launch_batch_vehicle_episode(const VehicleEpisodeArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_episode_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_vehicle_episode_restart(const int* list, const uint8_t* mask, const int* item_off, int* age, float* prev_goal_d2,
                                                int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_episode_restart_kernel, dim3(scenes), dim3(WAVE), 0, st, list, mask, item_off, age, prev_goal_d2);
    return hipGetLastError();
}

hipError_t launch_batch_vehicle_respawn(const VehicleRespawnArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_respawn_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
