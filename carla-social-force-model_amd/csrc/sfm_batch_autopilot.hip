// sfm_batch_autopilot.hip -- the vehicle autopilot of batched scenes for gfx950 (MI355X): ONE launch for the whole batch in front of
// every integrating tick (sfm_batch_set_vehicle_autopilot; the rule is specified in include/sfm_hip.h, operation by operation).
//
// Each autopiloted vehicle follows its path of waypoints under a bounded turn per tick and sets its speed by the Intelligent Driver
// Model against the nearest thing in its corridor: a pedestrian, a ring point of another vehicle, or the end of its path.  The kernel
// reads the buffers the tick behind it reads (state, the vehicles' half of the ping-pong, the headings) and writes the command of
// every autopiloted vehicle {speed, cos, sin, 2}, which that tick's vehicle prologue takes as a unicycle command (drive_vehicle),
// the cursor, and the record [M][8].  Entries of vehicles that are not autopiloted are not touched.
//
// Shape (workgroup b, 4 waves), sfm_batch_vehicle_observe_kernel's:
//   1. a scene without vehicles, or with none autopiloted, leaves at once; else the scene's {x, y, vx, vy} are staged in LDS once
//      (<= 16 KiB), then the one barrier;
//   2. a WAVE owns a vehicle: wave w takes the scene's vehicles k0 + w, k0 + w + 4, ... (k is wave-uniform: its centre, heading,
//      settings, cursor and path points are scalar loads), and its 64 lanes stride over the rows, and over each other vehicle's ring;
//   3. the leader is the minimum of (gap, kind << 28 | index) in lexicographic order: a lane walks its candidates in ascending key
//      with a strict `<`, then an xor-shuffle tree of widths 32 .. 1 takes the lower gap and, at equal gap, the lower key -- every
//      lane ends with the same pair, whatever the order of the tree.  A NaN gap is no candidate;
//   4. the cursor, the turn and the speed are computed by every lane alike (no divergence), lane 0 stores.
// Determinism: no atomics, no float sums over lanes, every order is a function of the scene alone -- a vehicle's command is bitwise
// the same alone or anywhere in any batch.
#include "sfm_device.h"
#include "sfm_interaction.h"

#pragma clang fp contract(off)     // every operation of the rule is a single rounding, or an explicit fmaf

namespace sfm {

struct AutopilotShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
};

constexpr int AUTOPILOT_NO_KEY = 0x7fffffff;
constexpr float AUTOPILOT_GAP_FLOOR = 0.01f;                           // SFM_AUTOPILOT_GAP_FLOOR

// the wave's minimum of (d, i) in lexicographic order, in every lane
__device__ __forceinline__ void autopilot_lex_min(float& d, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float od = __shfl_xor(d, m);
        const int oi = __shfl_xor(i, m);
        const bool take = od < d || (od == d && oi < i);
        d = take ? od : d;
        i = take ? oi : i;
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_autopilot_kernel(const AutopilotArgs a) {
    __shared__ AutopilotShared sh;
    const int b = blockIdx.x;
    const BatchGeo& gv = a.geo[2];
    const int k0 = gv.item_off[b], k1 = gv.item_off[b + 1];
    if (k1 <= k0) return;                                              // uniform: a scene without vehicles
    if (a.path_off[k1] == a.path_off[k0]) return;                      // uniform: none of them is autopiloted
    const int r0 = a.scene_off[b], n = a.scene_off[b + 1] - r0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    for (int t = threadIdx.x; t < n; t += BLOCK) sh.pk[t] = a.pk[r0 + t];
    __syncthreads();                                                   // (the only barrier: every wave is still here)
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = uniform((int)threadIdx.x >> 6);
    const float dt = a.prm[b].dt;
    const float inf = __builtin_inff();
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {            // wave-uniform
        const int p0 = a.path_off[k], P = a.path_off[k + 1] - p0;
        if (P <= 0) continue;                                          // not autopiloted: nothing of it is touched
        float4* rec = reinterpret_cast<float4*>(a.record + (size_t)k * 8);
        const float4 c = gv.ctr[k];
        if (!row_live(c.x, c.y)) {                                     // 1. absent: the tick keeps it absent, the cursor stays
            if (lane == 0) { a.cmd[k] = make_float4(0.f, 1.f, 0.f, 2.f); rec[0] = z4; rec[1] = z4; }
            continue;
        }
        const AutopilotVehicle s = a.set[k];
        const float2 h = a.rot[k];
        const bool loop = (s.flags & AUTOPILOT_LOOP) != 0;
        int cur = a.cursor[k];
        cur = (cur < 0 || cur >= P) ? 0 : cur;                         // (only this kernel and the restarts write it: always in range)
        // 2. the cursor: at most P steps while the waypoint is inside reach
        bool finished = false;
        float2 w = a.path[p0 + cur];
        float tx = w.x - c.x, ty = w.y - c.y;
        float n2 = fmaf(tx, tx, ty * ty);
#pragma unroll 1
        for (int i = 0; i < P && n2 < s.reach2; ++i) {
            if (!loop && cur == P - 1) { finished = true; break; }
            cur = cur + 1 == P ? 0 : cur + 1;
            w = a.path[p0 + cur];
            tx = w.x - c.x; ty = w.y - c.y;
            n2 = fmaf(tx, tx, ty * ty);
        }
        if (finished) {                                                // the end of an open path: stopped from then on
            if (lane == 0) {
                a.cursor[k] = cur;
                a.cmd[k] = make_float4(0.f, 1.f, 0.f, 2.f);
                rec[0] = make_float4((float)cur, 0.f, 0.f, 0.f);
                rec[1] = make_float4(0.f, 0.f, 0.f, 1.f);
            }
            continue;
        }
        // 3. the turn towards the waypoint, limited per tick
        float gx = h.x, gy = h.y;
        if (n2 > 0.0f) { const float nn = sqrtf(n2); gx = tx / nn; gy = ty / nn; }
        float cphi = fmaf(gx, h.x, gy * h.y);
        float sphi = fmaf(gy, h.x, -(gx * h.y));
        if (cphi < s.cos_max) { cphi = s.cos_max; sphi = sphi < 0.0f ? -s.sin_max : s.sin_max; }
        // 4. the leader: candidates in the frame of the stored heading, a lane's in ascending key
        float bg = inf, bu = 0.0f;
        int bkey = AUTOPILOT_NO_KEY;
        const float reachx = s.front + s.look;
        if (!(s.flags & AUTOPILOT_IGNORE_WALKERS)) {                   // uniform
            const float wide = s.half_width + s.ped_margin;
            for (int j = lane; j < n; j += WAVE) {
                const float4 pj = sh.pk[j];
                const float rx = pj.x - c.x, ry = pj.y - c.y;
                const float al = fmaf(rx, h.x, ry * h.y);
                const float ac = fmaf(rx, h.y, -(ry * h.x));
                const float gap = (al - s.front) - s.ped_margin;
                const bool take = row_live(pj.x, pj.y) && al > 0.0f && fabsf(ac) < wide && al < reachx && gap < bg;
                bg = take ? gap : bg;
                bu = take ? fmaf(pj.z, h.x, pj.w * h.y) : bu;
                bkey = take ? ((1 << AUTOPILOT_INDEX_BITS) | j) : bkey;
            }
        }
#pragma unroll 1
        for (int v = k0; v < k1; ++v) {                                // uniform: the other present vehicles, their rings by lanes
            if (v == k) continue;
            const float4 cv = gv.ctr[v];
            if (!row_live(cv.x, cv.y)) continue;
            const float uv = fmaf(cv.z, h.x, cv.w * h.y);
            const int o1 = gv.off[v + 1];
            for (int p = gv.off[v] + lane; p < o1; p += WAVE) {
                const float2 q = gv.pts[p];
                const float rx = q.x - c.x, ry = q.y - c.y;
                const float al = fmaf(rx, h.x, ry * h.y);
                const float ac = fmaf(rx, h.y, -(ry * h.x));
                const float gap = al - s.front;
                const bool take = al > 0.0f && fabsf(ac) < s.half_width && al < reachx && gap < bg;
                bg = take ? gap : bg;
                bu = take ? uv : bu;
                bkey = take ? ((2 << AUTOPILOT_INDEX_BITS) | (v - k0)) : bkey;
            }
        }
        if (!loop && cur == P - 1) {                                   // uniform: the end of an open path, no corridor test
            const float gap = sqrtf(n2);
            const bool take = gap < bg;
            bg = take ? gap : bg;
            bu = take ? 0.0f : bu;
            bkey = take ? (3 << AUTOPILOT_INDEX_BITS) : bkey;
        }
        const float lane_g = bg;
        const int lane_key = bkey;
        autopilot_lex_min(bg, bkey);
        const unsigned long long owner = __ballot(lane_g == bg && lane_key == bkey);
        bu = __shfl(bu, (int)__builtin_ctzll(owner | (1ull << 63)));    // the winner's speed along h (the same in each of its lanes)
        // 5. the speed: the Intelligent Driver Model; max(x, y) is x > y ? x : y throughout
        const float sp = fmaf(c.z, h.x, c.w * h.y);
        const float v = sp > 0.0f ? sp : 0.0f;
        const float q = v / s.v0;
        const float q2 = q * q;
        const float r4 = q2 * q2;
        float inter = 0.0f;
        const bool led = bkey != AUTOPILOT_NO_KEY;
        if (led) {                                                     // uniform
            const float g = bg > AUTOPILOT_GAP_FLOOR ? bg : AUTOPILOT_GAP_FLOOR;
            const float dv = v - bu;
            const float k2 = 2.0f * sqrtf(s.acc * s.dec);
            const float dyn = fmaf(v, s.T, (v * dv) / k2);
            const float sstar = s.s0 + (dyn > 0.0f ? dyn : 0.0f);
            const float ratio = sstar / g;
            inter = ratio * ratio;
        }
        const float araw = s.acc * ((1.0f - r4) - inter);
        const float nb = -s.brake;
        const float acc = araw > nb ? araw : nb;
        const float sn = fmaf(dt, acc, v);
        const float s1 = sn > 0.0f ? sn : 0.0f;
        // 6. the command, the cursor and the record
        if (lane == 0) {
            a.cursor[k] = cur;
            a.cmd[k] = make_float4(s1, cphi, sphi, 2.0f);
            rec[0] = make_float4((float)cur, led ? (float)(bkey >> AUTOPILOT_INDEX_BITS) : 0.0f,
                                 led ? (float)(bkey & ((1 << AUTOPILOT_INDEX_BITS) - 1)) : 0.0f, led ? bg : 0.0f);
            rec[1] = make_float4(led ? bu : 0.0f, acc, s1, 0.0f);
        }
    }
}

// The cursors of the chosen scenes back to the snapshot: launched behind sfm_batch_restart_kernel with the same choice of scenes
// (list / mask as in BatchRestart); other scenes are not touched.
__global__ __launch_bounds__(WAVE) void sfm_batch_autopilot_restart_kernel(const int* list, const uint8_t* mask, const int* item_off,
                                                                           int* cursor, const int* s_cursor) {
    const int b = list ? list[blockIdx.x] : (int)blockIdx.x;
    if (mask && mask[b] == 0) return;
    const int k1 = item_off[b + 1];
    for (int k = item_off[b] + (int)threadIdx.x; k < k1; k += WAVE) cursor[k] = s_cursor[k];
}

hipError_t launch_batch_vehicle_autopilot(const AutopilotArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_autopilot_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_autopilot_restart(const int* list, const uint8_t* mask, const int* item_off, int* cursor, const int* s_cursor,
                                          int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_autopilot_restart_kernel, dim3(scenes), dim3(WAVE), 0, st, list, mask, item_off, cursor, s_cursor);
    return hipGetLastError();
}

}  // namespace sfm
