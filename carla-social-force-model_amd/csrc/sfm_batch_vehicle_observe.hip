// sfm_batch_vehicle_observe.hip -- per-vehicle observations of batched scenes for gfx950 (MI355X): ONE launch for the whole batch
// (sfm_batch_observe_vehicles; the record is specified in include/sfm_hip.h).
//
// What a driving policy and its reward read per vehicle: its goal, velocity and heading, its K nearest pedestrians inside the scene's
// sense range and how they move relative to it, the clearance between its ring and the crowd, the distance to the scene's other
// vehicles, and the nearest border and static-obstacle points -- computed from the buffers the next tick reads (state, the scene
// offsets, the three geometry CSRs, the headings), into a device buffer [M][16 + 4k] of floats.  The kernel writes nothing else, so a
// tick before or after it computes what it computed without it.
//
// Shape (workgroup b, 4 waves):
//   1. the scene's {x, y, vx, vy} are staged in LDS once (<= 16 KiB), then the one barrier; a scene without vehicles leaves before it;
//   2. a WAVE owns a vehicle: wave w takes the scene's vehicles k0 + w, k0 + w + 4, ... (k is wave-uniform, its centre, heading and
//      goal are scalar loads), and its 64 lanes stride over whatever is searched: rows, ring points, polyline points, vehicles;
//   3. every search is a minimum of (d2, index) in lexicographic order: a lane walks its candidates in ascending index with a strict
//      `<` (the first minimum of its own), then an xor-shuffle tree of widths 32 .. 1 takes the lower d2 and, at equal d2, the lower
//      index -- every lane ends with the same pair, whatever the order of the tree.  A NaN distance is no candidate;
//   4. neighbours: slot s is the minimum over the live rows with d2 < R2 that come AFTER slot s - 1 in (d2, j) order -- k passes over
//      the staged rows, no sorting network, no register array; the passes stop at the first empty slot;
//   5. lane 0 stores the record with 16-byte stores.
// Frame 1 rotates every 2-vector but the heading into the vehicle's heading frame AFTER everything is selected, so selection, order,
// m, flags and the three distances are those of frame 0.
// Determinism: no atomics, every order is a function of the scene alone -- a vehicle's record is bitwise the same alone or anywhere
// in any batch.  A vehicle outside the mask is skipped by its wave: it costs nothing, and its record stays the zeros the buffer was
// filled with.
#include "sfm_device.h"
#include "sfm_interaction.h"

namespace sfm {

struct VehicleObserveShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
};

constexpr int NO_INDEX = 0x7fffffff;

// the wave's minimum of (d, i) in lexicographic order, in every lane
__device__ __forceinline__ void wave_lex_min(float& d, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float od = __shfl_xor(d, m);
        const int oi = __shfl_xor(i, m);
        const bool take = od < d || (od == d && oi < i);
        d = take ? od : d;
        i = take ? oi : i;
    }
}

// first minimum of the squared distance from (cx, cy) over all points of one kind of scene b, polylines in order, points in order
__device__ __forceinline__ void vehicle_nearest_point(const BatchGeo& g, int b, float cx, float cy, int lane, float& d2, float2& pt) {
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
    float bd = __builtin_inff();
    int bi = NO_INDEX;
    if (k1 > k0) {                                                     // uniform; the scene's points are one ascending range of pts
        const int p1 = g.off[k1];
        for (int p = g.off[k0] + lane; p < p1; p += WAVE) {
            const float2 q = g.pts[p];
            const float dx = q.x - cx, dy = q.y - cy;
            const float d = fmaf(dx, dx, dy * dy);
            const bool take = d < bd;
            bd = take ? d : bd;
            bi = take ? p : bi;
        }
    }
    wave_lex_min(bd, bi);
    d2 = bd;
    pt = make_float2(0.f, 0.f);
    if (bi != NO_INDEX) pt = g.pts[bi];                                // uniform
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_observe_kernel(const VehicleObserveArgs a) {
    __shared__ VehicleObserveShared sh;
    const int b = blockIdx.x;
    const BatchGeo& gv = a.geo[2];
    const int k0 = gv.item_off[b], k1 = gv.item_off[b + 1];
    if (k1 <= k0) return;                                              // uniform: a scene without vehicles
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    for (int t = threadIdx.x; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    __syncthreads();                                                   // (the only barrier: every wave is still here)
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = uniform((int)threadIdx.x >> 6);
    const float R2 = a.range2[b];
    const float inf = __builtin_inff();
    const int K = a.k;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {            // wave-uniform
        if (a.mask && a.mask[k] == 0) continue;                        // not observed: its record stays zeros
        float4* out = reinterpret_cast<float4*>(a.obs + (size_t)k * (size_t)(16 + 4 * K));
        const float4 c = gv.ctr[k];
        if (!row_live(c.x, c.y)) {                                     // absent (or not finite): the whole record is zeros
            for (int q = lane; q < 4 + K; q += WAVE) out[q] = z4;
            continue;
        }
        const float2 h = a.rot[k];
        const float2 goal = a.goal[k];
        auto rot = [&](float& p, float& q) {                           // frame 1: into the heading frame
            const float rp = fmaf(h.x, p, h.y * q), rq = fmaf(h.x, q, -(h.y * p));
            p = rp; q = rq;
        };
        // neighbours: slot s = the (d2, j) minimum behind slot s - 1
        float ld = -1.0f;                                              // (d2 >= 0: everything comes after it)
        int lj = -1, m = 0;
#pragma unroll 1
        for (int s = 0; s < K; ++s) {
            float bd = inf;
            int bj = NO_INDEX;
            for (int j = lane; j < n; j += WAVE) {
                const float4 pj = sh.pk[j];
                const float dx = pj.x - c.x, dy = pj.y - c.y;
                const float d = fmaf(dx, dx, dy * dy);
                const bool cand = row_live(pj.x, pj.y) && d < R2 && (d > ld || (d == ld && j > lj));
                const bool take = cand && d < bd;
                bd = take ? d : bd;
                bj = take ? j : bj;
            }
            wave_lex_min(bd, bj);
            if (bj == NO_INDEX) break;                                 // uniform: no row is left
            const float4 pj = sh.pk[bj];
            float4 e = make_float4(pj.x - c.x, pj.y - c.y, pj.z - c.z, pj.w - c.w);
            if (a.frame) { rot(e.x, e.y); rot(e.z, e.w); }
            if (lane == 0) out[4 + s] = e;
            ld = bd; lj = bj; m = s + 1;
        }
        for (int q = m + lane; q < K; q += WAVE) out[4 + q] = z4;      // the empty slots
        // clear_d2: ring points x live rows, not limited by the range
        float clear = inf;
        {
            const int o0 = gv.off[k], o1 = gv.off[k + 1];
            for (int j = lane; j < n; j += WAVE) {
                const float4 pj = sh.pk[j];
                if (!row_live(pj.x, pj.y)) continue;
                for (int p = o0; p < o1; ++p) {                        // uniform: scalar loads
                    const float2 q = gv.pts[p];
                    const float dx = pj.x - q.x, dy = pj.y - q.y;
                    const float d = fmaf(dx, dx, dy * dy);
                    clear = d < clear ? d : clear;
                }
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) { const float o = __shfl_xor(clear, w); clear = o < clear ? o : clear; }
        }
        // other_d2: the other present vehicles of the scene
        float other = inf;
        for (int v = k0 + lane; v < k1; v += WAVE) {
            const float4 cv = gv.ctr[v];
            const float dx = cv.x - c.x, dy = cv.y - c.y;
            const float d = fmaf(dx, dx, dy * dy);
            other = (v != k && row_live(cv.x, cv.y) && d < other) ? d : other;
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) { const float o = __shfl_xor(other, w); other = o < other ? o : other; }
        float db, ds;
        float2 pb, ps;
        vehicle_nearest_point(a.geo[0], b, c.x, c.y, lane, db, pb);
        vehicle_nearest_point(a.geo[1], b, c.x, c.y, lane, ds, ps);
        const bool hb = db < R2, hs = ds < R2;
        float4 h0 = make_float4(goal.x - c.x, goal.y - c.y, c.z, c.w);
        float4 h2 = make_float4(hb ? pb.x - c.x : 0.f, hb ? pb.y - c.y : 0.f, hs ? ps.x - c.x : 0.f, hs ? ps.y - c.y : 0.f);
        const float along = fmaf(c.z, h.x, c.w * h.y);
        if (a.frame) {                                                 // uniform
            rot(h0.x, h0.y); rot(h0.z, h0.w);
            rot(h2.x, h2.y); rot(h2.z, h2.w);
        }
        if (lane == 0) {
            out[0] = h0;
            out[1] = make_float4(h.x, h.y, 1.0f, (float)m);
            out[2] = make_float4(clear, other, h2.x, h2.y);
            out[3] = make_float4(h2.z, h2.w, (float)((hb ? 1 : 0) + (hs ? 2 : 0)), along);
        }
    }
}

hipError_t launch_batch_vehicle_observe(const VehicleObserveArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_observe_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
