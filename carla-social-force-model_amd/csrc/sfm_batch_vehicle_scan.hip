// sfm_batch_vehicle_scan.hip -- range scans cast from the vehicles of batched scenes for gfx950 (MI355X): ONE launch for the whole
// batch (sfm_batch_scan_vehicles; the record and its rules are specified in include/sfm_hip.h).
//
// What a driving policy sees per vehicle: R rays from a sensor mounted on the vehicle, each giving the distance to the first disc it
// meets -- every pedestrian of the scene is a disc of ped_radius, every sampled point of a border, a static-obstacle ring or the ring
// of ANOTHER vehicle a disc of point_radius -- and the kind of what it met.  The vehicle's own ring is left out: a lidar does not see
// the body it is bolted to.  Computed from the buffers the next tick reads (state, the scene offsets, the three geometry CSRs, the
// headings) into a device buffer [M][2R] of floats.  The kernel writes nothing else, so a tick before or after it computes what it
// computed without it.
//
// Shape (workgroup b, 4 waves), sfm_batch_scan_kernel's with vehicles in place of rows:
//   1. a scene without vehicles leaves at once; else the scene's {x, y, vx, vy} (possibly none: the geometry is still scanned) and
//      the R directions are staged in LDS, then a barrier;
//   2. the vehicles that are scanned (mask) and present are compacted, in ascending order, into an LDS list by ballots and per-wave
//      counts, BLOCK vehicles per chunk (a scene rarely has more than a handful; the chunk loop only keeps the list bounded).  The
//      thread that lists a vehicle forms its sensor origin once and notes where its own ring lies in the geometry's virtual run; a
//      vehicle that is scanned and not present gets its zeros here; a masked-out vehicle is never touched (the buffer was zero-filled);
//   3. a lane owns a (vehicle, ray) pair, the ray index fastest: item = list position * R + ray, 256 items per pass.  The lane forms
//      its ray (frame 1: rotated by the STORED heading) and walks the candidates in the record's fixed order -- every pedestrian j
//      ascending as broadcast LDS reads, then the scene's border, static and vehicle points, staged cooperatively in LDS tiles of
//      VSCAN_TILE points and read as broadcasts -- keeping the first minimum under strict `<`.  Among the vehicle points the lane's
//      own ring is skipped by its index range in the run, which may begin or end inside a tile or inside a wave's share.
//      With at most 64 (128) items -- one ego vehicle per scene -- 4 (2) waves share each item's candidates, a contiguous share of
//      the fixed order each, and the shares are combined in that order through LDS under strict `<`;
//   4. the lane stores its range and kind; consecutive lanes store consecutive floats.
// Which split a chunk takes cannot change a value: the first minimum of the fixed order does not depend on how the order is cut.
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or anywhere in
// any batch.
#include "sfm_device.h"
#include "sfm_scan_disc.h"     // scan_disc, scan_points: shared by the two scan kernels

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int VSCAN_TILE = 512;    // geometry points per LDS tile

struct VehicleScanShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    float2 tile[VSCAN_TILE];                                           // geometry points of the current tile
    float2 dir[VEHICLE_SCAN_MAX_RAYS];                                 // the ray directions
    float4 org[BLOCK];                                                 // the listed vehicles, ascending: {ox, oy, hx, hy} ...
    int4 who[BLOCK];                                                   // ... and {vehicle, own ring [lo, hi) in the virtual run, 0}
    int wcount[WAVES_PER_BLOCK];
    float2 part[WAVES_PER_BLOCK][WAVE];                                // few items: the (range, kind) each wave found in its share
};

// scan_points for the vehicle points: tile entries [own, own + len) are the lane's own ring and are no candidates (own may be
// negative or past hi: the ring begins before this tile, or lies outside it).  One unsigned compare per point, per lane.
__device__ __forceinline__ void scan_other_rings(const float2* tile, int lo, int hi, int own, unsigned len, float x, float y, float ux,
                                                 float uy, float r2, float rr, float& best, float& bkind) {
    int e = lo;
#pragma unroll 1
    for (; e + 4 <= hi; e += 4) {                                      // uniform: the LDS reads are broadcasts
        const float2 p0 = tile[e], p1 = tile[e + 1], p2 = tile[e + 2], p3 = tile[e + 3];
        scan_disc(p0.x - x, p0.y - y, ux, uy, r2, rr, (unsigned)(e - own) >= len, 4.0f, best, bkind);
        scan_disc(p1.x - x, p1.y - y, ux, uy, r2, rr, (unsigned)(e + 1 - own) >= len, 4.0f, best, bkind);
        scan_disc(p2.x - x, p2.y - y, ux, uy, r2, rr, (unsigned)(e + 2 - own) >= len, 4.0f, best, bkind);
        scan_disc(p3.x - x, p3.y - y, ux, uy, r2, rr, (unsigned)(e + 3 - own) >= len, 4.0f, best, bkind);
    }
#pragma unroll 1
    for (; e < hi; ++e) {
        const float2 p = tile[e];
        scan_disc(p.x - x, p.y - y, ux, uy, r2, rr, (unsigned)(e - own) >= len, 4.0f, best, bkind);
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_scan_kernel(const VehicleScanArgs a) {
    __shared__ VehicleScanShared sh;
    const int b = blockIdx.x;
    const int vk0 = a.geo[2].item_off[b], vk1 = a.geo[2].item_off[b + 1];
    if (vk1 <= vk0) return;                                            // uniform: a scene without vehicles, before any barrier
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host); 0 is scanned too
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R;                                                 // 1 .. VEHICLE_SCAN_MAX_RAYS (= BLOCK)
    for (int t = tid; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    if (tid < R) sh.dir[tid] = a.dir[tid];

    const BatchVehicleScanScene set = a.set[b];
    const float Rmax = set.max_range, ped_r2 = set.ped_r2, point_r2 = set.point_r2;
    // the scene's points per kind: one contiguous run of the kind's CSR (an empty kind's arrays are not read)
    const int bk0 = a.geo[0].item_off[b], bk1 = a.geo[0].item_off[b + 1];
    const int sk0 = a.geo[1].item_off[b], sk1 = a.geo[1].item_off[b + 1];
    const int bp0 = bk1 > bk0 ? a.geo[0].off[bk0] : 0, nb = bk1 > bk0 ? a.geo[0].off[bk1] - bp0 : 0;
    const int sp0 = sk1 > sk0 ? a.geo[1].off[sk0] : 0, ns = sk1 > sk0 ? a.geo[1].off[sk1] - sp0 : 0;
    const int vp0 = a.geo[2].off[vk0], nv = a.geo[2].off[vk1] - vp0;
    const int G = point_r2 > 0.0f ? nb + ns + nv : 0;                  // virtual index g: borders, static, vehicles
    const bool one_tile = G <= VSCAN_TILE;

    auto stage = [&](int g0, int cnt) {                                // points [g0, g0 + cnt) of the virtual run into the tile
        for (int e = tid; e < cnt; e += BLOCK) {
            const int g = g0 + e;
            sh.tile[e] = g < nb ? a.geo[0].pts[bp0 + g] : g < nb + ns ? a.geo[1].pts[sp0 + (g - nb)] : a.geo[2].pts[vp0 + (g - nb - ns)];
        }
    };
    if (one_tile) stage(0, G);                                         // the whole scene's geometry fits: staged once
    __syncthreads();

    const int T = n + G;                                               // candidates in the fixed order (the own ring included)
    const float ped_rr = sqrtf(ped_r2), point_rr = sqrtf(point_r2);
    const float mx = a.mount_x, my = a.mount_y;
#pragma unroll 1
    for (int base = vk0; base < vk1; base += BLOCK) {                  // uniform: one chunk of the scene's vehicles
        // 2. the scanned present vehicles of the chunk, ascending
        const int k = base + tid;
        bool scan = false;
        float4 org = make_float4(0.f, 0.f, 0.f, 0.f);
        int4 who = make_int4(0, 0, 0, 0);
        if (k < vk1 && (!a.mask || a.mask[k] != 0)) {
            const float4 c = a.geo[2].ctr[k];
            if (row_live(c.x, c.y)) {
                const float2 h = a.rot[k];
                const float rx = fmaf(h.x, mx, -(h.y * my));           // the mount, turned by the stored heading
                const float ry = fmaf(h.y, mx, h.x * my);
                org = make_float4(c.x + rx, c.y + ry, h.x, h.y);
                who = make_int4(k, nb + ns + (a.geo[2].off[k] - vp0), nb + ns + (a.geo[2].off[k + 1] - vp0), 0);
                scan = true;
            } else {                                                   // absent (or not finite): the whole record is zeros
                float* out = a.out + (size_t)k * (size_t)(2 * R);
                for (int q = 0; q < 2 * R; ++q) out[q] = 0.0f;
            }
        }
        const unsigned long long m = __ballot(scan);
        if (lane == 0) sh.wcount[wave] = __popcll(m);
        __syncthreads();                                               // (and every wave is done with the chunk before: org, who, part)
        int before = 0, n_scan = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) {
            const int cw = sh.wcount[w];
            before += w < wave ? cw : 0;
            n_scan += cw;
        }
        if (scan) {
            const int p = before + __popcll(m & ((1ull << lane) - 1ull));
            sh.org[p] = org;
            sh.who[p] = who;
        }
        __syncthreads();                                               // the list; and wcount is rewritten by the next chunk
        if (n_scan == 0) continue;                                     // uniform

        // Few items: `split` waves share an item's candidates -- each walks one contiguous share of the fixed order (pedestrians,
        // then the geometry's virtual run) and the shares' results are combined in that order under strict `<`: the first minimum
        // of the whole.  The own ring may lie in one share or across two: the skip is by index, whoever walks the point.
        const unsigned total = (unsigned)n_scan * (unsigned)R;         // <= BLOCK * VEHICLE_SCAN_MAX_RAYS
        const int split = total <= WAVE ? 4 : total <= 2 * WAVE ? 2 : 1;   // uniform
        const int sub = wave % split, group = wave / split;
        const int v0 = (int)((long long)T * sub / split), v1 = (int)((long long)T * (sub + 1) / split);
        const int j0 = min(v0, n), j1 = min(v1, n);                     // this wave's pedestrians ...
        const int w0 = max(v0 - n, 0), w1 = max(v1 - n, 0);             // ... and its part of the virtual run
        const unsigned per_pass = (unsigned)(BLOCK / split);
#pragma unroll 1
        for (unsigned c0 = 0; c0 < total; c0 += per_pass) {            // uniform
            const unsigned first = c0 + (unsigned)(group * WAVE);
            const bool wave_has = first < total;                       // uniform per wave
            const unsigned item = first + (unsigned)lane;
            const bool there = item < total;
            const unsigned it = there ? item : total - 1;              // (a lane without an item repeats the last: every lane votes)
            const unsigned pos = it / (unsigned)R;
            const int ray = (int)(it - pos * (unsigned)R);
            const float4 o = sh.org[pos];
            const int4 me = sh.who[pos];
            const float x = o.x, y = o.y;
            const float2 u0 = sh.dir[ray];
            float ux = u0.x, uy = u0.y;
            if (a.frame) {                                             // uniform: the ray in the vehicle's heading frame
                ux = fmaf(o.z, u0.x, -(o.w * u0.y));
                uy = fmaf(o.w, u0.x, o.z * u0.y);
            }
            float best = Rmax, bkind = 0.0f;                           // a range >= Rmax is never stored, so it is never taken
            if (wave_has && ped_r2 > 0.0f) {
                int j = j0;
#pragma unroll 1
                for (; j + 4 <= j1; j += 4) {                          // uniform: the LDS reads are broadcasts, four in flight
                    const float4 p0 = sh.pk[j], p1 = sh.pk[j + 1], p2 = sh.pk[j + 2], p3 = sh.pk[j + 3];
                    scan_disc(p0.x - x, p0.y - y, ux, uy, ped_r2, ped_rr, true, 1.0f, best, bkind);
                    scan_disc(p1.x - x, p1.y - y, ux, uy, ped_r2, ped_rr, true, 1.0f, best, bkind);
                    scan_disc(p2.x - x, p2.y - y, ux, uy, ped_r2, ped_rr, true, 1.0f, best, bkind);
                    scan_disc(p3.x - x, p3.y - y, ux, uy, ped_r2, ped_rr, true, 1.0f, best, bkind);
                }
#pragma unroll 1
                for (; j < j1; ++j) {
                    const float4 pj = sh.pk[j];
                    scan_disc(pj.x - x, pj.y - y, ux, uy, ped_r2, ped_rr, true, 1.0f, best, bkind);
                }
            }
#pragma unroll 1
            for (int g0 = 0; g0 < G; g0 += VSCAN_TILE) {               // uniform
                const int cnt = min(VSCAN_TILE, G - g0);
                if (!one_tile) {
                    __syncthreads();                                   // everyone is done with the tile before
                    stage(g0, cnt);
                    __syncthreads();
                }
                if (!wave_has) continue;
                // the tile's share of each kind, in order, cut to this wave's part [w0, w1) of the run
                const int lo = min(max(w0 - g0, 0), cnt), hi = min(max(w1 - g0, 0), cnt);
                const int e1 = min(max(nb - g0, lo), hi), e2 = min(max(nb + ns - g0, lo), hi);
                scan_points(sh.tile, lo, e1, x, y, ux, uy, point_r2, point_rr, 2.0f, best, bkind);
                scan_points(sh.tile, e1, e2, x, y, ux, uy, point_r2, point_rr, 3.0f, best, bkind);
                scan_other_rings(sh.tile, e2, hi, me.y - g0, (unsigned)(me.z - me.y), x, y, ux, uy, point_r2, point_rr, best, bkind);
            }
            if (split > 1) {                                           // uniform: the shares of an item, combined in order
                sh.part[wave][lane] = make_float2(best, bkind);
                __syncthreads();
                if (sub == 0) {
#pragma unroll
                    for (int w = 1; w < WAVES_PER_BLOCK; ++w) {
                        if (w >= split) break;                         // uniform
                        const float2 p = sh.part[wave + w][lane];
                        const bool take = p.x < best;
                        best = take ? p.x : best;
                        bkind = take ? p.y : bkind;
                    }
                }
                __syncthreads();                                       // (the next pass rewrites part: split > 1 has one pass only)
            }
            if (there && sub == 0) {
                float* out = a.out + (size_t)me.x * (size_t)(2 * R);
                out[ray] = best;
                out[R + ray] = bkind;
            }
        }
    }
}

hipError_t launch_batch_vehicle_scan(const VehicleScanArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_scan_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
