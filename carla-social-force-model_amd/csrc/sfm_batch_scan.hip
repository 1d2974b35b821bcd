// sfm_batch_scan.hip -- range scans (ray-cast observations) of batched scenes for gfx950 (MI355X): ONE launch for the whole batch
// (sfm_batch_scan, ABI 17; the record and its rules are specified in include/sfm_hip.h).
//
// What a policy sees per agent: R rays around the row, each giving the distance to the first disc it meets -- every other
// pedestrian of the scene is a disc of ped_radius, every sampled point of a border, a static-obstacle ring or a vehicle ring a disc
// of point_radius -- and the kind of what it met.  Computed from the buffers the tick reads (state, own, the scene offsets, the three
// geometry CSRs) into a device buffer [N_total][2R] of floats.  The kernel writes nothing else, so a tick before or after it
// computes what it computed without it.
//
// Shape (workgroup b, 4 waves):
//   1. the scene's {x, y, vx, vy} and the R directions are staged in LDS, then a barrier;
//   2. the rows that are scanned (mask) and live are compacted, in ascending order, into an LDS list by ballots and per-wave counts;
//      a row that is scanned and not live gets its zeros here; a masked-out row is never touched (the buffer was zero-filled);
//   3. a lane owns a (row, ray) pair, the ray index fastest: item = list position * R + ray, 256 items per pass.  The lane forms its
//      ray (frame 1: rotated by the row's heading) and walks the candidates in the record's fixed order -- pedestrians j ascending
//      as broadcast LDS reads, then the scene's border, static and vehicle points, staged cooperatively in LDS tiles of SCAN_TILE
//      points and read as broadcasts -- keeping the first minimum under strict `<`.  The scene's points of one kind are one
//      contiguous run of the kind's CSR (polylines in order, points in order), so the walk needs no polyline structure;
//      With at most 64 (128) items -- an RL loop's one agent row per scene -- 4 (2) waves share each item's candidates, a contiguous
//      share of the fixed order each, and the shares are combined in that order through LDS under strict `<`;
//   4. the lane stores its range and kind; consecutive lanes store consecutive floats.
// Skips, all exact: a kind whose r2 is 0 is not walked (q = -c^2 <= 0 is never a candidate); a range >= Rmax is never taken (it is
// never stored); the square root and what follows it are skipped while no lane of the wave can take the disc (scan_disc).
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or anywhere in
// any batch.
#include "sfm_device.h"
#include "sfm_scan_disc.h"     // scan_disc, scan_points: shared by the two scan kernels

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int SCAN_TILE = 512;     // geometry points per LDS tile

struct ScanShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    float2 tile[SCAN_TILE];                                            // geometry points of the current tile
    float2 dir[SCAN_MAX_RAYS];                                         // the ray directions
    unsigned short rows[BATCH_MAX_N];                                  // the scanned live rows, ascending
    int wcount[WAVES_PER_BLOCK];
    float2 part[WAVES_PER_BLOCK][WAVE];                                // few items: the (range, kind) each wave found in its share
};

__global__ __launch_bounds__(BLOCK) void sfm_batch_scan_kernel(const ScanArgs a) {
    __shared__ ScanShared sh;
    const int b = blockIdx.x;
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    if (n <= 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R;                                                 // 1 .. SCAN_MAX_RAYS
    for (int t = tid; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    if (tid < R) sh.dir[tid] = a.dir[tid];
    __syncthreads();

    // 2. the scanned live rows, ascending
    int n_scan = 0;
#pragma unroll 1
    for (int base = 0; base < n; base += BLOCK) {                      // uniform
        const int t = base + tid;
        bool scan = false;
        if (t < n) {
            const float4 s = sh.pk[t];
            const bool want = !a.mask || a.mask[s0 + t] != 0;
            const bool live = row_live(s.x, s.y);
            scan = want && live;
            if (want && !live) {
                float* out = a.out + (size_t)(s0 + t) * (size_t)(2 * R);
                for (int q = 0; q < 2 * R; ++q) out[q] = 0.0f;
            }
        }
        const unsigned long long m = __ballot(scan);
        if (lane == 0) sh.wcount[wave] = __popcll(m);
        __syncthreads();
        int before = n_scan, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) {
            const int cw = sh.wcount[w];
            before += w < wave ? cw : 0;
            all += cw;
        }
        if (scan) sh.rows[before + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)t;
        n_scan += all;
        __syncthreads();                                               // the list; and wcount is rewritten by the next pass
    }
    if (n_scan == 0) return;                                           // uniform

    const BatchScanScene set = a.set[b];
    const float Rmax = set.max_range, ped_r2 = set.ped_r2, point_r2 = set.point_r2;
    // the scene's points per kind: one contiguous run of the kind's CSR (an empty kind's arrays are not read)
    const int bk0 = a.geo[0].item_off[b], bk1 = a.geo[0].item_off[b + 1];
    const int sk0 = a.geo[1].item_off[b], sk1 = a.geo[1].item_off[b + 1];
    const int vk0 = a.geo[2].item_off[b], vk1 = a.geo[2].item_off[b + 1];
    const int bp0 = bk1 > bk0 ? a.geo[0].off[bk0] : 0, nb = bk1 > bk0 ? a.geo[0].off[bk1] - bp0 : 0;
    const int sp0 = sk1 > sk0 ? a.geo[1].off[sk0] : 0, ns = sk1 > sk0 ? a.geo[1].off[sk1] - sp0 : 0;
    const int vp0 = vk1 > vk0 ? a.geo[2].off[vk0] : 0, nv = vk1 > vk0 ? a.geo[2].off[vk1] - vp0 : 0;
    const int G = point_r2 > 0.0f ? nb + ns + nv : 0;                  // virtual index g: borders, static, vehicles
    const bool one_tile = G <= SCAN_TILE;

    auto stage = [&](int g0, int cnt) {                                // points [g0, g0 + cnt) of the virtual run into the tile
        for (int e = tid; e < cnt; e += BLOCK) {
            const int g = g0 + e;
            sh.tile[e] = g < nb ? a.geo[0].pts[bp0 + g] : g < nb + ns ? a.geo[1].pts[sp0 + (g - nb)] : a.geo[2].pts[vp0 + (g - nb - ns)];
        }
    };
    if (one_tile && G > 0) {                                           // the whole scene's geometry fits: staged once
        stage(0, G);
        __syncthreads();
    }

    // Few items: `split` waves share an item's candidates -- each walks one contiguous share of the fixed order (pedestrians, then
    // the geometry's virtual run) and the shares' results are combined in that order under strict `<`: the first minimum of the whole.
    const unsigned total = (unsigned)n_scan * (unsigned)R;
    const int split = total <= WAVE ? 4 : total <= 2 * WAVE ? 2 : 1;   // uniform
    const int sub = wave % split, group = wave / split;
    const int T = n + G;                                               // candidates in the fixed order (row i itself included)
    const int v0 = (int)((long long)T * sub / split), v1 = (int)((long long)T * (sub + 1) / split);
    const int j0 = min(v0, n), j1 = min(v1, n);                         // this wave's pedestrians ...
    const int w0 = max(v0 - n, 0), w1 = max(v1 - n, 0);                 // ... and its part of the virtual run
    const float ped_rr = sqrtf(ped_r2), point_rr = sqrtf(point_r2);
    const unsigned per_pass = (unsigned)(BLOCK / split);
#pragma unroll 1
    for (unsigned c0 = 0; c0 < total; c0 += per_pass) {                // uniform
        const unsigned first = c0 + (unsigned)(group * WAVE);
        const bool wave_has = first < total;                           // uniform per wave
        const unsigned item = first + (unsigned)lane;
        const bool there = item < total;
        const unsigned it = there ? item : total - 1;                  // (a lane without an item repeats the last: every lane votes)
        const unsigned pos = it / (unsigned)R;
        const int ray = (int)(it - pos * (unsigned)R);
        const int row = sh.rows[pos];
        const float4 s = sh.pk[row];
        const float x = s.x, y = s.y;
        const float2 u0 = sh.dir[ray];
        float ux = u0.x, uy = u0.y;
        if (a.frame) {                                                 // uniform: the ray in the row's heading frame (observe_store's rule)
            const float vx = s.z, vy = s.w;
            const float4 o = a.own[s0 + row];
            const float gx = o.x - x, gy = o.y - y;
            const float vv = fmaf(vx, vx, vy * vy), gg = fmaf(gx, gx, gy * gy);
            float hx = 1.0f, hy = 0.0f;
            if (vv > 0.0f) { const float l = sqrtf(vv); hx = vx / l; hy = vy / l; }
            else if (gg > 0.0f) { const float l = sqrtf(gg); hx = gx / l; hy = gy / l; }
            ux = fmaf(hx, u0.x, -(hy * u0.y));
            uy = fmaf(hy, u0.x, hx * u0.y);
        }
        float best = Rmax, bkind = 0.0f;                               // a range >= Rmax is never stored, so it is never taken
        if (wave_has && ped_r2 > 0.0f) {
            int j = j0;
#pragma unroll 1
            for (; j + 4 <= j1; j += 4) {                              // uniform: the LDS reads are broadcasts, four in flight
                const float4 p0 = sh.pk[j], p1 = sh.pk[j + 1], p2 = sh.pk[j + 2], p3 = sh.pk[j + 3];
                scan_disc(p0.x - x, p0.y - y, ux, uy, ped_r2, ped_rr, j != row, 1.0f, best, bkind);
                scan_disc(p1.x - x, p1.y - y, ux, uy, ped_r2, ped_rr, j + 1 != row, 1.0f, best, bkind);
                scan_disc(p2.x - x, p2.y - y, ux, uy, ped_r2, ped_rr, j + 2 != row, 1.0f, best, bkind);
                scan_disc(p3.x - x, p3.y - y, ux, uy, ped_r2, ped_rr, j + 3 != row, 1.0f, best, bkind);
            }
#pragma unroll 1
            for (; j < j1; ++j) {
                const float4 pj = sh.pk[j];
                scan_disc(pj.x - x, pj.y - y, ux, uy, ped_r2, ped_rr, j != row, 1.0f, best, bkind);
            }
        }
#pragma unroll 1
        for (int g0 = 0; g0 < G; g0 += SCAN_TILE) {                    // uniform
            const int cnt = min(SCAN_TILE, G - g0);
            if (!one_tile) {
                __syncthreads();                                       // everyone is done with the tile before
                stage(g0, cnt);
                __syncthreads();
            }
            if (!wave_has) continue;
            // the tile's share of each kind, in order, cut to this wave's part [w0, w1) of the run
            const int lo = min(max(w0 - g0, 0), cnt), hi = min(max(w1 - g0, 0), cnt);
            const int e1 = min(max(nb - g0, lo), hi), e2 = min(max(nb + ns - g0, lo), hi);
            scan_points(sh.tile, lo, e1, x, y, ux, uy, point_r2, point_rr, 2.0f, best, bkind);
            scan_points(sh.tile, e1, e2, x, y, ux, uy, point_r2, point_rr, 3.0f, best, bkind);
            scan_points(sh.tile, e2, hi, x, y, ux, uy, point_r2, point_rr, 4.0f, best, bkind);
        }
        if (split > 1) {                                               // uniform: the shares of an item, combined in order
            sh.part[wave][lane] = make_float2(best, bkind);
            __syncthreads();
            if (sub == 0) {
#pragma unroll
                for (int k = 1; k < WAVES_PER_BLOCK; ++k) {
                    if (k >= split) break;                             // uniform
                    const float2 o = sh.part[wave + k][lane];
                    const bool take = o.x < best;
                    best = take ? o.x : best;
                    bkind = take ? o.y : bkind;
                }
            }
            __syncthreads();                                           // (the next pass rewrites part: split > 1 has one pass only)
        }
        if (there && sub == 0) {
            float* out = a.out + (size_t)(s0 + row) * (size_t)(2 * R);
            out[ray] = best;
            out[R + ray] = bkind;
        }
    }
}

hipError_t launch_batch_scan(const ScanArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_scan_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
