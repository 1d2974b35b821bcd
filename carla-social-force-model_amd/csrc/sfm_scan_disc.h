// sfm_scan_disc.h -- what the two range-scan kernels share: one disc against one ray, a run of LDS points against a lane's ray, and
// the cast of a list of items (sfm_batch_scan.hip casts from pedestrian rows, sfm_batch_vehicle_scan.hip from vehicles; the rules are
// specified in include/sfm_hip.h).  Each kernel keeps its front half -- staging, the list of what is scanned, the zero fills -- and
// says what an item is.  Both keep their LDS and occupancy figures with the pieces here (csrc/resource_usage.txt).
#pragma once
#include "sfm_device.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

// one disc against one ray: the rules of include/sfm_hip.h, operation by operation.  `best` starts at Rmax (see scan_cast), rr is
// the correctly rounded sqrt(r2), `ok` false keeps the lane out.  The square root is skipped while no lane of the wave can take the
// disc, exactly: q <= r2 gives w <= rr (both roundings are monotone), so a candidate (t + w > 0) has t > -rr, and its range
// max(t - w, 0) >= t - rr, rounded or not, cannot be taken under strict `<` once t - rr >= best.
__device__ __forceinline__ void scan_disc(float ax, float ay, float ux, float uy, float r2, float rr, bool ok, float kind, float& best,
                                          float& bkind) {
    const float t = fmaf(ax, ux, ay * uy);
    const float c = fmaf(ax, uy, -(ay * ux));
    const float q = fmaf(-c, c, r2);
    const bool may = ok && q > 0.0f && (t - rr) < best && t > -rr;     // (NaN and +inf positions fail here by themselves)
    if (!__any(may)) return;
    const float w = sqrtf(q);                                          // correctly rounded (hipcc's default for fp32 sqrt and divide;
                                                                       // __fsqrt_rn is the native, 1-ulp instruction in this toolchain)
    const bool cand = may && (t + w) > 0.0f;
    const float s = t - w;
    const float range = s > 0.0f ? s : 0.0f;                           // inside the disc: 0
    const bool take = cand && range < best;
    best = take ? range : best;
    bkind = take ? kind : bkind;
}

// the points [lo, hi) of an LDS array (float2 tile points, or the float4 rows) against the lane's ray, in order; four loads are in
// flight before the first is used.  Entries [own, own + len) are no candidates of this lane: one unsigned compare per point (own may
// be negative or past hi), and none at all where len is 0 at compile time.
template <class P>
__device__ __forceinline__ void scan_points(const P* pts, int lo, int hi, int own, unsigned len, float x, float y, float ux, float uy,
                                            float r2, float rr, float kind, float& best, float& bkind) {
    int e = lo;
#pragma unroll 1
    for (; e + 4 <= hi; e += 4) {                                      // uniform: the LDS reads are broadcasts
        const P p0 = pts[e], p1 = pts[e + 1], p2 = pts[e + 2], p3 = pts[e + 3];
        scan_disc(p0.x - x, p0.y - y, ux, uy, r2, rr, (unsigned)(e - own) >= len, kind, best, bkind);
        scan_disc(p1.x - x, p1.y - y, ux, uy, r2, rr, (unsigned)(e + 1 - own) >= len, kind, best, bkind);
        scan_disc(p2.x - x, p2.y - y, ux, uy, r2, rr, (unsigned)(e + 2 - own) >= len, kind, best, bkind);
        scan_disc(p3.x - x, p3.y - y, ux, uy, r2, rr, (unsigned)(e + 3 - own) >= len, kind, best, bkind);
    }
#pragma unroll 1
    for (; e < hi; ++e) {
        const P p = pts[e];
        scan_disc(p.x - x, p.y - y, ux, uy, r2, rr, (unsigned)(e - own) >= len, kind, best, bkind);
    }
}

// The LDS both kernels' casts work in; each kernel's own list of items stands beside it.
template <int TILE, int RAYS>
struct ScanShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    float2 tile[TILE];                                                 // geometry points of the current tile
    float2 dir[RAYS];                                                  // the ray directions
    int wcount[WAVES_PER_BLOCK];
    float2 part[WAVES_PER_BLOCK][WAVE];                                // few items: the (range, kind) each wave found in its share
};

// What a kernel says of one item of its list: where its rays start, what turns them in frame 1, what is no candidate, where they go.
struct ScanItem {
    float x, y;                                                        // the origin
    float hx, hy;                                                      // frame 1: the heading (not read in frame 0)
    int self;                                                          // the n_self pedestrians from `self` on are no candidates
    unsigned n_self;                                                   //   (a row: itself; 0: every pedestrian is one)
    int ring;                                                          // the n_ring points from `ring` on of the virtual run likewise
    unsigned n_ring;                                                   //   (a vehicle: its own ring; 0: every point is a candidate)
    int rec;                                                           // the item's row of `out`
};

// The cast: n_list items of R rays each, item = list position * R + ray, 256 items per pass; item(pos) is the ScanItem of a list
// position.  The lane forms its ray (frame 1: turned by the item's heading) and walks the candidates in the record's fixed order --
// the n pedestrians of sh.pk ascending, then the G points of the virtual run in LDS tiles of TILE points, cut by kind -- keeping the
// first minimum under strict `<`, and stores its range and kind; consecutive lanes store consecutive floats.  G <= TILE: the caller
// has staged the run in sh.tile; else every pass stages tile by tile.
// Few items: `split` waves share an item's candidates -- each walks one contiguous share of the fixed order and the shares' results
// are combined in that order under strict `<`: the first minimum of the whole, however the order is cut.  An excluded range may lie
// in one share or across two: the skip is by index, whoever walks the point.
// Skips, all exact: a kind whose r2 is 0 is not walked (q = -c^2 <= 0 is never a candidate; the caller passes G = 0 then); a range
// >= Rmax is never taken (it is never stored); scan_disc's square root.
// Every lane of the workgroup must call it (barriers), with uniform arguments.
template <int TILE, int RAYS, class Item>
__device__ __forceinline__ void scan_cast(ScanShared<TILE, RAYS>& sh, const SceneRun& run, int n, int G, const BatchScanScene& set, int R,
                                          int frame, float* out, int n_list, Item&& item) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float Rmax = set.max_range, ped_r2 = set.ped_r2, point_r2 = set.point_r2;
    const float ped_rr = sqrtf(ped_r2), point_rr = sqrtf(point_r2);
    const bool one_tile = G <= TILE;
    const unsigned total = (unsigned)n_list * (unsigned)R;
    const int split = total <= WAVE ? 4 : total <= 2 * WAVE ? 2 : 1;   // uniform
    const int sub = wave % split, group = wave / split;
    const int T = n + G;                                               // candidates in the fixed order (the excluded ones included)
    const int v0 = (int)((long long)T * sub / split), v1 = (int)((long long)T * (sub + 1) / split);
    const int j0 = min(v0, n), j1 = min(v1, n);                         // this wave's pedestrians ...
    const int w0 = max(v0 - n, 0), w1 = max(v1 - n, 0);                 // ... and its part of the virtual run
    const unsigned per_pass = (unsigned)(BLOCK / split);
#pragma unroll 1
    for (unsigned c0 = 0; c0 < total; c0 += per_pass) {                // uniform
        const unsigned first = c0 + (unsigned)(group * WAVE);
        const bool wave_has = first < total;                           // uniform per wave
        const unsigned at = first + (unsigned)lane;
        const bool there = at < total;
        const unsigned it = there ? at : total - 1;                    // (a lane without an item repeats the last: every lane votes)
        const unsigned pos = it / (unsigned)R;
        const int ray = (int)(it - pos * (unsigned)R);
        const ScanItem me = item(pos);
        const float x = me.x, y = me.y;
        const float2 u0 = sh.dir[ray];
        float ux = u0.x, uy = u0.y;
        if (frame) {                                                   // uniform: the ray in the item's heading frame
            ux = fmaf(me.hx, u0.x, -(me.hy * u0.y));
            uy = fmaf(me.hy, u0.x, me.hx * u0.y);
        }
        float best = Rmax, bkind = 0.0f;                               // a range >= Rmax is never stored, so it is never taken
        if (wave_has && ped_r2 > 0.0f) scan_points(sh.pk, j0, j1, me.self, me.n_self, x, y, ux, uy, ped_r2, ped_rr, 1.0f, best, bkind);
#pragma unroll 1
        for (int g0 = 0; g0 < G; g0 += TILE) {                         // uniform
            const int cnt = min(TILE, G - g0);
            if (!one_tile) {
                __syncthreads();                                       // everyone is done with the tile before
                run.stage(sh.tile, g0, cnt);
                __syncthreads();
            }
            if (!wave_has) continue;
            // the tile's share of each kind, in order, cut to this wave's part [w0, w1) of the run
            const int lo = min(max(w0 - g0, 0), cnt), hi = min(max(w1 - g0, 0), cnt);
            const int e1 = min(max(run.nb - g0, lo), hi), e2 = min(max(run.nb + run.ns - g0, lo), hi);
            scan_points(sh.tile, lo, e1, 0, 0u, x, y, ux, uy, point_r2, point_rr, 2.0f, best, bkind);
            scan_points(sh.tile, e1, e2, 0, 0u, x, y, ux, uy, point_r2, point_rr, 3.0f, best, bkind);
            scan_points(sh.tile, e2, hi, me.ring - g0, me.n_ring, x, y, ux, uy, point_r2, point_rr, 4.0f, best, bkind);
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
            float* rec = out + (size_t)me.rec * (size_t)(2 * R);
            rec[ray] = best;
            rec[R + ray] = bkind;
        }
    }
}

}  // namespace sfm
