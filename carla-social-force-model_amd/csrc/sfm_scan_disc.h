// sfm_scan_disc.h -- one disc against one ray, and a run of LDS points against a lane's ray: what the two range-scan kernels share
// (sfm_batch_scan.hip casts from pedestrian rows, sfm_batch_vehicle_scan.hip from vehicles; the rules are specified in
// include/sfm_hip.h).  Both kernels keep their register, LDS and occupancy figures with the helpers here (csrc/resource_usage.txt).
#pragma once
#include "sfm_device.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

// one disc against one ray: the rules of include/sfm_hip.h, operation by operation.  `best` starts at Rmax (see the kernels), rr is
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

// the points [lo, hi) of the LDS tile against the lane's ray, in order; four loads are in flight before the first is used
__device__ __forceinline__ void scan_points(const float2* tile, int lo, int hi, float x, float y, float ux, float uy, float r2, float rr,
                                            float kind, float& best, float& bkind) {
    int e = lo;
#pragma unroll 1
    for (; e + 4 <= hi; e += 4) {                                      // uniform: the LDS reads are broadcasts
        const float2 p0 = tile[e], p1 = tile[e + 1], p2 = tile[e + 2], p3 = tile[e + 3];
        scan_disc(p0.x - x, p0.y - y, ux, uy, r2, rr, true, kind, best, bkind);
        scan_disc(p1.x - x, p1.y - y, ux, uy, r2, rr, true, kind, best, bkind);
        scan_disc(p2.x - x, p2.y - y, ux, uy, r2, rr, true, kind, best, bkind);
        scan_disc(p3.x - x, p3.y - y, ux, uy, r2, rr, true, kind, best, bkind);
    }
#pragma unroll 1
    for (; e < hi; ++e) {
        const float2 p = tile[e];
        scan_disc(p.x - x, p.y - y, ux, uy, r2, rr, true, kind, best, bkind);
    }
}

}  // namespace sfm
