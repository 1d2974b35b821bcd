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
//   3. the cast (scan_cast, sfm_scan_disc.h): a lane owns a (row, ray) pair, the ray index fastest: item = list position * R + ray,
//      256 items per pass.  The lane forms its ray (frame 1: rotated by the row's heading) and walks the candidates in the
//      record's fixed order -- pedestrians j ascending as broadcast LDS reads, then the scene's border, static and vehicle points, staged cooperatively in LDS tiles of SCAN_TILE
//      points and read as broadcasts -- keeping the first minimum under strict `<`.  The scene's points of one kind are one
//      contiguous run of the kind's CSR (polylines in order, points in order), so the walk needs no polyline structure;
//      With at most 64 (128) items -- an RL loop's one agent row per scene -- 4 (2) waves share each item's candidates, a contiguous
//      share of the fixed order each, and the shares are combined in that order through LDS under strict `<`;
//   4. the lane stores its range and kind; consecutive lanes store consecutive floats.
// Skips, all exact: a kind whose r2 is 0 is not walked (q = -c^2 <= 0 is never a candidate); a range >= Rmax is never taken (it is
// never stored); the square root and what follows it are skipped while no lane of the wave can take the disc (scan_disc).  The row
// itself is left out by its index among the pedestrians.
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or anywhere in
// any batch.
#include "sfm_device.h"
#include "sfm_scan_disc.h"     // scan_disc, scan_points, scan_cast: shared by the two scan kernels

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int SCAN_TILE = 512;     // geometry points per LDS tile

struct RowScanShared {
    ScanShared<SCAN_TILE, SCAN_MAX_RAYS> c;
    unsigned short rows[BATCH_MAX_N];                                  // the scanned live rows, ascending
};

__global__ __launch_bounds__(BLOCK) void sfm_batch_scan_kernel(const ScanArgs a) {
    __shared__ RowScanShared sh;
    const int b = blockIdx.x;
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    if (n <= 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R;                                                 // 1 .. SCAN_MAX_RAYS
    for (int t = tid; t < n; t += BLOCK) sh.c.pk[t] = a.pk[s0 + t];
    if (tid < R) sh.c.dir[tid] = a.dir[tid];
    __syncthreads();

    // 2. the scanned live rows, ascending
    int n_scan = 0;
#pragma unroll 1
    for (int base = 0; base < n; base += BLOCK) {                      // uniform
        const int t = base + tid;
        bool scan = false;
        if (t < n) {
            const float4 s = sh.c.pk[t];
            const bool want = !a.mask || a.mask[s0 + t] != 0;
            const bool live = row_live(s.x, s.y);
            scan = want && live;
            if (want && !live) {
                float* out = a.out + (size_t)(s0 + t) * (size_t)(2 * R);
                for (int q = 0; q < 2 * R; ++q) out[q] = 0.0f;
            }
        }
        n_scan += block_compact(scan, sh.c.wcount, lane, wave, n_scan, [&](int p) { sh.rows[p] = (unsigned short)t; });
    }
    if (n_scan == 0) return;                                           // uniform

    const BatchScanScene set = a.set[b];
    const SceneRun run(a.geo, b);
    const int G = set.point_r2 > 0.0f ? run.total() : 0;               // the virtual run, walked only while points can be hit
    if (G <= SCAN_TILE && G > 0) {                                     // the whole scene's geometry fits: staged once
        run.stage(sh.c.tile, 0, G);
        __syncthreads();
    }

    // 3. an item is a listed row: the rays start at the row and turn by its heading; the row is no candidate of its own rays
    scan_cast(sh.c, run, n, G, set, R, a.frame, a.out, n_scan, [&](unsigned pos) {
        const int row = sh.rows[pos];
        const float4 s = sh.c.pk[row];
        float2 h = make_float2(1.0f, 0.0f);
        if (a.frame) {                                                 // uniform
            const float4 o = a.own[s0 + row];
            h = row_heading(s.z, s.w, o.x - s.x, o.y - s.y);
        }
        return ScanItem{s.x, s.y, h.x, h.y, row, 1u, 0, 0u, s0 + row};
    });
}

hipError_t launch_batch_scan(const ScanArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_scan_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
