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
//   3. the cast (scan_cast, sfm_scan_disc.h): a lane owns a (vehicle, ray) pair, the ray index fastest: item = list position * R +
//      ray, 256 items per pass.  The lane forms its ray (frame 1: rotated by the STORED heading) and walks the candidates in the
//      record's fixed order -- every pedestrian j ascending as broadcast LDS reads, then the scene's border, static and vehicle points, staged cooperatively in LDS tiles of
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
#include "sfm_scan_disc.h"     // scan_disc, scan_points, scan_cast: shared by the two scan kernels

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int VSCAN_TILE = 512;    // geometry points per LDS tile

struct VehicleScanShared {
    ScanShared<VSCAN_TILE, VEHICLE_SCAN_MAX_RAYS> c;
    float4 org[BLOCK];                                                 // the listed vehicles, ascending: {ox, oy, hx, hy} ...
    int4 who[BLOCK];                                                   // ... and {vehicle, own ring [lo, hi) in the virtual run, 0}
};

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
    for (int t = tid; t < n; t += BLOCK) sh.c.pk[t] = a.pk[s0 + t];
    if (tid < R) sh.c.dir[tid] = a.dir[tid];

    const BatchScanScene set = a.set[b];
    const SceneRun run(a.geo, b);
    const int G = set.point_r2 > 0.0f ? run.total() : 0;               // the virtual run, walked only while points can be hit
    if (G <= VSCAN_TILE) run.stage(sh.c.tile, 0, G);                   // the whole scene's geometry fits: staged once
    __syncthreads();

    const int ring0 = run.nb + run.ns - run.vp0;                       // vehicle k's ring in the run: ring0 + off[k] .. ring0 + off[k + 1]
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
                who = make_int4(k, ring0 + a.geo[2].off[k], ring0 + a.geo[2].off[k + 1], 0);
                scan = true;
            } else {                                                   // absent (or not finite): the whole record is zeros
                float* out = a.out + (size_t)k * (size_t)(2 * R);
                for (int q = 0; q < 2 * R; ++q) out[q] = 0.0f;
            }
        }
        // (behind the compaction's first barrier every wave is done with the chunk before: org, who, part)
        const int n_scan = block_compact(scan, sh.c.wcount, lane, wave, 0, [&](int p) {
            sh.org[p] = org;
            sh.who[p] = who;
        });
        if (n_scan == 0) continue;                                     // uniform

        // 3. an item is a listed vehicle: the rays start at its sensor and turn by its stored heading; every pedestrian is a
        // candidate, the points of its own ring are not
        scan_cast(sh.c, run, n, G, set, R, a.frame, a.out, n_scan, [&](unsigned pos) {
            const float4 o = sh.org[pos];
            const int4 me = sh.who[pos];
            return ScanItem{o.x, o.y, o.z, o.w, 0, 0u, me.y, (unsigned)(me.z - me.y), me.x};
        });
    }
}

hipError_t launch_batch_vehicle_scan(const VehicleScanArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_scan_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
