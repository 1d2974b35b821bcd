// sfm_batch_vehicle_grid.hip -- bird's-eye grids around the vehicles of batched scenes for gfx950 (MI355X): ONE launch for the whole
// batch (sfm_batch_grid_vehicles; the record and its rules are specified in include/sfm_hip.h).
//
// What a driving policy sees per vehicle: a GU x GV raster whose middle lies at `centre` in the vehicle frame -- per cell the number
// of live pedestrians and the sum of their velocities relative to the vehicle, the number of sampled border and static-obstacle
// points, and the number of ring points of the scene's OTHER vehicles with the sum of their owners' relative velocities.  The
// vehicle's own ring is left out.  Computed from the buffers the next tick reads (state, the scene offsets, the three geometry CSRs,
// the headings) into a device buffer [M'][8][GV][GU] of floats, one compact slot per gridded vehicle.  The kernel writes nothing
// else, so a tick before or after it computes what it computed without it.
//
// Shape (workgroup b, 4 waves), sfm_batch_grid_kernel's with vehicles in place of rows:
//   1. a scene without vehicles leaves at once; else the scene's {x, y, vx, vy} (possibly none: the geometry is still gridded) is
//      staged in LDS and the geometry counts are cleared; when the scene's geometry fits one tile of VGRID_TILE points it is staged
//      once, else every vehicle reads it from memory (a point is used once per vehicle, by one lane);
//   2. the scene's vehicles are walked in ascending order by the whole workgroup (the loop is uniform: mask and presence are the
//      same for every lane).  A vehicle without a slot is passed over; a gridded vehicle that is not present gets its zeros;
//   3. per gridded present vehicle: the window is GU x GV cells around `centre`, turned by the stored heading (GridWindow,
//      sfm_grid_cells.h: the rotation and the cell rule live there);
//      (a) the live pedestrians are offered to the shared loop (GRID_OFFER): lane t takes pedestrians t, t + BLOCK, .., the sources
//          inside the window are compacted in ascending j into an LDS list {cell, relative velocity} of VGRID_LIST entries, which is
//          walked in order whenever VGRID_LIST rows have been offered and at the end, into the cells tid, tid + BLOCK, .. the lane
//          owns (GU GV <= 1024: up to 4; GRID_WALK and GRID_ADD, with the order and the wave test described there);
//      (b) every lane takes border and static points e, e + BLOCK, .. and counts the cell of each with an integer LDS add (order
//          does not matter);
//      (c) the ring points of the OTHER vehicles go through the same loop in ascending (vehicle, point) order, into a second set of
//          accumulators -- the own ring is skipped by its index range in the geometry's virtual run; the lane that holds a point
//          inside the window finds the owning vehicle by bisection of the ring offsets; the list now holds {cell, the owner's
//          relative velocity}, and the order holds at any number of points;
//   4. the lane stores the 8 channels of its cells (consecutive lanes store consecutive floats) and clears the counts it read.
// What is this kernel's own: the walk over the scene's vehicles with its barrier, the list's size, what a source is (every live
// pedestrian; every ring point but the own ring's, with its owner's velocity), and the store with its two sets of sums.
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no float atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or
// anywhere in any batch.
#include "sfm_grid_cells.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int VGRID_TILE = 1024;   // geometry points the LDS tile holds
constexpr int VGRID_LIST = 512;    // list entries: one chunk of pedestrians or of ring points
static_assert(VGRID_LIST % BLOCK == 0, "a chunk is whole passes of the workgroup");

struct VehicleGridShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    float2 tile[VGRID_TILE];                                           // the scene's geometry points, when they fit
    float2 rv[VGRID_LIST];                                             // the sources inside the window, in order: relative velocity ...
    unsigned short cid[VGRID_LIST];                                    // ... and cell
    int cnt[2][VEHICLE_GRID_MAX_CELLS];                                // border and static points per cell
    int wcount[WAVES_PER_BLOCK];
};
static_assert(sizeof(VehicleGridShared) <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");
static_assert(sizeof(VehicleGridShared) <= 40 * 1024, "... and four do: 1 024 scenes are resident on 256 CUs at once");

__global__ __launch_bounds__(BLOCK) void sfm_batch_vehicle_grid_kernel(const VehicleGridArgs a) {
    __shared__ VehicleGridShared sh;
    const int b = blockIdx.x;
    const int vk0 = a.geo[2].item_off[b], vk1 = a.geo[2].item_off[b + 1];
    if (vk1 <= vk0) return;                                            // uniform: a scene without vehicles, before any barrier
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host); 0 is gridded too
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int GU = a.GU, GV = a.GV, cells = GU * GV;                   // cells <= VEHICLE_GRID_MAX_CELLS (checked on the host)
    for (int t = tid; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    for (int q = tid; q < 2 * VEHICLE_GRID_MAX_CELLS; q += BLOCK) (&sh.cnt[0][0])[q] = 0;

    const SceneRun run(a.geo, b);
    const int nb = run.nb, nbs = run.nb + run.ns, P = run.total();     // virtual index e: borders, static, vehicles
    const bool one_tile = P <= VGRID_TILE;
    if (one_tile) run.stage(sh.tile, 0, P);                            // the whole scene's geometry fits: staged once
    __syncthreads();

    const int ring0 = nbs - run.vp0;                                   // vehicle v's ring in the run: ring0 + off[v] .. ring0 + off[v + 1]
    const int* __restrict__ voff = a.geo[2].off;
    GridWindow w(a.cell[b], GU, GV, a.frame != 0);                     // (rot: uniform)
    const float mx = a.centre_x, my = a.centre_y;
    const size_t per_slot = (size_t)VEHICLE_GRID_CHANNELS * (size_t)cells;
#pragma unroll 1
    for (int k = vk0; k < vk1; ++k) {                                  // uniform
        const int slot = a.slot ? a.slot[k] : k;
        if (slot < 0) continue;                                        // not gridded: never touched (the buffer was zero-filled)
        float* out = a.out + (size_t)slot * per_slot;
        const float4 ck = a.geo[2].ctr[k];                             // {cx, cy, vx, vy}
        if (!row_live(ck.x, ck.y)) {                                   // uniform: absent (or not finite) -- the whole record is zeros
            for (int q = tid; q < (int)per_slot; q += BLOCK) out[q] = 0.0f;
            continue;
        }
        const float2 h = a.rot[k];
        {
            const float rx = fmaf(h.x, mx, -(h.y * my));               // the centre, turned by the stored heading
            const float ry = fmaf(h.y, mx, h.x * my);
            w.ox = ck.x + rx;
            w.oy = ck.y + ry;
            w.hx = h.x;
            w.hy = h.y;
        }
        const float vxk = ck.z, vyk = ck.w;
        const int own_lo = ring0 + voff[k], own_hi = ring0 + voff[k + 1];
        __syncthreads();                                               // the counts the vehicle before read are cleared, its list is done with

        // a lane owns cells tid + q BLOCK and walks a list in order
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f, y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
        int d0 = 0, d1 = 0, d2 = 0, d3 = 0;
        float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f, u3 = 0.0f, z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;

        // (a), (b) the live pedestrians inside the window, ascending, with their cells and relative velocities
        auto walker = [&](int t, int& cell, float& rx, float& ry) {
            const float4 p = sh.pk[t];
            if (!row_live(p.x, p.y)) return;
            cell = w.cell(p.x, p.y);
            rx = p.z - vxk;
            ry = p.w - vyk;
            w.rotate(rx, ry);
        };
        GRID_OFFER(VGRID_LIST, 0, n, walker, c, x, y);
        // ... and the border and static points per cell
        for (int e = tid; e < nbs; e += BLOCK) {
            const float2 p = one_tile ? sh.tile[e] : run.point(e);
            const int cell = w.cell(p.x, p.y);
            if (cell >= 0) atomicAdd(&sh.cnt[e < nb ? 0 : 1][cell], 1);
        }
        __syncthreads();

        // (c) the ring points of the other vehicles, ascending (vehicle, point), each with its owner's relative velocity
        auto ring = [&](int e, int& cell, float& rx, float& ry) {
            if (e >= own_lo && e < own_hi) return;
            const float2 p = one_tile ? sh.tile[e] : run.point(e);
            cell = w.cell(p.x, p.y);
            if (cell < 0) return;
            const int pidx = e - ring0;                                // the point's index in the rings' array
            int lo = vk0, hi = vk1 - 1;                                // the owner: the last vehicle whose ring begins at or before it
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (voff[mid] <= pidx) lo = mid; else hi = mid - 1;
            }
            const float4 cv = a.geo[2].ctr[lo];
            rx = cv.z - vxk;
            ry = cv.w - vyk;
            w.rotate(rx, ry);
        };
        GRID_OFFER(VGRID_LIST, nbs, P, ring, d, u, z);

        // 4. the vehicle's 8 GU GV floats
        auto store = [&](int cell, int peds, float sx, float sy, int pts, float tx, float ty) {
            if (cell >= cells) return;
            out[cell] = (float)peds;
            out[cells + cell] = sx;
            out[2 * cells + cell] = sy;
#pragma unroll
            for (int kind = 0; kind < 2; ++kind) {
                const int g = sh.cnt[kind][cell];
                out[(3 + kind) * cells + cell] = (float)g;
                if (g) sh.cnt[kind][cell] = 0;                         // (only this lane reads or clears the cell)
            }
            out[5 * cells + cell] = (float)pts;
            out[6 * cells + cell] = tx;
            out[7 * cells + cell] = ty;
        };
        store(tid, c0, x0, y0, d0, u0, z0);
        store(tid + BLOCK, c1, x1, y1, d1, u1, z1);
        store(tid + 2 * BLOCK, c2, x2, y2, d2, u2, z2);
        store(tid + 3 * BLOCK, c3, x3, y3, d3, u3, z3);
    }
}

hipError_t launch_batch_vehicle_grid(const VehicleGridArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_vehicle_grid_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
