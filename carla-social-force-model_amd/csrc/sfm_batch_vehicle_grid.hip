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
//   3. per gridded present vehicle:
//      (a) lane t takes pedestrians t, t + BLOCK, ..: the cell of each and its relative velocity; the sources inside the window are
//          compacted, by ballots and so in ascending j, into an LDS list {cell, relative velocity}, which is walked as in (b)
//          whenever VGRID_LIST rows have been offered and at the end; every lane takes border and static points e, e + BLOCK, ..
//          and counts the cell of each with an integer LDS add (order does not matter);
//      (b) a lane owns the cells tid, tid + BLOCK, .. (GU GV <= 1024: up to 4) and walks the list in order -- broadcast LDS reads --
//          counting its matches and adding their velocities: ascending j, fp32 adds from 0.0f, no float atomic.  An entry's cell
//          is uniform, so the three waves that do not hold its owning lane pass over it on a scalar test;
//      (c) the ring points of the OTHER vehicles, BLOCK at a time in ascending (vehicle, point) order -- the own ring is skipped by
//          its index range in the geometry's virtual run; the lane that holds a point inside the window finds the owning vehicle
//          by bisection of the ring offsets -- are compacted into the same list, now {cell, the owner's relative velocity}.  The
//          list is walked as in (b), into a second set of accumulators, whenever VGRID_LIST points have been offered and at the
//          end: the order holds at any number of points;
//   4. the lane stores the 8 channels of its cells (consecutive lanes store consecutive floats) and clears the counts it read.
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no float atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or
// anywhere in any batch.
//
// The cell rule, the rotation and the accumulation macro are sfm_batch_grid.hip's, restated here for a window of two sides: that
// kernel keeps its own copies, so its code and registers are what they were.
#include "sfm_device.h"

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

// the rotation into the heading frame: the rules of include/sfm_hip.h
__device__ __forceinline__ void vgrid_rotate(bool rot, float hx, float hy, float& a, float& b) {
    if (rot) {
        const float ra = fmaf(hx, a, hy * b), rb = fmaf(hx, b, -(hy * a));
        a = ra;
        b = rb;
    }
}

// the window of one vehicle
struct VehicleGridWindow {
    float ox, oy, hx, hy;      // the window's middle in world axes; the stored heading
    float c, halfu, halfv, gu, gv;
    int GU;
    bool rot;
    // the cell [cv][cu] of a source at (px, py), as cv * GU + cu; -1: outside (NaN and +-inf fail the compares)
    __device__ __forceinline__ int cell(float px, float py) const {
        float ax = px - ox, ay = py - oy;
        vgrid_rotate(rot, hx, hy, ax, ay);
        const float pu = ax / c + halfu;                               // the division is rounded first (correctly: hipcc's default
        const float pv = ay / c + halfv;                               // for fp32 divide), then the sum
        const bool in = pu >= 0.0f && pu < gu && pv >= 0.0f && pv < gv;
        return in ? (int)pv * GU + (int)pu : -1;
    }
};

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
    VehicleGridWindow w;
    w.c = a.cell[b];
    w.gu = (float)GU;                                                  // (exact, and so are the halves)
    w.gv = (float)GV;
    w.halfu = 0.5f * w.gu;
    w.halfv = 0.5f * w.gv;
    w.GU = GU;
    w.rot = a.frame != 0;                                              // uniform
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
        // one source, in its turn (a macro: the accumulators stay plain registers)
#define VGRID_ADD(cell, v, C, X, Y)                                                                                            \
        do {                                                                                                                   \
            const int cid_ = __builtin_amdgcn_readfirstlane(cell);                                                             \
            if (((cid_ / WAVE) & (WAVES_PER_BLOCK - 1)) != wave) break; /* uniform: the owning lane sits in another wave */     \
            const bool mine_ = (cid_ & (BLOCK - 1)) == tid;                                                                    \
            const int q_ = cid_ / BLOCK; /* uniform */                                                                         \
            if (q_ == 0) { C##0 += mine_; X##0 = mine_ ? X##0 + (v).x : X##0; Y##0 = mine_ ? Y##0 + (v).y : Y##0; }            \
            else if (q_ == 1) { C##1 += mine_; X##1 = mine_ ? X##1 + (v).x : X##1; Y##1 = mine_ ? Y##1 + (v).y : Y##1; }       \
            else if (q_ == 2) { C##2 += mine_; X##2 = mine_ ? X##2 + (v).x : X##2; Y##2 = mine_ ? Y##2 + (v).y : Y##2; }       \
            else { C##3 += mine_; X##3 = mine_ ? X##3 + (v).x : X##3; Y##3 = mine_ ? Y##3 + (v).y : Y##3; }                    \
        } while (0)
#define VGRID_WALK(count, C, X, Y)                                                                                             \
        do {                                                                                                                   \
            int k_ = 0;                                                                                                        \
            _Pragma("unroll 1")                                                                                                \
            for (; k_ + 4 <= (count); k_ += 4) { /* uniform: the LDS reads are broadcasts, four in flight */                   \
                const int e0 = sh.cid[k_], e1 = sh.cid[k_ + 1], e2 = sh.cid[k_ + 2], e3 = sh.cid[k_ + 3];                      \
                const float2 v0 = sh.rv[k_], v1 = sh.rv[k_ + 1], v2 = sh.rv[k_ + 2], v3 = sh.rv[k_ + 3];                       \
                VGRID_ADD(e0, v0, C, X, Y);                                                                                    \
                VGRID_ADD(e1, v1, C, X, Y);                                                                                    \
                VGRID_ADD(e2, v2, C, X, Y);                                                                                    \
                VGRID_ADD(e3, v3, C, X, Y);                                                                                    \
            }                                                                                                                  \
            _Pragma("unroll 1")                                                                                                \
            for (; k_ < (count); ++k_) {                                                                                       \
                const int e_ = sh.cid[k_];                                                                                     \
                const float2 v_ = sh.rv[k_];                                                                                   \
                VGRID_ADD(e_, v_, C, X, Y);                                                                                    \
            }                                                                                                                  \
        } while (0)

        // (a), (b) the pedestrians inside the window, ascending, with their cells and relative velocities: offered BLOCK at a time,
        // walked per chunk
        int n_src = 0, offered = 0;
#pragma unroll 1
        for (int base = 0; base < n; base += BLOCK) {                  // uniform
            const int t = base + tid;
            int cell = -1;
            float rx = 0.0f, ry = 0.0f;
            if (t < n) {
                const float4 p = sh.pk[t];
                if (row_live(p.x, p.y)) {
                    cell = w.cell(p.x, p.y);
                    rx = p.z - vxk;
                    ry = p.w - vyk;
                    vgrid_rotate(w.rot, w.hx, w.hy, rx, ry);
                }
            }
            n_src += block_compact(cell >= 0, sh.wcount, lane, wave, n_src, [&](int p) {
                sh.cid[p] = (unsigned short)cell;
                sh.rv[p] = make_float2(rx, ry);
            });
            offered += BLOCK;
            if (offered == VGRID_LIST || base + BLOCK >= n) {          // uniform: the chunk is full, or the rows are over
                VGRID_WALK(n_src, c, x, y);
                n_src = 0;
                offered = 0;
            }
        }
        // ... and the border and static points per cell
        for (int e = tid; e < nbs; e += BLOCK) {
            const float2 p = one_tile ? sh.tile[e] : run.point(e);
            const int cell = w.cell(p.x, p.y);
            if (cell >= 0) atomicAdd(&sh.cnt[e < nb ? 0 : 1][cell], 1);
        }
        __syncthreads();


        // (c) the ring points of the other vehicles, ascending (vehicle, point): offered BLOCK at a time, walked per chunk
        int n_pts = 0;
#pragma unroll 1
        for (int base = nbs; base < P; base += BLOCK) {                // uniform
            const int e = base + tid;
            int cell = -1;
            float rx = 0.0f, ry = 0.0f;
            if (e < P && (e < own_lo || e >= own_hi)) {
                const float2 p = one_tile ? sh.tile[e] : run.point(e);
                cell = w.cell(p.x, p.y);
                if (cell >= 0) {
                    const int pidx = e - ring0;                        // the point's index in the rings' array
                    int lo = vk0, hi = vk1 - 1;                        // the owner: the last vehicle whose ring begins at or before it
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (voff[mid] <= pidx) lo = mid; else hi = mid - 1;
                    }
                    const float4 cv = a.geo[2].ctr[lo];
                    rx = cv.z - vxk;
                    ry = cv.w - vyk;
                    vgrid_rotate(w.rot, w.hx, w.hy, rx, ry);
                }
            }
            // (behind the compaction's first barrier everyone is done with the list walked before)
            n_pts += block_compact(cell >= 0, sh.wcount, lane, wave, n_pts, [&](int p) {
                sh.cid[p] = (unsigned short)cell;
                sh.rv[p] = make_float2(rx, ry);
            });
            offered += BLOCK;
            if (offered == VGRID_LIST || base + BLOCK >= P) {          // uniform: the chunk is full, or the run is over
                VGRID_WALK(n_pts, d, u, z);
                n_pts = 0;
                offered = 0;
            }
        }
#undef VGRID_WALK
#undef VGRID_ADD

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
