// sfm_batch_grid.hip -- egocentric occupancy grids of batched scenes for gfx950 (MI355X): ONE launch for the whole batch
// (sfm_batch_grid; the record and its rules are specified in include/sfm_hip.h).
//
// What a policy sees per agent: a G x G map centred on the row -- per cell the number of other pedestrians, the sum of their
// velocities relative to the row, and the number of sampled border, static-obstacle and vehicle points.  Computed from the buffers
// the tick reads (state, own, the scene offsets, the three geometry CSRs) into a device buffer [M][6][G][G] of floats, one compact
// slot per gridded row.  The kernel writes nothing else, so a tick before or after it computes what it computed without it.
//
// Shape (workgroup b, 4 waves):
//   1. the scene's {x, y, vx, vy} is staged in LDS and the geometry counts are cleared, then a barrier;
//   2. the rows that have a slot are compacted, in ascending order, into an LDS list by ballots and per-wave counts; when the
//      scene's geometry fits one tile of GRID_TILE points it is staged in LDS once, else every row reads it from memory (a point
//      is used once per row, by one lane);
//   3. per gridded row, in list order (a row that is not live gets its zeros and is done): the window is the row's -- G x G cells
//      around its position, in frame 1 turned by the scan kernel's heading (GridWindow, sfm_grid_cells.h: the rotation and the cell
//      rule live there);
//      (a) the OTHER live pedestrians are offered to the shared loop (GRID_OFFER): lane t takes pedestrians t, t + BLOCK, .., the
//          sources inside the grid are compacted in ascending j into the LDS list {cell, relative velocity}, and the list -- it holds
//          a whole scene, so once, at the end -- is walked in order into the cells tid, tid + BLOCK, .. the lane owns (G^2 <= 1024: up
//          to 4; GRID_WALK and GRID_ADD, with the order and the wave test described there);
//      (b) every lane takes geometry points e, e + BLOCK, .. of the three kinds' contiguous runs and counts the cell of each with an
//          integer LDS add (the result of integer adds does not depend on their order);
//   4. the lane stores the 6 channels of its cells (consecutive lanes store consecutive floats) and clears the geometry counts it
//      read; the next row's adds come behind the barriers of its phase (a).
// What is this kernel's own: the list of gridded rows, the one-line staging of the tile (SceneRun::stage costs set-up here, as in the
// scan kernel), that a source is a live row other than the gridded one, and the store with its three kinds of counts.
// No register array is indexed at run time, so nothing goes to scratch.
// Determinism: no float atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or
// anywhere in any batch.
#include "sfm_grid_cells.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

constexpr int GRID_TILE = 1024;    // geometry points the LDS tile holds

struct GridShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    float2 tile[GRID_TILE];                                            // the scene's geometry points, when they fit
    float2 rv[BATCH_MAX_N];                                            // the sources inside the grid, ascending: relative velocity ...
    unsigned short cid[BATCH_MAX_N];                                   // ... and cell
    unsigned short rows[BATCH_MAX_N];                                  // the gridded rows, ascending
    int cnt[3][GRID_MAX_CELLS];                                        // geometry points per kind and cell
    int wcount[WAVES_PER_BLOCK];
};
static_assert(sizeof(GridShared) <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");

__global__ __launch_bounds__(BLOCK) void sfm_batch_grid_kernel(const GridArgs a) {
    __shared__ GridShared sh;
    const int b = blockIdx.x;
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    if (n <= 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.G, cells = G * G;                                  // 1 .. GRID_MAX_G, cells <= GRID_MAX_CELLS
    for (int t = tid; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    for (int q = tid; q < 3 * GRID_MAX_CELLS; q += BLOCK) (&sh.cnt[0][0])[q] = 0;
    __syncthreads();

    // 2. the gridded rows, ascending
    int n_grid = 0;
#pragma unroll 1
    for (int base = 0; base < n; base += BLOCK) {                      // uniform
        const int t = base + tid;
        const bool want = t < n && (!a.slot || a.slot[s0 + t] >= 0);
        n_grid += block_compact(want, sh.wcount, lane, wave, n_grid, [&](int p) { sh.rows[p] = (unsigned short)t; });
    }
    if (n_grid == 0) return;                                           // uniform

    const SceneRun run(a.geo, b);
    const int nb = run.nb, ns = run.ns, P = run.total();               // virtual index e: borders, static, vehicles
    const bool one_tile = P <= GRID_TILE;
    if (one_tile && P > 0) {                                           // the whole scene's geometry fits: staged once
        for (int e = tid; e < P; e += BLOCK) sh.tile[e] = run.point(e);
        __syncthreads();
    }

    GridWindow w(a.cell[b], G, G, a.frame != 0);                       // (rot: uniform)
    const size_t per_row = (size_t)GRID_CHANNELS * (size_t)cells;
#pragma unroll 1
    for (int pos = 0; pos < n_grid; ++pos) {                           // uniform
        const int row = __builtin_amdgcn_readfirstlane((int)sh.rows[pos]);
        const float4 s = sh.pk[row];
        const size_t slot = a.slot ? (size_t)a.slot[s0 + row] : (size_t)(s0 + row);
        float* out = a.out + slot * per_row;
        if (!row_live(s.x, s.y)) {                                     // uniform: a gridded row that is not live reads zeros
            for (int q = tid; q < (int)per_row; q += BLOCK) out[q] = 0.0f;
            continue;
        }
        const float vx = s.z, vy = s.w;
        w.ox = s.x;
        w.oy = s.y;
        w.hx = 1.0f;
        w.hy = 0.0f;
        if (w.rot) {                                                   // the scan kernel's heading, fp32 throughout
            const float4 o = a.own[s0 + row];
            const float2 h = row_heading(vx, vy, o.x - s.x, o.y - s.y);
            w.hx = h.x;
            w.hy = h.y;
        }

        // (a), (b) the other live pedestrians inside the grid, ascending, with their cells and relative velocities: the list holds
        // them all, so it is walked once, at the end
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f, y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
        auto other = [&](int t, int& cell, float& rx, float& ry) {
            const float4 p = sh.pk[t];
            if (t == row || !row_live(p.x, p.y)) return;
            cell = w.cell(p.x, p.y);
            rx = p.z - vx;
            ry = p.w - vy;
            w.rotate(rx, ry);
        };
        GRID_OFFER(BATCH_MAX_N, 0, n, other, c, x, y);
        // ... and the geometry points per kind and cell (behind the barriers above: the counts of the row before were cleared)
        for (int e = tid; e < P; e += BLOCK) {
            const float2 p = one_tile ? sh.tile[e] : run.point(e);
            const int cell = w.cell(p.x, p.y);
            if (cell >= 0) atomicAdd(&sh.cnt[e < nb ? 0 : e < nb + ns ? 1 : 2][cell], 1);
        }
        if (P > 0) __syncthreads();                                    // uniform

        // 4. the row's 6 G^2 floats
        auto store = [&](int cell, int count, float sx, float sy) {
            if (cell >= cells) return;
            out[cell] = (float)count;
            out[cells + cell] = sx;
            out[2 * cells + cell] = sy;
#pragma unroll
            for (int kind = 0; kind < 3; ++kind) {
                const int pts = P > 0 ? sh.cnt[kind][cell] : 0;
                out[(3 + kind) * cells + cell] = (float)pts;
                if (pts) sh.cnt[kind][cell] = 0;                       // (only this lane reads or clears the cell)
            }
        };
        store(tid, c0, x0, y0);
        store(tid + BLOCK, c1, x1, y1);
        store(tid + 2 * BLOCK, c2, x2, y2);
        store(tid + 3 * BLOCK, c3, x3, y3);
    }
}

hipError_t launch_batch_grid(const GridArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_grid_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
