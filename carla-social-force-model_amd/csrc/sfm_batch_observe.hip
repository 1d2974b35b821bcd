// sfm_batch_observe.hip -- per-pedestrian observations of batched scenes for gfx950 (MI355X): ONE launch for the whole batch
// (sfm_batch_observe, ABI 15; the record is specified in include/sfm_hip.h).
//
// What a policy or a reward reads per agent: its K nearest neighbours inside the scene's sense range and how they move relative to
// it, the nearest point of the scene's borders, static obstacles and vehicle rings, its goal and its own motion -- computed from the
// buffers the tick reads (state, own, the scene offsets, the three geometry CSRs), into a device buffer [N_total][16 + 4k] of floats.
// The kernel writes nothing else, so a tick before or after it computes what it computed without it.
//
// Shape (workgroup b, 4 waves), the tick's own:
//   1. the scene's {x, y, vx, vy} are staged in LDS once (<= 16 KiB), then a barrier;
//   2. a lane owns a row.  N_b > 64: one wave per 64 rows, scenes above 256 rows in passes, a wave without rows leaves after the
//      barrier, and each lane does steps 3 to 5 for its row.  N_b <= 64: the four waves share the one block of rows by ROLE -- wave 0
//      selects the neighbours (step 3) while waves 1, 2 and 3 scan one geometry kind each (step 4) and leave what they found in LDS;
//      after a second barrier wave 0 stores the rows (step 5).  The roles compute what the one-wave form computes, value for value;
//   3. neighbours: the lane walks ALL j of the scene in ascending order as broadcast LDS reads and keeps its KT best (d2, j) in
//      registers, sorted.  A candidate is inserted behind every kept entry with d2' <= d2 (strict `<`), so among equal distances the
//      lower j stays in front: the first k of ascending (d2, j).  The insertion is a fully unrolled compare-and-select chain -- no
//      register array is indexed at run time, so nothing goes to scratch.  Empty slots hold d2 = +inf, and a j that is no candidate
//      (j == i, d2 >= R2, NaN) enters the chain as +inf, which no slot takes.  A wave skips the chain while no lane has a candidate
//      below its worst kept distance (the chain would select nothing: results are bitwise unchanged);
//   4. nearest points: per kind, lane_nearest per polyline (np.argmin's first-minimum rule inside it), dist2 to the returned point
//      recomputed with the same operations, strict `<` across polylines in order -- the first minimum over all points of the kind;
//   5. the lane stores its row with 16-byte stores.
// KT is a template parameter (1, 4, 8, 16; the host runs the smallest that holds k): the first k of the best KT are the best k.
// Frame 1 rotates every 2-vector into the row's heading frame AFTER everything is selected, so selection, order, m and flags are
// those of frame 0.
// Determinism: no atomics, every order is a function of the scene alone -- a scene's record is bitwise the same alone or anywhere in
// any batch.
#include "sfm_device.h"
#include "sfm_interaction.h"

namespace sfm {

struct ObserveNear {                                                   // what one kind's scan found for a row
    float d2;                                                          // +inf: the scene has no point of the kind
    float2 p, v;                                                       // the point, and its item's velocity (vehicles)
};

struct ObserveShared {
    float4 pk[BATCH_MAX_N];                                            // {x, y, vx, vy}
    __attribute__((aligned(16))) float2 row[WAVES_PER_BLOCK][WAVE];    // lane_nearest's per-wave rows
    ObserveNear near[3][WAVE];                                         // N_b <= 64: the geometry waves' results, [kind][row]
};

// nearest point of every polyline of one kind of scene b: first minimum over polylines in order, points in order
__device__ __forceinline__ ObserveNear observe_nearest(const BatchGeo& g, int b, float x, float y, float2* row, int lane) {
    ObserveNear r{__builtin_inff(), make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
    const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
#pragma unroll 1
    for (int k = k0; k < k1; ++k) {                                    // uniform
        const int o0 = g.off[k], o1 = g.off[k + 1];
        if (o1 <= o0) continue;                                        // a polyline without points has no nearest point
        const float2 sp = lane_nearest(g.pts, o0, o1, x, y, row, lane);
        const float d2 = dist2(x, y, sp.x, sp.y);
        const bool take = d2 < r.d2;
        const float4 c = g.ctr[k];
        r.d2 = take ? d2 : r.d2;
        r.p = take ? sp : r.p;
        r.v = take ? make_float2(c.z, c.w) : r.v;
    }
    return r;
}

// the KT best (d2, j) of row ii over all j of the scene, ascending, ties by ascending j; empty slots: d2 = +inf
template <int KT>
__device__ __forceinline__ void observe_select(const ObserveShared& sh, int n, int ii, float x, float y, float R2, float (&bd)[KT],
                                               int (&bj)[KT]) {
    const float inf = __builtin_inff();
#pragma unroll
    for (int q = 0; q < KT; ++q) { bd[q] = inf; bj[q] = 0; }
#pragma unroll 1
    for (int j = 0; j < n; ++j) {                                      // uniform: the LDS read is a broadcast
        const float4 pj = sh.pk[j];
        const float dx = pj.x - x, dy = pj.y - y;
        const float d2 = fmaf(dx, dx, dy * dy);
        const float d = (d2 < R2 && j != ii) ? d2 : inf;
        if (!__any(d < bd[KT - 1])) continue;                          // no lane of the wave would keep it
#pragma unroll
        for (int q = KT - 1; q >= 1; --q) {                            // behind every entry with bd <= d; the tail moves down
            const bool before = d < bd[q], before_prev = d < bd[q - 1];
            bd[q] = before_prev ? bd[q - 1] : before ? d : bd[q];
            bj[q] = before_prev ? bj[q - 1] : before ? j : bj[q];
        }
        const bool first = d < bd[0];
        bd[0] = first ? d : bd[0];
        bj[0] = first ? j : bj[0];
    }
}

// row i of the scene (staged as s) into the observation buffer
template <int KT>
__device__ __forceinline__ void observe_store(const ObserveArgs& a, const ObserveShared& sh, int s0, int i, const float4& s, float R2,
                                              const float (&bd)[KT], const int (&bj)[KT], const ObserveNear& nb, const ObserveNear& ns,
                                              const ObserveNear& nv) {
    const int k = a.k;                                                 // 1 <= k <= KT
    const float inf = __builtin_inff();
    const float x = s.x, y = s.y, vx = s.z, vy = s.w;
    float4* out = reinterpret_cast<float4*>(a.obs + (size_t)(s0 + i) * (size_t)(16 + 4 * k));
    const bool live = row_live(x, y);                                  // (a NaN position fails it)
    if (!live) {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        out[0] = z4; out[1] = z4; out[2] = z4; out[3] = z4;
#pragma unroll
        for (int q = 0; q < KT; ++q)
            if (q < k) out[4 + q] = z4;
        return;
    }
    const float4 o = a.own[s0 + i];
    const bool hb = nb.d2 < R2, hs = ns.d2 < R2, hv = nv.d2 < R2;
    int m = 0;
#pragma unroll
    for (int q = 0; q < KT; ++q) m += (q < k && bd[q] < inf) ? 1 : 0;
    float4 h0 = make_float4(o.x - x, o.y - y, vx, vy);
    float4 h2 = hv ? make_float4(nv.p.x - x, nv.p.y - y, nv.v.x - vx, nv.v.y - vy) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 h3 = make_float4(hb ? nb.p.x - x : 0.f, hb ? nb.p.y - y : 0.f, hs ? ns.p.x - x : 0.f, hs ? ns.p.y - y : 0.f);
    // frame 1: the heading is v / |v|, else the goal's direction, else (1, 0) (row_heading)
    float hx = 1.0f, hy = 0.0f;
    if (a.frame) {                                                     // uniform
        const float2 h = row_heading(vx, vy, h0.x, h0.y);
        hx = h.x;
        hy = h.y;
    }
    auto rot = [&](float& p, float& q) {
        const float rp = fmaf(hx, p, hy * q), rq = fmaf(-hy, p, hx * q);
        p = rp; q = rq;
    };
    if (a.frame) {
        rot(h0.x, h0.y); rot(h0.z, h0.w);
        rot(h2.x, h2.y); rot(h2.z, h2.w);
        rot(h3.x, h3.y); rot(h3.z, h3.w);
    }
    out[0] = h0;
    out[1] = make_float4(o.z, 1.0f, (float)m, (float)((hb ? 1 : 0) + (hs ? 2 : 0) + (hv ? 4 : 0)));
    out[2] = h2;
    out[3] = h3;
#pragma unroll
    for (int q = 0; q < KT; ++q) {
        if (q >= k) continue;                                          // uniform
        const float4 pj = sh.pk[bj[q]];
        const bool filled = bd[q] < inf;
        float4 e = filled ? make_float4(pj.x - x, pj.y - y, pj.z - vx, pj.w - vy) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.frame) { rot(e.x, e.y); rot(e.z, e.w); }
        out[4 + q] = e;
    }
}

template <int KT>
__global__ __launch_bounds__(BLOCK) void sfm_batch_observe_kernel(const ObserveArgs a) {
    __shared__ ObserveShared sh;
    const int b = blockIdx.x;
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;        // 0 <= n <= BATCH_MAX_N (checked on the host)
    if (n <= 0) return;
    for (int t = threadIdx.x; t < n; t += BLOCK) sh.pk[t] = a.pk[s0 + t];
    __syncthreads();
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const float R2 = a.range2[b];
    float bd[KT];
    int bj[KT];
    if (n <= WAVE) {                                                   // uniform: one block of rows, the waves split by role
        const bool there = lane < n;
        const int ii = there ? lane : n - 1;
        const float4 s = sh.pk[ii];
        if (wave == 0) {
            observe_select<KT>(sh, n, ii, s.x, s.y, R2, bd, bj);
        } else {                                                       // wave 1: borders, 2: static obstacles, 3: vehicles
            const BatchGeo g = wave == 1 ? a.geo[0] : wave == 2 ? a.geo[1] : a.geo[2];    // (selects: no indexed copy in scratch)
            sh.near[wave - 1][lane] = observe_nearest(g, b, s.x, s.y, sh.row[wave], lane);
        }
        __syncthreads();                                               // (every wave of the workgroup reaches it)
        if (wave == 0 && there) observe_store<KT>(a, sh, s0, lane, s, R2, bd, bj, sh.near[0][lane], sh.near[1][lane], sh.near[2][lane]);
        return;
    }
#pragma unroll 1
    for (int base = wave * WAVE; base < n; base += BLOCK) {            // uniform per wave
        const int i = base + lane;
        const bool there = i < n;
        const int ii = there ? i : n - 1;
        const float4 s = sh.pk[ii];
        observe_select<KT>(sh, n, ii, s.x, s.y, R2, bd, bj);
        const ObserveNear nb = observe_nearest(a.geo[0], b, s.x, s.y, sh.row[wave], lane);
        const ObserveNear ns = observe_nearest(a.geo[1], b, s.x, s.y, sh.row[wave], lane);
        const ObserveNear nv = observe_nearest(a.geo[2], b, s.x, s.y, sh.row[wave], lane);
        if (there) observe_store<KT>(a, sh, s0, i, s, R2, bd, bj, nb, ns, nv);
    }
}

hipError_t launch_batch_observe(const ObserveArgs& a, int B, hipStream_t st) {
    if (a.k <= 1) hipLaunchKernelGGL(sfm_batch_observe_kernel<1>, dim3(B), dim3(BLOCK), 0, st, a);
    else if (a.k <= 4) hipLaunchKernelGGL(sfm_batch_observe_kernel<4>, dim3(B), dim3(BLOCK), 0, st, a);
    else if (a.k <= 8) hipLaunchKernelGGL(sfm_batch_observe_kernel<8>, dim3(B), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL(sfm_batch_observe_kernel<16>, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
