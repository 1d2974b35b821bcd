// sfm_batch_route.hip -- routes of batched scenes for gfx950 (MI355X): ONE launch plans, for every chosen scene, the route of each
// routed row from where the row stands to its goal over the scene's walk graph (sfm_batch_set_routes; the rule is specified in
// include/sfm_hip.h), and leaves it where the tick pops waypoints from: the row's current waypoint and its span of the mode queue.
// What the reference does per pedestrian at spawn time on the host (path_planner.PedPathPlanner.generate_route) a batch does per
// scene and per restart, behind the restart and noise kernels, with nothing on the host.
//
// Shape (workgroup b, 4 waves; the same list / mask head as the restart kernel -- a scene that is not chosen leaves at once):
//   a wave per routed row: the scene's routed rows are dealt to the waves in turn (every wave walks the scene's graph types 64 rows
//   at a time and counts the routed ones; row number q of them belongs to wave q mod 4).  For its row the wave
//   1. finds s and t, the usable nodes nearest to the origin and to the goal: a lane owns nodes lane, lane + 64, ...; per lane a
//      strict < in ascending index, then a (d2, index) minimum over the lanes -- the lowest index wins a tie;
//   2. relaxes distances from t in synchronous rounds: two distance arrays and `next` in the wave's LDS (10 bytes per node); a lane pulls over
//      its nodes' CSR neighbours (ascending, so the lowest neighbour wins among equal minima), reads the round before only and
//      writes the other array; "anything changed" is a ballot; at most V rounds;
//   3. walks `next` from s to t (uniform LDS reads, at most V hops), lane 0 keeping the path in the distance array that is free by
//      then; trims the ends; the lanes then store the entries side by side: entry 0 into own[].xy, entries 1 .. L-1 right-aligned
//      into the row's queue span, the cursor, the mode and the target, the status and the info.
// No workgroup barrier: waves run different numbers of rounds and rows.  LDS writes and reads of a wave's lanes are ordered by
// wave_sync() (the LDS executes a wave's instructions in order; the fences keep the compiler from moving them).  Nothing the kernel
// stores to global memory is read back in it, so scalar loads (of wave-uniform indices) never meet its own vector stores.  Every
// loop is bounded by a constant or by a clamped count, whatever the data holds.  The scene's adjacency offsets, and its entries
// when they fit, are staged in LDS once per workgroup in front of the row loop (the kernel's one barrier), so a round costs LDS
// reads only.  No atomics.  The LDS is dynamic, sized for the batch's largest graph: 10 bytes per node and wave, 4 per node and
// 8 per staged adjacency entry -- 8 KiB for street graphs of 100 nodes, at most 64 KiB.
#include "sfm_device.h"
#include "sfm_interaction.h"

#pragma clang fp contract(off)     // every operation of the rule is a single rounding, or an explicit fmaf

namespace sfm {

constexpr uint32_t NEXT_NONE = 0xFFFFu;
// The kernel's LDS is dynamic, sized by the host for the batch's largest graph (route_lds_bytes): v_cap nodes (a multiple of 64)
// and a_cap staged adjacency entries.  A batch of street graphs of 100 nodes takes 8 KiB per workgroup, not the 60 KiB of the
// bounds, so a CU holds all the workgroups it is dealt at once.  Layout: off[v_cap + 2] ints, adj[a_cap] uint2, then per wave
// d[0][v_cap], d[1][v_cap] floats and nxt[v_cap] uint16.
struct RouteWave {
    float* d;                                                          // d[c * stride + v], c = 0 / 1: the round before and the round being written
    uint16_t* nxt;                                                     // neighbour | type of the edge << 10; NEXT_NONE
    int stride;                                                        // v_cap
};
// The scene's graph as every wave and every row of the workgroup reads it: the nodes' offsets into the scene's adjacency, relative
// to its first entry, and -- when the scene has no more than a_cap entries (a street graph has two to four per node) -- the entries
// themselves.  A round then costs LDS reads only; a larger adjacency is read from global memory (it is read only).
struct RouteGraph {
    const int* off;
    const uint2* adj;
    int A;                                                             // entries of the scene, clamped to >= 0
    bool staged;                                                       // adj holds them all
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float route_d2(float2 p, float2 q) {
    const float dx = p.x - q.x, dy = p.y - q.y;
    return fmaf(dx, dx, dy * dy);
}

// bit `type` set: graph type g drops edges of that type (path_planner._extract_subgraphs)
__device__ __forceinline__ uint32_t route_dropped(uint32_t g) { return g == 1u ? 0x38u : g == 2u ? 0x28u : 0u; }

// (d2, index) minimum over the wave; index -1 (no node) loses against every node
__device__ __forceinline__ void route_min(float& d, int& i) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const float od = __shfl_xor(d, m);
        const int oi = __shfl_xor(i, m);
        if (od < d || (od == d && (uint32_t)oi < (uint32_t)i)) { d = od; i = oi; }
    }
}

// The row walks straight: its waypoint is the goal and its queue is empty.
__device__ __forceinline__ void route_straight(const RouteArgs& a, int r, int C, float2 goal, int lane) {
    if (lane != 0) return;
    *reinterpret_cast<float2*>(a.own + r) = goal;
    a.cursor[r] = C;
    a.mode[r] = MODE_WALKING;
    a.target[r] = fsm_enter(MODE_WALKING, 0.0f, a.speeds[r].x, a.speeds[r].y);
}

__device__ __forceinline__ void route_result(const RouteArgs& a, int r, int status, int s, int t, int L, float cost, int lane) {
    if (lane != 0) return;
    a.status[r] = status;
    a.info[r] = make_int4(s, t, L, __float_as_int(cost));
}

// entry e of the scene's adjacency (uniform choice of the source)
__device__ __forceinline__ uint2 route_edge(const RouteGraph& gr, const uint2* __restrict__ adjg, int e) {
    return gr.staged ? gr.adj[e] : adjg[e];
}
// node v's entries [e0, e1): at most ROUTE_MAX_NODES of them, inside the scene's adjacency whatever the offsets hold
__device__ __forceinline__ void route_span(const RouteGraph& gr, int v, int& e0, int& e1) {
    e0 = min(max(gr.off[v], 0), gr.A);
    e1 = min(min(gr.off[v + 1], e0 + ROUTE_MAX_NODES), gr.A);
}

__device__ __forceinline__ void route_row(const RouteArgs& a, const RouteWave& sh, const RouteGraph& gr, int r, int V,
                                          const float2* __restrict__ nxy, const uint2* __restrict__ adjg, int lane) {
    const float inf = __builtin_inff();
    const float4 q = a.pk[r];
    if (!row_live(q.x, q.y) || a.mode[r] == MODE_DESPAWNED) { route_result(a, r, ROUTE_NOT_LIVE, -1, -1, 0, inf, lane); return; }
    const float2 goal = a.goal[r];
    if (!(fabsf(goal.x) < inf && fabsf(goal.y) < inf)) { route_result(a, r, ROUTE_BAD_GOAL, -1, -1, 0, inf, lane); return; }
    const float2 org = make_float2(q.x, q.y);
    const int e_row = a.wp_off[r];
    const int C = min(max(a.wp_off[r + 1] - e_row, 0), ROUTE_MAX_CAPACITY);
    const uint32_t drop = route_dropped(a.gtype[r]);

    // 1. the ends, and the fields' start values
    float ds = inf, dt = inf;
    int s = -1, t = -1;
    for (int v = lane; v < V; v += WAVE) {
        int e0, e1;
        route_span(gr, v, e0, e1);
        bool usable = false;
        for (int e = e0; e < e1 && !usable; ++e) usable = ((drop >> ((route_edge(gr, adjg, e).x >> 16) & 7u)) & 1u) == 0u;
        sh.d[v] = inf;
        sh.nxt[v] = (uint16_t)NEXT_NONE;
        if (!usable) continue;
        const float2 p = nxy[v];
        const float d_o = route_d2(p, org), d_g = route_d2(p, goal);
        if (d_o < ds) { ds = d_o; s = v; }
        if (d_g < dt) { dt = d_g; t = v; }
    }
    route_min(ds, s);
    route_min(dt, t);
    s = uniform(s);
    t = uniform(t);
    if (s < 0 || t < 0) {                                              // uniform: no usable node
        route_straight(a, r, C, goal, lane);
        route_result(a, r, ROUTE_NO_PATH, s, t, 1, inf, lane);
        return;
    }
    wave_sync();
    if (lane == 0) sh.d[t] = 0.0f;
    wave_sync();

    // 2. distances from t
    int cur = 0;
    for (int round = 0; round < V; ++round) {                          // uniform
        bool changed = false;
        for (int v = lane; v < V; v += WAVE) {
            int e0, e1;
            route_span(gr, v, e0, e1);
            const float old = sh.d[cur * sh.stride + v];
            float best = old;
            uint32_t nx = 0;
            for (int e = e0; e < e1; ++e) {
                const uint2 ad = route_edge(gr, adjg, e);
                const uint32_t type = (ad.x >> 16) & 7u, u = ad.x & 0xFFFFu;
                if (((drop >> type) & 1u) || u >= (uint32_t)V) continue;
                const float c = sh.d[cur * sh.stride + (int)u] + __uint_as_float(ad.y);
                if (c < best) { best = c; nx = u | (type << 10); }
            }
            sh.d[(cur ^ 1) * sh.stride + v] = best;
            if (best < old) { sh.nxt[v] = (uint16_t)nx; changed = true; }
        }
        wave_sync();
        cur ^= 1;
        if (!__any(changed)) break;                                    // uniform
    }
    const float cost = sh.d[cur * sh.stride + s];
    if (!(cost < inf)) {                                               // uniform: t is not reachable from s
        route_straight(a, r, C, goal, lane);
        route_result(a, r, ROUTE_NO_PATH, s, t, 1, inf, lane);
        return;
    }

    // 3. the walk: path[j] = node j of s .. t | type of the edge walked into it << 10
    uint32_t* path = reinterpret_cast<uint32_t*>(sh.d + (cur ^ 1) * sh.stride);
    wave_sync();                                                       // (everyone has read the last round)
    int v = s, m = 1;
    if (lane == 0) path[0] = (uint32_t)s;
    for (int h = 0; h < V - 1 && v != t; ++h) {                        // uniform
        const uint32_t nx = (uint32_t)uniform((int)sh.nxt[v]);
        if (nx == NEXT_NONE) break;
        if (lane == 0) path[m] = nx;
        v = (int)(nx & 0x3FFu);
        ++m;
    }
    wave_sync();
    if (v != t) {                                                      // uniform (cannot be while D[s] is finite)
        route_straight(a, r, C, goal, lane);
        route_result(a, r, ROUTE_NO_PATH, s, t, 1, inf, lane);
        return;
    }
    int first = 0, last = m - 1;
    if (m > 1) {                                                       // both tests on the untrimmed list
        const float2 n0 = nxy[s], n1 = nxy[path[1] & 0x3FFu], nl = nxy[t], np = nxy[path[m - 2] & 0x3FFu];
        if (route_d2(n0, n1) > route_d2(org, n1)) first = 1;
        if (route_d2(nl, np) > route_d2(goal, np)) last = m - 2;
    }
    const int cnt = last - first + 1 >= 2 ? last - first + 1 : 0;      // fewer than two nodes contribute nothing
    const int L = cnt + 1;
    if (L - 1 > C) {                                                   // uniform
        route_straight(a, r, C, goal, lane);
        route_result(a, r, ROUTE_TOO_LONG, s, t, L, cost, lane);
        return;
    }
    const int c0 = C - (L - 1);
    for (int k = lane; k < L; k += WAVE) {                             // entry k: node first + k, the last one the goal
        float2 w = goal;
        uint8_t cross = 0;
        if (k < cnt) {
            const uint32_t pe = path[first + k];
            const uint32_t type = pe >> 10;
            w = nxy[pe & 0x3FFu];
            cross = (k > 0 && type >= 2u && type <= 4u) ? 1 : 0;
        }
        if (k == 0) {
            *reinterpret_cast<float2*>(a.own + r) = w;
        } else {
            a.wp_xy[e_row + c0 + k - 1] = w;
            a.wp_cross[e_row + c0 + k - 1] = cross;
        }
    }
    if (lane == 0) {
        a.cursor[r] = c0;
        a.mode[r] = MODE_WALKING;
        a.target[r] = fsm_enter(MODE_WALKING, 0.0f, a.speeds[r].x, a.speeds[r].y);
    }
    route_result(a, r, ROUTE_PLANNED, s, t, L, cost, lane);
    wave_sync();                                                       // the path has been read before the next row's fields overwrite it
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_plan_routes_kernel(const RouteArgs a) {
    extern __shared__ __align__(16) unsigned char route_lds[];
    const int b = a.list ? a.list[blockIdx.x] : (int)blockIdx.x;
    if (a.mask && a.mask[b] == 0) return;                              // uniform: the scene is not chosen
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = uniform((int)threadIdx.x >> 6);
    const int s0 = a.scene_off[b], n = min(a.scene_off[b + 1] - s0, BATCH_MAX_N);
    const int v_cap = min(max(a.v_cap, 0), ROUTE_MAX_NODES), a_cap = max(a.a_cap, 0);
    const int v0 = a.node_off[b], V = min(max(a.node_off[b + 1] - v0, 0), v_cap);
    int* off_s = reinterpret_cast<int*>(route_lds);
    uint2* adj_s = reinterpret_cast<uint2*>(off_s + v_cap + 2);
    float* wave_s = reinterpret_cast<float*>(adj_s + a_cap) + (size_t)wave * (2 * v_cap + v_cap / 2);
    const RouteWave sh{wave_s, reinterpret_cast<uint16_t*>(wave_s + 2 * v_cap), v_cap};
    // the scene's graph into LDS, once for all waves and rows (the only barrier: in front of the row loop, reached by every wave)
    const int a0 = a.adj_off[v0], A = max(a.adj_off[v0 + V] - a0, 0);
    const RouteGraph gr{off_s, adj_s, A, A <= a_cap};                  // uniform
    for (int v = threadIdx.x; v <= V; v += BLOCK) off_s[v] = a.adj_off[v0 + v] - a0;
    if (gr.staged)
        for (int e = threadIdx.x; e < A; e += BLOCK) adj_s[e] = a.adj[a0 + e];
    __syncthreads();
    int seen = 0;                                                      // routed rows of the scene so far
    for (int i0 = 0; i0 < n; i0 += WAVE) {                             // uniform
        const int i = i0 + lane;
        const bool routed = i < n && a.gtype[s0 + i] != 0;
        unsigned long long todo = __ballot(routed);
        for (int k = 0; k < WAVE && todo; ++k) {                       // uniform
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            if ((seen++ & (WAVES_PER_BLOCK - 1)) != wave) continue;
            route_row(a, sh, gr, s0 + i0 + j, V, a.node_xy + v0, a.adj + a0, lane);
        }
    }
}

// LDS of a launch whose largest graph has v_cap nodes (a multiple of 64) with a_cap adjacency entries staged
size_t route_lds_bytes(int v_cap, int a_cap) {
    return sizeof(int) * ((size_t)v_cap + 2) + sizeof(uint2) * (size_t)a_cap + (size_t)WAVES_PER_BLOCK * 10 * (size_t)v_cap;
}

hipError_t launch_batch_plan_routes(const RouteArgs& a, int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_plan_routes_kernel, dim3(scenes), dim3(BLOCK), route_lds_bytes(a.v_cap, a.a_cap), st, a);
    return hipGetLastError();
}

}  // namespace sfm
