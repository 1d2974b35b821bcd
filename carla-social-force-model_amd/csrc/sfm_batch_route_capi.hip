// sfm_batch_route_capi.hip -- host side of the batch's routes (sfm_batch_set_routes; the rule is specified in include/sfm_hip.h):
// the graphs, the per-row settings and results, the queue CSR rebuilt for the routed rows, the explicit plan calls, and the launch
// every restart path puts behind batch_restart_noise (sfm_batch_route.hip).  The batch's types are in sfm_batch_host.h; the
// restarts themselves in sfm_batch_capi.hip.
#include "sfm_batch_host.h"

using namespace sfm;

int sfm::batch_plan_routes(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes) {
    const BatchRoutesDev& z = b->routes;
    if (!z.on || scenes <= 0 || b->n_total == 0) return SFM_OK;
    RouteArgs a;
    memset(&a, 0, sizeof(a));
    a.list = d_list;
    a.mask = d_mask;
    a.scene_off = b->d_scene_off;
    a.pk = b->pk;
    a.own = b->own;
    a.mode = b->modes.mode;
    a.target = b->modes.target;
    a.speeds = b->modes.speeds;
    a.wp_off = b->modes.off;
    a.wp_xy = b->modes.xy;
    a.wp_cross = b->modes.cross;
    a.cursor = b->modes.cursor;
    a.node_off = z.node_off;
    a.node_xy = z.node_xy;
    a.adj_off = z.adj_off;
    a.adj = z.adj;
    a.gtype = z.gtype;
    a.goal = z.goal;
    a.status = z.status;
    a.info = z.info;
    a.v_cap = z.v_cap;
    a.a_cap = z.a_cap;
    HIP_TRY(b, launch_batch_plan_routes(a, scenes, b->stream));
    return SFM_OK;
}

extern "C" {

// Everything is checked, and the new buffers are built, before anything of the batch changes: a refusal changes nothing.
int sfm_batch_set_routes(SfmBatch* b, const int32_t* node_off, const float* node_x, const float* node_y, const int32_t* adj_off,
                         const int32_t* adj_node, const float* adj_w, const uint8_t* adj_type, const uint8_t* graph_type,
                         const float* goal_x, const float* goal_y, int capacity) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!node_off) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a plan in flight may still read the buffers
        b->routes = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->modes.on)
        return bfail(b, SFM_ERR_STATE, "routes need modes: call sfm_batch_set_mode_fsm first (a route is walked as a mode queue)");
    if (b->spawns.on)
        return bfail(b, SFM_ERR_STATE, "routes are refused while a spawn schedule is set (unborn rows are not routed)");
    if (capacity < 1 || capacity > SFM_BATCH_MAX_ROUTE_CAPACITY)
        return bfail(b, SFM_ERR_INVALID, "capacity must be 1 .. " + std::to_string(SFM_BATCH_MAX_ROUTE_CAPACITY) + ", got " + std::to_string(capacity));
    const int B = b->B;
    const size_t n = (size_t)b->n_total;
    if (!adj_off) return bfail(b, SFM_ERR_INVALID, "adj_off is NULL");
    if (n > 0 && (!graph_type || !goal_x || !goal_y)) return bfail(b, SFM_ERR_INVALID, "graph_type, goal_x or goal_y is NULL");
    if (node_off[0] != 0) return bfail(b, SFM_ERR_INVALID, "node_off[0] must be 0");
    for (int k = 0; k < B; ++k) {
        const long long v = (long long)node_off[k + 1] - node_off[k];
        if (v < 0 || v > SFM_BATCH_MAX_ROUTE_NODES)
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": " + std::to_string(v) + " nodes, a scene's graph holds 0 .. " +
                                             std::to_string(SFM_BATCH_MAX_ROUTE_NODES));
    }
    const size_t Vt = (size_t)node_off[B];
    if (Vt > 0 && (!node_x || !node_y)) return bfail(b, SFM_ERR_INVALID, "node_x or node_y is NULL");
    if (adj_off[0] != 0) return bfail(b, SFM_ERR_INVALID, "adj_off[0] must be 0");
    for (size_t v = 0; v < Vt; ++v)
        if (adj_off[v + 1] < adj_off[v]) return bfail(b, SFM_ERR_INVALID, "adj_off must be non-decreasing (node " + std::to_string(v) + ")");
    const size_t A = (size_t)adj_off[Vt];
    if (A > 0 && (!adj_node || !adj_w || !adj_type)) return bfail(b, SFM_ERR_INVALID, "adj_node, adj_w or adj_type is NULL");
    std::vector<float2> xy(Vt);
    std::vector<uint2> adj(A);
    for (int k = 0; k < B; ++k) {
        const int V = node_off[k + 1] - node_off[k];
        for (int v = node_off[k]; v < node_off[k + 1]; ++v) {
            if (!std::isfinite(node_x[v]) || !std::isfinite(node_y[v]))
                return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": node " + std::to_string(v - node_off[k]) + " is not finite");
            xy[v] = make_float2(node_x[v], node_y[v]);
            int before = -1;
            for (int e = adj_off[v]; e < adj_off[v + 1]; ++e) {
                const std::string where = "scene " + std::to_string(k) + ", node " + std::to_string(v - node_off[k]) + ": ";
                const int u = adj_node[e];
                if (u < 0 || u >= V || u == v - node_off[k]) return bfail(b, SFM_ERR_INVALID, where + "neighbour " + std::to_string(u) + " is out of range or the node itself");
                if (u <= before) return bfail(b, SFM_ERR_INVALID, where + "the neighbours must be strictly ascending");
                if (adj_type[e] < 1 || adj_type[e] > 5) return bfail(b, SFM_ERR_INVALID, where + "edge type " + std::to_string(adj_type[e]) + " is no EdgeType value 1 .. 5");
                if (!std::isfinite(adj_w[e]) || adj_w[e] < 0.f) return bfail(b, SFM_ERR_INVALID, where + "an edge weight must be finite and >= 0");
                before = u;
                uint32_t wb;
                memcpy(&wb, &adj_w[e], 4);
                adj[e] = make_uint2((uint32_t)u | ((uint32_t)adj_type[e] << 16), wb);
            }
        }
    }
    for (size_t i = 0; i < n; ++i)
        if (graph_type[i] > 3) return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": graph_type must be 0 (not routed), 1, 2 or 3");

    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the queues and cursors as the last tick left them
    // the queue CSR: a routed row owns `capacity` slots, the others keep their lists
    std::vector<int32_t> off_old(n + 1), off_new(n + 1, 0), cursor(n);
    HIP_TRY(b, hipMemcpy(off_old.data(), b->modes.off, 4 * (n + 1), hipMemcpyDeviceToHost));
    if (n > 0) HIP_TRY(b, hipMemcpy(cursor.data(), b->modes.cursor, 4 * n, hipMemcpyDeviceToHost));
    const size_t W_old = (size_t)off_old[n];
    std::vector<float2> q_old(W_old);
    std::vector<uint8_t> c_old(W_old);
    if (W_old > 0) {
        HIP_TRY(b, hipMemcpy(q_old.data(), b->modes.xy, sizeof(float2) * W_old, hipMemcpyDeviceToHost));
        HIP_TRY(b, hipMemcpy(c_old.data(), b->modes.cross, W_old, hipMemcpyDeviceToHost));
    }
    long long W = 0;
    for (size_t i = 0; i < n; ++i) {
        W += graph_type[i] ? capacity : off_old[i + 1] - off_old[i];
        if (W > INT32_MAX) return bfail(b, SFM_ERR_INVALID, "the queues would hold more than 2^31 - 1 slots");
        off_new[i + 1] = (int32_t)W;
    }
    std::vector<float2> q_new((size_t)(W > 0 ? W : 1), make_float2(0.f, 0.f));
    std::vector<uint8_t> c_new(q_new.size(), 0);
    for (size_t i = 0; i < n; ++i) {
        if (graph_type[i]) { cursor[i] = capacity; continue; }   // an empty queue until the first plan
        std::copy(q_old.begin() + off_old[i], q_old.begin() + off_old[i + 1], q_new.begin() + off_new[i]);
        std::copy(c_old.begin() + off_old[i], c_old.begin() + off_old[i + 1], c_new.begin() + off_new[i]);
    }
    std::vector<float2> goal(n);
    for (size_t i = 0; i < n; ++i) goal[i] = make_float2(goal_x[i], goal_y[i]);

    BatchRoutesDev z;
    DevBuf<float2> q_dev;
    DevBuf<uint8_t> c_dev;
    HIP_TRY(b, z.node_off.alloc((size_t)B + 1)); HIP_TRY(b, z.node_xy.alloc(Vt > 0 ? Vt : 1)); HIP_TRY(b, z.adj_off.alloc(Vt + 1));
    HIP_TRY(b, z.adj.alloc(A > 0 ? A : 1));
    const size_t m = n > 0 ? n : 1;
    HIP_TRY(b, z.gtype.alloc(m)); HIP_TRY(b, z.goal.alloc(m)); HIP_TRY(b, z.status.alloc(m)); HIP_TRY(b, z.info.alloc(m));
    HIP_TRY(b, q_dev.alloc(q_new.size())); HIP_TRY(b, c_dev.alloc(c_new.size()));
    HIP_TRY(b, hipMemcpy(z.node_off, node_off, 4 * ((size_t)B + 1), hipMemcpyHostToDevice));
    if (Vt > 0) HIP_TRY(b, hipMemcpy(z.node_xy, xy.data(), sizeof(float2) * Vt, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(z.adj_off, adj_off, 4 * (Vt + 1), hipMemcpyHostToDevice));
    if (A > 0) HIP_TRY(b, hipMemcpy(z.adj, adj.data(), sizeof(uint2) * A, hipMemcpyHostToDevice));
    if (n > 0) {
        HIP_TRY(b, hipMemcpy(z.gtype, graph_type, n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(z.goal, goal.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    }
    HIP_TRY(b, hipMemset(z.status, 0, sizeof(int) * m));
    HIP_TRY(b, hipMemset(z.info, 0, sizeof(int4) * m));
    HIP_TRY(b, hipMemcpy(q_dev, q_new.data(), sizeof(float2) * q_new.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(c_dev, c_new.data(), c_new.size(), hipMemcpyHostToDevice));
    // nothing can fail from here on but a copy into buffers the batch already owns
    HIP_TRY(b, hipMemcpy(b->modes.off, off_new.data(), 4 * (n + 1), hipMemcpyHostToDevice));
    if (n > 0) HIP_TRY(b, hipMemcpy(b->modes.cursor, cursor.data(), 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(b, hipDeviceSynchronize());                          // (the blocking copies and fills above, whatever stream they ran on)
    b->modes.xy = std::move(q_dev);
    b->modes.cross = std::move(c_dev);
    // the plan kernel's LDS follows the batch's largest graph; its adjacency is staged as far as 64 KiB allow
    int v_max = 0, a_max = 0;
    for (int k = 0; k < B; ++k) {
        v_max = std::max(v_max, node_off[k + 1] - node_off[k]);
        a_max = std::max(a_max, adj_off[node_off[k + 1]] - adj_off[node_off[k]]);
    }
    z.v_cap = std::max(64, (v_max + 63) / 64 * 64);
    z.a_cap = (int)std::min<size_t>((size_t)a_max, (65536 - route_lds_bytes(z.v_cap, 0)) / sizeof(uint2));
    z.capacity = capacity;
    z.wp_off_h = std::move(off_new);
    z.on = true;
    b->routes = std::move(z);
    b->snap.on = false;                                           // (its cursors refer to the old queues)
    return SFM_OK;
}

int sfm_batch_plan_routes(SfmBatch* b, const uint8_t* mask) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->routes.on) return bfail(b, SFM_ERR_STATE, ROUTES_OFF);
    const int B = b->B;
    int chosen = B;
    if (mask) {
        chosen = 0;
        for (int k = 0; k < B; ++k) {
            if (mask[k] > 1) return bfail(b, SFM_ERR_INVALID, "mask must hold 0 or 1 (scene " + std::to_string(k) + ")");
            chosen += mask[k];
        }
    }
    if (chosen == 0) return SFM_OK;
    if (!mask) return batch_plan_routes(b, nullptr, nullptr, B);
    // the restarts' pinned list of chosen scenes, sent and guarded as sfm_batch_restart does
    BatchRestartDev& r = b->restart;
    if (!r.done) {
        HIP_TRY(b, r.list.alloc((size_t)B));
        HIP_TRY(b, r.list_h.alloc((size_t)B));
        HIP_TRY(b, r.done.create(hipEventDisableTiming));
    }
    if (r.pending) {
        HIP_TRY(b, hipEventSynchronize(r.done));
        r.pending = false;
    }
    for (int k = 0, q = 0; k < B; ++k)
        if (mask[k]) r.list_h[q++] = k;
    HIP_TRY(b, hipMemcpyAsync(r.list, r.list_h, sizeof(int) * (size_t)chosen, hipMemcpyHostToDevice, b->stream));
    rc = batch_plan_routes(b, r.list, nullptr, chosen);
    HIP_TRY(b, hipEventRecord(r.done, b->stream));
    r.pending = true;
    return rc;
}

int sfm_batch_plan_routes_device(SfmBatch* b, const uint8_t* d_mask) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->routes.on) return bfail(b, SFM_ERR_STATE, ROUTES_OFF);
    if (!d_mask) {
        if (!b->ep.on) return bfail(b, SFM_ERR_STATE, std::string("d_mask is NULL, which stands for the episodes' done mask, and ") + EPISODES_OFF);
        d_mask = b->ep.done;
    }
    return batch_plan_routes(b, nullptr, d_mask, b->B);
}

int sfm_batch_download_routes(SfmBatch* b, int32_t* status, int32_t* s, int32_t* t, float* cost, int32_t* L, int32_t* wp_offsets,
                              float* wp_x, float* wp_y, uint8_t* wp_crossing) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->routes.on) return bfail(b, SFM_ERR_STATE, ROUTES_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    const BatchRoutesDev& z = b->routes;
    if (wp_offsets) std::copy(z.wp_off_h.begin(), z.wp_off_h.end(), wp_offsets);
    if (n == 0) return SFM_OK;
    if (status) HIP_TRY(b, hipMemcpy(status, z.status, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (s || t || cost || L) {
        std::vector<int4> info(n);
        HIP_TRY(b, hipMemcpy(info.data(), z.info, sizeof(int4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (s) s[i] = info[i].x;
            if (t) t[i] = info[i].y;
            if (L) L[i] = info[i].z;
            if (cost) memcpy(&cost[i], &info[i].w, 4);
        }
    }
    const size_t W = (size_t)z.wp_off_h[n];
    if (W > 0 && (wp_x || wp_y)) {
        std::vector<float2> q(W);
        HIP_TRY(b, hipMemcpy(q.data(), b->modes.xy, sizeof(float2) * W, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < W; ++e) {
            if (wp_x) wp_x[e] = q[e].x;
            if (wp_y) wp_y[e] = q[e].y;
        }
    }
    if (W > 0 && wp_crossing) HIP_TRY(b, hipMemcpy(wp_crossing, b->modes.cross, W, hipMemcpyDeviceToHost));
    return SFM_OK;
}

}  // extern "C"
