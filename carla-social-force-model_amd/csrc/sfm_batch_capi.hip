// sfm_batch_capi.hip -- host side of the batched scenes (ABI 6 and later): B independent crowds on one SfmBatch, ONE launch of
// sfm_batch_tick_kernel per tick (sfm_batch.hip).  The batch's types are in sfm_batch_host.h; the read-only sensors (observations,
// episode ends, range scans) and the device pointers are in sfm_batch_sense_capi.hip.
#include "sfm_batch_host.h"

using namespace sfm;

// one scene's parameters, folded as fill_args folds a handle's
static BatchParams batch_params(const SfmParams& p) {
    BatchParams q;
    memset(&q, 0, sizeof(q));
    q.ped = fold(p.pedestrian);
    q.stat = fold(p.static_obstacle);
    q.dyn = fold(p.dynamic_obstacle);
    q.border_a = p.border_a;
    q.border_nlb = (float)(-1.4426950408889634 / (double)p.border_b);
    q.inv_tau = (float)(1.0 / (double)p.tau);
    q.dt = p.step_length;
    q.max_speed_factor = p.max_speed_factor;
    q.en_acc = p.enabled[SFM_FORCE_ACCELERATION] != 0;
    q.en_ped = p.enabled[SFM_FORCE_PEDESTRIAN] != 0;
    q.en_border = p.enabled[SFM_FORCE_BORDER] != 0;
    q.en_static = p.enabled[SFM_FORCE_STATIC_OBSTACLE] != 0;
    q.en_dynamic = p.enabled[SFM_FORCE_DYNAMIC_OBSTACLE] != 0;
    q.rad = p.use_ped_radius != 0;
    return q;
}

static int check_batch_params(SfmBatch* b, int B, const SfmParams* params) {
    if (!params) return bfail(b, SFM_ERR_INVALID, "params is NULL");
    for (int k = 0; k < B; ++k) {
        const char* why = nullptr;
        if (!check_params(&params[k], &why)) return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": " + why);
    }
    return SFM_OK;
}

// scene_off-style CSR over B entries: off[0] = 0, non-decreasing; *total receives off[B]
static int check_scene_csr(SfmBatch* b, const int32_t* off, const char* name, int max_per_scene, int* total) {
    if (!off) return bfail(b, SFM_ERR_INVALID, std::string(name) + " is NULL");
    if (off[0] != 0) return bfail(b, SFM_ERR_INVALID, std::string(name) + "[0] must be 0");
    for (int k = 0; k < b->B; ++k) {
        if (off[k + 1] < off[k]) return bfail(b, SFM_ERR_INVALID, std::string(name) + " must be non-decreasing (scene " + std::to_string(k) + ")");
        if (max_per_scene > 0 && off[k + 1] - off[k] > max_per_scene)
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + " has " + std::to_string(off[k + 1] - off[k]) +
                                             " pedestrians; a batch takes up to " + std::to_string(max_per_scene) + " per scene (larger crowds belong on a handle)");
    }
    *total = off[b->B];
    return SFM_OK;
}

// the velocities of a steering call: every array that is needed is there, and a steered row's command is finite
static int check_batch_commands(SfmBatch* b, const float4* kinds, const uint8_t* kind, const float* ux, const float* uy, const float* uz) {
    if (b->n_total > 0 && (!ux || !uy)) return bfail(b, SFM_ERR_INVALID, "ux or uy is NULL");
    for (int i = 0; i < b->n_total; ++i) {
        const bool steered = kind ? kind[i] != 0 : kinds[i].w != 0.0f;
        if (steered && !(std::isfinite(ux[i]) && std::isfinite(uy[i]) && (!uz || std::isfinite(uz[i]))))
            return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": the command of a steered row is not finite");
    }
    return SFM_OK;
}

// What the drops take along: the tracks refer to the boxes, the spawn schedule to the modes.  (The caller synchronised the stream.)
static void drop_batch_boxes(SfmBatch* b) {
    drop_noise_delays(b);
    b->tracks = {};
    b->drive = {};                                                // (the commands and the vehicle observations are per vehicle)
    b->vobs = {};
    b->vscan = {};                                                // (... and so are the vehicles' range scans)
    b->boxes = {};                                                // (with the vehicles' grids, which live inside)
}

static void drop_batch_modes(SfmBatch* b) {
    b->spawns = {};
    b->spawn_used = false;
    b->routes = {};                                               // (a route is walked as a mode queue)
    b->modes = {};
}

// one kind of per-scene CSR polylines; ctr4[K] built by the caller
static int set_batch_geo(SfmBatch* b, int kind, const int32_t* scene_item_off, const int32_t* offsets, const float* px, const float* py,
                         const std::vector<float4>& ctr4, int K) {
    BatchGeoDev& g = b->geo[kind];
    const int P = K > 0 ? offsets[K] : 0;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still read the arrays
    g = {};
    HIP_TRY(b, hipMemcpy(b->geo_item_off[kind], scene_item_off, sizeof(int) * ((size_t)b->B + 1), hipMemcpyHostToDevice));
    if (K == 0) return SFM_OK;
    std::vector<float2> pts((size_t)(P > 0 ? P : 1));
    for (int p = 0; p < P; ++p) pts[p] = make_float2(px[p], py[p]);
    HIP_TRY(b, g.off.alloc((size_t)K + 1));
    HIP_TRY(b, g.pts.alloc(pts.size()));
    HIP_TRY(b, g.ctr.alloc((size_t)K));
    HIP_TRY(b, hipMemcpy(g.off, offsets, sizeof(int) * ((size_t)K + 1), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(g.pts, pts.data(), sizeof(float2) * pts.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(g.ctr, ctr4.data(), sizeof(float4) * (size_t)K, hipMemcpyHostToDevice));
    g.K = K;
    g.P = P;
    return SFM_OK;
}

// validation shared by the three geometry calls: *K = polylines over all scenes
static int check_batch_geo(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px, const float* py,
                           const float* cx, const float* cy, int* K) {
    int rc = check_scene_csr(b, scene_item_off, "scene_item_off", 0, K);
    if (rc) return rc;
    if (*K == 0) return SFM_OK;
    if (!offsets) return bfail(b, SFM_ERR_INVALID, "offsets is NULL");
    if (offsets[0] != 0) return bfail(b, SFM_ERR_INVALID, "offsets[0] must be 0");
    for (int k = 0; k < *K; ++k)
        if (offsets[k + 1] < offsets[k]) return bfail(b, SFM_ERR_INVALID, "offsets must be non-decreasing");
    if (offsets[*K] > 0 && (!px || !py)) return bfail(b, SFM_ERR_INVALID, "point arrays are NULL");
    if (!cx || !cy) return bfail(b, SFM_ERR_INVALID, "centre arrays are NULL");
    return SFM_OK;
}

// flags a batch tick takes: SFM_TICK_INTEGRATE, and SFM_TICK_REDRAW_WAYPOINTS once the streams are set and while no modes are
int sfm::check_batch_flags(SfmBatch* b, uint32_t flags, const char* what) {
    if (b->modes.on && (flags & ~(uint32_t)SFM_TICK_INTEGRATE))
        return bfail(b, SFM_ERR_INVALID, std::string("a batch ") + what + " with modes set (sfm_batch_set_mode_fsm) takes SFM_TICK_INTEGRATE "
                                         "only: arrivals pop the waypoint queues, so SFM_TICK_REDRAW_WAYPOINTS does not apply");
    const uint32_t ok = SFM_TICK_INTEGRATE | (b->d_streams ? (uint32_t)SFM_TICK_REDRAW_WAYPOINTS : 0u);
    if (flags & ~ok)
        return bfail(b, SFM_ERR_INVALID, std::string("a batch ") + what + " takes SFM_TICK_INTEGRATE only, and "
                                         "SFM_TICK_REDRAW_WAYPOINTS once sfm_batch_set_waypoint_streams has been called");
    return SFM_OK;
}

// force mask -> the kernel's packed slot word (nibble k: slot of force k in index order, 15: not recorded) and K = popcount(mask)
static int batch_force_slots(SfmBatch* b, uint32_t force_mask, uint32_t* slots, int* K) {
    if (force_mask == 0 || (force_mask & ~0x3Fu))
        return bfail(b, SFM_ERR_INVALID, "force_mask must select forces 0..5 (bit k = SFM_FORCE_* index k, bit 5 = SFM_FORCE_TOTAL) "
                                         "and at least one of them");
    uint32_t w = 0xFFFFFFFFu;
    int k = 0;
    for (int f = 0; f <= SFM_FORCE_TOTAL; ++f)
        if (force_mask & (1u << f)) w = (w & ~(15u << (4 * f))) | ((uint32_t)k++ << (4 * f));
    *slots = w;
    *K = k;
    return SFM_OK;
}

// one tick of the whole batch; frame / zframe: this tick's frame slot of a recorded run (null: not recorded); force_rec: this
// tick's [K][N_total][C] force record with force_slots from batch_force_slots (null: not recorded)
int sfm::batch_launch(SfmBatch* b, uint32_t flags, float4* frame, float2* zframe, float* force_rec, uint32_t force_slots) {
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    a.scene_off = b->d_scene_off;
    a.prm = b->d_prm;
    a.pk = b->pk;
    a.zv = b->z3 ? b->zv : nullptr;
    a.own = b->own;
    a.crossing = b->crossing;
    for (int k = 0; k < 3; ++k) a.geo[k] = batch_geo(b, k);
    a.flags = flags;
    a.streams = b->d_streams;
    a.draws = b->draws;
    a.frame = frame;
    a.zframe = b->z3 ? zframe : nullptr;
    const bool move = b->boxes.on && (flags & SFM_TICK_INTEGRATE);
    if (move) {
        a.veh_ctr_out = b->boxes.ctr_alt;
        a.veh_pts_out = b->boxes.pts_alt;
        a.veh_local = b->boxes.local;
        a.veh_rot = b->boxes.rot;
        a.veh_on = 1;
        if (b->tracks.on) a.trk = BatchTracks{b->tracks.off, b->tracks.first, b->tracks.key, b->tracks.rot, b->tracks.tick + 1};   // this launch writes tick tau + 1
        if (b->drive.on && b->geo[2].K > 0) {                    // (no vehicles: no command buffer, and nobody to drive)
            a.veh_cmd = b->drive.cmd;
            a.veh_head = b->boxes.rot;
        }
    }
    if (b->modes.on)
        a.fsm = BatchModes{b->modes.mode, b->modes.target, b->modes.speeds, b->modes.off, b->modes.xy, b->modes.cross, b->modes.cursor, b->modes.scene, b->modes.time};
    a.force_rec = force_rec;
    a.force_n = b->n_total;
    a.force_slots = force_slots;
    if (b->spawns.on) a.spn = BatchSpawn{b->spawns.time, b->spawns.chain, b->spawns.born, b->spawns.birth, b->spawns.pk0, b->spawns.zv0};
    const bool steer = b->steer.on && b->n_total > 0;            // (no rows: no command buffer, and nobody to steer)
    if (steer) a.cmd = b->steer.cmd;
    const bool ext = (flags & SFM_TICK_REDRAW_WAYPOINTS) || frame || force_rec;
    if (move && b->drive.ap.on) {                                // the autopilot writes this tick's commands from what this tick reads
        const int rc = batch_autopilot_launch(b);
        if (rc) return rc;
    }
    HIP_TRY(b, launch_batch_tick(b->z3, ext, b->modes.on, b->modes.on && b->spawns.on, steer, a, b->B, b->stream));
    if (move) {                                          // the moved half is what the next tick sees
        swap(b->geo[2].ctr, b->boxes.ctr_alt);
        swap(b->geo[2].pts, b->boxes.pts_alt);
        if (b->tracks.on) ++b->tracks.tick;
    }
    return SFM_OK;
}

// One array into its snapshot copy, on the batch's stream.  The copy only grows, and only then does the host wait: a restart in
// flight may still read the buffer that is replaced.
template <typename T>
static int snap_copy(SfmBatch* b, DevBuf<T>& s, const DevBuf<T>& src, size_t count) {
    if (count == 0) return SFM_OK;
    if (!s || count > s.cap()) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        HIP_TRY(b, s.reserve(count));
    }
    HIP_TRY(b, hipMemcpyAsync(s, src, sizeof(T) * count, hipMemcpyDeviceToDevice, b->stream));
    return SFM_OK;
}

// The host's copy of the tracks' first ticks, current: after a restart by device mask it is read back from the device (the
// callers synchronise anyway).
static int refresh_track_first(SfmBatch* b) {
    if (!b->tracks.on || !b->tracks.first_stale) return SFM_OK;
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t M = (size_t)b->geo[2].K;
    if (M > 0) HIP_TRY(b, hipMemcpy(b->tracks.first_h.data(), b->tracks.first, sizeof(int) * M, hipMemcpyDeviceToHost));
    b->tracks.first_stale = false;
    return SFM_OK;
}

// The restart kernel's arguments but for the choice of scenes (list / mask): every live array beside its snapshot copy.
static BatchRestart restart_args(SfmBatch* b, long long shift) {
    BatchRestart r;
    memset(&r, 0, sizeof(r));
    r.scene_off = b->d_scene_off;
    r.pk = b->pk; r.s_pk = b->snap.pk;
    if (b->z3) { r.zv = b->zv; r.s_zv = b->snap.zv; }
    r.own = b->own; r.s_own = b->snap.own;
    r.draws = b->draws; r.s_draws = b->snap.draws;
    if (b->boxes.on) {
        const BatchGeoDev& g = b->geo[2];
        r.item_off = b->geo_item_off[2]; r.veh_off = g.off;
        r.ctr = g.ctr; r.s_ctr = b->snap.ctr;
        r.pts = g.P > 0 ? g.pts : nullptr; r.s_pts = b->snap.pts;
        r.rot = b->boxes.rot; r.s_rot = b->snap.rot;
    }
    if (b->modes.on) {
        r.mode = b->modes.mode; r.s_mode = b->snap.mode;
        r.target = b->modes.target; r.s_target = b->snap.target;
        r.cursor = b->modes.cursor; r.s_cursor = b->snap.cursor;
        r.sim_time = b->modes.time; r.s_sim_time = b->snap.time;
    }
    if (b->spawns.on) {
        r.born = b->spawns.born; r.s_born = b->snap.born;
        r.birth_time = b->spawns.birth; r.s_birth_time = b->snap.birth;
    }
    if (b->tracks.on) {
        r.first = b->tracks.first; r.s_first = b->snap.first;
        r.trk_off = b->tracks.off;
        r.shift = shift;
    }
    if (b->n_total == 0) { r.pk = nullptr; r.own = nullptr; r.draws = nullptr; r.zv = nullptr; r.mode = nullptr; r.target = nullptr;
                           r.cursor = nullptr; r.born = nullptr; r.birth_time = nullptr; }      // (no rows: no snapshot arrays either)
    if (b->ep.on) { r.age = b->ep.age; r.prev_goal_d2 = b->ep.prev; }  // a restarted scene's episode starts over
    return r;
}

int sfm::batch_restart_checks(SfmBatch* b, const uint8_t* mask, const std::string& bad_choice, long long* shift) {
    if (!b->snap.on) return bfail(b, SFM_ERR_STATE, NO_SNAPSHOT);
    if (!bad_choice.empty()) return bfail(b, SFM_ERR_INVALID, bad_choice);
    // track time per scene: the chosen scenes' tracked vehicles are found by tau at the keyframe the snapshot had them at
    *shift = b->tracks.on ? b->tracks.tick - b->snap.tick : 0;
    if (!b->tracks.on) return SFM_OK;
    for (int k = 0; k < b->B; ++k) {
        if (mask && !mask[k]) continue;
        for (int v = b->boxes.item_off_h[k]; v < b->boxes.item_off_h[k + 1]; ++v) {
            const long long first = (long long)b->snap.first_h[v] + *shift;
            if (b->tracks.off_h[v + 1] > b->tracks.off_h[v] && (first < INT32_MIN || first + b->noise.max_delay > INT32_MAX))
                return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ", vehicle " + std::to_string(v) + ": its first tick moved by the " +
                                                 std::to_string(*shift) + " ticks since the snapshot" +
                                                 (b->noise.max_delay ? " and by the largest delay of the restart noise, " + std::to_string(b->noise.max_delay) + "," : "") +
                                                 " does not fit int32: set the tracks "
                                                 "again (sfm_batch_set_vehicle_tracks restarts the tick counter)");
        }
    }
    return SFM_OK;
}

// sfm_batch_restart_device after its checks: ONE launch of B workgroups, the choice read on the device
int sfm::batch_restart_device(SfmBatch* b, const uint8_t* d_mask, long long shift) {
    BatchRestart r = restart_args(b, shift);
    r.mask = d_mask;
    HIP_TRY(b, launch_batch_restart(r, b->B, b->stream));
    if (b->tracks.on) b->tracks.first_stale = true;                     // who was chosen is known on the device only
    int rc = batch_restart_noise(b, nullptr, d_mask, b->B);
    if (!rc) rc = batch_plan_routes(b, nullptr, d_mask, b->B);          // (routes: from where the rows were placed)
    if (!rc) rc = batch_autopilot_restart(b, nullptr, d_mask, b->B);    // (the autopilot's cursors)
    if (!rc) rc = batch_row_restart(b, nullptr, d_mask, b->B);          // (the row episodes start over)
    return rc ? rc : batch_vehicle_episode_restart(b, nullptr, d_mask, b->B);   // (... and the vehicle episodes)
}

// sfm_batch_run_recorded, and with want_forces also the [F][K][N_total][C] force record of every recorded tick
static int batch_run_recorded(SfmBatch* b, int ticks, uint32_t flags, int stride, float* frames, float* zframes, int max_frames,
                              int* n_frames, bool want_forces, uint32_t force_mask, float* forces) {
    int rc = bbind(b);
    if (rc) return rc;
    if (ticks < 0 || stride <= 0 || max_frames < 0) return bfail(b, SFM_ERR_INVALID, "ticks < 0, stride <= 0 or max_frames < 0");
    if (!n_frames) return bfail(b, SFM_ERR_INVALID, "n_frames is NULL");
    *n_frames = 0;
    uint32_t slots = 0xFFFFFFFFu;
    int K = 0;
    if (want_forces) {
        rc = batch_force_slots(b, force_mask, &slots, &K);
        if (rc) return rc;
    }
    rc = check_batch_flags(b, flags, "recorded run");
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (zframes && !b->z3) return bfail(b, SFM_ERR_INVALID, "zframes on a planar batch (it has no z / vz to record)");
    const int F = (int)std::min<long long>(max_frames, ((long long)ticks + stride - 1) / stride);
    if (F > 0 && !frames) return bfail(b, SFM_ERR_INVALID, "frames is NULL");
    if (F > 0 && want_forces && !forces) return bfail(b, SFM_ERR_INVALID, "forces is NULL");
    const size_t n = (size_t)b->n_total;
    const size_t recs = n * (size_t)F;
    const size_t fvals = recs * (size_t)K * (b->z3 ? 3 : 2);          // per frame [K][N_total][C]
    const size_t bytes = recs * (sizeof(float4) + (zframes ? sizeof(float2) : 0)) + fvals * sizeof(float);
    if (bytes > SFM_BATCH_MAX_RECORD_BYTES)
        return bfail(b, SFM_ERR_INVALID, std::string("the frames ") + (want_forces ? "and forces " : "") + "of this call need " +
                                         std::to_string(bytes) + " bytes, more than the " +
                                         std::to_string((unsigned long long)SFM_BATCH_MAX_RECORD_BYTES) +
                                         " one call may record: split the run into several " +
                                         (want_forces ? "sfm_batch_run_recorded_forces" : "sfm_batch_run_recorded") + " calls");
    if (recs > 0) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a tick in flight may still write the old buffers
        HIP_TRY(b, b->rec.frames.reserve(recs));
        if (zframes) HIP_TRY(b, b->rec.zframes.reserve(recs));
        if (fvals > 0) HIP_TRY(b, b->rec.forces.reserve(fvals));
    }
    const size_t fstride = fvals / (F > 0 ? (size_t)F : 1);
    for (int t = 0, f = 0; t < ticks; ++t) {
        const bool rec = t % stride == 0 && f < F && recs > 0;
        rc = batch_launch(b, flags | SFM_TICK_INTEGRATE, rec ? b->rec.frames + n * (size_t)f : nullptr,
                          rec && zframes ? b->rec.zframes + n * (size_t)f : nullptr,
                          rec && fvals > 0 ? b->rec.forces + fstride * (size_t)f : nullptr, slots);
        if (rc) return rc;
        if (t % stride == 0) ++f;
    }
    if (recs > 0) {
        HIP_TRY(b, hipMemcpyAsync(frames, b->rec.frames, sizeof(float4) * recs, hipMemcpyDeviceToHost, b->stream));
        if (zframes) HIP_TRY(b, hipMemcpyAsync(zframes, b->rec.zframes, sizeof(float2) * recs, hipMemcpyDeviceToHost, b->stream));
        if (fvals > 0) HIP_TRY(b, hipMemcpyAsync(forces, b->rec.forces, sizeof(float) * fvals, hipMemcpyDeviceToHost, b->stream));
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    *n_frames = F;
    return SFM_OK;
}

extern "C" {

int sfm_batch_create(int B, const SfmParams* params, int device_id, SfmBatch** out) {
    if (!out) return bfail(nullptr, SFM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1) return bfail(nullptr, SFM_ERR_INVALID, "B must be >= 1");
    int rc = check_batch_params(nullptr, B, params);
    if (rc) return rc;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return bfail(nullptr, SFM_ERR_NO_DEVICE, "no HIP device visible (libsfm_hip needs an MI355X)");
    if (device_id < 0 || device_id >= ndev) return bfail(nullptr, SFM_ERR_INVALID, "device_id out of range");
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return bfail(nullptr, SFM_ERR_HIP, hipGetErrorString(e));
    SfmBatch* b = new SfmBatch();
    b->device = device_id;
    b->B = B;
    std::vector<BatchParams> q((size_t)B);
    for (int k = 0; k < B; ++k) q[k] = batch_params(params[k]);
    for (int k = 0; k < B; ++k) b->dt_h.push_back(params[k].step_length);
    std::vector<int> zeros((size_t)B + 1, 0);
    bool ok = b->d_prm.alloc((size_t)B) == hipSuccess && b->d_scene_off.alloc((size_t)B + 1) == hipSuccess &&
              hipMemcpy(b->d_prm, q.data(), sizeof(BatchParams) * (size_t)B, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(b->d_scene_off, zeros.data(), sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice) == hipSuccess;
    for (int k = 0; k < 3 && ok; ++k)
        ok = b->geo_item_off[k].alloc((size_t)B + 1) == hipSuccess &&
             hipMemcpy(b->geo_item_off[k], zeros.data(), sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice) == hipSuccess;
    for (int k = 0; k < B && ok; ++k) b->any_rad = b->any_rad || params[k].use_ped_radius != 0;
    if (!ok) {
        sfm_batch_destroy(b);
        return bfail(nullptr, SFM_ERR_HIP, "device allocation for the batch failed");
    }
    *out = b;
    return SFM_OK;
}

int sfm_batch_destroy(SfmBatch* b) {
    if (!b) return SFM_ERR_INVALID;
    hipSetDevice(b->device);
    hipStreamSynchronize(b->stream);
    delete b;
    return SFM_OK;
}

int sfm_batch_set_stream(SfmBatch* b, void* hip_stream) {
    if (!b) return SFM_ERR_INVALID;
    b->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return SFM_OK;
}

int sfm_batch_set_params(SfmBatch* b, const SfmParams* params) {
    int rc = bbind(b);
    if (rc) return rc;
    rc = check_batch_params(b, b->B, params);
    if (rc) return rc;
    bool any_rad = false;
    for (int k = 0; k < b->B; ++k) any_rad = any_rad || params[k].use_ped_radius != 0;
    if (any_rad && b->have_state && b->n_total > 0 && !b->any_rad)
        return bfail(b, SFM_ERR_STATE, "use_ped_radius on a batch whose state was uploaded without radii: upload the state again");
    std::vector<BatchParams> q((size_t)b->B);
    for (int k = 0; k < b->B; ++k) q[k] = batch_params(params[k]);
    std::vector<float> dt((size_t)b->B);
    for (int k = 0; k < b->B; ++k) dt[k] = params[k].step_length;
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if ((rc = batch_replay_step_lengths(b, dt.data()))) return rc;  // (observed tracks: 1 / (every * step_length) follows)
    HIP_TRY(b, hipMemcpy(b->d_prm, q.data(), sizeof(BatchParams) * (size_t)b->B, hipMemcpyHostToDevice));
    b->dt_h = dt;
    b->any_rad = any_rad;
    return SFM_OK;
}

int sfm_batch_upload_state(SfmBatch* b, const int32_t* scene_off, const float* x, const float* y, const float* z,
                           const float* vx, const float* vy, const float* vz, const float* wx, const float* wy,
                           const float* target_speed, const float* radius, const uint8_t* crossing_mask) {
    int rc = bbind(b);
    if (rc) return rc;
    int N = 0;
    rc = check_scene_csr(b, scene_off, "scene_off", BATCH_MAX_N, &N);
    if (rc) return rc;
    if (N > 0 && (!x || !y || !vx || !vy || !wx || !wy || !target_speed))
        return bfail(b, SFM_ERR_INVALID, "a required state array is NULL");
    if ((z == nullptr) != (vz == nullptr)) return bfail(b, SFM_ERR_INVALID, "z and vz must be given together");
    if (b->any_rad && N > 0 && !radius) return bfail(b, SFM_ERR_INVALID, "use_ped_radius needs radius");
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)N;
    if (n > b->draws.cap()) {                                    // (allocated last: it grew only if the other four did)
        HIP_TRY(b, b->pk.alloc(n));
        HIP_TRY(b, b->zv.alloc(n));
        HIP_TRY(b, b->own.alloc(n));
        HIP_TRY(b, b->crossing.alloc(n));
        HIP_TRY(b, b->draws.alloc(n));
    }
    drop_batch_modes(b);                                          // a new crowd: its modes are set anew
    b->steer = {};                                                // ... and so are its commands (the rows may differ)
    b->obs = {};                                                  // ... and its observations
    b->ep = {};                                                   // ... and its episodes, per scene and per row (the agents are rows)
    b->scan = {};                                                 // ... and its scans (the mask is per row)
    b->noise = {};                                                // ... and its restart noise (the boxes are per row)
    b->grid = {};                                                 // ... and its grids (the slots are per row)
    b->replay = {};                                               // ... and its observed tracks (the roles are per row)
    b->vscan = {};                                                // ... and the vehicles' scans of it
    b->boxes.vgrid = {};                                          // ... and the vehicles' grids of it
    b->boxes.vep = {};                                            // ... and the vehicles' episodes (whatever drops the grids drops them)
    b->snap.on = false;                                           // ... and so is its snapshot
    b->have_state = false;
    if (n > 0) {
        std::vector<float4> pk(n), own(n);
        std::vector<float2> zv(n);
        std::vector<uint8_t> cm(n);
        for (size_t i = 0; i < n; ++i) {
            pk[i] = make_float4(x[i], y[i], vx[i], vy[i]);
            own[i] = make_float4(wx[i], wy[i], target_speed[i], radius ? radius[i] : 0.f);
            zv[i] = z ? make_float2(z[i], vz[i]) : make_float2(0.f, 0.f);
            cm[i] = crossing_mask ? (crossing_mask[i] != 0) : 0;
        }
        HIP_TRY(b, hipMemcpy(b->pk, pk.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->zv, zv.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->own, own.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->crossing, cm.data(), n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemset(b->draws, 0, sizeof(uint32_t) * n));
    }
    HIP_TRY(b, hipMemcpy(b->d_scene_off, scene_off, sizeof(int) * ((size_t)b->B + 1), hipMemcpyHostToDevice));
    b->scene_off_h.assign(scene_off, scene_off + b->B + 1);
    b->n_total = N;
    b->z3 = z != nullptr;
    b->have_state = true;
    return SFM_OK;
}

int sfm_batch_set_borders(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px, const float* py,
                          const float* cx, const float* cy, const float* cull_len) {
    int rc = bbind(b);
    if (rc) return rc;
    int K = 0;
    rc = check_batch_geo(b, scene_item_off, offsets, px, py, cx, cy, &K);
    if (rc) return rc;
    if (K > 0 && !cull_len) return bfail(b, SFM_ERR_INVALID, "border length array is NULL");
    std::vector<float4> c4((size_t)K);
    for (int k = 0; k < K; ++k) c4[k] = make_float4(cx[k], cy[k], (float)((double)cull_len[k] * (double)cull_len[k]), 0.f);
    return set_batch_geo(b, 0, scene_item_off, offsets, px, py, c4, K);
}

int sfm_batch_set_static_obstacles(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px,
                                   const float* py, const float* cx, const float* cy) {
    int rc = bbind(b);
    if (rc) return rc;
    int K = 0;
    rc = check_batch_geo(b, scene_item_off, offsets, px, py, cx, cy, &K);
    if (rc) return rc;
    std::vector<float4> c4((size_t)K);
    for (int k = 0; k < K; ++k) c4[k] = make_float4(cx[k], cy[k], 0.f, 0.f);
    return set_batch_geo(b, 1, scene_item_off, offsets, px, py, c4, K);
}

int sfm_batch_set_dynamic_obstacles(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px,
                                    const float* py, const float* cx, const float* cy, const float* vx, const float* vy) {
    int rc = bbind(b);
    if (rc) return rc;
    int K = 0;
    rc = check_batch_geo(b, scene_item_off, offsets, px, py, cx, cy, &K);
    if (rc) return rc;
    if ((vx == nullptr) != (vy == nullptr)) return bfail(b, SFM_ERR_INVALID, "vx and vy must be given together");
    std::vector<float4> c4((size_t)K);
    for (int k = 0; k < K; ++k)       // velocities default to 0 like ObstacleForce (forces.py:212-213)
        c4[k] = make_float4(cx[k], cy[k], vx ? vx[k] : 0.f, vy ? vy[k] : 0.f);
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still move the boxes
    drop_batch_boxes(b);
    b->snap.on = false;
    return set_batch_geo(b, 2, scene_item_off, offsets, px, py, c4, K);
}

// Device-side vehicles (ABI 8), the batch form of sfm_set_dynamic_boxes: geo[2] holds the current half (its pts the world-frame rings),
// the rings of the given centres are generated by one launch of sfm_dynamic_boxes_kernel over every vehicle of the batch
int sfm_batch_set_dynamic_boxes(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* ux, const float* uy,
                                const float* cx, const float* cy, const float* yaw_cos, const float* yaw_sin, const float* vx,
                                const float* vy) {
    int rc = bbind(b);
    if (rc) return rc;
    int M = 0;
    rc = check_batch_geo(b, scene_item_off, offsets, ux, uy, cx, cy, &M);
    if (rc) return rc;
    if (M > 0 && (!yaw_cos || !yaw_sin)) return bfail(b, SFM_ERR_INVALID, "yaw arrays are NULL");
    if ((vx == nullptr) != (vy == nullptr)) return bfail(b, SFM_ERR_INVALID, "vx and vy must be given together");
    std::vector<float4> c4((size_t)M);
    std::vector<float2> rot((size_t)M);
    for (int k = 0; k < M; ++k) {     // velocities default to 0 like ObstacleForce (forces.py:212-213)
        c4[k] = make_float4(cx[k], cy[k], vx ? vx[k] : 0.f, vy ? vy[k] : 0.f);
        rot[k] = make_float2(yaw_cos[k], yaw_sin[k]);
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still move the old boxes
    drop_batch_boxes(b);
    b->snap.on = false;
    rc = set_batch_geo(b, 2, scene_item_off, offsets, ux, uy, c4, M);   // pts holds the local offsets until the launch below
    if (rc || M == 0) return rc;
    BatchGeoDev& g = b->geo[2];
    const size_t np = (size_t)(g.P > 0 ? g.P : 1);               // set_batch_geo's sizes: both halves alike
    HIP_TRY(b, b->boxes.local.alloc(np));
    HIP_TRY(b, b->boxes.rot.alloc((size_t)M));
    HIP_TRY(b, b->boxes.ctr_alt.alloc((size_t)M));
    HIP_TRY(b, b->boxes.pts_alt.alloc(np));
    HIP_TRY(b, hipMemcpy(b->boxes.local, g.pts, sizeof(float2) * np, hipMemcpyDeviceToDevice));
    HIP_TRY(b, hipMemcpy(b->boxes.rot, rot.data(), sizeof(float2) * (size_t)M, hipMemcpyHostToDevice));
    HIP_TRY(b, launch_dynamic_boxes(g.ctr, g.off, b->boxes.local, b->boxes.rot, g.pts, M, 0.f, 0, b->stream));
    b->boxes.item_off_h.assign(scene_item_off, scene_item_off + b->B + 1);
    b->boxes.on = true;
    return SFM_OK;
}

// Scripted vehicle tracks (ABI 12): everything is checked before anything is sent; the tracked vehicles are placed for tau = 0 by
// one launch of sfm_batch_place_tracks_kernel into the current half, in place
int sfm_batch_set_vehicle_tracks(SfmBatch* b, const int32_t* trk_off, const int32_t* first_tick, const float* kx, const float* ky,
                                 const float* kvx, const float* kvy, const float* kcos, const float* ksin) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->boxes.on)
        return bfail(b, SFM_ERR_STATE, "vehicle tracks need device-side vehicles: call sfm_batch_set_dynamic_boxes first");
    if (!trk_off) {                                              // tracks off: the vehicles run free from where they are
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        drop_noise_delays(b);
        b->tracks = {};
        b->snap.on = false;
        return SFM_OK;
    }
    const int M = b->geo[2].K;
    if (trk_off[0] != 0) return bfail(b, SFM_ERR_INVALID, "trk_off[0] must be 0");
    for (int k = 0; k < M; ++k) {
        if (trk_off[k + 1] < trk_off[k]) return bfail(b, SFM_ERR_INVALID, "trk_off must be non-decreasing (vehicle " + std::to_string(k) + ")");
        if (trk_off[k + 1] > SFM_BATCH_MAX_TRACK_KEYS)
            return bfail(b, SFM_ERR_INVALID, "the tracks hold more than " + std::to_string(SFM_BATCH_MAX_TRACK_KEYS) +
                                             " keyframes (SFM_BATCH_MAX_TRACK_KEYS): set shorter tracks and set them again later");
    }
    const int T = trk_off[M];
    if (T > 0 && (!first_tick || !kx || !ky || !kvx || !kvy || !kcos || !ksin))
        return bfail(b, SFM_ERR_INVALID, "first_tick or a keyframe array is NULL while a track has keyframes");
    for (const float* col : {kx, ky, kvx, kvy, kcos, ksin})
        for (int e = 0; e < T; ++e)
            if (!std::isfinite(col[e])) return bfail(b, SFM_ERR_INVALID, "keyframe " + std::to_string(e) + " holds a value that is not finite");
    std::vector<float4> key((size_t)(T > 0 ? T : 1));
    std::vector<float2> rot(key.size());
    for (int e = 0; e < T; ++e) {
        key[e] = make_float4(kx[e], ky[e], kvx[e], kvy[e]);
        rot[e] = make_float2(kcos[e], ksin[e]);
    }
    std::vector<int32_t> first((size_t)M, 0);
    if (first_tick) first.assign(first_tick, first_tick + M);
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still read the old tracks
    drop_noise_delays(b);
    b->tracks = {};
    b->snap.on = false;
    HIP_TRY(b, b->tracks.off.alloc((size_t)M + 1));
    HIP_TRY(b, b->tracks.first.alloc((size_t)M));
    HIP_TRY(b, b->tracks.key.alloc(key.size()));
    HIP_TRY(b, b->tracks.rot.alloc(rot.size()));
    HIP_TRY(b, hipMemcpy(b->tracks.off, trk_off, sizeof(int) * ((size_t)M + 1), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->tracks.first, first.data(), sizeof(int) * (size_t)M, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->tracks.key, key.data(), sizeof(float4) * key.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->tracks.rot, rot.data(), sizeof(float2) * rot.size(), hipMemcpyHostToDevice));
    b->tracks.off_h.assign(trk_off, trk_off + M + 1);
    b->tracks.first_h = first;
    b->tracks.tick = 0;
    const BatchGeoDev& g = b->geo[2];
    if (T > 0)
        HIP_TRY(b, launch_batch_place_tracks(BatchTracks{b->tracks.off, b->tracks.first, b->tracks.key, b->tracks.rot, 0}, g.off, b->boxes.local, g.ctr, g.pts, M,
                                             b->stream));
    b->tracks.on = true;
    return SFM_OK;
}

int sfm_batch_download_vehicle_tracks(SfmBatch* b, int64_t* tick, uint8_t* present) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->tracks.on) return bfail(b, SFM_ERR_STATE, "no vehicle tracks are set (sfm_batch_set_vehicle_tracks)");
    if ((rc = refresh_track_first(b))) return rc;
    if (tick) *tick = (int64_t)b->tracks.tick;
    const int M = b->geo[2].K;
    for (int k = 0; present && k < M; ++k) {
        const long long L = b->tracks.off_h[k + 1] - b->tracks.off_h[k], j = b->tracks.tick - (long long)b->tracks.first_h[k];
        present[k] = L == 0 || (j >= 0 && j < L);                // (a vehicle without keyframes runs free: always there)
    }
    return SFM_OK;
}

int sfm_batch_download_dynamic_obstacles(SfmBatch* b, float* cx, float* cy, float* px, float* py) {
    int rc = bbind(b);
    if (rc) return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const BatchGeoDev& g = b->geo[2];
    const int M = g.K, P = g.P;
    if (M == 0) return SFM_OK;
    std::vector<float4> c((size_t)M);
    std::vector<float2> p((size_t)(P > 0 ? P : 1));
    HIP_TRY(b, hipMemcpy(c.data(), g.ctr, sizeof(float4) * (size_t)M, hipMemcpyDeviceToHost));
    if (P > 0) HIP_TRY(b, hipMemcpy(p.data(), g.pts, sizeof(float2) * (size_t)P, hipMemcpyDeviceToHost));
    for (int k = 0; k < M; ++k) { if (cx) cx[k] = c[k].x; if (cy) cy[k] = c[k].y; }
    for (int q = 0; q < P; ++q) { if (px) px[q] = p[q].x; if (py) py[q] = p[q].y; }
    return SFM_OK;
}

int sfm_batch_tick(SfmBatch* b, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    rc = check_batch_flags(b, flags, "tick");
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    return batch_launch(b, flags);
}

int sfm_batch_tick_forces(SfmBatch* b, uint32_t flags, uint32_t force_mask, float* forces) {
    int rc = bbind(b);
    if (rc) return rc;
    uint32_t slots = 0;
    int K = 0;
    rc = batch_force_slots(b, force_mask, &slots, &K);
    if (rc) return rc;
    if (!forces) return bfail(b, SFM_ERR_INVALID, "forces is NULL");
    rc = check_batch_flags(b, flags, "tick");
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    const size_t vals = (size_t)K * (size_t)b->n_total * (b->z3 ? 3 : 2);
    if (vals > 0) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a tick in flight may still write the old buffer
        HIP_TRY(b, b->rec.forces.reserve(vals));
    }
    rc = batch_launch(b, flags, nullptr, nullptr, vals > 0 ? b->rec.forces : nullptr, slots);
    if (rc) return rc;
    if (vals > 0) HIP_TRY(b, hipMemcpyAsync(forces, b->rec.forces, sizeof(float) * vals, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return SFM_OK;
}

int sfm_batch_run(SfmBatch* b, int ticks, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    if (ticks < 0) return bfail(b, SFM_ERR_INVALID, "ticks < 0");
    rc = check_batch_flags(b, flags, "run");
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    for (int t = 0; t < ticks; ++t) {
        rc = batch_launch(b, flags | SFM_TICK_INTEGRATE);
        if (rc) return rc;
    }
    return SFM_OK;
}

int sfm_batch_download_state(SfmBatch* b, float* x, float* y, float* z, float* vx, float* vy, float* vz) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n == 0) return SFM_OK;
    std::vector<float4> pk(n);
    HIP_TRY(b, hipMemcpy(pk.data(), b->pk, sizeof(float4) * n, hipMemcpyDeviceToHost));
    std::vector<float2> zv;
    if (b->z3 && (z || vz)) {
        zv.resize(n);
        HIP_TRY(b, hipMemcpy(zv.data(), b->zv, sizeof(float2) * n, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; ++i) {
        if (x) x[i] = pk[i].x;
        if (y) y[i] = pk[i].y;
        if (vx) vx[i] = pk[i].z;
        if (vy) vy[i] = pk[i].w;
        if (b->z3) {
            if (z) z[i] = zv[i].x;
            if (vz) vz[i] = zv[i].y;
        } else if (vz) {
            vz[i] = 0.f;
        }
    }
    return SFM_OK;
}

int sfm_batch_set_waypoint_streams(SfmBatch* b, const uint32_t* seed, const float* world_side, const float* arrive_threshold) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!seed || !world_side || !arrive_threshold) return bfail(b, SFM_ERR_INVALID, "a waypoint stream array is NULL");
    std::vector<BatchStream> q((size_t)b->B);
    for (int k = 0; k < b->B; ++k) {
        const float side = world_side[k], thr = arrive_threshold[k];
        if (!std::isfinite(side) || side < 0.f || !std::isfinite(thr) || thr < 0.f)
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": world_side and arrive_threshold must be finite and >= 0");
        q[k] = BatchStream{seed[k], side, (float)((double)thr * (double)thr), 0.f};   // thr^2 as the handle rounds it
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still read the table
    if (!b->d_streams) {
        DevBuf<BatchStream> p;
        HIP_TRY(b, p.alloc((size_t)b->B));
        HIP_TRY(b, hipMemcpy(p, q.data(), sizeof(BatchStream) * (size_t)b->B, hipMemcpyHostToDevice));
        b->d_streams = std::move(p);
    } else {
        HIP_TRY(b, hipMemcpy(b->d_streams, q.data(), sizeof(BatchStream) * (size_t)b->B, hipMemcpyHostToDevice));
    }
    return SFM_OK;
}

int sfm_batch_download_waypoints(SfmBatch* b, float* wx, float* wy, uint32_t* draws) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n == 0) return SFM_OK;
    if (wx || wy) {
        std::vector<float4> own(n);
        HIP_TRY(b, hipMemcpy(own.data(), b->own, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (wx) wx[i] = own[i].x;
            if (wy) wy[i] = own[i].y;
        }
    }
    if (draws) HIP_TRY(b, hipMemcpy(draws, b->draws, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return SFM_OK;
}

// The mode state machine of every row (ABI 9), the batch form of sfm_set_mode_fsm.  Everything is checked before anything is sent.
int sfm_batch_set_mode_fsm(SfmBatch* b, const uint8_t* mode, const float* target_speed, const float* initial_speed,
                           const float* crossing_speed, const float* safety_margin, const float* next_mode_time,
                           const int32_t* wp_offsets, const float* wp_x, const float* wp_y, const uint8_t* wp_crossing,
                           const int32_t* despawn_on_arrival, const float* sim_time0, const float* arrive_threshold,
                           const float* first_vehicle_extent) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!mode) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a tick in flight may still read the arrays
        drop_batch_modes(b);
        b->snap.on = false;
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!target_speed || !initial_speed || !crossing_speed || !safety_margin || !next_mode_time || !wp_offsets || !despawn_on_arrival ||
        !sim_time0 || !arrive_threshold)
        return bfail(b, SFM_ERR_INVALID, "a required mode array is NULL");
    const int N = b->n_total, B = b->B;
    if (wp_offsets[0] != 0) return bfail(b, SFM_ERR_INVALID, "wp_offsets[0] must be 0");
    for (int i = 0; i < N; ++i) {
        if (wp_offsets[i + 1] < wp_offsets[i]) return bfail(b, SFM_ERR_INVALID, "wp_offsets must be non-decreasing (row " + std::to_string(i) + ")");
        if (mode[i] > 4) return bfail(b, SFM_ERR_INVALID, "mode must be a PedMode value 0..4 (row " + std::to_string(i) + ")");
    }
    const int W = wp_offsets[N];
    if (W > 0 && (!wp_x || !wp_y || !wp_crossing)) return bfail(b, SFM_ERR_INVALID, "waypoint arrays are NULL");
    std::vector<BatchModeScene> sc((size_t)B);
    std::vector<float> t0((size_t)B);
    for (int k = 0; k < B; ++k) {
        const float thr = arrive_threshold[k];
        if (!std::isfinite(thr) || thr < 0.f || !std::isfinite(sim_time0[k]))
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": arrive_threshold must be finite and >= 0, sim_time0 finite");
        sc[k] = BatchModeScene{(float)((double)thr * (double)thr),             // thr^2 as the handle rounds it
                               first_vehicle_extent ? first_vehicle_extent[2 * k] : 0.f,
                               first_vehicle_extent ? first_vehicle_extent[2 * k + 1] : 0.f, despawn_on_arrival[k] ? 1 : 0};
        t0[k] = sim_time0[k];
    }
    const size_t n = (size_t)N;
    std::vector<float4> speeds(n);
    for (size_t i = 0; i < n; ++i) speeds[i] = make_float4(initial_speed[i], crossing_speed[i], safety_margin[i], next_mode_time[i]);
    std::vector<float2> xy((size_t)(W > 0 ? W : 1));
    for (int e = 0; e < W; ++e) xy[e] = make_float2(wp_x[e], wp_y[e]);
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick in flight may still read the old arrays
    drop_batch_modes(b);
    b->replay = {};                                               // (observed tracks: the modes own parking and birth)
    b->snap.on = false;
    HIP_TRY(b, b->modes.mode.alloc(n)); HIP_TRY(b, b->modes.target.alloc(n)); HIP_TRY(b, b->modes.speeds.alloc(n));
    HIP_TRY(b, b->modes.off.alloc(n + 1)); HIP_TRY(b, b->modes.cursor.alloc(n));
    HIP_TRY(b, b->modes.xy.alloc(xy.size())); HIP_TRY(b, b->modes.cross.alloc(xy.size()));
    HIP_TRY(b, b->modes.scene.alloc((size_t)B)); HIP_TRY(b, b->modes.time.alloc((size_t)B));
    if (n > 0) {
        HIP_TRY(b, hipMemcpy(b->modes.mode, mode, n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->modes.target, target_speed, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->modes.speeds, speeds.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemset(b->modes.cursor, 0, 4 * n));
    }
    HIP_TRY(b, hipMemcpy(b->modes.off, wp_offsets, 4 * (n + 1), hipMemcpyHostToDevice));
    if (W > 0) {
        HIP_TRY(b, hipMemcpy(b->modes.xy, xy.data(), sizeof(float2) * (size_t)W, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->modes.cross, wp_crossing, (size_t)W, hipMemcpyHostToDevice));
    }
    HIP_TRY(b, hipMemcpy(b->modes.scene, sc.data(), sizeof(BatchModeScene) * (size_t)B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->modes.time, t0.data(), 4 * (size_t)B, hipMemcpyHostToDevice));
    b->modes.on = true;
    return SFM_OK;
}

int sfm_batch_download_modes(SfmBatch* b, uint8_t* mode, float* target_speed, int32_t* cursor, float* sim_time) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->modes.on) return bfail(b, SFM_ERR_STATE, "sfm_batch_set_mode_fsm has not been called (or the modes were switched off)");
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n > 0) {
        if (mode) HIP_TRY(b, hipMemcpy(mode, b->modes.mode, n, hipMemcpyDeviceToHost));
        if (target_speed) HIP_TRY(b, hipMemcpy(target_speed, b->modes.target, 4 * n, hipMemcpyDeviceToHost));
        if (cursor) HIP_TRY(b, hipMemcpy(cursor, b->modes.cursor, 4 * n, hipMemcpyDeviceToHost));
    }
    if (sim_time) HIP_TRY(b, hipMemcpy(sim_time, b->modes.time, 4 * (size_t)b->B, hipMemcpyDeviceToHost));
    if (b->spawns.on && n > 0 && (mode || target_speed || cursor)) {      // an unborn row: SFM_MODE_UNBORN, target 0, cursor 0
        std::vector<uint8_t> born(n);
        HIP_TRY(b, hipMemcpy(born.data(), b->spawns.born, n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (born[i]) continue;
            if (mode) mode[i] = MODE_UNBORN;
            if (target_speed) target_speed[i] = 0.f;
            if (cursor) cursor[i] = 0;
        }
    }
    return SFM_OK;
}

// The spawn schedule of every row (ABI 11).  Everything is checked before anything is sent.
int sfm_batch_set_spawn_schedule(SfmBatch* b, const float* spawn_time, const uint8_t* chain) {
    int rc = bbind(b);
    if (rc) return rc;
    const size_t n = b->have_state ? (size_t)b->n_total : 0;
    if (!spawn_time) {
        if (!b->spawns.on) { b->snap.on = false; return SFM_OK; }
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a tick in flight may still write born[]
        std::vector<uint8_t> born(n);
        if (n > 0) HIP_TRY(b, hipMemcpy(born.data(), b->spawns.born, n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i)
            if (!born[i])
                return bfail(b, SFM_ERR_STATE, "the spawn schedule cannot be switched off while a row is unborn (row " + std::to_string(i) +
                                               "): a ghost without a schedule could never enter");
        b->spawns = {};
        b->snap.on = false;
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->modes.on)
        return bfail(b, SFM_ERR_STATE, "a spawn schedule needs modes: call sfm_batch_set_mode_fsm first (a newborn starts from its initial mode)");
    if (b->spawn_used)
        return bfail(b, SFM_ERR_STATE, "a spawn schedule has already been set on these rows: upload the state and set the modes again "
                                       "before a second one");
    if (n > 0 && !chain) return bfail(b, SFM_ERR_INVALID, "chain is NULL");
    for (size_t i = 0; i < n; ++i) {
        if (std::isnan(spawn_time[i]))
            return bfail(b, SFM_ERR_INVALID, "spawn_time must not be NaN (row " + std::to_string(i) + "; -inf: there from the start, +inf: never)");
        if (chain[i] > 1) return bfail(b, SFM_ERR_INVALID, "chain must be 0 or 1 (row " + std::to_string(i) + ")");
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the clocks and the state as the last tick left them
    std::vector<int> off((size_t)b->B + 1);
    std::vector<float> clk((size_t)b->B);
    HIP_TRY(b, hipMemcpy(off.data(), b->d_scene_off, sizeof(int) * off.size(), hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(clk.data(), b->modes.time, 4 * clk.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < b->B; ++k)
        if (off[k + 1] > off[k] && chain[off[k]])
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": chain must be 0 on a scene's first row (it has no row to wait for)");
    // who is there already: spawn_time <= the scene's clock and nobody to wait for; the others wait as ghosts
    std::vector<uint8_t> born(n);
    std::vector<float> birth(n);
    bool any_unborn = false;
    for (int k = 0; k < b->B; ++k)
        for (int i = off[k]; i < off[k + 1]; ++i) {
            born[i] = spawn_time[i] <= clk[k] && !chain[i] ? BORN_AT_SET : BORN_NO;
            birth[i] = born[i] ? clk[k] : std::numeric_limits<float>::quiet_NaN();
            any_unborn = any_unborn || !born[i];
        }
    const size_t m = n > 0 ? n : 1;
    b->snap.on = false;
    b->replay = {};                                               // (observed tracks: the schedule owns parking and birth)
    HIP_TRY(b, b->spawns.time.alloc(m)); HIP_TRY(b, b->spawns.chain.alloc(m)); HIP_TRY(b, b->spawns.born.alloc(m));
    HIP_TRY(b, b->spawns.birth.alloc(m)); HIP_TRY(b, b->spawns.pk0.alloc(m)); HIP_TRY(b, b->spawns.zv0.alloc(m));
    if (n > 0) {
        HIP_TRY(b, hipMemcpy(b->spawns.time, spawn_time, 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->spawns.chain, chain, n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->spawns.born, born.data(), n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->spawns.birth, birth.data(), 4 * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(b->spawns.pk0, b->pk, sizeof(float4) * n, hipMemcpyDeviceToDevice));
        if (b->z3) HIP_TRY(b, hipMemcpy(b->spawns.zv0, b->zv, sizeof(float2) * n, hipMemcpyDeviceToDevice));
        if (any_unborn) {                                        // the unborn rows leave the live state (parked by the device's own rule)
            HIP_TRY(b, launch_batch_park_unborn(b->d_scene_off, b->spawns.born, b->pk, b->z3 ? b->zv : nullptr, b->B, b->stream));
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        }
    }
    b->spawns.on = true;
    b->spawn_used = true;
    return SFM_OK;
}

int sfm_batch_download_spawns(SfmBatch* b, uint8_t* born, float* birth_time) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->spawns.on) return bfail(b, SFM_ERR_STATE, "sfm_batch_set_spawn_schedule has not been called (or the schedule was dropped)");
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n > 0) {
        if (born) {
            HIP_TRY(b, hipMemcpy(born, b->spawns.born, n, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) born[i] = born[i] != BORN_NO;
        }
        if (birth_time) HIP_TRY(b, hipMemcpy(birth_time, b->spawns.birth, 4 * n, hipMemcpyDeviceToHost));
    }
    return SFM_OK;
}

// The snapshot (ABI 13): every array a tick can change, device to device on the batch's stream; the host does not wait.
int sfm_batch_snapshot(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    b->snap.on = false;                                             // (a failure below leaves the batch without a snapshot)
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    if ((rc = snap_copy(b, b->snap.pk, b->pk, n))) return rc;
    if (b->z3 && (rc = snap_copy(b, b->snap.zv, b->zv, n))) return rc;
    if ((rc = snap_copy(b, b->snap.own, b->own, n))) return rc;
    if ((rc = snap_copy(b, b->snap.draws, b->draws, n))) return rc;
    if (b->boxes.on) {                                              // the half of the ping-pong the next tick reads
        const BatchGeoDev& g = b->geo[2];
        if ((rc = snap_copy(b, b->snap.ctr, g.ctr, (size_t)g.K))) return rc;
        if ((rc = snap_copy(b, b->snap.pts, g.pts, (size_t)g.P))) return rc;
        if ((rc = snap_copy(b, b->snap.rot, b->boxes.rot, (size_t)g.K))) return rc;   // the headings: state once vehicles are driven
    }
    if (b->modes.on) {
        if ((rc = snap_copy(b, b->snap.mode, b->modes.mode, n))) return rc;
        if ((rc = snap_copy(b, b->snap.target, b->modes.target, n))) return rc;
        if ((rc = snap_copy(b, b->snap.cursor, b->modes.cursor, n))) return rc;
        if ((rc = snap_copy(b, b->snap.time, b->modes.time, B))) return rc;
    }
    if (b->spawns.on) {
        if ((rc = snap_copy(b, b->snap.born, b->spawns.born, n))) return rc;
        if ((rc = snap_copy(b, b->snap.birth, b->spawns.birth, n))) return rc;
    }
    if (b->tracks.on) {
        if ((rc = snap_copy(b, b->snap.first, b->tracks.first, (size_t)b->geo[2].K))) return rc;
        if ((rc = refresh_track_first(b))) return rc;
        b->snap.first_h = b->tracks.first_h;
        b->snap.tick = b->tracks.tick;
    }
    if ((rc = batch_autopilot_snapshot(b))) return rc;              // the autopilot's cursors
    b->snap.on = true;
    return SFM_OK;
}

// The chosen scenes back to the snapshot: ONE launch of sfm_batch_restart_kernel, a workgroup per chosen scene.  Everything is
// checked before anything is sent or launched.
int sfm_batch_restart(SfmBatch* b, const uint8_t* mask) {
    int rc = bbind(b);
    if (rc) return rc;
    const int B = b->B;
    int chosen = B;
    std::string bad;
    if (mask) {
        chosen = 0;
        for (int k = 0; k < B && bad.empty(); ++k) {
            if (mask[k] > 1) bad = "mask must hold 0 or 1 (scene " + std::to_string(k) + ")";
            chosen += mask[k];
        }
    }
    long long shift = 0;
    if ((rc = batch_restart_checks(b, mask, bad, &shift))) return rc;
    if (chosen == 0) return SFM_OK;
    if (mask) {
        if (!b->restart.done) {                                  // (created last: a first call that failed half-way starts over)
            HIP_TRY(b, b->restart.list.alloc((size_t)B));
            HIP_TRY(b, b->restart.list_h.alloc((size_t)B));
            HIP_TRY(b, b->restart.done.create(hipEventDisableTiming));
        }
        if (b->restart.pending) {                                      // the restart before this one may still read the pinned list
            HIP_TRY(b, hipEventSynchronize(b->restart.done));
            b->restart.pending = false;
        }
        for (int k = 0, q = 0; k < B; ++k)
            if (mask[k]) b->restart.list_h[q++] = k;
        HIP_TRY(b, hipMemcpyAsync(b->restart.list, b->restart.list_h, sizeof(int) * (size_t)chosen, hipMemcpyHostToDevice, b->stream));
    }
    BatchRestart r = restart_args(b, shift);
    r.list = mask ? b->restart.list : nullptr;
    HIP_TRY(b, launch_batch_restart(r, chosen, b->stream));
    if (mask) {
        HIP_TRY(b, hipEventRecord(b->restart.done, b->stream));
        b->restart.pending = true;
    }
    if (b->tracks.on)                                               // the host's copy, which sfm_batch_download_vehicle_tracks answers from
        for (int k = 0; k < B; ++k) {                               // (a stale copy stays stale: the scenes not chosen here are not known)
            if (mask && !mask[k]) continue;
            for (int v = b->boxes.item_off_h[k]; v < b->boxes.item_off_h[k + 1]; ++v)
                b->tracks.first_h[v] = b->tracks.off_h[v + 1] > b->tracks.off_h[v] ? (int32_t)((long long)b->snap.first_h[v] + shift) : b->snap.first_h[v];
        }
    rc = batch_restart_noise(b, r.list, nullptr, chosen);
    if (!rc) rc = batch_plan_routes(b, r.list, nullptr, chosen);        // (routes: from where the rows were placed)
    if (!rc) rc = batch_autopilot_restart(b, r.list, nullptr, chosen);  // (the autopilot's cursors)
    if (!rc) rc = batch_row_restart(b, r.list, nullptr, chosen);        // (the row episodes start over)
    return rc ? rc : batch_vehicle_episode_restart(b, r.list, nullptr, chosen);   // (... and the vehicle episodes)
}

// The restart with its mask on the device (ABI 16): no copy, no host scan, no event wait, no pinned list.
int sfm_batch_restart_device(SfmBatch* b, const uint8_t* d_mask) {
    int rc = bbind(b);
    if (rc) return rc;
    long long shift = 0;                                         // (every scene: the host cannot know who is chosen)
    if ((rc = batch_restart_checks(b, nullptr, d_mask ? "" : "d_mask is NULL (device memory, one byte per scene)", &shift))) return rc;
    return batch_restart_device(b, d_mask, shift);
}

int sfm_batch_run_recorded(SfmBatch* b, int ticks, uint32_t flags, int stride, float* frames, float* zframes, int max_frames,
                           int* n_frames) {
    return batch_run_recorded(b, ticks, flags, stride, frames, zframes, max_frames, n_frames, false, 0, nullptr);
}

int sfm_batch_run_recorded_forces(SfmBatch* b, int ticks, uint32_t flags, int stride, uint32_t force_mask, float* frames,
                                  float* zframes, float* forces, int max_frames, int* n_frames) {
    return batch_run_recorded(b, ticks, flags, stride, frames, zframes, max_frames, n_frames, true, force_mask, forces);
}

// Steering (ABI 14): per-row commands the ticks read.  Everything is checked before anything is sent or freed.
int sfm_batch_set_steering(SfmBatch* b, const uint8_t* kind, const float* ux, const float* uy, const float* uz) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    const size_t n = (size_t)b->n_total;
    if (kind) {
        for (size_t i = 0; i < n; ++i)
            if (kind[i] > 2)
                return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": kind must be 0 (not steered), 1 (velocity command) or 2 "
                                                 "(preferred velocity)");
        rc = check_batch_commands(b, nullptr, kind, ux, uy, uz);
        if (rc) return rc;
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick or a copy in flight may still read the buffers
    b->steer = {};
    if (!kind) { b->replay = {}; return SFM_OK; }                // (observed tracks are replayed through the commands)
    if (n > 0) {
        HIP_TRY(b, b->steer.cmd.alloc(n));
        HIP_TRY(b, b->steer.cmd_h.alloc(n));
        if (!b->c_done) HIP_TRY(b, b->c_done.create(hipEventDisableTiming));
        for (size_t i = 0; i < n; ++i) b->steer.cmd_h[i] = make_float4(ux[i], uy[i], uz ? uz[i] : 0.f, (float)kind[i]);
        HIP_TRY(b, hipMemcpy(b->steer.cmd, b->steer.cmd_h, sizeof(float4) * n, hipMemcpyHostToDevice));
    }
    b->steer.on = true;
    return SFM_OK;
}

int sfm_batch_set_commands(SfmBatch* b, const float* ux, const float* uy, const float* uz) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->steer.on) return bfail(b, SFM_ERR_STATE, STEERING_OFF);
    rc = check_batch_commands(b, b->steer.cmd_h, nullptr, ux, uy, uz);
    if (rc) return rc;
    const size_t n = (size_t)b->n_total;
    if (n == 0) return SFM_OK;
    if (b->steer.pending) {                                          // the copy before this one may still read the pinned block
        HIP_TRY(b, hipEventSynchronize(b->c_done));
        b->steer.pending = false;
    }
    for (size_t i = 0; i < n; ++i) { b->steer.cmd_h[i].x = ux[i]; b->steer.cmd_h[i].y = uy[i]; b->steer.cmd_h[i].z = uz ? uz[i] : 0.f; }
    HIP_TRY(b, hipMemcpyAsync(b->steer.cmd, b->steer.cmd_h, sizeof(float4) * n, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipEventRecord(b->c_done, b->stream));
    b->steer.pending = true;
    return SFM_OK;
}

int sfm_batch_download_steering(SfmBatch* b, uint8_t* kind, float* ux, float* uy, float* uz) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->steer.on) return bfail(b, SFM_ERR_STATE, STEERING_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n == 0) return SFM_OK;
    std::vector<float4> c(n);
    HIP_TRY(b, hipMemcpy(c.data(), b->steer.cmd, sizeof(float4) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (kind) kind[i] = c[i].w == 1.0f ? 1 : c[i].w == 2.0f ? 2 : 0;   // (what the tick makes of it)
        if (ux) ux[i] = c[i].x;
        if (uy) uy[i] = c[i].y;
        if (uz) uz[i] = c[i].z;
    }
    return SFM_OK;
}

const char* sfm_batch_last_error(const SfmBatch* b) { return b ? b->err.c_str() : g_create_error.c_str(); }

}  // extern "C"
