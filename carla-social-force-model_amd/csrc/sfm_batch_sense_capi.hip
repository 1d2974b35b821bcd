// sfm_batch_sense_capi.hip -- host side of the batch's read-only sensors (ABI 15 to 17): observations, episode ends, range scans (from
// the rows and from the vehicles) and occupancy grids, and the device pointers a caller shares with them.  Each sensor reads the scenes through one BatchSceneView and writes only its own
// buffers -- nothing a tick reads or writes.  The batch's types are in sfm_batch_host.h; the ticks, the restarts and everything else
// in sfm_batch_capi.hip.
#include "sfm_batch_host.h"

using namespace sfm;

// scene s's length `name`, squared into *sq: sfm_metres.h's check, as a refusal of the batch
static int batch_metres(SfmBatch* b, size_t s, const char* name, float r, bool strict, float* sq) {
    const std::string why = check_metres((int)s, name, r, strict, sq);
    return why.empty() ? SFM_OK : bfail(b, SFM_ERR_INVALID, why);
}

static int check_frame(SfmBatch* b, int frame, const char* whose = "row") {
    if (frame != SFM_OBS_FRAME_WORLD && frame != SFM_OBS_FRAME_HEADING)
        return bfail(b, SFM_ERR_INVALID, std::string("frame must be 0 (world axes) or 1 (the ") + whose + "'s heading frame), got " + std::to_string(frame));
    return SFM_OK;
}

// What sfm_batch_set_scan and sfm_batch_set_vehicle_scan share: every check from R on, then the settings and the zero-filled buffer of
// `items` records (rows, or vehicles) in *o.  `whose`: "row" or "vehicle", for the messages; mount: the vehicles' {x, y}, checked
// where sfm_batch_set_vehicle_scan always checked it, null for the rows.  Everything is checked before anything is allocated; the
// caller synchronises the stream (the zero fill) before it moves *o into the batch.
static int build_scan(SfmBatch* b, size_t items, int max_rays, const char* whose, int R, const float* dir_x, const float* dir_y,
                      const float* max_range, const float* ped_radius, const float* point_radius, const uint8_t* mask, int frame,
                      const float* mount, BatchScanDev* o) {
    int rc;
    if (R < 1 || R > max_rays)
        return bfail(b, SFM_ERR_INVALID, "R must be 1 .. " + std::to_string(max_rays) + " rays per " + whose + ", got " + std::to_string(R));
    if ((rc = check_frame(b, frame, whose))) return rc;
    if (!dir_x || !dir_y) return bfail(b, SFM_ERR_INVALID, "dir_x or dir_y is NULL");
    if (!ped_radius || !point_radius) return bfail(b, SFM_ERR_INVALID, "ped_radius or point_radius is NULL");
    if (mount && (!std::isfinite(mount[0]) || !std::isfinite(mount[1]) || std::fabs(mount[0]) > SFM_BATCH_MAX_SENSE_RANGE ||
                  std::fabs(mount[1]) > SFM_BATCH_MAX_SENSE_RANGE))
        return bfail(b, SFM_ERR_INVALID, "the mount must be finite and within 1e6 metres of the vehicle's centre");
    std::vector<float2> dir((size_t)R);
    for (int q = 0; q < R; ++q) {
        if (!std::isfinite(dir_x[q]) || !std::isfinite(dir_y[q]))
            return bfail(b, SFM_ERR_INVALID, "ray " + std::to_string(q) + ": its direction is not finite");
        dir[q] = make_float2(dir_x[q], dir_y[q]);
    }
    const size_t B = (size_t)b->B;
    std::vector<BatchScanScene> set(B);
    for (size_t s = 0; s < B; ++s) {
        set[s] = BatchScanScene{max_range[s], 0.f, 0.f, 0.f};    // (the range goes to the kernel as the fp32 value given)
        if ((rc = batch_metres(b, s, "max_range", max_range[s], true, nullptr))) return rc;
        if ((rc = batch_metres(b, s, "ped_radius", ped_radius[s], false, &set[s].ped_r2))) return rc;
        if ((rc = batch_metres(b, s, "point_radius", point_radius[s], false, &set[s].point_r2))) return rc;
    }
    const size_t vals = items * (size_t)(2 * R);
    HIP_TRY(b, o->set.alloc(B));
    HIP_TRY(b, o->dir.alloc((size_t)R));
    HIP_TRY(b, hipMemcpy(o->set, set.data(), sizeof(BatchScanScene) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(o->dir, dir.data(), sizeof(float2) * (size_t)R, hipMemcpyHostToDevice));
    if (mask && items > 0) {
        HIP_TRY(b, o->mask.alloc(items));
        HIP_TRY(b, hipMemcpy(o->mask, mask, items, hipMemcpyHostToDevice));
    }
    if (vals > 0) {
        HIP_TRY(b, o->buf.alloc(vals));
        HIP_TRY(b, hipMemsetAsync(o->buf, 0, sizeof(float) * vals, b->stream));
    }
    o->R = R;
    o->frame = frame;
    if (mount) { o->mount_x = mount[0]; o->mount_y = mount[1]; }
    o->on = true;
    return SFM_OK;
}

// What sfm_batch_set_grid and sfm_batch_set_vehicle_grid share: every check from the frame on, then the settings and the zero-filled
// buffer of the gridded ones of `items` rows, or vehicles, in *o -- GU x GV cells in `channels` channels each.  `whose` as for
// build_scan; centre: the middle of the vehicles' window {x, y}, checked where sfm_batch_set_vehicle_grid always checked it, null for
// the rows.  Everything is checked before anything is allocated; the caller synchronises the stream (the zero fill) before it moves
// *o into the batch.
static int build_grid(SfmBatch* b, size_t items, int channels, const char* whose, int GU, int GV, const float* cell, const uint8_t* mask,
                      int frame, const float* centre, BatchGridDev* o) {
    int rc;
    if ((rc = check_frame(b, frame, whose))) return rc;
    if (centre && (!std::isfinite(centre[0]) || !std::isfinite(centre[1]) || std::fabs(centre[0]) > SFM_BATCH_MAX_SENSE_RANGE ||
                   std::fabs(centre[1]) > SFM_BATCH_MAX_SENSE_RANGE))
        return bfail(b, SFM_ERR_INVALID, "the centre must be finite and within 1e6 metres of the vehicle's centre");
    const size_t B = (size_t)b->B;
    for (size_t s = 0; s < B; ++s)
        if ((rc = batch_metres(b, s, "cell", cell[s], true, nullptr))) return rc;   // (the size goes to the kernel as the fp32 value given)
    o->GU = GU;
    o->GV = GV;
    o->M = items;                                                // no mask: every item, slot = item
    if (mask && items > 0) {
        std::vector<int32_t> slot(items);
        o->M = pack_grid_slots(mask, items, slot.data());
        HIP_TRY(b, o->slot.alloc(items));
        HIP_TRY(b, hipMemcpy(o->slot, slot.data(), sizeof(int32_t) * items, hipMemcpyHostToDevice));
    }
    const size_t vals = o->vals(channels);
    HIP_TRY(b, o->cell.alloc(B));
    HIP_TRY(b, hipMemcpy(o->cell, cell, sizeof(float) * B, hipMemcpyHostToDevice));
    if (vals > 0) {
        HIP_TRY(b, o->buf.alloc(vals));
        HIP_TRY(b, hipMemsetAsync(o->buf, 0, sizeof(float) * vals, b->stream));
    }
    o->frame = frame;
    if (centre) { o->centre_x = centre[0]; o->centre_y = centre[1]; }
    o->on = true;
    return SFM_OK;
}

// One lookup for the device buffers a caller may see: which = SFM_BATCH_PTR_*, or PTR_OBSERVATIONS for sfm_batch_observation_ptr's.
// off: why there is none (its feature is off, no state was uploaded), else p and bytes -- both 0 where the buffer has no element.
constexpr int PTR_OBSERVATIONS = SFM_BATCH_PTR_VEHICLE_SCENE_DONE + 1;   // (not part of the ABI: sfm_batch_device_ptr refuses it)
struct BatchBuffer { const char* off; void* p; size_t bytes; };
static BatchBuffer batch_buffer(const SfmBatch* b, int which) {
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    auto have = [](void* p, size_t bytes) { return BatchBuffer{nullptr, bytes > 0 ? p : nullptr, bytes}; };
    switch (which) {
    case PTR_OBSERVATIONS:
        if (!b->obs.on) return {OBSERVATIONS_OFF, nullptr, 0};
        return have(b->obs.buf, sizeof(float) * n * (size_t)(SFM_BATCH_OBS_HEADER + 4 * b->obs.k));
    case SFM_BATCH_PTR_SCAN:
        if (!b->scan.on) return {SCANS_OFF, nullptr, 0};
        return have(b->scan.buf, sizeof(float) * n * (size_t)(2 * b->scan.R));
    case SFM_BATCH_PTR_EPISODES:
    case SFM_BATCH_PTR_DONE:
        if (!b->ep.on) return {EPISODES_OFF, nullptr, 0};
        return which == SFM_BATCH_PTR_EPISODES ? have(b->ep.record, 8 * sizeof(float) * B) : have(b->ep.done, B);
    case SFM_BATCH_PTR_ROW_EPISODES:
    case SFM_BATCH_PTR_ROW_DONE:
        if (!b->ep.rows.on) return {ROW_EPISODES_OFF, nullptr, 0};
        return which == SFM_BATCH_PTR_ROW_EPISODES ? have(b->ep.rows.record, 8 * sizeof(float) * n) : have(b->ep.rows.done, n);
    case SFM_BATCH_PTR_ROW_RESETS:
        if (!b->noise.on) return {NOISE_OFF, nullptr, 0};
        return have(b->noise.row_resets, sizeof(uint32_t) * n);
    case SFM_BATCH_PTR_RESETS:
        if (!b->noise.on) return {NOISE_OFF, nullptr, 0};
        return have(b->noise.resets, sizeof(uint32_t) * B);
    case SFM_BATCH_PTR_GRID:
        if (!b->grid.on) return {GRIDS_OFF, nullptr, 0};
        return have(b->grid.buf, sizeof(float) * b->grid.vals(SFM_BATCH_GRID_CHANNELS));
    case SFM_BATCH_PTR_ROW_SCORES:
    case SFM_BATCH_PTR_SCENE_SCORES:
        if (!b->replay.on) return {OBSERVED_OFF, nullptr, 0};
        return which == SFM_BATCH_PTR_ROW_SCORES ? have(b->replay.score, sizeof(float4) * n) : have(b->replay.scene, 5 * sizeof(float) * B);
    case SFM_BATCH_PTR_VEHICLE_COMMANDS:
        if (!b->drive.on) return {DRIVING_OFF, nullptr, 0};
        return have(b->drive.cmd, sizeof(float4) * (size_t)b->geo[2].K);
    case SFM_BATCH_PTR_VEHICLE_OBS:
        if (!b->vobs.on) return {VEHICLE_OBS_OFF, nullptr, 0};
        return have(b->vobs.buf, sizeof(float) * (size_t)b->geo[2].K * (size_t)(SFM_BATCH_OBS_HEADER + 4 * b->vobs.k));
    case SFM_BATCH_PTR_VEHICLE_SCAN:
        if (!b->vscan.on) return {VEHICLE_SCAN_OFF, nullptr, 0};
        return have(b->vscan.buf, sizeof(float) * (size_t)b->geo[2].K * (size_t)(2 * b->vscan.R));
    case SFM_BATCH_PTR_VEHICLE_GRID:
        if (!b->boxes.vgrid.on) return {VEHICLE_GRID_OFF, nullptr, 0};
        return have(b->boxes.vgrid.buf, sizeof(float) * b->boxes.vgrid.vals(SFM_BATCH_VEHICLE_GRID_CHANNELS));
    case SFM_BATCH_PTR_VEHICLE_EPISODES:
    case SFM_BATCH_PTR_VEHICLE_DONE:
    case SFM_BATCH_PTR_VEHICLE_SCENE_DONE:
        if (!b->boxes.vep.on) return {VEHICLE_EPISODES_OFF, nullptr, 0};
        if (which == SFM_BATCH_PTR_VEHICLE_SCENE_DONE) return have(b->boxes.vep.scene_done, B);
        return which == SFM_BATCH_PTR_VEHICLE_EPISODES ? have(b->boxes.vep.record, 8 * sizeof(float) * (size_t)b->geo[2].K)
                                                       : have(b->boxes.vep.done, (size_t)b->geo[2].K);
    case SFM_BATCH_PTR_ROUTE_GOALS:
    case SFM_BATCH_PTR_ROUTE_STATUS:
        if (!b->routes.on) return {ROUTES_OFF, nullptr, 0};
        return which == SFM_BATCH_PTR_ROUTE_GOALS ? have(b->routes.goal, sizeof(float2) * n) : have(b->routes.status, sizeof(int) * n);
    }
    if (!b->have_state) return {NO_STATE, nullptr, 0};
    if (which == SFM_BATCH_PTR_COMMANDS) {
        if (!b->steer.on) return {STEERING_OFF, nullptr, 0};
        return have(b->steer.cmd, sizeof(float4) * n);
    }
    if (which == SFM_BATCH_PTR_ZSTATE) return have(b->zv, b->z3 ? sizeof(float2) * n : 0);    // a planar batch has no {z, vz}
    return have(b->pk, sizeof(float4) * n);
}

// sfm_batch_download_observations / _scan: the sensor's whole buffer, after everything queued on the batch's stream
static int download_buffer(SfmBatch* b, int which, float* out) {
    int rc = bbind(b);
    if (rc) return rc;
    const BatchBuffer s = batch_buffer(b, which);
    if (s.off) return bfail(b, SFM_ERR_STATE, s.off);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (s.bytes == 0) return SFM_OK;
    if (!out) return bfail(b, SFM_ERR_INVALID, "out is NULL");
    HIP_TRY(b, hipMemcpy(out, s.p, s.bytes, hipMemcpyDeviceToHost));
    return SFM_OK;
}

static void* buffer_ptr(SfmBatch* b, int which, const char* so, int64_t* bytes) {
    const BatchBuffer s = batch_buffer(b, which);
    if (s.off) { bfail(b, SFM_ERR_STATE, std::string(s.off) + so); return nullptr; }
    if (bytes) *bytes = (int64_t)s.bytes;
    return s.p;
}

extern "C" {

void* sfm_batch_device_ptr(SfmBatch* b, int which, int64_t* bytes) {
    if (bytes) *bytes = 0;
    if (!b) return nullptr;
    // SFM_BATCH_PTR_RESETS came without an ABI bump: while restart noise is off it is refused as the unknown value it was, word for
    // word, so a caller of ABI 17 as it was sees no difference
    // (SFM_BATCH_PTR_GRID likewise, while grids are off, SFM_BATCH_PTR_ROW_SCORES / _SCENE_SCORES while observed tracks are off, and
    //  SFM_BATCH_PTR_VEHICLE_COMMANDS / _VEHICLE_OBS while driving / vehicle observations are off; SFM_BATCH_PTR_VEHICLE_SCAN is
    //  specified as SFM_ERR_STATE while the vehicle scan is off, so it is always known; SFM_BATCH_PTR_ROW_EPISODES / _ROW_DONE while
    //  row episodes are off, SFM_BATCH_PTR_ROW_RESETS while restart noise is off and SFM_BATCH_PTR_VEHICLE_EPISODES / _VEHICLE_DONE /
    //  _VEHICLE_SCENE_DONE while vehicle episodes are off are refused likewise)
    const bool known = (which >= SFM_BATCH_PTR_COMMANDS && which <= SFM_BATCH_PTR_SCAN) || (which == SFM_BATCH_PTR_RESETS && b->noise.on) ||
                       (which == SFM_BATCH_PTR_GRID && b->grid.on) ||
                       ((which == SFM_BATCH_PTR_ROW_SCORES || which == SFM_BATCH_PTR_SCENE_SCORES) && b->replay.on) ||
                       (which == SFM_BATCH_PTR_VEHICLE_COMMANDS && b->drive.on) || (which == SFM_BATCH_PTR_VEHICLE_OBS && b->vobs.on) ||
                       which == SFM_BATCH_PTR_VEHICLE_SCAN || (which == SFM_BATCH_PTR_VEHICLE_GRID && b->boxes.vgrid.on) ||
                       ((which == SFM_BATCH_PTR_ROUTE_GOALS || which == SFM_BATCH_PTR_ROUTE_STATUS) && b->routes.on) ||
                       ((which == SFM_BATCH_PTR_ROW_EPISODES || which == SFM_BATCH_PTR_ROW_DONE) && b->ep.rows.on) ||
                       (which == SFM_BATCH_PTR_ROW_RESETS && b->noise.on) ||
                       (which >= SFM_BATCH_PTR_VEHICLE_EPISODES && which <= SFM_BATCH_PTR_VEHICLE_SCENE_DONE && b->boxes.vep.on);
    if (!known) { bfail(b, SFM_ERR_INVALID, "which must be SFM_BATCH_PTR_COMMANDS, _STATE, _ZSTATE, _EPISODES, _DONE or _SCAN"); return nullptr; }
    return buffer_ptr(b, which, which == SFM_BATCH_PTR_SCAN ? ", so which = SFM_BATCH_PTR_SCAN has no buffer" :
                                which == SFM_BATCH_PTR_EPISODES || which == SFM_BATCH_PTR_DONE ? ", so which = SFM_BATCH_PTR_EPISODES / _DONE has no buffer" : "", bytes);
}

// Observations (ABI 15).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_observation(SfmBatch* b, int k, const float* sense_range, int frame) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!sense_range) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // an observe in flight may still write the buffer
        b->obs = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (k < 1 || k > SFM_BATCH_MAX_OBS_NEIGHBOURS)
        return bfail(b, SFM_ERR_INVALID, "k must be 1 .. " + std::to_string(SFM_BATCH_MAX_OBS_NEIGHBOURS) + " neighbour slots, got " + std::to_string(k));
    if ((rc = check_frame(b, frame))) return rc;
    std::vector<float> r2((size_t)b->B);
    for (size_t s = 0; s < r2.size(); ++s)
        if ((rc = batch_metres(b, s, "sense_range", sense_range[s], true, &r2[s]))) return rc;
    const size_t vals = (size_t)b->n_total * (size_t)(SFM_BATCH_OBS_HEADER + 4 * k);
    BatchObsDev o;
    HIP_TRY(b, o.range2.alloc((size_t)b->B));
    HIP_TRY(b, hipMemcpy(o.range2, r2.data(), sizeof(float) * r2.size(), hipMemcpyHostToDevice));
    if (vals > 0) {
        HIP_TRY(b, o.buf.alloc(vals));
        HIP_TRY(b, hipMemsetAsync(o.buf, 0, sizeof(float) * vals, b->stream));
    }
    o.k = k;
    o.frame = frame;
    o.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and an observe in flight may still write the old buffer
    b->obs = std::move(o);
    return SFM_OK;
}

int sfm_batch_observe(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->obs.on) return bfail(b, SFM_ERR_STATE, OBSERVATIONS_OFF);
    if (b->n_total == 0) return SFM_OK;
    const ObserveArgs a{batch_scene_view(b), b->obs.range2, b->obs.buf, b->obs.k, b->obs.frame};
    HIP_TRY(b, launch_batch_observe(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_observations(SfmBatch* b, float* out) { return download_buffer(b, PTR_OBSERVATIONS, out); }

void* sfm_batch_observation_ptr(SfmBatch* b, int64_t* bytes) {
    if (bytes) *bytes = 0;
    if (!b) return nullptr;
    return buffer_ptr(b, PTR_OBSERVATIONS, "", bytes);
}

// Episodes (ABI 16).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_episodes(SfmBatch* b, const int32_t* agent, const float* goal_radius, const float* ped_radius, const float* veh_radius,
                           const int32_t* max_steps) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!agent) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // an end_step or a restart in flight may still write the buffers
        BatchRowEpisodeDev rows = std::move(b->ep.rows);         // (the row episodes stay: they have a call of their own)
        b->ep = {};
        b->ep.rows = std::move(rows);
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!goal_radius || !ped_radius || !veh_radius || !max_steps)
        return bfail(b, SFM_ERR_INVALID, "goal_radius, ped_radius, veh_radius or max_steps is NULL");
    const size_t B = (size_t)b->B;
    std::vector<int> off(B + 1);
    HIP_TRY(b, hipMemcpy(off.data(), b->d_scene_off, sizeof(int) * off.size(), hipMemcpyDeviceToHost));
    std::vector<BatchEpisodeScene> set(B);
    for (size_t s = 0; s < B; ++s) {
        const int n = off[s + 1] - off[s];
        if (agent[s] < -1 || agent[s] >= n)
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(s) + ": agent must be -1 (none) or a row 0 .. " + std::to_string(n - 1) +
                                             " of the scene, got " + std::to_string(agent[s]));
        set[s] = BatchEpisodeScene{agent[s], max_steps[s], 0.f, 0.f, 0.f, {0, 0, 0}};
        if ((rc = batch_metres(b, s, "goal_radius", goal_radius[s], false, &set[s].goal_r2))) return rc;
        if ((rc = batch_metres(b, s, "ped_radius", ped_radius[s], false, &set[s].ped_r2))) return rc;
        if ((rc = batch_metres(b, s, "veh_radius", veh_radius[s], false, &set[s].veh_r2))) return rc;
        if (max_steps[s] < 0) return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(s) + ": max_steps must be >= 0 (0: no time limit)");
    }
    const std::vector<float> nan(B, std::numeric_limits<float>::quiet_NaN());
    BatchEpisodeDev e;
    HIP_TRY(b, e.set.alloc(B)); HIP_TRY(b, e.age.alloc(B)); HIP_TRY(b, e.prev.alloc(B));
    HIP_TRY(b, e.record.alloc(8 * B)); HIP_TRY(b, e.done.alloc(B));
    HIP_TRY(b, hipMemcpy(e.set, set.data(), sizeof(BatchEpisodeScene) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(e.prev, nan.data(), sizeof(float) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemsetAsync(e.age, 0, sizeof(int) * B, b->stream));
    HIP_TRY(b, hipMemsetAsync(e.record, 0, sizeof(float) * 8 * B, b->stream));
    HIP_TRY(b, hipMemsetAsync(e.done, 0, B, b->stream));
    e.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and an end_step or a restart in flight may still write the old buffers
    e.rows = std::move(b->ep.rows);                              // (the row episodes stay)
    b->ep = std::move(e);
    return SFM_OK;
}

int sfm_batch_end_step(SfmBatch* b, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    if (flags & ~(uint32_t)SFM_END_STEP_AUTO_RESTART) return bfail(b, SFM_ERR_INVALID, "sfm_batch_end_step takes SFM_END_STEP_AUTO_RESTART only");
    if (!b->ep.on) return bfail(b, SFM_ERR_STATE, EPISODES_OFF);
    const bool restart = (flags & SFM_END_STEP_AUTO_RESTART) != 0;
    long long shift = 0;                                         // the restart's refusals come first: nothing is launched then
    if (restart && (rc = batch_restart_checks(b, nullptr, "", &shift))) return rc;
    const EpisodeArgs a{batch_scene_view(b), b->ep.set, b->ep.age, b->ep.prev, b->ep.record, b->ep.done};
    HIP_TRY(b, launch_batch_episode(a, b->B, b->stream));
    return restart ? batch_restart_device(b, b->ep.done, shift) : SFM_OK;
}

int sfm_batch_download_episodes(SfmBatch* b, float* record, uint8_t* done) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->ep.on) return bfail(b, SFM_ERR_STATE, EPISODES_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t B = (size_t)b->B;
    if (record) HIP_TRY(b, hipMemcpy(record, b->ep.record, sizeof(float) * 8 * B, hipMemcpyDeviceToHost));
    if (done) HIP_TRY(b, hipMemcpy(done, b->ep.done, B, hipMemcpyDeviceToHost));
    return SFM_OK;
}

// Range scans (ABI 17).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_scan(SfmBatch* b, int R, const float* dir_x, const float* dir_y, const float* max_range, const float* ped_radius,
                       const float* point_radius, const uint8_t* mask, int frame) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!max_range) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a scan in flight may still write the buffer
        b->scan = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    BatchScanDev o;
    if ((rc = build_scan(b, (size_t)b->n_total, SFM_BATCH_MAX_SCAN_RAYS, "row", R, dir_x, dir_y, max_range, ped_radius, point_radius, mask,
                         frame, nullptr, &o)))
        return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and a scan in flight may still write the old buffer
    b->scan = std::move(o);
    return SFM_OK;
}

int sfm_batch_scan(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->scan.on) return bfail(b, SFM_ERR_STATE, SCANS_OFF);
    if (b->n_total == 0) return SFM_OK;
    const ScanArgs a{batch_scene_view(b), b->scan.set, b->scan.dir, b->scan.mask /* null: every row */, b->scan.buf, b->scan.R, b->scan.frame};
    HIP_TRY(b, launch_batch_scan(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_scan(SfmBatch* b, float* out) { return download_buffer(b, SFM_BATCH_PTR_SCAN, out); }

// Range scans from the vehicles (ABI 17, added without a bump).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_vehicle_scan(SfmBatch* b, int R, const float* dir_x, const float* dir_y, const float* max_range, const float* ped_radius,
                               const float* point_radius, const uint8_t* mask, int frame, float mount_x, float mount_y) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!max_range) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a scan in flight may still write the buffer
        b->vscan = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle scans: ") + NO_BOXES);
    const float mount[2] = {mount_x, mount_y};
    BatchScanDev o;
    if ((rc = build_scan(b, (size_t)b->geo[2].K, SFM_BATCH_MAX_VEHICLE_SCAN_RAYS, "vehicle", R, dir_x, dir_y, max_range, ped_radius,
                         point_radius, mask, frame, mount, &o)))
        return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and a scan in flight may still write the old buffer
    b->vscan = std::move(o);
    return SFM_OK;
}

int sfm_batch_scan_vehicles(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->vscan.on) return bfail(b, SFM_ERR_STATE, VEHICLE_SCAN_OFF);
    if (b->geo[2].K == 0) return SFM_OK;                         // no vehicle: nothing to write
    const VehicleScanArgs a{batch_scene_view(b), b->boxes.rot, b->vscan.set, b->vscan.dir, b->vscan.mask /* null: every vehicle */,
                            b->vscan.buf, b->vscan.R, b->vscan.frame, b->vscan.mount_x, b->vscan.mount_y};
    HIP_TRY(b, launch_batch_vehicle_scan(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_vehicle_scan(SfmBatch* b, float* out) { return download_buffer(b, SFM_BATCH_PTR_VEHICLE_SCAN, out); }

// Occupancy grids (ABI 17, added without a bump).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_grid(SfmBatch* b, int G, const float* cell, const uint8_t* mask, int frame) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!cell) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a grid launch in flight may still write the buffer
        b->grid = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (G < 1 || G > SFM_BATCH_MAX_GRID)
        return bfail(b, SFM_ERR_INVALID, "G must be 1 .. " + std::to_string(SFM_BATCH_MAX_GRID) + " cells per side, got " + std::to_string(G));
    BatchGridDev o;
    if ((rc = build_grid(b, (size_t)b->n_total, SFM_BATCH_GRID_CHANNELS, "row", G, G, cell, mask, frame, nullptr, &o))) return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and a grid launch in flight may still write the old buffer
    b->grid = std::move(o);
    return SFM_OK;
}

int sfm_batch_grid(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->grid.on) return bfail(b, SFM_ERR_STATE, GRIDS_OFF);
    if (b->grid.M == 0) return SFM_OK;                           // no gridded row: nothing to write
    const GridArgs a{batch_scene_view(b), b->grid.cell, b->grid.slot /* null: every row */, b->grid.buf, b->grid.GU, b->grid.frame};
    HIP_TRY(b, launch_batch_grid(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_grid(SfmBatch* b, float* out) { return download_buffer(b, SFM_BATCH_PTR_GRID, out); }

// Bird's-eye grids around the vehicles (ABI 17, added without a bump).  Everything is checked before anything is allocated or freed.
int sfm_batch_set_vehicle_grid(SfmBatch* b, int GU, int GV, const float* cell, const uint8_t* mask, int frame, float centre_x,
                               float centre_y) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!cell) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a grid launch in flight may still write the buffer
        b->boxes.vgrid = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle grids: ") + NO_BOXES);
    const int side = SFM_BATCH_MAX_VEHICLE_GRID_SIDE;
    if (GU < 1 || GU > side || GV < 1 || GV > side)
        return bfail(b, SFM_ERR_INVALID, "GU and GV must be 1 .. " + std::to_string(side) + " cells, got " + std::to_string(GU) + " x " + std::to_string(GV));
    if (GU * GV > VEHICLE_GRID_MAX_CELLS)
        return bfail(b, SFM_ERR_INVALID, "GU * GV must be at most " + std::to_string(VEHICLE_GRID_MAX_CELLS) + " cells, got " + std::to_string(GU * GV));
    const float centre[2] = {centre_x, centre_y};
    BatchGridDev o;
    if ((rc = build_grid(b, (size_t)b->geo[2].K, SFM_BATCH_VEHICLE_GRID_CHANNELS, "vehicle", GU, GV, cell, mask, frame, centre, &o)))
        return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and a grid launch in flight may still write the old buffer
    b->boxes.vgrid = std::move(o);
    return SFM_OK;
}

int sfm_batch_grid_vehicles(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->boxes.vgrid.on) return bfail(b, SFM_ERR_STATE, VEHICLE_GRID_OFF);
    if (b->boxes.vgrid.M == 0) return SFM_OK;                          // no gridded vehicle: nothing to write
    const VehicleGridArgs a{batch_scene_view(b), b->boxes.rot, b->boxes.vgrid.cell, b->boxes.vgrid.slot /* null: every vehicle */, b->boxes.vgrid.buf,
                            b->boxes.vgrid.GU, b->boxes.vgrid.GV, b->boxes.vgrid.frame, b->boxes.vgrid.centre_x, b->boxes.vgrid.centre_y, 0};
    HIP_TRY(b, launch_batch_vehicle_grid(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_vehicle_grid(SfmBatch* b, float* out) { return download_buffer(b, SFM_BATCH_PTR_VEHICLE_GRID, out); }

}  // extern "C"
