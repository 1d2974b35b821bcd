// sfm_batch_autopilot_capi.hip -- host side of the batch's vehicle autopilot: the controller that writes the commands of the
// autopiloted vehicles on the device in front of every integrating tick (sfm_batch_autopilot.hip; the rule is specified in
// include/sfm_hip.h).  It is a part of the driving (BatchDriveDev::ap in sfm_batch_host.h): dropped with it, and by every
// sfm_batch_set_vehicle_driving.  batch_launch, sfm_batch_snapshot and the restarts (sfm_batch_capi.hip) call the three hooks below.
#include "sfm_batch_host.h"

using namespace sfm;

// one setting of one vehicle: finite, and inside its bound
static std::string check_setting(size_t k, const char* name, float v, bool positive, float* out) {
    if (!std::isfinite(v) || (positive ? !(v > 0.0f) : !(v >= 0.0f)))
        return "vehicle " + std::to_string(k) + ": " + name + " must be finite and " + (positive ? "> 0" : ">= 0") + ", got " + std::to_string(v);
    *out = v;
    return "";
}

int sfm::batch_autopilot_launch(SfmBatch* b) {
    BatchAutopilotDev& p = b->drive.ap;
    AutopilotArgs a{batch_scene_view(b), b->d_prm, b->boxes.rot, p.path_off, p.path, p.set, p.cursor, b->drive.cmd, p.record};
    HIP_TRY(b, launch_batch_vehicle_autopilot(a, b->B, b->stream));
    ++p.launches;
    return SFM_OK;
}

int sfm::batch_autopilot_snapshot(SfmBatch* b) {
    BatchAutopilotDev& p = b->drive.ap;
    if (!p.on || b->geo[2].K == 0) return SFM_OK;
    HIP_TRY(b, hipMemcpyAsync(p.s_cursor, p.cursor, sizeof(int) * (size_t)b->geo[2].K, hipMemcpyDeviceToDevice, b->stream));
    return SFM_OK;
}

int sfm::batch_autopilot_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes) {
    BatchAutopilotDev& p = b->drive.ap;
    if (!p.on || scenes <= 0) return SFM_OK;
    HIP_TRY(b, launch_batch_autopilot_restart(d_list, d_mask, b->geo_item_off[2], p.cursor, p.s_cursor, scenes, b->stream));
    return SFM_OK;
}

extern "C" {

// Everything is checked before anything is allocated, sent or freed.
int sfm_batch_set_vehicle_autopilot(SfmBatch* b, const int32_t* path_off, const float* px, const float* py, const float* settings,
                                    const uint8_t* flags) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!path_off) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a launch in flight may still read the buffers
        b->drive.ap = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle autopilot: ") + NO_BOXES);
    const size_t M = (size_t)b->geo[2].K;
    if (!settings || !flags) return bfail(b, SFM_ERR_INVALID, "settings or flags is NULL");
    if (path_off[0] != 0) return bfail(b, SFM_ERR_INVALID, "path_off[0] must be 0");
    for (size_t k = 0; k < M; ++k) {
        if (path_off[k + 1] < path_off[k]) return bfail(b, SFM_ERR_INVALID, "path_off must be non-decreasing (vehicle " + std::to_string(k) + ")");
        if (path_off[k + 1] - path_off[k] > SFM_BATCH_MAX_AUTOPILOT_POINTS)
            return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + " has " + std::to_string(path_off[k + 1] - path_off[k]) +
                                             " path points; a path takes up to " + std::to_string(SFM_BATCH_MAX_AUTOPILOT_POINTS));
    }
    for (int s = 0; s < b->B; ++s)
        if (b->boxes.item_off_h[s + 1] - b->boxes.item_off_h[s] >= (1 << AUTOPILOT_INDEX_BITS))
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(s) + " has too many vehicles for the autopilot's leader index");
    const size_t P = (size_t)path_off[M];
    if (P > 0 && (!px || !py)) return bfail(b, SFM_ERR_INVALID, "px or py is NULL");
    std::vector<float2> path(P > 0 ? P : 1, make_float2(0.f, 0.f));
    for (size_t p = 0; p < P; ++p) {
        if (!std::isfinite(px[p]) || !std::isfinite(py[p])) return bfail(b, SFM_ERR_INVALID, "path point " + std::to_string(p) + " is not finite");
        path[p] = make_float2(px[p], py[p]);
    }
    std::vector<AutopilotVehicle> set(M);
    for (size_t k = 0; k < M; ++k) {
        const float* v = settings + k * SFM_BATCH_AUTOPILOT_SETTINGS;
        AutopilotVehicle& o = set[k];
        memset(&o, 0, sizeof(o));
        float reach = 0.f;
        std::string why;
        if ((why = check_setting(k, "v0", v[0], true, &o.v0)).empty() && (why = check_setting(k, "T", v[1], false, &o.T)).empty() &&
            (why = check_setting(k, "s0", v[2], true, &o.s0)).empty() && (why = check_setting(k, "acc", v[3], true, &o.acc)).empty() &&
            (why = check_setting(k, "dec", v[4], true, &o.dec)).empty() && (why = check_setting(k, "brake", v[5], true, &o.brake)).empty() &&
            (why = check_setting(k, "half_width", v[6], false, &o.half_width)).empty() &&
            (why = check_setting(k, "front", v[7], false, &o.front)).empty() && (why = check_setting(k, "look", v[8], true, &o.look)).empty() &&
            (why = check_setting(k, "reach", v[9], true, &reach)).empty() &&
            (why = check_setting(k, "ped_margin", v[10], false, &o.ped_margin)).empty() &&
            (why = check_setting(k, "cos_max", v[11], true, &o.cos_max)).empty())
            why = check_setting(k, "sin_max", v[12], false, &o.sin_max);
        if (!why.empty()) return bfail(b, SFM_ERR_INVALID, why);
        if (o.brake < o.dec) return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": brake must be >= dec");
        if (o.cos_max > 1.0f) return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": cos_max must be <= 1");
        o.reach2 = (float)((double)reach * (double)reach);
        if (!std::isfinite(o.reach2)) return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": reach^2 is not finite in float32");
        if (flags[k] > 3) return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": flags must be a sum of 1 (loop) and 2 (ignore walkers)");
        o.flags = flags[k];
    }
    BatchAutopilotDev o;
    HIP_TRY(b, o.path_off.alloc(M + 1));
    HIP_TRY(b, o.path.alloc(path.size()));
    HIP_TRY(b, o.set.alloc(M));
    HIP_TRY(b, o.cursor.alloc(M));
    HIP_TRY(b, o.s_cursor.alloc(M));
    HIP_TRY(b, o.record.alloc(M * 8));
    HIP_TRY(b, hipMemcpy(o.path_off, path_off, sizeof(int) * (M + 1), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(o.path, path.data(), sizeof(float2) * path.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(o.set, set.data(), sizeof(AutopilotVehicle) * M, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemsetAsync(o.cursor, 0, sizeof(int) * M, b->stream));
    HIP_TRY(b, hipMemsetAsync(o.s_cursor, 0, sizeof(int) * M, b->stream));
    HIP_TRY(b, hipMemsetAsync(o.record, 0, sizeof(float) * M * 8, b->stream));
    // The commands.  Driving off: it is switched on, every command of kind 0.  Either way an autopiloted vehicle's command becomes
    // {0, 1, 0, 2} at once -- what the controller writes for a vehicle that stands -- so that it counts as driven (the restart
    // noise, sfm_batch_download_vehicle_driving) before the first controller launch too; the other entries stay as they are.
    const float4 stop = make_float4(0.f, 1.f, 0.f, 2.f);
    DevBuf<float4> cmd;
    PinnedBuf<float4> cmd_h;
    const bool drive = !b->drive.on;
    if (drive) {
        HIP_TRY(b, cmd.alloc(M));
        HIP_TRY(b, cmd_h.alloc(M));
        if (!b->v_done) HIP_TRY(b, b->v_done.create(hipEventDisableTiming));
        for (size_t k = 0; k < M; ++k) cmd_h[k] = path_off[k + 1] > path_off[k] ? stop : make_float4(0.f, 0.f, 0.f, 0.f);
        HIP_TRY(b, hipMemcpy(cmd, cmd_h, sizeof(float4) * M, hipMemcpyHostToDevice));
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and a launch in flight may still read the old buffers
    if (drive) {
        b->drive.cmd = std::move(cmd);
        b->drive.cmd_h = std::move(cmd_h);
        b->drive.pending = false;
        b->drive.on = true;
    } else {                                                     // (the stream is idle: a pending copy of the commands has landed)
        std::vector<float4> now(M);
        HIP_TRY(b, hipMemcpy(now.data(), b->drive.cmd, sizeof(float4) * M, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < M; ++k)
            if (path_off[k + 1] > path_off[k]) now[k] = b->drive.cmd_h[k] = stop;
        HIP_TRY(b, hipMemcpy(b->drive.cmd, now.data(), sizeof(float4) * M, hipMemcpyHostToDevice));
        b->drive.pending = false;
    }
    o.on = true;
    b->drive.ap = std::move(o);
    b->snap.on = false;                                          // (the snapshot does not hold these cursors)
    return SFM_OK;
}

int sfm_batch_download_vehicle_autopilot(SfmBatch* b, int32_t* cursor, float* record) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->drive.ap.on) return bfail(b, SFM_ERR_STATE, AUTOPILOT_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t M = (size_t)b->geo[2].K;
    if (cursor) HIP_TRY(b, hipMemcpy(cursor, b->drive.ap.cursor, sizeof(int) * M, hipMemcpyDeviceToHost));
    if (record) HIP_TRY(b, hipMemcpy(record, b->drive.ap.record, sizeof(float) * M * 8, hipMemcpyDeviceToHost));
    return SFM_OK;
}

int sfm_batch_vehicle_autopilot_launches(SfmBatch* b, long long* launches) {
    if (!b) return SFM_ERR_INVALID;
    if (!launches) return bfail(b, SFM_ERR_INVALID, "launches is NULL");
    *launches = b->drive.ap.on ? b->drive.ap.launches : 0;
    return SFM_OK;
}

}  // extern "C"
