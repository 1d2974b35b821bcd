// sfm_batch_drive_capi.hip -- host side of the batch's driven vehicles and vehicle observations: per-vehicle commands the ticks'
// vehicle prologue reads (drive_vehicle in sfm_interaction.h, sfm_batch.hip), and the one sensor that is centred on a vehicle
// (sfm_batch_vehicle_observe.hip).  Both refer to the device-side vehicles and are dropped with them (drop_batch_boxes in
// sfm_batch_capi.hip); their device pointers are handed out by sfm_batch_device_ptr (sfm_batch_sense_capi.hip).  The batch's types
// are in sfm_batch_host.h.
#include "sfm_batch_host.h"

using namespace sfm;

static bool driven_kind(float w) { return w == 1.0f || w == 2.0f; }

// the commands of a driving call: every array is there, and a driven vehicle's command is finite
static int check_vehicle_commands(SfmBatch* b, const float4* kinds, const uint8_t* kind, const float* a, const float* b_, const float* c) {
    const int M = b->geo[2].K;
    if (!a || !b_ || !c) return bfail(b, SFM_ERR_INVALID, "a, b or c is NULL");
    for (int k = 0; k < M; ++k) {
        const bool driven = kind ? kind[k] != 0 : driven_kind(kinds[k].w);
        if (driven && !(std::isfinite(a[k]) && std::isfinite(b_[k]) && std::isfinite(c[k])))
            return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": the command of a driven vehicle is not finite");
    }
    return SFM_OK;
}

extern "C" {

// Everything is checked before anything is sent or freed.
int sfm_batch_set_vehicle_driving(SfmBatch* b, const uint8_t* kind, const float* a, const float* b_, const float* c) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle driving: ") + NO_BOXES);
    const size_t M = (size_t)b->geo[2].K;
    if (kind) {
        for (size_t k = 0; k < M; ++k)
            if (kind[k] > 2)
                return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": kind must be 0 (not driven), 1 (velocity) or 2 (unicycle)");
        if ((rc = check_vehicle_commands(b, nullptr, kind, a, b_, c))) return rc;
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // a tick or a copy in flight may still read the buffers
    b->drive = {};
    if (!kind) return SFM_OK;
    HIP_TRY(b, b->drive.cmd.alloc(M));
    HIP_TRY(b, b->drive.cmd_h.alloc(M));
    if (!b->v_done) HIP_TRY(b, b->v_done.create(hipEventDisableTiming));
    for (size_t k = 0; k < M; ++k) b->drive.cmd_h[k] = make_float4(a[k], b_[k], c[k], (float)kind[k]);
    HIP_TRY(b, hipMemcpy(b->drive.cmd, b->drive.cmd_h, sizeof(float4) * M, hipMemcpyHostToDevice));
    b->drive.on = true;
    return SFM_OK;
}

int sfm_batch_set_vehicle_commands(SfmBatch* b, const float* a, const float* b_, const float* c) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->drive.on) return bfail(b, SFM_ERR_STATE, DRIVING_OFF);
    if ((rc = check_vehicle_commands(b, b->drive.cmd_h, nullptr, a, b_, c))) return rc;
    const size_t M = (size_t)b->geo[2].K;
    if (b->drive.pending) {                                      // the copy before this one may still read the pinned block
        HIP_TRY(b, hipEventSynchronize(b->v_done));
        b->drive.pending = false;
    }
    for (size_t k = 0; k < M; ++k) { b->drive.cmd_h[k].x = a[k]; b->drive.cmd_h[k].y = b_[k]; b->drive.cmd_h[k].z = c[k]; }
    HIP_TRY(b, hipMemcpyAsync(b->drive.cmd, b->drive.cmd_h, sizeof(float4) * M, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipEventRecord(b->v_done, b->stream));
    b->drive.pending = true;
    return SFM_OK;
}

int sfm_batch_download_vehicle_driving(SfmBatch* b, uint8_t* kind, float* a, float* b_, float* c, float* hx, float* hy, float* vx,
                                       float* vy) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->drive.on) return bfail(b, SFM_ERR_STATE, DRIVING_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t M = (size_t)b->geo[2].K;
    std::vector<float4> u(M), ctr(M);
    std::vector<float2> h(M);
    HIP_TRY(b, hipMemcpy(u.data(), b->drive.cmd, sizeof(float4) * M, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(ctr.data(), b->geo[2].ctr, sizeof(float4) * M, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(h.data(), b->boxes.rot, sizeof(float2) * M, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < M; ++k) {
        if (kind) kind[k] = u[k].w == 1.0f ? 1 : u[k].w == 2.0f ? 2 : 0;   // (what the tick makes of it)
        if (a) a[k] = u[k].x;
        if (b_) b_[k] = u[k].y;
        if (c) c[k] = u[k].z;
        if (hx) hx[k] = h[k].x;
        if (hy) hy[k] = h[k].y;
        if (vx) vx[k] = ctr[k].z;
        if (vy) vy[k] = ctr[k].w;
    }
    return SFM_OK;
}

// Vehicle observations.  Everything is checked before anything is allocated or freed.
int sfm_batch_set_vehicle_observation(SfmBatch* b, int k, const float* sense_range, int frame, const float* goal_x, const float* goal_y,
                                      const uint8_t* mask) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!sense_range) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a launch in flight may still write the buffer
        b->vobs = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle observations: ") + NO_BOXES);
    if (k < 1 || k > SFM_BATCH_MAX_OBS_NEIGHBOURS)
        return bfail(b, SFM_ERR_INVALID, "k must be 1 .. " + std::to_string(SFM_BATCH_MAX_OBS_NEIGHBOURS) + " neighbour slots, got " + std::to_string(k));
    if (frame != SFM_OBS_FRAME_WORLD && frame != SFM_OBS_FRAME_HEADING)
        return bfail(b, SFM_ERR_INVALID, "frame must be 0 (world axes) or 1 (the vehicle's heading frame), got " + std::to_string(frame));
    if ((goal_x == nullptr) != (goal_y == nullptr)) return bfail(b, SFM_ERR_INVALID, "goal_x and goal_y must be given together");
    std::vector<float> r2((size_t)b->B);
    for (size_t s = 0; s < r2.size(); ++s) {
        const std::string why = check_metres((int)s, "sense_range", sense_range[s], true, &r2[s]);
        if (!why.empty()) return bfail(b, SFM_ERR_INVALID, why);
    }
    const size_t M = (size_t)b->geo[2].K;
    std::vector<float2> goal(M, make_float2(0.f, 0.f));
    for (size_t v = 0; goal_x && v < M; ++v) {
        if (!std::isfinite(goal_x[v]) || !std::isfinite(goal_y[v]))
            return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(v) + ": its goal is not finite");
        goal[v] = make_float2(goal_x[v], goal_y[v]);
    }
    const size_t vals = M * (size_t)(SFM_BATCH_OBS_HEADER + 4 * k);
    BatchVehObsDev o;
    HIP_TRY(b, o.range2.alloc((size_t)b->B));
    HIP_TRY(b, hipMemcpy(o.range2, r2.data(), sizeof(float) * r2.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, o.goal.alloc(M));
    HIP_TRY(b, hipMemcpy(o.goal, goal.data(), sizeof(float2) * M, hipMemcpyHostToDevice));
    if (mask) {
        HIP_TRY(b, o.mask.alloc(M));
        HIP_TRY(b, hipMemcpy(o.mask, mask, M, hipMemcpyHostToDevice));
    }
    HIP_TRY(b, o.buf.alloc(vals));
    HIP_TRY(b, hipMemsetAsync(o.buf, 0, sizeof(float) * vals, b->stream));
    o.k = k;
    o.frame = frame;
    o.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fill; and a launch in flight may still write the old buffer
    b->vobs = std::move(o);
    return SFM_OK;
}

int sfm_batch_observe_vehicles(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->vobs.on) return bfail(b, SFM_ERR_STATE, VEHICLE_OBS_OFF);
    VehicleObserveArgs a{batch_scene_view(b), b->boxes.rot, b->vobs.range2, b->vobs.goal, b->vobs.mask /* null: every vehicle */,
                         b->vobs.buf, b->vobs.k, b->vobs.frame};
    HIP_TRY(b, launch_batch_vehicle_observe(a, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_vehicle_observations(SfmBatch* b, float* out) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->vobs.on) return bfail(b, SFM_ERR_STATE, VEHICLE_OBS_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (!out) return bfail(b, SFM_ERR_INVALID, "out is NULL");
    const size_t vals = (size_t)b->geo[2].K * (size_t)(SFM_BATCH_OBS_HEADER + 4 * b->vobs.k);
    HIP_TRY(b, hipMemcpy(out, b->vobs.buf, sizeof(float) * vals, hipMemcpyDeviceToHost));
    return SFM_OK;
}

}  // extern "C"
