// sfm_batch_vehicle_episode_capi.hip -- host side of the batch's vehicle episodes and vehicle respawns
// (sfm_batch_set_vehicle_episodes, sfm_batch_end_vehicle_step, sfm_batch_respawn_vehicles_device; the record and the rules are
// specified in include/sfm_hip.h): the settings and the agent lists, the launches (sfm_batch_vehicle_episode.hip), and the small
// launch every scene restart puts behind its own so that a restarted scene's vehicle episodes start over.  The batch's types are in
// sfm_batch_host.h; the episodes live inside the boxes they refer to (BatchBoxesDev::vep).
#include "sfm_batch_host.h"

using namespace sfm;

// a radius as sfm_batch_set_episodes takes it: finite, >= 0, at most 1e6 metres; *sq = float32(double(r) * r)
static int bfail_metres(SfmBatch* b, size_t s, const char* name, float r, float* sq) {
    const std::string why = check_metres((int)s, name, r, false, sq);
    return why.empty() ? SFM_OK : bfail(b, SFM_ERR_INVALID, why);
}

int sfm::batch_vehicle_episode_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes) {
    const BatchVehEpisodeDev& e = b->boxes.vep;
    if (!e.on || scenes <= 0 || b->geo[2].K == 0) return SFM_OK;
    HIP_TRY(b, launch_batch_vehicle_episode_restart(d_list, d_mask, b->geo_item_off[2], e.age, e.prev, scenes, b->stream));
    return SFM_OK;
}

// What sfm_batch_respawn_vehicles_device refuses before anything is launched, in this order; *mask: the mask the launch reads.
static int respawn_checks(SfmBatch* b, const uint8_t** mask) {
    if (!b->snap.on) return bfail(b, SFM_ERR_STATE, NO_SNAPSHOT);
    if (!*mask) {
        if (!b->boxes.vep.on)
            return bfail(b, SFM_ERR_INVALID, "d_mask is NULL (device memory, one byte per vehicle) and vehicle episodes are off, so there is no "
                                             "vehicle_done to take");
        *mask = b->boxes.vep.done;
    }
    if (b->tracks.on)
        return bfail(b, SFM_ERR_STATE, "vehicle tracks are set: a tracked vehicle's time belongs to its scene's clock, which a vehicle respawn "
                                       "does not move (restart the scene, or drop the tracks with sfm_batch_set_vehicle_tracks)");
    return SFM_OK;
}

static int respawn_launch(SfmBatch* b, const uint8_t* mask) {
    if (!b->boxes.on || b->geo[2].K == 0) return SFM_OK;         // no device-side vehicle: nothing to copy
    const BatchGeoDev& g = b->geo[2];
    VehicleRespawnArgs a;
    memset(&a, 0, sizeof(a));
    a.mask = mask;
    a.item_off = b->geo_item_off[2]; a.veh_off = g.off;
    a.ctr = g.ctr; a.s_ctr = b->snap.ctr;
    a.rot = b->boxes.rot; a.s_rot = b->snap.rot;
    if (g.P > 0) { a.pts = g.pts; a.s_pts = b->snap.pts; }
    if (b->drive.ap.on) { a.cursor = b->drive.ap.cursor; a.s_cursor = b->drive.ap.s_cursor; }
    if (b->boxes.vep.on) { a.age = b->boxes.vep.age; a.prev_goal_d2 = b->boxes.vep.prev; }
    HIP_TRY(b, launch_batch_vehicle_respawn(a, b->B, b->stream));
    return SFM_OK;
}

extern "C" {

// Everything is checked, and the new buffers are built, before the old ones are dropped: a refusal changes nothing.
int sfm_batch_set_vehicle_episodes(SfmBatch* b, const uint8_t* agents, const float* goal_x, const float* goal_y, const float* extent,
                                   const float* goal_radius, const float* ped_radius, const float* veh_radius,
                                   const float* wall_radius, const int32_t* max_steps) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!agents) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // an end_vehicle_step, a respawn or a restart in flight may still write the buffers
        b->boxes.vep = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!b->boxes.on) return bfail(b, SFM_ERR_STATE, std::string("vehicle episodes: ") + NO_BOXES);
    if (!goal_x || !goal_y || !extent) return bfail(b, SFM_ERR_INVALID, "goal_x, goal_y or extent is NULL");
    if (!goal_radius || !ped_radius || !veh_radius || !wall_radius || !max_steps)
        return bfail(b, SFM_ERR_INVALID, "goal_radius, ped_radius, veh_radius, wall_radius or max_steps is NULL");
    const size_t B = (size_t)b->B, M = (size_t)b->geo[2].K;
    const std::vector<int32_t>& off = b->boxes.item_off_h;
    std::vector<VehicleEpisodeScene> set(B);
    std::vector<int> agent_off(B + 1, 0), agent_veh;
    std::vector<float4> goal_ext(M > 0 ? M : 1, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t s = 0; s < B; ++s) {
        set[s] = VehicleEpisodeScene{max_steps[s], 0.f, 0.f, 0.f, 0.f, {0, 0, 0}};
        if ((rc = bfail_metres(b, s, "goal_radius", goal_radius[s], &set[s].goal_r2))) return rc;
        if ((rc = bfail_metres(b, s, "ped_radius", ped_radius[s], &set[s].ped_r2))) return rc;
        if ((rc = bfail_metres(b, s, "veh_radius", veh_radius[s], &set[s].veh_r2))) return rc;
        if ((rc = bfail_metres(b, s, "wall_radius", wall_radius[s], &set[s].wall_r2))) return rc;
        if (max_steps[s] < 0) return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(s) + ": max_steps must be >= 0 (0: no time limit)");
        for (int k = off[s]; k < off[s + 1]; ++k) {
            if (!agents[k]) continue;
            const float ex = extent[2 * (size_t)k], ey = extent[2 * (size_t)k + 1];
            if (!std::isfinite(goal_x[k]) || !std::isfinite(goal_y[k]))
                return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": the goal of an agent vehicle must be finite");
            if (!std::isfinite(ex) || !std::isfinite(ey) || !(ex > 0.f) || !(ey > 0.f) || ex > SFM_BATCH_MAX_SENSE_RANGE ||
                ey > SFM_BATCH_MAX_SENSE_RANGE)
                return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": the half-extents of an agent vehicle must be finite, > 0 and <= 1e6 metres");
            goal_ext[k] = make_float4(goal_x[k], goal_y[k], ex, ey);
            agent_veh.push_back(k);
        }
        agent_off[s + 1] = (int)agent_veh.size();
    }
    BatchVehEpisodeDev e;
    HIP_TRY(b, e.set.alloc(B)); HIP_TRY(b, e.agent_off.alloc(B + 1)); HIP_TRY(b, e.agent_veh.alloc(agent_veh.size()));
    HIP_TRY(b, e.scene_done.alloc(B));
    HIP_TRY(b, hipMemcpy(e.set, set.data(), sizeof(VehicleEpisodeScene) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(e.agent_off, agent_off.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
    if (!agent_veh.empty()) HIP_TRY(b, hipMemcpy(e.agent_veh, agent_veh.data(), sizeof(int) * agent_veh.size(), hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemsetAsync(e.scene_done, 0, B, b->stream));
    if (M > 0) {
        HIP_TRY(b, e.goal_ext.alloc(M)); HIP_TRY(b, e.age.alloc(M)); HIP_TRY(b, e.prev.alloc(M));
        HIP_TRY(b, e.record.alloc(8 * M)); HIP_TRY(b, e.done.alloc(M));
        const std::vector<float> nan(M, std::numeric_limits<float>::quiet_NaN());
        HIP_TRY(b, hipMemcpy(e.goal_ext, goal_ext.data(), sizeof(float4) * M, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(e.prev, nan.data(), sizeof(float) * M, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemsetAsync(e.age, 0, sizeof(int) * M, b->stream));
        HIP_TRY(b, hipMemsetAsync(e.record, 0, sizeof(float) * 8 * M, b->stream));
        HIP_TRY(b, hipMemsetAsync(e.done, 0, M, b->stream));
    }
    e.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and a launch in flight may still write the old buffers
    b->boxes.vep = std::move(e);
    return SFM_OK;
}

int sfm_batch_end_vehicle_step(SfmBatch* b, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    const uint32_t both = SFM_END_VEHICLE_STEP_AUTO_RESTART | SFM_END_VEHICLE_STEP_AUTO_RESPAWN;
    if (flags & ~both) return bfail(b, SFM_ERR_INVALID, "sfm_batch_end_vehicle_step takes SFM_END_VEHICLE_STEP_AUTO_RESTART or _AUTO_RESPAWN only");
    if ((flags & both) == both)
        return bfail(b, SFM_ERR_INVALID, "SFM_END_VEHICLE_STEP_AUTO_RESTART and _AUTO_RESPAWN together: a restarted scene has nothing left to respawn");
    if (!b->boxes.vep.on) return bfail(b, SFM_ERR_STATE, VEHICLE_EPISODES_OFF);
    const bool restart = (flags & SFM_END_VEHICLE_STEP_AUTO_RESTART) != 0, respawn = (flags & SFM_END_VEHICLE_STEP_AUTO_RESPAWN) != 0;
    const BatchVehEpisodeDev& e = b->boxes.vep;
    long long shift = 0;                                         // the follow-up's refusals come first: nothing is launched then
    const uint8_t* mask = e.done;
    if (restart && (rc = batch_restart_checks(b, nullptr, "", &shift))) return rc;
    if (respawn && (rc = respawn_checks(b, &mask))) return rc;
    if (b->geo[2].K > 0) {
        VehicleEpisodeArgs a;
        static_cast<BatchSceneView&>(a) = batch_scene_view(b);
        a.rot = b->boxes.rot; a.set = e.set; a.agent_off = e.agent_off; a.agent_veh = e.agent_veh; a.goal_ext = e.goal_ext;
        a.age = e.age; a.prev_goal_d2 = e.prev; a.record = e.record; a.done = e.done; a.scene_done = e.scene_done;
        HIP_TRY(b, launch_batch_vehicle_episode(a, b->B, b->stream));
    }
    if (restart) return batch_restart_device(b, e.scene_done, shift);
    return respawn ? respawn_launch(b, mask) : SFM_OK;
}

int sfm_batch_download_vehicle_episodes(SfmBatch* b, float* record, uint8_t* vehicle_done, uint8_t* vehicle_scene_done) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->boxes.vep.on) return bfail(b, SFM_ERR_STATE, VEHICLE_EPISODES_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t M = (size_t)b->geo[2].K;
    const BatchVehEpisodeDev& e = b->boxes.vep;
    if (record && M > 0) HIP_TRY(b, hipMemcpy(record, e.record, sizeof(float) * 8 * M, hipMemcpyDeviceToHost));
    if (vehicle_done && M > 0) HIP_TRY(b, hipMemcpy(vehicle_done, e.done, M, hipMemcpyDeviceToHost));
    if (vehicle_scene_done) HIP_TRY(b, hipMemcpy(vehicle_scene_done, e.scene_done, (size_t)b->B, hipMemcpyDeviceToHost));
    return SFM_OK;
}

// ONE launch of B workgroups, the choice read on the device.
int sfm_batch_respawn_vehicles_device(SfmBatch* b, const uint8_t* d_mask) {
    int rc = bbind(b);
    if (rc) return rc;
    if ((rc = respawn_checks(b, &d_mask))) return rc;
    return respawn_launch(b, d_mask);
}

}  // extern "C"
