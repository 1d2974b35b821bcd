// sfm_batch_row_episode_capi.hip -- host side of the batch's row episodes and row respawns (sfm_batch_set_row_episodes,
// sfm_batch_end_row_step, sfm_batch_respawn_rows_device; the records and the rules are specified in include/sfm_hip.h): the settings
// and the agent lists, the launches (sfm_batch_row_episode.hip), and the small launch every scene restart puts behind its own so
// that a restarted scene's row episodes start over.  The batch's types are in sfm_batch_host.h.
#include "sfm_batch_host.h"

using namespace sfm;

// a radius as sfm_batch_set_episodes takes it: finite, >= 0, at most 1e6 metres; *sq = float32(double(r) * r)
static int bfail_metres(SfmBatch* b, size_t s, const char* name, float r, float* sq) {
    const std::string why = check_metres((int)s, name, r, false, sq);
    return why.empty() ? SFM_OK : bfail(b, SFM_ERR_INVALID, why);
}

int sfm::batch_row_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes) {
    const BatchRowEpisodeDev& e = b->ep.rows;
    if (!e.on || scenes <= 0 || b->n_total == 0) return SFM_OK;
    HIP_TRY(b, launch_batch_row_restart(d_list, d_mask, b->d_scene_off, e.age, e.prev, scenes, b->stream));
    return SFM_OK;
}

// What sfm_batch_respawn_rows_device refuses before anything is launched, in this order; *mask: the mask the launch reads.
static int respawn_checks(SfmBatch* b, const uint8_t** mask) {
    if (!b->snap.on) return bfail(b, SFM_ERR_STATE, NO_SNAPSHOT);
    if (!*mask) {
        if (!b->ep.rows.on)
            return bfail(b, SFM_ERR_INVALID, "d_mask is NULL (device memory, one byte per row) and row episodes are off, so there is no row_done to take");
        *mask = b->ep.rows.done;
    }
    if (b->spawns.on)
        return bfail(b, SFM_ERR_STATE, "a spawn schedule is set: a respawned row would have to enter the birth machine again, which a row "
                                       "respawn does not do (restart the scene, or drop the schedule with sfm_batch_set_mode_fsm)");
    if (b->routes.on)
        return bfail(b, SFM_ERR_STATE, "routes are set: a respawned row would have to be planned again, which a row respawn does not do "
                                       "(restart the scene, or drop the routes with sfm_batch_set_routes)");
    return SFM_OK;
}

static int respawn_launch(SfmBatch* b, const uint8_t* mask) {
    if (b->n_total == 0) return SFM_OK;
    RowRespawnArgs a;
    memset(&a, 0, sizeof(a));
    a.v = batch_scene_view(b);
    a.mask = mask;
    a.pk = b->pk; a.s_pk = b->snap.pk;
    if (b->z3) { a.zv = b->zv; a.s_zv = b->snap.zv; }
    a.own = b->own; a.s_own = b->snap.own;
    a.draws = b->draws; a.s_draws = b->snap.draws;
    if (b->modes.on) {
        a.mode = b->modes.mode; a.s_mode = b->snap.mode;
        a.target = b->modes.target; a.s_target = b->snap.target;
        a.cursor = b->modes.cursor; a.s_cursor = b->snap.cursor;
    }
    if (b->ep.rows.on) { a.row_age = b->ep.rows.age; a.row_prev_goal_d2 = b->ep.rows.prev; }
    const BatchNoiseDev& z = b->noise;
    if (z.on) {
        a.seed = z.seed;
        a.row_resets = z.row_resets;
        a.fallbacks = z.row_fallbacks;
        a.pos_box = z.pos_box;
        a.goal_box = z.goal_box;                                   // null: the goals stay
        a.gap2 = z.gap2;
        a.tries = z.tries;
    }
    HIP_TRY(b, launch_batch_row_respawn(a, b->B, b->stream));
    return SFM_OK;
}

extern "C" {

// Everything is checked, and the new buffers are built, before the old ones are dropped: a refusal changes nothing.
int sfm_batch_set_row_episodes(SfmBatch* b, const uint8_t* agents, const float* goal_radius, const float* ped_radius, const float* veh_radius,
                               const int32_t* max_steps) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!agents) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // an end_row_step, a respawn or a restart in flight may still write the buffers
        b->ep.rows = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (!goal_radius || !ped_radius || !veh_radius || !max_steps)
        return bfail(b, SFM_ERR_INVALID, "goal_radius, ped_radius, veh_radius or max_steps is NULL");
    const size_t B = (size_t)b->B, n = (size_t)b->n_total;
    const std::vector<int32_t>& off = b->scene_off_h;
    std::vector<BatchEpisodeScene> set(B);
    std::vector<int> agent_off(B + 1, 0), agent_rows;
    for (size_t s = 0; s < B; ++s) {
        set[s] = BatchEpisodeScene{-1, max_steps[s], 0.f, 0.f, 0.f, {0, 0, 0}};
        if ((rc = bfail_metres(b, s, "goal_radius", goal_radius[s], &set[s].goal_r2))) return rc;
        if ((rc = bfail_metres(b, s, "ped_radius", ped_radius[s], &set[s].ped_r2))) return rc;
        if ((rc = bfail_metres(b, s, "veh_radius", veh_radius[s], &set[s].veh_r2))) return rc;
        if (max_steps[s] < 0) return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(s) + ": max_steps must be >= 0 (0: no time limit)");
        for (int i = off[s]; i < off[s + 1]; ++i)
            if (agents[i]) agent_rows.push_back(i - off[s]);
        agent_off[s + 1] = (int)agent_rows.size();
    }
    BatchRowEpisodeDev e;
    HIP_TRY(b, e.set.alloc(B)); HIP_TRY(b, e.agent_off.alloc(B + 1)); HIP_TRY(b, e.agent_rows.alloc(agent_rows.size()));
    HIP_TRY(b, e.age.alloc(n)); HIP_TRY(b, e.prev.alloc(n)); HIP_TRY(b, e.record.alloc(8 * n)); HIP_TRY(b, e.done.alloc(n));
    HIP_TRY(b, hipMemcpy(e.set, set.data(), sizeof(BatchEpisodeScene) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(e.agent_off, agent_off.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
    if (!agent_rows.empty()) HIP_TRY(b, hipMemcpy(e.agent_rows, agent_rows.data(), sizeof(int) * agent_rows.size(), hipMemcpyHostToDevice));
    if (n > 0) {
        const std::vector<float> nan(n, std::numeric_limits<float>::quiet_NaN());
        HIP_TRY(b, hipMemcpy(e.prev, nan.data(), sizeof(float) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemsetAsync(e.age, 0, sizeof(int) * n, b->stream));
        HIP_TRY(b, hipMemsetAsync(e.record, 0, sizeof(float) * 8 * n, b->stream));
        HIP_TRY(b, hipMemsetAsync(e.done, 0, n, b->stream));
    }
    e.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and a launch in flight may still write the old buffers
    b->ep.rows = std::move(e);
    return SFM_OK;
}

int sfm_batch_end_row_step(SfmBatch* b, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    if (flags & ~(uint32_t)SFM_END_ROW_STEP_AUTO_RESPAWN)
        return bfail(b, SFM_ERR_INVALID, "sfm_batch_end_row_step takes SFM_END_ROW_STEP_AUTO_RESPAWN only");
    if (!b->ep.rows.on) return bfail(b, SFM_ERR_STATE, ROW_EPISODES_OFF);
    const bool respawn = (flags & SFM_END_ROW_STEP_AUTO_RESPAWN) != 0;
    const uint8_t* mask = b->ep.rows.done;                         // the respawn's refusals come first: nothing is launched then
    if (respawn && (rc = respawn_checks(b, &mask))) return rc;
    if (b->n_total == 0) return SFM_OK;
    const BatchRowEpisodeDev& e = b->ep.rows;
    RowEpisodeArgs a;
    static_cast<BatchSceneView&>(a) = batch_scene_view(b);
    a.set = e.set; a.agent_off = e.agent_off; a.agent_rows = e.agent_rows;
    a.row_age = e.age; a.row_prev_goal_d2 = e.prev; a.record = e.record; a.row_done = e.done;
    HIP_TRY(b, launch_batch_row_episode(a, b->B, b->stream));
    return respawn ? respawn_launch(b, mask) : SFM_OK;
}

int sfm_batch_download_row_episodes(SfmBatch* b, float* record, uint8_t* row_done, int32_t* row_age, float* row_prev_goal_d2) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->ep.rows.on) return bfail(b, SFM_ERR_STATE, ROW_EPISODES_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total;
    if (n == 0) return SFM_OK;
    const BatchRowEpisodeDev& e = b->ep.rows;
    if (record) HIP_TRY(b, hipMemcpy(record, e.record, sizeof(float) * 8 * n, hipMemcpyDeviceToHost));
    if (row_done) HIP_TRY(b, hipMemcpy(row_done, e.done, n, hipMemcpyDeviceToHost));
    if (row_age) HIP_TRY(b, hipMemcpy(row_age, e.age, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (row_prev_goal_d2) HIP_TRY(b, hipMemcpy(row_prev_goal_d2, e.prev, sizeof(float) * n, hipMemcpyDeviceToHost));
    return SFM_OK;
}

// ONE launch of B workgroups, the choice read on the device.
int sfm_batch_respawn_rows_device(SfmBatch* b, const uint8_t* d_mask) {
    int rc = bbind(b);
    if (rc) return rc;
    if ((rc = respawn_checks(b, &d_mask))) return rc;
    return respawn_launch(b, d_mask);
}

int sfm_batch_download_row_respawns(SfmBatch* b, uint32_t* row_resets, uint32_t* fallbacks) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->noise.on) return bfail(b, SFM_ERR_STATE, NOISE_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    if (row_resets && n > 0) HIP_TRY(b, hipMemcpy(row_resets, b->noise.row_resets, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (fallbacks) HIP_TRY(b, hipMemcpy(fallbacks, b->noise.row_fallbacks, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
    return SFM_OK;
}

}  // extern "C"
