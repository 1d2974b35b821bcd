// sfm_batch_reset_capi.hip -- host side of the batch's restart noise (sfm_batch_set_restart_noise; the rule is specified in
// include/sfm_hip.h): the settings, the two per-scene counters, and the launch every restart path puts right behind
// launch_batch_restart (sfm_batch_reset.hip).  The batch's types are in sfm_batch_host.h; the restarts themselves in sfm_batch_capi.hip.
#include "sfm_batch_host.h"

using namespace sfm;

// one half-extent of a box, or a gap: finite, >= 0 and <= SFM_BATCH_MAX_SENSE_RANGE
static bool extent_ok(float v) { return std::isfinite(v) && v >= 0.f && v <= SFM_BATCH_MAX_SENSE_RANGE; }

int sfm::batch_restart_noise(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes) {
    const BatchNoiseDev& z = b->noise;
    if (!z.on || scenes <= 0) return SFM_OK;
    RestartNoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.v = batch_scene_view(b);
    a.list = d_list;
    a.mask = d_mask;
    a.pk = b->pk;
    a.own = b->own;
    a.seed = z.seed;
    a.resets = z.resets;
    a.fallbacks = z.fallbacks;
    a.pos_box = z.pos_box;
    a.goal_box = z.goal_box;                                       // null: the goals stay
    a.gap2 = z.gap2;
    a.tries = z.tries;
    if (z.delay && b->tracks.on && b->boxes.on) {                  // (the delays are dropped with the tracks: both hold here)
        a.delay = z.delay;
        a.first = b->tracks.first;
        a.trk = BatchTracks{b->tracks.off, b->tracks.first, b->tracks.key, b->tracks.rot, b->tracks.tick};   // placed as the next tick reads them
        a.veh_local = b->boxes.local;
        a.veh_ctr = b->geo[2].ctr;
        a.veh_pts = b->geo[2].pts;
        if (b->drive.on) a.veh_cmd = b->drive.cmd;                 // (driven vehicles keep their snapshot pose)
        b->tracks.first_stale = true;                             // how far a first tick moved is known on the device only
    }
    HIP_TRY(b, launch_batch_restart_noise(a, scenes, b->stream));
    return SFM_OK;
}

extern "C" {

// Everything is checked, and the new buffers are built, before the old ones are dropped: a refusal changes nothing.
int sfm_batch_set_restart_noise(SfmBatch* b, const uint32_t* seeds, const float* pos_hx, const float* pos_hy, const float* goal_hx,
                                const float* goal_hy, const float* min_gap, const float* point_gap, int tries, const int32_t* track_delay) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!seeds) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a restart in flight may still read the buffers
        b->noise = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    if (tries < 1 || tries > SFM_BATCH_MAX_RESTART_TRIES)
        return bfail(b, SFM_ERR_INVALID, "tries must be 1 .. " + std::to_string(SFM_BATCH_MAX_RESTART_TRIES) + ", got " + std::to_string(tries));
    if (n > 0 && (!pos_hx || !pos_hy)) return bfail(b, SFM_ERR_INVALID, "pos_hx or pos_hy is NULL");
    if ((goal_hx == nullptr) != (goal_hy == nullptr)) return bfail(b, SFM_ERR_INVALID, "goal_hx and goal_hy must be given together");
    if (!min_gap || !point_gap) return bfail(b, SFM_ERR_INVALID, "min_gap or point_gap is NULL");
    std::vector<float2> pos(n), goal(goal_hx ? n : 0), gap2(B);
    for (size_t i = 0; i < n; ++i) {
        if (!extent_ok(pos_hx[i]) || !extent_ok(pos_hy[i]) || (goal_hx && (!extent_ok(goal_hx[i]) || !extent_ok(goal_hy[i]))))
            return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": the half-extents of a box must be finite, >= 0 and <= 1e6 metres");
        pos[i] = make_float2(pos_hx[i], pos_hy[i]);
        if (goal_hx) goal[i] = make_float2(goal_hx[i], goal_hy[i]);
    }
    for (size_t s = 0; s < B; ++s) {
        std::string why = check_metres((int)s, "min_gap", min_gap[s], false, &gap2[s].x);
        if (why.empty()) why = check_metres((int)s, "point_gap", point_gap[s], false, &gap2[s].y);
        if (!why.empty()) return bfail(b, SFM_ERR_INVALID, why);
    }
    const size_t M = track_delay ? (size_t)b->geo[2].K : 0;
    long long max_delay = 0;
    if (track_delay) {
        if (!b->tracks.on)
            return bfail(b, SFM_ERR_STATE, "track_delay needs vehicle tracks: call sfm_batch_set_vehicle_tracks first (or pass track_delay = NULL)");
        for (size_t k = 0; k < M; ++k) {
            if (track_delay[k] < 0) return bfail(b, SFM_ERR_INVALID, "vehicle " + std::to_string(k) + ": track_delay must be >= 0");
            max_delay = std::max(max_delay, (long long)track_delay[k]);
        }
    }
    BatchNoiseDev z;
    HIP_TRY(b, z.seed.alloc(B)); HIP_TRY(b, z.resets.alloc(B)); HIP_TRY(b, z.fallbacks.alloc(B)); HIP_TRY(b, z.gap2.alloc(B));
    HIP_TRY(b, hipMemcpy(z.seed, seeds, sizeof(uint32_t) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(z.gap2, gap2.data(), sizeof(float2) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemsetAsync(z.resets, 0, sizeof(uint32_t) * B, b->stream));
    HIP_TRY(b, hipMemsetAsync(z.fallbacks, 0, sizeof(uint32_t) * B, b->stream));
    HIP_TRY(b, z.row_fallbacks.alloc(B));                       // the row respawns' counters (sfm_batch_respawn_rows_device)
    HIP_TRY(b, hipMemsetAsync(z.row_fallbacks, 0, sizeof(uint32_t) * B, b->stream));
    if (n > 0) {
        HIP_TRY(b, z.row_resets.alloc(n));
        HIP_TRY(b, hipMemsetAsync(z.row_resets, 0, sizeof(uint32_t) * n, b->stream));
        HIP_TRY(b, z.pos_box.alloc(n));
        HIP_TRY(b, hipMemcpy(z.pos_box, pos.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
        if (goal_hx) {
            HIP_TRY(b, z.goal_box.alloc(n));
            HIP_TRY(b, hipMemcpy(z.goal_box, goal.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
        }
    }
    if (M > 0 && max_delay > 0) {                                  // (all delays 0: no traffic timing, nothing to keep)
        HIP_TRY(b, z.delay.alloc(M));
        HIP_TRY(b, hipMemcpy(z.delay, track_delay, sizeof(int) * M, hipMemcpyHostToDevice));
        z.max_delay = max_delay;
    }
    z.tries = tries;
    z.on = true;
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and a restart in flight may still read the old buffers
    b->noise = std::move(z);
    return SFM_OK;
}

int sfm_batch_download_restart_noise(SfmBatch* b, uint32_t* resets, uint32_t* fallbacks) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->noise.on) return bfail(b, SFM_ERR_STATE, NOISE_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t B = (size_t)b->B;
    if (resets) HIP_TRY(b, hipMemcpy(resets, b->noise.resets, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
    if (fallbacks) HIP_TRY(b, hipMemcpy(fallbacks, b->noise.fallbacks, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
    return SFM_OK;
}

}  // extern "C"
