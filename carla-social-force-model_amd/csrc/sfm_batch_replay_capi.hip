// sfm_batch_replay_capi.hip -- host side of the batch's observed tracks (sfm_batch_set_observed, sfm_batch_run_observed,
// sfm_batch_score, sfm_batch_download_scores; the rules are specified in include/sfm_hip.h): the recording and the roles go to the
// device once, a run launches one frame kernel (sfm_batch_replay.hip) per observed frame between the ticks, and the scores stay on
// the device until they are asked for.  The batch's types are in sfm_batch_host.h; the ticks themselves in sfm_batch_capi.hip.
#include "sfm_batch_host.h"

using namespace sfm;

// 1 / (every * step_length) of one scene, formed in double and rounded once; false: the product or its reciprocal is not finite and
// positive in fp32
static bool frame_rate(int every, float dt, float* inv_h) {
    const double h = (double)every * (double)dt;
    const float hf = (float)h, inv = (float)(1.0 / h);
    if (!std::isfinite(hf) || !(hf > 0.f) || !std::isfinite(inv) || !(inv > 0.f)) return false;
    *inv_h = inv;
    return true;
}

static int frame_rates(SfmBatch* b, int every, const float* dt, std::vector<float>* inv_h) {
    inv_h->resize((size_t)b->B);
    for (int k = 0; k < b->B; ++k)
        if (!frame_rate(every, dt[k], &(*inv_h)[k]))
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": every * step_length must be finite and positive in fp32 (every " +
                                             std::to_string(every) + ", step_length " + std::to_string(dt[k]) + ")");
    return SFM_OK;
}

int sfm::batch_replay_step_lengths(SfmBatch* b, const float* dt) {
    if (!b->replay.on) return SFM_OK;
    std::vector<float> inv_h;
    int rc = frame_rates(b, b->replay.every, dt, &inv_h);
    if (rc) return rc;
    HIP_TRY(b, hipMemcpy(b->replay.inv_h, inv_h.data(), sizeof(float) * inv_h.size(), hipMemcpyHostToDevice));
    return SFM_OK;
}

extern "C" {

// Everything is checked, and the new buffers are built, before the old ones are dropped: a refusal changes nothing.
int sfm_batch_set_observed(SfmBatch* b, const int64_t* obs_off, const int32_t* frames, const float* obs_xy, const uint8_t* role,
                           const float* v0_xy, int every) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!obs_off) {
        HIP_TRY(b, hipStreamSynchronize(b->stream));             // a frame kernel in flight may still read the buffers
        b->replay = {};
        return SFM_OK;
    }
    if (!b->have_state) return bfail(b, SFM_ERR_STATE, NO_STATE);
    if (b->z3) return bfail(b, SFM_ERR_INVALID, "observed tracks are planar: the batch is 3-D (upload a planar state)");
    if (b->modes.on || b->spawns.on)
        return bfail(b, SFM_ERR_STATE, "observed tracks cannot be set while modes or a spawn schedule are set: both own parking and birth "
                                       "(switch them off with sfm_batch_set_mode_fsm(mode = NULL))");
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    if (every < 1) return bfail(b, SFM_ERR_INVALID, "every must be >= 1 tick between two observed frames, got " + std::to_string(every));
    if (!frames) return bfail(b, SFM_ERR_INVALID, "frames is NULL");
    if (n > 0 && !role) return bfail(b, SFM_ERR_INVALID, "role is NULL");
    if (obs_off[0] != 0) return bfail(b, SFM_ERR_INVALID, "obs_off[0] must be 0");
    const std::vector<int32_t>& so = b->scene_off_h;
    for (size_t k = 0; k < B; ++k) {
        if (frames[k] < 0 || frames[k] > SFM_BATCH_MAX_OBSERVED_FRAMES)
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": frames must be 0 .. " + std::to_string(SFM_BATCH_MAX_OBSERVED_FRAMES) +
                                             ", got " + std::to_string(frames[k]));
        if (obs_off[k + 1] - obs_off[k] != (int64_t)frames[k] * (so[k + 1] - so[k]))
            return bfail(b, SFM_ERR_INVALID, "scene " + std::to_string(k) + ": obs_off must advance by frames * rows of the scene");
    }
    const size_t total = (size_t)obs_off[B];
    if (total * sizeof(float2) > SFM_BATCH_MAX_RECORD_BYTES)
        return bfail(b, SFM_ERR_INVALID, "the observed frames need " + std::to_string(total * sizeof(float2)) + " bytes, more than the " +
                                         std::to_string(SFM_BATCH_MAX_RECORD_BYTES) + " one batch may hold");
    if (total > 0 && !obs_xy) return bfail(b, SFM_ERR_INVALID, "obs_xy is NULL");
    for (size_t i = 0; i < n; ++i) {
        if (role[i] > SFM_ROLE_SCORED)
            return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": role must be 0 (not part of the data), 1 (replayed) or 2 (scored)");
        if (v0_xy) {
            const float vx = v0_xy[2 * i], vy = v0_xy[2 * i + 1];
            if (std::isnan(vx) != std::isnan(vy) || std::isinf(vx) || std::isinf(vy))
                return bfail(b, SFM_ERR_INVALID, "row " + std::to_string(i) + ": v0 must be finite, or NaN in both components (take it from the track)");
        }
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<int2> span(n, make_int2(1, 0));                     // empty: never seen
    for (size_t k = 0; k < B; ++k) {
        const size_t nb = (size_t)(so[k + 1] - so[k]);
        for (size_t f = 0; f < (size_t)frames[k]; ++f)
            for (size_t i = 0; i < nb; ++i) {
                const size_t e = (size_t)obs_off[k] + f * nb + i;
                const float x = obs_xy[2 * e], y = obs_xy[2 * e + 1];
                const std::string at = "scene " + std::to_string(k) + ", frame " + std::to_string(f) + ", row " + std::to_string(i);
                if (std::isnan(x) != std::isnan(y))
                    return bfail(b, SFM_ERR_INVALID, at + ": an observed position must be NaN in both components (not seen) or in none");
                if (std::isnan(x)) continue;
                if (!(std::fabs(x) <= SFM_BATCH_MAX_SENSE_RANGE) || !(std::fabs(y) <= SFM_BATCH_MAX_SENSE_RANGE))
                    return bfail(b, SFM_ERR_INVALID, at + ": an observed position must be finite and within 1e6 metres");
                int2& s = span[(size_t)so[k] + i];
                if (s.x > s.y) s = make_int2((int)f, (int)f); else s.y = (int)f;
            }
    }
    std::vector<float> inv_h;
    if ((rc = frame_rates(b, every, b->dt_h.data(), &inv_h))) return rc;
    std::vector<long long> off(B);
    for (size_t k = 0; k < B; ++k) off[k] = (long long)obs_off[k];
    std::vector<float2> v0(n, make_float2(nan, nan));
    if (v0_xy) for (size_t i = 0; i < n; ++i) v0[i] = make_float2(v0_xy[2 * i], v0_xy[2 * i + 1]);

    BatchReplayDev z;
    HIP_TRY(b, z.obs_off.alloc(B)); HIP_TRY(b, z.frames.alloc(B)); HIP_TRY(b, z.inv_h.alloc(B));
    HIP_TRY(b, z.scene.alloc(B * SFM_BATCH_SCENE_SCORE_WIDTH));
    HIP_TRY(b, hipMemcpy(z.obs_off, off.data(), sizeof(long long) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(z.frames, frames, sizeof(int) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(z.inv_h, inv_h.data(), sizeof(float) * B, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemsetAsync(z.scene, 0, sizeof(float) * B * SFM_BATCH_SCENE_SCORE_WIDTH, b->stream));
    if (total > 0) {
        HIP_TRY(b, z.obs.alloc(total));
        HIP_TRY(b, hipMemcpy(z.obs, obs_xy, sizeof(float2) * total, hipMemcpyHostToDevice));
    }
    if (n > 0) {
        HIP_TRY(b, z.role.alloc(n)); HIP_TRY(b, z.span.alloc(n)); HIP_TRY(b, z.v0.alloc(n)); HIP_TRY(b, z.score.alloc(n));
        HIP_TRY(b, hipMemcpy(z.role, role, n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(z.span, span.data(), sizeof(int2) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemcpy(z.v0, v0.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
        HIP_TRY(b, hipMemsetAsync(z.score, 0, sizeof(float4) * n, b->stream));
    }
    z.every = every;
    z.on = true;
    if (!b->steer.on) {                                          // observed rows are driven through the commands: every kind 0 to begin with
        const std::vector<uint8_t> kind(std::max<size_t>(n, 1), 0);
        const std::vector<float> zero(std::max<size_t>(n, 1), 0.f);
        if ((rc = sfm_batch_set_steering(b, kind.data(), zero.data(), zero.data(), nullptr))) return rc;
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                 // the zero fills; and a frame kernel in flight may still read the old buffers
    b->replay = std::move(z);
    return SFM_OK;
}

int sfm_batch_run_observed(SfmBatch* b, int first_frame, int frames, uint32_t flags) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->replay.on) return bfail(b, SFM_ERR_STATE, OBSERVED_OFF);
    if (!(flags & SFM_TICK_INTEGRATE))
        return bfail(b, SFM_ERR_INVALID, "flags must contain SFM_TICK_INTEGRATE: a replayed row reaches its next frame by the ticks' own step");
    if ((rc = check_batch_flags(b, flags, "run"))) return rc;
    if (first_frame < 0) return bfail(b, SFM_ERR_INVALID, "first_frame < 0");
    if (frames < 0) return bfail(b, SFM_ERR_INVALID, "frames < 0");
    if ((long long)first_frame + frames > std::numeric_limits<int>::max())
        return bfail(b, SFM_ERR_INVALID, "first_frame + frames must not exceed 2^31 - 1");
    BatchReplayDev& z = b->replay;
    const size_t n = (size_t)b->n_total;
    if (first_frame == 0 && n > 0) HIP_TRY(b, hipMemsetAsync(z.score, 0, sizeof(float4) * n, b->stream));
    ReplayArgs a;
    memset(&a, 0, sizeof(a));
    a.scene_off = b->d_scene_off;
    a.score = z.score;
    a.obs = z.obs;
    a.obs_off = z.obs_off;
    a.frames = z.frames;
    a.inv_h = z.inv_h;
    a.role = z.role;
    a.span = z.span;
    a.v0 = z.v0;
    for (int f = first_frame; f < first_frame + frames; ++f) {
        if (n > 0) {                                             // (no rows: nobody to place)
            a.pk = b->pk;
            a.cmd = b->steer.cmd;
            a.f = f;
            HIP_TRY(b, launch_batch_replay(a, b->B, b->stream));
        }
        for (int t = 0; t < z.every; ++t)
            if ((rc = batch_launch(b, flags))) return rc;
    }
    return SFM_OK;
}

int sfm_batch_score(SfmBatch* b) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->replay.on) return bfail(b, SFM_ERR_STATE, OBSERVED_OFF);
    HIP_TRY(b, launch_batch_score(ScoreArgs{b->d_scene_off, b->replay.score, b->replay.scene}, b->B, b->stream));
    return SFM_OK;
}

int sfm_batch_download_scores(SfmBatch* b, float* row_scores, float* scene_scores) {
    int rc = bbind(b);
    if (rc) return rc;
    if (!b->replay.on) return bfail(b, SFM_ERR_STATE, OBSERVED_OFF);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->n_total, B = (size_t)b->B;
    if (row_scores && n > 0) HIP_TRY(b, hipMemcpy(row_scores, b->replay.score, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (scene_scores) HIP_TRY(b, hipMemcpy(scene_scores, b->replay.scene, sizeof(float) * B * SFM_BATCH_SCENE_SCORE_WIDTH, hipMemcpyDeviceToHost));
    return SFM_OK;
}

}  // extern "C"
