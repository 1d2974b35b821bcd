// sfm_batch_replay.hip -- observed tracks of batched scenes for gfx950 (MI355X): the recording lives on the device, replayed rows are
// put on their track and scored rows are compared with theirs, with no host in the loop (sfm_batch_set_observed,
// sfm_batch_run_observed, sfm_batch_score; the rules are specified in include/sfm_hip.h).
//
// The calibration protocol of Johansson et al. 2007: a few pedestrians are simulated by the model (role 2), everybody else in the
// scene replays the recorded motion (role 1), and the simulated ones are scored by their displacement from their own tracks.
//
// sfm_batch_replay_kernel (the frame kernel): ONE launch per observed frame, between ticks, a workgroup per scene, 256 lanes striding
// the rows.  No LDS, no atomics, no state of its own: the frame f is a launch argument.  A frame's rows are contiguous float2, so the
// loads coalesce.  It writes {x, y, vx, vy} of the state, the command {ux, uy, uz, kind} and the score record of the rows of role 1
// and 2, and nothing of a row of role 0.  The lane that owns a row is its only writer, so a row's sums are taken in frame order.
//
// sfm_batch_score_kernel: ONE launch, a workgroup per scene; five sums over the scene's rows in a fixed order (lane t its rows
// t, t + 256, .. ascending from +0; an xor-shuffle tree of widths 32 .. 1 inside each wave, where both partners form the same sum
// since addition commutes; waves 0 .. 3 in ascending order by thread 0).  No float atomics, 80 bytes of LDS.
//
// Every value is one correctly rounded fp32 operation or an fmaf (sqrtf is correctly rounded in this toolchain, as sfm_batch_scan.hip
// relies on), every decision a plain comparison: replay.replay_frame and replay.score_scene are the NumPy twins, bit for bit.
#include "sfm_device.h"
#include "sfm_interaction.h"

namespace sfm {

__device__ __forceinline__ bool seen(float2 o) { return o.x == o.x; }      // (a position is NaN in both components or in none: the host checks)

__global__ __launch_bounds__(BLOCK) void sfm_batch_replay_kernel(const ReplayArgs a) {
    const int b = blockIdx.x;
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;
    if (n <= 0) return;                                                // uniform
    const int f = a.f, F = a.frames[b];
    const float inv_h = a.inv_h[b];
    const float nan = __builtin_nanf("");
    const float2* frame0 = a.obs + a.obs_off[b];                       // frame g of the scene: frame0 + g * n
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const int r = s0 + i;
        const uint8_t role = a.role[r];
        if (role == ROLE_NONE) continue;
        const float2 o = f < F ? frame0[(long long)f * n + i] : make_float2(nan, nan);
        const int2 sp = a.span[r];
        const bool in_span = sp.x <= sp.y && f >= sp.x && f <= sp.y;   // (f <= f1 < F: o was loaded)
        const bool placed = role == ROLE_REPLAYED ? seen(o) : in_span;
        if (!placed) {                                                 // parked where a despawned row is parked
            const float2 pp = park_position((uint32_t)i);
            a.pk[r] = make_float4(pp.x, pp.y, 0.f, 0.f);
            a.cmd[r] = make_float4(0.f, 0.f, 0.f, 1.0f);
            continue;
        }
        if (role == ROLE_SCORED && f != sp.x) {                        // the model moves it: compare it with its track
            a.cmd[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!seen(o)) continue;                                    // a gap inside the span is not scored
            const float4 s = a.pk[r];
            const float4 q = a.score[r];
            const float dx = s.x - o.x, dy = s.y - o.y;
            const float d2 = fmaf(dx, dx, dy * dy);
            const float d = sqrtf(d2);
            a.score[r] = make_float4(q.x + 1.0f, q.y + d, q.z + d2, d2);
            continue;
        }
        // placed on the track: a replayed row at every frame it is seen in, a scored row at its first
        const float2 u = a.v0[r];
        float2 v = make_float2(0.f, 0.f);
        bool have = false;
        if (role == ROLE_SCORED && seen(u)) { v = u; have = true; }
        if (!have && f + 1 < F) {
            const float2 o1 = frame0[(long long)(f + 1) * n + i];
            if (seen(o1)) { v = make_float2((o1.x - o.x) * inv_h, (o1.y - o.y) * inv_h); have = true; }
        }
        if (!have && role == ROLE_REPLAYED) {
            if (f >= 1) {
                const float2 om = frame0[(long long)(f - 1) * n + i];
                if (seen(om)) { v = make_float2((o.x - om.x) * inv_h, (o.y - om.y) * inv_h); have = true; }
            }
            if (!have && seen(u)) v = u;
        }
        a.pk[r] = make_float4(o.x, o.y, v.x, v.y);
        a.cmd[r] = role == ROLE_REPLAYED ? make_float4(v.x, v.y, 0.f, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_score_kernel(const ScoreArgs a) {
    __shared__ float red[WAVES_PER_BLOCK][SCENE_SCORE_WIDTH];          // 80 bytes
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;
    float v[SCENE_SCORE_WIDTH] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < n; i += BLOCK) {
        const float4 q = a.score[s0 + i];
        if (q.x > 0.f) {
            v[0] = v[0] + 1.0f;
            v[1] = v[1] + q.x;
            v[2] = v[2] + q.y;
            v[3] = v[3] + q.z;
            v[4] = v[4] + sqrtf(q.w);
        }
    }
#pragma unroll
    for (int k = 0; k < SCENE_SCORE_WIDTH; ++k) {
#pragma unroll
        for (int s = WAVE / 2; s >= 1; s >>= 1) v[k] = v[k] + __shfl_xor(v[k], s);
        if (lane == 0) red[wave][k] = v[k];
    }
    __syncthreads();                                                   // (every wave of the workgroup reaches it)
    if (tid != 0) return;
#pragma unroll
    for (int k = 0; k < SCENE_SCORE_WIDTH; ++k) {
        float s = v[k];                                                // wave 0's sum
#pragma unroll
        for (int w = 1; w < WAVES_PER_BLOCK; ++w) s = s + red[w][k];
        a.out[(size_t)b * SCENE_SCORE_WIDTH + k] = s;
    }
}

hipError_t launch_batch_replay(const ReplayArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_replay_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_score(const ScoreArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_score_kernel, dim3(B), dim3(BLOCK), 0, st, a);
    return hipGetLastError();
}

}  // namespace sfm
