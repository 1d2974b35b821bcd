// sfm_capi_common.h -- what the two halves of the C ABI share: sfm_capi.hip (one crowd on a handle) and sfm_batch_capi.hip with
// sfm_batch_sense_capi.hip (batched scenes).  The kernels' launch functions, the error plumbing, and the parameter checks and
// folding both apply.
#pragma once
#include "sfm_devbuf.h"
#include "sfm_device.h"
#include "sfm_hip.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace sfm {
hipError_t launch_tick(int ipw, int team, bool z3, bool rad, const TickArgs& a, hipStream_t st);
hipError_t launch_arrived(const float4* pk, const float4* own, int N, float thr2, uint8_t* mask, hipStream_t st);
hipError_t launch_sym_list(const TickArgs& a, const SymArgs& sa, hipStream_t st, int partners = 0, bool count_is_zero = false);
hipError_t launch_sym_pair(bool rad, const TickArgs& a, const SymArgs& sa, hipStream_t st);
hipError_t launch_sym_epilogue(bool rad, const TickArgs& a, const SymArgs& sa, hipStream_t st);
hipError_t launch_fused_tick(bool rad, const TickArgs& a, const FusedArgs& f, hipStream_t st, int waves);
bool fused_lean_takes(bool rad, const TickArgs& a, const FusedArgs& f);
hipError_t launch_fused_tick_lean(const TickArgs& a, const FusedArgs& f, hipStream_t st);
int fused_pair_workgroups(int n_g);
hipError_t launch_sym_pair_geo(bool rad, const TickArgs& a, const SymArgs& sa, hipStream_t st);
int sym_item_count(int n_t);
hipError_t launch_strip_bounds(const float4* box, const float* vmax, int n_t, int tps, int n_strips, float4* sbox, float* svmax,
                               hipStream_t st);
hipError_t launch_tile_strip_bounds(const float4* pk, int N, int n_t, int tps, int n_strips, float4* box, float* vmax, float4* sbox,
                                    float* svmax, hipStream_t st);
hipError_t launch_geometry(bool rad, const TickArgs& a, hipStream_t st);
hipError_t launch_modes(const TickArgs& a, hipStream_t st);
struct ReorderBufs { unsigned long long *key64_in, *key64_out; uint32_t *row_a, *row_b, *key32_in, *key32_out; void* temp; size_t temp_bytes; };
size_t reorder_temp_bytes(int N);
hipError_t launch_resort(const float4* pk, int N, int strip_rows, const ReorderBufs& b, hipStream_t st);
hipError_t launch_resort_blocks(const float4* pk, int N, const BlockPlan& pl, const ReorderBufs& b, hipStream_t st);
hipError_t launch_unpack_geo(const char* block, float4* ctr, int K, float2* pts, int P, int* off, bool with_off, hipStream_t st);
hipError_t launch_unpack_rows(const char* block, size_t b_own, size_t b_zv, size_t b_rr, size_t b_cm, int n_pad, float4* pk0,
                              float4* pk1, float4* own, float2* zv0, float2* zv1, float* radius, uint8_t* crossing, uint32_t* draws,
                              const char* geo_block, float4* ctr, int K, float2* pts, int P, int* off, bool with_off, hipStream_t st);
hipError_t launch_gather(const uint32_t* src, int N, const float4* pk_in, float4* pk_out, const float2* zv_in, float2* zv_out,
                         const float4* own_in, float4* own_out, const float* rad_in, float* rad_out, const uint8_t* cr_in,
                         uint8_t* cr_out, const uint32_t* dr_in, uint32_t* dr_out, const uint32_t* id_in, uint32_t* id_out,
                         hipStream_t st);
hipError_t launch_tile_bounds(const float4* pk, const float2* zv, int N, float4* box, float* vmax, hipStream_t st, int t_lo = 0,
                              int t_hi = -1);
int probe_dpp_direction(hipStream_t st);
hipError_t launch_batch_tick(bool z3, bool ext, bool modes, bool spawn, bool steer, const BatchArgs& a, int B, hipStream_t st);
hipError_t launch_batch_park_unborn(const int* scene_off, const uint8_t* born, float4* pk, float2* zv, int B, hipStream_t st);
hipError_t launch_batch_place_tracks(const BatchTracks& t, const int* off, const float2* local, float4* ctr, float2* pts, int M,
                                     hipStream_t st);
hipError_t launch_batch_restart(const BatchRestart& r, int scenes, hipStream_t st);
hipError_t launch_batch_restart_noise(const RestartNoiseArgs& a, int scenes, hipStream_t st);
hipError_t launch_batch_observe(const ObserveArgs& a, int B, hipStream_t st);
hipError_t launch_batch_episode(const EpisodeArgs& a, int B, hipStream_t st);
hipError_t launch_batch_scan(const ScanArgs& a, int B, hipStream_t st);
hipError_t launch_batch_grid(const GridArgs& a, int B, hipStream_t st);
hipError_t launch_batch_replay(const ReplayArgs& a, int B, hipStream_t st);
hipError_t launch_batch_score(const ScoreArgs& a, int B, hipStream_t st);
hipError_t launch_batch_vehicle_observe(const VehicleObserveArgs& a, int B, hipStream_t st);
hipError_t launch_dynamic_boxes(float4* ctr, const int* off, const float2* local, const float2* rot, float2* pts, int M,
                                float dt, int advance, hipStream_t st);

// what sfm_last_error(NULL) and sfm_batch_last_error(NULL) answer: the last failed create call of this thread
inline thread_local std::string g_create_error;

#define HIP_TRY(h, call)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return SFM_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

inline IxConst fold(const SfmInteraction& s) {
    const double log2e = 1.4426950408889634;
    IxConst c{};
    c.lam = (float)s.lambda;
    c.eg = (float)((double)s.epsilon * (double)s.gamma);
    c.c1 = (float)(-log2e / (double)s.gamma);
    c.k1 = (float)(-((double)s.n_prime * s.gamma) * ((double)s.n_prime * s.gamma) * log2e);
    c.k2 = (float)(-((double)s.n * s.gamma) * ((double)s.n * s.gamma) * log2e);
    c.negA = (float)(-(double)s.A);
    c.thr2 = (float)((double)s.perception_threshold * (double)s.perception_threshold);
    return c;
}

inline int check_params(const SfmParams* p, const char** why) {
    if (!p) { *why = "params is NULL"; return 0; }
    // ("Parameters the library refuses": a decay length gamma or b <= 0 turns exp(-d / B) into a growth that overflows
    //  fp32 within a few metres, where the float64 reference still holds a number; nothing the kernels return there can match it)
    if (!(p->step_length > 0.f) || std::isinf(p->step_length)) { *why = "step_length must be > 0 and finite"; return 0; }
    if (!(p->tau > 0.f) || std::isinf(p->tau)) { *why = "tau must be > 0 and finite"; return 0; }
    if (!std::isfinite(p->max_speed_factor)) { *why = "max_speed_factor must be finite"; return 0; }
    if (p->enabled[SFM_FORCE_PEDESTRIAN] && !(p->pedestrian.gamma > 0.f)) { *why = "pedestrian_force.gamma must be > 0"; return 0; }
    if (p->enabled[SFM_FORCE_BORDER] && !(p->border_b > 0.f)) { *why = "border_force.b must be > 0"; return 0; }
    if (p->enabled[SFM_FORCE_STATIC_OBSTACLE] && !(p->static_obstacle.gamma > 0.f)) { *why = "static_obstacle_force.gamma must be > 0"; return 0; }
    if (p->enabled[SFM_FORCE_DYNAMIC_OBSTACLE] && !(p->dynamic_obstacle.gamma > 0.f)) { *why = "dynamic_obstacle_force.gamma must be > 0"; return 0; }
    return 1;
}

}  // namespace sfm
