/*
 * sfm_hip.h -- C ABI of libsfm_hip.so: the MI355X (gfx950) Social-Force-Model stepper.
 *
 * Drop-in boundary for ONE hot path of felixlutz/carla-social-force-model: forces.py + stateutils.py +
 * the numeric half of pedestrian_simulation.py.  The reference is pure Python and has no FFI layer of
 * its own, so each entry point below names the reference interface it replaces (file:line, relative to
 * the upstream repository); INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * SfmStatus; sfm_last_error() gives the message of the last failure on a handle (or of the last failed
 * sfm_create when called with NULL).  The caller owns every host buffer; the library owns all device
 * memory behind the opaque handle.  A handle drives ONE GPU and is not thread-safe; distinct handles are
 * independent.  Arithmetic is fp32 on the device; host arrays are fp32 SoA (one array per component).
 * All work is issued on the handle's stream (sfm_set_stream; default: the null stream); the download /
 * query calls synchronise that stream.
 */
#ifndef SFM_HIP_H
#define SFM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_ABI_VERSION 17  /* 2: + sfm_tick_begin / sfm_tick_end, sfm_set_partition, sfm_get_pair_work; 3: + sfm_set_timing; 4: + sfm_step_packed, sfm_set_dynamic_obstacles_packed; 5: + sfm_step_records; 6: + sfm_batch_*; 7: + sfm_batch_set_waypoint_streams, sfm_batch_download_waypoints, sfm_batch_run_recorded; 8: + sfm_batch_set_dynamic_boxes, sfm_batch_download_dynamic_obstacles; 9: + sfm_batch_set_mode_fsm, sfm_batch_download_modes; 10: + sfm_batch_tick_forces, sfm_batch_run_recorded_forces; 11: + sfm_batch_set_spawn_schedule, sfm_batch_download_spawns, SFM_MODE_UNBORN; 12: + sfm_batch_set_vehicle_tracks, sfm_batch_download_vehicle_tracks; 13: + sfm_batch_snapshot, sfm_batch_restart; 14: + sfm_batch_set_steering, sfm_batch_set_commands, sfm_batch_download_steering, sfm_batch_device_ptr; 15: + sfm_batch_set_observation, sfm_batch_observe, sfm_batch_download_observations, sfm_batch_observation_ptr; 16: + sfm_batch_set_episodes, sfm_batch_end_step, sfm_batch_download_episodes, sfm_batch_restart_device, SFM_BATCH_PTR_EPISODES / _DONE; 17: + sfm_batch_set_scan, sfm_batch_scan, sfm_batch_download_scan, SFM_BATCH_PTR_SCAN (additions only) */

typedef struct SfmHandle SfmHandle;

typedef enum SfmStatus {
    SFM_OK = 0,
    SFM_ERR_INVALID = -1,   /* bad argument (NULL pointer, negative size, inconsistent CSR offsets ...) */
    SFM_ERR_HIP = -2,       /* a HIP runtime call failed; message in sfm_last_error */
    SFM_ERR_STATE = -3,     /* call order: e.g. sfm_tick before sfm_upload_state */
    SFM_ERR_NO_DEVICE = -4  /* no usable gfx950 device */
} SfmStatus;

/* Index of each force: the dict order of PedestrianSimulation.init_forces (pedestrian_simulation.py:37-48),
 * which is also the summation order of tick() (:81). */
enum { SFM_FORCE_ACCELERATION = 0, SFM_FORCE_PEDESTRIAN = 1, SFM_FORCE_BORDER = 2,
       SFM_FORCE_STATIC_OBSTACLE = 3, SFM_FORCE_DYNAMIC_OBSTACLE = 4, SFM_NUM_FORCES = 5,
       SFM_FORCE_TOTAL = 5 };

/* One Moussaid parameter table: [pedestrian_force] (forces.py:66-72), [static_obstacle_force] /
 * [dynamic_obstacle_force] (forces.py:196-206). perception_threshold is unused for pedestrians. */
typedef struct SfmInteraction {
    float lambda, A, gamma, n, n_prime, epsilon, perception_threshold;
} SfmInteraction;

/* Mirrors config/sfm_config.toml as the reference *reads* it. */
typedef struct SfmParams {
    int32_t use_ped_radius;            /* forces.py:18 */
    float   max_speed_factor;          /* pedestrian_state.py:15 (1.3) */
    float   tau;                       /* forces.py:44 (0.5) */
    float   step_length;               /* run_simulation.py:168 (0.05 s) */
    int32_t enabled[SFM_NUM_FORCES];   /* [forces] switches, pedestrian_simulation.py:33-48 */
    SfmInteraction pedestrian;
    float   border_a, border_b;        /* forces.py:134-136 */
    SfmInteraction static_obstacle;
    SfmInteraction dynamic_obstacle;
} SfmParams;

/* sfm_tick / sfm_run flags */
enum {
    SFM_TICK_INTEGRATE = 1u,        /* also x <- x + dt*v' : the CARLA-free stand-in for the simulator that moves
                                       the walkers between ticks (run_simulation.py:77-87, carla_simulation.py:126-129) */
    SFM_TICK_REDRAW_WAYPOINTS = 2u, /* on arrival (pedestrian_simulation.py:92-95) draw the next waypoint from the
                                       counter-based stream set by sfm_set_waypoint_stream (run_simulation.py:118-126) */
    SFM_TICK_RECORD_FORCES = 4u     /* keep the per-force arrays for sfm_download_forces (Force.get_force, forces.py:28-32) */
};

/* ---- lifetime ------------------------------------------------------------------------------------ */

/* PedestrianSimulation.__init__ + init_forces (pedestrian_simulation.py:11-55): capture the parameters,
 * create the device context on `device_id`. */
int sfm_create(const SfmParams* params, int device_id, SfmHandle** out);
int sfm_destroy(SfmHandle* h);                                   /* PedestrianSimulation.close (:85) */
int sfm_set_params(SfmHandle* h, const SfmParams* params);       /* Force.__init__ captures (forces.py:14-18) */
int sfm_set_stream(SfmHandle* h, void* hip_stream);              /* hipStream_t; NULL = null stream */

/* ---- geometry (CSR: offsets[K+1], points SoA) ------------------------------------------------------ */

/* BorderForce.__init__ (forces.py:127-136): K polylines, centre and full section_length as cull radius
 * (forces.py:149-150; obstacles.py:129-131,352-355). K = 0 clears. */
int sfm_set_borders(SfmHandle* h, int K, const int32_t* offsets, const float* px, const float* py,
                    const float* cx, const float* cy, const float* cull_len);
/* ObstacleForce.update_obstacles for the static force (forces.py:285-288; pedestrian_simulation.py:45-46). */
int sfm_set_static_obstacles(SfmHandle* h, int M, const int32_t* offsets, const float* px, const float* py,
                             const float* cx, const float* cy);
/* update_obstacles + update_obstacle_velocities for the dynamic force, once per tick
 * (pedestrian_simulation.py:108-115; forces.py:285-291). */
int sfm_set_dynamic_obstacles(SfmHandle* h, int M, const int32_t* offsets, const float* px, const float* py,
                              const float* cx, const float* cy, const float* vx, const float* vy);
/* The same from packed arrays (ABI 4): pts [P][2] {x, y}, cv [M][4] {cx, cy, vx, vy}; replaces the same two reference calls
 * (forces.py:285-291) for a caller that is handed the vehicles every tick (run_simulation.py:95, obstacles.py:297-329).
 * The arrays are copied before the call returns.  A small report (<= 64 KiB) is only STAGED: the next sfm_upload_state /
 * sfm_step_packed spreads it over the device arrays in its own launch, and any other call that reads them (a tick without an upload,
 * sfm_download_dynamic_obstacles, ...) does so first -- no caller-visible difference, one launch less per host-in-the-loop tick. */
int sfm_set_dynamic_obstacles_packed(SfmHandle* h, int M, const int32_t* offsets, const float* pts, const float* cv);

/* Device-side form of get_dynamic_obstacles (obstacles.py:297-329) for CARLA-free runs:
 * the vehicles are given once as oriented boxes -- ring-local offsets (the ellipse of obstacles.py:269-281 before
 * the transform; CSR offsets[M+1], ux, uy), centre, cos/sin of the yaw, velocity.  Ring points
 * p = c + R(yaw) u are generated on the device, and after every tick of sfm_run the centres advance by
 * step_length * v and the rings are regenerated (what the simulator + get_dynamic_obstacles do between ticks). */
int sfm_set_dynamic_boxes(SfmHandle* h, int M, const int32_t* offsets, const float* ux, const float* uy,
                          const float* cx, const float* cy, const float* yaw_cos, const float* yaw_sin,
                          const float* vx, const float* vy);
/* Current dynamic-obstacle centres (M) and ring points (P) as the next tick will see them; NULL skips. */
int sfm_download_dynamic_obstacles(SfmHandle* h, float* cx, float* cy, float* px, float* py);

/* ---- state ----------------------------------------------------------------------------------------- */

/* The numeric columns of PedState.state (pedestrian_state.py:17-19) as fp32 SoA: loc, vel, next_waypoint,
 * target_speed (already refreshed from the modes, :94-95), radius, and the border-force mask
 * mode in {CROSSING_ROAD, ROAD_TO_SIDEWALK} (forces.py:176-177).
 * z / vz may both be NULL (planar crowd: the 2-D kernel variant is used); radius may be NULL when
 * use_ped_radius is 0; crossing_mask may be NULL (all zero).  N = 0 is allowed (tick is a no-op, :60-61). */
int sfm_upload_state(SfmHandle* h, int N,
                     const float* x, const float* y, const float* z,
                     const float* vx, const float* vy, const float* vz,
                     const float* wx, const float* wy,
                     const float* target_speed, const float* radius, const uint8_t* crossing_mask);

/* Rows [i_begin, i_end) this handle computes and integrates (pedestrian index sharding across GPUs,
 * SURVEY.md section 8e).  Default after sfm_upload_state: [0, N).  All N pedestrians stay resident as the
 * j-operand set; after each tick the caller all-gathers the packed state (below) across ranks.
 * Rows are the library's internal order: for N >= 2048 sfm_upload_state packs the pedestrians spatially (sorted by x
 * into strips, each strip sorted by y: every 64-row tile is one rectangle of the map; a pure function of the uploaded
 * state, so every rank derives the same order), which makes a row block a vertical slab of the map.  A shard whose
 * bounds are multiples of 64 can use the symmetric pair kernel.  Every download writes a row's result at the CALLER's
 * index of that pedestrian; entries of pedestrians outside the shard are left untouched. */
int sfm_set_shard(SfmHandle* h, int i_begin, int i_end);
/* Row packing for sharded runs (no reference counterpart): cut the spatial packing into gx columns by x
 * and each column into gy blocks by y, block b = column * gy + position holding rows [bounds[b], bounds[b+1]) (multiples of
 * 64; NULL = equal split), every block strip-packed on its own.  A rank that owns the rows of one block then holds a compact
 * rectangle of the map instead of a slab across it: less boundary, fewer tile pairs evaluated one-sided by two ranks.  Takes
 * effect at the next sfm_upload_state / sfm_resort; gx = gy = 0 switches it off.  Results never depend on the packing. */
int sfm_set_partition(SfmHandle* h, int gx, int gy, const int32_t* bounds);

/* Counter-based waypoint stream of the synthetic scenarios: on arrival within `arrive_threshold`
 * (run_simulation.py:39) pedestrian i draws waypoint number k from hash(seed, i, k) in [0, world_side)^2. */
int sfm_set_waypoint_stream(SfmHandle* h, uint32_t seed, float world_side, float arrive_threshold);

/* Device-side pedestrian modes + waypoint queues + gap acceptance for device-resident runs (SURVEY.md section 8f
 * rows 1 and 3): what PedModeManager (ped_mode_manager.py:12-70), PedState.apply_current_mode /
 * update_next_waypoint (pedestrian_state.py:83-95), the CHECKING_TRAFFIC branch of PedestrianSimulation.tick
 * (pedestrian_simulation.py:63-73, check_traffic.py:7-61) and the arrival loop of SimulationRunner.tick
 * (run_simulation.py:118-132) do per pedestrian on the host.  All arrays are length N in the caller's index:
 * mode (PedMode values 0..4), target_speed (the mode objects' current target_speed), initial_speed,
 * crossing_speed, safety_margin, next_mode_time; wp_offsets[N+1] + wp_x/wp_y/wp_crossing: the remaining
 * waypoints of each pedestrian (waypoint_dict) with the crossing flag of the leg; despawn_on_arrival as in
 * run_simulation.py:41,127; sim_time0 = simulation time of the next tick; first_vehicle_extent = {ex, ey} of
 * vehicle 0 (check_traffic.py:35-36 uses it for every vehicle) or NULL.  While set, every tick starts with the
 * mode pass (target speeds, IDLE timers, gap acceptance, border-force mask) and arrivals pop the queue instead of
 * the hash stream; exhausted pedestrians are despawned (parked as ghosts, mode 255).  N = 0 switches it off.
 * Call after sfm_upload_state. */
int sfm_set_mode_fsm(SfmHandle* h, int N, const uint8_t* mode, const float* target_speed, const float* initial_speed,
                     const float* crossing_speed, const float* safety_margin, const float* next_mode_time,
                     const int32_t* wp_offsets, const float* wp_x, const float* wp_y, const uint8_t* wp_crossing,
                     int despawn_on_arrival, float sim_time0, const float* first_vehicle_extent);
/* Current mode (255 = despawned), mode target speed and queue cursor of every pedestrian; NULL skips. */
int sfm_download_modes(SfmHandle* h, uint8_t* mode, float* target_speed, int32_t* cursor);

/* ---- stepping -------------------------------------------------------------------------------------- */

/* One fused tick: F = sum of the enabled forces (pedestrian_simulation.py:81), v' = cap(v + dt*F,
 * max_speed_factor*target_speed) (:117-124; stateutils.py:18-23) written in place of v. */
int sfm_tick(SfmHandle* h, uint32_t flags);
/* `ticks` ticks back to back without host intervention (device-resident loop for benchmarks and the
 * CARLA-free harness; the loop of run_simulation.py:212-221 without the simulator); flags as above,
 * SFM_TICK_INTEGRATE is implied.  A whole crowd while the tile-pair list cutoff is off (default: up to 4096
 * pedestrians; SFM_CUTOFF=0: any size) -- planar or 3-D, with or
 * without border / obstacle forces and vehicles that move on the device -- takes ONE launch per tick here
 * (sfm_fused_tick_kernel) whatever `ticks` is, so what a run computes does not depend on how
 * the caller cuts it into calls; consecutive sfm_run / sfm_tick calls with no other call on the handle in
 * between carry on without the launch in front.  Results are those of `ticks` calls of sfm_tick up to the
 * order of the fp32 sums (each tick checked against the oracle to <= 1e-5). */
int sfm_run(SfmHandle* h, int ticks, uint32_t flags);
/* One integrating tick of a SHARD in two halves, so that the exchange of the previous tick's rows (the one all-gather per tick
 * of SURVEY.md section 8e; no reference counterpart, the reference is single-process) can run beside the part that does not
 * need it.  sfm_tick_begin: what only reads this handle's own rows -- their tile boxes, the border / obstacle forces, the tile
 * pairs whose two tiles are both own.  sfm_tick_end: once every other rank's rows are current in the packed state -- the pairs
 * with the other ranks' tiles, the epilogue (pedestrian_simulation.py:81-83, :117-124).  Results are those of sfm_tick with
 * SFM_TICK_INTEGRATE (bit-identical: the same terms reach the same slab rows).  When the handle is not a tile-aligned shard
 * on the symmetric path with the tile-pair list, sfm_tick_begin does nothing and sfm_tick_end runs the whole tick. */
int sfm_tick_begin(SfmHandle* h, uint32_t flags);
int sfm_tick_end(SfmHandle* h, uint32_t flags);

/* sfm_run that also records the trajectory (replaces the per-tick full-state Python
 * copy of PedState.record_current_state, pedestrian_state.py:100-104): frame f holds {x, y, vx, vy} of every
 * pedestrian (caller's index order) BEFORE tick f*stride, like the reference records before computing forces
 * (pedestrian_simulation.py:76).  frames: [max_frames][N][4] floats; *n_frames receives ceil(ticks/stride)
 * (clamped to max_frames).  Copies are asynchronous device->pinned-host between the ticks. */
int sfm_run_recorded(SfmHandle* h, int ticks, uint32_t flags, int stride, float* frames, int max_frames, int* n_frames);

/* ---- results --------------------------------------------------------------------------------------- */

/* get_new_velocities (pedestrian_simulation.py:126-127): v' of this handle's shard rows, written at
 * [i_begin, i_end) of the caller's length-N arrays.  vz may be NULL. */
int sfm_download_velocities(SfmHandle* h, float* vx, float* vy, float* vz);
/* One host-in-the-loop tick in one call (ABI 4): PedestrianSimulation.tick's numeric part as the reference's main loop drives it
 * (run_simulation.py:87-114: update_ped_info -> tick -> get_new_velocities; pedestrian_simulation.py:57-83, pedestrian_state.py:79-95)
 * = sfm_upload_state + sfm_tick + sfm_download_velocities on one packed block.
 *   rows  [N][9]  {x, y, vx, vy, waypoint x, waypoint y, target_speed, radius, border-force-off flag (0 / 1)}
 *   zvz   [N][2]  {z, vz}, or NULL: planar crowd (all z equal, no v_z)
 *   v_out [N][3]  {vx', vy', vz'}, the caller's index order.
 * Errors as the three calls it stands for. */
int sfm_step_packed(SfmHandle* h, int N, const float* rows, const float* zvz, uint32_t flags, float* v_out);
/* The same straight from the caller's pedestrian RECORDS (ABI 5): PedestrianState's structured-array rows (pedestrian_state.py:17-23),
 * `stride` bytes apart, float64 fields at byte offsets field_offsets[5] = {loc[3], vel[3], next_waypoint[3], radius, target_speed} (they
 * need not be aligned); border_off [N] = 1 where the border force is off (modes CROSSING_ROAD / ROAD_TO_SIDEWALK, forces.py:176-177),
 * or NULL.  The crowd is taken as planar iff all z are equal and every v_z is 0 -- or, planar_tolerance >= 0, iff the spread of z and
 * every |v_z| are within it; *was_planar (may be NULL) says which bodies ran.  v_out [N][3] as above. */
int sfm_step_records(SfmHandle* h, int N, const void* records, int64_t stride, const int32_t* field_offsets, const uint8_t* border_off,
                     float planar_tolerance, uint32_t flags, float* v_out, int32_t* was_planar);

/* Whole numeric state of the shard rows (any pointer may be NULL to skip that column). */
int sfm_download_state(SfmHandle* h, float* x, float* y, float* z, float* vx, float* vy, float* vz,
                       float* wx, float* wy);
/* Force.get_force (forces.py:28-32) of force `which` (SFM_FORCE_*, or SFM_FORCE_TOTAL) for the shard rows,
 * from the last tick run with SFM_TICK_RECORD_FORCES.  fz may be NULL. */
int sfm_download_forces(SfmHandle* h, int which, float* fx, float* fy, float* fz);
/* get_arrived_peds (pedestrian_simulation.py:88-97): mask[i] = |wp_xy - x_xy| < threshold, current state. */
int sfm_get_arrived(SfmHandle* h, float threshold, uint8_t* mask);
/* Number of waypoint draws per pedestrian so far (shard rows). */
int sfm_download_draw_counts(SfmHandle* h, uint32_t* counts);

/* ---- multi-GPU plumbing ---------------------------------------------------------------------------- */

/* Device pointer to the packed j-operand state the NEXT tick will read: N_pad records of 4 floats
 * {x, y, vx, vy}.  After a tick the shard rows are fresh; the caller all-gathers the other rows into
 * this buffer in place (one RCCL all-gather per tick).  *n_pad receives the padded record count. */
void* sfm_packed_state_ptr(SfmHandle* h, int* n_pad);
/* Same for the {z, vz} records (2 floats) of the 3-D variant; NULL when the crowd is planar. */
void* sfm_packed_z_ptr(SfmHandle* h);
/* Rows are kept in an internal spatial order (compact 64-row tiles); a device-resident whole-crowd run re-packs them
 * every SFM_RESORT_EVERY ticks by itself.  A sharded run cannot: a rank only keeps its own rows' waypoints and draw
 * counters current.  Its driver therefore, every few dozen ticks, all-gathers the two per-row arrays below (row-indexed
 * like the packed state, N_pad rows; which = 0: {waypoint x, waypoint y, target speed, radius}, 16 bytes per row;
 * which = 1: waypoint draw counter, 4 bytes per row) and then calls sfm_resort on every rank: the same state gives the
 * same order everywhere, and rank r goes on with rows [lo, hi) of the new order.  No-op when the order is off (N < 2048).
 * SFM_ERR_STATE on a shard whose mode state machine lives on the device (that state is keyed by pedestrian, not gathered). */
void* sfm_row_data_ptr(SfmHandle* h, int which, int* bytes_per_row);
int sfm_resort(SfmHandle* h);

/* ---- diagnostics ----------------------------------------------------------------------------------- */

const char* sfm_last_error(const SfmHandle* h);
/* HIP-event time of the last sfm_tick / sfm_run on its stream: total ms, ticks it covered and kernel
 * launches it issued. */
int sfm_get_timing(SfmHandle* h, float* elapsed_ms, int* ticks, int* launches);
/* Switches the HIP-event bracket of sfm_tick / sfm_run off (enable = 0) or back on (default): the two event records
 * cost ~11 us per call, which shows when a call is a few hundred microseconds of work (no reference counterpart: the
 * reference times nothing).  While off, sfm_get_timing fails with SFM_ERR_STATE. */
int sfm_set_timing(SfmHandle* h, int enable);
/* Times the DOMINANT kernel of a tick on its own: `reps` back-to-back launches of the pedestrian-pair kernel the
 * current state would use (the symmetric tile-pair kernel, or the ordered fused tick kernel with flags = 0),
 * bracketed by HIP events on the handle's stream.  The state is not advanced.  For roofline accounting. */
int sfm_profile_dominant_kernel(SfmHandle* h, int reps, float* avg_us);
/* Name of the pair kernel variant the last tick used (for profiles), static storage. */
const char* sfm_kernel_variant(const SfmHandle* h);
/* Which form of sfm_fused_tick_kernel the last launch of a device-resident run was: "sfm_fused_tick_kernel<lean>" (a whole planar
 * crowd of a multiple of 1024 pedestrians, up to 4096, without radii, border / obstacle forces or vehicles; SFM_FUSED_LEAN=0 at
 * sfm_create turns it off), "sfm_fused_tick_kernel<general>", or "none" when the last run was not a fused one.  The two forms
 * give the same bits; sfm_kernel_variant does not tell them apart.  Static storage. */
const char* sfm_fused_form(const SfmHandle* h);
/* Work the symmetric pair kernel did in the last tick (measurement only; no reference counterpart -- the reference
 * always evaluates all N(N-1) ordered pairs, forces.py:74-117): tile-pair work items (whole 2-D grid, or the compacted
 * list when the provably-negligible tile pairs are cut) and the Moussaid terms evaluated for them (one per unordered
 * pair of a two-sided item).  SFM_ERR_STATE if the last tick used the ordered kernel. */
int sfm_get_pair_work(SfmHandle* h, long long* tile_pair_items, long long* pair_terms);
int sfm_abi_version(void);

/* ---- batched scenes (ABI 6) ------------------------------------------------------------------------ */

/* Many small, independent crowds stepped together (no reference counterpart: the reference steps one PedestrianSimulation per
 * process; this is B of them, pedestrian_simulation.py:57-83 per scene).  A batch holds B scenes of 0 .. SFM_BATCH_MAX_N pedestrians
 * each, every scene with its own SfmParams (a parameter sweep is one batch) and its own borders / obstacles; each tick is ONE kernel
 * launch for the whole batch (sfm_batch.hip, a workgroup per scene).  A scene's result is bitwise the same whatever else is in the
 * batch and wherever it sits.  Larger crowds belong on a handle.  Waypoint redraw (per-scene streams) and on-device trajectories
 * are ABI 7, device-side vehicles ABI 8, the mode state machine (sfm_batch_set_mode_fsm) ABI 9, force records ABI 10, spawn schedules ABI 11, vehicle tracks ABI 12, restart ABI 13, steered pedestrians ABI 14.  Not
 * supported on a batch: sharding.  Host arrays are fp32 SoA over all scenes concatenated; scene b owns rows
 * [scene_off[b], scene_off[b+1]).  Geometry is per-scene CSR: scene b owns polylines [scene_item_off[b], scene_item_off[b+1]) of the
 * concatenated set, whose points are offsets[k] .. offsets[k+1]-1 (offsets[0] = 0).  Errors as for a handle: a negative SfmStatus,
 * the message in sfm_batch_last_error(b) (or sfm_batch_last_error(NULL) after a failed sfm_batch_create); nothing is launched on
 * bad input and the batch stays usable. */
#define SFM_BATCH_MAX_N 1024
typedef struct SfmBatch SfmBatch;

/* B >= 1 scenes, params[B]; the batch starts with no state and no geometry. */
int sfm_batch_create(int B, const SfmParams* params, int device_id, SfmBatch** out);
int sfm_batch_destroy(SfmBatch* b);
int sfm_batch_set_stream(SfmBatch* b, void* hip_stream);                 /* hipStream_t; NULL = null stream */
int sfm_batch_set_params(SfmBatch* b, const SfmParams* params);          /* params[B] */
/* The state of every scene, as sfm_upload_state per scene: z / vz both NULL = a planar batch (2-D bodies); given = the 3-D bodies
 * for every scene; radius may be NULL when no scene has use_ped_radius; crossing_mask may be NULL (all zero).  scene_off[B+1]:
 * scene_off[0] = 0, non-decreasing, every scene <= SFM_BATCH_MAX_N pedestrians. */
int sfm_batch_upload_state(SfmBatch* b, const int32_t* scene_off, const float* x, const float* y, const float* z,
                           const float* vx, const float* vy, const float* vz, const float* wx, const float* wy,
                           const float* target_speed, const float* radius, const uint8_t* crossing_mask);
/* Borders of every scene (sfm_set_borders per scene); scene_item_off[B] = 0 clears them all. */
int sfm_batch_set_borders(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px, const float* py,
                          const float* cx, const float* cy, const float* cull_len);
int sfm_batch_set_static_obstacles(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px,
                                   const float* py, const float* cx, const float* cy);
/* The vehicles as the caller last set them (vx / vy NULL: at rest); the batch does not move them.  Replaces device-side vehicles
 * (sfm_batch_set_dynamic_boxes): from then on the vehicles stay where they were set. */
int sfm_batch_set_dynamic_obstacles(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* px,
                                    const float* py, const float* cx, const float* cy, const float* vx, const float* vy);
/* Device-side vehicles of every scene (ABI 8, the batch form of sfm_set_dynamic_boxes): scene b owns vehicles
 * [scene_item_off[b], scene_item_off[b+1]); ring-local offsets CSR offsets[M+1], ux, uy; centre, cos/sin yaw, velocity per vehicle
 * (vx / vy NULL: at rest).  Rings are generated at the given centres when the call returns; after every INTEGRATING tick of a scene
 * (sfm_batch_tick with SFM_TICK_INTEGRATE, sfm_batch_run, sfm_batch_run_recorded) its centres advance by that scene's
 * step_length * v and its rings are regenerated, inside the tick's one launch: c' = fma(step_length, v, c), ring point
 * p = (fma(cos, ux, fma(-sin, uy, cx)), fma(sin, ux, fma(cos, uy, cy))) in fp32, as on a handle.  The vehicles move whether or not
 * the scene's dynamic obstacle force is on; a tick without SFM_TICK_INTEGRATE leaves them where they are, and so do
 * sfm_batch_upload_state and sfm_batch_set_params (a new step_length applies from the next integrating tick).
 * scene_item_off[B] = 0 clears every vehicle.  Refused: the CSR checks of sfm_batch_set_dynamic_obstacles, NULL ux / uy with
 * ring points, NULL centre or yaw arrays with vehicles, only one of vx / vy. */
int sfm_batch_set_dynamic_boxes(SfmBatch* b, const int32_t* scene_item_off, const int32_t* offsets, const float* ux,
                                const float* uy, const float* cx, const float* cy, const float* yaw_cos, const float* yaw_sin,
                                const float* vx, const float* vy);
/* Current centres (M) and ring points (P) of every scene's vehicles, concatenated in scene order, as the next tick will see them
 * (synchronises the batch's stream); NULL skips.  Also the rings of sfm_batch_set_dynamic_obstacles. */
int sfm_batch_download_dynamic_obstacles(SfmBatch* b, float* cx, float* cy, float* px, float* py);
/* Scripted vehicle tracks (ABI 12): the reference's trajectory vehicles (vehicle_spawner.py:140-144, run_simulation.py:56-67) inside
 * each tick's one launch.  Needs device-side vehicles (sfm_batch_set_dynamic_boxes, M of them over all scenes; SFM_ERR_STATE
 * otherwise).  Vehicle k owns keyframes [trk_off[k], trk_off[k+1]) (trk_off [M+1], trk_off[0] = 0, non-decreasing); an empty list
 * leaves the vehicle free-running exactly as without tracks.  Keyframe e is {kx, ky} the centre, {kvx, kvy} the velocity the
 * dynamic obstacle force and gap acceptance see, {kcos, ksin} the yaw of the ring; first_tick[M] may be negative.  Let tau count
 * the INTEGRATING ticks of the batch since this call (0 when it returns; ticks without SFM_TICK_INTEGRATE move no vehicle and do
 * not count).  In tick tau a tracked vehicle is present iff 0 <= tau - first_tick[k] < L_k and is then AT keyframe
 * j = tau - first_tick[k]: a teleport, the step length plays no part; ring point p = (fma(cos, ux, fma(-sin, uy, x)),
 * fma(sin, ux, fma(cos, uy, y))) with the ring-local offsets of sfm_batch_set_dynamic_boxes.  Otherwise it is ABSENT: centre and
 * every ring point (+inf, +inf), velocity 0 -- which is what sfm_batch_download_dynamic_obstacles returns for it.  Its squared
 * distance to any pedestrian is +inf, so it fails the strict-< perception cull for every threshold, and with speed 0 it never makes
 * gap acceptance refuse; a scene whose vehicles are all absent lets a CHECKING pedestrian cross.  Gap acceptance keeps the
 * first_vehicle_extent of sfm_batch_set_mode_fsm.  The call places the tracked vehicles for tau = 0 with one launch; every
 * integrating tick then writes the state of tick tau + 1 into the other half of the vehicles' ping-pong from the read-only track
 * arrays: no extra launch, copy or barrier per tick.  sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop the
 * tracks; sfm_batch_upload_state, sfm_batch_set_params, sfm_batch_set_mode_fsm and sfm_batch_set_spawn_schedule keep them; setting
 * them again restarts tau at 0.  trk_off = NULL switches the tracks off: every vehicle runs free from where it is (an absent one
 * stays absent).  Refused before anything is sent or launched, the batch staying as it was: no device-side vehicles, trk_off[0] != 0
 * or decreasing, more than SFM_BATCH_MAX_TRACK_KEYS keyframes in all, a NULL first_tick or keyframe array while any track has
 * keyframes, a keyframe value that is not finite. */
#define SFM_BATCH_MAX_TRACK_KEYS (1 << 22)
int sfm_batch_set_vehicle_tracks(SfmBatch* b, const int32_t* trk_off, const int32_t* first_tick, const float* kx, const float* ky,
                                 const float* kvx, const float* kvy, const float* kcos, const float* ksin);
/* tau (*tick) and, per vehicle [M], whether the next integrating tick sees it (1; a vehicle without keyframes is always there) or
 * it is absent (0); NULL skips.  SFM_ERR_STATE while no tracks are set. */
int sfm_batch_download_vehicle_tracks(SfmBatch* b, int64_t* tick, uint8_t* present);
/* One tick of every scene: flags 0 or SFM_TICK_INTEGRATE, plus SFM_TICK_REDRAW_WAYPOINTS once sfm_batch_set_waypoint_streams has
 * been called and while no modes are set (anything else is an error); v' (and x') in place. */
int sfm_batch_tick(SfmBatch* b, uint32_t flags);
/* `ticks` integrating ticks, one launch each (SFM_TICK_INTEGRATE implied; SFM_TICK_REDRAW_WAYPOINTS as for sfm_batch_tick; other
 * flags are an error). */
int sfm_batch_run(SfmBatch* b, int ticks, uint32_t flags);
/* Per-scene waypoint streams (ABI 7), the batch form of sfm_set_waypoint_stream: seed[B], world_side[B], arrive_threshold[B] (finite,
 * >= 0).  With SFM_TICK_REDRAW_WAYPOINTS a pedestrian whose pre-move position is within its scene's threshold of its waypoint
 * (strict <) takes draw d+1 of the scene's counter-based stream, keyed by its index INSIDE the scene (a one-scene batch draws what a
 * handle draws); the new waypoint takes effect next tick.  The streams stay in effect across sfm_batch_upload_state and
 * sfm_batch_set_params; every sfm_batch_upload_state zeroes the draw counters. */
int sfm_batch_set_waypoint_streams(SfmBatch* b, const uint32_t* seed, const float* world_side, const float* arrive_threshold);
/* Current waypoints and draw counters of every scene (synchronises the batch's stream); NULL skips a column. */
int sfm_batch_download_waypoints(SfmBatch* b, float* wx, float* wy, uint32_t* draws);
/* sfm_batch_run that also records the trajectory of every scene (ABI 7): frame f holds {x, y, vx, vy} (frames, [F][N_total][4]) and,
 * for a 3-D batch, {z, vz} (zframes, [F][N_total][2], or NULL) of every row in the concatenated scene order, BEFORE tick f*stride --
 * the handle's sfm_run_recorded convention.  F = min(max_frames, ceil(ticks / stride)) is written to *n_frames; all `ticks` are run.
 * One launch per tick: the kernel stores the frames into a device buffer of the batch, copied to the host once at the end.  flags:
 * SFM_TICK_INTEGRATE implied, SFM_TICK_REDRAW_WAYPOINTS as for sfm_batch_run.  Refused before any launch: ticks < 0, stride <= 0,
 * max_frames < 0, NULL frames with F > 0, NULL n_frames, zframes on a planar batch, other flags, and more than
 * SFM_BATCH_MAX_RECORD_BYTES of frames in one call (split the run). */
#define SFM_BATCH_MAX_RECORD_BYTES (1ull << 30)
/* The pedestrian mode state machine of every row (ABI 9), the batch form of sfm_set_mode_fsm, run inside each tick's one launch.
 * Per-row arrays over the concatenated rows (N_total of the last sfm_batch_upload_state): mode (PedMode 0..4), the mode objects'
 * target_speed, initial_speed, crossing_speed, safety_margin (< 0: crosses without looking), next_mode_time; each row's remaining
 * waypoints as CSR (wp_offsets [N_total+1], wp_offsets[0] = 0, non-decreasing; wp_x, wp_y, wp_crossing [W], W = wp_offsets[N_total],
 * may be NULL when W = 0; wp_crossing 1: the leg towards that waypoint crosses a road).  Per scene [B]: despawn_on_arrival, sim_time0
 * (the scene's clock, finite), arrive_threshold (finite, >= 0), first_vehicle_extent [B][2] (NULL: zeros; every vehicle of the scene
 * is offset by it in gap acceptance, like check_traffic.py:35-36).  Cursors start at 0.  Every tick, per row, in the handle's order:
 * the mode pass (target speed of this tick = the mode object's target before its tick; IDLE wakes up once next_mode_time <= the
 * scene's clock; CHECKING crosses once gap acceptance against the scene's vehicles, as this tick sees them, says so -- at once
 * without vehicles; the border force is off in CROSSING and ROAD_TO_SIDEWALK), the forces and the step, then the arrival test on the
 * pre-move position (strict <, every tick): an arrival takes the next waypoint of the row's list with the mode request of its leg,
 * or, with the list exhausted and despawn_on_arrival, despawns the row: mode 255, target 0, parked far away keyed by its index
 * inside the scene, velocity 0.  Each scene's clock advances by its step_length per tick.  While modes are set, sfm_batch_tick,
 * sfm_batch_run and sfm_batch_run_recorded take SFM_TICK_INTEGRATE only (SFM_TICK_REDRAW_WAYPOINTS is refused: arrivals pop the
 * queues).  mode = NULL switches the modes off; so does every sfm_batch_upload_state.  Refused before anything is sent: no state
 * uploaded (SFM_ERR_STATE), a NULL required array, a mode > 4, bad wp_offsets, NULL waypoint arrays with W > 0, a threshold that is
 * not finite or < 0, a sim_time0 that is not finite. */
int sfm_batch_set_mode_fsm(SfmBatch* b, const uint8_t* mode, const float* target_speed, const float* initial_speed,
                           const float* crossing_speed, const float* safety_margin, const float* next_mode_time,
                           const int32_t* wp_offsets, const float* wp_x, const float* wp_y, const uint8_t* wp_crossing,
                           const int32_t* despawn_on_arrival, const float* sim_time0, const float* arrive_threshold,
                           const float* first_vehicle_extent);
/* Modes (255 = despawned, 254 = SFM_MODE_UNBORN: waiting for its spawn time, with target 0 and cursor 0), mode target speeds and
 * queue cursors of every row [N_total], and each scene's clock [B] (synchronises the batch's stream); NULL skips a column.
 * SFM_ERR_STATE while no modes are set. */
int sfm_batch_download_modes(SfmBatch* b, uint8_t* mode, float* target_speed, int32_t* cursor, float* sim_time);
/* Pedestrian spawners on the device (ABI 11): the other half of the reference's life cycle (PedSpawnManager.tick at the top of every
 * tick, pedestrian_spawner.py:46-59, 219-229), inside each tick's one launch.  A scene keeps its N_b rows -- everyone who will ever
 * walk in it -- and the schedule says when each enters: spawn_time [N_total] on the scene's clock (-inf: there from the start, +inf:
 * never; NaN refused) and chain [N_total] (1: the row waits for row - 1 of its scene, which must have been born in an EARLIER tick:
 * one release per spawner per tick; 0 on every scene's first row; a row that is live when the schedule is set counts as born in the
 * first tick after that, as the reference's spawn manager would release it at the top of that tick).  Birth rule, in every tick form (integrating or not), with `now`
 * the scene's clock before the tick (what sfm_batch_download_modes returns before it): an unborn row i is born iff spawn_time[i] <= now
 * (fp32) and, if chain[i], row i - 1 was born before this tick.  A newborn takes part in its birth tick: it is staged at its spawn
 * state, so every row's pedestrian force of that tick includes it, its own v' (and x') come from that tick, and its mode machine
 * runs from its initial mode.  The spawn state is what sfm_batch_upload_state gave the row (position, velocity, z / vz, radius) and
 * what sfm_batch_set_mode_fsm gave it (waypoint, mode, speeds, margin, queue).  Setting the schedule decides who is there already
 * (spawn_time <= the scene's clock now and chain = 0: live, birth time = that clock; a schedule of such rows only leaves the batch
 * bit for bit what it is without one) and moves the others out of the live state: until birth they are ghosts like despawned rows
 * (parked far away keyed by the index inside the scene, velocity 0, no force on anyone, skipped by the mode pass; waypoint, queue
 * and cursor untouched).  While a row is unborn sfm_batch_download_state gives the parked ghost, sfm_batch_download_modes mode 254 /
 * target 0 / cursor 0, recorded frames the ghost (the frame of the birth tick too: frames hold the state before their tick) and
 * force records zeros.  Needs modes (SFM_ERR_STATE otherwise); sfm_batch_upload_state and sfm_batch_set_mode_fsm (mode = NULL
 * included) drop the schedule, sfm_batch_set_params keeps it.  A second schedule on the same rows is refused (SFM_ERR_STATE): upload
 * and set the modes again first.  spawn_time = NULL switches the schedule off, refused (SFM_ERR_STATE) while a row is unborn.
 * Refused before anything is sent, the batch staying as it was: NULL chain, a NaN spawn_time, a chain value > 1, chain = 1 on a
 * scene's first row. */
#define SFM_MODE_UNBORN 254
int sfm_batch_set_spawn_schedule(SfmBatch* b, const float* spawn_time, const uint8_t* chain);
/* Who has been born [N_total] (1 / 0) and the scene clock before each row's birth tick (the clock at which the schedule was set for
 * rows live from the start; NaN while unborn); synchronises the batch's stream; NULL skips a column.  SFM_ERR_STATE while no
 * schedule is set. */
int sfm_batch_download_spawns(SfmBatch* b, uint8_t* born, float* birth_time);
int sfm_batch_run_recorded(SfmBatch* b, int ticks, uint32_t flags, int stride, float* frames, float* zframes, int max_frames,
                           int* n_frames);
/* Force records of a batch (ABI 10): Force.get_force (forces.py:28-32) of every scene, from the tick's one launch.  force_mask
 * selects the forces: bit k = SFM_FORCE_* index k, bit 5 = SFM_FORCE_TOTAL; the K = popcount(force_mask) selected forces are stored
 * in index order, each as [N_total][C] over the concatenated rows, C = 2 {fx, fy} for a planar batch, 3 {fx, fy, fz} for a 3-D one.
 * Each force is what get_force returns: acceleration, the pedestrian force (-A times the pair sum), border, static, dynamic
 * obstacle force; the total is the exact fp32 F the tick passes to the velocity update, summed in the dict order acceleration,
 * pedestrian, border, static, dynamic (the -A products fused into their additions as the tick computes them: bitwise the float
 * sum of the recorded parts whenever those products are exact, e.g. for A a power of two).  A force that is switched off in a
 * scene records zeros; border, static and dynamic forces record z = 0; a planar batch has no z column for any force.  With
 * modes set the forces are those of the tick's mode pass (its target speed; no border force in CROSSING and ROAD_TO_SIDEWALK),
 * and a row despawned before the tick records zeros for every force.  SFM_TICK_RECORD_FORCES stays refused by sfm_batch_tick,
 * sfm_batch_run and sfm_batch_run_recorded.  Refused before any launch, the batch staying usable: force_mask 0 or a bit above 5,
 * NULL forces while K * F > 0, and every refusal of the call it extends. */
/* One tick exactly as sfm_batch_tick(b, flags) (the same flags), which also writes that tick's forces into forces
 * [K][N_total][C]; synchronises the batch's stream.  flags = 0: the forces of every scene with nothing moved. */
int sfm_batch_tick_forces(SfmBatch* b, uint32_t flags, uint32_t force_mask, float* forces);
/* sfm_batch_run_recorded (the same frames, F and refusals) that also stores, for every recorded tick f*stride, the forces that tick
 * computed from the state in frame f: forces [F][K][N_total][C], copied to the host once after the last tick.
 * SFM_BATCH_MAX_RECORD_BYTES applies to the frames and the forces together. */
int sfm_batch_run_recorded_forces(SfmBatch* b, int ticks, uint32_t flags, int stride, uint32_t force_mask, float* frames,
                                  float* zframes, float* forces, int max_frames, int* n_frames);
/* Restart from a device snapshot (ABI 13): episodes that end and start over -- RL environments, scenario sampling, calibration
 * sweeps -- without the host in the loop.  sfm_batch_snapshot records, on the batch's stream, every piece of state a tick can
 * change, for all scenes: positions and velocities (z / vz of a 3-D batch), waypoints and target speeds, the draw counters; with
 * device-side vehicles the centres, velocities and rings the next tick reads; with modes each row's mode, mode target speed and
 * queue cursor and each scene's clock; with a spawn schedule who is born and when; with tracks every vehicle's first tick and tau.
 * The copies are device to device into grow-only buffers of the batch; the host does not wait for them.  A second snapshot
 * replaces the first.  SFM_ERR_STATE before sfm_batch_upload_state. */
int sfm_batch_snapshot(SfmBatch* b);
/* Puts the chosen scenes back to the snapshot: mask [B] on the host, 1 = restart the scene, 0 = leave it alone (bit for bit);
 * NULL = every scene.  ONE launch (sfm_batch_restart_kernel, a workgroup per chosen scene) ordered on the batch's stream with the
 * ticks around it; the only copy is the list of chosen scenes (none with mask = NULL), and an all-zero mask launches nothing.
 * A restarted scene then computes what it computed after the snapshot, whatever the other scenes do -- under the parameters, waypoint
 * streams, borders and static obstacles of the moment, which may be set anew in between (the sweep: snapshot once, then per
 * candidate sfm_batch_set_params, sfm_batch_restart(b, NULL), sfm_batch_run).  Track time is per scene: tau stays the batch's one
 * counter (sfm_batch_download_vehicle_tracks goes on returning it), and a restart at tau_r of a snapshot taken at tau_s sets
 * first_tick[k] = first_tick_snapshot[k] + (tau_r - tau_s) for the tracked vehicles of the chosen scenes, so that their keyframe
 * index tau - first_tick[k], and with it their presence, is what it was at the snapshot.  sfm_batch_set_params,
 * sfm_batch_set_waypoint_streams, sfm_batch_set_borders and sfm_batch_set_static_obstacles keep the snapshot;
 * sfm_batch_upload_state, sfm_batch_set_dynamic_obstacles, sfm_batch_set_dynamic_boxes, sfm_batch_set_mode_fsm,
 * sfm_batch_set_spawn_schedule and sfm_batch_set_vehicle_tracks drop it, each also in its "off" form (they change which arrays
 * exist, or their sizes); a call that is refused drops nothing.  Refused with nothing sent or launched, the batch staying usable:
 * no snapshot (SFM_ERR_STATE), a mask value above 1, a moved first tick that does not fit int32 (SFM_ERR_INVALID: set the tracks
 * again, which restarts tau). */
int sfm_batch_restart(SfmBatch* b, const uint8_t* mask);
/* Pedestrians steered from outside (ABI 14): the reference's update_ped_info (run_simulation.py:79-87), where the simulator -- a
 * policy, a recording -- decides a walker's motion, inside each tick's one launch.  Every row has a command {ux, uy, uz, kind} in a
 * device buffer [N_total][4] of floats that the ticks read and never write; kind is held as a float: 0 not steered, 1 velocity
 * command, 2 preferred velocity, any other value counts as 0.  The lane that owns a row reads its command in the epilogue.
 * Kind 1: the row's new velocity IS the command, bit for bit, v' = (ux, uy[, uz]) -- no cap, no force applied -- and with
 * SFM_TICK_INTEGRATE it moves as every row does, x' = fma(step_length, v', x).  Its forces are computed and recorded as ever (what
 * Force.get_force returns for it); only the velocity update ignores them.  Kind 2: the row's acceleration term is (u - v) / tau
 * in every component instead of (v0 e_wp - v) / tau, summed only where the scene's acceleration force is on; everything else is
 * unchanged, the cap at max_speed_factor times this tick's target speed included; a force record holds the replaced term in
 * the acceleration slot and the F that was used in the total.  To everyone else a steered row is an ordinary pedestrian at its
 * staged position and velocity.  A planar batch ignores uz (it computes for uz = 0).  Nothing else about a steered row changes:
 * arrival tests on the pre-move position, waypoint redraws, the mode machine, gap acceptance, queue pops, despawn and birth go
 * on.  A despawned or unborn row ignores its command, parking overrides it (velocity 0; a kind 1 row that despawns
 * in a tick is parked exactly as if it were not steered, its z of a 3-D batch included), and a row born in a tick is steered in
 * that tick.  sfm_batch_run, sfm_batch_run_recorded and sfm_batch_run_recorded_forces hold the commands for all their ticks
 * (action repeat); a tick without SFM_TICK_INTEGRATE writes v' only.  Steering is an input like the parameters:
 * sfm_batch_set_params, sfm_batch_set_waypoint_streams, the geometry calls, sfm_batch_set_mode_fsm, sfm_batch_set_spawn_schedule,
 * sfm_batch_set_vehicle_tracks, sfm_batch_snapshot and sfm_batch_restart keep it (a snapshot does not contain commands, and the
 * steering calls keep the snapshot); sfm_batch_upload_state drops it, because the rows may differ.  A batch without steering
 * launches exactly the kernels it launched before.
 * sfm_batch_set_steering: kind [N_total] (0, 1, 2), ux, uy, uz [N_total] (uz NULL: zeros); kind = NULL switches steering off.
 * It (re)allocates the command buffer and waits for the batch's stream.  Refused with nothing sent or freed: no state uploaded
 * (SFM_ERR_STATE), a kind above 2, NULL ux / uy, a command that is not finite on a row with kind != 0. */
int sfm_batch_set_steering(SfmBatch* b, const uint8_t* kind, const float* ux, const float* uy, const float* uz);
/* New velocities for every row, the kinds staying those of the last sfm_batch_set_steering: ONE copy of the whole buffer from
 * pinned memory, ordered on the batch's stream (the host waits only for the copy before, if it is still in flight).  Since it
 * sends the kinds it knows, it overwrites kinds the caller changed on the device.  Refused: steering off (SFM_ERR_STATE), NULL
 * ux / uy, a value that is not finite on a steered row. */
int sfm_batch_set_commands(SfmBatch* b, const float* ux, const float* uy, const float* uz);
/* The commands as the next tick will read them (synchronises the batch's stream): kind as the tick understands it (0, 1, 2);
 * NULL skips a column.  SFM_ERR_STATE while steering is off. */
int sfm_batch_download_steering(SfmBatch* b, uint8_t* kind, float* ux, float* uy, float* uz);
/* Device pointers of a batch, the counterpart of sfm_row_data_ptr for a handle: which = SFM_BATCH_PTR_COMMANDS, the command buffer
 * ([N_total][4] float {ux, uy, uz, kind}; the caller may write it, on the batch's stream or ordered with it -- a policy's output
 * needs no host copy); SFM_BATCH_PTR_STATE, the state ([N_total][4] float {x, y, vx, vy}, as the last tick left it);
 * SFM_BATCH_PTR_ZSTATE, {z, vz} ([N_total][2] float; NULL for a planar batch).  *bytes (may be NULL) receives the size.  The pointers
 * stay valid until the next call that reallocates: sfm_batch_upload_state (all three) and sfm_batch_set_steering (the command
 * buffer).  What the caller writes into the command buffer on the device is NOT validated: a kind other than 1 or 2 counts as
 * 0, and a non-finite command of a steered row goes into the state as it is.  NULL (and the message in sfm_batch_last_error) for an
 * unknown `which`, before sfm_batch_upload_state, and for the command buffer while steering is off; NULL without rows.
 * ABI 16: SFM_BATCH_PTR_EPISODES, the episode record ([B][SFM_BATCH_EPISODE_WIDTH] float), and SFM_BATCH_PTR_DONE, the mask ([B]
 * uint8_t, 0 / 1), as the last sfm_batch_end_step left them; valid until the next sfm_batch_set_episodes or sfm_batch_upload_state;
 * NULL (and the message) while episodes are off.
 * ABI 17: SFM_BATCH_PTR_SCAN, the scan record ([N_total][2 R] float), as the last sfm_batch_scan left it; valid until the next
 * sfm_batch_set_scan or sfm_batch_upload_state; NULL (and the message) while scans are off; NULL without rows. */
#define SFM_BATCH_PTR_COMMANDS 0
#define SFM_BATCH_PTR_STATE 1
#define SFM_BATCH_PTR_ZSTATE 2
#define SFM_BATCH_PTR_EPISODES 3
#define SFM_BATCH_PTR_DONE 4
#define SFM_BATCH_PTR_SCAN 5
void* sfm_batch_device_ptr(SfmBatch* b, int which, int64_t* bytes);
/* Per-pedestrian observations computed on the device (ABI 15): what a policy or a reward reads per agent -- who is near it and how
 * they move relative to it, where the kerb, the nearest obstacle and the nearest vehicle are, where its goal is -- by ONE launch of
 * sfm_batch_observe_kernel (a workgroup per scene) straight from the buffers the tick reads, into a device buffer the caller reads
 * with no copy.  With sfm_batch_snapshot / sfm_batch_restart (the reset) and sfm_batch_set_steering (the action) it closes a
 * reinforcement-learning loop with no host in it.
 *
 * Settings.  k: neighbour slots per row, 1 .. SFM_BATCH_MAX_OBS_NEIGHBOURS, one value for the batch.  sense_range[b]: metres, per
 * scene, finite, 0 < R <= SFM_BATCH_MAX_SENSE_RANGE; the kernel uses R2 = float32(R * R), formed in double and rounded once, like
 * thr2.  frame: SFM_OBS_FRAME_WORLD (0, world axes) or SFM_OBS_FRAME_HEADING (1, the row's heading frame), one value for the batch.
 *
 * Inputs.  Only {x, y, vx, vy} of the state is used, for planar and 3-D batches alike; z and vz play no part, so a 3-D batch gives,
 * bit for bit, the record of the planar batch with the same x, y, vx, vy.
 *
 * Record.  Row i owns W = SFM_BATCH_OBS_HEADER + 4 k floats, row-major [N_total][W], in concatenated scene order:
 *     0-1      goal (wx - x, wy - y)
 *     2-3      own velocity (vx, vy)
 *     4        target speed (the value the next tick would read from `own`)
 *     5        live: 1.0 or 0.0
 *     6        m = number of filled neighbour slots, 0 .. k, as a float
 *     7        geometry flags as a float: 1 (border point present) + 2 (static point present) + 4 (vehicle point present)
 *     8-11     nearest vehicle ring point (px - x, py - y, ovx - vx, ovy - vy)
 *     12-13    nearest border point (px - x, py - y)
 *     14-15    nearest static-obstacle point (px - x, py - y)
 *     16+4s .. neighbour slot s: (x_j - x_i, y_j - y_i, vx_j - vx_i, vy_j - vy_i)
 *
 * Rules, all exact.
 * Live rows: row i is live iff |x_i| < NEAR_LIMIT and |y_i| < NEAR_LIMIT (1e12, sfm_device.h).  Despawned and unborn rows are parked
 * beyond that limit, so they are not live; a NaN position fails the test, so such a row is not live.  A row that is not live has an
 * all-zero record.
 * Neighbours: a candidate of row i is a row j != i of the same scene with d2 = fmaf(dx, dx, dy * dy) < R2 (dx = x_j - x_i; strict
 * `<`).  Ghosts sit at least FAR_STEP apart, far from anyone, so the range bound excludes them without a test of their own.  The
 * slots hold the first k candidates in ascending (d2, j) order -- among equal d2 the lower index inside the scene comes first --
 * and slots m .. k-1 are zeros.  A coincident pair (d2 == 0) is a candidate like any other.
 * Nearest points, per kind (border, static, vehicle): the nearest point over ALL points of ALL the scene's polylines of that kind,
 * with the tick's own distance d2 = fmaf(ax, ax, ay * ay), ax = x - px; the first minimum wins (polylines in order, points in
 * order: np.argmin's rule).  A point is present iff its d2 < R2; a point that is absent is zeros.  There is no cull by
 * section_length or by perception threshold, and no force switch and no crossing mask is consulted: this is what the row can see,
 * not what pushes it.
 * Vehicles are read as the next tick would read them (the current half of the ping-pong for device-side vehicles and tracks); a
 * tracked vehicle that is absent has its ring at +inf, so d2 = +inf and it fails the test.  A vehicle's velocity is that of its
 * item.
 * Frame 0: every value is a single fp32 subtraction or a copy, so the whole record is defined bit for bit.
 * Frame 1: the selection, order, m and flags are those of frame 0 -- they are decided before any rotation.  The heading is
 * h = v / |v| when fmaf(vx, vx, vy * vy) > 0; otherwise g / |g| of the goal entry g = (wx - x, wy - y) when fmaf(gx, gx, gy * gy) > 0;
 * otherwise (1, 0).  Every 2-vector (a, b) of the record -- the goal, the own velocity, both halves of the vehicle entry, the border
 * and static entries, both halves of every slot -- is replaced by (h_x a + h_y b, -h_y a + h_x b).
 * The kernel writes nothing but the observation buffer; it reads the state, `own`, the scene offsets, the three geometry CSRs and
 * the per-scene ranges.  No atomics, every order a function of the scene alone: a scene's record is bitwise the same alone or
 * anywhere in any batch.
 *
 * sfm_batch_set_observation: sense_range [B]; sense_range = NULL switches observations off and frees the buffer.  Otherwise it
 * allocates and zero-fills [N_total][SFM_BATCH_OBS_HEADER + 4 k] and waits for the batch's stream.  Refused with nothing changed:
 * before sfm_batch_upload_state (SFM_ERR_STATE), k outside 1 .. 16, frame outside {0, 1}, a sense_range that is NaN, infinite,
 * <= 0 or > 1e6.  sfm_batch_upload_state drops the observations because the rows may differ, as it drops steering; every other call
 * keeps them, and they keep the snapshot.  A snapshot neither holds nor restores observations. */
#define SFM_BATCH_OBS_HEADER 16
#define SFM_BATCH_MAX_OBS_NEIGHBOURS 16
#define SFM_BATCH_MAX_SENSE_RANGE 1.0e6f
#define SFM_OBS_FRAME_WORLD 0
#define SFM_OBS_FRAME_HEADING 1
int sfm_batch_set_observation(SfmBatch* b, int k, const float* sense_range, int frame);
/* ONE launch on the batch's stream, ordered with the ticks and restarts around it; the host does not wait.  SFM_ERR_STATE while
 * observations are off.  With no rows it launches nothing and succeeds. */
int sfm_batch_observe(SfmBatch* b);
/* Synchronises the batch's stream, then copies the buffer ([N_total][SFM_BATCH_OBS_HEADER + 4 k] floats) as the last
 * sfm_batch_observe left it; before the first observe that is zeros.  SFM_ERR_STATE while observations are off. */
int sfm_batch_download_observations(SfmBatch* b, float* out);
/* The observation buffer on the device; *bytes (may be NULL) receives N_total * (SFM_BATCH_OBS_HEADER + 4 k) * 4.  Valid until the
 * next sfm_batch_upload_state or sfm_batch_set_observation.  NULL (and the message in sfm_batch_last_error) while observations are
 * off; NULL without rows. */
void* sfm_batch_observation_ptr(SfmBatch* b, int64_t* bytes);
/* Episode ends on the device (ABI 16): the last piece of the loop observe -> act -> step -> reset.  Per scene one AGENT row, three
 * radii and a time limit; sfm_batch_end_step decides, by ONE launch of sfm_batch_episode_kernel (a workgroup per scene), whose
 * episode is over and why, leaves what a reward is made of in a record, and -- with SFM_END_STEP_AUTO_RESTART -- restarts the
 * scenes that are done from the snapshot with a second launch, the mask never leaving the device.
 *
 * Settings (sfm_batch_set_episodes; every array [B] on the host).  agent[b]: the row inside scene b whose fate ends the episode,
 * 0 .. N_b-1; -1: the scene has no agent, only the time limit can end it.  goal_radius, ped_radius, veh_radius: metres, finite,
 * 0 <= r <= SFM_BATCH_MAX_SENSE_RANGE, 0 switches the test off; the kernel compares against r2 = float32(double(r) * r), formed in
 * double and rounded once, like R2 and thr2.  max_steps[b] >= 0, 0: no time limit.
 *
 * State.  Per scene age (int32, evaluations since the scene's last restart, 0 at the start) and prev_goal_d2 (float; NaN: none
 * yet).  A snapshot neither holds nor restores them; instead EVERY restart of a scene, by host mask (sfm_batch_restart) or by
 * device mask (sfm_batch_restart_device, the auto restart), sets that scene's age = 0 and prev_goal_d2 = NaN.
 *
 * Record.  Scene b owns SFM_BATCH_EPISODE_WIDTH = 8 floats, [B][8], with a its agent row:
 *     0  done, 0.0 or 1.0
 *     1  reason bits as a float: SFM_EPISODE_ARRIVED 1, _TIME_LIMIT 2, _PED_HIT 4, _VEH_HIT 8, _NOT_LIVE 16
 *     2  age after this evaluation (age_old + 1), as a float
 *     3  goal_d2 = fmaf(gx, gx, gy * gy), g the goal entry exactly as sfm_batch_observe forms it (wx - x, wy - y)
 *     4  prev_goal_d2: the stored value, or goal_d2 itself while the stored value is NaN (the first live evaluation since the
 *        restart); the scene's stored value then becomes goal_d2
 *     5  ped_d2: min over the live rows j != a of the scene of fmaf(dx, dx, dy * dy), dx = x_j - x_a; +inf when there is none
 *     6  veh_d2: min over ALL ring points of ALL the scene's vehicles of the tick's own distance fmaf(ax, ax, ay * ay), ax = x - px;
 *        the points are read as the next tick would read them (the current half of the ping-pong); an absent tracked vehicle has
 *        its ring at +inf and contributes +inf; +inf when the scene has no vehicle
 *     7  wall_d2: the same minimum over all border and static-obstacle points of the scene; +inf when there are none
 * and done[b] (uint8_t) = slot 0.
 *
 * Rules, all exact.  A row is live by sfm_batch_observe's test: |x| < NEAR_LIMIT and |y| < NEAR_LIMIT (a NaN position fails it).
 * arrived iff goal_d2 < goal_r2; pedestrian hit iff ped_d2 < ped_r2; vehicle hit iff veh_d2 < veh_r2 -- all strict, so a radius of 0
 * never fires.  time limit iff max_steps > 0 and age_old + 1 >= max_steps.  An agent that is not live (despawned, unborn, NaN
 * position) gives reason 16, +inf in slots 3 .. 7, and leaves the stored prev_goal_d2 alone.  agent = -1 gives +inf in slots 3 .. 7
 * and only the time-limit bit.  done = (reason != 0).  wall_d2 ends nothing: it is an ingredient for a reward, as is the progress
 * sqrt(slot 4) - sqrt(slot 3); no reward is computed here.  Only x, y of the state are used, as in sfm_batch_observe: a 3-D batch
 * gives the planar batch's record bit for bit.
 * The kernel writes only the record, the mask and the episode state; a tick before or after it computes what it computed without
 * it.  No atomics; a minimum of floats without NaNs does not depend on the order it is taken in (the live test keeps NaN rows out,
 * ring points are finite or +inf): a scene's record is bitwise the same alone or anywhere in any batch.
 *
 * sfm_batch_set_episodes allocates the settings, the state (age zero-filled, prev_goal_d2 NaN-filled), the record and the mask
 * (zero-filled) and waits for the batch's stream; agent = NULL switches episodes off and frees them.  Refused with nothing changed:
 * before sfm_batch_upload_state (SFM_ERR_STATE), an agent outside -1 .. N_b-1, a radius that is NaN, negative, infinite or above
 * 1e6, a negative max_steps, a NULL array beside a non-NULL agent.  sfm_batch_upload_state drops the episodes (the agents are
 * rows), as it drops observations; every other call keeps them, and they keep the snapshot. */
#define SFM_BATCH_EPISODE_WIDTH 8
#define SFM_EPISODE_ARRIVED 1
#define SFM_EPISODE_TIME_LIMIT 2
#define SFM_EPISODE_PED_HIT 4
#define SFM_EPISODE_VEH_HIT 8
#define SFM_EPISODE_NOT_LIVE 16
#define SFM_END_STEP_AUTO_RESTART 1u
int sfm_batch_set_episodes(SfmBatch* b, const int32_t* agent, const float* goal_radius, const float* ped_radius,
                           const float* veh_radius, const int32_t* max_steps);
/* ONE launch on the batch's stream, ordered with the ticks, observations and restarts around it; the host does not wait.  flags:
 * 0, or SFM_END_STEP_AUTO_RESTART: the launch is followed by sfm_batch_restart_device with the mask it wrote -- two launches, no
 * copy; the record keeps the terminal values, and the restarted scenes' age is 0 afterwards.  SFM_ERR_STATE while episodes are
 * off; with the flag every refusal of sfm_batch_restart_device applies to the whole call, and nothing is launched. */
int sfm_batch_end_step(SfmBatch* b, uint32_t flags);
/* Synchronises the batch's stream, then copies the record ([B][8] floats) and the mask ([B] bytes) as the last
 * sfm_batch_end_step left them (zeros before the first); NULL skips a column.  SFM_ERR_STATE while episodes are off. */
int sfm_batch_download_episodes(SfmBatch* b, float* record, uint8_t* done);
/* sfm_batch_restart with its mask on the DEVICE: d_mask is [B] bytes of device memory -- the batch's own mask
 * (SFM_BATCH_PTR_DONE) or any buffer of the caller's, such as a torch bool tensor -- nonzero = restart the scene.  The values are
 * not validated, like the command buffer's.  ONE launch of B workgroups on the batch's stream: workgroup b returns at once while
 * d_mask[b] == 0 and otherwise does what sfm_batch_restart does for scene b.  No copy, no host scan, no wait.  Tracks: the first
 * tick moved by the ticks since the snapshot must fit int32 for the tracked vehicles of ALL scenes (the host cannot know who is
 * chosen; SFM_ERR_INVALID otherwise), and the host's copy of the first ticks is refreshed from the device by the next
 * sfm_batch_download_vehicle_tracks or sfm_batch_snapshot, which synchronise.  Refused with nothing launched: no snapshot
 * (SFM_ERR_STATE), d_mask NULL (SFM_ERR_INVALID). */
int sfm_batch_restart_device(SfmBatch* b, const uint8_t* d_mask);
/* Restart noise: randomised restarts, sampled on the device.  Without it a restarted scene is the snapshot bit for bit, so every
 * episode of a scene starts alike.  With it, every restart of a scene -- sfm_batch_restart, sfm_batch_restart_device, the auto
 * restart of sfm_batch_end_step -- is followed, on the batch's stream, by ONE more launch (sfm_batch_restart_noise_kernel, a
 * workgroup per scene with the same choice of scenes) that draws the starts from a box around each row's snapshot position,
 * re-draws them until nobody is too near anybody or anything, draws the goals from a box around the snapshot goal and lets
 * scripted traffic arrive later.  Every draw is keyed by a counter, so a restart is reproducible.  A batch that never sets restart
 * noise launches exactly what it launched before.
 * These two entry points and SFM_BATCH_PTR_RESETS were added WITHOUT a bump of SFM_ABI_VERSION (it stays 17): they are additions
 * only, nothing that existed changes its meaning, and a build that has them is recognised by the symbols themselves.
 *
 * Settings.  seeds [B] uint32.  pos_hx, pos_hy [N_total]: the half-extents (metres) of the box a row's start is drawn from, finite,
 * 0 <= h <= SFM_BATCH_MAX_SENSE_RANGE; goal_hx, goal_hy [N_total] likewise for the goal, both NULL: the goals stay.  min_gap,
 * point_gap [B]: metres, finite, 0 <= g <= SFM_BATCH_MAX_SENSE_RANGE; the kernel compares against g2 = float32(double(g) * g),
 * formed in double and rounded once like R2.  tries: 1 .. SFM_BATCH_MAX_RESTART_TRIES, one value for the batch.  track_delay [M]
 * int32 >= 0 per device-side vehicle, or NULL: none.
 *
 * The rule, all exact: every value is one correctly rounded fp32 operation or an fmaf, every decision a strict `<`.  For a scene b
 * that restarts, first sfm_batch_restart_kernel's copies run unchanged.  Then, with e = resets[b] read before this restart:
 * 1. Random numbers.  The word of component c of try t for item i (a row's index inside its scene, or a vehicle's) is
 *        h = mix32(seed_b ^ mix32(mix32(0x5BD1E995 ^ (8 i + c)) + 0x9E3779B9 (32 e + t)))      (mod 2^32; mix32: lowbias32,
 *    sfm_device.h, where this formula is reset_word), u = (h >> 8) * 2^-24 in [0, 1), and an offset inside a half-extent ext is
 *    o = fmaf(2 u, ext, -ext), in [-ext, ext); 2 u is exact.  The constant and the inner mix32 keep the words apart from the
 *    waypoint stream's under an equal seed.
 * 2. Row classes, from the restored state.  Not live (sfm_batch_observe's test fails: unborn, despawned, NaN): untouched, and never
 *    in anyone's way.  Fixed (live, hx == 0 and hy == 0): stays where it is and is a blocker from the start.  Movable: the rest.
 * 3. Placement rounds t = 0 .. tries-1.  Every movable row not yet placed proposes p = (x_s + o_x, y_s + o_y) around its snapshot
 *    position (components 0 and 1; each coordinate one fp32 add).  With d2 = fmaf(dx, dx, dy * dy) the proposal is rejected iff
 *    d2 < min_gap2 to a blocker (a fixed row, or a row placed in an earlier round); or d2 < min_gap2 to the proposal of a
 *    lower-index row of the SAME round, accepted or not; or d2 < point_gap2 to a point of the scene's borders, static obstacles
 *    or vehicle rings as they stand after step 5.  A gap of 0 never rejects.  Accepted rows are placed and become blockers for the
 *    next round.  (The lower-index rule is conservative on purpose: the outcome is a function of the proposals alone, whatever the
 *    order of evaluation.)
 * 4. Fallbacks.  A movable row still not placed after the last round stays at its snapshot position, unchecked; their number at the
 *    scene's latest restart is fallbacks[b].  Velocities, z, modes and everything else stay as restored.
 * 5. Traffic timing, BEFORE the rounds.  A tracked vehicle k (item i = its index inside the scene) with track_delay[k] = D > 0 gets
 *    first_tick[k] += (uint64(h) * (D + 1)) >> 32 with the word of c = 4, t = 0 -- 0 .. D ticks -- and is placed again as tau sees
 *    it, the computation of sfm_batch_set_vehicle_tracks: centre, velocity and ring of its keyframe, absent -> +inf.
 *    A restart's int32 fit check adds the largest delay, and the host's copy of the first ticks is refreshed from the device as
 *    after sfm_batch_restart_device.
 * 6. Goals.  With goal boxes, every live row's {wx, wy} gets + fmaf(2 u, g_ext, -g_ext) (components 2 and 3, t = 0); no rejection.
 * 7. resets[b] = e + 1.
 * A scene's result depends on its own seed, its own rows and e only: it is bitwise the same alone or anywhere in any batch.  Scenes
 * that are not chosen are not touched, counters included.
 *
 * sfm_batch_set_restart_noise allocates the settings and zero-fills resets and fallbacks, and waits for the batch's stream; seeds =
 * NULL switches the noise off and frees them.  It builds the new buffers before it drops the old ones.  Refused with nothing
 * changed (the noise set before stays in force): before sfm_batch_upload_state (SFM_ERR_STATE); tries outside 1 .. 32; a
 * half-extent or gap that is NaN, negative, infinite or > 1e6; NULL pos_hx / pos_hy with rows, only one of goal_hx / goal_hy, NULL
 * min_gap / point_gap; a negative track_delay; track_delay without vehicle tracks (SFM_ERR_STATE).  Restart noise is an input like
 * steering: sfm_batch_upload_state drops it, because the rows may differ; every other call keeps it, and it keeps the snapshot --
 * except that the delays go with the tracks they refer to (sfm_batch_set_vehicle_tracks, sfm_batch_set_dynamic_boxes and
 * sfm_batch_set_dynamic_obstacles drop the delays and keep the rest).
 * sfm_batch_download_restart_noise synchronises the batch's stream and copies resets and fallbacks ([B] uint32 each; NULL skips a
 * column); SFM_ERR_STATE while the noise is off.  SFM_BATCH_PTR_RESETS (sfm_batch_device_ptr): resets on the device, [B] uint32,
 * valid until the next sfm_batch_set_restart_noise or sfm_batch_upload_state; while the noise is off the value is refused as the
 * unknown `which` it was before. */
#define SFM_BATCH_PTR_RESETS 6
#define SFM_BATCH_MAX_RESTART_TRIES 32
int sfm_batch_set_restart_noise(SfmBatch* b, const uint32_t* seeds, const float* pos_hx, const float* pos_hy, const float* goal_hx,
                                const float* goal_hy, const float* min_gap, const float* point_gap, int tries,
                                const int32_t* track_delay);
int sfm_batch_download_restart_noise(SfmBatch* b, uint32_t* resets, uint32_t* fallbacks);
/* Range scans on the device (ABI 17): the sensor most crowd-navigation policies are trained on.  R rays around a row, each giving
 * the distance to the first thing it meets and what that was, by ONE launch of sfm_batch_scan_kernel (a workgroup per scene)
 * straight from the buffers the tick reads, into a device buffer the caller reads with no copy.  The record is defined bit for bit
 * in BOTH frames: every operation below is a single correctly rounded fp32 operation or an fmaf, and the kernel does no
 * trigonometry.
 *
 * Settings (sfm_batch_set_scan).  R: rays per row, 1 .. SFM_BATCH_MAX_SCAN_RAYS, one value for the batch.  dir_x, dir_y [R]: the
 * ray directions, fp32, finite; the kernel uses them as given and does not renormalise them (a caller forms cos and sin in double
 * and rounds once).  With unit directions the range is the distance along the ray to the first disc, to the rounding of the
 * rules below; with directions that are not unit vectors the record is defined by those rules alone and carries no geometric
 * meaning.  max_range[b]: per scene, finite, 0 < Rmax <= SFM_BATCH_MAX_SENSE_RANGE, used as the fp32 value.
 * ped_radius[b], point_radius[b]: per scene, finite, 0 <= r <= SFM_BATCH_MAX_SENSE_RANGE; the kernel uses r2 = float32(r * r),
 * formed in double and rounded once, like R2.  Every pedestrian is a disc of ped_radius; every sampled point of a border, of a
 * static-obstacle ring or of a vehicle ring is a disc of point_radius -- the model's own view of geometry: the forces see sampled
 * points, not segments (the reference samples them 0.1 m apart).  A radius of 0 switches that kind off.  The radius in `own` is
 * not used.  mask [N_total] uint8_t, or NULL for every row: which rows are scanned (nonzero); a masked-out row costs nothing and
 * has an all-zero record -- an RL loop scans its agents, not the crowd.  frame: SFM_OBS_FRAME_WORLD (0) or SFM_OBS_FRAME_HEADING
 * (1), one value for the batch.
 *
 * Record.  Row i owns 2 R floats, row-major [N_total][2 R], in concatenated scene order: floats 0 .. R-1 the ranges, floats
 * R .. 2R-1 the kind hit as a float: SFM_SCAN_NONE 0, _PEDESTRIAN 1, _BORDER 2, _STATIC 3, _VEHICLE 4.  A row that is masked out
 * is all zeros, and so is a row that is not live by sfm_batch_observe's test (|x| < NEAR_LIMIT and |y| < NEAR_LIMIT; a NaN
 * position fails it).
 *
 * Rules, all exact, for row i at (x, y), ray direction (ux, uy) and a disc at (px, py) with squared radius r2:
 *     ax = px - x;  ay = py - y
 *     t  = fmaf(ax, ux, ay * uy)
 *     c  = fmaf(ax, uy, -(ay * ux))
 *     q  = fmaf(-c, c, r2)
 *     candidate iff q > 0 and (t + w) > 0, with w = sqrt(q) correctly rounded
 *     s  = t - w;  range = s > 0 ? s : 0.0f        (inside a disc: 0)
 * The ray's value is the first minimum, under strict `<`, of range over the candidates in a fixed order: the scene's pedestrians
 * j != i ascending, then its border points, its static-obstacle points, its vehicle points; within a kind polylines in order and
 * points in order.  If the minimum is < Rmax it is stored with its kind; otherwise the ray stores Rmax and kind 0.  Ghosts, the
 * ring of an absent tracked vehicle (at +inf) and NaN positions fail q > 0 by themselves (c * c overflows or is NaN): there is no
 * test of their own.  Vehicles are read as the next tick would read them (the current half of the ping-pong), as in
 * sfm_batch_observe.  Only {x, y, vx, vy} of the state is used: a 3-D batch gives the planar record.
 * Frame 1 uses sfm_batch_observe's heading decision: v when fmaf(vx, vx, vy * vy) > 0, else the goal entry g = (wx - x, wy - y)
 * when fmaf(gx, gx, gy * gy) > 0, else (1, 0); with l = sqrt(.) and hx = a / l, hy = b / l, each correctly rounded, the ray is
 * u' = (fmaf(hx, ux, -(hy * uy)), fmaf(hy, ux, hx * uy)), and everything else is as in frame 0.
 * The kernel writes only the scan buffer and uses no atomics; every order is a function of the scene alone: a scene's record is
 * bitwise the same alone or anywhere in any batch.
 *
 * sfm_batch_set_scan allocates and zero-fills [N_total][2 R] and waits for the batch's stream; max_range = NULL switches scans
 * off and frees the buffer.  Refused with nothing changed: before sfm_batch_upload_state (SFM_ERR_STATE); R outside 1 .. 64; frame
 * outside {0, 1}; NULL dir_x, dir_y, ped_radius or point_radius; a direction that is not finite; a max_range that is NaN,
 * infinite, <= 0 or > 1e6; a radius that is NaN, negative, infinite or > 1e6.  sfm_batch_upload_state drops the scans (the mask
 * is per row), as it drops observations; every other call keeps them, and they keep the snapshot.  A snapshot neither holds nor
 * restores them. */
#define SFM_BATCH_MAX_SCAN_RAYS 64
#define SFM_SCAN_NONE 0
#define SFM_SCAN_PEDESTRIAN 1
#define SFM_SCAN_BORDER 2
#define SFM_SCAN_STATIC 3
#define SFM_SCAN_VEHICLE 4
int sfm_batch_set_scan(SfmBatch* b, int R, const float* dir_x, const float* dir_y, const float* max_range, const float* ped_radius,
                       const float* point_radius, const uint8_t* mask, int frame);
/* ONE launch on the batch's stream, ordered with the ticks, observations and restarts around it; the host does not wait.
 * SFM_ERR_STATE while scans are off.  With no rows it launches nothing and succeeds. */
int sfm_batch_scan(SfmBatch* b);
/* Synchronises the batch's stream, then copies the buffer ([N_total][2 R] floats) as the last sfm_batch_scan left it; before the
 * first scan that is zeros.  SFM_ERR_STATE while scans are off. */
int sfm_batch_download_scan(SfmBatch* b, float* out);
/* Egocentric occupancy grids on the device: the local map crowd-navigation policies are trained on beside the neighbour list and
 * the lidar.  A G x G grid centred on a row; per cell how many other pedestrians stand in it, how they move relative to the row,
 * and how many sampled points of borders, static obstacles and vehicles lie in it, by ONE launch of sfm_batch_grid_kernel (a
 * workgroup per scene) straight from the buffers the tick reads, into a device buffer a policy can feed to a convolution as it
 * stands.  The record is defined bit for bit in BOTH frames: every operation below is a single correctly rounded fp32 operation or
 * an fmaf.
 * These three entry points and SFM_BATCH_PTR_GRID were added WITHOUT a bump of SFM_ABI_VERSION (it stays 17), like the restart
 * noise: additions only, nothing that existed changes its meaning, and a build that has them is recognised by the symbols.
 *
 * Settings (sfm_batch_set_grid).  G: cells per side, 1 .. SFM_BATCH_MAX_GRID, one value for the batch.  cell[b]: the cell size in
 * metres, per scene, finite, 0 < c <= SFM_BATCH_MAX_SENSE_RANGE, used as the fp32 value.  mask [N_total] uint8_t, or NULL for every
 * row: which rows are gridded (nonzero); a row without a slot costs nothing.  frame: SFM_OBS_FRAME_WORLD (0) or
 * SFM_OBS_FRAME_HEADING (1), one value for the batch.
 *
 * Record.  The gridded rows get compact slots: a row's slot is its rank among the masked rows of the whole batch in ascending
 * (concatenated) row order; with M of them the buffer is [M][SFM_BATCH_GRID_CHANNELS][G][G] float, slot-major, the cell [cv][cu]
 * of channel ch at ((slot * 6 + ch) * G + cv) * G + cu.  The grid spans [-G/2 c, G/2 c) on both axes around the row; u runs along
 * x and v along y (frame 1: x is forward, y to the left).  Channel 0: the number of pedestrian sources in the cell -- a source is a
 * row j != i of the scene that is live by sfm_batch_observe's test.  Channels 1 and 2: the SUM (not the mean: divide by channel 0)
 * of those pedestrians' relative velocities (vx_j - vx, vy_j - vy), rotated in frame 1 like the positions, formed in ascending j by
 * fp32 adds starting from 0.0f.  Channels 3, 4, 5: the number of border points, static-obstacle ring points and vehicle ring points
 * in the cell -- the model's own sampled view of geometry, as in sfm_batch_scan.  Counts are exact in fp32.  A gridded row that is
 * not live (|x| < NEAR_LIMIT and |y| < NEAR_LIMIT fails; a NaN position fails it) is all zeros.
 *
 * Rules, all exact, for row i at (x, y), a cell size c and a source at (px, py):
 *     ax = px - x;  ay = py - y
 *     frame 0:  fx = ax;  fy = ay                                     (no rotation is performed)
 *     frame 1:  fx = fmaf(hx, ax, hy * ay);  fy = fmaf(hx, ay, -(hy * ax))
 *     half = 0.5f * G                                                 (exact)
 *     pu = fx / c + half;  pv = fy / c + half                         (the division is rounded first, then the sum)
 *     inside iff 0 <= pu < G and 0 <= pv < G                          (float compares)
 *     cu = (int)pu;  cv = (int)pv
 * (hx, hy) is sfm_batch_scan's heading of frame 1, fp32 throughout: v when fmaf(vx, vx, vy * vy) > 0, else the goal entry
 * g = (wx - x, wy - y) when fmaf(gx, gx, gy * gy) > 0, else (1, 0); with l = sqrt(.), hx = a / l, hy = b / l, each correctly
 * rounded.  NaN and +-inf fail the compares by themselves, so the ring of an absent tracked vehicle (at +inf) is never binned and
 * there is no test of its own.  The sum decides the cell: a source whose fx / c is a tiny negative number is rounded up to
 * pu = half and lies in cell (int)half, and one whose pu rounds up to G is outside.  Vehicles are read as the next tick would read
 * them.  Only {x, y, vx, vy} of the state is used: a 3-D batch gives the planar record.  Vehicle velocities per cell are not
 * recorded.
 * The kernel writes only the grid buffer and uses no float atomics; every order is a function of the scene alone: a scene's
 * record is bitwise the same alone or anywhere in any batch.
 *
 * sfm_batch_set_grid allocates and zero-fills the buffer (its size is computed in 64 bits) and waits for the batch's stream;
 * cell = NULL switches grids off and frees the buffer.  Refused with nothing changed: before sfm_batch_upload_state
 * (SFM_ERR_STATE); G outside 1 .. 32; frame outside {0, 1}; a cell size that is NaN, infinite, <= 0 or > 1e6.
 * sfm_batch_upload_state drops the grids (the slots are per row); every other call keeps them, and they keep the snapshot.  A
 * snapshot neither holds nor restores them.
 * SFM_BATCH_PTR_GRID (sfm_batch_device_ptr): the grid buffer, valid until the next sfm_batch_set_grid or sfm_batch_upload_state;
 * NULL without gridded rows; while grids are off the value is refused as the unknown `which` it was before. */
#define SFM_BATCH_PTR_GRID 7
#define SFM_BATCH_MAX_GRID 32
#define SFM_BATCH_GRID_CHANNELS 6
int sfm_batch_set_grid(SfmBatch* b, int G, const float* cell, const uint8_t* mask, int frame);
/* ONE launch on the batch's stream, ordered with the ticks, the other sensors and the restarts around it; the host does not wait.
 * SFM_ERR_STATE while grids are off.  With no gridded row it launches nothing and succeeds. */
int sfm_batch_grid(SfmBatch* b);
/* Synchronises the batch's stream, then copies the buffer ([M][6][G][G] floats) as the last sfm_batch_grid left it; before the
 * first that is zeros.  SFM_ERR_STATE while grids are off. */
int sfm_batch_download_grid(SfmBatch* b, float* out);
/* Observed tracks on the device: the calibration protocol of Johansson et al. 2007.  A few pedestrians are simulated by the model,
 * everybody else in the scene replays the recorded motion, and the simulated ones are scored by their displacement from their own
 * recorded tracks -- the reference's update_ped_info -> PedState.update_state (run_simulation.py:79-87, pedestrian_state.py:79-81)
 * with the recording and the error sums living on the device.  A sweep is sfm_batch_set_params, sfm_batch_run_observed(0, F),
 * sfm_batch_score, and one copy of B x 5 floats per candidate.
 * These four entry points and SFM_BATCH_PTR_ROW_SCORES / _SCENE_SCORES were added WITHOUT a bump of SFM_ABI_VERSION (it stays 17),
 * like the restart noise and the grids: additions only, and a build that has them is recognised by the symbols.
 *
 * Data (sfm_batch_set_observed), set once.  Per scene b its track frames: frames[b] = F_b, 0 <= F_b <=
 * SFM_BATCH_MAX_OBSERVED_FRAMES, of n_b positions each, float2 {x, y}, frame-major: the position of row i (inside the scene) in
 * frame f is obs_xy[2 (obs_off[b] + f n_b + i)] and the float behind it; obs_off [B+1] counts positions, obs_off[0] = 0,
 * obs_off[b+1] = obs_off[b] + F_b n_b.  A row not seen in a frame holds NaN in BOTH components; every other value is finite with
 * |x|, |y| <= SFM_BATCH_MAX_SENSE_RANGE (1e6 m).  All frames together hold at most SFM_BATCH_MAX_RECORD_BYTES.  Per row
 * role [N_total]: SFM_ROLE_NONE 0, not part of the data -- every kernel below leaves the row alone, bit for bit; SFM_ROLE_REPLAYED 1;
 * SFM_ROLE_SCORED 2, simulated by the model and compared with its track.  Per row an optional initial velocity v0_xy [N_total][2]
 * (NULL: none given): NaN in both components means "take it from the track"; otherwise finite.  every >= 1: the ticks between two
 * observed frames, one value for the batch.  Derived on the host: per scene inv_h[b] = float32(1 / (every * step_length_b)),
 * formed in double and rounded once (while observed tracks are on, sfm_batch_set_params forms it again from the new step lengths,
 * and refuses, with nothing changed, step lengths this call would refuse); per row the span
 * [f0, f1] of its first and last observed frame, empty for a row that is never seen.
 *
 * The frame kernel (sfm_batch_replay_kernel, ONE launch per frame, a workgroup per scene) takes the frame f as an argument and
 * writes only the state {x, y, vx, vy}, the command {ux, uy, uz, kind} and the score record of rows of role 1 and 2.  Every value
 * is one correctly rounded fp32 operation or an fmaf, every decision a plain comparison.  "Observed at g": 0 <= g < F_b and the
 * row's position in frame g is not NaN.  "Parked": position = where a despawned row waits (keyed by the index inside the scene,
 * beyond NEAR_LIMIT: sfm_batch_observe's live test fails for it and it exerts no force on anyone), velocity 0, command
 * {0, 0, 0, 1}, so the ticks hold it there.  With o = the row's position in frame f:
 *   Role 1, observed at f: position := o bit for bit; velocity v := (o' - o) * inv_h per component (one subtraction, one
 *     multiplication) with o' the position in frame f + 1 if the row is observed there; else (o - o") * inv_h with o" that of
 *     frame f - 1 if observed there; else v0 if given; else 0.  State velocity := v, command := {v.x, v.y, 0, 1}: the following
 *     `every` ticks move it by their own fma(step_length, v, x), and the next frame puts it back on the track -- nothing drifts.
 *   Role 1, not observed at f (f >= F_b, outside its span, or a gap): parked.
 *   Role 2 with f < f0, f > f1 or an empty span: parked.
 *   Role 2, f == f0: position := o; velocity := v0 if given, else the forward difference above if the row is observed at f + 1,
 *     else 0; command {0, 0, 0, 0}: the model moves it from here on.
 *   Role 2, f0 < f <= f1: state untouched, command {0, 0, 0, 0}.  If observed at f, with {x, y} of the state as the ticks left
 *     it: dx = x - o.x, dy = y - o.y, d2 = fmaf(dx, dx, dy * dy), d = sqrtf(d2) (correctly rounded), and the row's record
 *     {samples, sum_d, sum_d2, last_d2} becomes {samples + 1, sum_d + d, sum_d2 + d2, d2}.  The lane that owns the row is its only
 *     writer, so the sums are taken in frame order.  A gap inside the span is not scored.  A state that is not finite goes into
 *     the sums as it is (NaN or inf): nothing is filtered.
 * The record is four floats per row, [N_total][4]; samples is a count held as a float (exact: at most 16 384).
 *
 * Steering.  Observed rows are driven through the command buffer: if steering is off, sfm_batch_set_observed switches it on with
 * every kind 0, and the ticks' steered form is what runs from then on.  Rows of role 0 keep whatever steering the caller gave them,
 * so an ego policy can live in a replayed scene.  sfm_batch_set_steering and sfm_batch_set_commands overwrite the kinds and
 * commands the frame kernel wrote, as they overwrite what a caller changed on the device; the next frame writes them again.
 *
 * What drops the observed tracks: sfm_batch_upload_state (the roles are per row); the "on" forms of sfm_batch_set_mode_fsm and
 * sfm_batch_set_spawn_schedule (they own parking and birth); sfm_batch_set_steering(kind = NULL).  Every other call keeps them.
 * A snapshot neither holds nor restores the scores; sfm_batch_restart puts back rows of every role, and the next frame kernel places
 * roles 1 and 2 again.
 *
 * sfm_batch_set_observed uploads all this, zero-fills the scores and waits for the batch's stream; obs_off = NULL switches the
 * observed tracks off and frees them (steering stays as it is).  Refused with nothing sent, freed or launched, the batch staying
 * usable: no state uploaded (SFM_ERR_STATE); a 3-D batch; modes or a spawn schedule set (SFM_ERR_STATE); NULL frames or role (with
 * rows); NULL obs_xy with positions; every < 1; an F_b outside 0 .. 16384; obs_off that does not fit the frames; more than
 * SFM_BATCH_MAX_RECORD_BYTES of frames; a role above 2; a position that is half NaN, infinite or beyond 1e6 m; a v0 that is half
 * NaN or not finite; a scene whose every * step_length is not finite and positive in fp32. */
#define SFM_BATCH_MAX_OBSERVED_FRAMES 16384
#define SFM_ROLE_NONE 0
#define SFM_ROLE_REPLAYED 1
#define SFM_ROLE_SCORED 2
#define SFM_BATCH_PTR_ROW_SCORES 8
#define SFM_BATCH_PTR_SCENE_SCORES 9
#define SFM_BATCH_SCENE_SCORE_WIDTH 5
int sfm_batch_set_observed(SfmBatch* b, const int64_t* obs_off, const int32_t* frames, const float* obs_xy, const uint8_t* role,
                           const float* v0_xy, int every);
/* Frames first_frame .. first_frame + frames - 1: per frame ONE launch of the frame kernel, then `every` ticks exactly as
 * sfm_batch_run(b, every, flags) launches them -- all on the batch's stream, no copy and no wait in between.  flags must contain
 * SFM_TICK_INTEGRATE (SFM_TICK_REDRAW_WAYPOINTS as for sfm_batch_run).  first_frame = 0 first clears the row scores with one
 * hipMemsetAsync; a later first_frame continues a run.  Frames beyond a scene's F_b park its rows of role 1 and 2, so scenes of
 * different lengths share a batch.  Starting at frame 0 places every row of role 1 or 2: a scene made only of such rows needs no
 * snapshot between candidates (rows of role 0, waypoint draws and vehicles still need sfm_batch_restart).  Refused with nothing
 * launched: observed tracks off (SFM_ERR_STATE), flags without SFM_TICK_INTEGRATE or with a flag sfm_batch_run refuses,
 * first_frame < 0, frames < 0, first_frame + frames beyond 2^31 - 1. */
int sfm_batch_run_observed(SfmBatch* b, int first_frame, int frames, uint32_t flags);
/* Per scene five floats, [B][SFM_BATCH_SCENE_SCORE_WIDTH], from the row scores by ONE launch of sfm_batch_score_kernel (a
 * workgroup per scene) on the batch's stream: rows (those with samples > 0), samples, sum_d, sum_d2 and sum_final_d (the sum of
 * sqrtf(last_d2)), each over the rows with samples > 0.  ADE = sum_d / samples, RMSE = sqrt(sum_d2 / samples), FDE = sum_final_d /
 * rows.  The counts are exact in fp32 (1 024 rows x 16 384 frames = 2^24).  The order of summation is part of the definition: lane
 * t of 256 adds its rows t, t + 256, ... in ascending order starting from +0; then an xor-shuffle tree of widths 32, 16, .. 1
 * inside each wave of 64 (both partners form the same sum, addition commutes); then thread 0 adds waves 0 .. 3 in ascending
 * order.  No float atomics: a scene's scores are bitwise the same alone or anywhere in any batch.  SFM_ERR_STATE while observed
 * tracks are off. */
int sfm_batch_score(SfmBatch* b);
/* Synchronises the batch's stream, then copies the row scores ([N_total][4] floats, as the last frame kernel left them) and the
 * scene scores ([B][5] floats, as the last sfm_batch_score left them; zeros before the first); NULL skips either.  SFM_ERR_STATE
 * while observed tracks are off.  SFM_BATCH_PTR_ROW_SCORES and SFM_BATCH_PTR_SCENE_SCORES (sfm_batch_device_ptr) are the two
 * buffers on the device, valid until the next sfm_batch_set_observed or a call that drops the tracks; while observed tracks are off
 * the values are refused as the unknown `which` they were before. */
int sfm_batch_download_scores(SfmBatch* b, float* row_scores, float* scene_scores);
/* Driven vehicles: device-side vehicles (sfm_batch_set_dynamic_boxes) whose motion is decided while the batch runs -- a driving
 * policy being trained against the crowd, a planner under test, a braking controller.  The reference reads each vehicle's transform
 * and velocity from the simulator every tick, whoever drives it (obstacles.py:314-317); here the command lives in a device buffer
 * that the tick's one launch reads.  These entry points, the vehicle observations below and SFM_BATCH_PTR_VEHICLE_COMMANDS /
 * _VEHICLE_OBS were added WITHOUT a bump of SFM_ABI_VERSION (it stays 17), like the restart noise, the grids and the observed
 * tracks: additions only, and a build that has them is recognised by the symbols.
 *
 * Command.  Vehicle k (an index into the M vehicles of all scenes, as in sfm_batch_set_dynamic_boxes) has a command {a, b, c, kind},
 * [M] float4 with the kind held as a float.  Every tick with SFM_TICK_INTEGRATE reads it and never writes it; a tick without the
 * flag moves no vehicle and reads no command.  sfm_batch_run, sfm_batch_run_recorded and sfm_batch_run_recorded_forces hold the
 * commands for all their ticks (for kind 2 the turn applies every tick).
 *
 * Heading.  Each vehicle has a heading h = (cos, sin): the yaw sfm_batch_set_dynamic_boxes gave it.  A driven tick rewrites it, so
 * it is state: sfm_batch_snapshot holds it, and sfm_batch_restart, sfm_batch_restart_device and the auto restart put back the chosen
 * scenes' centres, rings, velocities and headings (other scenes are left bit for bit).  Restart noise leaves a driven vehicle at its
 * snapshot pose (its traffic-timing delay is not applied while its kind is 1 or 2).
 *
 * The rule (drive_vehicle, the one definition).  Every line is one correctly rounded fp32 operation or an fmaf, sqrtf and / are the
 * correctly rounded forms; dt is the scene's step_length and (cx, cy, vx, vy) the vehicle as this tick reads it.
 *   kind 0, or any value other than 1 and 2: not driven -- the vehicle runs free or follows its track exactly as without driving.
 *   kind 1, velocity: s2 = fmaf(a, a, b * b); h' = (a / s, b / s) with s = sqrtf(s2) when s2 > 0, else h' = h (a stopped vehicle
 *     keeps its heading); v' = (a, b); c is ignored.
 *   kind 2, unicycle: signed speed a and this tick's turn (b, c) = (cos dpsi, sin dpsi), supplied by the caller -- the kernel does
 *     no trigonometry.  g = (fmaf(b, hx, -(c * hy)), fmaf(c, hx, b * hy)); n2 = fmaf(gx, gx, gy * gy); h' = (gx / n, gy / n) with
 *     n = sqrtf(n2) when n2 > 0, else h' = h; v' = (a * h'x, a * h'y).  A negative a reverses.
 *   Both: centre' = (fmaf(dt, v'x, cx), fmaf(dt, v'y, cy)); the stored velocity becomes v' -- what the dynamic obstacle force and
 *     gap acceptance see from the next tick on; ring point p = (fmaf(h'x, ux, fmaf(-h'y, uy, cx')), fmaf(h'y, ux, fmaf(h'x, uy, cy')))
 *     for the ring-local offset (ux, uy), as every vehicle's ring is formed.
 *   A driven vehicle with keyframes (sfm_batch_set_vehicle_tracks) ignores them while its kind is 1 or 2; the tracks' tick counter
 *     goes on counting, and when the kind goes back to 0 the track takes over at that tick.
 *   A driven vehicle whose centre is not finite stays absent as an absent tracked vehicle is: centre and ring +inf, velocity 0, the
 *     heading kept.
 *
 * sfm_batch_set_vehicle_driving: kind [M] uint8 and a, b, c [M] float; kind = NULL switches driving off.  Refused with nothing
 * changed: no device-side vehicles (SFM_ERR_STATE); a kind above 2; a NULL a, b or c; a command of a driven vehicle that is not
 * finite.  sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop driving (and the vehicle observations), because the
 * vehicles may differ; every other call keeps it.  Commands are an input, like pedestrian steering: a snapshot neither holds nor
 * restores them.
 * sfm_batch_set_vehicle_commands: new a, b, c for the kinds of the last sfm_batch_set_vehicle_driving -- ONE copy from pinned memory,
 * ordered on the batch's stream, like sfm_batch_set_commands.  SFM_ERR_STATE while driving is off.
 * sfm_batch_download_vehicle_driving: synchronises the stream; kind as the tick takes it (0, 1 or 2), the command, and the headings
 * and velocities as the next tick reads them; NULL skips a column.  SFM_ERR_STATE while driving is off.
 * SFM_BATCH_PTR_VEHICLE_COMMANDS (sfm_batch_device_ptr): the command buffer on the device, [M] float4, valid until driving is set
 * again or dropped.  Values written on the device are not validated; a kind other than 1 or 2 counts as 0.  While driving is off
 * the value is refused as the unknown `which` it was before. */
#define SFM_BATCH_PTR_VEHICLE_COMMANDS 10
#define SFM_BATCH_PTR_VEHICLE_OBS 11
#define SFM_DRIVE_NONE 0
#define SFM_DRIVE_VELOCITY 1
#define SFM_DRIVE_UNICYCLE 2
int sfm_batch_set_vehicle_driving(SfmBatch* b, const uint8_t* kind, const float* a, const float* b_, const float* c);
int sfm_batch_set_vehicle_commands(SfmBatch* b, const float* a, const float* b_, const float* c);
int sfm_batch_download_vehicle_driving(SfmBatch* b, uint8_t* kind, float* a, float* b_, float* c, float* hx, float* hy, float* vx,
                                       float* vy);
/* Vehicle observations: what a driving policy and its reward read per vehicle, by ONE launch of sfm_batch_vehicle_observe_kernel (a
 * workgroup per scene, a wave per vehicle, lanes striding over pedestrians and points; every reduction a lexicographic (d2, index)
 * minimum by shuffles; no atomics) over the buffers the next tick would read.  It writes only its own buffer.
 *
 * Settings (sfm_batch_set_vehicle_observation): k neighbour slots, 1 .. SFM_BATCH_MAX_OBS_NEIGHBOURS, for the batch; sense_range
 * [B], validated and squared as sfm_batch_set_observation does it (R2 below); frame 0 or 1; goal_x, goal_y [M], finite (NULL, both:
 * zeros); mask [M] (NULL: every vehicle) -- a vehicle outside the mask costs nothing and reads zeros.  sense_range = NULL switches
 * the observations off.  The call zero-fills the buffer and waits for the stream.  Refused with nothing changed: no state
 * (SFM_ERR_STATE); no device-side vehicles (SFM_ERR_STATE); k, frame, a range or a goal out of bounds.
 *
 * Record: [M][SFM_BATCH_OBS_HEADER + 4 k] floats, for a vehicle with centre c, velocity v and heading h (d2 of a point q from c:
 * dx = q.x - cx, dy = q.y - cy, fmaf(dx, dx, dy * dy)):
 *   0-1   goal - centre                         2-3   velocity                      4-5   heading h, always in world axes
 *   6     present: 1.0 iff the centre is finite and |cx|, |cy| < 1e12; otherwise the WHOLE record is zeros
 *   7     m, the number of filled neighbour slots
 *   8     clear_d2: the minimum over this vehicle's ring points p and the scene's live rows j of fmaf(dx, dx, dy * dy) with
 *         dx = x_j - px; +inf with no live row or an empty ring; not limited by the range (collisions, near-miss rewards)
 *   9     other_d2: the minimum over the OTHER present vehicles of the scene of the squared centre distance; +inf when none
 *   10-11 nearest border point - centre: the first minimum over all border points of the scene in polyline order, then point
 *         order; present iff d2 < R2, else zeros          12-13 nearest static-obstacle point - centre, likewise
 *   14    flags: 1 border point present + 2 static point present
 *   15    signed speed along the heading, fmaf(vx, hx, vy * hy)
 *   16+4s slot s: (x_j - cx, y_j - cy, vx_j - vx, vy_j - vy) -- the slots hold the first k live rows with d2 < R2 (strict) in
 *         ascending (d2, j) order; empty slots are zeros.  "Live" is sfm_batch_observe's test.
 * Frame 1 decides everything in frame 0 first and then replaces every 2-vector (p, q) except slots 4-5 by
 * (fmaf(hx, p, hy * q), fmaf(hx, q, -(hy * p))); the heading is used as stored.  Both frames are defined bit for bit.
 * A tracked vehicle that is not driven is observed with the heading sfm_batch_set_dynamic_boxes gave it, not its keyframe's yaw: a
 * policy observes the vehicle it drives.
 * sfm_batch_observe_vehicles: the launch, on the batch's stream; the host does not wait.  sfm_batch_download_vehicle_observations
 * synchronises the stream and copies the buffer (zeros before the first launch).  SFM_BATCH_PTR_VEHICLE_OBS (sfm_batch_device_ptr):
 * the buffer on the device.  All SFM_ERR_STATE while the observations are off (the pointer value: refused as unknown). */
int sfm_batch_set_vehicle_observation(SfmBatch* b, int k, const float* sense_range, int frame, const float* goal_x, const float* goal_y,
                                      const uint8_t* mask);
int sfm_batch_observe_vehicles(SfmBatch* b);
int sfm_batch_download_vehicle_observations(SfmBatch* b, float* out);
/* Range scans from the vehicles: the lidar of a driving policy, by ONE launch of sfm_batch_vehicle_scan_kernel (a workgroup per
 * scene, a lane per (vehicle, ray) pair; no atomics) over the buffers the next tick would read.  It writes only its own buffer.
 * sfm_batch_scan casts from pedestrian rows, offers 64 rays and counts every vehicle ring as an obstacle; this casts from a sensor
 * mounted on a device-side vehicle (sfm_batch_set_dynamic_boxes), offers 256 rays and leaves the vehicle's OWN ring out.
 * These three entry points and SFM_BATCH_PTR_VEHICLE_SCAN were added WITHOUT a bump of SFM_ABI_VERSION (it stays 17), like the
 * driven vehicles: additions only, and a build that has them is recognised by the symbols.
 *
 * Settings (sfm_batch_set_vehicle_scan), for the whole batch unless marked per scene.  R: rays per vehicle, 1 ..
 * SFM_BATCH_MAX_VEHICLE_SCAN_RAYS.  dir_x, dir_y [R]: fp32, finite, used as given and NOT renormalised.  max_range[b]: per scene,
 * finite, 0 < Rmax <= SFM_BATCH_MAX_SENSE_RANGE, the fp32 value as given.  ped_radius[b], point_radius[b]: per scene, finite,
 * 0 <= r <= 1e6; the kernel uses r2 = float32(double(r) * r), and a radius of 0 switches that kind off.  mask [M] uint8_t, or NULL
 * for every vehicle, M the number of device-side vehicles (the items of sfm_batch_set_dynamic_boxes): a vehicle outside the mask
 * costs nothing and reads zeros.  frame: SFM_OBS_FRAME_WORLD (0) or SFM_OBS_FRAME_HEADING (1, the vehicle's heading frame).
 * mount_x, mount_y: where the sensor sits in the vehicle frame, metres, x forward; fp32, finite, |m| <= 1e6; one pair for the batch.
 *
 * Record: [M][2R] floats in the vehicles' concatenated order.  Floats 0 .. R-1: the ranges.  Floats R .. 2R-1: the kind hit, the
 * SFM_SCAN_* values (0 none, 1 pedestrian, 2 border, 3 static, 4 vehicle).
 *
 * Rules for vehicle k of scene b, all exact: every value is one correctly rounded fp32 operation or an fmaf.  (cx, cy) is the
 * vehicle's centre, (hx, hy) its stored heading {cos, sin} as sfm_batch_observe_vehicles reads it -- used as stored, never
 * renormalised, and for a tracked vehicle that is not driven the heading sfm_batch_set_dynamic_boxes gave it, not its keyframe's yaw.
 *   Present: iff |cx| < 1e12 and |cy| < 1e12 (sfm_batch_observe's live test; NaN fails it).  Otherwise the WHOLE record is zeros: an
 *     absent tracked vehicle sits at +inf and fails the test.
 *   Origin:  rx = fmaf(hx, mx, -(hy * my));  ry = fmaf(hy, mx, hx * my);  ox = cx + rx;  oy = cy + ry     (m the mount)
 *   Ray:     frame 0: (ux, uy) as given.  frame 1: (fmaf(hx, ux, -(hy * uy)), fmaf(hy, ux, hx * uy)) -- sfm_batch_scan's rule with
 *     the stored heading in place of the derived one.
 *   Per disc at (px, py) with r2, sfm_batch_scan's rules unchanged:
 *     ax = px - ox;  ay = py - oy;  t = fmaf(ax, ux, ay * uy);  c = fmaf(ax, uy, -(ay * ux));  q = fmaf(-c, c, r2)
 *     candidate iff q > 0 and (t + w) > 0 with w = sqrtf(q) correctly rounded;  range = max(t - w, 0)
 *   Ray value: the first minimum under strict `<` in this fixed order: the scene's pedestrians j ascending (EVERY row is walked,
 *     none is excluded: ghosts, NaN positions and rings at +inf fail q > 0 by themselves), then the border points, then the
 *     static-obstacle points, then the ring points of the scene's vehicles OTHER than k; within a kind polylines in order, points in
 *     order.  A minimum below Rmax is stored with its kind; otherwise the ray stores Rmax and kind 0.
 * Vehicles are read as the next tick would read them, from the current half of the ping-pong.  Only x and y of the state are used:
 * a 3-D batch gives the planar record.  A scene with vehicles and no pedestrians still scans its geometry.
 * The kernel uses no atomics and every order is a function of the scene alone: a scene's record is bitwise the same alone or
 * anywhere in any batch.
 *
 * sfm_batch_set_vehicle_scan allocates and zero-fills the buffer and waits for the batch's stream; max_range = NULL switches the
 * scan off and frees the buffer.  Refused with nothing changed: no state, or no device-side vehicles (SFM_ERR_STATE); R or frame
 * out of bounds; a direction, range, radius or mount that is not finite or out of bounds; a NULL dir_x, dir_y, ped_radius or
 * point_radius.  sfm_batch_upload_state drops the scan, and so do sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles,
 * exactly as they drop the vehicle observations (the buffer and the mask are per vehicle); every other call keeps it, and it keeps
 * the snapshot.  A snapshot neither holds nor restores the scan.
 * sfm_batch_scan_vehicles: ONE launch on the batch's stream, ordered with the ticks, the other sensors and the restarts around it;
 * the host does not wait.  With no vehicles it launches nothing and succeeds.  sfm_batch_download_vehicle_scan synchronises the
 * stream and copies the buffer ([M][2R] floats; zeros before the first launch).  SFM_BATCH_PTR_VEHICLE_SCAN (sfm_batch_device_ptr):
 * the buffer on the device, valid until the next sfm_batch_set_vehicle_scan or a call that drops the scan.  All three give
 * SFM_ERR_STATE while the scan is off. */
#define SFM_BATCH_PTR_VEHICLE_SCAN 12
#define SFM_BATCH_MAX_VEHICLE_SCAN_RAYS 256
int sfm_batch_set_vehicle_scan(SfmBatch* b, int R, const float* dir_x, const float* dir_y, const float* max_range,
                               const float* ped_radius, const float* point_radius, const uint8_t* mask, int frame,
                               float mount_x, float mount_y);
int sfm_batch_scan_vehicles(SfmBatch* b);
int sfm_batch_download_vehicle_scan(SfmBatch* b, float* out);
/* Current state of every scene (synchronises the batch's stream); NULL skips a column.  A planar batch leaves z alone and
 * writes vz = 0. */
int sfm_batch_download_state(SfmBatch* b, float* x, float* y, float* z, float* vx, float* vy, float* vz);
const char* sfm_batch_last_error(const SfmBatch* b);

#ifdef __cplusplus
}
#endif
#endif /* SFM_HIP_H */
