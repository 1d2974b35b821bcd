// sfm_batch_host.h -- what the two host files of the batched scenes share: the batch itself (SfmBatch and the struct of each of its
// features), its error plumbing, and the messages for a feature that is off.  sfm_batch_capi.hip holds the ticks and everything they
// read or write; sfm_batch_sense_capi.hip the read-only sensors (observations, episode ends, range scans, occupancy grids) and the device pointers;
// sfm_batch_reset_capi.hip the restart noise; sfm_batch_replay_capi.hip the observed tracks; sfm_batch_drive_capi.hip the driven
// vehicles and the vehicle observations (the vehicles' range scans are a sensor: sfm_batch_sense_capi.hip); sfm_batch_route_capi.hip
// the routes over walk graphs; sfm_batch_row_episode_capi.hip the row episodes and the row respawns; sfm_batch_vehicle_episode_capi.hip
// the vehicle episodes and the vehicle respawns.
#pragma once
#include "sfm_capi_common.h"
#include "sfm_metres.h"

namespace sfm {

// Each feature of a batch keeps its arrays in one struct whose default value is "off": dropping the feature is `x = {}`, after the
// caller has synchronised the stream (a tick in flight may still read the arrays).

struct BatchGeoDev {           // one kind of polylines over all scenes
    DevBuf<int> off;           // [K+1]
    DevBuf<float2> pts;        // [P]
    DevBuf<float4> ctr;        // [K]
    int K = 0;
    int P = 0;
};

// grids, around the rows (SfmBatch::grid: sfm_batch_set_grid) and around the vehicles (BatchBoxesDev::vgrid:
// sfm_batch_set_vehicle_grid): the settings and the buffer sfm_batch_grid / sfm_batch_grid_vehicles fills, one slot per gridded item
// -- a row, or a vehicle; nothing a tick reads or writes.  The vehicles' live inside the boxes they refer to (slots and buffer are per
// vehicle), so whatever replaces or drops the boxes drops them with no line of its own; sfm_batch_upload_state drops them too.
struct BatchGridDev {
    bool on = false;           // (not "buf is allocated": a batch without gridded items can be gridded and has no buffer)
    int GU = 0, GV = 0;        // the rows' grid: both G
    int frame = 0;
    float centre_x = 0.f, centre_y = 0.f;  // the middle of the window in the vehicle frame; the rows' window is centred on the row: 0
    size_t M = 0;              // gridded items: the slots of buf
    DevBuf<float> cell;        // [B]
    DevBuf<int> slot;          // [items]; not allocated: every item is gridded, slot = item
    DevBuf<float> buf;         // [M][channels][GV][GU]: 6 channels for a row, 8 for a vehicle
    size_t vals(int channels) const { return M * (size_t)channels * (size_t)GU * (size_t)GV; }    // (64 bits)
};

// vehicle episodes (sfm_batch_set_vehicle_episodes): the episodes per VEHICLE -- the settings, the scenes' agent lists, the
// per-vehicle episode state, and the record and the two masks sfm_batch_end_vehicle_step fills; nothing a tick reads or writes.  They
// live inside the boxes they refer to, like the vehicles' grids: whatever replaces or drops the boxes drops them.
struct BatchVehEpisodeDev {
    bool on = false;           // (not "record is allocated": a batch without vehicles can have vehicle episodes and has no buffers)
    DevBuf<VehicleEpisodeScene> set;   // [B]
    DevBuf<int> agent_off;             // [B+1]
    DevBuf<int> agent_veh;             // [agents] indices over the vehicles of all scenes, ascending
    DevBuf<float4> goal_ext;           // [M] {goal_x, goal_y, half length, half width}
    DevBuf<int> age;                   // [M]
    DevBuf<float> prev;                // [M] prev_goal_d2
    DevBuf<float> record;              // [M][8]
    DevBuf<uint8_t> done;              // [M]
    DevBuf<uint8_t> scene_done;        // [B]
};

// device-side vehicles (sfm_batch_set_dynamic_boxes): geo[2].ctr / .pts hold the vehicles the next tick sees, ctr_alt / pts_alt
// (the same sizes) the half an integrating tick writes; batch_launch swaps them after each such launch
struct BatchBoxesDev {
    bool on = false;
    DevBuf<float2> local;      // [P] ring-local offsets
    DevBuf<float2> rot;        // [M] {cos yaw, sin yaw}
    DevBuf<float4> ctr_alt;
    DevBuf<float2> pts_alt;
    std::vector<int32_t> item_off_h;   // the vehicles' scene_item_off [B+1] on the host
    BatchGridDev vgrid;        // the bird's-eye grids around these vehicles (sfm_batch_set_vehicle_grid)
    BatchVehEpisodeDev vep;    // the episodes of these vehicles (sfm_batch_set_vehicle_episodes)
};

// scripted vehicle tracks (sfm_batch_set_vehicle_tracks, ABI 12): read-only on the device; dropped with the boxes they refer to
struct BatchTracksDev {
    bool on = false;
    DevBuf<int> off;           // [M+1]
    DevBuf<int> first;         // [M]
    DevBuf<float4> key;        // [T] {x, y, vx, vy}
    DevBuf<float2> rot;        // [T] {cos yaw, sin yaw}
    long long tick = 0;        // tau: integrating ticks since the tracks were set (a kernel argument, not device state)
    std::vector<int32_t> off_h, first_h;   // host copies: sfm_batch_download_vehicle_tracks answers without the device
    bool first_stale = false;  // a restart by device mask moved `first` of scenes the host cannot know: first_h is refreshed from
                               // the device before it is read (refresh_track_first)
};

// the mode state machine (sfm_batch_set_mode_fsm, ABI 9): per row over the concatenated rows, per scene [B]
struct BatchModesDev {
    bool on = false;
    DevBuf<uint8_t> mode;
    DevBuf<float> target;
    DevBuf<float4> speeds;     // {initial_speed, crossing_speed, safety_margin, next_mode_time}
    DevBuf<int> off;           // [N_total+1]
    DevBuf<float2> xy;
    DevBuf<uint8_t> cross;
    DevBuf<int> cursor;
    DevBuf<BatchModeScene> scene;   // [B]
    DevBuf<float> time;        // [B] the scenes' clocks
};

// the spawn schedule (sfm_batch_set_spawn_schedule, ABI 11): per row; dropped with the modes it refers to
struct BatchSpawnDev {
    bool on = false;           // (not "time is allocated": a schedule over no rows still holds one element)
    DevBuf<float> time;
    DevBuf<uint8_t> chain;
    DevBuf<uint8_t> born;
    DevBuf<float> birth;
    DevBuf<float4> pk0;        // the spawn state: the rows as they were when the schedule was set
    DevBuf<float2> zv0;
};

// the snapshot (sfm_batch_snapshot / sfm_batch_restart, ABI 13): a copy of every array a tick can change, grow-only (`on = false`
// drops the snapshot and keeps the memory); what it holds follows boxes / modes / spawns / tracks, which cannot change while
// it is valid (every call that changes them drops it)
struct BatchSnapDev {
    bool on = false;
    DevBuf<float4> pk, own, ctr;
    DevBuf<float2> zv, pts, rot;
    DevBuf<uint32_t> draws;
    DevBuf<uint8_t> mode, born;
    DevBuf<float> target, time, birth;
    DevBuf<int> cursor, first;
    long long tick = 0;                // the tracks' tick when the snapshot was taken
    std::vector<int32_t> first_h;      // the tracks' first_h when the snapshot was taken
};

// sfm_batch_restart's list of chosen scenes: pinned on the host, copied to `list` on the stream; `done` is recorded behind the
// launch that reads it, and the next masked restart waits for it before it refills the pinned list
struct BatchRestartDev {
    DevBuf<int> list;
    PinnedBuf<int> list_h;
    Event done;
    bool pending = false;
};

// steering (sfm_batch_set_steering, ABI 14): the command of every row {ux, uy, uz, kind}, an input the ticks only read.  cmd_h
// is its pinned host copy (the kinds of the last sfm_batch_set_steering, the velocities of the last call that sent any):
// sfm_batch_set_commands refills it and sends it with one copy on the stream; SfmBatch::c_done is recorded behind that copy, and
// the next call waits for it before it refills
struct BatchSteerDev {
    bool on = false;           // (not "cmd is allocated": a batch without rows can be steered and has no buffers)
    DevBuf<float4> cmd;        // [N_total] on the device
    PinnedBuf<float4> cmd_h;
    bool pending = false;
};

// observations (sfm_batch_set_observation, ABI 15): the settings and the buffer sfm_batch_observe fills; nothing a tick reads or writes
struct BatchObsDev {
    bool on = false;           // (not "buf is allocated": a batch without rows can be observed and has no buffer)
    int k = 0;
    int frame = 0;
    DevBuf<float> range2;      // [B] sense_range^2
    DevBuf<float> buf;         // [N_total][16 + 4 k]
};

// row episodes (sfm_batch_set_row_episodes): the episodes per ROW -- the settings, the scenes' agent lists, the per-row episode
// state, and the record and mask sfm_batch_end_row_step fills; nothing a tick reads or writes
struct BatchRowEpisodeDev {
    bool on = false;           // (not "record is allocated": a batch without rows can have row episodes and has no buffers)
    DevBuf<BatchEpisodeScene> set;     // [B] (agent = -1: not read)
    DevBuf<int> agent_off;             // [B+1]
    DevBuf<int> agent_rows;            // [agents] row indices inside their scenes, ascending per scene
    DevBuf<int> age;                   // [N_total]
    DevBuf<float> prev;                // [N_total] row_prev_goal_d2
    DevBuf<float> record;              // [N_total][8]
    DevBuf<uint8_t> done;              // [N_total]
};

// episodes (sfm_batch_set_episodes, ABI 16): the settings, the per-scene episode state, and the record and mask sfm_batch_end_step
// fills; nothing a tick reads or writes.  The row episodes are the second half of the same block (`rows`), set and dropped by their
// own call: sfm_batch_upload_state drops both halves with one line, sfm_batch_set_episodes keeps `rows` and
// sfm_batch_set_row_episodes keeps the rest.
struct BatchEpisodeDev {
    bool on = false;
    DevBuf<BatchEpisodeScene> set;     // [B]
    DevBuf<int> age;                   // [B]
    DevBuf<float> prev;                // [B] prev_goal_d2
    DevBuf<float> record;              // [B][8]
    DevBuf<uint8_t> done;              // [B]
    BatchRowEpisodeDev rows;           // the row episodes (sfm_batch_set_row_episodes)
};

// range scans, from the rows (SfmBatch::scan: sfm_batch_set_scan, ABI 17) and from the vehicles (SfmBatch::vscan:
// sfm_batch_set_vehicle_scan): the settings and the buffer sfm_batch_scan / sfm_batch_scan_vehicles fills, one record per item -- a
// row, or a vehicle; nothing a tick reads or writes.  sfm_batch_upload_state drops both; the vehicles' goes with the boxes it refers to too.
struct BatchScanDev {
    bool on = false;           // (not "buf is allocated": a batch without items can be scanned and has no buffer)
    int R = 0;
    int frame = 0;
    float mount_x = 0.f, mount_y = 0.f;    // the vehicles' sensor in the vehicle frame; the rows' rays start at the row: 0
    DevBuf<BatchScanScene> set;    // [B]
    DevBuf<float2> dir;        // [R]
    DevBuf<uint8_t> mask;      // [items]; not allocated: every item is scanned
    DevBuf<float> buf;         // [items][2 R]
};

// restart noise (sfm_batch_set_restart_noise): how a restarted scene may differ from the snapshot, and the two per-scene counters the
// noise kernel keeps; an input the restarts only read, like steering.  The delays refer to the tracks and are dropped with them.
struct BatchNoiseDev {
    bool on = false;
    int tries = 0;
    DevBuf<uint32_t> seed;         // [B]
    DevBuf<uint32_t> resets;       // [B] restarts of the scene since the noise was set
    DevBuf<uint32_t> fallbacks;    // [B] rows of the scene's latest restart that no try could place
    DevBuf<float2> gap2;           // [B] {min_gap^2, point_gap^2}
    DevBuf<float2> pos_box;        // [N_total] {hx, hy}
    DevBuf<float2> goal_box;       // [N_total]; not allocated: the goals stay
    DevBuf<int> delay;             // [M]; not allocated: no traffic timing
    DevBuf<uint32_t> row_resets;   // [N_total] respawns of the row since the noise was set (sfm_batch_respawn_rows_device)
    DevBuf<uint32_t> row_fallbacks;    // [B] chosen rows of the scene's latest respawn that no try could place
    long long max_delay = 0;       // the largest delay: what a restart's int32 fit check adds
};

// observed tracks (sfm_batch_set_observed): the recording, each row's role in it, and the scores the frame kernel accumulates; the
// ticks read and write none of it (they see the state and the commands the frame kernel wrote)
struct BatchReplayDev {
    bool on = false;
    int every = 1;                 // ticks between two observed frames
    DevBuf<float2> obs;            // the frames of every scene, frame-major
    DevBuf<long long> obs_off;     // [B]
    DevBuf<int> frames;            // [B] F_b
    DevBuf<float> inv_h;           // [B] 1 / (every * step_length)
    DevBuf<uint8_t> role;          // [N_total]
    DevBuf<int2> span;             // [N_total] {f0, f1}
    DevBuf<float2> v0;             // [N_total]; NaN: take it from the track
    DevBuf<float4> score;          // [N_total] {samples, sum_d, sum_d2, last_d2}
    DevBuf<float> scene;           // [B][5] what sfm_batch_score left
};

// driven vehicles (sfm_batch_set_vehicle_driving): the command of every vehicle {a, b, c, kind}, an input the ticks only read, and
// its pinned host copy, kept and sent as the steering's (sfm_batch_set_vehicle_commands; SfmBatch::v_done is recorded behind the
// copy).  The headings the driven ticks turn are BatchBoxesDev::rot.  Dropped with the boxes they refer to.
// The autopilot (sfm_batch_set_vehicle_autopilot) is a part of the driving: a controller on the device that writes the commands of
// the autopiloted vehicles in front of every integrating tick.  Its lifetime is the driving's -- whatever drops the driving drops it,
// and so does every sfm_batch_set_vehicle_driving -- which is why it lives inside BatchDriveDev.  The cursors are state: the
// snapshot holds them in s_cursor (valid while SfmBatch::snap is; setting the autopilot drops the snapshot).
struct BatchAutopilotDev {
    bool on = false;
    DevBuf<int> path_off;      // [M+1]
    DevBuf<float2> path;       // [P]
    DevBuf<AutopilotVehicle> set;   // [M]
    DevBuf<int> cursor;        // [M]
    DevBuf<int> s_cursor;      // [M] the snapshot's copy
    DevBuf<float> record;      // [M][8]
    long long launches = 0;    // controller launches since the autopilot was set (sfm_batch_vehicle_autopilot_launches)
};
struct BatchDriveDev {
    bool on = false;           // (not "cmd is allocated": a batch without vehicles can be driven and has no buffers)
    DevBuf<float4> cmd;        // [M] on the device
    PinnedBuf<float4> cmd_h;
    bool pending = false;
    BatchAutopilotDev ap;
};

// vehicle observations (sfm_batch_set_vehicle_observation): the settings and the buffer sfm_batch_observe_vehicles fills; nothing a
// tick reads or writes.  Dropped with the boxes they refer to.
struct BatchVehObsDev {
    bool on = false;           // (not "buf is allocated": a batch without vehicles can be observed and has no buffer)
    int k = 0;
    int frame = 0;
    DevBuf<float> range2;      // [B] sense_range^2
    DevBuf<float2> goal;       // [M]
    DevBuf<uint8_t> mask;      // [M]; not allocated: every vehicle is observed
    DevBuf<float> buf;         // [M][16 + 4 k]
};

// routes (sfm_batch_set_routes): the scenes' walk graphs, each row's graph type and goal, and what the plan kernel leaves per row;
// the ticks read and write none of it (they see the waypoints, modes and queues the plan kernel wrote).  Dropped with the modes.
struct BatchRoutesDev {
    bool on = false;
    int capacity = 0;
    DevBuf<int> node_off;      // [B+1]
    DevBuf<float2> node_xy;    // [V_total]
    DevBuf<int> adj_off;       // [V_total+1]
    DevBuf<uint2> adj;         // [A] {neighbour | type << 16, bits of the weight}
    DevBuf<uint8_t> gtype;     // [N_total]
    DevBuf<float2> goal;       // [N_total]
    DevBuf<int> status;        // [N_total]
    DevBuf<int4> info;         // [N_total] {s, t, L, bits of D[s]}
    std::vector<int32_t> wp_off_h;     // the queue CSR [N_total+1] as sfm_batch_set_routes rebuilt it
    int v_cap = 64, a_cap = 0;         // the plan kernel's LDS: nodes (a multiple of 64) and staged adjacency entries (RouteArgs)
};

struct BatchRecordDev {        // grow-only device buffers of the recording calls
    DevBuf<float4> frames;     // sfm_batch_run_recorded
    DevBuf<float2> zframes;
    DevBuf<float> forces;      // sfm_batch_tick_forces / sfm_batch_run_recorded_forces
};
}  // namespace sfm

struct SfmBatch {
    int device = 0;
    int B = 0;
    hipStream_t stream = nullptr;
    sfm::DevBuf<sfm::BatchParams> d_prm;    // [B]
    sfm::DevBuf<int> d_scene_off;           // [B+1]
    int n_total = 0;
    bool z3 = false;
    bool have_state = false;
    sfm::DevBuf<float4> pk;                 // {x, y, vx, vy}; the five state arrays grow together
    sfm::DevBuf<float2> zv;                 // {z, vz}
    sfm::DevBuf<float4> own;                // {wx, wy, target_speed, radius}
    sfm::DevBuf<uint8_t> crossing;
    sfm::DevBuf<uint32_t> draws;            // waypoint draw counters (zeroed by every upload)
    bool any_rad = false;
    sfm::DevBuf<int> geo_item_off[3];       // [B+1] per kind, zero-filled while the kind has no polylines; they outlive the polylines
    sfm::BatchGeoDev geo[3];                // borders, static, dynamic obstacles
    sfm::DevBuf<sfm::BatchStream> d_streams;    // [B] once sfm_batch_set_waypoint_streams has been called
    sfm::BatchRecordDev rec;
    sfm::BatchBoxesDev boxes;
    sfm::BatchTracksDev tracks;
    sfm::BatchModesDev modes;
    sfm::BatchSpawnDev spawns;
    bool spawn_used = false;                // a schedule was set since the last sfm_batch_set_mode_fsm: a second one is refused
    sfm::BatchSnapDev snap;
    sfm::BatchRestartDev restart;
    sfm::BatchSteerDev steer;
    sfm::BatchObsDev obs;
    sfm::BatchEpisodeDev ep;
    sfm::BatchScanDev scan;
    sfm::BatchNoiseDev noise;
    sfm::BatchGridDev grid;
    sfm::BatchReplayDev replay;
    sfm::BatchDriveDev drive;
    sfm::BatchVehObsDev vobs;
    sfm::BatchScanDev vscan;
    sfm::BatchRoutesDev routes;
    sfm::Event v_done;                     // created by the first sfm_batch_set_vehicle_driving with vehicles; outlives every drop of the driving
    std::vector<int32_t> scene_off_h;      // the scene offsets [B+1] of the last sfm_batch_upload_state, on the host
    std::vector<float> dt_h;                // [B] the scenes' step lengths (sfm_batch_create, sfm_batch_set_params)
    sfm::Event c_done;                      // created by the first sfm_batch_set_steering with rows; outlives every drop of the steering
    std::string err;
};

namespace sfm {

inline int bfail(SfmBatch* b, int code, const std::string& msg) {
    if (b) b->err = msg; else g_create_error = msg;
    return code;
}

inline int bbind(SfmBatch* b) {
    if (!b) return SFM_ERR_INVALID;
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess) { b->err = std::string("hipSetDevice: ") + hipGetErrorString(e); return SFM_ERR_HIP; }
    return SFM_OK;
}

// one message per thing that is missing
constexpr const char* NO_STATE = "sfm_batch_upload_state has not been called";
constexpr const char* NO_SNAPSHOT = "the batch has no snapshot: call sfm_batch_snapshot first (sfm_batch_upload_state and the calls "
                                    "that set vehicles, modes, a spawn schedule or tracks drop it)";
constexpr const char* STEERING_OFF = "steering is off: call sfm_batch_set_steering first (sfm_batch_upload_state drops it)";
constexpr const char* OBSERVATIONS_OFF = "observations are off: call sfm_batch_set_observation first (sfm_batch_upload_state drops them)";
constexpr const char* EPISODES_OFF = "episodes are off: call sfm_batch_set_episodes first (sfm_batch_upload_state drops them)";
constexpr const char* ROW_EPISODES_OFF = "row episodes are off: call sfm_batch_set_row_episodes first (sfm_batch_upload_state drops them)";
constexpr const char* NOISE_OFF = "restart noise is off: call sfm_batch_set_restart_noise first (sfm_batch_upload_state drops it)";
constexpr const char* SCANS_OFF = "scans are off: call sfm_batch_set_scan first (sfm_batch_upload_state drops them)";
constexpr const char* OBSERVED_OFF = "observed tracks are off: call sfm_batch_set_observed first (sfm_batch_upload_state, setting modes or a "
                                     "spawn schedule and switching steering off drop them)";
constexpr const char* DRIVING_OFF = "vehicle driving is off: call sfm_batch_set_vehicle_driving first (sfm_batch_set_dynamic_boxes and "
                                    "sfm_batch_set_dynamic_obstacles drop it)";
constexpr const char* VEHICLE_OBS_OFF = "vehicle observations are off: call sfm_batch_set_vehicle_observation first "
                                        "(sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop them)";
constexpr const char* VEHICLE_SCAN_OFF = "vehicle scans are off: call sfm_batch_set_vehicle_scan first (sfm_batch_upload_state, "
                                         "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop them)";
constexpr const char* VEHICLE_GRID_OFF = "vehicle grids are off: call sfm_batch_set_vehicle_grid first (sfm_batch_upload_state, "
                                         "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop them)";
constexpr const char* VEHICLE_EPISODES_OFF = "vehicle episodes are off: call sfm_batch_set_vehicle_episodes first (sfm_batch_upload_state, "
                                             "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop them)";
constexpr const char* NO_BOXES = "this needs device-side vehicles: call sfm_batch_set_dynamic_boxes first";
constexpr const char* ROUTES_OFF = "routes are off: call sfm_batch_set_routes first (sfm_batch_upload_state and sfm_batch_set_mode_fsm drop them)";
constexpr const char* GRIDS_OFF ="grids are off: call sfm_batch_set_grid first (sfm_batch_upload_state drops them)";

// one kind of the scenes' geometry as the kernels take it, and what the sensors see of the scenes
inline BatchGeo batch_geo(const SfmBatch* b, int k) { return BatchGeo{b->geo_item_off[k], b->geo[k].off, b->geo[k].pts, b->geo[k].ctr}; }
inline BatchSceneView batch_scene_view(const SfmBatch* b) {
    return BatchSceneView{b->d_scene_off, b->pk, b->own, {batch_geo(b, 0), batch_geo(b, 1), batch_geo(b, 2)}};
}

// The restarts (sfm_batch_capi.hip), which sfm_batch_end_step shares.  batch_restart_checks: what every restart refuses before it
// sends or launches anything, in this order -- no snapshot; bad_choice, what the caller found wrong with its choice of scenes (empty:
// nothing); a tracked vehicle of scene k (mask null or mask[k]) whose first tick, moved by *shift, does not fit int32.
int batch_restart_checks(SfmBatch* b, const uint8_t* mask, const std::string& bad_choice, long long* shift);
int batch_restart_device(SfmBatch* b, const uint8_t* d_mask, long long shift);
// The noise launch of a restart (sfm_batch_reset_capi.hip), right behind launch_batch_restart on the batch's stream with the same
// choice of scenes; nothing while the noise is off.  With delays set it marks the host's copy of the tracks' first ticks stale.
int batch_restart_noise(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes);
// The route launch of a restart (sfm_batch_route_capi.hip), behind batch_restart_noise with the same choice of scenes; nothing
// while routes are off.
int batch_plan_routes(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes);
hipError_t launch_batch_plan_routes(const RouteArgs& a, int scenes, hipStream_t st);
size_t route_lds_bytes(int v_cap, int a_cap);
// What sfm_batch_run_observed shares with sfm_batch_run (sfm_batch_capi.hip, where both are described): the check of a tick's
// flags, and the launch of one tick of the whole batch.
int check_batch_flags(SfmBatch* b, uint32_t flags, const char* what);
int batch_launch(SfmBatch* b, uint32_t flags, float4* frame = nullptr, float2* zframe = nullptr, float* force_rec = nullptr,
                 uint32_t force_slots = 0xFFFFFFFFu);
// Observed tracks (sfm_batch_replay_capi.hip): inv_h follows the step lengths (sfm_batch_set_params calls it with the stream
// synchronised and b->dt_h current; it refuses what sfm_batch_set_observed refuses).
int batch_replay_step_lengths(SfmBatch* b, const float* dt);
// The vehicle scan's one launch (sfm_batch_vehicle_scan.hip).
hipError_t launch_batch_vehicle_scan(const VehicleScanArgs& a, int B, hipStream_t st);
// The vehicle grid's one launch (sfm_batch_vehicle_grid.hip).
hipError_t launch_batch_vehicle_grid(const VehicleGridArgs& a, int B, hipStream_t st);
// The autopilot (sfm_batch_autopilot_capi.hip, sfm_batch_autopilot.hip).  batch_autopilot_launch: the controller launch batch_launch
// puts in front of an integrating tick while the autopilot is on.  batch_autopilot_snapshot: the cursors into the snapshot, with
// the other arrays of sfm_batch_snapshot.  batch_autopilot_restart: the cursors of the chosen scenes back, one small launch behind
// the restart's own (and the noise and the routes) with the same choice of scenes; nothing while the autopilot is off.
int batch_autopilot_launch(SfmBatch* b);
int batch_autopilot_snapshot(SfmBatch* b);
int batch_autopilot_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes);
hipError_t launch_batch_vehicle_autopilot(const AutopilotArgs& a, int B, hipStream_t st);
hipError_t launch_batch_autopilot_restart(const int* list, const uint8_t* mask, const int* item_off, int* cursor, const int* s_cursor,
                                          int scenes, hipStream_t st);
constexpr const char* AUTOPILOT_OFF = "the vehicle autopilot is off: call sfm_batch_set_vehicle_autopilot first (sfm_batch_set_vehicle_driving, "
                                      "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop it)";
// Row episodes and row respawns (sfm_batch_row_episode_capi.hip, sfm_batch_row_episode.hip).  batch_row_restart: the row episodes
// of the chosen scenes start over, one small launch behind the restart's own (and the noise, the routes and the autopilot's) with the
// same choice of scenes; nothing while row episodes are off.
int batch_row_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes);
hipError_t launch_batch_row_episode(const RowEpisodeArgs& a, int B, hipStream_t st);
hipError_t launch_batch_row_restart(const int* list, const uint8_t* mask, const int* scene_off, int* row_age, float* row_prev_goal_d2,
                                    int scenes, hipStream_t st);
hipError_t launch_batch_row_respawn(const RowRespawnArgs& a, int B, hipStream_t st);
// Vehicle episodes and vehicle respawns (sfm_batch_vehicle_episode_capi.hip, sfm_batch_vehicle_episode.hip).
// batch_vehicle_episode_restart: the vehicle episodes of the chosen scenes start over, one small launch behind the restart's own (and
// the noise, the routes, the autopilot's and the row episodes') with the same choice of scenes; nothing while vehicle episodes are off.
int batch_vehicle_episode_restart(SfmBatch* b, const int* d_list, const uint8_t* d_mask, int scenes);
hipError_t launch_batch_vehicle_episode(const VehicleEpisodeArgs& a, int B, hipStream_t st);
hipError_t launch_batch_vehicle_episode_restart(const int* list, const uint8_t* mask, const int* item_off, int* age, float* prev_goal_d2,
                                                int scenes, hipStream_t st);
hipError_t launch_batch_vehicle_respawn(const VehicleRespawnArgs& a, int B, hipStream_t st);
// The delays go with the tracks they refer to (the caller synchronised the stream).
inline void drop_noise_delays(SfmBatch* b) { b->noise.delay = {}; b->noise.max_delay = 0; }

}  // namespace sfm
