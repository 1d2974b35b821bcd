// sfm_device.h -- device-side data layout and folded constants shared by the kernels and the C ABI.
// gfx950 (MI355X) only.  See DESIGN.md for the layout rationale.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfm {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;            // 4 waves per workgroup
constexpr int WAVES_PER_BLOCK = BLOCK / WAVE;
constexpr int TILE_J = BLOCK;         // j-records staged per LDS tile (one float4 per thread)
constexpr float TINY = 1e-30f;        // added under every rsq: zero vectors normalise to zero without a guard op
constexpr float COINCIDENT_RINV = 1e14f;  // rsq(d2) above this <=> a coincident (or < 1e-14 m) valid pair

// "Far away": padding rows and despawned pedestrians are ghosts parked near x = FAR_AWAY, FAR_STEP apart (distinct positions), and
// an empty polyline's nearest point is (FAR_AWAY, FAR_AWAY); every interaction with them underflows to exactly 0.  A row counts in
// a tile box while |x| < BOX_LIMIT, in the geometry kernel's tile box and the host's crowd extent while |x|, |y| < NEAR_LIMIT.
constexpr float FAR_AWAY = 3.0e15f;
constexpr float FAR_STEP = 1.0e12f;
constexpr float BOX_LIMIT = 1.0e14f;
constexpr float NEAR_LIMIT = 1.0e12f;

// Moussaid interaction constants, folded on the host in double and rounded once
// (forces.py:85-109 for pedestrians, :241-264 for obstacles).
struct IxConst {
    float lam;    // lambda                                   D = lam*(v_i - v_j) + e
    float eg;     // epsilon*gamma                            theta = angle - eg*|D|          (B = gamma*|D|)
    float c1;     // -log2(e)/gamma                           -d/B * log2(e) = d * (1/|D|) * c1
    float k1;     // -(n_prime*gamma)^2 * log2(e)             -(n' B theta)^2 * log2(e) = (|D| theta)^2 * k1
    float k2;     // -(n*gamma)^2 * log2(e)
    float negA;   // -A
    float thr2;   // perception_threshold^2 (obstacles only)
    float pad;
};

// Counter-based waypoint stream (SFM_TICK_REDRAW_WAYPOINTS): coordinate c of draw `draw` of pedestrian `ped` is
// side * (mix32(seed ^ mix32(2 ped + c + 0x9E3779B9 draw)) >> 8) * 2^-24.  Shared by the handle's kernels and the batch kernel.
__device__ __forceinline__ uint32_t mix32(uint32_t a) {   // lowbias32
    a ^= a >> 16; a *= 0x7FEB352Du; a ^= a >> 15; a *= 0x846CA68Bu; a ^= a >> 16;
    return a;
}
__device__ __forceinline__ float waypoint_coord(uint32_t seed, uint32_t ped, uint32_t draw, uint32_t c, float side) {
    const uint32_t h = mix32(seed ^ mix32(2u * ped + c + 0x9E3779B9u * draw));
    return (float)(h >> 8) * 5.9604644775390625e-08f * side;   // 2^-24
}

// Counter-based restart noise (sfm_batch_set_restart_noise): the random word of component c of try t of restart e of item i -- a row's
// index inside its scene, or a vehicle's -- under the scene's seed is
//     h = mix32(seed ^ mix32(mix32(RESET_SALT ^ (8 i + c)) + 0x9E3779B9 (32 e + t))),        u = (h >> 8) * 2^-24 in [0, 1)
// (c: 0, 1 the position offset; 2, 3 the goal offset, t = 0; 4 a vehicle's delay, t = 0; t < 32).  RESET_SALT and the inner mix keep
// the words apart from waypoint_coord's under an equal seed.  An offset inside a box of half-extent ext is o = fmaf(2 u, ext, -ext)
// in [-ext, ext): 2 u is exact.
constexpr uint32_t RESET_SALT = 0x5BD1E995u;
__device__ __forceinline__ uint32_t reset_word(uint32_t seed, uint32_t i, uint32_t e, uint32_t t, uint32_t c) {
    return mix32(seed ^ mix32(mix32(RESET_SALT ^ (8u * i + c)) + 0x9E3779B9u * (32u * e + t)));
}
__device__ __forceinline__ float reset_offset(uint32_t h, float ext) {
    const float u = (float)(h >> 8) * 5.9604644775390625e-08f;   // 2^-24
    return fmaf(2.0f * u, ext, -ext);
}

struct Geo {                  // CSR polylines / rings
    const int* off;           // [K+1]
    const float2* pts;        // [P] {x, y}
    const float4* ctr;        // [K] borders: {cx, cy, section_length^2, 0}; obstacles: {cx, cy, vx, vy}
    const float4* seg;        // [2K] borders only: {ax, ay, abx, aby}, {1/|ab|^2, max deviation from segment ab, P-1 if the border is a
                              // straight uniformly sampled line (verified on the host) else 0, 0}
    int K;
};

// Device-side pedestrian mode state machine + waypoint queues: the host loop of
// ped_mode_manager.py:30-70, pedestrian_state.py:83-95, pedestrian_simulation.py:63-73 and
// run_simulation.py:118-132 for device-resident runs.  mode == null: off.
constexpr uint8_t MODE_IDLE = 0, MODE_WALKING = 1, MODE_CROSSING = 2, MODE_ROAD_TO_SIDEWALK = 3, MODE_CHECKING = 4,
                  MODE_DESPAWNED = 255;
constexpr uint8_t MODE_UNBORN = 254;   // what sfm_batch_download_modes reports for a row that waits for its spawn time (SFM_MODE_UNBORN)
struct FsmArgs {
    uint8_t* mode;            // PedMode per pedestrian (MODE_DESPAWNED once removed)
    float* target;            // the mode object's target_speed (applied to the state one tick later, like the reference)
    const float* initial_speed;
    const float* crossing_speed;
    const float* safety_margin;
    const float* next_mode_time;
    const int* wp_off;        // [N+1] CSR of the remaining-waypoint lists (waypoint_dict, run_simulation.py:120-126)
    const float2* wp_xy;
    const uint8_t* wp_cross;  // 1: the leg towards this waypoint crosses a road
    int* cursor;              // next unused entry of each list
    float sim_time;
    float veh_ext_x, veh_ext_y;   // extent of the FIRST vehicle (check_traffic.py:35-36 offsets every vehicle by it)
    int despawn_on_arrival;
};

// Device-side vehicles (sfm_set_dynamic_boxes): after a tick's forces are computed the centres move by dt * v and the rings
// are regenerated.  The extra workgroups of the tick's last kernel do it (block index >= block0); M = 0: nothing to do.
struct DynAdvance {
    float4* ctr;              // [M] {cx, cy, vx, vy}
    const int* off;           // [M+1]
    const float2* local;      // [P] ring points in the vehicle frame
    const float2* rot;        // [M] {cos yaw, sin yaw}
    float2* pts;              // [P] ring points in the world frame (what the geometry kernel reads)
    int M;
    float dt;
    int block0;
    float4* ctr_out;          // fused tick with border / obstacle forces: the moved centres and rings go to the other half of a
    float2* pts_out;          // ping-pong (this launch's geometry workgroups still read ctr / pts); null: in place
};

struct TickArgs {
    // packed j-operand state, N_pad records (padding rows are never selected)
    const float4* pk_cur;     // {x, y, vx, vy}
    float4* pk_next;
    const float2* zv_cur;     // {z, vz}, 3-D variant only
    float2* zv_next;
    float4* own;              // {wx, wy, target_speed, radius}
    const float* radius;      // [N_pad] radius stream for the j side (use_ped_radius only)
    uint8_t* crossing;        // border-force mask (rewritten every tick by sfm_mode_kernel when the FSM is on)
    uint32_t* draws;          // waypoint draw counters
    const uint32_t* ids;      // caller's index of the pedestrian in each row (spatial reordering); null = identity
    float* rec;               // optional per-force record, layout [6][3][N]
    float4* host_pk;          // sfm_step_packed: the new rows are ALSO written here -- pinned host memory the device reaches by itself --
    float2* host_zv;          // so the caller's v' needs no copy after the tick (null: off)
    float* geo;               // geometry forces of this tick, layout [geo_slices][6][N_pad]: {fbx,fby,fsx,fsy,fdx,fdy}; null = none
    DynAdvance adv;
    int geo_slices;           // few tiles (small crowds): the polylines of a tile are split over this many workgroups, each
                              // leaving a partial sum; the consumer adds them in slice order
    int N, N_pad, i_begin, i_end;
    uint32_t flags;
    // parameters
    int en_acc, en_ped, en_border, en_static, en_dynamic;
    IxConst ped, stat, dyn;
    float border_a, border_nlb;   // a, -log2(e)/b
    float border_skip;            // distance beyond which a border term is < 2^-40 a (40 ln2 * b), <= 0: never skip
    float inv_tau, dt, max_speed_factor;
    // waypoint stream
    uint32_t seed;
    float world_side, arrive_thr2;
    Geo borders, statics, dynamics;
    // pedestrian-force cutoff at tile granularity (null = off): see tiles_negligible()
    const float4* tile_box;   // [n_t] {xmin, ymin, xmax, ymax} of the real pedestrians of each 64-tile
    const float* tile_vmax;   // [n_t] largest speed in the tile
    float cut_scale;          // gamma * 41 ln 2 (with margin): distance per unit of (lambda*(va+vb)+1)
    float cut_pad;            // 2 * largest radius when use_ped_radius, else 0
    float4* tile_box_out;     // the list cutoff of a whole crowd: the symmetric epilogue writes the boxes / speeds of
    float* tile_vmax_out;     // the NEXT tick's state here (saves the next tick's sfm_tile_bounds_kernel launch)
    FsmArgs fsm;
    // Flat tile-pair list of a whole crowd built by extra workgroups of the geometry launch (block index >= list_block0) instead of
    // a launch of its own: the boxes were left by the previous epilogue, so nothing stands in front of it.  list_work == null: off.
    uint32_t* list_work;
    int* list_count;
    int list_n_t, list_block0;
    uint32_t* list_idx;       // ... and the pool's index table (SymArgs::idx), null: dense slab
    uint32_t list_cap;        // ... and its capacity in row pairs
};

// Symmetric (antisymmetry-exploiting) pedestrian-force path, single shard only.
struct SymArgs {
    float2* slab;        // [n_t][stride]: slab[u][i] = -A-less force on pedestrian i from all pedestrians of tile u
    float* slabz;        // 3-D crowds: its z component, same indexing (null: planar)
    int n_t;             // number of 64-pedestrian tiles
    int stride;          // n_t * 64
    const uint32_t* work;    // cutoff on: compacted list of (bx | shift << 16) tile-pair items, else null
    const int* work_count;
    // vmax (largest speed per tile, this tick's input state) is set whenever the list cutoff is on: the pair kernel then also
    // skips the systolic steps whose 64 pairs are all beyond the reach of the two tiles' speeds, or below the exponent bound
    const float* vmax;
    float cut_scale, cut_pad;
    // two-level list building (large crowds): boxes / largest speeds of runs of `tps` consecutive tiles (= the x-strips of
    // the spatial packing); n_strips = 0: flat
    const float4* sbox;
    const float* svmax;
    int tps, n_strips;
    int t_lo, t_hi;      // tiles of this handle's rows (a shard; whole crowd: 0, n_t).  Pairs with a tile outside are
                         // evaluated one-sided: the other side belongs to another rank, which evaluates it itself
    int zero_count;      // epilogue launch: 1 = leave *work_count at 0 for the next tick's list kernel (saves its memset)
    // Round 4 -- list mode can keep its partial forces in a POOL of row pairs instead of the dense slab (8.6 GB at N = 262 144:
    // O(N^2 / 64); the pool is O(kept tile pairs)).  idx != null: `slab` / `slabz` ARE the pool, [2 * pairs][64]: list item p of this
    // launch owns row pair q = row_base + p -- row 2q the force on the travelling tile's pedestrians (a diagonal item: on tile bx's),
    // row 2q + 1 on the resident tile's (tile bx + half_up's) -- and the list kernels leave q in idx[(bx - t_lo) * n_t + shift], where
    // the epilogue looks it up for the partner tiles its predicate keeps.  An item beyond the list's share of the pool (p >= cap_pairs: a
    // crowd whose tiles overlap keeps everything) adds its sums to spill->ovf in 2^-36 fixed point by integer atomics -- exact,
    // order-independent, hence still deterministic -- and stamps spill->tick.  (Few fields on purpose: every one is two more SGPRs in
    // kernels that sit at the occupancy limit.)
    uint32_t* idx;       // [t_hi - t_lo][n_t]; null: dense slab
    uint32_t row_base;   // first row pair of this launch's list (the split tick's own-own list sits behind the main one)
    uint32_t cap_pairs;  // row pairs a list may use; item positions beyond spill
    struct SpillArgs* spill;
    int tick_serial;     // of the tick being computed (the two halves of a split tick share it)
};

struct SpillArgs {       // (device memory; read only by an item that spills and by the epilogue)
    long long* ovf;      // [4][N_pad]: x, y, z sums in 2^-36 fixed point, count of non-finite sums
    int n_pad;
    int tick;            // serial of the last tick in which an item spilled
};

// Fused tick of a whole planar crowd with the acceleration and pedestrian forces only (sfm_fused_tick_kernel):
// ONE launch per tick inside sfm_run.  Tiles go in groups of two; a workgroup owns one unordered group pair, first integrates its own
// four tiles from the previous launch's partial forces (every workgroup that needs a tile recomputes it -- the same arithmetic on
// the same operands, so all agree bit for bit; the workgroup of the group's diagonal item is the one that stores it), then
// evaluates its tile pairs of the NEW state.  State, waypoints and partial forces ping-pong between launches.
constexpr int FUSED_GEO_SLICES_MAX = 8;  // geometry workgroups per tile of the fused tick (each leaves one partial sum per pedestrian)
// (16-byte aligned: it follows TickArgs in the kernel arguments, and at an 8-byte offset c1's tick measured 8.7 instead of 8.5 us)
struct alignas(16) FusedArgs {
    const float2* slab_prev;  // [n_g][N_pad]: slab[r][i] = -A-less force on pedestrian i from the pedestrians of group r, previous state
    float2* slab_next;        // the same for the state this launch integrates to
    const float* slabz_prev;  // 3-D crowds: the z components, same indexing (null: planar)
    float* slabz_next;
    const float4* own_cur;    // {wx, wy, target_speed, radius} going with pk_cur
    float4* own_next;
    int n_g;                  // groups of two tiles
    int n_t;
    int blocked;              // 1: XCD-aware order of the work items (n_g a multiple of 8)
    const float2* geo_prev;   // [geo_slices][N_pad]: border + obstacle forces on the stored state, one partial sum per slice of the polylines
    float2* geo_next;         // the same for the state this launch integrates to
    int geo_slices;           // <= FUSED_GEO_SLICES_MAX
    int n_geo_wg;             // geometry workgroups in front of the grid = n_t * geo_slices (0: the crowd has no such forces)
    int n_pair_wg;            // pair workgroups behind them
    int mode;                 // 0: the stored state is the state (nothing to integrate, nothing stored but slab_next): the launch in
                              //    front of a run; 1: integrate by one tick, store, then the pairs of the new state
};

// The lean form of the fused tick (lean::sfm_fused_tick_kernel): a whole planar crowd of a multiple of 1024 pedestrians (up to 4096)
// without radii, border / obstacle forces or vehicles.  Only what that path reads: 128 bytes, two scalar loads.
constexpr uint32_t LEAN_EN_ACC = 0x100u, LEAN_EN_PED = 0x200u, LEAN_INTEGRATE = 0x400u;
struct alignas(16) LeanTickArgs {
    const float4* pk_cur;     // {x, y, vx, vy}
    float4* pk_next;
    const float4* own_cur;    // {wx, wy, target_speed, radius} going with pk_cur
    float4* own_next;
    const float2* slab_prev;  // [n_g][N]: FusedArgs::slab_prev
    float2* slab_next;
    uint32_t* draws;          // waypoint draw counters
    const uint32_t* ids;      // caller's index of the pedestrian in each row; null = identity
    IxConst ped;
    float inv_tau, dt, max_speed_factor, arrive_thr2;
    uint32_t seed;
    float world_side;
    uint32_t bits;            // TickArgs::flags (bits 0, 1) | LEAN_EN_ACC | LEAN_EN_PED | LEAN_INTEGRATE (FusedArgs::mode != 0)
    uint32_t pad;
};
static_assert(sizeof(LeanTickArgs) == 128, "the lean fused tick's arguments: two 64-byte scalar loads");

// Batched scenes (sfm_batch.hip, sfm_batch_* in the C ABI): B independent crowds of up to BATCH_MAX_N pedestrians, stepped by ONE
// launch per tick, a workgroup per scene.  State is fp32 SoA over all scenes concatenated (scene b owns rows
// [scene_off[b], scene_off[b+1])); every scene carries its own parameters and geometry.
constexpr int BATCH_MAX_N = 1024;
struct BatchParams {          // one scene's SfmParams, folded on the host like the handle's (fold(), fill_args)
    IxConst ped, stat, dyn;
    float border_a, border_nlb;   // a, -log2(e)/b
    float inv_tau, dt, max_speed_factor;
    int en_acc, en_ped, en_border, en_static, en_dynamic;
    int rad;                  // use_ped_radius
    int pad;
};
struct BatchGeo {             // per-scene CSR polylines: scene b owns polylines [item_off[b], item_off[b+1]) of the concatenated set
    const int* item_off;      // [B+1]
    const int* off;           // [K+1] into pts
    const float2* pts;        // [P]
    const float4* ctr;        // [K] borders: {cx, cy, section_length^2, 0}; obstacles: {cx, cy, vx, vy}
};
struct BatchStream {          // one scene's waypoint stream (sfm_batch_set_waypoint_streams)
    uint32_t seed;
    float world_side;
    float arrive_thr2;        // arrival threshold^2, rounded once from double like the handle's
    float pad;
};
struct BatchModeScene {       // one scene's mode constants (sfm_batch_set_mode_fsm)
    float arrive_thr2;        // arrival threshold^2, rounded once from double like the handle's
    float veh_ext_x, veh_ext_y;   // extent of the scene's FIRST vehicle (check_traffic.py:35-36 offsets every vehicle by it)
    int despawn_on_arrival;
};
struct BatchModes {           // the mode state machine of every row (FsmArgs over the concatenated rows); mode == null: off
    uint8_t* mode;            // [N_total] PedMode (MODE_DESPAWNED once removed)
    float* target;            // [N_total] the mode object's target_speed (applied to the state one tick later, like the reference)
    const float4* speeds;     // [N_total] {initial_speed, crossing_speed, safety_margin, next_mode_time}
    const int* wp_off;        // [N_total+1] CSR of the remaining-waypoint lists
    const float2* wp_xy;
    const uint8_t* wp_cross;  // 1: the leg towards this waypoint crosses a road
    int* cursor;              // [N_total] next unused entry of each list
    const BatchModeScene* scene;  // [B]
    float* sim_time;          // [B] each scene's clock: + its step_length per tick (read before the barrier, written by thread 0 after)
};
constexpr uint8_t BORN_NO = 0, BORN_YES = 1, BORN_AT_SET = 2;   // AT_SET: live since the schedule was set, no tick has run on it yet
struct BatchSpawn {           // the spawn schedule of every row (sfm_batch_set_spawn_schedule); the SPAWN instantiation only
    const float* spawn_time;  // [N_total] on the scene's clock
    const uint8_t* chain;     // [N_total] 1: the row waits for row - 1 of its scene to be born in an earlier tick
    uint8_t* born;            // [N_total] BORN_*; read while staging (before the barrier), set by the lane that owns the row (after it)
    float* birth_time;        // [N_total] the scene's clock before the birth tick; NaN while unborn
    const float4* pk0;        // [N_total] the spawn state {x, y, vx, vy}: what the upload gave the row
    const float2* zv0;        // [N_total] ... and {z, vz} of a 3-D batch
};
struct BatchTracks {          // scripted vehicle tracks (sfm_batch_set_vehicle_tracks); off == null: every vehicle runs free
    const int* off;           // [M+1] CSR of the keyframes of each vehicle; an empty list: that vehicle runs free
    const int* first;         // [M] first_tick: keyframe j of vehicle k is what tick first[k] + j sees
    const float4* key;        // [T] {x, y, vx, vy}
    const float2* rot;        // [T] {cos yaw, sin yaw}
    long long tick;           // the tick whose vehicle state this launch writes (tau + 1): kept by the host, the same for every scene
};
struct BatchArgs {
    const int* scene_off;     // [B+1]
    const BatchParams* prm;   // [B]
    float4* pk;               // {x, y, vx, vy}, updated in place (a scene is read and written by its own workgroup only)
    float2* zv;               // {z, vz}: 3-D batches only
    float4* own;              // {wx, wy, target_speed, radius}; wx / wy rewritten on a redraw
    const uint8_t* crossing;  // border-force mask
    BatchGeo geo[3];          // borders, static obstacles, dynamic obstacles
    uint32_t flags;           // SFM_TICK_INTEGRATE (1), SFM_TICK_REDRAW_WAYPOINTS (2: needs streams)
    const BatchStream* streams;   // [B], null until the caller sets them
    uint32_t* draws;          // [N_total] waypoint draw counters
    float4* frame;            // recording tick: the pre-tick {x, y, vx, vy} of every row go here (frame slot of this tick); null: off
    float2* zframe;           // ... and {z, vz} of a 3-D batch (null: off)
    // device-side vehicles (sfm_batch_set_dynamic_boxes): an integrating tick moves each scene's vehicles from geo[2].ctr / .pts
    // (what this tick's dynamic-force scan reads) into the other half of a ping-pong, which the host swaps in after the launch
    float4* veh_ctr_out;      // [M] {cx, cy, vx, vy} one step of the scene's dt later
    float2* veh_pts_out;      // [P] their rings
    const float2* veh_local;  // [P] ring points in the vehicle frame
    const float2* veh_rot;    // [M] {cos yaw, sin yaw}
    int veh_on;               // 1: boxes are set and the tick integrates; 0: the vehicles stay where they are
    BatchModes fsm;           // the MODES instantiation only (sfm_batch_set_mode_fsm)
    // per-force record (sfm_batch_tick_forces, sfm_batch_run_recorded_forces; EXT and MODES instantiations only): force k (the
    // SFM_FORCE_* index, 5 the total) of row r goes to force_rec[(slot_k * force_n + r) * C + c], C = 2 planar / 3 in 3-D, where
    // slot_k = (force_slots >> 4k) & 15 (filled on the host; 15: not recorded).  One packed word keeps the table in one SGPR.
    // Appended last, so the plain instantiations read every other field where they did.
    float* force_rec;         // null: off
    int force_n;              // N_total
    uint32_t force_slots;
    BatchSpawn spn;           // the SPAWN instantiation only (appended last for the same reason)
    BatchTracks trk;          // vehicle tracks, read in the vehicle prologue only (appended last for the same reason)
    // steering (sfm_batch_set_steering; the STEER instantiations only, appended last for the same reason): the command of every row,
    // {ux, uy, uz, kind} with kind 0 not steered, 1 velocity command, 2 preferred velocity (held as a float; any other value: 0).
    // Read by the lane that owns the row, never written by a tick -- the caller may write it on the batch's stream
    const float4* cmd;        // [N_total]
    // driven vehicles (sfm_batch_set_vehicle_driving; appended last for the same reason): the command of every vehicle {a, b, c, kind}
    // with kind 0 not driven, 1 velocity, 2 unicycle (held as a float; any other value: 0), read in the vehicle prologue by the wave
    // that moves the vehicle and never written by a tick -- the caller may write it on the batch's stream.  veh_head is veh_rot's
    // array, writable: the wave that drives vehicle k reads its heading there and lane 0 stores the new one in place
    const float4* veh_cmd;    // [M]; null: nobody is driven
    float2* veh_head;         // [M] {cos, sin}
};

// Restart of chosen scenes from the batch's snapshot (sfm_batch_restart, sfm_batch_restart_kernel): every array a tick can change,
// the live one and its snapshot copy (s_*) side by side; a null live pointer: the batch has no such array.
struct BatchRestart {
    const int* list;          // [grid] the chosen scenes, ascending; null: workgroup g restarts scene g
    const uint8_t* mask;      // [B] on the device (sfm_batch_restart_device; list is null then): workgroup g leaves at once while
                              // mask[g] == 0; null: every workgroup of the grid restarts its scene
    const int* scene_off;     // [B+1]
    float4* pk;         const float4* s_pk;
    float2* zv;         const float2* s_zv;       // 3-D batches only
    float4* own;        const float4* s_own;
    uint32_t* draws;    const uint32_t* s_draws;
    // device-side vehicles: the half of the ping-pong the next tick reads
    const int* item_off;      // [B+1] geo[2].item_off
    const int* veh_off;       // [M+1] geo[2].off
    float4* ctr;        const float4* s_ctr;
    float2* pts;        const float2* s_pts;
    // modes
    uint8_t* mode;      const uint8_t* s_mode;
    float* target;      const float* s_target;
    int* cursor;        const int* s_cursor;
    float* sim_time;    const float* s_sim_time;  // [B]
    // spawn schedule
    uint8_t* born;      const uint8_t* s_born;
    float* birth_time;  const float* s_birth_time;
    // vehicle tracks: a tracked vehicle's first tick moves with the scene, first = s_first + shift (checked on the host to fit)
    int* first;         const int* s_first;
    const int* trk_off;       // [M+1]
    long long shift;          // tau now - tau of the snapshot
    // episodes (sfm_batch_set_episodes): a restarted scene's episode starts over, age = 0 and prev_goal_d2 = NaN ("none yet"); null
    // while episodes are off
    int* age;                 // [B]
    float* prev_goal_d2;      // [B]
    // the vehicles' headings (state since vehicles can be driven, sfm_batch_set_vehicle_driving); null without device-side vehicles
    float2* rot;        const float2* s_rot;
};

// What the batch's read-only sensors (observations, episode ends, range scans) see of the scenes: the common head of their arguments.
struct BatchSceneView {
    const int* scene_off;     // [B+1]
    const float4* pk;         // {x, y, vx, vy}
    const float4* own;        // {wx, wy, target_speed, radius}: the goal, also of frame 1's heading
    BatchGeo geo[3];          // borders, static obstacles, dynamic obstacles (the half of the ping-pong the next tick reads)
};

// A live row: not a ghost parked far away, not a NaN position (which fails the comparison).
__device__ __forceinline__ bool row_live(float x, float y) { return fabsf(x) < NEAR_LIMIT && fabsf(y) < NEAR_LIMIT; }

// Observations of a batch (sfm_batch_observe, sfm_batch_observe_kernel in sfm_batch_observe.hip): everything but obs is read only.
struct ObserveArgs : BatchSceneView {
    const float* range2;      // [B] sense_range^2, formed in double and rounded once
    float* obs;               // [N_total][16 + 4 k]
    int k;                    // neighbour slots per row, 1 .. SFM_BATCH_MAX_OBS_NEIGHBOURS
    int frame;                // 0 world axes, 1 the row's heading frame
};

// Episode ends of a batch (sfm_batch_end_step, sfm_batch_episode_kernel in sfm_batch_episode.hip): everything above `age` is read only.
struct BatchEpisodeScene {    // one scene's episode settings (sfm_batch_set_episodes)
    int agent;                // the row inside the scene whose fate ends the episode, 0 .. N_b-1 (checked on the host); -1: no agent
    int max_steps;            // 0: no time limit
    float goal_r2, ped_r2, veh_r2;   // radius^2, each formed in double and rounded once like thr2; 0: the test never fires
    int pad[3];
};
struct EpisodeArgs : BatchSceneView {
    const BatchEpisodeScene* set;   // [B]
    int* age;                 // [B] evaluations since the scene's last restart
    float* prev_goal_d2;      // [B] goal_d2 of the evaluation before; NaN: none since the restart
    float* record;            // [B][8]
    uint8_t* done;            // [B]
};

// Range scans of a batch (sfm_batch_scan, sfm_batch_scan_kernel in sfm_batch_scan.hip): everything but out is read only.
constexpr int SCAN_MAX_RAYS = 64;
struct BatchScanScene {       // one scene's scan settings (sfm_batch_set_scan)
    float max_range;          // Rmax, the fp32 value as given
    float ped_r2, point_r2;   // radius^2, each formed in double and rounded once like R2; 0: the kind is never hit
    float pad;
};
struct ScanArgs : BatchSceneView {
    const BatchScanScene* set;    // [B]
    const float2* dir;        // [R] ray directions, used as given
    const uint8_t* mask;      // [N_total] nonzero: the row is scanned; null: every row
    float* out;               // [N_total][2 R]: ranges, then kinds
    int R;                    // rays per row, 1 .. SCAN_MAX_RAYS
    int frame;                // 0 world axes, 1 the row's heading frame
};

// Occupancy grids of a batch (sfm_batch_grid, sfm_batch_grid_kernel in sfm_batch_grid.hip): everything but out is read only.
constexpr int GRID_MAX_G = 32;                         // cells per side
constexpr int GRID_MAX_CELLS = GRID_MAX_G * GRID_MAX_G;
constexpr int GRID_CHANNELS = 6;
struct GridArgs : BatchSceneView {
    const float* cell;        // [B] the cell size, the fp32 value as given
    const int* slot;          // [N_total] the row's slot in out, -1: the row is not gridded; null: every row, slot = row
    float* out;               // [M][6][G][G]
    int G;                    // cells per side, 1 .. GRID_MAX_G
    int frame;                // 0 world axes, 1 the row's heading frame
};
static_assert(sizeof(GridArgs) == 120 + 32, "the grid kernel's arguments follow the view without padding");

// Vehicle observations of a batch (sfm_batch_observe_vehicles, sfm_batch_vehicle_observe_kernel in sfm_batch_vehicle_observe.hip):
// everything but obs is read only.  The vehicles are geo[2]'s items (device-side vehicles: the half the next tick reads).
struct VehicleObserveArgs : BatchSceneView {
    const float2* rot;        // [M] the vehicles' headings {cos, sin}, as the next tick reads them
    const float* range2;      // [B] sense_range^2, formed in double and rounded once
    const float2* goal;       // [M]
    const uint8_t* mask;      // [M] nonzero: the vehicle is observed; null: every vehicle
    float* obs;               // [M][16 + 4 k]
    int k;                    // neighbour slots per vehicle, 1 .. SFM_BATCH_MAX_OBS_NEIGHBOURS
    int frame;                // 0 world axes, 1 the vehicle's heading frame
};
static_assert(sizeof(VehicleObserveArgs) == 120 + 48, "the vehicle observation kernel's arguments follow the view without padding");

// Range scans from the vehicles of a batch (sfm_batch_scan_vehicles, sfm_batch_vehicle_scan_kernel in sfm_batch_vehicle_scan.hip):
// everything but out is read only.  The vehicles are geo[2]'s items; a vehicle's own ring is no candidate of its rays.
constexpr int VEHICLE_SCAN_MAX_RAYS = 256;
struct BatchVehicleScanScene {    // one scene's settings (sfm_batch_set_vehicle_scan): BatchScanScene's
    float max_range;          // Rmax, the fp32 value as given
    float ped_r2, point_r2;   // radius^2, each formed in double and rounded once; 0: the kind is never hit
    float pad;
};
struct VehicleScanArgs : BatchSceneView {
    const float2* rot;        // [M] the vehicles' headings {cos, sin}, as the next tick reads them
    const BatchVehicleScanScene* set;   // [B]
    const float2* dir;        // [R] ray directions, used as given
    const uint8_t* mask;      // [M] nonzero: the vehicle is scanned; null: every vehicle
    float* out;               // [M][2 R]: ranges, then kinds
    int R;                    // rays per vehicle, 1 .. VEHICLE_SCAN_MAX_RAYS
    int frame;                // 0 world axes, 1 the vehicle's heading frame
    float mount_x, mount_y;   // the sensor in the vehicle frame (x forward), one pair for the batch
};
static_assert(sizeof(VehicleScanArgs) == 120 + 56, "the vehicle scan kernel's arguments follow the view without padding");
static_assert(VEHICLE_SCAN_MAX_RAYS <= BLOCK, "the direction table is staged by one pass of the workgroup");

// Restart noise of a batch (sfm_batch_set_restart_noise, sfm_batch_restart_noise_kernel in sfm_batch_reset.hip): launched behind
// sfm_batch_restart_kernel with the same choice of scenes (list / mask as in BatchRestart); the rule is specified in include/sfm_hip.h.
constexpr int RESET_MAX_TRIES = 32;
struct RestartNoiseArgs {
    BatchSceneView v;         // the scene offsets and the geometry; v.pk / v.own are the arrays below
    const int* list;          // [grid] the chosen scenes; null: workgroup g takes scene g
    const uint8_t* mask;      // [B] on the device; null: every workgroup of the grid takes its scene
    float4* pk;               // {x, y, vx, vy}: x, y of the placed rows are rewritten
    float4* own;              // {wx, wy, ..}: wx, wy of the live rows are rewritten while goal_box is set
    const uint32_t* seed;     // [B]
    uint32_t* resets;         // [B] e: restarts of the scene since the noise was set
    uint32_t* fallbacks;      // [B] rows of the scene's latest restart that no try could place
    const float2* pos_box;    // [N_total] {hx, hy}
    const float2* goal_box;   // [N_total]; null: the goals stay
    const float2* gap2;       // [B] {min_gap^2, point_gap^2}, each formed in double and rounded once
    int tries;                // 1 .. RESET_MAX_TRIES
    // traffic timing; delay == null: off
    const int* delay;         // [M] per vehicle, >= 0
    int* first;               // [M] the tracks' first ticks (BatchTracks::first, writable)
    BatchTracks trk;          // .tick: the tick the vehicles are placed for (tau: what the next tick reads)
    const float2* veh_local;  // [P] ring points in the vehicle frame
    float4* veh_ctr;          // [M] the half of the ping-pong the next tick reads
    float2* veh_pts;          // [P]
    const float4* veh_cmd;    // [M] the driving commands (BatchArgs::veh_cmd); a driven vehicle stays at its snapshot pose.  null: none
};

// Observed tracks of a batch (sfm_batch_set_observed, sfm_batch_replay_kernel and sfm_batch_score_kernel in sfm_batch_replay.hip;
// the rules are specified in include/sfm_hip.h).  The frame kernel writes pk, cmd and score of the rows of role 1 and 2 only.
constexpr uint8_t ROLE_NONE = 0, ROLE_REPLAYED = 1, ROLE_SCORED = 2;
constexpr int SCENE_SCORE_WIDTH = 5;  // {rows, samples, sum_d, sum_d2, sum_final_d}
struct ReplayArgs {
    const int* scene_off;     // [B+1]
    float4* pk;               // {x, y, vx, vy}
    float4* cmd;              // {ux, uy, uz, kind}: the steering command buffer
    float4* score;            // [N_total] {samples, sum_d, sum_d2, last_d2}
    const float2* obs;        // the track frames of every scene, frame-major: obs[obs_off[b] + f * n_b + i]; NaN: not seen
    const long long* obs_off; // [B]
    const int* frames;        // [B] F_b
    const float* inv_h;       // [B] 1 / (every * step_length), formed in double and rounded once
    const uint8_t* role;      // [N_total] ROLE_*
    const int2* span;         // [N_total] {f0, f1}: first and last observed frame; f0 > f1: never seen
    const float2* v0;         // [N_total] initial velocity; NaN: take it from the track
    int f;                    // the frame this launch places
};
struct ScoreArgs {
    const int* scene_off;     // [B+1]
    const float4* score;      // [N_total]
    float* out;               // [B][SCENE_SCORE_WIDTH]
};

static_assert(sizeof(BatchSceneView) == 120 && sizeof(ObserveArgs) == 120 + 24 && sizeof(EpisodeArgs) == 120 + 40 && sizeof(ScanArgs) == 120 + 40,
              "the kernels' argument layout: the view is the head of each sensor's arguments, which follow it without padding");

// Block-major packing for sharded runs (sfm_set_partition, sfm_reorder.hip): the row order is cut into gx columns by x, each
// column into gy blocks by y -- block b = column * gy + position holds rows [bound[b], bound[b+1]) -- and every block is
// strip-packed on its own, so a rank's contiguous row range is a compact rectangle of the map instead of a slab across it.
constexpr int MAX_BLOCKS = 16;
struct BlockPlan {
    int n_blocks, gy;                 // n_blocks = gx * gy (1: plain strip packing of the whole crowd)
    int bound[MAX_BLOCKS + 1];        // row bounds of the blocks, multiples of 64, bound[n_blocks] >= N
    int strip_rows[MAX_BLOCKS];       // rows per strip inside each block
};

}  // namespace sfm
