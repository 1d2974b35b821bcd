// sfm_batch.hip -- batched scenes for gfx950 (MI355X): B independent crowds of 0 .. 1024 pedestrians, ONE launch per tick.
//
// Social-force models are run in bulk as many small scenes (scenario sampling, RL environments in lock-step, calibration sweeps over
// A / lambda / gamma / tau ...).  A handle per scene costs a launch per scene per tick and leaves most of the GPU idle; here a
// workgroup owns one scene and the whole batch is one grid.  Per scene, the handle's tick (acceleration_force, capped_velocity and
// next_waypoint of sfm_interaction.h, IEEE forms):
//   F_i = acceleration + pedestrian (Moussaid, N_b x N_b) + border + static + dynamic obstacle forces (each scene's own switches,
//   parameter tables and polylines),  v' = cap(v + dt F, max_speed_factor v0),  with SFM_TICK_INTEGRATE also x' = x + dt v'.
//
// Shape (workgroup b, 4 waves):
//   1. the scene's pedestrians are staged in LDS once (x, y, vx, vy [, z, vz], radius: <= 28 KiB);
//   2. pair sums: a lane owns row i and sums over ALL j of its j-slice in ascending order (the full N_b^2 terms -- at this size the
//      antisymmetric F_ji = -F_ij trick does not pay for its reduction).  N_b <= 64: the four waves take a quarter of j each, N_b <= 128:
//      a half; their partial sums meet in LDS in slice order.  Larger scenes: one slice, rows dealt to the 256 lanes in passes;
//   3. geometry: each lane scans its scene's polylines (lane_nearest, a polyline at a time for the whole wave);
//   4. epilogue: the forces in the reference's dict order, cap, integrate, store; with SFM_TICK_REDRAW_WAYPOINTS the arrival test on the
//      pre-move position and the next waypoint of the scene's counter-based stream (taking effect next tick).
// A recording tick (frame != null) also stores the pre-tick state of every row while the scene is staged (frame f of a recorded run
// is the state before tick f*stride).  Redraw and recording are the EXT instantiations; the plain tick is compiled without them.
// A force-recording tick (force_rec != null, EXT or MODES) also stores each selected force of a row, and the total F, from the
// epilogue's registers in the lane that owns the row.
// Device-side vehicles (sfm_batch_set_dynamic_boxes, a.veh_on): in the prologue, before the barrier, the waves of workgroup b move
// scene b's vehicles k0 + wave, k0 + wave + 4, ... by its dt (advance_vehicle, the handle's one vehicle step) from geo[2] -- what
// this tick's dynamic-force scan reads -- into the other half of a ping-pong (a.veh_*_out), which the host swaps in after the
// launch.  With vehicle tracks set (sfm_batch_set_vehicle_tracks, a.trk.off) a vehicle that has keyframes is not moved but
// teleported: the same waves write the keyframe the NEXT tick sees (or the absent state) from the read-only track arrays.
// With driving on (sfm_batch_set_vehicle_driving, a.veh_cmd) a vehicle whose command has kind 1 or 2 is moved by drive_vehicle instead,
// keyframes or not: centre, velocity and ring go to the other half like everyone's, and the heading -- state from then on -- is
// rewritten IN PLACE (a.veh_head) by lane 0 of the one wave that reads it in this launch.
// No launch reads what another wave of it writes, so no barrier is added: the one barrier below is followed by
// `if (slice != 0) return;`, and a later barrier would wait on waves that have left.
// Pedestrian modes (sfm_batch_set_mode_fsm, the MODES instantiation): the lane that owns a row runs the handle's sfm_mode_kernel for it
// after the barrier (target of this tick, idle wake-up on the scene's clock, gap acceptance against the scene's geo[2] items), the
// border mask follows the mode, and after the step an arrival pops the row's queue or despawns it (parked far away, keyed by its index
// inside the scene).  The scene's clock a.fsm.sim_time[b] is read before the barrier and advanced by thread 0 after it.
// Spawn schedule (sfm_batch_set_spawn_schedule, the SPAWN instantiation of MODES): a row may wait off the map as a ghost (parked like a
// despawned row, a.spn.born = 0) until the scene's clock reaches its spawn time.  The thread that stages row t decides its birth from
// values read before the barrier (born[t], born[t - 1] of a chained row, spawn_time[t], now), stages a newborn at its spawn state --
// so every row's pair sum of this tick sees it -- and leaves the decision in LDS (sh.st); the lane that owns the row reads it there
// after the barrier, starts the mode machine from the row's initial mode and stores born / birth_time.  born[] is never read after
// the barrier, so a chained row cannot see its predecessor's store of the same tick: one release per chain per tick.  A row that was
// due when the schedule was set never left the live state (born = BORN_AT_SET); the first tick after that is its birth tick as far
// as the row chained to it is concerned (the reference's spawn manager would release it at the top of that tick), and sets BORN_YES.
// Steered rows (sfm_batch_set_steering, the STEER instantiations of EXT, MODES and MODES + SPAWN): the lane that owns a row loads its
// command {ux, uy, uz, kind} from a.cmd in the epilogue -- an input like the parameters, never written here.  Kind 1: v' is the
// command bit for bit; kind 2: the command stands where v0 e_wp stands in the acceleration term; both by select, so any other row
// computes what it computes without STEER.  Everyone else sees the row as staged: nothing is ordered inside a launch.
// Planar bodies (moussaid_planar / moussaid_spatial) with the exact body (moussaid<.., EXACT>) recomputing a slice whose sum came out
// NaN (coincident pair, or two pedestrians above one another in 3-D), as the handle's kernels do.
// Determinism: no atomics, every order is a function of the scene alone (N_b, its rows, its polylines) -- a scene's result is
// bitwise the same whatever else is in the batch and wherever it sits.  The state is updated in place: a scene's rows are read
// (into LDS) and written by its own workgroup only, and every read comes before the barrier that precedes the first store; a row's
// waypoint and draw counter are read and rewritten by the lane that owns the row.
#include "sfm_device.h"
#include "sfm_interaction.h"

namespace sfm {

template <bool SPAWN>
struct BatchSpawnShared {};                        // (empty base: the other instantiations keep their LDS size)
template <>
struct BatchSpawnShared<true> {
    uint8_t st[BATCH_MAX_N];                       // SPAWN_GHOST / _LIVE / _NEWBORN / _SETTLED, decided while staging
};
constexpr uint8_t SPAWN_GHOST = 0, SPAWN_LIVE = 1, SPAWN_NEWBORN = 2, SPAWN_SETTLED = 3;   // (SETTLED: live, born[] still BORN_AT_SET)

template <bool Z3, bool SPAWN = false>
struct BatchShared : BatchSpawnShared<SPAWN> {
    float4 pk[BATCH_MAX_N];                        // {x, y, vx, vy}
    float2 zv[Z3 ? BATCH_MAX_N : 1];               // {z, vz}
    float r[BATCH_MAX_N];                          // radius
    float part[BLOCK][3];                          // j-slice partial sums, slot = slice * rows + row
    __attribute__((aligned(16))) float2 row[WAVES_PER_BLOCK][WAVE];   // lane_nearest's per-wave rows
};

// Pedestrian force on row i from rows [j0, j1) of the scene, without the factor -A; j == i is dropped (stateutils.py:41-49)
template <bool Z3, bool RAD, typename SH>
__device__ __forceinline__ void batch_pair_sum(const IxConst& c, const SH& sh, int i, int j0, int j1,
                                               float& gx, float& gy, float& gz) {
    const float4 si = sh.pk[i];
    const float zi = Z3 ? sh.zv[i].x : 0.0f, vzi = Z3 ? sh.zv[i].y : 0.0f;
    const float ri = RAD ? sh.r[i] : 0.0f;
    gx = 0.0f; gy = 0.0f; gz = 0.0f;
    for (int j = j0; j < j1; ++j) {                                    // wave-uniform: the LDS reads are broadcasts
        const float4 pj = sh.pk[j];
        const float dx = pj.x - si.x, dy = pj.y - si.y;
        const float rsum = RAD ? ri + sh.r[j] : 0.0f;
        float cx, cy, cz = 0.0f;
        if (Z3) {
            const float2 zj = sh.zv[j];
            const float dz = zj.x - zi;
            moussaid_spatial<RAD, false>(c, dx, dy, dz, fmaf(dx, dx, fmaf(dy, dy, dz * dz)), c.lam * (si.z - pj.z), c.lam * (si.w - pj.w),
                                         c.lam * (vzi - zj.y), rsum, cx, cy, cz);
        } else {
            moussaid_planar<RAD, false>(c, dx, dy, fmaf(dx, dx, dy * dy), c.lam * (si.z - pj.z), c.lam * (si.w - pj.w), rsum, cx, cy);
        }
        const bool valid = j != i;                                     // select, so the diagonal's NaN never leaks
        gx += valid ? cx : 0.0f;
        gy += valid ? cy : 0.0f;
        if (Z3) gz += valid ? cz : 0.0f;
    }
    // a NaN sum: a coincident pair (or, in 3-D, a pair above one another) needs the reference's zero-vector conventions -> this
    // lane redoes its slice with the exact body (rare; the lane's own decision, so the result still depends on the scene only)
    if (__builtin_isnan(gx) || __builtin_isnan(gy) || (Z3 && __builtin_isnan(gz))) {
        gx = 0.0f; gy = 0.0f; gz = 0.0f;
        for (int j = j0; j < j1; ++j) {
            const float4 pj = sh.pk[j];
            const float zj = Z3 ? sh.zv[j].x : 0.0f, vzj = Z3 ? sh.zv[j].y : 0.0f;
            float cx = 0.0f, cy = 0.0f, cz = 0.0f, rinv;
            moussaid<Z3, RAD, true>(c, pj.x - si.x, pj.y - si.y, zj - zi, si.z - pj.z, si.w - pj.w, vzi - vzj,
                                    RAD ? ri + sh.r[j] : 0.0f, cx, cy, cz, rinv);
            const bool valid = j != i;
            gx += valid ? cx : 0.0f;
            gy += valid ? cy : 0.0f;
            if (Z3) gz += valid ? cz : 0.0f;
        }
    }
}

// Border / static / dynamic obstacle forces on one pedestrian per lane from the scene's polylines, in polyline order per kind:
// BorderForce._get_force (forces.py:145-167) and ObstacleForce._get_force (forces.py:217-275) with the strict-< culls of the reference
// (|x - centre| < section_length, :149-150; < perception_threshold, :222-223) and np.argmin's first-minimum rule (lane_nearest).
template <bool RAD>
__device__ __forceinline__ void batch_geometry(const BatchArgs& a, const BatchParams& p, int b, float x, float y, float vx, float vy,
                                               float r, bool live, bool walk, float2* row, int lane, float (&f)[6]) {
#pragma unroll 1
    for (int kind = 0; kind < 3; ++kind) {
        const bool on = kind == 0 ? p.en_border : kind == 1 ? p.en_static : p.en_dynamic;
        if (!on) continue;                                             // uniform
        const BatchGeo g = kind == 0 ? a.geo[0] : kind == 1 ? a.geo[1] : a.geo[2];    // (selects: no indexed copy in scratch)
        const int k0 = g.item_off[b], k1 = g.item_off[b + 1];
        const float thr2 = kind == 1 ? p.stat.thr2 : p.dyn.thr2;
#pragma unroll 1
        for (int k = k0; k < k1; ++k) {
            const float4 c = g.ctr[k];
            const int o0 = g.off[k], o1 = g.off[k + 1];
            const float cdx = x - c.x, cdy = y - c.y;
            const float d2c = fmaf(cdx, cdx, cdy * cdy);
            const bool keep = kind == 0 ? (walk && d2c < c.z) : (live && d2c < thr2);
            if (!__any(keep)) continue;                                // no lane of the wave keeps it
            const float2 sp = lane_nearest(g.pts, o0, o1, x, y, row, lane);
            if (!keep) continue;
            if (kind == 0) {
                const float ddx = x - sp.x, ddy = y - sp.y;
                const float d = sqrtf(fmaf(ddx, ddx, ddy * ddy));
                const float inv = (d == 0.0f) ? 1.0f : 1.0f / d;               // stateutils.normalize zero guard
                const float dist = RAD ? d - r : d;                             // forces.py:160-161
                const float mag = p.border_a * ex2(dist * p.border_nlb);        // a*exp(-dist/b), :163
                f[0] = fmaf(ddx * inv, mag, f[0]);
                f[1] = fmaf(ddy * inv, mag, f[1]);
            } else {
                const bool moving = kind == 2;                                  // static obstacles: v = 0 (:212-213)
                const float ovx = moving ? c.z : 0.0f, ovy = moving ? c.w : 0.0f;
                float gx = 0.f, gy = 0.f, gz = 0.f, unused;
                moussaid<false, RAD, true>(moving ? p.dyn : p.stat, sp.x - x, sp.y - y, 0.0f, vx - ovx, vy - ovy, 0.0f, r,
                                           gx, gy, gz, unused);
                if (moving) { f[4] += gx; f[5] += gy; } else { f[2] += gx; f[3] += gy; }
            }
        }
    }
}

// acceleration_force<true, false> of a row that may be steered: for a kind 2 row (k2) the command u stands where v0 e_wp stands,
// F_acc = (u - v) / tau in every component.  The unsteered term is acceleration_force's own; the steered one is written as
// fma(-v, 1/tau, u * 1/tau), an expression of another shape, so that the compiler cannot merge the two sides of the select into
// shared operations and fuse them differently: a row that is not steered gets, bit for bit, what it gets without STEER.
template <bool Z3, class P>
__device__ __forceinline__ void steered_acceleration_force(const P& p, float wx, float wy, float x, float y, float vx, float vy, float vz,
                                                           float ts, bool k2, const float4& u, float& fax, float& fay, float& faz) {
    acceleration_force<true, false>(p, wx, wy, x, y, vx, vy, vz, ts, fax, fay, faz);
    fax = k2 ? __builtin_fmaf(-vx, p.inv_tau, u.x * p.inv_tau) : fax;
    fay = k2 ? __builtin_fmaf(-vy, p.inv_tau, u.y * p.inv_tau) : fay;
    if (Z3) faz = k2 ? __builtin_fmaf(-vz, p.inv_tau, u.z * p.inv_tau) : faz;   // (planar: uz = 0 is the term it has)
}

template <bool Z3, bool RAD, bool EXT, bool MODES, bool SPAWN, bool STEER>
__device__ __forceinline__ void batch_scene(const BatchArgs& a, const BatchParams& p, BatchShared<Z3, SPAWN>& sh, int b, int s0, int n,
                                            float now) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = uniform(tid >> 6);
    // j split over the waves of a small scene: S slices of R rows each (R a multiple of 64, so a wave's slice is uniform)
    const int S = n <= WAVE ? 4 : n <= 2 * WAVE ? 2 : 1;
    const int R = BLOCK / S;
    const int slice = uniform(tid / R), rloc = tid - slice * R;
    const int chunk = (n + S - 1) / S;
    const int j0 = min(n, slice * chunk), j1 = min(n, j0 + chunk);
#pragma unroll 1
    for (int base = 0; base < n; base += R) {                          // S > 1: one pass
        const int i = base + rloc;
        const bool live = i < n;
        const int ii = live ? i : n - 1;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (p.en_ped) batch_pair_sum<Z3, RAD>(p.ped, sh, ii, j0, j1, gx, gy, gz);
        if (S > 1) {                                                   // partial sums meet in LDS, slice order
            sh.part[tid][0] = gx; sh.part[tid][1] = gy; sh.part[tid][2] = gz;
            __syncthreads();
            if (slice != 0) return;                                    // (the last barrier of this workgroup)
            gx = sh.part[rloc][0]; gy = sh.part[rloc][1]; gz = sh.part[rloc][2];
            for (int s = 1; s < S; ++s) {
                gx += sh.part[s * R + rloc][0];
                gy += sh.part[s * R + rloc][1];
                gz += sh.part[s * R + rloc][2];
            }
        }
        float fpx = 0.f, fpy = 0.f, fpz = 0.f;
        if (p.en_ped) { fpx = p.ped.negA * gx; fpy = p.ped.negA * gy; fpz = Z3 ? p.ped.negA * gz : 0.f; }

        const float4 s = sh.pk[ii];
        const float x = s.x, y = s.y, vx = s.z, vy = s.w;
        const float z = Z3 ? sh.zv[ii].x : 0.0f, vz = Z3 ? sh.zv[ii].y : 0.0f;
        const float r = RAD ? sh.r[ii] : 0.0f;
        bool walk = live && !(a.crossing && a.crossing[s0 + ii]);         // forces.py:140-141,176-177
        // MODES: the batch form of sfm_mode_kernel -- apply_current_mode (this tick's target speed is the mode object's target BEFORE
        // its tick, pedestrian_state.py:94-95), the idle wake-up (ped_mode_manager.py:30-35) and gap acceptance against the scene's
        // own vehicles as this tick sees them (pedestrian_simulation.py:63-73); the border mask follows the new mode
        uint8_t m = MODE_DESPAWNED;
        float tgt = 0.0f;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        uint8_t born = SPAWN_LIVE;                                     // SPAWN: the staging thread's decision for this row
        if constexpr (SPAWN) born = sh.st[ii];
        if (MODES) {
            if (live) {
                // (an unborn row keeps its initial mode and target in a.fsm until its birth tick; here it is a ghost like a despawned row)
                m = SPAWN && born == SPAWN_GHOST ? MODE_DESPAWNED : a.fsm.mode[s0 + i];
                o = a.own[s0 + i];
                if (m != MODE_DESPAWNED) {
                    tgt = a.fsm.target[s0 + i];
                    const float4 sp = a.fsm.speeds[s0 + i];                  // {initial, crossing, margin, next_mode_time}
                    o.z = tgt;
                    if (m == MODE_IDLE && sp.w <= now) { m = MODE_WALKING; tgt = sp.x; }
                    if (m == MODE_CHECKING) {
                        const int k0 = a.geo[2].item_off[b], k1 = a.geo[2].item_off[b + 1];
                        const BatchModeScene ms = a.fsm.scene[b];
                        if (k0 == k1 || gap_accepted(a.geo[2].ctr, k0, k1, ms.veh_ext_x, ms.veh_ext_y, make_float2(x, y),
                                                     make_float2(o.x, o.y), sp.y, sp.z)) {
                            m = MODE_CROSSING;
                            tgt = sp.y;
                        }
                    }
                } else {
                    o.z = 0.0f;
                }
            }
            walk = live && m != MODE_CROSSING && m != MODE_ROAD_TO_SIDEWALK && m != MODE_DESPAWNED;   // forces.py:176-177
        }
        float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        batch_geometry<RAD>(a, p, b, x, y, vx, vy, r, live, walk, sh.row[wave], lane, f);
        const float fbx = f[0], fby = f[1];
        const float fsx = p.stat.negA * f[2], fsy = p.stat.negA * f[3];
        const float fdx = p.dyn.negA * f[4], fdy = p.dyn.negA * f[5];
        if (!live) continue;

        if (!MODES) o = a.own[s0 + i];
        const float ts = o.z;
        // STEER: the row's command {ux, uy, uz, kind}, one 16-byte load by the lane that owns the row; the kernel never writes it.
        // kind 1: v' is the command; kind 2: the command replaces v0 e_wp in the acceleration term; anything else: not steered.  A
        // ghost (despawned earlier, or unborn) ignores its command.  Selects, so a row with kind 0 runs the arithmetic it always ran
        bool k1 = false, k2 = false;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (STEER) {
            u = a.cmd[s0 + i];
            const bool there = !MODES || m != MODE_DESPAWNED;
            k1 = there && u.w == 1.0f;
            k2 = there && u.w == 2.0f;
            if (!Z3) u.z = 0.0f;                                       // a planar batch ignores uz
        }
        float fax = 0.f, fay = 0.f, faz = 0.f;
        // (the z lane even in a planar scene, where vz = 0 makes it exactly +0: <Z3, false> is shorter but measured 4% slower at 8192
        //  scenes, profiles/r07_batch_planar_z_lane.txt)
        if (p.en_acc) {
            if constexpr (STEER) steered_acceleration_force<Z3>(p, o.x, o.y, x, y, vx, vy, vz, ts, k2, u, fax, fay, faz);
            else acceleration_force<true, false>(p, o.x, o.y, x, y, vx, vy, vz, ts, fax, fay, faz);
        }
        // sum in the dict order acceleration, pedestrian, border, static, dynamic (pedestrian_simulation.py:37-48,81), as sfm_tick_kernel
        const float Fx = (((fax + fpx) + fbx) + fsx) + fdx;
        const float Fy = (((fay + fpy) + fby) + fsy) + fdy;
        const float Fz = faz + fpz;
        // force record: what get_force returns, from the values above (the total is F exactly); the lane owns the row, so a
        // planar wave stores 64 consecutive float2 per force -- no barrier, no atomics, nothing read back in this launch
        if ((EXT || MODES) && a.force_rec) {
            const float vx6[6] = {fax, fpx, fbx, fsx, fdx, Fx}, vy6[6] = {fay, fpy, fby, fsy, fdy, Fy};
            const float vz6[6] = {faz, fpz, 0.0f, 0.0f, 0.0f, Fz};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const uint32_t sl = (a.force_slots >> (4 * k)) & 15u;  // uniform
                if (sl == 15u) continue;
                const size_t row = (size_t)sl * (size_t)a.force_n + (size_t)(s0 + i);
                if (Z3) {
                    float* q = a.force_rec + 3 * row;
                    q[0] = vx6[k]; q[1] = vy6[k]; q[2] = vz6[k];
                } else {
                    reinterpret_cast<float2*>(a.force_rec)[row] = make_float2(vx6[k], vy6[k]);
                }
            }
        }
        float nvx, nvy, nvz;
        capped_velocity<true, false>(p, vx, vy, vz, Fx, Fy, Fz, ts, nvx, nvy, nvz);
        // arrival on the pre-move position against this tick's waypoint -> next draw of the scene's stream, keyed by the
        // scene-local index (pedestrian_simulation.py:92-95, run_simulation.py:118-126; the handle's fused tick)
        if (EXT && (a.flags & 2u)) {
            const BatchStream st = a.streams[b];
            const float ax_ = o.x - x, ay_ = o.y - y;
            if (fmaf(ax_, ax_, ay_ * ay_) < st.arrive_thr2) {
                const uint32_t nd = a.draws[s0 + i] + 1u;
                const float2 w = next_waypoint(st.seed, (uint32_t)i, nd, st.world_side);
                a.own[s0 + i] = make_float4(w.x, w.y, o.z, o.w);
                a.draws[s0 + i] = nd;
            }
        }
        // MODES: arrival on the pre-move position against this tick's waypoint pops the row's queue and requests the new leg's mode,
        // or despawns the row once its queue is exhausted (run_simulation.py:118-132, pedestrian_state.py:83-92; fsm_arrived)
        bool park = false;
        if (MODES) {
            const BatchModeScene ms = a.fsm.scene[b];
            const float ax_ = o.x - x, ay_ = o.y - y;
            park = m == MODE_DESPAWNED;                                 // despawned earlier: stays parked
            if (!park && fmaf(ax_, ax_, ay_ * ay_) < ms.arrive_thr2) {
                const int e0 = a.fsm.wp_off[s0 + i], c = a.fsm.cursor[s0 + i];
                if (c < a.fsm.wp_off[s0 + i + 1] - e0) {
                    const int e = e0 + c;
                    const float2 w = a.fsm.wp_xy[e];
                    const float4 sp = a.fsm.speeds[s0 + i];
                    o.x = w.x; o.y = w.y;
                    a.fsm.cursor[s0 + i] = c + 1;
                    m = fsm_request(m, a.fsm.wp_cross[e] ? MODE_CROSSING : MODE_WALKING);
                    tgt = fsm_enter(m, tgt, sp.x, sp.y);
                } else if (ms.despawn_on_arrival) {
                    park = true;
                    m = MODE_DESPAWNED;
                    tgt = 0.0f;
                }
            }
            if (!SPAWN || born != SPAWN_GHOST) {                       // (an unborn row's waypoint, mode and target wait as they were set)
                a.own[s0 + i] = o;                                     // this tick's target in .z (and the popped waypoint)
                a.fsm.mode[s0 + i] = m;
                a.fsm.target[s0 + i] = tgt;
            }
            if (SPAWN && born == SPAWN_NEWBORN) {                      // born in this tick, on the clock the tick started with
                a.spn.born[s0 + i] = BORN_YES;
                a.spn.birth_time[s0 + i] = now;
            }
            if (SPAWN && born == SPAWN_SETTLED) a.spn.born[s0 + i] = BORN_YES;
        }
        if constexpr (STEER) {                                         // kind 1: the command bit for bit, no cap; it moves below as
            const bool go = k1 && !park;                               // every row does.  A row that parks in this tick is not
            nvx = go ? u.x : nvx;                                      // steered: parking overrides the command altogether, so its
            nvy = go ? u.y : nvy;                                      // z (all that is left of the move) is the unsteered row's
            nvz = go ? u.z : nvz;
        }
        float nx = x, ny = y, nz = z;
        if (a.flags & 1u) { nx = fmaf(p.dt, nvx, x); ny = fmaf(p.dt, nvy, y); nz = fmaf(p.dt, nvz, z); }
        if (MODES && park) {                                           // destroy_pedestrian: parked as a ghost, keyed by the
            const float2 pp = park_position((uint32_t)i);                // scene-local index (a one-scene batch parks where a handle does)
            nx = pp.x; ny = pp.y; nvx = 0.f; nvy = 0.f; nvz = 0.f;
        }
        a.pk[s0 + i] = make_float4(nx, ny, nvx, nvy);
        if (Z3) a.zv[s0 + i] = make_float2(nz, nvz);
    }
}

template <bool Z3, bool EXT, bool MODES, bool SPAWN = false, bool STEER = false>
__global__ __launch_bounds__(BLOCK) void sfm_batch_tick_kernel(const BatchArgs a) {
    static_assert(!SPAWN || MODES, "a spawn schedule runs on the mode state machine");
    static_assert(!STEER || EXT || MODES, "steered rows ride the EXT and MODES forms");
    __shared__ BatchShared<Z3, SPAWN> sh;
    const int b = blockIdx.x;
    if (a.veh_on) {                                                     // uniform; also a scene without pedestrians: every vehicle
        const int k0 = a.geo[2].item_off[b], k1 = a.geo[2].item_off[b + 1];   // must reach the other half
        const int wave = uniform((int)threadIdx.x >> 6);
        // (geo[2] is only read here: the moved centres and rings go to veh_*_out, which nothing in this launch reads)
        const DynAdvance d{const_cast<float4*>(a.geo[2].ctr), a.geo[2].off, a.veh_local, a.veh_rot, const_cast<float2*>(a.geo[2].pts),
                           0, a.prm[b].dt, 0, a.veh_ctr_out, a.veh_pts_out};
        if (a.veh_cmd) {                                                // uniform: driving is on -- a vehicle whose command has kind 1 or 2
            const int lane = threadIdx.x & (WAVE - 1);                    // is moved by it (keyframes or not), the others as below
            for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {
                const float4 u = a.veh_cmd[k];
                if (u.w == 1.0f || u.w == 2.0f)
                    drive_vehicle(u, d.dt, a.geo[2].ctr, a.geo[2].off, a.veh_local, a.veh_head, a.veh_ctr_out, a.veh_pts_out, k, lane);
                else if (a.trk.off && a.trk.off[k + 1] > a.trk.off[k])
                    track_vehicle(a.trk, k, lane, a.geo[2].off, a.veh_local, a.veh_ctr_out, a.veh_pts_out);
                else
                    advance_vehicle(d, k, lane, true);
            }
        } else if (a.trk.off) {                                         // uniform: tracks are set -- a vehicle with keyframes is teleported
            for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) {       // to the one the next tick sees, the others run free as ever
                if (a.trk.off[k + 1] > a.trk.off[k])
                    track_vehicle(a.trk, k, threadIdx.x & (WAVE - 1), a.geo[2].off, a.veh_local, a.veh_ctr_out, a.veh_pts_out);
                else
                    advance_vehicle(d, k, threadIdx.x & (WAVE - 1), true);
            }
        } else {
            for (int k = k0 + wave; k < k1; k += WAVES_PER_BLOCK) advance_vehicle(d, k, threadIdx.x & (WAVE - 1), true);
        }
    }
    const int s0 = a.scene_off[b], n = a.scene_off[b + 1] - s0;       // 0 <= n <= BATCH_MAX_N (checked on the host)
    // MODES: the scene's clock, read by every thread before the barrier and advanced by thread 0 after it (a scene without
    // pedestrians has no barrier: there only thread 0 reads it), by one step_length per tick like the handle's sim_time
    float now = 0.0f;
    if (MODES && (n > 0 || threadIdx.x == 0)) now = a.fsm.sim_time[b];
    if (n <= 0) {
        if (MODES && threadIdx.x == 0) a.fsm.sim_time[b] = now + a.prm[b].dt;
        return;
    }
    const BatchParams& p = a.prm[b];                                    // (read through the pointer: uniform scalar loads)
    for (int t = threadIdx.x; t < n; t += BLOCK) {
        float4 q = a.pk[s0 + t];
        if ((EXT || MODES) && a.frame) a.frame[s0 + t] = q;             // recording tick: the pre-tick state, coalesced
        // SPAWN: the birth rule, on values this launch has not written yet (born[] is stored after the barrier only); row t - 1 of
        // a chained row is in the same scene (the host refuses chain = 1 on a scene's first row)
        uint8_t st = SPAWN_LIVE;
        if constexpr (SPAWN) {
            const uint8_t bn = a.spn.born[s0 + t];
            if (bn == BORN_NO) {
                const bool due = a.spn.spawn_time[s0 + t] <= now && (!a.spn.chain[s0 + t] || a.spn.born[s0 + t - 1] == BORN_YES);
                st = due ? SPAWN_NEWBORN : SPAWN_GHOST;
                if (due) q = a.spn.pk0[s0 + t];                        // the spawn state: every row's pair sum of this tick sees it
            } else if (bn == BORN_AT_SET) {                            // live since the schedule was set: this tick is its birth tick
                st = SPAWN_SETTLED;                                    // for the row chained to it, which waits one tick more
            }
            sh.st[t] = st;
        }
        sh.pk[t] = q;
        if (Z3) {
            float2 zq = a.zv[s0 + t];
            if ((EXT || MODES) && a.zframe) a.zframe[s0 + t] = zq;
            if (SPAWN && st == SPAWN_NEWBORN) zq = a.spn.zv0[s0 + t];
            sh.zv[t] = zq;
        }
        sh.r[t] = a.own[s0 + t].w;
    }
    __syncthreads();
    if (MODES && threadIdx.x == 0) a.fsm.sim_time[b] = now + p.dt;
    if (p.rad) batch_scene<Z3, true, EXT, MODES, SPAWN, STEER>(a, p, sh, b, s0, n, now);
    else batch_scene<Z3, false, EXT, MODES, SPAWN, STEER>(a, p, sh, b, s0, n, now);
}

// sfm_batch_set_spawn_schedule: the rows that are unborn when the schedule is set leave the live state -- parked where a despawned
// row of the same scene-local index would be, velocity 0 (not hot: once per schedule).  A workgroup per scene, as the tick.
__global__ __launch_bounds__(BLOCK) void sfm_batch_park_unborn_kernel(const int* scene_off, const uint8_t* born, float4* pk, float2* zv) {
    const int s0 = scene_off[blockIdx.x], n = scene_off[blockIdx.x + 1] - s0;
    for (int t = threadIdx.x; t < n; t += BLOCK) {
        if (born[s0 + t] != BORN_NO) continue;
        const float2 pp = park_position((uint32_t)t);
        pk[s0 + t] = make_float4(pp.x, pp.y, 0.f, 0.f);
        if (zv) zv[s0 + t].y = 0.f;
    }
}

hipError_t launch_batch_park_unborn(const int* scene_off, const uint8_t* born, float4* pk, float2* zv, int B, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_park_unborn_kernel, dim3(B), dim3(BLOCK), 0, st, scene_off, born, pk, zv);
    return hipGetLastError();
}

// sfm_batch_set_vehicle_tracks: the tracked vehicles as tick t.tick (0 when the tracks are set) sees them, in place -- no tick is in
// flight (not hot: once per call).  A wave per vehicle, like sfm_dynamic_boxes_kernel; a vehicle without keyframes is left alone.
__global__ __launch_bounds__(BLOCK) void sfm_batch_place_tracks_kernel(const BatchTracks t, const int* off, const float2* local, float4* ctr,
                                                                        float2* pts, int M) {
    const int k = uniform((int)(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)));
    if (k >= M || t.off[k + 1] == t.off[k]) return;
    track_vehicle(t, k, threadIdx.x & (WAVE - 1), off, local, ctr, pts);
}

hipError_t launch_batch_place_tracks(const BatchTracks& t, const int* off, const float2* local, float4* ctr, float2* pts, int M,
                                     hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_place_tracks_kernel, dim3((M + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), dim3(BLOCK), 0, st, t, off, local,
                       ctr, pts, M);
    return hipGetLastError();
}

// modes: the mode state machine is on (a.fsm; records frames and forces too, never redraws); else ext: the tick redraws waypoints or
// records a frame or forces (a.flags & 2, a.frame, a.force_rec); otherwise the plain kernel.  spawn (modes only): a spawn schedule
// is set (a.spn) -- its own instantiation, so a batch without one launches the kernel it always did.  steer: commands are set
// (a.cmd) -- instantiations of their own again: of the EXT form (a plain steered tick takes it), of MODES and of MODES + SPAWN
template <bool Z3>
static void launch_batch_tick_steered(bool modes, bool spawn, const BatchArgs& a, int B, hipStream_t st) {
    if (modes && spawn) hipLaunchKernelGGL((sfm_batch_tick_kernel<Z3, false, true, true, true>), dim3(B), dim3(BLOCK), 0, st, a);
    else if (modes) hipLaunchKernelGGL((sfm_batch_tick_kernel<Z3, false, true, false, true>), dim3(B), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((sfm_batch_tick_kernel<Z3, true, false, false, true>), dim3(B), dim3(BLOCK), 0, st, a);
}

hipError_t launch_batch_tick(bool z3, bool ext, bool modes, bool spawn, bool steer, const BatchArgs& a, int B, hipStream_t st) {
    if (steer) {
        if (z3) launch_batch_tick_steered<true>(modes, spawn, a, B, st);
        else launch_batch_tick_steered<false>(modes, spawn, a, B, st);
    } else if (modes && spawn) {
        if (z3) hipLaunchKernelGGL((sfm_batch_tick_kernel<true, false, true, true>), dim3(B), dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((sfm_batch_tick_kernel<false, false, true, true>), dim3(B), dim3(BLOCK), 0, st, a);
    } else if (z3) {
        if (modes) hipLaunchKernelGGL((sfm_batch_tick_kernel<true, false, true>), dim3(B), dim3(BLOCK), 0, st, a);
        else if (ext) hipLaunchKernelGGL((sfm_batch_tick_kernel<true, true, false>), dim3(B), dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((sfm_batch_tick_kernel<true, false, false>), dim3(B), dim3(BLOCK), 0, st, a);
    } else {
        if (modes) hipLaunchKernelGGL((sfm_batch_tick_kernel<false, false, true>), dim3(B), dim3(BLOCK), 0, st, a);
        else if (ext) hipLaunchKernelGGL((sfm_batch_tick_kernel<false, true, false>), dim3(B), dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((sfm_batch_tick_kernel<false, false, false>), dim3(B), dim3(BLOCK), 0, st, a);
    }
    return hipGetLastError();
}

// sfm_batch_restart: the chosen scenes go back to the batch's snapshot (sfm_batch_snapshot) -- every array a tick can change, and
// nothing else.  A workgroup per chosen scene, as the tick: it copies the scene's rows of every per-row array, its vehicles (the half
// of the ping-pong the next tick reads) with their ring points, and its clock.  Plain loads and stores, no LDS, no atomics: a scene
// is written by its own workgroup only, and the scenes that are not chosen are not touched.  A tracked vehicle's first tick moves
// by r.shift (the batch's ticks since the snapshot), so that the batch-wide tick counter tau finds it at the keyframe it was at.
// With r.mask (sfm_batch_restart_device) the grid is all B scenes and the choice is made here: workgroup b reads mask[b] from device
// memory and leaves at once while it is 0 -- a uniform branch, no list, no copy.  With episodes on, a restarted scene's episode
// state starts over.
template <typename T>
__device__ __forceinline__ void restart_copy(T* dst, const T* src, int i0, int i1) {
    if (!dst) return;                                                   // uniform: the batch has no such array
    for (int i = i0 + (int)threadIdx.x; i < i1; i += BLOCK) dst[i] = src[i];
}

__global__ __launch_bounds__(BLOCK) void sfm_batch_restart_kernel(const BatchRestart r) {
    const int b = r.list ? r.list[blockIdx.x] : (int)blockIdx.x;
    if (r.mask && r.mask[b] == 0) return;                               // uniform: the scene is not chosen
    const int s0 = r.scene_off[b], s1 = r.scene_off[b + 1];
    restart_copy(r.pk, r.s_pk, s0, s1);
    restart_copy(r.zv, r.s_zv, s0, s1);
    restart_copy(r.own, r.s_own, s0, s1);
    restart_copy(r.draws, r.s_draws, s0, s1);
    restart_copy(r.mode, r.s_mode, s0, s1);
    restart_copy(r.target, r.s_target, s0, s1);
    restart_copy(r.cursor, r.s_cursor, s0, s1);
    restart_copy(r.born, r.s_born, s0, s1);
    restart_copy(r.birth_time, r.s_birth_time, s0, s1);
    if (r.ctr) {                                                        // uniform: device-side vehicles
        const int k0 = r.item_off[b], k1 = r.item_off[b + 1];
        restart_copy(r.ctr, r.s_ctr, k0, k1);
        restart_copy(r.pts, r.s_pts, r.veh_off[k0], r.veh_off[k1]);
        restart_copy(r.rot, r.s_rot, k0, k1);                           // the headings: a driven vehicle's tick turns them
        if (r.first)
            for (int k = k0 + (int)threadIdx.x; k < k1; k += BLOCK)
                r.first[k] = r.trk_off[k + 1] > r.trk_off[k] ? (int)((long long)r.s_first[k] + r.shift) : r.s_first[k];
    }
    if (r.sim_time && threadIdx.x == 0) r.sim_time[b] = r.s_sim_time[b];
    if (r.age && threadIdx.x == 0) {                                    // the episode starts over
        r.age[b] = 0;
        r.prev_goal_d2[b] = __builtin_nanf("");
    }
}

hipError_t launch_batch_restart(const BatchRestart& r, int scenes, hipStream_t st) {
    hipLaunchKernelGGL(sfm_batch_restart_kernel, dim3(scenes), dim3(BLOCK), 0, st, r);
    return hipGetLastError();
}

}  // namespace sfm
