"""Batched scenes: many small, independent crowds stepped by ONE kernel launch per tick (C ABI: sfm_batch_*, ABI 6; waypoint
streams and recorded runs, ABI 7; device-side vehicles, ABI 8; pedestrian modes, ABI 9; force records, ABI 10; spawn schedules, ABI 11;
vehicle tracks, ABI 12; snapshot and restart, ABI 13; steered pedestrians, ABI 14; observations, ABI 15; episode ends and the restart
by device mask, ABI 16; range scans, ABI 17).

Social-force models are run in bulk as many small scenes -- scenario sampling, RL environments stepped in lock-step, calibration
sweeps over A / lambda / gamma / tau.  ``SfmBatch`` holds B scenes of 0 .. 1024 pedestrians, each with its own parameters (its own
sfm_config) and its own borders / obstacles, and steps all of them in one launch.  A scene's result is bitwise the same whatever
else is in the batch and wherever it sits (for batches of the same kind: planar, or 3-D).  Crowds above 1024 pedestrians belong on
an ``SfmEngine`` handle.

A scene is a dict in the formats ``SfmEngine`` accepts:
  loc, vel, waypoint (N,3); target_speed (N,); radius (N,) or None; crossing (N,) bool or None (border force off);
  borders: list of (P_k,2), border_centers (K,2), border_lengths (K,);
  static_obstacles / dynamic_obstacles: lists of (center(2), ring(P,2)); dynamic_vel (M,2) or None (at rest).
Missing geometry keys mean none.  ``vars(scenarios.make_scenario(...))`` is such a dict.

Rollouts longer than one crossing of a scene use per-scene waypoint streams (``set_waypoint_streams`` + ``redraw=True``: on arrival
a pedestrian takes the next waypoint of its scene's counter-based stream, as a handle does), and ``run_recorded`` returns the
trajectory of every scene from one launch per tick and one device-to-host copy.

Traffic moves on the device (``set_dynamic_boxes`` or ``upload(..., device_vehicles=True)``, ABI 8): each vehicle is given once as
an oriented box (the scene keys ``dynamic_obstacles`` centres, ``dynamic_yaw``, ``dynamic_extent``, ``dynamic_vel``), and every
integrating tick of a scene moves its centres by that scene's step_length * v and regenerates the rings inside the tick's one launch,
as a handle's ``set_dynamic_boxes`` does.  ``dynamic_obstacles()`` reads them back.

Pedestrian modes run on the device too (``set_modes``, ABI 9): per scene a plan of mode objects (``pack_modes``, or
``plan_from_managers`` from PedModeManager mirrors) and waypoint queues like the reference's waypoint_dict.  Inside the tick's one
launch every row applies its mode's target speed, wakes up from IDLE on its scene's clock, waits at the kerb in CHECKING_TRAFFIC
until gap acceptance against its scene's vehicles lets it cross, walks without the border force on the road, pops its queue on
arrival and despawns (parked far away) once the queue runs out -- as a handle's ``set_mode_fsm`` does.  ``modes()`` and ``clocks()``
read them back.  While modes are set, ``redraw=True`` is refused (arrivals pop the queues).

Force records (ABI 10): ``tick_forces`` returns what ``Force.get_force`` gives for every scene (each force of the reference's dict
and the total the velocity update takes) from the tick's one launch, and ``run_recorded_forces`` records them beside every frame
of a recorded run -- for datasets of (state, force) pairs, calibration against observed accelerations, or rewards on single forces.

Spawn schedules (ABI 11): pedestrians enter a scene on the device as they leave it.  A scene keeps a fixed set of rows -- everyone
who will ever walk in it -- and ``set_spawns`` says when each enters (``spawn_time`` on the scene's clock, ``chain`` for the
reference's one release per spawner per tick; ``spawner.scene_from_spawners`` builds rows, mode plan and schedule from PedSpawner
mirrors).  Until its birth tick a row is a ghost like a despawned one (``modes()`` reports 254); in that tick it is staged at its
spawn state before anyone's forces are summed, so it pushes and is pushed from its first tick on.  ``spawns()`` reads back who
is born and on which clock value.

Vehicle tracks (ABI 12): the reference's scripted traffic.  ``set_vehicle_tracks`` gives a device-side vehicle a list of keyframes
(centre, yaw, speed) and a first tick; every integrating tick teleports it to the keyframe of that tick inside the tick's one launch
-- it can turn, brake, stop and pull away -- and outside its list it is absent: centre and ring at +inf, velocity 0, no force on
anyone and no say in gap acceptance.  ``vehicle_tracks()`` reads back the tick counter and who is present;
``scenarios.place_tracked`` is the host twin and ``vehicle_spawner.tracks_from_spawners`` builds tracks from VehicleSpawner mirrors.

Starting over (ABI 13): ``snapshot()`` copies, on the device, everything a tick can change -- state, waypoints, draw counters,
vehicles, modes, clocks, births, track time -- and ``restart(scenes)`` puts the chosen scenes back to it with one launch, leaving the
others alone bit for bit: episodes of an RL loop that end at different times, or a calibration sweep (``snapshot()`` once, then per
candidate ``set_params``, ``restart()``, ``run``: a restarted scene runs under the parameters, waypoint streams, borders and static
obstacles of the moment).  ``upload`` and the calls that set vehicles, modes, spawn schedules or tracks drop the snapshot
(``has_snapshot``).  Scripted traffic restarts per scene as well: a restarted scene's tracked vehicles are where they were at the
snapshot, while ``vehicle_tracks()`` goes on counting the batch's ticks.

Steered pedestrians (ABI 14): rows whose motion the caller decides -- the ego agent of an RL policy, observed pedestrians replayed
along their recorded motion, the reference's ``update_ped_info``.  ``set_steering(kinds, commands)`` gives every row a kind (0 not
steered, 1 velocity command: v' is the command bit for bit; 2 preferred velocity: the command replaces v0 * e_wp in the
acceleration term) and a command; the tick's one launch reads them, everyone else sees a steered row as an ordinary pedestrian,
and arrivals, modes, despawn and birth go on for it.  ``set_commands`` sends new velocities with one copy per step;
``command_tensor()`` is the command buffer as a torch tensor a policy writes on the device, ``state_tensor()`` / ``zstate_tensor()``
the state it reads.  Steering is an input like the parameters: only ``upload`` drops it, and a snapshot neither holds nor loses it.

Observations (ABI 15): what a policy or a reward reads per agent, computed on the device by one launch per call.
``set_observation(k, sense_range, frame)`` chooses k neighbour slots, a sense range per scene and world axes or the row's heading
frame; ``observe()`` fills, per row, ``16 + 4k`` floats -- goal, own velocity, target speed, a live flag, the number of neighbours
found, which kinds of geometry are in range, the nearest vehicle ring point with the vehicle's relative velocity, the nearest border
and static-obstacle points, and the k nearest neighbours in ascending (distance, index) order as relative positions and velocities
(the record and its exact rules: include/sfm_hip.h).  ``observations()`` downloads them per scene, ``observation_tensor()`` is the
buffer as a torch tensor a policy reads on the device, and ``observe.observe_scene`` is the host twin, bit for bit in frame 0.
Observing changes nothing a tick reads.  With ``snapshot`` / ``restart`` (the reset) and steering (the action) this closes an RL
loop with no host in it: examples/batch_rl_loop.py.

Episode ends (ABI 16): who is done, decided on the device.  ``set_episodes(agent, goal_radius, ped_radius, veh_radius, max_steps)``
names one agent row per scene, three radii and a time limit; ``end_step()`` is one launch that writes, per scene, a record of 8
floats (``EP_*``: done, the reason bits ``REASON_*``, the episode's age, the squared distances to the goal now and one evaluation
ago, to the nearest live pedestrian, vehicle ring point and border / static-obstacle point -- what a reward is made of) and a byte
mask ``done``; ``end_step(auto_restart=True)`` follows it with ``restart_device()``, the restart whose mask stays on the device, so
a step of the loop copies nothing and waits for nothing: examples/batch_rl_loop_device.py.  Every restart of a scene starts its
episode clock over.  ``episodes()`` downloads record and mask, ``episode_tensor()`` / ``done_tensor()`` alias them, and
``episode.episode_scene`` is the host twin, bit for bit.

Range scans (ABI 17): the sensor most crowd-navigation policies are trained on, computed on the device by one launch per call.
``set_scan(max_range, ped_radius, point_radius, R=..., mask=..., frame=...)`` chooses R rays around every scanned row (2 pi q / R
by default, or ``angles``, or ``directions`` used as given), a range limit and two radii per scene: every other pedestrian is a disc
of ``ped_radius``, every sampled point of a border, a static-obstacle ring or a vehicle ring a disc of ``point_radius`` (the
model's own view of geometry; 0.1 m, the reference's sampling resolution, by default).  ``scan()`` fills, per row, ``2R`` floats:
the distance along each ray to the first disc it meets (``max_range`` when there is none nearer) and the kind of what was hit (0
nothing, 1 pedestrian, 2 border, 3 static obstacle, 4 vehicle) -- an occluding wall, a gap between two parked cars, a kerb
alongside, which a list of k neighbours cannot express.  ``mask`` names the rows that are scanned (an RL loop scans its agents,
not the crowd); the others cost nothing and read zeros.  ``scans()`` downloads them per scene, ``scan_tensor()`` is the buffer as a
torch tensor a policy reads on the device, and ``scan.scan_scene`` is the host twin, bit for bit in both frames (the record and its
exact rules: include/sfm_hip.h).  Scanning changes nothing a tick reads: examples/batch_lidar_loop.py.

Restart noise (ABI 17, added without a bump): resets that sample.  A plain restart is the snapshot bit for bit, so every episode of
a scene starts alike; ``set_restart_noise(seeds, pos_box, goal_box, min_gap, point_gap, tries, track_delay)`` lets every restart
(``restart``, ``restart_device``, ``end_step(auto_restart=True)``) be followed by one more launch that draws each row's start from a
box around its snapshot position, again while it is too near a row already placed, a lower-index proposal or a point of the
scene's geometry, draws the goals from a box around the snapshot goal and lets tracked vehicles arrive up to ``track_delay`` ticks
later -- all keyed by the scene's seed and its restart counter, so reproducible and the same alone or in any batch.
``restart_noise()`` downloads the counters (restarts per scene, rows of the latest restart no try could place),
``reset_count_tensor()`` aliases the first, and ``reset.resample_scene`` is the host twin, bit for bit (the exact rule:
include/sfm_hip.h): examples/batch_rl_loop_randomised.py.

Occupancy grids (ABI 17, added without a bump): the local map of a CNN policy, computed on the device by one launch per call.
``set_grid(cell, G=..., mask=..., frame=...)`` chooses a G x G grid (G <= 32) of ``cell`` metres per cell (one value, or one per
scene) centred on every gridded row, in world axes or in the row's heading frame (x forward).  ``grid()`` fills, per gridded row,
6 channels of G x G floats: the number of other live pedestrians per cell, the sum of their velocities relative to the row (two
channels; a sum, divide by the count for a mean), and the number of sampled border, static-obstacle and vehicle points per cell
-- the geometry a torch sequence over ``state_tensor()`` cannot see.  The rows named by ``mask`` get compact slots in ascending
row order, so the buffer is ``(M, 6, G, G)`` for M gridded rows, not one record per row of the batch.  ``grids()`` downloads them
per scene, ``grid_rows()`` names the row of every slot, ``grid_tensor()`` is the buffer as a torch tensor a conv layer reads as it
stands, and ``grid.grid_scene`` is the host twin, bit for bit in both frames, velocity sums included (the record and its exact
rules: include/sfm_hip.h).  Gridding changes nothing a tick reads: examples/batch_grid_loop.py.

Observed tracks (ABI 17, added without a bump): calibration against recorded motion with no host in the loop, the protocol of
Johansson et al. 2007.  ``set_observed(tracks, roles, every, v0)`` puts each scene's recording on the device -- ``(F_b, n_b, 2)``
positions per scene, NaN where a pedestrian is not seen, one frame every ``every`` ticks -- and gives every row a role: 0 not part
of the data (left alone bit for bit), 1 replayed, 2 scored.  ``run_observed(first, frames)`` launches, per frame, one frame kernel
and then ``every`` ticks: a replayed row is put on its track with the velocity that carries it to its next frame (a velocity
command, so nothing drifts), parked like a despawned row while it is not seen -- people enter and leave --, and a scored row is
placed at its first frame, simulated by the model from there on and compared with its track at every later frame it is seen in;
the error sums stay on the device.  ``score()`` reduces them per scene to ``{rows, samples, sum_d, sum_d2, sum_final_d}``
(``replay.metrics``: ADE, RMSE, FDE); ``scene_scores()`` / ``row_scores()`` download them, ``scene_score_tensor()`` /
``row_score_tensor()`` alias them.  A sweep is ``set_params``, ``run_observed(0, F)``, ``scene_scores()``: one copy of B x 5
floats per candidate.  Steering is switched on if it is off (rows of role 0 keep the caller's commands); ``upload``, ``set_modes``,
``set_spawns`` and ``set_steering(None)`` drop the tracks.  ``replay.replay_frame`` and ``replay.score_scene`` are the host twins, bit for
bit, and ``replay.scene_from_tracks`` packs a recording into a scene (the exact rules: include/sfm_hip.h):
examples/batch_calibration_sweep.py.

Driven vehicles (ABI 17, added without a bump): device-side vehicles whose motion is decided while the batch runs -- a driving
policy trained against the crowd, a planner under test, a braking controller.  ``set_vehicle_driving(kinds, commands)`` gives
every vehicle a command ``(a, b, c)`` that each integrating tick reads inside its one launch: kind 1 takes ``(a, b)`` as the new
velocity and turns the heading to it (a stopped vehicle keeps its heading); kind 2 is a unicycle -- signed speed ``a`` along the
heading, which this tick first turns by ``(b, c) = (cos, sin)`` of the turn (the kernel does no trigonometry; ``a < 0``
reverses); kind 0 runs free or follows its track as ever.  The stored velocity becomes the commanded one, so the dynamic obstacle
force and gap acceptance see it from the next tick on.  ``set_vehicle_commands`` sends new commands with one copy on the stream,
``vehicle_command_tensor()`` aliases the buffer for torch, ``vehicle_driving()`` downloads kinds, commands, headings and
velocities.  The heading is state: ``snapshot`` holds it, every restart puts it back.  ``set_vehicle_observation(k, sense_range,
frame, goals, mask)`` and ``observe_vehicles()`` are the sensor centred on a vehicle, one launch: goal, velocity, heading, the
``k`` nearest live pedestrians in ``(d2, j)`` order, ``clear_d2`` (ring to crowd, for collisions and near misses), ``other_d2``
(the scene's other vehicles), the nearest border and static points, the signed speed; ``vehicle_observations()`` downloads it,
``vehicle_observation_tensor()`` aliases it.  ``upload`` and ``set_dynamic_boxes`` drop both, every other call keeps them.
``scenarios.drive_vehicles`` and ``observe.observe_vehicles_scene`` are the host twins, bit for bit (the exact rules:
include/sfm_hip.h): examples/batch_av_loop.py.

Range scans from the vehicles (ABI 17, added without a bump): the lidar of a driving policy.  ``set_vehicle_scan(max_range,
ped_radius, point_radius, R=..., mask=..., frame=..., mount=...)`` chooses up to 256 rays from a sensor mounted at ``mount`` in the
vehicle frame; ``scan_vehicles()`` fills, per vehicle, ``2R`` floats in one launch -- ranges, then kinds as for ``scan()`` -- with
every pedestrian, border, static obstacle and OTHER vehicle of the scene as candidates and the vehicle's own ring left out.
Frame 1 turns the rays by the stored heading.  ``vehicle_scans()`` downloads per scene, ``vehicle_scan_tensor()`` aliases the
buffer, ``scan.scan_vehicles_scene`` is the host twin, bit for bit in both frames.  ``upload`` and ``set_dynamic_boxes`` drop it,
every other call keeps it: examples/batch_av_lidar_loop.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import grid as _grid
from . import replay as _replay
from . import scan as _scan
from ._args import FRAME_HEADING, FRAME_WORLD, MAX_METRES as MAX_SENSE_RANGE, check_frame, per_scene, per_scene_metres
from ._lib import SfmLibraryError, f32, fptr, iptr, u8ptr

MAX_RECORD_BYTES = 1 << 30       # SFM_BATCH_MAX_RECORD_BYTES: frames one run_recorded call may hold
from .engine import _csr, params_from_config

MAX_SCENE_PEDESTRIANS = 1024     # SFM_BATCH_MAX_N
MAX_TRACK_KEYS = 1 << 22         # SFM_BATCH_MAX_TRACK_KEYS: keyframes one set_vehicle_tracks call may hold

# the forces a batch records, in SFM_FORCE_* index order: the reference's force-dict keys and the total (SfmEngine.forces' names)
FORCE_RECORD_NAMES = tuple(_lib.FORCE_NAMES) + ("total",)


def _rows(a, n, width, name, k):
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(-1, width) if width else a.reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"scene {k}: {name} has {a.shape[0]} rows, expected {n}")
    return a


def _polylines(polys, name, k):
    out = []
    for q, pl in enumerate(polys):
        a = np.asarray(pl, dtype=np.float64)
        if a.size and (a.ndim != 2 or a.shape[1] != 2):
            raise ValueError(f"scene {k}: {name} {q} must be a (P,2) array, got shape {a.shape}")
        out.append(a.reshape(-1, 2))
    return out


def _obstacles(obstacles, name, k):
    obstacles = [] if obstacles is None else list(obstacles)
    cs = []
    for q, ob in enumerate(obstacles):
        if len(ob) != 2:
            raise ValueError(f"scene {k}: {name} {q} must be a (center, ring) pair")
        c = np.asarray(ob[0], dtype=np.float64).reshape(-1)
        if c.size < 2:
            raise ValueError(f"scene {k}: {name} {q} has a centre of {c.size} coordinates")
        cs.append(c[:2])
    rings = _polylines([ob[1] for ob in obstacles], name, k)
    return np.array(cs, dtype=np.float64).reshape(-1, 2), rings


def _scene_csr(per_scene_polys):
    """Concatenate per-scene polyline lists: (scene_item_off [B+1] int32, offsets [K+1] int32, px, py)."""
    item_off = np.zeros(len(per_scene_polys) + 1, dtype=np.int32)
    for b, polys in enumerate(per_scene_polys):
        item_off[b + 1] = item_off[b] + len(polys)
    off, px, py = _csr([pl for polys in per_scene_polys for pl in polys])
    return item_off, off, px, py


def pack_scenes(scenes):
    """Scenes (list of dicts, see the module docstring) -> the concatenated fp32 SoA and CSR arrays of the C ABI.  Pure NumPy.

    Returns a dict: ``scene_off`` int32 [B+1]; ``x y z vx vy vz wx wy target_speed radius`` float32 [N_total]; ``crossing`` uint8
    [N_total]; ``planar`` (bool: every scene has a single z and no v_z -- SfmEngine.upload_state's planar=None rule, per scene,
    applied batch-wide: one 3-D scene makes the whole batch 3-D); ``borders`` = (scene_item_off, offsets, px, py, cx, cy,
    cull_len); ``static`` = (scene_item_off, offsets, px, py, cx, cy); ``dynamic`` = (scene_item_off, offsets, px, py, cx, cy, vx, vy).
    Raises ValueError on a scene of more than 1024 pedestrians and on malformed state or geometry."""
    scenes = list(scenes)
    if not scenes:
        raise ValueError("a batch needs at least one scene")
    B = len(scenes)
    scene_off = np.zeros(B + 1, dtype=np.int32)
    cols = {k: [] for k in ("loc", "vel", "wp", "ts", "rad", "cross")}
    planar = True
    border_polys, border_c, border_l = [], [], []
    stat_polys, stat_c = [], []
    dyn_polys, dyn_c, dyn_v = [], [], []
    for k, sc in enumerate(scenes):
        loc = np.asarray(sc["loc"], dtype=np.float64)
        if loc.size % 3:
            raise ValueError(f"scene {k}: loc must be (N,3)")
        loc = loc.reshape(-1, 3)
        n = loc.shape[0]
        if n > MAX_SCENE_PEDESTRIANS:
            raise ValueError(f"scene {k} has {n} pedestrians; a batch takes up to {MAX_SCENE_PEDESTRIANS} per scene "
                             "(larger crowds belong on an SfmEngine handle)")
        vel = _rows(sc["vel"], n, 3, "vel", k)
        wp = _rows(sc["waypoint"], n, 3, "waypoint", k)
        ts = _rows(sc["target_speed"], n, 0, "target_speed", k)
        rad = sc.get("radius")
        rad = np.zeros(n) if rad is None else _rows(rad, n, 0, "radius", k)
        cr = sc.get("crossing")
        cr = np.zeros(n, dtype=bool) if cr is None else _rows(cr, n, 0, "crossing", k).astype(bool)
        if n and not (bool(np.all(loc[:, 2] == loc[0, 2])) and not bool(np.any(vel[:, 2] != 0.0))):
            planar = False
        for key, v in zip(("loc", "vel", "wp", "ts", "rad", "cross"), (loc, vel, wp, ts, rad, cr)):
            cols[key].append(v)
        scene_off[k + 1] = scene_off[k] + n

        borders = sc.get("borders")
        borders = _polylines([] if borders is None else borders, "border", k)
        K = len(borders)
        cen = sc.get("border_centers")
        ln = sc.get("border_lengths")
        cen = np.zeros((0, 2)) if cen is None else np.asarray(cen, dtype=np.float64)
        ln = np.zeros(0) if ln is None else np.asarray(ln, dtype=np.float64).reshape(-1)
        if cen.size != 2 * K or ln.size != K:
            raise ValueError(f"scene {k}: {K} borders need {K} centres and {K} lengths (got {cen.size} centre coordinates "
                             f"and {ln.size} lengths)")
        border_polys.append(borders)
        border_c.append(cen.reshape(K, 2))
        border_l.append(ln)
        c, rings = _obstacles(sc.get("static_obstacles"), "static obstacle", k)
        stat_polys.append(rings)
        stat_c.append(c)
        c, rings = _obstacles(sc.get("dynamic_obstacles"), "dynamic obstacle", k)
        M = len(rings)
        v = sc.get("dynamic_vel")
        v = np.zeros((M, 2)) if v is None else np.asarray(v, dtype=np.float64)
        if v.size != 2 * M:
            raise ValueError(f"scene {k}: {M} dynamic obstacles need {M} velocities (got {v.size / 2:g})")
        dyn_polys.append(rings)
        dyn_c.append(c)
        dyn_v.append(v.reshape(M, 2))

    cat = lambda key, width: (np.concatenate(cols[key], axis=0) if cols[key] else np.zeros((0, width) if width else 0))
    loc, vel, wp = cat("loc", 3), cat("vel", 3), cat("wp", 3)
    bc, sc_, dc, dv = (np.concatenate(a, axis=0) for a in (border_c, stat_c, dyn_c, dyn_v))
    return {
        "scene_off": scene_off,
        "x": f32(loc[:, 0]), "y": f32(loc[:, 1]), "z": f32(loc[:, 2]),
        "vx": f32(vel[:, 0]), "vy": f32(vel[:, 1]), "vz": f32(vel[:, 2]),
        "wx": f32(wp[:, 0]), "wy": f32(wp[:, 1]),
        "target_speed": f32(cat("ts", 0)), "radius": f32(cat("rad", 0)),
        "crossing": np.ascontiguousarray(cat("cross", 0), dtype=np.uint8),
        "planar": planar,
        "borders": (*_scene_csr(border_polys), f32(bc[:, 0]), f32(bc[:, 1]), f32(np.concatenate(border_l))),
        "static": (*_scene_csr(stat_polys), f32(sc_[:, 0]), f32(sc_[:, 1])),
        "dynamic": (*_scene_csr(dyn_polys), f32(dc[:, 0]), f32(dc[:, 1]), f32(dv[:, 0]), f32(dv[:, 1])),
    }


def pack_boxes(scenes, resolution=0.1):
    """Scenes (list of dicts) -> the arguments of sfm_batch_set_dynamic_boxes: (scene_item_off int32 [B+1], offsets int32 [M+1],
    ux, uy float32 [P], cx, cy, yaw_cos, yaw_sin, vx, vy float32 [M]), concatenated in scene order.  Per scene exactly what
    ``SfmEngine.set_dynamic_boxes`` passes for it: ring-local offsets from ``scenarios.ring_local_offsets(ex, ey, resolution)``, fp32
    cos / sin of the float64 yaw.  Uses the centres of ``dynamic_obstacles`` (their rings are ignored), ``dynamic_yaw`` (M,),
    ``dynamic_extent`` (M,2) half-extents and ``dynamic_vel`` (M,2) or None (at rest).  Pure NumPy; raises ValueError on count
    mismatches."""
    from .scenarios import ring_local_offsets
    scenes = list(scenes)
    item_off = np.zeros(len(scenes) + 1, dtype=np.int32)
    locs, cs, yaws, vs = [], [], [], []
    for k, sc in enumerate(scenes):
        c, _ = _obstacles(sc.get("dynamic_obstacles"), "dynamic obstacle", k)
        M = c.shape[0]
        cols = []
        for key, width in (("dynamic_yaw", 1), ("dynamic_extent", 2), ("dynamic_vel", 2)):
            a = sc.get(key)
            if a is None and (M == 0 or key == "dynamic_vel"):
                a = np.zeros((M, width))
            elif a is None:
                raise ValueError(f"scene {k}: {M} vehicles need {key}")
            a = np.asarray(a, dtype=np.float64)
            if a.size != width * M:
                raise ValueError(f"scene {k}: {M} vehicles need {M} rows of {key} (got {a.size / width:g})")
            cols.append(a.reshape(M, width))
        yaw, ext, v = cols
        locs += [ring_local_offsets(ex, ey, resolution) for ex, ey in ext]
        cs.append(c)
        yaws.append(yaw[:, 0])
        vs.append(v)
        item_off[k + 1] = item_off[k] + M
    off, ux, uy = _csr(locs)
    c = np.concatenate(cs, axis=0) if cs else np.zeros((0, 2))
    yaw = np.concatenate(yaws) if yaws else np.zeros(0)
    v = np.concatenate(vs, axis=0) if vs else np.zeros((0, 2))
    return (item_off, off, ux, uy, f32(c[:, 0]), f32(c[:, 1]), f32(np.cos(yaw)), f32(np.sin(yaw)), f32(v[:, 0]), f32(v[:, 1]))


def batch_params(configs, step_lengths, B=None, honour_file_keys=False):
    """One config (dict) or a list of B configs, one step length or B of them -> a ctypes array of B SfmParams
    (``params_from_config`` per scene)."""
    cfgs = [configs] if isinstance(configs, dict) else list(configs)
    steps = np.atleast_1d(np.asarray(step_lengths, dtype=np.float64))
    if B is None:
        B = max(len(cfgs), len(steps))
    if len(cfgs) not in (1, B) or len(steps) not in (1, B):
        raise ValueError(f"{len(cfgs)} configs and {len(steps)} step lengths for {B} scenes")
    arr = (_lib.SfmParamsC * B)()
    for k in range(B):
        arr[k] = params_from_config(cfgs[k if len(cfgs) > 1 else 0], float(steps[k if len(steps) > 1 else 0]), honour_file_keys)
    return arr


def stream_arrays(B, seeds, world_sides, arrive_thresholds=2.0):
    """Per-scene waypoint stream arguments -> (seed uint32[B], world_side float32[B], arrive_threshold float32[B]).  Each argument is
    a scalar (broadcast to every scene) or B values.  Seeds are integers (taken mod 2^32, like SfmEngine.set_waypoint_stream); sides
    and thresholds must be finite and >= 0.  Pure NumPy; raises ValueError."""
    s = per_scene(seeds, "seeds", B, "iu", shape_first=True)
    out = [np.ascontiguousarray(s.astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)]
    for v, name in ((world_sides, "world_sides"), (arrive_thresholds, "arrive_thresholds")):
        a = f32(per_scene(v, name, B, shape_first=True))
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"{name} must be finite and >= 0")
        out.append(a)
    return tuple(out)


MODE_KEYS = ("mode", "target_speed", "initial_speed", "crossing_speed", "safety_margin", "next_mode_time")


def plan_from_managers(managers, queues):
    """A scene's mode plan from its PedModeManager mirror objects (the attributes SfmEngine.set_mode_fsm reads: current_mode,
    target_speed, initial_target_speed, crossing_speed, crossing_safety_margin, next_mode_time) and its waypoint queues
    (``queues[i]`` = [(waypoint (2|3), crossing_road), ...] like waypoint_dict).  Pure NumPy."""
    managers = list(managers)
    f = lambda attr: np.array([float(getattr(m, attr)) for m in managers], dtype=np.float64)
    return {"mode": np.array([int(m.current_mode) for m in managers], dtype=np.int64),
            "target_speed": f("target_speed"), "initial_speed": f("initial_target_speed"), "crossing_speed": f("crossing_speed"),
            "safety_margin": f("crossing_safety_margin"), "next_mode_time": f("next_mode_time"),
            "queues": [list(q) for q in queues]}


def pack_modes(plans, scene_off, scenes=None):
    """One mode plan per scene (dicts: ``mode``, ``target_speed``, ``initial_speed``, ``crossing_speed``, ``safety_margin``,
    ``next_mode_time`` (N_b,) each; ``queues`` N_b lists of (waypoint (2|3), crossing_road); optionally ``first_vehicle_extent``
    (2,), default the scene's ``dynamic_extent[0]`` when ``scenes`` is given and the scene has vehicles, else zeros) -> the
    per-row arguments of sfm_batch_set_mode_fsm, concatenated in scene order: a dict of ``mode`` uint8, the five float32 columns,
    ``wp_offsets`` int32 [N_total+1], ``wp_x``, ``wp_y`` float32 [W], ``wp_crossing`` uint8 [W] and ``first_vehicle_extent``
    float32 [B,2].  Pure NumPy; raises ValueError naming the scene and the key."""
    so = np.asarray(scene_off)
    B = len(so) - 1
    plans = list(plans)
    if len(plans) != B:
        raise ValueError(f"{len(plans)} mode plans for {B} scenes")
    if scenes is not None and len(scenes) != B:
        raise ValueError(f"{len(scenes)} scenes for {B} mode plans")
    cols = {k: [] for k in MODE_KEYS}
    counts, wx, wy, wc = [], [], [], []
    ext = np.zeros((B, 2))
    for b, plan in enumerate(plans):
        n = int(so[b + 1] - so[b])
        if not isinstance(plan, dict):
            raise ValueError(f"scene {b}: a mode plan must be a dict")
        for key in MODE_KEYS + ("queues",):
            if key not in plan:
                raise ValueError(f"scene {b}: the mode plan has no {key}")
        for key in MODE_KEYS:
            a = np.asarray(plan[key], dtype=np.float64).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"scene {b}: {key} has {a.shape[0]} rows, expected {n}")
            if key == "mode" and n and not (np.all(a == np.round(a)) and a.min() >= 0 and a.max() <= 4):
                raise ValueError(f"scene {b}: mode must hold PedMode values 0..4")
            cols[key].append(a)
        queues = list(plan["queues"])
        if len(queues) != n:
            raise ValueError(f"scene {b}: queues has {len(queues)} lists, expected {n}")
        for i, q in enumerate(queues):
            counts.append(len(q))
            for e, item in enumerate(q):
                if len(item) != 2:
                    raise ValueError(f"scene {b}: queues[{i}][{e}] must be a (waypoint, crossing_road) pair")
                w = np.asarray(item[0], dtype=np.float64).reshape(-1)
                if w.size not in (2, 3):
                    raise ValueError(f"scene {b}: queues[{i}][{e}] has a waypoint of {w.size} coordinates")
                wx.append(w[0]); wy.append(w[1]); wc.append(1 if item[1] else 0)
        e0 = plan.get("first_vehicle_extent")
        if e0 is None and scenes is not None:
            de = scenes[b].get("dynamic_extent") if isinstance(scenes[b], dict) else getattr(scenes[b], "dynamic_extent", None)
            if de is not None and len(de):
                e0 = np.asarray(de, dtype=np.float64).reshape(-1, 2)[0]
        if e0 is not None:
            e0 = np.asarray(e0, dtype=np.float64).reshape(-1)
            if e0.size != 2:
                raise ValueError(f"scene {b}: first_vehicle_extent must have 2 values, got {e0.size}")
            ext[b] = e0
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=off[1:])
    cat = lambda key: np.concatenate(cols[key]) if cols[key] else np.zeros(0)
    out = {"mode": np.ascontiguousarray(cat("mode"), dtype=np.uint8)}
    out.update({k: f32(cat(k)) for k in MODE_KEYS[1:]})
    out.update(wp_offsets=off, wp_x=f32(wx), wp_y=f32(wy), wp_crossing=np.ascontiguousarray(wc, dtype=np.uint8),
               first_vehicle_extent=f32(ext))
    return out


def pack_spawns(schedules, scene_off):
    """One spawn schedule per scene (``None``: everyone is there from the start; or a dict ``spawn_time`` (N_b,) -- seconds on the
    scene's clock, -inf: there from the start, +inf: never -- and ``chain`` (N_b,) 0 / 1, default zeros: 1 = the row waits for row
    i - 1 of its scene to be born in an earlier tick) -> the per-row arguments of sfm_batch_set_spawn_schedule, concatenated in
    scene order: (spawn_time float32 [N_total], chain uint8 [N_total]).  Pure NumPy; raises ValueError naming the scene."""
    so = np.asarray(scene_off)
    B = len(so) - 1
    schedules = list(schedules)
    if len(schedules) != B:
        raise ValueError(f"{len(schedules)} spawn schedules for {B} scenes")
    times, chains = [], []
    for b, sch in enumerate(schedules):
        n = int(so[b + 1] - so[b])
        if sch is None:
            times.append(np.full(n, -np.inf)); chains.append(np.zeros(n))
            continue
        if not isinstance(sch, dict):
            raise ValueError(f"scene {b}: a spawn schedule must be a dict or None")
        if "spawn_time" not in sch:
            raise ValueError(f"scene {b}: the spawn schedule has no spawn_time")
        t = np.asarray(sch["spawn_time"], dtype=np.float64).reshape(-1)
        c = np.zeros(n) if sch.get("chain") is None else np.asarray(sch["chain"], dtype=np.float64).reshape(-1)
        for key, a in (("spawn_time", t), ("chain", c)):
            if a.shape[0] != n:
                raise ValueError(f"scene {b}: {key} has {a.shape[0]} rows, expected {n}")
        if np.isnan(t).any():
            raise ValueError(f"scene {b}: spawn_time must not be NaN (-inf: there from the start, +inf: never)")
        if n and not np.isin(c, (0.0, 1.0)).all():
            raise ValueError(f"scene {b}: chain must hold 0 or 1")
        if n and c[0] != 0:
            raise ValueError(f"scene {b}: chain must be 0 on the scene's first row (it has no row to wait for)")
        times.append(t); chains.append(c)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    with np.errstate(over="ignore"):
        return f32(cat(times)), np.ascontiguousarray(cat(chains), dtype=np.uint8)


TRACK_KEYS = ("xy", "yaw", "speed", "first_tick")


def _vehicle_counts(scenes):
    """``scenes`` as pack_tracks takes it -> vehicles per scene: a list of scene dicts / Scenario objects (their
    ``dynamic_obstacles``), or the vehicles' scene_item_off [B+1] (what ``pack_boxes`` returns first)."""
    if isinstance(scenes, np.ndarray):
        off = scenes.reshape(-1)
        if off.dtype.kind not in "iu" or off.size < 2 or off[0] != 0 or (np.diff(off) < 0).any():
            raise ValueError("scenes given as an array must be the vehicles' scene_item_off: integers from 0, non-decreasing")
        return [int(c) for c in np.diff(off)]
    counts = []
    for sc in scenes:
        dyn = sc.get("dynamic_obstacles") if isinstance(sc, dict) else getattr(sc, "dynamic_obstacles", None)
        counts.append(0 if dyn is None else len(dyn))
    return counts


def pack_tracks(tracks, scenes):
    """Vehicle tracks -> the arguments of sfm_batch_set_vehicle_tracks.  ``tracks``: per scene ``None`` (no vehicle of the scene is
    tracked) or a list with one entry per vehicle, each ``None`` (free-running) or a dict ``xy`` (L,2), ``yaw`` (L,) radians,
    ``speed`` (L,), L >= 1, and ``first_tick`` (an integer, may be negative): keyframe j is what integrating tick first_tick + j
    after the call sees.  ``scenes``: what says how many vehicles each scene has (see ``_vehicle_counts``).

    Returns a dict: ``trk_off`` int32 [M+1], ``first_tick`` int32 [M] (0 for untracked vehicles), ``kx ky kvx kvy kcos ksin``
    float32 [T], concatenated in scene order.  Velocity is (speed cos yaw, speed sin yaw), each product formed in float64 and
    rounded to float32 once; ``kcos`` / ``ksin`` are the float32 cos / sin of the float64 yaw, as ``scenarios.place_ring_f32``
    rounds them.  Pure NumPy; raises ValueError naming the scene and the vehicle."""
    counts = _vehicle_counts(scenes)
    tracks = list(tracks)
    if len(tracks) != len(counts):
        raise ValueError(f"{len(tracks)} track lists for {len(counts)} scenes")
    lens, first, cols = [], [], {k: [] for k in ("x", "y", "vx", "vy", "cos", "sin")}
    for b, (per, M) in enumerate(zip(tracks, counts)):
        per = [None] * M if per is None else list(per)
        if len(per) != M:
            raise ValueError(f"scene {b}: {len(per)} tracks for {M} vehicles")
        for k, tr in enumerate(per):
            if tr is None:
                lens.append(0); first.append(0)
                continue
            if not isinstance(tr, dict):
                raise ValueError(f"scene {b}, vehicle {k}: a track must be a dict or None")
            for key in TRACK_KEYS:
                if key not in tr:
                    raise ValueError(f"scene {b}, vehicle {k}: the track has no {key}")
            xy = np.asarray(tr["xy"], dtype=np.float64)
            yaw = np.asarray(tr["yaw"], dtype=np.float64).reshape(-1)
            sp = np.asarray(tr["speed"], dtype=np.float64).reshape(-1)
            if xy.ndim != 2 or xy.shape[1] != 2:
                raise ValueError(f"scene {b}, vehicle {k}: xy must be (L,2), got shape {xy.shape}")
            L = xy.shape[0]
            if L < 1:
                raise ValueError(f"scene {b}, vehicle {k}: a track needs at least one keyframe (None: free-running)")
            if yaw.shape[0] != L or sp.shape[0] != L:
                raise ValueError(f"scene {b}, vehicle {k}: {L} keyframes need {L} yaw and speed values "
                                 f"(got {yaw.shape[0]} and {sp.shape[0]})")
            ft = tr["first_tick"]
            if isinstance(ft, (bool, np.bool_)) or not isinstance(ft, (int, np.integer)) or not -2**31 <= int(ft) < 2**31:
                raise ValueError(f"scene {b}, vehicle {k}: first_tick must be an integer that fits int32, got {ft!r}")
            with np.errstate(over="ignore", invalid="ignore"):
                vx, vy = sp * np.cos(yaw), sp * np.sin(yaw)
                vals = [f32(xy[:, 0]), f32(xy[:, 1]), f32(vx), f32(vy), f32(np.cos(yaw)), f32(np.sin(yaw))]
            if not all(np.isfinite(v).all() for v in vals):
                raise ValueError(f"scene {b}, vehicle {k}: keyframes must be finite in float32")
            for key, v in zip(cols, vals):
                cols[key].append(v)
            lens.append(L); first.append(int(ft))
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] > MAX_TRACK_KEYS:
        raise ValueError(f"the tracks hold {int(off[-1])} keyframes, more than the {MAX_TRACK_KEYS} one call may set: "
                         "set shorter tracks and set them again later")
    cat = lambda key: np.concatenate(cols[key]) if cols[key] else np.zeros(0, np.float32)
    out = {"trk_off": off.astype(np.int32), "first_tick": np.asarray(first, dtype=np.int32).reshape(-1)}
    out.update({"k" + key: f32(cat(key)) for key in cols})
    return out


def mode_scene_arrays(B, despawn_on_arrival=True, sim_time0=0.0, arrive_thresholds=2.0):
    """Per-scene mode arguments -> (despawn_on_arrival int32[B], sim_time0 float32[B], arrive_threshold float32[B]).  Each argument
    is a scalar (broadcast to every scene) or B values; clocks must be finite, thresholds finite and >= 0.  Pure NumPy; raises
    ValueError."""
    col = lambda v, name: per_scene(v, name, B, "biuf", shape_first=True)
    despawn = np.ascontiguousarray(col(despawn_on_arrival, "despawn_on_arrival").astype(bool), dtype=np.int32)
    t0 = f32(col(sim_time0, "sim_time0"))
    if not np.isfinite(t0).all():
        raise ValueError("sim_time0 must be finite")
    thr = f32(col(arrive_thresholds, "arrive_thresholds"))
    if not (np.isfinite(thr).all() and (thr >= 0).all()):
        raise ValueError("arrive_thresholds must be finite and >= 0")
    return despawn, t0, thr


def restart_mask(B, scenes=None):
    """Which scenes ``SfmBatch.restart`` restarts -> the mask of sfm_batch_restart, uint8 [B] of 0 / 1.  ``scenes``: None (every
    scene), a bool array (B,), or a sequence of scene indices 0 .. B-1 (duplicates are fine, an empty one chooses nobody).  Pure
    NumPy; raises ValueError on a bool array of another length, an index outside 0 .. B-1, or an index that is not an integer."""
    B = int(B)
    if scenes is None:
        return np.ones(B, dtype=np.uint8)
    a = np.asarray(scenes)
    if a.dtype == np.bool_:
        if a.shape != (B,):
            raise ValueError(f"a bool mask of shape {a.shape} for a batch of {B} scenes")
        return np.ascontiguousarray(a, dtype=np.uint8)
    a = a.reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"scene indices must be integers, got {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= B):
        raise ValueError(f"scene indices must lie in 0 .. {B - 1}, got {int(a.min())} .. {int(a.max())}")
    mask = np.zeros(B, dtype=np.uint8)
    mask[a.astype(np.int64)] = 1
    return mask


STEER_OFF, STEER_VELOCITY, STEER_PREFERRED = 0, 1, 2   # the kinds of a steered row (held as floats in the command buffer)
PTR_COMMANDS, PTR_STATE, PTR_ZSTATE = 0, 1, 2          # SFM_BATCH_PTR_*: what sfm_batch_device_ptr / SfmBatch.device_ptr select
PTR_EPISODES, PTR_DONE = 3, 4                          # ... the episode record [B][8] and the mask done[B] (while episodes are on)
PTR_SCAN = 5                                           # ... the scan record [N_total][2R] (while scans are on)
PTR_GRID = 7                                           # ... the grid record [M][6][G][G] (while grids are on; 6 is PTR_RESETS)
PTR_ROW_SCORES, PTR_SCENE_SCORES = 8, 9                # ... the row scores [N_total][4] and scene scores [B][5] (while observed tracks are on)


def _per_scene(v, so, width, name):
    """A list / tuple with one entry per scene, or one ndarray over the concatenated rows -> a float64 array of N_total rows
    (``width`` 0: flat values; else 2 or 3 columns, padded with zeros to 3).  One value (flat) or one (2|3,) vector stands for every
    row of its scene, or of the batch."""
    B, n = len(so) - 1, int(so[-1])

    def rows(e, nb, where):
        a = np.asarray(e, dtype=np.float64)
        if not width:
            a = np.broadcast_to(a, (nb,)) if a.ndim == 0 else a
            ok = a.ndim == 1 and a.shape[0] == nb
        else:
            if a.ndim == 1 and a.shape[0] in (2, 3):
                a = np.broadcast_to(a, (nb, a.shape[0]))
            if a.size == 0 and nb == 0:
                a = np.zeros((0, 3))
            ok = a.ndim == 2 and a.shape[0] == nb and a.shape[1] in (2, 3)
            if ok and a.shape[1] == 2:
                a = np.concatenate([a, np.zeros((nb, 1))], axis=1)
        if not ok:
            raise ValueError(f"{where}{name} of shape {a.shape} for {nb} rows")
        return a

    if isinstance(v, (list, tuple)):
        if len(v) != B:
            raise ValueError(f"{len(v)} entries of {name} for {B} scenes (a list is per scene; pass an ndarray for concatenated rows)")
        parts = [rows(np.zeros(3 if width else ()) if e is None else e, int(so[b + 1] - so[b]), f"scene {b}: ") for b, e in enumerate(v)]
        return np.concatenate(parts, axis=0)
    return rows(v, n, "")


def pack_steering(kinds, commands, scene_off):
    """Steering -> the arguments of sfm_batch_set_steering: (kind uint8 [N_total], ux, uy, uz float32 [N_total]).  ``kinds``: a list
    with one entry per scene (each (N_b,), or one value for the whole scene), or an ndarray (N_total,) over the concatenated rows, or
    one value for every row; 0 not steered, 1 velocity command, 2 preferred velocity.  ``commands``: a list with one entry per
    scene (each (N_b,2|3), one (2|3,) command for the whole scene, or None: zeros), or an ndarray (N_total,2|3), or None (zeros);
    two columns leave uz = 0.  ``kinds=None``: (None, ux, uy, uz), the commands alone.  Pure NumPy; raises ValueError on a shape that
    does not fit, a kind that is not 0, 1 or 2, and a command that is not finite in float32 on a steered row (with ``kinds=None``:
    on any row)."""
    so = np.asarray(scene_off)
    n = int(so[-1])
    kd = None
    if kinds is not None:
        k = _per_scene(kinds, so, 0, "kinds")
        if n and not np.isin(k, (0.0, 1.0, 2.0)).all():
            raise ValueError("kinds must hold 0 (not steered), 1 (velocity command) or 2 (preferred velocity)")
        kd = np.ascontiguousarray(k, dtype=np.uint8)
    c = np.zeros((n, 3)) if commands is None else _per_scene(commands, so, 3, "commands")
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.ascontiguousarray(c, dtype=np.float32)
    bad = ~np.isfinite(u).all(axis=1) & (np.ones(n, bool) if kd is None else kd != 0)
    if bad.any():
        raise ValueError(f"row {int(np.flatnonzero(bad)[0])}: the command of a steered row must be finite in float32")
    return kd, f32(u[:, 0]), f32(u[:, 1]), f32(u[:, 2])


DRIVE_OFF, DRIVE_VELOCITY, DRIVE_UNICYCLE = 0, 1, 2    # the kinds of a driven vehicle (held as floats in the vehicle command buffer)
PTR_VEHICLE_COMMANDS, PTR_VEHICLE_OBS = 10, 11         # ... the vehicle commands [M][4] (while driving is on) and the vehicle
                                                       # observations [M][16 + 4k] (while vehicle observations are on)


def _per_vehicle(v, item_off, width, name):
    """``_per_scene`` over the vehicles: a list / tuple with one entry per scene, or one ndarray over the M vehicles of all scenes, or
    one value (``width`` 0) / one (``width``,) vector for every vehicle -> a float64 array (M,) or (M, width)."""
    io = np.asarray(item_off)
    B, M = len(io) - 1, int(io[-1])

    def rows(e, nb, where):
        a = np.asarray(e, dtype=np.float64)
        if a.ndim == (1 if width else 0) and (not width or a.shape[0] == width):
            a = np.broadcast_to(a, (nb, width) if width else (nb,))
        if a.size == 0 and nb == 0:
            a = np.zeros((0, width) if width else (0,))
        if a.shape != ((nb, width) if width else (nb,)):
            raise ValueError(f"{where}{name} of shape {a.shape} for {nb} vehicles")
        return a

    if isinstance(v, (list, tuple)):
        if len(v) != B:
            raise ValueError(f"{len(v)} entries of {name} for {B} scenes (a list is per scene; pass an ndarray for all vehicles)")
        parts = [rows(np.zeros(width if width else ()) if e is None else e, int(io[b + 1] - io[b]), f"scene {b}: ") for b, e in enumerate(v)]
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, width) if width else (0,))
    return rows(v, M, "")


def pack_vehicle_driving(kinds, commands, item_off):
    """Driving -> the arguments of sfm_batch_set_vehicle_driving: (kind uint8 [M], a, b, c float32 [M]).  ``item_off`` (B+1,): the
    vehicles' scene offsets (``pack_boxes(...)[0]``).  ``kinds``: a list with one entry per scene (each (M_b,), or one value for the
    scene's vehicles), or an ndarray (M,) over the vehicles of all scenes, or one value for every vehicle; 0 not driven, 1 velocity
    (a, b) = v', 2 unicycle (a, b, c) = (signed speed, cos, sin of the tick's turn).  ``commands``: likewise with (M_b, 3) / (3,)
    entries, or None (zeros).  ``kinds=None``: (None, a, b, c), the commands alone.  Pure NumPy; raises ValueError on a shape that
    does not fit, a kind that is not 0, 1 or 2, and a command that is not finite in float32 on a driven vehicle (with
    ``kinds=None``: on any vehicle)."""
    io = np.asarray(item_off)
    M = int(io[-1])
    kd = None
    if kinds is not None:
        k = _per_vehicle(kinds, io, 0, "kinds")
        if M and not np.isin(k, (0.0, 1.0, 2.0)).all():
            raise ValueError("kinds must hold 0 (not driven), 1 (velocity) or 2 (unicycle)")
        kd = np.ascontiguousarray(k, dtype=np.uint8)
    c = np.zeros((M, 3)) if commands is None else _per_vehicle(commands, io, 3, "commands")
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.ascontiguousarray(c, dtype=np.float32)
    bad = ~np.isfinite(u).all(axis=1) & (np.ones(M, bool) if kd is None else kd != 0)
    if bad.any():
        raise ValueError(f"vehicle {int(np.flatnonzero(bad)[0])}: the command of a driven vehicle must be finite in float32")
    return kd, f32(u[:, 0]), f32(u[:, 1]), f32(u[:, 2])


def vehicle_observation_arrays(item_off, k, sense_range, frame=0, goals=None, mask=None):
    """Vehicle observation settings -> the arguments of sfm_batch_set_vehicle_observation: (k int, sense_range float32 [B], frame
    int, goal_x, goal_y float32 [M] or None, mask uint8 [M] or None).  ``sense_range`` as for ``observation_arrays``; ``goals``: None
    (zeros) or, as for ``pack_vehicle_driving``, (M_b, 2) per scene / (M, 2) / one (2,) goal, finite in float32; ``mask``: None (every
    vehicle) or bools likewise.  Pure NumPy; raises ValueError on what the library would refuse."""
    io = np.asarray(item_off)
    obs_width(k)
    frame = check_frame(frame)
    r = per_scene_metres(sense_range, "sense_range", len(io) - 1, True)
    gx = gy = None
    if goals is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            g = np.ascontiguousarray(_per_vehicle(goals, io, 2, "goals"), dtype=np.float32)
        if not np.isfinite(g).all():
            raise ValueError("goals must be finite in float32")
        gx, gy = f32(g[:, 0]), f32(g[:, 1])
    mk = None if mask is None else np.ascontiguousarray(_per_vehicle(mask, io, 0, "mask") != 0, dtype=np.uint8)
    return int(k), r, frame, gx, gy, mk


PTR_VEHICLE_SCAN = 12            # SFM_BATCH_PTR_VEHICLE_SCAN: the vehicle scan record [M][2R] (while the vehicle scan is on)


def vehicle_scan_arrays(item_off, max_range, ped_radius, point_radius=_scan.POINT_RADIUS, frame=0, mask=None, mount=(0.0, 0.0)):
    """Vehicle scan settings -> the arguments of sfm_batch_set_vehicle_scan behind the directions: (max_range, ped_radius,
    point_radius float32 [B], mask uint8 [M] or None, frame int, mount_x, mount_y float32).  The three lengths as for
    ``scan.scan_arrays``; ``mask``: None (every vehicle) or bools as for ``vehicle_observation_arrays``; ``mount``: the sensor's (x, y)
    in the vehicle frame, metres, x forward.  Pure NumPy; raises ValueError on what the library would refuse."""
    io = np.asarray(item_off)
    rm, rp, rq, frame = _scan.scan_arrays(len(io) - 1, max_range, ped_radius, point_radius, frame)
    mx, my = _scan.check_mount(mount)
    mk = None if mask is None else np.ascontiguousarray(_per_vehicle(mask, io, 0, "mask") != 0, dtype=np.uint8)
    return rm, rp, rq, mk, frame, mx, my


PTR_RESETS = 6                   # SFM_BATCH_PTR_RESETS: the restart counters [B] uint32 (while restart noise is on)
MAX_RESTART_TRIES = 32           # SFM_BATCH_MAX_RESTART_TRIES


def pack_restart_noise(seeds, pos_box, scene_off, goal_box=None, min_gap=0.0, point_gap=0.0, tries=8, track_delay=None, vehicles=None):
    """Restart noise -> the arguments of sfm_batch_set_restart_noise: (seeds uint32 [B], pos_hx, pos_hy float32 [N_total], goal_hx,
    goal_hy float32 [N_total] or None, min_gap, point_gap float32 [B], tries int, track_delay int32 [M] or None).  ``seeds``: a
    scalar (broadcast to every scene) or B integers 0 .. 2^32-1.  ``pos_box`` / ``goal_box``: half-extents (hx, hy) in metres -- a
    list with one entry per scene (each (N_b,2), or one (2,) pair for the whole scene), or an ndarray (N_total,2), or one (2,) pair
    for every row; finite, >= 0 and <= 1e6 in float32; ``goal_box=None``: the goals stay.  ``min_gap`` / ``point_gap``: a scalar or B
    values in metres, finite, >= 0 and <= 1e6.  ``tries``: an integer 1 .. 32.  ``track_delay``: None, or ``vehicles`` (M) integers
    0 .. 2^31-1, one per device-side vehicle in scene order (a scalar is broadcast).  Pure NumPy; raises ValueError on a shape that
    does not fit and on every value the library would refuse."""
    so = np.asarray(scene_off)
    B, n = len(so) - 1, int(so[-1])
    sd = per_scene(seeds, "seeds", B, "iu")
    if (sd < 0).any() or (sd > 0xFFFFFFFF).any():
        raise ValueError("seeds must be integers 0 .. 2^32-1")
    if isinstance(tries, (bool, np.bool_)) or not isinstance(tries, (int, np.integer)) or not 1 <= int(tries) <= MAX_RESTART_TRIES:
        raise ValueError(f"tries must be an integer 1 .. {MAX_RESTART_TRIES}, got {tries!r}")

    def box(v, name):
        a = _per_scene(v, so, 3, name)
        if a.shape[0] and a[:, 2].any():
            raise ValueError(f"{name} must hold two half-extents (hx, hy) per row")
        with np.errstate(over="ignore", invalid="ignore"):
            h = np.ascontiguousarray(a[:, :2], dtype=np.float32)
        if not (np.isfinite(h).all() and (h >= 0).all() and (h <= np.float32(MAX_SENSE_RANGE)).all()):
            raise ValueError(f"{name} must be finite, >= 0 and <= {MAX_SENSE_RANGE:g} metres")
        return f32(h[:, 0]), f32(h[:, 1])

    phx, phy = box(pos_box, "pos_box")
    ghx, ghy = (None, None) if goal_box is None else box(goal_box, "goal_box")
    gaps = [per_scene_metres(v, name, B, False) for v, name in ((min_gap, "min_gap"), (point_gap, "point_gap"))]
    delay = None
    if track_delay is not None:
        if vehicles is None:
            raise ValueError("track_delay needs the number of device-side vehicles (vehicles=M)")
        d = per_scene(track_delay, "track_delay", int(vehicles), "iu").astype(np.int64)
        if (d < 0).any() or (d >= 2**31).any():
            raise ValueError("track_delay must be >= 0 and fit int32")
        delay = np.ascontiguousarray(d, dtype=np.int32)
    return np.ascontiguousarray(sd, dtype=np.uint32), phx, phy, ghx, ghy, gaps[0], gaps[1], int(tries), delay


OBS_HEADER = 16                  # SFM_BATCH_OBS_HEADER: floats of a row's record in front of its neighbour slots
MAX_OBS_NEIGHBOURS = 16          # SFM_BATCH_MAX_OBS_NEIGHBOURS


def obs_width(k):
    """Floats of one row's observation record with ``k`` neighbour slots: OBS_HEADER + 4 k.  Raises ValueError outside 1 .. 16."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_OBS_NEIGHBOURS:
        raise ValueError(f"k must be an integer 1 .. {MAX_OBS_NEIGHBOURS} (neighbour slots per row), got {k!r}")
    return OBS_HEADER + 4 * int(k)


def observation_arrays(B, k, sense_range, frame=0):
    """Observation settings -> the arguments of sfm_batch_set_observation: (k int, sense_range float32 [B], frame int).
    ``sense_range`` is a scalar (broadcast to every scene, like ``stream_arrays``) or B values, in metres: finite, > 0 and <= 1e6
    in float32.  Pure NumPy; raises ValueError on a k outside 1 .. 16, a frame other than 0 or 1, and a range the library would
    refuse."""
    obs_width(k)
    frame = check_frame(frame)
    return int(k), per_scene_metres(sense_range, "sense_range", int(B), True), frame


def _split_rows(scene_off, *cols):
    """Arrays over the concatenated rows -> per scene, in scene order, its rows of each (views): a list of B arrays for one array,
    of B tuples for several."""
    so = scene_off
    if len(cols) == 1:
        return [cols[0][so[b]:so[b + 1]] for b in range(len(so) - 1)]
    return [tuple(c[so[b]:so[b + 1]] for c in cols) for b in range(len(so) - 1)]


def split_observations(buf, scene_off):
    """Observations of the concatenated batch, (N_total, W), -> a list of B arrays (N_b, W), one per scene in scene order
    (views).  Pure NumPy."""
    so = np.asarray(scene_off)
    buf = np.asarray(buf)
    if buf.ndim != 2 or buf.shape[0] != int(so[-1]):
        raise ValueError(f"observations of shape {buf.shape} for {int(so[-1])} pedestrians")
    return _split_rows(so, buf)


EPISODE_WIDTH = 8                # SFM_BATCH_EPISODE_WIDTH: floats of a scene's episode record
EP_DONE, EP_REASON, EP_AGE, EP_GOAL_D2, EP_PREV_GOAL_D2, EP_PED_D2, EP_VEH_D2, EP_WALL_D2 = range(8)     # its slots
REASON_ARRIVED, REASON_TIME_LIMIT, REASON_PED_HIT, REASON_VEH_HIT, REASON_NOT_LIVE = 1, 2, 4, 8, 16     # SFM_EPISODE_*: bits of slot 1
END_STEP_AUTO_RESTART = 1        # SFM_END_STEP_AUTO_RESTART


def episode_arrays(B, agent, goal_radius=0.0, ped_radius=0.0, veh_radius=0.0, max_steps=0):
    """Episode settings -> the arguments of sfm_batch_set_episodes: (agent int32 [B], goal_radius, ped_radius, veh_radius float32
    [B], max_steps int32 [B]).  Each argument is a scalar (broadcast to every scene, like ``stream_arrays``) or B values.  ``agent``:
    integers >= -1 (-1: the scene has no agent; the upper bound N_b is the library's to check, or ``SfmBatch.set_episodes``');
    radii in metres, finite, >= 0 and <= 1e6 in float32 (0: the test is off); ``max_steps`` integers >= 0 (0: no time limit).  Pure
    NumPy; raises ValueError on a shape that does not fit and on every value the library would refuse."""
    B = int(B)
    ag = per_scene(agent, "agent", B, "iu").astype(np.int64)
    if (ag < -1).any() or (ag >= MAX_SCENE_PEDESTRIANS).any():
        raise ValueError(f"agent must be -1 (no agent) or a row 0 .. N_b-1 of its scene, got {int(ag.min())} .. {int(ag.max())}")
    radii = [per_scene_metres(v, name, B, False)
             for v, name in ((goal_radius, "goal_radius"), (ped_radius, "ped_radius"), (veh_radius, "veh_radius"))]
    ms = per_scene(max_steps, "max_steps", B, "iu").astype(np.int64)
    if (ms < 0).any() or (ms >= 2**31).any():
        raise ValueError("max_steps must be >= 0 (0: no time limit) and fit int32")
    return (np.ascontiguousarray(ag, dtype=np.int32), *radii, np.ascontiguousarray(ms, dtype=np.int32))


class _DeviceSpan:
    """Minimal __cuda_array_interface__ carrier so torch can alias a raw device pointer (no copy), as stepper._DevSpan."""

    def __init__(self, ptr, shape, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(int(d) for d in shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def split_frames(frames, scene_off):
    """Frames of the concatenated batch, (F, N_total, C), -> a list of B arrays (F, N_b, C), one per scene in scene order (views).
    Pure NumPy."""
    so = np.asarray(scene_off)
    if frames.ndim != 3 or frames.shape[1] != int(so[-1]):
        raise ValueError(f"frames of shape {frames.shape} for {int(so[-1])} pedestrians")
    return [frames[:, so[b]:so[b + 1]] for b in range(len(so) - 1)]


def _record_names(names):
    """Force names (None = all six) -> the selected names in index order; ValueError on an unknown or empty selection."""
    if names is None:
        return FORCE_RECORD_NAMES
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in FORCE_RECORD_NAMES]
    if bad or not names:
        raise ValueError(f"forces must be a non-empty selection of {FORCE_RECORD_NAMES}, got {names}")
    return tuple(n for n in FORCE_RECORD_NAMES if n in names)


def force_mask(names=None):
    """Force names (an iterable of FORCE_RECORD_NAMES, or one name; None = all six) -> the force_mask of sfm_batch_tick_forces /
    sfm_batch_run_recorded_forces: bit k for FORCE_RECORD_NAMES[k].  Pure NumPy; raises ValueError."""
    return sum(1 << FORCE_RECORD_NAMES.index(n) for n in _record_names(names))


def split_forces(buf, scene_off, names=None):
    """A force record of the concatenated batch, (..., K, N_total, C) with the K forces of ``names`` in index order, -> a list of B
    dicts name -> (..., N_b, C), one per scene in scene order (views).  Pure NumPy."""
    names = _record_names(names)
    so = np.asarray(scene_off)
    buf = np.asarray(buf)
    if buf.ndim < 3 or buf.shape[-3] != len(names) or buf.shape[-2] != int(so[-1]):
        raise ValueError(f"a force record of shape {buf.shape} for {len(names)} forces of {int(so[-1])} pedestrians")
    return [{n: buf[..., k, so[b]:so[b + 1], :] for k, n in enumerate(names)} for b in range(len(so) - 1)]


def record_bytes(n_total, frames, planar, forces=None, zframes=False):
    """Bytes one run_recorded_forces call records (frames, zframes and forces together; the library refuses more than
    MAX_RECORD_BYTES).  ``forces`` as for force_mask."""
    C_ = 2 if planar else 3
    per_row = 16 + (8 if zframes else 0) + 4 * C_ * len(_record_names(forces))
    return int(n_total) * int(frames) * per_row


def n_frames(ticks, stride, max_frames=None):
    """Frames a recorded run of ``ticks`` ticks keeps: min(max_frames, ceil(ticks / stride)) (0 for invalid arguments, which the
    library refuses)."""
    if ticks <= 0 or stride <= 0:
        return 0
    f = (ticks + stride - 1) // stride
    return f if max_frames is None else max(0, min(f, max_frames))


class SfmBatch:
    """B independent scenes on one GPU, one launch per tick.  Raises SfmLibraryError on any failure; never falls back to the CPU."""

    def __init__(self, configs, step_lengths, device=0, honour_file_keys=False, B=None):
        self._lib = _lib.load()
        self._b = C.c_void_p()
        self.params = batch_params(configs, step_lengths, B, honour_file_keys)
        self.B = len(self.params)
        rc = self._lib.sfm_batch_create(self.B, self.params, int(device), C.byref(self._b))
        if rc != 0:
            msg = self._lib.sfm_batch_last_error(None)
            self._b = C.c_void_p()
            raise SfmLibraryError(f"sfm_batch_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.scene_off = None
        self.planar = True
        self._z = None
        self._dyn = None                  # (scene_item_off, offsets) of the vehicles last set, for dynamic_obstacles()
        self.has_snapshot = False         # snapshot() has been taken and no later call has dropped it
        self.obs_k = None                 # neighbour slots of set_observation (None: observations are off)
        self.has_episodes = False         # set_episodes has been called and no later call has dropped it
        self.scan_rays = None             # rays per row of set_scan (None: scans are off)
        self.grid_cells = None            # cells per side of set_grid (None: grids are off)
        self._grid_rows = self._grid_counts = None
        self.has_restart_noise = False    # set_restart_noise has been called and no later call has dropped it
        self.observed_every = None        # ticks per observed frame of set_observed (None: observed tracks are off)
        self._boxes = False               # the vehicles last set move on the device (set_dynamic_boxes with at least one vehicle)
        self.driving = False              # set_vehicle_driving has been called and no later call has dropped it
        self.vobs_k = None                # pedestrian slots of set_vehicle_observation (None: vehicle observations are off)
        self.vscan_rays = None            # rays per vehicle of set_vehicle_scan (None: the vehicle scan is off)

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.sfm_batch_last_error(self._b)
            raise SfmLibraryError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")

    def _need_upload(self, name):
        if self.scene_off is None:
            raise SfmLibraryError(f"SfmBatch.{name}: upload() has not been called")

    def _alias(self, ptr, shape, device, typestr="<f4"):
        """A device buffer as a torch tensor of ``shape`` that aliases it (no copy); ``ptr`` 0 (no rows): an empty float32 tensor."""
        import torch
        dev = f"cuda:{torch.cuda.current_device() if device is None else int(device)}"
        if not ptr:
            return torch.zeros((0,) + tuple(shape[1:]), dtype=torch.float32, device=dev)
        return torch.as_tensor(_DeviceSpan(ptr, shape, typestr), device=dev)

    def _check_drops(self, rc, what):
        """``_check`` for the calls that drop the snapshot once they succeed (a refused call drops nothing)."""
        self._check(rc, what)
        self.has_snapshot = False

    def close(self):
        if getattr(self, "_b", None) is not None and self._b:
            self._lib.sfm_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self._check(self._lib.sfm_batch_set_stream(self._b, C.c_void_p(int(stream_ptr))), "sfm_batch_set_stream")

    def set_params(self, configs, step_lengths, honour_file_keys=False):
        params = batch_params(configs, step_lengths, self.B, honour_file_keys)
        self._check(self._lib.sfm_batch_set_params(self._b, params), "sfm_batch_set_params")
        self.params = params

    def upload(self, scenes, planar=None, device_vehicles=False):
        """State and geometry of every scene (a list of B scene dicts).  ``planar`` None = pack_scenes' decision.
        ``device_vehicles``: False -- the vehicles' rings as given, which stay where they are (sfm_batch_set_dynamic_obstacles);
        True -- the vehicles as boxes that move on the device (``set_dynamic_boxes``)."""
        scenes = list(scenes)
        if len(scenes) != self.B:
            raise ValueError(f"{len(scenes)} scenes for a batch of {self.B}")
        boxes = pack_boxes(scenes) if device_vehicles else None     # (malformed boxes are refused before anything is sent)
        self.upload_packed(pack_scenes(scenes), planar)
        if boxes is not None:
            self.set_dynamic_boxes(boxes)

    def upload_packed(self, pk, planar=None):
        """``upload`` from the output of ``pack_scenes`` (pack once, upload many times)."""
        planar = pk["planar"] if planar is None else bool(planar)
        L = self._lib
        so = pk["scene_off"]
        if len(so) != self.B + 1:
            raise ValueError(f"packed scenes hold {len(so) - 1} scenes, the batch {self.B}")
        bo, st, dy = pk["borders"], pk["static"], pk["dynamic"]
        self._check(L.sfm_batch_set_borders(self._b, *(iptr(a) for a in bo[:2]), *(fptr(a) for a in bo[2:])), "sfm_batch_set_borders")
        self._check(L.sfm_batch_set_static_obstacles(self._b, *(iptr(a) for a in st[:2]), *(fptr(a) for a in st[2:])),
                    "sfm_batch_set_static_obstacles")
        self._check_drops(L.sfm_batch_set_dynamic_obstacles(self._b, *(iptr(a) for a in dy[:2]), *(fptr(a) for a in dy[2:])),
                          "sfm_batch_set_dynamic_obstacles")
        self._dyn = (dy[0].copy(), dy[1].copy())
        self._boxes, self.driving, self.vobs_k = False, False, None    # (the vehicles were replaced: driving and their observations go)
        self.vscan_rays = None            # ... and their scans
        z, vz =(None, None) if planar else (pk["z"], pk["vz"])
        self._check_drops(L.sfm_batch_upload_state(self._b, iptr(so), fptr(pk["x"]), fptr(pk["y"]), fptr(z), fptr(pk["vx"]),
                                                   fptr(pk["vy"]), fptr(vz), fptr(pk["wx"]), fptr(pk["wy"]),
                                                   fptr(pk["target_speed"]), fptr(pk["radius"]), u8ptr(pk["crossing"])),
                          "sfm_batch_upload_state")
        self.scene_off = so.copy()
        self.obs_k = None                 # (the upload dropped the observations with the rows)
        self.has_episodes = False         # ... and the episodes
        self.scan_rays = None             # ... and the scans
        self.grid_cells = None            # ... and the grids
        self._grid_rows = self._grid_counts = None
        self.has_restart_noise = False    # ... and the restart noise
        self.observed_every = None        # ... and the observed tracks
        self.planar = planar
        self._z = pk["z"].copy()          # a planar batch keeps each scene's z on the host (the device holds x / y only)

    def set_dynamic_boxes(self, scenes):
        """Vehicles of every scene as oriented boxes that move on the device: a list of B scene dicts (see ``pack_boxes``) or the
        tuple ``pack_boxes`` returns.  Replaces the scenes' vehicles; scenes without vehicles clear them."""
        boxes = scenes if isinstance(scenes, tuple) else pack_boxes(scenes)
        if len(boxes[0]) != self.B + 1:
            raise ValueError(f"boxes of {len(boxes[0]) - 1} scenes for a batch of {self.B}")
        self._check_drops(self._lib.sfm_batch_set_dynamic_boxes(self._b, *(iptr(a) for a in boxes[:2]),
                                                                *(fptr(a) for a in boxes[2:])), "sfm_batch_set_dynamic_boxes")
        self._dyn = (boxes[0].copy(), boxes[1].copy())
        self._boxes, self.driving, self.vobs_k = int(boxes[0][-1]) > 0, False, None    # (new vehicles: driving and their observations go)
        self.vscan_rays = None            # ... and their scans

    def dynamic_obstacles(self):
        """Per scene, its vehicles as the next tick sees them: a list of (center (2,), ring (P,2)) float64 like
        ``SfmEngine.dynamic_obstacles()``."""
        if self._dyn is None:
            return [[] for _ in range(self.B)]
        item_off, off = self._dyn
        M, P = int(item_off[-1]), int(off[-1])
        cx, cy, px, py = (np.zeros(n, np.float32) for n in (M, M, P, P))
        self._check(self._lib.sfm_batch_download_dynamic_obstacles(self._b, fptr(cx), fptr(cy), fptr(px), fptr(py)),
                    "sfm_batch_download_dynamic_obstacles")
        pts = np.stack([px, py], axis=1).astype(np.float64)
        veh = [(np.array([cx[k], cy[k]], dtype=np.float64), pts[off[k]:off[k + 1]]) for k in range(M)]
        return [veh[item_off[b]:item_off[b + 1]] for b in range(self.B)]

    def set_vehicle_tracks(self, tracks):
        """Scripted tracks for the device-side vehicles (sfm_batch_set_vehicle_tracks): ``tracks`` per scene ``None`` or one entry
        per vehicle (see ``pack_tracks``), or the dict ``pack_tracks`` returns.  Needs ``upload(..., device_vehicles=True)`` or
        ``set_dynamic_boxes`` first.  The tracked vehicles are placed for tick 0 at once; ``upload``, ``set_dynamic_boxes`` and
        ``sfm_batch_set_dynamic_obstacles`` drop the tracks, ``set_params``, ``set_modes`` and ``set_spawns`` keep them, setting
        them again restarts the tick counter.  ``tracks=None`` switches them off (the vehicles run free from where they are)."""
        L = self._lib
        if tracks is None:
            self._check_drops(L.sfm_batch_set_vehicle_tracks(self._b, *([None] * 8)), "sfm_batch_set_vehicle_tracks")
            return
        if self._dyn is None:
            raise SfmLibraryError("SfmBatch.set_vehicle_tracks: upload() has not been called")
        pt = tracks if isinstance(tracks, dict) else pack_tracks(tracks, self._dyn[0])
        if len(pt["trk_off"]) != int(self._dyn[0][-1]) + 1:
            raise ValueError(f"tracks of {len(pt['trk_off']) - 1} vehicles for a batch of {int(self._dyn[0][-1])}")
        T = int(pt["trk_off"][-1])
        keys = [fptr(pt[k]) if T else None for k in ("kx", "ky", "kvx", "kvy", "kcos", "ksin")]
        self._check_drops(L.sfm_batch_set_vehicle_tracks(self._b, iptr(pt["trk_off"]),
                                                         iptr(pt["first_tick"]) if len(pt["first_tick"]) else None, *keys),
                          "sfm_batch_set_vehicle_tracks")

    def vehicle_tracks(self):
        """(tick, present): the integrating ticks since ``set_vehicle_tracks`` and, per scene, a bool array (M_b,) -- does the next
        integrating tick see the vehicle (an untracked one is always there)?  Raises SfmLibraryError while no tracks are set."""
        item_off = self._dyn[0] if self._dyn is not None else np.zeros(self.B + 1, np.int32)
        pres = np.zeros(max(int(item_off[-1]), 1), np.uint8)
        tick = C.c_int64(0)
        self._check(self._lib.sfm_batch_download_vehicle_tracks(self._b, C.byref(tick), u8ptr(pres)),
                    "sfm_batch_download_vehicle_tracks")
        return int(tick.value), [pres[item_off[b]:item_off[b + 1]].astype(bool) for b in range(self.B)]

    def snapshot(self):
        """Record every scene as it is now (sfm_batch_snapshot): device-to-device copies on the batch's stream of everything a tick
        can change; the host does not wait.  A second snapshot replaces the first.  ``upload``, ``set_dynamic_boxes``,
        ``set_modes``, ``set_spawns`` and ``set_vehicle_tracks`` (``None`` included) drop it; ``set_params`` and
        ``set_waypoint_streams`` keep it."""
        self.has_snapshot = False
        self._check(self._lib.sfm_batch_snapshot(self._b), "sfm_batch_snapshot")
        self.has_snapshot = True

    def restart(self, scenes=None):
        """Put the chosen scenes back to the snapshot with one launch (sfm_batch_restart); the others are not touched.  ``scenes``
        as for ``restart_mask``: None (every scene), a bool array (B,), or scene indices.  A restarted scene runs under the
        parameters and static geometry of the moment; its tracked vehicles are where they were at the snapshot."""
        mask = None if scenes is None else restart_mask(self.B, scenes)
        self._check(self._lib.sfm_batch_restart(self._b, u8ptr(mask)), "sfm_batch_restart")

    def restart_device(self, mask=None):
        """``restart`` with its mask on the device (sfm_batch_restart_device): one launch, no copy, no wait.  ``mask``: None -- the
        batch's own ``done`` as the last ``end_step`` left it; or a torch tensor of B one-byte elements (bool, uint8 or int8) on the
        batch's device, contiguous, nonzero = restart.  Put torch and the batch on one stream so that the mask's writer and the
        launch are ordered; keep the tensor alive until the launch has run."""
        if mask is None:
            ptr, _ = self.device_ptr(PTR_DONE)
        else:
            import torch
            if not isinstance(mask, torch.Tensor):
                raise ValueError("restart_device takes a torch tensor on the device (or None: the batch's done); a host mask goes to restart()")
            if not mask.is_cuda:
                raise ValueError("the mask of restart_device must be on the device (a host mask goes to restart())")
            if mask.element_size() != 1 or mask.dtype not in (torch.bool, torch.uint8, torch.int8):
                raise ValueError(f"the mask of restart_device must be bool, uint8 or int8, got {mask.dtype}")
            if mask.numel() != self.B or not mask.is_contiguous():
                raise ValueError(f"the mask of restart_device must hold {self.B} contiguous elements, got shape {tuple(mask.shape)}"
                                 f"{'' if mask.is_contiguous() else ' (not contiguous)'}")
            ptr = mask.data_ptr()
        self._check(self._lib.sfm_batch_restart_device(self._b, C.c_void_p(ptr or None)), "sfm_batch_restart_device")

    def set_restart_noise(self, seeds, pos_box, goal_box=None, min_gap=0.0, point_gap=0.0, tries=8, track_delay=None):
        """How a restarted scene may differ from the snapshot (sfm_batch_set_restart_noise; see ``pack_restart_noise`` and the
        module docstring): every restart -- ``restart``, ``restart_device``, ``end_step(auto_restart=True)`` -- is followed by one
        more launch that draws each row's start from the box ``pos_box`` around its snapshot position, again (up to ``tries``
        times) while it is nearer than ``min_gap`` to a row that is placed or to a lower-index proposal, or nearer than
        ``point_gap`` to a point of the scene's geometry; draws each live row's goal from ``goal_box`` around the snapshot goal;
        and lets a tracked vehicle arrive up to ``track_delay`` ticks later.  Keyed by the scene's seed and its restart counter:
        reproducible, and the same alone or in any batch (``reset.resample_scene`` is the host twin).  ``pos_box=None`` switches it
        off.  Needs ``upload`` first, which also drops it; every other call keeps it (the delays go with the tracks), and it
        keeps the snapshot.  Zeroes the counters (``reset_count_tensor()`` must be taken again)."""
        L = self._lib
        if pos_box is None:
            self._check(L.sfm_batch_set_restart_noise(self._b, *([None] * 7), 0, None), "sfm_batch_set_restart_noise")
            self.has_restart_noise = False
            return
        self._need_upload("set_restart_noise")
        M = int(self._dyn[0][-1]) if self._dyn is not None else 0
        sd, phx, phy, ghx, ghy, g1, g2, tries, delay = pack_restart_noise(seeds, pos_box, self.scene_off, goal_box, min_gap, point_gap,
                                                                           tries, track_delay, M)
        if phx.shape[0] == 0:                                          # (no rows: the library takes any non-NULL pointer)
            phx = phy = np.zeros(1, np.float32)
            ghx = ghy = None if ghx is None else np.zeros(1, np.float32)
        if delay is not None and delay.shape[0] == 0:
            delay = np.zeros(1, np.int32)
        self._check(L.sfm_batch_set_restart_noise(self._b, sd.ctypes.data, fptr(phx), fptr(phy), fptr(ghx), fptr(ghy), fptr(g1), fptr(g2),
                                                  tries, iptr(delay)), "sfm_batch_set_restart_noise")
        self.has_restart_noise = True

    def restart_noise(self):
        """(resets (B,) uint32, fallbacks (B,) uint32): how often each scene has restarted since ``set_restart_noise``, and how many
        rows of its latest restart no try could place (they start at their snapshot position).  Synchronises the batch's stream;
        raises SfmLibraryError while restart noise is off."""
        resets, fallbacks = np.zeros(self.B, np.uint32), np.zeros(self.B, np.uint32)
        self._check(self._lib.sfm_batch_download_restart_noise(self._b, resets.ctypes.data, fallbacks.ctypes.data),
                    "sfm_batch_download_restart_noise")
        return resets, fallbacks

    def reset_count_tensor(self, device=None):
        """``resets`` as a torch tensor (B,) that aliases device memory (no copy; int32 bits of the uint32 counters): the episode
        index a curriculum or a logger reads on the device.  Take it again after ``upload`` or ``set_restart_noise``.  Raises
        SfmLibraryError while restart noise is off."""
        if not self.has_restart_noise:
            raise SfmLibraryError("SfmBatch.reset_count_tensor: restart noise is off (set_restart_noise; upload drops it)")
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_device_ptr(self._b, PTR_RESETS, C.byref(nbytes))
        if not ptr:
            self._check(-1, "sfm_batch_device_ptr")
        return self._alias(ptr, (self.B,), device, "<i4")

    def set_episodes(self, agent, goal_radius=0.0, ped_radius=0.0, veh_radius=0.0, max_steps=0):
        """Which row of every scene is its agent and what ends its episode (sfm_batch_set_episodes; see ``episode_arrays`` and the
        module docstring).  ``agent=None`` switches episodes off and frees the buffers.  Needs ``upload`` first, which also drops
        them; every other call keeps them, and they keep the snapshot.  Allocates and fills the record, the mask and the episode
        state (``episode_tensor()`` / ``done_tensor()`` must be taken again)."""
        L = self._lib
        if agent is None:
            self._check(L.sfm_batch_set_episodes(self._b, None, None, None, None, None), "sfm_batch_set_episodes")
            self.has_episodes = False
            return
        self._need_upload("set_episodes")
        ag, rg, rp, rv, ms = episode_arrays(self.B, agent, goal_radius, ped_radius, veh_radius, max_steps)
        n = np.diff(self.scene_off)
        if (ag >= n).any():
            k = int(np.flatnonzero(ag >= n)[0])
            raise ValueError(f"scene {k}: agent {int(ag[k])} is no row of a scene of {int(n[k])} pedestrians")
        self._check(L.sfm_batch_set_episodes(self._b, iptr(ag), fptr(rg), fptr(rp), fptr(rv), iptr(ms)), "sfm_batch_set_episodes")
        self.has_episodes = True

    def end_step(self, auto_restart=False):
        """Decide whose episode is over (sfm_batch_end_step): one launch on the batch's stream fills the record and ``done``; the
        host does not wait.  ``auto_restart=True``: a second launch restarts the scenes that are done from the snapshot
        (``restart_device()``), the record keeping the terminal values.  Raises SfmLibraryError while episodes are off and, with
        ``auto_restart``, while there is no snapshot."""
        self._check(self._lib.sfm_batch_end_step(self._b, END_STEP_AUTO_RESTART if auto_restart else 0), "sfm_batch_end_step")

    def episodes(self):
        """(record (B, 8) float32, done (B,) bool) as the last ``end_step`` left them (synchronises the batch's stream)."""
        rec, done = np.zeros((self.B, EPISODE_WIDTH), np.float32), np.zeros(self.B, np.uint8)
        self._check(self._lib.sfm_batch_download_episodes(self._b, fptr(rec), u8ptr(done)), "sfm_batch_download_episodes")
        return rec, done.astype(bool)

    def episode_tensor(self, device=None):
        """The episode record as a torch tensor (B, 8) float32 that aliases device memory (no copy): what a reward reads after
        ``end_step()``.  Put torch and the batch on one stream.  Take it again after ``upload`` or ``set_episodes``.  Raises
        SfmLibraryError while episodes are off."""
        return self._alias(self.device_ptr(PTR_EPISODES)[0], (self.B, EPISODE_WIDTH), device)

    def done_tensor(self, device=None):
        """The mask ``done`` as a torch tensor (B,) uint8 (0 / 1) that aliases device memory: what ``restart_device`` takes."""
        return self._alias(self.device_ptr(PTR_DONE)[0], (self.B,), device, "|u1")

    def set_steering(self, kinds, commands=None):
        """Which rows the caller steers, and their first commands (sfm_batch_set_steering; see ``pack_steering``): kind 1 rows take
        the command as their new velocity, kind 2 rows as their preferred velocity.  ``kinds=None`` switches steering off.  Needs
        ``upload`` first, which also drops it; every other call keeps it, and it keeps the snapshot.  Reallocates the command buffer
        (``command_tensor()`` must be taken again)."""
        L = self._lib
        if kinds is None:
            self._check(L.sfm_batch_set_steering(self._b, None, None, None, None), "sfm_batch_set_steering")
            self.observed_every = None                                 # (observed tracks are replayed through the commands)
            return
        self._need_upload("set_steering")
        kd, ux, uy, uz = pack_steering(kinds, commands, self.scene_off)
        if kd.shape[0] == 0:                                           # (no rows: still a call, so that steering is on)
            kd, ux, uy, uz = np.zeros(1, np.uint8), np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
        self._check(L.sfm_batch_set_steering(self._b, u8ptr(kd), fptr(ux), fptr(uy), fptr(uz)), "sfm_batch_set_steering")

    def set_commands(self, commands):
        """New commands for every row, kinds as ``set_steering`` set them (sfm_batch_set_commands): one host-to-device copy on the
        batch's stream, no wait.  ``commands`` as for ``pack_steering``; rows that are not steered may hold anything finite or
        not -- they are validated by the library against the kinds it knows."""
        self._need_upload("set_commands")
        so = self.scene_off
        c = np.zeros((int(so[-1]), 3)) if commands is None else _per_scene(commands, so, 3, "commands")
        with np.errstate(over="ignore", invalid="ignore"):
            u = np.ascontiguousarray(c, dtype=np.float32)
        ux, uy, uz = f32(u[:, 0]), f32(u[:, 1]), f32(u[:, 2])
        if ux.shape[0] == 0:
            ux = uy = uz = np.zeros(1, np.float32)
        self._check(self._lib.sfm_batch_set_commands(self._b, fptr(ux), fptr(uy), fptr(uz)), "sfm_batch_set_commands")

    def steering(self):
        """Per scene (kind (N_b,) uint8, command (N_b,3) float32) as the next tick reads them, in scene order (synchronises the
        batch's stream).  Raises SfmLibraryError while steering is off."""
        n = int(self.scene_off[-1]) if self.scene_off is not None else 0
        kd = np.zeros(max(n, 1), np.uint8)
        u = [np.zeros(max(n, 1), np.float32) for _ in range(3)]
        self._check(self._lib.sfm_batch_download_steering(self._b, u8ptr(kd), *(fptr(a) for a in u)), "sfm_batch_download_steering")
        so = self.scene_off if self.scene_off is not None else np.zeros(self.B + 1, np.int32)
        return _split_rows(so, kd, np.stack(u, axis=1))

    def device_ptr(self, which):
        """(address, bytes) of a device buffer of the batch (sfm_batch_device_ptr): ``PTR_COMMANDS``, ``PTR_STATE``,
        ``PTR_ZSTATE`` ((0, 0) for a planar batch), ``PTR_EPISODES``, ``PTR_DONE``, ``PTR_SCAN`` or, while restart noise is on,
        ``PTR_RESETS``, or, while grids are on, ``PTR_GRID`` ((0, 0) without gridded rows).  Valid until the next ``upload`` (the
        command buffer: or ``set_steering``; the episode buffers: or ``set_episodes``; the scan buffer: or ``set_scan``; the
        restart counters: or ``set_restart_noise``; the grid buffer: or ``set_grid``)."""
        nbytes = C.c_int64(0)
        self._need_upload("device_ptr")
        ptr = self._lib.sfm_batch_device_ptr(self._b, int(which), C.byref(nbytes))
        if not ptr and which in (PTR_EPISODES, PTR_DONE):
            self._check(-1, "sfm_batch_device_ptr")                    # (episodes are off: the library's message)
        if not ptr and which == PTR_GRID and self.grid_cells is not None and len(self._grid_rows) == 0:
            return 0, 0                                                # (grids are on and no row is gridded: no buffer)
        if not ptr and int(self.scene_off[-1]) > 0 and not (which == PTR_ZSTATE and self.planar):
            self._check(-1, "sfm_batch_device_ptr")                    # (without rows, and {z, vz} of a planar batch: no buffer)
        return int(ptr or 0), int(nbytes.value)

    def _tensor(self, which, width, device):
        ptr, nbytes = self.device_ptr(which)
        return self._alias(ptr, (nbytes // (4 * width), width), device)

    def command_tensor(self, device=None):
        """The command buffer as a torch tensor (N_total, 4) float32 {ux, uy, uz, kind} that aliases device memory (no copy): what a
        policy writes.  Put torch and the batch on one stream (``set_stream(torch.cuda.current_stream().cuda_stream)``) so that
        writes and ticks are ordered.  What is written here is not validated: a kind other than 1 or 2 counts as 0, and a
        command that is not finite goes into the state.  ``set_commands`` sends the kinds of ``set_steering`` and so overwrites
        kinds changed here.  Take it again after ``upload`` or ``set_steering``."""
        return self._tensor(PTR_COMMANDS, 4, device)

    def state_tensor(self, device=None):
        """The state as a torch tensor (N_total, 4) float32 {x, y, vx, vy} that aliases device memory: what a policy reads, current
        once the batch's stream has run the ticks issued.  Take it again after ``upload``."""
        return self._tensor(PTR_STATE, 4, device)

    def zstate_tensor(self, device=None):
        """{z, vz} of a 3-D batch as a torch tensor (N_total, 2) float32 aliasing device memory; None for a planar batch."""
        if self.planar:
            return None
        return self._tensor(PTR_ZSTATE, 2, device)

    def set_observation(self, k, sense_range=None, frame=0):
        """What ``observe`` computes (sfm_batch_set_observation; see ``observation_arrays`` and the module docstring): ``k``
        neighbour slots per row, a sense range in metres (one value, or one per scene), world axes (``frame=0``) or the row's
        heading frame (``frame=1``).  ``k=None`` switches observations off and frees the buffer.  Needs ``upload`` first, which
        also drops them; every other call keeps them, and they keep the snapshot.  Allocates and zero-fills the buffer
        (``observation_tensor()`` must be taken again)."""
        L = self._lib
        if k is None:
            self._check(L.sfm_batch_set_observation(self._b, 0, None, 0), "sfm_batch_set_observation")
            self.obs_k = None
            return
        self._need_upload("set_observation")
        if sense_range is None:
            raise ValueError("set_observation needs a sense_range (metres)")
        k, r, frame = observation_arrays(self.B, k, sense_range, frame)
        self._check(L.sfm_batch_set_observation(self._b, k, fptr(r), frame), "sfm_batch_set_observation")
        self.obs_k = k

    def observe(self):
        """Compute every row's observation as the state is now (sfm_batch_observe): one launch on the batch's stream, ordered
        with the ticks and restarts around it; the host does not wait.  Raises SfmLibraryError while observations are off."""
        self._check(self._lib.sfm_batch_observe(self._b), "sfm_batch_observe")

    def observations(self):
        """``observe()`` and a download: a list of B float32 arrays (N_b, 16 + 4k) in scene order (synchronises the batch's
        stream)."""
        self.observe()
        n = int(self.scene_off[-1])
        buf = np.zeros((n, obs_width(self.obs_k)), np.float32)
        self._check(self._lib.sfm_batch_download_observations(self._b, fptr(buf) if n else None), "sfm_batch_download_observations")
        return split_observations(buf, self.scene_off)

    def observation_tensor(self, device=None):
        """The observation buffer as a torch tensor (N_total, 16 + 4k) float32 that aliases device memory (no copy): what a
        policy reads after ``observe()``.  Put torch and the batch on one stream
        (``set_stream(torch.cuda.current_stream().cuda_stream)``) so that the launch and the reads are ordered.  Take it again
        after ``upload`` or ``set_observation``.  Raises SfmLibraryError while observations are off."""
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_observation_ptr(self._b, C.byref(nbytes))
        if not ptr and (self.obs_k is None or self.scene_off is None or int(self.scene_off[-1]) > 0):
            self._check(-1, "sfm_batch_observation_ptr")
        w = obs_width(self.obs_k)
        return self._alias(ptr, (int(nbytes.value) // (4 * w), w), device)

    def _vehicle_off(self, name):
        """The device-side vehicles' scene offsets (B+1,), or SfmLibraryError: ``name`` needs them."""
        if self._dyn is None or not self._boxes:
            raise SfmLibraryError(f"SfmBatch.{name}: this needs device-side vehicles (upload(..., device_vehicles=True) or "
                                  "set_dynamic_boxes)")
        return self._dyn[0]

    def set_vehicle_driving(self, kinds, commands=None):
        """Which device-side vehicles the caller drives, and their first commands (sfm_batch_set_vehicle_driving; see
        ``pack_vehicle_driving`` and the module docstring): a kind 1 vehicle takes (a, b) as its velocity, a kind 2 vehicle moves at
        the signed speed a along its heading turned by (b, c) = (cos, sin) of this tick's turn.  ``kinds=None`` switches driving
        off.  Needs device-side vehicles; ``upload`` and ``set_dynamic_boxes`` drop it, every other call keeps it, and it keeps the
        snapshot.  Reallocates the command buffer (``vehicle_command_tensor()`` must be taken again)."""
        L = self._lib
        if kinds is None:
            self._check(L.sfm_batch_set_vehicle_driving(self._b, None, None, None, None), "sfm_batch_set_vehicle_driving")
            self.driving = False
            return
        kd, a, b, c = pack_vehicle_driving(kinds, commands, self._vehicle_off("set_vehicle_driving"))
        self._check(L.sfm_batch_set_vehicle_driving(self._b, u8ptr(kd), fptr(a), fptr(b), fptr(c)), "sfm_batch_set_vehicle_driving")
        self.driving = True

    def set_vehicle_commands(self, commands):
        """New commands for every vehicle, kinds as ``set_vehicle_driving`` set them (sfm_batch_set_vehicle_commands): one
        host-to-device copy on the batch's stream, no wait.  ``commands`` as for ``pack_vehicle_driving``; a vehicle that is not
        driven may hold anything -- the library validates against the kinds it knows."""
        io = self._vehicle_off("set_vehicle_commands")
        c = np.zeros((int(io[-1]), 3)) if commands is None else _per_vehicle(commands, io, 3, "commands")
        with np.errstate(over="ignore", invalid="ignore"):
            u = np.ascontiguousarray(c, dtype=np.float32)
        a, b, c = f32(u[:, 0]), f32(u[:, 1]), f32(u[:, 2])                    # (kept alive across the call)
        self._check(self._lib.sfm_batch_set_vehicle_commands(self._b, fptr(a), fptr(b), fptr(c)), "sfm_batch_set_vehicle_commands")

    def vehicle_driving(self):
        """Per scene (kind (M_b,) uint8, command (M_b,3), heading (M_b,2), velocity (M_b,2) float32): kinds and commands as the next
        tick reads them, headings and velocities as the last tick left them (synchronises the batch's stream).  Raises
        SfmLibraryError while driving is off."""
        io = self._dyn[0] if self._dyn is not None else np.zeros(self.B + 1, np.int32)
        M = max(int(io[-1]), 1)
        kd = np.zeros(M, np.uint8)
        cols = [np.zeros(M, np.float32) for _ in range(7)]
        self._check(self._lib.sfm_batch_download_vehicle_driving(self._b, u8ptr(kd), *(fptr(a) for a in cols)),
                    "sfm_batch_download_vehicle_driving")
        return _split_rows(io, kd, np.stack(cols[0:3], axis=1), np.stack(cols[3:5], axis=1), np.stack(cols[5:7], axis=1))

    def _vehicle_tensor(self, which, width, device):
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_device_ptr(self._b, int(which), C.byref(nbytes))
        if not ptr:
            self._check(-1, "sfm_batch_device_ptr")
        return self._alias(ptr, (int(nbytes.value) // (4 * width), width), device)

    def vehicle_command_tensor(self, device=None):
        """The vehicle command buffer as a torch tensor (M, 4) float32 {a, b, c, kind} that aliases device memory (no copy): what a
        driving policy writes.  Put torch and the batch on one stream so that writes and ticks are ordered.  What is written here is
        not validated: a kind other than 1 or 2 counts as 0.  ``set_vehicle_commands`` sends the kinds of ``set_vehicle_driving``
        and so overwrites kinds changed here.  Take it again after ``set_vehicle_driving``."""
        if not self.driving:
            raise SfmLibraryError("SfmBatch.vehicle_command_tensor: vehicle driving is off (set_vehicle_driving)")
        return self._vehicle_tensor(PTR_VEHICLE_COMMANDS, 4, device)

    def set_vehicle_observation(self, k, sense_range=None, frame=0, goals=None, mask=None):
        """What ``observe_vehicles`` computes (sfm_batch_set_vehicle_observation; see ``vehicle_observation_arrays`` and the module
        docstring): ``k`` pedestrian slots per vehicle, a sense range in metres, world axes (``frame=0``) or the vehicle's heading
        frame (``frame=1``), a goal per vehicle and a mask of the vehicles that are observed.  ``k=None`` switches the
        observations off.  Needs ``upload`` and device-side vehicles; ``upload`` and ``set_dynamic_boxes`` drop them, every other
        call keeps them.  Allocates and zero-fills the buffer (``vehicle_observation_tensor()`` must be taken again)."""
        L = self._lib
        if k is None:
            self._check(L.sfm_batch_set_vehicle_observation(self._b, 0, None, 0, None, None, None), "sfm_batch_set_vehicle_observation")
            self.vobs_k = None
            return
        self._need_upload("set_vehicle_observation")
        if sense_range is None:
            raise ValueError("set_vehicle_observation needs a sense_range (metres)")
        k, r, frame, gx, gy, mk = vehicle_observation_arrays(self._vehicle_off("set_vehicle_observation"), k, sense_range, frame, goals, mask)
        self._check(L.sfm_batch_set_vehicle_observation(self._b, k, fptr(r), frame, fptr(gx), fptr(gy), u8ptr(mk)),
                    "sfm_batch_set_vehicle_observation")
        self.vobs_k = k

    def observe_vehicles(self):
        """Compute every observed vehicle's record as the batch is now (sfm_batch_observe_vehicles): one launch on the batch's
        stream; the host does not wait.  Raises SfmLibraryError while vehicle observations are off."""
        self._check(self._lib.sfm_batch_observe_vehicles(self._b), "sfm_batch_observe_vehicles")

    def vehicle_observations(self):
        """``observe_vehicles()`` and a download: a list of B float32 arrays (M_b, 16 + 4k) in scene order (synchronises the
        batch's stream)."""
        self.observe_vehicles()
        io = self._dyn[0]
        buf = np.zeros((int(io[-1]), obs_width(self.vobs_k)), np.float32)
        self._check(self._lib.sfm_batch_download_vehicle_observations(self._b, fptr(buf)), "sfm_batch_download_vehicle_observations")
        return _split_rows(io, buf)

    def vehicle_observation_tensor(self, device=None):
        """The vehicle observation buffer as a torch tensor (M, 16 + 4k) float32 that aliases device memory (no copy): what a
        driving policy and its reward read after ``observe_vehicles()``.  Put torch and the batch on one stream.  Take it again
        after ``set_vehicle_observation``.  Raises SfmLibraryError while vehicle observations are off."""
        if self.vobs_k is None:
            raise SfmLibraryError("SfmBatch.vehicle_observation_tensor: vehicle observations are off (set_vehicle_observation)")
        return self._vehicle_tensor(PTR_VEHICLE_OBS, obs_width(self.vobs_k), device)

    def set_vehicle_scan(self, max_range, ped_radius=None, point_radius=_scan.POINT_RADIUS, R=None, angles=None, directions=None,
                         mask=None, frame=0, mount=(0.0, 0.0)):
        """What ``scan_vehicles`` computes (sfm_batch_set_vehicle_scan; see ``vehicle_scan_arrays`` and the module docstring): per
        scanned vehicle R rays (up to 256) from a sensor at ``mount`` = (x, y) in the vehicle frame (x forward), each the distance to
        the first disc it meets -- every pedestrian a disc of ``ped_radius``, every border, static-obstacle and OTHER vehicle's ring
        point a disc of ``point_radius`` (0 switches a kind off); the vehicle's own ring is left out -- up to ``max_range``; the
        three lengths one value or one per scene, in metres.  The rays as for ``set_scan``: ``R``, ``angles`` or ``directions``.
        ``mask``: which vehicles are scanned, as for ``set_vehicle_observation``.  ``frame``: 0 world axes, 1 the vehicle's heading
        frame.  ``max_range=None`` switches the scan off and frees the buffer.  Needs ``upload`` and device-side vehicles;
        ``upload`` and ``set_dynamic_boxes`` drop it, every other call keeps it, and it keeps the snapshot.  Allocates and
        zero-fills the buffer (``vehicle_scan_tensor()`` must be taken again)."""
        L = self._lib
        if max_range is None:
            self._check(L.sfm_batch_set_vehicle_scan(self._b, 0, None, None, None, None, None, None, 0, 0.0, 0.0), "sfm_batch_set_vehicle_scan")
            self.vscan_rays = None
            return
        self._need_upload("set_vehicle_scan")
        if ped_radius is None:
            raise ValueError("set_vehicle_scan needs a ped_radius (metres; 0: pedestrians are not seen)")
        if sum(v is not None for v in (R, angles, directions)) != 1:
            raise ValueError("set_vehicle_scan takes exactly one of R, angles and directions")
        lim = _scan.MAX_VEHICLE_SCAN_RAYS
        if directions is not None:
            dx, dy = _scan.check_directions(directions, lim)
        else:
            dx, dy = _scan.ray_directions(_scan.default_angles(R, lim) if angles is None else angles, lim)
        rm, rp, rq, mk, frame, mx, my = vehicle_scan_arrays(self._vehicle_off("set_vehicle_scan"), max_range, ped_radius, point_radius,
                                                            frame, mask, mount)
        self._check(L.sfm_batch_set_vehicle_scan(self._b, int(dx.shape[0]), fptr(dx), fptr(dy), fptr(rm), fptr(rp), fptr(rq), u8ptr(mk),
                                                 frame, float(mx), float(my)), "sfm_batch_set_vehicle_scan")
        self.vscan_rays = int(dx.shape[0])

    def scan_vehicles(self):
        """Scan from every scanned vehicle as the batch is now (sfm_batch_scan_vehicles): one launch on the batch's stream, ordered
        with the ticks and restarts around it; the host does not wait.  Raises SfmLibraryError while the vehicle scan is off."""
        self._check(self._lib.sfm_batch_scan_vehicles(self._b), "sfm_batch_scan_vehicles")

    def vehicle_scans(self):
        """``scan_vehicles()`` and a download: a list of B float32 arrays (M_b, 2R) in scene order -- ranges, then kinds
        (synchronises the batch's stream)."""
        self.scan_vehicles()
        io = self._dyn[0]
        buf = np.zeros((int(io[-1]), 2 * (self.vscan_rays or 0)), np.float32)
        self._check(self._lib.sfm_batch_download_vehicle_scan(self._b, fptr(buf)), "sfm_batch_download_vehicle_scan")
        return _split_rows(io, buf)

    def vehicle_scan_tensor(self, device=None):
        """The vehicle scan buffer as a torch tensor (M, 2R) float32 that aliases device memory (no copy): what a driving policy
        reads after ``scan_vehicles()``.  Put torch and the batch on one stream.  Take it again after ``set_vehicle_scan``.  Raises
        SfmLibraryError while the vehicle scan is off."""
        if self.vscan_rays is None:
            raise SfmLibraryError("SfmBatch.vehicle_scan_tensor: the vehicle scan is off (set_vehicle_scan)")
        return self._vehicle_tensor(PTR_VEHICLE_SCAN, 2 * self.vscan_rays, device)

    def set_scan(self, max_range, ped_radius=None, point_radius=_scan.POINT_RADIUS, R=None, angles=None, mask=None, frame=0,
                 directions=None):
        """What ``scan`` computes (sfm_batch_set_scan; see ``scan.scan_arrays`` and the module docstring): per scanned row R rays,
        each the distance to the first disc it meets -- pedestrians are discs of ``ped_radius``, every sampled point of a border, a
        static-obstacle ring or a vehicle ring a disc of ``point_radius`` (0 switches a kind off) -- up to ``max_range``; all three
        one value or one per scene, in metres.  The rays: ``R`` of them at 2 pi q / R, or ``angles`` (radians; cos and sin are
        formed in double and rounded once), or ``directions`` = (dir_x, dir_y) used as given.  ``mask``: which rows are scanned
        (``scan.scan_mask``: None every row, a list per scene of bool arrays or row indices, or a bool array over the concatenated
        rows).  ``frame``: 0 world axes, 1 the row's heading frame.  ``max_range=None`` switches scans off and frees the buffer.
        Needs ``upload`` first, which also drops them; every other call keeps them, and they keep the snapshot.  Allocates and
        zero-fills the buffer (``scan_tensor()`` must be taken again)."""
        L = self._lib
        if max_range is None:
            self._check(L.sfm_batch_set_scan(self._b, 0, None, None, None, None, None, None, 0), "sfm_batch_set_scan")
            self.scan_rays = None
            return
        self._need_upload("set_scan")
        if ped_radius is None:
            raise ValueError("set_scan needs a ped_radius (metres; 0: pedestrians are not seen)")
        if sum(v is not None for v in (R, angles, directions)) != 1:
            raise ValueError("set_scan takes exactly one of R, angles and directions")
        if directions is not None:
            dx, dy = _scan.check_directions(directions)
        else:
            dx, dy = _scan.ray_directions(_scan.default_angles(R) if angles is None else angles)
        rm, rp, rq, frame = _scan.scan_arrays(self.B, max_range, ped_radius, point_radius, frame)
        m = _scan.scan_mask(mask, self.scene_off)
        if m is not None and m.shape[0] == 0:
            m = None
        self._check(L.sfm_batch_set_scan(self._b, int(dx.shape[0]), fptr(dx), fptr(dy), fptr(rm), fptr(rp), fptr(rq), u8ptr(m), frame),
                    "sfm_batch_set_scan")
        self.scan_rays = int(dx.shape[0])

    def scan(self):
        """Scan as the state is now (sfm_batch_scan): one launch on the batch's stream, ordered with the ticks and restarts around
        it; the host does not wait.  Raises SfmLibraryError while scans are off."""
        self._check(self._lib.sfm_batch_scan(self._b), "sfm_batch_scan")

    def scans(self):
        """``scan()`` and a download: a list of B float32 arrays (N_b, 2R) in scene order -- ranges, then kinds (synchronises the
        batch's stream)."""
        self.scan()
        n = int(self.scene_off[-1])
        buf = np.zeros((n, 2 * (self.scan_rays or 0)), np.float32)
        self._check(self._lib.sfm_batch_download_scan(self._b, fptr(buf) if n else None), "sfm_batch_download_scan")
        return split_observations(buf, self.scene_off)

    def scan_tensor(self, device=None):
        """The scan buffer as a torch tensor (N_total, 2R) float32 that aliases device memory (no copy): what a policy reads after
        ``scan()``.  Put torch and the batch on one stream.  Take it again after ``upload`` or ``set_scan``.  Raises
        SfmLibraryError while scans are off."""
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_device_ptr(self._b, PTR_SCAN, C.byref(nbytes))
        if not ptr and (self.scan_rays is None or self.scene_off is None or int(self.scene_off[-1]) > 0):
            self._check(-1, "sfm_batch_device_ptr")
        w = 2 * self.scan_rays
        return self._alias(ptr, (int(nbytes.value) // (4 * w), w), device)

    def set_grid(self, cell, G=16, mask=None, frame=0):
        """What ``grid`` computes (sfm_batch_set_grid; see ``grid.grid_arrays`` and the module docstring): per gridded row a
        ``G`` x ``G`` grid (1 .. 32) of ``cell`` metres per cell (one value or one per scene) centred on the row, 6 channels.
        ``mask``: which rows are gridded (``scan.scan_mask``: None every row, a list per scene of bool arrays or row indices, or a
        bool array over the concatenated rows); they get the slots 0 .. M-1 in ascending row order (``grid_rows()``).  ``frame``: 0
        world axes, 1 the row's heading frame.  ``cell=None`` switches grids off and frees the buffer.  Needs ``upload`` first,
        which also drops them; every other call keeps them, and they keep the snapshot.  Allocates and zero-fills the buffer
        (``grid_tensor()`` must be taken again)."""
        L = self._lib
        if cell is None:
            self._check(L.sfm_batch_set_grid(self._b, 0, None, None, 0), "sfm_batch_set_grid")
            self.grid_cells = self._grid_rows = self._grid_counts = None
            return
        self._need_upload("set_grid")
        G, c, frame = _grid.grid_arrays(self.B, G, cell, frame)
        m = _scan.scan_mask(mask, self.scene_off)
        rows, counts = _grid.grid_slots(m, self.scene_off)
        if m is not None and m.shape[0] == 0:
            m = None
        self._check(L.sfm_batch_set_grid(self._b, G, fptr(c), u8ptr(m), frame), "sfm_batch_set_grid")
        self.grid_cells, self._grid_rows, self._grid_counts = G, rows, counts

    def _need_grid(self, name):
        if self.grid_cells is None:                                    # (the library's message, from the call itself)
            self._check(self._lib.sfm_batch_grid(self._b), "sfm_batch_grid")
            raise SfmLibraryError(f"SfmBatch.{name}: grids are off")

    def grid(self):
        """Compute the grids as the state is now (sfm_batch_grid): one launch on the batch's stream, ordered with the ticks and
        restarts around it; the host does not wait.  Raises SfmLibraryError while grids are off."""
        self._check(self._lib.sfm_batch_grid(self._b), "sfm_batch_grid")

    def grid_rows(self):
        """The global (concatenated) row of every slot of the grid buffer, int64 [M], ascending."""
        self._need_grid("grid_rows")
        return self._grid_rows.copy()

    def grids(self):
        """``grid()`` and a download: a list of B float32 arrays (m_b, 6, G, G) in scene order, m_b the scene's gridded rows in
        ascending order (synchronises the batch's stream)."""
        self.grid()
        self._need_grid("grids")
        G, M = self.grid_cells, len(self._grid_rows)
        buf = np.zeros((M, _grid.GRID_CHANNELS, G, G), np.float32)
        self._check(self._lib.sfm_batch_download_grid(self._b, fptr(buf) if M else None), "sfm_batch_download_grid")
        cut = np.concatenate([[0], np.cumsum(self._grid_counts)])
        return [buf[cut[s]:cut[s + 1]] for s in range(self.B)]

    def grid_tensor(self, device=None):
        """The grid buffer as a torch tensor (M, 6, G, G) float32 that aliases device memory (no copy): what a conv policy reads
        after ``grid()``.  Put torch and the batch on one stream.  Take it again after ``upload`` or ``set_grid``.  Raises
        SfmLibraryError while grids are off."""
        self._need_grid("grid_tensor")
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_device_ptr(self._b, PTR_GRID, C.byref(nbytes))
        if not ptr and len(self._grid_rows) > 0:
            self._check(-1, "sfm_batch_device_ptr")
        G = self.grid_cells
        return self._alias(ptr, (int(nbytes.value) // (4 * _grid.GRID_CHANNELS * G * G), _grid.GRID_CHANNELS, G, G), device)

    def set_observed(self, tracks, roles=None, every=1, v0=None):
        """The recording every scene is calibrated against (sfm_batch_set_observed; see ``replay.pack_observed`` and the module
        docstring).  ``tracks``: a list of B arrays (F_b, n_b, 2), NaN in both components where a row is not seen, F_b <= 16384;
        ``roles``: per row 0 (not part of the data), 1 (replayed) or 2 (scored), a list of B arrays or one array over the
        concatenated rows; ``every``: ticks between two frames; ``v0``: optional initial velocities (n_b, 2), NaN = take it from
        the track.  ``tracks=None`` switches the observed tracks off.  Needs a planar ``upload`` first and no modes; switches
        steering on (every kind 0) if it is off -- ``command_tensor()`` must then be taken again.  ``upload``, ``set_modes``,
        ``set_spawns`` and ``set_steering(None)`` drop the tracks; every other call keeps them."""
        L = self._lib
        if tracks is None:
            self._check(L.sfm_batch_set_observed(self._b, None, None, None, None, None, 0), "sfm_batch_set_observed")
            self.observed_every = None
            return
        self._need_upload("set_observed")
        if roles is None:
            raise ValueError("set_observed needs roles")
        if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)):
            raise ValueError(f"every must be an integer >= 1, got {every!r}")
        off, frames, obs, r, v = _replay.pack_observed(tracks, roles, self.scene_off, v0)
        one_f, one_u = np.zeros((1, 2), np.float32), np.zeros(1, np.uint8)
        self._check(L.sfm_batch_set_observed(self._b, off.ctypes.data, iptr(frames), fptr(obs if obs.shape[0] else one_f),
                                             u8ptr(r if r.shape[0] else one_u), None if v is None else fptr(v if v.shape[0] else one_f),
                                             int(every)), "sfm_batch_set_observed")
        self.observed_every = int(every)

    def _need_observed(self, name):
        if self.observed_every is None:                                # (the library's message, from the call itself)
            self._check(self._lib.sfm_batch_score(self._b), "sfm_batch_score")
            raise SfmLibraryError(f"SfmBatch.{name}: observed tracks are off")

    def run_observed(self, first, frames, redraw=False):
        """Frames ``first`` .. ``first + frames - 1`` of the recording (sfm_batch_run_observed): per frame one frame kernel, then
        ``every`` integrating ticks, all on the batch's stream with no copy and no wait.  ``first=0`` clears the row scores and
        places every row of role 1 or 2; a later ``first`` continues a run.  Raises SfmLibraryError while observed tracks are off."""
        self._check(self._lib.sfm_batch_run_observed(self._b, int(first), int(frames), self._flags(True, redraw)), "sfm_batch_run_observed")

    def score(self):
        """Reduce the row scores to per-scene scores (sfm_batch_score): one launch on the batch's stream; the host does not wait."""
        self._check(self._lib.sfm_batch_score(self._b), "sfm_batch_score")

    def row_scores(self):
        """Per scene (n_b, 4) float32 {samples, sum_d, sum_d2, last_d2} as the last frame kernel left them, in scene order
        (synchronises the batch's stream)."""
        self._need_observed("row_scores")
        n = int(self.scene_off[-1])
        buf = np.zeros((n, 4), np.float32)
        self._check(self._lib.sfm_batch_download_scores(self._b, fptr(buf) if n else None, None), "sfm_batch_download_scores")
        return _split_rows(self.scene_off, buf)

    def scene_scores(self):
        """``score()`` and a download: (B, 5) float32 {rows, samples, sum_d, sum_d2, sum_final_d} (``replay.metrics`` turns them
        into ADE, RMSE, FDE); synchronises the batch's stream."""
        self.score()
        buf = np.zeros((self.B, _replay.SCENE_SCORE_WIDTH), np.float32)
        self._check(self._lib.sfm_batch_download_scores(self._b, None, fptr(buf)), "sfm_batch_download_scores")
        return buf

    def _score_tensor(self, which, width, name, device):
        self._need_observed(name)
        nbytes = C.c_int64(0)
        ptr = self._lib.sfm_batch_device_ptr(self._b, which, C.byref(nbytes))
        if not ptr and (which == PTR_SCENE_SCORES or int(self.scene_off[-1]) > 0):
            self._check(-1, "sfm_batch_device_ptr")
        return self._alias(ptr, (int(nbytes.value) // (4 * width), width), device)

    def row_score_tensor(self, device=None):
        """The row scores as a torch tensor (N_total, 4) float32 that aliases device memory (no copy).  Take it again after
        ``set_observed``.  Raises SfmLibraryError while observed tracks are off."""
        return self._score_tensor(PTR_ROW_SCORES, 4, "row_score_tensor", device)

    def scene_score_tensor(self, device=None):
        """The scene scores as a torch tensor (B, 5) float32 that aliases device memory, as the last ``score()`` left them: an
        argmin over candidates needs no copy.  Take it again after ``set_observed``."""
        return self._score_tensor(PTR_SCENE_SCORES, _replay.SCENE_SCORE_WIDTH, "scene_score_tensor", device)

    def set_waypoint_streams(self, seeds, world_sides, arrive_thresholds=2.0):
        """Per-scene waypoint streams for ``redraw=True`` (see ``stream_arrays``; scalars broadcast to every scene).  They stay in
        effect across ``upload`` and ``set_params``; every upload zeroes the draw counters."""
        seed, side, thr = stream_arrays(self.B, seeds, world_sides, arrive_thresholds)
        self._check(self._lib.sfm_batch_set_waypoint_streams(self._b, seed.ctypes.data, fptr(side), fptr(thr)),
                    "sfm_batch_set_waypoint_streams")

    @staticmethod
    def _flags(integrate, redraw):
        return (_lib.TICK_INTEGRATE if integrate else 0) | (_lib.TICK_REDRAW_WAYPOINTS if redraw else 0)

    def tick(self, integrate=False, redraw=False):
        self._check(self._lib.sfm_batch_tick(self._b, self._flags(integrate, redraw)), "sfm_batch_tick")

    def run(self, ticks, redraw=False):
        self._check(self._lib.sfm_batch_run(self._b, int(ticks), self._flags(True, redraw)), "sfm_batch_run")

    def run_recorded(self, ticks, stride=1, redraw=False, max_frames=None):
        """``run`` that records every scene's state before tick 0, stride, 2*stride, ... on the device.  Returns (frames, ticks_idx,
        zframes): frames a list of B float32 arrays (F, N_b, 4) {x, y, vx, vy}; ticks_idx [0, stride, ...]; zframes a list of
        (F, N_b, 2) {z, vz} for a 3-D batch, None for a planar one."""
        self._need_upload("run_recorded")
        n = int(self.scene_off[-1])
        F = n_frames(int(ticks), int(stride), None if max_frames is None else int(max_frames))
        frames = np.zeros((F, n, 4), np.float32)
        zframes = None if self.planar else np.zeros((F, n, 2), np.float32)
        got = C.c_int(0)
        self._check(self._lib.sfm_batch_run_recorded(self._b, int(ticks), self._flags(True, redraw), int(stride),
                                                     fptr(frames) if F else None, fptr(zframes) if F and zframes is not None else None,
                                                     F if max_frames is None else int(max_frames), C.byref(got)),
                    "sfm_batch_run_recorded")
        F = got.value
        idx = np.arange(F) * int(stride)
        return (split_frames(frames[:F], self.scene_off), idx,
                None if zframes is None else split_frames(zframes[:F], self.scene_off))

    def _force_cols(self):
        return 2 if self.planar else 3

    def tick_forces(self, integrate=False, redraw=False, forces=None):
        """One tick exactly as ``tick`` that also returns its forces: a list of B dicts name -> (N_b, C) float32, C = 2 {fx, fy}
        for a planar batch, 3 for a 3-D one; ``forces`` a selection of FORCE_RECORD_NAMES (None: all six).  With
        ``integrate=False`` it is Force.get_force of every scene, with nothing moved."""
        self._need_upload("tick_forces")
        names = _record_names(forces)
        buf = np.zeros((len(names), int(self.scene_off[-1]), self._force_cols()), np.float32)
        self._check(self._lib.sfm_batch_tick_forces(self._b, self._flags(integrate, redraw), force_mask(names), fptr(buf)),
                    "sfm_batch_tick_forces")
        return split_forces(buf, self.scene_off, names)

    def run_recorded_forces(self, ticks, stride=1, redraw=False, max_frames=None, forces=None):
        """``run_recorded`` that also records, for every recorded tick f*stride, the forces that tick computed from frame f's
        state.  Returns (frames, ticks_idx, zframes, forces): the first three exactly as ``run_recorded``; forces a list of B dicts
        name -> (F, N_b, C) float32."""
        self._need_upload("run_recorded_forces")
        names = _record_names(forces)
        n = int(self.scene_off[-1])
        F = n_frames(int(ticks), int(stride), None if max_frames is None else int(max_frames))
        need = record_bytes(n, F, self.planar, names, zframes=not self.planar)
        if need > MAX_RECORD_BYTES:                   # the library's refusal, before the host buffers are allocated
            raise SfmLibraryError(f"sfm_batch_run_recorded_forces: the frames and forces of this call need {need} bytes, more "
                                  f"than the {MAX_RECORD_BYTES} one call may record: split the run")
        frames = np.zeros((F, n, 4), np.float32)
        zframes = None if self.planar else np.zeros((F, n, 2), np.float32)
        buf = np.zeros((F, len(names), n, self._force_cols()), np.float32)
        got = C.c_int(0)
        self._check(self._lib.sfm_batch_run_recorded_forces(self._b, int(ticks), self._flags(True, redraw), int(stride),
                                                            force_mask(names), fptr(frames) if F else None,
                                                            fptr(zframes) if F and zframes is not None else None,
                                                            fptr(buf) if F else None, F if max_frames is None else int(max_frames),
                                                            C.byref(got)), "sfm_batch_run_recorded_forces")
        F = got.value
        idx = np.arange(F) * int(stride)
        return (split_frames(frames[:F], self.scene_off), idx,
                None if zframes is None else split_frames(zframes[:F], self.scene_off), split_forces(buf[:F], self.scene_off, names))

    def set_modes(self, plans, despawn_on_arrival=True, sim_time0=0.0, arrive_thresholds=2.0, scenes=None):
        """The pedestrian mode state machine of every scene (sfm_batch_set_mode_fsm): ``plans`` one mode plan per scene (see
        ``pack_modes``; ``scenes`` supplies each scene's default first-vehicle extent), the per-scene scalars as in
        ``mode_scene_arrays`` (each a scalar broadcast to every scene, or B values).  ``plans=None`` switches the modes off; so does
        every ``upload``."""
        L = self._lib
        if plans is None:
            self._check_drops(L.sfm_batch_set_mode_fsm(self._b, *([None] * 14)), "sfm_batch_set_mode_fsm")
            return
        self._need_upload("set_modes")
        pm = pack_modes(plans, self.scene_off, scenes)
        despawn, t0, thr = mode_scene_arrays(self.B, despawn_on_arrival, sim_time0, arrive_thresholds)
        W = int(pm["wp_offsets"][-1])
        self._check_drops(L.sfm_batch_set_mode_fsm(self._b, u8ptr(pm["mode"]), *(fptr(pm[k]) for k in MODE_KEYS[1:]),
                                                   iptr(pm["wp_offsets"]), fptr(pm["wp_x"]) if W else None,
                                                   fptr(pm["wp_y"]) if W else None, u8ptr(pm["wp_crossing"]) if W else None,
                                                   iptr(despawn), fptr(t0), fptr(thr), fptr(pm["first_vehicle_extent"])),
                          "sfm_batch_set_mode_fsm")
        self.observed_every = None                                     # (the modes own parking and birth: the observed tracks are dropped)

    def set_spawns(self, schedules):
        """The spawn schedule of every scene (sfm_batch_set_spawn_schedule): ``schedules`` one per scene (see ``pack_spawns``;
        ``None`` for a scene whose rows are all there).  Needs ``set_modes`` first.  Rows that are not due on their scene's clock
        (or wait for their predecessor) leave the live state until their birth tick.  ``upload`` and ``set_modes`` drop the
        schedule, ``set_params`` keeps it; a second schedule without an ``upload`` + ``set_modes`` in between is refused.
        ``schedules=None`` switches the schedule off, refused while a row is unborn."""
        L = self._lib
        if schedules is None:
            self._check_drops(L.sfm_batch_set_spawn_schedule(self._b, None, None), "sfm_batch_set_spawn_schedule")
            return
        self._need_upload("set_spawns")
        t, c = pack_spawns(schedules, self.scene_off)
        if t.shape[0] == 0:                                            # (no rows: still a call, so that the refusals are the library's)
            t, c = np.zeros(1, np.float32), np.zeros(1, np.uint8)
        self._check_drops(L.sfm_batch_set_spawn_schedule(self._b, fptr(t), u8ptr(c)), "sfm_batch_set_spawn_schedule")
        self.observed_every = None

    def spawns(self):
        """Per scene (born (N_b,) bool, birth_time (N_b,) float32: the scene's clock before the row's birth tick -- the clock
        at ``set_spawns`` for rows live from the start -- NaN while unborn), in scene order.  Raises SfmLibraryError while no
        schedule is set."""
        n = int(self.scene_off[-1]) if self.scene_off is not None else 0
        born, when = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32)
        self._check(self._lib.sfm_batch_download_spawns(self._b, u8ptr(born), fptr(when)), "sfm_batch_download_spawns")
        so = self.scene_off if self.scene_off is not None else np.zeros(self.B + 1, np.int32)
        return _split_rows(so, born.astype(bool), when)

    def _modes(self):
        n = int(self.scene_off[-1]) if self.scene_off is not None else 0
        m, t, c = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.int32)
        clk = np.zeros(self.B, np.float32)
        self._check(self._lib.sfm_batch_download_modes(self._b, u8ptr(m) if n else None, fptr(t) if n else None,
                                                       iptr(c) if n else None, fptr(clk)), "sfm_batch_download_modes")
        return m, t, c, clk

    def modes(self):
        """Per scene (mode (N_b,) uint8 with 255 = despawned and 254 = not yet spawned, mode target speed (N_b,) float32, queue cursor (N_b,) int32), in
        scene order.  Raises SfmLibraryError while no modes are set."""
        return _split_rows(self.scene_off, *self._modes()[:3])

    def clocks(self):
        """Each scene's mode clock (sim_time, float32 [B]): sim_time0 plus one step_length per tick since ``set_modes``."""
        return self._modes()[3]

    def waypoints(self):
        """Per scene (waypoint (N_b,2) float32, draw counter (N_b,) uint32), in scene order."""
        self._need_upload("waypoints")
        n = int(self.scene_off[-1])
        wx, wy = np.zeros(n, np.float32), np.zeros(n, np.float32)
        draws = np.zeros(n, np.uint32)
        self._check(self._lib.sfm_batch_download_waypoints(self._b, fptr(wx), fptr(wy), draws.ctypes.data),
                    "sfm_batch_download_waypoints")
        return _split_rows(self.scene_off, np.stack([wx, wy], axis=1), draws)

    def state_arrays(self):
        """Concatenated state: (loc (N_total,3), vel (N_total,3)) float64."""
        self._need_upload("state")
        n = int(self.scene_off[-1])
        a = {k: np.zeros(n, np.float32) for k in ("x", "y", "z", "vx", "vy", "vz")}
        if self.planar:
            a["z"][:] = self._z
        self._check(self._lib.sfm_batch_download_state(self._b, *(fptr(a[k]) for k in ("x", "y", "z", "vx", "vy", "vz"))),
                    "sfm_batch_download_state")
        loc = np.stack([a["x"], a["y"], a["z"]], axis=1).astype(np.float64)
        vel = np.stack([a["vx"], a["vy"], a["vz"]], axis=1).astype(np.float64)
        return loc, vel

    def state(self):
        """Per scene (loc (N_b,3), vel (N_b,3)) float64, in scene order."""
        return _split_rows(self.scene_off, *self.state_arrays())
