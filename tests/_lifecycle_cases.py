"""Crowds, call lists and the drop table of the lifecycle tests (tests/test_lifecycle_gpu.py, tests/test_lifecycle_host.py).  Pure
NumPy on top of the package's packers: nothing here needs a GPU, the functions that take a batch only call its methods.

Three generations of a three-scene crowd, so that going from one to the next both grows and shrinks something:

    gen   rows per scene   vehicles (scene 2)   graph nodes (scene 2)   k / R / G / route capacity / vehicle k / vehicle R
    A     0, 5, 70         2                    12                      2 / 8 / 4 / 8 / 2 / 6
    B     3, 130, 300      3                    257 (read from global)  8 / 24 / 12 / 32 / 6 / 40
    C     1, 64, 65        1                    65                      3 / 12 / 6 / 12 / 3 / 10

Scenes of at most 64 rows, at most 128 and above 128 meet the three j-split forms of the batch tick.  Where a mask is optional (row
scan, grid, vehicle observation, vehicle scan, routes) A sets one, B sets none and C sets another one.

Two profiles, because the header's exclusions allow no single one (include/sfm_hip.h: routes need modes and refuse a spawn schedule;
observed tracks refuse a 3-D batch, modes and a spawn schedule):

    policy   3-D in A and C, planar in B: device vehicles with one track, modes, routes, steering, driving, row observation / scan /
             grid, vehicle observation / scan, episodes, restart noise with a track delay, a snapshot, plan_routes
    replay   planar: device vehicles with one track, observed tracks (roles 0, 1, 2; they switch steering on), row observation /
             scan / grid, episodes, restart noise with a track delay, a snapshot

``last_calls(b, crowd)`` is what a fresh batch gets and a reused one gets last; ``read_all(b, crowd)`` is everything a batch hands
back; ``DROPS`` says, per (call, feature) the header's drop rules name, whether the call keeps or drops the feature."""
from functools import lru_cache

import numpy as np

import _replay_cases as RP
import _route_cases as RC
import test_batch_modes_gpu as M
from carla_social_force_model_amd import reset, scenarios
from carla_social_force_model_amd._lib import fptr, iptr
from carla_social_force_model_amd.batch import pack_scenes

DTS = (0.05, 0.04, 0.05)
T0 = (4.5, 4.5, 4.7)
VEHICLE_SCENE = 2                    # the scene with the vehicles, the first of them on a track
TRACK_TICKS = 12                     # what the track plans cover
FRAMES = 5                           # observed frames per scene of the replay profile (one tick apart)
PROFILES = ("policy", "replay")

GEN = {
    "A": dict(rows=(0, 5, 70), vehicles=2, street=(3, 4), nodes=12, extra=1.5, k=2, R=8, G=4, cell=1.5, cap=8, vk=2, vR=6, frame=0,
              drive=(0, 1)),
    "B": dict(rows=(3, 130, 300), vehicles=3, street=(6, 6), nodes=257, extra=14.0, k=8, R=24, G=12, cell=0.75, cap=32, vk=6, vR=40,
              frame=1, drive=(0, 1, 2)),
    "C": dict(rows=(1, 64, 65), vehicles=1, street=(4, 4), nodes=65, extra=1.5, k=3, R=12, G=6, cell=1.0, cap=12, vk=3, vR=10, frame=1,
              drive=(2,)),           # (its one vehicle has a track and is driven: a driven vehicle ignores its keyframes)
}
SEEDS = {"policy": {"A": 6100, "B": 6200, "C": 6300}, "replay": {"A": 6400, "B": 6500, "C": 6600}}
MAX_STEPS = (0, 1, 0)                # scene 1 runs into its time limit at the first end_step
TRACK_DELAY = 5                      # the tracked vehicle of a restarted scene arrives up to 5 ticks later


def configs(shift=0):
    return [M._config(k + shift) for k in range(len(DTS))]


def _fit(graph, loc, side):
    """The graph with its nodes moved onto a square of ``side`` metres around the rows."""
    nodes = np.asarray(graph["nodes"], dtype=np.float64)
    lo = nodes.min(axis=0)
    span = np.maximum(nodes.max(axis=0) - lo, 1.0e-9)
    mid = loc[:, :2].mean(axis=0)
    return dict(graph, nodes=mid - 0.5 * side + (nodes - lo) / span * side)


def _delayed_seed(s):
    """The first seed from ``s`` on under which the vehicle scene's first restart delays its tracked vehicle (vehicle 0)."""
    while reset.delay_ticks(reset.reset_word(s, 0, 0, 0, reset.C_DELAY), TRACK_DELAY) == 0:
        s += 1
    return s


def _masks(gen, sizes, a, c):
    """The optional mask of a per-row sensor: generation A sets ``a`` (a rule on the row index), B none, C ``c``."""
    rule = {"A": a, "B": None, "C": c}[gen]
    return None if rule is None else [rule(np.arange(n)) for n in sizes]


@lru_cache(maxsize=None)
def crowd(profile, gen, variant=0):
    """Everything ``set_everything`` takes for one crowd (built once per argument set; nothing below changes it)."""
    g = GEN[gen]
    seed = SEEDS[profile][gen] + 1000 * variant
    sizes = g["rows"]
    z = 1.5 if profile == "policy" and gen in "AC" else 0.0
    made = [M._scene(n, seed + k, g["vehicles"] if k == VEHICLE_SCENE else 0, z_spread=z, borders=2) for k, n in enumerate(sizes)]
    scenes = [m[0] for m in made]
    rng = np.random.default_rng(seed + 99)
    veh = g["vehicles"]
    c = dict(profile=profile, gen=gen, seed=seed, sizes=sizes, scenes=scenes, planar=z == 0.0, vehicles=veh)
    tracked = scenarios.make_track_plan(scenes[VEHICLE_SCENE], seed + 90, TRACK_TICKS, dt=DTS[VEHICLE_SCENE])
    c["tracks"] = [[tracked[0]] + [None] * (veh - 1) if k == VEHICLE_SCENE else None for k in range(len(sizes))]
    c["track_delay"] = [TRACK_DELAY] + [0] * (veh - 1)
    # the sensors of the rows
    c["obs"] = dict(k=g["k"], sense_range=(6.0, 5.0, 7.0), frame=g["frame"])
    c["scan"] = dict(max_range=(8.0, 6.0, 7.0), ped_radius=0.3, R=g["R"], frame=g["frame"],
                     mask=_masks(gen, sizes, lambda i: i % 5 == 0, lambda i: i % 2 == 1))
    c["grid"] = dict(cell=g["cell"], G=g["G"], frame=1 - g["frame"], mask=_masks(gen, sizes, lambda i: i % 7 == 1, lambda i: i % 3 == 0))
    c["episodes"] = dict(agent=[n // 2 if n else -1 for n in sizes], goal_radius=0.5, ped_radius=0.25, veh_radius=0.4, max_steps=MAX_STEPS)
    c["noise"] = dict(seeds=[seed + 11, seed + 12, _delayed_seed(seed + 13)], pos_box=np.array([0.6, 0.6]), goal_box=np.array([0.4, 0.4]), min_gap=0.2, point_gap=0.05,
                      tries=4)
    if profile == "replay":
        packs = [RP.tracks_for(sc, FRAMES, 1, seed + 40 + k, dt=DTS[k]) for k, sc in enumerate(scenes)]
        c["observed"] = dict(tracks=[p[0] for p in packs], roles=[p[1] for p in packs], v0=[p[2] for p in packs], every=1)
        return c
    c["plans"] = [m[1] for m in made]
    c["scheds"] = [scenarios.make_spawn_plan(sc, seed + 70 + k, dt=DTS[k], t0=T0[k], present=0.35, horizon=1.5) for k, sc in enumerate(scenes)]
    c["kinds"] = [rng.integers(0, 3, n) for n in sizes]
    c["cmds"] = [np.float32(rng.uniform(-1.5, 1.5, (n, 3))) for n in sizes]
    # driving: kind 1 takes (a, b) as the velocity, kind 2 (speed, cos, sin of the tick's turn); the tracked vehicle of A and B runs free
    command = {0: (0.0, 0.0, 0.0), 1: (0.9, -0.6, 0.0), 2: (1.1, np.cos(0.04), np.sin(0.04))}
    c["vkinds"] = [np.asarray(g["drive"]) if k == VEHICLE_SCENE else None for k in range(len(sizes))]
    c["vcmds"] = [np.array([command[d] for d in g["drive"]]) if k == VEHICLE_SCENE else None for k in range(len(sizes))]
    vmask = {"A": [True, False], "B": None, "C": [True]}[gen]
    smask = {"A": [False, True], "B": None, "C": [True]}[gen]
    per_vehicle = lambda m: None if m is None else [np.asarray(m) if k == VEHICLE_SCENE else None for k in range(len(sizes))]
    c["vobs"] = dict(k=g["vk"], sense_range=10.0, frame=g["frame"], mask=per_vehicle(vmask),
                     goals=[np.float32(rng.uniform(-20.0, 20.0, (veh, 2))) if k == VEHICLE_SCENE else None for k in range(len(sizes))])
    c["vscan"] = dict(max_range=(9.0, 9.0, 6.0), ped_radius=0.3, R=g["vR"], frame=g["frame"], mask=per_vehicle(smask), mount=(0.5, 0.0))
    # routes: no graph in scene 0, a street grid in scene 1, a random graph in scene 2, each laid over its rows
    side = [max(float(scenes[k]["world_side"]), 12.0) for k in range(len(sizes))]
    graphs = [None, _fit(RC.street_grid(*g["street"], seed + 31), scenes[1]["loc"], side[1]),
              _fit(RC.random_graph(g["nodes"], seed + 32, extra=g["extra"]), scenes[2]["loc"], side[2])]
    goals = []
    for k, n in enumerate(sizes):
        mid = scenes[k]["loc"][:, :2].mean(axis=0) if n else np.zeros(2)
        gl = np.zeros((n, 3))
        gl[:, :2] = mid + rng.uniform(-0.55 * side[k], 0.55 * side[k], (n, 2))
        goals.append(gl)
    mask = _masks(gen, sizes, lambda i: i % 2 == 0, lambda i: i % 3 != 1)
    lost = max(i for i in range(sizes[VEHICLE_SCENE]) if mask is None or mask[VEHICLE_SCENE][i])
    goals[VEHICLE_SCENE][lost, 0] = np.nan                         # a routed row whose goal is not finite: status 5, left as it is
    c["routes"] = dict(graphs=graphs, graph_types=[rng.integers(1, 4, n) for n in sizes], goals=goals, capacity=g["cap"], mask=mask)
    return c


# ---- the call lists --------------------------------------------------------------------------------------------------------------
def set_everything(b, c):
    """Every feature of the crowd's profile, in an order the header allows, and a snapshot (policy: the routes planned behind it)."""
    b.set_params(configs(), list(DTS))
    b.upload(c["scenes"], device_vehicles=True)
    assert b.planar == c["planar"]
    b.set_vehicle_tracks(c["tracks"])
    if c["profile"] == "policy":
        b.set_modes(c["plans"], despawn_on_arrival=True, sim_time0=list(T0), arrive_thresholds=2.0, scenes=c["scenes"])
        b.set_routes(**c["routes"])
        b.set_steering(c["kinds"], c["cmds"])
        b.set_vehicle_driving(c["vkinds"], c["vcmds"])
        b.set_vehicle_observation(**c["vobs"])
        b.set_vehicle_scan(**c["vscan"])
    else:
        b.set_observed(**c["observed"])
    b.set_observation(**c["obs"])
    b.set_scan(**c["scan"])
    b.set_grid(**c["grid"])
    b.set_episodes(**c["episodes"])
    b.set_restart_noise(track_delay=c["track_delay"], **c["noise"])
    b.snapshot()
    if c["profile"] == "policy":
        b.plan_routes()


def sense(b, c):
    """Every sensor launch of the profile."""
    b.observe()
    b.scan()
    b.grid()
    if c["profile"] == "policy":
        b.observe_vehicles()
        b.scan_vehicles()
    else:
        b.score()


def run(b, c, first, ticks):
    if c["profile"] == "policy":
        for _ in range(ticks):
            b.tick(integrate=True)
    else:
        b.run_observed(first, ticks)


def last_calls(b, c, device_mask):
    """Set everything, three ticks, the episode ends with their automatic restart (scene 1 is at its time limit), scene 2 restarted
    by the host, scenes 0 and 1 by ``device_mask`` (a one-byte tensor on the device holding 1, 1, 0), one more tick, every sensor."""
    set_everything(b, c)
    run(b, c, 0, 3)
    b.end_step(auto_restart=True)
    b.restart([VEHICLE_SCENE])
    b.restart_device(device_mask)
    run(b, c, 3, 1)
    sense(b, c)


def read_all(b, c):
    """Everything a batch hands back: (scenes, whole).  ``scenes``: per scene a dict name -> array, or list of arrays;  ``whole``: one
    such dict for what is per batch.  NaN stands where a record holds NaN by its rule (an episode's first prev_goal_d2)."""
    policy = c["profile"] == "policy"
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [ctr for ctr, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    tick, present = b.vehicle_tracks()
    rec, done = b.episodes()
    resets, fallbacks = b.restart_noise()
    whole = {"tick": np.int64(tick), "episodes": rec, "done": done, "resets": resets, "fallbacks": fallbacks,
             "grid_rows": b.grid_rows(), "planar": np.bool_(b.planar),
             "route_capacity": np.int64(-1 if b.route_capacity is None else b.route_capacity)}
    for k, (p, (kd, cmd), o, s, gr) in enumerate(zip(present, b.steering(), b.observations(), b.scans(), b.grids())):
        out[k].update(present=p, kind=kd, cmd=cmd, obs=o, scan=s, grid=gr)
    if policy:
        clocks = b.clocks()
        for k, ((m, t, cur), (vk, vc, vh, vv), vo, vs, r) in enumerate(zip(b.modes(), b.vehicle_driving(), b.vehicle_observations(),
                                                                             b.vehicle_scans(), b.routes())):
            out[k].update(mode=m, target=t, cursor=cur, clock=clocks[k:k + 1], vkind=vk, vcmd=vc, vheading=vh, vvel=vv, vobs=vo, vscan=vs,
                          queue_xy=[q[0] for q in r["queue"]], queue_cross=[q[1] for q in r["queue"]],
                          **{"route_" + name: r[name] for name in ("status", "s", "t", "L", "cost", "graph_type", "cursor")})
    else:
        whole["scene_scores"] = b.scene_scores()
        for k, rs in enumerate(b.row_scores()):
            out[k].update(row_scores=rs)
    return out, whole


def vehicles_of(c):
    """(centres (M,2), velocities (M,2)) of the vehicle scene as uploaded, float32."""
    sc = c["scenes"][VEHICLE_SCENE]
    return (np.float32([ctr for ctr, _ in sc["dynamic_obstacles"]]).reshape(-1, 2), np.float32(sc["dynamic_vel"]).reshape(-1, 2))


# ---- the calls of the drop table ---------------------------------------------------------------------------------------------------
def _rings(b, c):
    dy = pack_scenes(c["scenes"])["dynamic"]                     # the vehicles as rings that stay where they are: no boxes
    b._check_drops(b._lib.sfm_batch_set_dynamic_obstacles(b._b, *(iptr(x) for x in dy[:2]), *(fptr(x) for x in dy[2:])),
                   "sfm_batch_set_dynamic_obstacles")


# name -> (the SfmBatch method, or None and the library's symbol; the call on a batch that holds crowd c)
CALLS = {
    "upload": ("upload", lambda b, c: b.upload(c["scenes"], device_vehicles=True)),
    "set_modes": ("set_modes", lambda b, c: b.set_modes(crowd("policy", c["gen"])["plans"], despawn_on_arrival=True, sim_time0=list(T0),
                                                         arrive_thresholds=2.0, scenes=c["scenes"])),
    "set_modes_off": ("set_modes", lambda b, c: b.set_modes(None)),
    "set_spawns": ("set_spawns", lambda b, c: b.set_spawns([None] * len(DTS))),      # (everyone is there: nobody is parked)
    "set_spawns_off": ("set_spawns", lambda b, c: b.set_spawns(None)),
    "set_steering_off": ("set_steering", lambda b, c: b.set_steering(None)),
    "set_dynamic_boxes": ("set_dynamic_boxes", lambda b, c: b.set_dynamic_boxes(c["scenes"])),
    "set_dynamic_obstacles": ("sfm_batch_set_dynamic_obstacles", _rings),
    "set_vehicle_tracks": ("set_vehicle_tracks", lambda b, c: b.set_vehicle_tracks(c["tracks"])),
    "set_vehicle_tracks_off": ("set_vehicle_tracks", lambda b, c: b.set_vehicle_tracks(None)),
    "set_params": ("set_params", lambda b, c: b.set_params(configs(1), list(DTS))),
    "set_observation_off": ("set_observation", lambda b, c: b.set_observation(None)),
    "set_episodes_off": ("set_episodes", lambda b, c: b.set_episodes(None)),
    "set_scan_off": ("set_scan", lambda b, c: b.set_scan(None)),
    "set_grid_off": ("set_grid", lambda b, c: b.set_grid(None)),
    "set_restart_noise_off": ("set_restart_noise", lambda b, c: b.set_restart_noise(None, None)),
    "set_observed_off": ("set_observed", lambda b, c: b.set_observed(None)),
    "set_vehicle_driving_off": ("set_vehicle_driving", lambda b, c: b.set_vehicle_driving(None)),
    "set_vehicle_observation_off": ("set_vehicle_observation", lambda b, c: b.set_vehicle_observation(None)),
    "set_vehicle_scan_off": ("set_vehicle_scan", lambda b, c: b.set_vehicle_scan(None)),
    "set_routes_off": ("set_routes", lambda b, c: b.set_routes(None, None, None)),
}
# The set-ups a call is made on: "policy" and "replay" are the profiles with everything set; "spawns" is the policy profile with its
# routes switched off and a spawn schedule set instead (routes refuse a schedule), "born" the same with a schedule under which everyone
# is there from the start (the schedule cannot be switched off while a row is unborn).  HOLDS says which features a set-up holds before
# the call: a row of DROPS is checked on every set-up of its call that holds its feature, and a feature a set-up is said to hold
# must answer there (tests/test_lifecycle_host.py: every row but those of UNREACHABLE is held by a set-up of its call).  Every call
# is made on both profiles; the on form of set_spawns on "policy" alone, since it needs modes, which "replay" cannot have.
_COMMON = ("snapshot", "steering", "observations", "episodes", "scans", "grids", "noise", "noise delays", "tracks")
_POLICY = _COMMON + ("driving", "vehicle observations", "vehicle scans", "modes")
HOLDS = {"policy": _POLICY + ("routes",), "replay": _COMMON + ("observed tracks",), "spawns": _POLICY + ("spawns",), "born": _POLICY + ("spawns",)}
SETUPS = {name: ("policy", "replay") for name in CALLS}
SETUPS["set_spawns"] = ("policy",)
SETUPS["set_spawns_off"] += ("born",)
for _name in ("upload", "set_modes", "set_modes_off", "set_params"):          # (the calls whose rows name the schedule)
    SETUPS[_name] += ("spawns",)
# rows of the header that no sequence of accepted calls reaches:
UNREACHABLE = {("set_spawns", "observed tracks"): "the on form of sfm_batch_set_spawn_schedule needs modes, and observed tracks are refused while "
                                                  "modes are set: on a batch that holds observed tracks the call is refused"}

# feature -> (the member of struct SfmBatch that holds it; the getter of SfmBatch that reads it; what the error says once the feature
# is gone: the messages of csrc/sfm_batch_host.h and of the three downloads that have their own; and a call of the library that only
# asks -- its symbol and how many NULL arguments follow the batch -- because SfmBatch keeps flags of its own that could answer for it)
FEATURES = {
    "snapshot": ("snap", "restart", "no snapshot", ("sfm_batch_restart", 1)),
    "steering": ("steer", "steering", "steering is off", ("sfm_batch_download_steering", 4)),
    "observations": ("obs", "observations", "observations are off", ("sfm_batch_observe", 0)),
    "episodes": ("ep", "episodes", "episodes are off", ("sfm_batch_download_episodes", 2)),
    "scans": ("scan", "scans", "scans are off", ("sfm_batch_scan", 0)),
    "grids": ("grid", "grids", "grids are off", ("sfm_batch_grid", 0)),
    "noise": ("noise", "restart_noise", "restart noise is off", ("sfm_batch_download_restart_noise", 2)),
    "noise delays": ("noise", None, None, None),                 # (no getter: seen by where a restarted scene's tracked vehicle is)
    "observed tracks": ("replay", "row_scores", "observed tracks are off", ("sfm_batch_score", 0)),
    "driving": ("drive", "vehicle_driving", "vehicle driving is off", ("sfm_batch_download_vehicle_driving", 8)),
    "vehicle observations": ("vobs", "vehicle_observations", "vehicle observations are off", ("sfm_batch_observe_vehicles", 0)),
    "vehicle scans": ("vscan", "vehicle_scans", "vehicle scans are off", ("sfm_batch_scan_vehicles", 0)),
    "routes": ("routes", "routes", "routes are off", ("sfm_batch_plan_routes", 1)),
    "modes": ("modes", "modes", "the modes were switched off", ("sfm_batch_download_modes", 4)),
    "spawns": ("spawns", "spawns", "the schedule was dropped", ("sfm_batch_download_spawns", 2)),
    "tracks": ("tracks", "vehicle_tracks", "no vehicle tracks are set", ("sfm_batch_download_vehicle_tracks", 2)),
}
# Members of struct SfmBatch of a Batch...Dev type that are no feature a caller sets and drops:
NOT_FEATURES = {
    "geo": "the scenes' polylines: every upload sets all three kinds anew, there is no 'off'",
    "rec": "grow-only scratch of the recording calls; holds nothing between two calls",
    "restart": "the pinned list of one masked restart and its event; no setting",
    "boxes": "how the vehicles are held (device-side or as rings); what goes with them are the features tracks, driving, vehicle "
             "observations and vehicle scans",
}

KEPT, DROPPED = "kept", "dropped"
# every "off" form and the feature it switches off
OWN_FEATURE = {"set_modes_off": "modes", "set_spawns_off": "spawns", "set_steering_off": "steering", "set_vehicle_tracks_off": "tracks",
               "set_observation_off": "observations", "set_episodes_off": "episodes", "set_scan_off": "scans", "set_grid_off": "grids",
               "set_restart_noise_off": "noise", "set_observed_off": "observed tracks", "set_vehicle_driving_off": "driving",
               "set_vehicle_observation_off": "vehicle observations", "set_vehicle_scan_off": "vehicle scans", "set_routes_off": "routes"}
_VEHICLES = ("upload", "set_dynamic_boxes", "set_dynamic_obstacles")      # (upload sends the vehicles through one of the other two)

DROPS = {}                           # (call, feature) -> (KEPT | DROPPED, the header's sentence)


def _rule(feature, quote, dropped=(), kept=()):
    for outcome, calls in ((DROPPED, dropped), (KEPT, kept)):
        for call in calls:
            assert (call, feature) not in DROPS and call in CALLS, (call, feature)
            DROPS[(call, feature)] = (outcome, quote)


def _others(*dropping):
    return tuple(name for name in CALLS if name not in dropping)


_rule("snapshot", 'sfm_batch_upload_state, sfm_batch_set_dynamic_obstacles, sfm_batch_set_dynamic_boxes, sfm_batch_set_mode_fsm, '
      'sfm_batch_set_spawn_schedule and sfm_batch_set_vehicle_tracks drop it, each also in its "off" form',
      dropped=("upload", "set_dynamic_obstacles", "set_dynamic_boxes", "set_modes", "set_modes_off", "set_spawns", "set_spawns_off",
               "set_vehicle_tracks", "set_vehicle_tracks_off"))
_rule("snapshot", "sfm_batch_set_params, sfm_batch_set_waypoint_streams, sfm_batch_set_borders and sfm_batch_set_static_obstacles keep the snapshot",
      kept=("set_params",))
_rule("snapshot", "the steering calls keep the snapshot", kept=("set_steering_off",))
_rule("snapshot", "every other call keeps them, and they keep the snapshot", kept=("set_observation_off", "set_episodes_off", "set_scan_off", "set_grid_off"))
_rule("snapshot", "every other call keeps it, and it keeps the snapshot", kept=("set_restart_noise_off", "set_vehicle_scan_off"))
_rule("steering", "sfm_batch_upload_state drops it, because the rows may differ", dropped=("upload",))
_rule("steering", "kind = NULL switches steering off", dropped=("set_steering_off",))
_rule("steering", "sfm_batch_set_params, sfm_batch_set_waypoint_streams, the geometry calls, sfm_batch_set_mode_fsm, sfm_batch_set_spawn_schedule, "
      "sfm_batch_set_vehicle_tracks, sfm_batch_snapshot and sfm_batch_restart keep it",
      kept=("set_params", "set_dynamic_boxes", "set_dynamic_obstacles", "set_modes", "set_modes_off", "set_spawns", "set_spawns_off",
            "set_vehicle_tracks", "set_vehicle_tracks_off"))
_rule("observations", "sfm_batch_upload_state drops the observations because the rows may differ, as it drops steering; every other call "
      "keeps them", dropped=("upload",), kept=_others("upload", "set_observation_off"))
_rule("observations", "sense_range = NULL switches observations off and frees the buffer", dropped=("set_observation_off",))
_rule("episodes", "sfm_batch_upload_state drops the episodes (the agents are rows), as it drops observations; every other call keeps them",
      dropped=("upload",), kept=_others("upload", "set_episodes_off"))
_rule("episodes", "agent = NULL switches episodes off", dropped=("set_episodes_off",))
_rule("scans", "sfm_batch_upload_state drops the scans (the mask is per row), as it drops observations; every other call keeps them",
      dropped=("upload",), kept=_others("upload", "set_scan_off"))
_rule("scans", "max_range = NULL switches scans off and frees the buffer", dropped=("set_scan_off",))
_rule("grids", "sfm_batch_upload_state drops the grids (the slots are per row); every other call keeps them",
      dropped=("upload",), kept=_others("upload", "set_grid_off"))
_rule("grids", "cell = NULL switches grids off", dropped=("set_grid_off",))
_rule("noise", "sfm_batch_upload_state drops it, because the rows may differ; every other call keeps it, and it keeps the snapshot",
      dropped=("upload",), kept=_others("upload", "set_restart_noise_off"))
_rule("noise", "seeds = NULL switches the noise off and frees them", dropped=("set_restart_noise_off",))
_rule("noise delays", "the delays go with the tracks they refer to (sfm_batch_set_vehicle_tracks, sfm_batch_set_dynamic_boxes and "
      "sfm_batch_set_dynamic_obstacles drop the delays and keep the rest)",
      dropped=_VEHICLES + ("set_vehicle_tracks", "set_vehicle_tracks_off"),
      kept=_others(*_VEHICLES, "set_vehicle_tracks", "set_vehicle_tracks_off", "set_restart_noise_off"))
# (The delays have no getter.  While tracks and noise are both still there -- after set_vehicle_tracks and after every call that keeps
#  them -- they are seen by where a restarted scene's tracked vehicle is.  After upload, set_dynamic_boxes, set_dynamic_obstacles and
#  set_vehicle_tracks_off the tracks are gone, and setting tracks again drops the delays by its own rule; after set_restart_noise_off
#  the noise is gone: nothing can show a delay then, and those five rows are held by the rows of "tracks" and "noise" alone.)
_rule("noise delays", "seeds = NULL switches the noise off and frees them", dropped=("set_restart_noise_off",))
_rule("observed tracks", 'What drops the observed tracks: sfm_batch_upload_state (the roles are per row); the "on" forms of sfm_batch_set_mode_fsm and '
      "sfm_batch_set_spawn_schedule (they own parking and birth); sfm_batch_set_steering(kind = NULL).  Every other call keeps them.",
      dropped=("upload", "set_modes", "set_spawns", "set_steering_off"),
      kept=_others("upload", "set_modes", "set_spawns", "set_steering_off", "set_observed_off"))
_rule("observed tracks", "obs_off = NULL switches the observed tracks off and frees them (steering stays as it is)", dropped=("set_observed_off",))
_rule("driving", "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop driving (and the vehicle observations), because the "
      "vehicles may differ; every other call keeps it", dropped=_VEHICLES, kept=_others(*_VEHICLES, "set_vehicle_driving_off"))
_rule("driving", "kind = NULL switches driving off", dropped=("set_vehicle_driving_off",))
_rule("vehicle observations", "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop driving (and the vehicle observations), because the "
      "vehicles may differ; every other call keeps it", dropped=_VEHICLES, kept=_others(*_VEHICLES, "set_vehicle_observation_off"))
_rule("vehicle observations", "sense_range = NULL switches the observations off", dropped=("set_vehicle_observation_off",))
_rule("vehicle scans", "sfm_batch_upload_state drops the scan, and so do sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles, exactly as "
      "they drop the vehicle observations (the buffer and the mask are per vehicle); every other call keeps it",
      dropped=_VEHICLES, kept=_others(*_VEHICLES, "set_vehicle_scan_off"))
_rule("vehicle scans", "max_range = NULL switches the scan off and frees the buffer", dropped=("set_vehicle_scan_off",))
_rule("routes", "sfm_batch_upload_state and sfm_batch_set_mode_fsm drop the routes", dropped=("upload", "set_modes", "set_modes_off"))
_rule("routes", "node_off = NULL switches the routes off (the queues stay as they are)", dropped=("set_routes_off",))
_rule("modes", "mode = NULL switches the modes off; so does every sfm_batch_upload_state", dropped=("upload", "set_modes_off"))
_rule("modes", "node_off = NULL switches the routes off (the queues stay as they are)", kept=("set_routes_off",))
_rule("spawns", "sfm_batch_upload_state and sfm_batch_set_mode_fsm (mode = NULL included) drop the schedule, sfm_batch_set_params keeps it",
      dropped=("upload", "set_modes", "set_modes_off"), kept=("set_params",))
_rule("spawns", "spawn_time = NULL switches the schedule off, refused (SFM_ERR_STATE) while a row is unborn", dropped=("set_spawns_off",))
_rule("tracks", "sfm_batch_set_dynamic_boxes and sfm_batch_set_dynamic_obstacles drop the tracks; sfm_batch_upload_state, sfm_batch_set_params, "
      "sfm_batch_set_mode_fsm and sfm_batch_set_spawn_schedule keep them",
      dropped=_VEHICLES, kept=("set_params", "set_modes", "set_modes_off", "set_spawns", "set_spawns_off"))
_rule("tracks", "trk_off = NULL switches the tracks off", dropped=("set_vehicle_tracks_off",))

# what goes between two generations of a reused batch: every call of the table but the on forms that need a crowd's own arguments
# again (upload, set_modes, set_spawns, set_vehicle_tracks), rotated per turn
DROP_SEQUENCE = tuple(name for name in CALLS if name not in ("upload", "set_modes", "set_spawns", "set_vehicle_tracks"))
_NEED_BOXES = ("set_vehicle_tracks_off", "set_vehicle_driving_off")      # (refused once the vehicles are rings: they go in front of those)


def drop_sequence(turn):
    """The calls between two generations: ``DROP_SEQUENCE`` rotated by ``turn`` and, for an odd ``turn``, reversed; the two off forms
    that need device-side vehicles are then moved in front of the call that turns the vehicles into rings."""
    k = turn % len(DROP_SEQUENCE)
    seq = DROP_SEQUENCE[k:] + DROP_SEQUENCE[:k]
    seq = [name for name in (seq[::-1] if turn % 2 else seq) if name not in _NEED_BOXES]
    at = seq.index("set_dynamic_obstacles")
    return tuple(seq[:at]) + (_NEED_BOXES[::-1] if turn % 2 else _NEED_BOXES) + tuple(seq[at:])
