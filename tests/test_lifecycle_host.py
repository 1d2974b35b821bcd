"""Host tests of the lifecycle cases (tests/_lifecycle_cases.py): the drop table covers every feature block of struct SfmBatch and
quotes the header; every call and getter it names exists; and the designed crowds are not vacuous -- checked with the package's own
twins on the initial states, before any GPU is involved."""
import os
import re

import numpy as np
import pytest

import _lifecycle_cases as LC
from carla_social_force_model_amd import _lib, grid, reset, route, scan
from carla_social_force_model_amd.batch import SfmBatch, pack_route_rows, pack_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carla-social-force-model_amd", "csrc")
CROWDS = [(p, g, v) for p in LC.PROFILES for g, v in (("A", 0), ("B", 0), ("B", 1), ("C", 0))]
VS = LC.VEHICLE_SCENE


def _text(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


def batch_members():
    """name -> type of every member of struct SfmBatch whose type is an sfm::Batch...Dev struct (csrc/sfm_batch_host.h)."""
    body = re.search(r"^struct SfmBatch \{(.*?)^\};", _text(CSRC, "sfm_batch_host.h"), re.S | re.M).group(1)
    return {name: typ for typ, name in re.findall(r"^\s*sfm::(Batch\w+Dev)\s+(\w+)", body, re.M)}


def test_every_feature_block_of_the_batch_has_a_lifecycle_row():
    """A Batch...Dev member of struct SfmBatch is the member of a feature of DROPS, or is listed in NOT_FEATURES with the reason."""
    members = batch_members()
    assert len(members) >= 19 and {"snap", "routes", "rec", "geo"} <= set(members), members      # (the parse found the struct)
    in_drops = {f for _, f in LC.DROPS}
    assert in_drops == set(LC.FEATURES), in_drops ^ set(LC.FEATURES)
    covered = {LC.FEATURES[f][0] for f in in_drops} | set(LC.NOT_FEATURES)
    assert set(members) - covered == set(), f"no lifecycle row for {sorted(set(members) - covered)}"
    assert covered - set(members) == set(), f"not in struct SfmBatch: {sorted(covered - set(members))}"


def test_a_member_without_a_row_is_noticed():
    """The check above with one feature's rows taken out: its member is reported."""
    members = batch_members()
    left = {f for _, f in LC.DROPS if f != "grids"}
    covered = {LC.FEATURES[f][0] for f in left} | set(LC.NOT_FEATURES)
    assert set(members) - covered == {"grid"}


def test_every_row_quotes_the_header():
    header = re.sub(r"\s*\n \*\s*", " ", _text(ROOT, "include", "sfm_hip.h"))
    flat = lambda s: re.sub(r"\s+", " ", s)
    header = flat(header)
    for (call, feature), (outcome, quote) in LC.DROPS.items():
        assert outcome in (LC.KEPT, LC.DROPPED) and call in LC.CALLS and feature in LC.FEATURES
        assert len(quote) > 20 and flat(quote) in header, (call, feature, quote)


def test_calls_and_getters_exist():
    host = _text(CSRC, "sfm_batch_host.h") + "".join(_text(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith("_capi.hip"))
    for name, (method, _) in LC.CALLS.items():
        assert callable(getattr(SfmBatch, method, None)) or method in _lib.SYMBOLS, name
        assert LC.SETUPS[name] and set(LC.SETUPS[name]) <= set(LC.HOLDS)
    for feature, (member, getter, message, probe) in LC.FEATURES.items():
        if getter is not None:
            assert callable(getattr(SfmBatch, getter, None)), feature
            assert message in host, (feature, message)
            assert len(_lib.SYMBOLS[probe[0]][1]) == 1 + probe[1], (feature, probe)


def test_every_off_form_drops_its_own_feature():
    offs = {name for name in LC.CALLS if name.endswith("_off")}
    assert offs == set(LC.OWN_FEATURE)
    for call, feature in LC.OWN_FEATURE.items():
        assert LC.DROPS.get((call, feature), (None,))[0] == LC.DROPPED, (call, feature)


def test_every_row_is_held_by_a_set_up_of_its_call():
    """A row of DROPS is checked on the set-ups of its call that hold its feature: there is one for every row, but for those that no
    sequence of accepted calls reaches, which are listed with the reason."""
    assert all(set(held) <= set(LC.FEATURES) for held in LC.HOLDS.values())
    unheld = {(call, f) for call, f in LC.DROPS if not any(f in LC.HOLDS[s] for s in LC.SETUPS[call])}
    assert unheld == set(LC.UNREACHABLE), unheld ^ set(LC.UNREACHABLE)
    assert all(row in LC.DROPS and len(why) > 20 for row, why in LC.UNREACHABLE.items())


@pytest.mark.parametrize("profile,gen,variant", CROWDS)
def test_the_crowds_are_what_the_table_says(profile, gen, variant):
    c = LC.crowd(profile, gen, variant)
    g = LC.GEN[gen]
    pk = pack_scenes(c["scenes"])
    assert tuple(np.diff(pk["scene_off"])) == g["rows"] and pk["planar"] == c["planar"]
    assert c["planar"] == (not (profile == "policy" and gen in "AC"))
    assert len(c["scenes"][VS]["dynamic_obstacles"]) == g["vehicles"] and all(not c["scenes"][k]["dynamic_obstacles"] for k in (0, 1))
    masks = [c["scan"]["mask"], c["grid"]["mask"]] + ([c["vobs"]["mask"], c["vscan"]["mask"], c["routes"]["mask"]] if profile == "policy" else [])
    assert all((m is None) == (gen == "B") for m in masks)
    if profile == "replay":
        roles = np.concatenate(c["observed"]["roles"])
        assert set(roles) == {0, 1, 2}
    else:
        assert set(np.concatenate(c["kinds"])) == {0, 1, 2}
        assert len(route.pack_graph(c["routes"]["graphs"][VS])["xy"]) == g["nodes"]


def test_the_generations_grow_and_shrink():
    a, b, c = (LC.GEN[k] for k in "ABC")
    for key in ("vehicles", "nodes", "k", "R", "G", "cap", "vk", "vR"):
        assert a[key] < c[key] < b[key] or (key == "vehicles" and c[key] < a[key] < b[key]), key
    rows = [r for g in (a, b, c) for r in g["rows"] if r]                 # the three j-split forms of the batch tick
    assert any(r <= 64 for r in rows) and any(64 < r <= 128 for r in rows) and any(r > 128 for r in rows)
    assert all(x < y for x, y in zip(c["rows"], b["rows"])) and c["rows"][:2] == (1, 64) and c["rows"][2] == 65


def _route_plans(c):
    r = c["routes"]
    so = pack_scenes(c["scenes"])["scene_off"]
    gt = pack_route_rows(r["graph_types"], r["goals"], r["mask"], so)[0]
    out = []
    for k, sc in enumerate(c["scenes"]):
        plans = route.plan_scene(route.pack_graph(r["graphs"][k]), gt[so[k]:so[k + 1]], sc["loc"], r["goals"][k], r["capacity"],
                                 modes=c["plans"][k]["mode"])
        out += [p for p in plans if p is not None]
    return out


@pytest.mark.parametrize("gen,variant", [("A", 0), ("B", 0), ("B", 1), ("C", 0)])
def test_routes_are_planned_and_refused(gen, variant):
    """From where the rows stand at the upload: a planned route of at least three entries, and a row with another status."""
    plans = _route_plans(LC.crowd("policy", gen, variant))
    assert any(p["status"] == route.STATUS_PLANNED and p["L"] >= 3 for p in plans)
    assert any(p["status"] != route.STATUS_PLANNED for p in plans), sorted({p["status"] for p in plans})


def route_lds_bytes(v_cap, a_cap):
    """csrc/sfm_batch_route.hip's route_lds_bytes, with its four waves per workgroup."""
    src = _text(CSRC, "sfm_batch_route.hip")
    assert "sizeof(int) * ((size_t)v_cap + 2) + sizeof(uint2) * (size_t)a_cap + (size_t)WAVES_PER_BLOCK * 10 * (size_t)v_cap" in src
    assert re.search(r"constexpr int BLOCK = 256;", _text(CSRC, "sfm_device.h"))
    return 4 * (v_cap + 2) + 8 * a_cap + 4 * 10 * v_cap


@pytest.mark.parametrize("gen,staged", [("A", True), ("B", False), ("C", True)])
def test_where_the_plan_kernel_reads_the_adjacency(gen, staged):
    """B's largest graph has more adjacency entries than the launch's LDS stages (they are read from global memory); A's and C's
    have fewer."""
    graphs = [route.pack_graph(g) for g in LC.crowd("policy", gen)["routes"]["graphs"] if g is not None]
    v_cap = max(64, (max(len(g["xy"]) for g in graphs) + 63) // 64 * 64)
    room = (65536 - route_lds_bytes(v_cap, 0)) // 8
    entries = max(int(g["off"][-1]) for g in graphs)
    assert (entries <= room) == staged, (entries, room)
    if gen == "B":
        assert entries > 2559


def _scene_value(v, k):
    return v[k] if isinstance(v, (tuple, list)) else v


@pytest.mark.parametrize("profile,gen,variant", CROWDS)
def test_the_row_sensors_see_something(profile, gen, variant):
    """Over the scenes of a crowd: a scan ray that hits and one that misses, a grid with a pedestrian cell and a geometry cell."""
    c = LC.crowd(profile, gen, variant)
    s, gr = c["scan"], c["grid"]
    hit = miss = peds = geo = False
    for k, sc in enumerate(c["scenes"]):
        if not len(sc["loc"]):
            continue
        m = None if s["mask"] is None else s["mask"][k]
        rec = scan.scan_scene(sc, scan.default_angles(s["R"]), s["max_range"][k], s["ped_radius"], scan.POINT_RADIUS, frame=s["frame"], mask=m)
        kinds = rec[:, s["R"]:][slice(None) if m is None else m]
        hit, miss = hit or bool((kinds > 0).any()), miss or bool((kinds == 0).any())
        cells = grid.grid_scene(sc, gr["G"], _scene_value(gr["cell"], k), frame=gr["frame"], mask=None if gr["mask"] is None else gr["mask"][k])
        peds, geo = peds or bool(cells[:, 0].any()), geo or bool(cells[:, 3:].any())
    assert hit and miss and peds and geo, (hit, miss, peds, geo)


@pytest.mark.parametrize("gen,variant", [("A", 0), ("B", 0), ("B", 1), ("C", 0)])
def test_the_vehicle_scan_sees_something(gen, variant):
    c = LC.crowd("policy", gen, variant)
    s = c["vscan"]
    m = None if s["mask"] is None else s["mask"][VS]
    rec = scan.scan_vehicles_scene(c["scenes"][VS], scan.default_angles(s["R"], scan.MAX_VEHICLE_SCAN_RAYS), s["max_range"][VS], s["ped_radius"],
                                   scan.POINT_RADIUS, frame=s["frame"], mask=m, mount=s["mount"])
    kinds = rec[:, s["R"]:][slice(None) if m is None else m]
    assert (kinds > 0).any() and (kinds == 0).any()


@pytest.mark.parametrize("profile,gen,variant", CROWDS)
def test_the_restart_noise_moves_rows_and_delays_the_track(profile, gen, variant):
    """A restart of the uploaded state under the crowd's noise: scene 1 (the one whose episode ends) has a row that moves, and the
    tracked vehicle of scene 2 arrives later at the scene's first restart."""
    c = LC.crowd(profile, gen, variant)
    nz = c["noise"]
    sc = c["scenes"][1]
    xy = reset.resample_scene(sc, nz["seeds"][1], 0, nz["pos_box"], nz["goal_box"], nz["min_gap"], nz["point_gap"], nz["tries"])[0]
    assert (xy != np.float32(sc["loc"][:, :2])).any()
    word = reset.reset_word(int(nz["seeds"][VS]), 0, 0, 0, reset.C_DELAY)
    assert reset.delay_ticks(word, c["track_delay"][0]) > 0
