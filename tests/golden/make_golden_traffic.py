#!/usr/bin/env python3
"""Golden gap-acceptance decisions and vehicle rings from the REFERENCE's own check_traffic.check_traffic and
obstacles.generate_ellipse_border, imported unmodified and called with the argument types their call sites pass
(pedestrian_simulation.py:70).  Build-container only.

check_traffic.py imports shapely and obstacles.py imports carla.  Where a real one is importable it is used; otherwise the
stand-ins under tests/golden/_standins/ are put into sys.modules first: two-point LineString / Point with exact rational
intersection and distance, and carla.Location / Rotation / Transform with the documented transform().  The fixture records which
(``backend``).  What the fixtures pin is therefore the reference's control flow and arithmetic around those primitives; the
primitives themselves are pinned only as far as the stand-ins state their definition.

Inputs come from tests/_traffic_cases.py and are not stored; each fixture holds the reference's outputs, the oracle's decision
slack and the SHA-256 of its inputs.  ``--inputs-only`` writes the digests alone (no reference code runs): the drift guard of
tests/test_traffic_golden.py.  Files are written with fixed zip time stamps, so a re-run reproduces them byte for byte."""
import argparse
import importlib
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import _traffic_cases as TC                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--inputs-only", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "traffic"))
args = ap.parse_args()


def save(name, **arrays):
    """np.savez_compressed with fixed time stamps."""
    os.makedirs(args.out, exist_ok=True)
    with zipfile.ZipFile(os.path.join(args.out, name + ".npz"), "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


sets = {"gap_random": TC.random_cases(), "gap_exact": TC.exact_cases()}
rings = TC.ring_cases()
digests = {k: TC.digest(v) for k, v in sets.items()}
digests.update({"rings_" + k: TC.digest(TC.ring_inputs(v)) for k, v in rings.items()})

if args.inputs_only:
    for name, d in digests.items():
        save(name, digest=np.array(d))
    sys.exit(0)

REF = os.environ.get("SFM_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    print("reference checkout not present -- nothing to do")
    sys.exit(0)


def backend(module):
    try:
        importlib.import_module(module)
        return "real " + module
    except ImportError:
        if os.path.join(HERE, "_standins") not in sys.path:
            sys.path.insert(1, os.path.join(HERE, "_standins"))
        importlib.import_module(module)
        return "stand-in " + module


backends = np.array([backend("shapely.geometry"), backend("carla")])
sys.path.insert(0, REF)
import carla                                              # noqa: E402  (real or stand-in)
from check_traffic import check_traffic                   # noqa: E402  (reference)
from obstacles import generate_ellipse_border             # noqa: E402  (reference)
from oracle import sfm_oracle as O                        # noqa: E402

for name, cs in sets.items():
    C = len(cs["loc"])
    decision, slack = np.zeros(C, np.uint8), np.zeros(C, np.float32)
    for g in range(len(cs["group_off"]) - 1):
        vl, vv, ve, sl = TC.group(cs, g)
        vehicles = [(vl[k].copy(), np.zeros((6, 2))) for k in range(len(vl))]          # dynamic-obstacle tuples (position, ring)
        velocities, extents = vv.copy(), [e.copy() for e in ve]
        for i in range(sl.start, sl.stop):
            ped = {"loc": np.append(cs["loc"][i], 0.0), "next_waypoint": np.append(cs["goal"][i], 0.0),
                   "mode": SimpleNamespace(crossing_speed=float(cs["speed"][i]), crossing_safety_margin=float(cs["margin"][i]))}
            decision[i] = bool(check_traffic(ped, vehicles, velocities, extents))
            slack[i] = O.gap_slack(cs["loc"][i], cs["goal"][i], cs["speed"][i], cs["margin"][i], vl, vv, ve)
    extra = {}
    if name == "gap_exact":
        # the claims of the hand-built cases, case by case: fp32 exactness, and for the diagonal headings a wide berth instead
        kinds = np.array(TC.KINDS)[cs["kind"]]
        for i in range(C):
            if kinds[i] in TC.EXACT_KINDS or kinds[i] in TC.DEGENERATE_KINDS:
                assert TC.assert_exact(cs, i) == bool(decision[i]), TC.describe(cs, i)
            else:
                assert slack[i] >= TC.ROBUST_SLACK, (TC.describe(cs, i), slack[i])
        # what a real shapely makes of a zero-length line is not the stand-in's to settle
        extra["project_defined"] = (np.isin(kinds, TC.DEGENERATE_KINDS) & backends[0].startswith("stand-in")).astype(np.uint8)
        for k in TC.KINDS[1:]:
            d = decision[kinds == k]
            print(f"  {k:28s} {len(d):4d} cases, {int((d == 0).sum()):4d} refused")
    save(name, decision=decision, slack=slack, digest=np.array(digests[name]), backend=backends, **extra)
    und = float((slack < TC.SLACK_BAND).mean())
    print(f"wrote {name}.npz: {C} cases, {100 * (decision == 0).mean():.1f} % refused, {100 * und:.2f} % below the band")

for name, (center, yaw, extent) in rings.items():
    counts, pts = [], []
    for c, y, e in zip(center, yaw, extent):
        tf = carla.Transform(carla.Location(float(c[0]), float(c[1]), 0.0), carla.Rotation(yaw=float(np.degrees(y))))
        ring = generate_ellipse_border(tf, float(e[0]), float(e[1]), TC.RESOLUTION)
        counts.append(len(ring))
        pts += [(p.x, p.y) for p in ring]
    save("rings_" + name, count=np.array(counts, np.int32), points=np.array(pts, np.float64), digest=np.array(digests["rings_" + name]),
         backend=backends)
    print(f"wrote rings_{name}.npz: {len(counts)} vehicles, {len(pts)} points, counts {min(counts)}..{max(counts)}")
