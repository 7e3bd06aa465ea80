"""What it costs to deform a live scene's geometry, against what it replaces and against the rigid floor, on one handle in
one process (include/hpt.h, "skinning").

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one, the sphere is twisted by
5 degrees per step about the vertical axis through its centre for --steps steps, through a two-bone skin weighted by height
(bone 0 at identity, bone 1 the turn; the walls have four zero weights).  Three ways, one after the other on the same handle:

  host_skin_update hpt_skin_host followed by hpt_scene_update_triangles with its records: what the feature replaces.  Run
                   first, before the handle has a deformer, so that no rest pose is copied after it
  skin             hpt_scene_skin: two records of twelve floats
  pose             hpt_scene_pose with a one-part turn of the same sphere (the walls at identity): the rigid floor -- the
                   difference to `skin` is what the influence table costs

One JSON line with, per scene and way, the device part (ms_refit of hpt_scene_get_update_info: the skin or pose kernel and
the refit) and the wall clock of the whole call, the first step apart (it allocates) and median and range over steps 2 to
--steps; for host_skin_update the wall clock is the sum of both calls and skin_host_ms gives the first alone.  Also whether
the handle's records after the last skin were hpt_skin_host's bytes.

Usage: python scripts/bench_skin.py [--steps 16] [--tris 100000 1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import path_tracing_amd as hpt                                     # noqa: E402
from path_tracing_amd import scene_io as sio                        # noqa: E402

NWALL = 12
CENTRE = np.array((-0.15, 0.2, 0.45))
WAYS = ("host_skin_update", "skin", "pose")
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32).reshape(3, 4)


def turn_record(degrees):
    """x -> R (x - c) + c about the vertical axis through the sphere's centre, built in double and rounded once."""
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    r = np.zeros((3, 4))
    r[:, :3] = R
    r[:, 3] = CENTRE - R @ CENTRE
    return np.stack([IDENTITY, r.astype(np.float32)]).astype(np.float32)


def height_weights(tr):
    """t = clamp((y - ymin) / (ymax - ymin), 0, 1) on bone 1 and 1 - t on bone 0 for the sphere's corners, in float32."""
    n = len(tr)
    bone, weight = np.zeros((n, 3, 4), np.int32), np.zeros((n, 3, 4), np.float32)
    y = np.stack([tr["v0"], tr["v1"], tr["v2"]], axis=1)[NWALL:, :, 1].astype(np.float32)
    lo, hi = np.float32(y.min()), np.float32(y.max())
    t = np.clip((y - lo) / (hi - lo), np.float32(0), np.float32(1)).astype(np.float32)
    bone[NWALL:, :, 1] = 1
    weight[NWALL:, :, 0] = np.float32(1) - t
    weight[NWALL:, :, 1] = t
    return bone, weight


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def med_range(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def one_scene(n_target, a):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    nt = len(tr0)
    bone, weight = height_weights(tr0)
    part = np.ones(nt, np.int32)
    part[:NWALL] = 0
    out = {"triangles": int(nt), "steps": a.steps}
    rows = {w: [] for w in WAYS}
    steps = range(1, a.steps + 1)
    with hpt.Scene(L, sp, tr0) as scene:
        for k in steps:                                              # 1. what the feature replaces
            rec = turn_record(5.0 * k)
            t_host, tr = ms(lambda: hpt.skin_host(tr0, bone, weight, rec))
            t_up, _ = ms(lambda: scene.update_triangles(tr))
            info = scene.update_info()
            rows["host_skin_update"].append(dict(wall=t_host + t_up, device=info["ms_refit"], skin_host_ms=t_host))
        scene.update_triangles(tr0)
        scene.set_skin(bone, weight, 2)
        for k in steps:                                              # 2. the skin
            rec = turn_record(5.0 * k)
            wall, _ = ms(lambda: scene.skin(rec))
            info = scene.update_info()
            rows["skin"].append(dict(wall=wall, device=info["ms_refit"], upload=info["ms_upload"]))
        out["same_records_as_skin_host"] = bool(scene.read_triangles().tobytes() == tr.tobytes())
        scene.update_triangles(tr0)
        scene.set_parts(part, 2)
        for k in steps:                                              # 3. the rigid floor
            rec = turn_record(5.0 * k)
            wall, _ = ms(lambda: scene.pose(rec))
            info = scene.update_info()
            rows["pose"].append(dict(wall=wall, device=info["ms_refit"], upload=info["ms_upload"]))
    out["ways"] = {w: {"first_call": rows[w][0], "later_calls": {key: med_range([s[key] for s in rows[w][1:]]) for key in rows[w][0]}} for w in WAYS}
    later = {w: out["ways"][w]["later_calls"] for w in WAYS}
    out["skin_to_pose"] = {k: later["skin"][k]["median"] / later["pose"][k]["median"] for k in ("wall", "device")}
    out["host_to_skin_wall"] = later["host_skin_update"]["wall"]["median"] / later["skin"]["wall"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    a = ap.parse_args()
    if hpt.device_count() < 1:
        raise SystemExit("bench_skin.py: no HIP device visible")
    import torch
    torch.cuda.set_device(0)
    res = {"bench": "skinning: hpt_scene_skin against hpt_skin_host + hpt_scene_update_triangles and against hpt_scene_pose",
           "scenes": [one_scene(n, a) for n in a.tris]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
