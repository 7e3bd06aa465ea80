"""What it costs to morph a live scene's geometry, against what it replaces and against the rigid floor, on one handle in
one process (include/hpt.h, "morph targets").

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one, the sphere is morphed for
--steps steps under weights that change every step, with two sets of targets:

  sparse4   4 targets that all name the same contiguous tenth of the scene's corners (a region of the sphere, as the targets
            of a face share the face): 0.4 entries per corner overall
  dense8    8 targets that each name every corner of the sphere: 8 entries per corner

Per set, one after the other on the same handle:

  host_morph_update  hpt_morph_host followed by hpt_scene_update_triangles with its records: what the feature replaces.  Run
                     before the handle has targets, so that no rest pose is copied after it
  morph              hpt_scene_morph: one float per target

and then, once:

  pose               hpt_scene_pose with a one-part turn of the same sphere (the walls at identity): the floor the refit sets.
                     The handle holds targets by then (a deformer cannot be taken off a scene, so the morphs are timed first);
                     the pose kernel reads the morphed rest pose, which has the rest pose's bits
  morph_skin         hpt_scene_morph (sparse4) and hpt_scene_skin (bench_skin's two bones by height) in the same step, on a
                     handle that holds both: the wall clock and device part are the sums of the two calls

One JSON line with, per scene and way, the device part (ms_refit of hpt_scene_get_update_info: the morph and deformer
kernels and the refit) and the wall clock of the whole call, the first step apart (it allocates) and median and range over
steps 2 to --steps; for host_morph_update the wall clock is the sum of both calls and morph_host_ms gives the first alone.
Also whether the handle's records after the last morph were hpt_morph_host's bytes.

Usage: python scripts/bench_morph.py [--steps 16] [--tris 100000 1000000]"""
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
SETS = ("sparse4", "dense8")
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


def make_targets(tr, num_targets, corners):
    """num_targets targets over the same `corners`: target t pushes a corner away from the sphere's centre by
    0.05 * (t + 1) of its offset, turned a little further about the vertical axis with every target."""
    v = np.stack([tr["v0"], tr["v1"], tr["v2"]], axis=1).reshape(-1, 3)[corners].astype(np.float64) - CENTRE
    deltas = []
    for t in range(num_targets):
        a = 0.3 * t
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        deltas.append((v @ R.T * (0.05 * (t + 1))).astype(np.float32))
    tb = (np.arange(num_targets + 1) * len(corners)).astype(np.int32)
    return tb, np.tile(corners.astype(np.int32), num_targets), np.concatenate(deltas)


def weights_at(k, num_targets):
    return (0.5 * np.sin(0.4 * k + 0.7 * np.arange(num_targets))).astype(np.float32)


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
    part = np.ones(nt, np.int32)
    part[:NWALL] = 0
    tenth = np.arange(NWALL * 3, NWALL * 3 + (nt * 3) // 10, dtype=np.int32)
    sets = {"sparse4": make_targets(tr0, 4, tenth), "dense8": make_targets(tr0, 8, np.arange(NWALL * 3, nt * 3, dtype=np.int32))}
    out = {"triangles": int(nt), "steps": a.steps, "entries": {s: int(len(sets[s][1])) for s in SETS}}
    rows = {}
    steps = range(1, a.steps + 1)
    with hpt.Scene(L, sp, tr0) as scene:
        for s in SETS:                                               # 1. what the feature replaces
            tb, ec, ed = sets[s]
            rows["host_morph_update_" + s] = []
            for k in steps:
                w = weights_at(k, len(tb) - 1)
                t_host, tr = ms(lambda: hpt.morph_host(tr0, tb, ec, ed, w))
                t_up, _ = ms(lambda: scene.update_triangles(tr))
                info = scene.update_info()
                rows["host_morph_update_" + s].append(dict(wall=t_host + t_up, device=info["ms_refit"], morph_host_ms=t_host))
            sets[s] = (tb, ec, ed, tr)
        for s in SETS:                                               # 2. the morph
            tb, ec, ed, last = sets[s]
            scene.update_triangles(tr0)
            scene.set_morphs(tb, ec, ed)
            rows["morph_" + s] = []
            for k in steps:
                w = weights_at(k, len(tb) - 1)
                wall, _ = ms(lambda: scene.morph(w))
                info = scene.update_info()
                rows["morph_" + s].append(dict(wall=wall, device=info["ms_refit"], upload=info["ms_upload"]))
            out["same_records_as_morph_host_" + s] = bool(scene.read_triangles().tobytes() == last.tobytes())
        # 3. the rigid floor, on the same handle: it holds dense8's targets at zero weights by now, so the pose kernel reads
        # the morphed rest pose M, which has the rest pose's bits, in place of the rest pose: the same kernel, the same bytes
        scene.update_triangles(tr0)
        scene.set_parts(part, 2)
        rows["pose"] = []
        for k in steps:
            rec = turn_record(5.0 * k)
            wall, _ = ms(lambda: scene.pose(rec))
            info = scene.update_info()
            rows["pose"].append(dict(wall=wall, device=info["ms_refit"], upload=info["ms_upload"]))
        bone, weight = height_weights(tr0)                           # 4. morph and skin in one step
        scene.update_triangles(tr0)
        scene.set_skin(bone, weight, 2)
        del bone, weight
        tb, ec, ed, _ = sets["sparse4"]
        del sets["dense8"]
        scene.set_morphs(tb, ec, ed)
        rows["morph_skin"] = []
        for k in steps:
            w, rec = weights_at(k, 4), turn_record(5.0 * k)
            wall_m, _ = ms(lambda: scene.morph(w))
            dev_m = scene.update_info()["ms_refit"]
            wall_s, _ = ms(lambda: scene.skin(rec))
            dev_s = scene.update_info()["ms_refit"]
            rows["morph_skin"].append(dict(wall=wall_m + wall_s, device=dev_m + dev_s, morph_wall=wall_m, skin_wall=wall_s))
        want = hpt.skin_host(hpt.morph_host(tr0, tb, ec, ed, w), *height_weights(tr0), rec)
        out["same_records_as_morph_host_then_skin_host"] = bool(scene.read_triangles().tobytes() == want.tobytes())
    out["ways"] = {w: {"first_call": rows[w][0], "later_calls": {key: med_range([s[key] for s in rows[w][1:]]) for key in rows[w][0]}} for w in rows}
    later = {w: out["ways"][w]["later_calls"] for w in rows}
    for s in SETS:
        out["morph_to_pose_" + s] = {k: later["morph_" + s][k]["median"] / later["pose"][k]["median"] for k in ("wall", "device")}
        out["host_to_morph_wall_" + s] = later["host_morph_update_" + s]["wall"]["median"] / later["morph_" + s]["wall"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    a = ap.parse_args()
    if hpt.device_count() < 1:
        raise SystemExit("bench_morph.py: no HIP device visible")
    import torch
    torch.cuda.set_device(0)
    res = {"bench": "morph targets: hpt_scene_morph against hpt_morph_host + hpt_scene_update_triangles and against hpt_scene_pose",
           "scenes": [one_scene(n, a) for n in a.tris]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
