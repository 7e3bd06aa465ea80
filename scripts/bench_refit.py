"""What a scene update costs, against the only alternative (destroy + create), and what it costs afterwards.

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one, with the sphere turned
by 5 degrees per step about its centre, one JSON line with, per scene:

  update_ms        hpt_scene_update_triangles per step, split as hpt_update_info reports it: pack (36 bytes per triangle
                   on the host), upload (the first also allocates the scratch: given apart) and refit (HIP events around
                   the device part), and the wall clock of the whole call; median and range over the steps
  rebuild_ms       the same handle's destroy + create + first render in the same process, after the last step (the first
                   render pays for the workspaces a new handle has to allocate again); and, after 1, 4 and 16 steps,
                   create and first render of a second handle built from the step's vertices
  render_ms        the 8-spp render that follows a refit against the one that follows a rebuild of the same vertices, after
                   1, 4 and 16 steps: refitted boxes overlap more, and this is what the caller pays for not rebuilding.
                   Median of --repeats blocking renders each; the two images must be the same bytes.

Usage: python scripts/bench_refit.py [--size 512] [--spp 8] [--repeats 7] [--tris 100000 1000000]"""
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
AFTER = (1, 4, 16)


def turned(tr, degrees):
    """The sphere's triangles turned about the vertical axis through its centre."""
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    out = tr.copy()
    for k in ("v0", "v1", "v2"):
        v = out[k].astype(np.float64)
        v[NWALL:] = (v[NWALL:] - CENTRE) @ R.T + CENTRE
        out[k] = v.astype(np.float32)
    return out


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def med_range(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def render_ms(scene, cam, a):
    times, img = [], None
    for _ in range(a.repeats):
        t, img = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
        times.append(t)
    return med_range(times), img


def one_scene(n_target, a):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, a.size, a.size)
    out = {"triangles": int(len(tr0)), "image": [a.size, a.size], "spp": a.spp}
    scene = hpt.Scene(L, sp, tr0)
    out["create_ms_first"] = {"bvh_build": scene.stats()["ms_bvh_build"], "upload": scene.stats()["ms_upload"]}
    base_ms, _ = render_ms(scene, cam, a)
    out["render_ms_built_tree"] = base_ms
    steps, renders, rebuilds = [], {}, {}
    for k in range(1, max(AFTER) + 1):
        tr = turned(tr0, 5.0 * k)
        wall, _ = ms(lambda: scene.update_triangles(tr))
        info = scene.update_info()
        steps.append(dict(wall=wall, pack=info["ms_pack"], upload=info["ms_upload"], refit=info["ms_refit"]))
        if k in AFTER:
            after_refit, img_refit = render_ms(scene, cam, a)
            # a rebuild of the same vertices, on a handle of its own
            t_create, fresh = ms(lambda: hpt.Scene(L, sp, tr))
            t_first, _ = ms(lambda: fresh.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
            after_rebuild, img_rebuild = render_ms(fresh, cam, a)
            build = fresh.stats()["ms_bvh_build"]
            fresh.close()
            renders[str(k)] = {"after_refit": after_refit, "after_rebuild": after_rebuild,
                               "ratio_of_medians": after_refit["median"] / after_rebuild["median"],
                               "same_image": bool(np.array_equal(img_refit, img_rebuild))}
            rebuilds[str(k)] = {"create": t_create, "first_render": t_first, "bvh_build": build}
    # the only alternative to an update: the live handle destroyed, created again and rendered once, in the same process
    t_destroy, _ = ms(scene.close)
    t_create, scene = ms(lambda: hpt.Scene(L, sp, tr))
    t_first, _ = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
    rebuilds["same_handle"] = {"destroy": t_destroy, "create": t_create, "first_render": t_first, "total": t_destroy + t_create + t_first}
    scene.close()
    out["update_ms"] = {"first_call": steps[0],
                        "later_calls": {key: med_range([s[key] for s in steps[1:]]) for key in ("wall", "pack", "upload", "refit")}}
    out["rebuild_ms"] = rebuilds
    out["render_ms"] = renders
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tris", type=int, nargs="+", default=[100000, 1000000])
    a = ap.parse_args()
    if hpt.device_count() < 1:
        raise SystemExit("bench_refit.py: no HIP device visible")
    print(json.dumps({"bench": "scene updates: refit against rebuild", "scenes": [one_scene(n, a) for n in a.tris]}))


if __name__ == "__main__":
    main()
