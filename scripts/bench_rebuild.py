"""What it costs to measure a live tree and to rebuild it in place, and what a rebuild buys (include/hpt.h, "tree cost" and
"rebuild"), on one handle per scene in one process.

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one, one JSON line with, per
scene:

  tree_cost    hpt_scene_tree_cost, --steps calls: the wall clock of the whole blocking call and the time between two events
               on the null stream around it (the memset, the kernel and the 96-byte read-back); beside it a device-to-device
               copy of the same num_nodes * 32 bytes between events, and the --spp render at --size^2 it would accompany
               each frame.  First call apart (it allocates the result), median and range over calls 2 to --steps
  rebuild      the sphere twisted 5 degrees further per step through a two-bone skin weighted by height (bench_skin.py's),
               then hpt_scene_rebuild: the wall clock of the whole call and its three parts as hpt_rebuild_info reports them
               (the lazy download of the vertices, the host builder, the upload with the triangle frames), and the first
               render afterwards; against what it replaces, on the same records: destroy + create + first render
  twist        the same skin at 90, 180, 360 and 1080 degrees, each from the tree built for the rest pose (the skin at 0
               degrees and a rebuild come first): sah, the render's time (median of --repeats) and the counting kernels'
               nodes and triangles per closest-hit and per shadow ray on the refitted tree, then the same three after a rebuild; the two images must be
               the same bytes.  (Bone 1 turns, bone 0 stays, and the blend is linear: at a multiple of 360 degrees bone 1 is
               the identity up to rounding and the mesh is back at its rest pose; at 180 its waist has collapsed.)

Usage: python scripts/bench_rebuild.py [--steps 16] [--size 512] [--spp 8] [--repeats 7] [--tris 100000 1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_tracing_amd as hpt                                     # noqa: E402
from path_tracing_amd import scene_io as sio                        # noqa: E402
from bench_skin import height_weights, med_range, ms, turn_record   # noqa: E402

TWISTS = (90.0, 180.0, 360.0, 1080.0)


def render_ms(scene, cam, a, flags=0):
    times, img = [], None
    for _ in range(a.repeats):
        t, img = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7, flags=flags)))
        times.append(t)
    return med_range(times), img


def work_per_ray(scene, cam, a):
    """The counting kernels' work on this tree: nodes visited (two boxes each) and triangles tested per closest-hit ray and
    per shadow ray."""
    scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7, flags=hpt.FLAG_COUNT_WORK))
    st = scene.stats()
    c, s = max(st["closest_rays"], 1), max(st["shadow_rays"], 1)
    return {"boxes_per_closest_ray": st["boxes_closest"] / 2 / c, "tris_per_closest_ray": st["tris_closest"] / c,
            "boxes_per_shadow_ray": st["boxes_shadow"] / 2 / s, "tris_per_shadow_ray": st["tris_shadow"] / s}


def later(rows):
    return {"first_call": rows[0], "later_calls": {k: med_range([r[k] for r in rows[1:]]) for k in rows[0]}}


def one_scene(torch, n_target, a):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, a.size, a.size)
    bone, weight = height_weights(tr0)
    out = {"triangles": int(len(tr0)), "image": [a.size, a.size], "spp": a.spp, "steps": a.steps}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    scene = hpt.Scene(L, sp, tr0)
    base_render, _ = render_ms(scene, cam, a)
    out["render_ms_built_tree"] = base_render

    # 1. the measurement
    rows = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        ev[0].record()
        wall, cost = ms(scene.tree_cost)
        ev[1].record()
        torch.cuda.synchronize()
        rows.append(dict(wall=wall, device=ev[0].elapsed_time(ev[1])))
    nbytes = cost["num_nodes"] * 32
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    copies = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        copies.append(dict(device=ev[0].elapsed_time(ev[1])))
    out["tree_cost"] = {"num_nodes": cost["num_nodes"], "qnodes_bytes": nbytes, "sah": cost["sah"], "call": later(rows), "d2d_copy": later(copies)}
    out["tree_cost"]["wall_share_of_render"] = out["tree_cost"]["call"]["later_calls"]["wall"]["median"] / base_render["median"]

    # 2. the rebuild, against destroy + create + first render of the same records
    scene.set_skin(bone, weight, 2)
    rows = []
    for k in range(1, a.steps + 1):
        scene.skin(turn_record(5.0 * k))
        wall, _ = ms(scene.rebuild)
        ri = scene.rebuild_info()
        first, _ = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
        rows.append(dict(wall=wall, download=ri["ms_download"], build=ri["ms_build"], upload=ri["ms_upload"], first_render=first))
    T = scene.read_triangles()
    t_destroy, _ = ms(scene.close)
    t_create, scene = ms(lambda: hpt.Scene(L, sp, T))
    t_first, _ = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
    replaced = {"destroy": t_destroy, "create": t_create, "first_render": t_first, "total": t_destroy + t_create + t_first}
    out["rebuild"] = {"call": later(rows), "destroy_create_first_render": replaced}
    lc = out["rebuild"]["call"]["later_calls"]
    out["rebuild"]["replaced_to_rebuild_with_first_render"] = replaced["total"] / (lc["wall"]["median"] + lc["first_render"]["median"])
    scene.close()

    # 3. what it buys: a twist far from the built pose
    scene = hpt.Scene(L, sp, tr0)
    scene.set_skin(bone, weight, 2)
    twists = {}
    for deg in TWISTS:
        scene.skin(turn_record(0.0))
        scene.rebuild()                                              # the tree of the rest pose
        scene.skin(turn_record(deg))
        r = {"refitted": {}, "rebuilt": {}}
        imgs = []
        for key in ("refitted", "rebuilt"):
            if key == "rebuilt":
                scene.rebuild()
            t, img = render_ms(scene, cam, a)
            imgs.append(img)
            cost = scene.tree_cost()
            r[key] = dict(work_per_ray(scene, cam, a), sah=cost["sah"], box_visits=cost["box_visits"], tri_tests=cost["tri_tests"], render_ms=t)
        r["render_ratio_of_medians"] = r["refitted"]["render_ms"]["median"] / r["rebuilt"]["render_ms"]["median"]
        r["same_image"] = bool(np.array_equal(imgs[0], imgs[1]))
        twists[str(int(deg))] = r
    out["twist"] = twists
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    a = ap.parse_args()
    if hpt.device_count() < 1:
        raise SystemExit("bench_rebuild.py: no HIP device visible")
    import torch
    torch.cuda.set_device(0)
    print(json.dumps({"bench": "tree cost and rebuild in place", "scenes": [one_scene(torch, n, a) for n in a.tris]}))


if __name__ == "__main__":
    main()
