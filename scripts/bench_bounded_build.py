"""What a bounded device build costs against the unbounded one and the host rebuild, and what its tree costs to trace
(include/hpt.h, "bounded device builds"), on one handle per scene in one process: bench_device_build.py's protocol and scenes
(cornell_with_sphere(100000): 99 024 triangles, and the 998 296-triangle one; bench_rebuild.py's two-bone twist).

One JSON line with --runs runs of, per scene:

  build        the sphere twisted 5 degrees further per step, then on the same geometry and the same handle
               hpt_scene_rebuild_device, hpt_scene_rebuild_device_bounded(--depth) and hpt_scene_rebuild: the wall clock of each
               call, the four phases of hpt_device_build_info for the bounded build, sah and the --spp render at --size^2 after
               the bounded and the host one.  First step apart (it allocates), median and range over steps 2 to --steps.
               fallbacks: how many of the --steps calls fell back to the host builder, per kind; bvh_depth, wide_depth,
               forced_nodes and first_forced_level of the last bounded build
  poses        the skin at 0 (rest), 90, 180 and 1080 degrees from the tree built for the rest pose: the skin call, then per
               tree -- refitted, host rebuilt, bounded, unbounded -- the build (median of three), sah and the render's time
               (median of --repeats), whether each device build fell back, the depths and forced nodes, and what a frame
               costs when it refits only, builds bounded every frame, or rebuilds on the host every frame.  Same image bytes
  --host-only  no device: hpt_bvh_device_build_bounded_host on both scenes at those poses -- bvh_depth, wide_depth,
               forced_nodes, fell_back of the bounded definition at --depth and of the unbounded one

Usage: python scripts/bench_bounded_build.py [--depth 0] [--steps 16] [--runs 2] [--size 512] [--spp 8] [--repeats 7]
                                             [--tris 100000 1000000] [--host-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_tracing_amd as hpt                                     # noqa: E402
from path_tracing_amd import scene_io as sio                        # noqa: E402
from bench_device_build import later, render_ms                     # noqa: E402
from bench_skin import height_weights, med_range, ms, turn_record   # noqa: E402

POSES = (0.0, 90.0, 180.0, 1080.0)


def tree_of(scene):
    di, bi = scene.device_build_info(), scene.bounded_build_info()
    return {"fell_back": int(di["fell_back"]), "bvh_depth": di["depth_after"], "wide_depth": di["wide_depth"], "nodes": di["nodes_after"],
            "forced_nodes": bi["forced_nodes"], "first_forced_level": bi["first_forced_level"], "max_depth": bi["max_depth"]}


def one_scene(n_target, a):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, a.size, a.size)
    bone, weight = height_weights(tr0)
    bounded = lambda s: s.rebuild_device_bounded(a.depth)
    out = {"triangles": int(len(tr0)), "image": [a.size, a.size], "spp": a.spp, "steps": a.steps, "depth": a.depth}
    with hpt.Scene(L, sp, tr0) as scene:
        scene.set_skin(bone, weight, 2)
        # 1. the three builds on the same geometry, step after step
        plain, bnd, host, fell_plain, fell_bounded = [], [], [], 0, 0
        for k in range(1, a.steps + 1):
            scene.skin(turn_record(5.0 * k))
            wall, _ = ms(scene.rebuild_device)
            fell_plain += scene.device_build_info()["fell_back"]
            plain.append(dict(wall=wall))
            wall, _ = ms(lambda: bounded(scene))
            di = scene.device_build_info()
            fell_bounded += di["fell_back"]
            r, img_b = render_ms(scene, cam, a)
            bnd.append(dict(wall=wall, sort=di["ms_sort"], topology=di["ms_topology"], refit=di["ms_refit"], collapse=di["ms_collapse"],
                            sah=scene.tree_cost()["sah"], render=r["median"]))
            last = tree_of(scene)
            wall, _ = ms(scene.rebuild)
            ri = scene.rebuild_info()
            r, img_h = render_ms(scene, cam, a)
            host.append(dict(wall=wall, download=ri["ms_download"], build=ri["ms_build"], upload=ri["ms_upload"], sah=scene.tree_cost()["sah"], render=r["median"]))
            assert np.array_equal(img_b, img_h)
        out["build"] = {"bounded": later(bnd), "unbounded": later(plain), "host": later(host),
                        "fallbacks": {"unbounded": int(fell_plain), "bounded": int(fell_bounded), "of": a.steps}, "last_bounded": last}
        b, h = out["build"]["bounded"]["later_calls"], out["build"]["host"]["later_calls"]
        out["build"]["host_wall_over_bounded_wall"] = h["wall"]["median"] / b["wall"]["median"]
        out["build"]["bounded_render_over_host_render"] = b["render"]["median"] / h["render"]["median"]
        # 2. the poses: what a frame costs under each policy
        poses = {}
        for deg in POSES:
            scene.skin(turn_record(0.0))
            scene.rebuild()                                          # the tree of the rest pose
            skins = []
            for _ in range(a.repeats):
                scene.skin(turn_record(0.0))
                skins.append(ms(lambda: scene.skin(turn_record(deg)))[0])
            r = {"skin_ms": med_range(skins), "sah_rest": scene.tree_cost()["sah"] if deg == 0.0 else poses["0"]["sah_rest"]}
            imgs = []
            for key, build in (("refitted", None), ("host", scene.rebuild), ("bounded", lambda: bounded(scene)), ("unbounded", scene.rebuild_device)):
                walls = []
                if build:
                    for _ in range(3):
                        walls.append(ms(build)[0])
                t, img = render_ms(scene, cam, a)
                imgs.append(img)
                r[key] = {"sah": scene.tree_cost()["sah"], "render_ms": t, "build_ms": med_range(walls) if walls else None}
                if key in ("bounded", "unbounded"):
                    r[key]["tree"] = tree_of(scene)
            r["same_image"] = bool(all(np.array_equal(imgs[0], i) for i in imgs[1:]))
            skin = r["skin_ms"]["median"]
            r["frame_ms"] = {"refit_only": skin + r["refitted"]["render_ms"]["median"],
                             "bounded_build_every_frame": skin + r["bounded"]["build_ms"]["median"] + r["bounded"]["render_ms"]["median"],
                             "host_rebuild_every_frame": skin + r["host"]["build_ms"]["median"] + r["host"]["render_ms"]["median"]}
            poses[str(int(deg))] = r
        out["poses"] = poses
    return out


def host_only(n_target, a):
    """The definitions alone: the depths of both trees at every pose."""
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    bone, weight = height_weights(tr0)
    out = {"triangles": int(len(tr0)), "depth": a.depth, "poses": {}}
    for deg in POSES:
        tr = hpt.skin_host(tr0, bone, weight, turn_record(deg)) if deg else tr0
        row = {}
        for key, bvh in (("bounded", hpt.device_build_bounded_bvh_host(L, sp, tr, None, a.depth)), ("unbounded", hpt.device_build_bvh_host(L, sp, tr))):
            row[key] = {"bvh_depth": bvh["bvh_depth"], "wide_depth": bvh["build"]["wide_depth"], "fell_back": bvh["build"]["fell_back"], "nodes": bvh["num_nodes"]}
            if key == "bounded":
                row[key].update(bvh["bounded"])
        out["poses"][str(int(deg))] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    out = {"bench": "bounded device build against the unbounded one and the host rebuild", "depth": a.depth}
    if a.host_only:
        out["host"] = [host_only(n, a) for n in a.tris]
    else:
        if hpt.device_count() < 1:
            raise SystemExit("bench_bounded_build.py: no HIP device visible")
        out["runs"] = [[one_scene(n, a) for n in a.tris] for _ in range(a.runs)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
