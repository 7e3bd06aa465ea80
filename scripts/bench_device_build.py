"""What a device build costs against the host rebuild it stands beside, and what its tree costs to trace (include/hpt.h,
"device builds"), on one handle per scene in one process.

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one -- bench_rebuild.py's scenes,
its two-bone twist -- one JSON line with --runs runs of, per scene:

  build        the sphere twisted 5 degrees further per step, then hpt_scene_rebuild_device and, on the same geometry and the same
               handle, hpt_scene_rebuild: the wall clock of each call, the four phases of hpt_device_build_info (HIP events) and
               the three of hpt_rebuild_info, sah and the --spp render at --size^2 after each.  First step apart (it allocates),
               median and range over steps 2 to --steps.  fell_back says whether any device build fell back to the host builder
  twist        the skin at 90, 180 and 1080 degrees from the tree built for the rest pose: the skin call (the refit every frame
               pays), then per tree -- refitted, host rebuilt, device built -- sah and the render's time (median of --repeats),
               and what a frame costs under three policies: refit only; the host rebuild when the refitted sah is above 1.5
               times the rest pose's (else refit only); a device build every frame.  The three images must be the same bytes
  kernels      with --resources: VGPRs, SGPRs, scratch and LDS of every kernel of lbvh_kernels.hip as the compiler reports them
               (hipcc -Rpass-analysis=kernel-resource-usage; needs no device)

Usage: python scripts/bench_device_build.py [--steps 16] [--runs 2] [--size 512] [--spp 8] [--repeats 7] [--tris 100000 1000000] [--resources]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_tracing_amd as hpt                                     # noqa: E402
from path_tracing_amd import scene_io as sio                        # noqa: E402
from bench_skin import height_weights, med_range, ms, turn_record   # noqa: E402

TWISTS = (90.0, 180.0, 1080.0)
POLICY_RATIO = 1.5
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")


def render_ms(scene, cam, a):
    times, img = [], None
    for _ in range(a.repeats):
        t, img = ms(lambda: scene.render_pt(cam, a.size, a.size, 4, a.spp, hpt.make_params(seed=7)))
        times.append(t)
    return med_range(times), img


def later(rows):
    return {"first_call": rows[0], "later_calls": {k: med_range([r[k] for r in rows[1:]]) for k in rows[0]}}


def one_scene(n_target, a):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, a.size, a.size)
    bone, weight = height_weights(tr0)
    out = {"triangles": int(len(tr0)), "image": [a.size, a.size], "spp": a.spp, "steps": a.steps}
    with hpt.Scene(L, sp, tr0) as scene:
        scene.set_skin(bone, weight, 2)
        # 1. the two builds on the same geometry, step after step
        dev, host, fell = [], [], 0
        for k in range(1, a.steps + 1):
            scene.skin(turn_record(5.0 * k))
            wall, _ = ms(scene.rebuild_device)
            di = scene.device_build_info()
            fell += di["fell_back"]
            r, img_d = render_ms(scene, cam, a)
            dev.append(dict(wall=wall, sort=di["ms_sort"], topology=di["ms_topology"], refit=di["ms_refit"], collapse=di["ms_collapse"],
                            sah=scene.tree_cost()["sah"], render=r["median"]))
            wall, _ = ms(scene.rebuild)
            ri = scene.rebuild_info()
            r, img_h = render_ms(scene, cam, a)
            host.append(dict(wall=wall, download=ri["ms_download"], build=ri["ms_build"], upload=ri["ms_upload"], sah=scene.tree_cost()["sah"], render=r["median"]))
            assert np.array_equal(img_d, img_h)
        di = scene.device_build_info()
        out["build"] = {"device": later(dev), "host": later(host), "fell_back": int(fell), "nodes": di["nodes_after"], "depth": di["depth_after"],
                        "wide_depth": di["wide_depth"], "host_nodes": scene.stats()["bvh_nodes"], "host_depth": scene.stats()["bvh_depth"]}
        d, h = out["build"]["device"]["later_calls"], out["build"]["host"]["later_calls"]
        out["build"]["host_wall_over_device_wall"] = h["wall"]["median"] / d["wall"]["median"]
        out["build"]["device_render_over_host_render"] = d["render"]["median"] / h["render"]["median"]
        # 2. the twist: what a frame costs under each policy
        twists = {}
        for deg in TWISTS:
            scene.skin(turn_record(0.0))
            scene.rebuild()                                          # the tree of the rest pose
            sah_rest = scene.tree_cost()["sah"]
            skins = []
            for _ in range(a.repeats):
                scene.skin(turn_record(0.0))
                skins.append(ms(lambda: scene.skin(turn_record(deg)))[0])
            r = {"skin_ms": med_range(skins), "sah_rest": sah_rest}
            imgs = []
            for key, build in (("refitted", None), ("host", scene.rebuild), ("device", scene.rebuild_device)):
                walls = []
                if build:
                    for _ in range(3):
                        walls.append(ms(build)[0])
                t, img = render_ms(scene, cam, a)
                imgs.append(img)
                r[key] = {"sah": scene.tree_cost()["sah"], "render_ms": t, "build_ms": med_range(walls) if walls else None}
            r["same_image"] = bool(all(np.array_equal(imgs[0], i) for i in imgs[1:]))
            skin = r["skin_ms"]["median"]
            over = r["refitted"]["sah"] > POLICY_RATIO * sah_rest
            r["frame_ms"] = {"refit_only": skin + r["refitted"]["render_ms"]["median"],
                             "host_rebuild_above_1.5": skin + (r["host"]["build_ms"]["median"] + r["host"]["render_ms"]["median"] if over else r["refitted"]["render_ms"]["median"]),
                             "host_policy_rebuilds": bool(over),
                             "device_build_every_frame": skin + r["device"]["build_ms"]["median"] + r["device"]["render_ms"]["median"]}
            r["fell_back"] = int(scene.device_build_info()["fell_back"])
            twists[str(int(deg))] = r
        out["twist"] = twists
    return out


def kernel_resources():
    """Per kernel of lbvh_kernels.hip what the compiler's resource remarks say."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(CSRC, "lbvh_kernels.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark: \S*\s*(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return {k: v for k, v in out.items() if "lbvh" in k}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    out = {"bench": "device build against host rebuild"}
    if a.resources:
        out["kernels"] = kernel_resources()
    if a.tris:
        if hpt.device_count() < 1:
            raise SystemExit("bench_device_build.py: no HIP device visible")
        out["runs"] = [[one_scene(n, a) for n in a.tris] for _ in range(a.runs)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
