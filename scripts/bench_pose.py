"""What it costs to move a live scene's geometry, three ways, on one handle in one process (include/hpt.h, "poses").

On config 3's scene (cornell_with_sphere(100000): 99 024 triangles) and the 998 296-triangle one, the sphere is turned by
5 degrees per step about its centre for --steps steps.  Every step brings the SAME vertices to the handle three times, in
this order, each followed by the 8-spp render:

  pose             hpt_scene_pose: two records of twelve floats (the walls at identity, the sphere's turn)
  device_verts     hpt_scene_update_vertices_device, from vertices a torch kernel turned on the device with the pose's own
                   operations in the pose's order (its time is given apart, as torch_ms)
  update_triangles hpt_scene_update_triangles, the yardstick: the records of hpt_pose_host, made before the clock starts

Between steps the handle is taken back to the rest pose by an update_triangles that is not timed (an update that is not a
pose resets the rest pose, and poses are absolute).  One JSON line with, per scene and way, the wall clock of the whole
call and its split as hpt_scene_get_update_info reports it (pack, upload, refit), the first step apart (it allocates) and
median and range over steps 2 to --steps, the render that follows, and whether the three images of every step were the same
bytes.  With --cli, pt_cli --spin against --spin-device on an OBJ of --cli-tris triangles: seconds per frame, from the
difference between a long and a short run.

Usage: python scripts/bench_pose.py [--size 512] [--spp 8] [--steps 16] [--repeats 3] [--tris 100000 1000000] [--cli]   (--tris with no value: the CLI part alone)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import path_tracing_amd as hpt                                     # noqa: E402
from path_tracing_amd import scene_io as sio                        # noqa: E402

NWALL = 12
CENTRE = np.array((-0.15, 0.2, 0.45))
WAYS = ("pose", "device_verts", "update_triangles")
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32).reshape(3, 4)


def turn_record(degrees):
    """x -> R (x - c) + c about the vertical axis through the sphere's centre, built in double and rounded once."""
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    r = np.zeros((3, 4))
    r[:, :3] = R
    r[:, 3] = CENTRE - R @ CENTRE
    return np.stack([IDENTITY, r.astype(np.float32)]).astype(np.float32)


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
    return float(np.median(times)), img


def torch_turn(torch, rest, rec):
    """The pose's arithmetic on the sphere's vertices, one torch kernel per operation: the same float32 bytes."""
    v = rest.clone()
    x, y, z = (rest[NWALL:, :, k] for k in range(3))
    for a in range(3):
        s = rec[a, 0] * x
        s = s + rec[a, 1] * y
        s = s + rec[a, 2] * z
        v[NWALL:, :, a] = s + rec[a, 3]
    return v


def one_scene(n_target, a, torch):
    L, sp, tr0 = sio.cornell_with_sphere(n_target)
    nt = len(tr0)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, a.size, a.size)
    part = np.ones(nt, np.int32)
    part[:NWALL] = 0
    rest = torch.from_numpy(np.ascontiguousarray(np.stack([tr0["v0"], tr0["v1"], tr0["v2"]], axis=1), np.float32)).cuda()
    out = {"triangles": int(nt), "image": [a.size, a.size], "spp": a.spp, "steps": a.steps}
    rows = {w: [] for w in WAYS}
    same, torch_ms = [], []
    with hpt.Scene(L, sp, tr0) as scene:
        render_ms(scene, cam, a)
        scene.set_parts(part, 2)
        for k in range(1, a.steps + 1):
            rec = turn_record(5.0 * k)
            tr = hpt.pose_host(tr0, part, rec)
            if k > 1:
                scene.update_triangles(tr0)                          # back to the rest pose: not timed
            images = []
            # 1. the pose
            wall, _ = ms(lambda: scene.pose(rec))
            info = scene.update_info()
            r_ms, img = render_ms(scene, cam, a)
            rows["pose"].append(dict(wall=wall, pack=info["ms_pack"], upload=info["ms_upload"], refit=info["ms_refit"], render=r_ms))
            images.append(img)
            # 2. vertices a torch kernel turned
            drec = torch.from_numpy(rec[1]).cuda()
            torch.cuda.synchronize()
            t_torch, v = ms(lambda: (torch_turn(torch, rest, drec), torch.cuda.synchronize())[0])
            torch_ms.append(t_torch)
            wall, _ = ms(lambda: scene.update_vertices_device(v))
            info = scene.update_info()
            r_ms, img = render_ms(scene, cam, a)
            rows["device_verts"].append(dict(wall=wall, pack=info["ms_pack"], upload=info["ms_upload"], refit=info["ms_refit"], render=r_ms))
            images.append(img)
            # 3. the yardstick
            wall, _ = ms(lambda: scene.update_triangles(tr))
            info = scene.update_info()
            r_ms, img = render_ms(scene, cam, a)
            rows["update_triangles"].append(dict(wall=wall, pack=info["ms_pack"], upload=info["ms_upload"], refit=info["ms_refit"], render=r_ms))
            images.append(img)
            same.append(bool(np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])))
    keys = ("wall", "pack", "upload", "refit", "render")
    out["ways"] = {w: {"first_call": rows[w][0], "later_calls": {key: med_range([s[key] for s in rows[w][1:]]) for key in keys}} for w in WAYS}
    yard = out["ways"]["update_triangles"]["later_calls"]["wall"]["median"]
    out["wall_ratio_to_update_triangles"] = {w: out["ways"][w]["later_calls"]["wall"]["median"] / yard for w in WAYS[:2]}
    out["torch_ms"] = med_range(torch_ms[1:])
    out["same_image_every_step"] = all(same)
    return out


def cli_frames(a):
    """Seconds per frame of pt_cli --spin and --spin-device: (a run of `long` frames - a run of `short` frames) / the difference."""
    cli = os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_cli")
    n = max(int(round((a.cli_tris / 2.0) ** 0.5)), 3)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "mesh.obj")
        rows = sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, n, n)
        sio.write_obj(obj, sio._tris_from(rows, np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (len(rows), 1))))
        out["triangles"] = len(rows)
        scene_file = os.path.join(ROOT, "tests", "golden", "scenes", "input.txt")
        base = [cli, "--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", "13", "--width", "256", "--height", "256", "--frame-spp", "2",
                "--guide-spp", "2", "--reproject", "--output", os.path.join(tmp, "out.png")]
        short, long_ = 2, 2 + a.cli_frames
        for flag in ("--spin", "--spin-device"):
            t = {}
            for frames in (short, long_):
                run = subprocess.run(base + ["--frames", str(frames), flag, "5"], capture_output=True, text=True)
                if run.returncode != 0:
                    raise SystemExit("pt_cli failed: " + run.stdout[-2000:] + run.stderr[-2000:])
                m = re.search(r"\[Render\] Finished in (\d+) ms", run.stdout)
                t[frames] = float(m.group(1))
            out[flag.lstrip("-")] = {"ms_per_frame": (t[long_] - t[short]) / (long_ - short), "ms_short_run": t[short], "ms_long_run": t[long_]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tris", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-tris", type=int, default=1000000)
    ap.add_argument("--cli-frames", type=int, default=8)
    a = ap.parse_args()
    if hpt.device_count() < 1:
        raise SystemExit("bench_pose.py: no HIP device visible")
    import torch
    torch.cuda.set_device(0)
    res = {"bench": "poses: hpt_scene_pose and device vertices against hpt_scene_update_triangles", "scenes": [one_scene(n, a, torch) for n in a.tris]}
    if a.cli:
        res["cli"] = cli_frames(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
