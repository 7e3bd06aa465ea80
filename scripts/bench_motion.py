"""What following moving geometry costs, and what it keeps (include/hpt.h, "motion"): one GPU, 1024 x 1024, the scene of
tests/golden/scenes/input.txt plus the tessellated sphere of cornell_with_sphere(100000) (99 012 triangles) turned 5
degrees per frame about its centre under a still camera.

One JSON line on stdout, every time the median of --repeat frames after --warmup frames, all measured in this process:
  ms_guides_motion / ms_guides     hpt_render_guides_motion_device (five images) against hpt_render_guides_device (four) at
                                   --guide-spp on the same scene in the same pose (blocking calls, host clock); the two
                                   take turns at going first, frame by frame
  ms_advance_motion                hpt_history_advance_motion, HIP events.  Algorithmic traffic per pixel: the plain moved
                                   advance's 148 B plus the motion guide's 12 B = 160 B
  ms_advance_moved                 hpt_history_advance from a moved camera (two cameras 2 degrees apart, alternating, on the
                                   unturned scene), 148 B per pixel
  ms_copy_*, *_over_copy           beside each, a device-to-device copy that moves the same number of bytes
  ms_keep_previous, ms_copy_keep   hpt_scene_keep_previous (host clock, blocking) against a device copy of its 36 bytes per
                                   triangle
  ms_update                        hpt_scene_update_triangles (host clock), for scale
  kept_share_motion                kept / pixels of every measured frame's advance with the motion guide
  kept_share_reset                 the same frames on a second history that is reset after every update, which is what a
                                   history without the motion guide has to do: 0 by construction, measured all the same"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import path_tracing_amd as hpt
from path_tracing_amd import scene_io

NWALL = 12
CENTRE = np.array((-0.15, 0.2, 0.45))


def turned(tr, first, degrees):
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    out = tr.copy()
    for k in ("v0", "v1", "v2"):
        v = out[k].astype(np.float64)
        v[first:] = (v[first:] - CENTRE) @ R.T + CENTRE
        out[k] = v.astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=12)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--degrees", type=float, default=5.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion: no GPU visible")
    torch.cuda.set_device(0)
    from history_cases import orbit_eye
    W = H = a.size
    npx = W * H
    med = lambda v: float(np.median(v))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sc = scene_io.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr_in = scene_io.flatten_for_pt(sc)
    ball = scene_io.cornell_with_sphere(100000)[2][NWALL:]
    tr0 = np.concatenate([tr_in, ball])
    tr0["id"] = np.arange(len(tr0))
    first = len(tr_in)
    cams = [scene_io.make_camera(orbit_eye(sc.eye, sc.look_at, sc.view_up, d), sc.look_at, sc.view_up, 50.0, W, H) for d in (0.0, 2.0)]
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device="cuda")
    g5 = dict(albedo=f3(), normal=f3(), position=f3(), coverage=f1(), prev_position=f3())
    g4 = dict(albedo=f3(), normal=f3(), position=f3(), coverage=f1())
    cam_guides = [dict(normal=f3(), position=f3(), coverage=f1()) for _ in cams]
    frame, mean = f3(), f3()
    copies = {}
    for name, nbytes in (("motion", 80 * npx), ("moved", 74 * npx), ("keep", 36 * len(tr0))):
        src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    p0 = hpt.make_params()
    local = torch.zeros((hpt.local_pixels(W, H, p0), 3), dtype=torch.float32, device="cuda")
    t = {k: [] for k in ("guides_motion", "guides", "advance_motion", "advance_moved", "copy_motion", "copy_moved", "copy_keep", "keep_previous", "update")}
    kept_motion, kept_reset = [], []
    with hpt.Scene(L, sp, tr0) as scene, hpt.History(W, H) as hist, hpt.History(W, H) as plain, hpt.History(W, H) as reset:
        torch.cuda.synchronize()
        # the plain advance from a moved camera, on the unturned scene
        for k, cam in enumerate(cams):
            scene.render_guides_device(cam, W, H, a.guide_spp, hpt.make_params(seed=5), **cam_guides[k])
        scene.render_pt_device(cams[0], W, H, 4, a.spp, hpt.make_params(seed=5), local.data_ptr(), stream)
        hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, p0, stream)
        plain.advance(cams[0], frame, mean_out=mean, stream=stream, **cam_guides[0])
        for it in range(a.warmup + a.repeat):
            k = (it + 1) % 2
            e0, e1 = ev(), ev()
            e0.record(); plain.advance(cams[k], frame, mean_out=mean, stream=stream, **cam_guides[k]); e1.record()
            c0, c1 = ev(), ev()
            c0.record(); copies["moved"][1].copy_(copies["moved"][0], non_blocking=True); c1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                t["advance_moved"].append(e0.elapsed_time(e1)); t["copy_moved"].append(c0.elapsed_time(c1))
        # the turning sphere under a still camera
        cam = cams[0]
        for it in range(a.warmup + a.repeat + 1):
            p = hpt.make_params(seed=5, sample_offset=it * a.spp)
            if it:
                tr = turned(tr0, first, a.degrees * it)
                t0 = time.perf_counter(); scene.update_triangles(tr); t_update = (time.perf_counter() - t0) * 1e3
            first_call, second_call = (g4, g5) if it % 2 else (g5, g4)         # the two calls take turns at going first
            t0 = time.perf_counter(); scene.render_guides_device(cam, W, H, a.guide_spp, p, **first_call); t1 = time.perf_counter()
            scene.render_guides_device(cam, W, H, a.guide_spp, p, **second_call); t2 = time.perf_counter()
            ms_g4, ms_g5 = ((t1 - t0) * 1e3, (t2 - t1) * 1e3) if it % 2 else ((t2 - t1) * 1e3, (t1 - t0) * 1e3)
            scene.render_pt_device(cam, W, H, 4, a.spp, p, local.data_ptr(), stream)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, p0, stream)
            e0, e1, c0, c1, k0, k1 = (ev() for _ in range(6))
            e0.record()
            hist.advance(cam, frame, g5["normal"], g5["position"], g5["coverage"], mean_out=mean, stream=stream, prev_position=g5["prev_position"])
            e1.record()
            c0.record(); copies["motion"][1].copy_(copies["motion"][0], non_blocking=True); c1.record()
            k0.record(); copies["keep"][1].copy_(copies["keep"][0], non_blocking=True); k1.record()
            if it:
                reset.reset(stream=stream)
            reset.advance(cam, frame, g5["normal"], g5["position"], g5["coverage"], mean_out=mean, stream=stream)
            torch.cuda.synchronize()
            t3 = time.perf_counter(); scene.keep_previous(); t4 = time.perf_counter()
            if it > a.warmup:
                t["update"].append(t_update); t["guides"].append(ms_g4); t["guides_motion"].append(ms_g5)
                t["advance_motion"].append(e0.elapsed_time(e1)); t["copy_motion"].append(c0.elapsed_time(c1))
                t["copy_keep"].append(k0.elapsed_time(k1)); t["keep_previous"].append((t4 - t3) * 1e3)
                kept_motion.append(hist.metrics()["kept"] / float(npx)); kept_reset.append(reset.metrics()["kept"] / float(npx))
    out = {"workload": "%dx%d, input.txt + %d-triangle sphere turned %g degrees per frame" % (W, H, len(ball), a.degrees), "pixels": npx,
           "triangles": int(len(tr0)), "guide_spp": a.guide_spp}
    for k, v in t.items():
        out["ms_" + k] = med(v)
    out["guides_motion_over_guides"] = out["ms_guides_motion"] / out["ms_guides"]
    out["bytes_advance_motion"], out["bytes_advance_moved"] = 160 * npx, 148 * npx
    out["motion_over_copy"] = out["ms_advance_motion"] / out["ms_copy_motion"]
    out["moved_over_copy"] = out["ms_advance_moved"] / out["ms_copy_moved"]
    out["motion_over_moved"] = out["ms_advance_motion"] / out["ms_advance_moved"]
    out["keep_over_copy"] = out["ms_keep_previous"] / out["ms_copy_keep"]
    out["kept_share_motion"] = [round(v, 4) for v in kept_motion]
    out["kept_share_reset"] = [round(v, 4) for v in kept_reset]
    out["warmup"], out["repeat"] = a.warmup, a.repeat
    print(json.dumps(out))


if __name__ == "__main__":
    main()
