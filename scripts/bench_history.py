"""Timing of the temporal history on one GPU at 1024 x 1024 (include/hpt.h, "history across camera moves"), guides and
frames from tests/golden/scenes/input.txt.

One JSON line on stdout, every figure the median of --repeat runs after --warmup runs:
  ms_advance_moved     hpt_history_advance with guides from a camera that differs from the previous advance's (two cameras
                       2 degrees apart, alternating), HIP events.  Algorithmic traffic per pixel: frame, normal, position
                       and coverage read (40 B), the previous set's three records read once (48 B; the four taps of
                       neighbouring pixels share them), the new set and the mean written (60 B) = 148 B.
  ms_advance_still     the same camera again, no guides: frame and the mean record read (28 B), the record and the mean
                       written (28 B) = 56 B.
  ms_copy_*            beside each, a device-to-device copy that moves the same number of bytes (a buffer of half the
                       traffic: read once, written once), measured in the same run, and the ratio advance / copy.
  kept_share           of the moved advances.
  ms_guides            hpt_render_guides_device at --guide-spp (blocking call, host clock).
  ms_render            the --spp path-traced frame it accompanies: hpt_render_pt_device + hpt_untile, host clock around
                       the enqueue and a synchronise.
  moved_frame_over_render   (ms_guides + ms_advance_moved) / ms_render: what a moved frame costs on top of its render."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--degrees", type=float, default=2.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_history: no GPU visible")
    torch.cuda.set_device(0)
    from history_cases import orbit_eye
    W = H = a.size
    npx = W * H
    med = lambda v: float(np.median(v))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sc = scene_io.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr = scene_io.flatten_for_pt(sc)
    cams = [scene_io.make_camera(orbit_eye(sc.eye, sc.look_at, sc.view_up, d), sc.look_at, sc.view_up, 50.0, W, H) for d in (0.0, a.degrees)]
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    guides = [dict(normal=f3(), position=f3(), coverage=torch.zeros((H, W), dtype=torch.float32, device="cuda")) for _ in cams]
    frames = [f3() for _ in cams]
    mean = f3()
    copies = {}
    for name, per_pixel in (("moved", 74), ("still", 28)):
        src = torch.zeros(per_pixel * npx, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    p0 = hpt.make_params()
    local = torch.zeros((hpt.local_pixels(W, H, p0), 3), dtype=torch.float32, device="cuda")
    t = {k: [] for k in ("moved", "still", "copy_moved", "copy_still", "guides", "render")}
    kept = []
    with hpt.Scene(L, sp, tr) as scene, hpt.History(W, H) as hist:
        torch.cuda.synchronize()
        for k, cam in enumerate(cams):
            scene.render_guides_device(cam, W, H, a.guide_spp, hpt.make_params(seed=5), **guides[k])
            scene.render_pt_device(cam, W, H, 4, a.spp, hpt.make_params(seed=5), local.data_ptr(), stream)
            hpt.untile(local.data_ptr(), frames[k].data_ptr(), W, H, p0, stream)
            torch.cuda.synchronize()
        hist.advance(cams[0], frames[0], mean_out=mean, stream=stream, **guides[0])
        for it in range(a.warmup + a.repeat):
            k = (it + 1) % 2
            e = [ev() for _ in range(3)]
            e[0].record(); hist.advance(cams[k], frames[k], mean_out=mean, stream=stream, **guides[k]); e[1].record()
            share = hist.metrics()["kept"] / float(npx)
            hist.advance(cams[k], frames[k], mean_out=mean, stream=stream); e[2].record()
            ce = {}
            for name, (src, dst) in copies.items():
                c0, c1 = ev(), ev()
                c0.record(); dst.copy_(src, non_blocking=True); c1.record()
                ce[name] = (c0, c1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scene.render_guides_device(cams[k], W, H, a.guide_spp, hpt.make_params(seed=5, sample_offset=it), **guides[k])
            t1 = time.perf_counter()
            scene.render_pt_device(cams[k], W, H, 4, a.spp, hpt.make_params(seed=5, sample_offset=it * a.spp), local.data_ptr(), stream)
            hpt.untile(local.data_ptr(), frames[k].data_ptr(), W, H, p0, stream)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= a.warmup:
                t["moved"].append(e[0].elapsed_time(e[1])); t["still"].append(e[1].elapsed_time(e[2]))
                for name, (c0, c1) in ce.items():
                    t["copy_" + name].append(c0.elapsed_time(c1))
                t["guides"].append((t1 - t0) * 1e3); t["render"].append((t2 - t1) * 1e3)
                kept.append(share)
    out = {"workload": "%dx%d, input.txt, cameras %g degrees apart" % (W, H, a.degrees), "pixels": npx,
           "ms_advance_moved": med(t["moved"]), "bytes_advance_moved": 148 * npx, "ms_copy_moved": med(t["copy_moved"]),
           "ms_advance_still": med(t["still"]), "bytes_advance_still": 56 * npx, "ms_copy_still": med(t["copy_still"]),
           "kept_share": med(kept), "ms_guides": med(t["guides"]), "guide_spp": a.guide_spp, "ms_render": med(t["render"]), "spp": a.spp}
    for k in ("moved", "still"):
        out["%s_over_copy" % k] = out["ms_advance_" + k] / out["ms_copy_" + k]
        out["%s_GBps" % k] = out["bytes_advance_" + k] / (out["ms_advance_" + k] * 1e6)
    out["moved_frame_over_render"] = (out["ms_guides"] + out["ms_advance_moved"]) / out["ms_render"]
    out["warmup"], out["repeat"] = a.warmup, a.repeat
    print(json.dumps(out))


if __name__ == "__main__":
    main()
