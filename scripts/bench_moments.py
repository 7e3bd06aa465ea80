"""Timing of the temporal variance on one GPU at 1024 x 1024 (include/hpt.h, "temporal variance"), guides and frames from
tests/golden/scenes/input.txt: a history with HPT_HISTORY_MOMENTS beside a plain one, alternating in one process (the order
swaps every iteration).  The two histories, the denoiser and the images together exceed the 256 MiB Infinity Cache, so two
untimed moved advances first bring a history's own records back into it -- the condition scripts/bench_history.py measures
a single history under; the windows of the advances, the chain and the variance call start on an idle device, as there.

One JSON line on stdout, every figure the median of --repeat runs after --warmup runs, HIP events around each call:
  ms_advance_moved / _moments     hpt_history_advance with guides from a camera that differs from the previous advance's (two
                                  cameras --degrees apart).  Algorithmic traffic per pixel: the plain advance's 148 B
                                  (scripts/bench_history.py) plus the second-moment record read once and written once:
                                  148 + 16 + 16 = 180 B.
  ms_advance_still / _moments     the same camera again, no guides: 56 B, and 56 + 32 = 88 B with moments.
  ms_variance                     hpt_history_variance in place: the mean and moment records and the fallback read, the
                                  output written: 16 + 16 + 12 + 12 = 56 B.
  ms_copy_*                       beside each, a device-to-device copy that moves the same number of bytes (a buffer of half
                                  the traffic: read once, written once), in the same iteration, and the ratio step / copy.
  ms_chain / ms_chain_moments     a moved --reproject --guided frame behind its render: advance with guides, length,
                                  estimate, guided run (5 levels); with moments also hpt_history_variance in place before the
                                  guided run.  temporal_variance_adds_ms is the difference of the two medians."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import path_tracing_amd as hpt
from path_tracing_amd import scene_io

BYTES = {"moved": 148, "moved_moments": 148 + 16 + 16, "still": 56, "still_moments": 56 + 32, "variance": 16 + 16 + 12 + 12}


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
        raise SystemExit("bench_moments: no GPU visible")
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
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device="cuda")
    guides = [dict(normal=f3(), position=f3(), coverage=f1()) for _ in cams]
    albedo = f3()
    frames = [f3() for _ in cams]
    mean, var, out, length = f3(), f3(), f3(), f1()
    copies = {}
    for name, per_pixel in BYTES.items():
        src = torch.zeros(per_pixel // 2 * npx, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    p0 = hpt.make_params()
    local = torch.zeros((hpt.local_pixels(W, H, p0), 3), dtype=torch.float32, device="cuda")
    t = {k: [] for k in list(BYTES) + ["copy_" + k for k in BYTES] + ["chain", "chain_moments"]}
    kept, temporal_share = [], []
    with hpt.Scene(L, sp, tr) as scene, hpt.History(W, H) as plain, hpt.History(W, H, moments=True) as moments, hpt.Denoiser(W, H) as den:
        torch.cuda.synchronize()
        for k, cam in enumerate(cams):
            scene.render_guides_device(cam, W, H, a.guide_spp, hpt.make_params(seed=5), albedo=albedo if k == 0 else None, **guides[k])
            scene.render_pt_device(cam, W, H, 4, a.spp, hpt.make_params(seed=5), local.data_ptr(), stream)
            hpt.untile(local.data_ptr(), frames[k].data_ptr(), W, H, p0, stream)
            torch.cuda.synchronize()
        den.set_guides(albedo, guides[0]["normal"], guides[0]["position"], guides[0]["coverage"], stream=stream)     # the chain's camera
        for h in (plain, moments):
            h.advance(cams[0], frames[0], mean_out=mean, stream=stream, **guides[0])
        for it in range(a.warmup + a.repeat):
            order = [("", plain), ("_moments", moments)]
            if it % 2:
                order.reverse()
            rec = {}
            for suffix, h in order:
                e = [ev() for _ in range(5)]
                for k in (1, 0):                     # untimed: this history's records back into the cache behind the other one's work
                    h.advance(cams[k], frames[k], mean_out=mean, stream=stream, **guides[k])
                torch.cuda.synchronize()             # the window starts on an idle device, as in bench_history.py
                e[0].record(); h.advance(cams[1], frames[1], mean_out=mean, stream=stream, **guides[1]); e[1].record()
                share = h.metrics()["kept"] / float(npx)
                h.advance(cams[1], frames[1], mean_out=mean, stream=stream); e[2].record()
                rec["moved" + suffix], rec["still" + suffix] = (e[0], e[1]), (e[1], e[2])
                # the chain of a moved --reproject --guided frame, back at the first camera
                torch.cuda.synchronize()
                e[3].record()
                h.advance(cams[0], frames[0], mean_out=mean, stream=stream, **guides[0])
                h.length(length, stream=stream)
                den.estimate_variance(frames[0], var, length, stream=stream)
                if suffix:
                    h.variance(var, fallback=var, stream=stream)
                den.run_guided(mean, var, out, stream=stream)
                e[4].record()
                rec["chain" + suffix] = (e[3], e[4])
                if suffix:
                    v0, v1 = ev(), ev()
                    torch.cuda.synchronize()
                    v0.record(); h.variance(var, fallback=var, stream=stream); v1.record()
                    rec["variance"] = (v0, v1)
                    kept.append(share)
            copies["moved"][1].copy_(copies["moved"][0], non_blocking=True)        # untimed: the timed copies run on a busy device
            for name, (src, dst) in copies.items():
                c0, c1 = ev(), ev()
                c0.record(); dst.copy_(src, non_blocking=True); c1.record()
                rec["copy_" + name] = (c0, c1)
            torch.cuda.synchronize()
            if it >= a.warmup:
                for name, (e0, e1) in rec.items():
                    t[name].append(e0.elapsed_time(e1))
                temporal_share.append(float((moments.read()["length"] >= 4).mean()))
    out_json = {"workload": "%dx%d, input.txt, cameras %g degrees apart" % (W, H, a.degrees), "pixels": npx, "kept_share": med(kept),
                "temporal_share": med(temporal_share)}
    for name, per_pixel in BYTES.items():
        key = "ms_variance" if name == "variance" else "ms_advance_" + name
        out_json[key] = med(t[name])
        out_json["bytes_" + name] = per_pixel * npx
        out_json["ms_copy_" + name] = med(t["copy_" + name])
        out_json[name + "_over_copy"] = out_json[key] / out_json["ms_copy_" + name]
        out_json[name + "_GBps"] = per_pixel * npx / (out_json[key] * 1e6)
    out_json["ms_chain"], out_json["ms_chain_moments"] = med(t["chain"]), med(t["chain_moments"])
    out_json["temporal_variance_adds_ms"] = out_json["ms_chain_moments"] - out_json["ms_chain"]
    out_json["warmup"], out_json["repeat"] = a.warmup, a.repeat
    print(json.dumps(out_json))


if __name__ == "__main__":
    main()
