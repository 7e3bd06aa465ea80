"""Timing of the variance-guided filter on one GPU at 1024 x 1024 (include/hpt.h, "variance-guided filtering"), guides and
frames from tests/golden/scenes/input.txt: two cameras --degrees apart, the second frame advanced into a history that holds
--history frames of the first, so converged and restarted pixels sit side by side.

One JSON line on stdout, every figure the median of --repeat runs after --warmup runs, HIP events:
  ms_guided_levels / ms_plain_levels   hpt_denoiser_run_guided and hpt_denoiser_run at the same level count on the same
                       denoiser, alternating, each level's own time (HPT_DENOISE_TIME), with the pack and the total of the
                       levels.  guided_over_plain is the ratio of the totals; a guided level loads 34 records per lane where
                       a plain one loads 25 (loads_ratio = 1.36).
  ms_estimate          hpt_denoiser_estimate_variance with a length image.  Algorithmic traffic per pixel: the frame and the
                       two guide records the 49 taps share, read once (12 + 32 B), the length read (4 B), the variance
                       written (12 B) = 60 B.  Beside it a device-to-device copy that moves the same number of bytes (a
                       buffer of half the traffic: read once, written once) and the ratio.
  ms_length            hpt_history_length: one 16-byte record read and 4 bytes written per pixel = 20 B, copy and ratio.
  ms_frame / ms_extra  a moved --reproject frame as pt_cli enqueues it (hpt_render_pt_device at --spp, hpt_untile,
                       hpt_history_advance with guides, hpt_display_present) and what --guided adds to it
                       (hpt_history_length, estimate, guided run), each between two events on the one stream."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--degrees", type=float, default=2.0)
    ap.add_argument("--history", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided: no GPU visible")
    torch.cuda.set_device(0)
    from history_cases import orbit_eye
    W = H = a.size
    npx = W * H
    n = a.iterations
    med = lambda v: float(np.median(v))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sc = scene_io.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr = scene_io.flatten_for_pt(sc)
    cams = [scene_io.make_camera(orbit_eye(sc.eye, sc.look_at, sc.view_up, d), sc.look_at, sc.view_up, 50.0, W, H) for d in (0.0, a.degrees)]
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device="cuda")
    guides = [dict(albedo=f3(), normal=f3(), position=f3(), coverage=f1()) for _ in cams]
    hist_guides = lambda k: {key: guides[k][key] for key in ("normal", "position", "coverage")}
    frame, mean, var, out, out_plain = f3(), f3(), f3(), f3(), f3()
    length, vout = f1(), f1()
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    copies = {}
    for name, per_pixel in (("estimate", 30), ("length", 10)):
        src = torch.zeros(per_pixel * npx, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    p0 = hpt.make_params()
    local = torch.zeros((hpt.local_pixels(W, H, p0), 3), dtype=torch.float32, device="cuda")
    gp = hpt.make_guided_params(iterations=n, time=True)
    dp = hpt.make_denoise_params(iterations=n, time=True)
    gp_loop = hpt.make_guided_params(iterations=n)
    t = {k: [] for k in ("estimate", "length", "copy_estimate", "copy_length", "frame", "extra", "guided_pack", "plain_pack")}
    lv = {"guided": [], "plain": []}
    with hpt.Scene(L, sp, tr) as scene, hpt.History(W, H) as hist, hpt.Denoiser(W, H) as den, hpt.Display(W, H) as disp:

        def render(k, offset):
            scene.render_pt_device(cams[k], W, H, 4, a.spp, hpt.make_params(seed=5, sample_offset=offset), local.data_ptr(), stream)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, p0, stream)

        torch.cuda.synchronize()
        for k, cam in enumerate(cams):
            scene.render_guides_device(cam, W, H, a.guide_spp, hpt.make_params(seed=5), **guides[k])
        kept = []
        for it in range(a.warmup + a.repeat):
            # a history of the first camera, then the moved frame
            hist.reset(stream=stream)
            for f in range(a.history):
                render(0, (it * (a.history + 1) + f) * a.spp)
                hist.advance(cams[0], frame, mean_out=mean, stream=stream, **(hist_guides(0) if f == 0 else {}))
            den.set_guides(stream=stream, **guides[1])
            e = [ev() for _ in range(3)]
            e[0].record()
            render(1, (it * (a.history + 1) + a.history) * a.spp)
            hist.advance(cams[1], frame, mean_out=mean, stream=stream, **hist_guides(1))
            disp.present(mean, out=rgb8, stream=stream)
            e[1].record()
            hist.length(length, stream=stream)
            den.estimate_variance(frame, var, length, gp_loop, stream=stream)
            den.run_guided(mean, var, out, None, gp_loop, stream=stream)
            e[2].record()
            kept.append(hist.metrics()["kept"] / float(npx))
            # the stages on their own, each beside its copy
            s = [ev() for _ in range(6)]
            s[0].record(); den.estimate_variance(frame, var, length, gp_loop, stream=stream); s[1].record()
            src, dst = copies["estimate"]
            dst.copy_(src, non_blocking=True); s[2].record()
            s[3].record(); hist.length(length, stream=stream); s[4].record()
            src, dst = copies["length"]
            dst.copy_(src, non_blocking=True); s[5].record()
            # the two filters, alternating, timed per level by the library's own events
            den.run_guided(mean, var, out, vout, gp, stream=stream)
            ms_g = den.last_ms()
            den.run(mean, out_plain, dp, stream=stream)
            ms_p = den.last_ms()
            torch.cuda.synchronize()
            if it >= a.warmup:
                t["frame"].append(e[0].elapsed_time(e[1])); t["extra"].append(e[1].elapsed_time(e[2]))
                t["estimate"].append(s[0].elapsed_time(s[1])); t["copy_estimate"].append(s[1].elapsed_time(s[2]))
                t["length"].append(s[3].elapsed_time(s[4])); t["copy_length"].append(s[4].elapsed_time(s[5]))
                t["guided_pack"].append(ms_g["pack"]); t["plain_pack"].append(ms_p["pack"])
                lv["guided"].append(ms_g["levels"][:n]); lv["plain"].append(ms_p["levels"][:n])
    levels = {k: [med([r[j] for r in v]) for j in range(n)] for k, v in lv.items()}
    totals = {k: med([sum(r) for r in v]) for k, v in lv.items()}
    out = {"workload": "%dx%d, input.txt, cameras %g degrees apart, %d frames of history, %d spp" % (W, H, a.degrees, a.history, a.spp),
           "pixels": npx, "iterations": n, "kept_share": med(kept[a.warmup:]),
           "ms_guided_levels": levels["guided"], "ms_plain_levels": levels["plain"],
           "ms_guided_total": totals["guided"], "ms_plain_total": totals["plain"], "guided_over_plain": totals["guided"] / totals["plain"],
           "level_ratios": [g / p for g, p in zip(levels["guided"], levels["plain"])], "loads_ratio": 34.0 / 25.0,
           "ms_guided_pack": med(t["guided_pack"]), "ms_plain_pack": med(t["plain_pack"]),
           "ms_estimate": med(t["estimate"]), "bytes_estimate": 60 * npx, "ms_copy_estimate": med(t["copy_estimate"]),
           "ms_length": med(t["length"]), "bytes_length": 20 * npx, "ms_copy_length": med(t["copy_length"]),
           "ms_frame": med(t["frame"]), "ms_extra": med(t["extra"])}
    for k in ("estimate", "length"):
        out["%s_over_copy" % k] = out["ms_" + k] / out["ms_copy_" + k]
        out["%s_GBps" % k] = out["bytes_" + k] / (out["ms_" + k] * 1e6)
    out["extra_over_frame"] = out["ms_extra"] / out["ms_frame"]
    out["warmup"], out["repeat"] = a.warmup, a.repeat
    print(json.dumps(out))


if __name__ == "__main__":
    main()
