"""Timing of the guide buffers and the denoiser on one GPU: input.txt at 1024 x 1024, 4 guide samples per pixel, 5 filter
levels with demodulation (the defaults).

One JSON line on stdout.  Guides: device ms of hpt_render_guides (HIP events of the library, first kernel to last untile)
and host wall ms of the blocking call with its four downloads.  Denoiser: ms of set_guides (the guide pack), of the colour
pack, of all levels and of each level (HIP events; the per-level and colour-pack times are the library's own events
under DENOISE_TIME).  Each level moves 64 algorithmic bytes per pixel (16 colour + 32 guides read, 16 written); beside
each level stands the time of a device-to-device copy with that traffic (a 32 B x W x H buffer: 32 read + 32 written)
and of one that copies a 64 B x W x H buffer, measured in the same run, and the ratio level / copy.  Every figure is the
median of --repeat runs after --warmup runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import path_tracing_amd as hpt
from path_tracing_amd import scene_io as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8, help="samples of the path-traced frame that is filtered")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise: no GPU visible")
    torch.cuda.set_device(0)
    sc = S.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr = S.flatten_for_pt(sc)
    W = H = a.size
    cam = S.camera_for(sc, W, H)
    med = lambda v: float(np.median(v))

    guides_dev, guides_wall = [], []
    with hpt.Scene(L, sp, tr) as s:
        frame = s.render_pt(cam, W, H, 4, a.spp, hpt.make_params(seed=a.seed))
        for it in range(a.warmup + a.repeat):
            t0 = time.perf_counter()
            g = s.render_guides(cam, W, H, a.guide_spp, hpt.make_params(seed=a.seed))
            wall = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                guides_wall.append(wall); guides_dev.append(s.ppm_stats()["ms_total"])

    dg = [torch.from_numpy(g[k]).cuda() for k in ("albedo", "normal", "position", "coverage")]
    din = torch.from_numpy(frame).cuda()
    dout = torch.empty_like(din)
    copies = {}
    for name, per_px in (("copy_64B_traffic", 32), ("copy_64B_buffer", 64)):
        src = torch.zeros(per_px * W * H, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    params = hpt.make_denoise_params(iterations=a.iterations, time=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    pack, color, filt, levels, copy_ms = [], [], [], [], {k: [] for k in copies}
    with hpt.Denoiser(W, H) as d:
        for it in range(a.warmup + a.repeat):
            e0, e1 = ev(), ev()
            e0.record(); d.set_guides(*dg, stream=stream); e1.record()
            d.run(din, dout, params, stream=stream)
            ms = d.last_ms()
            ce = {}
            for k, (src, dst) in copies.items():
                c0, c1 = ev(), ev()
                c0.record(); dst.copy_(src, non_blocking=True); c1.record()
                ce[k] = (c0, c1)
            torch.cuda.synchronize()
            if it >= a.warmup:
                pack.append(e0.elapsed_time(e1)); color.append(ms["pack"]); filt.append(ms["filter"])
                levels.append(ms["levels"][: a.iterations])
                for k, (c0, c1) in ce.items():
                    copy_ms[k].append(c0.elapsed_time(c1))
    denoised = dout.cpu().numpy()
    lv = [med([r[k] for r in levels]) for k in range(a.iterations)]
    cp = {k: med(v) for k, v in copy_ms.items()}
    out = {
        "workload": "input.txt %dx%d, %d guide spp, %d levels, demodulated, PT %d spp frame" % (W, H, a.guide_spp, a.iterations, a.spp),
        "ms_guides_device": med(guides_dev), "ms_guides_call": med(guides_wall),
        "ms_pack_guides": med(pack), "ms_pack_color": med(color), "ms_filter": med(filt), "ms_per_level": lv,
        "bytes_per_level": 64 * W * H,
        "ms_copy_64B_traffic": cp["copy_64B_traffic"], "ms_copy_64B_buffer": cp["copy_64B_buffer"],
        "level_over_copy_64B_traffic": [v / cp["copy_64B_traffic"] for v in lv],
        "level_over_copy_64B_buffer": [v / cp["copy_64B_buffer"] for v in lv],
        "level_GBps": [64 * W * H / (v * 1e6) for v in lv],
        "coverage_mean": float(g["coverage"].mean()), "finite": bool(np.isfinite(denoised).all()),
        "warmup": a.warmup, "repeat": a.repeat,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
