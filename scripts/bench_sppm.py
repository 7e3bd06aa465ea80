"""Timing of progressive photon mapping on one GPU: scripts/bench_ppm.py's workload (input.txt, 1024 x 1024, one
million photons per light and pass) rendered into ONE state with alpha = 0.7, one pass per call.

One JSON line on stdout: ms per pass (first, median, last; HIP events) and gather ms per pass (TIME_KERNELS),
candidate and accepted pairs per pass from a separate COUNT_WORK run of the same passes, and the mean R2 / radius^2
over the image at the end."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import path_tracing_amd as hpt
from path_tracing_amd import scene_io as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spl", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--alpha", type=float, default=0.7)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sc = S.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr = S.flatten_for_pt(sc)
    W = H = a.size
    cam = S.camera_for(sc, W, H)
    timed, counted = [], []
    with hpt.Scene(L, sp, tr) as s:
        s.render_ppm(cam, W, H, 4, 4, 1, a.spl, a.radius, hpt.make_params(seed=a.seed))          # warm-up
        p = hpt.make_params(seed=a.seed)
        with s.sppm(cam, W, H, 4, 4, a.spl, a.radius, a.alpha, p) as z:
            for _ in range(a.passes):
                z.render(1, hpt.FLAG_TIME_KERNELS)
                timed.append(s.ppm_stats())
            r2 = z.state()["radius2"]
        with s.sppm(cam, W, H, 4, 4, a.spl, a.radius, a.alpha, p) as z:
            for _ in range(a.passes):
                z.render(1, hpt.FLAG_COUNT_WORK)
                counted.append(s.ppm_stats())
    ms = [t["ms_total"] for t in timed]
    gather = [t["ms_gather"] for t in timed]
    r0 = np.float32(a.radius) * np.float32(a.radius)
    out = {
        "workload": "input.txt %dx%d, %d lights x %d photons per pass, alpha %g, %d passes on one state" % (W, H, len(L), a.spl, a.alpha, a.passes),
        "ms_per_pass_first": ms[0], "ms_per_pass_median": float(np.median(ms)), "ms_per_pass_last": ms[-1],
        "ms_gather_first": gather[0], "ms_gather_median": float(np.median(gather)), "ms_gather_last": gather[-1],
        "ms_per_pass": ms, "ms_gather": gather,
        "candidates_per_pass": [c["candidates"] for c in counted], "accepted_per_pass": [c["accepted"] for c in counted],
        "hit_points": timed[-1]["hit_points"], "live_deposits": timed[-1]["deposits"],
        "mean_r2_over_radius2_end": float(np.mean(r2.astype(np.float64)) / float(r0)),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
