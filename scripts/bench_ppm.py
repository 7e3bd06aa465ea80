"""Timing of the photon-mapping path on one GPU: the reference GUI's own workload (input.txt, 1024 x 1024,
move_data_to_cuda_ppm(..., 1000000): one million photons per light, one pass per frame, src/main.cpp:262,406).

One JSON line on stdout: ms per pass split into eye / photon / grid / gather (HIP events, median of `--reps` timed
passes after a warm-up), photon rays per second, live deposits, candidate and accepted (hit point, deposit) pairs per
hit point (median and maximum, from a separate COUNT_WORK pass), and a roofline note for the gather: the bytes it
reads per candidate against HBM and the pairs it evaluates per second."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import path_tracing_amd as hpt
from path_tracing_amd import scene_io as S

HBM_GBPS = 8000.0            # MI355X HBM3E peak (datasheet)
BYTES_PER_CANDIDATE = 48     # position | cell x, normal | cell y, direction | cell z (three 16-B loads)
BYTES_PER_ACCEPTED = 16      # + the flux record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spl", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sc = S.load_scene(os.path.join(ROOT, "tests", "golden", "scenes", "input.txt"))
    L, sp, tr = S.flatten_for_pt(sc)
    W = H = a.size
    cam = S.camera_for(sc, W, H)
    runs = []
    with hpt.Scene(L, sp, tr) as s:
        s.render_ppm(cam, W, H, 4, 4, 1, a.spl, params=hpt.make_params(seed=a.seed, flags=hpt.FLAG_TIME_KERNELS))   # warm-up
        for k in range(a.reps):
            s.render_ppm(cam, W, H, 4, 4, 1, a.spl, params=hpt.make_params(seed=a.seed + 1 + k, flags=hpt.FLAG_TIME_KERNELS))
            runs.append(s.ppm_stats())
        s.render_ppm(cam, W, H, 4, 4, 1, a.spl, params=hpt.make_params(seed=a.seed, flags=hpt.FLAG_COUNT_WORK))
        cnt = s.ppm_stats()
    med = lambda key: float(np.median([r[key] for r in runs]))
    gather_ms = med("ms_gather")
    gbps = (cnt["candidates"] * BYTES_PER_CANDIDATE + cnt["accepted"] * BYTES_PER_ACCEPTED) / (gather_ms * 1e-3) / 1e9
    out = {
        "workload": "input.txt %dx%d, %d lights x %d photons, one pass" % (W, H, len(L), a.spl),
        "ms_per_pass": med("ms_total"), "ms_eye": med("ms_eye"), "ms_photon": med("ms_photon"),
        "ms_grid": med("ms_grid"), "ms_gather": gather_ms,
        "photons": runs[-1]["photons"], "photon_rays": runs[-1]["photon_rays"],
        "photon_rays_per_s": runs[-1]["photon_rays"] / (med("ms_photon") * 1e-3),
        "live_deposits": runs[-1]["deposits"], "hit_points": runs[-1]["hit_points"], "grid_buckets": runs[-1]["grid_buckets"],
        "candidates": cnt["candidates"], "accepted": cnt["accepted"],
        "candidates_per_hit_point_median": cnt["cand_median"], "candidates_per_hit_point_max": cnt["cand_max"],
        "accepted_per_hit_point_median": cnt["acc_median"], "accepted_per_hit_point_max": cnt["acc_max"],
        "gather_pairs_per_s": cnt["candidates"] / (gather_ms * 1e-3),
        "gather_candidate_GBps": gbps,
        "gather_roofline": ("candidate bytes at %.0f GB/s = %.0f %% of HBM peak: %s" %
                            (gbps, 100.0 * gbps / HBM_GBPS,
                             "bound by bytes" if gbps > 0.5 * HBM_GBPS else
                             "not bound by HBM bytes (cell lists are shared by neighbouring hit points and served from cache); "
                             "the per-lane list walk and BSDF VALU with uneven list lengths per wave set the time")),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
