"""Timing of the progressive display on one GPU at 1024 x 1024 (include/hpt.h, "progressive display").

One JSON line on stdout, every device figure the median of --repeat runs after --warmup runs, timed with HIP events:
  ms_add, ms_add_moments   hpt_accum_add with mean-out, without and with HPT_ACCUM_MOMENTS.  Algorithmic traffic per value:
                           frame and sum read, sum and mean written = 16 B (24 B with the squares read and written).
  ms_present               hpt_display_present with `other`, flipped BGR into the middle panel of a three-panel
                           framebuffer (pitch 9 W).  Per value: 4 B read, `last` and other's `last` read, `last` and the
                           panel byte written = 8 B.
  ms_copy_*                beside each, a device-to-device copy that moves the same number of bytes (a buffer of half the
                           traffic: read once, written once), measured in the same run, and the ratio step / copy.
  ms_frame_device          the whole per-frame step of the reference's three panels: three adds and three presents.
  ms_host_*                the host path it replaces, on the same box (src/main.cpp:421-531): three downloads, the numpy
                           running average, hpt_tonemap_reference (the reference's clamp / powf / truncate loop) and the
                           numpy sums of squared byte differences; wall time, median of --host-repeat runs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import path_tracing_amd as hpt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--host-repeat", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_display: no GPU visible")
    torch.cuda.set_device(0)
    W = H = a.size
    n = W * H * 3
    med = lambda v: float(np.median(v))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rng = np.random.default_rng(1)
    host_frames = [(rng.uniform(0.0, 1.1, size=(H, W, 3)) ** 2).astype(np.float32) for _ in range(3)]
    frames = [torch.from_numpy(f).cuda() for f in host_frames]
    means = [torch.empty_like(f) for f in frames]
    fb = torch.zeros(H * 9 * W, dtype=torch.uint8, device="cuda")
    copies = {}
    for name, per_value in (("add", 8), ("add_moments", 12), ("present", 4)):
        src = torch.zeros(per_value * n, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))
    stream = torch.cuda.current_stream().cuda_stream
    t = {k: [] for k in ("add", "add_moments", "present", "frame", "copy_add", "copy_add_moments", "copy_present")}

    acc = [hpt.Accumulator(W, H) for _ in range(3)]
    mom = hpt.Accumulator(W, H, moments=True)
    disp = [hpt.Display(W, H) for _ in range(3)]
    panel = lambda p, other=None: disp[p].present(means[p], out=fb, other=other, pitch=9 * W, x_offset=3 * W * p, bgr=True,
                                                  flip_y=True, stream=stream)
    for it in range(a.warmup + a.repeat):
        e = [ev() for _ in range(8)]
        e[0].record(); acc[0].add(frames[0], mean_out=means[0], stream=stream); e[1].record()
        mom.add(frames[1], mean_out=means[1], stream=stream); e[2].record()
        panel(0)
        e[3].record(); panel(1, disp[0]); e[4].record()
        # the three panels' whole step
        e[5].record()
        for p in range(3):
            acc[p].add(frames[p], mean_out=means[p], stream=stream)
        panel(0); panel(1, disp[0]); panel(2)
        e[6].record()
        ce = {}
        for k, (src, dst) in copies.items():
            c0, c1 = ev(), ev()
            c0.record(); dst.copy_(src, non_blocking=True); c1.record()
            ce[k] = (c0, c1)
        torch.cuda.synchronize()
        if it >= a.warmup:
            t["add"].append(e[0].elapsed_time(e[1])); t["add_moments"].append(e[1].elapsed_time(e[2]))
            t["present"].append(e[3].elapsed_time(e[4])); t["frame"].append(e[5].elapsed_time(e[6]))
            for k, (c0, c1) in ce.items():
                t["copy_" + k].append(c0.elapsed_time(c1))
    for o in acc + [mom] + disp:
        o.close()

    # the host path: what src/main.cpp:421-531 does per frame for its three panels
    lib = hpt.load_library()
    lib.hpt_tonemap_reference.restype = None
    bufs = [np.zeros((H, W, 3), np.float32) for _ in range(3)]
    last = [np.zeros((H, W, 3), np.uint8) for _ in range(3)]
    h = {k: [] for k in ("download", "accumulate", "tonemap", "rms", "total")}
    ssd = lambda x, y: int(((x.astype(np.int32) - y.astype(np.int32)) ** 2).sum(dtype=np.int64))
    for it in range(a.host_repeat):
        count = np.float32(it + 1)
        t0 = time.perf_counter()
        got = [f.cpu().numpy() for f in frames]
        t1 = time.perf_counter()
        avg = []
        for p in range(3):
            bufs[p] += got[p]
            avg.append(bufs[p] / count)
        t2 = time.perf_counter()
        cur = []
        for p in range(3):
            b = np.empty((H, W, 3), np.uint8)
            lib.hpt_tonemap_reference(avg[p].ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_int64(W * H), 0)
            cur.append(b)
        t3 = time.perf_counter()
        sums = [ssd(cur[p], last[p]) for p in range(3)] + [ssd(cur[0], cur[1])]      # three histories and the DIFF RMS
        last = cur
        t4 = time.perf_counter()
        for k, v in zip(("download", "accumulate", "tonemap", "rms", "total"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            h[k].append(v * 1e3)

    out = {"workload": "%dx%d, 3 panels" % (W, H), "values": n,
           "ms_add": med(t["add"]), "bytes_add": 16 * n, "ms_copy_add": med(t["copy_add"]),
           "ms_add_moments": med(t["add_moments"]), "bytes_add_moments": 24 * n, "ms_copy_add_moments": med(t["copy_add_moments"]),
           "ms_present": med(t["present"]), "bytes_present": 8 * n, "ms_copy_present": med(t["copy_present"]),
           "ms_frame_device": med(t["frame"])}
    for k in ("add", "add_moments", "present"):
        out["%s_over_copy" % k] = out["ms_" + k] / out["ms_copy_" + k]
        out["%s_GBps" % k] = out["bytes_" + k] / (out["ms_" + k] * 1e6)
    for k, v in h.items():
        out["ms_host_" + k] = med(v)
    out["host_over_device"] = out["ms_host_total"] / out["ms_frame_device"]
    out["warmup"], out["repeat"], out["host_repeat"] = a.warmup, a.repeat, a.host_repeat
    print(json.dumps(out))


if __name__ == "__main__":
    main()
