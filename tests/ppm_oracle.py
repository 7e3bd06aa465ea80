"""TEST INFRASTRUCTURE ONLY -- ctypes front-end of the PPM oracle (tests/ppm_oracle.cpp).

The shared library is compiled with the flags of oracle/Makefile into a directory the caller gives (pytest's
tmp dir), so nothing new lands in the tree."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function"]


def build(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libppm_oracle.so")
    subprocess.check_call(["g++"] + CXXFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "ppm_oracle.cpp")])
    lib = C.CDLL(so)
    lib.ppm_oracle_render.restype = C.c_int
    return lib


def scene_bounds(spheres, tris):
    """The reference helper's bounds (src/ppm_cu_helper.cpp:21-52): spheres +- r, triangle vertices, from +-1e9."""
    mn = np.full(3, 1e9, np.float32)
    mx = np.full(3, -1e9, np.float32)
    for s in spheres:
        c = np.asarray(s["center"], np.float32); r = np.float32(s["r"])
        mx = np.maximum(mx, c + r); mn = np.minimum(mn, c - r)
    for t in tris:
        for v in ("v0", "v1", "v2"):
            p = np.asarray(t[v], np.float32)
            mx = np.maximum(mx, p); mn = np.minimum(mn, p)
    return mn, mx


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


WORK = ("candidates", "accepted", "cand_median", "cand_max", "acc_median", "acc_max")


def render(lib, lights, spheres, tris, camera, W, H, eye_depth=4, light_depth=4, spp=1, spl=8, radius=0.05, seed=1,
           sample_offset=0, max_delta=64, output_sum=False, scene_min=None, scene_max=None, brute=False, want_flux=False,
           want_work=False, want_pos=False):
    """Returns (image [H, W, 3] f32, stats dict[, flux [H, W, 3] of the last pass][, hit point positions [H, W, 3] of
    the last pass, NaN where a pixel has none]).  want_work: stats also hold the WORK counts of hpt_ppm_stats
    (candidates and accepted over all passes; medians and maxima per hit point of the last pass)."""
    lights = np.ascontiguousarray(lights); spheres = np.ascontiguousarray(spheres); tris = np.ascontiguousarray(tris)
    cam = np.ascontiguousarray(camera).reshape(1)
    if scene_min is None or scene_max is None:
        mn, mx = scene_bounds(spheres, tris)
        scene_min = mn if scene_min is None else scene_min
        scene_max = mx if scene_max is None else scene_max
    mn = np.ascontiguousarray(scene_min, np.float32); mx = np.ascontiguousarray(scene_max, np.float32)
    img = np.zeros((H, W, 3), np.float32)
    st = np.zeros(5, np.uint64)
    flux = np.zeros((H, W, 3), np.float32) if want_flux else None
    work = np.zeros(len(WORK), np.uint64) if want_work else None
    pos = np.zeros((H, W, 3), np.float32) if want_pos else None
    rc = lib.ppm_oracle_render(_p(lights), len(lights), _p(spheres), len(spheres), _p(tris), len(tris), _p(cam), W, H,
                               eye_depth, light_depth, spp, spl, C.c_float(radius), _p(mn), _p(mx), C.c_uint64(seed),
                               sample_offset, max_delta, int(output_sum), int(brute), _p(img), _p(st),
                               _p(flux) if flux is not None else None, _p(work) if work is not None else None,
                               _p(pos) if pos is not None else None)
    assert rc == 0
    stats = dict(zip(("photons", "photon_rays", "deposits", "hit_points", "direct_pixels"), (int(v) for v in st)))
    if want_work:
        stats.update(zip(WORK, (int(v) for v in work)))
    out = (img, stats) + ((flux,) if want_flux else ()) + ((pos,) if want_pos else ())
    return out
