"""TEST INFRASTRUCTURE ONLY -- ctypes front-end of the motion-guide oracle (tests/motion_oracle.cpp), which includes
ppm_oracle.cpp like the guides oracle.  Built into a directory the caller gives."""
import ctypes as C
import os
import subprocess

import numpy as np

import ppm_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_p = ppm_oracle._p
KEYS = ("albedo", "normal", "position", "coverage", "prev_position")


def build(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libmotion_oracle.so")
    subprocess.check_call(["g++"] + ppm_oracle.CXXFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "motion_oracle.cpp")])
    lib = C.CDLL(so)
    lib.motion_oracle_render.restype = C.c_int
    return lib


def render(lib, lights, spheres, tris, prev_spheres, prev_tris, camera, W, H, spp=4, seed=1, sample_offset=0, max_delta=0):
    """The five guide images of the current records seen against the previous ones: (dict(albedo, normal, position,
    prev_position [H, W, 3], coverage [H, W]), hit points per sample [spp])."""
    lights = np.ascontiguousarray(lights); spheres = np.ascontiguousarray(spheres); tris = np.ascontiguousarray(tris)
    prev_spheres = np.ascontiguousarray(prev_spheres); prev_tris = np.ascontiguousarray(prev_tris)
    assert len(prev_spheres) == len(spheres) and len(prev_tris) == len(tris)
    cam = np.ascontiguousarray(camera).reshape(1)
    g = {k: np.zeros((H, W) if k == "coverage" else (H, W, 3), np.float32) for k in KEYS}
    hp = np.zeros(spp, np.uint64)
    rc = lib.motion_oracle_render(_p(lights), len(lights), _p(spheres), len(spheres), _p(tris), len(tris), _p(prev_spheres),
                                  _p(prev_tris), _p(cam), W, H, spp, C.c_uint64(seed), sample_offset, max_delta, _p(g["albedo"]),
                                  _p(g["normal"]), _p(g["position"]), _p(g["coverage"]), _p(g["prev_position"]), _p(hp))
    assert rc == 0
    return g, [int(v) for v in hp]
