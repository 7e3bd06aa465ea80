"""TEST INFRASTRUCTURE ONLY -- ctypes front-end of the guide-buffer oracle (tests/guides_oracle.cpp), which includes
ppm_oracle.cpp: the library also exports ppm_oracle_render.  Built into a directory the caller gives."""
import ctypes as C
import os
import subprocess

import numpy as np

import ppm_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_p = ppm_oracle._p


def build(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libguides_oracle.so")
    subprocess.check_call(["g++"] + ppm_oracle.CXXFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "guides_oracle.cpp")])
    lib = C.CDLL(so)
    lib.guides_oracle_render.restype = C.c_int
    lib.ppm_oracle_render.restype = C.c_int
    return lib


def render(lib, lights, spheres, tris, camera, W, H, spp=4, seed=1, sample_offset=0, max_delta=0):
    """Returns (dict(albedo, normal, position [H, W, 3], coverage [H, W]), hit points per sample [spp])."""
    lights = np.ascontiguousarray(lights); spheres = np.ascontiguousarray(spheres); tris = np.ascontiguousarray(tris)
    cam = np.ascontiguousarray(camera).reshape(1)
    g = dict(albedo=np.zeros((H, W, 3), np.float32), normal=np.zeros((H, W, 3), np.float32),
             position=np.zeros((H, W, 3), np.float32), coverage=np.zeros((H, W), np.float32))
    hp = np.zeros(spp, np.uint64)
    rc = lib.guides_oracle_render(_p(lights), len(lights), _p(spheres), len(spheres), _p(tris), len(tris), _p(cam), W, H, spp,
                                  C.c_uint64(seed), sample_offset, max_delta, _p(g["albedo"]), _p(g["normal"]), _p(g["position"]),
                                  _p(g["coverage"]), _p(hp))
    assert rc == 0
    return g, [int(v) for v in hp]
