"""TEST INFRASTRUCTURE ONLY -- ctypes front-end of the progressive photon-mapping oracle (tests/sppm_oracle.cpp).

Built like ppm_oracle into a directory the caller gives (pytest's tmp dir).  State mirrors hpt_sppm: the caller
keeps a State and advances it with render()."""
import ctypes as C
import os
import subprocess

import numpy as np

import ppm_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))


def build(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libsppm_oracle.so")
    subprocess.check_call(["g++"] + ppm_oracle.CXXFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "sppm_oracle.cpp")])
    lib = C.CDLL(so)
    lib.sppm_oracle_render.restype = C.c_int
    lib.ppm_oracle_render.restype = C.c_int
    return lib


_p = ppm_oracle._p
STATS = ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels", "candidates", "accepted")


class State:
    """One progressive state: scene, camera and estimator parameters fixed, per-pixel R2 / N / tau / D."""

    def __init__(self, lib, lights, spheres, tris, camera, W, H, eye_depth=4, light_depth=4, spl=8, radius=0.05, alpha=0.7,
                 seed=1, sample_offset=0, max_delta=64, scene_min=None, scene_max=None, cull=True):
        self.lib = lib
        self.lights = np.ascontiguousarray(lights); self.spheres = np.ascontiguousarray(spheres); self.tris = np.ascontiguousarray(tris)
        self.cam = np.ascontiguousarray(camera).reshape(1)
        if scene_min is None or scene_max is None:
            mn, mx = ppm_oracle.scene_bounds(self.spheres, self.tris)
            scene_min = mn if scene_min is None else scene_min
            scene_max = mx if scene_max is None else scene_max
        self.mn = np.ascontiguousarray(scene_min, np.float32); self.mx = np.ascontiguousarray(scene_max, np.float32)
        self.W, self.H, self.eye_depth, self.light_depth, self.spl = W, H, eye_depth, light_depth, spl
        self.radius = np.float32(radius if radius > 0 else 0.05)
        self.alpha, self.seed, self.sample_offset, self.max_delta, self.cull = alpha, seed, sample_offset, max_delta, cull
        self.reset()

    def reset(self):
        self.r2 = np.full((self.H, self.W), self.radius * self.radius, np.float32)
        self.n = np.zeros((self.H, self.W), np.float32)
        self.tau = np.zeros((self.H, self.W, 3), np.float32)
        self.d = np.zeros((self.H, self.W, 3), np.float32)
        self.k = np.zeros(1, np.int64)

    def render(self, passes=1):
        """Advances by `passes` passes; returns (image [H, W, 3], stats dict of this call)."""
        img = np.zeros((self.H, self.W, 3), np.float32)
        st = np.zeros(7, np.uint64)
        rc = self.lib.sppm_oracle_render(_p(self.lights), len(self.lights), _p(self.spheres), len(self.spheres), _p(self.tris),
                                         len(self.tris), _p(self.cam), self.W, self.H, self.eye_depth, self.light_depth, self.spl,
                                         C.c_float(self.radius), C.c_float(self.alpha), _p(self.mn), _p(self.mx), C.c_uint64(self.seed),
                                         self.sample_offset, self.max_delta, passes, int(self.cull), _p(self.r2), _p(self.n),
                                         _p(self.tau), _p(self.d), _p(self.k), _p(img), _p(st))
        assert rc == 0
        return img, dict(zip(STATS, (int(v) for v in st)))

    @property
    def passes(self):
        return int(self.k[0])
