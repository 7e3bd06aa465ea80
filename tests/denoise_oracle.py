"""TEST INFRASTRUCTURE ONLY -- ctypes front-end of the denoiser oracle (tests/denoise_oracle.cpp).

Built like ppm_oracle into a directory the caller gives (pytest's tmp dir)."""
import ctypes as C
import os
import subprocess

import numpy as np

import ppm_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_p = ppm_oracle._p


def build(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libdenoise_oracle.so")
    subprocess.check_call(["g++"] + ppm_oracle.CXXFLAGS + ["-shared", "-o", so, os.path.join(_HERE, "denoise_oracle.cpp")])
    lib = C.CDLL(so)
    lib.denoise_oracle_run.restype = C.c_int
    return lib


def run(lib, colour, guides, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=True, want_levels=False):
    """Returns the filtered image [H, W, 3] f32 (and, want_levels, c_0 .. c_n as [n + 1, H, W, 3])."""
    colour = np.ascontiguousarray(colour, np.float32)
    H, W = colour.shape[:2]
    g = [np.ascontiguousarray(guides[k], np.float32) for k in ("albedo", "normal", "position", "coverage")]
    assert g[0].shape == g[1].shape == g[2].shape == (H, W, 3) and g[3].shape == (H, W)
    out = np.zeros((H, W, 3), np.float32)
    n = iterations if iterations else 5
    levels = np.zeros((n + 1, H, W, 3), np.float32) if want_levels else None
    rc = lib.denoise_oracle_run(_p(colour), _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), _p(out), W, H, int(iterations), C.c_float(sigma_color),
                                C.c_float(sigma_normal), C.c_float(sigma_position), 1 if demodulate else 0,
                                _p(levels) if levels is not None else None)
    assert rc == 0
    return (out, levels) if want_levels else out


def random_guides(rng, W, H, invalid=None):
    """Valid guides with structure: unit normals from a few directions in blocks, positions on a bumpy sheet, albedo in
    (0.05, 1), coverage 1..4; `invalid` (bool [H, W]) pixels get coverage 0 and zero guides, as hpt_render_guides leaves them."""
    dirs = rng.normal(size=(4, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)
    pick = rng.integers(0, 4, size=((H + 7) // 8, (W + 7) // 8))
    normal = dirs[np.kron(pick, np.ones((8, 8), np.int64))[:H, :W]].astype(np.float32)
    normal = (normal + rng.normal(scale=0.02, size=(H, W, 3))).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    position = np.stack([xx * np.float32(0.01), yy * np.float32(0.01), rng.normal(scale=0.01, size=(H, W)).astype(np.float32)], -1).astype(np.float32)
    albedo = rng.uniform(0.05, 1.0, size=(H, W, 3)).astype(np.float32)
    coverage = rng.integers(1, 5, size=(H, W)).astype(np.float32)
    if invalid is not None:
        coverage[invalid] = 0; albedo[invalid] = 0; normal[invalid] = 0; position[invalid] = 0
    return dict(albedo=albedo, normal=np.ascontiguousarray(normal), position=position, coverage=coverage)
