"""CPU tests of the guide-buffer oracle (tests/guides_oracle.cpp) that the GPU tests compare hpt_render_guides with:
ranges of the four images on input.txt and the hit-point counts against the PPM oracle's eye pass."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import guides_oracle
import ppm_oracle

W, H, SPP = 32, 24, 3


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


@pytest.fixture(scope="module")
def scene(sio):
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", "input.txt"))
    L, sp, tr = sio.flatten_for_pt(sc)
    return L, sp, tr, sio.camera_for(sc, W, H)


@pytest.fixture(scope="module")
def guides(glib, scene):
    return guides_oracle.render(glib, *scene, W, H, spp=SPP, seed=5, sample_offset=2)


def test_ranges(guides, scene):
    g, _ = guides
    cov = g["coverage"]
    assert (cov >= 0).all() and (cov <= SPP).all() and (cov == np.round(cov)).all()
    assert (cov > 0).any() and (cov == SPP).any()
    empty = cov == 0
    assert (g["albedo"][empty] == 0).all() and (g["normal"][empty] == 0).all() and (g["position"][empty] == 0).all()
    assert (g["albedo"][~empty].max(axis=-1) > 0).all()          # albedo is zero exactly where coverage is zero
    assert (np.linalg.norm(g["normal"].astype(np.float64), axis=-1) <= 1 + 1e-6).all()
    mn, mx = ppm_oracle.scene_bounds(scene[1], scene[2])
    pos = g["position"][~empty]
    assert (pos >= mn - 1e-4).all() and (pos <= mx + 1e-4).all()


def test_hit_points_per_sample_are_the_ppm_eye_pass(glib, guides, scene):
    _, hp = guides
    for s in range(SPP):
        _, st = ppm_oracle.render(glib, *scene, W, H, 4, 4, 1, 0, 0.05, seed=5, sample_offset=2 + s)
        assert hp[s] == st["hit_points"] and hp[s] > 0
    assert sum(hp) == int(guides[0]["coverage"].sum())


def test_one_sample_is_the_hit_point_itself(glib, scene):
    g, _ = guides_oracle.render(glib, *scene, W, H, spp=1, seed=5, sample_offset=2)
    _, _, pos = ppm_oracle.render(glib, *scene, W, H, 4, 4, 1, 0, 0.05, seed=5, sample_offset=2, want_pos=True)
    hit = ~np.isnan(pos[..., 0])
    assert (hit == (g["coverage"] == 1)).all()
    assert g["position"][hit].tobytes() == pos[hit].tobytes()
    n = np.linalg.norm(g["normal"][hit].astype(np.float64), axis=-1)
    assert np.abs(n - 1).max() < 1e-5
