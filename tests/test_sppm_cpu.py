"""CPU tests of progressive photon mapping: the exported entry points, the CLI's help, and self-checks of the SPPM
oracle (tests/sppm_oracle.cpp) that the GPU tests compare against."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import ppm_oracle
import sppm_oracle

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")


@pytest.fixture(scope="module")
def slib(tmp_path_factory):
    return sppm_oracle.build(tmp_path_factory.mktemp("sppm_oracle"))


@pytest.fixture(scope="module")
def small_input(sio):
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", "input.txt"))
    L, sp, tr = sio.flatten_for_pt(sc)
    return L, sp, tr, sio.camera_for(sc, 24, 20), 24, 20


@pytest.fixture(scope="module")
def cornell(sio):
    from conftest import scene_by_name
    (L, sp, tr), (eye, look, up) = scene_by_name(sio, "cornell_sphere_2k")
    return L, sp, tr, sio.make_camera(eye, look, up, 50.0, 20, 20), 20, 20


def spot_scene():
    """test_ppm_cpu's two triangles (a diffuse floor, a glossy wall) under a spot light."""
    from path_tracing_amd.layouts import CAMERA, LIGHT, SPHERE, TRIANGLE
    tr = np.zeros(2, TRIANGLE)
    tr[0]["v0"], tr[0]["v1"], tr[0]["v2"] = (-1, 0, -1), (1, 0, -1), (0, 0, 1)
    tr[0]["mtl"]["base_color"] = (0.8, 0.7, 0.6); tr[0]["mtl"]["roughness"] = 1.0
    tr[1]["v0"], tr[1]["v1"], tr[1]["v2"] = (-1, 0, -1), (1, 0, -1), (0, 1.5, -1)
    tr[1]["mtl"]["base_color"] = (0.5, 0.6, 0.9); tr[1]["mtl"]["roughness"] = 0.3; tr[1]["mtl"]["metallic"] = 0.5
    L = np.zeros(1, LIGHT)
    L[0]["pos"] = (0, 1, 0.3); L[0]["dir"] = (0, -1, -0.2); L[0]["illum"] = (3, 3, 3)
    L[0]["light_ball"]["center"] = (0, 1, 0.3); L[0]["light_ball"]["r"] = 0.05; L[0]["cutoff"] = 1.2
    cam = np.zeros((), CAMERA)
    cam["eye"] = (0, 0.6, 2.0); cam["UL"] = (-0.5, 1.0, 1.0); cam["dx"] = (1 / 16, 0, 0); cam["dy"] = (0, -1 / 16, 0)
    return L, np.zeros(0, SPHERE), tr, cam, 16, 16


def test_library_exports_the_sppm_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(CSRC, "libhpt.so")], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ("hpt_sppm_create", "hpt_sppm_render", "hpt_sppm_reset", "hpt_sppm_read_state", "hpt_sppm_destroy"):
        assert n in names, n
    host = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(CSRC, "libhpt_host.so")], text=True)
    assert any("run_cuda_sppm" in ln for ln in host.splitlines())


def test_cli_help_lists_sppm_and_alpha():
    out = subprocess.run([os.path.join(CSRC, "pt_cli"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "pt, bdpt, ppm" in out.stdout and "sppm" in out.stdout and "--alpha" in out.stdout


def test_one_pass_alpha_one_is_a_ppm_pass(slib, small_input, cornell):
    for L, sp, tr, cam, W, H in (small_input, cornell):
        for off in (0, 3):
            ref, rst = ppm_oracle.render(slib, L, sp, tr, cam, W, H, spl=64, seed=5, sample_offset=off)
            s = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=64, alpha=1.0, seed=5, sample_offset=off)
            img, st = s.render(1)
            assert rst["hit_points"] > 0
            for k in ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels"):
                assert st[k] == rst[k], k
            assert img.tobytes() == ref.tobytes()


@pytest.mark.parametrize("case", ["input", "cornell_sphere_2k", "spot", "tiny_radius"])
def test_cull_changes_no_bit_and_visits_fewer_pairs(slib, small_input, cornell, case):
    if case == "input":
        L, sp, tr, cam, W, H = small_input; spl, radius = 256, 0.05
    elif case == "cornell_sphere_2k":
        L, sp, tr, cam, W, H = cornell; spl, radius = 256, 0.05
    elif case == "spot":
        L, sp, tr, cam, W, H = spot_scene(); spl, radius = 1000, 0.2
    else:
        L, sp, tr, cam, W, H = small_input; spl, radius = 256, 1e-3
    a = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=spl, radius=radius, alpha=0.5, seed=9, cull=True)
    b = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=spl, radius=radius, alpha=0.5, seed=9, cull=False)
    cand_a = cand_b = 0
    for it in range(4):
        ia, sa = a.render(1)
        ib, sb = b.render(1)
        assert ia.tobytes() == ib.tobytes(), it
        assert a.r2.tobytes() == b.r2.tobytes() and a.n.tobytes() == b.n.tobytes(), it
        assert sa["accepted"] == sb["accepted"]
        assert sa["candidates"] <= sb["candidates"]
        cand_a += sa["candidates"]; cand_b += sb["candidates"]
    assert cand_a <= cand_b
    if case != "tiny_radius":                  # (a 1e-3 radius: almost no pair is ever examined)
        assert sb["accepted"] > 0
        assert (a.n > 0).any()                 # some radii shrank ...
        assert sa["candidates"] < sb["candidates"]   # ... and the last pass examined strictly fewer pairs


def test_passes_split_across_calls_give_the_same_bytes(slib, small_input):
    L, sp, tr, cam, W, H = small_input
    a = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=64, alpha=0.7, seed=3)
    a.render(3)
    ia, _ = a.render(2)
    b = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=64, alpha=0.7, seed=3)
    ib, _ = b.render(5)
    assert a.passes == b.passes == 5
    assert ia.tobytes() == ib.tobytes()
    assert a.r2.tobytes() == b.r2.tobytes() and a.n.tobytes() == b.n.tobytes() and a.tau.tobytes() == b.tau.tobytes()


def test_radius_never_grows_and_shrinks_where_photons_land(slib, small_input):
    L, sp, tr, cam, W, H = small_input
    r0 = np.float32(0.05) * np.float32(0.05)
    s = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=128, alpha=0.6, seed=7)
    prev_r2, prev_n = s.r2.copy(), s.n.copy()
    for _ in range(4):
        s.render(1)
        assert (s.r2 <= prev_r2).all()
        got = s.n > prev_n                     # pixels whose hit point had M > 0 this pass
        assert got.any()
        assert (s.r2[got] < prev_r2[got]).all()
        assert (s.r2[~got] == prev_r2[~got]).all()
        prev_r2, prev_n = s.r2.copy(), s.n.copy()
    assert (s.r2 < r0).any()
    one = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=128, alpha=1.0, seed=7)
    one.render(4)
    assert (one.r2 == r0).all() and (one.n > 0).any()
