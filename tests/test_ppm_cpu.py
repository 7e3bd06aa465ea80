"""CPU tests of the photon-mapping path: the reference-named symbol, the CLI's help, and self-checks of the PPM
oracle (tests/ppm_oracle.cpp) that the GPU tests compare against."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import ppm_oracle

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return ppm_oracle.build(tmp_path_factory.mktemp("ppm_oracle"))


@pytest.fixture(scope="module")
def small_input(sio):
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", "input.txt"))
    L, sp, tr = sio.flatten_for_pt(sc)
    return L, sp, tr, sio.camera_for(sc, 24, 20)


def test_reference_named_ppm_wrapper_symbol(tmp_path):
    """libhpt_ref.so defines ppm_render_wrapper under the name a caller compiled against the reference's declaration
    (include/ppm_cu.cuh:8-15) asks for; the name is derived here from a probe translation unit."""
    so = os.path.join(CSRC, "libhpt_ref.so")
    probe = tmp_path / "probe.cpp"
    probe.write_text(
        "struct float3 { float x, y, z; };\n"
        "struct CudaLight; struct CudaSphere; struct CudaTriangle;\n"
        "struct CudaCamera { float3 eye, U, V, W, UL, dx, dy; };\n"
        "void ppm_render_wrapper(const CudaLight *, int, const CudaSphere *, int, const CudaTriangle *, int,\n"
        "                        float3, float3, const CudaCamera, float3 *, int, int, int, int, int, int);\n"
        "void call(const CudaLight *l, const CudaSphere *s, const CudaTriangle *t, CudaCamera c, float3 *img){\n"
        "    float3 z = {0, 0, 0}; ppm_render_wrapper(l, 1, s, 1, t, 1, z, z, c, img, 8, 8, 4, 8, 4, 1); }\n")
    obj = tmp_path / "probe.o"
    subprocess.check_call(["g++", "-c", "-o", str(obj), str(probe)])
    undefined = subprocess.check_output(["nm", "-u", str(obj)], text=True)
    wanted = [ln.split()[-1] for ln in undefined.splitlines() if "ppm_render_wrapper" in ln]
    assert len(wanted) == 1
    defined = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert wanted[0] in defined.split()


def test_cli_help_lists_ppm():
    out = subprocess.run([os.path.join(CSRC, "pt_cli"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "pt, bdpt, ppm" in out.stdout and "--radius" in out.stdout


def test_oracle_is_deterministic_and_passes_sum(plib, small_input):
    L, sp, tr, cam = small_input
    a, sa = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spp=2, spl=64, seed=5, output_sum=True)
    b, sb = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spp=2, spl=64, seed=5, output_sum=True)
    assert a.tobytes() == b.tobytes() and sa == sb
    assert sa["deposits"] > 0 and sa["hit_points"] > 0 and a.max() > 0
    p0, s0 = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spp=1, spl=64, seed=5, sample_offset=0)
    p1, s1 = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spp=1, spl=64, seed=5, sample_offset=1)
    assert np.array_equal(a, p0 + p1)
    assert sa["deposits"] == s0["deposits"] + s1["deposits"]
    mean, _ = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spp=2, spl=64, seed=5)
    assert np.array_equal(mean, a / np.float32(2))


def test_oracle_without_photons_is_the_direct_term(plib, small_input):
    L, sp, tr, cam = small_input
    d, st = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spl=0, seed=3, want_flux=False)
    full, _, flux = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spl=64, seed=3, want_flux=True)
    assert st["deposits"] == 0 and st["photons"] == 0
    assert st["direct_pixels"] > 0
    hp = flux.any(axis=2)                 # pixels whose hit point received flux
    assert hp.any()
    assert not d[hp].any()                # without photons those pixels are black
    assert np.array_equal(d[~hp], full[~hp])


def test_oracle_tiny_radius_reaches_no_deposit(plib, small_input):
    L, sp, tr, cam = small_input
    d, _ = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spl=0, seed=3)
    tiny, st = ppm_oracle.render(plib, L, sp, tr, cam, 24, 20, spl=64, seed=3, radius=1e-7)
    assert st["deposits"] > 0
    assert np.array_equal(tiny, d)


def test_oracle_grid_gather_equals_brute_force_double_loop(plib):
    """Two triangles (a diffuse floor, a glossy wall) under a spot light: the sorted grid's gather and the scan over every
    deposit for each of the 27 cells give the same accumulated flux, bit for bit, and examine the same pairs."""
    from path_tracing_amd.layouts import LIGHT, SPHERE, TRIANGLE
    tr = np.zeros(2, TRIANGLE)
    tr[0]["v0"], tr[0]["v1"], tr[0]["v2"] = (-1, 0, -1), (1, 0, -1), (0, 0, 1)
    tr[0]["mtl"]["base_color"] = (0.8, 0.7, 0.6); tr[0]["mtl"]["roughness"] = 1.0
    tr[1]["v0"], tr[1]["v1"], tr[1]["v2"] = (-1, 0, -1), (1, 0, -1), (0, 1.5, -1)
    tr[1]["mtl"]["base_color"] = (0.5, 0.6, 0.9); tr[1]["mtl"]["roughness"] = 0.3; tr[1]["mtl"]["metallic"] = 0.5
    L = np.zeros(1, LIGHT)
    L[0]["pos"] = (0, 1, 0.3); L[0]["dir"] = (0, -1, -0.2); L[0]["illum"] = (3, 3, 3)
    L[0]["light_ball"]["center"] = (0, 1, 0.3); L[0]["light_ball"]["r"] = 0.05; L[0]["cutoff"] = 1.2
    sp = np.zeros(0, SPHERE)
    from path_tracing_amd.layouts import CAMERA
    cam = np.zeros((), CAMERA)
    cam["eye"] = (0, 0.6, 2.0); cam["UL"] = (-0.5, 1.0, 1.0); cam["dx"] = (1 / 16, 0, 0); cam["dy"] = (0, -1 / 16, 0)
    img_a, st_a, fa = ppm_oracle.render(plib, L, sp, tr, cam, 16, 16, spl=2000, radius=0.2, seed=2, want_flux=True, want_work=True)
    img_b, st_b, fb = ppm_oracle.render(plib, L, sp, tr, cam, 16, 16, spl=2000, radius=0.2, seed=2, want_flux=True, brute=True,
                                        want_work=True)
    assert st_a["deposits"] > 100 and st_a["hit_points"] > 0
    assert fa.any()
    assert fa.tobytes() == fb.tobytes() and img_a.tobytes() == img_b.tobytes()
    assert st_a == st_b and st_a["accepted"] > 0 and st_a["cand_max"] >= st_a["cand_median"] > 0
