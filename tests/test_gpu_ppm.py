"""Photon mapping on the MI355X: Scene.render_ppm against the PPM oracle (tests/ppm_oracle.cpp) bit for bit, run to
run reproducibility, the reference-named wrapper, the CLI, argument errors, and PT renders untouched by it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import ppm_oracle

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return ppm_oracle.build(tmp_path_factory.mktemp("ppm_oracle"))


def _parallel(L):
    L = L.copy()
    L[0]["is_parallel"] = 1
    return L


CASES = [
    # name, W, H, spl, spp, radius, max_delta, parallel
    ("input", 64, 64, 256, 2, 0.05, 0, False),
    ("mis_test", 48, 48, 256, 1, 0.05, 0, False),
    ("cornell_sphere_2k", 48, 48, 256, 1, 0.05, 0, False),
    ("input_parallel", 48, 48, 256, 1, 0.05, 0, True),
    ("input_delta_cap", 48, 48, 128, 1, 0.05, 1, False),
    ("input_radius", 48, 48, 128, 1, 0.13, 0, False),
]


def _load(sio, name, W, H):
    base = name.split("_")[0] if name.startswith("input") else name
    if base in ("input", "mis_test"):
        sc = sio.load_scene(os.path.join(GOLDEN, "scenes", base + ".txt"))
        (L, sp, tr), cam = sio.flatten_for_pt(sc), sio.camera_for(sc, W, H)
    else:
        from conftest import scene_by_name
        (L, sp, tr), (eye, look, up) = scene_by_name(sio, name)
        cam = sio.make_camera(eye, look, up, 50.0, W, H)
    return L, sp, tr, cam


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_render_ppm_matches_the_oracle(hpt, sio, plib, case):
    name, W, H, spl, spp, radius, max_delta, parallel = case
    L, sp, tr, cam = _load(sio, name, W, H)
    if parallel:
        L = _parallel(L)
    with hpt.Scene(L, sp, tr) as s:
        img = s.render_ppm(cam, W, H, 4, 4, spp, spl, radius, hpt.make_params(seed=11, max_delta=max_delta))
        st = s.ppm_stats()
    ref, rst = ppm_oracle.render(plib, L, sp, tr, cam, W, H, 4, 4, spp, spl, radius, seed=11, max_delta=max_delta)
    assert rst["deposits"] > 0 and rst["hit_points"] > 0
    for k in ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert float(np.abs(img - ref).max()) == 0.0
    assert img.tobytes() == ref.tobytes()


def test_same_seed_same_bytes_and_counts(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 64, 64)
    with hpt.Scene(L, sp, tr) as s:
        p = hpt.make_params(seed=4, flags=hpt.FLAG_COUNT_WORK | hpt.FLAG_TIME_KERNELS)
        a = s.render_ppm(cam, 64, 64, 4, 4, 1, 512, params=p)
        sa = s.ppm_stats()
        b = s.render_ppm(cam, 64, 64, 4, 4, 1, 512, params=p)
        sb = s.ppm_stats()
    assert a.tobytes() == b.tobytes()
    assert sa["candidates"] == sb["candidates"] > 0 and sa["accepted"] == sb["accepted"] > 0
    assert sa["cand_max"] >= sa["cand_median"] and sa["ms_gather"] > 0


def test_reference_named_wrapper_is_one_pass_of_render_ppm(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 48, 40)
    mn, mx = ppm_oracle.scene_bounds(sp, tr)
    mn = mn - np.float32(0.25)                         # bounds as given, not the scene's own
    with hpt.Scene(L, sp, tr) as s:
        ref = s.render_ppm(cam, 48, 40, 4, 4, 1, 128, params=hpt.make_params(seed=21), scene_min=mn, scene_max=mx)
    ref_so = C.CDLL(os.path.join(CSRC, "libhpt_ref.so"))
    sym = [ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(CSRC, "libhpt_ref.so")],
                                                          text=True).splitlines() if "ppm_render_wrapper" in ln][0]
    fn = getattr(ref_so, sym)
    fn.restype = None

    class F3(C.Structure):
        _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    class Cam(C.Structure):
        _fields_ = [(n, F3) for n in ("eye", "U", "V", "W", "UL", "dx", "dy")]

    camc = Cam.from_buffer_copy(np.ascontiguousarray(cam).tobytes())
    L = np.ascontiguousarray(L); sp = np.ascontiguousarray(sp); tr = np.ascontiguousarray(tr)
    os.environ["HPT_SEED"] = "21"
    try:
        outs = []
        for spp in (1, 7):
            img = np.zeros((40, 48, 3), np.float32)
            fn(L.ctypes.data_as(C.c_void_p), len(L), sp.ctypes.data_as(C.c_void_p), len(sp), tr.ctypes.data_as(C.c_void_p), len(tr),
               F3(*mn), F3(*mx), camc, img.ctypes.data_as(C.c_void_p), 48, 40, 4, 128, 4, spp)
            outs.append(img)
    finally:
        del os.environ["HPT_SEED"]
    assert outs[0].tobytes() == ref.tobytes()
    assert outs[1].tobytes() == ref.tobytes()


def test_cli_ppm_png_equals_tonemapped_c_abi_image(tmp_path, hpt, sio):
    cli = os.path.join(CSRC, "pt_cli")
    scene = os.path.join(GOLDEN, "scenes", "input.txt")
    out = str(tmp_path / "ppm.png")
    run = subprocess.run([cli, "--mode", "ppm", "--input", scene, "--output", out, "--spp", "2", "--spl", "64", "--seed", "13",
                          "--width", "40", "--height", "32"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "Mode   : ppm" in run.stdout and "[Success] Image saved!" in run.stdout
    from test_host_mirror import _decode_png
    png = _decode_png(open(out, "rb").read())
    sc = sio.load_scene(scene)
    L, sp, tr = sio.flatten_for_pt(sc)
    cam = sio.camera_for(sc, 40, 32, 50.0)
    with hpt.Scene(L, sp, tr) as s:
        img = s.render_ppm(cam, 40, 32, 4, 4, 2, 64, params=hpt.make_params(seed=13))
    assert img.max() > 0
    assert np.array_equal(png, hpt.tonemap(img))


def test_invalid_arguments(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 16, 16)
    with hpt.Scene(L, sp, tr) as s:
        for p, spl in ((hpt.make_params(world=2, rank=0), 8), (hpt.make_params(flags=hpt.FLAG_RUSSIAN_ROULETTE), 8),
                       (hpt.make_params(flags=hpt.FLAG_SINGLE_PIPELINE), 8), (hpt.make_params(), -1)):
            with pytest.raises(hpt.HptError, match="hpt error 1:"):
                s.render_ppm(cam, 16, 16, 4, 4, 1, spl, params=p)


def test_pt_render_unchanged_by_a_ppm_render(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 48, 48)
    with hpt.Scene(L, sp, tr) as s:
        a = s.render_pt(cam, 48, 48, 4, 8, hpt.make_params(seed=3))
        s.render_ppm(cam, 64, 64, 4, 4, 1, 2048, params=hpt.make_params(seed=3))
        b = s.render_pt(cam, 48, 48, 4, 8, hpt.make_params(seed=3))
    assert a.tobytes() == b.tobytes()
