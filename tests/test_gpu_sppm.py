"""Progressive photon mapping on the MI355X: Scene.sppm against the SPPM oracle (tests/sppm_oracle.cpp) bit for bit,
including the cull's candidate counts; a first pass with alpha = 1 against render_ppm; passes split across calls,
reset and reruns; state untouched by other renders on the scene; argument errors; the CLI."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import sppm_oracle
from test_gpu_ppm import CASES, _load, _parallel

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slib(tmp_path_factory):
    return sppm_oracle.build(tmp_path_factory.mktemp("sppm_oracle"))


def _case(sio, case):
    name, W, H, spl, _spp, radius, max_delta, parallel = case
    L, sp, tr, cam = _load(sio, name, W, H)
    if parallel:
        L = _parallel(L)
    return L, sp, tr, cam, W, H, spl, radius, max_delta


@pytest.mark.parametrize("alpha", [0.5, 0.7])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sppm_matches_the_oracle(hpt, sio, slib, case, alpha):
    L, sp, tr, cam, W, H, spl, radius, max_delta = _case(sio, case)
    ref = sppm_oracle.State(slib, L, sp, tr, cam, W, H, spl=spl, radius=radius, alpha=alpha, seed=11, max_delta=max_delta)
    with hpt.Scene(L, sp, tr) as s:
        with s.sppm(cam, W, H, 4, 4, spl, radius, alpha, hpt.make_params(seed=11, max_delta=max_delta)) as z:
            for it in range(4):
                img = z.render(1, flags=hpt.FLAG_COUNT_WORK)
                st = s.ppm_stats()
                rimg, rst = ref.render(1)
                for k in ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels", "candidates", "accepted"):
                    assert st[k] == rst[k], (it, k, st[k], rst[k])
                assert img.tobytes() == rimg.tobytes(), it
            state = z.state()
    assert rst["hit_points"] > 0 and rst["deposits"] > 0
    assert state["passes"] == 4
    assert state["radius2"].tobytes() == ref.r2.tobytes()
    assert state["photons"].tobytes() == ref.n.tobytes()


@pytest.mark.parametrize("name", ["input", "cornell_sphere_2k"])
def test_one_pass_alpha_one_is_render_ppm(hpt, sio, name):
    L, sp, tr, cam = _load(sio, name, 48, 40)
    with hpt.Scene(L, sp, tr) as s:
        ppm = s.render_ppm(cam, 48, 40, 4, 4, 1, 256, 0.05, hpt.make_params(seed=7, sample_offset=2))
        with s.sppm(cam, 48, 40, 4, 4, 256, 0.05, 1.0, hpt.make_params(seed=7, sample_offset=2)) as z:
            img = z.render(1)
    assert ppm.max() > 0
    assert img.tobytes() == ppm.tobytes()


def test_split_calls_reset_and_reruns(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 48, 48)
    with hpt.Scene(L, sp, tr) as s:
        p = hpt.make_params(seed=19)
        with s.sppm(cam, 48, 48, 4, 4, 256, 0.05, 0.7, p) as a, s.sppm(cam, 48, 48, 4, 4, 256, 0.05, 0.7, p) as b:
            a.render(3)
            split = a.render(2)
            sa = a.state()
            whole = b.render(5)
            sb = b.state()
            a.reset()
            assert a.state()["passes"] == 0
            again = a.render(5)
            sr = a.state()
        with s.sppm(cam, 48, 48, 4, 4, 256, 0.05, 0.7, p) as c:
            rerun = c.render(5)
    assert sa["passes"] == sb["passes"] == sr["passes"] == 5
    assert split.tobytes() == whole.tobytes() == again.tobytes() == rerun.tobytes()
    assert sa["radius2"].tobytes() == sb["radius2"].tobytes() == sr["radius2"].tobytes()
    assert sa["photons"].tobytes() == sb["photons"].tobytes()
    r0 = np.float32(0.05) * np.float32(0.05)
    assert (sa["radius2"] <= r0).all() and (sa["radius2"] < r0).any()


def test_other_renders_in_between_change_nothing(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 48, 48)
    p = hpt.make_params(seed=23)
    with hpt.Scene(L, sp, tr) as s:                   # references: no state alive
        pt_ref = s.render_pt(cam, 40, 32, 4, 4, hpt.make_params(seed=3))
        ppm_ref = s.render_ppm(cam, 64, 64, 4, 4, 1, 512, 0.07, hpt.make_params(seed=3))
        with s.sppm(cam, 48, 48, 4, 4, 256, 0.05, 0.7, p) as z:
            z.render(2)
            ref = z.render(2)
    with hpt.Scene(L, sp, tr) as s:
        with s.sppm(cam, 48, 48, 4, 4, 256, 0.05, 0.7, p) as z:
            z.render(2)
            pt = s.render_pt(cam, 40, 32, 4, 4, hpt.make_params(seed=3))
            ppm = s.render_ppm(cam, 64, 64, 4, 4, 1, 512, 0.07, hpt.make_params(seed=3))
            got = z.render(2)
    assert got.tobytes() == ref.tobytes()
    assert pt.tobytes() == pt_ref.tobytes() and ppm.tobytes() == ppm_ref.tobytes()


def test_invalid_arguments(hpt, sio):
    L, sp, tr, cam = _load(sio, "input", 16, 16)
    err = pytest.raises
    with hpt.Scene(L, sp, tr) as s:
        for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=-0.5), dict(alpha=float("nan")), dict(eye_depth=0),
                   dict(eye_depth=256), dict(light_depth=0), dict(light_depth=256), dict(spl=-1),
                   dict(params=hpt.make_params(world=2, rank=0))):
            with err(hpt.HptError, match="hpt error 1:"):
                s.sppm(cam, 16, 16, **kw)
        bad = hpt.make_params()
        bad.reserved = 2
        with err(hpt.HptError, match="hpt error 1:"):
            s.sppm(cam, 16, 16, params=bad)
        with s.sppm(cam, 16, 16, spl=8) as z:
            for passes, flags in ((0, 0), (-1, 0), (1, hpt.FLAG_OUTPUT_SUM), (1, hpt.FLAG_RUSSIAN_ROULETTE), (1, hpt.FLAG_BRUTE_FORCE)):
                with err(hpt.HptError, match="hpt error 1:"):
                    z.render(passes, flags)
            assert z.state()["passes"] == 0
            z.render(1, hpt.FLAG_TIME_KERNELS | hpt.FLAG_COUNT_WORK)
            st = s.ppm_stats()
            assert st["ms_gather"] > 0 and st["candidates"] > 0 and z.state()["passes"] == 1


def test_cli_sppm_png_equals_tonemapped_python_image(tmp_path, hpt, sio):
    cli = os.path.join(CSRC, "pt_cli")
    scene = os.path.join(GOLDEN, "scenes", "input.txt")
    out = str(tmp_path / "sppm.png")
    run = subprocess.run([cli, "--mode", "sppm", "--input", scene, "--output", out, "--spp", "3", "--spl", "64", "--seed", "13",
                          "--alpha", "0.6", "--radius", "0.08", "--width", "40", "--height", "32"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "Mode   : sppm" in run.stdout and "[Success] Image saved!" in run.stdout
    from test_host_mirror import _decode_png
    png = _decode_png(open(out, "rb").read())
    sc = sio.load_scene(scene)
    L, sp, tr = sio.flatten_for_pt(sc)
    cam = sio.camera_for(sc, 40, 32, 50.0)
    with hpt.Scene(L, sp, tr) as s:
        with s.sppm(cam, 40, 32, 4, 4, 64, 0.08, 0.6, hpt.make_params(seed=13)) as z:
            img = z.render(3)
    assert img.max() > 0
    assert np.array_equal(png, hpt.tonemap(img))
