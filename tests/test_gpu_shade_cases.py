"""k_shade, the BSDF functions, the host-filled material and light tables and the photon-mapping kernels on the MI355X, on
the hostile material and light records of tests/shade_cases.py: fields that are NaN, infinite, negative, denormal or
-0.0, a zero or non-finite light direction, a light ball whose centre is not the light's position.  Records are not
validated (include/hpt.h), so the image must be what the reference's expressions give on those bits: every comparison is
of bytes against the CPU oracle, which tests/test_shade_cases_cpu.py holds to the reference's own code on the same
records, and which that file shows lit, finite and reached by the hostile records (so nothing here can agree by being
black).  Every render is 48 x 40 at 3 spp and eye depth 4."""
import os

import numpy as np
import pytest

import pt_cases as pc
import shade_cases as sc
from conftest import GOLDEN
from kat_records import same_bits
from test_gpu_ppm_coverage import olib, ppm_parity, sppm_parity               # noqa: F401  (olib: the fixture)
from test_gpu_reference_pin import TRIG_FREE, TRIG_FREE_ON_DELTA

pytestmark = pytest.mark.gpu


def _render(hpt, scene, args, **more):
    L, sp, tr, cam, w, h, depth, spp, kw = args
    return scene.render_pt(cam, w, h, depth, spp, hpt.make_params(**dict(kw, **more)))


def _same(what, img, ref):
    bad = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1)
    print("%s: %d of %d pixels differ, lit %.1f %%" % (what, int(bad.sum()), bad.size, 100.0 * pc.lit_share(ref)))
    assert np.array_equal(img, ref), "%s: %d of %d pixels differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist())


# ---- function level -------------------------------------------------------------------------------------------------
def test_device_functions_equal_the_oracle_on_hostile_materials(hpt, oracle_mod):
    """k_probe_functions (the per-hit route: no MatPre) against the oracle with the shared polynomial trig, all 40 columns."""
    _, rec = sc.hostile_records()
    got, want = hpt.probe_functions(rec), oracle_mod.function_kats(rec)
    ok = same_bits(got, want)
    assert ok.all(), "columns %s, records %s" % (sorted(set(np.nonzero(~ok)[1])), sorted(set(np.nonzero(~ok)[0]))[:20])


def test_device_functions_equal_the_reference_on_hostile_materials(hpt):
    g = np.load(os.path.join(GOLDEN, "ref_hostile_functions.npz"))
    rec, ref = g["records"], g["table"]
    ok = same_bits(hpt.probe_functions(rec), ref)
    bad = ~ok[:, TRIG_FREE]
    assert not bad.any(), "columns %s, records %s" % (sorted({TRIG_FREE[c] for c in np.nonzero(bad)[1]}), sorted(set(np.nonzero(bad)[0]))[:20])
    delta = ref[:, 11] == 1.0
    assert delta.sum() > 200
    bad = ~ok[np.ix_(delta, TRIG_FREE_ON_DELTA)]
    assert not bad.any(), "delta records: columns %s, records %s" % (sorted({TRIG_FREE_ON_DELTA[c] for c in np.nonzero(bad)[1]}),
                                                                     sorted(set(np.nonzero(delta)[0][np.nonzero(bad)[0]]))[:20])


# ---- path tracing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_render_equals_the_oracle(hpt, oracle_mod, name):
    """Every case, the 129-material and 33-light variants (tables read from global memory) and the hostile triangles."""
    args, ref, _ = sc.reference(oracle_mod, name)
    with hpt.Scene(*args[:3]) as scene:
        _same(name, _render(hpt, scene, args), ref)
        st = scene.stats()
    if name == "rough-out-129":
        assert st["n_materials"] == sc.N_MATS
    if name == "radius-out-33":
        assert len(args[0]) == sc.N_LIGHTS


@pytest.mark.parametrize("name", sc.ROUTE_CASES)
def test_every_route_through_the_shade_kernels_gives_the_oracles_image(hpt, oracle_mod, name):
    args, ref, _ = sc.reference(oracle_mod, name)
    rr, _ = pc.oracle_render(oracle_mod, args, russian_roulette=True)
    assert not np.array_equal(rr, ref)
    with hpt.Scene(*args[:3]) as scene:
        _same("single pipeline", _render(hpt, scene, args, flags=hpt.FLAG_SINGLE_PIPELINE), ref)
        _same("no host wait", _render(hpt, scene, args, flags=hpt.FLAG_NO_HOST_WAIT), ref)
        _same("one sample per pass", _render(hpt, scene, args, samples_per_pass=1), ref)
        _same("brute force", _render(hpt, scene, args, flags=hpt.FLAG_BRUTE_FORCE), ref)
        _same("russian roulette", _render(hpt, scene, args, flags=hpt.FLAG_RUSSIAN_ROULETTE), rr)


@pytest.mark.parametrize("name", sc.UPDATE_CASES)
def test_a_light_update_refills_the_table_with_hostile_lights_and_back(hpt, oracle_mod, name):
    """update_rounds from ordinary lights to the block's and back, one render per step: for `split` the update changes
    light_ball.center on one light and light_ball.r alone on another."""
    args, ref, _ = sc.reference(oracle_mod, name)
    good = (sc.good_lights(name),) + tuple(args[1:])
    gref, _ = pc.oracle_render(oracle_mod, good)
    assert not np.array_equal(gref, ref)
    with hpt.Scene(*good[:3]) as scene:
        _same("good lights", _render(hpt, scene, good), gref)
        scene.update_rounds(args[0], args[1])
        _same("hostile lights", _render(hpt, scene, args), ref)
        scene.update_rounds(good[0], good[1])
        _same("good lights again", _render(hpt, scene, good), gref)


# ---- photon mapping -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.PPM_SPL))
def test_ppm_equals_its_oracle(hpt, olib, name):                                # noqa: F811
    L, sp, tr, cam, w, h = sc.CASE_BY_NAME[name].make()[:6]
    img, st = ppm_parity(hpt, olib, L, sp, tr, cam, w, h, eye_depth=sc.DEPTH, spl=sc.PPM_SPL[name])
    assert st["deposits"] >= sc.PPM_MIN_DEPOSITS and st["accepted"] >= sc.PPM_MIN_ACCEPTED


@pytest.mark.parametrize("name", sc.SPPM_CASES)
def test_sppm_equals_its_oracle(hpt, olib, name):                               # noqa: F811
    L, sp, tr, cam, w, h = sc.CASE_BY_NAME[name].make()[:6]
    _, rst = sppm_parity(hpt, olib, L, sp, tr, cam, w, h, calls=(1, 2), eye_depth=sc.DEPTH, spl=sc.PPM_SPL[name])
    assert rst["accepted"] >= sc.PPM_MIN_ACCEPTED
