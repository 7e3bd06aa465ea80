"""The hostile material and light records of tests/shade_cases.py on the CPU: the oracle held to what the reference's own
code computed on them (tests/golden/ref_hostile_functions.npz, ref_hostile_pt.npz; generator tests/golden/make_ref_golden.py,
regenerated and compared by test_reference_pin_cpu.py), the conditions under which the GPU comparisons of
test_gpu_shade_cases.py mean something (lit shares, NaN caps, pixels per hostile sphere, rays per light block), and the two
oracles under the address and undefined-behaviour sanitizers (tests/shade_check.cpp).  No tolerance anywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ppm_oracle
import pt_cases as pc
import shade_cases as sc
from kat_records import same_bits
from path_tracing_amd.layouts import CAMERA, LIGHT, SPHERE, TRIANGLE
from test_reference_pin_cpu import REPLAY, _load, _rec, _scene

ALL = [c.name for c in sc.CASES]
LIGHT_NAMES = [c.name for c in sc.LIGHT_CASES] + ["radius-out-33"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- function level -------------------------------------------------------------------------------------------------
def test_oracle_functions_equal_the_reference_on_hostile_materials(oracle_mod):
    g = _load("ref_hostile_functions.npz")
    assert g["table"].shape == (len(g["records"]), 40)
    got = oracle_mod.function_kats(g["records"], trig_mode=1)
    same = same_bits(got, g["table"])
    assert same.all(), "columns %s, records %s" % (sorted(set(np.nonzero(~same)[1])), sorted(set(np.nonzero(~same)[0]))[:20])


def test_hostile_function_fixture_holds_every_value_bit_for_bit():
    g = _load("ref_hostile_functions.npz")
    names, rec = sc.hostile_records()
    assert np.array_equal(_bits(g["records"]), _bits(rec)) and list(g["block_names"]) == list(names)
    assert len(sc.FUNCTION_BLOCKS) == 37 and len(set(names)) == 37 and (np.unique(names, return_counts=True)[1] == 10 * sc.FUNCTION_N).all()
    for name, col, v in sc.FUNCTION_BLOCKS:
        block = g["records"][g["block_names"] == name]
        want = np.asarray(v, np.float32).reshape(-1)
        cols = [0, 1, 2] if col == 0 else [col]
        for c, w in zip(cols, want):
            assert (_bits(block[:, c]) == _bits(w)).all(), (name, c)
    den = np.float32(sc.DEN)
    assert 0 < den < np.finfo(np.float32).tiny                                  # the denormal is one in float32
    assert (_bits(g["records"][g["block_names"] == "roughness=nzero", 3]) == 0x80000000).all()


def test_hostile_function_table_reaches_every_branch_and_is_mostly_numbers():
    g = _load("ref_hostile_functions.npz")
    t, rec, names = g["table"], g["records"], g["block_names"]
    delta = t[:, 11] == 1.0
    assert (delta & (rec[:, 5] > 0)).sum() > 100                                # smooth dielectric: reflection or refraction
    assert (delta & ~(rec[:, 5] > 0)).sum() > 100                               # mirror
    assert (delta & (t[:, 12] != rec[:, 18])).sum() > 40                        # refractions that change the medium
    assert (~delta & (t[:, 10] > 0)).sum() > 1000                               # the rough branch
    assert (~delta & (t[:, 10] == 0.0)).sum() > 100                             # rejected samples: pdf == 0
    shares = {}
    for name in dict.fromkeys(names):
        b = t[names == name]
        shares[name] = float(np.isnan(b).mean())
        print("%-28s NaN %5.1f %%  inf %4d  delta %3d  pdf == 0 %3d" % (name, 100 * shares[name], int(np.isinf(b).sum()), int((b[:, 11] == 1).sum()),
                                                                       int((b[:, 10] == 0).sum())))
    assert any(np.isinf(t[names == n]).any() for n in shares) and any(np.isnan(t[names == n]).any() for n in shares)
    assert max(shares.values()) <= sc.MAX_BLOCK_NAN, max(shares, key=shares.get)
    assert float((~np.isnan(t)).mean()) >= sc.MIN_ALL_NON_NAN
    assert shares["roughness=nan"] < 0.01                                       # fmaxf swallows it


# ---- the PT kernel --------------------------------------------------------------------------------------------------
def test_pt_fixture_holds_the_cases_of_the_table():
    g = _load("ref_hostile_pt.npz")
    assert [str(c) for c in g["cases"]] == sc.FIXTURE_PT
    assert set(ALL) - set(sc.FIXTURE_PT) == {"rough-out-129", "radius-out-33"}
    for case in sc.FIXTURE_PT:
        L, sp, tr, cam, W, H, depth, spp, kw = sc.CASE_BY_NAME[case].make()
        fl, fs, ft = _scene(g, case)
        assert fl.tobytes() == L.tobytes() and fs.tobytes() == sp.tobytes() and ft.tobytes() == tr.tobytes(), case
        assert _rec(g[case + "/camera"], CAMERA).tobytes() == np.asarray(cam).tobytes()
        assert [int(v) for v in g[case + "/params"]] == [sc.W, sc.H, sc.DEPTH, sc.SPP, sc.SEED] == [W, H, depth, spp, kw["seed"]]


@pytest.mark.parametrize("case", sc.FIXTURE_PT)
def test_oracle_replay_equals_the_reference_kernel_on_hostile_records(oracle_mod, case):
    g = _load("ref_hostile_pt.npz")
    L, sp, tr = _scene(g, case)
    W, H, depth, spp, seed = (int(v) for v in g[case + "/params"])
    cam = _rec(g[case + "/camera"], CAMERA)[0]
    img, st = oracle_mod.pt_render(L, sp, tr, cam, W, H, depth, spp, seed=seed, threads=1, **REPLAY)
    assert st["max_delta_run"] <= 32, "a path came near the cap of 64 free delta bounces: %d" % st["max_delta_run"]
    assert np.array_equal(img.view(np.uint32), g[case + "/image"].view(np.uint32))


# ---- the conditions of the GPU comparisons, on the oracle's default mode -------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_case_is_lit_finite_and_reaches_its_hostile_records(oracle_mod, name):
    args, img, st = sc.reference(oracle_mod, name)
    first = sc.first_hits(oracle_mod, name, args)
    nonfinite = int((~np.isfinite(img)).any(axis=-1).sum())
    print("%-15s lit %5.1f %%  closest %6d  shadow %5d  odd %d  nonfinite %d  first %s" % (
        name, 100 * pc.lit_share(img), st["closest_rays"], st["shadow_rays"], st["odd_bounce_rays"], nonfinite, first))
    assert (name in sc.DARK) == (sc.CASE_BY_NAME[name].dark is not None)
    if name not in sc.DARK:
        assert pc.lit_share(img) >= 0.5
    assert nonfinite == 0
    assert st["odd_bounce_rays"] == 0                       # k_trace meets no non-finite or denormal ray: k_shade and the tables are under test
    assert st["max_delta_run"] <= 32
    if name in LIGHT_NAMES:
        assert len(first) == 1 and first[0] >= 1            # light hits at depth 0: a primary ray ends on a hostile light ball
        if name != "eye-inside":
            assert st["shadow_rays"] >= sc.MIN_SHADOW_RAYS
        else:
            assert first[0] == sc.W * sc.H and st["shadow_rays"] == 0
    else:
        assert min(first) >= sc.MIN_FIRST_HIT, first


def test_blocks_hold_the_listed_records():
    for name, mats in sc.MATERIAL_BLOCKS.items():
        sp = sc.CASE_BY_NAME[name].make()[1]
        got = np.stack([sp["mtl"]["base_color"][:, 0], sp["mtl"]["base_color"][:, 1], sp["mtl"]["base_color"][:, 2], sp["mtl"]["roughness"],
                        sp["mtl"]["metallic"], sp["mtl"]["eta"]], axis=1)
        assert np.array_equal(_bits(got), _bits(np.asarray(mats, np.float32))), name
    rough = np.asarray(sc.TRIANGLE_MATS, np.float32)
    assert {0x80000000, int(_bits(np.array([sc.DEN], np.float32))[0])} <= set(_bits(rough[:, 3]).tolist())
    tr = sc.CASE_BY_NAME["rough-tris"].make()[2]
    assert len(tr) == 12 + 2 * len(rough) and np.array_equal(_bits(tr["mtl"]["roughness"][12::2]), _bits(rough[:, 3]))
    assert np.isnan(tr["mtl"]["roughness"]).any() and np.isnan(tr["mtl"]["eta"]).sum() == 4
    L = sc.CASE_BY_NAME["radius-out"].make()[0]
    r = L["light_ball"]["r"]
    assert np.isin(_bits(np.array([0.0, -0.05, 1e-30, 5.0, np.inf, 3e-20], np.float32)), _bits(r)).all()
    assert np.isnan(r).sum() == 1 and (L["pos"][7] == L["pos"][8]).all() and r[7] != r[8]
    area = np.float32(4.0) * np.float32(np.pi) * np.float32(3e-20) * np.float32(3e-20)
    assert 0 < area < np.finfo(np.float32).tiny              # the denormal area
    L = sc.CASE_BY_NAME["cone-out"].make()[0]
    assert np.isnan(L["cutoff"]).sum() == 1 and np.isinf(L["cutoff"]).sum() == 1 and {0.0, -1.0, 7.0} <= set(L["cutoff"].tolist())
    assert ((L["dir"] == 0).all(axis=1) & (L["is_parallel"] == 1)).sum() == 1 and ((L["dir"] == 0).all(axis=1) & (L["is_parallel"] == 0)).sum() == 1
    assert np.isnan(L["dir"]).any() and np.isinf(L["dir"]).any()
    L = sc.CASE_BY_NAME["illum-out"].make()[0]
    assert np.isnan(L["illum"]).any(axis=1).sum() == 2 and (L["is_parallel"] == 1).sum() == 2 and np.isinf(L["illum"]).any()
    L = sc.CASE_BY_NAME["split"].make()[0]
    assert (L["light_ball"]["center"][0] != L["pos"][0]).all() and (L["light_ball"]["center"][1:] == L["pos"][1:]).all()


def test_table_size_variants_pass_the_lds_copies():
    L, sp, tr = sc.CASE_BY_NAME["rough-out-129"].make()[:3]
    assert pc.n_materials(sp, tr) == sc.N_MATS == 129
    assert sp.tobytes() == sc.CASE_BY_NAME["rough-out"].make()[1].tobytes()
    L33 = sc.CASE_BY_NAME["radius-out-33"].make()[0]
    L8 = sc.CASE_BY_NAME["radius-out"].make()[0]
    assert len(L33) == sc.N_LIGHTS == 33 and L33[:len(L8)].tobytes() == L8.tobytes()


@pytest.mark.parametrize("name", sc.UPDATE_CASES)
def test_good_lights_are_ordinary_and_render_another_image(oracle_mod, name):
    args, img, _ = sc.reference(oracle_mod, name)
    G = sc.good_lights(name)
    assert len(G) == len(args[0]) and G.tobytes() != args[0].tobytes()
    assert np.isfinite(G["light_ball"]["r"]).all() and (G["light_ball"]["r"] > 0).all() and (G["light_ball"]["center"] == G["pos"]).all()
    if name == "split":
        a, b = G.copy(), args[0].copy()
        assert a[2].tobytes() == b[2].tobytes()
        a["light_ball"]["r"][1] = b["light_ball"]["r"][1]
        assert a[1].tobytes() == b[1].tobytes()              # light 1: light_ball.r alone
        a["light_ball"]["center"][0] = b["light_ball"]["center"][0]
        assert a.tobytes() == b.tobytes()                    # light 0: light_ball.center alone
    good, _ = pc.oracle_render(oracle_mod, (G,) + tuple(args[1:]))
    assert pc.lit_share(good) >= 0.5 and not np.array_equal(good, img)


def test_a_moved_ball_centre_alone_changes_the_image(oracle_mod):
    args, img, _ = sc.reference(oracle_mod, "split")
    L = args[0].copy()
    L["light_ball"]["center"][0] = L["pos"][0]
    unmoved, _ = pc.oracle_render(oracle_mod, (L,) + tuple(args[1:]))
    assert not np.array_equal(unmoved, img)


# ---- photon mapping -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def olib(tmp_path_factory):
    return ppm_oracle.build(tmp_path_factory.mktemp("shade_ppm_oracle"))


def test_ppm_cases_are_the_ones_the_issue_names():
    assert set(sc.PPM_SPL) == set(sc.MATERIAL_BLOCKS) | {"radius-out", "illum-out", "cone-out", "split"}
    assert sc.SPPM_CASES == ["mixed", "cone-out"] and set(sc.PPM_DARK) <= set(sc.PPM_SPL)


@pytest.mark.parametrize("name", list(sc.PPM_SPL))
def test_ppm_case_is_lit_at_its_photon_count(olib, name):
    L, sp, tr, cam, W, H = sc.CASE_BY_NAME[name].make()[:6]
    img, st = ppm_oracle.render(olib, L, sp, tr, cam, W, H, sc.DEPTH, 4, 1, sc.PPM_SPL[name], 0.05, seed=11, max_delta=0, want_work=True)
    print("%-15s spl %5d  lit %5.1f %%  deposits %6d  accepted %6d" % (name, sc.PPM_SPL[name], 100 * pc.lit_share(img), st["deposits"], st["accepted"]))
    assert np.isfinite(img).all()
    if name in sc.PPM_DARK:
        assert st["deposits"] >= sc.PPM_MIN_DEPOSITS and st["accepted"] >= sc.PPM_MIN_ACCEPTED
    else:
        assert pc.lit_share(img) >= 0.5


# ---- the oracles under the sanitizers -------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CHECK_SPL = 256                       # photons per light of the cases PPM_SPL does not list


def _fnv1a(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_oracles_are_defined_behaviour_on_every_case(oracle_mod, olib, tmp_path):
    """tests/shade_check.cpp with oracle/pt_oracle.cpp and tests/ppm_oracle.cpp as one stand-alone program, address and
    undefined-behaviour sanitizers in (a float-to-int cast of a non-finite value included): it must exit 0 on every case,
    and its checksums must be those of the unsanitized oracles."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "shade_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-pthread"] + SAN_FLAGS + static
                          + ["-o", exe, os.path.join(_HERE, "shade_check.cpp"), os.path.join(_ROOT, "oracle", "pt_oracle.cpp"),
                             os.path.join(_HERE, "ppm_oracle.cpp")])
    src = str(tmp_path / "cases.bin")
    want = []
    with open(src, "wb") as f:
        f.write(np.array([len(sc.CASES)], np.int32).tobytes())
        for c in sc.CASES:
            args, img, _ = sc.reference(oracle_mod, c.name)
            L, sp, tr, cam, W, H, depth, spp, kw = args
            L, sp, tr = (np.ascontiguousarray(a) for a in (L, sp, tr))
            assert (L.dtype, sp.dtype, tr.dtype) == (LIGHT, SPHERE, TRIANGLE)
            spl = sc.PPM_SPL.get(c.name, CHECK_SPL)
            mn, mx = ppm_oracle.scene_bounds(sp, tr)
            f.write(np.array([len(L), len(sp), len(tr), W, H, depth, spp, spl], np.int32).tobytes())
            f.write(np.array([kw["seed"]], np.uint64).tobytes())
            f.write(np.concatenate([mn, mx]).astype(np.float32).tobytes())
            f.write(np.asarray(cam).tobytes()); f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
            replay, _ = oracle_mod.pt_render(L, sp, tr, cam, W, H, depth, spp, seed=kw["seed"], threads=1, **REPLAY)
            ppm, _ = ppm_oracle.render(olib, L, sp, tr, cam, W, H, depth, 4, 1, spl, 0.05, seed=11, max_delta=0, scene_min=mn, scene_max=mx)
            want.append("case %d pt=%016x replay=%016x ppm=%016x" % (len(want), _fnv1a(img.tobytes()), _fnv1a(replay.tobytes()), _fnv1a(ppm.tobytes())))
    run = subprocess.run([exe, src], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.splitlines() == want
