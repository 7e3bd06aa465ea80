"""Motion (include/hpt.h, "motion") without a device: the oracle's motion guide against closed forms, the numpy restatement
of hpt_history_advance_motion against the plain history's and against its own definition, what the feature is for on the
CPU oracles alone, the boundary, and every refusal that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rmse
import history_cases as hc
import moments_oracle as mo
import motion_cases as mc
import motion_history_oracle as mho
import motion_oracle
import refit_cases as rc

f32 = np.float32
HPT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def mlib(tmp_path_factory):
    return motion_oracle.build(tmp_path_factory.mktemp("motion_oracle"))


def _bits_equal(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(-1)


# ---- the oracle's guide --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["none", "keep_after_update", "alive_then_dead"])
def test_static_geometry_gives_the_position_bits(mlib, name):
    """G' = G byte for byte (never updated, or kept after the update), or only never-hit dead triangles differ."""
    g, hp = mc.guide_oracle(mlib, name)
    assert sum(hp) > 0 and g["prev_position"].tobytes() == g["position"].tobytes()


def test_the_first_four_images_are_the_guides_oracle(mlib, tmp_path):
    import guides_oracle
    glib = guides_oracle.build(tmp_path)
    case = mc.GUIDE_BY_NAME["turn_5"]
    (L, sp, tr), _, _ = mc.replay(case)
    ref, hp = guides_oracle.render(glib, L, sp, tr, mc.guide_camera(case), case.W, case.H, case.spp, seed=mc.SEED, sample_offset=case.offset)
    g, hp2 = mc.guide_oracle(mlib, "turn_5")
    assert hp == hp2 and all(g[k].tobytes() == ref[k].tobytes() for k in ref)


def _one_sample(mlib, name):
    """The case at one sample per pixel, where a pixel is one hit point: (guides, pixels on moved geometry)."""
    case = mc.GUIDE_BY_NAME[name]
    (L, sp, tr), (psp, ptr), _ = mc.replay(case)
    g, _ = motion_oracle.render(mlib, L, sp, tr, psp, ptr, mc.guide_camera(case), case.W, case.H, 1, seed=mc.SEED, sample_offset=case.offset)
    moved = (g["coverage"] > 0) & ~_bits_equal(g["position"], g["prev_position"])
    return g, moved


# "A few ulp of the scene's extent": X and the vertices are coordinates no larger than the room (extent 2.1, ulp 2.4e-7);
# X itself carries one such rounding from ro + rd * t, the reconstruction adds about ten float operations whose
# cancellation in den grows with the triangles' aspect (close to 1 on the 12 x 12 tessellation), and the closed form is
# evaluated in double from the float X: 8 ulp of the extent.
EXTENT_TOL = 8 * float(np.spacing(f32(2.1)))


def test_a_translation_gives_the_point_minus_the_translation(mlib):
    g, moved = _one_sample(mlib, "translation")
    assert moved.sum() > 50
    err = np.abs(g["position"][moved].astype(np.float64) - np.array((0.125, -0.0625, -0.25)) - g["prev_position"][moved])
    print("translation: max error %.3g (bound %.3g)" % (err.max(), EXTENT_TOL))
    assert err.max() <= EXTENT_TOL


@pytest.mark.parametrize("name,deg", [("turn_5", 5.0), ("turn_40", 40.0)])
def test_a_turn_gives_the_inverse_turn(mlib, name, deg):
    g, moved = _one_sample(mlib, name)
    assert moved.sum() > 50
    back = rc.rotate_y(g["position"][moved].astype(np.float64), mc.MESH_C, -deg)
    err = np.abs(back - g["prev_position"][moved])
    print("%s: max error %.3g (bound %.3g)" % (name, err.max(), EXTENT_TOL))
    assert err.max() <= EXTENT_TOL


def test_a_moved_sphere_maps_onto_the_previous_sphere(mlib):
    g, moved = _one_sample(mlib, "sphere_both")
    (_, sp, _), (psp, _), _ = mc.replay(mc.GUIDE_BY_NAME["sphere_both"])
    on = moved & (np.abs(np.linalg.norm(g["position"].astype(np.float64) - sp[0]["center"], axis=-1) - sp[0]["r"]) < 1e-5)
    assert on.sum() > 20
    d = np.linalg.norm(g["prev_position"][on].astype(np.float64) - psp[0]["center"], axis=-1)
    assert np.abs(d - psp[0]["r"]).max() < 1e-5


def test_dead_and_sliver_cases_poison_exactly_the_pixels_they_should(mlib):
    # previous vertices that were dead: the pixels whose hit point lies on a revived triangle, and no other
    g, _ = mc.guide_oracle(mlib, "dead_then_alive")
    case = mc.GUIDE_BY_NAME["dead_then_alive"]
    (L, sp, tr), (psp, ptr), _ = mc.replay(case)
    bad = ~np.isfinite(g["prev_position"]).all(-1)
    assert bad.sum() > 0 and np.isfinite(g["position"]).all()
    assert g["prev_position"][~bad].tobytes() == g["position"][~bad].tobytes()
    # the same pixels see another surface (or a hole) when the revived triangles are taken out of the current scene
    holes, _ = motion_oracle.render(mlib, L, sp, ptr, psp, ptr, mc.guide_camera(case), case.W, case.H, case.spp, seed=mc.SEED, sample_offset=case.offset)
    assert (bad == ~_bits_equal(holes["position"], g["position"])).all()
    # den = 0 on a triangle that has area: non-finite where a sliver is hit, the rest of the image untouched
    g, _ = mc.guide_oracle(mlib, "sliver")
    bad = ~np.isfinite(g["prev_position"]).all(-1)
    assert bad.sum() > 0 and g["prev_position"][~bad].tobytes() == g["position"][~bad].tobytes()
    # ... and those pixels are the ones a sliver covers: without the slivers they show something else
    case = mc.GUIDE_BY_NAME["sliver"]
    (L, sp, tr), _, _ = mc.replay(case)
    bare, _ = motion_oracle.render(mlib, L, sp, tr[:-8], sp, tr[:-8], mc.guide_camera(case), case.W, case.H, case.spp, seed=mc.SEED, sample_offset=case.offset)
    assert (bad == ~_bits_equal(bare["position"], g["position"])).all()


def test_keep_previous_decides_what_an_update_is_measured_against(mlib):
    a, _ = mc.guide_oracle(mlib, "keep_between_updates")        # 10 degrees seen against 5
    b, _ = mc.guide_oracle(mlib, "two_updates_no_keep")         # 10 degrees seen against 0
    assert a["position"].tobytes() == b["position"].tobytes() and a["prev_position"].tobytes() != b["prev_position"].tobytes()
    for case in mc.GUIDE_CASES:
        _, _, motion = mc.replay(case)
        assert motion == (bool(case.steps) and case.steps[-1][0] != "keep")


# ---- the history oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["orbit_5", "bad_guides", "null_guides_moved", "border_4", "reset_mid_sequence"])
def test_without_the_motion_guide_the_oracle_is_the_plain_one(name):
    steps = hc.CASES[name]
    W, H = hc.size_of(steps)
    plain = hc.run_oracle(steps, W, H)
    h, q = mho.MotionHistory(W, H), mo.MomentHistory(W, H)
    k = 0
    for step in steps:
        if step[0] == "reset":
            h.reset(); q.reset()
            continue
        a = step[1]
        g = a["guides"] or {}
        args = (a["camera"], a["frame"], g.get("normal"), g.get("position"), g.get("coverage"))
        mean = h.advance(*args, **a["params"])
        q.advance(*args, **a["params"])
        assert mean.tobytes() == plain[k][0].tobytes() and h.n.tobytes() == plain[k][1].tobytes()
        assert (h.kept, h.restarted, h.K) == plain[k][2:] and h.q.tobytes() == q.q.tobytes()
        k += 1


def test_still_static_pixels_are_an_exact_running_mean():
    steps = mc.HISTORY_CASES["still_cover_uncover"]
    W, H = mc.size_of(steps)
    out = mc.run_history_oracle(steps, W, H)
    adv = [s[1] for s in steps]
    static = np.ones((H, W), bool)          # never on or behind the sphere, in any frame
    for a in adv:
        g = a["guides"]
        static &= _bits_equal(g["position"], g["prev_position"]) & _bits_equal(g["position"], adv[0]["guides"]["position"])
    assert 0.5 < static.mean() < 1.0
    mean = adv[0]["frame"].copy()
    for k in range(1, len(adv)):
        mean = ((mean * f32(k) + adv[k]["frame"]) / (f32(k) + f32(1.0))).astype(f32)
        assert out[k]["mean"][static].tobytes() == mean[static].tobytes()
        assert (out[k]["length"][static] == k + 1).all()


def test_every_branch_is_reached_in_the_table():
    total = dict.fromkeys(mho.BRANCHES, 0)
    for name, steps in mc.HISTORY_CASES.items():
        W, H = mc.size_of(steps)
        for o in mc.run_history_oracle(steps, W, H):
            assert o["kept"] + o["restarted"] == (W * H if o["frames"] > 1 else 0)
            if sum(o["branches"].values()):
                assert sum(o["branches"].values()) == W * H          # every pixel takes exactly one
            for k, v in o["branches"].items():
                total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_the_poisoned_pixels_restart():
    steps = mc.HISTORY_CASES["poisoned"]
    W, H = mc.size_of(steps)
    out = mc.run_history_oracle(steps, W, H)
    n = out[2]["length"]
    for y, x in [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]:
        assert n[y, x] == 1.0, (y, x)
    assert n[5, 5] == 1.0                     # its previous record had no coverage (3')
    assert np.isfinite(out[2]["mean"]).all() and np.isfinite(out[3]["mean"]).all()
    assert out[2]["branches"]["3_no_cover"] == 1


def test_no_geometry_motion_equals_the_plain_history():
    for name in ("static_scene",):
        steps = mc.HISTORY_CASES[name]
        W, H = mc.size_of(steps)
        a, b = mc.run_history_oracle(steps, W, H), mc.run_history_oracle(steps, W, H, motion=False)
        for x, y in zip(a, b):
            assert x["mean"].tobytes() == y["mean"].tobytes() and x["length"].tobytes() == y["length"].tobytes()
            assert (x["kept"], x["restarted"]) == (y["kept"], y["restarted"]) and x["q"].tobytes() == y["q"].tobytes()


# ---- what the feature is for ---------------------------------------------------------------------------------------

SPIN = dict(W=48, H=36, frames=8, deg=5.0, spp=2, guide_spp=4, depth=4, ref_spp=512)


def spin_records(f):
    L, sp, tr = mc.base()
    return L, sp, mc.moved_mesh(tr, mc.turn(SPIN["deg"] * f)) if f else tr


def spin_chain(oracle_mod, mlib, seed):
    """A still camera, the mesh turned 5 degrees more every frame: (mean under motion reprojection, last frame alone --
    what a reset after every update leaves --, static pixels of the last frame, kept share of the last frame)."""
    k = SPIN
    cam = mc.sio.make_camera(mc.sio.CORNELL_EYE, mc.sio.CORNELL_LOOK, mc.sio.CORNELL_UP, 50.0, k["W"], k["H"])
    h = mho.MotionHistory(k["W"], k["H"])
    for f in range(k["frames"]):
        L, sp, tr = spin_records(f)
        _, _, ptr = spin_records(max(f - 1, 0))
        off = f * k["spp"]
        img, _ = oracle_mod.pt_render(L, sp, tr, cam, k["W"], k["H"], k["depth"], k["spp"], seed=seed, sample_offset=off)
        g, _ = motion_oracle.render(mlib, L, sp, tr, sp, ptr, cam, k["W"], k["H"], k["guide_spp"], seed=seed, sample_offset=off)
        mean = h.advance(cam, img, g["normal"], g["position"], g["coverage"], prev_position=g["prev_position"])
    static = (g["coverage"] > 0) & _bits_equal(g["position"], g["prev_position"])
    return mean, img, static, h.kept / float(k["W"] * k["H"])


@pytest.fixture(scope="module")
def spin_reference(oracle_mod):
    k = SPIN
    cam = mc.sio.make_camera(mc.sio.CORNELL_EYE, mc.sio.CORNELL_LOOK, mc.sio.CORNELL_UP, 50.0, k["W"], k["H"])
    L, sp, tr = spin_records(k["frames"] - 1)
    ref, _ = oracle_mod.pt_render(L, sp, tr, cam, k["W"], k["H"], k["depth"], k["ref_spp"], seed=99)
    return ref


@pytest.mark.parametrize("seed", [3, 17, 41])
def test_following_the_motion_beats_a_reset_after_every_update(oracle_mod, mlib, spin_reference, seed):
    """48 x 36, 2 spp frames, the 264-triangle mesh turning 5 degrees a frame for 8 frames under a still camera, against a
    512 spp oracle render of the last pose.  Measured RMSE, motion reprojection / reset after every update: seed 3 0.1161 /
    0.3424 over all pixels and 0.1073 / 0.3397 over the static ones; seed 17 0.1794 / 0.2744 and 0.0989 / 0.1681; seed 41
    0.1334 / 0.2588 and 0.1216 / 0.2360; 93 % of the pixels kept on the last frame."""
    mean, last, static, kept = spin_chain(oracle_mod, mlib, seed)
    e_m, e_r = rmse(mean, spin_reference), rmse(last, spin_reference)
    s_m, s_r = rmse(mean[static], spin_reference[static]), rmse(last[static], spin_reference[static])
    print("seed %d: all pixels motion %.4f reset %.4f (ratio %.3f); static pixels motion %.4f reset %.4f (ratio %.3f); kept %.1f %%"
          % (seed, e_m, e_r, e_m / e_r, s_m, s_r, s_m / s_r, 100 * kept))
    assert np.isfinite(mean).all() and 0.5 < static.mean() < 1.0
    assert e_m < e_r
    assert s_m < s_r


# ---- the boundary --------------------------------------------------------------------------------------------------

DECLARED = ["hpt_scene_keep_previous", "hpt_scene_has_motion", "hpt_render_guides_motion", "hpt_render_guides_motion_device",
            "hpt_history_advance_motion", "hpt_history_motion_check"]


def test_header_declares_the_calls_and_python_has_the_front_end(hpt):
    text = open(os.path.join(ROOT, "include", "hpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hpt.load_library()
    for name in DECLARED:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    for word in ("den = d00 * d11 - d01 * d01", "k = r' / r", "sky stays sky", "acos(normal_min)", "hpt_scene_keep_previous sets G' := G"):
        assert word in text, word
    assert "reset the history after an\n * update" not in text and "no notion of a scene over time" not in text
    assert hasattr(hpt.Scene, "keep_previous") and hasattr(hpt.Scene, "has_motion") and hasattr(hpt, "history_motion_check")


def _refused(lib, rc, *words):
    assert rc == HPT_ERR_INVALID, (rc, lib.hpt_last_error())
    msg = lib.hpt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_refusals_before_the_device_is_touched(hpt):
    lib = hpt.load_library()
    _refused(lib, lib.hpt_scene_keep_previous(None), b"null scene")
    assert lib.hpt_scene_has_motion(None) < 0 and b"null scene" in lib.hpt_last_error()
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    W, H = 5, 3
    n = W * H * 3 * 4
    cam = np.ascontiguousarray(hc.camera(W, H), hpt.CAMERA).reshape(1)
    camp = cam.ctypes.data_as(C.c_void_p)
    vp = lambda off: C.c_void_p(base + off)
    frame, nrm, pos, cov, out, prev = vp(0), vp(n), vp(2 * n), vp(3 * n), vp(4 * n), vp(5 * n)
    for fn in (lib.hpt_render_guides_motion, lib.hpt_render_guides_motion_device):
        _refused(lib, fn(None, camp, W, H, 1, None, frame, nrm, pos, cov, prev), b"null scene")
    _refused(lib, lib.hpt_history_advance_motion(None, camp, frame, nrm, pos, cov, prev, None, out, None), b"null history")

    def check(camera=camp, f=frame, a=nrm, b=pos, c=cov, q=prev, p=None, o=out, W=W, H=H):
        return lib.hpt_history_motion_check(W, H, camera, f, a, b, c, q, p, o)

    assert check() == 0 and check(o=None) == 0 and check(o=frame) == 0 and check(q=pos) == 0
    # a null motion guide is hpt_history_check, refusal for refusal
    assert check(q=None) == 0 and check(q=None, a=None, b=None, c=None) == 0
    _refused(lib, check(q=None, a=None), b"all three or not at all")
    _refused(lib, check(a=None, b=None, c=None), b"needs the three guide images")
    _refused(lib, check(a=None), b"all three or not at all")
    _refused(lib, check(W=0), b"positive")
    _refused(lib, check(camera=None), b"null camera")
    _refused(lib, check(f=None), b"null frame")
    bad = hpt.make_history_params(); bad.flags = 1
    _refused(lib, check(p=C.byref(bad)), b"flags")
    _refused(lib, check(p=C.byref(hpt.make_history_params(max_history=0.5))), b"hpt_history_params")
    c2 = cam.copy(); c2["dx"] = (0.0, 0.0, 0.0)
    _refused(lib, check(camera=c2.ctypes.data_as(C.c_void_p)), b"degenerate camera")
    for kw in (dict(q=frame), dict(q=vp(n - 4)), dict(q=out), dict(q=vp(4 * n + 8)), dict(q=vp(5 * n), o=vp(5 * n + n - 4)), dict(q=frame, o=frame)):
        _refused(lib, check(**kw), b"must not overlap")
    with pytest.raises(hpt.HptError, match="needs the three guide images"):
        hpt.history_motion_check(W, H, cam, base, prev_position=base + 5 * n)
    hpt.history_motion_check(W, H, cam, base, base + n, base + 2 * n, base + 3 * n, base + 5 * n, mean_out=base + 4 * n)
