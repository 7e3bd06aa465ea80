"""CPU tests of the temporal history (include/hpt.h, "history across camera moves"): the sanity of the numpy oracle and
of the case table the device is held to, the projection's round trip, the presence of the calls in the header and of the
Python classes, the refusals the host makes before it touches a device, and the end-to-end chain of the oracles -- path
tracer, guides, history -- on the project's scene."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import history_cases as hc
import history_oracle as ho
from conftest import GOLDEN, ROOT, rmse

HPT_ERR_INVALID = 1
f32 = np.float32


@pytest.fixture(scope="module")
def expected():
    return {name: hc.run_oracle(steps, *hc.size_of(steps)) for name, steps in hc.CASES.items()}


def _advance(h, cam, g, f, **params):
    return h.advance(cam, f, g["normal"], g["position"], g["coverage"], **params)


# ---- the oracle ---------------------------------------------------------------------------------------------------------

def test_reprojected_mean_is_closer_to_the_noise_free_colour_than_a_restart():
    W, H = 96, 64
    A, B = hc.camera(W, H), hc.orbit(W, H, 5.0)
    gA, gB = hc.guides(A, W, H), hc.guides(B, W, H)
    h = ho.History(W, H)
    for k in range(8):
        _advance(h, A, gA, hc.frame(gA, k))
    fB = hc.frame(gB, 99)
    mean = _advance(h, B, gB, fB)
    kept = h.n > 1
    truth = hc.colour_of(gB["position"])
    assert h.kept == kept.sum() > 0.9 * W * H and h.restarted == (~kept).sum() > 0
    e_hist, e_restart = rmse(mean[kept], truth[kept]), rmse(fB[kept], truth[kept])
    print("5 degree orbit, 8 frames behind it: rmse of the history %.4f, of the restart %.4f (noise sigma 0.15)" % (e_hist, e_restart))
    assert e_hist < 0.5 * e_restart                 # 8 frames + 1: sigma / 3 were the reprojection exact
    assert (mean[~kept] == fB[~kept]).all() and (h.n[~kept] == 1).all()
    assert h.n[kept].max() <= 9.0 + 1e-5 and np.median(h.n[kept]) > 8.9


def test_pixels_that_were_behind_the_sphere_restart():
    """A wall point of the new view whose segment to the PREVIOUS eye passes well inside the sphere was not on screen a
    frame ago; what the previous frame stored along that line is the sphere's surface, a long way off the wall's plane."""
    W, H = 96, 64
    A, B = hc.camera(W, H), hc.orbit(W, H, 15.0)
    gA, gB = hc.guides(A, W, H), hc.guides(B, W, H)
    h = ho.History(W, H)
    _advance(h, A, gA, hc.frame(gA, 1))
    _advance(h, B, gB, hc.frame(gB, 2))
    X = gB["position"].astype(np.float64)
    eye = np.asarray(A["eye"], np.float64)
    d = X - eye
    t = np.clip(((hc.SPHERE_C - eye) * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
    closest = np.linalg.norm(eye + t[..., None] * d - hc.SPHERE_C, axis=-1)
    on_wall = np.linalg.norm(X - hc.SPHERE_C, axis=-1) > hc.SPHERE_R + 0.05
    hidden = on_wall & (closest < 0.8 * hc.SPHERE_R)
    assert hidden.sum() >= 20
    assert (h.n[hidden] == 1).all()
    assert (h.n[on_wall & (closest > 1.5 * hc.SPHERE_R)] == 2).mean() > 0.8      # the rest entered the image at its border


def test_unmoved_camera_is_a_running_mean(expected):
    steps = hc.CASES["still_default"]
    frames = np.stack([s[1]["frame"] for s in steps]).astype(np.float64)
    out = expected["still_default"]
    for k, (mean, n, kept, restarted, K) in enumerate(out):
        assert K == k + 1 and (n == k + 1).all() and (kept, restarted) == ((0, 0) if k == 0 else (mean.shape[0] * mean.shape[1], 0))
        exact = frames[:k + 1].mean(0)
        # k float operations of relative error 2^-24 each on values below 2 (a mean of colours around 0.5)
        assert np.abs(mean - exact).max() <= 4 * (k + 1) * 2.0 ** -24
    # max_history 4: an exponential average with weight 1/4 from the fourth frame on; 1: the frame itself
    capped = expected["still_max_history_4"]
    f4 = [s[1]["frame"] for s in hc.CASES["still_max_history_4"]]
    assert (capped[3][1] == 4).all() and (capped[6][1] == 4).all()
    want = (capped[5][0].astype(np.float64) * 3 + f4[6]) / 4
    assert np.abs(capped[6][0] - want).max() <= 2.0 ** -21
    one = expected["still_max_history_1"]
    f1 = [s[1]["frame"] for s in hc.CASES["still_max_history_1"]]
    for k in range(8):
        assert one[k][0].tobytes() == f1[k].tobytes() and (one[k][1] == 1).all()
    assert one[3][2] == 23 * 5                      # kept all the same: the history's weight is 0, not its presence


def test_kept_plus_restarted_is_the_pixel_count(expected):
    for name, out in expected.items():
        W, H = hc.size_of(hc.CASES[name])
        for step, res in zip([s for s in hc.CASES[name] if s[0] == "advance"], out):
            mean, n, kept, restarted, K = res
            if K == 1:
                assert (kept, restarted) == (0, 0) and (n == 1).all(), name
            else:
                assert kept + restarted == W * H, name
            if "max_history_1" not in name:
                assert kept == (n > 1).sum(), name


def test_case_table_is_sane(expected):
    assert [hc.size_of(hc.CASES["size_%dx%d" % s]) for s in hc.SIZES] == [(1, 1), (1, 7), (7, 1), (5, 3), (67, 3), (96, 64)]
    share = lambda name, k: expected[name][k][2] / float(np.prod(hc.size_of(hc.CASES[name])))
    assert share("orbit_0.5", 3) == 1.0 and 0.9 < share("orbit_5", 3) < 1.0 and 0.8 < share("orbit_15", 3) < share("orbit_5", 3)
    assert 0.5 < share("dolly", 4) < 1.0
    assert [r[2] for r in expected["turn_180"]] == [0, 1200, 0, 0]                 # everything restarts, twice
    assert [r[2] for r in expected["null_guides_moved"]] == [0, 0, 0, 1200]        # restart, coverage 0 stored, restart, still
    assert expected["null_guides_unmoved"][2][2] > 1100                            # the kept guides still reproject
    assert [r[2] for r in expected["null_guides_first"]][:3] == [0, 1200, 0]
    base = [r[2] for r in expected["orbit_5"]]
    for name in ("plane_off", "normal_off", "both_off", "tight"):
        assert expected["switch_" + name][2][0].tobytes() != expected["switch_both_off" if name != "both_off" else "switch_tight"][2][0].tobytes()
    assert expected["switch_both_off"][2][2] >= expected["switch_plane_off"][2][2] >= expected["switch_tight"][2][2]
    assert expected["switch_both_off"][2][2] > expected["switch_tight"][2][2] and base[3] > 0
    for name in ("bad_guides", "bad_guides_tests_off"):
        for mean, n, kept, restarted, K in expected[name]:
            assert np.isfinite(mean).all() and np.isfinite(n).all() and (n >= 1).all(), name
        n_moved = expected[name][2][1]
        assert (n_moved[0, :2] == 1).all() and (n_moved[1, :4] == 1).all() and (n_moved[2, :2] == 1).all() and (n_moved[3, :3] == 1).all()
        steps = hc.CASES[name]
        assert expected[name][2][0][1, :4].tobytes() == steps[2][1]["frame"][1, :4].tobytes()     # a restart writes the frame's colour
    assert expected["reset_mid_sequence"][3][2:] == (0, 0, 1) and expected["reset_mid_sequence"][4][4] == 2


def test_border_and_weight_floor_cases_reach_what_they_are_for():
    seen = set()
    for k in range(6):
        steps = hc.CASES["border_%d" % k]
        h = ho.History(13, 9)
        for s in steps:
            _advance(h, s[1]["camera"], s[1]["guides"], s[1]["frame"])
        w = np.where(np.isnan(h.wsum), f32(0), h.wsum)      # NaN: the previous coordinate left the range, no tap was read
        for side, edge in (("left", w[:, 0]), ("right", w[:, -1]), ("top", w[0, :]), ("bottom", w[-1, :])):
            if (edge < 0.999).all() and (edge > 0).any():
                seen.add(side)                       # taps of that border's pixels fell outside the image, others counted
        if np.isnan(h.wsum).any():
            seen.add("out of range")
    assert seen == {"left", "right", "top", "bottom", "out of range"}
    sums = {}
    for name in ("below", "above"):
        steps = hc.CASES["weight_floor_" + name]
        h = ho.History(13, 9)
        for s in steps:
            _advance(h, s[1]["camera"], s[1]["guides"], s[1]["frame"])
        sums[name] = h.wsum[:, -1]
        assert (h.wsum[:, :-1] == 1).all()
        assert ((h.n[:, -1] == 1) == (name == "below")).all()
    assert (sums["below"] > 0.007).all() and (sums["below"] < 0.0099).all()
    assert (sums["above"] > 0.0101).all() and (sums["above"] < 0.013).all()


# ---- the projection -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", [(96, 64, hc.EYE, hc.LOOK, hc.UP), (33, 77, (0.0, 0.0, -2.0), (0.5, 0.5, 1.0), (0.0, 1.0, 0.0)),
                                  (1024, 1024, (0.3, 1.2, -3.0), (0.1, 0.2, 0.5), (0.1, 1.0, 0.05)), (640, 360, (5.0, 2.0, 7.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))])
def test_projection_round_trip(sio, view):
    """Points at distances 0.5 .. 50 along primary rays, rounded to float, come back under their pixel coordinate.  The
    error grows with the coordinate (it is a float of that size) and with the rounding of the point itself: observed here
    at most 4.9e-7 x max(W, H) pixels over these four cameras (1.7e-5 pixel at 96 x 64, 3.9e-4 at 1024 x 1024); the bound is
    4 x that.  Either is far below the one pixel the direct-view test allows."""
    W, H, eye, look, up = view
    cam = sio.make_camera(eye, look, up, hc.FOV, W, H)
    c = ho.constants(cam)
    rng = np.random.default_rng(5)
    n = 100000
    u, v, dist = rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(0.5, 50.0, n)
    e = np.asarray(cam["eye"], np.float64)
    d = (np.asarray(cam["UL"], np.float64) - e) + u[:, None] * np.asarray(cam["dx"], np.float64) + v[:, None] * np.asarray(cam["dy"], np.float64)
    d /= np.linalg.norm(d, axis=1)[:, None]
    s, uu, vv, dist2 = ho.project(c, (e + dist[:, None] * d).astype(f32))
    err = max(np.abs(uu - u).max(), np.abs(vv - v).max())
    print("%d x %d: round trip within %.3g pixel = %.3g x max(W, H)" % (W, H, err, err / max(W, H)))
    assert (s > 0).all() and err <= 4 * 4.9e-7 * max(W, H)
    assert np.abs(np.sqrt(dist2) / dist - 1).max() < 1e-5
    sb, _, _, _ = ho.project(c, (e - dist[:, None] * d).astype(f32))
    assert (sb < 0).all()                            # behind the camera


# ---- the boundary -------------------------------------------------------------------------------------------------------

DECLARED = ["hpt_history_create", "hpt_history_advance", "hpt_history_metrics", "hpt_history_read", "hpt_history_reset",
            "hpt_history_destroy", "hpt_history_check", "hpt_render_guides_device"]


def test_header_declares_the_calls_and_python_has_the_classes(hpt):
    text = open(os.path.join(ROOT, "include", "hpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hpt.load_library()
    for name in DECLARED:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    for field in ("max_history", "plane_tolerance", "normal_min", "flags"):
        assert re.search(r"\b%s\s*;" % field, code[code.index("typedef struct hpt_history_params"):]), field
    for word in ("direct view", "wsum > 0.01f", "BEFORE any conversion", "no motion vectors", "exponential average", "colour only"):
        assert word in text, word
    for m in ("advance", "metrics", "read", "reset", "close", "__enter__", "__exit__"):
        assert hasattr(hpt.History, m), m
    assert hasattr(hpt.Scene, "render_guides_device") and C.sizeof(hpt.HistoryParams) == 16


def _refused(lib, rc, *words):
    assert rc == HPT_ERR_INVALID, (rc, lib.hpt_last_error())
    msg = lib.hpt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_refusals_before_the_device_is_touched(hpt, sio):
    """No device is needed (and none is there under -m "not gpu").  hpt_history_check is the list of checks an advance
    makes on a live object, in the same order, callable without one; tests/test_gpu_history.py repeats a few through
    hpt_history_advance itself."""
    lib = hpt.load_library()
    h = C.c_void_p()
    for W, H in ((0, 4), (4, 0), (-1, 4), (4, -7)):
        _refused(lib, lib.hpt_history_create(W, H, C.byref(h)), b"positive")
        assert not h.value
    _refused(lib, lib.hpt_history_create(1 << 15, 1 << 14, C.byref(h)), b"too large")
    _refused(lib, lib.hpt_history_create(4, 4, None), b"null")
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    W, H = 5, 3
    n = W * H * 3 * 4
    cam = np.ascontiguousarray(hc.camera(W, H), hpt.CAMERA).reshape(1)
    camp = cam.ctypes.data_as(C.c_void_p)
    vp = lambda off: C.c_void_p(base + off)
    frame, nrm, pos, cov, out = vp(0), vp(n), vp(2 * n), vp(3 * n), vp(4 * n)
    _refused(lib, lib.hpt_history_advance(None, camp, frame, nrm, pos, cov, None, out, None), b"null history")
    _refused(lib, lib.hpt_history_metrics(None, None, None, None), b"null history")
    _refused(lib, lib.hpt_history_read(None, None, None, None), b"null history")
    _refused(lib, lib.hpt_history_reset(None, None), b"null history")
    lib.hpt_history_destroy(None)

    def check(camera=camp, f=frame, a=nrm, b=pos, c=cov, p=None, o=out, W=W, H=H):
        return lib.hpt_history_check(W, H, camera, f, a, b, c, p, o)

    assert check() == 0 and check(a=None, b=None, c=None) == 0 and check(o=None) == 0 and check(o=frame) == 0
    _refused(lib, check(W=0), b"positive")
    _refused(lib, check(camera=None), b"null camera")
    _refused(lib, check(f=None), b"null frame")
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(a=None, b=None), dict(a=None, c=None), dict(b=None, c=None)):
        _refused(lib, check(**kw), b"all three or not at all")
    P = hpt.make_history_params
    for p in (P(max_history=0.5), P(max_history=-3), P(max_history=float("nan")), P(plane_tolerance=float("nan")), P(normal_min=float("nan"))):
        _refused(lib, check(p=C.byref(p)), b"hpt_history_params")
    bad = P(); bad.flags = 1
    _refused(lib, check(p=C.byref(bad)), b"flags")
    for p in (P(), P(max_history=1), P(max_history=1e9), P(plane_tolerance=-1), P(normal_min=-5), P(normal_min=1.5), P(plane_tolerance=1e30)):
        assert check(p=C.byref(p)) == 0, lib.hpt_last_error()

    def broken(**fields):
        c2 = cam.copy()
        for k, v in fields.items():
            c2[k] = v
        return c2

    zero = (0.0, 0.0, 0.0)
    for c2 in (broken(dx=zero), broken(dy=zero), broken(dy=cam["dx"][0]), broken(UL=cam["eye"][0]), broken(eye=(np.nan, 0, 0)),
               broken(UL=(np.inf, 0, 0)), broken(dx=(1e30, 0, 0), dy=(0, 1e30, 0)), broken(UL=cam["eye"][0] + cam["dx"][0])):
        _refused(lib, check(camera=c2.ctypes.data_as(C.c_void_p)), b"degenerate camera")
    # overlaps: any two of the five images but mean-out on the frame itself
    for kw in (dict(o=vp(4)), dict(o=vp(n - 4)), dict(a=vp(n - 4)), dict(b=vp(n + 8)), dict(c=vp(4 * n + n - 4)), dict(o=pos), dict(o=nrm),
               dict(c=vp(n - 4)), dict(a=frame), dict(b=nrm), dict(c=pos), dict(o=vp(3 * n + W * H * 4 - 4))):
        _refused(lib, check(**kw), b"must not overlap")
    assert check(c=vp(3 * n), o=vp(3 * n + W * H * 4)) == 0          # the coverage image is a third as long: what follows it is free


# ---- end to end: path tracer, guides, history, all as oracles ------------------------------------------------------------

def chain_inputs(sio):
    """Cameras and per-frame parameters of the end-to-end chain (also run on the device by tests/test_gpu_history.py)."""
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", "input.txt"))
    W, H = 48, 36
    A = sio.make_camera(sc.eye, sc.look_at, sc.view_up, hc.FOV, W, H)
    B = sio.make_camera(hc.orbit_eye(sc.eye, sc.look_at, sc.view_up, 2.0), sc.look_at, sc.view_up, hc.FOV, W, H)
    return sc, W, H, [A, A, A, A, B], dict(seed=29, spp=2, guide_spp=4, depth=4)


def cpu_chain(sio, oracle_mod, glib):
    """Per frame (frame, guides or None, mean, kept): guides on frame 0 and on the moved frame."""
    import guides_oracle
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    h = ho.History(W, H)
    out = []
    for f, cam in enumerate(cams):
        off = f * k["spp"]
        img, _ = oracle_mod.pt_render(L, sp, tr, cam, W, H, k["depth"], k["spp"], seed=k["seed"], sample_offset=off)
        g = None
        if f == 0 or cam.tobytes() != cams[f - 1].tobytes():
            g, _ = guides_oracle.render(glib, L, sp, tr, cam, W, H, k["guide_spp"], seed=k["seed"], sample_offset=off)
        mean = h.advance(cam, img, *((g["normal"], g["position"], g["coverage"]) if g else (None, None, None)))
        out.append((img, g, mean, h.kept))
    return out


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    import guides_oracle
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


def test_end_to_end_chain_beats_the_restart(sio, oracle_mod, glib):
    """input.txt at 48 x 36: four frames of 2 spp from the scene's camera, then one from the camera orbited by 2 degrees.
    The moved frame's history against a 1024 spp oracle render of the moved camera has a lower RMSE than the moved frame
    alone, which is what a restart shows.  Measured: history 0.5779, restart 0.6611 (both carry the
    fireflies of 2 spp frames around the light), 70.1 % of the pixels kept."""
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    out = cpu_chain(sio, oracle_mod, glib)
    converged, _ = oracle_mod.pt_render(L, sp, tr, cams[-1], W, H, k["depth"], 1024, seed=7)
    frame, _, mean, kept = out[-1]
    e_hist, e_restart = rmse(mean, converged), rmse(frame, converged)
    print("moved frame vs 1024 spp: history %.4f, restart %.4f, kept %.1f %%" % (e_hist, e_restart, 100.0 * kept / (W * H)))
    assert np.isfinite(mean).all() and kept > 0
    assert e_hist < e_restart
