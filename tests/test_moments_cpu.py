"""CPU tests of the temporal variance (include/hpt.h, "temporal variance"): the sanity of the numpy oracle
(tests/moments_oracle.py) and of the case table the device is held to (tests/moments_cases.py), what the definition is for
-- a variance that is right for stationary noise and that sees the remnant of a rare bright sample where the spatial
estimate does not -- and the refusals the host makes before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guided_oracle as go
import history_cases as hc
import history_oracle as ho
import moments_cases as mc
import moments_oracle as mo
from conftest import GOLDEN, ROOT

HPT_ERR_INVALID = 1
f32 = np.float32


@pytest.fixture(scope="module")
def expected():
    return {name: mc.run_oracle(case) for name, case in mc.CASES.items()}


# ---- the table ----------------------------------------------------------------------------------------------------------

def test_every_history_case_is_run_with_moments_and_every_combination_occurs():
    names = {n[:-len("_fallback_only")] if n.endswith("_fallback_only") else n for n in mc.CASES}
    assert set(hc.CASES) <= names
    combos = {(c["min_length"], c["fallback"]) for c in mc.CASES.values()}
    assert combos == {(L, fb) for L in (0.0, 2.0) for fb in mc.FALLBACKS}
    assert {mc.size_of(mc.CASES["size_%dx%d" % s]) for s in hc.SIZES} == set(hc.SIZES)


def test_cases_reach_both_branches_unless_their_name_says_otherwise(expected):
    for name, res in expected.items():
        L = f32(mc.CASES[name]["min_length"] or 4.0)
        temporal = any((r["length"] >= L).any() for r in res)
        fallback = any((r["length"] < L).any() for r in res)
        assert fallback, name
        assert temporal == (not name.endswith("fallback_only")), name
        for r in res:                                           # the result is never NaN: bits can be compared on the device
            assert not np.isnan(r["variance"]).any(), name


def test_mean_length_and_counts_are_the_plain_historys_bytes(expected):
    for name, case in mc.CASES.items():
        plain = hc.run_oracle(case["steps"], *mc.size_of(case))
        assert len(plain) == len(expected[name])
        for k, (p, r) in enumerate(zip(plain, expected[name])):
            assert p[0].tobytes() == r["mean"].tobytes() and p[1].tobytes() == r["length"].tobytes(), (name, k)
            assert p[2:] == (r["kept"], r["restarted"], r["frames"]), (name, k)


def test_fallback_pattern_null_and_in_place(expected):
    for name, res in expected.items():
        case = mc.CASES[name]
        W, H = mc.size_of(case)
        L = f32(case["min_length"] or 4.0)
        fb = np.zeros((H, W, 3), f32) if case["fallback"] == "null" else mc.pattern(W, H)
        for r in res:
            short = r["length"] < L
            assert r["variance"][short].tobytes() == fb[short].tobytes(), name


def test_the_cases_about_the_second_moment_reach_what_they_are_for(expected):
    # n passes exactly 4 on a still camera: frame 3 (n = 3) is fallback everywhere, frame 4 (n = 4) temporal everywhere
    res = expected["still_passes_4"]
    fb = mc.pattern(23, 5)
    assert [float(r["length"].max()) for r in res] == [1, 2, 3, 4, 5, 6]
    assert res[2]["variance"].tobytes() == fb.tobytes() and (res[3]["variance"] < 1.0).all() and (res[3]["variance"] > 0).any()
    # ... against the two-pass variance of the frames in double: float rounding of q - m * m on values below 2 is about
    # 4 * 2^-24 * q absolute, q <= 1.6, against variances of the mean around 0.15^2 / 4 = 5.6e-3
    frames = np.stack([s[1]["frame"] for s in mc.CASES["still_passes_4"]["steps"]]).astype(np.float64)
    for k in (3, 4, 5):
        exact = frames[:k + 1].var(0) / k
        assert np.abs(res[k]["variance"] - exact).max() <= 2e-6
    # max_history 1: n = 1 forever, q = c * c, never temporal; 4: n - 1 = 3 from the fourth frame on
    one = expected["max_history_1_fallback_only"]
    for r, s in zip(one, mc.CASES["max_history_1_fallback_only"]["steps"]):
        c = s[1]["frame"]
        assert (r["length"] == 1).all() and r["q"].tobytes() == (c * c).tobytes() and not r["variance"].any()
    four = expected["max_history_4"]
    assert all((r["length"] == 4).all() for r in four[3:]) and all((r["variance"] < 1.0).all() for r in four[3:])
    # a reprojected n strictly between 1 and 2, so n - 1 is a fraction between 1 and 2, under min_length 2
    n = expected["fractional_length_min_2"][-1]["length"]
    frac = (n > 2) & (n < 3)
    assert frac.sum() >= 5 and (expected["fractional_length_min_2"][-1]["variance"][frac] < 1.0).all()
    assert (expected["fractional_length_min_2"][1]["length"] == 1).any()
    # non-finite colours: c * c overflows, q - m * m is inf - inf or NaN, and the variance there is 0, not NaN
    for name in ("non_finite", "non_finite_min_2_in_place"):
        res = expected[name]
        last = res[3]
        assert np.isinf(last["q"][1, 5]).all() and np.isfinite(last["mean"][1, 5]).all() and not last["variance"][1, 5].any()
        assert np.isnan(last["mean"][1, 2, 0]) and last["variance"][1, 2, 0] == 0
        assert np.isinf(last["mean"][1, 3]).all() and not last["variance"][1, 3].any()
        assert any(np.isnan(r["q"]).any() for r in res) and any(np.isinf(r["q"]).any() for r in res)
    # a reset: the frame after it is a first frame again, q = c * c, and the variance is the fallback
    res = expected["reset_between_advances"]
    c = mc.CASES["reset_between_advances"]["steps"][6][1]["frame"]
    assert [r["frames"] for r in res] == [1, 2, 3, 4, 5, 1, 2]
    assert res[5]["q"].tobytes() == (c * c).tobytes() and res[5]["variance"].tobytes() == mc.pattern(23, 5).tobytes()


# ---- what it is for -----------------------------------------------------------------------------------------------------

def test_still_camera_variance_is_sigma_squared_over_n():
    """32 frames of the room under Gaussian noise of sigma 0.15: the median over pixels and channels of
    variance / (sigma^2 / n) lies within [0.8, 1.25]."""
    W, H = hc.MOTION_SIZE
    cam = hc.camera(W, H)
    g = hc.guides(cam, W, H)
    h = mo.MomentHistory(W, H)
    for k in range(32):
        h.advance(cam, hc.frame(g, 500 + k, noise=0.15), g["normal"], g["position"], g["coverage"])
    assert (h.n == 32).all()
    ratio = float(np.median(h.variance() / (0.15 ** 2 / 32)))
    print("median variance / (sigma^2 / n) = %.3f" % ratio)
    assert 0.8 <= ratio <= 1.25


def _wall_scenario(seed, firefly):
    """The back wall at 64 x 48: 32 still frames, then a slide of (0.4, 0.3) pixel.  Noise: Gaussian of sigma 0.05 plus, with
    probability 1/200 per pixel and frame, a sample of +20 on all three channels (firefly), or plain Gaussian of sigma 0.15.
    The guided filter at its defaults, albedo 1, under the spatial estimate of the moved frame divided by the history
    length, and under that estimate patched with the temporal variance.  RMSE against the frames' expectation (the colour,
    plus 20 / 200 with fireflies) over the pixels at least 4 from the border with n >= 4: (input, spatial, temporal)."""
    W, H = 64, 48
    A, B = hc.wall_camera(W, H), hc.wall_camera(W, H, 0.4, 0.3)
    gA, gB = hc.guides(A, W, H, sphere=False), hc.guides(B, W, H, sphere=False)
    rng = np.random.default_rng(seed)

    def frame(g):
        if firefly:
            f = hc.colour_of(g["position"]) + rng.normal(0.0, 0.05, (H, W, 3)) + 20.0 * (rng.random((H, W, 1)) < 1.0 / 200.0)
        else:
            f = hc.colour_of(g["position"]) + rng.normal(0.0, 0.15, (H, W, 3))
        return f.astype(f32)

    h = mo.MomentHistory(W, H)
    for _ in range(32):
        h.advance(A, frame(gA), gA["normal"], gA["position"], gA["coverage"])
    fB = frame(gB)
    mean = h.advance(B, fB, gB["normal"], gB["position"], gB["coverage"])
    g = dict(gB, albedo=np.ones((H, W, 3), f32))
    spatial = go.estimate_variance(fB, g, h.n)
    temporal = h.variance(spatial)
    out_s, _ = go.run_guided(mean, spatial, g)
    out_t, _ = go.run_guided(mean, temporal, g)
    truth = hc.colour_of(gB["position"]) + (20.0 / 200.0 if firefly else 0.0)
    inner = np.zeros((H, W), bool)
    inner[4:-4, 4:-4] = True
    inner &= h.n >= 4
    assert inner.sum() > 2000
    e = lambda a: float(np.sqrt(((a[inner] - truth[inner]) ** 2).mean()))
    return e(mean), e(out_s), e(out_t)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_temporal_variance_removes_the_remnants_of_fireflies(seed):
    """Filtering under the temporal variance gives at most 0.75 of the RMSE under the spatial estimate.  Measured
    (input, spatial, temporal, ratio): seed 1: 0.1430, 0.1094, 0.0495, 0.453; seed 2: 0.1391, 0.1094, 0.0487, 0.446;
    seed 3: 0.1259, 0.1113, 0.0459, 0.413."""
    e_in, e_s, e_t = _wall_scenario(seed, True)
    print("seed %d: input %.4f, spatial %.4f, temporal %.4f, ratio %.3f" % (seed, e_in, e_s, e_t, e_t / e_s))
    assert e_t <= 0.75 * e_s


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plain_gaussian_noise_loses_nothing(seed):
    """Where the spatial estimate was already good the two agree: the ratio stays within [0.95, 1.05].  Measured 0.992,
    0.998, 0.996."""
    e_in, e_s, e_t = _wall_scenario(seed, False)
    print("seed %d: input %.4f, spatial %.4f, temporal %.4f, ratio %.3f" % (seed, e_in, e_s, e_t, e_t / e_s))
    assert 0.95 <= e_t / e_s <= 1.05


# ---- the boundary -------------------------------------------------------------------------------------------------------

DECLARED = ["hpt_history_create_flags", "hpt_history_variance", "hpt_history_read_moments", "hpt_history_variance_check"]


def test_header_declares_the_calls_and_python_has_them(hpt):
    text = open(os.path.join(ROOT, "include", "hpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hpt.load_library()
    for name in DECLARED:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+HPT_HISTORY_MOMENTS\s+1\b", code) and hpt.HISTORY_MOMENTS == 1
    for word in ("temporal variance", "q_r = qsum / wsum", "q = c * c", "fmaxf(d, 0.0f) / (n - 1.0f)", "errs on the high side", "exponential"):
        assert word in text, word
    assert hasattr(hpt.History, "variance") and hasattr(hpt, "history_variance_check")


def _refused(lib, rc, *words):
    assert rc == HPT_ERR_INVALID, (rc, lib.hpt_last_error())
    msg = lib.hpt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_refusals_before_the_device_is_touched(hpt):
    lib = hpt.load_library()
    lib.hpt_history_variance_check.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_float, C.c_void_p]
    h = C.c_void_p()
    for flags in (2, 3, 4, -1, 1 << 30):
        _refused(lib, lib.hpt_history_create_flags(4, 4, C.c_int32(flags), C.byref(h)), b"unknown flag")
        assert not h.value
    _refused(lib, lib.hpt_history_create_flags(0, 4, C.c_int32(1), C.byref(h)), b"positive")
    _refused(lib, lib.hpt_history_create_flags(4, 4, C.c_int32(1), None), b"null")
    lib.hpt_history_variance.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    _refused(lib, lib.hpt_history_variance(None, None, 0.0, None, None), b"null history")
    _refused(lib, lib.hpt_history_read_moments(None, None), b"null history")
    W, H = 5, 3
    n = W * H * 3 * 4
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    out, fb = base, base + n

    def check(fallback=fb, L=0.0, o=out, flags=1, W=W, H=H):
        return lib.hpt_history_variance_check(W, H, flags, fallback, L, o)

    assert check() == 0 and check(fallback=None) == 0 and check(fallback=out) == 0 and check(L=2.0) == 0 and check(L=1e9) == 0
    _refused(lib, check(W=0), b"positive")
    _refused(lib, check(flags=0), b"without HPT_HISTORY_MOMENTS")
    _refused(lib, check(flags=2), b"unknown flag")
    _refused(lib, check(o=None), b"null variance")
    for L in (1.0, 1.999, -4.0, float("nan"), float("-inf")):
        _refused(lib, check(L=L), b"min_length")
    for f, o in ((out + 4, out), (out + n - 4, out), (out, out + 4), (out, out + n - 4)):      # any overlap but the image itself
        _refused(lib, check(fallback=f, o=o), b"must not overlap")
    assert check(fallback=out + n) == 0
    with pytest.raises(hpt.HptError, match="hpt error 1:.*min_length"):
        hpt.history_variance_check(W, H, out, fb, min_length=1.5)
    with pytest.raises(hpt.HptError, match="hpt error 1:.*without HPT_HISTORY_MOMENTS"):
        hpt.history_variance_check(W, H, out, fb, moments=False)
    hpt.history_variance_check(W, H, out, out)


def test_cli_temporal_variance_needs_its_three_companions(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    png = tmp_path / "x.png"
    cli = os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_cli")
    companions = (["--frames", "2"], ["--reproject"], ["--guided"])
    for leave_out in range(4):
        extra = [w for k, c in enumerate(companions) if k != leave_out for w in c]
        if leave_out == 3:
            extra = []
        run = subprocess.run([cli, "--mode", "pt", "--input", scene_file, "--output", str(png), "--temporal-variance"] + extra,
                             capture_output=True, text=True)
        assert run.returncode != 0 and "--temporal-variance needs --frames" in run.stderr, (extra, run.stderr)
    assert not os.path.exists(png)
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert usage.returncode == 0 and "--temporal-variance" in usage.stdout


# ---- end to end: path tracer, guides, moments history, estimate, temporal variance, guided filter, all as oracles --------------

def chain_inputs(sio):
    """Cameras and per-frame parameters of the end-to-end chain (also run on the device by tests/test_gpu_moments.py): two
    frames from the scene's camera, then an orbit that grows by 0.5 degree per frame."""
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", "input.txt"))
    W, H = 48, 36
    cams = [sio.make_camera(hc.orbit_eye(sc.eye, sc.look_at, sc.view_up, 0.5 * max(f - 1, 0)), sc.look_at, sc.view_up, hc.FOV, W, H) for f in range(6)]
    return sc, W, H, cams, dict(seed=29, spp=2, guide_spp=4, depth=4)


def cpu_chain(sio, oracle_mod, glib):
    """Per frame dict(frame, length, q, estimate, variance, out, v): guides on frame 0 and on every moved frame."""
    import guides_oracle
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    h = mo.MomentHistory(W, H)
    out = []
    for f, cam in enumerate(cams):
        off = f * k["spp"]
        img, _ = oracle_mod.pt_render(L, sp, tr, cam, W, H, k["depth"], k["spp"], seed=k["seed"], sample_offset=off)
        moved = f == 0 or cam.tobytes() != cams[f - 1].tobytes()
        if moved:
            g, _ = guides_oracle.render(glib, L, sp, tr, cam, W, H, k["guide_spp"], seed=k["seed"], sample_offset=off)
        mean = h.advance(cam, img, *((g["normal"], g["position"], g["coverage"]) if moved else (None, None, None)))
        est = go.estimate_variance(img, g, h.n)
        var = h.variance(est)
        filtered, v = go.run_guided(mean, var, g)
        out.append(dict(frame=img, mean=mean, length=h.n.copy(), q=h.q.copy(), estimate=est, variance=var, out=filtered, v=v, kept=h.kept))
    return out


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    import guides_oracle
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


def test_end_to_end_chain_of_the_oracles_reaches_both_branches(sio, oracle_mod, glib):
    sc, W, H, cams, k = chain_inputs(sio)
    assert [a.tobytes() == b.tobytes() for a, b in zip(cams, cams[1:])] == [True, False, False, False, False]
    last = cpu_chain(sio, oracle_mod, glib)[-1]
    n = last["length"]
    print("last frame: %d pixels with n >= 4, %d below, longest %g" % ((n >= 4).sum(), (n < 4).sum(), n.max()))
    assert (n >= 4).sum() > 100 and (n < 4).sum() > 100
    assert last["variance"][n >= 4].tobytes() != last["estimate"][n >= 4].tobytes()
    assert last["variance"][n < 4].tobytes() == last["estimate"][n < 4].tobytes()
    assert np.isfinite(last["out"]).all() and last["out"].tobytes() != last["mean"].tobytes()
