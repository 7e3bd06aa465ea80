"""CPU tests of the variance-guided filter (include/hpt.h, "variance-guided filtering"): what the numpy oracle the device
is held to is worth -- the scenario the filter exists for, the variance it hands on, the spatial estimate, the cases in
which nothing may change -- the presence of the calls in the header and in Python, and the refusals the host makes before
it touches a device (hpt_guided_check needs neither a device nor a handle)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_cases as dc
import denoise_oracle
import guided_cases as gc
import guided_oracle as go
from conftest import ROOT, rmse

HPT_ERR_INVALID = 1
f32 = np.float32


@pytest.fixture(scope="module")
def dlib(tmp_path_factory):
    return denoise_oracle.build(tmp_path_factory.mktemp("denoise_oracle"))


@pytest.fixture(scope="module")
def scenario():
    return gc.checker(seed=5)


def _halves(s, img):
    return rmse(img[s["left"]], s["truth"][s["left"]]), rmse(img[s["right"]], s["truth"][s["right"]])


def test_guided_filter_serves_converged_and_restarted_pixels_at_once(scenario, dlib):
    """The checker of guided_cases.py: RMSE against the truth, 4 pixels away from the seam, converged | restarted half.
    Observed on the oracle:   input 0.0192 | 0.1498;   guided, true variance 0.0039 | 0.0451;   guided, estimated variance
    0.0024 | 0.0454;   fixed sigma 1.0: 0.1152 | 0.1156 (the checker is blurred away), 0.3: 0.0020 | 0.0951, 0.1: 0.0010 | 0.1485."""
    s = scenario
    e_in = _halves(s, s["mean"])
    true_var, _ = go.run_guided(s["mean"], s["variance"], s["guides"])
    estimate = go.estimate_variance(s["frame"], s["guides"], s["length"])
    est_var, _ = go.run_guided(s["mean"], estimate, s["guides"])
    fixed = {sg: _halves(s, denoise_oracle.run(dlib, s["mean"], s["guides"], sigma_color=sg)) for sg in (1.0, 0.3, 0.1)}
    print("input %.4f | %.4f" % e_in)
    for name, img in (("true variance", true_var), ("estimated variance", est_var)):
        e = _halves(s, img)
        print("guided, %s %.4f | %.4f" % ((name,) + e))
        assert e[0] < e_in[0] and e[1] < e_in[1], name
        for sg, ef in fixed.items():
            assert e[1] < ef[1], (name, sg)
    for sg, ef in fixed.items():
        print("fixed sigma %.1f %.4f | %.4f" % ((sg,) + ef))


def test_variance_after_one_level_of_plain_b3_weights():
    """Colour term off on one plane: every weight is h[j] h[i], so v_1 = v_0 * sum w^2 / (sum w)^2 = v_0 * (70/256)^2 at
    pixels whose 25 taps lie inside the image.  25 products and sums of exact constants: relative 4e-6."""
    W, H = 40, 24
    rng = np.random.default_rng(11)
    img = (0.5 + rng.normal(0.0, 0.15, (H, W, 3))).astype(f32)
    var = np.full((H, W, 3), f32(0.0225), f32)
    _, v1, levels = go.run_guided(img, var, gc.plane_guides(W, H), iterations=1, sigma_color=-1.0, want_levels=True)
    v0 = levels[0][1]
    assert v0.tobytes() == np.full((H, W), (f32(0.0225) + f32(0.0225)) + f32(0.0225), f32).tobytes()
    ratio = v1[2:-2, 2:-2].astype(np.float64) / v0[2:-2, 2:-2]
    print("v_1 / v_0 in the interior: %.7f .. %.7f, (70/256)^2 = %.7f" % (ratio.min(), ratio.max(), (70.0 / 256.0) ** 2))
    assert np.abs(ratio / (70.0 / 256.0) ** 2 - 1).max() <= 4e-6
    assert (v1[0, 0] > v1[2, 2])                    # a corner averages 9 taps, not 25
    # the colour of that level is the plain filter's with every term off
    c1 = levels[1][0]
    assert np.abs(c1[2:-2, 2:-2].astype(np.float64).std() / 0.15 - 70.0 / 256.0) < 0.03


def test_spatial_estimate_finds_the_noise_inside_a_block(scenario):
    """One frame at noise 0.15: over the 576 values whose 7 x 7 window lies inside one block the median of estimate / 0.0225
    is 0.973 on the oracle (the weighted estimate is biased low by 1/49; the median of 576 estimates of 48 degrees of freedom
    has a relative sigma of about 0.01)."""
    s = scenario
    est = go.estimate_variance(s["frame"], s["guides"])
    inside = gc.inside_one_block()
    values = est[inside] / 0.0225
    assert values.size == 576
    med = float(np.median(values))
    print("median of estimate / 0.0225 over %d values: %.4f" % (values.size, med))
    assert 0.9 <= med <= 1.1
    # the length divides: the variance of the mean
    with_len = go.estimate_variance(s["frame"], s["guides"], s["length"])
    assert with_len[:, :32].tobytes() == (est[:, :32] / f32(64)).astype(f32).tobytes() and with_len[:, 32:].tobytes() == est[:, 32:].tobytes()
    # a window across a block edge counts the edge as noise: (0.3 / 2)^2 on top
    assert np.median(est[~inside]) > 1.3 * 0.0225


def test_zero_variance_passes_the_image_through():
    """inv_c = 1e12: another tap takes part only where its colour is (almost) the pixel's own.  On colours k / 1024 apart the
    centre stands alone and fl(fl(c * 9/64) / (9/64)) = c exactly (12 significant bits, denoise_cases.grid_noise)."""
    W, H = 33, 9
    rng = np.random.default_rng(12)
    g = gc.plane_guides(W, H)
    zero = np.zeros((H, W, 3), f32)
    grid = dc.grid_noise(rng, W, H)
    out, v = go.run_guided(grid, zero, g, demodulate=False)
    assert out.tobytes() == grid.tobytes() and not v.any()
    img = dc.noisy(rng, W, H)
    out, v = go.run_guided(img, zero, g, demodulate=False)
    assert np.abs(out / img - 1).max() <= 2.0 ** -22 and not v.any()        # two roundings per level at the most, not a blur
    out8, _ = go.run_guided(img, np.full((H, W, 3), f32(0.03), f32), g, demodulate=False)
    assert np.abs(out8 / img - 1).max() > 0.01                              # with a variance the same image is filtered


def test_levels_whose_stride_exceeds_the_image_hand_their_input_on():
    W, H = 3, 2
    img, g, var, _ = gc.inputs(gc.SHAPES[1])
    g = dict(g, coverage=np.ones((H, W), f32))
    kw = dict(sigma_normal=4.0, sigma_position=1.0)
    _, _, levels = go.run_guided(img, var, g, iterations=8, want_levels=True, **kw)
    assert levels[0][0].tobytes() != levels[1][0].tobytes() != levels[2][0].tobytes()      # strides 1 and 2 reach a neighbour
    for k in range(2, 8):                           # strides 4 .. 128 reach nobody in a 3 x 2 image
        assert levels[k + 1][0].tobytes() == levels[k][0].tobytes() and levels[k + 1][1].tobytes() == levels[k][1].tobytes(), k
    one = np.array([[[0.3, 0.7, 1.1]]], f32)
    g1 = {k: v[:1, :1] for k, v in g.items()}
    v1 = np.array([[[0.01, 0.02, 0.03]]], f32)
    out, v = go.run_guided(one, v1, g1, iterations=8, demodulate=False)
    assert out.tobytes() == one.tobytes() and v.tobytes() == ((v1[..., 0] + v1[..., 1]) + v1[..., 2]).tobytes()


def test_invalid_pixels_leave_with_their_input_bits_and_variance():
    shape = gc.SHAPES[4]
    img, g, var, length = gc.inputs(shape, hostile=True)
    invalid = ~(g["coverage"] > 0)
    assert 300 < invalid.sum() < 1000
    for demod in (True, False):
        out, v = go.run_guided(img, var, g, demodulate=demod)
        assert out[invalid].tobytes() == img[invalid].tobytes()
        want = np.fmax((var[..., 0] + var[..., 1]) + var[..., 2], f32(0))
        assert v[invalid].tobytes() == want[invalid].tobytes()
        assert np.isfinite(out).all() and np.isfinite(v).all() and (v >= 0).all()
        assert (out[~invalid] != img[~invalid]).any(-1).mean() > 0.9
    est = go.estimate_variance(img, g, length)
    assert not est[invalid].any() and (est[~invalid] > 0).all() and np.isfinite(est).all()


def test_case_table_is_sane():
    assert [(s.W, s.H, s.iterations) for s in gc.SHAPES] == [(1, 1, 0), (3, 2, 8), (65, 5, 0), (131, 2, 8), (96, 64, 0)]
    assert len(gc.SWITCHES) == 16 and len({tuple(sorted(s.items())) for s in gc.SWITCHES}) == 16
    for shape in gc.SHAPES:
        img, g, var, length = gc.inputs(shape, hostile=True)
        again = gc.inputs(shape, hostile=True)
        assert img.tobytes() == again[0].tobytes() and var.tobytes() == again[2].tobytes() and length.tobytes() == again[3].tobytes()
        assert img.shape == (shape.H, shape.W, 3) and var.shape == img.shape and length.shape == (shape.H, shape.W)
        if shape.W * shape.H >= 24:
            assert np.isnan(var).any() and (var < 0).any() and (var == 0).any() and (var == f32(1e30)).any()
            assert all((length == x).any() for x in (0.0, 0.5, 300.0))
    # 131 x 2 at 8 levels: the stride of 128 takes part (7 levels give another image), and the switches matter
    shape = gc.SHAPES[3]
    img, g, var, _ = gc.inputs(shape)
    kws = gc.switches_for(shape)
    seven = go.run_guided(img, var, g, **dict(kws[0], iterations=7))[0]
    outs = [go.run_guided(img, var, g, **kw)[0].tobytes() for kw in kws]
    assert seven.tobytes() != outs[0] and len(set(outs)) == 16


# ---- the boundary -------------------------------------------------------------------------------------------------------

DECLARED = ["hpt_denoiser_run_guided", "hpt_denoiser_estimate_variance", "hpt_history_length", "hpt_guided_check"]


def test_header_declares_the_calls_and_python_has_the_front_end(hpt):
    text = open(os.path.join(ROOT, "include", "hpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hpt.load_library()
    for name in DECLARED:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    for field in ("iterations", "sigma_color", "sigma_normal", "sigma_position", "flags"):
        assert re.search(r"\b%s\s*;" % field, code[code.index("typedef struct hpt_guided_params"):]), field
    for word in ("NOT halved", "WORKING SPACE", "SINGLE NEW FRAME", "biased low", "no sqrt", "NOT a general-purpose variance"):
        assert word in text, word
    assert C.sizeof(hpt.GuidedParams) == 20
    for m in ("run_guided", "estimate_variance"):
        assert hasattr(hpt.Denoiser, m), m
    assert hasattr(hpt.History, "length") and callable(hpt.guided_check) and callable(hpt.make_guided_params)
    p = hpt.make_guided_params(iterations=3, sigma_color=1.5, demodulate=False, time=True)
    assert (p.iterations, p.sigma_color, p.flags) == (3, 1.5, hpt.DENOISE_TIME)


def _refused(lib, rc, *words):
    assert rc == HPT_ERR_INVALID, (rc, lib.hpt_last_error())
    msg = lib.hpt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_refusals_before_the_device_is_touched(hpt):
    """No device is needed (and none is there under -m "not gpu").  hpt_guided_check is the list of checks a guided run
    makes, callable without a denoiser; the two refusals that need a live object (a run before set_guides,
    hpt_history_length before the first advance) are in tests/test_gpu_guided.py."""
    lib = hpt.load_library()
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    W, H = 5, 3
    n3, n1 = W * H * 3 * 4, W * H * 4
    vp = lambda off: C.c_void_p(base + off)
    rgb, var, out, vout = vp(0), vp(n3), vp(2 * n3), vp(3 * n3)
    P = hpt.make_guided_params

    def check(a=rgb, v=var, o=out, vo=vout, p=None, W=W, H=H):
        return lib.hpt_guided_check(W, H, a, v, o, vo, C.byref(p) if p is not None else None)

    assert check() == 0, lib.hpt_last_error()
    assert check(vo=None) == 0 and check(vo=vp(3 * n3 + n1)) == 0
    for p in (P(), P(iterations=1), P(iterations=8), P(sigma_color=-1), P(sigma_color=1e30), P(sigma_normal=-1, sigma_position=-1),
              P(demodulate=False, time=True)):
        assert check(p=p) == 0, lib.hpt_last_error()
    for kw in (dict(W=0), dict(H=0), dict(W=-3)):
        _refused(lib, check(**kw), b"positive")
    _refused(lib, check(W=1 << 15, H=1 << 14), b"too large")
    _refused(lib, check(a=None), b"null image")
    _refused(lib, check(o=None), b"null image")
    _refused(lib, check(v=None), b"null variance")
    # d_out against either input: the same image, one float inside at either end
    for kw in (dict(o=rgb), dict(o=var), dict(o=vp(4)), dict(o=vp(n3 - 4)), dict(o=vp(2 * n3 - 4)), dict(o=vp(n3 + 4))):
        _refused(lib, check(vo=None, **kw), b"d_out must not overlap")
    # d_variance_out (a third as long) against each of the other three
    for kw in (dict(vo=rgb), dict(vo=vp(n3 - 4)), dict(vo=var), dict(vo=vp(2 * n3 - 4)), dict(vo=out), dict(vo=vp(3 * n3 - 4)),
               dict(vo=vp(2 * n3 - n1 + 4)), dict(vo=vp(3 * n3), o=vp(3 * n3 + n1 - 4))):
        _refused(lib, check(**kw), b"d_variance_out must not overlap")
    assert check(vo=vp(3 * n3), o=vp(3 * n3 + n1)) == 0
    for it in (-1, 9, 100):
        _refused(lib, check(p=P(iterations=it)), b"iterations")
    for flags in (4, 8, 1 << 30, -1):
        bad = P()
        bad.flags = flags
        _refused(lib, check(p=bad), b"flags")
    nan = float("nan")
    for p in (P(sigma_color=nan), P(sigma_normal=nan), P(sigma_position=nan)):
        _refused(lib, check(p=p), b"NaN")
    # null handles
    _refused(lib, lib.hpt_denoiser_run_guided(None, rgb, var, out, vout, None, None), b"null denoiser")
    _refused(lib, lib.hpt_denoiser_estimate_variance(None, rgb, None, out, None, None), b"null denoiser")
    _refused(lib, lib.hpt_history_length(None, vout, None), b"null history")
    with pytest.raises(hpt.HptError, match="hpt error 1:.*iterations"):
        hpt.guided_check(W, H, base, base + n3, base + 2 * n3, None, P(iterations=9))
    hpt.guided_check(W, H, base, base + n3, base + 2 * n3)
