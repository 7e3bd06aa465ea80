"""The denoiser on the MI355X: hpt_denoiser_* and hpt_denoise_host against the oracle (tests/denoise_oracle.cpp) byte for
byte -- ragged sizes, tiny images with strides beyond them, invalid pixels, every term switched off in turn, frames
that share one set of guides, a caller stream shared with hpt_tonemap -- and argument errors as return codes."""
import ctypes as C

import numpy as np
import pytest

import denoise_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlib(tmp_path_factory):
    return denoise_oracle.build(tmp_path_factory.mktemp("denoise_oracle"))


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


def _noisy(rng, W, H):
    """Colours with structure at the scale of the colour sigma: smooth ramps plus noise and a few fireflies."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.5 + 0.01 * xx, 0.8 - 0.005 * yy, 0.3 + 0.002 * (xx + yy)], -1) + rng.normal(scale=0.3, size=(H, W, 3))
    img = np.abs(img).astype(np.float32)
    img[rng.uniform(size=(H, W)) < 0.02] *= np.float32(20)
    return img


def _device_run(hpt, torch, img, g, params, frames=None):
    """The device-pointer path; `frames`: further colour images filtered with the same guides."""
    H, W = img.shape[:2]
    dg = [torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("albedo", "normal", "position", "coverage")]
    outs = []
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for f in [img] + list(frames or []):
            din = torch.from_numpy(np.ascontiguousarray(f)).cuda()
            dout = torch.empty_like(din)
            d.run(din, dout, params)
            torch.cuda.synchronize()
            outs.append(dout.cpu().numpy())
    return outs if frames is not None else outs[0]


def _check_case(hpt, torch, dlib, W, H, seed, invalid=None, **kw):
    rng = np.random.default_rng(seed)
    g = denoise_oracle.random_guides(rng, W, H, invalid=invalid)
    img = _noisy(rng, W, H)
    ref = denoise_oracle.run(dlib, img, g, **kw)
    got = _device_run(hpt, torch, img, g, hpt.make_denoise_params(**kw))
    assert np.isfinite(ref).all() and not np.array_equal(ref, img)
    assert got.tobytes() == ref.tobytes(), float(np.abs(got - ref).max())
    return img, g, ref


@pytest.mark.parametrize("demod", [True, False])
def test_ragged_image_matches_the_oracle(hpt, torch, dlib, demod):
    _check_case(hpt, torch, dlib, 67, 35, 1, iterations=5, demodulate=demod)       # ragged in x and y, two workgroups in x


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (5, 5)])
def test_strides_beyond_tiny_images(hpt, torch, dlib, size):
    W, H = size
    rng = np.random.default_rng(2)
    g = denoise_oracle.random_guides(rng, W, H)
    img = _noisy(rng, W, H)
    ref = denoise_oracle.run(dlib, img, g, iterations=8)
    got = _device_run(hpt, torch, img, g, hpt.make_denoise_params(iterations=8))
    assert got.tobytes() == ref.tobytes()


def test_three_levels_on_several_workgroups(hpt, torch, dlib):
    _check_case(hpt, torch, dlib, 130, 70, 3, iterations=3)


def test_checkerboard_of_invalid_pixels(hpt, torch, dlib):
    yy, xx = np.mgrid[0:64, 0:64]
    invalid = (xx + yy) % 2 == 1
    img, _, ref = _check_case(hpt, torch, dlib, 64, 64, 4, invalid=invalid, iterations=4)
    assert ref[invalid].tobytes() == img[invalid].tobytes()


@pytest.mark.parametrize("off", ["sigma_color", "sigma_normal", "sigma_position"])
def test_each_term_switched_off(hpt, torch, dlib, off):
    _check_case(hpt, torch, dlib, 45, 33, 5, iterations=3, **{off: -1.0})


def test_non_default_sigmas(hpt, torch, dlib):
    _check_case(hpt, torch, dlib, 45, 33, 6, iterations=4, sigma_color=0.37, sigma_normal=0.9, sigma_position=0.013, demodulate=False)


def test_host_call_equals_the_device_path(hpt, torch, dlib):
    rng = np.random.default_rng(7)
    W, H = 50, 41
    g = denoise_oracle.random_guides(rng, W, H, invalid=rng.uniform(size=(H, W)) < 0.1)
    img = _noisy(rng, W, H)
    host = hpt.denoise(img, g, iterations=4)
    dev = _device_run(hpt, torch, img, g, hpt.make_denoise_params(iterations=4))
    assert host.tobytes() == dev.tobytes() == denoise_oracle.run(dlib, img, g, iterations=4).tobytes()


def test_two_frames_on_one_set_of_guides(hpt, torch, dlib):
    rng = np.random.default_rng(8)
    W, H = 70, 20
    g = denoise_oracle.random_guides(rng, W, H)
    a, b = _noisy(rng, W, H), _noisy(rng, W, H) * np.float32(3)
    p = hpt.make_denoise_params(iterations=4)
    got = _device_run(hpt, torch, a, g, p, frames=[b, a])
    ra, rb = denoise_oracle.run(dlib, a, g, iterations=4), denoise_oracle.run(dlib, b, g, iterations=4)
    assert got[0].tobytes() == ra.tobytes() and got[1].tobytes() == rb.tobytes() and got[2].tobytes() == ra.tobytes()


def test_run_and_tonemap_on_one_caller_stream(hpt, torch, dlib):
    rng = np.random.default_rng(9)
    W, H = 67, 35
    g = denoise_oracle.random_guides(rng, W, H)
    img = _noisy(rng, W, H) * np.float32(0.5)
    hpt.tonemap(np.zeros((1, 1, 3), np.float32))              # the threshold table is on the device before the stream starts
    dg = [torch.from_numpy(g[k]).cuda() for k in ("albedo", "normal", "position", "coverage")]
    din = torch.from_numpy(img).cuda()
    dout = torch.empty_like(din)
    d8 = torch.zeros(W * H * 3 + 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg, stream=stream.cuda_stream)
        d.run(din, dout, hpt.make_denoise_params(), stream=stream.cuda_stream)
        hpt.tonemap_device(dout, d8, W * H, stream=stream.cuda_stream)
        stream.synchronize()
    ref = denoise_oracle.run(dlib, img, g)
    ref8 = np.zeros((H, W, 3), np.uint8)
    lib = hpt.load_library()
    lib.hpt_tonemap_reference.restype = None
    lib.hpt_tonemap_reference(ref.ctypes.data_as(C.c_void_p), ref8.ctypes.data_as(C.c_void_p), C.c_int64(W * H), 0)
    assert dout.cpu().numpy().tobytes() == ref.tobytes()
    assert d8.cpu().numpy()[: W * H * 3].tobytes() == ref8.tobytes()
    assert len(np.unique(ref8)) > 50


def test_timed_run_reports_its_levels(hpt, torch, dlib):
    rng = np.random.default_rng(10)
    W, H = 64, 16
    g = denoise_oracle.random_guides(rng, W, H)
    img = _noisy(rng, W, H)
    dg = [torch.from_numpy(g[k]).cuda() for k in ("albedo", "normal", "position", "coverage")]
    din = torch.from_numpy(img).cuda()
    dout = torch.empty_like(din)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        d.run(din, dout, hpt.make_denoise_params(iterations=3, time=True))
        ms = d.last_ms()
        assert ms["pack"] > 0 and ms["filter"] > 0 and all(v > 0 for v in ms["levels"][:3]) and ms["levels"][3:] == [0.0] * 5
        assert dout.cpu().numpy().tobytes() == denoise_oracle.run(dlib, img, g, iterations=3).tobytes()
        d.run(din, dout)                                      # an untimed run has no times
        with pytest.raises(hpt.HptError, match="hpt error 1:"):
            d.last_ms()
        torch.cuda.synchronize()


def test_argument_errors_are_return_codes(hpt, torch):
    err = pytest.raises
    for W, H in ((0, 4), (4, 0), (-1, 4), (4, -3)):
        with err(hpt.HptError, match="hpt error 1:"):
            hpt.Denoiser(W, H)
    W, H = 16, 8
    buf = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    other = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    cov = torch.ones(W * H, dtype=torch.float32, device="cuda")
    with hpt.Denoiser(W, H) as d:
        with err(hpt.HptError, match="before hpt_denoiser_set_guides"):
            d.run(buf, other)
        with err(hpt.HptError, match="hpt error 1:"):
            d.set_guides(buf, buf, 0, cov)
        d.set_guides(buf, buf, buf, cov)
        with err(hpt.HptError, match="overlap"):
            d.run(buf, buf)
        with err(hpt.HptError, match="hpt error 1:"):
            d.run(buf, 0)
        bad = hpt.make_denoise_params()
        bad.flags = 4
        with err(hpt.HptError, match="hpt error 1:"):
            d.run(buf, other, bad)
        for it in (9, -1):
            with err(hpt.HptError, match="iterations"):
                d.run(buf, other, hpt.make_denoise_params(iterations=it))
        d.run(buf, other, hpt.make_denoise_params(iterations=8))
        torch.cuda.synchronize()
    g = dict(albedo=np.zeros((H, W, 3), np.float32), normal=np.zeros((H, W, 3), np.float32),
             position=np.zeros((H, W, 3), np.float32), coverage=np.ones((H, W), np.float32))
    with err(hpt.HptError, match="iterations"):
        hpt.denoise(np.zeros((H, W, 3), np.float32), g, iterations=9)
    with err(ValueError):
        hpt.denoise(np.zeros((H, W + 1, 3), np.float32), g)
