"""CPU tests of the denoiser's definition (include/hpt.h, "guides and denoiser") on its oracle (tests/denoise_oracle.cpp),
which the GPU tests compare the kernels with byte for byte: edges that stop the filter exactly, a constant kept,
invalid pixels, strides beyond the image, and noise reduced on a flat wall."""
import numpy as np
import pytest

import denoise_oracle


@pytest.fixture(scope="module")
def dlib(tmp_path_factory):
    return denoise_oracle.build(tmp_path_factory.mktemp("denoise_oracle"))


def flat_guides(W, H, normal=(0, 0, 1)):
    """A wall in the plane z = 0, 1 cm per pixel."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return dict(albedo=np.full((H, W, 3), 0.5, np.float32), normal=np.tile(np.asarray(normal, np.float32), (H, W, 1)),
                position=np.stack([xx * np.float32(0.01), yy * np.float32(0.01), np.zeros((H, W), np.float32)], -1),
                coverage=np.ones((H, W), np.float32))


def test_a_normal_edge_is_exact(dlib):
    W, H = 24, 16
    rng = np.random.default_rng(1)
    g = flat_guides(W, H)
    g["normal"][:, : W // 2] = (1, 0, 0)
    g["normal"][:, W // 2:] = (0, 1, 0)                    # |dn|^2 = 2: xn = 8 at sigma_normal = 0.5, e = 0 exactly
    g["position"][...] = 0                                 # position term sees one point: no edge of its own
    a = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    b = a.copy()
    b[:, W // 2:] = rng.uniform(0, 50, (H, W - W // 2, 3)).astype(np.float32)
    for demod in (False, True):
        oa = denoise_oracle.run(dlib, a, g, iterations=4, demodulate=demod)
        ob = denoise_oracle.run(dlib, b, g, iterations=4, demodulate=demod)
        assert oa[:, : W // 2].tobytes() == ob[:, : W // 2].tobytes()
        assert oa[:, W // 2:].tobytes() != ob[:, W // 2:].tobytes()
        assert not np.array_equal(oa, a)                   # and the filter did something


def test_a_depth_step_between_parallel_planes_is_exact(dlib):
    W, H = 24, 16
    rng = np.random.default_rng(2)
    g = flat_guides(W, H)
    g["position"][:, W // 2:, 2] = 0.5                     # t = 0.5: xp = 0.25 / 0.0025 = 100 >= 8 at the default sigma_position
    a = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    b = a.copy()
    b[:, W // 2:] = rng.uniform(0, 50, (H, W - W // 2, 3)).astype(np.float32)
    oa = denoise_oracle.run(dlib, a, g, iterations=4)
    ob = denoise_oracle.run(dlib, b, g, iterations=4)
    assert oa[:, : W // 2].tobytes() == ob[:, : W // 2].tobytes()
    assert oa[:, W // 2:].tobytes() != ob[:, W // 2:].tobytes()


@pytest.mark.parametrize("demod", [False, True])
def test_a_constant_is_kept(dlib, demod):
    W, H, n = 37, 29, 5
    rng = np.random.default_rng(3)
    g = denoise_oracle.random_guides(rng, W, H)
    const = np.asarray((0.7312, 1.9, 0.043), np.float32)
    if demod:
        # constant in the space the filter works in: colour = const * a(p), so c_0 = const up to the divide's half ulp
        img = (const * np.maximum(g["albedo"], np.float32(1e-3))).astype(np.float32)
    else:
        img = np.tile(const, (H, W, 1))
    out, levels = denoise_oracle.run(dlib, img, g, iterations=n, demodulate=demod, want_levels=True)
    # per level 25 products, 24 adds and one divide, each at most half an ulp: under 27 * 2^-24 = 1.6e-6 < 4e-6
    for k in range(1, n + 1):
        rel = np.abs(levels[k].astype(np.float64) - levels[k - 1]) / np.abs(levels[k - 1])
        assert rel.max() <= 4e-6, (k, rel.max())
    if not demod:
        assert (np.abs(out.astype(np.float64) - const) / const).max() <= 4e-6 * n


def test_invalid_pixels_pass_through_and_feed_nobody(dlib):
    W, H = 20, 14
    rng = np.random.default_rng(4)
    invalid = rng.uniform(size=(H, W)) < 0.3
    g = denoise_oracle.random_guides(rng, W, H, invalid=invalid)
    a = rng.uniform(0, 3, (H, W, 3)).astype(np.float32)
    b = a.copy()
    b[invalid] = rng.uniform(10, 99, (int(invalid.sum()), 3)).astype(np.float32)
    for demod in (False, True):
        oa = denoise_oracle.run(dlib, a, g, iterations=3, demodulate=demod)
        ob = denoise_oracle.run(dlib, b, g, iterations=3, demodulate=demod)
        assert oa[invalid].tobytes() == a[invalid].tobytes() and ob[invalid].tobytes() == b[invalid].tobytes()
        assert oa[~invalid].tobytes() == ob[~invalid].tobytes()
        assert not np.array_equal(oa[~invalid], a[~invalid])


def test_strides_beyond_the_image(dlib):
    W, H = 3, 2
    rng = np.random.default_rng(5)
    g = denoise_oracle.random_guides(rng, W, H)
    img = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    out, levels = denoise_oracle.run(dlib, img, g, iterations=8, demodulate=False, want_levels=True)
    assert levels[0].tobytes() == img.tobytes()
    # from level 2 on (stride 4 > W - 1) only the centre tap is inside, and a pixel whose other taps are all skipped
    # keeps its value by definition (c * w / w would not): the level hands its input on unchanged
    for k in range(2, 8):
        assert levels[k + 1].tobytes() == levels[k].tobytes(), k
    assert levels[1].tobytes() != levels[0].tobytes()
    assert out.tobytes() == levels[8].tobytes()


def test_noise_falls_on_a_flat_wall(dlib):
    W, H = 48, 40
    rng = np.random.default_rng(6)
    g = flat_guides(W, H)
    img = (1.0 + rng.normal(scale=0.2, size=(H, W, 3))).astype(np.float32)
    out = denoise_oracle.run(dlib, img, g, iterations=1, sigma_color=-1.0, demodulate=False)
    # with the colour term off every interior pixel is the plain 5 x 5 B3 average: variance falls by the sum of the
    # squared weights, (70/256)^2 = 0.0748 for iid noise
    inner = (slice(2, H - 2), slice(2, W - 2))
    assert out[inner].var() < img[inner].var()


def test_cli_help_lists_the_denoise_flags():
    import os
    import subprocess
    from conftest import ROOT
    cli = os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_cli")
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--denoise ", "--guide-spp", "--denoise-iterations", "--sigma-color", "--sigma-normal", "--sigma-position"):
        assert flag in out.stdout, flag
