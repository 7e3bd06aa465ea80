"""Case table of the denoiser coverage suite: images, guides and parameters at which k_denoise_pack, k_denoise_pack_color and
k_atrous (csrc/denoise_kernels.hip) and the level loop of csrc/denoise.cpp can go wrong and the tests of test_gpu_denoise.py
do not look.  A plain module: no GPU, no tests.

  deep levels   257 x 9 and 9 x 257 at 8 levels, 129 x 6 at 7, 70 x 65 at 6, with parameters under which the taps of strides
                32, 64 and 128 take part: every term off (a plain B3 pyramid), or sigma_color = 64 with the default normal and
                position terms on guides smooth enough to pass them (smooth_guides)
  level counts  1 .. 8 on one ragged image, demodulated and not.  The image is 133 x 19, not 67 x 35: a stride of 128 reaches
                nobody on a 67 wide image, so 7 and 8 levels would give one image there
  shapes        1 x 300, 300 x 1, 64 x 4, 65 x 5, 63 x 3, 128 x 8 and 2 x 2 at the default parameters (one pixel wide or high,
                the 64 x 4 workgroup tile met exactly, one short of it and one past it)
  values        albedo 0, negative, -0, denormal, exactly 1e-3f and its two float neighbours; coverage fractional, denormal,
                -0 and negative; zero-length normals; positions around 1e6 (the float grid is 1/16 there, so millimetres
                collapse onto it); colours 0, denormal and 1e30 among ordinary ones with the colour term on and off (a
                squared difference overflows to inf and must weigh 0); a falloff argument of exactly 8.0f and one a float
                above it.  make(False) gives the same case with the hostile value replaced by an ordinary one
  sigmas        1e-17, 1e-18, 1e-20, 1e-30 and the smallest denormal (the inverse square overflows: the clamp to FLT_MAX),
                1e19 (inverse denormal), 1e20 and 3e38 (s * s overflows: inverse 0), in each of the three terms, at 1 and at
                8 levels.  The colours lie on a grid of 2^-10 in (0, 4): c * 9/64 is then exact, so a pixel whose every
                other tap weighs 0 keeps its bits (fl(fl(c * 9/64) / (9/64)) is not c for every float, include/hpt.h)

Every case is `Case(name, make)`; make() returns (image [H, W, 3] f32, guides dict, kw) where kw are keywords both of
denoise_oracle.run and of path_tracing_amd.make_denoise_params.  VALUES' make takes `hostile` (default True); SIGMAS are
`SigmaCase(name, make, term, small)`.

Observed on the CPU oracle (tests/denoise_oracle.cpp).  Deep levels: valid pixels that level 1, 2, ... changes, of the valid:
  deep-257x9-off           2313 2313 2313 2313 2313 2313 2313 2313  of 2313
  deep-9x257-smooth        2313 2313 2313 2313 2313 2313 2313 2313  of 2313
  deep-129x6-smooth-demod   710  710  710  710  709  708  653       of  710
  deep-70x65-smooth        4089 4089 4089 4089 4089 4085            of 4089
Level counts (133 x 19, 2445 valid pixels): pixels in which n + 1 levels differ from n, n = 1 .. 7:
  demodulated  2445 2442 2442 2442 2440 2374 176       not  2445 2445 2445 2445 2443 2378 176
  (the eighth level's stride of 128 reaches from the first and the last five columns only)
Values: valid pixels changed (all finite) / valid; pixels in which the image differs from the ordinary case's:
  albedo-edge          1920 / 1920   1920
  coverage-edge        1564 / 1714   1334
  normal-zero          1895 / 1920   1888
  position-far         1891 / 1920   1876
  colour-extreme-on    1658 / 1920   1548
  colour-extreme-off   1920 / 1920   1920
  falloff-exact-8      1920 / 1920   1542
Sigmas (40 x 20): every output finite; up to the smallest denormal's the output is the input, bit for bit; from 1e19 up it
is the image of the run with the term off, which changes all 800 pixels.  On the arithmetic before the clamp
(inv = 1 / (s * s) alone) 20 of the 30 small cases came out NaN: sigma_color = 1e-18 at 8 levels and every term from 1e-20 down
at 1 and at 8 levels (tests/test_denoise_cases_cpu.py fails there).
"""
import collections

import numpy as np

import denoise_oracle

Case = collections.namedtuple("Case", "name make")
SigmaCase = collections.namedtuple("SigmaCase", "name make term small")

F = np.float32
DENORM_MIN = float(np.finfo(np.float32).smallest_subnormal)
ALBEDO_CLAMP = F(1e-3)                 # k_denoise_pack, include/hpt.h: a(p) = max(albedo[p], 1e-3f)


def noisy(rng, W, H):
    """Smooth ramps plus noise at the scale of the default colour sigma and a few fireflies."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.5 + 0.01 * xx, 0.8 - 0.005 * yy, 0.3 + 0.002 * (xx + yy)], -1) + rng.normal(scale=0.3, size=(H, W, 3))
    img = np.abs(img).astype(np.float32)
    img[rng.uniform(size=(H, W)) < 0.02] *= F(20)
    return img


def grid_noise(rng, W, H):
    """Independent colours k / 1024, k = 1 .. 4095: 12 significant bits, so c * 9/64 and the division back are exact."""
    return (rng.integers(1, 4096, size=(H, W, 3)).astype(np.float32) / F(1024)).astype(np.float32)


def smooth_guides(rng, W, H, invalid=None):
    """A gently curved sheet: unit normals turning by 0.001 per pixel, positions 1 mm apart with a shallow bowl, albedo
    ramps, coverage 1 .. 4.  At the default sigmas a tap 256 pixels away still weighs more than a tenth."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    n = np.stack([0.001 * (xx - W / 2), 0.0015 * (yy - H / 2), np.ones_like(xx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    position = np.stack([0.001 * xx, 0.001 * yy, 1e-6 * ((xx - W / 2) ** 2 + (yy - H / 2) ** 2)], -1)
    albedo = np.stack([0.2 + 0.6 * xx / W, 0.9 - 0.5 * yy / H, 0.3 + 0.2 * (xx + yy) / (W + H)], -1)
    albedo = albedo * rng.uniform(0.9, 1.1, size=(H, W, 3))
    g = dict(albedo=albedo.astype(np.float32), normal=np.ascontiguousarray(n.astype(np.float32)),
             position=position.astype(np.float32), coverage=rng.integers(1, 5, size=(H, W)).astype(np.float32))
    if invalid is not None:
        for k in g:
            g[k][invalid] = 0
    return g


# ---- deep levels ----------------------------------------------------------------------------------------------------
def _deep_off():
    rng = np.random.default_rng(201)
    W, H = 257, 9
    return noisy(rng, W, H), denoise_oracle.random_guides(rng, W, H), \
        dict(iterations=8, sigma_color=-1.0, sigma_normal=-1.0, sigma_position=-1.0, demodulate=False)


def _deep_smooth(W, H, levels, seed, demod, holes):
    def make():
        rng = np.random.default_rng(seed)
        invalid = rng.uniform(size=(H, W)) < holes if holes else None
        return noisy(rng, W, H), smooth_guides(rng, W, H, invalid), dict(iterations=levels, sigma_color=64.0, demodulate=demod)
    return make


DEEP = [
    Case("deep-257x9-off", _deep_off),
    Case("deep-9x257-smooth", _deep_smooth(9, 257, 8, 202, False, 0.0)),
    Case("deep-129x6-smooth-demod", _deep_smooth(129, 6, 7, 203, True, 0.07)),
    Case("deep-70x65-smooth", _deep_smooth(70, 65, 6, 204, False, 0.1)),
]

# ---- level counts ---------------------------------------------------------------------------------------------------
LEVEL_W, LEVEL_H = 133, 19


def _levels(n, demod):
    def make():
        rng = np.random.default_rng(210)                   # one image for all sixteen
        invalid = rng.uniform(size=(LEVEL_H, LEVEL_W)) < 0.03
        g = smooth_guides(rng, LEVEL_W, LEVEL_H, invalid)
        return noisy(rng, LEVEL_W, LEVEL_H), g, dict(iterations=n, sigma_color=64.0, demodulate=demod)
    return make


LEVELS = [Case("levels-%d-%s" % (n, "demod" if demod else "plain"), _levels(n, demod)) for demod in (True, False) for n in range(1, 9)]

# ---- shapes at the default parameters -------------------------------------------------------------------------------
SHAPE_SIZES = [(1, 300), (300, 1), (64, 4), (65, 5), (63, 3), (128, 8), (2, 2)]


def _shape(W, H):
    def make():
        rng = np.random.default_rng(220 + W + H)
        invalid = rng.uniform(size=(H, W)) < 0.05
        invalid[0, 0] = False
        return noisy(rng, W, H), denoise_oracle.random_guides(rng, W, H, invalid=invalid), dict(demodulate=(W + H) % 2 == 1)
    return make


SHAPES = [Case("shape-%dx%d" % (W, H), _shape(W, H)) for W, H in SHAPE_SIZES]

# ---- values ---------------------------------------------------------------------------------------------------------
VAL_W, VAL_H = 48, 40


def _base(seed):
    rng = np.random.default_rng(seed)
    g = denoise_oracle.random_guides(rng, VAL_W, VAL_H)
    img = noisy(rng, VAL_W, VAL_H)
    mask = rng.uniform(size=(VAL_H, VAL_W)) < 0.25
    return rng, img, g, mask


def _cycle(values, count):
    return np.asarray([values[k % len(values)] for k in range(count)], np.float32)


def _albedo_edge(hostile=True):
    rng, img, g, mask = _base(230)
    up, down = np.nextafter(ALBEDO_CLAMP, F(1)), np.nextafter(ALBEDO_CLAMP, F(0))
    vals = [0.0, -0.5, ALBEDO_CLAMP, down, up, -0.0, 1e-40, -1e30]
    n = int(mask.sum())
    g["albedo"][mask] = np.stack([_cycle(vals, n), _cycle(vals[3:] + vals[:3], n), _cycle(vals[5:] + vals[:5], n)], -1) if hostile else F(0.5)
    return img, g, dict(iterations=3, sigma_color=-1.0, demodulate=True)        # colour off: the 1000-fold pixels mix


def _coverage_edge(hostile=True):
    rng, img, g, mask = _base(231)
    vals = [0.25, 1e-40, -0.0, -1.0, 2.5, DENORM_MIN, 0.0, -1e-40, 0.999]
    g["coverage"][mask] = _cycle(vals, int(mask.sum())) if hostile else F(1)
    return img, g, dict(iterations=3, demodulate=True)


def _normal_zero(hostile=True):
    rng, img, g, mask = _base(232)
    if hostile:
        g["normal"][mask] = 0
    return img, g, dict(iterations=3, sigma_color=4.0, demodulate=False)


def _position_far(hostile=True):
    rng, img, g, mask = _base(233)
    yy, xx = np.mgrid[0:VAL_H, 0:VAL_W].astype(np.float64)
    pos = np.stack([0.004 * xx, 0.004 * yy, 0.02 * rng.normal(size=(VAL_H, VAL_W))], -1)         # millimetres
    g["position"] = ((pos + 1e6) if hostile else pos).astype(np.float32)
    return img, g, dict(iterations=3, sigma_color=4.0, sigma_normal=2.0, demodulate=True)


def _colour_extreme(colour_on):
    def make(hostile=True):
        rng, img, g, mask = _base(234)
        n = int(mask.sum())
        if hostile:
            img[mask] = np.stack([_cycle([0.0, 1e-40, 1e30, 1e30, 0.3], n), _cycle([0.0, 1e-40, 1e30, 0.0, 1e30], n),
                                  _cycle([0.0, DENORM_MIN, 1e30, 1e-40, 0.0], n)], -1)
        else:
            img[mask] = F(0.5)
        return img, g, dict(iterations=3, sigma_color=0.0 if colour_on else -1.0, sigma_normal=2.0, demodulate=True)
    return make


def _falloff_exact_8(hostile=True):
    """sigma_normal = 1: (1, 1, 0) against (-1, -1, 0) differ by (2, 2, 0), argument exactly 8.0f, weight exactly 0; the
    third band's (-1, -1, 1e-3) gives (2, 2, -1e-3) against the first, one float above 8, and mixes with the second."""
    rng, img, g, mask = _base(235)
    third = VAL_W // 3
    g["normal"][...] = (1, 1, 0)
    if hostile:
        g["normal"][:, third: 2 * third] = (-1, -1, 0)
        g["normal"][:, 2 * third:] = (-1, -1, 1e-3)
    return img, g, dict(iterations=3, sigma_color=-1.0, sigma_normal=1.0, sigma_position=-1.0, demodulate=False)


VALUES = [
    Case("albedo-edge", _albedo_edge),
    Case("coverage-edge", _coverage_edge),
    Case("normal-zero", _normal_zero),
    Case("position-far", _position_far),
    Case("colour-extreme-on", _colour_extreme(True)),
    Case("colour-extreme-off", _colour_extreme(False)),
    Case("falloff-exact-8", _falloff_exact_8),
]

# ---- sigmas ---------------------------------------------------------------------------------------------------------
SIGMA_W, SIGMA_H = 40, 20
SMALL_SIGMAS = [("1e-17", 1e-17), ("1e-18", 1e-18), ("1e-20", 1e-20), ("1e-30", 1e-30), ("denorm", DENORM_MIN)]
LARGE_SIGMAS = [("1e19", 1e19), ("1e20", 1e20), ("3e38", 3e38)]
TERMS = ("sigma_color", "sigma_normal", "sigma_position")


def _sigma(term, value, levels):
    def make():
        rng = np.random.default_rng(240)                   # one image and one set of guides for all of them
        g = denoise_oracle.random_guides(rng, SIGMA_W, SIGMA_H)
        return grid_noise(rng, SIGMA_W, SIGMA_H), g, {"iterations": levels, term: value, "demodulate": False}
    return make


SIGMAS = [SigmaCase("%s-%s-n%d" % (term, tag, levels), _sigma(term, value, levels), term, small)
          for term in TERMS for small, table in ((True, SMALL_SIGMAS), (False, LARGE_SIGMAS)) for tag, value in table for levels in (1, 8)]

ALL = DEEP + LEVELS + SHAPES + VALUES + [Case(c.name, c.make) for c in SIGMAS]
# run through hpt_denoise_host as well (the one-pixel-wide and one-pixel-high images and every sigma case among them)
HOST = [c for c in ALL if c.name in ("shape-1x300", "shape-300x1", "shape-2x2", "deep-257x9-off", "levels-1-demod", "levels-8-plain",
                                     "albedo-edge", "coverage-edge") or c.name.startswith("sigma_")]
