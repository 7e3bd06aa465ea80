"""Case table of the variance-guided filter's tests (include/hpt.h, "variance-guided filtering").  A plain module: no GPU, no
tests.

  checker   the scenario the filter exists for: a 64 x 48 image on ONE plane (the guides see nothing of its content) that
            carries a checker of 8-pixel blocks at 0.5 / 0.2; the left half is the mean of 64 frames, the right half of one,
            noise sigma 0.15 per frame, seed 5.
  shapes    the smallest images at which k_guided_pack, k_atrous_guided and k_variance_spatial can go wrong: one pixel;
            3 x 2 at 8 levels (every stride but 1 leaves the image); 65 x 5 (one past the 64 x 4 tile both ways); 131 x 2 at 8
            levels (a stride of 128 reaches from the first and last three columns); 96 x 64 = 32 workgroups on the analytic
            room of history_cases.py with a tenth of the coverage knocked out.
  variance  images with zeros, a NaN, a negative value and 1e30 among ordinary ones.
  lengths   0, 0.5 and 300 among ordinary history lengths.
"""
import collections
import itertools

import numpy as np

import denoise_cases as dc
import denoise_oracle
import history_cases as hc

f32 = np.float32
Shape = collections.namedtuple("Shape", "name W H iterations make")

# ---- the checker ----------------------------------------------------------------------------------------------------
CHECKER_W, CHECKER_H, BLOCK = 64, 48, 8
NOISE = 0.15
N_LEFT = 64
SEAM_MARGIN = 4


def plane_guides(W, H):
    """One plane facing the viewer, albedo 1: every guide term is 1.0 between any two pixels."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    normal = np.zeros((H, W, 3), f32)
    normal[..., 2] = 1
    position = np.stack([xx * f32(0.01), yy * f32(0.01), np.zeros((H, W), f32)], -1).astype(f32)
    return dict(albedo=np.ones((H, W, 3), f32), normal=normal, position=position, coverage=np.ones((H, W), f32))


def checker_truth(W=CHECKER_W, H=CHECKER_H):
    ys, xs = np.mgrid[0:H, 0:W]
    t = np.where(((xs // BLOCK) + (ys // BLOCK)) % 2 == 0, 0.5, 0.2)
    return np.repeat(t[..., None], 3, -1)


def checker(seed=5):
    """dict(truth, frame: the single new frame, mean: the image to filter, length, variance: the true variance of `mean`,
    guides, left, right: the masks the RMSE is taken over)."""
    W, H = CHECKER_W, CHECKER_H
    rng = np.random.default_rng(seed)
    truth = checker_truth()
    frame = (truth + rng.normal(0.0, NOISE, truth.shape)).astype(f32)
    older = (truth + rng.normal(0.0, NOISE / np.sqrt(N_LEFT), truth.shape)).astype(f32)       # the mean of 64 frames
    xs = np.mgrid[0:H, 0:W][1]
    left_half = xs < W // 2
    mean = np.where(left_half[..., None], older, frame).astype(f32)
    length = np.where(left_half, f32(N_LEFT), f32(1)).astype(f32)
    variance = np.repeat((f32(NOISE * NOISE) / length)[..., None], 3, -1).astype(f32)
    return dict(truth=truth, frame=frame, mean=mean, length=length, variance=variance, guides=plane_guides(W, H),
                left=xs < W // 2 - SEAM_MARGIN, right=xs >= W // 2 + SEAM_MARGIN)


def inside_one_block(W=CHECKER_W, H=CHECKER_H):
    """Pixels whose 7 x 7 window lies inside one block of the checker."""
    ys, xs = np.mgrid[0:H, 0:W]
    ok = lambda a: (a % BLOCK >= 3) & (a % BLOCK <= BLOCK - 4)
    return ok(xs) & ok(ys)


# ---- shapes -----------------------------------------------------------------------------------------------------------
def hostile_variance(rng, W, H):
    """Per-channel variances around 0.02 with zeros, a NaN, a negative value and 1e30 placed at random (on an
    image too small for that, in its first pixels)."""
    var = rng.uniform(0.005, 0.05, size=(H, W, 3)).astype(f32)
    flat = var.reshape(-1, 3)
    specials = [(0.0, 0.0, 0.0), (np.nan, 0.01, 0.01), (-0.5, 0.01, 0.01), (1e30, 1e30, 1e30), (0.01, -0.0, 1e30), (-1.0, -1.0, np.nan)]
    if len(flat) >= 4 * len(specials):
        for k, at in enumerate(rng.choice(len(flat), 4 * len(specials), replace=False)):
            flat[at] = specials[k % len(specials)]
    else:
        for k in range(min(len(flat), len(specials))):
            flat[k] = specials[k]
    return var


def lengths(rng, W, H):
    n = rng.integers(1, 65, size=(H, W)).astype(f32)
    flat = n.reshape(-1)
    for k, at in enumerate(rng.choice(len(flat), min(len(flat), 9), replace=False)):
        flat[at] = (0.0, 0.5, 300.0)[k % 3]
    return n


def _random(W, H, seed):
    def make():
        rng = np.random.default_rng(seed)
        invalid = rng.uniform(size=(H, W)) < 0.06
        invalid[0, 0] = False
        g = denoise_oracle.random_guides(rng, W, H, invalid=invalid)
        return dc.noisy(rng, W, H), g, rng
    return make


def _room():
    W, H = 96, 64
    rng = np.random.default_rng(305)
    g = dict(hc.guides(hc.orbit(W, H, 5.0), W, H))
    g["albedo"] = rng.uniform(0.05, 1.0, size=(H, W, 3)).astype(f32)
    hole = rng.uniform(size=(H, W)) < 0.1
    g["coverage"] = np.where(hole, f32(0), g["coverage"]).astype(f32)
    return hc.frame(g, 306), g, rng


def _ordinary_variance(rng, W, H):
    return rng.uniform(0.005, 0.05, size=(H, W, 3)).astype(f32)


SHAPES = [
    Shape("1x1", 1, 1, 0, _random(1, 1, 301)),
    Shape("3x2-n8", 3, 2, 8, _random(3, 2, 302)),
    Shape("65x5", 65, 5, 0, _random(65, 5, 303)),
    Shape("131x2-n8", 131, 2, 8, _random(131, 2, 304)),
    Shape("room-96x64", 96, 64, 0, _room),
]
# DEMODULATE on / off, and each of the three terms on (0.0: its default) or off
SWITCHES = [dict(demodulate=d, sigma_color=c, sigma_normal=n, sigma_position=p)
            for d, c, n, p in itertools.product((True, False), (0.0, -1.0), (0.0, -1.0), (0.0, -1.0))]
# the guides of the random shapes are rough (normals from four directions, a bumpy sheet): wide guide sigmas let taps through
WIDE = dict(sigma_normal=4.0, sigma_position=1.0)


def inputs(shape, hostile=False):
    """(image, guides, variance [H, W, 3], length [H, W]) of a shape, the same at every call."""
    img, g, rng = shape.make()
    var = hostile_variance(rng, shape.W, shape.H) if hostile else _ordinary_variance(rng, shape.W, shape.H)
    return img, g, var, lengths(rng, shape.W, shape.H)


def switches_for(shape):
    """The sixteen parameter sets of a shape: a term that is on takes its default on the room and a wide value elsewhere."""
    out = []
    for s in SWITCHES:
        kw = dict(s, iterations=shape.iterations)
        if not shape.name.startswith("room"):
            for k, wide in WIDE.items():
                if kw[k] == 0.0:
                    kw[k] = wide
        out.append(kw)
    return out
