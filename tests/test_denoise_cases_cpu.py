"""The case table of the denoiser coverage suite (denoise_cases.py) on the CPU oracle alone: the conditions that keep
test_gpu_denoise_coverage.py's byte comparisons from being empty -- deep levels that still move pixels, level counts that
give different images, hostile values that matter and stay finite -- and the definition at sigmas whose inverse square
leaves the float range (include/hpt.h: clamped to FLT_MAX below, 0 above).  The figures are in denoise_cases.py."""
import numpy as np
import pytest

import denoise_cases as dc
import denoise_oracle


@pytest.fixture(scope="module")
def dlib(tmp_path_factory):
    return denoise_oracle.build(tmp_path_factory.mktemp("denoise_oracle"))


def _differ(a, b):
    """[...] bool: pixels whose bits differ in some channel."""
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(-1)


def _ids(cases):
    return [c.name for c in cases]


def test_the_table_is_complete():
    names = _ids(dc.ALL)
    assert len(set(names)) == len(names)
    sizes = {c.name: c.make()[0].shape[:2] for c in dc.DEEP + dc.SHAPES}
    assert [sizes[c.name] for c in dc.DEEP] == [(9, 257), (257, 9), (6, 129), (65, 70)]
    assert [c.make()[2]["iterations"] for c in dc.DEEP] == [8, 8, 7, 6]
    assert [sizes[c.name][::-1] for c in dc.SHAPES] == [(1, 300), (300, 1), (64, 4), (65, 5), (63, 3), (128, 8), (2, 2)]
    assert sorted(c.make()[2]["iterations"] for c in dc.LEVELS) == sorted(list(range(1, 9)) * 2)
    assert len(dc.SIGMAS) == 3 * 8 * 2 and {c.term for c in dc.SIGMAS} == set(dc.TERMS)
    for c in dc.ALL:
        img = c.make()[0]
        assert img.shape[0] <= 300 and img.shape[1] <= 300 and img.shape[0] * img.shape[1] <= 300 * 65, c.name
    assert {"shape-1x300", "shape-300x1"} <= set(_ids(dc.HOST)) and set(_ids(dc.SIGMAS)) <= set(_ids(dc.HOST))


@pytest.mark.parametrize("case", dc.DEEP, ids=_ids(dc.DEEP))
def test_every_deep_level_moves_a_tenth_of_the_pixels(dlib, case):
    img, g, kw = case.make()
    out, levels = denoise_oracle.run(dlib, img, g, want_levels=True, **kw)
    valid = g["coverage"] > 0
    assert np.isfinite(out).all() and kw["iterations"] >= 6
    moved = [int(_differ(levels[k + 1], levels[k])[valid].sum()) for k in range(kw["iterations"])]
    print(case.name, moved, "of", int(valid.sum()))
    assert min(moved) * 10 >= int(valid.sum()), moved
    if case.name == "deep-257x9-off":
        assert moved == [2313] * 8


@pytest.mark.parametrize("demod", [True, False])
def test_consecutive_level_counts_give_different_images(dlib, demod):
    cases = [c for c in dc.LEVELS if c.make()[2]["demodulate"] == demod]
    outs = [denoise_oracle.run(dlib, *c.make()[:2], **c.make()[2]) for c in cases]
    assert [c.make()[2]["iterations"] for c in cases] == list(range(1, 9))
    moved = [int(_differ(outs[k], outs[k + 1]).sum()) for k in range(7)]
    print("levels, demodulated" if demod else "levels", moved)
    assert all(np.isfinite(o).all() for o in outs) and min(moved) > 0, moved


@pytest.mark.parametrize("case", dc.SHAPES, ids=_ids(dc.SHAPES))
def test_shape_cases_are_filtered(dlib, case):
    img, g, kw = case.make()
    out = denoise_oracle.run(dlib, img, g, **kw)
    valid = g["coverage"] > 0
    assert np.isfinite(out).all() and valid.sum() > (~valid).sum()
    assert _differ(out, img)[valid].sum() * 2 >= valid.sum()
    assert out[~valid].tobytes() == img[~valid].tobytes()


@pytest.mark.parametrize("case", dc.VALUES, ids=_ids(dc.VALUES))
def test_hostile_values_matter_and_stay_finite(dlib, case):
    img, g, kw = case.make()
    out = denoise_oracle.run(dlib, img, g, **kw)
    valid = g["coverage"] > 0
    assert np.isfinite(img).all() and all(np.isfinite(g[k]).all() for k in g)      # hostile, but within "inputs are finite"
    assert np.isfinite(out).all()
    moved = int(_differ(out, img)[valid].sum())
    assert moved * 2 >= int(valid.sum()), (moved, int(valid.sum()))
    assert out[~valid].tobytes() == img[~valid].tobytes()
    img2, g2, kw2 = case.make(False)
    assert kw2 == kw
    indifferent = int(_differ(out, denoise_oracle.run(dlib, img2, g2, **kw2)).sum())
    print(case.name, moved, "of", int(valid.sum()), "moved;", indifferent, "differ from the ordinary case")
    assert indifferent * 10 >= img.shape[0] * img.shape[1]


def test_the_value_cases_hold_their_values():
    img, g, _ = dc.VALUES[0].make()
    a = g["albedo"]
    for v in (0.0, dc.ALBEDO_CLAMP, np.nextafter(dc.ALBEDO_CLAMP, np.float32(0)), np.nextafter(dc.ALBEDO_CLAMP, np.float32(1))):
        assert (a == np.float32(v)).any(), v
    assert (a < 0).any() and (np.signbit(a) & (a == 0)).any() and ((a > 0) & (a < 1e-38)).any()
    cov = dc.VALUES[1].make()[1]["coverage"]
    assert ((cov > 0) & (cov < 1e-38)).any() and (np.signbit(cov) & (cov == 0)).any() and (cov < 0).any() and (cov % 1 != 0).any()
    n = dc.VALUES[2].make()[1]["normal"]
    assert ((n == 0).all(-1) & (dc.VALUES[2].make()[1]["coverage"] > 0)).any()
    p = dc.VALUES[3].make()[1]["position"]
    assert p.min() > 999999 and len(np.unique(p)) > 3
    for case in dc.VALUES[4:6]:
        c = case.make()[0]
        assert (c == 0).any() and ((c > 0) & (c < 1e-38)).any() and (c == np.float32(1e30)).any()
        d = np.float32(1e30) - np.float32(0.5)
        with np.errstate(over="ignore"):
            assert np.isinf(d * d)
    nrm, kw = dc.VALUES[6].make()[1]["normal"], dc.VALUES[6].make()[2]
    a, b, c = nrm[0, 0], nrm[0, dc.VAL_W // 3], nrm[0, -1]
    inv = np.float32(1) / (np.float32(kw["sigma_normal"]) * np.float32(kw["sigma_normal"]))

    def arg(u, v):
        d = u - v
        return (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * inv
    assert arg(a, b) == np.float32(8) and arg(a, c) == np.nextafter(np.float32(8), np.float32(9)) and 0 < arg(b, c) < 1e-5


SMALL = [c for c in dc.SIGMAS if c.small]
LARGE = [c for c in dc.SIGMAS if not c.small]


@pytest.mark.parametrize("case", SMALL, ids=_ids(SMALL))
def test_a_sigma_below_the_clamp_keeps_the_image(dlib, case):
    """The inverse square is FLT_MAX (or, at 1e-17, merely huge): the centre weighs 9/64, every tap with a difference
    weighs 0, and on colours for which c * 9/64 is exact the output is the input.  Before the clamp 0 * inf made NaN."""
    img, g, kw = case.make()
    out = denoise_oracle.run(dlib, img, g, **kw)
    assert not kw["demodulate"] and 0 < kw[case.term] < 1e-16
    assert np.isfinite(out).all(), int(np.isnan(out).any(-1).sum())
    assert out.tobytes() == img.tobytes(), int(_differ(out, img).sum())


@pytest.mark.parametrize("case", LARGE, ids=_ids(LARGE))
def test_a_huge_sigma_is_the_term_switched_off(dlib, case):
    img, g, kw = case.make()
    out = denoise_oracle.run(dlib, img, g, **kw)
    off = denoise_oracle.run(dlib, img, g, **dict(kw, **{case.term: -1.0}))
    assert kw[case.term] >= 1e19
    assert np.isfinite(out).all()
    assert out.tobytes() == off.tobytes() and _differ(out, img).sum() * 4 >= dc.SIGMA_W * dc.SIGMA_H
    other = denoise_oracle.run(dlib, img, g, **dict(kw, **{case.term: 0.0}))
    assert other.tobytes() != out.tobytes()                 # at its default the term does matter on this image


def test_full_mantissa_noise_at_a_clamped_sigma_is_the_centre_tap_alone(dlib):
    """On arbitrary floats a clamped sigma gives fl(fl(c * 9/64) / (9/64)) wherever another tap is inside the image: the
    centre's weight is exactly 9/64 and every other product is an exact zero."""
    W, H = 40, 20
    rng = np.random.default_rng(5)
    g = denoise_oracle.random_guides(rng, W, H)
    img = rng.uniform(0.01, 4, (H, W, 3)).astype(np.float32)
    out = denoise_oracle.run(dlib, img, g, iterations=1, sigma_color=1e-20, demodulate=False)
    w = np.float32(0.140625)
    assert out.tobytes() == ((img * w) / w).astype(np.float32).tobytes()
    assert _differ(out, img).any()
