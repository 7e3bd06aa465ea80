"""A coordinate of k_shade's unit-ball try, for every draw there is (no GPU, exhaustive).

A draw is k * 2^-24 for a 24-bit integer k (rng_next, csrc/pt_device_math.h) and the try turns it into 2 * u - 1.  The
kernel forms the coordinate with one fused multiply-add, fmaf((float) k, 2^-23, -1) (ball_coordinate), where it used to
convert, multiply by 2^-24, multiply by 2 and subtract 1, rounding after each step.  The two agree in every bit because no
step ever rounds: k, k * 2^-24, 2 k * 2^-24 and (k - 2^23) * 2^-23 are all floats for k < 2^24.  A fused multiply-add rounds
the exact k * 2^-23 - 1 once, so it is compared here as float32 of that exact value, computed in float64 (where
k * 2^-23 - 1 is exact as well: 24 significant bits at most)."""
import numpy as np

N = 1 << 24


def test_the_fused_coordinate_is_the_stepwise_one_for_every_draw():
    f = np.float32
    k = np.arange(N, dtype=np.uint32)
    kf = k.astype(f)
    assert (kf.astype(np.uint32) == k).all()                      # the conversion is exact
    u = kf * f(2.0 ** -24)                                        # rng_next's draw
    assert u.dtype == f
    stepwise = u * f(2.0) - f(1.0)                                # mk3(a, b, c) * 2.0f - mk3(1.0f, 1.0f, 1.0f), one component
    assert stepwise.dtype == f
    exact = k.astype(np.float64) * 2.0 ** -23 - 1.0               # no rounding in float64: |k - 2^23| < 2^24
    assert ((exact + 1.0) * 2.0 ** 23 == k).all()
    fused = exact.astype(f)                                       # one rounding of the exact value: what fmaf returns
    assert (fused.astype(np.float64) == exact).all()              # ... and that one does not round either
    differ = stepwise.view(np.uint32) != fused.view(np.uint32)
    print("draws whose coordinate differs: %d of %d" % (int(differ.sum()), N))
    assert not differ.any()
    assert stepwise[0] == -1.0 and stepwise[N // 2] == 0.0 and stepwise[N - 1] == f(1.0) - f(2.0 ** -23)
