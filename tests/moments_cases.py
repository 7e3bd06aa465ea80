"""The case table of the temporal variance's tests (include/hpt.h, "temporal variance"): every sequence of
history_cases.CASES run on a history with moments, a variance call after every advance, plus the sequences that are about
the second moment itself.

A case is dict(steps, min_length, fallback): `steps` as in history_cases; `min_length` 0 (the default, 4) or 2; `fallback`
"image" (a recognisable pattern in an image of its own), "null" or "in_place" (the pattern lies in the output image).  The
table cycles through the six combinations.  A case whose name ends in "fallback_only" never reaches n >= L; every other
case has pixels on both sides of it somewhere in its sequence (tests/test_moments_cpu.py checks that)."""
import numpy as np

import history_cases as hc

f32 = np.float32
FALLBACKS = ("image", "null", "in_place")

# sequences of history_cases whose history never gets as long as the minimum they are given here
FALLBACK_ONLY = {"still_max_history_1": 2.0}
# ... and those that need the shorter minimum to reach the temporal branch at all (their histories stay below 4)
SHORT = ("turn_180", "reset_mid_sequence", "null_guides_moved", "null_guides_first", "weight_floor_below", "weight_floor_above", "in_place",
         "border_0", "border_1", "border_2", "border_3", "border_4", "border_5")


def pattern(W, H):
    """The fallback image: k / 1024 + 1 for the k-th float, exact in float and unlike any variance of these frames."""
    return (np.arange(3 * W * H, dtype=np.float64) / 1024.0 + 1.0).astype(f32).reshape(H, W, 3)


def _still(W, H, frames, params=None, seed=0):
    return hc._sequence(W, H, [hc.camera(W, H)] * frames, params, seed=seed)


def _non_finite():
    """Four still frames and a moved one whose colours hold NaN, +-inf and 1e20 in a few pixels: c * c overflows, and
    q - m * m is inf - inf."""
    W, H = 23, 5
    steps = hc._sequence(W, H, [hc.camera(W, H)] * 4 + [hc.orbit(W, H, 1.0)], seed=41)
    f = steps[0][1]["frame"]
    f[1, 2, 0] = np.nan; f[1, 3] = np.inf; f[1, 4, 1] = -np.inf; f[1, 5] = 1e20; f[1, 6, 2] = -1e20
    f = steps[2][1]["frame"]
    f[2, 2] = np.nan; f[2, 3, 0] = -np.inf; f[2, 7] = (1e20, -1e20, 3e38); f[2, 8, 1] = np.inf
    f = steps[4][1]["frame"]
    f[3, 10] = (np.inf, -np.inf, np.nan); f[3, 11] = 1e20
    return steps


def _fractional_length():
    """The back wall: one frame, a slide by (1.6, -1.3) pixels that leaves restarted pixels (n = 1) beside kept ones
    (n = 2), then a slide by (0.4, 0.3) more: pixels whose taps hold both get a reprojected n strictly between 1 and 2."""
    W, H = 13, 9
    return hc._sequence(W, H, [hc.wall_camera(W, H), hc.wall_camera(W, H, 1.6, -1.3), hc.wall_camera(W, H, 2.0, -1.0)], seed=43, sphere=False)


def _cases():
    out = {}
    for k, name in enumerate(sorted(hc.CASES)):
        L = FALLBACK_ONLY.get(name, 2.0 if name in SHORT else (0.0, 2.0)[k % 2])
        key = name + "_fallback_only" if name in FALLBACK_ONLY else name
        out[key] = dict(steps=hc.CASES[name], min_length=L, fallback=FALLBACKS[k % 3])
    out["non_finite"] = dict(steps=_non_finite(), min_length=0.0, fallback="image")
    out["non_finite_min_2_in_place"] = dict(steps=_non_finite(), min_length=2.0, fallback="in_place")
    # n = 1 .. 6 under the default minimum: frames 3 and 4 lie on either side of n >= 4
    out["still_passes_4"] = dict(steps=_still(23, 5, 6, seed=44), min_length=0.0, fallback="image")
    out["still_passes_4_in_place"] = dict(steps=_still(23, 5, 6, seed=44), min_length=0.0, fallback="in_place")
    out["max_history_1_fallback_only"] = dict(steps=_still(23, 5, 5, dict(max_history=1.0), seed=45), min_length=0.0, fallback="null")
    out["max_history_4"] = dict(steps=_still(23, 5, 8, dict(max_history=4.0), seed=46), min_length=0.0, fallback="image")      # n - 1 = 3 forever
    out["fractional_length_min_2"] = dict(steps=_fractional_length(), min_length=2.0, fallback="image")
    seq = _still(23, 5, 7, seed=47)
    out["reset_between_advances"] = dict(steps=seq[:5] + [("reset",)] + seq[5:], min_length=0.0, fallback="in_place")
    return out


CASES = _cases()


def size_of(case):
    return hc.size_of(case["steps"])


def run_oracle(case):
    """Per advance: dict(mean, length, q, variance, kept, restarted, frames)."""
    import moments_oracle as mo
    W, H = size_of(case)
    h = mo.MomentHistory(W, H)
    fb = None if case["fallback"] == "null" else pattern(W, H)
    out = []
    for step in case["steps"]:
        if step[0] == "reset":
            h.reset()
            continue
        a = step[1]
        g = a["guides"] or {}
        mean = h.advance(a["camera"], a["frame"], g.get("normal"), g.get("position"), g.get("coverage"), **a["params"])
        out.append(dict(mean=mean, length=h.n.copy(), q=h.q.copy(), variance=h.variance(fb, case["min_length"]), kept=h.kept,
                        restarted=h.restarted, frames=h.K))
    return out
