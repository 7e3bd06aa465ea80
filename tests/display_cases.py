"""The case table of the progressive display's tests: which sizes, frames and panel layouts the device is held to, and the
frames themselves.  Shapes are the smallest at which the kernels can go wrong: below one 16-byte access, a scalar tail,
one workgroup plus a remainder (accumulator, 256 lanes of 4 values); below one word, rows that are no multiple of 4
bytes, exactly one word per lane, several workgroups (present, 256 lanes of one packed word)."""
import numpy as np

import display_oracle

f32 = np.float32

# ---- accumulator ------------------------------------------------------------------------------------------------------
# 1 x 1: 3 values, below one 16-byte access.  5 x 3: 45 values = 11 groups + a tail of 1.  67 x 3: 603 values = 150 groups
# + 3 on the vector path, and 603 lanes = two full workgroups plus a remainder on the scalar path that an unaligned
# pointer takes.  347 x 3: 1041 values = 260 groups + 1, so the vector path too spans a full workgroup plus a remainder
# and its tail sits in the second one.
ACCUM_SIZES = [(1, 1), (5, 3), (67, 3), (347, 3)]
ACCUM_COUNTS = [1, 2, 3, 17]


def accum_frames(W, H, K, seed=0):
    """K frames [H, W, 3] with zeros, negatives and values above 1; every frame differs from the others."""
    rng = np.random.default_rng(1000 * seed + 10 * W + H)
    frames = []
    for k in range(K):
        f = rng.normal(loc=0.4, scale=0.8, size=(H, W, 3)).astype(f32)
        flat = f.reshape(-1)
        flat[k % flat.size] = f32(0.0)
        if flat.size > 4:
            flat[(k + 2) % flat.size] = f32(-1.5) - f32(k)
            flat[(k + 3) % flat.size] = f32(37.25) + f32(k)
        frames.append(f)
    return frames


# ---- present ----------------------------------------------------------------------------------------------------------
PRESENT_SIZES = [(1, 1), (3, 2), (50, 37), (64, 4), (65, 5), (256, 1), (130, 67)]
FLAG_COMBOS = [(False, False), (True, False), (False, True), (True, True)]        # (bgr, flip_y)
SENTINEL = 0xA5


def special_values():
    """NaN, +-inf, -0, 1 and its neighbours, and for a few bytes the threshold itself and the float just below it."""
    thr = display_oracle.thresholds()
    v = [np.nan, np.inf, -np.inf, -0.0, 1.0, np.nextafter(f32(1.0), f32(0.0)), np.nextafter(f32(1.0), f32(2.0)), -1e-30, 1e30]
    for k in (1, 2, 127, 128, 200, 255):
        v += [thr[k], np.nextafter(thr[k], f32(-np.inf))]
    return np.array(v, f32)


def present_frames(W, H, count=3, seed=0, specials=True):
    """`count` linear images whose bytes spread over 0..255; from 3 x 2 up the first values of frame 0 and the last of
    frame 1 are the special values (as many as fit)."""
    rng = np.random.default_rng(7000 + 100 * seed + 3 * W + H)
    sp = special_values()
    frames = []
    for k in range(count):
        f = (rng.uniform(-0.05, 1.02, size=(H, W, 3)) ** 2).astype(f32)
        flat = f.reshape(-1)
        if specials and flat.size >= 18:
            m = min(len(sp), flat.size // 2)
            if k == 0:
                flat[:m] = sp[:m]
            elif k == 1:
                flat[flat.size - m:] = sp[:m]
        frames.append(f)
    return frames


# name, W, H, frames (a callable), repeat (a later frame equals an earlier one), flat (the bytes may be all 0 or all 255)
def _black_white(W, H):
    return [np.zeros((H, W, 3), f32), np.ones((H, W, 3), f32)]


def _repeat(W, H):
    a, b = present_frames(W, H, 2, seed=5)
    return [a, b, b, a]


CASES = [dict(name="%dx%d" % (W, H), W=W, H=H, frames=(lambda W=W, H=H: present_frames(W, H)), repeat=False, flat=False)
         for W, H in PRESENT_SIZES]
CASES.append(dict(name="black_white_256x96", W=256, H=96, frames=lambda: _black_white(256, 96), repeat=False, flat=True))
CASES.append(dict(name="black_white_10x10", W=10, H=10, frames=lambda: _black_white(10, 10), repeat=False, flat=True))
CASES.append(dict(name="repeat_33x9", W=33, H=9, frames=lambda: _repeat(33, 9), repeat=True, flat=False))

BLACK_WHITE_SSD = 65025 * 3 * 256 * 96            # 4 793 683 200 > 2^32: a 32-bit accumulation wraps


def case(name):
    return next(c for c in CASES if c["name"] == name)


def expected(c):
    """Per frame of the case: (canonical bytes, ssd_prev) from the oracle, presented in order on one display."""
    d = display_oracle.Display(c["W"], c["H"])
    out = []
    for f in c["frames"]():
        s_prev, _ = d.present(f)
        out.append((d.last, s_prev))
    return out
