"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the variance-guided filter and of the spatial variance estimate
(include/hpt.h, "variance-guided filtering"), written from the header's definition: float32, operation by operation, every
pixel at once, taps in the defined order.  numpy's elementwise float32 add, subtract, multiply and divide are the IEEE
operations, one rounding each and no contraction, which is what the library's -ffp-contract=off code computes; fmaxf and
fminf are np.fmax and np.fmin (a NaN operand gives the other one)."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
H5 = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]        # the B3 taps h
G3 = [f32(0.25), f32(0.5), f32(0.25)]                                     # the prefilter's taps g
KEYS = ("albedo", "normal", "position", "coverage")


def falloff(x):
    """e(x) = fmaxf(0, 1 - x * 0.125f)^8 by three squarings."""
    q = np.fmax(f32(0.0), f32(1.0) - x * f32(0.125))
    q = q * q
    q = q * q
    return q * q


def inv_sq(s):
    s = f32(s)
    with np.errstate(all="ignore"):
        return np.fmin(f32(1.0) / (s * s), FLT_MAX).astype(f32)


def _sum3(v):
    """v.x + v.y + v.z, left to right, over the last axis."""
    return (v[..., 0] + v[..., 1]) + v[..., 2]


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def resolve(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0):
    """(levels, sigma_color, sigma_normal, sigma_position) with the defaults of hpt_guided_params filled in."""
    n = int(iterations) if iterations else 5
    assert 1 <= n <= 8
    sc, sn, sp = f32(sigma_color), f32(sigma_normal), f32(sigma_position)
    return n, (f32(2.0) if sc == 0 else sc), (f32(0.5) if sn == 0 else sn), (f32(0.05) if sp == 0 else sp)


def _guides(guides, H, W):
    alb = np.fmax(np.asarray(guides["albedo"], f32).reshape(H, W, 3), f32(1e-3))
    nrm = np.asarray(guides["normal"], f32).reshape(H, W, 3)
    pos = np.asarray(guides["position"], f32).reshape(H, W, 3)
    with np.errstate(invalid="ignore"):
        valid = np.asarray(guides["coverage"], f32).reshape(H, W) > 0
    return alb, nrm, pos, valid


def _shift(H, W, dx, dy):
    """(inside, clipped row index, clipped column index) of the pixel at offset (dx, dy) from every pixel."""
    ys, xs = np.mgrid[0:H, 0:W]
    qx, qy = xs + dx, ys + dy
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    return inside, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)


def _edge_terms(nrm, pos, cy, cx, sn, sp):
    """(e(xn), e(xp)) of every pixel against its tap at [cy, cx]; a term switched off is 1.0f."""
    one = np.ones(nrm.shape[:2], f32)
    en = ep = one
    if sn > 0:
        en = falloff(_sq3(nrm - nrm[cy, cx]) * inv_sq(sn))
    if sp > 0:
        t = _dot3(nrm, pos[cy, cx] - pos)
        ep = falloff(t * t * inv_sq(sp))
    return en, ep


def run_guided(colour, variance, guides, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=True,
               want_levels=False):
    """(image [H, W, 3], variance_out [H, W]) of hpt_denoiser_run_guided; want_levels adds the list of (c_k, v_k), k = 0 .. n."""
    colour = np.asarray(colour, f32)
    H, W = colour.shape[:2]
    var3 = np.asarray(variance, f32).reshape(H, W, 3)
    n, sc, sn, sp = resolve(iterations, sigma_color, sigma_normal, sigma_position)
    alb, nrm, pos, valid = _guides(guides, H, W)
    with np.errstate(all="ignore"):
        dm = valid & bool(demodulate)
        c = np.where(dm[..., None], colour / alb, colour).astype(f32)
        v = np.where(dm, np.fmax(_sum3(var3 / (alb * alb)), f32(0.0)), np.fmax(_sum3(var3), f32(0.0))).astype(f32)
        s2 = sc * sc if sc > 0 else f32(0.0)
        levels = [(c.copy(), v.copy())]
        for k in range(n):
            stride = 1 << k
            inv_c = None
            if sc > 0:
                num = np.zeros((H, W), f32)
                den = np.zeros((H, W), f32)
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        inside, cy, cx = _shift(H, W, i, j)
                        take = inside & valid[cy, cx]
                        gw = G3[j + 1] * G3[i + 1]
                        num = np.where(take, num + v[cy, cx] * gw, num)
                        den = np.where(take, den + gw, den)
                vbar = num / den
                inv_c = np.fmin(f32(1.0) / (s2 * vbar + f32(1e-12)), FLT_MAX)
            total = np.zeros((H, W, 3), f32)
            vsum = np.zeros((H, W), f32)
            wsum = np.zeros((H, W), f32)
            others = np.zeros((H, W), bool)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    inside, cy, cx = _shift(H, W, i * stride, j * stride)
                    take = inside & valid[cy, cx]
                    if i or j:
                        others |= take
                    cq = c[cy, cx]
                    ec = falloff(_sq3(c - cq) * inv_c) if sc > 0 else np.ones((H, W), f32)
                    en, ep = _edge_terms(nrm, pos, cy, cx, sn, sp)
                    w = H5[j + 2] * H5[i + 2] * ec * en * ep
                    total = np.where(take[..., None], total + cq * w[..., None], total)
                    vsum = np.where(take, vsum + v[cy, cx] * (w * w), vsum)
                    wsum = np.where(take, wsum + w, wsum)
            mix = valid & others
            c = np.where(mix[..., None], total / wsum[..., None], c).astype(f32)
            v = np.where(mix, vsum / (wsum * wsum), v).astype(f32)
            levels.append((c.copy(), v.copy()))
        out = np.where(dm[..., None], c * alb, c).astype(f32)
    return (out, v, levels) if want_levels else (out, v)


def estimate_variance(frame, guides, length=None, sigma_normal=0.0, sigma_position=0.0):
    """hpt_denoiser_estimate_variance: [H, W, 3]."""
    frame = np.asarray(frame, f32)
    H, W = frame.shape[:2]
    _, _, sn, sp = resolve(0, 0.0, sigma_normal, sigma_position)
    _, nrm, pos, valid = _guides(guides, H, W)
    with np.errstate(all="ignore"):
        s = np.zeros((H, W, 3), f32)
        t = np.zeros((H, W, 3), f32)
        ws = np.zeros((H, W), f32)
        for j in range(-3, 4):
            for i in range(-3, 4):
                inside, cy, cx = _shift(H, W, i, j)
                take = inside & valid[cy, cx]
                en, ep = _edge_terms(nrm, pos, cy, cx, sn, sp)
                w = en * ep
                cq = frame[cy, cx]
                s = np.where(take[..., None], s + cq * w[..., None], s)
                t = np.where(take[..., None], t + (cq * cq) * w[..., None], t)
                ws = np.where(take, ws + w, ws)
        m = s / ws[..., None]
        var = np.fmax(t / ws[..., None] - m * m, f32(0.0))
        if length is not None:
            var = var / np.fmax(np.asarray(length, f32).reshape(H, W), f32(1.0))[..., None]
        return np.where(valid[..., None], var, f32(0.0)).astype(f32)
