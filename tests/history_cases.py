"""The case table of the temporal history's tests (include/hpt.h, "history across camera moves"): which sizes, camera
motions, parameters and guide data the device is held to, and the inputs themselves.

Guides are analytic, built here from scene_io.make_camera: a closed room of axis-aligned planes with a sphere in front
of its back wall, seen through the pixel centres.  Bounded scenes only -- on an open floor that runs to the horizon the
grazing pixels alias whatever colour function is laid over the position.  Frame colours are a smooth function of the
guide position plus seeded noise, so a reprojected mean can be told from a restart.

A case is a list of steps run in order on one history: ("advance", dict(camera, guides or None, frame, params, in_place))
or ("reset",).  Sizes are the smallest at which the kernel can go wrong: one pixel, one row, one column, less than a wave,
a row longer than a wave (67 x 3 = 201 lanes: one workgroup with idle lanes), and 96 x 64 = 24 workgroups."""
import math

import numpy as np

from path_tracing_amd import scene_io

f32 = np.float32
FOV = 50.0

ROOM_LO = np.array([-2.0, -1.5, -2.5])
ROOM_HI = np.array([2.0, 1.5, 2.5])
SPHERE_C = np.array([0.3, -0.2, 1.2])
SPHERE_R = 0.5
EYE = (0.0, 0.0, -2.0)
LOOK = (0.0, 0.0, 1.0)
UP = (0.0, 1.0, 0.0)
GUIDE_SPP = 4.0

SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (67, 3), (96, 64)]
MOTION_SIZE = (40, 30)


def orbit_eye(eye, look, up, degrees):
    """`eye` rotated by `degrees` about the axis through `look` along `up` (Rodrigues, in double), rounded to float."""
    e, c, k = (np.asarray(v, np.float64) for v in (eye, look, up))
    k = k / math.sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2])
    v = e - c
    t = degrees * math.pi / 180.0
    cs, sn = math.cos(t), math.sin(t)
    kxv = np.array([k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]])
    r = v * cs + kxv * sn + k * ((k[0] * v[0] + k[1] * v[1] + k[2] * v[2]) * (1.0 - cs))
    return tuple(float(f32(x)) for x in (c + r))


def camera(W, H, eye=EYE, look=LOOK, up=UP):
    return scene_io.make_camera(eye, look, up, FOV, W, H)


def orbit(W, H, degrees):
    return camera(W, H, eye=orbit_eye(EYE, LOOK, UP, degrees))


def dolly(W, H, step):
    return camera(W, H, eye=(EYE[0], EYE[1], EYE[2] + step))


def turned(W, H):
    """The same eye looking the other way."""
    return camera(W, H, look=tuple(2.0 * e - l for e, l in zip(EYE, LOOK)))


WALL_EYE = (0.0, 0.0, 0.5)      # two units from the back wall: at 50 degrees nothing else is in view
WALL_LOOK = (0.0, 0.0, 2.5)


def wall_camera(W, H, px_x=0.0, px_y=0.0):
    """A camera facing the back wall alone, moved parallel to its image plane so that the wall slides by (px_x, px_y)
    pixels against wall_camera(W, H)."""
    cam = scene_io.make_camera(WALL_EYE, WALL_LOOK, UP, FOV, W, H)
    dx, dy = np.asarray(cam["dx"], np.float64), np.asarray(cam["dy"], np.float64)
    shift = (px_x * dx + px_y * dy) * (ROOM_HI[2] - WALL_EYE[2])
    return scene_io.make_camera(tuple(np.asarray(WALL_EYE) + shift), tuple(np.asarray(WALL_LOOK) + shift), UP, FOV, W, H)


def colour_of(X):
    """The noise-free colour laid over the room: smooth in the position."""
    X = np.asarray(X, np.float64)
    with np.errstate(invalid="ignore"):
            return np.stack([0.5 + 0.35 * np.sin(1.3 * X[..., 0] + 0.7 * X[..., 1]), 0.5 + 0.35 * np.cos(0.9 * X[..., 1] - 1.1 * X[..., 2]),
                         0.4 + 0.3 * np.sin(0.8 * X[..., 2] + 0.5 * X[..., 0] + 1.0)], -1)


def guides(cam, W, H, sphere=True):
    """Position, ray-facing normal and coverage of the room seen through the pixel centres of `cam` (double, rounded)."""
    eye = np.asarray(cam["eye"], np.float64)
    a = np.asarray(cam["UL"], np.float64) - eye
    ys, xs = np.mgrid[0:H, 0:W]
    d = a + (xs[..., None] + 0.5) * np.asarray(cam["dx"], np.float64) + (ys[..., None] + 0.5) * np.asarray(cam["dy"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ax = np.where(d > 0, (ROOM_HI - eye) / d, np.where(d < 0, (ROOM_LO - eye) / d, np.inf))
    axis = t_ax.argmin(-1)
    t = t_ax.min(-1)
    nrm = np.zeros((H, W, 3))
    np.put_along_axis(nrm, axis[..., None], -np.sign(np.take_along_axis(d, axis[..., None], -1)), -1)
    if sphere:
        oc = eye - SPHERE_C
        A, B, Cc = (d * d).sum(-1), 2.0 * (d * oc).sum(-1), float(oc @ oc) - SPHERE_R ** 2
        disc = B * B - 4 * A * Cc
        ts = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        hit = (ts > 0) & (ts < t)
        t = np.where(hit, ts, t)
        ns = (eye + np.where(hit, ts, 0.0)[..., None] * d - SPHERE_C) / SPHERE_R
        nrm = np.where(hit[..., None], ns, nrm)
    pos = eye + t[..., None] * d
    return dict(position=pos.astype(f32), normal=nrm.astype(f32), coverage=np.full((H, W), GUIDE_SPP, f32))


def frame(g, seed, noise=0.15):
    rng = np.random.default_rng(seed)
    return (colour_of(g["position"]) + rng.normal(0.0, noise, g["position"].shape)).astype(f32)


def _adv(cam, g, seed, params=None, in_place=False, with_guides=True):
    return ("advance", dict(camera=cam, guides=g if with_guides else None, frame=frame(g, seed), params=params or {}, in_place=in_place))


def _sequence(W, H, cams, params=None, seed=0, sphere=True):
    """One advance per camera, each with its own guides and a fresh frame."""
    return [_adv(c, guides(c, W, H, sphere), 100 * seed + k, params) for k, c in enumerate(cams)]


def _bad_guides(W, H):
    """A 5 degree orbit whose moved frame holds, in a few pixels: a point exactly at the new eye, one at the previous eye,
    NaN and infinite positions, a NaN coverage and a zero coverage; and whose first frame stores a NaN position and a NaN
    normal for the moved frame's taps to meet."""
    A, B = camera(W, H), orbit(W, H, 5.0)
    gA, gB = guides(A, W, H), guides(B, W, H)
    fA1, fA2, fB = frame(gA, 1), frame(gA, 2), frame(gB, 3)       # the colours stay finite
    gA["position"][H // 2, W // 2] = np.nan
    gA["normal"][H // 2, W // 2 + 1] = np.nan
    gA["coverage"][H // 2 + 1, W // 2] = 0.0
    p = gB["position"]
    p[0, 0] = B["eye"]; p[0, 1] = A["eye"]
    p[1, 0] = (np.nan, 0.0, 0.0); p[1, 1] = (np.inf, 1.0, 1.0); p[1, 2] = (0.0, -np.inf, 1.0); p[1, 3] = (np.nan, np.nan, np.nan)
    p[2, 0] = (1e38, 1e38, 1e38); p[2, 1] = (-1e38, 0.0, 3e38)
    gB["coverage"][3, 0] = np.nan; gB["coverage"][3, 1] = 0.0; gB["coverage"][3, 2] = -1.0
    gB["normal"][3, 3] = np.nan
    steps = [_adv(A, gA, 1), _adv(A, gA, 2), _adv(B, gB, 3), _adv(orbit(W, H, 10.0), guides(orbit(W, H, 10.0), W, H), 4)]
    for step, f in zip(steps, (fA1, fA2, fB)):
        step[1]["frame"] = f
    return steps


def _cases():
    out = {}
    for W, H in SIZES:      # still, still, 5 degrees, 10 degrees
        out["size_%dx%d" % (W, H)] = _sequence(W, H, [camera(W, H), camera(W, H), orbit(W, H, 5.0), orbit(W, H, 10.0)], seed=W + H)
    W, H = MOTION_SIZE
    for deg in (0.5, 5.0, 15.0):
        out["orbit_%g" % deg] = _sequence(W, H, [camera(W, H)] * 3 + [orbit(W, H, deg), orbit(W, H, 2 * deg)], seed=int(10 * deg))
    out["dolly"] = _sequence(W, H, [camera(W, H)] * 2 + [dolly(W, H, 0.4), dolly(W, H, 0.8), dolly(W, H, 0.4)], seed=7)
    out["turn_180"] = _sequence(W, H, [camera(W, H)] * 2 + [turned(W, H), camera(W, H)], seed=8)
    for mh in (1.0, 4.0):
        out["still_max_history_%g" % mh] = _sequence(23, 5, [camera(23, 5)] * 7 + [orbit(23, 5, 1.0)], dict(max_history=mh), seed=int(mh))
    out["still_default"] = _sequence(23, 5, [camera(23, 5)] * 5, seed=9)
    # guides NULL: on a moved frame (the reference's restart; the frame after it finds coverage 0 everywhere), and on an
    # unmoved frame (the stored guides are kept, so the moved frame after it still reprojects)
    A, B, C2 = camera(W, H), orbit(W, H, 3.0), orbit(W, H, 6.0)
    gA, gB, gC = guides(A, W, H), guides(B, W, H), guides(C2, W, H)
    out["null_guides_moved"] = [_adv(A, gA, 1), _adv(B, gB, 2, with_guides=False), _adv(C2, gC, 3), _adv(C2, gC, 4, with_guides=False)]
    out["null_guides_unmoved"] = [_adv(A, gA, 1), _adv(A, gA, 2, with_guides=False), _adv(B, gB, 3), _adv(C2, gC, 4)]
    out["null_guides_first"] = [_adv(A, gA, 1, with_guides=False), _adv(A, gA, 2, with_guides=False), _adv(B, gB, 3), _adv(C2, gC, 4)]
    for name, prm in (("plane_off", dict(plane_tolerance=-1.0)), ("normal_off", dict(normal_min=-2.0)),
                      ("both_off", dict(plane_tolerance=-1.0, normal_min=-2.0)), ("tight", dict(plane_tolerance=1e-4, normal_min=0.999))):
        out["switch_" + name] = _sequence(W, H, [camera(W, H)] * 2 + [orbit(W, H, 5.0), orbit(W, H, 10.0)], prm, seed=11)
    out["bad_guides"] = _bad_guides(W, H)
    out["bad_guides_tests_off"] = [(op, dict(a, params=dict(plane_tolerance=-1.0, normal_min=-2.0))) for op, a in _bad_guides(W, H)]
    # the back wall alone, sliding by fractions of a pixel: taps leave the image at every border
    for k, (sx, sy) in enumerate([(0.4, 0.0), (-0.4, 0.0), (0.0, 0.3), (0.0, -0.3), (1.6, -1.3), (-0.7, 0.6)]):
        out["border_%d" % k] = _sequence(13, 9, [wall_camera(13, 9), wall_camera(13, 9), wall_camera(13, 9, sx, sy)], seed=20 + k, sphere=False)
    # ... and by just under / over 0.99 pixel: the border column is left with wsum = 1 - fx on either side of 0.01
    for name, sx in (("below", 0.9915), ("above", 0.9885)):
        out["weight_floor_" + name] = _sequence(13, 9, [wall_camera(13, 9), wall_camera(13, 9), wall_camera(13, 9, sx, 0.0)], seed=30, sphere=False)
    out["in_place"] = [(op, dict(a, in_place=True)) for op, a in _sequence(W, H, [camera(W, H)] * 2 + [orbit(W, H, 5.0)], seed=12)]
    seq = _sequence(W, H, [camera(W, H)] * 2 + [orbit(W, H, 5.0), orbit(W, H, 5.0), orbit(W, H, 10.0)], seed=13)
    out["reset_mid_sequence"] = seq[:3] + [("reset",)] + seq[3:]
    return out


CASES = _cases()


def run_oracle(steps, W, H):
    """Per advance: (mean, length, kept, restarted, frames)."""
    import history_oracle as ho
    h = ho.History(W, H)
    out = []
    for step in steps:
        if step[0] == "reset":
            h.reset()
            continue
        a = step[1]
        g = a["guides"] or {}
        mean = h.advance(a["camera"], a["frame"], g.get("normal"), g.get("position"), g.get("coverage"), **a["params"])
        out.append((mean, h.n.copy(), h.kept, h.restarted, h.K))
    return out


def size_of(steps):
    f = next(s[1]["frame"] for s in steps if s[0] == "advance")
    return f.shape[1], f.shape[0]
