"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the temporal history (include/hpt.h, "history across camera moves"),
written from the header's definition: float32, operation by operation, every pixel at once.  numpy's elementwise float32
add, subtract, multiply and divide are the IEEE operations, one rounding each and no contraction, which is what the
library's -ffp-contract=off code computes."""
import numpy as np

f32 = np.float32


def _dot(a, b):
    """a.x*b.x + a.y*b.y + a.z*b.z, left to right, over the last axis."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def constants(camera):
    """The camera constants, or None for a camera the library refuses."""
    eye, UL, dx, dy = (np.asarray(camera[k], f32).reshape(3) for k in ("eye", "UL", "dx", "dy"))
    with np.errstate(all="ignore"):
        a = UL - eye
        nrm = _cross(dx, dy)
        an = _dot(a, nrm)
        cu = _cross(dy, nrm)
        gu = cu / _dot(dx, cu)
        cv = _cross(nrm, dx)
        gv = cv / _dot(dy, cv)
    c = dict(eye=eye, a=a, nrm=nrm, an=f32(an), gu=gu.astype(f32), gv=gv.astype(f32))
    if not all(np.isfinite(v).all() for v in c.values()) or c["an"] == 0:
        return None
    return c


def project(c, X):
    """(s, u, v, dist2) of points X [..., 3]."""
    with np.errstate(all="ignore"):
        d = X - c["eye"]
        den = _dot(d, c["nrm"])
        s = c["an"] / den
        r = d * s[..., None] - c["a"]
        return s, _dot(r, c["gu"]), _dot(r, c["gv"]), _dot(d, d)


def resolve(max_history=0.0, plane_tolerance=0.0, normal_min=0.0):
    """(max_history - 1, tol2 or None when the plane test is off, normal_min or None when the normal test is off)."""
    mh = f32(256.0) if f32(max_history) == 0 else f32(max_history)
    tol = f32(0.01) if f32(plane_tolerance) == 0 else f32(plane_tolerance)
    nm = f32(0.9) if f32(normal_min) == 0 else f32(normal_min)
    assert mh >= 1
    return mh - f32(1.0), (None if tol < 0 else tol * tol), (None if nm < -1 else nm)


class History:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.reset()

    def reset(self):
        H, W = self.H, self.W
        self.mean = np.zeros((H, W, 3), f32)
        self.n = np.zeros((H, W), f32)
        self.pos = np.zeros((H, W, 3), f32)
        self.nrm = np.zeros((H, W, 3), f32)
        self.cov = np.zeros((H, W), f32)
        self.K = 0
        self.camera = None
        self.kept = self.restarted = 0
        self.wsum = None

    def advance(self, camera, frame, normal=None, position=None, coverage=None, **params):
        """Returns the new mean [H, W, 3]; kept / restarted hold the frame's counts, wsum the taps' weight sums of a moved
        frame (NaN where the pixel never got to its taps)."""
        H, W = self.H, self.W
        mh1, tol2, nmin = resolve(**params)
        cam = constants(camera)
        assert cam is not None
        guides = position is not None
        assert (normal is not None) == guides == (coverage is not None)
        c = np.asarray(frame, f32).reshape(H, W, 3)
        m = np.zeros((H, W, 3), f32)
        n_r = np.zeros((H, W), f32)
        self.wsum = None
        first = self.K == 0
        identity = not first and camera.tobytes() == self.camera.tobytes()
        if identity:
            m, n_r = self.mean.copy(), self.n.copy()
        elif not first and guides:
            m, n_r = self._reproject(cam, np.asarray(position, f32).reshape(H, W, 3), np.asarray(normal, f32).reshape(H, W, 3),
                                     np.asarray(coverage, f32).reshape(H, W), tol2, nmin)
        with np.errstate(all="ignore"):
            keep = n_r > 0
            n_c = np.fmin(n_r, mh1)
            n1 = n_c + f32(1.0)
            blended = (m * n_c[..., None] + c) / n1[..., None]
        self.mean = np.where(keep[..., None], blended, c).astype(f32)
        self.n = np.where(keep, n1, f32(1.0)).astype(f32)
        if guides:
            self.pos = np.array(position, f32).reshape(H, W, 3)
            self.nrm = np.array(normal, f32).reshape(H, W, 3)
            self.cov = np.array(coverage, f32).reshape(H, W)
        elif not identity:
            self.pos = np.zeros((H, W, 3), f32); self.nrm = np.zeros((H, W, 3), f32); self.cov = np.zeros((H, W), f32)
        self.kept = int(keep.sum())
        self.restarted = 0 if first else int((~keep).sum())
        self.camera = camera.copy()
        self.cam_prev = cam
        self.K += 1
        return self.mean.copy()

    def _reproject(self, cam, X, N, cov, tol2, nmin):
        H, W = self.H, self.W
        ys, xs = np.mgrid[0:H, 0:W]
        with np.errstate(all="ignore"):
            s, u, v, dist2 = project(cam, X)
            direct = (s > 0) & (np.abs(u - (xs.astype(f32) + f32(0.5))) <= 1) & (np.abs(v - (ys.astype(f32) + f32(0.5))) <= 1)
            sp, uq, vq, _ = project(self.cam_prev, X)
            up, vp = uq - f32(0.5), vq - f32(0.5)
            ok = (cov > 0) & direct & (sp > 0) & (up >= -1) & (up < f32(W)) & (vp >= -1) & (vp < f32(H))
            up, vp = np.where(ok, up, f32(0)), np.where(ok, vp, f32(0))        # only pixels that passed are converted
            fx0, fy0 = np.floor(up), np.floor(vp)
            fx, fy = up - fx0, vp - fy0
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            lim = None if tol2 is None else tol2 * dist2
            total = np.zeros((H, W, 3), f32)
            nsum = np.zeros((H, W), f32)
            wsum = np.zeros((H, W), f32)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    take = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    take &= self.cov[cy, cx] > 0
                    if lim is not None:
                        t = _dot(N, self.pos[cy, cx] - X)
                        take &= t * t <= lim
                    if nmin is not None:
                        take &= _dot(N, self.nrm[cy, cx]) >= nmin
                    w = (fx if i else f32(1.0) - fx) * (fy if j else f32(1.0) - fy)
                    total = np.where(take[..., None], total + self.mean[cy, cx] * w[..., None], total)
                    nsum = np.where(take, nsum + self.n[cy, cx] * w, nsum)
                    wsum = np.where(take, wsum + w, wsum)
            good = ok & (wsum > f32(0.01))
            m = np.where(good[..., None], total / wsum[..., None], f32(0)).astype(f32)
            n_r = np.where(good, nsum / wsum, f32(0)).astype(f32)
        self.wsum = np.where(ok, wsum, f32(np.nan))
        return m, n_r
