"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the temporal variance (include/hpt.h, "temporal variance"), written from
the header's definition on top of history_oracle.History: float32, operation by operation, every pixel at once.  The second
moment q goes through the steps the mean goes through -- History._reproject is run a second time with q in the place of the
mean, which gives the same taps, skips, weights and order -- and variance() restates hpt_history_variance."""
import numpy as np

import history_oracle as ho

f32 = np.float32


class MomentHistory(ho.History):
    """A history created with HPT_HISTORY_MOMENTS: mean, n, the stored guides and the counts are History's."""

    def reset(self):
        super().reset()
        self.q = np.zeros((self.H, self.W, 3), f32)

    def advance(self, camera, frame, normal=None, position=None, coverage=None, **params):
        H, W = self.H, self.W
        mh1, tol2, nmin = ho.resolve(**params)
        guides = position is not None
        c = np.asarray(frame, f32).reshape(H, W, 3)
        q_r = np.zeros((H, W, 3), f32)
        n_r = np.zeros((H, W), f32)
        first = self.K == 0
        identity = not first and camera.tobytes() == self.camera.tobytes()
        if identity:
            q_r, n_r = self.q.copy(), self.n.copy()
        elif not first and guides:
            mean = self.mean
            self.mean = self.q                       # the same operations in the same order, on q
            try:
                q_r, n_r = self._reproject(ho.constants(camera), np.asarray(position, f32).reshape(H, W, 3),
                                           np.asarray(normal, f32).reshape(H, W, 3), np.asarray(coverage, f32).reshape(H, W), tol2, nmin)
            finally:
                self.mean = mean
        out = super().advance(camera, frame, normal, position, coverage, **params)
        with np.errstate(all="ignore"):
            keep = n_r > 0
            n_c = np.fmin(n_r, mh1)
            n1 = n_c + f32(1.0)
            cc = c * c
            blended = (q_r * n_c[..., None] + cc) / n1[..., None]
        self.q = np.where(keep[..., None], blended, cc).astype(f32)
        return out

    def variance(self, fallback=None, min_length=0.0):
        """hpt_history_variance: [H, W, 3]; fallback [H, W, 3] or None."""
        L = f32(4.0) if f32(min_length) == 0 else f32(min_length)
        assert L >= 2
        fb = np.zeros((self.H, self.W, 3), f32) if fallback is None else np.asarray(fallback, f32).reshape(self.H, self.W, 3)
        with np.errstate(all="ignore"):
            d = self.q - self.mean * self.mean
            v = np.fmax(d, f32(0.0)) / (self.n - f32(1.0))[..., None]          # fmaxf: a NaN d gives 0
            return np.where((self.n >= L)[..., None], v, fb).astype(f32)
