"""TEST INFRASTRUCTURE ONLY -- numpy restatement of hpt_history_advance_motion (include/hpt.h, "motion"), written from the
header's steps 2', 3' and 4' on top of history_oracle.History and moments_oracle.MomentHistory: float32, operation by
operation, every pixel at once.  The second moment q is always carried (it rides through the same steps and does not touch
mean or n), so one object stands for a plain history and for one created with HPT_HISTORY_MOMENTS.

branches counts, per advance with the motion guide, the pixels that took each branch of the definition."""
import numpy as np

import history_oracle as ho
import moments_oracle as mo

f32 = np.float32
BRANCHES = ("2_sky_kept", "2_restart", "3_taken", "3_no_cover", "3_plane", "3_normal", "4_direct", "4_range", "4_weight", "4_taken")


def _same_bits(a, b):
    return (np.ascontiguousarray(a, f32).view(np.uint32) == np.ascontiguousarray(b, f32).view(np.uint32)).all(-1)


class MotionHistory(mo.MomentHistory):
    def reset(self):
        super().reset()
        self.branches = dict.fromkeys(BRANCHES, 0)

    def advance(self, camera, frame, normal=None, position=None, coverage=None, prev_position=None, **params):
        if prev_position is None or self.K == 0:          # the plain advance; the first frame is kHistoryFirst either way
            self.branches = dict.fromkeys(BRANCHES, 0)
            return super().advance(camera, frame, normal, position, coverage, **params)
        H, W = self.H, self.W
        mh1, tol2, nmin = ho.resolve(**params)
        cam = ho.constants(camera)
        assert cam is not None and normal is not None and position is not None and coverage is not None
        c = np.asarray(frame, f32).reshape(H, W, 3)
        X = np.array(position, f32).reshape(H, W, 3)
        Xp = np.asarray(prev_position, f32).reshape(H, W, 3)
        N = np.array(normal, f32).reshape(H, W, 3)
        cov = np.array(coverage, f32).reshape(H, W)
        still = camera.tobytes() == self.camera.tobytes()
        br = dict.fromkeys(BRANCHES, 0)
        with np.errstate(all="ignore"):
            hit = cov > 0
            cprev = self.cov > 0
            same = _same_bits(X, Xp)
            # 2'
            sky = ~hit & still & ~cprev
            br["2_sky_kept"] = int(sky.sum()); br["2_restart"] = int((~hit & ~sky).sum())
            # 3'
            own = hit & still & same
            _, _, _, dist2 = ho.project(cam, X)
            take = own & cprev
            br["3_no_cover"] = int((own & ~cprev).sum())
            if tol2 is not None:
                t = ho._dot(N, self.pos - X)
                ok = t * t <= tol2 * dist2
                br["3_plane"] = int((take & ~ok).sum())
                take &= ok
            if nmin is not None:
                ok = ho._dot(N, self.nrm) >= nmin
                br["3_normal"] = int((take & ~ok).sum())
                take &= ok
            br["3_taken"] = int(take.sum())
            # 4'
            m4, q4, n4 = self._taps(cam, X, Xp, N, hit & ~own, dist2, tol2, nmin, br)
            keep_own = sky | take
            m = np.where(keep_own[..., None], self.mean, m4)
            q_r = np.where(keep_own[..., None], self.q, q4)
            n_r = np.where(keep_own, self.n, n4)
            keep = n_r > 0
            n_c = np.fmin(n_r, mh1)
            n1 = n_c + f32(1.0)
            cc = c * c
            mean = (m * n_c[..., None] + c) / n1[..., None]
            q = (q_r * n_c[..., None] + cc) / n1[..., None]
        self.mean = np.where(keep[..., None], mean, c).astype(f32)
        self.q = np.where(keep[..., None], q, cc).astype(f32)
        self.n = np.where(keep, n1, f32(1.0)).astype(f32)
        self.pos, self.nrm, self.cov = X, N, cov
        self.kept = int(keep.sum()); self.restarted = int((~keep).sum())
        self.camera = camera.copy(); self.cam_prev = cam
        self.K += 1
        self.branches = br
        return self.mean.copy()

    def _taps(self, cam, X, Xp, N, todo, dist2, tol2, nmin, br):
        """Step 4' for the pixels in `todo`: (m, q_r, n_r), zero where the pixel restarts."""
        H, W = self.H, self.W
        ys, xs = np.mgrid[0:H, 0:W]
        s, u, v, _ = ho.project(cam, X)
        direct = (s > 0) & (np.abs(u - (xs.astype(f32) + f32(0.5))) <= 1) & (np.abs(v - (ys.astype(f32) + f32(0.5))) <= 1)
        sp, uq, vq, _ = ho.project(self.cam_prev, Xp)
        up, vp = uq - f32(0.5), vq - f32(0.5)
        inr = (sp > 0) & (up >= -1) & (up < f32(W)) & (vp >= -1) & (vp < f32(H))
        br["4_direct"] = int((todo & ~direct).sum()); br["4_range"] = int((todo & direct & ~inr).sum())
        ok = todo & direct & inr
        up, vp = np.where(ok, up, f32(0)), np.where(ok, vp, f32(0))            # only pixels that passed are converted
        fx0, fy0 = np.floor(up), np.floor(vp)
        fx, fy = up - fx0, vp - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        lim = None if tol2 is None else tol2 * dist2
        total = np.zeros((H, W, 3), f32); qtot = np.zeros((H, W, 3), f32)
        nsum = np.zeros((H, W), f32); wsum = np.zeros((H, W), f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                take = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                take &= self.cov[cy, cx] > 0
                if lim is not None:
                    t = ho._dot(N, self.pos[cy, cx] - Xp)
                    take &= t * t <= lim
                if nmin is not None:
                    take &= ho._dot(N, self.nrm[cy, cx]) >= nmin
                w = (fx if i else f32(1.0) - fx) * (fy if j else f32(1.0) - fy)
                total = np.where(take[..., None], total + self.mean[cy, cx] * w[..., None], total)
                qtot = np.where(take[..., None], qtot + self.q[cy, cx] * w[..., None], qtot)
                nsum = np.where(take, nsum + self.n[cy, cx] * w, nsum)
                wsum = np.where(take, wsum + w, wsum)
        good = ok & (wsum > f32(0.01))
        br["4_weight"] = int((ok & ~good).sum()); br["4_taken"] = int(good.sum())
        m = np.where(good[..., None], total / wsum[..., None], f32(0)).astype(f32)
        q = np.where(good[..., None], qtot / wsum[..., None], f32(0)).astype(f32)
        n_r = np.where(good, nsum / wsum, f32(0)).astype(f32)
        return m, q, n_r
