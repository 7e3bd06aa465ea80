"""The photon-mapping estimator against an expected value that does not come from its restatement.

The HIP kernels equal the PPM oracle (tests/ppm_oracle.cpp) bit for bit, so the oracle stands in for them here, on
the CPU.  With light_depth 1 and a rough opaque plane (roughness 1, metallic 0), a pass's radiance at a hit point h is
a sum over the photons that land within r of h, and its expectation is

    E(h) = 1 / (pi r^2) * integral over |x - h| < r of  illum * nl * p(x) * cos(theta_x) * f(wo, wi(x)) dA

with p the density of first hits per unit area facing the light: for a spot light 1 / (2 pi (1 - cos cutoff)) /
|x - pos|^2 inside the cone, for a parallel light 1 / (2 R)^2 on the emission square of half side R = half the
bounds' diagonal; f is the BSDF (oracle.bsdf_eval_pdf).  The integral is taken by quadrature in float64, the
estimate is the mean of K independent passes at probe pixels whose disks are disjoint and lie well inside the cone
and the plane; every z score must stay within 5 and their mean within 3 / sqrt(n)."""
import numpy as np
import pytest

import ppm_oracle

MAT = (0.8, 0.8, 0.8, 1.0, 0.0, 0.0)      # r, g, b, roughness, metallic, eta


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return ppm_oracle.build(tmp_path_factory.mktemp("ppm_estimator_oracle"))


def _quad(sio, a, b, c, d):
    return sio._tris_from([tuple(a) + tuple(b) + tuple(c), tuple(a) + tuple(c) + tuple(d)], [MAT, MAT])


def _floor(sio, h):
    return _quad(sio, (-h, 0, -h), (h, 0, -h), (h, 0, h), (-h, 0, h))


def _wall(sio, h):                        # the plane x = 0
    return _quad(sio, (0, -h, -h), (0, h, -h), (0, h, h), (0, -h, h))


def _disk(r, n, nr=10, nt=24):
    """Equal-area quadrature points of the disk of radius r in the plane with normal n."""
    t = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    t /= np.linalg.norm(t)
    b = np.cross(n, t)
    rr = r * np.sqrt((np.arange(nr) + 0.5) / nr)
    th = 2 * np.pi * (np.arange(nt) + 0.5) / nt
    R, T = np.meshgrid(rr, th, indexing="ij")
    return (R.reshape(-1, 1) * (np.cos(T).reshape(-1, 1) * t + np.sin(T).reshape(-1, 1) * b))


def _inside_cone(L, x, margin=0.0):
    w = np.asarray(L["dir"], np.float64)
    w /= np.linalg.norm(w)
    v = x - np.asarray(L["pos"], np.float64)
    ang = np.arccos(np.clip(v @ w / np.linalg.norm(v, axis=-1), -1, 1))
    return ang < float(L["cutoff"]) - margin


def _expected(oracle_mod, lights, h, n, eye, r, bounds):
    """E(h) of the docstring, channel 0."""
    nl = len(lights)
    wo = np.asarray(eye, np.float64) - h
    wo /= np.linalg.norm(wo)
    xs = h + _disk(r, n)
    total = 0.0
    for L in lights:
        illum = float(L["illum"][0])
        if L["is_parallel"]:
            w = np.asarray(L["dir"], np.float64); w /= np.linalg.norm(w)
            R = np.linalg.norm(np.asarray(bounds[1], np.float64) - np.asarray(bounds[0], np.float64)) * 0.5
            wi = np.broadcast_to(-w, xs.shape)
            p = np.full(len(xs), 1.0 / (2 * R) ** 2)
        else:
            d = np.asarray(L["pos"], np.float64) - xs
            dist2 = (d * d).sum(axis=1)
            wi = d / np.sqrt(dist2)[:, None]
            p = np.where(_inside_cone(L, xs), 1.0 / (2 * np.pi * (1 - np.cos(float(L["cutoff"])))) / dist2, 0.0)
        cos = wi @ n
        f = np.array([oracle_mod.bsdf_eval_pdf(MAT, wo, wi[k], n)[0][0] for k in range(len(xs))], np.float64)
        total += illum * nl * float(np.mean(p * cos * f))      # mean over equal areas = integral / (pi r^2)
    return total


def _probes(pos, ok, key, min_sep, max_n=12):
    """Pixels whose hit point exists in every pass, taken greedily in ascending key(mean position) (a geometric
    order, not one of the estimates) with mean positions at least min_sep apart."""
    valid = np.isfinite(pos).all(axis=(0, 3))
    mean = np.where(np.isfinite(pos), pos, 0).mean(axis=0)
    cand = [(key(mean[iy, ix].astype(np.float64)), iy, ix) for iy, ix in zip(*np.nonzero(valid))]
    picked = []
    for _, iy, ix in sorted(cand):
        h = mean[iy, ix].astype(np.float64)
        if not ok(h):
            continue
        if all(np.linalg.norm(h - q[2]) >= min_sep for q in picked):
            picked.append((iy, ix, h))
        if len(picked) == max_n:
            break
    return picked


CASES = {
    # name: lights (pos, dir, illum, cutoff deg, parallel, ball r), plane, half size, eye, look, spl per pass, radius
    "spot_tilted": ([((0.0, 1.0, 0.0), (0.3, -1.0, 0.2), (1.0, 1.0, 1.0), 45.0, 0, 0.02)], "floor", 2.0,
                    (0.0, 2.2, -1.6), (0.25, 0.0, 0.25), 160000, 0.08),
    "spot_on_wall": ([((-1.0, 0.3, 0.1), (1.0, -0.1, 0.12), (1.0, 1.0, 1.0), 40.0, 0, 0.02)], "wall", 2.0,
                     (-2.4, 0.6, -0.6), (0.0, 0.25, 0.2), 160000, 0.08),
    "two_spots": ([((-0.45, 1.0, 0.0), (-0.2, -1.0, 0.1), (1.0, 1.0, 1.0), 40.0, 0, 0.02),
                   ((0.45, 1.0, 0.1), (0.25, -1.0, -0.1), (0.5, 0.5, 0.5), 40.0, 0, 0.02)], "floor", 2.0,
                  (0.0, 2.4, -1.8), (0.0, 0.0, 0.1), 160000, 0.08),
    "parallel": ([((4.0, 6.0, 4.0), (0.5, -1.0, 0.2), (1.0, 1.0, 1.0), 0.0, 1, 0.02)], "floor", 0.6,
                 (0.0, 1.9, -1.4), (0.0, 0.0, 0.05), 160000, 0.1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ppm_passes_estimate_the_expected_radiance(plib, oracle_mod, sio, name):
    """(spot_tilted) cone sampling in the frame of a direction with |w.x| <= 0.9; (spot_on_wall) |w.x| > 0.9, the
    other frame branch; (two_spots) the flux's factor nl; (parallel) the emission square of an oblique parallel light."""
    spec, plane, half, eye, look, spl, r = CASES[name]
    lights = np.concatenate([sio._one_light(*s) for s in spec])
    tris = _floor(sio, half) if plane == "floor" else _wall(sio, half)
    n = np.array((0.0, 1.0, 0.0) if plane == "floor" else (-1.0, 0.0, 0.0))
    sp = np.zeros(0, sio.SPHERE)
    W, H, K = 24, 18, 16
    cam = sio.make_camera(eye, look, (0.0, 1.0, 0.0), 40.0, W, H)
    bounds = ppm_oracle.scene_bounds(sp, tris)
    r = float(np.float32(r))
    vals, pos = [], []
    for k in range(K):
        _, st, flux, p = ppm_oracle.render(plib, lights, sp, tris, cam, W, H, eye_depth=1, light_depth=1, spl=spl, radius=r,
                                           seed=9, sample_offset=k, want_flux=True, want_pos=True)
        assert st["photons"] == spl * len(lights) and st["deposits"] > 0
        vals.append(flux[..., 0].astype(np.float64) / (np.pi * r * r))
        pos.append(p)
    vals, pos = np.stack(vals), np.stack(pos)

    def ok(h):
        inplane = np.all(np.abs(np.delete(h, 1 if plane == "floor" else 0)) < half - 2 * r)
        ring = h + _disk(2 * r, n, nr=1, nt=16) * np.sqrt(2.0)  # 16 points at 2r around h
        inside = [_inside_cone(L, ring) for L in lights if not L["is_parallel"]]
        clear = all(c.all() or not c.any() for c in inside)      # 2r away from every cone's edge
        return inplane and clear and (not inside or any(c.all() for c in inside))

    def key(h):                                                  # distance to the nearest cone axis on the plane
        ks = [0.0]
        for L in lights:
            if not L["is_parallel"]:
                o, w = np.asarray(L["pos"], np.float64), np.asarray(L["dir"], np.float64)
                t = -(o @ n) / (w @ n)
                ks.append(np.linalg.norm(h - (o + t * w)))
        return min(ks[1:]) if len(ks) > 1 else 0.0
    probes = _probes(pos, ok, key, 2 * r + 0.05)
    assert len(probes) >= 8, len(probes)
    z = []
    for iy, ix, h in probes:
        e = _expected(oracle_mod, lights, h, n, eye, r, bounds)
        v = vals[:, iy, ix]
        se = v.std(ddof=1) / np.sqrt(K)
        assert se < 0.02 * e, (name, h, e, v.mean(), se)
        z.append((v.mean() - e) / se)
    z = np.array(z)
    assert np.abs(z).max() < 5, (name, z)
    assert abs(z.mean()) < 3 / np.sqrt(len(z)), (name, z)
