"""k_shade's per-scene constants on the MI355X, bit for bit against the CPU oracle.

The scene's tables carry what k_shade used to work out at every hit (csrc/hpt_scene.h): per light the area pdf of a
next-event sample, 1 / (number of lights * area), and per material the GGX width and four class bits (smooth dielectric,
mirror, next-event eligible, metallic > 0).  The host fills them (csrc/scene_build.cpp) with the float operations the kernel
used, and the oracle still evaluates them per hit the reference's way, so one differently rounded constant or one class bit
on the wrong side of its threshold is a different image.  Every case is 64 x 64 at 2-4 samples and eye depth 4, the
smallest shape at which its part can go wrong:

  a   three ball lights of different radii and a parallel light: 1 / (n * area) is inexact, and a parallel light counts in n
      (a3: the three balls alone, n = 3, where n * area rounds as well)
  b   33 lights and 129 materials: both tables are read from global memory, not from their LDS copies
  c   a mirror, smooth glass, a rough metal, a rough dielectric with eta > 0 and plain diffuse (r g b 1 0 0) in one scene,
      plus materials just past each threshold of the class bits (roughness 0.001 and 0.01, metallic 0.01 and 0.99)
  d   scene c on one pipeline, without host waits (the strided kernel) and one sample per pass: three more routes to the
      same image
  e   a live scene whose lights change (update_rounds re-fills the light table: radius, hence area and pdf, and position)

Every comparison is np.array_equal."""
import numpy as np
import pytest

import pt_cases as pc
from path_tracing_amd import scene_io as sio
from path_tracing_amd.layouts import SPHERE

pytestmark = pytest.mark.gpu

W = H = 64
DEPTH = 4
_SHARED = {}


def _walls():
    return sio._tris_from([t for _, tl in sio._CORNELL_WALLS for t in tl], [m6 for m6, tl in sio._CORNELL_WALLS for _ in tl])


def _spheres(mats, r=0.09):
    """One sphere per material in rows above the floor, in front of the camera."""
    sp = np.zeros(len(mats), SPHERE)
    for k, m in enumerate(mats):
        col, row = k % 4, k // 4
        sp[k]["center"] = (-0.33 + 0.22 * col, -0.38 + 0.24 * row, 0.45 + 0.12 * row)
        sp[k]["r"] = r
        sp[k]["mtl"]["base_color"] = m[0:3]
        sp[k]["mtl"]["roughness"], sp[k]["mtl"]["metallic"], sp[k]["mtl"]["eta"] = m[3], m[4], m[5]
        sp[k]["id"] = k
    return sp


def _ball_lights(radii):
    spots = [(-0.3, 0.4, 0.2), (0.25, 0.42, 0.5), (0.0, 0.35, 0.75)]
    illum = [(0.9, 0.8, 0.7), (0.3, 0.5, 0.9), (0.8, 0.4, 0.3)]
    return [sio._one_light(spots[k], (0.0, -1.0, 0.0), illum[k], 180.0 if k != 1 else 60.0, 0, radii[k]) for k in range(3)]


CLASS_MATS = [
    (0.95, 0.95, 0.95, 0.0, 1.0, 0.0),       # mirror
    (1.0, 1.0, 1.0, 0.0, 0.0, 1.5),          # smooth glass
    (0.9, 0.8, 0.3, 0.3, 0.9, 0.0),          # rough metal
    (0.8, 0.9, 1.0, 0.4, 0.0, 1.5),          # rough dielectric, eta > 0: no delta lobe and no next-event candidate
    (0.7, 0.6, 0.5, 1.0, 0.0, 0.0),          # plain diffuse
    (0.9, 0.9, 0.9, 0.001, 1.0, 0.0),        # roughness AT 0.001: not a mirror; metallic > 0.99 and roughness <= 0.01: no next event
    (0.9, 0.7, 0.6, 0.02, 1.0, 0.0),         # metallic > 0.99 past roughness 0.01: next event again
    (0.9, 0.9, 1.0, 0.0, 0.01, 1.5),         # eta > 0, smooth, metallic AT 0.01: not the delta dielectric
    (0.8, 0.8, 0.8, 0.0, 0.99, 0.0),         # metallic AT 0.99, smooth: neither a mirror (needs > 0.99) nor eligible (needs < 0.99)
    (0.6, 0.8, 0.6, 0.0005, 0.0, 0.0),       # below the alpha clamp of 1e-3, metallic exactly 0: the dielectric Fresnel branch
    (0.8, 0.6, 0.8, 0.5, 1e-6, 0.0),         # metallic barely > 0: Schlick, specular weight 1
]


def _scene(which):
    if which in ("a", "a3"):
        L = _ball_lights((0.05, 0.07, 0.03))
        if which == "a":
            L.append(sio._one_light((0.0, 0.3, 0.0), (0.2, -1.0, 0.3), (0.15, 0.15, 0.12), 0.0, 1, 0.02))
        return np.concatenate(L), _spheres(CLASS_MATS[2:5]), _walls()
    if which == "b":
        L, sp, tr = pc.staging_case("mats", 129)[:3]
        L = pc._lights(np.random.default_rng(33), 33)
        L["illum"] *= np.float32(1.5)
        return L, sp, tr
    if which == "c":
        return np.concatenate(_ball_lights((0.05, 0.07, 0.03))), _spheres(CLASS_MATS), _walls()
    raise KeyError(which)


def _args(which, spp, seed, **kw):
    L, sp, tr = _scene(which)
    return L, sp, tr, pc._cornell_cam(W, H), W, H, DEPTH, spp, dict(seed=seed, **kw)


CASES = {"a": ("a", 3, 11), "a3": ("a3", 3, 12), "b": ("b", 2, 13), "c": ("c", 4, 14)}


def _reference(oracle_mod, name):
    """(args, oracle image) of a case, computed once and shared: not to be written to."""
    if name not in _SHARED:
        args = _args(*CASES[name])
        img, _ = pc.oracle_render(oracle_mod, args)
        img.setflags(write=False)
        _SHARED[name] = (args, img)
    return _SHARED[name]


def _render(hpt, scene, args, **more):
    L, sp, tr, cam, w, h, depth, spp, kw = args
    return scene.render_pt(cam, w, h, depth, spp, hpt.make_params(**dict(kw, **more)))


def _same(what, img, ref):
    print("%s: %d of %d pixels differ, max abs %.3e, lit %.1f %%" % (what, int((img != ref).any(axis=-1).sum()), W * H,
                                                                     float(np.abs(img - ref).max()), 100.0 * pc.lit_share(ref)))
    assert pc.lit_share(ref) > 0.5                                 # a black image would agree with anything
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("name", list(CASES))
def test_table_constants_give_the_oracles_image(hpt, oracle_mod, name):
    args, ref = _reference(oracle_mod, name)
    L, sp, tr = args[:3]
    if name == "a":
        assert len(L) == 4 and int(L["is_parallel"].sum()) == 1
    if name == "a3":
        assert len(L) == 3 and len(set(L["light_ball"]["r"].tolist())) == 3
    if name == "b":
        assert len(L) == 33 and pc.n_materials(sp, tr) == 129
    if name == "c":
        assert pc.n_materials(sp, tr) == len(CLASS_MATS) + len({m6 for m6, _ in sio._CORNELL_WALLS})
    with hpt.Scene(L, sp, tr) as scene:
        _same(name, _render(hpt, scene, args), ref)


def test_every_route_through_the_shade_kernels_gives_one_image(hpt, oracle_mod):
    """Case d: the two-pipeline default, one pipeline, no host waits (k_shade<0,1> walks the chunks with a stride) and one
    sample per pass all render scene c's image."""
    args, ref = _reference(oracle_mod, "c")
    with hpt.Scene(*args[:3]) as scene:
        images = {"default": _render(hpt, scene, args),
                  "single pipeline": _render(hpt, scene, args, flags=hpt.FLAG_SINGLE_PIPELINE),
                  "no host wait": _render(hpt, scene, args, flags=hpt.FLAG_NO_HOST_WAIT),
                  "one sample per pass": _render(hpt, scene, args, samples_per_pass=1)}
    for what, img in images.items():
        assert np.array_equal(img, images["default"]), what
        _same(what, img, ref)


def test_a_light_update_refills_the_light_table(hpt, oracle_mod):
    """Case e: update_rounds keeps the counts, and any light field may change: a new radius is a new area and a new pdf, and
    the table entry has to follow it."""
    args, ref = _reference(oracle_mod, "a")
    L, sp, tr = args[:3]
    L2 = L.copy()
    L2["light_ball"]["r"][0] = 0.085
    L2["light_ball"]["r"][2] = 0.045
    L2["pos"][1] = (0.2, 0.38, 0.55)
    L2["light_ball"]["center"][1] = L2["pos"][1]
    args2 = (L2,) + tuple(args[1:])
    ref2, _ = pc.oracle_render(oracle_mod, args2)
    assert not np.array_equal(ref2, ref)
    with hpt.Scene(L, sp, tr) as scene:
        _same("before the update", _render(hpt, scene, args), ref)
        scene.update_rounds(L2, sp)
        _same("after the update", _render(hpt, scene, args2), ref2)
        scene.update_rounds(L, sp)
        _same("back again", _render(hpt, scene, args), ref)
