"""Records what the REFERENCE'S OWN CODE computes, as data: tests/golden/ref_functions.npz, ref_rays.npz,
ref_pt_kernel.npz, ref_cpu_bdpt.npz, and on the hostile material and light records of tests/shade_cases.py
ref_hostile_functions.npz and ref_hostile_pt.npz.

It drives oracle/_ref/libref_probe.so -- the reference's sources compiled in place for the host against the stand-in
headers of oracle/shim/ (oracle/Makefile, target `ref`; driver oracle/ref_probe.cpp) -- on the inputs tests/ref_pin_cases.py
builds, and stores inputs and answers together, so that the tests read nothing but these files.  It needs the reference
tree (build() makes oracle/_ref/ where the tree exists); no text of the reference and nothing compiled from it is
written here, only numbers its functions returned.

    python tests/golden/make_ref_golden.py                   # rewrite the six fixtures
    python tests/golden/make_ref_golden.py --validate-survey # also replay the survey-stage images (about two minutes)

The files are written without time stamps, so a second run gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_TESTS = os.path.dirname(_HERE)
_ROOT = os.path.dirname(_TESTS)
for _p in (_ROOT, _TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from path_tracing_amd import scene_io as sio              # noqa: E402
from oracle import ref_probe as rp                        # noqa: E402
import ref_pin_cases as rc                                # noqa: E402
import shade_cases as shc                                 # noqa: E402

FILES = ["ref_functions.npz", "ref_rays.npz", "ref_pt_kernel.npz", "ref_cpu_bdpt.npz", "ref_hostile_functions.npz", "ref_hostile_pt.npz"]
MAX_BYTES = 256 * 1024


def _raw(a):
    """record arrays as bytes: [n, itemsize] uint8"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize) if len(a) else np.zeros((0, a.dtype.itemsize), np.uint8)


def npz_bytes(arrays: dict) -> bytes:
    """A compressed .npz with fixed time stamps and key order: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in arrays:
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def with_mtl_old(sp, tr, mode):
    """The two settings of the field the reference leaves uninitialised and its shadow test reads: `opaque` zeroes it
    (refract 0: every blocker opaque), `eta` sets refract = mtl.eta and Ks = 1 (glass passes light)."""
    sp, tr = sp.copy(), tr.copy()
    for a in (sp, tr):
        if not len(a):
            continue
        a["mtl_old"] = np.zeros((), a.dtype["mtl_old"])
        if mode == "eta":
            a["mtl_old"]["refract"] = a["mtl"]["eta"]
            a["mtl_old"]["Ks"] = 1.0
    return sp, tr


def functions():
    names, edge = rc.edge_records()
    rec = np.concatenate([rc.committed_records(), edge]).astype(np.float32)
    return dict(records=rec, edge_names=names.astype("U16"), table=rp.functions(rec))


def rays():
    out = dict(scenes=np.array(rc.SCENES, "U16"))
    for name in rc.SCENES:
        L, sp, tr, _ = rc.scene(name)
        o, d, p1, p2 = rc.rays(name)
        spz, trz = with_mtl_old(sp, tr, "opaque")
        t, prim = rp.closest_hits(L, spz, trz, o, d)
        vo = rp.visibility(spz, trz, p1, p2)
        spe, tre = with_mtl_old(sp, tr, "eta")
        ve = rp.visibility(spe, tre, p1, p2)
        for v in (vo, ve):
            assert np.isin(v, (0.0, 1.0)).all()              # with Ks = 1 a triple is 0 or 1: stored as one byte each
        out.update({name + "/lights": _raw(L), name + "/spheres": _raw(spz), name + "/tris": _raw(trz),
                    name + "/o": o, name + "/d": d, name + "/t": t, name + "/ordinal": prim,
                    name + "/p1": p1, name + "/p2": p2, name + "/vis_opaque": vo.astype(np.uint8), name + "/vis_eta": ve.astype(np.uint8)})
        print("rays %-9s prims %2d rays %4d (hit %4.1f %%) segments %4d (open %4.1f %% / %4.1f %%)"
              % (name, len(L) + len(sp) + len(tr), len(o), 100 * (prim >= 0).mean(), len(p1), 100 * vo[:, 0].mean(), 100 * ve[:, 0].mean()))
    # the reference's PT flattening of its two scene files (the scene model is built object by object from our parse)
    for name in ("input", "mis_test"):
        (L, sp, tr), sc = rc.scene_file(name)
        raw = L.copy()
        for i, l in enumerate(sc.lights):
            raw[i]["dir"] = l["dir"]                          # as parsed: the flattening normalises
        fl, fs, ft, bounds = rp.flatten_pt(raw, sp, tr, sio.object_order(sc))
        for a in (fs, ft):                                    # the flattening never writes mtl_old: those 52 bytes are whatever
            if len(a):                                        # the stack held, so they are stored as zeros (the named exclusion)
                a["mtl_old"] = np.zeros((), a.dtype["mtl_old"])
        out.update({name + "/flat_lights": _raw(fl), name + "/flat_spheres": _raw(fs), name + "/flat_tris": _raw(ft), name + "/flat_bounds": bounds})
    return out


def pt_kernel():
    out = dict(cases=np.array([r[0] for r in rc.RENDERS], "U24"))
    for case, name, W, H, depth, spp, seed in rc.RENDERS:
        L, sp, tr, (eye, look, up) = rc.scene(name)
        sp, tr = with_mtl_old(sp, tr, "opaque")
        cam = sio.make_camera(eye, look, up, 50.0, W, H)
        img = rp.pt_render(L, sp, tr, cam, W, H, depth, spp, seed)
        out.update({case + "/lights": _raw(L), case + "/spheres": _raw(sp), case + "/tris": _raw(tr), case + "/camera": _raw(cam.reshape(1)),
                    case + "/params": np.array([W, H, depth, spp, seed], np.int64), case + "/image": img})
        print("pt   %-20s mean %.5f lit %4.1f %%" % (case, img.mean(), 100 * (img != 0).any(axis=2).mean()))
    return out


def cpu_bdpt():
    out = dict(cases=np.array([b[0] for b in rc.BDPT], "U16"))
    for name, W, H, spp, spl in rc.BDPT:
        (L, sp, tr), sc = rc.scene_file(name)
        raw = L.copy()
        for i, l in enumerate(sc.lights):
            raw[i]["dir"] = l["dir"]                          # run_cpu_bdpt gets the lights as parsed
        kind, index, group = sio.object_order(sc)
        img = rp.cpu_bdpt(raw, sp, tr, (kind, index, group), sc.eye, sc.look_at, sc.view_up, sc.fov, W, H, 4, 4, spp, spl)
        out.update({name + "/lights": _raw(raw), name + "/spheres": _raw(sp), name + "/tris": _raw(tr),
                    name + "/order": np.stack([kind, index, group]).astype(np.int32),
                    name + "/camera": np.concatenate([sc.eye, sc.look_at, sc.view_up, [sc.fov]]).astype(np.float32),
                    name + "/params": np.array([W, H, 4, 4, spp, spl], np.int64), name + "/image": img})
        print("bdpt %-9s mean %.5f" % (name, img.mean()))
    return out


def hostile_functions():
    """shade_cases.hostile_records(): one material field out of range per block."""
    names, rec = shc.hostile_records()
    return dict(records=rec, block_names=names.astype("U32"), table=rp.functions(rec))


def hostile_pt():
    """The PT kernel on shade_cases.FIXTURE_PT, stored as pt_kernel() stores its cases."""
    out = dict(cases=np.array(shc.FIXTURE_PT, "U24"))
    for case in shc.FIXTURE_PT:
        L, sp, tr, cam, W, H, depth, spp, kw = shc.CASE_BY_NAME[case].make()
        sp, tr = with_mtl_old(sp, tr, "opaque")
        img = rp.pt_render(L, sp, tr, cam, W, H, depth, spp, kw["seed"])
        out.update({case + "/lights": _raw(L), case + "/spheres": _raw(sp), case + "/tris": _raw(tr), case + "/camera": _raw(np.asarray(cam).reshape(1)),
                    case + "/params": np.array([W, H, depth, spp, kw["seed"]], np.int64), case + "/image": img})
        print("hostile pt %-16s mean %.5f lit %4.1f %%" % (case, np.nanmean(img), 100 * (img != 0).any(axis=2).mean()))
    return out


def generate() -> dict:
    """file name -> bytes"""
    parts = {"ref_functions.npz": functions(), "ref_rays.npz": rays(), "ref_pt_kernel.npz": pt_kernel(), "ref_cpu_bdpt.npz": cpu_bdpt(),
             "ref_hostile_functions.npz": hostile_functions(), "ref_hostile_pt.npz": hostile_pt()}
    assert list(parts) == FILES
    return {k: npz_bytes(v) for k, v in parts.items()}


def validate_survey_bdpt():
    """The rebuilt reference against the survey stage's run_cpu_bdpt rows (an independent earlier build of the same
    sources): bit for bit.  About a minute on one thread."""
    (L, sp, tr), sc = rc.scene_file("input")
    raw = L.copy()
    for i, l in enumerate(sc.lights):
        raw[i]["dir"] = l["dir"]
    ref = np.fromfile(os.path.join(_HERE, "survey_cpu_bdpt_input_256x256_4spp_spl8_rows0-63.f32"), np.float32).reshape(64, 256, 3)
    img = rp.cpu_bdpt(raw, sp, tr, sio.object_order(sc), sc.eye, sc.look_at, sc.view_up, sc.fov, 256, 256, 4, 4, 4, 8)
    return bool(np.array_equal(img[:64].view(np.uint32), ref.view(np.uint32)))


def validate_survey_pt():
    """The two survey PT images came from a RESTATED loop that drew bsdf_sample's uniforms in the written order; the
    reference's kernel as g++ compiles it draws them right to left, so it cannot give those bytes.  What holds, and is
    checked here at both survey shapes: the oracle's replay in the written order gives the survey image, and the same
    replay with bsdf_draw_reversed gives the rebuilt kernel's image -- both bit for bit."""
    import oracle
    (L, sp, tr), sc = rc.scene_file("input")
    ok = True
    for fname, W, spp in (("survey_pt_probe_input_200x200_64spp.f32", 200, 64), ("survey_pt_probe_input_128x128_512spp.f32", 128, 512)):
        survey = np.fromfile(os.path.join(_HERE, fname), np.float32).reshape(W, W, 3)
        cam = sio.camera_for(sc, W, W, 50.0)
        kw = dict(seed=4242, rng_mode=1, trig_mode=1, glass_shadow_opaque=1, ball_draw_reversed=True)
        a, _ = oracle.pt_render(L, sp, tr, cam, W, W, 4, spp, **kw)
        b, _ = oracle.pt_render(L, sp, tr, cam, W, W, 4, spp, bsdf_draw_reversed=True, **kw)
        k = rp.pt_render(L, sp, tr, cam, W, W, 4, spp, 4242)
        print("survey %s: oracle(written order) == survey %s; oracle(reversed) == rebuilt kernel %s; rebuilt kernel == survey %s"
              % (fname, np.array_equal(a, survey), np.array_equal(b, k), np.array_equal(k, survey)))
        ok = ok and np.array_equal(a, survey) and np.array_equal(b, k)
    return ok


if __name__ == "__main__":
    if not rp.available():
        sys.exit("oracle/_ref/libref_probe.so is missing: run build() where the reference tree exists")
    if "--validate-survey" in sys.argv:
        print("survey cpu_bdpt rows reproduced bit for bit:", validate_survey_bdpt())
        print("survey pt relations hold:", validate_survey_pt())
    for fname, data in generate().items():
        assert len(data) <= MAX_BYTES, (fname, len(data))
        with open(os.path.join(_HERE, fname), "wb") as fh:
            fh.write(data)
        print("wrote %s (%d bytes)" % (fname, len(data)))
