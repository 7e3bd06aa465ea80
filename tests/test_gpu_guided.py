"""The variance-guided filter on the MI355X: hpt_denoiser_run_guided, hpt_denoiser_estimate_variance and hpt_history_length
against the numpy oracle (tests/guided_oracle.py), bit for bit, colour and variance alike, over the shapes and switches of
tests/guided_cases.py; hostile variance and length images; every caller image a view of one arena between sentinel bands;
a plain run before and after a guided one on the same denoiser; two denoisers on two streams; the refusals that need a
live object; and the chain render -> untile -> guides -> history -> length -> estimate -> guided run on the project's scene
against the chain of the oracles."""
import os
import subprocess

import numpy as np
import pytest

import denoise_oracle
import guided_cases as gc
import guided_oracle as go
import history_cases as hc
import history_oracle as ho
from conftest import GOLDEN, ROOT
from test_history_cpu import chain_inputs

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = go.KEYS
SENTINEL = np.uint32(0x7FC0DEAD)          # a quiet NaN with a payload: no kernel computes it


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def _dev_guides(torch, g):
    return [_dev(torch, g[k]) for k in KEYS]


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert np.isfinite(ref).all(), what                     # the cases keep NaN out of the results: bits can be compared
    bad = got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32)
    assert not bad.any(), (what, "%d of %d values differ" % (int(bad.sum()), bad.size), np.argwhere(bad)[:4].ravel().tolist())


def _filter_kw(kw):
    return {k: v for k, v in kw.items() if k in ("sigma_normal", "sigma_position")}


# ---- shapes and switches ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", gc.SHAPES, ids=[s.name for s in gc.SHAPES])
def test_shape_under_every_switch(hpt, torch, shape):
    img, g, var, length = gc.inputs(shape)
    W, H = shape.W, shape.H
    dg, din, dvar, dlen = _dev_guides(torch, g), _dev(torch, img), _dev(torch, var), _dev(torch, length)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for kw in gc.switches_for(shape):
            ref, ref_v = go.run_guided(img, var, g, **kw)
            dout = torch.full_like(din, float("nan"))
            dv = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
            d.run_guided(din, dvar, dout, dv, hpt.make_guided_params(**kw))
            torch.cuda.synchronize()
            _same(dout.cpu().numpy(), ref, ("colour", kw))
            _same(dv.cpu().numpy(), ref_v, ("variance", kw))
            dout2 = torch.full_like(din, float("nan"))
            d.run_guided(din, dvar, dout2, None, hpt.make_guided_params(**kw))             # without the variance image
            torch.cuda.synchronize()
            _same(dout2.cpu().numpy(), ref, ("colour alone", kw))
        for kw in gc.switches_for(shape)[:4]:                   # the estimator reads the two guide sigmas only
            for use_len in (False, True):
                ref = go.estimate_variance(img, g, length if use_len else None, **_filter_kw(kw))
                de = torch.full_like(din, float("nan"))
                d.estimate_variance(din, de, dlen if use_len else None, hpt.make_guided_params(**kw))
                torch.cuda.synchronize()
                _same(de.cpu().numpy(), ref, ("estimate", use_len, kw))
    assert din.cpu().numpy().tobytes() == img.tobytes() and dvar.cpu().numpy().tobytes() == var.tobytes()


@pytest.mark.parametrize("shape", gc.SHAPES, ids=[s.name for s in gc.SHAPES])
def test_variance_with_zeros_nan_negative_and_1e30(hpt, torch, shape):
    img, g, var, _ = gc.inputs(shape, hostile=True)
    W, H = shape.W, shape.H
    dg, din, dvar = _dev_guides(torch, g), _dev(torch, img), _dev(torch, var)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for kw in (gc.switches_for(shape)[0], gc.switches_for(shape)[8]):                 # demodulated and not, every term on
            ref, ref_v = go.run_guided(img, var, g, **kw)
            dout = torch.full_like(din, float("nan"))
            dv = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
            d.run_guided(din, dvar, dout, dv, hpt.make_guided_params(**kw))
            torch.cuda.synchronize()
            _same(dout.cpu().numpy(), ref, ("colour", kw))
            _same(dv.cpu().numpy(), ref_v, ("variance", kw))


# ---- the history's length image -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["orbit_5", "still_default", "size_67x3"])
def test_history_length_is_the_n_that_read_returns(hpt, torch, name):
    steps = hc.CASES[name]
    W, H = hc.size_of(steps)
    modes = set()
    oracle_n = [r[1] for r in hc.run_oracle(steps, W, H)]
    with hpt.History(W, H) as h:
        out = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            h.length(out)
        last = None
        for k, step in enumerate(steps):
            assert step[0] == "advance"
            a = step[1]
            g = a["guides"]
            dev = {key: _dev(torch, v) for key, v in dict(g, frame=a["frame"]).items()}
            h.advance(a["camera"], dev["frame"], dev["normal"], dev["position"], dev["coverage"],
                      params=hpt.make_history_params(**a["params"]) if a["params"] else None)
            modes.add("first" if k == 0 else "unmoved" if np.asarray(a["camera"]).tobytes() == last else "moved")
            last = np.asarray(a["camera"]).tobytes()
            out.fill_(float("nan"))
            h.length(out)
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == h.read()["length"].tobytes() == oracle_n[k].tobytes(), (name, k)
        h.reset()
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            h.length(out)
    assert "first" in modes and ("moved" in modes or "unmoved" in modes)


def test_history_length_cases_cover_first_unmoved_and_moved():
    def modes(name):
        cams = [np.asarray(s[1]["camera"]).tobytes() for s in hc.CASES[name]]
        return {"unmoved" if a == b else "moved" for a, b in zip(cams, cams[1:])}
    assert "moved" in modes("orbit_5") and modes("still_default") == {"unmoved"}


# ---- one arena ------------------------------------------------------------------------------------------------------------

GUARDS = (37, 33, 35, 31, 34, 41, 39, 43, 38, 45, 36)      # floats before each of the ten images, and after the last


@pytest.mark.parametrize("shape", [gc.SHAPES[0], gc.SHAPES[2], gc.SHAPES[4]], ids=lambda s: s.name)
def test_views_of_one_arena_between_sentinel_bands(hpt, torch, shape):
    """colour | variance | length | albedo | normal | position | coverage | estimate | output | variance-out in one tensor at
    4-byte alignment: the three outputs get the oracle's bits and no other float changes."""
    img, g, var, length = gc.inputs(shape, hostile=True)
    W, H = shape.W, shape.H
    kw = gc.switches_for(shape)[0]
    ref_e = go.estimate_variance(img, g, length, **_filter_kw(kw))
    ref, ref_v = go.run_guided(img, var, g, **kw)
    parts = [img, var, length] + [g[k] for k in KEYS] + [ref_e, ref, ref_v]
    n_in = 7
    offs, at = [], 0
    for guard, a in zip(GUARDS, parts):
        at += guard
        offs.append(at)
        at += a.size
    total = at + GUARDS[-1]
    host = np.full(total, SENTINEL, np.uint32)
    for o, a in list(zip(offs, parts))[:n_in]:
        host[o: o + a.size] = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
    assert sum(1 for o in offs if o % 4) >= 5                                   # 4-byte alignment only
    arena = torch.from_numpy(host.view(np.float32).copy()).cuda()
    v = [arena[o: o + a.size] for o, a in zip(offs, parts)]
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*v[3:7])
        d.estimate_variance(v[0], v[7], v[2], hpt.make_guided_params(**kw))
        d.run_guided(v[0], v[1], v[8], v[9], hpt.make_guided_params(**kw))
        torch.cuda.synchronize()
    back = arena.cpu().numpy().view(np.uint32)
    want = host.copy()
    for o, a in list(zip(offs, parts))[n_in:]:
        want[o: o + a.size] = a.reshape(-1).view(np.uint32)
        _same(back[o: o + a.size].view(np.float32), a, "output at %d" % o)
    wrong = np.nonzero(back != want)[0]
    assert wrong.size == 0, ("floats outside the outputs changed", wrong[:8].tolist(), offs)


# ---- state ----------------------------------------------------------------------------------------------------------------

def test_plain_run_before_and_after_a_guided_run_gives_its_old_bytes(hpt, torch, tmp_path):
    dlib = denoise_oracle.build(tmp_path)
    shape = gc.SHAPES[4]
    img, g, var, length = gc.inputs(shape)
    W, H = shape.W, shape.H
    plain_kw = dict(iterations=4, sigma_color=2.0)
    ref_plain = denoise_oracle.run(dlib, img, g, **plain_kw)
    ref, ref_v = go.run_guided(img, var, g)
    assert ref_plain.tobytes() != ref.tobytes()
    dg, din, dvar, dlen = _dev_guides(torch, g), _dev(torch, img), _dev(torch, var), _dev(torch, length)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for step in ("plain", "guided", "plain", "estimate", "plain", "guided"):
            dout = torch.full_like(din, float("nan"))
            if step == "plain":
                d.run(din, dout, hpt.make_denoise_params(**plain_kw))
                want = ref_plain
            elif step == "guided":
                d.run_guided(din, dvar, dout)                                   # params None: the defaults
                want = ref
            else:
                d.estimate_variance(din, dout, dlen)
                want = go.estimate_variance(img, g, length)
            torch.cuda.synchronize()
            _same(dout.cpu().numpy(), want, step)


def test_two_denoisers_interleaved_on_two_streams(hpt, torch):
    shapes = (gc.SHAPES[2], gc.SHAPES[4])
    data = [gc.inputs(s) for s in shapes]
    kws = [gc.switches_for(s)[0] for s in shapes]
    kws[1] = dict(kws[1], iterations=3, demodulate=False)
    refs = []
    for (img, g, var, length), kw in zip(data, kws):
        est = go.estimate_variance(img, g, length, **_filter_kw(kw))
        refs.append((est,) + go.run_guided(img, est, g, **kw))
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert st[0].cuda_stream != st[1].cuda_stream != 0
    dev = [dict(g=_dev_guides(torch, g), img=_dev(torch, img), len=_dev(torch, length)) for img, g, var, length in data]
    for k, s in enumerate(shapes):
        dev[k]["est"] = torch.full_like(dev[k]["img"], float("nan"))
        dev[k]["out"] = [torch.full_like(dev[k]["img"], float("nan")) for _ in range(2)]
        dev[k]["v"] = [torch.full((s.H, s.W), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with hpt.Denoiser(shapes[0].W, shapes[0].H) as d0, hpt.Denoiser(shapes[1].W, shapes[1].H) as d1:
        den = (d0, d1)
        for k in range(2):
            den[k].set_guides(*dev[k]["g"], stream=st[k].cuda_stream)
        for k in range(2):
            den[k].estimate_variance(dev[k]["img"], dev[k]["est"], dev[k]["len"], hpt.make_guided_params(**kws[k]), stream=st[k].cuda_stream)
        for rep in range(2):
            for k in range(2):
                den[k].run_guided(dev[k]["img"], dev[k]["est"], dev[k]["out"][rep], dev[k]["v"][rep], hpt.make_guided_params(**kws[k]),
                                  stream=st[k].cuda_stream)
        for s in st:
            s.synchronize()
    for k in range(2):
        _same(dev[k]["est"].cpu().numpy(), refs[k][0], ("estimate", k))
        for rep in range(2):
            _same(dev[k]["out"][rep].cpu().numpy(), refs[k][1], ("colour", k, rep))
            _same(dev[k]["v"][rep].cpu().numpy(), refs[k][2], ("variance", k, rep))


def test_refusals_on_a_live_object_enqueue_nothing(hpt, torch):
    W, H = 5, 3
    n3, n1 = W * H * 3, W * H
    buf = torch.full((8 * n3,), -7.25, dtype=torch.float32, device="cuda")
    rgb, var, out, vout = buf[:n3], buf[n3:2 * n3], buf[2 * n3:3 * n3], buf[3 * n3:3 * n3 + n1]
    img, g, _, _ = gc.inputs(gc.SHAPES[2])
    dg = _dev_guides(torch, {k: v[:H, :W] for k, v in g.items()})
    with hpt.Denoiser(W, H) as d:
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before hpt_denoiser_set_guides"):
            d.run_guided(rgb, var, out, vout)
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before hpt_denoiser_set_guides"):
            d.estimate_variance(rgb, out)
        d.set_guides(*dg)
        P = hpt.make_guided_params
        nan = float("nan")
        bad_flags = P()
        bad_flags.flags = 4
        for args, kw, word in (((rgb, var, buf[1:1 + n3]), {}, "d_out must not overlap"),
                               ((rgb, var, buf[2 * n3 - 1:3 * n3 - 1]), {}, "d_out must not overlap"),
                               ((rgb, var, out), dict(variance_out=buf[3 * n3 - 1:3 * n3 - 1 + n1]), "d_variance_out must not overlap"),
                               ((rgb, var, out), dict(variance_out=buf[n3 - 1:n3 - 1 + n1]), "d_variance_out must not overlap"),
                               ((rgb, var, out), dict(params=P(iterations=9)), "iterations"),
                               ((rgb, var, out), dict(params=bad_flags), "flags"),
                               ((rgb, var, out), dict(params=P(sigma_color=nan)), "NaN")):
            with pytest.raises(hpt.HptError, match="hpt error 1:.*" + word):
                d.run_guided(*args, **kw)
        for args, kw, word in (((rgb, buf[1:1 + n3]), {}, "must not overlap"),
                               ((rgb, out), dict(length=buf[3 * n3 - 1:3 * n3 - 1 + n1]), "must not overlap"),
                               ((rgb, out), dict(params=P(sigma_normal=nan)), "NaN"),
                               ((rgb, out), dict(params=bad_flags), "flags")):
            with pytest.raises(hpt.HptError, match="hpt error 1:.*" + word):
                d.estimate_variance(*args, **kw)
        d.estimate_variance(rgb, out, params=P(iterations=99, sigma_color=nan))         # neither is read by the estimator
        torch.cuda.synchronize()
        back = buf.cpu().numpy()
        assert (back[:2 * n3] == f32(-7.25)).all() and (back[3 * n3:] == f32(-7.25)).all() and (back[2 * n3:3 * n3] != f32(-7.25)).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_chain_on_the_device_equals_the_chain_of_the_oracles(hpt, torch, sio, oracle_mod, tmp_path):
    """input.txt at 48 x 36, the cameras of the history's chain test (four frames from the scene's camera, one orbited by 2
    degrees): on the moved frame the mean is filtered under the spatial estimate divided by the history length."""
    import guides_oracle
    glib = guides_oracle.build(tmp_path)
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    # the oracles
    h = ho.History(W, H)
    want = []
    for f, cam in enumerate(cams):
        off = f * k["spp"]
        img, _ = oracle_mod.pt_render(L, sp, tr, cam, W, H, k["depth"], k["spp"], seed=k["seed"], sample_offset=off)
        moved = f == 0 or cam.tobytes() != cams[f - 1].tobytes()
        if moved:
            g, _ = guides_oracle.render(glib, L, sp, tr, cam, W, H, k["guide_spp"], seed=k["seed"], sample_offset=off)
        mean = h.advance(cam, img, *((g["normal"], g["position"], g["coverage"]) if moved else (None, None, None)))
        est = go.estimate_variance(img, g, h.n)
        out, v = go.run_guided(mean, est, g)
        want.append((img, h.n.copy(), est, out, v))
    # the device
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    local = torch.zeros((hpt.local_pixels(W, H, hpt.make_params()), 3), dtype=torch.float32, device="cuda")
    frame, mean, alb, nrm, pos, est, out = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(7))
    cov, length, vout = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    with hpt.Scene(L, sp, tr) as scene, hpt.History(W, H) as hist, hpt.Denoiser(W, H) as den:
        for f, cam in enumerate(cams):
            p = hpt.make_params(seed=k["seed"], sample_offset=f * k["spp"])
            moved = f == 0 or cam.tobytes() != cams[f - 1].tobytes()
            if moved:
                stream.synchronize()                             # the guide images are free: the last frame's filter has run
                scene.render_guides_device(cam, W, H, k["guide_spp"], p, albedo=alb, normal=nrm, position=pos, coverage=cov)
                den.set_guides(alb, nrm, pos, cov, stream=st)
            scene.render_pt_device(cam, W, H, k["depth"], k["spp"], p, local.data_ptr(), st)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, hpt.make_params(), st)
            hist.advance(cam, frame, *((nrm, pos, cov) if moved else (None, None, None)), mean_out=mean, stream=st)
            hist.length(length, stream=st)
            den.estimate_variance(frame, est, length, stream=st)
            den.run_guided(mean, est, out, vout, stream=st)
            stream.synchronize()
            w_img, w_n, w_est, w_out, w_v = want[f]
            assert frame.cpu().numpy().tobytes() == w_img.tobytes(), f
            assert length.cpu().numpy().tobytes() == w_n.tobytes(), f
            _same(est.cpu().numpy(), w_est, ("estimate", f))
            _same(out.cpu().numpy(), w_out, ("colour", f))
            _same(vout.cpu().numpy(), w_v, ("variance", f))
    assert (want[-1][1] == 1).any() and (want[-1][1] > 4).any()           # the moved frame holds restarted and kept pixels
    assert want[-1][3].tobytes() != want[-1][0].tobytes()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def _python_loop(hpt, torch, sio, scene_file, W, H, frames, spp, guide_spp, seed, orbit_deg, reproject):
    """pt_cli --frames --guided in Python: the filtered image of the last frame."""
    sc = sio.load_scene(scene_file)
    L, sp, tr = sio.flatten_for_pt(sc)
    cams = [sio.make_camera(hc.orbit_eye(sc.eye, sc.look_at, sc.view_up, f * orbit_deg), sc.look_at, sc.view_up, 50.0, W, H) if orbit_deg
            else sio.camera_for(sc, W, H, 50.0) for f in range(frames)]
    local = torch.zeros((hpt.local_pixels(W, H, hpt.make_params()), 3), dtype=torch.float32, device="cuda")
    frame, mean, alb, nrm, pos, var, out = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(7))
    cov, length = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(2))
    paths = set()
    with hpt.Scene(L, sp, tr) as scene, hpt.History(W, H) as hist, hpt.Accumulator(W, H, moments=True) as acc, hpt.Denoiser(W, H) as den:
        for f, cam in enumerate(cams):
            p = hpt.make_params(seed=seed, sample_offset=f * spp)
            moved = f > 0 and cam.tobytes() != cams[f - 1].tobytes()
            guides = f == 0 or moved
            if guides:
                torch.cuda.synchronize()
                scene.render_guides_device(cam, W, H, guide_spp, p, albedo=alb, normal=nrm, position=pos, coverage=cov)
                den.set_guides(alb, nrm, pos, cov)
            scene.render_pt_device(cam, W, H, 4, spp, p, local.data_ptr(), 0)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, hpt.make_params(), 0)
            if reproject:
                hist.advance(cam, frame, *((nrm, pos, cov) if guides else (None, None, None)), mean_out=mean)
                hist.length(length)
                den.estimate_variance(frame, var, length)
                paths.add("history")
            else:
                if moved:
                    acc.reset()
                acc.add(frame, mean)
                if acc.count >= 4:
                    acc.variance(var)
                    paths.add("moments")
                else:
                    length.fill_(float(acc.count))
                    den.estimate_variance(frame, var, length)
                    paths.add("estimate")
            den.run_guided(mean, var, out)
        torch.cuda.synchronize()
        return out.cpu().numpy(), mean.cpu().numpy(), paths


@pytest.mark.parametrize("reproject", [False, True], ids=["accumulate", "reproject"])
def test_cli_guided_writes_the_image_of_the_python_loop(tmp_path, hpt, torch, sio, reproject):
    from test_host_mirror import _decode_png
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    W, H, frames = 48, 36, 5
    png = str(tmp_path / "out.png")
    extra = ["--orbit", 2, "--reproject"] if reproject else []
    run = _cli("--mode", "pt", "--input", scene_file, "--seed", 13, "--width", W, "--height", H, "--frames", frames, "--frame-spp", 2,
               "--guided", "--guide-spp", 3, "--output", png, *extra)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    out, mean, paths = _python_loop(hpt, torch, sio, scene_file, W, H, frames, 2, 3, 13, 2.0 if reproject else 0.0, reproject)
    assert paths == ({"history"} if reproject else {"estimate", "moments"})
    shown = _decode_png(open(png, "rb").read())
    assert np.array_equal(shown, hpt.tonemap(out))
    assert not np.array_equal(shown, hpt.tonemap(mean))                     # the filtered mean, not the mean


def test_cli_guided_refusals(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    png = tmp_path / "x.png"
    run = _cli("--mode", "pt", "--input", scene_file, "--output", png, "--guided")
    assert run.returncode != 0 and "--guided needs --frames" in run.stderr
    run = _cli("--mode", "pt", "--input", scene_file, "--output", png, "--frames", 2, "--guided", "--guide-spp", 0)
    assert run.returncode != 0 and "--guide-spp of at least 1" in run.stderr
    assert not os.path.exists(png)
