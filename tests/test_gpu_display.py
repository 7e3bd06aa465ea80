"""The progressive display on the MI355X: hpt_accum_* and hpt_display_* against the numpy oracle (tests/display_oracle.py),
byte for byte and integer for integer -- no tolerance anywhere.  Shapes and frames come from tests/display_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_cases as dc
import display_oracle as do
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
f32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


# ---- accumulator -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", dc.ACCUM_COUNTS)
@pytest.mark.parametrize("size", dc.ACCUM_SIZES)
def test_add_mean_variance_read(hpt, torch, size, K):
    W, H = size
    frames = dc.accum_frames(W, H, K)
    ref = do.Accum(W, H, moments=True)
    with hpt.Accumulator(W, H, moments=True) as acc:
        assert acc.count == 0
        for k, f in enumerate(frames):
            want = ref.add(f)
            mean = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
            acc.add(_dev(torch, f), mean_out=mean if k % 2 == 0 or k == K - 1 else None)      # both mean-out instances
            if k % 2 == 0 or k == K - 1:
                assert _same(mean, want), (k, float(np.abs(mean.cpu().numpy() - want).max()))
        assert acc.count == K
        got = acc.read()
        assert got["count"] == K and _same(got["sum"], ref.sum) and _same(got["sumsq"], ref.sq)
        out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        acc.mean(out)
        assert _same(out, ref.mean())
        out.fill_(-7.0)
        acc.variance(out)
        assert _same(out, ref.variance())
        if K == 1:
            assert not out.cpu().numpy().any()
        elif W * H > 1:
            assert (out.cpu().numpy() > 0).any()


def test_without_moments_and_in_place_mean_out(hpt, torch):
    W, H = 67, 3
    frames = dc.accum_frames(W, H, 3, seed=1)
    ref = do.Accum(W, H)
    with hpt.Accumulator(W, H) as acc:
        for f in frames:
            want = ref.add(f)
            d = _dev(torch, f)
            acc.add(d, mean_out=d)                  # in place
            assert _same(d, want)
        got = acc.read()
        assert got["sumsq"] is None and _same(got["sum"], ref.sum)


@pytest.mark.parametrize("size", [(5, 3), (67, 3)])
def test_pointers_offset_by_one_float_take_the_scalar_path(hpt, torch, size):
    W, H = size
    n = W * H * 3
    frames = dc.accum_frames(W, H, 3, seed=2)
    ref = do.Accum(W, H, moments=True)
    with hpt.Accumulator(W, H, moments=True) as acc:
        for k, f in enumerate(frames):
            want = ref.add(f)
            src = torch.full((n + 9,), 99.0, dtype=torch.float32, device="cuda")
            dst = torch.full((n + 9,), -7.0, dtype=torch.float32, device="cuda")
            src[1:1 + n] = _dev(torch, f.reshape(-1))
            assert src[1:].data_ptr() % 16 == 4
            # frame unaligned; then mean-out unaligned only; then both
            a, b = (src[1:1 + n], dst[4:4 + n]) if k == 0 else (src[1:1 + n].clone(), dst[1:1 + n]) if k == 1 else (src[1:1 + n], dst[1:1 + n])
            lo = 4 if k == 0 else 1
            acc.add(a, mean_out=b)
            got = dst.cpu().numpy()
            assert _same(got[lo:lo + n], want.reshape(-1))
            assert (got[:lo] == -7.0).all() and (got[lo + n:] == -7.0).all()
        out = torch.full((n + 9,), -7.0, dtype=torch.float32, device="cuda")
        acc.variance(out[1:1 + n])
        got = out.cpu().numpy()
        assert _same(got[1:1 + n], ref.variance().reshape(-1)) and got[0] == -7.0 and (got[1 + n:] == -7.0).all()
        g = acc.read()
        assert _same(g["sum"], ref.sum) and _same(g["sumsq"], ref.sq)


def test_constant_frames_have_variance_exactly_zero(hpt, torch):
    W, H = 5, 3
    f = dc.accum_frames(W, H, 1, seed=3)[0]
    with hpt.Accumulator(W, H, moments=True) as acc:
        for _ in range(4):                          # sums of 1, 2 and 4 equal terms are exact; so are their quotients
            acc.add(_dev(torch, f))
        out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        acc.variance(out)
        ref = do.Accum(W, H, moments=True)
        for _ in range(4):
            ref.add(f)
        assert _same(out, ref.variance()) and not out.cpu().numpy().any()


def test_reset_then_the_same_frames_is_a_fresh_accumulator(hpt, torch):
    W, H = 67, 3
    frames = dc.accum_frames(W, H, 3, seed=4)
    with hpt.Accumulator(W, H, moments=True) as acc, hpt.Accumulator(W, H, moments=True) as fresh:
        acc.add(_dev(torch, frames[2] * f32(5)))
        acc.add(_dev(torch, frames[1]))
        acc.reset()
        assert acc.count == 0
        with pytest.raises(hpt.HptError, match="hpt error 1:"):
            acc.mean(torch.empty((H, W, 3), dtype=torch.float32, device="cuda"))
        means = []
        for a in (acc, fresh):
            m = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            for f in frames:
                a.add(_dev(torch, f), mean_out=m)
            means.append(m.cpu().numpy())
        x, y = acc.read(), fresh.read()
        assert x["count"] == y["count"] == 3
        assert _same(x["sum"], y["sum"]) and _same(x["sumsq"], y["sumsq"]) and _same(means[0], means[1])
        ref = do.Accum(W, H, moments=True)
        for f in frames:
            ref.add(f)
        assert _same(x["sum"], ref.sum)


def test_two_accumulators_interleaved_on_one_stream(hpt, torch):
    W, H = 67, 3
    fa, fb = dc.accum_frames(W, H, 3, seed=5), dc.accum_frames(W, H, 3, seed=6)
    ra, rb = do.Accum(W, H, moments=True), do.Accum(W, H)
    da, db = [_dev(torch, f) for f in fa], [_dev(torch, f) for f in fb]
    ma = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    mb = torch.empty_like(ma)
    va = torch.empty_like(ma)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with hpt.Accumulator(W, H, moments=True) as a, hpt.Accumulator(W, H) as b:
        for k in range(3):
            a.add(da[k], mean_out=ma, stream=stream.cuda_stream)
            b.add(db[k], mean_out=mb, stream=stream.cuda_stream)
            wa, wb = ra.add(fa[k]), rb.add(fb[k])
        a.variance(va, stream=stream.cuda_stream)
        stream.synchronize()
        assert _same(ma, wa) and _same(mb, wb) and _same(va, ra.variance())
        assert _same(a.read()["sum"], ra.sum) and _same(b.read()["sum"], rb.sum)


def test_accumulator_refusals_on_a_live_object(hpt, torch):
    lib = hpt.load_library()
    W, H = 5, 3
    n = W * H * 3
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    with hpt.Accumulator(W, H) as acc, hpt.Accumulator(W, H, moments=True) as mom:
        for call in (lambda: acc.variance(buf),                         # no MOMENTS
                     lambda: acc.mean(buf),                             # K = 0
                     lambda: acc.add(buf[:n], mean_out=buf[1:1 + n]),   # overlap that is not in place
                     lambda: acc.add(buf[4:4 + n], mean_out=buf[:n])):
            with pytest.raises(hpt.HptError, match="hpt error 1:"):
                call()
        assert lib.hpt_accum_add(acc._h, None, None, None) == 1 and b"null frame" in lib.hpt_last_error()
        assert lib.hpt_accum_mean(mom._h, None, None) == 1 and lib.hpt_accum_variance(mom._h, None, None) == 1
        host = np.zeros(n, f32)
        assert lib.hpt_accum_read(acc._h, None, host.ctypes.data_as(C.c_void_p), None) == 1
        assert acc.count == 0 and mom.count == 0                        # a refused call enqueues and counts nothing
        torch.cuda.synchronize()
        assert not acc.read()["sum"].any()


# ---- present ---------------------------------------------------------------------------------------------------------------

def _present_case(hpt, torch, c, bgr, flip, stream=0):
    """Every frame of the case on one display, pitch 0, into a view one byte into a sentinel-filled tensor."""
    W, H = c["W"], c["H"]
    n = W * H * 3
    ref = do.Display(W, H)
    seen = []
    with hpt.Display(W, H) as d:
        for k, f in enumerate(c["frames"]()):
            big = torch.full((n + 9,), dc.SENTINEL, dtype=torch.uint8, device="cuda")
            want = np.full(n + 9, dc.SENTINEL, np.uint8)
            s_prev, _ = ref.present(f, out=want[1:1 + n], bgr=bgr, flip_y=flip)
            lin = _dev(torch, f)
            torch.cuda.synchronize()                # the sentinel fill ran on torch's stream
            d.present(lin, out=big[1:], bgr=bgr, flip_y=flip, stream=stream)
            m = d.metrics()
            assert _same(big, want), (k, int((big.cpu().numpy() != want).sum()))
            assert (m["ssd_prev"], m["ssd_other"], m["presented"]) == (s_prev, 0, k + 1), (k, m, s_prev)
            assert m["rms_prev"] == do.rms(s_prev) and m["rms_other"] == 0.0
            if k == 0:
                assert m["ssd_prev"] == 0
            seen.append(m["ssd_prev"])
    return seen


@pytest.mark.parametrize("flags", dc.FLAG_COMBOS)
@pytest.mark.parametrize("size", dc.PRESENT_SIZES)
def test_present_bytes_and_metrics(hpt, torch, size, flags):
    seen = _present_case(hpt, torch, dc.case("%dx%d" % size), *flags)
    assert all(s > 0 for s in seen[1:])


@pytest.mark.parametrize("size", [(3, 2), (50, 37), (65, 5), (64, 4)])
def test_three_panels_of_one_framebuffer_from_three_streams(hpt, torch, size):
    """pitch = 9 W, x_offset = panel * 3 W, flipped BGR like the reference's framebuffer (main.cpp:431-437); the buffer
    starts one byte into its tensor, so with odd W every panel edge falls inside a word.  Panel 1 is compared with panel 0."""
    W, H = size
    pitch = 9 * W
    total = H * pitch
    frames = [dc.present_frames(W, H, 2, seed=10 + p) for p in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    refs = [do.Display(W, H) for _ in range(3)]
    disp = [hpt.Display(W, H) for _ in range(3)]
    try:
        for k in range(2):
            big = torch.full((total + 9,), dc.SENTINEL, dtype=torch.uint8, device="cuda")
            want = np.full(total + 9, dc.SENTINEL, np.uint8)
            lin = [_dev(torch, frames[p][k]) for p in range(3)]
            torch.cuda.synchronize()
            exp = []
            for p in (0, 2, 1):                                         # panel 1 reads panel 0's `last`: present 0 first and wait
                other = 0 if p == 1 else None
                exp.append((p, refs[p].present(frames[p][k], other=refs[0] if p == 1 else None, out=want[1:1 + total], pitch=pitch,
                                               x_offset=3 * W * p, bgr=True, flip_y=True)))
                disp[p].present(lin[p], out=big[1:], other=disp[0] if other is not None else None, pitch=pitch, x_offset=3 * W * p,
                                bgr=True, flip_y=True, stream=streams[p].cuda_stream)
                if p == 0:
                    streams[0].synchronize()                            # the caller orders the two displays' work
            for p, (s_prev, s_other) in exp:
                m = disp[p].metrics()
                assert (m["ssd_prev"], m["ssd_other"], m["presented"]) == (s_prev, s_other, k + 1), (p, k)
                if p == 1:
                    assert s_other > 0 and m["rms_other"] == do.rms(s_other)
            torch.cuda.synchronize()
            assert _same(big, want)
    finally:
        for d in disp:
            d.close()


def test_no_output_buffer_keeps_last_and_metrics(hpt, torch):
    W, H = 65, 5
    a, b = dc.present_frames(W, H, 2, seed=20)
    with hpt.Display(W, H) as d:
        d.present(_dev(torch, a))
        d.present(_dev(torch, b))
        assert d.metrics()["ssd_prev"] == do.ssd(do.tone_bytes(a), do.tone_bytes(b)) > 0


def test_other_equal_images_give_zero_and_different_the_oracle_sum(hpt, torch):
    W, H = 50, 37
    a, b = dc.present_frames(W, H, 2, seed=21)
    ba, bb = do.tone_bytes(a), do.tone_bytes(b)
    with hpt.Display(W, H) as x, hpt.Display(W, H) as y:
        x.present(_dev(torch, a))
        y.present(_dev(torch, a), other=x, bgr=True, flip_y=True)      # flags do not reach `last`
        m = y.metrics()
        assert (m["ssd_prev"], m["ssd_other"], m["rms_other"]) == (0, 0, 0.0)
        y.present(_dev(torch, b), other=x)
        m = y.metrics()
        assert m["ssd_other"] == m["ssd_prev"] == do.ssd(ba, bb) > 0
        x.present(_dev(torch, b), other=y)
        m = x.metrics()
        assert m["ssd_other"] == 0 and m["ssd_prev"] == do.ssd(ba, bb)


def test_display_refusals_on_a_live_object(hpt, torch):
    lib = hpt.load_library()
    W, H = 5, 3
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    out = torch.full((H * 64,), dc.SENTINEL, dtype=torch.uint8, device="cuda")
    with hpt.Display(W, H) as d, hpt.Display(W, H) as never, hpt.Display(W + 1, H) as wide:
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            d.metrics()
        wide.present(torch.zeros((H, W + 1, 3), dtype=torch.float32, device="cuda"))
        for kw, word in ((dict(other=never), "not presented"), (dict(other=wide), "another size"), (dict(other=d), "different display"),
                         (dict(out=out, pitch=3 * W - 1), "pitch"), (dict(out=out, pitch=3 * W + 2, x_offset=3), "pitch"),
                         (dict(out=out, x_offset=1), "pitch"), (dict(out=out, pitch=64, x_offset=-1), "x_offset")):
            with pytest.raises(hpt.HptError, match="hpt error 1:.*" + word):
                d.present(lin, **kw)
        assert lib.hpt_display_present(d._h, None, None, None, C.c_int64(0), C.c_int64(0), 0, None) == 1
        assert lib.hpt_display_present(d._h, C.c_void_p(lin.data_ptr()), None, None, C.c_int64(0), C.c_int64(0), 4, None) == 1
        assert b"HPT_DISPLAY_BGR" in lib.hpt_last_error()
        with pytest.raises(hpt.HptError):
            d.metrics()                                                 # nothing was presented by the refused calls
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == dc.SENTINEL).all()
        d.present(lin, out=out, pitch=3 * W + 2, x_offset=2)           # the tightest legal panel
        assert d.metrics()["presented"] == 1
        d.reset()
        with pytest.raises(hpt.HptError):
            d.metrics()
        d.present(lin)
        assert d.metrics() == dict(rms_prev=0.0, rms_other=0.0, ssd_prev=0, ssd_other=0, presented=1)


def test_black_then_white_needs_more_than_32_bits(hpt, torch):
    seen = _present_case(hpt, torch, dc.case("black_white_256x96"), False, False)
    assert seen == [0, dc.BLACK_WHITE_SSD] and dc.BLACK_WHITE_SSD > 2 ** 32


def test_the_same_two_images_twice_give_the_same_integers(hpt, torch):
    c = dc.case("repeat_33x9")                                          # a, b, b, a
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first = _present_case(hpt, torch, c, True, False, stream=stream.cuda_stream)
    second = _present_case(hpt, torch, c, False, True)
    assert first == second and first[2] == 0 and first[1] == first[3] > 0


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _frame_loop(hpt, torch, scene, cam, W, H, mode, frames=3, spp=2, seed=17):
    """render_*_device, untile, Accumulator.add(mean_out), Display.present on one stream: per frame (mean, bytes, ssd_prev)."""
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    n_local = hpt.local_pixels(W, H, hpt.make_params())
    local = torch.zeros((n_local, 3), dtype=torch.float32, device="cuda")
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    mean = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = []
    with hpt.Accumulator(W, H) as acc, hpt.Display(W, H) as disp:
        for f in range(frames):
            p = hpt.make_params(seed=seed, sample_offset=f * spp)
            if mode == "pt":
                scene.render_pt_device(cam, W, H, 4, spp, p, local.data_ptr(), st)
            else:
                scene.render_bdpt_device(cam, W, H, 4, 4, spp, 4, p, local.data_ptr(), st)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, hpt.make_params(), st)
            acc.add(frame, mean_out=mean, stream=st)
            disp.present(mean, out=rgb8, stream=st)
            m = disp.metrics()                                          # waits for this frame's present
            stream.synchronize()
            out.append((mean.cpu().numpy(), rgb8.cpu().numpy(), m["ssd_prev"], m["rms_prev"]))
    return out


def _oracle_loop(frames, W, H):
    acc, disp = do.Accum(W, H), do.Display(W, H)
    out = []
    for f in frames:
        mean = acc.add(f)
        s_prev, _ = disp.present(mean)
        out.append((mean, disp.last, s_prev, do.rms(s_prev)))
    return out


@pytest.mark.parametrize("mode", ["pt", "bdpt"])
def test_end_to_end_frame_loop(hpt, torch, sio, input_scene, mode):
    sc, (L, sp, tr) = input_scene
    W, H = 50, 37
    cam = sio.camera_for(sc, W, H)
    with hpt.Scene(L, sp, tr) as scene:
        got = _frame_loop(hpt, torch, scene, cam, W, H, mode)
        host = []
        for f in range(3):
            p = hpt.make_params(seed=17, sample_offset=2 * f)
            host.append(scene.render_pt(cam, W, H, 4, 2, p) if mode == "pt" else scene.render_bdpt(cam, W, H, 4, 4, 2, 4, p))
    want = _oracle_loop(host, W, H)
    assert host[0].tobytes() != host[1].tobytes() and want[1][2] > 0 and want[2][2] > 0
    for f in range(3):
        assert _same(got[f][0], want[f][0]), f
        assert _same(got[f][1], want[f][1]), f
        assert got[f][2] == want[f][2] and got[f][3] == want[f][3], f


# ---- CLI ---------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("mode", ["pt", "ppm"])
def test_cli_frames(tmp_path, hpt, torch, sio, mode):
    from test_host_mirror import _decode_png
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    W, H = 40, 32
    png, log = str(tmp_path / "out.png"), str(tmp_path / "rms.txt")
    base = ["--mode", mode, "--input", scene_file, "--seed", 13, "--width", W, "--height", H, "--spl", 64, "--frame-spp", 2]
    run = _cli(*base, "--frames", 3, "--output", png, "--rms-log", log)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    sc = sio.load_scene(scene_file)
    L, sp, tr = sio.flatten_for_pt(sc)
    cam = sio.camera_for(sc, W, H, 50.0)
    with hpt.Scene(L, sp, tr) as s:
        frames = []
        for f in range(3):
            p = hpt.make_params(seed=13, sample_offset=2 * f)
            frames.append(s.render_pt(cam, W, H, 4, 2, p) if mode == "pt" else s.render_ppm(cam, W, H, 4, 4, 2, 64, params=p))
    want = _oracle_loop(frames, W, H)
    assert np.array_equal(_decode_png(open(png, "rb").read()), want[2][1])
    assert want[2][1].tobytes() == do.tone_bytes(want[2][0]).tobytes() and want[2][0].max() > 0
    # the Python pipeline on the same frames gives the log's numbers
    py = []
    with hpt.Accumulator(W, H) as acc, hpt.Display(W, H) as disp:
        mean = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for f in frames:
            acc.add(_dev(torch, f), mean_out=mean)
            disp.present(mean)
            py.append(disp.metrics()["rms_prev"])
    assert py == [w[3] for w in want] and py[0] == 0.0 and py[1] > 0 and py[2] > 0
    assert open(log).read() == "".join("%d %.9g\n" % (k + 1, r) for k, r in enumerate(py))
    # an early stop: frame 2 is the first that may end the loop
    run = _cli(*base, "--frames", 3, "--output", png, "--rms-log", log, "--until-rms", 1e9)
    assert run.returncode == 0, run.stderr
    assert open(log).read() == "".join("%d %.9g\n" % (k + 1, r) for k, r in enumerate(py[:2]))
    assert np.array_equal(_decode_png(open(png, "rb").read()), want[1][1])


def test_cli_refuses_frames_for_sppm_and_several_devices(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    run = _cli("--mode", "sppm", "--frames", 2, "--input", scene_file, "--output", tmp_path / "x.png")
    assert run.returncode != 0 and "--frames does not apply to --mode sppm" in run.stderr
    run = _cli("--mode", "pt", "--frames", 2, "--gpus", 2, "--input", scene_file, "--output", tmp_path / "x.png")
    assert run.returncode != 0 and "--gpus" in run.stderr
    assert not os.path.exists(tmp_path / "x.png")
