"""The denoiser on the MI355X at the cases of denoise_cases.py, byte for byte against the oracle (tests/denoise_oracle.cpp):
deep levels whose taps of strides 32 to 128 take part, every level count, one-pixel-wide and tile-edge shapes, hostile
albedo, coverage, normals, positions and colours, sigmas whose inverse square is clamped or zero; all buffers as views of
one arena between sentinel bands (the kernels write their output and nothing else, at 4-byte alignment); outputs that
touch, or overlap by one float, the input; one denoiser across changing guides, level counts and flags; two denoisers
interleaved on one and on two streams; a NULL parameter record.
tests/test_denoise_cases_cpu.py keeps the oracle images of these cases from being indifferent to what they are about.

Wrong-value builds, one change each (never committed), and the tests here that fail on them; "old" is test_gpu_denoise.py:
   1  B3 taps 1/4 and 3/8 swapped          52 cases and every other test here; old: all comparisons
   2  stride k + 1 for 1 << k              38 cases, arena, overlap, state, defaults; old: all comparisons
   3  colour sigma not halved              33 cases, arena, overlap, state, defaults; old: all but one term-off case
   4  ping-pong index of k + 1 from k = 5  13 cases (6 or more levels), arena 257 x 9, the 8-1-8 state test; old: nothing
   5  bound qx > W for qx >= W             38 cases, arena, state, defaults; old: six tests (not the ragged images)
   6  the `others` rule dropped            7 cases (deep-70x65, levels 6 to 8 plain, three sigma cases), 8-1-8; old: tiny images
   7  albedo clamp 1e-4f                   albedo-edge on both paths; old: nothing
   8  invalid pixels re-modulated          12 demodulated cases with invalid pixels, both state tests; old: checkerboard, host call
   9  two squarings in the falloff         51 cases and every other test here; old: all comparisons
  10  the clamp of 1 / (s * s) removed     19 sigma cases on both paths; old: nothing
These were observed with the kernel bodies and the level loop compiled as host C++ behind the same C ABI (no device could
be reached when the file was written).  Change 5 reads one record past the buffers, so it belongs on such a build in any
case, with the read of the last row's neighbour left out."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_oracle

pytestmark = pytest.mark.gpu
KEYS = ("albedo", "normal", "position", "coverage")
SENTINEL = np.uint32(0x7FC0DEAD)          # a quiet NaN with a payload: no kernel computes it


@pytest.fixture(scope="module")
def dlib(tmp_path_factory):
    return denoise_oracle.build(tmp_path_factory.mktemp("denoise_oracle"))


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


_REF = {}


def _case(dlib, case):
    """(image, guides, kw, oracle image) of a case, computed once and read-only."""
    if case.name not in _REF:
        img, g, kw = case.make()
        ref = denoise_oracle.run(dlib, img, g, **kw)
        for a in [img, ref] + list(g.values()):
            a.flags.writeable = False
        _REF[case.name] = (img, g, kw, ref)
    return _REF[case.name]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()         # a copy: the cached cases are read-only


def _dev_guides(torch, g):
    return [_dev(torch, g[k]) for k in KEYS]


def _same(got, ref):
    got = np.ascontiguousarray(got)
    assert got.tobytes() == ref.tobytes(), "%d of %d pixels differ" % (
        int((got.reshape(-1, 3).view(np.uint32) != ref.reshape(-1, 3).view(np.uint32)).any(-1).sum()), ref.size // 3)


@pytest.mark.parametrize("case", dc.ALL, ids=[c.name for c in dc.ALL])
def test_case_on_the_device_path(hpt, torch, dlib, case):
    img, g, kw, ref = _case(dlib, case)
    H, W = img.shape[:2]
    dg, din = _dev_guides(torch, g), _dev(torch, img)
    dout = torch.full_like(din, float("nan"))
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        d.run(din, dout, hpt.make_denoise_params(**kw))
        torch.cuda.synchronize()
    _same(dout.cpu().numpy(), ref)
    assert din.cpu().numpy().tobytes() == img.tobytes()


@pytest.mark.parametrize("case", dc.HOST, ids=[c.name for c in dc.HOST])
def test_case_through_the_host_call(hpt, dlib, case):
    img, g, kw, ref = _case(dlib, case)
    _same(hpt.denoise(img, g, **kw), ref)


# ---- one arena ------------------------------------------------------------------------------------------------------
def _tiny_case():
    rng = np.random.default_rng(250)
    return dc.noisy(rng, 1, 1), denoise_oracle.random_guides(rng, 1, 1), dict(iterations=8)


ARENA = [dc.Case("arena-1x1", _tiny_case)] + [c for c in dc.ALL if c.name in ("shape-63x3", "shape-65x5", "deep-257x9-off")]
GUARDS = (37, 33, 35, 31, 34, 41, 39)     # floats before colour, output, albedo, normal, position, coverage, and after it


@pytest.mark.parametrize("case", ARENA, ids=[c.name for c in ARENA])
def test_views_of_one_arena_between_sentinel_bands(hpt, torch, dlib, case):
    """Every address the kernels may touch lies inside one tensor; only the output's floats may change."""
    img, g, kw, ref = _case(dlib, case)
    H, W = img.shape[:2]
    parts = [img, np.empty_like(img)] + [g[k] for k in KEYS]
    offs, at = [], 0
    for guard, a in zip(GUARDS, parts):
        at += guard
        offs.append(at)
        at += a.size
    total = at + GUARDS[-1]
    host = np.full(total, SENTINEL, np.uint32)
    for k, (o, a) in enumerate(zip(offs, parts)):
        if k != 1:
            host[o: o + a.size] = np.ascontiguousarray(a).reshape(-1).view(np.uint32)
    assert offs[0] % 4 and sum(1 for o in offs if o % 4) >= 2                  # 4-byte alignment only
    arena = torch.from_numpy(host.view(np.float32).copy()).cuda()
    v = [arena[o: o + a.size] for o, a in zip(offs, parts)]
    base, end = arena.data_ptr(), arena.data_ptr() + total * 4
    assert all(base < t.data_ptr() and t.data_ptr() + t.numel() * 4 < end for t in v)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*v[2:])
        d.run(v[0], v[1], hpt.make_denoise_params(**kw))
        torch.cuda.synchronize()
    back = arena.cpu().numpy().view(np.uint32)
    want = host.copy()
    want[offs[1]: offs[1] + ref.size] = ref.reshape(-1).view(np.uint32)
    _same(back[offs[1]: offs[1] + ref.size].view(np.float32), ref)
    wrong = np.nonzero(back != want)[0]
    assert wrong.size == 0, ("floats outside the output changed", wrong[:8].tolist(), offs)


# ---- overlap --------------------------------------------------------------------------------------------------------
def test_outputs_that_overlap_by_one_float_or_touch(hpt, torch, dlib):
    rng = np.random.default_rng(251)
    W, H = 16, 8
    n3 = W * H * 3
    g = denoise_oracle.random_guides(rng, W, H)
    img = dc.noisy(rng, W, H)
    ref = denoise_oracle.run(dlib, img, g)
    buf = torch.zeros(3 * n3, dtype=torch.float32, device="cuda")
    din = buf[n3: 2 * n3]
    din.copy_(_dev(torch, img).reshape(-1))
    dg = _dev_guides(torch, g)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for start in (n3 + 1, 2 * n3 - 1, 1, n3 - 1):          # inside on either side; one float short of clear, above and below
            with pytest.raises(hpt.HptError, match="overlap"):
                d.run(din, buf[start: start + n3])
        torch.cuda.synchronize()
        assert not buf[:n3].any() and not buf[2 * n3:].any()                     # a rejected run writes nothing
        for start in (2 * n3, 0):                             # the output begins where the input ends, and the reverse
            d.run(din, buf[start: start + n3])
            torch.cuda.synchronize()
            _same(buf[start: start + n3].cpu().numpy().reshape(H, W, 3), ref)
            assert din.cpu().numpy().tobytes() == img.tobytes()


# ---- state ----------------------------------------------------------------------------------------------------------
def test_guides_set_again_on_one_denoiser(hpt, torch, dlib):
    rng = np.random.default_rng(252)
    W, H = 45, 33
    ga = denoise_oracle.random_guides(rng, W, H, invalid=rng.uniform(size=(H, W)) < 0.1)
    gb = dc.smooth_guides(rng, W, H, rng.uniform(size=(H, W)) < 0.1)
    img = dc.noisy(rng, W, H)
    kw = dict(iterations=4, sigma_color=2.0)
    ra, rb = denoise_oracle.run(dlib, img, ga, **kw), denoise_oracle.run(dlib, img, gb, **kw)
    assert ra.tobytes() != rb.tobytes()
    da, db, din = _dev_guides(torch, ga), _dev_guides(torch, gb), _dev(torch, img)
    with hpt.Denoiser(W, H) as d:
        for dg, ref in ((da, ra), (db, rb), (da, ra)):
            dout = torch.full_like(din, float("nan"))
            d.set_guides(*dg)
            d.run(din, dout, hpt.make_denoise_params(**kw))
            torch.cuda.synchronize()
            _same(dout.cpu().numpy(), ref)


def test_level_counts_and_flags_change_on_one_denoiser(hpt, torch, dlib):
    """8 levels, 1, 8; demodulated, not, demodulated (and 1 level undemodulated): a stale ping-pong or albedo buffer shows."""
    by_name = {c.name: c for c in dc.LEVELS}
    order = ["levels-8-demod", "levels-1-demod", "levels-8-demod", "levels-8-plain", "levels-8-demod", "levels-1-plain", "levels-7-demod"]
    img, g, _, _ = _case(dlib, by_name[order[0]])
    H, W = img.shape[:2]
    dg, din = _dev_guides(torch, g), _dev(torch, img)
    with hpt.Denoiser(W, H) as d:
        d.set_guides(*dg)
        for name in order:
            img2, _, kw, ref = _case(dlib, by_name[name])
            assert img2.tobytes() == img.tobytes()
            dout = torch.full_like(din, float("nan"))
            d.run(din, dout, hpt.make_denoise_params(**kw))
            torch.cuda.synchronize()
            _same(dout.cpu().numpy(), ref)


@pytest.mark.parametrize("streams", [1, 2])
def test_two_denoisers_alive_and_interleaved(hpt, torch, dlib, streams):
    rng = np.random.default_rng(253)
    sizes = ((33, 17), (70, 20))
    g = [denoise_oracle.random_guides(rng, W, H) for W, H in sizes]
    imgs = [[dc.noisy(rng, W, H), dc.noisy(rng, W, H) * np.float32(3)] for W, H in sizes]
    kw = [dict(iterations=5), dict(iterations=4, demodulate=False)]
    refs = [[denoise_oracle.run(dlib, f, g[k], **kw[k]) for f in imgs[k]] for k in range(2)]
    dg = [_dev_guides(torch, g[k]) for k in range(2)]
    din = [[_dev(torch, f) for f in imgs[k]] for k in range(2)]
    dout = [[torch.full_like(t, float("nan")) for t in din[k]] for k in range(2)]
    torch.cuda.synchronize()
    st = [torch.cuda.Stream() for _ in range(streams)]
    st = [st[0], st[-1]]
    with hpt.Denoiser(*sizes[0]) as d0, hpt.Denoiser(*sizes[1]) as d1:
        den = (d0, d1)
        for k in range(2):
            den[k].set_guides(*dg[k], stream=st[k].cuda_stream)
        for frame in range(2):
            for k in range(2):
                den[k].run(din[k][frame], dout[k][frame], hpt.make_denoise_params(**kw[k]), stream=st[k].cuda_stream)
        for s in st:
            s.synchronize()
        for k in range(2):
            for frame in range(2):
                _same(dout[k][frame].cpu().numpy(), refs[k][frame])


# ---- defaults -------------------------------------------------------------------------------------------------------
def test_null_parameters_are_the_zero_record_are_the_defaults(hpt, dlib):
    rng = np.random.default_rng(254)
    W, H = 37, 21
    g = denoise_oracle.random_guides(rng, W, H, invalid=rng.uniform(size=(H, W)) < 0.1)
    img = dc.noisy(rng, W, H)
    lib = hpt.load_library()
    ptr = [np.ascontiguousarray(a).ctypes.data_as(C.c_void_p) for a in [img] + [g[k] for k in KEYS]]
    outs = []
    for p in (None, C.byref(hpt.DenoiseParams())):
        out = np.full((H, W, 3), np.nan, np.float32)
        assert lib.hpt_denoise_host(*ptr, out.ctypes.data_as(C.c_void_p), W, H, p) == 0
        outs.append(out)
    ref = denoise_oracle.run(dlib, img, g, iterations=5, sigma_color=1.0, sigma_normal=0.5, sigma_position=0.05, demodulate=False)
    _same(outs[0], ref)
    _same(outs[1], ref)
    assert ref.tobytes() == denoise_oracle.run(dlib, img, g, demodulate=False).tobytes() != img.tobytes()
