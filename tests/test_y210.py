"""10-bit packed 4:2:2 frames (MM_Y210, both ranges, the matrix bits) through
the C-ABI on the HIP path.

A frame is the RGBA32F frame of its decode (include/mm.h), so the reference is
the existing oracle on y210.decode(frame, float32), encoded by y210.encode:
tests/y210.py holds the definitions, in float64 numpy.

The bar is tests/test_p010.py's, on the luma words and the chroma words apart:
every word differs by 0 or 64 (one 10-bit code), the low 6 bits of every output
word are zero, and at most 4 * mmtest.U8_FRAC = 4e-3 of the words differ (a
10-bit code is a quarter of an 8-bit one, so four times as many roundings can
fall the other way).  The first frame is bitwise the input, and on every later
frame more than 0.5 of the luma codes and more than 0.3 of the chroma codes
differ from the input.

Reference noise under this comparison (the fp32 oracle against the float64 twin
np_twin.process_frame, both encoded, on exactly the inputs below, measured on
the CPU; worst frame of each case; fractions of the words that differ, all by
one code):
  case (W x H, frames, matrix / range, stress, low bits, edge)   luma             chroma
  64 x 48, 4, 709                                                  3.3e-4           0
  200 x 120, 4, 709                                                1.7e-4           0
  200 x 120, 4, 601 full, stress, low bits                         2.1e-4           4.2e-5
  200 x 120, 4, 2020, stress                                       2.1e-4           8.3e-5
  98 x 62, 4, 709, low bits                                        1.7e-4           0
  128 x 128, 4, 709, stress, repeat / clamp                        2.4e-4 / 1.2e-4  0
  128 x 128, 4, 601, stress, low bits, clamp                       1.2e-4           0
  136 x 520, 5, 601, stress, low bits, repeat                      3.1e-4           1.1e-4
  136 x 520, 5, 709, stress, clamp                                 3.4e-4           1.3e-4
  136 x 518, 5, 601, stress, clamp                                 2.4e-4           7.1e-5
  136 x 518, 5, 709, stress, low bits, repeat                      3.0e-4           7.1e-5
  96 x 64, 4, 709, standard mode                                   6.5e-4           0
  1920 x 128, 3, 709                                               3.2e-4           9.0e-5
every case below one sixth of the cap, so the cap is a condition on the
kernels, not on the reference's own noise; the reference itself moves at least
0.995 of the luma codes and at least 0.95 of the chroma codes.
The kernels themselves, on the MI355X, every case and call form of this module:
against the oracle in pyramid mode at most 3.4e-4 of a frame's luma words and
1.2e-4 of its chroma words differ from the reference (1920 x 128: 3.1e-4 and
3.3e-5), in standard mode 2.1e-3 of the luma words on the first magnified frame
(4.9e-4 and 3.3e-4 on the next two) and no chroma word, against the encoded
RGBA32F path in steerable mode 6.1e-5 and 8.1e-5; each by one code.  The
matrixed K1 state is within 7.6e-6 of its decoded frame's (bar 6.4e-4, the
BT.601 reading 4.7 to 9.0 away); a YUY2 frame in the high bytes gives the YUY2
frame's state exactly.

Kernel forms reached (tests/test_yuv422.py's shapes, for the same reasons): K1
one-pair (LAT) form in frame calls and short streams; 136 x 520, N = 1024, 260
row pairs x 5 frames in one launch the batch form with six shared rows;
136 x 518, 259 pairs, the regular four-row form; each in the luma-only (BT.601)
and the matrixed instance.  Compose: k_rows_inv_compose4 at 200 x 120, the
walking fused kernel with MM_K34_ROWS, the unfused pair at 64 x 48 (x0 = 0),
98 x 62 (W % 8 != 0) and for one-frame calls at N = 2048.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmtest as T
import oracle_py as O
import surface as SF
import y210
import yuv422

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
FRAC = 4 * T.U8_FRAC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")

# (matrix, full range)
V709 = (709, False)
V601 = (601, False)
V601_FULL = (601, True)
V2020 = (2020, False)
V2020_FULL = (2020, True)


@functools.lru_cache(maxsize=None)
def _frames(W, H, n, v=V709, stress=False, lowbits=False):
    out = []
    rng = np.random.default_rng(16)
    for t, rgb in enumerate(T.synth(W, H, n, fmt="u8")):
        buf = y210.encode(rgb, *v)
        if stress:
            buf = y210.chroma_stress(buf, t)
        if lowbits:     # Y216-style content: the low 6 bits carry signal
            buf = y210.low_bits(buf, rng)
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, v=V709, stress=False, lowbits=False, edge=0, std=False):
    """The oracle on the decoded frames, encoded (computed once per case)."""
    fr = [y210.decode(b, np.float32, *v) for b in _frames(W, H, n, v, stress, lowbits)]
    ref = T.oracle_run(W, H, fr, L, S, edge, standard={} if std else None)
    return tuple(y210.encode(r, *v) for r in ref)


def _run(W, H, frames, *a, **kw):
    """T.gpu_run on uint16 frames [H][2 W], moved as their bytes."""
    got = T.gpu_run(W, H, [np.ascontiguousarray(f).view(np.uint8) for f in frames], *a, **kw)
    return [np.ascontiguousarray(g).view(np.uint16) for g in got]


def _planes(buf):
    y, cb, cr = y210.split(buf)
    return y, np.stack([cb, cr])


def _bar(got, ref, what=""):
    """The bar of the module docstring on one frame."""
    assert got.dtype == np.uint16 and got.shape == ref.shape
    assert not np.any(got & 63), "low 6 bits of every output word are zero"
    fr = []
    for name, g, r in zip(("luma", "chroma"), _planes(got), _planes(ref)):
        d = np.abs(g.astype(np.int32) - r.astype(np.int32))
        fr.append((name, int(d.max()), float((d > 0).mean())))
    print(f"{what}: " + "  ".join(f"{n} max {m} frac {f:.2e}" for n, m, f in fr))
    for name, m, f in fr:
        assert m in (0, 64), (what, name, m)
        assert f <= FRAC, (what, name, f)


def _check(got, frames, ref):
    assert np.array_equal(got[0], frames[0]), "first frame passes through bitwise"
    for k in range(1, len(frames)):
        _bar(got[k], ref[k], f"frame {k}")
        # not a passthrough nor a chroma copy: the operator moved luma and chroma
        (gy, gc), (iy, ic) = _planes(got[k]), _planes(frames[k])
        assert ((gy >> 6) != (iy >> 6)).mean() > 0.5
        assert ((gc >> 6) != (ic >> 6)).mean() > 0.3


# W, H, frames, (matrix, range), chroma stress, low bits, edge, MM_K34_ROWS and batch of the stream leg
CASES = [
    (64, 48, 4, V709, False, False, 0, None),         # K1 one-pair form; x0 = 0: unfused K3 -> K4
    (200, 120, 4, V709, False, False, 0, None),       # N = 256: k_rows_inv_compose4
    (200, 120, 4, V601_FULL, True, True, 0, None),
    (200, 120, 4, V2020, True, False, 0, None),
    (200, 120, 12, V709, False, False, 0, "64"),      # the walking fused K34, batch 12
    (98, 62, 4, V709, False, True, 0, None),          # W % 8 != 0: unfused; rows of 49 macropixels
    (128, 128, 4, V709, True, False, 0, None),        # N = W = H: every border column and row wraps ...
    (128, 128, 4, V709, True, False, 1, None),        # ... or clamps, then halves onto the macropixels
    (128, 128, 4, V601, True, True, 1, None),
    (136, 520, 5, V601, True, True, 0, None),         # N = 1024, 5 x 260 pairs in one launch: K1 batch form
    (136, 520, 5, V709, True, False, 1, None),
    (136, 518, 5, V601, True, False, 1, None),        # 259 pairs per frame: K1 regular four-row form
    (136, 518, 5, V709, True, True, 0, None),
]


@pytest.mark.parametrize("W,H,n,v,stress,lowbits,edge,rows", CASES)
def test_y210_vs_oracle(W, H, n, v, stress, lowbits, edge, rows):
    fmt = y210.fmt_code(*v)
    fr, ref = _frames(W, H, n, v, stress, lowbits), _ref(W, H, n, v, stress, lowbits, edge)
    got = _run(W, H, fr, L, S, edge, mode="frame", batch=1, fmt=fmt)
    _check(got, fr, ref)
    with SF.env(MM_K34_ROWS=rows):
        got = _run(W, H, fr, L, S, edge, mode="stream", batch=12 if rows else 8, fmt=fmt)
    _check(got, fr, ref)


def test_y210_n2048_vs_oracle():
    """The N = 2048 instances at 1920 x 128: one-frame calls (unfused K3 -> K4
    there) and a stream through the walking K34, two 64-row strips."""
    W, H, n = 1920, 128, 3
    O.set_threads(16)
    fmt = y210.fmt_code(*V709)
    fr, ref = _frames(W, H, n, V709), _ref(W, H, n, V709)
    got = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
    _check(got, fr, ref)
    with SF.env(MM_K34_ROWS="64"):
        got = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
    _check(got, fr, ref)


def test_y210_standard_mode_vs_oracle():
    W, H, n = 96, 64, 4
    fr, ref = _frames(W, H, n, V709), _ref(W, H, n, V709, std=True)
    for mode, batch in (("frame", 1), ("stream", 8)):
        got = _run(W, H, fr, L, S, mode=mode, batch=batch, standard={}, fmt=y210.fmt_code(*V709))
        _check(got, fr, ref)


@pytest.mark.parametrize("v", [V709, V601])
def test_y210_steerable_equals_f32_path_encoded(v):
    """Steerable (O = 4, DIFF): the output against encode() of the GPU's own
    RGBA32F output on the decoded frames (that path is held to
    oracle/steerable_ref.py), at the format's bar."""
    W, H, n = 256, 192, 4
    extra = {"mode": 2, "orientations": 4}
    fr = _frames(W, H, n, v)
    f32 = T.gpu_run(W, H, [y210.decode(b, np.float32, *v) for b in fr], L, S, mode="stream", extra=extra)
    got = _run(W, H, fr, L, S, mode="stream", extra=extra, fmt=y210.fmt_code(*v))
    _check(got, fr, [y210.encode(f, *v) for f in f32])


# ---- exact tests ---------------------------------------------------------------
def _dev(frames):
    """uint16 frames -> one CUDA uint8 tensor [n][...bytes]."""
    import torch
    return torch.from_numpy(np.stack([np.ascontiguousarray(f).view(np.uint8) for f in frames])).cuda()


def _p010_with_luma(buf, rng):
    """A P010 frame with the packed frame's luma words (any chroma will do)."""
    y = y210.split(buf)[0]
    H, W = y.shape
    return np.concatenate([y, rng.integers(0, 65536, (H // 2, W)).astype(np.uint16)])


@pytest.mark.parametrize("v", [V601, V601_FULL])
def test_bt601_k1_is_the_p010_luma_plane_path(v):
    """compute_state of a BT.601 frame (random chroma words, low bits) is
    bitwise compute_state of the P010 frame with the same luma words; so is the
    final state of a 5-frame stream through K1's batch form (136 x 520) and
    regular form (136 x 518)."""
    import torch
    import mm355
    rng = np.random.default_rng(210)
    fmt = y210.fmt_code(*v)
    pf = mm355.P010_FULL if v[1] else mm355.P010
    for W, H, n in ((200, 120, 1), (136, 520, 5), (136, 518, 5)):
        fr = []
        for f in _frames(W, H, max(n, 2), v, True, True)[-n:]:
            y = y210.split(f)[0]
            c = rng.integers(0, 65536, (2, H, W // 2)).astype(np.uint16)
            fr.append(y210.join(y, c[0], c[1]))
        p10 = [_p010_with_luma(f, rng) for f in fr]
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
        h.set_batch(8)
        st = [torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
        a, b = _dev(fr), _dev(p10)
        if n == 1:
            h.compute_state(a[0], fmt, st[0])
            h.compute_state(b[0], pf, st[1])
        else:
            h.process_stream(a, torch.empty_like(a), n, fmt)
            h.get_state(st[0])
            h.reset()
            h.process_stream(b, torch.empty_like(b), n, pf)
            h.get_state(st[1])
        torch.cuda.synchronize()
        h.close()
        assert torch.equal(st[0], st[1]) and bool(st[0].any()), (W, H)


@pytest.mark.parametrize("v", [V709, V2020_FULL])
def test_matrixed_k1_is_the_decoded_frames_state(v):
    """The state of a matrixed stress frame is the state of its RGBA32F decode
    (tests/test_matrix.py's bar) and far from the BT.601 reading; with neutral
    chroma (0x8000) it is bitwise the BT.601 state."""
    import torch
    import mm355
    W, H = 200, 120
    fmt = y210.fmt_code(*v)
    buf = _frames(W, H, 4, v, True, True)[3]
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = _dev([buf])[0]
    f32 = torch.from_numpy(y210.decode(buf, np.float32, *v)).cuda()
    st = [torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda") for _ in range(5)]
    h.compute_state(dev, fmt, st[0])
    h.compute_state(f32, mm355.RGBA32F, st[1])
    h.compute_state(dev, mm355.base_format(fmt), st[2])
    grey = np.array(buf)
    grey[:, 1::2] = 0x8000
    gdev = _dev([grey])[0]
    h.compute_state(gdev, fmt, st[3])
    h.compute_state(gdev, mm355.base_format(fmt), st[4])
    torch.cuda.synchronize()
    a, b, c = (T.state_rows(s, h.N, H) for s in st[:3])
    h.close()
    bar = 1e-5 * np.abs(b).max()
    print(f"state: |matrixed - decoded| {np.abs(a - b).max():.3e}  bar {bar:.3e}  "
          f"|matrixed - BT.601| {np.abs(a - c).max():.3e}")
    assert np.abs(a - b).max() <= bar
    assert np.abs(a - c).max() > 100 * bar
    assert torch.equal(st[3], st[4]) and bool(st[3].any())


@pytest.mark.parametrize("matrix", [601, 709])
def test_a_yuy2_frame_in_the_high_bytes_has_the_yuy2_state(matrix):
    """from_yuy2(frame) as MM_Y210 is the same picture as the YUY2 frame
    (limited range: code 4 b): the two states agree within the bar above."""
    import torch
    import mm355
    W, H = 200, 120
    rgb = T.synth(W, H, 4, fmt="u8")[3]
    b8 = yuv422.chroma_stress(yuv422.encode(rgb, matrix, False, False), 3)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    st = [torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
    h.compute_state(_dev([y210.from_yuy2(b8)])[0], y210.fmt_code(matrix), st[0])
    h.compute_state(torch.from_numpy(b8).cuda(), yuv422.fmt_code(matrix), st[1])
    torch.cuda.synchronize()
    a, b = (T.state_rows(s, h.N, H) for s in st)
    h.close()
    bar = 1e-5 * np.abs(b).max()
    print(f"state: |Y210 - YUY2| {np.abs(a - b).max():.3e}  bar {bar:.3e}")
    assert np.abs(a - b).max() <= bar and np.abs(b).max() > 0


def test_call_forms_agree_bytewise():
    """A stream call, frame calls and host-pointer calls give the same bytes;
    so do the three compose forms (walking K34, one-shot K34, unfused K3 -> K4)
    and K1's three load forms (one-pair in frame calls; batch and regular form
    in the 5-frame streams at N = 1024)."""
    W, H, n = 200, 120, 4
    for v in (V601_FULL, V2020):
        fr = _frames(W, H, n, v, True, True)
        fmt = y210.fmt_code(*v)
        a = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)      # one-shot K34
        for what, kw, env in (("stream", dict(mode="stream", batch=8), {}),
                              ("host", dict(mode="host"), {}),
                              ("walking K34", dict(mode="stream", batch=8), {"MM_K34_ROWS": "16"}),
                              ("one-shot K34", dict(mode="stream", batch=8), {"MM_K34_ONESHOT": "2"}),
                              ("unfused", dict(mode="stream", batch=8), {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"})):
            with SF.env(**env):
                b = _run(W, H, fr, L, S, fmt=fmt, **kw)
            for k in range(n):
                assert np.array_equal(a[k], b[k]), (what, v, k, int((a[k] != b[k]).sum()))
    for (W, H), v in (((136, 520), V709), ((136, 518), V601), ((136, 520), V601), ((136, 518), V709)):
        fr = _frames(W, H, 5, v, True, True)
        fmt = y210.fmt_code(*v)
        a = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
        b = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
        for k in range(5):
            assert np.array_equal(a[k], b[k]), ("K1 forms", W, H, v, k, int((a[k] != b[k]).sum()))


def _flat(frames):
    return [np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in frames]


def _surface_run(W, H, n, fmt, flat, lin, lout, mode, poison, in_base=0, out_base=0, in_size=None, out_size=None):
    """The frames through the surface entry points, every byte that is no sample
    poisoned; returns the gathered output after asserting the padding is untouched."""
    import torch
    import mm355
    in_size = in_size or y210.buffer_bytes(W, H, lin, n, in_base)
    out_size = out_size or y210.buffer_bytes(W, H, lout, n, out_base)
    src = y210.scatter(W, H, flat, lin, in_base, fill=poison, size=in_size)
    keep = ~y210.sample_mask(W, H, lout, n, out_size, out_base)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    h.set_batch(8)
    a = torch.from_numpy(src).cuda()
    b = torch.full((out_size,), poison ^ 0x55, dtype=torch.uint8, device="cuda")
    if mode == "stream":
        h.process_stream_surfaces(a[in_base:], lin, b[out_base:], lout, n)
    else:
        for k in range(n):
            h.process_surface(a[in_base + k * lin.frame_stride:], lin, b[out_base + k * lout.frame_stride:], lout)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    assert np.all(res[keep] == (poison ^ 0x55)), "output padding is untouched"
    return y210.gather(W, H, res, lout, n, out_base)


@pytest.mark.parametrize("v", [V709, V601])
def test_decoder_surfaces(v):
    """Input and output in mm_surface_aligned(256, 16) layout, all padding
    poisoned, with two different bytes, in stream and in frame mode: the
    samples are bitwise the tight run's and no padding byte is written (nor
    read: the two runs agree)."""
    import mm355
    W, H, n = 200, 120, 4
    fmt = y210.fmt_code(*v)
    fr = _frames(W, H, n, v, True, True)
    flat = _flat(fr)
    want = _flat(_run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt))
    lay = mm355.Surface.aligned(W, H, fmt, 256, 16)
    assert (lay.format, lay.pitch, lay.chroma_offset, lay.frame_stride) == (fmt, 1024, 0, 1024 * 128)
    for mode in ("stream", "frame"):
        for poison in (0xFF, 0x3C):
            got = _surface_run(W, H, n, fmt, flat, lay, lay, mode, poison)
            SF.assert_same(got, want, (mode, hex(poison)))


def test_surfaces_roi_and_mixed_layouts():
    """A region of interest at an even column and row inside a larger frame
    (input) into an aligned(256, 16) surface (output), and the reverse: the
    two sides' layouts differ; same bytes as the tight run."""
    import mm355
    W, H, n = 200, 120, 3
    v = V709
    fmt = y210.fmt_code(*v)
    fr = _frames(W, H, n, v, True, True)
    flat = _flat(fr)
    want = _flat(_run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt))
    roi, base, psize = y210.lay_roi(fmt, W, H, 240, 140, 22, 14)
    assert base % 8 == 0 and base % 16 == 8 and roi.pitch == 960
    al = mm355.Surface.aligned(W, H, fmt, 256, 16)
    size = base + (n - 1) * roi.frame_stride + roi.bytes(W, H) + y210.TAIL
    for mode in ("stream", "frame"):
        got = _surface_run(W, H, n, fmt, flat, roi, al, mode, 0xFF, in_base=base, in_size=size)
        SF.assert_same(got, want, ("roi -> aligned", mode))
        got = _surface_run(W, H, n, fmt, flat, al, roi, mode, 0x3C, out_base=base, out_size=size)
        SF.assert_same(got, want, ("aligned -> roi", mode))


@pytest.mark.parametrize("v", [V709, V601])
def test_surfaces_8_but_not_16_byte_aligned(v):
    """Base + 8, a pitch that is 8 mod 16 and a stride that is 8 mod 16: every
    row of every other frame starts 8 bytes off a 16-byte boundary on both
    sides.  The fused kernels (one-shot and walking) and the unfused pair give
    the tight run's bytes and leave the padding alone."""
    import mm355
    W, H, n = 200, 120, 4
    fmt = y210.fmt_code(*v)
    fr = _frames(W, H, n, v, True, True)
    flat = _flat(fr)
    want = _flat(_run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt))
    lay = mm355.Surface(format=fmt, pitch=4 * W + 8)
    lay.frame_stride = lay.pitch * H + 8
    assert lay.pitch % 16 == 8 and lay.frame_stride % 16 == 8 and lay.bytes(W, H) == lay.pitch * (H - 1) + 4 * W
    for env in ({}, {"MM_K34_ROWS": "16"}, {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"}):
        with SF.env(**env):
            for mode in ("stream", "frame"):
                got = _surface_run(W, H, n, fmt, flat, lay, lay, mode, 0xFF, in_base=8, out_base=8)
                SF.assert_same(got, want, (mode, env))


def test_passthrough():
    import torch
    import mm355
    W, H, n = 200, 120, 3
    for v in (V709, V601_FULL):
        fr = _frames(W, H, n, v, True, True)
        got = _run(W, H, fr, L, S, mode="stream", apply=False, fmt=y210.fmt_code(*v))
        for k in range(n):
            assert np.array_equal(got[k], fr[k])
            assert np.any(got[k] & 63)                  # the low bits went through
    # the frame after mm_reset passes through bitwise, tight and pitched
    fmt = y210.fmt_code(*V709)
    fr = _frames(W, H, n, V709, True, True)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = _dev(fr)
    out = torch.zeros_like(dev)
    h.process(dev[0], out[0], fmt)
    h.process(dev[1], out[1], fmt)
    h.reset()
    h.process(dev[2], out[2], fmt)
    lay = mm355.Surface.aligned(W, H, fmt, 256, 16)
    src = torch.from_numpy(y210.scatter(W, H, [_flat(fr)[1]], lay)).cuda()
    dst = torch.full_like(src, 0x77)
    h.reset()
    h.process_surface(src, lay, dst, lay)
    torch.cuda.synchronize()
    got = [g.view(np.uint16) for g in out.cpu().numpy()]
    h.close()
    assert np.array_equal(got[0], fr[0]) and np.array_equal(got[2], fr[2]) and not np.array_equal(got[1], fr[1])
    res = dst.cpu().numpy()
    assert np.array_equal(y210.gather(W, H, res, lay, 1)[0], _flat(fr)[1])
    assert np.all(res[~y210.sample_mask(W, H, lay, 1, res.size)] == 0x77)


def test_refusals_leave_the_handle_usable():
    """Odd sizes, a debug view, fmt | 128, both matrix bits, the unknown
    neighbours, a misaligned device pointer, a stride that is no multiple of 8
    and differing in / out formats are refused before anything is queued: the
    Y210 stream around them continues bitwise as if they had never been made."""
    import torch
    import mm355
    W, H, n = 64, 48, 4
    fmt = mm355.Y210
    fr = _frames(W, H, n, V601)
    want = _run(W, H, fr, L, S, mode="frame", batch=64, fmt=fmt)
    p = mm355.Params.make(levels=L, phase_scale=S)
    h = mm355.Handle(W, H, p)
    dev = _dev(fr)
    out = torch.zeros_like(dev)
    junk = torch.zeros(2 * W * H * 4 + 16, dtype=torch.uint8, device="cuda")
    state = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    for k in range(2):
        h.process(dev[k], out[k], fmt)

    def refused(bad, src, code):
        for call in (lambda: h.process(src, junk.clone(), bad),
                     lambda: h.process_stream(src, junk.clone(), 1, bad),
                     lambda: h.compute_state(src, bad, state.clone())):
            with pytest.raises(mm355.MMError) as ei:
                call()
            assert ei.value.code == code, (bad, ei.value.code)

    for bad in (fmt | 128, fmt | mm355.MATRIX_BT709 | mm355.MATRIX_BT2020, mm355.Y210_FULL | 128, 21, 20, 21 | 32,
                28 | mm355.MATRIX_BT709):
        refused(bad, junk, -1)                                # MM_ERR_INVALID
    for off in (4, 1, 2, 12):                                 # a device pointer that is no multiple of 8
        refused(fmt | mm355.MATRIX_BT709, junk[off:], -1)
    with pytest.raises(mm355.MMError) as ei:
        h.process(junk, junk[4:], fmt)                        # ... on the output side
    assert ei.value.code == -1
    tight = mm355.Surface.tight(W, H, fmt)
    other = mm355.Surface.tight(W, H, mm355.Y210_FULL)
    with pytest.raises(mm355.MMError) as ei:
        h.process_surface(junk, tight, junk.clone(), other)   # in / out formats differ
    assert ei.value.code == -1
    odd = mm355.Surface.tight(W, H, fmt)
    odd.frame_stride += 4                                     # a stride that is no multiple of 8
    with pytest.raises(mm355.MMError) as ei:
        h.process_stream_surfaces(junk, odd, junk.clone(), tight, 2)
    assert ei.value.code == -1
    h.process(dev[2], out[2], fmt)
    h.set_params(mm355.Params.make(levels=L, phase_scale=S, show_phase=1))
    for bad in (fmt, mm355.Y210_FULL | mm355.MATRIX_BT2020):
        for call in (lambda: h.process(dev[3], out[3], bad), lambda: h.process_stream(dev[3], out[3], 1, bad)):
            with pytest.raises(mm355.MMError) as ei:
                call()
            assert ei.value.code == -2                        # MM_ERR_UNSUPPORTED
    h.set_params(mm355.Params.make(levels=L, phase_scale=S, show_magnitude=1))
    with pytest.raises(mm355.MMError) as ei:
        h.process(dev[3], out[3], fmt)
    assert ei.value.code == -2
    h.set_params(p)
    # odd sizes: another handle's geometry, refused before anything is queued
    for OW, OH in ((63, 48), (64, 47)):
        ho = mm355.Handle(OW, OH, p)
        sto = torch.zeros(ho.state_bytes, dtype=torch.uint8, device="cuda")
        for call in (lambda: ho.process(junk, junk.clone(), fmt), lambda: ho.process_stream(junk, junk.clone(), 1, fmt),
                     lambda: ho.compute_state(junk, fmt, sto)):
            with pytest.raises(mm355.MMError) as ei:
                call()
            assert ei.value.code == -2
        ho.close()
    h.process(dev[3], out[3], fmt)
    torch.cuda.synchronize()
    got = [g.view(np.uint16) for g in out.cpu().numpy()]
    h.close()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k


def test_python_layer_takes_word_frames():
    """OnRenderImage(fmt=mm355.Y210 | ...) on [H, 2 W] uint16 tensors,
    contiguous and as a row-strided view, gives the binding's words."""
    import torch
    import mm355
    W, H, n = 64, 48, 3
    v = V709
    fmt = y210.fmt_code(*v)
    fr = _frames(W, H, n, v, True, True)
    want = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
    for strided in (False, True):
        proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
        src = _dev(fr).view(torch.uint16)
        assert tuple(src.shape) == (n, H, 2 * W)
        # (allocated, filled and read back as int16: the same words)
        parent = torch.full((n, H + 6, 2 * W + 24), 0x1111, dtype=torch.int16, device="cuda")
        tight = torch.zeros((n, H, 2 * W), dtype=torch.int16, device="cuda")
        for k in range(n):
            words = parent[k, 4:4 + H, 8:8 + 2 * W] if strided else tight[k]
            dst = (parent if strided else tight).view(torch.uint16)[k]
            dst = dst[4:4 + H, 8:8 + 2 * W] if strided else dst
            assert dst.data_ptr() == words.data_ptr() and dst.is_contiguous() != strided
            proc.OnRenderImage(src[k], dst, fmt=fmt)
            torch.cuda.synchronize()
            got = words.cpu().numpy().view(np.uint16)
            assert np.array_equal(got, want[k]), (strided, k)
        proc.OnDestroy()
        if strided:
            edge = parent.clone()
            edge[:, 4:4 + H, 8:8 + 2 * W] = 0x1111
            assert bool((edge == 0x1111).all())
    # host arrays too
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(n):
        o = np.empty((H, 2 * W), np.uint16)
        proc.OnRenderImage(np.array(fr[k]), o, fmt=fmt)
        assert np.array_equal(o, want[k]), k
    proc.OnDestroy()


def test_cli_matches_binding(tmp_path):
    """mm_cli --y210 --matrix 709 on a C422p10 clip writes a C422p10 file whose
    planes, << 6 and re-packed, are the binding's Y210 | BT709 output on the
    same words (and not its BT.601 output); --surface-align 256,16 writes the
    same file, --full-range another; any other extension holds the raw frames."""
    import mm355
    W, H, n = 64, 48, 4
    fr = _frames(W, H, n, V709, True)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with open(src, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C422p10\n".encode())
        for b in fr:
            y, cb, cr = (np.ascontiguousarray(p >> 6) for p in y210.split(b))
            f.write(b"FRAME\n" + y.tobytes() + cb.tobytes() + cr.tobytes())
    base = ["--matrix", "709", "-i", src, "-l", str(L), "-s", str(S), "-b", "4"]
    subprocess.check_call([CLI, "--y210", "-o", dst] + base, timeout=120)
    raw = open(dst, "rb").read()
    head, body = raw.split(b"\n", 1)
    assert head.startswith(b"YUV4MPEG2") and b"C422p10" in head and f"W{W} H{H}".encode() in head
    fb = 4 * W * H
    assert len(body) == n * (6 + fb)
    want = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=mm355.Y210 | mm355.MATRIX_BT709)
    as601 = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=mm355.Y210)
    for k in range(n):
        rec = body[k * (6 + fb):(k + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n"
        p = np.frombuffer(rec[6:], np.uint16)
        assert p.max() <= 1023
        got = y210.join(p[:W * H].reshape(H, W) << 6, p[W * H:W * H * 3 // 2].reshape(H, W // 2) << 6,
                        p[W * H * 3 // 2:].reshape(H, W // 2) << 6)
        assert np.array_equal(got, want[k]), k
        assert k == 0 or not np.array_equal(got, as601[k])
    other = str(tmp_path / "other.y4m")
    subprocess.check_call([CLI, "--y210", "--surface-align", "256,16", "-o", other] + base, timeout=120)
    assert open(other, "rb").read() == raw
    subprocess.check_call([CLI, "--y210", "--full-range", "-o", other] + base, timeout=120)
    full = open(other, "rb").read()
    assert len(full) == len(raw) and full != raw
    # any other extension: the raw Y210 frames
    rawp = str(tmp_path / "out.y210")
    subprocess.check_call([CLI, "--y210", "-o", rawp] + base, timeout=120)
    assert open(rawp, "rb").read() == b"".join(w.tobytes() for w in want)
