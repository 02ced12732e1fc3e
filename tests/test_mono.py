"""MM_Y8 / MM_Y10 / MM_Y12 / MM_Y16 grayscale frames through the C-ABI on the HIP path.

A gray frame is the RGBA32F frame R = G = B = sample / max (include/mm.h), so
the reference is the existing oracle on mono.decode(frame, float32), encoded by
mono.encode: tests/mono.py holds the definitions, in float64 numpy.

Bar, per compared frame: every sample differs by at most ONE code, the bits of
a Y10 / Y12 output word above the code are zero, and the share of differing
samples is at most
    Y8  mmtest.U8_FRAC (1e-3)    Y10  4 x U8_FRAC    Y12  16 x U8_FRAC    Y16  0.05
(P010's rule for 8 / 10 / 12 bits: the code step shrinks, the same fp32 error
crosses a boundary that much more often; for 16 bits the rule would give 0.26,
which no longer binds, hence 0.05).  Y16 must also meet the project's fp32 bar
on word / 65535 (mmtest.TOL_MAX, TOL_RMSE).  The first frame is bitwise the
input, and every compared frame differs from its input on more than half of
its samples (not a passthrough).

The caps bind on the kernels, not on the reference's own noise: the fp32 oracle
against the float64 twin (np_twin.process_frame), both encoded, on the exact
inputs below, worst frame of each case, maximum difference 1 code everywhere:
    Y8   64x48 3.3e-4   200x120 4.2e-5   98x62 0   97x63 1.6e-4
         128x128 REPEAT / CLAMP 6.1e-5   1920x128 1.3e-4   stretched 200x120 4.2e-5
    Y10  200x120 2.1e-4   stretched 1.7e-4
    Y12  200x120 6.7e-4   stretched 5.4e-4
    Y16  64x48 8.5e-3   200x120 8.0e-3   98x62 7.6e-3   97x63 5.2e-3
         128x128 5.8e-3 / 5.6e-3   stretched 200x120 1.05e-2
         1920x128 1.6e-2 on the clip at half brightness (mono.frames dim=0.5).
    standard mode 96x64: Y8 3.3e-4, Y16 1.5e-2 (half brightness)
Every figure is below half its cap.  At full brightness the 1920x128 Y16 figure
was 3.1e-2 (the N = 2048 transforms' fp32 error against a 1.5e-5 code step) and
the standard-mode Y16 one 2.8e-2, more than half the cap, so those cases' INPUT
is the dimmer clip; the cap stays.

Debug views: the reference is the R channel of the GPU's own RGBA32F output,
and the formats of these cases follow from that reference's own fp32 noise,
measured as the fp32 oracle's view against the float64 twin's
(np_twin.debug_view), both as codes, on the same frames.  The phase view is
|atan2| of spectrum bins, ill-conditioned where a bin is nearly zero, so at 16
bits the fp32 oracle itself is up to 76 codes (8.5 % of the samples) from the
twin, and at 12 bits up to 2 codes: no fp32 path can be held to one code there,
and the phase and split views are checked at 8 and 10 bits, where the figures
are max 1 code and
    Y8   magnitude 1.3e-4 / 1.6e-4 (200x120 / 97x63)   split 1.3e-4 / 3.3e-4   phase 200x120 4.6e-4
    Y10  magnitude 4.2e-4 / 4.9e-4   phase 1.6e-3 / 9.8e-4   split 1.1e-3 / 1.1e-3
all below half their caps (the Y8 phase view at 97x63 measures 6.5e-4, above
half of 1e-3: that combination is left to Y10).  The magnitude view at 16 bits:
max 1 code, 1.5e-2 at 97x63 (checked) and 2.7e-2 at 200x120 (above half of
0.05: not checked at that size).  Every view and both sizes are reached by the
byte instance and by the word instance.

Kernels reached: K1 k_rows_fwd in its regular, one-pair and GEN (odd sizes)
forms, all three the luma-plane instances; the compose forms k_rows_inv_compose
(walking), k_rows_inv_compose4 (one shot), k_compose_mono (unfused) and
k_compose_odd, k_dbg_out for the views, k_copy_rows for pitched passthrough.
Words go to the device as their bytes, so nothing depends on a 16-bit tensor
type.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmtest as T
import mono

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
CAP = {8: T.U8_FRAC, 10: 4 * T.U8_FRAC, 12: 16 * T.U8_FRAC, 16: 0.05}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(W, H, frames, bits, *a, **kw):
    """T.gpu_run on [H][W] sample frames, moved as their bytes."""
    got = T.gpu_run(W, H, [mono.as_bytes(f) for f in frames], *a, fmt=mono.fmt_of(bits), **kw)
    return [mono.from_bytes(g, bits) for g in got]


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, bits, edge=0, std=False, stretch=False, dim=1.0):
    """The oracle on the decoded frames, encoded (computed once per case)."""
    fr = [mono.decode(b, bits, np.float32) for b in mono.frames(W, H, n, bits, stretch=stretch, dim=dim)]
    ref = T.oracle_run(W, H, fr, L, S, edge, standard={} if std else None)
    return tuple(mono.encode(r, bits) for r in ref)


def _bar(got, ref, bits, what=""):
    """The bar of the module docstring on one frame."""
    assert got.dtype == mono.dtype_of(bits) and got.shape == ref.shape
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    frac = float((d > 0).mean())
    print(f"{what}: Y{bits} max {int(d.max())} frac {frac:.2e} (cap {CAP[bits]:.1e})")
    assert int(got.max()) <= mono.vmax(bits), "no bit above the code"
    assert d.max() <= 1, (what, int(d.max()))
    assert frac <= CAP[bits], (what, frac)
    if bits == 16:
        T.assert_close_f32(got / 65535.0, ref / 65535.0)


def _check(got, frames, ref, bits, what=""):
    assert np.array_equal(got[0], frames[0]), "first frame passes through bitwise"
    for k in range(1, len(frames)):
        _bar(got[k], ref[k], bits, f"{what} frame {k}")
        assert (got[k] != frames[k]).mean() > 0.5, "not a passthrough"


# W, H, frames, edge, MM_K34_ROWS of the stream leg, brightness
GEOMETRIES = [
    (64, 48, 4, 0, None, 1.0),       # K1 one-pair form; x0 = 0: unfused K3 -> k_compose_mono
    (200, 120, 4, 0, None, 1.0),     # N = 256: k_rows_inv_compose4
    (200, 120, 12, 0, "64", 1.0),    # the walking fused K34
    (98, 62, 4, 0, None, 1.0),       # W % 8 != 0: unfused; Y8 rows (98 B) and odd frames (6,076 B apart)
                                     # are not dword aligned: single-sample stores
    (97, 63, 4, 0, None, 1.0),       # odd: GEN K1 and k_compose_odd
    (128, 128, 4, 0, None, 1.0),     # N = W = H: no margins, every border wraps
    (128, 128, 4, 1, None, 1.0),     # ... or clamps
    (1920, 128, 3, 0, None, 0.5),    # the N = 2048 instances at a fraction of 1080p's work
]                                    # (half brightness at 16 bits only: module docstring)
CASES = ([(b,) + g[:5] + (g[5] if b == 16 else 1.0,) for g in GEOMETRIES for b in (8, 16)] +
         [(b,) + GEOMETRIES[1] for b in (10, 12)])


@pytest.mark.parametrize("bits,W,H,n,edge,rows,dim", CASES)
def test_mono_vs_oracle(bits, W, H, n, edge, rows, dim):
    fr, ref = mono.frames(W, H, n, bits, dim=dim), _ref(W, H, n, bits, edge, dim=dim)
    got = _run(W, H, fr, bits, L, S, edge, mode="frame", batch=1)
    _check(got, fr, ref, bits, "frame calls")
    with _env(MM_K34_ROWS=rows):
        got = _run(W, H, fr, bits, L, S, edge, mode="stream", batch=12 if rows else 8)
    _check(got, fr, ref, bits, "stream")


@pytest.mark.parametrize("bits", mono.BITS)
def test_mono_saturate_stress(bits):
    """Frames stretched about mid-gray by a gain of 3: the output clamp is
    really exercised (>= 1 % of the reference's samples sit at code max)."""
    W, H, n = 200, 120, 4
    fr, ref = mono.frames(W, H, n, bits, stretch=True), _ref(W, H, n, bits, stretch=True)
    for k in range(1, n):
        assert (ref[k] == mono.vmax(bits)).mean() >= 0.01, k
    for kw in (dict(mode="frame", batch=1), dict(mode="stream", batch=8)):
        _check(_run(W, H, fr, bits, L, S, **kw), fr, ref, bits, kw["mode"])


@pytest.mark.parametrize("bits", [10, 12])
def test_mono_first_frame_bitwise_with_stray_high_bits(bits):
    """Words with bits above the code: the first frame returns them as they
    are; every later frame has them zero."""
    W, H, n = 200, 120, 3
    fr = mono.frames(W, H, n, bits, stray=True)
    assert all(int((f > mono.vmax(bits)).sum()) >= 8 for f in fr)
    for kw in (dict(mode="frame", batch=1), dict(mode="stream", batch=8), dict(mode="host")):
        got = _run(W, H, fr, bits, L, S, **kw)
        assert np.array_equal(got[0], fr[0]), kw
        for k in range(1, n):
            assert int(got[k].max()) <= mono.vmax(bits), (kw, k)
            assert (got[k] != fr[k]).mean() > 0.5


@pytest.mark.parametrize("bits", [8, 16])
def test_mono_call_forms_agree_bytewise(bits):
    """A stream call, frame calls and host-pointer calls give the same bytes;
    so do the compose forms (walking K34, one-shot K34, unfused K3 -> K4): the
    same blur expression, sat and code in each."""
    W, H, n = 200, 120, 4
    fr = mono.frames(W, H, n, bits)
    a = _run(W, H, fr, bits, L, S, mode="frame", batch=1)
    for what, kw, env in (("stream", dict(mode="stream", batch=8), {}),
                          ("host", dict(mode="host"), {}),
                          ("walking K34", dict(mode="stream", batch=8), {"MM_K34_ROWS": "16"}),
                          ("one-shot K34", dict(mode="stream", batch=8), {"MM_K34_ONESHOT": "2"}),
                          ("unfused", dict(mode="stream", batch=8), {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"})):
        with _env(**env):
            b = _run(W, H, fr, bits, L, S, **kw)
        for k in range(n):
            assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("bits,W,H", [(8, 200, 120), (16, 200, 120), (8, 97, 63), (12, 98, 62)])
def test_mono_pitched_surfaces(bits, W, H):
    """aligned(256, 16) in, another pitch out: the guard bytes in all padding
    stay as they were, and the samples are bytewise the tight run's (the first
    frame's passthrough through k_copy_rows included)."""
    import torch
    import mm355
    n = 4
    fmt, u = mono.fmt_of(bits), (1 if bits == 8 else 2)
    fr = mono.frames(W, H, n, bits)
    want = _run(W, H, fr, bits, L, S, mode="stream", batch=8)
    lin = mm355.Surface.aligned(W, H, fmt, 256, 16)
    lout = mm355.Surface(format=fmt, pitch=W * u + 3 * u)        # a multiple of the unit and of nothing wider
    lout.frame_stride = lout.bytes(W, H) + 5 * u
    for mode in ("stream", "frame"):
        in_size = (n - 1) * lin.frame_stride + lin.bytes(W, H) + 64
        out_size = (n - 1) * lout.frame_stride + lout.bytes(W, H) + 64
        src = mono.scatter(fr, lin.pitch, lin.frame_stride, in_size)
        sent = mono.sentinel(out_size)
        a, b = torch.from_numpy(src).cuda(), torch.from_numpy(sent).cuda()
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
        h.set_batch(8)
        if mode == "stream":
            h.process_stream_surfaces(a, lin, b, lout, n)
        else:
            for k in range(n):
                h.process_surface(a[k * lin.frame_stride:], lin, b[k * lout.frame_stride:], lout)
        torch.cuda.synchronize()
        res = b.cpu().numpy()
        h.close()
        assert np.array_equal(a.cpu().numpy(), src), "the input surface is read only"
        keep = ~mono.sample_mask(H, W * u, n, lout.pitch, lout.frame_stride, out_size)
        bad = np.flatnonzero(keep & (res != sent))
        assert bad.size == 0, f"{mode}: {bad.size} padding bytes written, first at {bad[:8]}"
        got = mono.gather(res, H, W * u, n, lout.pitch, lout.frame_stride, bits)
        for k in range(n):
            assert np.array_equal(got[k], want[k]), (mode, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("bits", [8, 16])
def test_mono_standard_mode_vs_oracle(bits):
    W, H, n = 96, 64, 4
    dim = 0.5 if bits == 16 else 1.0                     # (module docstring)
    fr, ref = mono.frames(W, H, n, bits, dim=dim), _ref(W, H, n, bits, std=True, dim=dim)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _check(_run(W, H, fr, bits, L, S, mode=mode, batch=batch, standard={}), fr, ref, bits, mode)


@pytest.mark.parametrize("bits", [8, 16])
def test_mono_steerable_equals_f32_path_encoded(bits):
    """Steerable (O = 4, DIFF): against encode() of the GPU's own RGBA32F
    output on the decoded frames (that path is held to oracle/steerable_ref.py)."""
    W, H, n = 256, 192, 4
    extra = {"mode": 2, "orientations": 4}
    fr = mono.frames(W, H, n, bits)
    f32 = T.gpu_run(W, H, [mono.decode(b, bits, np.float32) for b in fr], L, S, mode="stream", extra=extra)
    got = _run(W, H, fr, bits, L, S, mode="stream", extra=extra)
    _check(got, fr, [mono.encode(f, bits) for f in f32], bits, "steerable")


MAG, PHASE, BOTH, SIZES = (1, 0), (0, 1), (1, 1), ((200, 120), (97, 63))
DEBUG_CASES = ([(8, v, W, H) for v in (MAG, BOTH) for W, H in SIZES] + [(8, PHASE, 200, 120)] +
               [(10, v, W, H) for v in (MAG, PHASE, BOTH) for W, H in SIZES] + [(16, MAG, 97, 63)])


@pytest.mark.parametrize("bits,debug,W,H", DEBUG_CASES)
def test_mono_debug_views(bits, debug, W, H):
    """show_magnitude / show_phase / split screen: the views are R-channel
    pictures, the output code is the view's R value: against the codes of the R
    channel of the RGBA32F path's output on the decoded frames.  (Which format
    checks which view: the module docstring.)"""
    n = 3
    fr = mono.frames(W, H, n, bits)
    f32 = T.gpu_run(W, H, [mono.decode(b, bits, np.float32) for b in fr], L, S, mode="stream", debug=debug)
    got = _run(W, H, fr, bits, L, S, mode="stream", debug=debug)
    assert np.array_equal(got[0], fr[0])
    for k in range(1, n):
        ref = mono.codes(f32[k][..., 0], bits)
        assert np.ptp(ref) > mono.vmax(bits) // 8, "a picture, not a constant"
        _bar(got[k], ref, bits, f"debug {debug} frame {k}")


@pytest.mark.parametrize("bits", [8, 12])
def test_mono_apply_off_passes_through_and_keeps_state(bits):
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fr = mono.frames(W, H, n, bits, stray=bits == 12)
    got = _run(W, H, fr, bits, L, S, mode="stream", apply=False)
    for k in range(n):
        assert np.array_equal(got[k], fr[k])             # stray high bits included
    # the state still follows the input: compute_state(last frame) == the held state
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S, apply_magnification=False))
    dev = torch.from_numpy(np.stack([mono.as_bytes(f) for f in fr])).cuda()
    out = torch.empty_like(dev)
    h.process_stream(dev, out, n, mono.fmt_of(bits))
    held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    made = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.get_state(held)
    h.compute_state(dev[n - 1], mono.fmt_of(bits), made)
    torch.cuda.synchronize()
    assert torch.equal(held, made)
    h.close()


def test_mono_state_is_the_gray_rgba32f_frames_state():
    """mm_get_state after a Y8 frame against the state after the same frame
    sent as RGBA32F gray: within the fp32 bar, NOT bitwise.  K1 takes the byte
    as an exact integer and folds 1 / 255 into the resample weights, while the
    RGBA32F instance sums 0.299 v + 0.587 v + 0.114 v of the already rounded
    v = float32(byte / 255): the same number, rounded in another order."""
    import torch
    import mm355
    W, H = 200, 120
    fr = mono.frames(W, H, 2, 8)
    states = []
    for fmt, frames in ((mm355.Y8, [mono.as_bytes(f) for f in fr]),
                        (mm355.RGBA32F, [mono.decode(f, 8, np.float32) for f in fr])):
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
        dev = torch.from_numpy(np.stack(frames)).cuda()
        out = torch.empty_like(dev)
        for k in range(2):
            h.process(dev[k], out[k], fmt)
        st = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(st)
        torch.cuda.synchronize()
        states.append(T.state_rows(st, h.N, H))
        h.close()
    a, b = states
    assert np.abs(b).max() > 1.0
    assert np.abs(a - b).max() <= 1e-5 * max(1.0, np.abs(b).max())


def test_mono_on_render_image_named_format():
    """OnRenderImage(fmt=): [H, W] tensors, and row-strided views of a larger
    one, give the bytes of the C-ABI call."""
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fr = mono.frames(W, H, n, 8)
    want = _run(W, H, fr, 8, L, S, mode="frame", batch=1)
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    big_in = torch.zeros((H + 8, W + 24), dtype=torch.uint8, device="cuda")
    big_out = torch.full((H + 8, W + 24), 7, dtype=torch.uint8, device="cuda")
    for k in range(n):
        big_in[4:4 + H, 8:8 + W] = torch.from_numpy(np.array(fr[k])).cuda()
        proc.OnRenderImage(big_in[4:4 + H, 8:8 + W], big_out[4:4 + H, 8:8 + W], fmt=mm355.Y8)
        torch.cuda.synchronize()
        assert np.array_equal(big_out[4:4 + H, 8:8 + W].cpu().numpy(), want[k]), k
    edge = big_out.clone()
    edge[4:4 + H, 8:8 + W] = 7
    assert bool((edge == 7).all()), "nothing outside the view is written"
    proc.OnDestroy()


def _write_clip(path, W, H, frames, bits):
    tag = "mono" if bits == 8 else f"mono{bits}"
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F120:1 Ip A1:1 C{tag}\n".encode())
        for b in frames:
            f.write(b"FRAME\n" + np.ascontiguousarray(b).tobytes())


@pytest.mark.parametrize("bits", [8, 12])
def test_cli_mono_matches_binding(tmp_path, bits):
    """mm_cli --mono on a Cmono / Cmono12 clip writes a clip of the same type
    whose samples are the library call's output on the same bytes."""
    W, H, n = 200, 120, 4
    fr = mono.frames(W, H, n, bits)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    _write_clip(src, W, H, fr, bits)
    subprocess.check_call([CLI, "--mono", "-i", src, "-o", dst, "-l", str(L), "-s", str(S), "-b", "4"], timeout=120)
    raw = open(dst, "rb").read()
    head, body = raw.split(b"\n", 1)
    tag = b"Cmono" if bits == 8 else f"Cmono{bits}".encode()
    assert head.startswith(b"YUV4MPEG2") and head.split()[-1] == tag and f"W{W} H{H}".encode() in head
    fb = W * H * (1 if bits == 8 else 2)
    assert len(body) == n * (6 + fb)
    want = _run(W, H, fr, bits, L, S, mode="stream", batch=8)
    for k in range(n):
        rec = body[k * (6 + fb):(k + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n"
        got = np.frombuffer(rec[6:], mono.dtype_of(bits)).reshape(H, W)
        assert np.array_equal(got, want[k]), k
