"""MM_RGB24 / MM_BGR24 packed RGB frames through the C-ABI on the HIP path.

A frame is the MM_RGBA8 frame with the same colour bytes and alpha 255
(include/mm.h).  Inputs are the project's synthetic stream without its alpha
byte (mmtest.synth(..., fmt="u8")[..., :3]; the alpha is 255 everywhere, so the
RGBA8 twin of a frame is the synth frame itself), L = 5, S = 25.

Two identities carry most of the checks, both BITWISE:
  1. the output bytes are the MM_RGBA8 path's R, G, B bytes on the same picture,
     and the temporal state is that RGBA8 frame's state;
  2. MM_BGR24 on the byte-swapped frame gives the byte-swapped output of
     MM_RGB24, and the same state.

Bar against the oracle (the CPU reference on the RGBA8 twin, its R, G, B bytes),
per compared frame: mmtest.assert_close_u8 on the 3 W H bytes (at most 1 LSB, on
at most U8_FRAC = 1e-3 of them); the first frame is bitwise the input; more than
half the bytes differ from the input (not a passthrough).

The cap binds on the kernels, not on the reference: the fp32 oracle against the
float64 twin (np_twin.process_frame), both encoded, measured on the CPU, worst
frame of each case (max LSB, fraction of differing bytes):
    64x48 0, 0             200x120 1, 1.4e-5        98x62 0, 0
    97x63 1, 5.5e-5        128x128 REPEAT and CLAMP 1, 4.1e-5
    standard mode 96x64 1, 1.6e-4                   1920x128 1, 1.5e-4
    saturate stress 200x120 (bytes stretched about 128 by 3) 1, 4.2e-5
All are below a fifth of the cap, and in every case 98 to 100 % of the
reference's bytes differ from the input.  Saturate stress: 22.6 % of the input
bytes sit at 0 or 255; the reference has 0.8-0.9 % of its bytes at 255 and
1.0-1.1 % at 0.

Kernels reached: K1 k_rows_fwd<.., kFmtRGB24> in its regular, shared-rows,
one-pair and GEN forms (byte-aligned dword loads) at N = 64 .. 8192; the compose
forms k_rows_inv_compose (walking) and k_rows_inv_compose4 (one shot) with their
12-byte quads, k_compose (unfused, also every layout whose rows are not dword
aligned), k_compose_odd, k_dbg_out for the views, k_copy_rows for pitched
passthrough.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmtest as T
import rgb24

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
ORDERS = ("rgb", "bgr")
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


def _run(W, H, frames, order, *a, **kw):
    """T.gpu_run on R G B frames sent in byte order `order`; the result back in R G B."""
    got = T.gpu_run(W, H, [rgb24.in_order(f, order) for f in frames], *a, fmt=rgb24.fmt_of(order), **kw)
    return [rgb24.in_order(g, order) for g in got]


def _rgba8(W, H, frames, *a, **kw):
    """The MM_RGBA8 path on the frames' twins: its R, G, B bytes."""
    got = T.gpu_run(W, H, [rgb24.twin(f) for f in frames], *a, **kw)
    for g in got[1:]:
        assert int(g[..., 3].min()) == 255
    return [rgb24.colour(g) for g in got]


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, edge=0, std=False, stretch=False):
    """The oracle on the RGBA8 twins, its R, G, B bytes (computed once per case)."""
    fr = [rgb24.twin(f) for f in rgb24.frames(W, H, n, stretch=stretch)]
    ref = T.oracle_run(W, H, fr, L, S, edge, standard={} if std else None)
    return tuple(rgb24.colour(r) for r in ref)


def _check(got, frames, ref, what=""):
    assert got[0].dtype == np.uint8 and got[0].shape == frames[0].shape
    assert np.array_equal(got[0], frames[0]), "first frame passes through bitwise"
    for k in range(1, len(frames)):
        d = np.abs(got[k].astype(np.int32) - ref[k].astype(np.int32))
        print(f"{what} frame {k}: max {int(d.max())} frac {float((d > 0).mean()):.2e} (cap {T.U8_FRAC:.0e})")
        T.assert_close_u8(got[k], ref[k])
        assert (got[k] != frames[k]).mean() > 0.5, "not a passthrough"


def _same(a, b, what):
    assert len(a) == len(b)
    for k in range(len(a)):
        assert np.array_equal(a[k], b[k]), (what, k, int((np.asarray(a[k]) != np.asarray(b[k])).sum()))


# W, H, frames, edge, MM_K34_ROWS of the stream leg
GEOMETRIES = [
    (64, 48, 4, 0, None),        # K1 one-pair form; x0 = 0: unfused K3 -> k_compose
    (200, 120, 4, 0, None),      # N = 256: k_rows_inv_compose4, 12-byte quads
    (200, 120, 12, 0, "64"),     # the walking fused K34
    (98, 62, 4, 0, None),        # W % 8 != 0: unfused; rows (294 B) are not dword aligned
    (97, 63, 4, 0, None),        # odd: GEN K1 and k_compose_odd
    (128, 128, 4, 0, None),      # N = W = H: no margins, every border wraps
    (128, 128, 4, 1, None),      # ... or clamps
    (1920, 128, 3, 0, None),     # the N = 2048 instances at a fraction of 1080p's work
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,H,n,edge,rows", GEOMETRIES)
def test_rgb24_vs_oracle(W, H, n, edge, rows, order):
    fr, ref = rgb24.frames(W, H, n), _ref(W, H, n, edge)
    got = _run(W, H, fr, order, L, S, edge, mode="frame", batch=1)
    _check(got, fr, ref, f"{order} frame calls")
    with _env(MM_K34_ROWS=rows):
        got = _run(W, H, fr, order, L, S, edge, mode="stream", batch=12 if rows else 8)
    _check(got, fr, ref, f"{order} stream")


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_standard_mode_vs_oracle(order):
    W, H, n = 96, 64, 4
    fr, ref = rgb24.frames(W, H, n), _ref(W, H, n, std=True)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _check(_run(W, H, fr, order, L, S, mode=mode, batch=batch, standard={}), fr, ref, f"{order} {mode}")
    _same(_run(W, H, fr, order, L, S, mode="stream", standard={}),
          _rgba8(W, H, fr, L, S, mode="stream", standard={}), "identity 1, standard mode")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,H,n,edge,rows", GEOMETRIES + [(4104, 48, 2, 0, None)])   # ... and the N = 8192 instances
def test_rgb24_is_the_rgba8_path_bytewise(W, H, n, edge, rows, order):
    """Identity 1 over the stream, frame and host call forms."""
    fr = rgb24.frames(W, H, n)
    with _env(MM_K34_ROWS=rows):
        batch = 12 if rows else 8
        _same(_run(W, H, fr, order, L, S, edge, mode="stream", batch=batch),
              _rgba8(W, H, fr, L, S, edge, mode="stream", batch=batch), "stream")
    want = _rgba8(W, H, fr, L, S, edge, mode="frame", batch=1)
    assert (want[1] != fr[1]).mean() > 0.5
    _same(_run(W, H, fr, order, L, S, edge, mode="frame", batch=1), want, "frame calls")
    _same(_run(W, H, fr[:2], order, L, S, edge, mode="host"), want[:2], "host calls")


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_compose_forms_agree_bytewise(order):
    """The walking K34, the one-shot K34 and the unfused K3 -> K4 give the RGBA8
    path's bytes, each against the RGBA8 run under the same switch."""
    W, H, n = 200, 120, 4
    fr = rgb24.frames(W, H, n)
    base = _run(W, H, fr, order, L, S, mode="frame", batch=1)
    for what, env in (("walking K34", {"MM_K34_ROWS": "16"}), ("one-shot K34", {"MM_K34_ONESHOT": "2"}),
                      ("unfused", {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"})):
        with _env(**env):
            a = _run(W, H, fr, order, L, S, mode="stream", batch=8)
            b = _rgba8(W, H, fr, L, S, mode="stream", batch=8)
        _same(a, b, what)
        _same(a, base, what + " against frame calls")


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_steerable_is_the_rgba8_path_bytewise(order):
    W, H, n = 256, 192, 4
    extra = {"mode": 2, "orientations": 4}                # O = 4, DIFF
    fr = rgb24.frames(W, H, n)
    got = _run(W, H, fr, order, L, S, mode="stream", extra=extra)
    want = _rgba8(W, H, fr, L, S, mode="stream", extra=extra)
    assert np.array_equal(got[0], fr[0]) and (got[1] != fr[1]).mean() > 0.5
    _same(got, want, "steerable")


MAG, PHASE, BOTH = (1, 0), (0, 1), (1, 1)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
@pytest.mark.parametrize("debug", [MAG, PHASE, BOTH])
def test_rgb24_debug_views(debug, W, H, order):
    """The output is the RGBA8 view's R, G, B bytes: R the view, G = B = 0."""
    n = 3
    fr = rgb24.frames(W, H, n)
    got = _run(W, H, fr, order, L, S, mode="stream", debug=debug)
    want = _rgba8(W, H, fr, L, S, mode="stream", debug=debug)
    _same(got, want, f"debug {debug}")
    for k in range(1, n):
        assert np.ptp(got[k][..., 0]) > 32, "a picture, not a constant"
        assert not got[k][..., 1:].any()


def _states(W, H, fmt, frames):
    """(mm_get_state after the frames, mm_compute_state of the last one), as bytes."""
    import torch
    import mm355
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = torch.from_numpy(np.stack(frames)).cuda()
    out = torch.empty_like(dev)
    for k in range(len(frames)):
        h.process(dev[k], out[k], fmt)
    held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    made = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.get_state(held)
    h.compute_state(dev[len(frames) - 1], fmt, made)
    torch.cuda.synchronize()
    res = held.cpu().numpy(), made.cpu().numpy()
    h.close()
    return res


@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
def test_rgb24_state_is_the_rgba8_frames_state_bitwise(W, H):
    """Identity 1 and 2 on the state: K1 forms the same exact integer luma."""
    import mm355
    fr = rgb24.frames(W, H, 2)
    held8, made8 = _states(W, H, mm355.RGBA8, [rgb24.twin(f) for f in fr])
    assert np.array_equal(held8, made8) and np.abs(held8.view(np.float32)).max() > 1.0
    for order in ORDERS:
        held, made = _states(W, H, rgb24.fmt_of(order), [rgb24.in_order(f, order) for f in fr])
        assert np.array_equal(held, held8), order
        assert np.array_equal(made, made8), order


@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
def test_bgr24_is_rgb24_on_the_swapped_frame(W, H):
    """Identity 2: the same picture in both orders gives the same picture."""
    n = 4
    fr = rgb24.frames(W, H, n)
    for kw in (dict(mode="stream", batch=8), dict(mode="frame", batch=1)):
        a = T.gpu_run(W, H, list(fr), L, S, fmt=rgb24.fmt_of("rgb"), **kw)
        b = T.gpu_run(W, H, [rgb24.swap(f) for f in fr], L, S, fmt=rgb24.fmt_of("bgr"), **kw)
        assert (a[1] != fr[1]).mean() > 0.5
        _same([rgb24.swap(x) for x in b], a, kw["mode"])
    # and they are different calls: RGB24 on the swapped bytes is another picture
    c = T.gpu_run(W, H, [rgb24.swap(f) for f in fr], L, S, fmt=rgb24.fmt_of("rgb"), mode="stream")
    assert not np.array_equal(rgb24.swap(c[1]), a[1])


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_saturate_stress(order):
    """Bytes stretched about 128 by a gain of 3: the output clamp is really
    exercised (>= 1 % of the reference's bytes sit at 0 or 255)."""
    W, H, n = 200, 120, 4
    fr, ref = rgb24.frames(W, H, n, stretch=True), _ref(W, H, n, stretch=True)
    assert ((np.stack(fr) == 0) | (np.stack(fr) == 255)).mean() > 0.2
    for k in range(1, n):
        assert ((ref[k] == 0) | (ref[k] == 255)).mean() >= 0.01, k
    for kw in (dict(mode="frame", batch=1), dict(mode="stream", batch=8)):
        _check(_run(W, H, fr, order, L, S, **kw), fr, ref, f"{order} stretched {kw['mode']}")


def _pitched(W, H, n, fmt, fr, lin, lout, in_base, out_base, mode):
    """One run with pitched surfaces; returns (input buffer after, its source,
    output buffer, its sentinel, sizes)."""
    import torch
    import mm355
    in_size = in_base + (n - 1) * lin.frame_stride + lin.bytes(W, H) + 64
    out_size = out_base + (n - 1) * lout.frame_stride + lout.bytes(W, H) + 64
    src = rgb24.scatter(fr, lin.pitch, lin.frame_stride, in_size, base=in_base)
    sent = rgb24.sentinel(out_size)
    a, b = torch.from_numpy(src).cuda(), torch.from_numpy(sent).cuda()
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    h.set_batch(8)
    if mode == "stream":
        h.process_stream_surfaces(a[in_base:], lin, b[out_base:], lout, n)
    else:
        for k in range(n):
            h.process_surface(a[in_base + k * lin.frame_stride:], lin, b[out_base + k * lout.frame_stride:], lout)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    assert np.array_equal(a.cpu().numpy(), src), "the input surface is read only"
    keep = ~rgb24.sample_mask(W, H, n, lout.pitch, lout.frame_stride, out_size, base=out_base)
    bad = np.flatnonzero(keep & (res != sent))
    assert bad.size == 0, f"{mode}: {bad.size} padding bytes written, first at {bad[:8]}"
    return rgb24.gather(res, W, H, n, lout.pitch, lout.frame_stride, base=out_base)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,H", [(200, 120), (97, 63), (98, 62)])
def test_rgb24_pitched_surfaces(W, H, order):
    """aligned(256, 16) in; out: pitch 3 W + 3, frame stride extent + 5, base
    offset 1.  The sentinel bytes in all padding (the byte after a row's last
    pixel included) stay as they were, the input surface is unchanged, and the
    samples are bytewise the tight run's (the first frame's passthrough through
    k_copy_rows included)."""
    import mm355
    n, fmt = 4, rgb24.fmt_of(order)
    fr = [rgb24.in_order(f, order) for f in rgb24.frames(W, H, n)]
    want = T.gpu_run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
    lin = mm355.Surface.aligned(W, H, fmt, 256, 16)
    lout = mm355.Surface(format=fmt, pitch=3 * W + 3)
    lout.frame_stride = lout.bytes(W, H) + 5
    for mode in ("stream", "frame"):
        _same(_pitched(W, H, n, fmt, fr, lin, lout, 0, 1, mode), want, f"{mode} aligned in, unaligned out")


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_pitched_surfaces_reversed(order):
    """Unaligned in (base offset 1, pitch 3 W + 3), aligned(256, 16) out: the
    12-byte quads need both sides on multiples of 4, so this layout takes the
    unfused kernels: the same bytes."""
    import mm355
    W, H, n, fmt = 200, 120, 4, rgb24.fmt_of(order)
    fr = [rgb24.in_order(f, order) for f in rgb24.frames(W, H, n)]
    want = T.gpu_run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
    lin = mm355.Surface(format=fmt, pitch=3 * W + 3)
    lin.frame_stride = lin.bytes(W, H) + 5
    lout = mm355.Surface.aligned(W, H, fmt, 256, 16)
    for mode in ("stream", "frame"):
        _same(_pitched(W, H, n, fmt, fr, lin, lout, 1, 0, mode), want, f"{mode} unaligned in, aligned out")
    # aligned on both sides (pitch 768): the fused kernels' quads at a pitch that is not 3 W
    _same(_pitched(W, H, n, fmt, fr, lout, lout, 0, 0, "stream"), want, "aligned in and out")


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_apply_off_passes_through_and_keeps_state(order):
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fmt = rgb24.fmt_of(order)
    fr = [rgb24.in_order(f, order) for f in rgb24.frames(W, H, n)]
    got = T.gpu_run(W, H, fr, L, S, mode="stream", apply=False, fmt=fmt)
    _same(got, fr, "apply_magnification = 0")
    # the state still follows the input: compute_state(last frame) == the held state
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S, apply_magnification=False))
    dev = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.empty_like(dev)
    h.process_stream(dev, out, n, fmt)
    held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    made = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.get_state(held)
    h.compute_state(dev[n - 1], fmt, made)
    torch.cuda.synchronize()
    assert torch.equal(held, made)
    h.close()


@pytest.mark.parametrize("order", ORDERS)
def test_rgb24_on_render_image_named_format(order):
    """OnRenderImage(fmt=): [H, W, 3] device tensors, a view at pixel offset
    (4, 7) of a larger tensor (byte offset 21: misaligned) and host numpy
    arrays all give the bytes of the C-ABI call; an unnamed frame raises."""
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fmt = rgb24.fmt_of(order)
    fr = [rgb24.in_order(f, order) for f in rgb24.frames(W, H, n)]
    want = T.gpu_run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
    assert (want[1] != fr[1]).mean() > 0.5
    # contiguous device tensors
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(n):
        src = torch.from_numpy(fr[k]).cuda()
        dst = torch.empty_like(src)
        proc.OnRenderImage(src, dst, fmt=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want[k]), k
    with pytest.raises(mm355.MMError) as ei:
        proc.OnRenderImage(src, dst)
    assert ei.value.code == -1 and "RGB24" in str(ei.value) and "BGR24" in str(ei.value)
    proc.OnDestroy()
    # a region of interest of a larger tensor, on both sides
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    big_in = torch.zeros((H + 9, W + 11, 3), dtype=torch.uint8, device="cuda")
    big_out = torch.full((H + 9, W + 11, 3), 7, dtype=torch.uint8, device="cuda")
    vin, vout = big_in[4:4 + H, 7:7 + W], big_out[4:4 + H, 7:7 + W]
    assert (vin.data_ptr() - big_in.data_ptr()) % (3 * (W + 11)) == 21
    for k in range(n):
        vin.copy_(torch.from_numpy(fr[k]).cuda())
        proc.OnRenderImage(vin, vout, fmt=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(vout.cpu().numpy(), want[k]), k
    edge = big_out.clone()
    edge[4:4 + H, 7:7 + W] = 7
    assert bool((edge == 7).all()), "nothing outside the view is written"
    proc.OnDestroy()
    # host numpy arrays (synchronous), a cv2 frame as it is
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(n):
        dst = np.empty_like(fr[k])
        proc.OnRenderImage(fr[k], dst, fmt=fmt)
        assert np.array_equal(dst, want[k]), k
    proc.OnDestroy()


def test_refusals_leave_the_stream_untouched():
    """Invalid codes, differing in / out orders and a debug-view-free sanity
    call between the frames of an RGB24 stream: each refused before anything is
    queued, the stream continues bitwise as if they had never been made."""
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fr = list(rgb24.frames(W, H, n))
    want = T.gpu_run(W, H, fr, L, S, mode="frame", batch=1, fmt=mm355.RGB24)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.zeros_like(dev)
    junk = torch.full_like(dev[0], 9)
    state = torch.full((h.state_bytes,), 9, dtype=torch.uint8, device="cuda")
    tight = {f: mm355.Surface.tight(W, H, f) for f in mm355.RGB24_FORMATS}
    for k in range(n):
        for bad in (0 | 128, 3 | 128, 14, 13 | 32, 13 | 64, 141 | 32, 13 | 256, -13):
            for call in (lambda: h.process(dev[k], junk, bad), lambda: h.process_stream(dev, junk, 1, bad),
                         lambda: h.compute_state(dev[k], bad, state)):
                with pytest.raises(mm355.MMError) as ei:
                    call()
                assert ei.value.code == -1, bad
        for a, b in ((mm355.RGB24, mm355.BGR24), (mm355.BGR24, mm355.RGB24)):
            for call in (lambda: h.process_surface(dev[k], tight[a], junk, tight[b]),
                         lambda: h.process_stream_surfaces(dev[k], tight[a], junk, tight[b], 1)):
                with pytest.raises(mm355.MMError) as ei:
                    call()
                assert ei.value.code == -1, (a, b)
        with pytest.raises(mm355.MMError):                # a pitch shorter than a row
            h.process_surface(dev[k], mm355.Surface(format=mm355.RGB24, pitch=3 * W - 1), junk, tight[mm355.RGB24])
        h.process_stream(dev[k], junk, 0, mm355.RGB24)    # the sanity call: no frames, MM_OK, nothing changes
        h.process(dev[k], out[k], mm355.RGB24)
    torch.cuda.synchronize()
    assert bool((junk == 9).all()) and bool((state == 9).all()), "a refused call writes nothing"
    _same(list(out.cpu().numpy()), want, "the stream around the refusals")
    h.close()


def _ppm_stream(frames):
    return b"".join(f"P6\n{f.shape[1]} {f.shape[0]}\n255\n".encode() + np.ascontiguousarray(f).tobytes()
                    for f in frames)


@pytest.mark.parametrize("flags", [[], ["--bgr"], ["--surface-align", "256,16"], ["--bgr", "--standard"]])
def test_cli_ppm_matches_binding(tmp_path, flags):
    """mm_cli --ppm [--bgr] on a 200x120 clip of 4 frames gives the same
    container back, its bytes the binding's output (--bgr swaps on read and on
    write: the file is the run without it)."""
    W, H, n = 200, 120, 4
    fr = rgb24.frames(W, H, n)
    src, dst = str(tmp_path / "in.ppm"), str(tmp_path / "out.ppm")
    with open(src, "wb") as f:
        f.write(_ppm_stream(fr))
    subprocess.check_call([CLI, "--ppm", "-i", src, "-o", dst, "-l", str(L), "-s", str(S), "-b", "4"] + flags,
                          timeout=120)
    std = {} if "--standard" in flags else None
    want = _run(W, H, fr, "bgr" if "--bgr" in flags else "rgb", L, S, mode="stream", batch=8, standard=std)
    assert (want[1] != fr[1]).mean() > 0.5
    raw = open(dst, "rb").read()
    assert raw == _ppm_stream(want)
