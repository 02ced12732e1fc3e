"""MM_BGRA8 / MM_BGRA8_SRGB frames through the C-ABI on the HIP path.

A BGRA frame IS the MM_RGBA8 (MM_RGBA8_SRGB) frame with bytes 0 and 2 of every
pixel exchanged (include/mm.h "BGRA frames"; bgra.swap).  No tolerance is
introduced here: every check is BITWISE against the RGBA path on the same GPU,
which test_gpu_parity.py, test_formats.py, test_convert.py and test_lanes.py
hold to the oracle.
  1. out_BGRA8(x) == swap(out_RGBA8(swap(x))), alpha byte included;
  2. the temporal state is bitwise that RGBA8 frame's;
  3. the first frame and apply_magnification = 0 pass all 4 W H bytes through.
Inputs are the project's synthetic stream with a non-trivial alpha plane
(bgra.frames), L = 5, S = 25.

Kernels reached: K1 k_rows_fwd<.., kFmtBGRA8 / kFmtBGRA8S> in its regular,
one-pair and GEN forms at N = 64 .. 8192; k_rows_inv_compose staged by LDS-DMA
and with register loads, k_rows_inv_compose4, k_compose, k_compose_odd,
k_dbg_out, k_copy_rows, k_convert and the three BGRA pairs of the compose kernels.
"""
import os
import subprocess

import numpy as np
import pytest

import bgra
import convert as C
import mmtest as T
from bgra import L, S, same, swap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")

# W, H, frames, edge, MM_K34_ROWS of the stream leg
GEOMETRIES = [
    (64, 48, 4, 0, None),        # x0 = 0: unfused pair; K1 one-pair form
    (200, 120, 4, 0, None),      # k_rows_inv_compose4
    (200, 120, 12, 0, "64"),     # the walking fused K34, staged by LDS-DMA
    (98, 62, 4, 0, None),        # W % 8 != 0: unfused
    (97, 63, 4, 0, None),        # odd: GEN K1 and k_compose_odd
    (128, 128, 4, 0, None),      # no margins, every border wraps
    (128, 128, 4, 1, None),      # ... or clamps
    (1920, 128, 3, 0, None),     # N = 2048
    (4104, 48, 2, 0, None),      # N = 8192
]


def _fmts():
    import mm355
    return mm355.BGRA8, mm355.BGRA8_SRGB


@pytest.mark.parametrize("W,H,n,edge,rows", GEOMETRIES)
def test_bgra8_is_the_rgba8_path_on_the_swapped_frames(W, H, n, edge, rows):
    """Identity 1 over single calls and the stream form."""
    fmt = _fmts()[0]
    fr = bgra.frames(W, H, n)
    sent = [swap(f) for f in fr]
    got = bgra.run(W, H, fr, fmt, L, S, edge, mode="frame", batch=1)
    same(got, bgra.run_twin(W, H, fr, fmt, L, S, edge, mode="frame", batch=1), "frame calls")
    assert np.array_equal(got[0], sent[0]), "the first frame passes through, alpha included"
    bgra.ran(got, sent, "frame calls")
    for g in got[1:]:
        assert int(g[..., 3].min()) == 255, "output alpha after the first frame"
    with bgra.env(MM_K34_ROWS=rows):
        batch = 12 if rows else 8
        got = bgra.run(W, H, fr, fmt, L, S, edge, mode="stream", batch=batch)
        same(got, bgra.run_twin(W, H, fr, fmt, L, S, edge, mode="stream", batch=batch), "stream")
    bgra.ran(got, sent, "stream")


def test_bgra8_host_memory_calls():
    W, H, n = 200, 120, 3
    fmt = _fmts()[0]
    fr = bgra.frames(W, H, n)
    got = bgra.run(W, H, fr, fmt, L, S, mode="host")
    same(got, bgra.run_twin(W, H, fr, fmt, L, S, mode="host"), "host calls")
    bgra.ran(got, [swap(f) for f in fr], "host calls")


@pytest.mark.parametrize("W,H,n,rows", [(200, 120, 4, None), (200, 120, 12, "64"), (97, 63, 4, None)])
def test_bgra8_srgb_is_the_rgba8_srgb_path(W, H, n, rows):
    fmt = _fmts()[1]
    fr = bgra.frames(W, H, n)
    got = bgra.run(W, H, fr, fmt, L, S, mode="frame", batch=1)
    same(got, bgra.run_twin(W, H, fr, fmt, L, S, mode="frame", batch=1), "frame calls")
    bgra.ran(got, [swap(f) for f in fr], "sRGB")
    with bgra.env(MM_K34_ROWS=rows):
        batch = 12 if rows else 8
        same(bgra.run(W, H, fr, fmt, L, S, mode="stream", batch=batch),
             bgra.run_twin(W, H, fr, fmt, L, S, mode="stream", batch=batch), "stream")
    # and it is another format than MM_BGRA8: the same bytes give another picture
    assert not np.array_equal(bgra.run(W, H, fr[:2], _fmts()[0], L, S)[1], got[1])


@pytest.mark.parametrize("fmt_i", [0, 1])
def test_standard_mode(fmt_i):
    W, H, n = 128, 96, 4
    fmt = _fmts()[fmt_i]
    fr = bgra.frames(W, H, n)
    for kw in (dict(mode="frame", batch=1), dict(mode="stream", batch=8)):
        got = bgra.run(W, H, fr, fmt, L, S, standard={}, **kw)
        same(got, bgra.run_twin(W, H, fr, fmt, L, S, standard={}, **kw), f"standard {kw['mode']}")
        bgra.ran(got, [swap(f) for f in fr], "standard")


def test_steerable_mode():
    W, H, n = 200, 120, 4
    fmt = _fmts()[0]
    extra = {"mode": 2, "orientations": 4}                # O = 4, DIFF
    fr = bgra.frames(W, H, n)
    got = bgra.run(W, H, fr, fmt, L, S, mode="stream", extra=extra)
    same(got, bgra.run_twin(W, H, fr, fmt, L, S, mode="stream", extra=extra), "steerable")
    assert np.array_equal(got[0], swap(fr[0]))
    bgra.ran(got, [swap(f) for f in fr], "steerable")


@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
@pytest.mark.parametrize("debug", [(1, 0), (0, 1), (1, 1)])
def test_debug_views(debug, W, H):
    """The RGBA8 view with bytes 0 and 2 exchanged: the view's value in byte 2."""
    n = 3
    for fmt in _fmts():
        fr = bgra.frames(W, H, n)
        got = bgra.run(W, H, fr, fmt, L, S, mode="stream", debug=debug)
        same(got, bgra.run_twin(W, H, fr, fmt, L, S, mode="stream", debug=debug), f"debug {debug} fmt {fmt}")
        for k in range(1, n):
            assert np.ptp(got[k][..., 2]) > 32, "a picture, not a constant"
            assert not got[k][..., :2].any() and int(got[k][..., 3].min()) == 255


def _surface_run(W, H, fr, fmt, lay, base, n):
    """The stream form on one pitched layout for both sides, frames scattered
    from `base`; -> the output samples."""
    import torch
    import mm355
    size = base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + 64
    a = torch.from_numpy(bgra.scatter(fr, lay.pitch, lay.frame_stride, size, base=base)).cuda()
    b = torch.from_numpy(bgra.sentinel(size)).cuda()
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    h.set_batch(12)
    h.process_stream_surfaces(a[base:], lay, b[base:], lay, n)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    return bgra.gather(res, W, H, n, lay.pitch, lay.frame_stride, base=base)


def test_compose_forms_agree_bytewise():
    """The walking K34 at two strip heights (staged by LDS-DMA), the unfused pair,
    and the register-load K34 of a surface whose rows lie at 4 mod 16."""
    import mm355
    W, H, n = 200, 120, 12
    for fmt in _fmts():
        fr = bgra.frames(W, H, n)
        sent = [swap(f) for f in fr]
        base = None
        for rows in ("0", "16", "64"):
            with bgra.env(MM_K34_ROWS=rows):
                got = bgra.run(W, H, fr, fmt, L, S, mode="stream", batch=12)
                if rows == "64":
                    same(got, bgra.run_twin(W, H, fr, fmt, L, S, mode="stream", batch=12), "identity 1, staged")
            base = base or got
            same(got, base, f"MM_K34_ROWS={rows} fmt {fmt}")
        bgra.ran(base, sent)
        lay = mm355.Surface(format=fmt, pitch=4 * W + 4)
        lay.frame_stride = lay.pitch * H
        with bgra.env(MM_K34_ROWS="64"):
            same(_surface_run(W, H, sent, fmt, lay, 4, n), base, f"rows at 4 mod 16, fmt {fmt}")


def _states(W, H, fmt, frames):
    """(mm_get_state after the frames, mm_compute_state_surface of the last one), as bytes."""
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
    h.compute_state_surface(dev[len(frames) - 1], mm355.Surface.tight(W, H, fmt), made)
    torch.cuda.synchronize()
    res = held.cpu().numpy(), made.cpu().numpy()
    h.close()
    return res


@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
def test_state_is_the_rgba8_frames_state_bitwise(W, H):
    """Identity 2: K1 forms the same exact integer luma from the other bytes."""
    import mm355
    fr = bgra.frames(W, H, 3)
    held8, made8 = _states(W, H, mm355.RGBA8, list(fr))
    assert np.array_equal(held8, made8) and np.abs(held8.view(np.float32)).max() > 1.0
    held, made = _states(W, H, mm355.BGRA8, [swap(f) for f in fr])
    assert np.array_equal(held, held8) and np.array_equal(made, made8)
    helds, mades = _states(W, H, mm355.BGRA8_SRGB, [swap(f) for f in fr])
    held3, made3 = _states(W, H, mm355.RGBA8_SRGB, list(fr))
    assert np.array_equal(helds, held3) and np.array_equal(mades, made3)
    assert not np.array_equal(held3, held8)


def test_apply_off_passes_through_and_the_state_follows_the_input():
    import torch
    import mm355
    W, H, n = 200, 120, 3
    for fmt in _fmts():
        sent = [swap(f) for f in bgra.frames(W, H, n)]
        got = T.gpu_run(W, H, sent, L, S, mode="stream", apply=False, fmt=fmt)
        same(got, sent, "apply_magnification = 0")
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S, apply_magnification=False))
        dev = torch.from_numpy(np.stack(sent)).cuda()
        out = torch.empty_like(dev)
        h.process_stream(dev, out, n, fmt)
        held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
        made = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(held)
        h.compute_state(dev[n - 1], fmt, made)
        torch.cuda.synchronize()
        assert torch.equal(held, made)
        h.close()


def _pitched(W, H, n, sent, lin, lout, in_base, out_base):
    """The stream form on pitched surfaces with poisoned padding on both sides;
    -> the output samples.  The input surface stays as it was and no padding
    byte of the output is written."""
    import torch
    import mm355
    in_size = in_base + (n - 1) * lin.frame_stride + lin.bytes(W, H) + 64
    out_size = out_base + (n - 1) * lout.frame_stride + lout.bytes(W, H) + 64
    src = bgra.scatter(sent, lin.pitch, lin.frame_stride, in_size, base=in_base)
    sentinel = bgra.sentinel(out_size)
    a, b = torch.from_numpy(src).cuda(), torch.from_numpy(sentinel).cuda()
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    h.set_batch(8)
    h.process_stream_surfaces(a[in_base:], lin, b[out_base:], lout, n)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    assert np.array_equal(a.cpu().numpy(), src), "the input surface is read only"
    keep = ~bgra.sample_mask(W, H, n, lout.pitch, lout.frame_stride, out_size, base=out_base)
    bad = np.flatnonzero(keep & (res != sentinel))
    assert bad.size == 0, f"{bad.size} padding bytes written, first at {bad[:8]}"
    return bgra.gather(res, W, H, n, lout.pitch, lout.frame_stride, base=out_base)


@pytest.mark.parametrize("W,H", [(200, 120), (97, 63)])
def test_pitched_surfaces(W, H):
    """Decoder layout (256, 16) in, pitch 4 W + 4 and a stride of its own out, and
    a region of interest inside a larger frame: the tight run's samples (the first
    frame's passthrough through k_copy_rows included), padding untouched."""
    import mm355
    n = 4
    for fmt in _fmts():
        sent = [swap(f) for f in bgra.frames(W, H, n)]
        want = T.gpu_run(W, H, sent, L, S, mode="stream", batch=8, fmt=fmt)
        assert np.array_equal(want[0], sent[0])
        lin = mm355.Surface.aligned(W, H, fmt, 256, 16)
        lout = mm355.Surface(format=fmt, pitch=4 * W + 4)
        lout.frame_stride = lout.bytes(W, H) + 12
        same(_pitched(W, H, n, sent, lin, lout, 0, 4), want, f"aligned in, pitched out, fmt {fmt}")
        same(_pitched(W, H, n, sent, lout, lin, 8, 0), want, f"pitched in, aligned out, fmt {fmt}")
        # a region of interest at pixel (5, 7) of a frame 24 columns and 16 rows larger
        roi = mm355.Surface(format=fmt, pitch=4 * (W + 24))
        roi.frame_stride = roi.pitch * (H + 16)
        at = 7 * roi.pitch + 4 * 5
        same(_pitched(W, H, n, sent, roi, roi, at, at), want, f"region of interest, fmt {fmt}")


# ---- convert pairs -----------------------------------------------------------------
CONVERT_GEOMETRIES = [(64, 48, 4, None), (200, 120, 4, None), (200, 120, 12, "64"), (98, 62, 4, None)]


@pytest.mark.parametrize("W,H,n,rows", CONVERT_GEOMETRIES)
@pytest.mark.parametrize("in_fmt", [16, 16 | 32, 18])             # NV12, NV12 | BT709, P010
def test_decode_to_bgra8_is_the_rgba8_decode_swapped(in_fmt, W, H, n, rows):
    import mm355
    fr = C.frames(W, H, n, in_fmt)
    with bgra.env(MM_K34_ROWS=rows):
        for mode, batch in (("frame", 1), ("stream", 12 if rows else 8)):
            got = bgra.convert(W, H, fr, in_fmt, mm355.BGRA8, mode=mode, batch=batch)
            want = C.run(W, H, fr, in_fmt, mm355.RGBA8, L, S, mode=mode, batch=batch)
            same(got, [swap(w) for w in want], f"{mode}")
    # the first frame is the plain conversion, the rest is not
    plain = bgra.convert(W, H, fr, in_fmt, mm355.BGRA8, mode="stream", apply=False)
    assert np.array_equal(got[0], plain[0]) and (got[1][..., :3] != plain[1][..., :3]).mean() > 0.5
    same(plain, [swap(w) for w in C.run(W, H, fr, in_fmt, mm355.RGBA8, L, S, mode="stream", apply=False)], "plain")


@pytest.mark.parametrize("W,H,n,rows", CONVERT_GEOMETRIES)
@pytest.mark.parametrize("out_fmt", [16, 17 | 64])                # NV12, NV12_FULL | BT2020
def test_encode_from_bgra8_is_the_rgba8_encode_on_the_swapped_frames(out_fmt, W, H, n, rows):
    import mm355
    fr = bgra.frames(W, H, n)
    sent = [swap(f) for f in fr]
    with bgra.env(MM_K34_ROWS=rows):
        for mode, batch in (("frame", 1), ("stream", 12 if rows else 8)):
            got = bgra.convert(W, H, sent, mm355.BGRA8, out_fmt, mode=mode, batch=batch)
            same(got, C.run(W, H, list(fr), mm355.RGBA8, out_fmt, L, S, mode=mode, batch=batch), mode)
    plain = bgra.convert(W, H, sent, mm355.BGRA8, out_fmt, mode="stream", apply=False)
    assert np.array_equal(got[0], plain[0]) and (got[1][:H] != plain[1][:H]).mean() > 0.5
    same(plain, C.run(W, H, list(fr), mm355.RGBA8, out_fmt, L, S, mode="stream", apply=False), "plain")


def test_convert_state_and_alternation_on_one_handle():
    """The state after a convert call is the same-format call's on the in format,
    and convert and same-format calls alternate on one handle."""
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fr = bgra.frames(W, H, n)
    sent = [swap(f) for f in fr]

    def state(h):
        buf = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(buf)
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    p = mm355.Params.make(levels=L, phase_scale=S)
    ha, hb = mm355.Handle(W, H, p), mm355.Handle(W, H, p)
    enc = bgra.convert(W, H, sent[:2], mm355.BGRA8, mm355.NV12, handle=ha)
    dev = torch.from_numpy(np.stack(sent)).cuda()
    out = torch.empty_like(dev)
    for k in range(2):
        hb.process(dev[k], out[k], mm355.BGRA8)
    assert np.array_equal(state(ha), state(hb)), "the state is the in format's"
    # frame 2 as a same-format call on the handle that converted, frame 3 converted again
    ha.process(dev[2], out[2], mm355.BGRA8)
    hb.process(dev[2], out[3], mm355.BGRA8)
    torch.cuda.synchronize()
    assert torch.equal(out[2], out[3])
    enc3 = bgra.convert(W, H, sent[3:], mm355.BGRA8, mm355.NV12, handle=ha)
    want = C.run(W, H, list(fr), mm355.RGBA8, mm355.NV12, L, S, mode="frame", batch=1)
    same(enc + enc3, [want[0], want[1], want[3]], "alternating calls")
    ha.close()
    hb.close()
    # a decode's state is the NV12 same-format call's
    nv = C.frames(W, H, 2, mm355.NV12)
    ha, hb = mm355.Handle(W, H, p), mm355.Handle(W, H, p)
    bgra.convert(W, H, nv, mm355.NV12, mm355.BGRA8, handle=ha)
    src = torch.from_numpy(np.stack(nv)).cuda()
    dst = torch.empty_like(src)
    for k in range(2):
        hb.process(src[k], dst[k], mm355.NV12)
    assert np.array_equal(state(ha), state(hb))
    ha.close()
    hb.close()


# ---- lanes ---------------------------------------------------------------------------
def test_lanes_equal_handles_of_their_own():
    """3 lanes, two mm_process_lanes calls and one mm_process_lanes_mask(0b101):
    each lane is a handle of its own, and the lanes' states are the RGBA8 lanes'."""
    import torch
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 3
    fmt = mm355.BGRA8
    fr = bgra.frames(W, H, lanes * ticks)
    clip = np.stack([swap(f) for f in fr]).reshape(ticks, lanes, H, W, 4)      # lane k of tick t: frame t * lanes + k
    twin = np.stack(fr).reshape(ticks, lanes, H, W, 4)
    p = mm355.Params.make(levels=L, phase_scale=S)

    def run(f, frames):
        lay = mm355.Surface.tight(W, H, f)
        src = torch.from_numpy(frames).cuda()
        hl = mm355.Handle(W, H, p)
        hl.set_lanes(lanes)
        hs = [mm355.Handle(W, H, p) for _ in range(lanes)]
        out = torch.zeros_like(src)
        ref = torch.zeros_like(src)
        for t, mask in enumerate((0b111, 0b111, 0b101)):
            if mask == 0b111:
                hl.process_lanes(src[t], lay, out[t], lay)
            else:
                hl.process_lanes_mask(mask, src[t], lay, out[t], lay)
            for k in range(lanes):
                if (mask >> k) & 1:
                    hs[k].process(src[t, k], ref[t, k], f)
        states = []
        for k in range(lanes):
            buf = torch.zeros(hl.state_bytes, dtype=torch.uint8, device="cuda")
            own = torch.ones(hl.state_bytes, dtype=torch.uint8, device="cuda")
            hl.get_lane_state(k, buf)
            hs[k].get_state(own)
            torch.cuda.synchronize()
            assert torch.equal(buf, own), k
            states.append(buf.cpu().numpy())
        torch.cuda.synchronize()
        res = out.cpu().numpy(), ref.cpu().numpy(), states
        for h in [hl] + hs:
            h.close()
        return res

    out, ref, states = run(fmt, clip)
    assert np.array_equal(out, ref), "each lane equals a handle of its own"
    assert not out[2, 1].any(), "the unselected lane's slot is untouched"
    assert (out[1, 0][..., :3] != clip[1, 0][..., :3]).mean() > 0.5
    out8, _, states8 = run(mm355.RGBA8, twin)
    assert np.array_equal(out, swap(out8))
    for k in range(lanes):
        assert np.array_equal(states[k], states8[k]), k


# ---- refusals ------------------------------------------------------------------------
def test_refusals_leave_the_next_output_unchanged():
    import torch
    import mm355
    W, H, n = 200, 120, 3
    sent = [swap(f) for f in bgra.frames(W, H, n)]
    want = T.gpu_run(W, H, sent, L, S, mode="frame", batch=1, fmt=mm355.BGRA8)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = torch.from_numpy(np.stack(sent)).cuda()
    out = torch.zeros_like(dev)
    junk = torch.full((dev[0].numel() + 16,), 9, dtype=torch.uint8, device="cuda")
    state = torch.full((h.state_bytes,), 9, dtype=torch.uint8, device="cuda")
    tight = {f: mm355.Surface.tight(W, H, f) for f in (mm355.RGBA8, mm355.BGRA8, mm355.RGBA8_SRGB, mm355.BGRA8_SRGB)}
    for k in range(n):
        for a, b in ((mm355.RGBA8, mm355.BGRA8), (mm355.BGRA8, mm355.RGBA8), (mm355.BGRA8, mm355.BGRA8_SRGB),
                     (mm355.RGBA8_SRGB, mm355.BGRA8_SRGB)):
            for call in (lambda: h.process_surface(dev[k], tight[a], junk, tight[b]),
                         lambda: h.process_stream_surfaces(dev[k], tight[a], junk, tight[b], 1)):
                with pytest.raises(mm355.MMError) as ei:
                    call()
                assert ei.value.code == -1, (a, b)
            with pytest.raises(mm355.MMError) as ei:
                h.process_convert(dev[k], tight[a], junk, tight[b])
            assert ei.value.code == -2, (a, b)
        for bad in (128, 131, 8193, 8194, 8192 | 32, 8192 | 128, 8192 | 4096, 16384, -8192):
            for call in (lambda: h.process(dev[k], junk, bad), lambda: h.process_stream(dev, junk, 1, bad),
                         lambda: h.compute_state(dev[k], bad, state)):
                with pytest.raises(mm355.MMError) as ei:
                    call()
                assert ei.value.code == -1, bad
        # the unit is 4: a device base or a pitch at 2 mod 4
        with pytest.raises(mm355.MMError) as ei:
            h.process_surface(dev[k], tight[mm355.BGRA8], junk[2:], tight[mm355.BGRA8])
        assert ei.value.code == -1
        with pytest.raises(mm355.MMError) as ei:
            h.process_surface(dev[k], mm355.Surface(format=mm355.BGRA8, pitch=4 * W + 2), junk, tight[mm355.BGRA8])
        assert ei.value.code == -1
        h.process(dev[k], out[k], mm355.BGRA8)
    torch.cuda.synchronize()
    assert bool((junk == 9).all()) and bool((state == 9).all()), "a refused call writes nothing"
    same(list(out.cpu().numpy()), want, "the stream around the refusals")
    h.close()


# ---- binding and CLI -----------------------------------------------------------------
def test_on_render_image_named_format():
    """OnRenderImage(fmt=BGRA8): a device tensor, a strided view of a larger one
    and host arrays all give the bytes of the C-ABI call; so does dst_fmt=."""
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fmt = mm355.BGRA8
    sent = [swap(f) for f in bgra.frames(W, H, n)]
    want = T.gpu_run(W, H, sent, L, S, mode="frame", batch=1, fmt=fmt)
    assert (want[1][..., :3] != sent[1][..., :3]).mean() > 0.5
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(n):
        src = torch.from_numpy(sent[k]).cuda()
        dst = torch.empty_like(src)
        proc.OnRenderImage(src, dst, fmt=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want[k]), k
    proc.OnDestroy()
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    big_in = torch.zeros((H + 9, W + 11, 4), dtype=torch.uint8, device="cuda")
    big_out = torch.full((H + 9, W + 11, 4), 7, dtype=torch.uint8, device="cuda")
    vin, vout = big_in[4:4 + H, 7:7 + W], big_out[4:4 + H, 7:7 + W]
    for k in range(n):
        vin.copy_(torch.from_numpy(sent[k]).cuda())
        proc.OnRenderImage(vin, vout, fmt=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(vout.cpu().numpy(), want[k]), k
    edge = big_out.clone()
    edge[4:4 + H, 7:7 + W] = 7
    assert bool((edge == 7).all()), "nothing outside the view is written"
    proc.OnDestroy()
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(n):
        dst = np.empty_like(sent[k])
        proc.OnRenderImage(sent[k], dst, fmt=fmt)
        assert np.array_equal(dst, want[k]), k
    proc.OnDestroy()
    # dst_fmt: NV12 in, BGRA8 out, host arrays
    nv = C.frames(W, H, 2, mm355.NV12)
    dec = bgra.convert(W, H, nv, mm355.NV12, fmt, mode="frame", batch=1)
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(2):
        dst = np.zeros((H, W, 4), np.uint8)
        proc.OnRenderImage(nv[k], dst, fmt=mm355.NV12, dst_fmt=fmt)
        assert np.array_equal(dst, dec[k]), k
    proc.OnDestroy()


def _ppm_stream(frames):
    return b"".join(f"P6\n{f.shape[1]} {f.shape[0]}\n255\n".encode() + np.ascontiguousarray(f).tobytes()
                    for f in frames)


def test_cli_ppm_bgra_is_ppm_byte_for_byte(tmp_path):
    W, H, n = 200, 120, 4
    fr = [np.ascontiguousarray(f[..., :3]) for f in bgra.frames(W, H, n)]
    src = str(tmp_path / "in.ppm")
    with open(src, "wb") as f:
        f.write(_ppm_stream(fr))
    outs = []
    for name, flags in (("rgb.ppm", []), ("bgra.ppm", ["--bgra"]), ("bgra_pitched.ppm", ["--bgra", "--surface-align", "256,16"])):
        dst = str(tmp_path / name)
        subprocess.check_call([CLI, "--ppm", "-i", src, "-o", dst, "-l", str(L), "-s", str(S), "-b", "4"] + flags,
                              timeout=120)
        outs.append(open(dst, "rb").read())
    assert len(outs[0]) == len(_ppm_stream(fr)) and outs[0] != _ppm_stream(fr)
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_cli_out_bgra8_is_out_rgba8_swapped(tmp_path):
    W, H, n = 200, 120, 4
    src = str(tmp_path / "in.y4m")
    with open(src, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420\n".encode())
        for b in C.frames(W, H, n, 16):
            y, c = b[:H], b[H:].reshape(H // 2, W // 2, 2)
            f.write(b"FRAME\n" + y.tobytes() + np.ascontiguousarray(c[..., 0]).tobytes() +
                    np.ascontiguousarray(c[..., 1]).tobytes())
    outs = []
    for flag in ("--out-rgba8", "--out-bgra8"):
        dst = str(tmp_path / (flag[2:] + ".raw"))
        subprocess.check_call([CLI, "--nv12", flag, "-i", src, "-o", dst, "-l", str(L), "-s", str(S), "-b", "4"],
                              timeout=120)
        outs.append(np.fromfile(dst, np.uint8).reshape(n, H, W, 4))
    assert np.array_equal(outs[1], swap(outs[0]))
    assert (outs[0][1][..., 0] != outs[0][1][..., 2]).any()
