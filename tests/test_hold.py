"""A held reference frame: mm_set_hold / mm_set_lanes_hold (include/mm.h "Held
reference frame").

The contract is bitwise.  While hold is set, the output of frame x is the output
a handle of its own with the same parameters gives for mm_set_state(R) followed
by one one-frame call on x, R being the state the holding handle had when its
call began; and mm_get_state after the call returns R bit for bit.  That twin is
what every bitwise test below compares against: a handle of its own that gets
set_state(R), R = compute_state(x0), before every one-frame call.  It uses entry
points from before the hold only.  One test compares with the CPU oracle as
well, so held frames are right and not merely equal to their twins.

The shapes are those by which test_lanes.py reaches each K2 configuration; the
frame counts make the tails run (26 frames in one batch) and a call cross batch
boundaries (set_batch(5), 12 frames)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before anything loads the library: torch brings the HIP runtime both share)

import mmtest as T
import mono
import nv12
import oracle_py as O
import surface as SF
import yuv422

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")
L, S = 5, 25.0
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _fmt(name):
    import mm355
    return {"rgba8": mm355.RGBA8, "nv12": mm355.NV12, "yuy2": mm355.YUY2, "y16": mm355.Y16}[name]


def _encode(name, rgba):
    """An RGBA8 picture as one tight frame of the format, as bytes."""
    if name == "rgba8":
        e = rgba
    elif name == "nv12":
        e = nv12.encode(rgba)
    elif name == "yuy2":
        e = yuv422.encode(rgba)
    else:
        e = mono.encode(rgba[..., :3].astype(np.float64) / 255.0, 16)
    return np.ascontiguousarray(e).view(np.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def _clip(W, H, name, n, seed=0x5EED0000):
    """uint8 [n][frame bytes]: a synthetic stream in the format, made once per shape."""
    return np.stack([_encode(name, f) for f in T.synth(W, H, n, seed=seed, fmt="u8")])


def _params(**kw):
    import mm355
    kw.setdefault("levels", L)
    kw.setdefault("phase_scale", S)
    if kw.pop("standard", False):
        kw.update(mode=mm355.MODE_STANDARD, **T._std_fields({}))
    return mm355.Params.make(**kw)


def _code(call):
    import mm355
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def _state(h, lane=None):
    st = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    if lane is None:
        h.get_state(st)
    else:
        h.get_lane_state(lane, st)
    return st


class Twin:
    """The reference of the contract: a handle of its own; frame x against the
    reference frame r is set_state(compute_state(r)) and one one-frame call on x."""

    def __init__(self, W, H, li, lo=None, **pk):
        import mm355
        self.h = mm355.Handle(W, H, _params(**pk))
        self.li, self.lo = li, lo or li
        self.fbo = mm355.frame_bytes(W, H, self.lo.format)
        self.call = self.h.process_convert if self.li.format != self.lo.format else self.h.process_surface

    def state_of(self, frame):
        st = torch.zeros(self.h.state_bytes, dtype=torch.uint8, device="cuda")
        self.h.compute_state_surface(frame, self.li, st)
        return st

    def run(self, R, frames, size=None):
        """[len(frames)][output bytes]: each frame against the state R."""
        out = torch.zeros((len(frames), size or self.fbo), dtype=torch.uint8, device="cuda")
        for k in range(len(frames)):
            self.h.set_state(R)
            self.call(frames[k], self.li, out[k], self.lo)
        torch.cuda.synchronize()
        return out

    def close(self):
        self.h.close()


def _same(a, b, what):
    assert a.shape == b.shape, what
    for k in range(a.shape[0]):
        assert torch.equal(a[k], b[k]), (what, "frame", k, int((a[k] != b[k]).sum()))


# ---- 1. the stream, every K2 instance, bitwise ---------------------------------------
# W, H, format, parameters, frames
CASES = [
    (200, 120, "rgba8", {}, 26),                       # N = 256, several groups per workgroup; tabled one-band op
    (200, 120, "rgba8", {"levels": 6}, 26),            # 0.05 / 0.45: the two-band op
    (200, 120, "rgba8", {"levels": 7}, 26),            # the generic op
    (200, 120, "rgba8", {"standard": True}, 26),       # standard mode
    (97, 63, "rgba8", {"edge_mode": 1}, 26),           # odd, N = 128, clamp
    (640, 360, "yuy2", {}, 26),                        # N = 1024
    (1100, 64, "rgba8", {}, 26),                       # N = 2048, two columns per workgroup, hoisted table bases
    (2100, 64, "y16", {}, 26),                         # N = 4096, the 30 % tail
    (4100, 16, "rgba8", {}, 3),                        # N = 8192
    # the small sizes' standard-mode hold instances are laid out unlike their twins (about 1,000
    # instructions fewer: profiles/hold_isa_counts.txt), and N = 512 has no case above
    (97, 63, "rgba8", {"standard": True}, 26),         # N = 128, standard mode, odd
    (60, 44, "rgba8", {"standard": True}, 26),         # N = 64, standard mode
    (30, 22, "rgba8", {"standard": True}, 26),         # N = 32, standard mode
    (400, 300, "rgba8", {}, 26),                       # N = 512
]


@pytest.mark.parametrize("W,H,name,pk,n", CASES,
                         ids=[f"{c[0]}x{c[1]}-{c[2]}" + "".join(f"-{k}{v}" for k, v in c[3].items()) for c in CASES])
def test_held_stream_equals_its_twin_bitwise(W, H, name, pk, n):
    import mm355
    fmt = _fmt(name)
    lay = mm355.Surface.tight(W, H, fmt)
    src = torch.from_numpy(_clip(W, H, name, n)).cuda()
    tw = Twin(W, H, lay, **pk)
    R = tw.state_of(src[0])
    want = tw.run(R, src)
    tw.close()
    h = mm355.Handle(W, H, _params(**pk))
    assert n <= h.batch, "the first call is one batch: the tails run"
    h.set_hold(True)
    got = torch.zeros_like(src)
    h.process_stream(src, got, n, fmt)                 # no state: frame 0 passes through and becomes R
    torch.cuda.synchronize()
    assert torch.equal(got[0], src[0]), "the first frame passes through"
    _same(got[1:], want[1:], "one batch")
    assert torch.equal(_state(h), R), "the state is frame 0's"
    assert (got[n - 1] != src[n - 1]).float().mean() > 0.05, "the operator ran"
    # a call that crosses batch boundaries, with state: every frame pairs with R, frame 0 too
    m = min(n, 12)
    h.set_batch(5 if n > 3 else 2)
    assert torch.equal(_state(h), R), "set_batch keeps R"
    got.zero_()
    h.process_stream(src, got, m, fmt)
    torch.cuda.synchronize()
    _same(got[:m], want[:m], "batches of 5")
    assert torch.equal(_state(h), R), "the state stays"
    # one-frame calls
    for k in (m - 1, 1):
        h.process(src[k], got[0], fmt)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[k]), ("one-frame call", k)
    assert torch.equal(_state(h), R)
    h.close()


# ---- 2. not vacuous ------------------------------------------------------------------
def test_held_outputs_differ_from_rolling_outputs():
    import mm355
    W, H, n = 200, 120, 7
    src = torch.from_numpy(_clip(W, H, "rgba8", 26)[:n]).cuda()
    out = []
    for hold in (False, True):
        h = mm355.Handle(W, H, _params())
        h.set_hold(hold)
        o = torch.zeros_like(src)
        h.process_stream(src, o, n, mm355.RGBA8)
        torch.cuda.synchronize()
        h.close()
        out.append(o.cpu().numpy().reshape(n, H, W, 4)[..., :3])
    assert np.array_equal(out[0][1], out[1][1]), "frame 1 pairs with frame 0 either way"
    for k in (2, 3, 6):
        share = float((out[0][k] != out[1][k]).mean())
        print(f"frame {k}: {share:.3f} of the colour bytes differ")
        assert share > 0.5, (k, share)


# ---- 3. against the CPU oracle -------------------------------------------------------
def test_held_frames_vs_oracle():
    import mm355
    W, H, n = 200, 120, 25
    frames = T.synth(W, H, n, fmt="u8")
    src = torch.from_numpy(np.stack(frames)).cuda()
    got = torch.zeros_like(src)
    h = mm355.Handle(W, H, _params())
    h.set_hold(True)
    h.process_stream(src, got, n, mm355.RGBA8)
    torch.cuda.synchronize()
    h.close()
    got = got.cpu().numpy()
    assert np.array_equal(got[0], frames[0])
    for k in (1, 2, 3, 5, 8, 12, 24):
        o = O.Oracle(W, H, levels=L, phase_scale=S)
        o.process(frames[0])
        ref = o.process(frames[k])
        o.close()
        d = np.abs(got[k].astype(np.int32) - ref.astype(np.int32))
        print(f"lag {k}: max {d.max()}  share {(d > 0).mean():.2e}")
        T.assert_close_u8(got[k], ref)


# ---- 4. the first frame and toggles ---------------------------------------------------
def test_first_frame_and_toggles():
    import mm355
    W, H, n = 200, 120, 12
    fmt = mm355.RGBA8
    lay = mm355.Surface.tight(W, H, fmt)
    clip = _clip(W, H, "rgba8", 26)[:n]
    src = torch.from_numpy(clip).cuda()
    tw = Twin(W, H, lay)
    R0, R5, R9 = tw.state_of(src[0]), tw.state_of(src[5]), tw.state_of(src[9])
    h = mm355.Handle(W, H, _params())
    got = torch.zeros_like(src)
    assert h.hold() is False
    h.set_hold(True)
    assert h.hold() is True
    # reset plus hold plus a stream: frame 0 comes back bitwise and is R
    h.reset()
    h.process_stream(src[:5], got[:5], 5, fmt)
    torch.cuda.synchronize()
    assert torch.equal(got[0], src[0]) and torch.equal(_state(h), R0)
    _same(got[1:5], tw.run(R0, src[1:5]), "against frame 0")
    # hold off for one frame: still against the old R, and that frame is the new R
    h.set_hold(False)
    h.process(src[5], got[5], fmt)
    torch.cuda.synchronize()
    assert torch.equal(got[5], tw.run(R0, src[5:6])[0]), "the re-referencing frame pairs with the old R"
    assert torch.equal(_state(h), R5), "... and is the new one"
    h.set_hold(True)
    h.process_stream(src[6:9], got[6:9], 3, fmt)
    h.set_batch(2)                                       # set_batch between calls keeps R
    h.process_stream(src[9:12], got[9:12], 3, fmt)
    torch.cuda.synchronize()
    _same(got[6:12], tw.run(R5, src[6:12]), "against frame 5")
    assert torch.equal(_state(h), R5)
    # set_state of another frame's state mid-stream
    h.set_state(R9)
    h.process_stream(src[2:6], got[2:6], 4, fmt)
    torch.cuda.synchronize()
    _same(got[2:6], tw.run(R9, src[2:6]), "against frame 9, installed with set_state")
    assert torch.equal(_state(h), R9)
    # a host-memory one-frame call
    o = np.zeros_like(clip[0])
    h.process(clip[7], o, fmt, on_device=False)
    assert np.array_equal(o, tw.run(R9, src[7:8])[0].cpu().numpy()), "host memory"
    assert torch.equal(_state(h), R9)
    # apply_magnification = 0 with state: every frame passes through, nothing else happens
    h.set_params(_params(apply_magnification=False))
    h.process_stream(src[:4], got[:4], 4, fmt)
    torch.cuda.synchronize()
    assert torch.equal(got[:4], src[:4]) and torch.equal(_state(h), R9)
    # ... without state: the first frame of the call becomes R
    h.reset()
    h.process_stream(src[5:9], got[5:9], 4, fmt)
    torch.cuda.synchronize()
    assert torch.equal(got[5:9], src[5:9]) and torch.equal(_state(h), R5)
    h.process_stream(src[9:11], got[9:11], 2, fmt)
    torch.cuda.synchronize()
    assert torch.equal(got[9:11], src[9:11]) and torch.equal(_state(h), R5)
    h.set_params(_params())
    h.process_stream(src[1:4], got[1:4], 3, fmt)
    torch.cuda.synchronize()
    _same(got[1:4], tw.run(R5, src[1:4]), "magnification on again")
    # switching hold off: the first frame pairs with R, then the state follows the input
    h.set_hold(False)
    h.process_stream(src[6:9], got[6:9], 3, fmt)
    torch.cuda.synchronize()
    roll = mm355.Handle(W, H, _params())
    roll.set_state(R5)
    want = torch.zeros_like(src[6:9])
    roll.process_stream(src[6:9], want, 3, fmt)
    torch.cuda.synchronize()
    _same(got[6:9], want, "hold off: as always")
    assert torch.equal(_state(h), _state(roll))
    for x in (roll, h):
        x.close()
    tw.close()


def test_processor_hold_reference_and_rehold():
    """MotionMagnificationProcessor(hold_reference=True): the first frame is the
    reference; rehold() makes the next frame the new one (one frame with hold off)."""
    import mm355
    W, H, n = 200, 120, 8
    src = torch.from_numpy(_clip(W, H, "rgba8", 26)[:n].reshape(n, H, W, 4)).cuda()
    dst = torch.zeros_like(src)
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S, hold_reference=True).Start()
    assert proc.handle.hold() is True
    for k in range(n):
        if k == 4:
            proc.rehold()
        proc.OnRenderImage(src[k], dst[k])
    torch.cuda.synchronize()
    assert proc.handle.hold() is True
    flat, got = src.reshape(n, -1), dst.reshape(n, -1)
    tw = Twin(W, H, mm355.Surface.tight(W, H, mm355.RGBA8))
    tw.h.set_params(proc._params())
    R0, R4 = tw.state_of(flat[0]), tw.state_of(flat[4])
    assert torch.equal(got[0], flat[0])
    _same(got[1:5], tw.run(R0, flat[1:5]), "against frame 0, the re-referencing frame too")
    _same(got[5:], tw.run(R4, flat[5:]), "against frame 4")
    assert torch.equal(_state(proc.handle), R4)
    proc.hold_reference = False
    proc.OnValidate()
    assert proc.handle.hold() is False
    tw.close()
    proc.OnDestroy()


# ---- 5. formats -----------------------------------------------------------------------
def test_convert_stream_with_hold():
    import mm355
    W, H, n = 200, 120, 7
    li, lo = mm355.Surface.tight(W, H, mm355.NV12), mm355.Surface.tight(W, H, mm355.RGBA8)
    src = torch.from_numpy(_clip(W, H, "nv12", n)).cuda()
    tw = Twin(W, H, li, lo)
    R = tw.state_of(src[0])
    want = tw.run(R, src)
    tw.close()
    h = mm355.Handle(W, H, _params())
    h.set_hold(True)
    h.set_batch(3)
    got = torch.zeros_like(want)
    h.process_stream_convert(src, li, got, lo, n)
    torch.cuda.synchronize()
    plain = mm355.Handle(W, H, _params())                # frame 0: the plain conversion, as for any first frame
    first = torch.zeros_like(want[0])
    plain.process_convert(src[0], li, first, lo)
    torch.cuda.synchronize()
    plain.close()
    assert torch.equal(got[0], first)
    _same(got[1:], want[1:], "NV12 -> RGBA8")
    assert torch.equal(_state(h), R), "the in frame's state"
    assert (got[3] != want[0]).float().mean() > 0.05
    h.close()


def test_pitched_nv12_surface_with_hold():
    import mm355
    W, H, n = 200, 120, 6
    clip = _clip(W, H, "nv12", 7)[:n]
    dec, tight = SF.lay_aligned("nv12", W, H), mm355.Surface.tight(W, H, mm355.NV12)
    src = torch.from_numpy(clip).cuda()
    tw = Twin(W, H, tight)
    R = tw.state_of(src[0])
    want = tw.run(R, src).cpu().numpy()
    tw.close()
    h = mm355.Handle(W, H, _params())
    h.set_hold(True)
    h.set_batch(4)
    size = SF.buffer_bytes("nv12", W, H, dec, n)
    a = torch.from_numpy(SF.scatter("nv12", W, H, list(clip), dec)).cuda()
    sent = SF.sentinel(size)
    b = torch.from_numpy(sent).cuda()
    h.process_stream_surfaces(a, dec, b, dec, n)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    keep = ~SF.sample_mask("nv12", W, H, dec, n, size)
    assert not (keep & (res != sent)).any(), "padding bytes written"
    got = SF.gather("nv12", W, H, res, dec, n)
    assert np.array_equal(got[0], clip[0])
    for k in range(1, n):
        assert np.array_equal(got[k], want[k]), k
    assert torch.equal(_state(h), R), "the state does not depend on a layout"
    h.close()


# ---- 6. lanes ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lane_clips(W, H, lanes, ticks):
    return np.stack([_clip(W, H, "rgba8", ticks, seed=0x5EED0000 + 977 * k) for k in range(lanes)], axis=1)


@pytest.mark.parametrize("variant", ["all", "mask", "reset", "in_place"])
def test_held_lanes_beside_a_rolling_lane(variant):
    """Hold mask 0b101: lane 1 is a rolling stream, lanes 0 and 2 hold their first frame."""
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 7
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    src = torch.from_numpy(_lane_clips(W, H, lanes, ticks)).cuda()      # [t][k]
    h = mm355.Handle(W, H, _params())
    h.set_lanes(lanes)
    h.set_lanes_hold(0b101)
    assert h.lanes_hold() == 0b101
    roll = mm355.Handle(W, H, _params())
    tw = Twin(W, H, lay)
    R = {0: None, 2: None}
    sentinel = torch.from_numpy(SF.sentinel(src[0].numel()).reshape(src[0].shape)).cuda()
    try:
        for t in range(ticks):
            mask = 0b011 if variant == "mask" and t % 2 else 0b111
            if variant == "reset" and t == 3:
                h.reset_lane(0)
                R[0] = None
            if variant == "in_place":
                out = src[t].clone()
                h.process_lanes_mask(mask, out, lay, out, lay)
            else:
                out = sentinel.clone()
                h.process_lanes_mask(mask, src[t], lay, out, lay)
            torch.cuda.synchronize()
            for k in range(lanes):
                if not (mask >> k) & 1:
                    assert torch.equal(out[k], sentinel[k]), ("a lane that sits out is not written", t, k)
                    continue
                if k == 1:
                    want = torch.zeros_like(src[t, k])
                    roll.process_surface(src[t, k], lay, want, lay)
                    torch.cuda.synchronize()
                elif R[k] is None:
                    want, R[k] = src[t, k], tw.state_of(src[t, k])       # passes through and is the reference
                else:
                    want = tw.run(R[k], src[t, k:k + 1])[0]
                assert torch.equal(out[k], want), (variant, "tick", t, "lane", k, int((out[k] != want).sum()))
            for k in (0, 2):
                assert torch.equal(_state(h, k), R[k]), ("the held lane's state stays", t, k)
            assert torch.equal(_state(h, 1), _state(roll)), ("the rolling lane's state follows", t)
        assert not torch.equal(out[0], src[ticks - 1, 0]), "the operator ran"
    finally:
        for x in (h, roll):
            x.close()
        tw.close()


def test_held_lanes_with_magnification_off():
    """apply_magnification = 0: every lane passes through; a held lane with state
    keeps it (nothing else happens), the rolling lane's state follows its input."""
    import mm355
    W, H, lanes = 200, 120, 3
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    src = torch.from_numpy(_lane_clips(W, H, lanes, 7)).cuda()
    h = mm355.Handle(W, H, _params())
    h.set_lanes(lanes)
    h.set_lanes_hold(0b101)
    tw = Twin(W, H, lay)
    out = torch.zeros_like(src[0])
    h.process_lanes(src[0], lay, out, lay)
    R = [tw.state_of(src[0, k]) for k in range(lanes)]
    h.set_params(_params(apply_magnification=False))
    for t in (1, 2):
        h.process_lanes(src[t], lay, out, lay)
        torch.cuda.synchronize()
        assert torch.equal(out, src[t])
        for k in (0, 2):
            assert torch.equal(_state(h, k), R[k]), (t, k)
        assert torch.equal(_state(h, 1), tw.state_of(src[t, 1])), t
    h.set_params(_params())
    h.process_lanes(src[3], lay, out, lay)
    torch.cuda.synchronize()
    for k in (0, 2):
        assert torch.equal(out[k], tw.run(R[k], src[3, k:k + 1])[0]), k
    assert torch.equal(out[1], tw.run(tw.state_of(src[2, 1]), src[3, 1:2])[0])
    h.close()
    tw.close()


def test_lanes_hold_mask_rules():
    import mm355
    h = mm355.Handle(200, 120, _params())
    assert _code(lambda: h.set_lanes_hold(1)) == INVALID, "no lanes: every bit is past the count"
    h.set_lanes(3)
    h.set_lanes_hold(0b110)
    assert _code(lambda: h.set_lanes_hold(0b1000)) == INVALID, "a bit at the lane count"
    assert h.lanes_hold() == 0b110, "a refusal leaves the mask"
    h.set_lanes(3)
    assert h.lanes_hold() == 0b110, "the same count keeps it"
    h.set_lanes(4)
    assert h.lanes_hold() == 0, "another count clears it"
    h.set_lanes_hold(0b1000)
    assert h.lanes_hold() == 0b1000
    assert mm355.lib().mm_get_lanes_hold(h.h, None) == INVALID
    h.close()


# ---- 7. refusals ------------------------------------------------------------------------
def test_refusals_leave_state_and_flags():
    import mm355
    W, H = 200, 120
    fmt = mm355.RGBA8
    lay, nv = mm355.Surface.tight(W, H, fmt), mm355.Surface.tight(W, H, mm355.NV12)
    src = torch.from_numpy(_clip(W, H, "rgba8", 26)[:4]).cuda()
    nsrc = torch.from_numpy(_clip(W, H, "nv12", 7)[:2]).cuda()
    tw = Twin(W, H, lay)
    R = tw.state_of(src[0])
    h = mm355.Handle(W, H, _params())
    lib = mm355.lib()
    assert lib.mm_set_hold(h.h, 2) == INVALID and lib.mm_set_hold(h.h, -1) == INVALID
    assert h.hold() is False
    assert lib.mm_get_hold(h.h, None) == INVALID
    h.set_hold(True)
    h.set_hold(False)
    assert h.hold() is False
    h.set_hold(True)
    assert lib.mm_set_hold(h.h, 2) == INVALID and h.hold() is True
    h.set_lanes(2)
    h.set_lanes_hold(0b11)
    h.process(src[0], torch.zeros_like(src[0]), fmt)
    torch.cuda.synchronize()
    assert torch.equal(_state(h), R)
    junk = torch.zeros(W * H * 4 * 2 + 64, dtype=torch.uint8, device="cuda")
    for pk in ({"mode": mm355.MODE_STEERABLE, "orientations": 4}, {"show_magnitude": 1}, {"show_phase": 1}):
        h.set_params(_params(**pk))                      # the flag may be set in any mode; the frame calls refuse
        assert h.hold() is True
        assert _code(lambda: h.process(src[1], junk, fmt)) == UNSUPPORTED, pk
        assert _code(lambda: h.process(src[1].cpu().numpy(), np.zeros(W * H * 4, np.uint8), fmt, on_device=False)) == UNSUPPORTED, pk
        assert _code(lambda: h.process_stream(src, junk, 2, fmt)) == UNSUPPORTED, pk
        assert _code(lambda: h.process_stream_surfaces(src, lay, junk, lay, 2)) == UNSUPPORTED, pk
        assert _code(lambda: h.process_convert(nsrc[0], nv, junk, lay)) == UNSUPPORTED, pk
        assert _code(lambda: h.process_stream_convert(nsrc, nv, junk, lay, 2)) == UNSUPPORTED, pk
        assert _code(lambda: h.process_lanes(src[:2], lay, junk, lay)) == UNSUPPORTED, pk
        torch.cuda.synchronize()
        assert not bool(junk.any()), "nothing was queued"
        assert h.hold() is True and h.lanes_hold() == 0b11
    h.set_params(_params())
    assert torch.equal(_state(h), R), "the state is as it was"
    got = torch.zeros_like(src[:2])
    h.process_stream(src[2:4], got, 2, fmt)
    torch.cuda.synchronize()
    _same(got, tw.run(R, src[2:4]), "a pyramid frame after set_params is right")
    # with hold off the same modes run as always
    h.set_hold(False)
    h.set_params(_params(show_magnitude=1))
    h.process(src[1], junk, fmt)
    torch.cuda.synchronize()
    h.close()
    tw.close()


# ---- 8. mm_cli --hold -------------------------------------------------------------------
@pytest.mark.parametrize("R,b", [(0, 4), (4, 3)], ids=["hold0", "hold4"])
def test_cli_hold(tmp_path, R, b):
    import mm355
    W, H, n = 64, 48, 10
    clip = _clip(W, H, "rgba8", n)
    src_path, dst_path = str(tmp_path / "in.rgba"), str(tmp_path / "out.rgba")
    clip.tofile(src_path)
    subprocess.check_call([CLI, "-w", str(W), "-h", str(H), "-n", str(n), "-l", str(L), "-s", str(S), "-b", str(b),
                           "-i", src_path, "-o", dst_path, "--hold", str(R)], timeout=120, stdout=subprocess.DEVNULL)
    got = np.fromfile(dst_path, np.uint8).reshape(n, -1)
    src = torch.from_numpy(clip).cuda()
    out = torch.zeros_like(src)
    h = mm355.Handle(W, H, _params())
    for k in range(n):                                   # frames R, 2 R, ... re-reference: one frame with hold off
        h.set_hold(not (R > 0 and k > 0 and k % R == 0))
        h.process(src[k], out[k], mm355.RGBA8)
    torch.cuda.synchronize()
    h.close()
    want = out.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    assert np.array_equal(got[0], clip[0]) and not np.array_equal(got[n - 1], clip[n - 1])
    # the two options give different clips from frame R + 1 on (not vacuous), and equal ones up to frame R
    if R:
        other = str(tmp_path / "other.rgba")
        subprocess.check_call([CLI, "-w", str(W), "-h", str(H), "-n", str(n), "-l", str(L), "-s", str(S),
                               "-i", src_path, "-o", other, "--hold", "0"], timeout=120, stdout=subprocess.DEVNULL)
        o = np.fromfile(other, np.uint8).reshape(n, -1)
        assert np.array_equal(o[:R + 1], got[:R + 1]) and not np.array_equal(o[R + 1], got[R + 1])


def test_cli_hold_with_lanes(tmp_path):
    """--hold with --lanes: every lane holds, R counts ticks; lane k's frames are a single --hold run's."""
    W, H, M, n = 64, 48, 2, 12
    clips = _lane_clips(W, H, M, n // M)                 # [t][k]: input frame t * M + k
    src_path, dst_path = str(tmp_path / "in.rgba"), str(tmp_path / "out.rgba")
    clips.tofile(src_path)
    base = [CLI, "-w", str(W), "-h", str(H), "-l", str(L), "-s", str(S), "--hold", "3"]
    subprocess.check_call(base + ["-n", str(n), "-i", src_path, "-o", dst_path, "--lanes", str(M)], timeout=120,
                          stdout=subprocess.DEVNULL)
    got = np.fromfile(dst_path, np.uint8).reshape(n // M, M, -1)
    for k in range(M):
        one, out = str(tmp_path / f"lane{k}.rgba"), str(tmp_path / f"out{k}.rgba")
        np.ascontiguousarray(clips[:, k]).tofile(one)
        subprocess.check_call(base + ["-n", str(n // M), "-i", one, "-o", out, "-b", "2"], timeout=120,
                              stdout=subprocess.DEVNULL)
        assert np.array_equal(got[:, k], np.fromfile(out, np.uint8).reshape(n // M, -1)), k
