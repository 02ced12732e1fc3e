"""Several live streams in one call: mm_set_lanes / mm_process_lanes and the
lane-state calls (include/mm.h "Several live streams in one call").

The contract is bitwise.  Lane k's outputs, and its state after every call, are
those of a handle of its own with the same parameters, fed lane k's frames
through one mm_process_surface / mm_process_convert call each: that reference
is what every test below compares against (M independent mm355.Handle objects),
byte for byte.  One test compares the lanes with the CPU oracle as well, so the
lanes are right and not merely equal to their twins.

The sizes are the smallest that reach each K2 configuration (k_cols_lanes runs
k_cols_body's instances per lane): N = 128 and 256 with several column groups
per workgroup, N = 1024 with the one-shot K34, N = 2048 with two columns per
workgroup and the LDS-DMA K34, N = 4096; the tabled one-band op (L = 5), the
two-band op (L = 6 at 0.05 / 0.45), the generic op (L = 7) and the standard
mode; both edge modes; odd sizes; 1, 2, 3, 5 and MM_LANES_MAX lanes."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before anything loads the library: torch brings the HIP runtime both share)

import convert as C
import mmtest as T
import mono
import nv12
import surface as SF
import yuv422

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")
L, S = 5, 25.0
OK, INVALID, UNSUPPORTED, NO_STATE = 0, -1, -2, -6


def _fmt(name):
    import mm355
    return {"rgba8": mm355.RGBA8, "rgba32f": mm355.RGBA32F, "nv12": mm355.NV12, "yuy2": mm355.YUY2,
            "y16": mm355.Y16, "nv12_709": mm355.NV12 | mm355.MATRIX_BT709}[name]


def _encode(name, rgba):
    """An RGBA8 picture as one tight frame of the format, as bytes."""
    if name == "rgba8":
        e = rgba
    elif name == "rgba32f":
        e = rgba.astype(np.float32) / np.float32(255)
    elif name.startswith("nv12"):
        e = nv12.encode(rgba)
    elif name == "yuy2":
        e = yuv422.encode(rgba)
    else:
        e = mono.encode(rgba[..., :3].astype(np.float64) / 255.0, 16)
    return np.ascontiguousarray(e).view(np.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def _clips(W, H, name, lanes, ticks):
    """uint8 [ticks][lanes][frame bytes]: lane k's frame t at [t][k], as a call
    takes them.  Every lane is a synthetic stream of its own (another seed and
    another start), made once per shape."""
    a = [T.synth(W, H, ticks, t0=3 * k, seed=0x5EED0000 + 977 * k, fmt="u8") for k in range(lanes)]
    out = np.stack([np.stack([_encode(name, a[k][t]) for k in range(lanes)]) for t in range(ticks)])
    if lanes > 1:
        assert (out[:, 0] != out[:, 1]).mean() > 0.2, "the lanes carry different streams"
    return out


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


def _single(h, fi, fo):
    """The one-frame call of the reference: a handle of its own, one call per frame."""
    return h.process_convert if fi != fo else h.process_surface


def _state(h, lane=None):
    import torch
    st = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    if lane is None:
        h.get_state(st)
    else:
        h.get_lane_state(lane, st)
    return st


class Rig:
    """One handle with `lanes` lanes next to `lanes` reference handles of their
    own; tick(t) runs frame t of every stream through both and asserts that
    they agree byte for byte."""

    def __init__(self, W, H, name, lanes, ticks, out_name=None, **pk):
        import torch
        import mm355
        self.W, self.H, self.lanes = W, H, lanes
        self.fi, self.fo = _fmt(name), _fmt(out_name or name)
        self.li, self.lo = mm355.Surface.tight(W, H, self.fi), mm355.Surface.tight(W, H, self.fo)
        self.fbo = mm355.frame_bytes(W, H, self.fo)
        self.src = torch.from_numpy(_clips(W, H, name, lanes, ticks)).cuda()
        self.hl = mm355.Handle(W, H, _params(**pk))
        self.hl.set_lanes(lanes)
        self.hs = [mm355.Handle(W, H, _params(**pk)) for _ in range(lanes)]

    def set_params(self, **pk):
        for h in [self.hl] + self.hs:
            h.set_params(_params(**pk))

    def tick(self, t, what=""):
        import torch
        a = torch.zeros((self.lanes, self.fbo), dtype=torch.uint8, device="cuda")
        b = torch.zeros_like(a)
        self.hl.process_lanes(self.src[t], self.li, a, self.lo)
        for k, h in enumerate(self.hs):
            _single(h, self.fi, self.fo)(self.src[t, k], self.li, b[k], self.lo)
        torch.cuda.synchronize()
        for k in range(self.lanes):
            assert torch.equal(a[k], b[k]), (what, "tick", t, "lane", k, int((a[k] != b[k]).sum()))
        return a

    def passes_through(self, t, out, lanes=None):
        """Which of the lanes' outputs of tick t are their input frames, bitwise."""
        import torch
        assert self.fi == self.fo
        return [bool(torch.equal(out[k], self.src[t, k])) for k in (range(self.lanes) if lanes is None else lanes)]

    def assert_states_equal(self, what=""):
        import torch
        for k, h in enumerate(self.hs):
            assert torch.equal(_state(self.hl, k), _state(h)), (what, "state of lane", k)

    def close(self):
        for h in [self.hl] + self.hs:
            h.close()


# ---- 1. every K2 configuration, bitwise --------------------------------------------
# W, H, format, lanes, ticks, parameters
CASES = [
    (200, 120, "rgba8", 3, 4, {}),                     # N = 256, several groups per workgroup
    (98, 62, "nv12", 2, 3, {"edge_mode": 1}),          # N = 128, clamp; rows at 2 mod 4: unfused compose
    (97, 63, "rgba32f", 2, 3, {"standard": True}),     # standard mode, odd size
    (640, 360, "yuy2", 5, 3, {}),                      # N = 1024, the one-shot K34
    (1920, 1080, "rgba8", 3, 3, {}),                   # N = 2048, two columns per workgroup, LDS-DMA K34
    (2100, 64, "y16", 2, 3, {}),                       # N = 4096
    (200, 120, "rgba8", 2, 3, {"levels": 6}),          # 0.05 / 0.45: the two-band op (MM_K2_PYR_TAB2)
    (200, 120, "rgba8", 2, 3, {"levels": 7}),          # ... the generic op
    (200, 120, "rgba8", 64, 2, {}),                    # the lane cap
]


@pytest.mark.parametrize("W,H,name,lanes,ticks,pk", CASES,
                         ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}lanes" + "".join(f"-{k}{v}" for k, v in c[5].items())
                              for c in CASES])
def test_lanes_equal_handles_of_their_own_bitwise(W, H, name, lanes, ticks, pk):
    import torch
    import mm355
    clips = _clips(W, H, name, lanes, ticks)
    fmt = _fmt(name)
    lay = mm355.Surface.tight(W, H, fmt)
    src = torch.from_numpy(clips).cuda()
    got = torch.zeros_like(src)
    hl = mm355.Handle(W, H, _params(**pk))
    hl.set_lanes(lanes)
    assert hl.lanes() == lanes
    for t in range(ticks):
        hl.process_lanes(src[t], lay, got[t], lay)
    states = [_state(hl, k) for k in range(lanes)]
    torch.cuda.synchronize()
    hl.close()
    # the references one at a time: a handle of its own per lane, one call per frame
    want = torch.zeros((ticks, clips.shape[2]), dtype=torch.uint8, device="cuda")
    for k in range(lanes):
        h = mm355.Handle(W, H, _params(**pk))
        for t in range(ticks):
            h.process_surface(src[t, k], lay, want[t], lay)
        st = _state(h)
        torch.cuda.synchronize()
        h.close()
        for t in range(ticks):
            assert torch.equal(got[t, k], want[t]), ("lane", k, "tick", t, int((got[t, k] != want[t]).sum()))
        assert torch.equal(states[k], st), ("state of lane", k)
        assert torch.equal(got[0, k], src[0, k]), "a lane's first frame passes through"
        assert (got[1, k] != src[1, k]).float().mean() > 0.05, "the operator ran"


def test_one_lane_equals_mm_process():
    import torch
    import mm355
    W, H, ticks = 200, 120, 4
    src = torch.from_numpy(_clips(W, H, "rgba8", 1, ticks)).cuda()
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    hl, h = mm355.Handle(W, H, _params()), mm355.Handle(W, H, _params())
    hl.set_lanes(1)
    a, b = torch.zeros_like(src), torch.zeros_like(src)
    for t in range(ticks):
        hl.process_lanes(src[t], lay, a[t], lay)
        h.process(src[t, 0], b[t, 0], mm355.RGBA8)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(_state(hl, 0), _state(h))
    assert not torch.equal(a[1], src[1])
    hl.close()
    h.close()


# ---- 2. the lanes against the CPU oracle -------------------------------------------
def test_lanes_vs_oracle():
    import torch
    import mm355
    W, H, lanes, ticks = 128, 96, 3, 4
    clips = [T.synth(W, H, ticks, t0=5 * k, seed=0x5EED0000 + 31 * k, fmt="u8") for k in range(lanes)]
    refs = [T.oracle_run(W, H, clips[k], L, S) for k in range(lanes)]
    src = torch.from_numpy(np.stack([np.stack([clips[k][t] for k in range(lanes)]) for t in range(ticks)])).cuda()
    got = torch.zeros_like(src)
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    hl = mm355.Handle(W, H, _params())
    hl.set_lanes(lanes)
    for t in range(ticks):
        hl.process_lanes(src[t], lay, got[t], lay)
    torch.cuda.synchronize()
    hl.close()
    out = got.cpu().numpy()
    for k in range(lanes):
        assert np.array_equal(out[0, k], clips[k][0])
        for t in range(1, ticks):
            d = np.abs(out[t, k].astype(np.int32) - refs[k][t].astype(np.int32))
            print(f"lane {k} tick {t}: max {d.max()}  share {(d > 0).mean():.2e}")
            T.assert_close_u8(out[t, k], refs[k][t])
    assert not np.array_equal(out[1, 0], out[1, 1])


# ---- 3. reset_lane -----------------------------------------------------------------
def test_reset_lane_mid_stream():
    r = Rig(200, 120, "rgba8", 3, 7)
    try:
        r.tick(0)
        r.tick(1)
        r.hl.reset_lane(1)
        r.hs[1].reset()
        assert r.passes_through(2, r.tick(2, "lane 1 reset")) == [False, True, False]
        assert r.passes_through(3, r.tick(3, "lane 1 restarted")) == [False, False, False]
        r.assert_states_equal("after the restart")
        r.hl.reset_lane()                       # -1: every lane
        for h in r.hs:
            h.reset()
        assert r.passes_through(4, r.tick(4, "all reset")) == [True, True, True]
        assert r.passes_through(5, r.tick(5)) == [False, False, False]
        r.hl.reset_lane(-1)
        assert _code(lambda: _state(r.hl, 0)) == NO_STATE
        for h in r.hs:
            h.reset()
        assert r.passes_through(6, r.tick(6)) == [True, True, True]
        r.assert_states_equal("at the end")
    finally:
        r.close()


# ---- 4. a stream moves between a handle and a lane ----------------------------------
def test_state_hand_over():
    import torch
    import mm355
    W, H, ticks = 200, 120, 6
    src = torch.from_numpy(_clips(W, H, "rgba8", 2, ticks)).cuda()     # [t][0]: the stream; [t][1]: another
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    ref = mm355.Handle(W, H, _params())                  # the stream on one handle, start to end
    want = torch.zeros((ticks,) + tuple(src.shape[2:]), dtype=torch.uint8, device="cuda")
    for t in range(ticks):
        ref.process_surface(src[t, 0], lay, want[t], lay)
    # handle -> lane 1
    a = mm355.Handle(W, H, _params())
    out = torch.zeros_like(src[0])
    for t in range(2):
        a.process_surface(src[t, 0], lay, out[0], lay)
    hl = mm355.Handle(W, H, _params())
    hl.set_lanes(2)
    hl.set_lane_state(1, _state(a))
    pair = torch.stack([src[2, 1], src[2, 0]])           # lane 0: a stream that starts; lane 1: the stream goes on
    hl.process_lanes(pair, lay, out, lay)
    torch.cuda.synchronize()
    assert torch.equal(out[1], want[2]), "handle -> lane"
    assert torch.equal(out[0], src[2, 1]), "the lane without state passes through"
    # lane 1 -> lane 0: both lanes now continue the one stream
    hl.set_lane_state(0, _state(hl, 1))
    pair = torch.stack([src[3, 0], src[3, 0]])
    hl.process_lanes(pair, lay, out, lay)
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[3]) and torch.equal(out[1], want[3]), "lane -> lane"
    # lane 0 -> another handle
    b = mm355.Handle(W, H, _params())
    b.set_state(_state(hl, 0))
    b.process_surface(src[4, 0], lay, out[0], lay)
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[4]), "lane -> handle"
    assert not torch.equal(want[4], src[4, 0])
    for h in (ref, a, hl, b):
        h.close()


# ---- 5. apply_magnification = 0 -----------------------------------------------------
def test_apply_magnification_off_and_on_again():
    r = Rig(200, 120, "rgba8", 3, 6)
    try:
        r.tick(0)
        r.tick(1)
        r.set_params(apply_magnification=False)
        for t in (2, 3):
            assert r.passes_through(t, r.tick(t, "off")) == [True, True, True]
            r.assert_states_equal("the states follow the inputs")
        r.set_params()
        for t in (4, 5):
            assert r.passes_through(t, r.tick(t, "on again")) == [False, False, False]
        r.assert_states_equal()
    finally:
        r.close()


def test_apply_magnification_off_from_the_start():
    r = Rig(98, 62, "nv12", 2, 3, apply_magnification=False)
    try:
        assert r.passes_through(0, r.tick(0)) == [True, True]
        r.assert_states_equal("K1 over all lanes")
        r.set_params()
        assert r.passes_through(1, r.tick(1)) == [False, False]
        r.tick(2)
    finally:
        r.close()


# ---- 6. set_params between ticks ----------------------------------------------------
def test_set_params_between_ticks():
    r = Rig(200, 120, "rgba8", 3, 9)
    try:
        r.tick(0)
        r.tick(1)
        r.set_params(phase_scale=10.0)
        a = r.tick(2, "phase_scale 10")
        r.set_params(phase_scale=10.0, edge_mode=1)
        r.tick(3, "edge_mode: old-edge state, new-edge frame")
        r.tick(4, "edge_mode: both new")
        r.set_params(phase_scale=10.0, edge_mode=1, levels=6)     # another K2 table and op
        r.tick(5, "levels 6")
        r.tick(6, "levels 6")
        r.set_params()
        r.tick(7, "back")
        r.assert_states_equal()
        # the new phase scale took effect: tick 2 differs from a rig that kept S
        q = Rig(200, 120, "rgba8", 3, 9)
        try:
            for t in range(3):
                b = q.tick(t)
            assert not bool((a == b).all())
        finally:
            q.close()
    finally:
        r.close()


# ---- 7. pitched surfaces -------------------------------------------------------------
def _stride_plus(lay, W, H, more):
    import mm355
    s = mm355.Surface(format=lay.format, pitch=lay.pitch, chroma_offset=lay.chroma_offset,
                      chroma_pitch=lay.chroma_pitch, frame_stride=lay.frame_stride)
    s.frame_stride = max(lay.frame_stride, lay.bytes(W, H)) + more
    return s


@pytest.mark.parametrize("which", ["decoder_in_tight_out", "strides_past_the_extent"])
def test_pitched_surfaces(which):
    import torch
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 3
    clips = _clips(W, H, "nv12", lanes, ticks)
    dec, tight = mm355.Surface.aligned(W, H, mm355.NV12, 256, 16), mm355.Surface.tight(W, H, mm355.NV12)
    if which == "decoder_in_tight_out":
        lin, lout = dec, tight
    else:
        lin, lout = _stride_plus(dec, W, H, 512), _stride_plus(tight, W, H, 66)   # (66: frames at 2 mod 4)
    r = Rig(W, H, "nv12", lanes, ticks)
    hp = mm355.Handle(W, H, _params())                   # the pitched calls, in step with the rig's tight ones
    hp.set_lanes(lanes)
    try:
        size = SF.buffer_bytes("nv12", W, H, lout, lanes)
        keep = ~SF.sample_mask("nv12", W, H, lout, lanes, size)
        assert keep.sum() >= SF.TAIL
        for t in range(ticks):
            if t == 2:                                   # a lane without state among lanes that have it
                r.hl.reset_lane(1)
                r.hs[1].reset()
                hp.reset_lane(1)
            want = r.tick(t).cpu().numpy()               # tight lanes == reference handles
            a = torch.from_numpy(SF.scatter("nv12", W, H, list(clips[t]), lin)).cuda()
            sent = SF.sentinel(size)
            b = torch.from_numpy(sent).cuda()
            hp.process_lanes(a, lin, b, lout)
            torch.cuda.synchronize()
            res = b.cpu().numpy()
            bad = np.flatnonzero(keep & (res != sent))
            assert bad.size == 0, f"tick {t}: {bad.size} padding bytes written, first at {bad[:8]}"
            got = SF.gather("nv12", W, H, res, lout, lanes)
            for k in range(lanes):
                assert np.array_equal(got[k], want[k]), (t, k)
                if t == 0 or (t == 2 and k == 1):
                    assert np.array_equal(got[k], clips[t, k]), "a lane without state passes through"
        for k in range(lanes):
            assert torch.equal(_state(hp, k), _state(r.hl, k)), "the state does not depend on a layout"
    finally:
        hp.close()
        r.close()


# ---- 8. a convert pair ---------------------------------------------------------------
def test_convert_pair_in_lanes():
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 4
    r = Rig(W, H, "nv12_709", lanes, ticks, out_name="rgba8")
    try:
        clips = _clips(W, H, "nv12_709", lanes, ticks)
        out = r.tick(0, "the plain conversion").cpu().numpy()
        for k in range(lanes):
            plain = C.plain(clips[0, k].reshape(H * 3 // 2, W), r.fi, mm355.RGBA8)
            T.assert_close_u8(out[k].reshape(H, W, 4), plain)
        for t in range(1, ticks):
            o = r.tick(t).cpu().numpy()
            plain = C.plain(clips[t, 0].reshape(H * 3 // 2, W), r.fi, mm355.RGBA8)
            assert (o[0].reshape(H, W, 4)[..., :3] != plain[..., :3]).mean() > 0.05, "the operator ran"
        r.assert_states_equal("the in frame's state")
    finally:
        r.close()


# ---- 9. single-stream calls between lane calls ----------------------------------------
def test_interleaving_with_the_handles_own_stream():
    import torch
    import mm355
    W, H, ticks = 200, 120, 6
    r = Rig(W, H, "rgba8", 2, ticks)
    own = torch.from_numpy(_clips(W, H, "rgba8", 3, ticks)).cuda()[:, 2]      # a third stream
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    twin = mm355.Handle(W, H, _params())
    a, b = torch.zeros_like(own[0]), torch.zeros_like(own[0])
    try:
        for t in range(ticks):
            r.hl.process(own[t], a, mm355.RGBA8)          # the lanes' handle runs a stream of its own too
            twin.process(own[t], b, mm355.RGBA8)
            r.tick(t, "between single calls")
            torch.cuda.synchronize()
            assert torch.equal(a, b), ("the handle's own stream", t)
            if t == 2:
                r.hl.set_batch(3)                         # keeps the lanes, their states and the single state
            if t == 3:
                r.hl.reset()                              # the single stream's reset leaves the lanes alone
                twin.reset()
        assert not torch.equal(a, own[ticks - 1])
        assert torch.equal(_state(r.hl), _state(twin))
        r.assert_states_equal()
    finally:
        twin.close()
        r.close()


# ---- 10. another lane count -----------------------------------------------------------
def test_set_lanes_again():
    import torch
    import mm355
    W, H, ticks = 200, 120, 5
    src = torch.from_numpy(_clips(W, H, "rgba8", 5, ticks)).cuda()
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    h = mm355.Handle(W, H, _params())
    out = torch.zeros_like(src[0])
    h.set_lanes(3)
    for t in range(2):
        h.process_lanes(src[t, :3], lay, out[:3], lay)
    torch.cuda.synchronize()
    assert not torch.equal(out[:3], src[1, :3])
    h.set_lanes(5)                                        # another count: every state dropped
    assert h.lanes() == 5
    assert _code(lambda: _state(h, 0)) == NO_STATE
    h.process_lanes(src[2], lay, out, lay)
    torch.cuda.synchronize()
    assert torch.equal(out, src[2]), "the next frames pass through"
    st = [_state(h, k) for k in range(5)]
    h.set_lanes(5)                                        # the same count: nothing happens
    for k in range(5):
        assert torch.equal(_state(h, k), st[k])
    h.process_lanes(src[3], lay, out, lay)
    torch.cuda.synchronize()
    for k in range(5):
        assert not torch.equal(out[k], src[3, k]), k
    h.set_lanes(0)
    assert h.lanes() == 0
    assert _code(lambda: h.process_lanes(src[4], lay, out, lay)) == INVALID
    assert _code(lambda: _state(h, 0)) == INVALID
    h.set_lanes(2)                                        # ... and lanes again afterwards
    h.process_lanes(src[4, :2], lay, out[:2], lay)
    torch.cuda.synchronize()
    assert torch.equal(out[:2], src[4, :2])
    h.close()


# ---- 11. refusals ---------------------------------------------------------------------
def test_refusals_leave_the_lanes_as_they_were():
    import torch
    import mm355
    W, H, lanes = 200, 120, 3
    r = Rig(W, H, "rgba8", lanes, 4)
    lib = mm355.lib()
    try:
        r.tick(0)
        r.tick(1)
        before = [_state(r.hl, k) for k in range(lanes)]
        h, lay, src = r.hl, r.li, r.src
        junk = torch.zeros(W * H * 16 * lanes + 64, dtype=torch.uint8, device="cuda")
        st = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")

        def unchanged(what):
            assert h.lanes() == lanes, what
            for k in range(lanes):
                assert torch.equal(_state(h, k), before[k]), (what, k)

        # the modes lanes do not take: the call and the two lane-state calls
        for pk in ({"mode": mm355.MODE_STEERABLE, "orientations": 4}, {"show_magnitude": 1}, {"show_phase": 1}):
            h.set_params(_params(**pk))
            assert _code(lambda: h.process_lanes(src[2], lay, junk, lay)) == UNSUPPORTED, pk
            assert lib.mm_get_lane_state(h.h, 0, st.data_ptr(), st.numel(), None) == UNSUPPORTED, pk
            assert lib.mm_set_lane_state(h.h, 0, st.data_ptr(), st.numel(), None) == UNSUPPORTED, pk
            h.set_params(_params())
            unchanged(pk)
        # null pointers
        null = ctypes.POINTER(mm355.Surface)()
        assert lib.mm_process_lanes(h.h, None, ctypes.byref(lay), junk.data_ptr(), ctypes.byref(lay), None) == INVALID
        assert lib.mm_process_lanes(h.h, src[2].data_ptr(), ctypes.byref(lay), None, ctypes.byref(lay), None) == INVALID
        assert lib.mm_process_lanes(h.h, src[2].data_ptr(), null, junk.data_ptr(), ctypes.byref(lay), None) == INVALID
        assert lib.mm_process_lanes(h.h, src[2].data_ptr(), ctypes.byref(lay), junk.data_ptr(), null, None) == INVALID
        assert lib.mm_get_lane_state(h.h, 0, None, st.numel(), None) == INVALID
        assert lib.mm_set_lane_state(h.h, 0, None, st.numel(), None) == INVALID
        assert lib.mm_get_lanes(h.h, None) == INVALID
        unchanged("null pointers")
        # a lane index out of range; a lane count out of range
        for lane in (-1, lanes, 64):
            assert lib.mm_get_lane_state(h.h, lane, st.data_ptr(), st.numel(), None) == INVALID, lane
            assert lib.mm_set_lane_state(h.h, lane, st.data_ptr(), st.numel(), None) == INVALID, lane
        for lane in (-2, lanes, 64):
            assert _code(lambda: h.reset_lane(lane)) == INVALID, lane
        for n in (-1, mm355.LANES_MAX + 1):
            assert _code(lambda: h.set_lanes(n)) == INVALID, n
        unchanged("a lane index or count out of range")
        # too few bytes
        assert lib.mm_get_lane_state(h.h, 0, st.data_ptr(), st.numel() - 8, None) == INVALID
        assert lib.mm_set_lane_state(h.h, 0, st.data_ptr(), st.numel() - 8, None) == INVALID
        unchanged("too few bytes")
        # two formats that are no pair; an unknown code; layouts by the stream entry points' rules
        assert _code(lambda: h.process_lanes(src[2], lay, junk, mm355.Surface.tight(W, H, mm355.RGBA32F))) == INVALID
        assert _code(lambda: h.process_lanes(junk, mm355.Surface.tight(W, H, mm355.NV12), junk,
                                             mm355.Surface.tight(W, H, mm355.P010))) == INVALID
        bad = mm355.Surface.tight(W, H, mm355.RGBA8)
        bad.format = 20
        assert _code(lambda: h.process_lanes(src[2], bad, junk, bad)) == INVALID
        short = mm355.Surface.tight(W, H, mm355.RGBA8)
        short.frame_stride -= 4                               # count = lanes: frames may not overlap
        assert _code(lambda: h.process_lanes(src[2], short, junk, lay)) == INVALID
        assert _code(lambda: h.process_lanes(src[2], lay, junk[2:], lay)) == INVALID       # RGBA8: unit 4
        unchanged("formats and layouts")
        assert r.passes_through(2, r.tick(2, "after the refusals")) == [False] * lanes
        r.assert_states_equal()
        # no lanes set; N = 8192; odd sizes of a Y'CbCr format
        assert _code(lambda: r.hs[0].process_lanes(src[3], lay, junk, lay)) == INVALID
        assert _code(lambda: r.hs[0].reset_lane(0)) == INVALID
        r.hs[0].reset_lane(-1)                                # (every lane of none)
        big = mm355.Handle(4100, 16, _params())
        assert big.N == 8192 and _code(lambda: big.set_lanes(2)) == UNSUPPORTED and big.lanes() == 0
        big.close()
        odd = mm355.Handle(97, 63, _params())
        odd.set_lanes(2)
        nv = mm355.Surface.tight(98, 64, mm355.NV12)           # (no NV12 layout exists for an odd size)
        assert _code(lambda: odd.process_lanes(junk, nv, junk, nv)) == UNSUPPORTED
        assert _code(lambda: odd.process_lanes(junk, nv, junk, mm355.Surface.tight(97, 63, mm355.RGBA8))) == UNSUPPORTED
        odd.close()
        r.tick(3, "at the end")
    finally:
        r.close()


# ---- 12. mm_cli --lanes ---------------------------------------------------------------
def _write_y4m(path, W, H, fr):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420\n".encode())
        for b in fr:
            b = b.reshape(H * 3 // 2, W)
            c = b[H:].reshape(H // 2, W // 2, 2)
            f.write(b"FRAME\n" + b[:H].tobytes() + np.ascontiguousarray(c[..., 0]).tobytes() +
                    np.ascontiguousarray(c[..., 1]).tobytes())


def _y4m_frames(path, n):
    """The n frame records of a .y4m file (all of one size), headers included."""
    body = open(path, "rb").read().split(b"\n", 1)[1]
    assert len(body) % n == 0 and body.startswith(b"FRAME\n")
    step = len(body) // n
    return [body[k * step:(k + 1) * step] for k in range(n)]


@pytest.mark.parametrize("opt", [["--nv12"], []], ids=["nv12", "default"])
def test_cli_lanes(tmp_path, opt):
    W, H, M, n = 64, 48, 3, 9
    clips = _clips(W, H, "nv12", M, n // M + 1)             # [t][k]: input frame t * M + k
    inter = [clips[j // M, j % M] for j in range(n + 1)]
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    _write_y4m(src, W, H, inter[:n])
    base = opt + ["-l", str(L), "-s", str(S)]
    subprocess.check_call([CLI] + base + ["-i", src, "-o", dst, "--lanes", str(M)], timeout=120,
                          stdout=subprocess.DEVNULL)
    got = _y4m_frames(dst, n)
    for k in range(M):
        one, out = str(tmp_path / f"lane{k}.y4m"), str(tmp_path / f"out{k}.y4m")
        _write_y4m(one, W, H, inter[k:n:M])
        subprocess.check_call([CLI] + base + ["-i", one, "-o", out, "-b", "1"], timeout=120,
                              stdout=subprocess.DEVNULL)
        want = _y4m_frames(out, n // M)
        for t in range(n // M):
            assert got[t * M + k] == want[t], (k, t)
    assert got[M] != got[0] and len(set(got)) == n
    # a clip that is no whole number of ticks: a usage error naming both numbers, no output file
    ten, none = str(tmp_path / "ten.y4m"), str(tmp_path / "none.y4m")
    _write_y4m(ten, W, H, inter)
    rr = subprocess.run([CLI] + base + ["-i", ten, "-o", none, "--lanes", str(M)], capture_output=True, timeout=120)
    assert rr.returncode == 2 and b"3" in rr.stderr and b"10" in rr.stderr, rr.stderr
    assert not os.path.exists(none)
