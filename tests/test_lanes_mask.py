"""A subset of the lanes per call: mm_process_lanes_mask / mm_lanes_with_state
(include/mm.h "Several live streams in one call").

The contract is bitwise, per lane, over the frames of the calls that selected
the lane: lane k's outputs, and its state after every call, are those of a
handle of its own with the same parameters, fed exactly those frames through one
mm_process_surface / mm_process_convert call each.  That reference (MaskRig: M
independent mm355.Handle objects, each fed only when its lane is selected) is
what every test below compares against.  Every tick compares three things: the
selected lanes' outputs byte for byte, the unselected lanes' output slots
against their 0xA5 prefill, and every lane's state (MM_ERR_NO_STATE where the
reference has seen no frame) with mm_lanes_with_state.

The masks make lanes sit out one call and two (a lane's bank bit ends up either
way), put lanes with different bank bits in one call, leave holes, and select a
lane for the first time beside lanes that are composed.  The shapes are those of
test_lanes.py's CASES (every K2 configuration k_cols_lanes has)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before anything loads the library: torch brings the HIP runtime both share)

import convert as C
import mmtest as T
import surface as SF
from test_lanes import (CLI, INVALID, L, NO_STATE, S, UNSUPPORTED, _clips, _code, _fmt, _params, _single, _state,
                        _write_y4m, _y4m_frames)

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _bits(mask, lanes):
    return [k for k in range(lanes) if (mask >> k) & 1]


class MaskRig:
    """One handle with `lanes` lanes next to `lanes` reference handles of their
    own.  tick(t, mask) runs frame t of the selected streams through both, each
    reference seeing only the frames of its lane's calls, and asserts outputs,
    untouched slots, states and mm_lanes_with_state."""

    def __init__(self, W, H, name, lanes, ticks, out_name=None, **pk):
        import mm355
        self.W, self.H, self.lanes = W, H, lanes
        self.fi, self.fo = _fmt(name), _fmt(out_name or name)
        self.li, self.lo = mm355.Surface.tight(W, H, self.fi), mm355.Surface.tight(W, H, self.fo)
        self.fbo = mm355.frame_bytes(W, H, self.fo)
        self.src = torch.from_numpy(_clips(W, H, name, lanes, ticks)).cuda()
        self.hl = mm355.Handle(W, H, _params(**pk))
        self.hl.set_lanes(lanes)
        self.hs = [mm355.Handle(W, H, _params(**pk)) for _ in range(lanes)]
        self.has = [False] * lanes          # the reference of lane k has state
        self.seen = [0] * lanes             # frames lane k was selected for
        self.second = {}                    # lane -> (its second selected frame's output, that input)

    def set_params(self, **pk):
        for h in [self.hl] + self.hs:
            h.set_params(_params(**pk))

    def reset_lane(self, k):
        self.hl.reset_lane(k)
        self.hs[k].reset()
        self.has[k] = False

    def call(self, mask, src, dst):
        self.hl.process_lanes_mask(mask, src, self.li, dst, self.lo)

    def tick(self, t, mask, what="", in_place=False, call=None):
        """-> the lanes' output slots.  in_place: the call's in and out are one
        buffer, whose unselected slots must keep their frames."""
        if in_place:
            assert self.fi == self.fo
            a = self.src[t].clone()
            pre = a.clone()
            src = a
        else:
            a = torch.full((self.lanes, self.fbo), FILL, dtype=torch.uint8, device="cuda")
            pre = a.clone()
            src = self.src[t]
        b = torch.zeros((self.lanes, self.fbo), dtype=torch.uint8, device="cuda")
        (call or self.call)(mask, src, a)
        for k in _bits(mask, self.lanes):
            _single(self.hs[k], self.fi, self.fo)(self.src[t, k], self.li, b[k], self.lo)
            self.has[k] = True
            self.seen[k] += 1
        torch.cuda.synchronize()
        for k in range(self.lanes):
            if (mask >> k) & 1:
                assert torch.equal(a[k], b[k]), (what, "tick", t, "lane", k, int((a[k] != b[k]).sum()))
                if self.seen[k] == 2 and self.fi == self.fo:
                    self.second[k] = float((a[k] != self.src[t, k]).float().mean())
            else:
                assert torch.equal(a[k], pre[k]), (what, "tick", t, "unselected lane", k, "was written")
        self.assert_states(f"{what} tick {t}")
        return a

    def assert_states(self, what=""):
        for k, h in enumerate(self.hs):
            if self.has[k]:
                assert torch.equal(_state(self.hl, k), _state(h)), (what, "state of lane", k)
            else:
                assert _code(lambda: _state(self.hl, k)) == NO_STATE, (what, "lane", k)
        assert self.hl.lanes_with_state() == sum(1 << k for k in range(self.lanes) if self.has[k]), what

    def passes_through(self, t, out, lanes):
        assert self.fi == self.fo
        return [bool(torch.equal(out[k], self.src[t, k])) for k in lanes]

    def close(self):
        for h in [self.hl] + self.hs:
            h.close()


# ---- 1. the schedule ---------------------------------------------------------------
SCHEDULE = [0b01111, 0b01011, 0b01111, 0b10100, 0b00110, 0b11001, 0b00000, 0b11111, 0b10101, 0b11111]


def test_schedule_of_masks():
    r = MaskRig(200, 120, "rgba8", 5, len(SCHEDULE))
    try:
        for t, mask in enumerate(SCHEDULE):
            out = r.tick(t, mask, "schedule")
            if t == 3:       # lane 4's first frame passes through beside lane 2, which is composed
                assert r.passes_through(3, out, [2, 4]) == [False, True]
        assert sorted(r.second) == [0, 1, 2, 3, 4]
        for k, share in r.second.items():
            assert share > 0.05, ("the operator ran on lane", k, share)
    finally:
        r.close()


# ---- 2. every K2 configuration -----------------------------------------------------
M3 = [0b111, 0b101, 0b111, 0b010]           # lane 1 skips a call (a hole), then banks differ, then it runs alone
ALT = 0x5555555555555555
# W, H, format, lanes, masks, parameters
CASES = [
    (98, 62, "nv12", 3, M3, {"edge_mode": 1}),                         # N = 128, clamp, unfused compose
    (97, 63, "rgba32f", 3, M3, {"standard": True}),                    # standard mode, odd size
    (640, 360, "yuy2", 5, [0b11111, 0b10101, 0b11011], {}),            # N = 1024, the one-shot K34
    (1920, 1080, "rgba8", 3, M3[:3], {}),                              # N = 2048, LDS-DMA K34
    (2100, 64, "y16", 3, M3, {}),                                      # N = 4096
    (200, 120, "rgba8", 3, M3, {"levels": 6}),                         # the two-band op (MM_K2_PYR_TAB2)
    (200, 120, "rgba8", 3, M3, {"levels": 7}),                         # the generic op
    # the lane cap; then lanes of both words sit out, so that the bank bits differ above lane 31 too
    (200, 120, "rgba8", 64, [ALT, ~ALT & (2 ** 64 - 1), 2 ** 64 - 1, 0xFFFF0000FFFF0000, 2 ** 64 - 1, 0x00FFFF0000FFFF00], {}),
]


@pytest.mark.parametrize("W,H,name,lanes,masks,pk", CASES,
                         ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}lanes" + "".join(f"-{k}{v}" for k, v in c[5].items())
                              for c in CASES])
def test_masks_over_k2_configurations(W, H, name, lanes, masks, pk):
    r = MaskRig(W, H, name, lanes, len(masks), **pk)
    try:
        for t, mask in enumerate(masks):
            r.tick(t, mask)
        assert r.second and all(v > 0.05 for v in r.second.values()), r.second
    finally:
        r.close()


# ---- 3. the all-lanes mask is mm_process_lanes ---------------------------------------
def test_full_mask_is_process_lanes():
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 5
    src = torch.from_numpy(_clips(W, H, "rgba8", lanes, ticks)).cuda()
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    ha, hb, hc = (mm355.Handle(W, H, _params()) for _ in range(3))
    for h in (ha, hb, hc):
        h.set_lanes(lanes)
    a, b, c = (torch.zeros_like(src[0]) for _ in range(3))
    full = (1 << lanes) - 1
    try:
        for t in range(ticks):
            ha.process_lanes(src[t], lay, a, lay)
            hb.process_lanes_mask(full, src[t], lay, b, lay)
            if t % 2:                                     # the two calls alternate on one handle
                hc.process_lanes(src[t], lay, c, lay)
            else:
                hc.process_lanes_mask(full, src[t], lay, c, lay)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(a, c), t
            assert torch.equal(a, src[t]) == (t == 0)
            for k in range(lanes):
                assert torch.equal(_state(ha, k), _state(hb, k)) and torch.equal(_state(ha, k), _state(hc, k)), (t, k)
            assert ha.lanes_with_state() == hb.lanes_with_state() == hc.lanes_with_state() == full
    finally:
        for h in (ha, hb, hc):
            h.close()


def test_process_lanes_between_mask_calls():
    """mm_process_lanes on a handle whose lanes have different bank bits."""
    r = MaskRig(200, 120, "rgba8", 4, 5)
    full = lambda mask, src, dst: r.hl.process_lanes(src, r.li, dst, r.lo)
    try:
        r.tick(0, 0b1111, call=full)
        r.tick(1, 0b0101)
        r.tick(2, 0b1111, "mixed banks", call=full)
        r.tick(3, 0b1010)
        r.tick(4, 0b1111, "mixed banks again", call=full)
    finally:
        r.close()


def test_the_handles_own_stream_between_mask_calls():
    import mm355
    W, H, ticks = 200, 120, 5
    r = MaskRig(W, H, "rgba8", 2, ticks)
    own = torch.from_numpy(_clips(W, H, "rgba8", 3, ticks)).cuda()[:, 2]      # a third stream
    twin = mm355.Handle(W, H, _params())
    a, b = torch.zeros_like(own[0]), torch.zeros_like(own[0])
    try:
        for t, mask in enumerate([0b11, 0b01, 0b10, 0b00, 0b11]):
            r.hl.process(own[t], a, mm355.RGBA8)          # the lanes' handle runs a stream of its own too
            twin.process(own[t], b, mm355.RGBA8)
            r.tick(t, mask, "between single calls")
            assert torch.equal(a, b), ("the handle's own stream", t)
        assert not torch.equal(a, own[ticks - 1])
        assert torch.equal(_state(r.hl), _state(twin))
    finally:
        twin.close()
        r.close()


# ---- 4. in place ---------------------------------------------------------------------
@pytest.mark.parametrize("W,H,name", [(200, 120, "rgba8"), (640, 360, "yuy2"), (98, 62, "nv12")])
def test_in_place_with_and_without_state(W, H, name):
    """in == out.  The compose reads source rows beside the ones it writes (its
    chroma taps), other workgroups' rows among them, so a composed lane's frame
    must not be read where it is being written: equal to the reference, which
    runs with buffers of its own, every time."""
    r = MaskRig(W, H, name, 3, 4)
    try:
        r.tick(0, 0b011, in_place=True)
        out = r.tick(1, 0b111, "lane 2 starts beside two that are composed", in_place=True)
        assert r.passes_through(1, out, [0, 1, 2]) == [False, False, True]
        r.tick(2, 0b101, in_place=True)
        r.tick(3, 0b110, in_place=True)
    finally:
        r.close()


# ---- 5. per-lane operations between mask calls -----------------------------------------
def test_reset_lane_between_mask_calls():
    r = MaskRig(200, 120, "rgba8", 3, 5)
    try:
        r.tick(0, 0b111)
        r.tick(1, 0b111)
        r.reset_lane(1)
        r.assert_states("after the reset")
        out = r.tick(2, 0b110, "lane 1 reset, lane 0 sits out")
        assert r.passes_through(2, out, [1, 2]) == [True, False]
        out = r.tick(3, 0b111)
        assert r.passes_through(3, out, [0, 1, 2]) == [False, False, False]
        r.reset_lane(0)                                   # a reset lane that then sits a call out
        r.tick(4, 0b110)
    finally:
        r.close()


def test_set_lane_state_onto_a_lane_that_sat_out():
    r = MaskRig(200, 120, "rgba8", 3, 4)
    try:
        r.tick(0, 0b111)
        r.tick(1, 0b101)                                  # lane 1 sat out: its bank bit differs from its neighbours'
        st = _state(r.hs[2])                              # lane 1 takes over stream 2's state
        r.hl.set_lane_state(1, st)
        r.hs[1].set_state(st)
        r.assert_states("after set_lane_state")
        out = r.tick(2, 0b010)
        assert r.passes_through(2, out, [1]) == [False]
        r.tick(3, 0b111)
        # ... and onto a lane that never ran, on a handle of its own
        q = MaskRig(200, 120, "rgba8", 3, 4)
        try:
            q.tick(0, 0b101)
            q.hl.set_lane_state(1, st)
            q.hs[1].set_state(st)
            q.has[1] = True
            q.tick(1, 0b111)
            q.tick(2, 0b010)
        finally:
            q.close()
    finally:
        r.close()


def test_apply_magnification_off_and_on_between_mask_calls():
    r = MaskRig(200, 120, "rgba8", 3, 6)
    try:
        r.tick(0, 0b111)
        r.tick(1, 0b111)
        r.set_params(apply_magnification=False)
        assert r.passes_through(2, r.tick(2, 0b011, "off"), [0, 1]) == [True, True]
        assert r.passes_through(3, r.tick(3, 0b110, "off"), [1, 2]) == [True, True]
        r.set_params()
        assert r.passes_through(4, r.tick(4, 0b111, "on again"), [0, 1, 2]) == [False, False, False]
        r.tick(5, 0b101)
    finally:
        r.close()


def test_set_params_with_a_lane_that_sits_out_the_next_tick():
    r = MaskRig(200, 120, "rgba8", 3, 7)
    try:
        r.tick(0, 0b111)
        r.tick(1, 0b111)
        r.set_params(phase_scale=10.0, edge_mode=1)
        r.tick(2, 0b101, "edge_mode: lanes 0 and 2 take the new-edge frame")
        r.tick(3, 0b111, "lane 1: old-edge state, new-edge frame, a tick late")
        r.tick(4, 0b010)
        r.set_params(phase_scale=10.0, edge_mode=1, levels=6)     # another K2 table and op
        r.tick(5, 0b110, "levels 6")
        r.set_params()
        r.tick(6, 0b111, "back")
    finally:
        r.close()


# ---- 6. layouts and pairs ------------------------------------------------------------
def test_convert_pair_with_masks():
    import mm355
    W, H, lanes, ticks = 200, 120, 3, 4
    r = MaskRig(W, H, "nv12", lanes, ticks, out_name="rgba8")
    try:
        clips = _clips(W, H, "nv12", lanes, ticks)
        out = r.tick(0, 0b101, "the plain conversion").cpu().numpy()
        for k in (0, 2):
            T.assert_close_u8(out[k].reshape(H, W, 4), C.plain(clips[0, k].reshape(H * 3 // 2, W), r.fi, mm355.RGBA8))
        out = r.tick(1, 0b111, "lane 1: the plain conversion beside composed lanes").cpu().numpy()
        T.assert_close_u8(out[1].reshape(H, W, 4), C.plain(clips[1, 1].reshape(H * 3 // 2, W), r.fi, mm355.RGBA8))
        plain = C.plain(clips[1, 0].reshape(H * 3 // 2, W), r.fi, mm355.RGBA8)
        assert (out[0].reshape(H, W, 4)[..., :3] != plain[..., :3]).mean() > 0.05, "the operator ran"
        r.tick(2, 0b110)
        r.tick(3, 0b011)
    finally:
        r.close()


def test_pitched_pair_and_a_buffer_that_ends_with_the_last_selected_lane():
    """Decoder layout in, tight out; both buffers end with the extent of the
    highest selected lane's frame (the layouts are validated with count = that
    lane + 1), and nothing but the selected frames' samples is written."""
    import mm355
    W, H, lanes = 200, 120, 4
    masks = [0b0111, 0b0101, 0b0011, 0b1111]
    clips = _clips(W, H, "nv12", lanes, len(masks))
    lin, lout = mm355.Surface.aligned(W, H, mm355.NV12, 256, 16), mm355.Surface.tight(W, H, mm355.NV12)
    assert lin.frame_stride > lin.bytes(W, H) or lin.pitch > W
    r = MaskRig(W, H, "nv12", lanes, len(masks))
    hp = mm355.Handle(W, H, _params())                   # the pitched calls, in step with the rig's tight ones
    hp.set_lanes(lanes)
    try:
        for t, mask in enumerate(masks):
            want = r.tick(t, mask).cpu().numpy()
            n = mask.bit_length()                        # frames the buffers hold
            size_in = (n - 1) * lin.frame_stride + lin.bytes(W, H)
            size_out = (n - 1) * lout.frame_stride + lout.bytes(W, H)
            a = torch.from_numpy(SF.scatter("nv12", W, H, list(clips[t, :n]), lin, size=size_in)).cuda()
            sent = SF.sentinel(size_out)
            b = torch.from_numpy(sent).cuda()
            assert a.numel() == size_in and b.numel() == size_out
            hp.process_lanes_mask(mask, a, lin, b, lout)
            torch.cuda.synchronize()
            res = b.cpu().numpy()
            got = SF.gather("nv12", W, H, res, lout, n)
            keep = np.ones(size_out, bool)
            for k in _bits(mask, lanes):
                assert np.array_equal(got[k], want[k]), (t, k)
                keep &= ~SF.sample_mask("nv12", W, H, lout, k + 1, size_out) | SF.sample_mask("nv12", W, H, lout, k, size_out)
            bad = np.flatnonzero(keep & (res != sent))
            assert bad.size == 0, f"tick {t}: {bad.size} bytes outside the selected frames written, first at {bad[:8]}"
        for k in range(lanes):
            assert torch.equal(_state(hp, k), _state(r.hl, k)), "the state does not depend on a layout"
        assert hp.lanes_with_state() == r.hl.lanes_with_state()
    finally:
        hp.close()
        r.close()


# ---- 7. refusals ---------------------------------------------------------------------
def test_refusals_leave_every_lane_as_it_was():
    import mm355
    W, H, lanes = 200, 120, 3
    r = MaskRig(W, H, "rgba8", lanes, 4)
    lib = mm355.lib()
    try:
        r.tick(0, 0b011)
        r.tick(1, 0b001)
        h, lay, src = r.hl, r.li, r.src
        before = [_state(h, k) for k in (0, 1)]
        junk = torch.full((lanes, r.fbo), FILL, dtype=torch.uint8, device="cuda")

        def unchanged(what):
            assert h.lanes() == lanes and h.lanes_with_state() == 0b011, what
            for k in (0, 1):
                assert torch.equal(_state(h, k), before[k]), (what, k)
            assert _code(lambda: _state(h, 2)) == NO_STATE, what
            assert bool((junk == FILL).all()), (what, "the output was written")

        # a bit at or above the lane count
        for mask in (0b1000, 0b1111, 1 << 63, 2 ** 64 - 1):
            assert _code(lambda: h.process_lanes_mask(mask, src[2], lay, junk, lay)) == INVALID, hex(mask)
        unchanged("a bit at or above the lane count")
        # no lanes set (the empty mask too)
        for mask in (0b1, 0):
            assert _code(lambda: r.hs[0].process_lanes_mask(mask, src[2], lay, junk, lay)) == INVALID
        assert r.hs[0].lanes_with_state() == 0
        # the modes lanes do not take
        for pk in ({"mode": mm355.MODE_STEERABLE, "orientations": 4}, {"show_magnitude": 1}, {"show_phase": 1}):
            h.set_params(_params(**pk))
            assert _code(lambda: h.process_lanes_mask(0b111, src[2], lay, junk, lay)) == UNSUPPORTED, pk
            h.set_params(_params())
            unchanged(pk)
        # null pointers
        null = ctypes.POINTER(mm355.Surface)()
        p, q, bl = src[2].data_ptr(), junk.data_ptr(), ctypes.byref(lay)
        assert lib.mm_process_lanes_mask(h.h, 0b111, p, null, q, bl, None) == INVALID
        assert lib.mm_process_lanes_mask(h.h, 0b111, p, bl, q, null, None) == INVALID
        assert lib.mm_process_lanes_mask(h.h, 0, p, null, q, bl, None) == INVALID
        assert lib.mm_process_lanes_mask(h.h, 0b111, None, bl, q, bl, None) == INVALID
        assert lib.mm_process_lanes_mask(h.h, 0b111, p, bl, None, bl, None) == INVALID
        assert lib.mm_lanes_with_state(h.h, None) == INVALID
        unchanged("null pointers")
        # two formats that are no pair; odd sizes of a Y'CbCr format
        assert _code(lambda: h.process_lanes_mask(0b111, src[2], lay, junk,
                                                  mm355.Surface.tight(W, H, mm355.RGBA32F))) == INVALID
        unchanged("no pair")
        odd = mm355.Handle(97, 63, _params())
        odd.set_lanes(2)
        nv = mm355.Surface.tight(98, 64, mm355.NV12)           # (no NV12 layout exists for an odd size)
        assert _code(lambda: odd.process_lanes_mask(0b11, junk, nv, junk, nv)) == UNSUPPORTED
        assert odd.lanes_with_state() == 0
        odd.close()
        # the empty mask: MM_OK, nothing queued, nothing changed, whatever in and out are
        assert lib.mm_process_lanes_mask(h.h, 0, None, bl, None, bl, None) == 0
        unchanged("the empty mask")
        out = r.tick(2, 0b111, "after the refusals")
        assert r.passes_through(2, out, [0, 1, 2]) == [False, False, True]
    finally:
        r.close()


# ---- 8. a lane's selected frames against the CPU oracle ---------------------------------
def test_masked_lane_vs_oracle():
    import mm355
    W, H, lanes = 128, 96, 3
    masks = [0b111, 0b111, 0b101, 0b111, 0b010, 0b111]
    ticks = len(masks)
    clips = [T.synth(W, H, ticks, t0=5 * k, seed=0x5EED0000 + 31 * k, fmt="u8") for k in range(lanes)]
    src = torch.from_numpy(np.stack([np.stack([clips[k][t] for k in range(lanes)]) for t in range(ticks)])).cuda()
    got = torch.zeros_like(src)
    lay = mm355.Surface.tight(W, H, mm355.RGBA8)
    hl = mm355.Handle(W, H, _params())
    hl.set_lanes(lanes)
    for t, mask in enumerate(masks):
        hl.process_lanes_mask(mask, src[t], lay, got[t], lay)
    torch.cuda.synchronize()
    hl.close()
    out = got.cpu().numpy()
    k = 1                                                 # sits out tick 2, runs alone at tick 4
    sel = [t for t, mask in enumerate(masks) if (mask >> k) & 1]
    assert sel == [0, 1, 3, 4, 5]
    ref = T.oracle_run(W, H, [clips[k][t] for t in sel], L, S)
    assert np.array_equal(out[sel[0], k], clips[k][sel[0]])
    for j, t in enumerate(sel[1:], 1):
        d = np.abs(out[t, k].astype(np.int32) - ref[j].astype(np.int32))
        print(f"lane {k} tick {t}: max {d.max()}  share {(d > 0).mean():.2e}")
        T.assert_close_u8(out[t, k], ref[j])
    assert not np.array_equal(out[3, k], clips[k][3])


# ---- 9. mm_cli --lanes --lane-drop -----------------------------------------------------
@pytest.mark.parametrize("opt", [["--nv12"], []], ids=["nv12", "default"])
def test_cli_lane_drop(tmp_path, opt):
    W, H, M, ticks = 64, 48, 2, 5
    n = M * ticks
    clips = _clips(W, H, "nv12", M, ticks)                 # [t][k]: input frame t * M + k
    inter = [clips[j // M, j % M] for j in range(n)]
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    _write_y4m(src, W, H, inter)
    base = opt + ["-l", str(L), "-s", str(S)]
    subprocess.check_call([CLI] + base + ["-i", src, "-o", dst, "--lanes", str(M), "--lane-drop", "1:2"], timeout=120,
                          stdout=subprocess.DEVNULL)
    got = _y4m_frames(dst, n)

    def single(name, frames):
        one, out = str(tmp_path / f"{name}.y4m"), str(tmp_path / f"{name}_out.y4m")
        _write_y4m(one, W, H, frames)
        subprocess.check_call([CLI] + base + ["-i", one, "-o", out, "-b", "1"], timeout=120, stdout=subprocess.DEVNULL)
        return _y4m_frames(out, len(frames))

    want0 = single("lane0", [clips[t, 0] for t in range(ticks)])
    for t in range(ticks):
        assert got[t * M] == want0[t], ("lane 0", t)
    kept = [t for t in range(ticks) if t != 2]
    want1 = single("lane1", [clips[t, 1] for t in kept])
    for j, t in enumerate(kept):
        assert got[t * M + 1] == want1[j], ("lane 1", t)
    assert got[2 * M + 1] == single("dropped", [clips[2, 1]])[0], "the dropped slot: the passthrough of its input"
    assert got[3 * M + 1] != single("lane1_all", [clips[t, 1] for t in range(ticks)])[3], "the drop changed lane 1's next frame"
