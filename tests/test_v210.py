"""MM_V210 on the GPU.  A V210 frame IS the MM_Y210 frame whose words are
code << 6 (include/mm.h), so every check here is BITWISE against the MM_Y210
path, which tests/test_y210.py holds to the oracle: the same codes go in through
both formats (tests/v210.py packs the Y210 frame), the V210 output must be the
Y210 output >> 6 packed again with zero unused fields and zero bits 30-31, and
the temporal state (mm_get_state) must be the Y210 run's, byte for byte.  No
tolerance anywhere.

Every V210 run goes through one runner that lays the frames out in a surface
(the tight one included: 98 x 62, 64 x 48, 200 x 120, 208 x 120 and 1280 x 720
have row padding even there), poisons every byte of both buffers that is no
used dword and asserts afterwards that the output buffer's poison is all still
there: row tails, the unused dwords of a partial last group's pitch, the gap
between frames, the bytes before the base and after the last extent.  Input
dwords carry random bits 30-31 and random unused fields of a partial last group,
which must not matter; the passthrough frames (the first, and
apply_magnification = 0) must carry them through bitwise.

Sizes: 48 x 32 (one group block of K1 and one column tile, N = 64), 64 x 48
(W % 6 = 4), 98 x 62 (W % 6 = 2, N = 128), 200 x 120 and 208 x 120 (past one
192-column tile of the compose; W % 6 = 2 and 4), and one 1280 x 720 two-frame
case (pitch 3,456 against 3,416 row bytes, N = 2048).  Without the feature every
test fails at mm_frame_bytes (the runner asks Surface.tight first).
"""
import functools

import numpy as np
import pytest

import mmtest as T
import v210
import y210

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
V601 = (601, False)
V601_FULL = (601, True)
V709 = (709, False)
V709_FULL = (709, True)
V2020 = (2020, False)
V2020_FULL = (2020, True)
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """torch is imported before the library is loaded (mm355 loads it on first
    use, Params.make included), as tests/mmtest.py's gpu_run does: loaded the
    other way round, torch finds no device."""
    import torch  # noqa: F401


@functools.lru_cache(maxsize=None)
def _frames(W, H, n, v=V709):
    """(Y210 frames, V210 frames) of the same codes: a moving synthetic scene
    encoded by tests/y210.py, with a tenth of the words replaced by random
    10-bit codes, the ends of the code range (0 .. 3, 1020 .. 1023) among them;
    the V210 frames with random stray bits (v210.pack)."""
    rng = np.random.default_rng(2100 + W + 7 * H)
    ys, vs = [], []
    for rgb in T.synth(W, H, n, fmt="u8"):
        f = y210.encode(rgb, *v) >> 6
        hit = rng.random(f.shape) < 0.1
        f[hit] = rng.integers(0, 1024, int(hit.sum())).astype(np.uint16)
        f.reshape(-1)[:8] = np.array([0, 1, 2, 3, 1020, 1021, 1022, 1023], np.uint16)
        f = (f << 6).astype(np.uint16)
        p = v210.pack(f, stray=rng)
        f.setflags(write=False)
        p.setflags(write=False)
        ys.append(f)
        vs.append(p)
    return tuple(ys), tuple(vs)


def _params(edge=0, apply=True, extra=None):
    import mm355
    return mm355.Params.make(levels=L, phase_scale=S, edge_mode=edge, apply_magnification=apply, **(extra or {}))


def _go(C, W, H, fmt, flat, *, mode="stream", batch=8, lay=None, lay_out=None, base=0, params=None, poison=0xA5,
        lanes=0):
    """`flat`: the frames as their sample bytes (C.flat's / y210's tight bytes),
    C: the codec module (v210 or y210: the same surface helpers).  Lays them out
    in `lay` (default: the tight surface) at byte `base`, everything else
    poisoned, runs them, asserts that no byte of the output buffer outside the
    samples changed, and returns (the output frames' sample bytes, the state's
    bytes after the last frame).  lay / lay_out None: the tight entry points
    (mm_process, mm_process_stream); else the surface ones.  mode: "stream",
    "frame", "host" (frame calls on host memory) or "lanes" (frame k is lane
    k % lanes' frame k / lanes: one mm_process_lanes call per tick)."""
    import torch
    import mm355
    n = len(flat)
    tight = mm355.Surface.tight(W, H, fmt)      # (fails here without the feature: mm_surface_tight -> mm_frame_bytes' check)
    assert mm355.frame_bytes(W, H, fmt) == tight.frame_stride
    li, lo = lay or tight, lay_out or lay or tight
    named = lay is not None or lay_out is not None or mode == "lanes"
    in_size, out_size = C.buffer_bytes(W, H, li, n, base), C.buffer_bytes(W, H, lo, n, base)
    src = C.scatter(W, H, flat, li, base, fill=poison, size=in_size)
    keep = ~C.sample_mask(W, H, lo, n, out_size, base)
    h = mm355.Handle(W, H, params or _params())
    h.set_batch(batch)
    if mode == "host":
        a, b = src, np.full(out_size, poison ^ 0x55, np.uint8)
        for k in range(n):
            ak, bk = a[base + k * li.frame_stride:], b[base + k * lo.frame_stride:]
            if named:
                h.process_surface(ak, li, bk, lo, on_device=False)
            else:
                h.process(ak, bk, fmt, on_device=False)
        res = b
    else:
        a = torch.from_numpy(src).cuda()
        b = torch.full((out_size,), poison ^ 0x55, dtype=torch.uint8, device="cuda")
        if mode == "stream":
            if named:
                h.process_stream_surfaces(a[base:], li, b[base:], lo, n)
            else:
                h.process_stream(a[base:], b[base:], n, fmt)
        elif mode == "frame":
            for k in range(n):
                ak, bk = a[base + k * li.frame_stride:], b[base + k * lo.frame_stride:]
                if named:
                    h.process_surface(ak, li, bk, lo)
                else:
                    h.process(ak, bk, fmt)
        else:
            assert mode == "lanes" and n % lanes == 0
            h.set_lanes(lanes)
            for t in range(n // lanes):
                h.process_lanes(a[base + t * lanes * li.frame_stride:], li, b[base + t * lanes * lo.frame_stride:], lo)
        torch.cuda.synchronize()
        res = b.cpu().numpy()
    st = None
    if mode != "lanes":
        buf = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(buf)
        torch.cuda.synchronize()
        st = buf.cpu().numpy()
    h.close()
    assert np.all(res[keep] == (poison ^ 0x55)), "a byte that is no used sample was written"
    return C.gather(W, H, res, lo, n, base), st


def _yflat(frames):
    return [np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in frames]


def _vflat(frames, W):
    return [v210.flat(p, W) for p in frames]


def _expect(W, H, yout):
    """The Y210 path's output frames (tight bytes) as the used dwords V210 must write."""
    return [v210.used(v210.pack(np.ascontiguousarray(f).view(np.uint16).reshape(H, 2 * W)), W) for f in yout]


def _same(W, H, got, want, vin, first=1, what=""):
    """got: V210 outputs (sample bytes); want: _expect's; the first `first`
    frames pass through bitwise, stray bits included."""
    for k, (g, w) in enumerate(zip(got, want)):
        g = v210.unflat(g, W, H)
        if k < first:
            assert np.array_equal(g, v210.used(vin[k], W)), (what, k, "passthrough is bitwise, stray bits included")
            continue
        assert not np.any(g >> 30), (what, k, "bits 30-31 of every output dword are zero")
        bad = g != w
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert np.array_equal(g, v210.clean(g, W)), (what, k, "unused fields of a written dword are zero")
    # not a passthrough: the operator moved the codes
    moved = np.mean(v210.unflat(got[-1], W, H) != v210.clean(v210.used(vin[-1], W), W)) if first < len(got) else 1.0
    assert moved > 0.3, (what, moved)


def _pair(W, H, n, v, *, edge=0, extra=None, apply=True, **kw):
    """The same codes through MM_Y210 and MM_V210 with the same call form and
    parameters: (y outputs, y state, v outputs, v state, the V210 input frames)."""
    ys, vs = _frames(W, H, n, v)
    yo, yst = _go(y210, W, H, y210.fmt_code(*v), _yflat(ys), params=_params(edge, apply, extra), **kw)
    vo, vst = _go(v210, W, H, v210.fmt_code(*v), _vflat(vs, W), params=_params(edge, apply, extra), **kw)
    return yo, yst, vo, vst, vs


# W, H, frames, (matrix, range), edge mode
CASES = [
    (48, 32, 3, V601, 0),            # one group block, one column tile, N = 64
    (48, 32, 3, V709_FULL, 1),
    (64, 48, 3, V709, 0),            # W % 6 = 4: a 12-byte last group
    (64, 48, 3, V601_FULL, 1),
    (64, 48, 3, V2020, 0),
    (98, 62, 3, V709, 1),            # W % 6 = 2: an 8-byte last group; N = 128
    (98, 62, 3, V601, 0),
    (98, 62, 3, V2020_FULL, 0),
    (200, 120, 3, V709, 0),          # two column tiles, the second one 8 columns (W % 6 = 2)
    (200, 120, 3, V601_FULL, 1),
    (208, 120, 3, V2020, 1),         # ... 16 columns (W % 6 = 4)
    (208, 120, 3, V601, 0),
]


@pytest.mark.parametrize("W,H,n,v,edge", CASES)
def test_v210_is_the_y210_path_bitwise(W, H, n, v, edge):
    """Single calls and stream calls with batch 1 and 3, pyramid mode: output
    and state bitwise the MM_Y210 path's; the tight frames' padding untouched."""
    for what, kw in (("frame", dict(mode="frame", batch=1)), ("stream 1", dict(mode="stream", batch=1)),
                     ("stream 3", dict(mode="stream", batch=3))):
        yo, yst, vo, vst, vin = _pair(W, H, n, v, edge=edge, **kw)
        _same(W, H, vo, _expect(W, H, yo), vin, what=what)
        assert np.array_equal(yst, vst) and yst.any(), (what, "the state is the Y210 frame's")


@pytest.mark.parametrize("W,H,v", [(64, 48, V709), (98, 62, V601_FULL), (200, 120, V2020)])
def test_standard_mode(W, H, v):
    extra = dict(mode=1, **T._std_fields({}))
    for kw in (dict(mode="frame", batch=1), dict(mode="stream", batch=3)):
        yo, yst, vo, vst, vin = _pair(W, H, 3, v, extra=extra, **kw)
        _same(W, H, vo, _expect(W, H, yo), vin, what="standard")
        assert np.array_equal(yst, vst) and yst.any()


@pytest.mark.parametrize("W,H,v", [(64, 48, V709), (98, 62, V601)])
def test_steerable_mode(W, H, v):
    """MM_MODE_STEERABLE (O = 4, DIFF) wherever Y210 has it: the same bytes and
    the same local-phase state."""
    extra = dict(mode=2, orientations=4)
    yo, yst, vo, vst, vin = _pair(W, H, 3, v, extra=extra, mode="stream", batch=3)
    _same(W, H, vo, _expect(W, H, yo), vin, what="steerable")
    assert np.array_equal(yst, vst) and yst.any()


@pytest.mark.parametrize("W,H,v", [(64, 48, V709), (98, 62, V601_FULL), (208, 120, V2020)])
def test_host_memory_frames(W, H, v):
    """Frames in host memory (staged plane by plane: the host frame's padding
    is neither read nor written, in the tight frame too)."""
    yo, yst, vo, vst, vin = _pair(W, H, 3, v, mode="host", batch=1)
    _same(W, H, vo, _expect(W, H, yo), vin, what="host")
    assert np.array_equal(yst, vst)


@pytest.mark.parametrize("W,H,v", [(98, 62, V709), (64, 48, V601)])
def test_pitched_surfaces(W, H, v):
    """Input and output in different pitched layouts at a base that is a
    multiple of 16 and no multiple of 32, stream and frame calls and host
    memory: the used dwords are the tight run's, every other byte is untouched
    (nor read: two poisons give the same result)."""
    import mm355
    fmt = v210.fmt_code(*v)
    ys, vs = _frames(W, H, 3, v)
    want, wst = _go(v210, W, H, fmt, _vflat(vs, W), mode="stream", batch=3)
    lin = mm355.Surface.aligned(W, H, fmt, 256, 16)
    lout = mm355.Surface.tight(W, H, fmt)
    lout.pitch = (v210.row_bytes(W) + 15) // 16 * 16 + 16       # the row's bytes and one group of padding
    lout.frame_stride = lout.pitch * H + 48
    for mode in ("stream", "frame", "host"):
        for poison in (0xA5, 0x3C):
            got, st = _go(v210, W, H, fmt, _vflat(vs, W), mode=mode, batch=3, lay=lin, lay_out=lout, base=16,
                          poison=poison)
            for k in range(3):
                assert np.array_equal(got[k], want[k]), (mode, hex(poison), k)
            assert np.array_equal(st, wst)


def test_lanes():
    """Four live streams, one frame each per mm_process_lanes call: lane k's
    frames are bitwise its own MM_Y210 stream's (always the unfused pair for
    V210), the first tick passes through, padding untouched."""
    W, H, M, ticks, v = 98, 62, 4, 3, V709
    ys, vs = _frames(W, H, M * ticks, v)
    # lane k's stream: a scene of its own (frames k, k + M, ...)
    vo, _ = _go(v210, W, H, v210.fmt_code(*v), _vflat(vs, W), mode="lanes", lanes=M)
    for k in range(M):
        yo, _ = _go(y210, W, H, y210.fmt_code(*v), _yflat(ys[k::M]), mode="stream", batch=1)
        _same(W, H, vo[k::M], _expect(W, H, yo), vs[k::M], what=f"lane {k}")


def test_passthrough_is_bitwise():
    """apply_magnification = 0 passes every used dword through bitwise, bits
    30-31 and a partial group's unused fields included, in tight and pitched
    layouts; the state still follows the input (the Y210 run's)."""
    import mm355
    for W, H, v in ((98, 62, V709), (64, 48, V601), (48, 32, V2020)):
        ys, vs = _frames(W, H, 3, v)
        fmt = v210.fmt_code(*v)
        _, yst = _go(y210, W, H, y210.fmt_code(*v), _yflat(ys), params=_params(apply=False), mode="stream", batch=3)
        for lay in (None, mm355.Surface.aligned(W, H, fmt, 256, 16)):
            for mode in ("stream", "frame"):
                got, st = _go(v210, W, H, fmt, _vflat(vs, W), params=_params(apply=False), mode=mode, batch=3, lay=lay)
                _same(W, H, got, [None] * 3, vs, first=3, what="apply_magnification = 0")
                assert np.array_equal(st, yst)


@pytest.mark.parametrize("W,H,v", [(136, 520, V601), (136, 520, V709), (136, 518, V601), (136, 518, V2020_FULL)])
def test_k1_load_forms(W, H, v):
    """K1's other two load forms at N = 1024, as tests/test_y210.py reaches them:
    a 5-frame stream of 260 row pairs per frame in one launch (the batch form:
    six source rows per column shared by two row pairs) and of 259 (the regular
    four-row form); frame calls run the one-pair form.  Output and state."""
    yo, yst, vo, vst, vin = _pair(W, H, 5, v, mode="stream", batch=8)
    _same(W, H, vo, _expect(W, H, yo), vin, what="K1 form")
    assert np.array_equal(yst, vst) and yst.any()


def test_720p_two_frames():
    """1280 x 720: pitch 3,456 against 3,416 row bytes, N = 2048 and seven
    column tiles (the last one 128 columns, W % 6 = 2)."""
    W, H, v = 1280, 720, V709
    assert (v210.row_bytes(W), v210.pitch(W)) == (3416, 3456)
    yo, yst, vo, vst, vin = _pair(W, H, 2, v, mode="stream", batch=2)
    _same(W, H, vo, _expect(W, H, yo), vin, what="720p")
    assert np.array_equal(yst, vst) and yst.any()


def _code(call):
    import mm355
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_refusals_leave_the_handle_usable():
    """Odd sizes, the debug views, V210 in with Y210 out, a base or a frame
    stride at 8 mod 16: refused before anything is queued; the handle then runs
    the next frames as if nothing had happened."""
    import torch
    import mm355
    W, H, v = 64, 48, V709
    fmt = v210.fmt_code(*v)
    ys, vs = _frames(W, H, 3, v)
    want, _ = _go(v210, W, H, fmt, _vflat(vs, W), mode="frame", batch=1)
    tight = mm355.Surface.tight(W, H, fmt)
    a = torch.from_numpy(np.stack([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in vs])).cuda()
    b = torch.zeros_like(a)
    h = mm355.Handle(W, H, _params())
    h.process(a[0], b[0], fmt)
    # a frame pointer at 8 mod 16, on either side; a frame stride at 8 mod 16
    assert _code(lambda: h.process(a[0][8:], b[1], fmt)) == INVALID
    assert _code(lambda: h.process(a[1], b[0][8:], fmt)) == INVALID
    s8 = mm355.Surface.tight(W, H, fmt)
    s8.frame_stride += 8
    assert _code(lambda: h.process_stream_surfaces(a, s8, b, tight, 2)) == INVALID
    # V210 in with Y210 out, and the other way round
    ty = mm355.Surface.tight(W, H, y210.fmt_code(*v))
    big = torch.zeros(ty.frame_stride, dtype=torch.uint8, device="cuda")
    assert _code(lambda: h.process_surface(a[1], tight, big, ty)) == INVALID
    assert _code(lambda: h.process_convert(a[1], tight, big, ty)) == UNSUPPORTED
    assert _code(lambda: h.process_convert(big, ty, b[1], tight)) == UNSUPPORTED
    # the debug views
    for view in ("show_magnitude", "show_phase"):
        h.set_params(_params(extra={view: True}))
        assert _code(lambda: h.process(a[1], b[1], fmt)) == UNSUPPORTED
    h.set_params(_params())
    h.process(a[1], b[1], fmt)
    h.process(a[2], b[2], fmt)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    for k in range(3):
        got = v210.flat(res[k].view(np.uint32).reshape(H, -1), W)
        assert np.array_equal(got, want[k]), k
    # odd sizes: unsupported from every entry point of a handle of that size
    for Wo, Ho in ((63, 48), (64, 47)):
        ho = mm355.Handle(Wo, Ho, _params())
        junk = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        assert _code(lambda: ho.process(junk, junk, fmt)) == UNSUPPORTED
        assert _code(lambda: ho.process_stream(junk, junk, 1, fmt)) == UNSUPPORTED
        ho.process(torch.zeros(Wo * Ho * 4, dtype=torch.uint8, device="cuda"),
                   torch.zeros(Wo * Ho * 4, dtype=torch.uint8, device="cuda"), mm355.RGBA8)   # still usable
        torch.cuda.synchronize()
        ho.close()


def test_python_layer():
    """OnRenderImage(src, dst, fmt=mm355.V210) on [H, pitch / 4] uint32 frames,
    device tensors (as int32 storage where torch has no uint32 arithmetic: the
    bytes are what travels) and host arrays: the runner's bytes."""
    import mm355
    W, H, v = 98, 62, V709
    fmt = v210.fmt_code(*v)
    ys, vs = _frames(W, H, 3, v)
    want, _ = _go(v210, W, H, fmt, _vflat(vs, W), mode="frame", batch=1)
    proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
    for k in range(3):
        dst = np.full_like(vs[k], 0x5A5A5A5A)
        proc.OnRenderImage(np.array(vs[k]), dst, fmt=fmt)
        assert np.array_equal(v210.flat(dst, W), want[k]), k
        assert np.all(dst[:, v210.dwords(W):] == 0x5A5A5A5A), "the host frame's row padding is not written"
    with pytest.raises(mm355.MMError):
        proc.OnRenderImage(np.zeros((H, 2 * W), np.uint16), np.zeros((H, 2 * W), np.uint16), fmt=fmt)
    proc.OnDestroy()


def test_cli_writes_the_y210_file(tmp_path):
    """mm_cli --v210 on a C422p10 clip (98 x 62: a partial last group, row
    padding in the tight frame) writes --y210's output file byte for byte, with
    --matrix, --full-range, --surface-align and --lanes too; any other
    extension holds the raw v210 frames at the standard pitch, padding zero,
    whose used dwords are the binding's."""
    import os
    import subprocess
    W, H, n, v = 98, 62, 4, V709
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "phase-based-motion-manipulation_amd", "bin", "mm_cli")
    ys, vs = _frames(W, H, n, v)
    src = str(tmp_path / "in.y4m")
    with open(src, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C422p10\n".encode())
        for b in ys:
            y, cb, cr = (np.ascontiguousarray(p >> 6) for p in y210.split(b))
            f.write(b"FRAME\n" + y.tobytes() + cb.tobytes() + cr.tobytes())
    base = ["-i", src, "-l", str(L), "-s", str(S), "-b", "4"]
    outs = {}
    for what, extra in (("709", ["--matrix", "709"]), ("601 full", ["--full-range"]),
                        ("surfaces", ["--matrix", "709", "--surface-align", "256,16"]),
                        ("lanes", ["--matrix", "709", "--lanes", "2"])):
        for opt in ("--y210", "--v210"):
            dst = str(tmp_path / f"{opt[2:]}_{what.replace(' ', '_')}.y4m")
            subprocess.check_call([cli, opt, "-o", dst] + base + extra, timeout=120)
            outs[opt, what] = open(dst, "rb").read()
        assert outs["--v210", what] == outs["--y210", what], what
        assert len(outs["--v210", what]) > n * 4 * W * H
    assert outs["--v210", "709"] == outs["--v210", "surfaces"] and outs["--v210", "709"] != outs["--v210", "601 full"]
    assert outs["--v210", "709"] != outs["--v210", "lanes"]          # (two streams of two frames: another result)
    rawp = str(tmp_path / "out.v210")
    subprocess.check_call([cli, "--v210", "--matrix", "709", "-o", rawp] + base, timeout=120)
    raw = np.frombuffer(open(rawp, "rb").read(), np.uint32).reshape(n, H, v210.pitch(W) // 4)
    # the clip holds clean codes: the runner's frames without their stray bits
    clean = [v210.pack(f) for f in ys]
    want, _ = _go(v210, W, H, v210.fmt_code(*v), _vflat(clean, W), mode="stream", batch=4)
    for k in range(n):
        assert np.array_equal(v210.flat(raw[k], W), want[k]), k
        assert not raw[k][:, v210.dwords(W):].any(), "the raw file's row padding is zero"
