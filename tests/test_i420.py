"""MM_I420 / MM_I420_FULL three-plane 4:2:0 frames through the C-ABI on the HIP path.

An I420 frame IS the NV12 frame with the same samples (include/mm.h): where a
pixel's two chroma samples lie is a matter of loads and stores.  So the
yardstick is exact: the output is the shipped NV12 path's output on the
interleaved frame, de-interleaved, and the temporal state is that NV12
frame's, both BITWISE, in every mode, call form, batch size, edge mode and
layout.  Frames are tests/ycbcr.py's encodes of mmtest.synth, permuted by
tests/i420.py's from_nv12.

So that the suite does not rest on the NV12 path alone, test_i420_vs_oracle
compares with the CPU oracle directly at the project's 8-bit bar
(mmtest.assert_close_u8: +-1 code on at most 0.1 % of the bytes of the whole
buffer).  The cap is a condition on the kernels: on exactly these inputs the
fp32 oracle differs from the float64 twin by at most 1 code on 2.8e-5
(200 x 120), 1.1e-4 (98 x 62) and 6.2e-5 (1920 x 128) of the bytes, shares the
permutation does not change, all below an eighth of the cap.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import i420
import mmtest as T
import oracle_py as O
import ycbcr

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")
STEER = {"mode": 2, "orientations": 4}     # O = 4, DIFF


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _nv12(W, H, n, matrix=601, full=False, stress=False, neutral=False):
    """The interleaved frames (NV12 bytes [H * 3 / 2][W]), computed once per case."""
    out = []
    for t, rgb in enumerate(T.synth(W, H, n, fmt="u8")):
        buf = ycbcr.encode(rgb, matrix, full)
        if stress:
            buf = ycbcr.chroma_stress(buf, t)
        if neutral:
            buf[H:] = 128
        out.append(buf)
    return tuple(out)


def _planar(frames):
    return [i420.from_nv12(f) for f in frames]


def _params(edge=0, apply=True, extra=None, standard=None):
    import mm355
    extra = dict(extra or {})
    if standard is not None:
        extra.update(mode=mm355.MODE_STANDARD, **T._std_fields(standard))
    return mm355.Params.make(levels=L, phase_scale=S, edge_mode=edge, apply_magnification=apply, **extra)


def _go(W, H, frames, fmt, mode="stream", batch=8, **pkw):
    """The frames through one handle; -> (output frames, mm_get_state's bytes)."""
    import torch
    import mm355
    h = mm355.Handle(W, H, _params(**pkw))
    h.set_batch(batch)
    if mode == "host":
        outs = []
        for f in frames:
            o = np.empty_like(f)
            h.process(f, o, fmt, on_device=False)
            outs.append(o)
    else:
        dev_in = torch.from_numpy(np.stack(frames)).cuda()
        dev_out = torch.empty_like(dev_in)
        if mode == "frame":
            for k in range(len(frames)):
                h.process(dev_in[k], dev_out[k], fmt)
        else:
            h.process_stream(dev_in, dev_out, len(frames), fmt)
    held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.get_state(held)
    torch.cuda.synchronize()
    if mode != "host":
        outs = list(dev_out.cpu().numpy())
    state = held.cpu().numpy()
    h.close()
    return outs, state


def _same(a, b, what):
    assert len(a) == len(b)
    for k in range(len(a)):
        assert np.array_equal(a[k], b[k]), (what, k, int((np.asarray(a[k]) != np.asarray(b[k])).sum()))


def _identities(W, H, nv, fmt, what, moved=True, **kw):
    """Identity 1 and 2 of include/mm.h for one run: output and state against
    the NV12 path under the same switches, bitwise.  -> the NV12 path's output."""
    want, st_want = _go(W, H, list(nv), fmt, **kw)
    got, st_got = _go(W, H, _planar(nv), fmt | i420.PLANAR, **kw)
    assert np.array_equal(got[0].reshape(-1), i420.from_nv12(nv[0]).reshape(-1)), (what, "the first frame passes through")
    _same([i420.to_nv12(g) for g in got], want, what)
    assert np.array_equal(st_got, st_want), (what, "state")
    assert np.abs(st_want.view(np.float32)).max() > 1.0
    if moved:
        for k in range(1, len(nv)):   # no passthrough can pass
            assert (got[k].reshape(-1)[:W * H] != nv[k][:H].reshape(-1)).mean() > 0.5, (what, k)
    return want


# W, H, frames, edge, environment
GEOMETRIES = [
    (64, 48, 4, 0, {}),                                                # x0 = 0: unfused; K1 one-pair form
    (200, 120, 4, 0, {}),                                              # one-shot K34 at N = 256
    (200, 120, 12, 0, {"MM_K34_ROWS": "64"}),                          # the walking K34
    (98, 62, 4, 0, {}),                                                # chroma rows of 49 bytes: the single-byte paths
    (128, 128, 4, 0, {}),                                              # no margins: every border wraps
    (128, 128, 4, 1, {}),                                              # ... or clamps
    (1920, 128, 3, 0, {}),                                             # the three N = 2048 compose instances:
    (1920, 128, 3, 0, {"MM_K34_ROWS": "16"}),                          #   walking
    (1920, 128, 3, 0, {"MM_K34_ONESHOT": "2"}),                        #   one-shot (its LDS attribute)
    (1920, 128, 3, 0, {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"}),    #   unfused
    (2056, 32, 2, 0, {"MM_K34_ROWS": "16"}),                           # the N = 4096 walking instance and its LDS attribute
]


@pytest.mark.parametrize("W,H,n,edge,env", GEOMETRIES)
def test_i420_is_the_nv12_path_bitwise(W, H, n, edge, env):
    import mm355
    nv = _nv12(W, H, n)
    with _env(**env):
        _identities(W, H, nv, mm355.NV12, "frame calls", mode="frame", batch=1, edge=edge)
        _identities(W, H, nv, mm355.NV12, "stream", mode="stream", batch=12 if n > 8 else 8, edge=edge)


# matrix, full range, chroma stress
VARIANTS = [(601, True, False), (709, False, False), (2020, True, False), (601, False, True), (709, False, True)]


@pytest.mark.parametrize("matrix,full,stress", VARIANTS)
def test_i420_variants_are_the_nv12_path_bitwise(matrix, full, stress):
    W, H, n = 200, 120, 4
    nv = _nv12(W, H, n, matrix, full, stress)
    fmt = ycbcr.fmt_code(matrix, full)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _identities(W, H, nv, fmt, f"{matrix} {full} {stress} {mode}", mode=mode, batch=batch)


def test_matrixed_i420_at_n8192_is_the_nv12_path_bitwise():
    """The N = 8192 instances: K1's matrixed three-plane forms load their columns
    in two batches there (one-pair form: frame calls; batch form: the stream)."""
    W, H, n = 4104, 48, 2
    nv = _nv12(W, H, n, 709)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _identities(W, H, nv, ycbcr.fmt_code(709), f"N = 8192 {mode}", mode=mode, batch=batch)


@pytest.mark.parametrize("matrix", [709, 2020])
def test_matrixed_frame_with_neutral_chroma_has_the_bt601_state(matrix):
    """k1_chroma adds exactly 0 for (128, 128): K1's matrixed three-plane
    instance gives the luma-plane instance's state, bit for bit."""
    W, H, n = 200, 120, 2
    fr = _planar(_nv12(W, H, n, 601, False, neutral=True))
    _, st601 = _go(W, H, fr, i420.fmt_code(601), mode="frame", batch=1)
    _, st = _go(W, H, fr, i420.fmt_code(matrix), mode="frame", batch=1)
    assert np.array_equal(st, st601)


def test_i420_standard_and_steerable_are_the_nv12_path_bitwise():
    import mm355
    for mode, batch in (("frame", 1), ("stream", 8)):
        _identities(128, 96, _nv12(128, 96, 4), mm355.NV12, f"standard {mode}", mode=mode, batch=batch, standard={})
    _identities(256, 192, _nv12(256, 192, 4), mm355.NV12, "steerable", mode="stream", extra=STEER)


@functools.lru_cache(maxsize=None)
def _ref(W, H, n):
    """The oracle on the decoded interleaved frames, encoded and permuted."""
    fr = [ycbcr.decode(b, np.float32) for b in _nv12(W, H, n)]
    return tuple(i420.from_nv12(ycbcr.encode(r)) for r in T.oracle_run(W, H, fr, L, S))


@pytest.mark.parametrize("W,H,n", [(200, 120, 4), (98, 62, 4), (1920, 128, 3)])
def test_i420_vs_oracle(W, H, n):
    import mm355
    O.set_threads(16)
    fr, ref = _planar(_nv12(W, H, n)), _ref(W, H, n)
    for mode, batch in (("frame", 1), ("stream", 8)):
        got, _ = _go(W, H, fr, mm355.I420, mode=mode, batch=batch)
        assert np.array_equal(got[0], fr[0]), "the first frame passes through bitwise"
        for k in range(1, n):
            d = np.abs(got[k].astype(np.int32) - ref[k].astype(np.int32))
            print(f"{W}x{H} {mode} frame {k}: max {int(d.max())} frac {float((d > 0).mean()):.2e} (cap {T.U8_FRAC:.0e})")
            T.assert_close_u8(got[k], ref[k])
            assert (got[k] != fr[k]).mean() > 0.5


@pytest.mark.parametrize("W,H", [(200, 120), (98, 62)])
def test_i420_passthrough(W, H):
    """apply_magnification = 0 and the first frame pass all W H 3/2 bytes through."""
    import mm355
    n = 3
    fr = _planar(_nv12(W, H, n, 709, False, True))
    for mode in ("frame", "stream", "host"):
        got, _ = _go(W, H, fr, i420.fmt_code(709), mode=mode, apply=False)
        _same(got, fr, f"apply_magnification = 0, {mode}")
        got, _ = _go(W, H, fr[:1], mm355.I420_FULL, mode=mode)
        _same(got, fr[:1], f"first frame, {mode}")
    # host-memory frames give the device calls' bytes
    a, sa = _go(W, H, fr, mm355.I420, mode="host")
    b, sb = _go(W, H, fr, mm355.I420, mode="frame", batch=1)
    _same(a, b, "host calls")
    assert np.array_equal(sa, sb) and (a[1] != fr[1]).mean() > 0.5


def test_layouts_and_formats_alternate_on_one_handle():
    """The state does not depend on the layout: NV12 and I420 calls (tight and
    pitched) alternating on one handle give the unmixed runs' outputs, bitwise."""
    import torch
    import mm355
    W, H, n = 200, 120, 6
    nv = _nv12(W, H, n)
    want, _ = _go(W, H, list(nv), mm355.NV12, mode="frame", batch=1)
    h = mm355.Handle(W, H, _params())
    lay = mm355.Surface.aligned(W, H, mm355.I420, 256, 16)
    tight = mm355.Surface.tight(W, H, mm355.I420)
    for k in range(n):
        if k % 3 == 0:      # NV12
            src = torch.from_numpy(nv[k]).cuda()
            dst = torch.empty_like(src)
            h.process(src, dst, mm355.NV12)
            got = dst.cpu().numpy()
        elif k % 3 == 1:    # I420, tight
            src = torch.from_numpy(i420.from_nv12(nv[k])).cuda()
            dst = torch.empty_like(src)
            h.process(src, dst, mm355.I420)
            got = i420.to_nv12(dst.cpu().numpy())
        else:               # I420, pitched in, tight out
            buf = i420.scatter(W, H, [i420.from_nv12(nv[k])], lay)
            src = torch.from_numpy(buf).cuda()
            dst = torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda")
            h.process_surface(src, lay, dst, tight)
            got = i420.to_nv12(dst.cpu().numpy().reshape(H * 3 // 2, W))
        assert np.array_equal(got, want[k]), k
    h.close()


def _layouts(W, H, fmt):
    import mm355
    t = mm355.Surface.tight(W, H, fmt)
    odd = i420.layout(fmt, W + 1, (W + 1) * H, W // 2 + 1)             # odd pitches: the byte paths
    odd.frame_stride = odd.bytes(W, H)
    pushed = i420.layout(fmt, W, W * H + 3, W // 2)                    # the Cb plane 3 bytes past the luma end
    pushed.frame_stride = pushed.bytes(W, H) + 1
    loose = i420.layout(fmt, t.pitch, t.chroma_offset, t.chroma_pitch, t.frame_stride + 1)   # stride = extent + 1
    return {"tight": t, "aligned": mm355.Surface.aligned(W, H, fmt, 256, 16), "odd": odd, "pushed": pushed,
            "loose": loose}


def _pitched(W, H, fr, lin, lout, mode, in_base=0, out_base=0):
    import torch
    import mm355
    n = len(fr)
    src = i420.scatter(W, H, fr, lin, base=in_base)                    # padding poisoned with 0xFF
    out_size = i420.buffer_bytes(W, H, lout, n, out_base)
    sent = ((np.arange(out_size, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
    a, b = torch.from_numpy(src).cuda(), torch.from_numpy(sent).cuda()
    h = mm355.Handle(W, H, _params())
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
    keep = ~i420.sample_mask(W, H, lout, n, out_size, out_base)
    bad = np.flatnonzero(keep & (res != sent))
    assert bad.size == 0, f"{mode}: {bad.size} padding bytes written, first at {bad[:8]}"
    return i420.gather(W, H, res, lout, n, out_base)


@pytest.mark.parametrize("W,H", [(200, 120), (98, 62)])
@pytest.mark.parametrize("lin,lout", [("aligned", "aligned"), ("odd", "odd"), ("pushed", "pushed"), ("loose", "loose"),
                                      ("aligned", "odd"), ("pushed", "aligned"), ("tight", "loose")])
def test_i420_pitched_surfaces(W, H, lin, lout):
    """Against the tight run: the gathered samples bitwise, every non-sample
    byte of the output buffer untouched (the first frame's k_copy_rows and the
    fused and unfused composes alike)."""
    import mm355
    n, fmt = 4, mm355.I420
    fr = [f.reshape(-1) for f in _planar(_nv12(W, H, n))]
    want, _ = _go(W, H, [f.reshape(H * 3 // 2, W) for f in fr], fmt, mode="stream")
    want = [w.reshape(-1) for w in want]
    lays = _layouts(W, H, fmt)
    for mode in ("stream", "frame"):
        _same(_pitched(W, H, fr, lays[lin], lays[lout], mode), want, f"{mode} {lin} -> {lout}")
    if lin == "odd":    # frame pointers at odd addresses: the unit is 1
        _same(_pitched(W, H, fr, lays[lin], lays[lout], "stream", in_base=1, out_base=3), want, "odd bases")


def test_fused_kernels_run_where_the_layout_allows():
    """The launch rule: the walking K34 for tight W % 8 == 0 frames and for the
    decoder layout; the unfused pair where a chroma row or a frame pointer is
    odd.  (The bytes are the same: test_i420_pitched_surfaces.)"""
    import torch
    import mm355
    W, H, n, fmt = 200, 120, 9, mm355.I420
    fr = [f.reshape(-1) for f in _planar(_nv12(W, H, n))]
    lays = _layouts(W, H, fmt)
    with _env(MM_K34_ROWS="16"):
        for name, base, fused in (("tight", 0, True), ("aligned", 0, True), ("pushed", 0, False), ("odd", 0, False),
                                  ("tight", 1, False), ("tight", 2, False)):   # (base 2: luma rows at 2 mod 4)
            lay = lays[name]
            a = torch.from_numpy(i420.scatter(W, H, fr, lay, base=base)).cuda()
            b = torch.zeros_like(a)
            h = mm355.Handle(W, H, _params())
            h.set_batch(n)
            h.profile_begin()
            h.process_stream_surfaces(a[base:], lay, b[base:], lay, n)
            prof = h.profile_end()
            h.close()
            assert (prof["k_rows_inv_compose"][1] > 0) == fused, (name, base, prof)
            assert (prof["k_compose"][1] > 0) == (not fused), (name, base, prof)


def test_i420_refusals_leave_the_handle_usable():
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fr = _planar(_nv12(W, H, n))
    want, _ = _go(W, H, fr, mm355.I420, mode="frame", batch=1)
    fb = W * H * 3 // 2

    def code(call):
        with pytest.raises(mm355.MMError) as ei:
            call()
        return ei.value.code

    # a debug view and an odd-sized handle: MM_ERR_UNSUPPORTED
    junk = torch.zeros(2 * fb + 64, dtype=torch.uint8, device="cuda")
    for hw, extra in (((W, H), {"show_phase": 1}), ((97, 63), {})):
        h = mm355.Handle(hw[0], hw[1], mm355.Params.make(levels=L, phase_scale=S, **extra))
        assert code(lambda: h.process(junk, junk.clone(), mm355.I420)) == -2
        assert code(lambda: h.process_stream(junk, junk.clone(), 1, mm355.I420_FULL | mm355.MATRIX_BT709)) == -2
        h.close()
    h = mm355.Handle(W, H, _params())
    dev = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.zeros_like(dev)
    for k in range(2):
        h.process(dev[k], out[k], mm355.I420)
    held = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    after = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.get_state(held)
    ti, tn = mm355.Surface.tight(W, H, mm355.I420), mm355.Surface.tight(W, H, mm355.NV12)
    scratch = junk.clone()
    assert code(lambda: h.process_surface(junk, ti, scratch, tn)) == -1          # one format on both sides
    assert code(lambda: h.process_convert(junk, ti, scratch, tn)) == -2          # no mixed pair with a planar code
    assert code(lambda: h.process_convert(junk, mm355.Surface.tight(W, H, mm355.RGBA8), scratch, ti)) == -2
    short = i420.layout(mm355.I420, ti.pitch, ti.chroma_offset, ti.chroma_pitch, ti.bytes(W, H) - 1)
    assert code(lambda: h.process_stream_surfaces(junk, short, scratch, ti, 2)) == -1   # stride = extent - 1, two frames
    h.process_stream_surfaces(junk, short, scratch, ti, 0)                       # (no frame: nothing to check the stride for)
    for bad in (528 | 128, 528 | 256, 512, 18 | 512):
        assert code(lambda: h.process(junk, scratch, bad)) == -1
    h.get_state(after)
    torch.cuda.synchronize()
    assert torch.equal(held, after), "refused calls leave the state alone"
    assert not scratch.any(), "... and write nothing"
    # a device pointer at an odd address is accepted: the unit is 1
    odd_in = torch.zeros(fb + 1, dtype=torch.uint8, device="cuda")
    odd_out = torch.zeros(fb + 1, dtype=torch.uint8, device="cuda")
    odd_in[1:].copy_(dev[2].reshape(-1))
    assert odd_in[1:].data_ptr() % 2 == 1
    h.process(odd_in[1:], odd_out[1:], mm355.I420)
    h.process(dev[3], out[3], mm355.I420)
    torch.cuda.synchronize()
    h.close()
    assert np.array_equal(odd_out[1:].cpu().numpy().reshape(H * 3 // 2, W), want[2])
    got = out.cpu().numpy()
    for k in (0, 1, 3):
        assert np.array_equal(got[k], want[k]), k


def test_on_render_image_named_format():
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fr = _planar(_nv12(W, H, n, 709))
    fmt = i420.fmt_code(709)
    want, _ = _go(W, H, fr, fmt, mode="frame", batch=1)
    for on_dev in (True, False):
        proc = mm355.MotionMagnificationProcessor(W, H, pyramid_levels=L, phase_scale=S).Start()
        for k in range(n):
            src = torch.from_numpy(fr[k]).cuda() if on_dev else fr[k]
            dst = torch.empty_like(src) if on_dev else np.empty_like(src)
            proc.OnRenderImage(src, dst, fmt=fmt)
            if on_dev:
                torch.cuda.synchronize()
                dst = dst.cpu().numpy()
            assert np.array_equal(dst, want[k]), (on_dev, k)
        proc.OnDestroy()


def _write_y4m(path, W, H, frames):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420\n".encode())
        for b in frames:
            f.write(b"FRAME\n" + b.tobytes())


def _cli(args):
    r = subprocess.run([CLI] + args, capture_output=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return [ln for ln in r.stdout.decode().splitlines() if ln.startswith("frame ")]


def test_cli_i420_writes_the_nv12_file(tmp_path):
    """mm_cli --i420 on a C420 .y4m writes --nv12's file, byte for byte; with
    --surface-align 256,16 the file and the checksums are the same again."""
    import mm355
    W, H, n = 64, 48, 4
    fr = _planar(_nv12(W, H, n))
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, W, H, fr)
    common = ["-i", src, "-l", str(L), "-s", str(S), "-b", "4", "--checksum"]
    a, b, c = (str(tmp_path / f"{x}.y4m") for x in "abc")
    _cli(["--nv12", "-o", a] + common)
    sums = _cli(["--i420", "-o", b] + common)
    sums_al = _cli(["--i420", "-o", c, "--surface-align", "256,16"] + common)
    A = open(a, "rb").read()
    assert len(A) > n * W * H * 3 // 2 and open(b, "rb").read() == A and open(c, "rb").read() == A
    assert len(sums) == n and sums_al == sums
    # ... and the frames in it are the binding's
    want, _ = _go(W, H, fr, mm355.I420, mode="stream")
    body = A.split(b"\n", 1)[1]
    fb = W * H * 3 // 2
    for k in range(n):
        rec = body[k * (6 + fb):(k + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n" and np.array_equal(np.frombuffer(rec[6:], np.uint8), want[k].reshape(-1)), k
    assert not np.array_equal(want[1], fr[1])
    # raw I420 frames under any other extension, with a range and a matrix: the binding's bytes
    raw_in, raw_out = str(tmp_path / "in.yuv"), str(tmp_path / "out.yuv")
    with open(raw_in, "wb") as f:
        for x in fr:
            f.write(x.tobytes())
    _cli(["--i420", "--full-range", "--matrix", "709", "--standard", "-w", str(W), "-h", str(H), "-i", raw_in,
          "-o", raw_out, "-l", str(L), "-s", str(S), "-b", "4"])
    want, _ = _go(W, H, fr, mm355.I420_FULL | mm355.MATRIX_BT709, mode="stream", standard={})
    assert open(raw_out, "rb").read() == b"".join(w.tobytes() for w in want)
