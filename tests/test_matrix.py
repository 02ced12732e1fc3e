"""BT.709 / BT.2020 video frames (MM_MATRIX_BT709 / MM_MATRIX_BT2020 on the
4:2:0 formats) through the C-ABI on the HIP path.

A matrixed frame is the RGBA32F frame of its decode (include/mm.h), so the
reference is the existing oracle on ycbcr.decode(frame, float32), encoded by
ycbcr.encode: tests/ycbcr.py holds the definitions, in float64 numpy.

Bars, the project's own: 8-bit frames mmtest.assert_close_u8 on the whole
buffer (+-1 code on at most 1e-3 of the bytes); 10-bit frames
tests/test_p010.py's per-plane bar (|dword| in {0, 64}, low 6 bits zero, at
most 4e-3 of a plane's words).  The first frame is bitwise the input.

Reference noise under the same comparisons (the fp32 oracle against the float64
twin np_twin.process_frame, both encoded, on the inputs of CASES, measured on
the CPU, worst frame of the worst case, the standard-mode and N = 2048 cases
included):
  8-bit  (cap 1e-3, whole buffer)   <= 1.4e-4 (luma plane 2.0e-4, chroma 2.9e-5), max 1 code
  10-bit (cap 4e-3, per plane)      luma <= 3.3e-4, chroma <= 1.7e-4, max 1 code
every case below a quarter of its cap, so the caps are conditions on the
kernels, not on the reference's own noise.  (The kernels themselves, on the
MI355X: 8-bit <= 4.9e-4 of a plane, 10-bit <= 4.9e-4 of a plane, max 1 code.)

K1 forms reached (the new code: every form reads the chroma plane): frame calls
and short streams take the one-pair (LAT) form; 136 x 520, N = 1024, 260 row
pairs x 5 frames in one launch the batch form with six shared luma rows on four
chroma rows; 136 x 518, 259 pairs (odd: the two groups of a workgroup may lie
in different frames), the regular four-row form.  Compose forms as
tests/test_nv12.py: k_rows_inv_compose4 at 200 x 120, the walking fused kernel
with MM_K34_ROWS, the unfused pair at 64 x 48, 98 x 62 and for one-frame calls
at N = 2048.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmtest as T
import oracle_py as O
import surface as SF
import ycbcr

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
FRAC10 = 4 * T.U8_FRAC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")

# (matrix, full range, depth)
BT709 = (709, False, 8)
BT709_FULL = (709, True, 8)
BT2020_P010 = (2020, False, 10)
BT2020_P010_FULL = (2020, True, 10)


def _run(W, H, frames, *a, **kw):
    """T.gpu_run on frames [H*3/2][W] (uint8, or uint16 moved as their bytes)."""
    wide = frames[0].dtype == np.uint16
    got = T.gpu_run(W, H, [np.ascontiguousarray(f).view(np.uint8) for f in frames], *a, **kw)
    return [np.ascontiguousarray(g).view(np.uint16) if wide else g for g in got]


@functools.lru_cache(maxsize=None)
def _frames(W, H, n, v=BT709, stress=False):
    out = []
    for t, rgb in enumerate(T.synth(W, H, n, fmt="u8")):
        buf = ycbcr.encode(rgb, *v)
        if stress:
            buf = ycbcr.chroma_stress(buf, t, v[2])
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, v=BT709, stress=False, edge=0, std=False):
    """The oracle on the decoded frames, encoded (computed once per case)."""
    fr = [ycbcr.decode(b, np.float32, *v) for b in _frames(W, H, n, v, stress)]
    ref = T.oracle_run(W, H, fr, L, S, edge, standard={} if std else None)
    return tuple(ycbcr.encode(r, *v) for r in ref)


def _bar(got, ref, H, what=""):
    """The bar of the module docstring on one frame."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    fr = []
    for name, sl in (("luma", slice(0, H)), ("chroma", slice(H, None))):
        d = np.abs(got[sl].astype(np.int32) - ref[sl].astype(np.int32))
        fr.append((name, int(d.max()), float((d > 0).mean())))
    print(f"{what}: " + "  ".join(f"{n} max {m} frac {f:.2e}" for n, m, f in fr))
    if got.dtype == np.uint8:
        T.assert_close_u8(got, ref)
        return
    assert not np.any(got & 63), "low 6 bits of every output word are zero"
    for name, m, f in fr:
        assert m in (0, 64), (what, name, m)
        assert f <= FRAC10, (what, name, f)


def _check(got, frames, ref):
    assert np.array_equal(got[0], frames[0]), "first frame passes through bitwise"
    H = frames[0].shape[0] * 2 // 3
    sh = 6 if frames[0].dtype == np.uint16 else 0
    for k in range(1, len(frames)):
        _bar(got[k], ref[k], H, f"frame {k}")
        # not a passthrough nor a chroma copy: the operator moved both planes
        assert ((got[k][:H] >> sh) != (frames[k][:H] >> sh)).mean() > 0.5
        assert ((got[k][H:] >> sh) != (frames[k][H:] >> sh)).mean() > 0.3


# W, H, frames, (matrix, range, depth), chroma stress, edge, MM_K34_ROWS of the stream leg
CASES = [
    (64, 48, 4, BT709, False, 0, None),              # K1 one-pair form; x0 = 0: unfused K3 -> K4
    (200, 120, 4, BT709, False, 0, None),            # N = 256: k_rows_inv_compose4
    (200, 120, 4, BT709_FULL, True, 0, None),
    (200, 120, 4, BT2020_P010, True, 0, None),
    (200, 120, 4, BT2020_P010_FULL, False, 0, None),
    (200, 120, 4, (2020, False, 8), True, 0, None),  # 8-bit BT.2020 is allowed
    (200, 120, 12, BT709, False, 0, "64"),           # the walking fused K34, full strips, N = 256
    (98, 62, 4, BT709, False, 0, None),              # W % 8 != 0: unfused; chroma rows of 49 pairs; NV12 frame
                                                     # stride 9,114 and row stride 98: not multiples of 4
    (128, 128, 4, BT709, True, 0, None),             # N = W = H: every border row wraps, then halves ...
    (128, 128, 4, BT709, True, 1, None),             # ... or clamps, onto the chroma plane
    (128, 128, 4, BT2020_P010, True, 0, None),
    (128, 128, 4, BT2020_P010, True, 1, None),
    (136, 520, 5, BT709, True, 0, None),             # N = 1024, 5 x 260 pairs in one launch: K1 batch form
    (136, 520, 5, BT2020_P010, True, 1, None),
    (136, 518, 5, BT709, True, 0, None),             # 259 pairs per frame: K1 regular four-row form
    (136, 518, 5, BT2020_P010, True, 1, None),
]


@pytest.mark.parametrize("W,H,n,v,stress,edge,rows", CASES)
def test_matrix_vs_oracle(W, H, n, v, stress, edge, rows):
    fmt = ycbcr.fmt_code(*v)
    fr, ref = _frames(W, H, n, v, stress), _ref(W, H, n, v, stress, edge)
    got = _run(W, H, fr, L, S, edge, mode="frame", batch=1, fmt=fmt)
    _check(got, fr, ref)
    with SF.env(MM_K34_ROWS=rows):
        got = _run(W, H, fr, L, S, edge, mode="stream", batch=12 if rows else 8, fmt=fmt)
    _check(got, fr, ref)


@pytest.mark.parametrize("v", [BT709, BT2020_P010])
def test_matrix_n2048_vs_oracle(v):
    """The N = 2048 instances at 1920 x 128: one-frame calls (unfused K3 -> K4
    there) and a stream through the walking K34, two 64-row strips."""
    W, H, n = 1920, 128, 3
    O.set_threads(16)
    fmt = ycbcr.fmt_code(*v)
    fr, ref = _frames(W, H, n, v), _ref(W, H, n, v)
    got = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
    _check(got, fr, ref)
    with SF.env(MM_K34_ROWS="64"):
        got = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
    _check(got, fr, ref)


@pytest.mark.parametrize("v", [BT709, BT2020_P010])
def test_matrix_is_not_the_bt601_reading(v):
    """What makes the suite meaningful: the same bytes read as BT.601 give
    another picture and another state, far outside the bars above."""
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fmt = ycbcr.fmt_code(*v)
    fr = _frames(W, H, n, v, True)
    got = _run(W, H, fr, L, S, mode="stream", fmt=fmt)
    as601 = _run(W, H, fr, L, S, mode="stream", fmt=mm355.base_format(fmt))
    for k in range(1, n):
        frac = (got[k][:H] != as601[k][:H]).mean()
        print(f"frame {k}: luma samples that differ from the BT.601 reading {frac:.3f}")
        assert frac > 0.5
    # the state is the state of the decoded frame: K1's luma is RGBToYIQ's of the decode
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    dev = torch.from_numpy(np.array(fr[n - 1]).view(np.uint8)).cuda()
    f32 = torch.from_numpy(ycbcr.decode(fr[n - 1], np.float32, *v)).cuda()
    st = [torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda") for _ in range(3)]
    h.compute_state(dev, fmt, st[0])
    h.compute_state(f32, mm355.RGBA32F, st[1])
    h.compute_state(dev, mm355.base_format(fmt), st[2])
    torch.cuda.synchronize()
    a, b, c = (T.state_rows(s, h.N, H) for s in st)
    h.close()
    bar = 1e-5 * np.abs(b).max()
    print(f"state: |matrixed - decoded| {np.abs(a - b).max():.3e}  bar {bar:.3e}  "
          f"|matrixed - BT.601| {np.abs(a - c).max():.3e}")
    assert np.abs(a - b).max() <= bar
    assert np.abs(a - c).max() > 100 * bar


def test_matrix_neutral_chroma_is_the_luma_plane():
    """Neutral chroma adds exactly zero to K1's luma: the state of a grey
    BT.709 / BT.2020 frame is bitwise the state of the same bytes as BT.601."""
    import torch
    import mm355
    W, H = 200, 120
    for v in (BT709, BT2020_P010_FULL):
        fmt = ycbcr.fmt_code(*v)
        buf = _frames(W, H, 2, v)[1].copy()
        buf[H:] = 128 if v[2] == 8 else 0x8000
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
        dev = torch.from_numpy(buf.view(np.uint8)).cuda()
        st = [torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
        h.compute_state(dev, fmt, st[0])
        h.compute_state(dev, mm355.base_format(fmt), st[1])
        torch.cuda.synchronize()
        h.close()
        assert torch.equal(st[0], st[1]) and bool(st[0].any())


def test_matrix_call_forms_agree_bytewise():
    """A stream call, frame calls and host-pointer calls give the same bytes;
    so do the three compose forms (walking K34, one-shot K34, unfused K3 -> K4)
    and K1's three load forms (one-pair in frame calls; batch and regular form
    in the 5-frame streams at N = 1024)."""
    W, H, n = 200, 120, 4
    for v, stress in ((BT709_FULL, True), (BT2020_P010, True)):
        fr = _frames(W, H, n, v, stress)
        fmt = ycbcr.fmt_code(*v)
        a = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
        for what, kw, env in (("stream", dict(mode="stream", batch=8), {}),
                              ("host", dict(mode="host"), {}),
                              ("walking K34", dict(mode="stream", batch=8), {"MM_K34_ROWS": "16"}),
                              ("unfused", dict(mode="stream", batch=8), {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"})):
            with SF.env(**env):
                b = _run(W, H, fr, L, S, fmt=fmt, **kw)
            for k in range(n):
                assert np.array_equal(a[k], b[k]), (what, v, k, int((a[k] != b[k]).sum()))
    for (W, H), v in (((136, 520), BT709), ((136, 518), BT2020_P010)):
        fr = _frames(W, H, 5, v, True)
        fmt = ycbcr.fmt_code(*v)
        a = _run(W, H, fr, L, S, mode="frame", batch=1, fmt=fmt)
        b = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)
        for k in range(5):
            assert np.array_equal(a[k], b[k]), ("K1 forms", W, H, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("v,name", [(BT709, "nv12"), (BT2020_P010, "p010")])
def test_matrix_decoder_surfaces(v, name):
    """Input and output in mm_surface_aligned(256, 16) layout (K1's first use of
    the chroma offset and pitch), all padding poisoned, with two different
    bytes: the samples are bitwise the tight run's and no padding byte is
    written (nor read: the two runs agree)."""
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fmt = ycbcr.fmt_code(*v)
    fr = _frames(W, H, n, v, True)
    flat = [np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in fr]
    want = [np.ascontiguousarray(g).view(np.uint8).reshape(-1)
            for g in _run(W, H, fr, L, S, mode="stream", batch=8, fmt=fmt)]
    lay = mm355.Surface.aligned(W, H, fmt, 256, 16)
    assert lay.format == fmt and lay.pitch == (256 if name == "nv12" else 512) and lay.chroma_offset == lay.pitch * 128
    size = SF.buffer_bytes(name, W, H, lay, n)
    keep = ~SF.sample_mask(name, W, H, lay, n, size)
    for mode in ("stream", "frame"):
        for poison in (0xFF, 0x3C):
            src = SF.scatter(name, W, H, flat, lay, fill=poison, size=size)
            h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
            h.set_batch(8)
            a = torch.from_numpy(src).cuda()
            b = torch.full((size,), poison ^ 0x55, dtype=torch.uint8, device="cuda")
            if mode == "stream":
                h.process_stream_surfaces(a, lay, b, lay, n)
            else:
                for k in range(n):
                    h.process_surface(a[k * lay.frame_stride:], lay, b[k * lay.frame_stride:], lay)
            torch.cuda.synchronize()
            res = b.cpu().numpy()
            h.close()
            assert np.all(res[keep] == (poison ^ 0x55)), "output padding is untouched"
            SF.assert_same(SF.gather(name, W, H, res, lay, n), want, (name, mode, hex(poison)))


def test_matrix_standard_mode_vs_oracle():
    W, H, n = 96, 64, 4
    for v in (BT709, BT2020_P010):
        fr, ref = _frames(W, H, n, v), _ref(W, H, n, v, std=True)
        for mode, batch in (("frame", 1), ("stream", 8)):
            got = _run(W, H, fr, L, S, mode=mode, batch=batch, standard={}, fmt=ycbcr.fmt_code(*v))
            _check(got, fr, ref)


@pytest.mark.parametrize("v", [BT709, BT2020_P010])
def test_matrix_steerable_equals_f32_path_encoded(v):
    """Steerable (O = 4, DIFF): the matrixed output against encode() of the
    GPU's own RGBA32F output on the decoded frames (that path is held to
    oracle/steerable_ref.py), at the format's bar."""
    W, H, n = 256, 192, 4
    extra = {"mode": 2, "orientations": 4}
    fr = _frames(W, H, n, v)
    f32 = T.gpu_run(W, H, [ycbcr.decode(b, np.float32, *v) for b in fr], L, S, mode="stream", extra=extra)
    got = _run(W, H, fr, L, S, mode="stream", extra=extra, fmt=ycbcr.fmt_code(*v))
    _check(got, fr, [ycbcr.encode(f, *v) for f in f32])


def test_matrix_passthrough():
    W, H, n = 200, 120, 3
    for v in (BT709, BT2020_P010_FULL):
        fr = _frames(W, H, n, v, True)
        got = _run(W, H, fr, L, S, mode="stream", apply=False, fmt=ycbcr.fmt_code(*v))
        for k in range(n):
            assert np.array_equal(got[k], fr[k])


def test_matrix_refusals_leave_the_handle_usable():
    """A matrix bit on RGBA8 (invalid) and show_phase with a matrixed format
    (unsupported) are refused before anything is queued: the BT.709 stream
    around them continues bitwise as if they had never been made."""
    import torch
    import mm355
    W, H, n = 64, 48, 4
    fmt = mm355.NV12 | mm355.MATRIX_BT709
    fr = _frames(W, H, n)
    want = _run(W, H, fr, L, S, mode="frame", batch=64, fmt=fmt)
    p = mm355.Params.make(levels=L, phase_scale=S)
    h = mm355.Handle(W, H, p)
    dev = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.zeros_like(dev)
    junk = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    for k in range(2):
        h.process(dev[k], out[k], fmt)
    for bad in (mm355.RGBA8 | mm355.MATRIX_BT709, fmt | mm355.MATRIX_BT2020, fmt | 128):
        for call in (lambda: h.process(junk, junk.clone(), bad),
                     lambda: h.process_stream(junk, junk.clone(), 1, bad),
                     lambda: h.compute_state(junk, bad, junk.clone()),
                     lambda: h.process(np.zeros(W * H * 4, np.uint8), np.zeros(W * H * 4, np.uint8), bad,
                                       on_device=False)):
            with pytest.raises(mm355.MMError) as ei:
                call()
            assert ei.value.code == -1                       # MM_ERR_INVALID
    h.process(dev[2], out[2], fmt)
    h.set_params(mm355.Params.make(levels=L, phase_scale=S, show_phase=1))
    for call in (lambda: h.process(dev[3], out[3], fmt),
                 lambda: h.process_stream(dev[3], out[3], 1, fmt)):
        with pytest.raises(mm355.MMError) as ei:
            call()
        assert ei.value.code == -2                           # MM_ERR_UNSUPPORTED
    h.set_params(p)
    h.process(dev[3], out[3], fmt)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    h.close()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k


def test_cli_matrix_matches_binding(tmp_path):
    """mm_cli --nv12 --matrix 709 on a 4:2:0 clip writes a C420 file whose
    planes, re-interleaved, are the binding's NV12 | BT709 output on the same
    bytes (and not its BT.601 output); --matrix without --nv12 / --p010 is a
    usage error."""
    import mm355
    W, H, n = 64, 48, 4
    fr = _frames(W, H, n, BT709, True)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with open(src, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420\n".encode())
        for b in fr:
            c = b[H:].reshape(H // 2, W // 2, 2)
            f.write(b"FRAME\n" + b[:H].tobytes() + np.ascontiguousarray(c[..., 0]).tobytes() +
                    np.ascontiguousarray(c[..., 1]).tobytes())
    subprocess.check_call([CLI, "--nv12", "--matrix", "709", "-i", src, "-o", dst, "-l", str(L), "-s", str(S),
                           "-b", "4"], timeout=120)
    raw = open(dst, "rb").read()
    head, body = raw.split(b"\n", 1)
    assert head.startswith(b"YUV4MPEG2") and b"C420" in head and f"W{W} H{H}".encode() in head
    fb = W * H * 3 // 2
    assert len(body) == n * (6 + fb)
    want = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=mm355.NV12 | mm355.MATRIX_BT709)
    as601 = _run(W, H, fr, L, S, mode="stream", batch=8, fmt=mm355.NV12)
    for k in range(n):
        rec = body[k * (6 + fb):(k + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n"
        p = np.frombuffer(rec[6:], np.uint8)
        got = np.empty((H * 3 // 2, W), np.uint8)
        got[:H] = p[:W * H].reshape(H, W)
        got[H:, 0::2] = p[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
        got[H:, 1::2] = p[W * H * 5 // 4:].reshape(H // 2, W // 2)
        assert np.array_equal(got, want[k]), k
        assert k == 0 or not np.array_equal(got, as601[k])
    # --matrix goes with --nv12 or --p010 only, and takes 601, 709 or 2020
    for args in (["--matrix", "709", "-i", src], ["--srgb", "--matrix", "2020", "-i", src],
                 ["--matrix", "709", "-w", "64", "-h", "48", "-n", "2"],
                 ["--nv12", "--matrix", "240", "-i", src]):
        r = subprocess.run([CLI, "-o", dst, "-b", "4"] + args, capture_output=True, timeout=120)
        assert r.returncode == 2 and b"--matrix" in r.stderr, (args, r.returncode, r.stderr)
