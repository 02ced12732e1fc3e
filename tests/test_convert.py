"""Frames that go in as one format and come out as another, through
mm_process_convert / mm_process_stream_convert on the HIP path: NV12 / P010
codes in with RGBA8 out, RGBA8 in with an NV12 code out (include/mm.h
"Different formats in and out").  tests/convert.py holds the definitions.

Reference: mmtest.oracle_run on the in rule's float32 frames, stored by the out
rule; the first frame (and apply_magnification = 0) against the plain
conversion.  Bar: the project's 8-bit bar, mmtest.assert_close_u8 (+-1 code on
at most 0.1 % of bytes), on the WHOLE output buffer.

The cap is a condition on the kernels: under the same comparison the fp32
oracle differs from the float64 twin (np_twin.process_frame, stored by the same
out rule) by at most these shares of the bytes, never by more than 1 code,
measured on the CPU on exactly the inputs below (L = 5, S = 25, frames 1 .. n-1):
  decode (in > RGBA8)                     encode (RGBA8 > out)
  NV12 64x48        8.1e-5                NV12 64x48        0
  NV12 200x120      3.1e-5                NV12 200x120      2.8e-5
  NV12 98x62        8.2e-5                NV12 98x62        0
  NV12 128x128      1.5e-5 (both edges)   NV12 128x128      4.1e-5 (both edges)
  NV12 1920x128     8.2e-5                NV12 1920x128     7.6e-5
  NV12 256x192      2.0e-5                NV12 256x192      4.1e-5
  NV12_FULL         2.1e-5                NV12_FULL         0
  NV12|BT709        3.1e-5                NV12|BT709        2.8e-5
  P010|BT2020       3.1e-5
  P010, low bits    2.1e-5
  NV12 stress       4.2e-5
  P010 stress       6.3e-5
  standard 128x96   4.1e-5                standard 128x96   5.4e-5
Standard mode at 96x64, 160x96 and 200x120 left the reference alone above 1e-4
(1.2e-4 / 2.2e-4 at 96x64), so that case runs at 128x96.

Kernels reached: 64x48 has x0 = 0 (unfused K3 -> k_compose, K1's one-pair
form); 200x120 one-frame calls k_rows_inv_compose4 at N = 256, and with
MM_K34_ROWS=64 over 12 frames the walking k_rows_inv_compose; 98x62 has
W % 8 != 0 and NV12 rows and frames that are no multiples of 4 (unfused, and
k_convert's single-sample form); 128x128 has no margins; 1920x128 runs the
N = 2048 instances.  The first frame of every run is k_convert.  The encode
pair's walking K34 has two instances, source rows staged by LDS-DMA (16-byte
aligned rows: every tight RGBA8 frame here) and register loads.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import convert as C
import mmtest as T
import surface as SF

pytestmark = pytest.mark.gpu

L, S = 5, 25.0
NV12, NV12_FULL, P010, RGBA8, BT709, BT2020 = 16, 17, 18, 0, 32, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "bin", "mm_cli")
DIRS = [(NV12, RGBA8), (RGBA8, NV12)]


@functools.lru_cache(maxsize=None)
def _frames(W, H, n, fmt, stress=False, low_bits=False):
    fr = C.frames(W, H, n, fmt, stress=stress, low_bits=low_bits)
    for f in fr:
        f.setflags(write=False)
    return tuple(fr)


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, fi, fo, edge=0, std=False, stress=False, low_bits=False):
    ref = C.reference(W, H, list(_frames(W, H, n, fi, stress, low_bits)), fi, fo, L, S, edge,
                      standard={} if std else None)
    for r in ref:
        r.setflags(write=False)
    return tuple(ref)


def _check(got, fr, ref, fi, fo, what=""):
    """Every frame at the bar (frame 0: the plain conversion); after the first,
    the operator ran: more than half of the bytes differ from the plain conversion."""
    assert len(got) == len(ref)
    for k in range(len(ref)):
        d = np.abs(got[k].astype(np.int32) - ref[k].astype(np.int32))
        print(f"{what} frame {k}: max {d.max()}  share {(d > 0).mean():.2e}")
        T.assert_close_u8(got[k], ref[k])
        if k:
            moved = got[k] != C.plain(fr[k], fi, fo)
            if fo == RGBA8:
                moved = moved[..., :3]
            assert moved.mean() > 0.5, (what, k, moved.mean())


# W, H, frames, edge, MM_K34_ROWS of the stream leg
SHAPES = [
    (64, 48, 4, 0, None),
    (200, 120, 4, 0, None),
    (200, 120, 12, 0, "64"),
    (98, 62, 4, 0, None),
    (128, 128, 4, 0, None),
    (128, 128, 4, 1, None),
    (1920, 128, 3, 0, None),
]


@pytest.mark.parametrize("fi,fo", DIRS)
@pytest.mark.parametrize("W,H,n,edge,rows", SHAPES)
def test_convert_vs_oracle(W, H, n, edge, rows, fi, fo):
    fr, ref = list(_frames(W, H, n, fi)), _ref(W, H, n, fi, fo, edge)
    got = C.run(W, H, fr, fi, fo, L, S, edge, mode="frame", batch=1)
    _check(got, fr, ref, fi, fo, "single calls")
    with SF.env(MM_K34_ROWS=rows):
        got = C.run(W, H, fr, fi, fo, L, S, edge, mode="stream", batch=12 if rows else 8)
    _check(got, fr, ref, fi, fo, "stream")


VARIANTS = [
    (NV12_FULL, RGBA8, False, False),
    (NV12 | BT709, RGBA8, False, False),
    (P010 | BT2020, RGBA8, False, False),
    (P010, RGBA8, False, True),          # P016 content: the low 6 bits count
    (NV12, RGBA8, True, False),          # chroma stress: far out of gamut, the store saturates
    (P010, RGBA8, True, False),
    (RGBA8, NV12 | BT709, False, False),
    (RGBA8, NV12_FULL, False, False),
]


@pytest.mark.parametrize("fi,fo,stress,low_bits", VARIANTS)
def test_convert_variants_vs_oracle(fi, fo, stress, low_bits):
    W, H, n = 200, 120, 4
    fr = list(_frames(W, H, n, fi, stress, low_bits))
    ref = _ref(W, H, n, fi, fo, 0, False, stress, low_bits)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _check(C.run(W, H, fr, fi, fo, L, S, mode=mode, batch=batch), fr, ref, fi, fo, mode)


def test_p010_low_bits_reach_the_output():
    """The words' low bits are honoured: the same frames with the low 6 bits
    cleared give other RGBA8 bytes (the plain conversion already does)."""
    W, H, n = 200, 120, 2
    fr = list(_frames(W, H, n, P010, False, True))
    a = C.run(W, H, fr, P010, RGBA8, L, S, mode="stream")
    b = C.run(W, H, [f & 0xFFC0 for f in fr], P010, RGBA8, L, S, mode="stream")
    assert (a[0] != b[0]).mean() > 0.01 and (a[1] != b[1]).mean() > 0.01


@pytest.mark.parametrize("fi,fo", DIRS)
def test_convert_standard_mode_vs_oracle(fi, fo):
    W, H, n = 128, 96, 4     # (96 x 64: the reference alone exceeds 1e-4 there, see above)
    fr, ref = list(_frames(W, H, n, fi)), _ref(W, H, n, fi, fo, 0, True)
    for mode, batch in (("frame", 1), ("stream", 8)):
        _check(C.run(W, H, fr, fi, fo, L, S, mode=mode, batch=batch, standard={}), fr, ref, fi, fo, mode)


@pytest.mark.parametrize("fi,fo", DIRS)
def test_convert_steerable_equals_f32_path_stored(fi, fo):
    """Steerable (O = 4, DIFF), which reaches the unfused compose through
    launch_k4: against the GPU's own RGBA32F output on the in rule's frames
    (that path is held to oracle/steerable_ref.py), stored by the out rule."""
    W, H, n = 256, 192, 4
    extra = {"mode": 2, "orientations": 4}
    fr = list(_frames(W, H, n, fi))
    f32 = T.gpu_run(W, H, [C.to_rgba(f, fi, np.float32) for f in fr], L, S, mode="stream", extra=extra)
    ref = [C.plain(fr[0], fi, fo)] + [C.store(f, fo) for f in f32[1:]]
    got = C.run(W, H, fr, fi, fo, L, S, mode="stream", extra=extra)
    _check(got, fr, ref, fi, fo, "steerable")


@pytest.mark.parametrize("fi,fo", DIRS + [(P010 | BT709, RGBA8), (RGBA8, NV12_FULL | BT2020)])
@pytest.mark.parametrize("W,H", [(200, 120), (98, 62)])
def test_first_frame_and_apply_off_are_the_plain_conversion(W, H, fi, fo):
    n = 3
    fr = list(_frames(W, H, n, fi))
    want = [C.plain(f, fi, fo) for f in fr]
    for mode in ("frame", "stream", "host"):
        got = C.run(W, H, fr, fi, fo, L, S, mode=mode, apply=False)
        for k in range(n):
            T.assert_close_u8(got[k], want[k])
    T.assert_close_u8(C.run(W, H, fr[:1], fi, fo, L, S, mode="frame")[0], want[0])


@pytest.mark.parametrize("fi,fo", DIRS + [(P010, RGBA8)])
def test_state_is_the_same_format_calls(fi, fo):
    """mm_get_state after convert calls is bitwise the state after the
    same-format calls on the in format's frames (K1 has no out side), and
    mm_compute_state_surface gives it too."""
    import torch
    import mm355
    W, H, n = 200, 120, 3
    fr = list(_frames(W, H, n, fi))
    li, lo = mm355.Surface.tight(W, H, fi), mm355.Surface.tight(W, H, fo)
    src = torch.from_numpy(np.ascontiguousarray(np.stack(fr)).view(np.uint8)).cuda()
    states = []
    for convert in (True, False):
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
        out = torch.from_numpy(C.out_frames(n, W, H, fo if convert else fi).view(np.uint8)).cuda()
        for k in range(n):
            if convert:
                h.process_convert(src[k], li, out[k], lo)
            else:
                h.process(src[k], out[k], fi)
        st = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(st)
        made = torch.ones(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.compute_state_surface(src[n - 1], li, made)
        torch.cuda.synchronize()
        assert torch.equal(st, made)
        states.append(st.cpu())
        h.close()
    assert torch.equal(states[0], states[1])


@pytest.mark.parametrize("fi,fo", DIRS + [(P010, RGBA8)])
def test_call_forms_agree_bytewise(fi, fo):
    W, H, n = 200, 120, 4
    fr = list(_frames(W, H, n, fi))
    a = C.run(W, H, fr, fi, fo, L, S, mode="frame", batch=1)
    for what, kw, env in (("stream, batch 1", dict(mode="stream", batch=1), {}),
                          ("stream, batch 8", dict(mode="stream", batch=8), {}),
                          ("host", dict(mode="host"), {}),
                          ("walking K34", dict(mode="stream", batch=8), {"MM_K34_ROWS": "16"}),
                          ("unfused", dict(mode="stream", batch=8), {"MM_K34_ROWS": "0", "MM_K34_ONESHOT": "0"})):
        with SF.env(**env):
            b = C.run(W, H, fr, fi, fo, L, S, **kw)
        for k in range(n):
            assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def test_one_handle_alternates_call_kinds():
    """Same-format NV12 call, convert call, same-format call on ONE handle: each
    output equals that of a handle of its own fed the same prefix."""
    import torch
    import mm355
    W, H, n = 200, 120, 4
    fr = list(_frames(W, H, n, NV12))
    same = T.gpu_run(W, H, fr, L, S, mode="frame", batch=1, fmt=NV12)
    conv = C.run(W, H, fr, NV12, RGBA8, L, S, mode="frame", batch=1)
    li, lo = mm355.Surface.tight(W, H, NV12), mm355.Surface.tight(W, H, RGBA8)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    src = torch.from_numpy(np.stack(fr)).cuda()
    o_nv = torch.zeros_like(src)
    o_rgba = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda")
    h.process(src[0], o_nv[0], NV12)
    h.process_convert(src[1], li, o_rgba[1], lo)
    h.process(src[2], o_nv[2], NV12)
    h.process_convert(src[3], li, o_rgba[3], lo)
    torch.cuda.synchronize()
    h.close()
    assert np.array_equal(o_nv[0].cpu().numpy(), same[0]) and np.array_equal(o_nv[2].cpu().numpy(), same[2])
    assert np.array_equal(o_rgba[1].cpu().numpy(), conv[1]) and np.array_equal(o_rgba[3].cpu().numpy(), conv[3])


def _name(fmt):
    return "rgba8" if fmt == RGBA8 else "nv12"


def _run_pitched(W, H, fr, fi, fo, lin, lout, mode, in_base=0, out_base=0, in_size=None, out_size=None):
    """surface.run_pitched for the convert entry points: the input scattered
    into a poisoned buffer, the output buffer a sentinel pattern; asserts that
    no byte of the destination that is no sample was written."""
    import torch
    import mm355
    ni, no, n = _name(fi), _name(fo), len(fr)
    flat = [np.ascontiguousarray(f).reshape(-1) for f in fr]
    src = SF.scatter(ni, W, H, flat, lin, in_base, size=in_size)
    out_size = out_size or SF.buffer_bytes(no, W, H, lout, n, out_base)
    sent = SF.sentinel(out_size)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    h.set_batch(8)
    a, b = torch.from_numpy(src).cuda(), torch.from_numpy(sent).cuda()
    if mode == "stream":
        h.process_stream_convert(a[in_base:], lin, b[out_base:], lout, n)
    else:
        for k in range(n):
            h.process_convert(a[in_base + k * lin.frame_stride:], lin, b[out_base + k * lout.frame_stride:], lout)
    torch.cuda.synchronize()
    res = b.cpu().numpy()
    h.close()
    keep = ~SF.sample_mask(no, W, H, lout, n, out_size, out_base)
    bad = np.flatnonzero(keep & (res != sent))
    assert bad.size == 0, f"{bad.size} padding bytes written, first at {bad[:8]}"
    return SF.gather(no, W, H, res, lout, n, out_base)


@pytest.mark.parametrize("mode", ["frame", "stream"])
def test_surfaces_give_the_tight_runs_samples(mode):
    import mm355
    W, H, n = 200, 120, 4
    # a decoder's NV12 layout in, tight RGBA8 out
    fr = list(_frames(W, H, n, NV12))
    tight = [g.reshape(-1) for g in C.run(W, H, fr, NV12, RGBA8, L, S, mode="stream")]
    got = _run_pitched(W, H, fr, NV12, RGBA8, mm355.Surface.aligned(W, H, NV12, 256, 16),
                       mm355.Surface.tight(W, H, RGBA8), mode)
    SF.assert_same(got, tight, "decoder layout in")
    # ... and a pitched RGBA8 destination (a pitch of row bytes + 4: quads at dword-aligned addresses only)
    got = _run_pitched(W, H, fr, NV12, RGBA8, mm355.Surface.tight(W, H, NV12), SF.lay_plus_unit("rgba8", W, H), mode)
    SF.assert_same(got, tight, "pitched RGBA8 out")
    # tight RGBA8 in, an NV12 region of interest of a larger frame out
    fr = list(_frames(W, H, n, RGBA8))
    tight = [g.reshape(-1) for g in C.run(W, H, fr, RGBA8, NV12, L, S, mode="stream")]
    lay, base, size = SF.lay_roi("nv12", W, H, 320, 200, 36, 18)
    got = _run_pitched(W, H, fr, RGBA8, NV12, mm355.Surface.tight(W, H, RGBA8), lay, mode, out_base=base,
                       out_size=base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + SF.TAIL)
    SF.assert_same(got, tight, "NV12 region of interest out")
    # ... at a column that is 2 mod 4: the output's rows fail the quads' alignment (unfused, single samples)
    lay, base, size = SF.lay_roi("nv12", W, H, 320, 200, 38, 18)
    got = _run_pitched(W, H, fr, RGBA8, NV12, mm355.Surface.tight(W, H, RGBA8), lay, mode, out_base=base,
                       out_size=base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + SF.TAIL)
    SF.assert_same(got, tight, "NV12 region of interest at 2 mod 4")


def test_nv12_rows_at_2_mod_4_take_the_unfused_path():
    """An NV12 input whose rows are 2 mod 4 apart (pitch W + 2) gives the bytes
    of the same frames in an aligned buffer."""
    W, H, n = 200, 120, 4
    fr = list(_frames(W, H, n, NV12))
    import mm355
    tight = [g.reshape(-1) for g in C.run(W, H, fr, NV12, RGBA8, L, S, mode="stream")]
    for mode in ("frame", "stream"):
        got = _run_pitched(W, H, fr, NV12, RGBA8, SF.lay_plus_unit("nv12", W, H), mm355.Surface.tight(W, H, RGBA8), mode)
        SF.assert_same(got, tight, mode)


def test_encode_walking_k34_staged_and_register_loads_agree():
    """RGBA8 in, NV12 out through the walking K34 (MM_K34_ROWS=16): tight source
    rows are 16-byte aligned and go to LDS by DMA (the staged instance); a pitch
    of row bytes + 4 keeps the register loads.  Both give the unfused pair's bytes."""
    import mm355
    W, H, n = 200, 120, 4
    fr = list(_frames(W, H, n, RGBA8))
    with SF.env(MM_K34_ROWS="0", MM_K34_ONESHOT="0"):
        want = [g.reshape(-1) for g in C.run(W, H, fr, RGBA8, NV12, L, S, mode="stream")]
    with SF.env(MM_K34_ROWS="16"):
        for lin in (mm355.Surface.tight(W, H, RGBA8), SF.lay_plus_unit("rgba8", W, H)):
            got = _run_pitched(W, H, fr, RGBA8, NV12, lin, mm355.Surface.tight(W, H, NV12), "stream")
            SF.assert_same(got, want, f"pitch {lin.pitch}")


def test_refusals_leave_the_next_output_unchanged():
    import torch
    import mm355

    def code(call):
        with pytest.raises(mm355.MMError) as ei:
            call()
        return ei.value.code

    W, H, n = 200, 120, 3
    fr = list(_frames(W, H, n, NV12))
    want = C.run(W, H, fr, NV12, RGBA8, L, S, mode="frame", batch=1)
    li, lo = mm355.Surface.tight(W, H, NV12), mm355.Surface.tight(W, H, RGBA8)
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S))
    src = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda")
    junk = torch.zeros(W * H * 16 + 64, dtype=torch.uint8, device="cuda")
    for k in range(2):
        h.process_convert(src[k], li, out[k], lo)
    # an unsupported pair; an unknown code; differing formats through the old entry points
    assert code(lambda: h.process_convert(src[2], li, junk, mm355.Surface.tight(W, H, mm355.RGBA32F))) == -2
    assert code(lambda: h.process_stream_convert(junk, lo, junk, mm355.Surface.tight(W, H, P010), 1)) == -2
    bad = mm355.Surface.tight(W, H, RGBA8)
    bad.format = 20
    assert code(lambda: h.process_convert(src[2], li, junk, bad)) == -1
    assert code(lambda: h.process_surface(src[2], li, junk, lo)) == -1
    assert code(lambda: h.process_stream_surfaces(src[2], li, junk, lo, 1)) == -1
    assert code(lambda: h.process_stream_convert(src[2], li, junk, lo, -1)) == -1
    # each layout by its own format's rules: a misaligned device pointer on either side
    assert code(lambda: h.process_convert(src.view(-1)[1:], li, junk, lo)) == -1       # NV12: unit 2
    assert code(lambda: h.process_convert(src[2], li, junk[2:], lo)) == -1             # RGBA8: unit 4
    short = mm355.Surface.tight(W, H, RGBA8)
    short.pitch = 4 * W - 4
    assert code(lambda: h.process_convert(src[2], li, junk, short)) == -1
    h.process_convert(src[2], li, out[2], lo)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    h.close()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k
    # a debug view and odd sizes: MM_ERR_UNSUPPORTED, the union of both formats' restrictions
    h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S, show_phase=1))
    assert code(lambda: h.process_convert(src[0], li, junk, lo)) == -2
    assert code(lambda: h.process_convert(junk, lo, junk, li)) == -2
    h.close()
    h = mm355.Handle(97, 63, mm355.Params.make(levels=L, phase_scale=S))
    rg = mm355.Surface.tight(97, 63, RGBA8)
    nv = mm355.Surface.tight(98, 64, NV12)      # (no NV12 layout exists for an odd size)
    assert code(lambda: h.process_convert(junk, rg, junk, nv)) == -2
    assert code(lambda: h.process_convert(junk, nv, junk, rg)) == -2
    # ... and the handle still runs its own format
    rgba = T.synth(97, 63, 2, fmt="u8")
    a = torch.from_numpy(np.stack(rgba)).cuda()
    b = torch.zeros_like(a)
    for k in range(2):
        h.process(a[k], b[k], RGBA8)
    torch.cuda.synchronize()
    h.close()
    assert np.array_equal(b[0].cpu().numpy(), rgba[0])


def _write_y4m(path, W, H, fr):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420\n".encode())
        for b in fr:
            c = b[H:].reshape(H // 2, W // 2, 2)
            f.write(b"FRAME\n" + b[:H].tobytes() + np.ascontiguousarray(c[..., 0]).tobytes() +
                    np.ascontiguousarray(c[..., 1]).tobytes())


def _cli_hashes(args):
    out = subprocess.run([CLI] + args, capture_output=True, timeout=120, check=True).stdout.decode()
    return [line.split()[2] for line in out.splitlines() if line.startswith("frame ")]


def _fnv(frame):
    """mm_cli's frame hash: 64-bit FNV-1a over the frame's 8-byte words."""
    b = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
    w = np.frombuffer(b[:b.size // 8 * 8].tobytes(), "<u8")
    hsh = 0xcbf29ce484222325
    for v in w.tolist():
        hsh = ((hsh ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    for v in b[b.size // 8 * 8:].tolist():
        hsh = ((hsh ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return str(hsh)


def _y4m_rgba(path, n):
    """The RGBA8 frames host/y4m.c expands a C420 file to, as BT.601 limited range."""
    import ctypes

    class Info(ctypes.Structure):
        _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("fps_num", ctypes.c_int),
                    ("fps_den", ctypes.c_int), ("aspect_num", ctypes.c_int),
                    ("aspect_den", ctypes.c_int), ("chroma", ctypes.c_int), ("interlace", ctypes.c_char)]

    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(CLI)), "lib", "liby4m.so"))
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    lib.y4m_read_header.argtypes = [ctypes.c_void_p, ctypes.POINTER(Info)]
    lib.y4m_frame_bytes.restype = ctypes.c_size_t
    lib.y4m_frame_bytes.argtypes = [ctypes.POINTER(Info)]
    lib.y4m_read_frame.argtypes = [ctypes.c_void_p, ctypes.POINTER(Info), ctypes.c_void_p]
    lib.y4m_to_rgba.argtypes = [ctypes.POINTER(Info), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    fp, info, out = libc.fopen(path.encode(), b"rb"), Info(), []
    assert fp and lib.y4m_read_header(fp, ctypes.byref(info)) == 0
    buf = np.empty(lib.y4m_frame_bytes(ctypes.byref(info)), np.uint8)
    for _ in range(n):
        assert lib.y4m_read_frame(fp, ctypes.byref(info), buf.ctypes.data) == 1
        rgba = np.empty((info.height, info.width, 4), np.uint8)
        lib.y4m_to_rgba(ctypes.byref(info), buf.ctypes.data, rgba.ctypes.data, 0)
        out.append(rgba)
    libc.fclose(fp)
    return out


def test_cli_out_nv12_expands_a_y4m_input_as_limited_range(tmp_path):
    """--full-range and --matrix name the output code alone: the .y4m input is
    expanded on the host as BT.601 limited range, as without them."""
    W, H, n = 64, 48, 3
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, W, H, list(_frames(W, H, n, NV12)))
    rgba = _y4m_rgba(src, n)
    base = ["--out-nv12", "-i", src, "-l", str(L), "-s", str(S), "-b", "4", "--checksum"]
    for args, fo in ((["--full-range", "--matrix", "709"], NV12_FULL | BT709), ([], NV12)):
        want = C.run(W, H, rgba, RGBA8, fo, L, S, mode="stream", batch=4)
        assert _cli_hashes(base + args) == [_fnv(w) for w in want], args


def test_cli_out_rgba8_and_out_nv12(tmp_path):
    W, H, n = 64, 48, 4
    # decode: a C420 clip in as MM_NV12, raw RGBA8 out
    fr = list(_frames(W, H, n, NV12))
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.rgba")
    _write_y4m(src, W, H, fr)
    want = C.run(W, H, fr, NV12, RGBA8, L, S, mode="stream", batch=4)
    base = ["--nv12", "--out-rgba8", "-i", src, "-l", str(L), "-s", str(S), "-b", "4", "--checksum"]
    got = _cli_hashes(base + ["-o", dst])
    raw = np.fromfile(dst, np.uint8).reshape(n, H, W, 4)
    for k in range(n):
        assert np.array_equal(raw[k], want[k]), k
    assert got == _cli_hashes(base + ["--surface-align", "256,16"]) and len(got) == n
    assert got == [_fnv(w) for w in want]
    # encode: raw RGBA8 in, raw NV12 out (BT.709, full range: the options name the output code)
    rgba = list(_frames(W, H, n, RGBA8))
    src2, dst2 = str(tmp_path / "in.rgba"), str(tmp_path / "out.nv12")
    np.stack(rgba).tofile(src2)
    fo = NV12_FULL | BT709
    want = C.run(W, H, rgba, RGBA8, fo, L, S, mode="stream", batch=4)
    base = ["--out-nv12", "--full-range", "--matrix", "709", "-w", str(W), "-h", str(H), "-i", src2, "-l", str(L),
            "-s", str(S), "-b", "4", "--checksum"]
    got = _cli_hashes(base + ["-o", dst2])
    raw = np.fromfile(dst2, np.uint8).reshape(n, H * 3 // 2, W)
    for k in range(n):
        assert np.array_equal(raw[k], want[k]), k
    assert got == _cli_hashes(base + ["--surface-align", "256,16"]) and len(got) == n
    assert got == [_fnv(w) for w in want]
    # a .y4m output of the encode leg is a C420 file of those frames
    dst3 = str(tmp_path / "out.y4m")
    subprocess.check_call([CLI] + base + ["-o", dst3], timeout=120, stdout=subprocess.DEVNULL)
    head, body = open(dst3, "rb").read().split(b"\n", 1)
    assert head.startswith(b"YUV4MPEG2") and b"C420" in head and len(body) == n * (6 + W * H * 3 // 2)
    p = np.frombuffer(body[6:6 + W * H * 3 // 2], np.uint8)
    assert np.array_equal(p[:W * H].reshape(H, W), want[0][:H])
    assert np.array_equal(p[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), want[0][H:, 0::2])
    # refused combinations exit with the usage status
    for args in (["--out-rgba8", "-w", "64", "-h", "48", "-n", "2"],
                 ["--nv12", "--out-rgba8", "--out-nv12", "-i", src],
                 ["--out-nv12", "--nv12", "-i", src],
                 ["--out-nv12", "--srgb", "-w", "64", "-h", "48", "-n", "2"],
                 ["--out-nv12", "-w", "63", "-h", "48", "-n", "2"]):
        r = subprocess.run([CLI] + args, capture_output=True, timeout=120)
        assert r.returncode == 2 and b"--out-" in r.stderr, args
