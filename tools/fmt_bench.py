#!/usr/bin/env python3
"""RGBA8 against NV12, P010, grayscale (Y8, Y16) and packed 4:2:2 (YUY2, UYVY, 10-bit Y210, v210) frames on
one GPU, same process, alternating legs.

The flagship stream (1920x1080, 5 levels, phase scale 25, batches of 150
frames as bench.py) in the three frame formats.  Frames are generated on the
device (mm_synth_frames) and converted to NV12 and P010 with torch ops once,
outside the timing.  Every launch shape is warmed up; a leg is `calls` back-to-back
mm_process_stream calls (>= --leg-seconds of device work) between two events
on the handle's stream, synchronised at its end; the formats alternate
--rounds times.  Reports each format's median frames/s and spread, and the
per-kernel device time (mm_profile_begin/end) of one call of each.

Pitched legs (<format>_pitched): the same frames held in decoder-layout
surfaces, mm_surface_aligned(256, 16), on both sides, through
mm_process_stream_surfaces; in the same rounds, next to the tight legs.  A
library from before the pitched surfaces (MM355_LIB, A/B runs) runs the tight
legs only.

Matrixed legs (nv12_bt709, p010_bt2020, and their _pitched forms): the NV12 and
P010 legs' own bytes taken as MM_NV12 | MM_MATRIX_BT709 and MM_P010 |
MM_MATRIX_BT2020 (the timing does not depend on the sample values), whose K1
reads the chroma plane too; in the same rounds, so that their K1 stands next to
the luma-only K1 and to RGBA8's.  A library from before the matrix bits runs
without them.

Grayscale legs (y8, y16, and their _pitched forms): the luma of the same
frames as MM_Y8 bytes and MM_Y16 words (code Yl max, rounded), one sample per
pixel each way; their K34 reads no input.  A library from before the
single-plane formats runs without them.

Packed 4:2:2 legs (yuy2, uyvy, yuy2_bt709, and their _pitched forms): the same
frames as MM_YUY2 macropixels (BT.601 limited range, chroma the mean of each
pixel pair), the same bytes pair-swapped as MM_UYVY, and the YUY2 bytes taken
as MM_YUY2 | MM_MATRIX_BT709, whose K1 reads whole macropixels; 2 bytes per
pixel each way.  A library from before these formats runs without them.

10-bit packed 4:2:2 legs (y210, y210_bt709, and their _pitched forms): the
YUY2 legs' pictures at 10 bits as MM_Y210 macropixels (words Y0 Cb Y1 Cr, code
<< 6), and the same words taken as MM_Y210 | MM_MATRIX_BT709, whose K1 reads
whole 8-byte macropixels; 4 bytes per pixel each way.  A library from before
this format runs without them.

v210 legs (v210, v210_bt709, and their _pitched forms): the Y210 legs' own codes
packed three to a dword as MM_V210 (rows at the standard pitch, 128 ceil(W / 48)),
and the same dwords taken as MM_V210 | MM_MATRIX_BT709, whose K1 loads the pixel
pair's two dwords; 2.67 bytes per pixel each way, so Y210 of the same run is the
comparison.  Their compose is always the unfused pair (k_rows_inv, k_compose:
no fused K34 instance), whose per-kernel times stand beside Y210's fused
k_rows_inv_compose.  A library from before this format runs without them.

Packed RGB legs (rgb24, bgr24, rgb24_pitched): the RGBA8 leg's pictures with
the alpha byte dropped as MM_RGB24, the same pixels byte-swapped as MM_BGR24, 3
bytes per pixel each way; computed by the RGBA8 path's own expressions, so the
legs compare addressing alone (K1's byte-aligned dword loads, K34's 12-byte
quads without RGBA8's LDS-DMA source staging).  A library from before these
formats runs without them.

Three-plane 4:2:0 legs (i420, i420_bt709, i420_pitched): the NV12 legs' own
bytes with the chroma de-interleaved as MM_I420, the same bytes taken as
MM_I420 | MM_MATRIX_BT709 (K1's matrixed three-plane instance), and the I420
frames in mm_surface_aligned(256, 16) surfaces; the same 1.5 bytes per pixel
each way, so NV12 of the same run is the comparison.  A library from before
this format runs without them.

10-bit three-plane 4:2:0 legs (i010, i010_bt709, i010_pitched): the P010 legs'
own codes, shifted to the words' low bits and de-interleaved, as MM_I010, the
same words taken as MM_I010 | MM_MATRIX_BT709 (K1's matrixed instance: two word
loads where P010's takes one pair; p010_bt709 runs beside it), and the I010
frames in mm_surface_aligned(256, 16) surfaces; the same 3 bytes per pixel each
way, so P010 of the same run is the comparison, and I420 the 8-bit one.  A
library from before this format runs without them.

Convert legs (nv12>rgba8, nv12_bt709>rgba8, p010>rgba8, rgba8>nv12,
rgba8>nv12_bt709, and their _pitched forms): the NV12 / P010 / RGBA8 legs' own
frames in as the one format and out as the other through
mm_process_stream_convert, tight, and with the Y'CbCr side in the decoder
layout (the RGBA8 side tight).  Plain legs (<pair>_plain): the same call on a
handle with apply_magnification = 0, which runs the conversion kernel alone on
every frame (plus K1 of the batch's last frame, which keeps the state): its
time per frame and its bandwidth against the bytes it must move.  The summary
sets the same-format stream's time per frame plus that conversion pass against
the mixed leg: two passes against one.  A library from before the conversion
runs without them; --no-convert gives this library that leg set (an A/B of the
existing legs alone, with the same number of legs in every round).

B G R A legs (bgra8, bgra8_pitched, bgra8_srgb, nv12>bgra8, bgra8>nv12 and their
_plain / _pitched forms): the RGBA8 leg's pictures with bytes 0 and 2 of every
pixel exchanged as MM_BGRA8, the same bytes taken as MM_BGRA8_SRGB, and the
convert pairs with MM_BGRA8 as the 4-byte side.  Each runs instances that differ
from its RGBA twin's in byte indices and constants alone, so the yardstick of
each is its twin of the same run: rgba8, rgba8_pitched, rgba8_srgb (the RGBA8
leg's bytes taken as MM_RGBA8_SRGB), nv12>rgba8, rgba8>nv12; "bgra_twins" sets
them side by side with K1's and the compose's times.  A library from before these
formats runs without them; --no-bgra gives this library that leg set (an A/B of
the existing legs alone: the sRGB legs spend 50 us per frame in their encode, and
a round that holds them is not the round the parent's library runs).

--only a,b,c: time these legs alone (every leg is still built, since legs take
their frames from one another; the others are closed before the warm-up).

usage: fmt_bench.py [--rounds 5] [--leg-seconds 0.6] [--no-pitched] [--no-convert] [--no-bgra] [--only LEGS] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-based-motion-manipulation_amd"))


def to_420(torch, rgba, ten_bit=False):
    """[n][H][W][4] uint8 (device) -> [n][H*3/2][W] NV12 (uint8), BT.601 limited
    range, chroma the mean of each 2 x 2 block (y4m_from_rgba's formulas); or,
    ten_bit, P010: the same with 10-bit codes (Y 64 .. 940, C 64 .. 960), each
    stored as code << 6 in an int16 word (the bit pattern of the uint16)."""
    n, H, W, _ = rgba.shape
    ys, y0, cs, c0, top = (876.0, 64.0, 896.0, 512.0, 1023) if ten_bit else (219.0, 16.0, 224.0, 128.0, 255)
    out = torch.empty((n, H * 3 // 2, W), dtype=torch.int16 if ten_bit else torch.uint8, device=rgba.device)
    for k in range(n):       # frame by frame: float planes of one frame at a time
        f = rgba[k, ..., :3].float() / 255.0
        r, g, b = f[..., 0], f[..., 1], f[..., 2]
        yl = 0.299 * r + 0.587 * g + 0.114 * b
        cb = ((b - yl) * (0.5 / 0.886)).reshape(H // 2, 2, W // 2, 2).mean(dim=(1, 3))
        cr = ((r - yl) * (0.5 / 0.701)).reshape(H // 2, 2, W // 2, 2).mean(dim=(1, 3))
        if ten_bit:          # code << 6 as int16: codes >= 512 wrap to the negative half
            code = lambda v: ((torch.clamp(torch.floor(v + 0.5), 0, top).to(torch.int32) << 6) & 0xFFFF
                              ).to(torch.int16)
        else:
            code = lambda v: torch.clamp(torch.floor(v + 0.5), 0, top).to(torch.uint8)
        out[k, :H] = code(yl * ys + y0)
        out[k, H:, 0::2] = code(cb * cs + c0)
        out[k, H:, 1::2] = code(cr * cs + c0)
    return out


def to_422(torch, rgba):
    """[n][H][W][4] uint8 (device) -> [n][H][2 W] YUY2 (uint8): BT.601 limited
    range, bytes Y0 Cb Y1 Cr, chroma the mean of each pixel pair."""
    n, H, W, _ = rgba.shape
    out = torch.empty((n, H, 2 * W), dtype=torch.uint8, device=rgba.device)
    code = lambda v: torch.clamp(torch.floor(v + 0.5), 0, 255).to(torch.uint8)
    for k in range(n):
        f = rgba[k, ..., :3].float() / 255.0
        r, g, b = f[..., 0], f[..., 1], f[..., 2]
        yl = 0.299 * r + 0.587 * g + 0.114 * b
        out[k, :, 0::2] = code(yl * 219.0 + 16.0)
        out[k, :, 1::4] = code(((b - yl) * (0.5 / 0.886)).reshape(H, W // 2, 2).mean(dim=2) * 224.0 + 128.0)
        out[k, :, 3::4] = code(((r - yl) * (0.5 / 0.701)).reshape(H, W // 2, 2).mean(dim=2) * 224.0 + 128.0)
    return out


def to_y210(torch, rgba):
    """[n][H][W][4] uint8 (device) -> [n][H][2 W] Y210 words (the bit pattern of
    the uint16 in an int16): to_422's picture with 10-bit codes (Y 64 .. 940,
    C 64 .. 960), each stored as code << 6, words Y0 Cb Y1 Cr."""
    n, H, W, _ = rgba.shape
    out = torch.empty((n, H, 2 * W), dtype=torch.int16, device=rgba.device)
    code = lambda v: ((torch.clamp(torch.floor(v + 0.5), 0, 1023).to(torch.int32) << 6) & 0xFFFF).to(torch.int16)
    for k in range(n):
        f = rgba[k, ..., :3].float() / 255.0
        r, g, b = f[..., 0], f[..., 1], f[..., 2]
        yl = 0.299 * r + 0.587 * g + 0.114 * b
        out[k, :, 0::2] = code(yl * 876.0 + 64.0)
        out[k, :, 1::4] = code(((b - yl) * (0.5 / 0.886)).reshape(H, W // 2, 2).mean(dim=2) * 896.0 + 512.0)
        out[k, :, 3::4] = code(((r - yl) * (0.5 / 0.701)).reshape(H, W // 2, 2).mean(dim=2) * 896.0 + 512.0)
    return out


def to_v210(torch, y210, W):
    """[n][H][2 W] Y210 words (int16 bit patterns, device) -> [n][H][pitch / 4]
    v210 dwords (int32 bit patterns): the codes word >> 6 in the order Cb Y0 Cr Y1,
    three to a dword, unused fields and the row padding zero."""
    n, H, _ = y210.shape
    D = 4 * (W // 6) + (0, 2, 3)[(W % 6) // 2]
    codes = ((y210.to(torch.int32) & 0xFFFF) >> 6).reshape(n, H, W // 2, 4)[..., [1, 0, 3, 2]].reshape(n, H, 2 * W)
    s = torch.zeros((n, H, 3 * D), dtype=torch.int32, device=y210.device)
    s[..., :2 * W] = codes
    s = s.reshape(n, H, D, 3)
    out = torch.zeros((n, H, 32 * ((W + 47) // 48)), dtype=torch.int32, device=y210.device)
    out[..., :D] = s[..., 0] | s[..., 1] << 10 | s[..., 2] << 20
    return out


def to_mono(torch, rgba, bits):
    """[n][H][W][4] uint8 (device) -> [n][H][W] gray samples: the BT.601 luma of
    the frame, code floor(Yl max + 0.5); uint8, or (16 bits) the bit pattern of
    the uint16 word in an int16."""
    n, H, W, _ = rgba.shape
    top = (1 << bits) - 1
    out = torch.empty((n, H, W), dtype=torch.uint8 if bits == 8 else torch.int16, device=rgba.device)
    for k in range(n):
        f = rgba[k, ..., :3].float() / 255.0
        c = torch.clamp(torch.floor((0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]) * top + 0.5), 0, top)
        out[k] = c.to(torch.uint8) if bits == 8 else (c.to(torch.int32) & 0xFFFF).to(torch.int16)
    return out


def to_surface(torch, src, lay, W, H, planar):
    """Tight frames [n][...] (device) -> one uint8 buffer holding them in layout
    `lay` (padding zero), with strided views of the planes."""
    n = src.shape[0]
    flat = src.contiguous().view(torch.uint8).reshape(n, -1)
    buf = torch.zeros(n * lay.frame_stride, dtype=torch.uint8, device=src.device)
    rb = flat.shape[1] // (H * 3 // 2 if planar else H)
    buf.as_strided((n, H, rb), (lay.frame_stride, lay.pitch, 1)).copy_(flat[:, :H * rb].reshape(n, H, rb))
    if planar:
        buf.as_strided((n, H // 2, rb), (lay.frame_stride, lay.chroma_pitch, 1), lay.chroma_offset).copy_(
            flat[:, H * rb:].reshape(n, H // 2, rb))
    return buf


def nv12_to_i420(torch, nv):
    """[n][H*3/2][W] NV12 (device) -> the same bytes as I420, in the same shape."""
    n, H32, W = nv.shape
    H = H32 * 2 // 3
    c = nv[:, H:].reshape(n, H // 2, W // 2, 2)
    return torch.cat([nv[:, :H].reshape(n, -1), c[..., 0].reshape(n, -1), c[..., 1].reshape(n, -1)],
                     dim=1).reshape(n, H32, W).contiguous()


def to_surface_i420(torch, src, lay, W, H):
    """Tight I420 or I010 frames (device) -> one uint8 buffer holding them in
    layout `lay` (padding zero): the Cr plane chroma_pitch x H/2 after the Cb
    plane.  (Rows in bytes: W samples of the frames' item size.)"""
    n = src.shape[0]
    rb = W * src.element_size()
    flat = src.contiguous().view(torch.uint8).reshape(n, -1)
    buf = torch.zeros(n * lay.frame_stride, dtype=torch.uint8, device=src.device)
    buf.as_strided((n, H, rb), (lay.frame_stride, lay.pitch, 1)).copy_(flat[:, :rb * H].reshape(n, H, rb))
    q = rb * H // 4
    for j in range(2):
        buf.as_strided((n, H // 2, rb // 2), (lay.frame_stride, lay.chroma_pitch, 1),
                       lay.chroma_offset + j * lay.chroma_pitch * (H // 2)).copy_(
            flat[:, rb * H + j * q:rb * H + (j + 1) * q].reshape(n, H // 2, rb // 2))
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.6)
    ap.add_argument("--no-pitched", action="store_true")
    ap.add_argument("--no-convert", action="store_true",
                    help="leave the convert legs out (the leg set of a library from before the conversion)")
    ap.add_argument("--no-bgra", action="store_true",
                    help="leave the B G R A legs and rgba8_srgb out (the leg set of a library from before them)")
    ap.add_argument("--only", default=None, help="comma-separated leg names: time these alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import mm355

    W, H, B = a.width, a.height, a.batch
    p = mm355.Params.make(levels=5, phase_scale=25.0)
    legs = {}
    rgba = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
    fmts = [("rgba8", mm355.RGBA8), ("nv12", mm355.NV12), ("p010", mm355.P010)]
    try:
        mm355.frame_bytes(W, H, mm355.NV12 | mm355.MATRIX_BT709)
        fmts += [("nv12_bt709", mm355.NV12 | mm355.MATRIX_BT709), ("p010_bt2020", mm355.P010 | mm355.MATRIX_BT2020)]
    except mm355.MMError:
        pass    # a build from before the matrix bits
    try:
        mm355.frame_bytes(W, H, mm355.Y8)
        fmts += [("y8", mm355.Y8), ("y16", mm355.Y16)]
    except mm355.MMError:
        pass    # a build from before the single-plane formats
    try:
        mm355.frame_bytes(W, H, mm355.YUY2)
        fmts += [("yuy2", mm355.YUY2), ("uyvy", mm355.UYVY), ("yuy2_bt709", mm355.YUY2 | mm355.MATRIX_BT709)]
    except mm355.MMError:
        pass    # a build from before the packed 4:2:2 formats
    try:
        mm355.frame_bytes(W, H, mm355.Y210)
        fmts += [("y210", mm355.Y210), ("y210_bt709", mm355.Y210 | mm355.MATRIX_BT709)]
    except (mm355.MMError, AttributeError):
        pass    # a build from before the 10-bit packed 4:2:2 format
    try:
        mm355.frame_bytes(W, H, mm355.RGB24)
        fmts += [("rgb24", mm355.RGB24), ("bgr24", mm355.BGR24)]
    except (mm355.MMError, AttributeError):
        pass    # a build from before the packed RGB formats
    try:
        mm355.frame_bytes(W, H, mm355.I420)
        fmts += [("i420", mm355.I420), ("i420_bt709", mm355.I420 | mm355.MATRIX_BT709)]
    except (mm355.MMError, AttributeError):
        pass    # a build from before the three-plane 4:2:0 format
    try:
        mm355.frame_bytes(W, H, mm355.I010)
        fmts += [("p010_bt709", mm355.P010 | mm355.MATRIX_BT709), ("i010", mm355.I010),
                 ("i010_bt709", mm355.I010 | mm355.MATRIX_BT709)]
    except (mm355.MMError, AttributeError):
        pass    # a build from before the 10-bit three-plane format
    try:
        mm355.frame_bytes(W, H, mm355.V210)
        fmts += [("v210", mm355.V210), ("v210_bt709", mm355.V210 | mm355.MATRIX_BT709)]
    except (mm355.MMError, AttributeError):
        pass    # a build from before the v210 format
    bgra = False
    if not a.no_bgra:
        try:
            mm355.frame_bytes(W, H, mm355.BGRA8)
            fmts += [("rgba8_srgb", mm355.RGBA8_SRGB), ("bgra8", mm355.BGRA8), ("bgra8_srgb", mm355.BGRA8_SRGB)]
            bgra = True
        except (mm355.MMError, AttributeError):
            pass    # a build from before the B G R A formats
    for name, fmt in fmts:
        h = mm355.Handle(W, H, p)
        h.set_batch(B)
        if name == "rgba8":
            h.synth(rgba, 0, B, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            src = rgba
        elif name in ("nv12_bt709", "p010_bt2020", "p010_bt709", "yuy2_bt709", "y210_bt709", "i420_bt709", "i010_bt709", "v210_bt709"):
            src = legs[name.split("_")[0]]["src"]
        elif name == "i420":       # the NV12 leg's bytes, de-interleaved
            src = nv12_to_i420(torch, legs["nv12"]["src"])
        elif name == "i010":       # the P010 leg's codes in the words' low bits, de-interleaved
            words = ((legs["p010"]["src"].to(torch.int32) & 0xFFFF) >> 6).to(torch.int16)
            src = nv12_to_i420(torch, words)
        elif name == "rgba8_srgb":  # the RGBA8 leg's bytes, taken as sRGB-encoded
            src = rgba
        elif name == "bgra8":      # the RGBA8 leg's pictures, bytes 0 and 2 of every pixel exchanged
            src = rgba[..., [2, 1, 0, 3]].contiguous()
        elif name == "bgra8_srgb":
            src = legs["bgra8"]["src"]
        elif name == "rgb24":      # the RGBA8 leg's pictures without their alpha
            src = rgba[..., :3].contiguous()
        elif name == "bgr24":
            src = legs["rgb24"]["src"].flip(3).contiguous()
        elif name == "yuy2":
            src = to_422(torch, rgba)
        elif name == "y210":
            src = to_y210(torch, rgba)
        elif name == "v210":       # the Y210 leg's codes, three to a dword
            src = to_v210(torch, legs["y210"]["src"], W)
        elif name == "uyvy":       # the same picture: every byte pair swapped
            src = legs["yuy2"]["src"].reshape(B, H, W, 2).flip(3).reshape(B, H, 2 * W).contiguous()
        elif name in ("y8", "y16"):
            src = to_mono(torch, rgba, 8 if name == "y8" else 16)
        else:
            src = to_420(torch, rgba, ten_bit=name == "p010")
        legs[name] = dict(h=h, fmt=fmt, src=src, dst=torch.empty_like(src), fps=[], lay=None,
                          bytes_per_frame=mm355.frame_bytes(W, H, fmt))
        if not a.no_pitched and mm355.has_surfaces() and name not in ("bgr24", "i420_bt709", "p010_bt709", "i010_bt709", "rgba8_srgb", "bgra8_srgb"):   # (one pitched packed RGB leg, one of each three-plane form)
            lay = mm355.Surface.aligned(W, H, fmt, 256, 16)
            h = mm355.Handle(W, H, p)
            h.set_batch(B)
            buf = (to_surface_i420(torch, src, lay, W, H) if name in ("i420", "i010") else
                   to_surface(torch, src, lay, W, H, name.startswith(("nv12", "p010"))))
            legs[name + "_pitched"] = dict(h=h, fmt=fmt, src=buf, dst=torch.zeros_like(buf), fps=[], lay=lay,
                                           bytes_per_frame=lay.frame_stride)
    convs = []
    if not a.no_convert and getattr(mm355, "has_convert", lambda: False)():
        convs = [("nv12>rgba8", "nv12", mm355.NV12, mm355.RGBA8),
                 ("nv12_bt709>rgba8", "nv12", mm355.NV12 | mm355.MATRIX_BT709, mm355.RGBA8),
                 ("p010>rgba8", "p010", mm355.P010, mm355.RGBA8),
                 ("rgba8>nv12", "rgba8", mm355.RGBA8, mm355.NV12),
                 ("rgba8>nv12_bt709", "rgba8", mm355.RGBA8, mm355.NV12 | mm355.MATRIX_BT709)]
        if bgra:
            convs += [("nv12>bgra8", "nv12", mm355.NV12, mm355.BGRA8), ("bgra8>nv12", "bgra8", mm355.BGRA8, mm355.NV12)]
    px4 = (mm355.RGBA8, getattr(mm355, "BGRA8", mm355.RGBA8))   # the 4-byte side of a pair
    p_off = mm355.Params.make(levels=5, phase_scale=25.0, apply_magnification=False)

    def out_of(fo):
        return torch.empty((B, H, W, 4) if fo in px4 else (B, H * 3 // 2, W), dtype=torch.uint8, device="cuda")

    for name, base, fi, fo in convs:
        src = legs[base]["src"]
        forms = [(name, p, False)]
        if not name.startswith("nv12_bt709") and not name.endswith("bt709"):
            forms.append((name + "_plain", p_off, False))
        if not a.no_pitched:
            forms.append((name + "_pitched", p, True))
        for leg_name, prm, pitched in forms:
            h = mm355.Handle(W, H, prm)
            h.set_batch(B)
            li, lo = mm355.Surface.tight(W, H, fi), mm355.Surface.tight(W, H, fo)
            s_in, s_out = src, out_of(fo)
            if pitched:   # the Y'CbCr side as a decoder lays it out, the RGBA8 / BGRA8 side tight
                if fi not in px4:
                    li = mm355.Surface.aligned(W, H, fi, 256, 16)
                    s_in = to_surface(torch, src, li, W, H, True)
                else:
                    lo = mm355.Surface.aligned(W, H, fo, 256, 16)
                    s_out = torch.zeros(B * lo.frame_stride, dtype=torch.uint8, device="cuda")
            legs[leg_name] = dict(h=h, fmt=fi, ofmt=fo, src=s_in, dst=s_out, fps=[], lay=li, olay=lo, convert=True,
                                  bytes_per_frame=mm355.frame_bytes(W, H, fi) + mm355.frame_bytes(W, H, fo))
    if a.only:
        keep = set(a.only.split(","))
        missing = keep - set(legs)
        if missing:
            sys.exit(f"--only: no leg named {sorted(missing)} (legs: {sorted(legs)})")
        for name in [n for n in legs if n not in keep]:
            legs.pop(name)["h"].close()
        torch.cuda.empty_cache()
    st = torch.cuda.Stream()

    def call(L):
        if L.get("convert"):
            L["h"].process_stream_convert(L["src"], L["lay"], L["dst"], L["olay"], B, stream=st.cuda_stream)
        elif L["lay"] is None:
            L["h"].process_stream(L["src"], L["dst"], B, L["fmt"], stream=st.cuda_stream)
        else:
            L["h"].process_stream_surfaces(L["src"], L["lay"], L["dst"], L["lay"], B, stream=st.cuda_stream)

    def leg(L, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            for _ in range(calls):
                call(L)
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    # warm-up: the first call holds the passthrough frame; then the timed launch shape
    for L in legs.values():
        leg(L, 1)
        t = min(leg(L, 2) for _ in range(2)) / 2
        L["calls"] = max(2, int(a.leg_seconds / t) + 1)
    for _ in range(a.rounds):
        for L in legs.values():
            t = leg(L, L["calls"])
            L["fps"].append(L["calls"] * B / t)
    out = {"workload": f"{W}x{H}, 5 levels, phase scale 25, mm_process_stream of {B} frames, batch {B}",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "library": "MM355_LIB override" if os.environ.get("MM355_LIB") else "the tree's build", "formats": {}}
    for name, L in legs.items():
        L["h"].profile_begin()
        call(L)
        st.synchronize()
        prof = L["h"].profile_end()
        f = L["fps"]
        out["formats"][name] = {
            "bytes_per_frame": L["bytes_per_frame"], "calls_per_leg": L["calls"],
            **({"pitch": L["lay"].pitch, "chroma_offset": L["lay"].chroma_offset} if L["lay"] is not None else {}),
            **({"out_format": L["ofmt"], "out_pitch": L["olay"].pitch} if L.get("convert") else {}),
            "leg_seconds": round(L["calls"] * B / statistics.median(f), 3),
            "fps_legs": [round(x, 1) for x in f], "fps_median": round(statistics.median(f), 1),
            "fps_min": round(min(f), 1), "fps_max": round(max(f), 1),
            "spread_pct": round(100.0 * (max(f) - min(f)) / statistics.median(f), 2),
            "kernel_us_per_frame": {k: round(1e3 * ms / fr, 3) for k, (ms, n, fr) in prof.items() if n},
        }
        L["h"].close()
    if bgra:   # each B G R A leg beside its RGBA twin of the same run
        ku = lambda n, k: out["formats"][n]["kernel_us_per_frame"].get(k)
        out["bgra_twins"] = {}
        for name, twin in (("bgra8", "rgba8"), ("bgra8_pitched", "rgba8_pitched"), ("bgra8_srgb", "rgba8_srgb"),
                           ("nv12>bgra8", "nv12>rgba8"), ("bgra8>nv12", "rgba8>nv12"),
                           ("nv12>bgra8_plain", "nv12>rgba8_plain"), ("bgra8>nv12_plain", "rgba8>nv12_plain"),
                           ("nv12>bgra8_pitched", "nv12>rgba8_pitched"), ("bgra8>nv12_pitched", "rgba8>nv12_pitched")):
            if name in out["formats"] and twin in out["formats"]:
                x, y = out["formats"][name], out["formats"][twin]
                out["bgra_twins"][name] = {
                    "twin": twin, "fps_median": x["fps_median"], "twin_fps_median": y["fps_median"],
                    "over_twin": round(x["fps_median"] / y["fps_median"], 4),
                    "twin_fps_min": y["fps_min"], "twin_fps_max": y["fps_max"],
                    "inside_twin_range": y["fps_min"] <= x["fps_median"] <= y["fps_max"],
                    "kernel_us": {n: {k: ku(n, k) for k in ("k_rows_fwd", "k_rows_inv_compose")} for n in (name, twin)}}
    if not a.only:   # (these set whole families of legs against one another)
        r = out["formats"]["rgba8"]
        for name in ("nv12", "p010"):
            out[name + "_over_rgba8"] = round(out["formats"][name]["fps_median"] / r["fps_median"], 4)
        for name, base in (("nv12_bt709", "nv12"), ("p010_bt2020", "p010")):
            if name in out["formats"]:
                out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                    out["formats"][base]["fps_median"], 4)
                k1 = lambda n: out["formats"][n]["kernel_us_per_frame"]["k_rows_fwd"]
                out[name + "_k1_us"] = {"matrixed": k1(name), base: k1(base), "rgba8": k1("rgba8")}
        for name in ("y8", "y16"):
            if name in out["formats"]:
                out[name + "_over_nv12"] = round(out["formats"][name]["fps_median"] /
                                                 out["formats"]["nv12"]["fps_median"], 4)
                out[name + "_over_rgba8"] = round(out["formats"][name]["fps_median"] / r["fps_median"], 4)
        for name in ("yuy2", "uyvy", "yuy2_bt709"):
            if name in out["formats"]:
                out[name + "_over_rgba8"] = round(out["formats"][name]["fps_median"] / r["fps_median"], 4)
                out[name + "_over_nv12"] = round(out["formats"][name]["fps_median"] /
                                                 out["formats"]["nv12"]["fps_median"], 4)
        if "yuy2_bt709" in out["formats"]:
            k1 = lambda n: out["formats"][n]["kernel_us_per_frame"]["k_rows_fwd"]
            out["yuy2_bt709_k1_us"] = {"matrixed": k1("yuy2_bt709"), "yuy2": k1("yuy2"), "nv12_bt709": k1("nv12_bt709"),
                                       "rgba8": k1("rgba8")}
        for name in ("y210", "y210_bt709"):
            if name in out["formats"]:
                for base in ("rgba8", "p010", "yuy2"):
                    out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                        out["formats"][base]["fps_median"], 4)
        if "y210_bt709" in out["formats"]:
            k1 = lambda n: out["formats"][n]["kernel_us_per_frame"]["k_rows_fwd"]
            out["y210_bt709_k1_us"] = {"matrixed": k1("y210_bt709"), "y210": k1("y210"), "yuy2_bt709": k1("yuy2_bt709"),
                                       "p010": k1("p010"), "rgba8": k1("rgba8")}
        if "v210" in out["formats"]:
            for name in ("v210", "v210_bt709"):
                for base in ("rgba8", "y210", "yuy2"):
                    out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                        out["formats"][base]["fps_median"], 4)
            # K1, and K3 + K4 (v210: the unfused pair; the others: the fused K34)
            kk = lambda n: out["formats"][n]["kernel_us_per_frame"]
            out["v210_kernel_us"] = {n: {"k_rows_fwd": kk(n).get("k_rows_fwd"),
                                         "k3_k4": round(sum(kk(n).get(k, 0.0) for k in
                                                            ("k_rows_inv", "k_compose", "k_rows_inv_compose")), 3)}
                                     for n in ("v210", "v210_bt709", "y210", "y210_bt709", "yuy2", "rgba8")}
        for name in ("rgb24", "bgr24"):
            if name in out["formats"]:
                for base in ("rgba8", "nv12"):
                    out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                        out["formats"][base]["fps_median"], 4)
        if "rgb24" in out["formats"]:
            ku = lambda n, k: out["formats"][n]["kernel_us_per_frame"].get(k)
            out["rgb24_kernel_us"] = {n: {"k_rows_fwd": ku(n, "k_rows_fwd"), "k_rows_inv_compose": ku(n, "k_rows_inv_compose")}
                                      for n in ("rgb24", "bgr24", "rgba8", "nv12")}
        if "i420" in out["formats"]:
            ku = lambda n, k: out["formats"][n]["kernel_us_per_frame"].get(k)
            for name, base in (("i420", "nv12"), ("i420_bt709", "nv12_bt709"), ("i420_pitched", "nv12_pitched")):
                if name in out["formats"] and base in out["formats"]:
                    out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                        out["formats"][base]["fps_median"], 4)
            out["i420_kernel_us"] = {n: {"k_rows_fwd": ku(n, "k_rows_fwd"), "k_rows_inv_compose": ku(n, "k_rows_inv_compose")}
                                     for n in ("i420", "nv12", "i420_bt709", "nv12_bt709", "i420_pitched", "nv12_pitched")
                                     if n in out["formats"]}
        if "i010" in out["formats"]:
            ku = lambda n, k: out["formats"][n]["kernel_us_per_frame"].get(k)
            for name, base in (("i010", "p010"), ("i010", "i420"), ("i010_bt709", "p010_bt709"),
                               ("i010_pitched", "p010_pitched")):
                if name in out["formats"] and base in out["formats"]:
                    out[name + "_over_" + base] = round(out["formats"][name]["fps_median"] /
                                                        out["formats"][base]["fps_median"], 4)
            out["i010_kernel_us"] = {n: {"k_rows_fwd": ku(n, "k_rows_fwd"), "k_rows_inv_compose": ku(n, "k_rows_inv_compose")}
                                     for n in ("i010", "p010", "i420", "i010_bt709", "p010_bt709", "i010_pitched",
                                               "p010_pitched") if n in out["formats"]}
        for name in ("rgba8", "nv12", "p010", "nv12_bt709", "p010_bt2020", "y8", "y16", "yuy2", "uyvy", "yuy2_bt709",
                     "y210", "y210_bt709", "rgb24", "i420", "i010", "v210", "v210_bt709"):
            if name + "_pitched" in out["formats"]:
                out[name + "_pitched_over_tight"] = round(out["formats"][name + "_pitched"]["fps_median"] /
                                                          out["formats"][name]["fps_median"], 4)
        # two passes against one: the same-format stream plus a conversion pass of its own, against the mixed leg
        us = lambda n: 1e6 / out["formats"][n]["fps_median"]
        for name, same in (("nv12>rgba8", "nv12"), ("p010>rgba8", "p010"), ("rgba8>nv12", "rgba8")):
            if name in out["formats"] and name + "_plain" in out["formats"]:
                conv_us = us(name + "_plain")
                out[name + "_two_pass"] = {
                    "same_format_us_per_frame": round(us(same), 3), "convert_pass_us_per_frame": round(conv_us, 3),
                    "two_pass_us_per_frame": round(us(same) + conv_us, 3), "mixed_us_per_frame": round(us(name), 3),
                    "mixed_over_two_pass": round(us(name) / (us(same) + conv_us), 4),
                    "convert_pass_GBps": round(out["formats"][name]["bytes_per_frame"] / conv_us * 1e-3, 1),
                }
                out[name + "_kernel_us"] = {n: out["formats"][n]["kernel_us_per_frame"] for n in (name, "rgba8", "nv12")}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(txt + "\n")


if __name__ == "__main__":
    main()
